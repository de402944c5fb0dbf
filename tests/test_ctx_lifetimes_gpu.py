"""What a context knows belongs to one of four lifetimes (swarm_amd/csrc/swa_internal.h): the context, the
uploaded database, the d = 1 index in place, the resident network.  Every test here walks ONE context of its own through
a chain of the events that end a lifetime — uploads of databases that take other routes, owner changes, a table given
another content, rebuilds, a guard retry — and checks the network against the CPU oracle after every link of the chain:
nothing a link leaves behind may reach the next one's result."""
import os
import subprocess
import sys
import textwrap
from contextlib import contextmanager

import numpy as np
import pytest

import support as S
from d1_sets import giant_group_db, length_mix_db, link_keys, oracle_sorted_rows, upload

pytestmark = pytest.mark.gpu


@contextmanager
def _own_context():
    from swarm_amd import Context
    ctx = Context(0)
    try:
        yield ctx
    finally:
        ctx.close()


def _generated(tmp_path, name, n, length, seed, light=0.0):
    fa = tmp_path / f"{name}.fa"
    S.gen_fasta(fa, n, length, seed, 1, light)
    return fa


def _network_is_the_oracles(ctx, db, what):
    off, nb = ctx.d1_network()
    woff, wnb, _ = oracle_sorted_rows(db)
    assert np.array_equal(off, woff) and np.array_equal(nb, wnb), what
    return len(nb)


def _built_network_is_the_oracles(ctx, db, what):
    upload(ctx, db)
    assert ctx.d1_index_build() is False, what
    return _network_is_the_oracles(ctx, db, what)


def _line_quads(ctx):
    return int(ctx.d1_debug(16, 4 * 8 + 2)[33])               # (selector 16: the list regions, their end, the quads a line)


def _fallback_seeds(ctx):
    return int(ctx.d1_debug(14, 128).view(np.uint32)[2])      # (kCounterFallback of the last network call)


def test_line_width_and_width_class_change_across_uploads(tmp_path):
    """150 nt (4 quads a line) -> 200 nt (8 quads, the next width class) -> a 500-nt sequence among 150-nt ones (16 quads)
    -> the first set again: lines, populations of the width classes and windows are each upload's own"""
    first = S.db_from_fasta(_generated(tmp_path, "a", 600, 150, 101))
    wider = S.db_from_fasta(_generated(tmp_path, "b", 500, 200, 102))
    rng = np.random.default_rng(103)
    long_one = "".join(rng.choice(list("ACGT"), size=500))
    recs = S.read_fasta(tmp_path / "a.fa")[:400] + [(b"long_9", long_one.encode()), (b"longer_2", (long_one[:250] + "A" + long_one[250:]).encode())]
    with_long = S.build_db(recs)
    assert first.longest <= 160 < wider.longest <= 480 < with_long.longest
    with _own_context() as ctx:
        for what, db, quads in (("150 nt", first, 4), ("200 nt", wider, 8), ("a 500-nt sequence", with_long, 16), ("150 nt again", first, 4)):
            assert _built_network_is_the_oracles(ctx, db, what) > 50, what
            assert _line_quads(ctx) == quads, what
        assert ctx.d1_guard_retries() == 0


def test_route_changes_across_uploads(tmp_path):
    """a sequence too short for two windows (seeds left to the plain kernel: a member table) -> a lean build (no table) ->
    two groups of thousands (the tiled pair kernel, another table size) -> a lean build: the table, its size and the marks
    of the members left to the plain kernel are each index's own"""
    lean = S.db_from_fasta(_generated(tmp_path, "lean", 800, 150, 111))
    other = S.db_from_fasta(_generated(tmp_path, "other", 700, 150, 112))
    with _own_context() as ctx:
        for what, db, plain_seeds in (("length mix", length_mix_db(), True), ("lean", lean, False), ("giant groups", giant_group_db(), False),
                                      ("lean again", other, False)):
            assert _built_network_is_the_oracles(ctx, db, what) > 50, what
            assert (_fallback_seeds(ctx) > 0) == plain_seeds, what   # (the route the chain is about was taken)
        assert ctx.d1_guard_retries() == 0


def test_the_order_flag_falls_with_the_upload(tmp_path):
    """abundances not descending (the plain kernel serves the database) -> the same records in db order: the second is served
    by the pair route"""
    recs = S.read_fasta(_generated(tmp_path, "in", 900, 150, 121))
    rng = np.random.default_rng(122)
    abund = rng.permutation(len(recs)) + 1
    recs = [(h.rsplit(b"_", 1)[0] + b"_%d" % a, s) for (h, s), a in zip(recs, abund)]
    ordered = S.build_db(recs)
    unordered = S.build_db(recs)
    order = rng.permutation(ordered.n)                          # the same records, in another order
    unordered.headers = [ordered.headers[i] for i in order]
    unordered.seqs = np.ascontiguousarray(np.concatenate([ordered.words(i) for i in order]))
    unordered.seqlen = np.ascontiguousarray(ordered.seqlen[order])
    unordered.abundance = np.ascontiguousarray(ordered.abundance[order])
    unordered.seq_off = np.concatenate([[0], np.cumsum([len(ordered.words(i)) for i in order])]).astype(np.uint64)
    assert (np.diff(unordered.abundance.astype(np.int64)) > 0).any()
    with _own_context() as ctx:
        assert _built_network_is_the_oracles(ctx, unordered, "unordered") > 50
        assert _built_network_is_the_oracles(ctx, ordered, "ordered") > 50
        assert ctx.d1_lists_form() >= 0                         # a streaming index is in place ...
        assert _fallback_seeds(ctx) == 0                        # ... and served every seed: nothing was left to the plain kernel
        assert ctx.d1_guard_retries() == 0


def test_the_owner_changes_without_an_upload(tmp_path):
    """one upload, one index build, then owner (0, 2), (1, 2), (0, 1): the two partial networks add up to the oracle's, the
    last is the oracle's"""
    db = S.db_from_fasta(_generated(tmp_path, "in", 900, 150, 131))
    woff, wnb, _ = oracle_sorted_rows(db)
    whole = link_keys(woff, wnb)
    with _own_context() as ctx:
        assert _built_network_is_the_oracles(ctx, db, "whole") > 50
        parts = []
        for rank in range(2):
            ctx.d1_set_ownership(rank, 2)
            parts.append(link_keys(*ctx.d1_network()))
        assert all(len(p) > 0 for p in parts)
        assert np.array_equal(np.sort(np.concatenate(parts)), whole)
        ctx.d1_set_ownership(0, 1)
        _network_is_the_oracles(ctx, db, "one owner again")
        assert ctx.d1_guard_retries() == 0


def test_the_table_given_another_content_ends_the_index(tmp_path, monkeypatch):
    """the dereplication, and the Bloom route of --fastidious, use the d = 1 table for contents of their own: a network call
    behind them is refused until the index is built again, and then is the oracle's"""
    from swarm_amd import D1Clusters, HostDb, capi
    fa = _generated(tmp_path, "in", 900, 150, 141, 0.3)
    hdb = HostDb(fa)
    db = S.db_from_fasta(fa)

    def refused_then_rebuilt(what):
        with pytest.raises(capi.SwaError, match="call swa_d1_index_build first") as e:
            ctx.d1_network()
        assert e.value.code == 2, what                          # SWA_E_ARG
        assert ctx.d1_index_build() is False, what
        _network_is_the_oracles(ctx, db, what)

    with _own_context() as ctx:
        ctx.upload_hostdb(hdb)
        assert ctx.d1_index_build() is False
        off, nb = ctx.d1_network()
        assert np.array_equal(capi.derep(ctx), S.oracle_derep(db))
        refused_then_rebuilt("after the dereplication")
        monkeypatch.setenv("SWA_FAST_BLOOM", "1")
        flags, stats = D1Clusters(hdb, off, nb).light_flags(3)
        graft, _ = ctx.d1_fastidious(flags, stats[2], 16)
        monkeypatch.delenv("SWA_FAST_BLOOM")
        assert np.array_equal(graft, S.oracle_fastidious(db, flags, 16)[0])
        refused_then_rebuilt("after the Bloom route")
        assert ctx.d1_guard_retries() == 0


def test_a_plain_rebuild_over_a_streaming_index(tmp_path, monkeypatch):
    """index builds on the plain route (SWA_D1_PLAIN=1) over a streaming index, and back: the oracle's network every time, and
    behind a plain build the readers of the streaming index say that there is none"""
    from swarm_amd import capi
    db = S.db_from_fasta(_generated(tmp_path, "in", 900, 150, 151))
    with _own_context() as ctx:
        assert _built_network_is_the_oracles(ctx, db, "streaming") > 50
        plan = ctx.d1_part_plan()
        assert plan[0] >= 1 and ctx.d1_lists_form() >= 0 and len(ctx.d1_debug(10, (db.n + 1) // 2)) > 0
        for turn in range(2):
            monkeypatch.setenv("SWA_D1_PLAIN", "1")
            assert ctx.d1_index_build() is False
            _network_is_the_oracles(ctx, db, ("plain", turn))
            with pytest.raises(capi.SwaError):
                ctx.d1_lists_form()
            if turn == 1:
                break
            monkeypatch.delenv("SWA_D1_PLAIN")
            assert ctx.d1_index_build() is False                # (and a streaming index again)
            _network_is_the_oracles(ctx, db, "streaming again")
            assert ctx.d1_part_plan() == plan and ctx.d1_lists_form() >= 0
        # The ONE place where the library differs from its state before the context's members were grouped by lifetime: there
        # these two answered from the streaming index that the plain build had replaced
        with pytest.raises(capi.SwaError):
            ctx.d1_part_plan()
        with pytest.raises(capi.SwaError, match="no streaming index in place"):
            ctx.d1_debug(10, (db.n + 1) // 2)
        assert ctx.d1_guard_retries() == 0


_RETRY_WORKER = textwrap.dedent('''
    import os, sys
    import numpy as np
    sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
    import support as S
    from d1_sets import oracle_sorted_rows, upload
    from swarm_amd import Context
    dbs = [S.db_from_fasta(p) for p in sys.argv[2:4]]
    ctx = Context(0)
    def step(db, what):
        upload(ctx, db)
        assert ctx.d1_index_build() is False, what
        off, nb = ctx.d1_network()
        woff, wnb, _ = oracle_sorted_rows(db)
        assert np.array_equal(off, woff) and np.array_equal(nb, wnb), what
        print(what, "retries", ctx.d1_guard_retries())
    step(dbs[0], "before")
    os.environ["SWA_D1_GUARD_TEST"] = "drop-once"             # (the first build from here on loses a key record)
    step(dbs[1], "faulted")
    step(dbs[0], "after")
    step(dbs[1], "again")
    ctx.close()
''')


def test_a_guard_retry_on_a_used_context(tmp_path):
    """a context that has served another database meets a transient fault (SWA_D1_GUARD_TEST=drop-once, in a process of its
    own: the hook counts the builds of the process): one retry, the oracle's network, and ordinary builds behind it — of the
    other database and of the same — are the oracle's too"""
    fas = [_generated(tmp_path, "a", 700, 150, 161), _generated(tmp_path, "b", 800, 200, 162)]
    script = tmp_path / "worker.py"
    script.write_text(_RETRY_WORKER)
    env = dict(os.environ)
    env.pop("SWA_D1_GUARD_TEST", None)
    r = subprocess.run([sys.executable, str(script), str(S.ROOT)] + [str(f) for f in fas], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert [line for line in r.stdout.splitlines() if "retries" in line] == ["before retries 0", "faulted retries 1", "after retries 1",
                                                                           "again retries 1"], r.stdout
    assert "repeating the step" in r.stderr
