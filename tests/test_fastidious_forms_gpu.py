"""Every kernel form of the --fastidious pass (seam B2; swarm_amd/csrc/fastidious.hip: fast_plan, d1_fast.inc) against the
oracle, with the longest sequence of the database on each boundary of the dispatch and next to it.

The pass chooses its kernels from the longest sequence alone (swa_d1_fastidious_plan reports the choice, the launches
read the same plan):

  longest      pair kernel              count kernel
  112 .. 159   k_fast_pairs_lines<5>    k_fast_count_sites<5>
  160          k_fast_pairs_lines<5>    k_fast_count_sites<8>
  161 .. 255   k_fast_pairs_lines<8>    k_fast_count_sites<8>
  256          k_fast_pairs_lines<8>    k_fast_count, 4 waves x 4096 slots
  257 .. 389   k_fast_pairs_lines<13>   k_fast_count, 4 waves x 4096
  390 .. 416   k_fast_pairs_lines<13>   k_fast_count, 2 waves x 8192
  417 .. 779   k_fast_pairs             k_fast_count, 2 waves x 8192
  780 .. 1004  k_fast_pairs             k_fast_count, 1 wave x 16384
  1005 .. 3070 none: the Bloom route for every pair, Zobrist table in LDS
  >= 3071      the Bloom route, Zobrist table read from memory

Natural cells: tests/fastidious_sets.py's edit_atlas(L) with its longest record exactly L.  Borrowed cells:
edit_atlas(150) and one unrelated sequence of X nt, which sends the same 150-nt pairs through the kernels of X.
Expected values come from S.oracle_fastidious (the reference's Bloom scheme restated on the CPU) and are integers:
compared exactly.  test_fastidious_identity.py checks on the CPU that every set here is worth running."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import fastidious_sets as FS
import support as S
from swarm_amd import Context, D1Clusters, HostDb

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
BORROWED = [160, 200, 256, 300, 400, 500, 900, 1005, 3071]
# plan[:4] + [plan[6]] of every row of the table above
ROWS = {(1, 5, 5, 0, 1), (1, 5, 8, 0, 1), (1, 8, 8, 0, 1), (1, 8, 0, 4, 1), (1, 13, 0, 4, 1), (1, 13, 0, 2, 1), (1, 0, 0, 2, 1),
        (1, 0, 0, 1, 1), (0, 0, 0, 0, 1), (0, 0, 0, 0, 0)}
_reached = {}                                                   # row -> the cases that ran it and passed


def _pipeline(ctx, fasta, boundary=3, bits=16, shard=None):
    hdb = HostDb(fasta)
    ctx.upload_hostdb(hdb)
    assert ctx.d1_index_build() is False
    off, nb = ctx.d1_network()
    cl = D1Clusters(hdb, off, nb)
    flags, stats = cl.light_flags(boundary)
    graft, counters = ctx.d1_fastidious(flags, stats[2], bits) if shard is None else ctx.d1_fastidious(flags, stats[2], bits, *shard)
    return hdb, cl, flags, stats, graft, counters


def _case(ctx, tmp_path, L, outlier=None, label=None):
    """one set through the pass on the GPU and through the oracle: the plan, the flags, both results"""
    fa = tmp_path / "in.fa"
    db, want_flags, three = FS.build_case(L, fa, outlier)
    hdb, cl, flags, stats, graft, counters = _pipeline(ctx, fa)
    plan = ctx.d1_fastidious_plan()
    totals = ctx.d1_fastidious_totals()
    assert np.array_equal(flags, want_flags)
    want_graft, want_counters = S.oracle_fastidious(db, flags, 16)
    FS.assert_not_trivial(db, flags, want_graft, three)
    longest = L if outlier is None else outlier
    assert db.longest == longest and plan == FS.expected_plan(longest), (plan, FS.expected_plan(longest))
    print(f"longest {longest} n {db.n} plan {plan} totals {totals} candidates {int(counters[2])} / {int(want_counters[2])} "
          f"grafts differ at {int((graft != want_graft).sum())}")
    assert np.array_equal(graft, want_graft)
    assert [int(x) for x in counters[:5]] == [int(x) for x in want_counters[:5]]
    if plan[0]:
        assert totals[0] > 0 and totals[3] >= 1
    else:
        assert totals[0] == 0 and totals[3] == 0 and totals[1] > 0 and totals[2] > 0
    _reached.setdefault(tuple(plan[:4] + plan[6:7]), []).append(label or f"{L}+{outlier}")
    return db, flags, graft, counters, plan, totals


@pytest.fixture(scope="module")
def alone(gpu_ctx, tmp_path_factory):
    """edit_atlas(L) without an outlier, once per L: what the borrowed cells must reproduce on the shared records"""
    memo = {}

    def get(L):
        if L not in memo:
            memo[L] = _case(gpu_ctx, tmp_path_factory.mktemp(f"alone{L}"), L, label=f"{L} alone")
        return memo[L]
    return get


@pytest.mark.parametrize("L", FS.NATURAL)
def test_natural_cell_matches_oracle(gpu_ctx, tmp_path, L):
    _case(gpu_ctx, tmp_path, L, label=f"natural {L}")


@pytest.mark.parametrize("X", BORROWED)
def test_borrowed_cell_matches_oracle_and_the_run_without_outlier(gpu_ctx, tmp_path, alone, X):
    db0, flags0, graft0, counters0, plan0, _ = alone(150)
    db, flags, graft, counters, plan, _ = _case(gpu_ctx, tmp_path, 150, X)
    assert db.headers[-1].decode() == FS.OUTLIER and db.headers[:-1] == db0.headers
    assert np.array_equal(graft[:-1], graft0) and graft[-1] == FS.NO_GRAFT
    assert int(counters[2]) == int(counters0[2]) and int(counters[1]) == int(counters0[1])
    assert plan0[:3] == [1, 5, 5] and plan[:7] != plan0[:7]


@pytest.mark.parametrize("L", [112, 113])
def test_both_routes_work_at_once(gpu_ctx, tmp_path, alone, L):
    """a 500-nt outlier next to sequences of 110 .. 113 nt: packed-word pair kernel and LDS-set counter for the pairs of
    two sequences of >= 112 nt, the Bloom route for the pairs with a shorter member"""
    db0, flags0, graft0, counters0, plan0, _ = alone(L)
    db, flags, graft, counters, plan, totals = _case(gpu_ctx, tmp_path, L, 500)
    assert plan[:4] == [1, 0, 0, 2]
    assert totals[0] > 0 and totals[1] > 0 and totals[2] > 0
    assert np.array_equal(graft[:-1], graft0) and int(counters[2]) == int(counters0[2])


def test_pair_list_regrows(tmp_path, monkeypatch):
    """SWA_FAST_PAIR_CAP=64: the first attempt overflows the pair list, the list is sized from the count of the complete
    run and the pass repeated; a second call on the context starts from the grown list"""
    monkeypatch.setenv("SWA_FAST_PAIR_CAP", "64")
    ctx = Context(0)
    try:
        db, flags, graft, counters, plan, totals = _case(ctx, tmp_path, 150, label="150 regrow")
        assert totals[0] > 64 and totals[3] >= 2
        assert ctx.d1_index_build() is False                    # the pass re-purposes the table
        graft2, counters2 = ctx.d1_fastidious(flags, int(db.seqlen[flags != 0].sum()), 16)
        assert ctx.d1_fastidious_totals()[3] == 1 and ctx.d1_fastidious_totals()[0] == totals[0]
        assert np.array_equal(graft2, graft) and [int(x) for x in counters2[:5]] == [int(x) for x in counters[:5]]
    finally:
        ctx.close()


def test_switches_show_in_the_plan(tmp_path, monkeypatch):
    fa = tmp_path / "in.fa"
    FS.build_case(150, fa)
    for name, value, want in (("SWA_FAST_PAIRS", "words", FS.expected_plan(150, words=True)),
                              ("SWA_FAST_BLOOM", "1", FS.expected_plan(150, bloom=True))):
        monkeypatch.setenv(name, value)
        ctx = Context(0)
        ctx.upload_hostdb(HostDb(fa))
        assert ctx.d1_fastidious_plan() == want                 # valid once a database is resident
        ctx.close()
        monkeypatch.delenv(name)


@pytest.mark.parametrize("words", [False, True])
def test_a_group_of_more_tiles_than_items_matches_oracle(gpu_ctx, tmp_path, monkeypatch, words):
    """FS.shared_ends: the prefix group and the suffix group hold all 530 light and 530 heavy amplicons, 81 tiles dealt to
    64 items, so the pair kernel's strided walk (tile = item.tile, + 64) takes a second turn and the items kernel deals
    a group more tiles than items: on k_fast_pairs_lines<5> and, under SWA_FAST_PAIRS=words, on k_fast_pairs.
    (tests/test_fastidious_identity.py checks on the CPU that the set is what it says.)"""
    if words:
        monkeypatch.setenv("SWA_FAST_PAIRS", "words")
    recs, three, planted = FS.shared_ends()
    fa = tmp_path / "in.fa"
    db, want_flags = FS.cluster_records(recs, fa)
    hdb, cl, flags, stats, graft, counters = _pipeline(gpu_ctx, fa)
    plan, totals = gpu_ctx.d1_fastidious_plan(), gpu_ctx.d1_fastidious_totals()
    assert np.array_equal(flags, want_flags)
    assert plan == FS.expected_plan(db.longest, words=words) and plan[:3] == ([1, 0, 5] if words else [1, 5, 5])
    want_graft, want_counters = S.oracle_fastidious(db, flags, 16)
    FS.assert_not_trivial(db, flags, want_graft, three)
    print(f"words {words} n {db.n} plan {plan} totals {totals} candidates {int(counters[2])} / {int(want_counters[2])} "
          f"grafts {int((want_graft != FS.NO_GRAFT).sum())}, differ at {int((graft != want_graft).sum())}")
    assert np.array_equal(graft, want_graft)
    assert [int(x) for x in counters[:5]] == [int(x) for x in want_counters[:5]]
    assert totals[0] >= len(planted) - len(three) and totals[3] == 1


@pytest.mark.parametrize("X", [500, 1005])
def test_shards_of_borrowed_cells_combine_to_the_oracle(gpu_ctx, tmp_path, X):
    fa = tmp_path / "in.fa"
    db, flags, three = FS.build_case(150, fa, X)
    want_graft, want_counters = S.oracle_fastidious(db, flags, 16)
    merged = np.full(db.n, FS.NO_GRAFT, dtype=np.uint32)
    heavy_variants = candidates = 0
    for shard in range(3):
        hdb, cl, got_flags, stats, g, c = _pipeline(gpu_ctx, fa, shard=(shard, 3))
        assert np.array_equal(got_flags, flags)
        assert [int(c[i]) for i in (0, 3, 4)] == [int(want_counters[i]) for i in (0, 3, 4)]
        merged = np.minimum(merged, g)
        heavy_variants += int(c[1])
        candidates += int(c[2])
    assert np.array_equal(merged, want_graft)
    assert (heavy_variants, candidates) == (int(want_counters[1]), int(want_counters[2]))
    assert (want_graft != FS.NO_GRAFT).sum() >= 50


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("devices", [None, "0,0"])
def test_cli_on_a_borrowed_cell_is_byte_identical_to_the_reference(tmp_path, devices):
    fa = tmp_path / "in.fa"
    FS.build_case(150, fa, 500)
    ref_cmd, our_cmd = ["-d", "1", "-f"], [str(BIN), "-d", "1", "-f"]
    for k in "osi":
        ref_cmd += [f"-{k}", str(tmp_path / f"r{k}")]
        our_cmd += [f"-{k}", str(tmp_path / f"g{k}")]
    r = S.run_ref_swarm(ref_cmd + ["-l", "/dev/null", str(fa)])
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, SWARM_AMD_DEVICES=devices) if devices else dict(os.environ)
    g = subprocess.run(our_cmd + ["-l", "/dev/null", str(fa)], capture_output=True, text=True, env=env)
    assert g.returncode == 0, g.stderr
    for k in "osi":
        assert filecmp.cmp(tmp_path / f"r{k}", tmp_path / f"g{k}", shallow=False), k


@pytest.mark.parametrize("name", ["d1_fastidious", "d1_fastidious_b10_y8"])
def test_golden_inputs_keep_their_cell(gpu_ctx, name):
    hdb = HostDb(S.GOLDEN / f"{name}.fasta")
    gpu_ctx.upload_hostdb(hdb)
    longest = S.db_from_fasta(S.GOLDEN / f"{name}.fasta").longest
    assert gpu_ctx.d1_fastidious_plan() == FS.expected_plan(longest)
    print(name, "longest", longest, gpu_ctx.d1_fastidious_plan())


def test_every_row_of_the_dispatch_table_was_reached():
    """(after the cells above, in file order)"""
    print({row: len(cases) for row, cases in _reached.items()})
    assert set(_reached) == ROWS, (ROWS - set(_reached), set(_reached) - ROWS)
