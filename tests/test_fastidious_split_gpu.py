"""SWA_FAST_LONG=split on the GPU (seam B2; swarm_amd/csrc/fastidious.hip: fast_plan, d1_fast.inc) against the oracle: a database
with sequences longer than the pair route's cap (1004 nt) keeps the pair route for the pairs whose two lengths lie in
[112, cap]; every other pair takes the Bloom route.  Without the switch such a database takes the Bloom route for every
pair (tests/test_fastidious_forms_gpu.py pins that).

Sets: tests/fastidious_split_sets.py; tests/test_fastidious_split_identity.py checks on the CPU that each is worth
running.  Expected values come from S.oracle_fastidious and are integers: compared exactly."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import fastidious_sets as FS
import fastidious_split_sets as SS
import support as S
from swarm_amd import Context, D1Clusters, HostDb

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a set on disk with the oracle's result, made once: (fasta, db, flags, three, graft, counters)"""
    memo = {}

    def get(name):
        if name not in memo:
            fa = tmp_path_factory.mktemp("split") / "in.fa"
            db, flags, three = SS.build(name, fa)
            graft, counters = S.oracle_fastidious(db, flags, 16)
            memo[name] = (fa, db, flags, three, graft, counters)
        return memo[name]
    return get


def _run(ctx, fasta, shard=None):
    hdb = HostDb(fasta)
    ctx.upload_hostdb(hdb)
    assert ctx.d1_index_build() is False
    off, nb = ctx.d1_network()
    flags, stats = D1Clusters(hdb, off, nb).light_flags(3)
    graft, counters = ctx.d1_fastidious(flags, stats[2], 16, *(shard or ()))
    return flags, graft, counters


def _check(ctx, case, name, want_plan, want_split):
    """the set through the pass on `ctx`: flags, plan, split report and both results against the oracle"""
    fa, db, want_flags, three, want_graft, want_counters = case(name)
    flags, graft, counters = _run(ctx, fa)
    plan, split, totals = ctx.d1_fastidious_plan(), ctx.d1_fastidious_split(), ctx.d1_fastidious_totals()
    print(f"{name}: n {db.n} longest {db.longest} plan {plan} split {split} totals {totals} candidates {int(counters[2])} / "
          f"{int(want_counters[2])} grafts differ at {int((graft != want_graft).sum())}")
    assert np.array_equal(flags, want_flags)
    assert plan == want_plan, (plan, want_plan)
    assert split == want_split, (split, want_split)
    assert np.array_equal(graft, want_graft)
    assert [int(x) for x in counters[:5]] == [int(x) for x in want_counters[:5]]
    return graft, counters, totals


def _split_plan(pair_longest, longest):
    return FS.expected_plan(pair_longest, words=True)[:6] + FS.expected_plan(longest)[6:]


@pytest.mark.parametrize("X", [1005, 3071])
def test_borrowed_cell_keeps_the_pair_route(case, tmp_path, monkeypatch, X):
    """edit_atlas(150) and one sequence of X nt: the 150-nt pairs stay on the pair route (without the switch: plan[0] == 0
    and totals[0] == 0, every pair on the Bloom route)"""
    monkeypatch.setenv("SWA_FAST_LONG", "split")
    ctx = Context(0)
    try:
        ctx.upload_hostdb(HostDb(case(f"150+{X}")[0]))
        assert ctx.d1_fastidious_split() == [1, SS.CAP, 150, 1]  # valid once a database is resident
        graft, counters, totals = _check(ctx, case, f"150+{X}", _split_plan(150, X), [1, SS.CAP, 150, 1])
        assert totals[0] > 0 and totals[3] >= 1
        assert totals[1] == 1 and totals[2] == 0               # the long band: the outlier (light) alone, so no Bloom pass
        graft0, counters0, totals0 = _check(ctx, case, "150", FS.expected_plan(150), [0, SS.CAP, 150, 0])
        assert np.array_equal(graft[:-1], graft0) and graft[-1] == FS.NO_GRAFT
        assert int(counters[2]) == int(counters0[2]) and totals[0] == totals0[0]
    finally:
        ctx.close()


def test_long_cell_runs_both_routes_at_once(case, monkeypatch):
    monkeypatch.setenv("SWA_FAST_LONG", "split")
    ctx = Context(0)
    try:
        db = case("long")[1]
        n_long = int((db.seqlen > SS.CAP).sum())
        graft, counters, totals = _check(ctx, case, "long", _split_plan(SS.CAP, SS.LONG), [1, SS.CAP, SS.CAP, n_long])
        assert ctx.d1_fastidious_plan()[:5] == [1, 0, 0, 1, 16384]
        assert totals[0] > 0 and totals[1] > 0 and totals[2] > 0
    finally:
        ctx.close()


def test_three_classes_in_one_database(case, monkeypatch):
    """short band, pair route and long band at once, the Zobrist table read from memory on the Bloom route"""
    monkeypatch.setenv("SWA_FAST_LONG", "split")
    ctx = Context(0)
    try:
        db, flags = case("three")[1:3]
        n_long = int((db.seqlen > SS.CAP).sum())
        want_plan = _split_plan(SS.CAP, 3071)
        assert want_plan[6] == 0 and n_long > 100
        graft, counters, totals = _check(ctx, case, "three", want_plan, [1, SS.CAP, SS.CAP, n_long])
        assert totals[0] > 0
        bands = SS.in_bands(db.seqlen)
        assert totals[1] == int((bands & (flags != 0)).sum()) and totals[2] == int((bands & (flags == 0)).sum())
    finally:
        ctx.close()


def test_shards_combine_to_the_oracle(case, monkeypatch):
    monkeypatch.setenv("SWA_FAST_LONG", "split")
    fa, db, flags, three, want_graft, want_counters = case("three")
    ctx = Context(0)
    try:
        merged = np.full(db.n, FS.NO_GRAFT, dtype=np.uint32)
        heavy_variants = candidates = 0
        for shard in range(3):
            got_flags, g, c = _run(ctx, fa, shard=(shard, 3))
            assert ctx.d1_fastidious_split()[0] == 1 and ctx.d1_fastidious_totals()[0] > 0
            assert np.array_equal(got_flags, flags)
            assert [int(c[i]) for i in (0, 3, 4)] == [int(want_counters[i]) for i in (0, 3, 4)]
            merged = np.minimum(merged, g)
            heavy_variants += int(c[1])
            candidates += int(c[2])
        assert np.array_equal(merged, want_graft)
        assert (heavy_variants, candidates) == (int(want_counters[1]), int(want_counters[2]))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["150", "1004"])
def test_no_change_up_to_the_cap(case, monkeypatch, name):
    monkeypatch.setenv("SWA_FAST_LONG", "split")
    ctx = Context(0)
    try:
        L = int(name)
        graft, counters, totals = _check(ctx, case, name, FS.expected_plan(L), [0, SS.CAP, L, 0])
        assert ctx.d1_fastidious_plan()[1] == (5 if L == 150 else 0)          # the lines kernel stays at 150
        assert totals[0] > 0
    finally:
        ctx.close()


def test_no_change_where_every_sequence_is_longer_than_the_cap(case, monkeypatch):
    monkeypatch.setenv("SWA_FAST_LONG", "split")
    ctx = Context(0)
    try:
        db = case("all_long")[1]
        graft, counters, totals = _check(ctx, case, "all_long", FS.expected_plan(SS.LONG), [0, SS.CAP, 0, db.n])
        assert (graft != FS.NO_GRAFT).sum() >= 5
        assert totals[0] == 0 and totals[3] == 0 and totals[1] > 0 and totals[2] > 0
    finally:
        ctx.close()


def test_bloom_switch_wins(case, monkeypatch):
    monkeypatch.setenv("SWA_FAST_LONG", "split")
    monkeypatch.setenv("SWA_FAST_BLOOM", "1")
    ctx = Context(0)
    try:
        graft, counters, totals = _check(ctx, case, "150+1005", FS.expected_plan(1005, bloom=True), [0, SS.CAP, 150, 1])
        assert totals[0] == 0 and totals[3] == 0
    finally:
        ctx.close()


def test_without_the_switch_the_long_cell_is_all_bloom(case, monkeypatch):
    """the default: the plan of the parent commit, and the report still tells what the switch would find"""
    monkeypatch.delenv("SWA_FAST_LONG", raising=False)
    ctx = Context(0)
    try:
        db = case("long")[1]
        n_long = int((db.seqlen > SS.CAP).sum())
        graft, counters, totals = _check(ctx, case, "long", FS.expected_plan(SS.LONG), [0, SS.CAP, SS.CAP, n_long])
        assert totals[0] == 0 and totals[3] == 0
    finally:
        ctx.close()


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("devices", [None, "0,0"])
def test_cli_under_the_switch_is_byte_identical_to_the_reference(case, tmp_path, monkeypatch, devices):
    monkeypatch.setenv("SWA_FAST_LONG", "split")
    fa = case("three")[0]
    ref_cmd, our_cmd = ["-d", "1", "-f"], [str(BIN), "-d", "1", "-f"]
    for k in "osi":
        ref_cmd += [f"-{k}", str(tmp_path / f"r{k}")]
        our_cmd += [f"-{k}", str(tmp_path / f"g{k}")]
    r = S.run_ref_swarm(ref_cmd + ["-l", "/dev/null", str(fa)])
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, SWARM_AMD_DEVICES=devices) if devices else dict(os.environ)
    assert env["SWA_FAST_LONG"] == "split"
    g = subprocess.run(our_cmd + ["-l", "/dev/null", str(fa)], capture_output=True, text=True, env=env)
    assert g.returncode == 0, g.stderr
    for k in "osi":
        assert filecmp.cmp(tmp_path / f"r{k}", tmp_path / f"g{k}", shallow=False), k
