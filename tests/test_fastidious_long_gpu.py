"""SWA_FAST_LONG=pairs and SWA_FAST_COUNT=sites on the GPU (seam B2; swarm_amd/csrc/d1_fast.inc: k_fast_count_sites_words,
fastidious.hip: fast_plan) against the oracle.

  pairs   a database whose longest sequence exceeds 1004 nt keeps the pair route for every pair whose two lengths lie in
          [112, C], C = 327 584 nt or SWA_FAST_SITES_CAP; the count kernel of the whole pass is k_fast_count_sites_words
  sites   the same kernel in k_fast_count's place on the rows 256 .. 1004, compared with k_fast_count on the same context

Sets: tests/fastidious_long_sets.py; tests/test_fastidious_long_identity.py checks on the CPU that each is worth running
and restates the kernel.  Expected values come from S.oracle_fastidious and are integers: compared exactly."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import fastidious_long_sets as LS
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
            fa = tmp_path_factory.mktemp("long") / "in.fa"
            if name == "shared+300":
                recs, three, _ = FS.shared_ends()
                db, flags = FS.cluster_records(FS.with_outlier(recs, 300), fa)
            else:
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


@pytest.mark.parametrize("L", LS.LONG_ATLASES)
def test_long_atlas_stays_on_the_pair_route(case, monkeypatch, L):
    """edit_atlas(L) alone, L past k_fast_count's cap: every pair on the pair route, nothing for the Bloom route"""
    monkeypatch.setenv("SWA_FAST_LONG", "pairs")
    ctx = Context(0)
    try:
        want_plan = LS.sites_plan(L, L)
        assert want_plan[:5] == [1, 0, 1, 4, 0] and want_plan[5] == 64 * ((L + 31) // 32 + 3)
        graft, counters, totals = _check(ctx, case, str(L), want_plan, [2, LS.SITES_CAP, L, 0])
        assert totals[0] > 0 and totals[1] == 0 and totals[2] == 0 and totals[3] == 1
        assert (graft != FS.NO_GRAFT).sum() >= 50
    finally:
        ctx.close()


def test_three_classes_under_pairs(case, monkeypatch):
    """the short band takes the Bloom route, everything else — the 1001 .. 1005-nt atlas included — the pair route; the
    3071-nt outlier lies on the pair route's side of the cap and sets the staged words (96 + 3 a copy)"""
    monkeypatch.setenv("SWA_FAST_LONG", "pairs")
    ctx = Context(0)
    try:
        db, flags = case("three")[1:3]
        want_plan = LS.sites_plan(3071, 3071)
        assert want_plan == [1, 0, 1, 4, 0, 64 * 99, 0, 112]
        graft, counters, totals = _check(ctx, case, "three", want_plan, [2, LS.SITES_CAP, 3071, 0])
        short = db.seqlen <= SS.MIN_LEN + 1
        assert np.array_equal(short, SS.in_bands(db.seqlen, cap=LS.SITES_CAP))
        assert totals[0] > 0 and totals[1] == int((short & (flags != 0)).sum()) and totals[2] == int((short & (flags == 0)).sum())
        assert totals[1] > 0 and totals[2] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["long", "three"])
def test_division_at_the_kernels_own_cap(case, monkeypatch, name):
    """SWA_FAST_SITES_CAP=1004: the pairs beyond 1004 nt take the Bloom route, the others k_fast_count_sites_words"""
    monkeypatch.setenv("SWA_FAST_LONG", "pairs")
    monkeypatch.setenv("SWA_FAST_SITES_CAP", "1004")
    ctx = Context(0)
    try:
        db, flags = case(name)[1:3]
        n_long = int((db.seqlen > 1004).sum())
        assert n_long > 100
        graft, counters, totals = _check(ctx, case, name, LS.sites_plan(1004, db.longest), [2, 1004, 1004, n_long])
        bands = SS.in_bands(db.seqlen, cap=1004)
        assert totals[0] > 0 and totals[1] > 0 and totals[2] > 0
        assert totals[1] == int((bands & (flags != 0)).sum()) and totals[2] == int((bands & (flags == 0)).sum())
    finally:
        ctx.close()


@pytest.mark.parametrize("L", [256, 257, 416, 417, 1004])
def test_count_sites_equals_the_lds_set(case, monkeypatch, L):
    """SWA_FAST_COUNT=sites on the rows of k_fast_count: the oracle's result, and the default run's on the same context"""
    ctx = Context(0)
    try:
        today = FS.expected_plan(L)
        assert today[0] == 1 and today[2] == 0
        monkeypatch.setenv("SWA_FAST_COUNT", "sites")
        graft, counters, totals = _check(ctx, case, str(L), LS.sites_plan(L, L, pair_w=today[1]), [0, SS.CAP, L, 0])
        assert ctx.d1_fastidious_plan()[2] == 1
        monkeypatch.delenv("SWA_FAST_COUNT")
        graft0, counters0, totals0 = _check(ctx, case, str(L), today, [0, SS.CAP, L, 0])
        assert np.array_equal(graft, graft0) and [int(x) for x in counters[:5]] == [int(x) for x in counters0[:5]]
        assert totals[0] == totals0[0] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("L", [150, 255])
def test_count_sites_leaves_the_register_rows_alone(case, monkeypatch, L):
    monkeypatch.setenv("SWA_FAST_COUNT", "sites")
    ctx = Context(0)
    try:
        assert FS.expected_plan(L)[2] in (5, 8)
        graft, counters, totals = _check(ctx, case, str(L), FS.expected_plan(L), [0, SS.CAP, L, 0])
        assert totals[0] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("pair_cap", [None, "64"])
def test_count_sites_on_a_long_pair_list(case, monkeypatch, pair_cap):
    """FS.shared_ends (a group of more tiles than items: thousands of pairs) with a 300-nt outlier, which moves the pass to
    k_fast_pairs_lines<13> and k_fast_count's row; once more with a pair list that has to grow"""
    monkeypatch.setenv("SWA_FAST_COUNT", "sites")
    if pair_cap:
        monkeypatch.setenv("SWA_FAST_PAIR_CAP", pair_cap)
    ctx = Context(0)
    try:
        fa, db, flags, three, want_graft, want_counters = case("shared+300")
        assert db.longest == 300
        FS.assert_not_trivial(db, flags, want_graft, three)
        graft, counters, totals = _check(ctx, case, "shared+300", LS.sites_plan(300, 300, pair_w=13), [0, SS.CAP, 300, 0])
        assert totals[0] > 64 and (totals[3] >= 2 if pair_cap else totals[3] == 1)
    finally:
        ctx.close()


def test_shards_combine_to_the_oracle(case, monkeypatch):
    monkeypatch.setenv("SWA_FAST_LONG", "pairs")
    fa, db, flags, three, want_graft, want_counters = case("2049")
    ctx = Context(0)
    try:
        merged = np.full(db.n, FS.NO_GRAFT, dtype=np.uint32)
        heavy_variants = candidates = 0
        for shard in range(3):
            got_flags, g, c = _run(ctx, fa, shard=(shard, 3))
            assert ctx.d1_fastidious_split() == [2, LS.SITES_CAP, 2049, 0] and ctx.d1_fastidious_totals()[0] > 0
            assert ctx.d1_fastidious_plan() == LS.sites_plan(2049, 2049)
            assert np.array_equal(got_flags, flags)
            assert [int(c[i]) for i in (0, 3, 4)] == [int(want_counters[i]) for i in (0, 3, 4)]
            merged = np.minimum(merged, g)
            heavy_variants += int(c[1])
            candidates += int(c[2])
        assert np.array_equal(merged, want_graft)
        assert (heavy_variants, candidates) == (int(want_counters[1]), int(want_counters[2]))
    finally:
        ctx.close()


def test_bloom_switch_and_unknown_values_change_nothing(case, monkeypatch):
    ctx = Context(0)
    try:
        ctx.upload_hostdb(HostDb(case("1025")[0]))
        for env in ({"SWA_FAST_LONG": "pairs", "SWA_FAST_BLOOM": "1"}, {"SWA_FAST_LONG": "pair"}, {"SWA_FAST_COUNT": "site"},
                    {"SWA_FAST_COUNT": "sites"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            assert ctx.d1_fastidious_plan() == FS.expected_plan(1025, bloom=True) == FS.expected_plan(1025), env
            assert ctx.d1_fastidious_split()[:2] == [0, SS.CAP], env
            for k in env:
                monkeypatch.delenv(k)
    finally:
        ctx.close()


def test_cli_under_pairs_writes_the_same_files(case, tmp_path, monkeypatch):
    """swarm -d 1 -f -o -s -i on the 1025 set: byte-identical output files with and without SWA_FAST_LONG=pairs"""
    fa = case("1025")[0]
    monkeypatch.delenv("SWA_FAST_LONG", raising=False)
    for tag, env in (("a", dict(os.environ)), ("b", dict(os.environ, SWA_FAST_LONG="pairs"))):
        cmd = [str(BIN), "-d", "1", "-f"]
        for k in "osi":
            cmd += [f"-{k}", str(tmp_path / f"{tag}{k}")]
        g = subprocess.run(cmd + ["-l", "/dev/null", str(fa)], capture_output=True, text=True, env=env, timeout=120)
        assert g.returncode == 0, g.stderr
    for k in "osi":
        assert (tmp_path / f"a{k}").stat().st_size > 0
        assert filecmp.cmp(tmp_path / f"a{k}", tmp_path / f"b{k}", shallow=False), k
