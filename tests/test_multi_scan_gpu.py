"""The d >= 2 scan route divided among several ranks (swa_multi_scan_*, multi.hip over scan.hip's owned kernel forms): rank
r scans the amplicons i with (i >> 5) % world == r against every seed, the host merges the ranks' hits.  All ranks run
on device 0.  Every call is compared exactly with the plain model of tests/scan_model.py — triples, return codes, nhits
and what the call adds to the totals —, the rare branches are checked per rank through swa_multi_ctx, and the command
line is compared with the reference's files and with the single-GPU run."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import multi_scan_sets as MX
import scan_model as M
import scan_sets as X
import support as S
from swarm_amd import MultiContext, scan_owner_for, scan_share_for

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
G = S.GOLDEN
FLAG = {"o": "-o", "s": "-s", "i": "-i", "w": "-w", "u": "-u"}


@pytest.fixture(scope="module")
def multis():
    made = {}

    def get(world: int) -> MultiContext:
        if world not in made:
            made[world] = MultiContext([0] * world)
        return made[world]
    yield get
    for m in made.values():
        m.close()


_SETS = {}


def _set(name: str):
    """(db, d, ncb, model, the model's whole greedy walk): made once, shared by the worlds (the model's caches with it)"""
    if name not in _SETS:
        if name == "chain":
            db, d, ncb = X.chain_set()[0], 2, False
        elif name in ("tie", "tie_ncb"):
            db, d, ncb = X.tie_set()[0], 3, name == "tie_ncb"
        elif name == "star":
            db, d, ncb = X.star_set()[0], 2, False
        else:
            raise ValueError(name)
        model = M.ScanModel(db, d)
        _SETS[name] = (db, d, ncb, model, M.model_greedy(model, ncb))
    return _SETS[name]


# ------------------------------------------------------------------------------------------------ lock-step with the model

@pytest.mark.parametrize("world", MX.WORLDS)
@pytest.mark.parametrize("name", ["chain", "tie", "tie_ncb", "star"])
def test_walk_in_lockstep_with_the_model(multis, name, world):
    db, d, ncb, model, want = _set(name)
    m = multis(world)
    before = MX.rank_states(m)
    lock = MX.MultiLockstep(m, db, d, ncb, model=model)
    got = lock.walk()
    assert got == want
    if name == "chain":                                    # the sub-seed c8 outgrows the first candidate list: on every rank that holds a part of it
        assert any(x["relists"] >= 1 for x in MX.rank_deltas(m, before))
    if name == "star":                                     # one batch of 2260 sub-seeds
        assert max(len(c[0]) for c in lock.calls) > 0 and any(len(set(k for k, _, _ in c[0])) > 1 for c in lock.calls)
    # launch sequences are batches, not a sum; a rank launches only while it owns an amplicon at or above lowest_unswarmed
    per_rank = [m.ctx(r).scan_totals() for r in range(world)]
    assert m.scan_totals()["launch_sequences"] == len(lock.calls) >= max(t["launch_sequences"] for t in per_rank)
    if world == 1:
        assert per_rank[0] == m.scan_totals()
    assert sum(t["aligned_pairs"] for t in per_rank) == sum(c[2] for c in lock.calls)


@pytest.mark.parametrize("world", [2, 3])
def test_chain_with_lowest_unswarmed_raised(multis, world):
    """scan_sets.run_chain's raised walk: later generations with lowest_unswarmed moved up to c3, the w* left to later swarms"""
    db, ids = X.chain_set()
    d = 2
    model = _set("chain")[3]
    lo_of = lambda gen, lo: max(lo, ids["c3"]) if gen >= 2 else lo
    log = X.model_walk(model, lo_of=lo_of)
    lock = MX.MultiLockstep(multis(world), db, d, model=model)
    swarms, _ = lock.walk(lo_of=lo_of)
    assert len(swarms) > 1 and len(lock.calls) == len(log)


# ------------------------------------------------------------------------------------------------ edges of the blocks

@pytest.fixture(scope="module")
def wide():
    return MX.wide_tie_set()


def _edge_sizes(world: int) -> list:
    return sorted({1, 31, 32, 33, 32 * world - 1, 32 * world, 32 * world + 1})


@pytest.mark.parametrize("world", [2, 3, 8])
def test_block_edges(multis, wide, world):
    d = 3
    m = multis(world)
    crossed_first = crossed_later = False
    for n in _edge_sizes(world):
        db = MX.cut(wide, n)
        model = M.ScanModel(db, d)
        want = M.model_greedy(model)
        lock = MX.MultiLockstep(m, db, d, model=model)
        # the whole walk: lowest_unswarmed = seed + 1 passes through every place of every block, and ends at n
        assert lock.walk() == want, n
        shares = [scan_share_for(n, 0, r, world)[0] for r in range(world)]
        assert sum(shares) == n
        launched = [m.ctx(r).scan_totals()["launch_sequences"] for r in range(world)]
        for r in range(world):                             # a rank without an amplicon has launched nothing at all
            assert shares[r] != 0 or launched[r] == 0, (n, r, launched)
        if n == 33 and world == 8:
            assert shares == [32, 1, 0, 0, 0, 0, 0, 0] and launched[2:] == [0] * 6 and launched[0] > 0 and launched[1] > 0
        # seeds owned by another rank than their hits, in a first generation and in a later one
        model.begin()
        for gen, seeds, hits, _, _, _ in X.model_walk(model):
            for k, i, _ in hits:
                if scan_owner_for(seeds[k], world) != scan_owner_for(i, world):
                    crossed_first |= gen == 0
                    crossed_later |= gen > 0
        # lowest_unswarmed inside a block, on a block edge, at n and above n (always above the seeds so far)
        lock.begin()
        for seed, lo in ((0, min(17, n)), (min(17, n - 1), 32), (min(40, n - 1), 64), (n - 1, n), (n - 1, n + 5)):
            if seed < lo:
                first = lock.call([seed], [0], lo, True)
                if first and lo < n:
                    lock.call([i for _, i, _ in first], [df for _, _, df in first], lo + 1, False)
    assert crossed_first and crossed_later


# ------------------------------------------------------------------------------------------------ the rare branches, per rank

def test_pair_overflow_on_one_rank_only():
    """a process of its own under SWA_SCAN_PAIR_CAP: rank 0's share of one batch's pairs exceeds the starting capacity,
    rank 1's does not; rank 0 alone repeats its pass (multi_scan_sets.run_lopsided)"""
    code = (f"import sys\nsys.path[:0] = [{str(S.ROOT)!r}, {str(S.ROOT / 'tests')!r}]\n"
            f"import multi_scan_sets\nmulti_scan_sets.child('lopsided', {MX.OVERFLOW_CAP})\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(os.environ, SWA_SCAN_PAIR_CAP=str(MX.OVERFLOW_CAP)), timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr


def test_more_hits_than_the_mirror_on_one_rank():
    """two_shell_set at 190 x 180: the second-generation batch has 34200 hits, more than 16384 of them on one rank of two
    and fewer on the other (counted on the model with swa_scan_owner_for); that rank alone fetches by copy"""
    d, n_a, n_b = 8, 190, 180
    db, _ = X.two_shell_set(3, 120, n_a, n_b)
    model = M.ScanModel(db, d)
    log = X.model_walk(model)
    gen, seeds, hits, _, _, _ = log[1]
    assert gen == 1 and len(seeds) == n_a and len(hits) == n_a * n_b
    per_rank = np.bincount([scan_owner_for(i, 2) for _, i, _ in hits], minlength=2)
    assert per_rank.max() > X.MIRROR_HITS >= per_rank.min(), per_rank
    m = MultiContext([0, 0])
    try:
        before = MX.rank_states(m)
        lock = MX.MultiLockstep(m, db, d, model=model)
        swarms, _ = lock.walk()
        assert len(swarms) == 1 and len(swarms[0]) == db.n
        delta = MX.rank_deltas(m, before)
        assert [x["by_copy"] for x in delta] == [int(c > X.MIRROR_HITS) for c in per_rank], (delta, per_rank)
        # the same batch with room for 100 hits: SWA_E_CAPACITY with the whole count, then swa_multi_scan_fetch
        lock.begin()
        first = lock.call([0], [0], 1, True)
        assert len(first) == n_a
        lock.call([i for _, i, _ in first], [df for _, _, df in first], 1, False, cap=100)
    finally:
        m.close()


def test_hit_buffer_too_small(multis):
    db, d, ncb, model, _ = _set("star")
    for world in (2, 3):
        lock = MX.MultiLockstep(multis(world), db, d, ncb, model=model)
        first = lock.call([0], [0], 1, True, cap=100)          # (Lockstep.call: SWA_E_CAPACITY, nhits = all, then the fetch)
        assert len(first) > 2000
        lock.call([i for _, i, _ in first], [df for _, _, df in first], 1, False, cap=0)


def test_refusals(multis):
    db, d, ncb, model, _ = _set("tie")
    fresh = MultiContext([0, 0])
    try:
        fresh.upload_db(db.seqs, db.seq_off, db.seqlen, db.abundance, db.longest)
        fresh.dn_begin(d)
        rc, nh, *_ = fresh.scan_batch([0], [0], 1, True, False)      # before swa_multi_scan_begin
        assert rc == X.SWA_E_ARG
        fresh.scan_begin()
        t = fresh.scan_totals()
        assert (t["qgram_comparisons"], t["aligned_pairs"], t["launch_sequences"]) == (0, 0, 0)
    finally:
        fresh.close()
    for world in (1, 3):
        lock = MX.MultiLockstep(multis(world), db, d, ncb, model=model)
        lock.refused([0, 1], [0, 0], 2, True)                        # two seeds in a first generation
        lock.refused([db.n], [0], 1, True)                           # a seed >= n
        lock.refused([0, db.n + 7], [0, 0], 1, False)
        lock.call([0], [0], 1, True)                                 # and the scan goes on as if nothing had been asked


# ------------------------------------------------------------------------------------------------ command line

def _cli(args, kinds, fasta, out, env):
    out.mkdir()
    cmd = [str(BIN)] + args
    for k in kinds:
        cmd += [FLAG[k], str(out / k)]
    cmd += ["-l", str(out / "log"), str(fasta)]
    keep = {k: v for k, v in os.environ.items() if k not in ("SWARM_AMD_DEVICES", "SWARM_AMD_DN", "SWARM_AMD_MULTI_SCAN", "SWARM_AMD_MULTI_REPORT")}
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(keep, **env))
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("name", ["d2_small", "d3_400", "d5_ties", "d8_16bit"])
@pytest.mark.parametrize("devices", ["0,0", "0,0,0"])
def test_cli_scan_with_several_ranks_matches_reference_files(tmp_path, name, devices):
    """The golden d >= 2 cases (files written by the unmodified reference) under SWARM_AMD_DN=scan through 2 and 3 ranks"""
    args = (G / f"{name}.args").read_text().split()
    kinds = [k for k in FLAG if (G / f"{name}.{k}").exists()]
    r = _cli(args, kinds, G / f"{name}.fasta", tmp_path / "run",
             {"SWARM_AMD_DEVICES": devices, "SWARM_AMD_DN": "scan", "SWARM_AMD_MULTI_REPORT": "1"})
    for k in kinds:
        assert filecmp.cmp(tmp_path / "run" / k, G / f"{name}.{k}", shallow=False), k
    ranks = devices.count(",") + 1
    assert f"multi: scan divided among {ranks} ranks" in r.stderr.splitlines(), r.stderr


def test_cli_d17_takes_the_divided_scan_without_a_switch(tmp_path):
    """-d 17 is beyond the graph route: several ranks divide the scan by default, SWARM_AMD_MULTI_SCAN=root leaves it to
    rank 0; both write the files and the log of the single-GPU run, and the report names the route"""
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 3000, 200, 91, 12)
    kinds, args = "osiwu", ["-d", "17"]
    one = _cli(args, kinds, fa, tmp_path / "one", {"SWARM_AMD_MULTI_REPORT": "1"})
    assert "multi:" not in one.stderr
    summary = lambda p: [ln for ln in (p / "log").read_text().splitlines() if ln.startswith(("Number", "Largest", "Max"))]
    assert len(summary(tmp_path / "one")) == 3
    for tag, env, line in (("two", {"SWARM_AMD_DEVICES": "0,0"}, "multi: scan divided among 2 ranks"),
                           ("three", {"SWARM_AMD_DEVICES": "0,0,0"}, "multi: scan divided among 3 ranks"),
                           ("root", {"SWARM_AMD_DEVICES": "0,0", "SWARM_AMD_MULTI_SCAN": "root"}, "multi: scan on rank 0 alone")):
        r = _cli(args, kinds, fa, tmp_path / tag, dict(env, SWARM_AMD_MULTI_REPORT="1"))
        lines = r.stderr.splitlines()
        assert line in lines and sum(ln.startswith("multi: scan") for ln in lines) == 1, r.stderr
        for k in kinds:
            assert filecmp.cmp(tmp_path / "one" / k, tmp_path / tag / k, shallow=False), (tag, k)
        assert summary(tmp_path / tag) == summary(tmp_path / "one")
    assert (tmp_path / "one" / "o").read_text().count("\n") < 3000          # (swarms of more than one member exist)


def test_binding_runs_the_cluster_call_and_names_the_route(tmp_path):
    """MultiContext.dn_cluster: route() and the totals of the divided scan = those of one context"""
    from swarm_amd import Context, DnClusters, HostDb
    hdb = HostDb(G / "d5_ties.fasta")
    old = os.environ.get("SWARM_AMD_DN")
    os.environ["SWARM_AMD_DN"] = "scan"
    try:
        ctx = Context(0)
        ctx.upload_hostdb(hdb)
        single = DnClusters(ctx, hdb, 5)
        assert single.route() == ("scan", 1)
        want = single.scan_totals()
        m = MultiContext([0, 0, 0])
        m.upload_hostdb(hdb)
        cl = m.dn_cluster(hdb, 5)
        assert cl.route() == ("scan", 3)
        assert cl.scan_totals() == want and cl.summary() == single.summary()
        cl.write_swarms(tmp_path / "o")
        single.write_swarms(tmp_path / "o1")
        cl.write_stats(tmp_path / "s")
        assert (tmp_path / "o").read_bytes() == (tmp_path / "o1").read_bytes()
        assert (tmp_path / "s").read_bytes() == (G / "d5_ties.s").read_bytes()
        for h in (cl, single, m, ctx):
            h.close()
    finally:
        if old is None:
            del os.environ["SWARM_AMD_DN"]
        else:
            os.environ["SWARM_AMD_DN"] = old
