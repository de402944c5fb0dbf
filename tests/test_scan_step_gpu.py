"""The fused d >= 2 scan step (scan.hip: swa_scan_begin / swa_scan_batch / swa_scan_fetch / swa_scan_totals) driven call
by call through the C ABI, next to the plain model of tests/scan_model.py fed with the same calls.  After every call,
exactly: the sorted (seed index, id, diff) triples, nhits, and the increments of the q-gram comparison and aligned pair
counts.  Every case is built for one of the step's rare branches and asserts — from the model before the GPU is asked,
from swa_scan_debug_state afterwards — that it took it:

  A  more pairs than the pair arrays hold (redo), more hits than the pinned mirror holds (copy), a hit buffer smaller
     than the result (SWA_E_CAPACITY + swa_scan_fetch)
  B  the candidate list of later generations and its re-listing, lowest_unswarmed above listed candidates
  C  more sub-seeds in a batch than 8 workgroups a compute unit; the argument checks
  D  a generation of more than 65535 sub-seeds, end to end
  E  -n, abundance ties, an empty span, tiny databases, a pool that is all swarmed
  F  a second database on a context that has scanned another one

SWA_SCAN_PAIR_CAP is read when a context first sizes its pair arrays: cases that set it run in a process of their own."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_model as M
import scan_sets as X
import support as S
from swarm_amd import Context, DnClusters, HostDb

pytestmark = pytest.mark.gpu


def _child(case: str, first_cap: int) -> str:
    code = (f"import sys\nsys.path[:0] = [{str(S.ROOT)!r}, {str(S.ROOT / 'tests')!r}]\n"
            f"import scan_sets\nscan_sets.child({case!r}, {first_cap})\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(os.environ, SWA_SCAN_PAIR_CAP=str(first_cap)), timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
    return r.stdout


# ---------------------------------------------------------------------------------------------------- A

def test_two_shells_overflow_pairs_mirror_and_hit_buffer():
    """150 x 150: 22500 pairs against 4096 places (SWA_SCAN_PAIR_CAP), 22500 hits against a mirror of 16384, then the
    same batch into a buffer of 100 hits"""
    _child("two_shell", 4096)


def test_two_shells_overflow_the_default_pair_capacity():
    """780 x 85 = 66300 pairs in one batch (80 nt: the model aligns every one of them): more than the 65536 places the
    pair arrays of a new context start with"""
    ctx = Context(0)
    try:
        X.run_two_shell(ctx, 4, 80, 780, 85, X.DEFAULT_PAIR_CAP, small_cap=None)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------- B

@pytest.fixture(scope="module")
def chain_model():
    db, _ = X.chain_set()
    return M.ScanModel(db, 2)


@pytest.mark.parametrize("raised", [False, True], ids=["plain", "lowest_unswarmed_raised"])
def test_chain_relists_candidates(gpu_ctx, chain_model, raised):
    """a chain 11 generations deep: the first list (est <= 16) lacks what c8 .. c10 reach; raised: from the batch of c2
    on, lowest_unswarmed lies above three listed, unswarmed neighbours of c2"""
    X.run_chain(gpu_ctx, raised=raised, model=chain_model)


def test_chain_relists_and_redoes_in_one_batch():
    """SWA_SCAN_PAIR_CAP=64: the batch that lists again has 81 pairs"""
    _child("chain", 64)


# ---------------------------------------------------------------------------------------------------- C

def test_many_seeds_in_one_batch_and_argument_checks(gpu_ctx):
    d = 2
    db, ids = X.star_set()
    lock = X.Lockstep(gpu_ctx, db, d)
    n = db.n
    # refused before anything is launched (a first generation is one seed; grid.y holds 65535)
    lock.refused([], [], 1, False)
    lock.refused(np.zeros(65536, dtype=np.uint32), np.zeros(65536, dtype=np.uint32), 1, False)
    lock.refused([0, 1], [0, 0], 1, True)
    lock.refused([n], [0], 1, True)
    first = lock.call([0], [0], 1, True)
    seeds, radii = [i for _, i, _ in first], [df for _, _, df in first]
    # 256 compute units x 8 workgroups = 2048: above it every sub-seed gets one workgroup
    assert len(seeds) >= 2200 and set(radii) == {1, 2}
    lock.refused(seeds + [n + 7], radii + [1], 1, False)
    lock.refused(seeds, radii, 1, True)
    hits = lock.call(seeds, radii, 1, False)
    targets = {}
    for k, i, _ in hits:
        targets.setdefault(i, []).append(k)
    assert len(targets) == 30 == n - 1 - len(seeds) and sum(len(v) > 1 for v in targets.values()) >= 10
    assert max(k for k, _, _ in hits) > 2048
    # the batch of the whole generation at the limit of grid.y: every sub-seed 29 times over + 5 = 65535 seeds, nothing left
    reps = (65535 // len(seeds)) + 1
    many = (seeds * reps)[:65535]
    assert lock.call(many, (radii * reps)[:65535], 1, False) == []


# ---------------------------------------------------------------------------------------------------- D

def test_generation_split_at_65535_subseeds(gpu_ctx, tmp_path, monkeypatch):
    """70000 sub-seeds in one generation: two batches.  Members within d of a sub-seed in either half belong to the
    first in queue order; members that only the second half reaches must still be found.  -o, -i, -s against the
    graph route walked on the host, and against the reference where it is compiled."""
    fa = tmp_path / "in.fa"
    parents = X.split_star_fasta(fa)

    def index(name: str) -> int:
        return int(name[1:])
    assert all(len(v) == 2 and index(v[0]) < X.SPLIT <= index(v[1]) for k, v in parents.items() if k.startswith("both"))
    assert all(len(v) == 2 and index(v[0]) < index(v[1]) < X.SPLIT for k, v in parents.items() if k.startswith("twin"))
    assert all(len(v) == 1 and index(v[0]) >= X.SPLIT for k, v in parents.items() if k.startswith("late"))
    assert all(len(v) == 1 and index(v[0]) < X.SPLIT for k, v in parents.items() if k.startswith("early"))
    hdb = HostDb(fa, check_duplicate_sequences=True)
    assert hdb.n == 70000 + 1 + len(parents)
    for route in ("scan", "graph"):
        monkeypatch.setenv("SWARM_AMD_DN", route)
        if route == "graph":
            monkeypatch.setenv("SWARM_AMD_DN_WALK", "host")
        before = gpu_ctx.scan_debug_state()
        gpu_ctx.upload_hostdb(hdb)
        cl = DnClusters(gpu_ctx, hdb, 2)
        assert cl.scan_totals()["route"] == route
        if route == "scan":
            assert cl.scan_totals()["launch_sequences"] == 4          # the centre, 65535 + 4465 sub-seeds, the 48
            assert X.state_delta(gpu_ctx, before)["by_copy"] >= 1     # (70000 hits of the centre)
        for suffix, writer in (("o", cl.write_swarms), ("i", cl.write_structure), ("s", cl.write_stats)):
            writer(tmp_path / (route + suffix))
        cl.close()
    for suffix in "ois":
        assert filecmp.cmp(tmp_path / ("scan" + suffix), tmp_path / ("graph" + suffix), shallow=False), suffix
    link = {}
    for line in (tmp_path / "scani").read_text().splitlines():
        p, c, df, _, gen = line.split("\t")
        link[c] = (p, int(df), int(gen))
    for name, near in parents.items():
        assert link[name] == (near[0], 1 if len(near) == 2 else 2, 2), (name, link[name], near)
    assert (tmp_path / "scano").read_text().count("\n") == 1
    if S.have_reference():
        r = S.run_ref_swarm(["-d", 2, "-o", tmp_path / "ro", "-i", tmp_path / "ri", "-s", tmp_path / "rs", "-l", "/dev/null", fa])
        assert r.returncode == 0, r.stderr
        for suffix in "ois":
            assert filecmp.cmp(tmp_path / ("scan" + suffix), tmp_path / ("r" + suffix), shallow=False), suffix


# ---------------------------------------------------------------------------------------------------- E

@pytest.mark.parametrize("ncb", [False, True], ids=["abundance_rule", "no_cluster_breaking"])
def test_rules_on_a_set_of_ties(gpu_ctx, ncb):
    d = 3
    db, _ = X.tie_set()
    lock = X.Lockstep(gpu_ctx, db, d, ncb=ncb)
    swarms, _ = lock.walk()
    assert 12 <= len(swarms) < db.n
    assert any(len(hits) == 0 and comparisons > 0 for hits, comparisons, _ in lock.calls)
    ref = M.model_greedy(M.ScanModel(db, d), ncb=not ncb)[0]
    assert [[m[0] for m in sw] for sw in ref] != [[m[0] for m in sw] for sw in swarms], "a set on which -n changes nothing"
    # lowest_unswarmed = n (and beyond): nothing to scan, nothing counted but the launch sequence
    lock.begin()
    first = lock.call([0], [0], 1, True)
    assert first
    for lo in (db.n, db.n + 5):
        assert lock.call([i for _, i, _ in first], [df for _, _, df in first], lo, False) == []
        assert lock.calls[-1] == ([], 0, 0)
    assert lock.call([1], [0], db.n, True) == []
    # a seed whose whole pool is swarmed already: every amplicon taken by hand, then one more batch
    lock.begin()
    for i in range(db.n):
        lock.call([i], [0], 0, True)
    assert lock.model.swarmed.all()
    assert lock.call([0, 5, db.n - 1], [0, 1, 2], 0, False) == []
    assert lock.calls[-1] == ([], 0, 0)


@pytest.mark.parametrize("n", [1, 2])
def test_tiny_databases(gpu_ctx, n):
    d = 2
    s = "ACGTTGCAAGGCTTACGATCGGATTACACGTGCA"
    db, _ = X.make_db([("a", 5, s), ("b", 3, X.sub(s, 17, 1))][:n])
    lock = X.Lockstep(gpu_ctx, db, d)
    swarms, links = lock.walk()
    assert len(swarms) == 1 and len(links) == n - 1 and len(lock.calls) == n
    assert lock.calls[0][1] == n - 1


# ---------------------------------------------------------------------------------------------------- F

def test_second_database_on_a_used_context(gpu_ctx, chain_model):
    """after the chain (a list re-listed to est <= 32, estimates up to 22, grown buffers): a smaller database, after
    swa_scan_begin, must give call for call what a context of its own gives"""
    X.run_chain(gpu_ctx, model=chain_model)
    used = gpu_ctx.scan_debug_state()
    assert used["relists"] >= 1 and used["pair_cap"] > 0
    d = 3
    db, _ = X.tie_set(seed=22, families=8)
    assert db.n < chain_model.db.n
    model = M.ScanModel(db, d)
    lock = X.Lockstep(gpu_ctx, db, d, model=model)
    shared = lock.walk()
    shared_calls = lock.calls
    fresh_ctx = Context(0)
    try:
        lock = X.Lockstep(fresh_ctx, db, d, model=model)
        fresh = lock.walk()
        assert lock.calls == shared_calls and fresh == shared and len(shared_calls) > len(shared[0])
    finally:
        fresh_ctx.close()
