"""The d >= 2 graph route (dn_graph.hip -> the walk of cluster_gpu.hip -> cluster_on_device, host/cluster_dn.cpp) past
the sizes its buffers are laid out for, each against an independent computation:

  * 2^20 amplicons: swa_d1_cluster_device faults the host pages of its result arrays in (swa_touch_pages, from 4 MiB on)
    — before the downloads into them are queued, not after (it used to clear a byte a page of generation / parent);
  * one window shared by ~100 k amplicons: a group's blocks of k_dg_pairs_lds grow with t q, the item list linearly
    with n — the items are capped a group and the blocks dealt round-robin (items past the cap used to be dropped);
  * more aligned pairs than the first pair list holds (16 n + 2^20): the search runs again with room for them all."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import support as S
from swarm_amd import Context, D1Clusters, DnClusters, HostDb, MultiContext

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
OUTS = ("o", "s", "i", "w")


def _cli(tmp_path, tag, fa, d, env=None, extra=(), timeout=300):
    cmd = [str(BIN), "-d", str(d)] + list(extra)
    for k in OUTS:
        cmd += [f"-{k}", str(tmp_path / f"{tag}.{k}")]
    cmd += ["-l", str(tmp_path / f"{tag}.log"), str(fa)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(_clean_env(), **(env or {})))
    assert r.returncode == 0, r.stderr
    return {k: (tmp_path / f"{tag}.{k}").read_bytes() for k in OUTS}


def _clean_env():
    return {k: v for k, v in os.environ.items() if k not in ("SWARM_AMD_DN", "SWARM_AMD_DN_WALK", "SWARM_AMD_CLUSTER_TIMING")}


def _count_records(fa) -> int:
    with open(fa, "rb") as fh:
        return sum(1 for line in fh if line.startswith(b">"))


# ---- 1. the 2^20 boundary through the command line ----------------------------------------------------------------------------
def test_cli_d2_at_two_to_the_twenty_walks_the_graph_like_the_host(tmp_path):
    """-d 2 -o -s -i -w on 2^20 amplicons: the walk on the device (as it runs, and with SWARM_AMD_CLUSTER_TIMING=1, which
    synchronises before the page touch — read once a process, hence fresh processes), byte for byte the host's walk over
    the downloaded graph (SWARM_AMD_DN_WALK=host)."""
    n = 1 << 20
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, n, 150, 2020, 2)
    assert _count_records(fa) == n
    assert n * 4 >= 4 << 20                                       # the result arrays are where swa_touch_pages starts
    host = _cli(tmp_path, "host", fa, 2, {"SWARM_AMD_DN_WALK": "host"})
    dev = _cli(tmp_path, "dev", fa, 2)
    timed = _cli(tmp_path, "timed", fa, 2, {"SWARM_AMD_CLUSTER_TIMING": "1"})
    assert host["o"].count(b"\n") > 1000
    for k in OUTS:
        assert dev[k] == host[k], k
        assert timed[k] == host[k], k


# ---- 2. the 2^20 boundary through the C ABI: all five result arrays -------------------------------------------------------------
def _d1_device_equals_serial_walk(fa) -> None:
    hdb = HostDb(fa)
    ctx = Context(0)
    try:
        ctx.upload_hostdb(hdb)
        assert ctx.d1_index_build() is False
        total = ctx.d1_network_resident(False)
        off, nb = ctx.d1_network_fetch(total)
        sid, gen, par, order, begins = ctx.d1_cluster_device()
    finally:
        ctx.close()
    os.environ["SWARM_AMD_CLUSTER"] = "serial"
    try:
        host = D1Clusters(hdb, off, nb)
    finally:
        del os.environ["SWARM_AMD_CLUSTER"]
    hsid, hgen, hpar = host.swarmid(), host.generation(), host.parent()
    assert np.array_equal(sid, hsid)
    assert np.array_equal(gen, hgen)
    assert np.array_equal(par, hpar)
    # members by (swarm, generation, id); begins = where each swarm starts, then n
    assert np.array_equal(order, np.lexsort((np.arange(hdb.n), hgen, hsid)).astype(np.uint32))
    want_begins = np.concatenate(([0], np.cumsum(np.bincount(hsid)))).astype(np.uint32)
    assert np.array_equal(begins, want_begins)
    assert host.summary()["swarms"] == len(begins) - 1 > 1000


@pytest.mark.parametrize("timing", [False, True])
def test_device_clustering_at_two_to_the_twenty_equals_the_serial_walk(tmp_path, timing):
    """swa_d1_cluster_device with swarmid, generation, parent, order and begins all requested, d = 1, n = 2^20, against
    the serial host walk of the same network; timing = in a fresh process with SWARM_AMD_CLUSTER_TIMING=1."""
    n = 1 << 20
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, n, 150, 1048)
    assert _count_records(fa) == n
    if not timing:
        _d1_device_equals_serial_walk(fa)
        return
    env = dict(_clean_env(), SWARM_AMD_CLUSTER_TIMING="1", PYTHONPATH=os.pathsep.join([str(S.ROOT), str(S.ROOT / "tests")]))
    code = f"import test_dn_scale_gpu as T; T._d1_device_equals_serial_walk({str(fa)!r}); print('ok')"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=str(S.ROOT))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


# ---- 3. one window shared by the whole database -------------------------------------------------------------------------------
def _edit(rng, s: str, lo: int) -> str:
    p = int(rng.integers(lo, len(s)))
    how = int(rng.integers(0, 3))
    b = "ACGT"[int(rng.integers(0, 4))]
    return s[:p] + b + s[p + 1:] if how == 0 else (s[:p] + s[p + 1:] if how == 1 else s[:p] + b + s[p:])


def _giant_window_set(path, n: int, length: int, d: int, wlen: int, seed: int) -> None:
    """n distinct amplicons in families of ~20: every centroid starts with the same wlen nucleotides (one window-0 group
    for all), members 0..d edits from their centroid, none inside that first window; abundances with ties."""
    rng = np.random.default_rng(seed)
    head = "".join("ACGT"[v] for v in rng.integers(0, 4, wlen))
    seen, recs = set(), []
    fam = 0
    while len(recs) < n:
        cent = head + "".join("ACGT"[v] for v in rng.integers(0, 4, length - wlen))
        for m in range(20):
            s = cent
            for _ in range(int(rng.integers(1, d + 1)) if m else 0):
                s = _edit(rng, s, wlen)
            if s in seen or len(recs) == n:
                continue
            seen.add(s)
            ab = int(rng.choice([5, 5, 8, 20])) if m == 0 else int(rng.choice([1, 1, 1, 2, 3]))
            recs.append((f"f{fam}m{m}_{ab}", s))
        fam += 1
    path.write_text("".join(f">{h}\n{s}\n" for h, s in recs))


def _item_cap(n: int, d: int) -> int:
    return n + n * (2 * d + 2) // 2 + 64       # swa_dn_graph_compute's item_cap


def _overflow_size(d: int) -> int:
    """the smallest window group that, holding the whole database, made more blocks than item_cap (uncapped items)"""
    g = 2
    while (g + 63) // 64 * ((g + 255) // 256) <= _item_cap(g, d):
        g += 64
    return g


def _gpu_graph_rows_equal_the_oracle(fa, d: int, rows: int, seed: int) -> None:
    """the graph (swa_dn_graph) row by row for a seeded sample of queries against q-gram signatures (orc_findqgrams), the
    popcount bound over all n targets, orc_nw_diff on the survivors and the direction rule of k_dg_worklist"""
    hdb = HostDb(fa)
    m = MultiContext([0])
    try:
        m.upload_hostdb(hdb)
        got = m.dn_graph(d)
    finally:
        m.close()
    assert got is not None
    off, nb, df = got
    db = S.db_from_fasta(fa)
    n = db.n
    assert n == hdb.n and db.headers[0] == hdb.header(0) and db.headers[-1] == hdb.header(n - 1)
    lib = S.oracle()
    sig = np.zeros((n, 128), dtype=np.uint8)
    for i in range(n):
        lib.orc_findqgrams(S._p(db.words(i), S.u64p), int(db.seqlen[i]), S._p(sig[i], S.u8p))
    sig64 = sig.view(np.uint64)
    lens = db.seqlen.astype(np.int64)
    rng = np.random.default_rng(seed)
    linked = 0
    for q in sorted(rng.choice(n, size=min(rows, n), replace=False).tolist()):
        pop = np.bitwise_count(sig64 ^ sig64[q]).sum(axis=1)
        cand = np.nonzero(((pop + 9) // 10 <= d) & (np.abs(lens - lens[q]) <= d))[0]
        want = []
        for t in cand.tolist():
            if t == q or (t < q and db.abundance[t] != db.abundance[q]):
                continue
            diff = lib.orc_nw_diff(S._p(db.words(t), S.u64p), int(db.seqlen[t]), S._p(db.words(q), S.u64p),
                                   int(db.seqlen[q]), 18, 24, 13, None, None)
            if diff <= d:
                want.append((t, diff))
        a, b = int(off[q]), int(off[q + 1])
        assert list(zip(nb[a:b].tolist(), df[a:b].tolist())) == want, q
        linked += len(want)
    assert linked > rows


@pytest.mark.parametrize("d,n,length,wlen", [(2, 100_000, 150, 32), (3, 130_000, 150, 32), (2, 100_000, 60, 16)])
def test_dn_graph_with_one_window_shared_by_everybody(tmp_path, d, n, length, wlen):
    """One window-0 group holding every amplicon, >= 1.5 x the size whose blocks outgrew item_cap: the graph route's
    -o -s -i -w equal the fused scan's (no windows, no items) and the reference's; sampled graph rows equal the oracle's."""
    fa = tmp_path / "in.fa"
    _giant_window_set(fa, n, length, d, wlen, 500 + d + length)
    recs = S.read_fasta(fa)
    assert len(recs) == n
    shortest = min(len(s) for _, s in recs)
    assert (32 if shortest >= 32 * (d + 1) else 16 if shortest >= 16 * (d + 1) else 0) == wlen
    largest = Counter(s[:wlen] for _, s in recs).most_common(1)[0][1]
    assert largest >= 1.5 * _overflow_size(d), (largest, _overflow_size(d))
    env = _clean_env()
    graph = _cli(tmp_path, "graph", fa, d, {"SWARM_AMD_DN": "graph"})
    scan = _cli(tmp_path, "scan", fa, d, {"SWARM_AMD_DN": "scan"})
    assert graph["o"].count(b"\n") > 1000
    for k in OUTS:
        assert graph[k] == scan[k], k
    if S.have_reference():
        r = subprocess.run([str(S.ref_swarm_bin()), "-d", str(d), "-t", "16", "-o", str(tmp_path / "ro"), "-s", str(tmp_path / "rs"),
                            "-i", str(tmp_path / "ri"), "-w", str(tmp_path / "rw"), "-l", "/dev/null", str(fa)],
                           capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0, r.stderr
        for k in OUTS:
            assert graph[k] == (tmp_path / f"r{k}").read_bytes(), k
    _gpu_graph_rows_equal_the_oracle(fa, d, 256, 7 + d)


# ---- 4. more aligned pairs than the first pair list holds ---------------------------------------------------------------------
def _tight_families(path, families: int, members: int, length: int, seed: int) -> None:
    rng = np.random.default_rng(seed)
    seen, recs = set(), []
    for f in range(families):
        cent = "".join("ACGT"[v] for v in rng.integers(0, 4, length))
        seen.add(cent)
        recs.append((f"c{f}_{int(rng.choice([40, 40, 60]))}", cent))
        while len(recs) < (f + 1) * members:
            s = _edit(rng, cent, 0)
            if s not in seen:
                seen.add(s)
                recs.append((f"c{f}m{len(recs)}_{int(rng.choice([1, 1, 2, 3]))}", s))
    path.write_text("".join(f">{h}\n{s}\n" for h, s in recs))


def test_dn_graph_pair_list_regrows(tmp_path, monkeypatch):
    """60 families x 500 members within one edit of their centroid (d = 2): every pair of a family is a pair of the graph,
    far more than the first pair list (16 n + 2^20) holds — the search runs again with room, and its outputs are the scan's."""
    fa = tmp_path / "in.fa"
    _tight_families(fa, 60, 500, 150, 404)
    hdb = HostDb(fa, check_duplicate_sequences=True)
    n = hdb.n
    assert n == 30_000
    out = {}
    for route in ("graph", "scan"):
        monkeypatch.setenv("SWARM_AMD_DN", route)
        ctx = Context(0)                                      # (fresh: the pair list's capacity lives in the context)
        try:
            ctx.upload_hostdb(hdb)
            cl = DnClusters(ctx, hdb, 2)
            t = cl.scan_totals()
            assert t["route"] == route
            if route == "graph":
                assert t["aligned_pairs"] > 2 * (16 * n + (1 << 20)), t
            for k, fn in (("o", cl.write_swarms), ("s", cl.write_stats), ("i", cl.write_structure), ("w", cl.write_seeds)):
                fn(tmp_path / f"{route}.{k}")
                out[route, k] = (tmp_path / f"{route}.{k}").read_bytes()
            cl.close()
        finally:
            ctx.close()
    for k in OUTS:
        assert out["graph", k] == out["scan", k], k
    assert out["graph", "o"].count(b"\n") == 60
