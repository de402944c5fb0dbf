"""The d >= 2 graph route (dn_graph.hip) on databases with SHORT sequences — fewer than 16 (d + 1) nucleotides, no room
for d + 1 windows.  They used to send the whole database to the fused scan; now they stay out of the window groups and
k_dg_brute finds their pairs (each against every sequence whose length differs by at most d), into the same pair list,
as long as the number B of those candidates stays within the cap (16 n + 2^20, or SWA_DN_BRUTE_CAP).

Against the reference binary, against the scan route (which does not know the new code), against alignments of all
pairs, past the cap, through a regrown pair list and from several ranks."""
import os
import subprocess

import numpy as np
import pytest

import dn_short_sets as D
import support as S
from swarm_amd import Context, DnClusters, HostDb, MultiContext, SwaError, reduced_penalties
from swarm_amd.capi import SWA_E_ARG

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
OUTS = "oisu"
REFUSED = "SWARM_AMD_DN=graph: a sequence is too short for d + 1 windows"

# (d, CLI scoring options, bulk of the mixed set, extra CLI options): the default scoring at d = 2, 3, 5; at d = 8 the
# scoring of test_align_forms_gpu's d8_generic_graph (the default one can meet the reference's 16-bit divergence there)
CASES = [
    pytest.param(2, [], ((2000, 150), (1000, 400)), [], id="d2"),
    pytest.param(3, [], ((2000, 150), (1000, 400)), [], id="d3"),
    pytest.param(3, [], ((2000, 150), (1000, 400)), ["-n"], id="d3_n"),
    pytest.param(5, [], ((2000, 150), (1000, 400)), [], id="d5"),
    pytest.param(8, ["-m", "1", "-p", "1", "-g", "1", "-e", "0"], ((1200, 160), (600, 400)), [], id="d8_generic"),
]


def _penalties(opts):
    v = {"-m": 5, "-p": 4, "-g": 12, "-e": 4}
    for k in range(0, len(opts), 2):
        v[opts[k]] = int(opts[k + 1])
    return reduced_penalties(v["-m"], v["-p"], v["-g"], v["-e"])


def _route_env(monkeypatch, route):
    monkeypatch.delenv("SWARM_AMD_DN_WALK", raising=False)
    monkeypatch.delenv("SWA_DN_BRUTE_CAP", raising=False)
    if route is None:
        monkeypatch.delenv("SWARM_AMD_DN", raising=False)
    else:
        monkeypatch.setenv("SWARM_AMD_DN", route)


def _cluster(ctx, hdb, tmp_path, tag, d, opts=(), ncb=False, want_route=None):
    """-o -i -s -u of one clustering through DnClusters, as bytes"""
    ctx.upload_hostdb(hdb)
    cl = DnClusters(ctx, hdb, d, no_cluster_breaking=ncb, penalties=_penalties(list(opts)))
    try:
        totals = cl.scan_totals()
        if want_route is not None:
            assert totals["route"] == want_route, totals
        cl.write_swarms(tmp_path / f"{tag}.o")
        cl.write_structure(tmp_path / f"{tag}.i")
        cl.write_stats(tmp_path / f"{tag}.s")
        cl.write_uclust(tmp_path / f"{tag}.u", ctx=ctx)
    finally:
        cl.close()
    return {k: (tmp_path / f"{tag}.{k}").read_bytes() for k in OUTS}, totals


def _reference(tmp_path, fa, d, opts=(), extra=()):
    cmd = ["-d", d] + list(opts) + list(extra)
    for k in OUTS:
        cmd += [f"-{k}", tmp_path / f"ref.{k}"]
    r = S.run_ref_swarm(cmd + ["-l", "/dev/null", fa])
    assert r.returncode == 0, r.stderr
    return {k: (tmp_path / f"ref.{k}").read_bytes() for k in OUTS}


def _check_inputs(recs, d):
    """what the set must be for the test to mean anything: no sequence twice, short and long sequences, B within the cap"""
    seqs = [s for _, s in recs]
    assert len(set(seqs)) == len(seqs)
    lens = np.array([len(s) for s in seqs])
    T = D.short_below(d)
    assert (lens < T).sum() > 100 and (lens >= 32 * (d + 1)).sum() > 500
    assert 0 < D.brute_candidates(lens, d) <= D.default_cap(len(seqs))


def _links_by_kind(structure: bytes, recs, d):
    """accepted links of an -i file counted by how many of their two sequences are short"""
    T = D.short_below(d)
    length = {}
    for h, s in recs:
        length[h] = len(s)
        length[h.rsplit("_", 1)[0]] = len(s)
    kinds = [0, 0, 0]
    for line in structure.decode().splitlines():
        a, b = line.split("\t")[:2]
        kinds[int(length[a] < T) + int(length[b] < T)] += 1
    return kinds


# ---- 1. + 3. against the reference binary, both ways of asking for the graph --------------------------------------------------
@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("route", [None, "graph"], ids=["default", "graph"])
@pytest.mark.parametrize("d,opts,bulk,extra", CASES)
def test_mixed_set_takes_the_graph_route_and_equals_the_reference(gpu_ctx, tmp_path, monkeypatch, d, opts, bulk, extra, route):
    """Fails without the brute-force part: SWARM_AMD_DN=graph is then refused (SWA_E_ARG) for these sets and the default
    reports the route `scan`."""
    _route_env(monkeypatch, route)
    fa = tmp_path / "in.fa"
    recs = D.mixed_set(fa, d, 3100 + d, bulk)
    _check_inputs(recs, d)
    want = _reference(tmp_path, fa, d, opts, extra)
    hdb = HostDb(fa, check_duplicate_sequences=True)
    got, totals = _cluster(gpu_ctx, hdb, tmp_path, "gpu", d, opts, "-n" in extra, want_route="graph")
    assert totals["qgram_comparisons"] >= D.brute_candidates([len(s) for _, s in recs], d)
    for k in OUTS:
        assert got[k] == want[k], k
    # the seams were met: links between two long, a short and a long, and two short sequences
    kinds = _links_by_kind(want["i"], recs, d)
    assert min(kinds) > 0, kinds


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("d,opts,bulk,extra", [CASES[1], CASES[4]])
def test_mixed_set_through_the_command_line(tmp_path, d, opts, bulk, extra):
    fa = tmp_path / "in.fa"
    D.mixed_set(fa, d, 3100 + d, bulk)
    want = _reference(tmp_path, fa, d, opts, extra)
    env = {k: v for k, v in os.environ.items() if k not in ("SWARM_AMD_DN_WALK", "SWA_DN_BRUTE_CAP")}
    for route in (None, "graph"):
        cmd = [str(BIN), "-d", str(d)] + list(opts) + list(extra)
        for k in OUTS:
            cmd += [f"-{k}", str(tmp_path / f"cli.{k}")]
        env.pop("SWARM_AMD_DN", None)
        r = subprocess.run(cmd + ["-l", "/dev/null", str(fa)], capture_output=True, text=True, timeout=300,
                           env=dict(env, SWARM_AMD_DN=route) if route else env)
        assert r.returncode == 0, r.stderr
        for k in OUTS:
            assert (tmp_path / f"cli.{k}").read_bytes() == want[k], (route, k)


# ---- 2. the same graph as the scan route, and as alignments of all pairs ------------------------------------------------------
@pytest.mark.parametrize("d,opts,bulk,extra", CASES)
def test_mixed_set_default_route_equals_the_scan(gpu_ctx, tmp_path, monkeypatch, d, opts, bulk, extra):
    fa = tmp_path / "in.fa"
    D.mixed_set(fa, d, 3100 + d, bulk)
    hdb = HostDb(fa, check_duplicate_sequences=True)
    _route_env(monkeypatch, "scan")
    scan, _ = _cluster(gpu_ctx, hdb, tmp_path, "scan", d, opts, "-n" in extra, want_route="scan")
    _route_env(monkeypatch, None)
    graph, _ = _cluster(gpu_ctx, hdb, tmp_path, "graph", d, opts, "-n" in extra, want_route="graph")
    for k in OUTS:
        assert graph[k] == scan[k], k


def test_fragments_far_below_leave_the_windows_at_32(gpu_ctx, tmp_path, monkeypatch):
    """400-nt amplicons plus fragments of 1-40 nt, d = 3: nothing between 64 and 128 nt, so the long sequences keep their
    windows of 32 (the shape of the one-primer-dimer-in-a-million case)"""
    d = 3
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 2500, 400, 3200, d)
    long_recs = [(h.decode(), s.decode()) for h, s in S.read_fasta(fa)]
    assert min(len(s) for _, s in long_recs) >= 32 * (d + 1)
    short = D.short_material(np.random.default_rng(3201), d, {s for _, s in long_recs}, straddlers=0, below=20)
    fa.write_text("".join(f">{h}\n{s}\n" for h, s in long_recs + short))
    hdb = HostDb(fa, check_duplicate_sequences=True)
    _route_env(monkeypatch, "scan")
    scan, _ = _cluster(gpu_ctx, hdb, tmp_path, "scan", d, want_route="scan")
    _route_env(monkeypatch, None)
    graph, _ = _cluster(gpu_ctx, hdb, tmp_path, "graph", d, want_route="graph")
    for k in OUTS:
        assert graph[k] == scan[k], k
    kinds = _links_by_kind(graph["i"], long_recs + short, d)
    assert kinds[0] > 1000 and kinds[2] > 20, kinds


@pytest.mark.parametrize("d,ncb", [(2, False), (3, True), (5, False)])
def test_graph_of_a_small_mixed_set_equals_alignments_of_all_pairs(tmp_path, monkeypatch, d, ncb):
    """swa_dn_graph's CSR against swa_search_do of every sequence against every other: a link q -> t for every pair
    within d differences, towards the higher id always and towards the lower one when the abundances tie (or with -n)"""
    _route_env(monkeypatch, None)
    rng = np.random.default_rng(40 + d)
    seen = set()
    T = D.short_below(d)
    recs = D.short_material(rng, d, seen, straddlers=12, below=6)
    recs += D.families(rng, "l", 12, 8, [T + d, T + d + 1, 2 * T + 5, 150], d, seen)
    fa = tmp_path / "in.fa"
    fa.write_text("".join(f">{h}\n{s}\n" for h, s in recs))
    hdb = HostDb(fa, check_duplicate_sequences=True)
    n = hdb.n
    assert 200 < n < 600
    m = MultiContext([0])
    try:
        m.upload_hostdb(hdb)
        got = m.dn_graph(d, ncb)
    finally:
        m.close()
    assert got is not None
    off, nb, df = got
    ctx = Context(0)
    try:
        ctx.upload_hostdb(hdb)
        ctx.search_begin(18, 24, 13, d)
        abundance = np.asarray(hdb.abundance)
        woff, wnb, wdf = [0], [], []
        for q in range(n):
            targets = np.array([t for t in range(n) if t != q], dtype=np.uint64)
            _, diffs, _ = ctx.search_do(q, targets, lengths=False)
            for t, diff in zip(targets.tolist(), diffs.tolist()):
                if diff <= d and (t > q or ncb or abundance[t] == abundance[q]):
                    wnb.append(t)
                    wdf.append(diff)
            woff.append(len(wnb))
    finally:
        ctx.close()
    assert len(wnb) > n
    assert np.array_equal(off, np.array(woff, dtype=np.uint64))
    assert np.array_equal(nb, np.array(wnb, dtype=np.uint32))
    assert np.array_equal(df, np.array(wdf, dtype=np.uint8))


# ---- 4. past the cap: the scan serves, and asking for the graph is refused as before ------------------------------------------
def _expect_scan_and_refusal(gpu_ctx, tmp_path, monkeypatch, fa, d):
    hdb = HostDb(fa, check_duplicate_sequences=True)
    monkeypatch.delenv("SWARM_AMD_DN", raising=False)
    got, _ = _cluster(gpu_ctx, hdb, tmp_path, "auto", d, want_route="scan")
    monkeypatch.setenv("SWARM_AMD_DN", "graph")
    gpu_ctx.upload_hostdb(hdb)
    with pytest.raises(SwaError) as e:
        DnClusters(gpu_ctx, hdb, d)
    assert e.value.code == SWA_E_ARG and REFUSED in str(e.value)
    monkeypatch.delenv("SWARM_AMD_DN", raising=False)
    if S.have_reference():
        want = _reference(tmp_path, fa, d)
        for k in OUTS:
            assert got[k] == want[k], k
    return got


def test_brute_cap_of_zero_sends_a_mixed_set_to_the_scan(gpu_ctx, tmp_path, monkeypatch):
    d = 3
    fa = tmp_path / "in.fa"
    D.mixed_set(fa, d, 3100 + d)
    _route_env(monkeypatch, None)
    monkeypatch.setenv("SWA_DN_BRUTE_CAP", "0")
    _expect_scan_and_refusal(gpu_ctx, tmp_path, monkeypatch, fa, d)
    # ... and a cap of exactly B serves it on the graph route again, B - 1 does not
    recs = S.read_fasta(fa)
    b = D.brute_candidates([len(s) for _, s in recs], d)
    hdb = HostDb(fa, check_duplicate_sequences=True)
    monkeypatch.setenv("SWA_DN_BRUTE_CAP", str(b))
    _cluster(gpu_ctx, hdb, tmp_path, "at", d, want_route="graph")
    monkeypatch.setenv("SWA_DN_BRUTE_CAP", str(b - 1))
    _cluster(gpu_ctx, hdb, tmp_path, "below", d, want_route="scan")


def test_all_short_set_past_the_default_cap_goes_to_the_scan(gpu_ctx, tmp_path, monkeypatch):
    """1 700 sequences of 40 nt at d = 2: every pair is a candidate, n (n - 1) / 2 > 16 n + 2^20"""
    d = 2
    rng = np.random.default_rng(17)
    seen = set()
    recs = D.families(rng, "f", 60, 5, [40], 1, seen)
    recs = [(h, s) for h, s in recs if len(s) == 40]
    k = 0
    while len(recs) < 1700:
        s = "".join("ACGT"[v] for v in rng.integers(0, 4, 40))
        if s not in seen:
            seen.add(s)
            recs.append((f"r{k}_{int(rng.choice([1, 2, 3]))}", s))
            k += 1
    lens = [len(s) for _, s in recs]
    assert D.brute_candidates(lens, d) == 1700 * 1699 // 2 > D.default_cap(1700)
    fa = tmp_path / "in.fa"
    fa.write_text("".join(f">{h}\n{s}\n" for h, s in recs))
    _route_env(monkeypatch, None)
    got = _expect_scan_and_refusal(gpu_ctx, tmp_path, monkeypatch, fa, d)
    assert got["i"].count(b"\n") > 50


def test_all_short_set_within_the_cap_takes_the_graph_route(gpu_ctx, tmp_path, monkeypatch):
    """no long sequence at all: the windows find nothing, the brute-force part everything"""
    d = 2
    rng = np.random.default_rng(18)
    recs = D.short_material(rng, d, set(), straddlers=0, below=40)
    assert max(len(s) for _, s in recs) < D.short_below(d)
    fa = tmp_path / "in.fa"
    fa.write_text("".join(f">{h}\n{s}\n" for h, s in recs))
    hdb = HostDb(fa, check_duplicate_sequences=True)
    _route_env(monkeypatch, "scan")
    scan, _ = _cluster(gpu_ctx, hdb, tmp_path, "scan", d, want_route="scan")
    _route_env(monkeypatch, "graph")
    graph, totals = _cluster(gpu_ctx, hdb, tmp_path, "graph", d, want_route="graph")
    assert totals["qgram_comparisons"] == D.brute_candidates([len(s) for _, s in recs], d)
    assert graph["i"].count(b"\n") > 50
    for k in OUTS:
        assert graph[k] == scan[k], k


# ---- 5. the pair list regrows with brute-force pairs in it --------------------------------------------------------------------
def test_pair_list_regrows_with_short_families_in_it(tmp_path, monkeypatch):
    """test_dn_scale_gpu's set that overflows the first pair list through the windows (60 tight families x 500 long
    members, d = 2) plus short families: the second attempt repeats the brute-force pass; outputs equal the scan's."""
    import test_dn_scale_gpu as T
    d = 2
    fa = tmp_path / "in.fa"
    T._tight_families(fa, 60, 500, 150, 404)
    long_recs = [(h.decode(), s.decode()) for h, s in S.read_fasta(fa)]
    seen = {s for _, s in long_recs}
    short = D.short_material(np.random.default_rng(405), d, seen, straddlers=30, below=30)
    fa.write_text("".join(f">{h}\n{s}\n" for h, s in long_recs + short))
    hdb = HostDb(fa, check_duplicate_sequences=True)
    n = hdb.n
    assert n == 30_000 + len(short)
    _route_env(monkeypatch, None)
    out = {}
    for route in ("graph", "scan"):
        monkeypatch.setenv("SWARM_AMD_DN", route)
        ctx = Context(0)                                      # (fresh: the pair list's capacity lives in the context)
        try:
            out[route], totals = _cluster(ctx, hdb, tmp_path, route, d, want_route=route)
            if route == "graph":
                assert totals["aligned_pairs"] > 2 * (16 * n + (1 << 20)), totals
        finally:
            ctx.close()
    for k in OUTS:
        assert out["graph"][k] == out["scan"][k], k
    kinds = _links_by_kind(out["graph"]["i"], long_recs + short, d)
    assert min(kinds) > 0, kinds


# ---- 6. several ranks: every brute-force pair from exactly one of them --------------------------------------------------------
@pytest.mark.parametrize("ncb", [False, True])
def test_ranks_add_up_to_the_single_graph_on_a_mixed_set(tmp_path, monkeypatch, ncb):
    _route_env(monkeypatch, None)
    d = 3
    fa = tmp_path / "in.fa"
    D.mixed_set(fa, d, 3100 + d)
    hdb = HostDb(fa)
    want = None
    for devices in ([0], [0, 0], [0, 0, 0]):
        m = MultiContext(devices)
        try:
            m.upload_hostdb(hdb)
            got = m.dn_graph(d, ncb)
        finally:
            m.close()
        assert got is not None
        if want is None:
            want = got
            assert len(got[1]) > 1000
        else:
            for a, b in zip(got, want):
                assert np.array_equal(a, b)
