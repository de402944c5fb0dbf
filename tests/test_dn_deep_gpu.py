"""The d >= 2 graph route (dn_graph.hip) at 9 <= d <= 16: up to 17 windows at up to 33 shifts, a length histogram of
288 entries, and the pair kernel of these d (k_dg_pairs_deep).  Before, swa_dn_graph_supported was false for d > 8.

Two oracles, neither of which knows the new code: the host's nw() (swarm_amd.nw_align_host — "diffs == nw() whenever
<= d", with pairs passed over by their length difference alone) and the same build's scan route (SWARM_AMD_DN=scan).
The sets are small: every window index and both extreme shifts are built on purpose (dn_deep_sets)."""
import os
import subprocess

import numpy as np
import pytest

import dn_deep_sets as DS
import dn_short_sets as D
import support as S
from swarm_amd import Context, DnClusters, HostDb, MultiContext, reduced_penalties
from swarm_amd.capi import SWA_E_ARG, SWA_E_CAPACITY, SWA_OK

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
DEFAULT = reduced_penalties()
NO_WFA = reduced_penalties(5, 1, 5, 7)            # -m 5 -p 1 -g 5 -e 7: the scoring of test_align_forms_gpu's d9_banded32_16
# shape -> (d, window length, families); about 200-250 sequences each (up to 6 (d + 1) - 2 a family)
SHAPES = {"d9": (9, 16, 4), "d12": (12, 16, 3), "d16": (16, 16, 2), "d9_w32": (9, 32, 4)}


@pytest.fixture(autouse=True)
def _no_route_switches(monkeypatch):
    for k in ("SWARM_AMD_DN", "SWARM_AMD_DN_WALK", "SWA_DN_BRUTE_CAP"):
        monkeypatch.delenv(k, raising=False)


class _Set:
    """A database of the tests: written once, its nw() differences computed once per scoring (the expected graphs of both
    abundance rules come from the same table)."""

    def __init__(self, tmp, name, recs, d, built=None, wlen=16):
        self.d, self.wlen, self.recs, self.built = d, wlen, recs, built
        self.path = tmp / f"{name}.fa"
        DS.write_fasta(self.path, recs)
        self.hdb = HostDb(self.path, check_duplicate_sequences=True)
        self._diffs = {}

    def expected(self, ncb, penalties=DEFAULT):
        if penalties not in self._diffs:
            self._diffs[penalties] = DS.all_pair_diffs(self.hdb, self.d, penalties)
        return DS.graph_from_diffs(self.hdb, self._diffs[penalties], self.d, ncb)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("deep")
    cache = {}

    def get(name):
        if name not in cache:
            if name in SHAPES:
                d, wlen, centres = SHAPES[name]
                recs, built = DS.family_set(900 + d + wlen, d, wlen, centres)
                cache[name] = _Set(tmp, name, recs, d, built, wlen)
            elif name == "mixed":                              # shape 3: both sides of short_below = 208 at d = 12
                d = 12
                T = D.short_below(d)
                rng = np.random.default_rng(1203)
                recs = D.families(rng, "x", 15, 10, list(range(T - 10, T + 11, 3)), d, set())
                recs = [(h, s) for h, s in recs if T - 14 <= len(s) <= T + 14]
                cache[name] = _Set(tmp, name, recs, d)
            elif name == "chains":                             # long sequences only, swarms many generations deep
                d = 12
                cache[name] = _Set(tmp, name, DS.chain_set(1208, d, DS.centre_length(d, 16), 3, 40), d)
            elif name == "lowc":
                d = 12
                cache[name] = _Set(tmp, name, DS.low_complexity_set(1205, d, DS.centre_length(d, 16)), d)
        return cache[name]
    return get


def _graph(ctx, st, ncb=False, penalties=DEFAULT):
    ctx.upload_hostdb(st.hdb)
    ctx.qgram_build()
    ctx.search_begin(*penalties, st.d)
    assert ctx.search_form(False)[1] == 65535              # these d are past the 8-bit range at both scorings
    assert ctx.dn_graph_supported()
    return ctx.dn_graph(ncb)


def _same(got, want):
    for name, a, b in zip(("offsets", "neighbours", "diffs"), got, want):
        assert np.array_equal(a, b), name


def _classes(st):
    """{(kind, k)} -> pairs (query id, target id) of a centre and the variant built for that window and shift, with the
    class checked on the strings: window k of the centre lies in the variant at the shift the kind stands for, and for
    `sub` / `mixins` / `mixdel` no earlier window lies there at any shift"""
    ids = DS.ids_by_header(st.recs, st.hdb)
    seq = dict(st.recs)
    out = {}
    for ch, kind, k, h in st.built:
        if kind == "far":
            continue
        assert DS.window_at(seq[ch], seq[h], k, DS.wanted_shift(kind, k, st.d), st.wlen), (ch, kind, k)
        if kind in ("sub", "mixins", "mixdel"):
            assert DS.first_shared_window(seq[ch], seq[h], st.d, st.wlen)[0] == k, (ch, kind, k)
        assert ids[ch] < ids[h]
        out.setdefault((kind, k), []).append((ids[ch], ids[h]))
    return out


def _row(graph, q):
    off, nb, _ = graph
    return set(nb[int(off[q]):int(off[q + 1])].tolist())


# ---- 1. + 2. every window, every extreme shift; windows of 16 and of 32 ------------------------------------------------------
@pytest.mark.parametrize("ncb", [False, True], ids=["rule", "n"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_window_and_both_extreme_shifts(gpu_ctx, sets, name, ncb):
    """Fails on a library whose graph route ends at d = 8 (dn_graph_supported is false)."""
    st = sets(name)
    d = st.d
    lens = np.asarray(st.hdb.seqlen)
    assert 190 <= st.hdb.n <= 250 and lens.min() >= D.short_below(d)
    assert (lens.min() >= 32 * (d + 1)) == (st.wlen == 32)
    want = st.expected(ncb)
    classes = _classes(st)
    # the construction is not vacuous: every class holds a pair that nw() accepts ...
    # (k = 0 has no shift -d: the window would start before the target; mixdel needs room in window k - 1)
    for k in range(d + 1):
        kinds = ["sub", "ins"] + (["del", "mixins"] if k >= 1 else []) + (["mixdel"] if k >= 1 and d - k + 1 <= st.wlen - 2 else [])
        for kind in kinds:
            assert any(t in _row(want, q) for q, t in classes[(kind, k)]), (kind, k)
    # ... and no variant d + 1 substitutions away from its centre is a neighbour of it
    ids = DS.ids_by_header(st.recs, st.hdb)
    far = [(ids[ch], ids[h]) for ch, kind, _, h in st.built if kind == "far"]
    assert len(far) == SHAPES[name][2] * (d + 1) and not any(t in _row(want, q) for q, t in far)
    _same(_graph(gpu_ctx, st, ncb), want)


# ---- 3. short and long sequences together, lengths the old histogram did not count ---------------------------------------------
@pytest.mark.parametrize("ncb", [False, True], ids=["rule", "n"])
def test_short_and_long_together_at_d12(gpu_ctx, sets, ncb):
    st = sets("mixed")
    lens = np.asarray(st.hdb.seqlen)
    T = D.short_below(st.d)
    assert 120 <= st.hdb.n <= 180
    assert ((lens >= 152) & (lens < T)).sum() > 30 and (lens >= T).sum() > 30 and lens.max() > T + 5
    assert 0 < D.brute_candidates(lens, st.d) <= D.default_cap(st.hdb.n)
    want = st.expected(ncb)
    # links between two long, a short and a long, and two short sequences
    off, nb, _ = want
    kinds = [0, 0, 0]
    for q in range(st.hdb.n):
        for t in nb[int(off[q]):int(off[q + 1])]:
            kinds[int(lens[q] < T) + int(lens[t] < T)] += 1
    assert min(kinds) > 0, kinds
    _same(_graph(gpu_ctx, st, ncb), want)
    assert gpu_ctx.dn_graph_totals()["qgram_comparisons"] >= D.brute_candidates(lens, st.d)


# ---- 4. a scoring without the wavefront form -----------------------------------------------------------------------------------
def test_d9_with_the_banded_16_bit_scoring(gpu_ctx, sets):
    st = sets("d9")
    got = _graph(gpu_ctx, st, False, NO_WFA)
    assert gpu_ctx.search_form(False)[0] == "banded32"
    _same(got, st.expected(False, NO_WFA))


# ---- 5. low complexity: one window at many shifts of one target ----------------------------------------------------------------
@pytest.mark.parametrize("ncb", [False, True], ids=["rule", "n"])
def test_low_complexity_at_d12(gpu_ctx, sets, ncb):
    st = sets("lowc")
    assert 80 <= st.hdb.n <= 120
    want = st.expected(ncb)
    assert len(want[1]) > st.hdb.n
    _same(_graph(gpu_ctx, st, ncb), want)


# ---- 6. where the route ends -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d9", "d12", "d16"])
def test_supported_from_9_to_16(gpu_ctx, sets, name):
    st = sets(name)
    gpu_ctx.upload_hostdb(st.hdb)
    gpu_ctx.qgram_build()
    gpu_ctx.search_begin(*DEFAULT, st.d)
    assert gpu_ctx.dn_graph_supported()


def test_not_supported_at_17(gpu_ctx, sets):
    st = sets("d16")
    gpu_ctx.upload_hostdb(st.hdb)
    gpu_ctx.qgram_build()
    gpu_ctx.search_begin(*DEFAULT, 17)
    assert not gpu_ctx.dn_graph_supported()
    rc, _, _, _, _ = gpu_ctx.dn_graph_raw(0)
    assert rc == SWA_E_ARG


def test_not_supported_past_the_brute_force_cap(gpu_ctx, sets, monkeypatch):
    st = sets("mixed")
    gpu_ctx.upload_hostdb(st.hdb)
    gpu_ctx.qgram_build()
    gpu_ctx.search_begin(*DEFAULT, st.d)
    assert gpu_ctx.dn_graph_supported()
    monkeypatch.setenv("SWA_DN_BRUTE_CAP", "1")
    assert not gpu_ctx.dn_graph_supported()
    rc, _, _, _, _ = gpu_ctx.dn_graph_raw(0)
    assert rc == SWA_E_ARG


# ---- 7. the capacity protocol ----------------------------------------------------------------------------------------------------
def test_capacity_protocol_at_d12(gpu_ctx, sets):
    st = sets("d12")
    want = st.expected(False)
    gpu_ctx.upload_hostdb(st.hdb)
    gpu_ctx.qgram_build()
    gpu_ctx.search_begin(*DEFAULT, st.d)
    rc, off0, _, _, total = gpu_ctx.dn_graph_raw(0)
    assert rc == SWA_E_CAPACITY and total == len(want[1]) > 0
    assert np.array_equal(off0, want[0])
    work = gpu_ctx.dn_graph_totals()
    rc, off1, nb, df, total1 = gpu_ctx.dn_graph_raw(total)
    assert rc == SWA_OK and total1 == total
    _same((off1, nb, df), want)
    assert gpu_ctx.dn_graph_totals() == work                # (the second call fetched: nothing was searched again)


# ---- 8. the graph left in HBM, walked there ------------------------------------------------------------------------------------
def _host_walk(n, graph):
    """the agglomeration of cluster_over_graph (host/cluster_dn.cpp) on a CSR: (swarm id, generation, parent, parent diff)"""
    off, nb, df = graph
    swarm = np.full(n, -1, dtype=np.int64)
    gen = np.zeros(n, dtype=np.int64)
    parent = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    pdiff = np.zeros(n, dtype=np.uint8)
    ns = 0
    for seed in range(n):
        if swarm[seed] >= 0:
            continue
        swarm[seed] = ns
        queue = [seed]
        at = 0
        while at < len(queue):
            # a generation at a time: its members in id order, each taking its unswarmed neighbours in id order
            end = len(queue)
            new = []
            for v in queue[at:end]:
                for e in range(int(off[v]), int(off[v + 1])):
                    t = int(nb[e])
                    if swarm[t] < 0:
                        swarm[t] = ns
                        gen[t] = gen[v] + 1
                        parent[t] = v
                        pdiff[t] = df[e]
                        new.append(t)
            queue += sorted(new)
            at = end
        ns += 1
    return swarm, gen, parent, pdiff


@pytest.mark.parametrize("name", ["chains", "mixed"])
def test_resident_graph_walk_and_parent_diffs_at_d12(gpu_ctx, sets, name):
    st = sets(name)
    n = st.hdb.n
    graph = _graph(gpu_ctx, st, False)
    total = gpu_ctx.dn_graph_resident(False)
    assert total == len(graph[1])
    swarmid, generation, parent, order, begins = gpu_ctx.d1_cluster_device()
    pdiff = gpu_ctx.dn_parent_diffs()
    wswarm, wgen, wparent, wpdiff = _host_walk(n, graph)
    assert len(begins) - 1 == wswarm.max() + 1 < n
    assert wgen.max() >= 2
    assert np.array_equal(parent, wparent)
    assert np.array_equal(pdiff, wpdiff)
    assert np.array_equal(generation.astype(np.int64) - int(generation.min()), wgen)      # (seeds: the lowest generation)
    # the same partition (swarms numbered by their first member on both sides)
    def canon(labels):
        _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
        return first[inverse]
    assert np.array_equal(canon(swarmid), canon(wswarm))


# ---- 9. the command line: graph and scan write the same files -------------------------------------------------------------------
@pytest.mark.parametrize("extra", [[], ["-n"]], ids=["rule", "n"])
def test_cli_d12_graph_equals_scan(tmp_path, extra):
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 600, 300, 1209, 12)
    env = {k: v for k, v in os.environ.items() if k not in ("SWARM_AMD_DN", "SWARM_AMD_DN_WALK", "SWA_DN_BRUTE_CAP")}
    out = {}
    for route in ("graph", "scan"):
        cmd = ["timeout", "-k", "10", "120", str(BIN), "-d", "12"] + extra
        for k in "oiswu":
            cmd += [f"-{k}", str(tmp_path / f"{route}.{k}")]
        r = subprocess.run(cmd + ["-l", "/dev/null", str(fa)], capture_output=True, text=True, env=dict(env, SWARM_AMD_DN=route))
        assert r.returncode == 0, (route, r.returncode, r.stderr)
        out[route] = {k: (tmp_path / f"{route}.{k}").read_bytes() for k in "oiswu"}
    assert out["graph"]["i"].count(b"\n") > 100
    for k in "oiswu":
        assert out["graph"][k] == out["scan"][k], k


def test_library_d12_graph_equals_scan_and_the_default_is_the_scan(gpu_ctx, sets, tmp_path, monkeypatch):
    """DnClusters: SWARM_AMD_DN=graph is served at d = 12 (it was refused), writes what the scan writes, and without the
    switch d > 8 still takes the scan (profiles/r10/NOTES.md)."""
    st = sets("d12")
    out = {}
    for route in ("graph", "scan", None):
        if route is None:
            monkeypatch.delenv("SWARM_AMD_DN")
        else:
            monkeypatch.setenv("SWARM_AMD_DN", route)
        gpu_ctx.upload_hostdb(st.hdb)
        cl = DnClusters(gpu_ctx, st.hdb, st.d)
        try:
            assert cl.scan_totals()["route"] == (route or "scan")
            for k, w in (("o", cl.write_swarms), ("i", cl.write_structure), ("s", cl.write_stats)):
                w(tmp_path / f"{route}.{k}")
            cl.write_uclust(tmp_path / f"{route}.u", ctx=gpu_ctx)
        finally:
            cl.close()
        out[route] = {k: (tmp_path / f"{route}.{k}").read_bytes() for k in "oisu"}
    for k in "oisu":
        assert out["graph"][k] == out["scan"][k] == out[None][k], k


# ---- 10. several ranks on one device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncb", [False, True], ids=["rule", "n"])
def test_three_ranks_on_one_device_at_d12(sets, ncb):
    st = sets("d12")
    m = MultiContext([0, 0, 0])
    try:
        m.upload_hostdb(st.hdb)
        got = m.dn_graph(st.d, ncb)
    finally:
        m.close()
    assert got is not None
    _same(got, st.expected(ncb))
