"""The agglomeration kernels of swarm_amd/csrc/cluster_gpu.hip — k_label_sweep, k_level_sweep, k_swarm_keys<K>,
k_swarm_bounds<K> and the sort between them — handed synthetic graphs directly (swa_d1_network_adopt, which checks every graph
on the host before it reaches the device) instead of whatever graphs sequence sets happen to produce: both key widths with the
32-bit one filled to its last bit, the restart of the sweep numbering, the edges of the sweep and level batches, every value
where the number of generation bits changes, n = 1, odd and even n, both values of "the last vertex is a seed", a swarm table
one entry short, and one context reused for graphs of very different sizes.  The expected results are the closed forms of
tests/cluster_sets.py (checked against the reference's loop in tests/test_cluster_sets_identity.py) or that loop itself;
everything is integer equality."""
import os

import numpy as np
import pytest

import cluster_sets as CS
from swarm_amd import Context, D1Clusters, HostDb, SwaError, capi

pytestmark = pytest.mark.gpu


def _placeholders(ctx, n):
    """n placeholder amplicons as the resident database: one word each, falling abundances"""
    seqs = np.arange(n, dtype=np.uint64)
    seq_off = np.arange(n + 1, dtype=np.uint64)
    seqlen = np.full(n, 32, dtype=np.uint32)
    abundance = (n - np.arange(n)).astype(np.uint64)
    ctx.upload_db(seqs, seq_off, seqlen, abundance, 32)


def _cluster(ctx, csr, want, with_diffs=True, upload=True, **how):
    """one adopt, one clustering; all five arrays, the deepest generation and the number of swarms compared exactly"""
    offsets, neighbours, diffs = csr
    if upload:
        _placeholders(ctx, len(offsets) - 1)
    assert ctx.d1_network_adopt(offsets, neighbours, diffs if with_diffs else None) == len(neighbours)
    got = ctx.d1_cluster_device(**how)
    _same(ctx, got, want)
    return got


def _same(ctx, got, want):
    swarmid, generation, parent, order, begins = got
    assert len(begins) - 1 == len(want.begins) - 1
    assert ctx.d1_cluster_maxgen() == want.maxgen
    assert np.array_equal(begins, want.begins)
    assert np.array_equal(order, want.order)
    assert np.array_equal(swarmid, want.swarmid)
    assert np.array_equal(generation, want.generation)
    assert np.array_equal(parent, want.parent)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 3001])
def test_random_graphs(gpu_ctx, n):
    """against the reference's loop: every density and share of ties, links in arbitrary directions as well; with the links'
    differences swa_dn_parent_diffs gives diff(parent, v) and the radii of the walk follow, without them it refuses"""
    rng = np.random.default_rng(1000 + n)
    _placeholders(gpu_ctx, n)
    cases = [(density, ties, False) for density in (0, 0.3, 1.5, 3) for ties in (0, 0.3, 0.7, 1)]
    cases += [(density, 0, True) for density in (0.3, 1.5, 3, 6)]
    for k, (density, ties, arbitrary) in enumerate(cases):
        csr, want, radius = CS.random_graph(rng, n, density, ties, arbitrary)
        with_diffs = k % 4 != 3
        got = _cluster(gpu_ctx, csr, want, with_diffs=with_diffs, upload=False)
        if not with_diffs:
            with pytest.raises(SwaError) as e:
                gpu_ctx.dn_parent_diffs()
            assert e.value.code == capi.SWA_E_ARG
            continue
        pdiff = gpu_ctx.dn_parent_diffs()
        rows = CS.rows_from_csr(*csr)
        parent, order = got[2], got[3]
        assert [int(d) for d in pdiff] == [0 if p == CS.NO_AMPLICON else dict(rows[p])[v] for v, p in enumerate(int(p) for p in parent)]
        acc = np.zeros(n, dtype=np.uint32)
        for v in order:                                           # (a parent stands before its children in the order)
            if parent[v] != CS.NO_AMPLICON:
                acc[v] = acc[parent[v]] + pdiff[v]
        assert np.array_equal(acc, radius)


@pytest.mark.parametrize("last_is_chain", [False, True])
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65])
def test_generation_batches_and_bit_widths(gpu_ctx, depth, last_is_chain):
    """deepest generations on either side of every change of bit_width(maxgen) and of a level batch's last sweep (32
    generations a batch: its last flag decides whether another batch runs), the last vertex a seed or not"""
    csr, want = CS.rising_chain(depth, 300, 3, last_is_chain)
    assert want.maxgen == depth
    _cluster(gpu_ctx, csr, want)
    sweeps, restarts, batches = gpu_ctx.d1_cluster_effort()
    assert batches == depth // 32 + 1 and restarts == 0 and sweeps >= 1


@pytest.mark.parametrize("m", [8, 9, 10, 11, 12, 13])
def test_fixed_point_around_a_sweep_batch_end(gpu_ctx, m):
    """falling chains that need about m sweeps, around the 10 of a batch; how many sweeps the device took depends on how it
    scheduled the lanes and is only recorded"""
    csr, want = CS.falling_chain(m)
    _cluster(gpu_ctx, csr, want)
    print(f"falling_chain({m}): sweeps launched, restarts, level batches = {gpu_ctx.d1_cluster_effort()}")


def test_restart_of_the_sweep_numbering(gpu_ctx):
    """A falling chain of 4096: neighbours on the chain have adjacent ids and mostly sit in one wave, where every lane's load
    of label[u] precedes every lane's atomicMin — a label crosses a wave's 64 members in no fewer than 63 sweeps, some 4000
    sweeps in all against the 1023 flags of one numbering."""
    csr, want = CS.falling_chain(4096)
    _cluster(gpu_ctx, csr, want)
    sweeps, restarts, batches = gpu_ctx.d1_cluster_effort()
    print(f"falling_chain(4096): sweeps launched, restarts, level batches = {(sweeps, restarts, batches)}")
    assert restarts >= 1 and sweeps > 1023
    assert batches == 4096 // 32 + 1


def _key_width_graph(depth):
    return CS.rising_chain(depth, 524288, 100, False)


@pytest.mark.parametrize("depth", [4095, 4096])
def test_key_width(gpu_ctx, depth):
    """524 289 swarms (20 bits) and a chain 4095 deep (12 bits of generations: the 32-bit keys filled to the last bit) or
    4096 deep (13 bits: the 64-bit keys); 528 k vertices, so the kernels' grid-stride loops go round more than once.  Then
    the same with swarm / generation / parent left in HBM and fetched afterwards."""
    csr, want = _key_width_graph(depth)
    assert len(want.begins) - 1 == 524289 and want.maxgen == depth
    _cluster(gpu_ctx, csr, want)
    assert gpu_ctx.d1_cluster_effort()[2] == depth // 32 + 1
    _, _, _, order, begins = gpu_ctx.d1_cluster_device(details=False)
    _same(gpu_ctx, gpu_ctx.d1_cluster_fetch() + (order, begins), want)


@pytest.mark.parametrize("width,depth", [(300, 40), (5, 200)])
def test_layers(gpu_ctx, width, depth):
    """parents = the smallest of several claimants, links back into generations already claimed, links into another swarm"""
    csr, want = CS.layers(width, depth, np.random.default_rng(width))
    _cluster(gpu_ctx, csr, want)


def test_swarm_table_one_entry_short(gpu_ctx):
    csr, want, _ = CS.random_graph(np.random.default_rng(8), 500, 0.8, 0.3)
    need = len(want.begins) - 1
    assert need > 10
    _placeholders(gpu_ctx, 500)
    gpu_ctx.d1_network_adopt(*csr)
    with pytest.raises(SwaError) as e:
        gpu_ctx.d1_cluster_device(swarm_cap=need - 1)
    assert e.value.code == capi.SWA_E_CAPACITY and e.value.nswarms == need
    with pytest.raises(SwaError) as e:
        gpu_ctx.d1_cluster_fetch()
    assert e.value.code == capi.SWA_E_ARG and "no clustering in place" in str(e.value)
    _same(gpu_ctx, gpu_ctx.d1_cluster_device(swarm_cap=need), want)
    _same(gpu_ctx, gpu_ctx.d1_cluster_device(swarm_cap=need + 7), want)


def test_one_context_many_graphs(gpu_ctx):
    """a large graph, two small ones, the large one again: nothing of a run (stamps, flags, generations, keys of the wider
    form) may reach the next"""
    big, big_want = _key_width_graph(4096)
    small, small_want, _ = CS.random_graph(np.random.default_rng(9), 65, 1.5, 0.3)
    chain, chain_want = CS.falling_chain(50)
    for csr, want in ((big, big_want), (small, small_want), (chain, chain_want), (big, big_want)):
        _cluster(gpu_ctx, csr, want)


def test_writers_over_an_adopted_graph(gpu_ctx, tmp_path):
    """the three forms of the result the command line and the library build on the device's arrays — eager, lazy, pinned —
    against the serial host walk of the same graph: summary, arrays and the -o -s -i -w files byte for byte"""
    from test_d1_gpu import _same_clustering
    n = 3001
    rng = np.random.default_rng(10)
    seqs = set()
    while len(seqs) < n:
        seqs.add("".join(rng.choice(list("ACGT"), 40)))
    fa = tmp_path / "in.fa"
    with open(fa, "w") as fh:
        for k, q in enumerate(sorted(seqs)):
            fh.write(f">a{k}_{1 + (n - k) // 3}\n{q}\n")
    hdb = HostDb(fa)
    assert hdb.n == n
    (offsets, neighbours, diffs), want, _ = CS.random_graph(rng, n, 1.5, 0.3)
    os.environ["SWARM_AMD_CLUSTER"] = "serial"
    try:
        host = D1Clusters(hdb, offsets, neighbours)
    finally:
        del os.environ["SWARM_AMD_CLUSTER"]
    assert np.array_equal(host.swarmid(), want.swarmid) and host.summary()["maxgen"] == want.maxgen
    gpu_ctx.upload_hostdb(hdb)
    gpu_ctx.d1_network_adopt(offsets, neighbours)
    for form in ({}, {"lazy": True}, {"pinned": True}):
        dev = D1Clusters.from_resident(gpu_ctx, hdb, **form)
        _same_clustering(dev, host, tmp_path, "_" + ("_".join(form) or "eager"))
        dev.close()
    host.close()


_GOOD = ([0, 2, 4, 5, 5, 7], [1, 3, 2, 4, 3, 0, 2])           # 5 vertices, 7 links


def _malformed():
    off, nb = (np.array(a) for a in _GOOD)
    a = nb.copy(); a[3] = 5
    yield "a neighbour = n", off, a
    a = nb.copy(); a[0], a[1] = 3, 1
    yield "a descending row", off, a
    a = nb.copy(); a[1] = 1
    yield "a duplicate in a row", off, a
    a = nb.copy(); a[2] = 1
    yield "a self link", off, a
    o = off.copy(); o[5] = 6
    yield "offsets[n] != total", o, nb
    o = off.copy(); o[2] = 1
    yield "a decreasing offset", o, nb
    o = off.copy(); o[0] = 1
    yield "offsets[0] != 0", o, nb
    o = off.copy(); o[3] = 9
    yield "an offset beyond the links", o, nb


def test_malformed_graphs_are_refused_on_the_host(gpu_ctx):
    """every one is refused before anything is copied or launched, and no resident network is left: these calls launch nothing"""
    _placeholders(gpu_ctx, 5)
    seen = 0
    for what, off, nb in _malformed():
        gpu_ctx.d1_network_adopt(*_GOOD)                         # (a network is in place: the refusal has to take it away)
        for diffs in (None, np.ones(len(nb), dtype=np.uint8)):
            with pytest.raises(SwaError) as e:
                gpu_ctx.d1_network_adopt(off, nb, diffs)
            assert e.value.code == capi.SWA_E_ARG, what
            with pytest.raises(SwaError) as e:
                gpu_ctx.d1_cluster_device()
            assert e.value.code == capi.SWA_E_ARG and "no resident network" in str(e.value), what
        seen += 1
    assert seen == 8
    gpu_ctx.d1_network_adopt(*_GOOD)
    assert len(gpu_ctx.d1_cluster_device()[4]) - 1 == 1          # (0 reaches everybody)
    empty = Context(0)                                           # no database
    try:
        with pytest.raises(SwaError) as e:
            empty.d1_network_adopt([0], [])
        assert e.value.code == capi.SWA_E_ARG
        with pytest.raises(SwaError) as e:
            empty.d1_cluster_device()
        assert e.value.code == capi.SWA_E_ARG and "no resident network" in str(e.value)
    finally:
        empty.close()
