"""swa_dn_tables_device / swa_dn_tables_fetch (swarm_amd/csrc/dn_tables.inc) handed synthetic graphs directly
(swa_d1_network_adopt with a byte of differences per link; no alignment runs): the radius of every amplicon, the four sums of
every swarm and the four link arrays against the reference's greedy loop restated on the CPU (tests/dn_tables_sets.py, whose
identities tests/test_dn_tables_identity.py checks).  Everything is integer equality.  Sizes: n around the wave and the
workgroup, depths on either side of every change in the number of jumping rounds, a swarm whose run spans waves and
workgroups beside swarms of one and two, radii past 8 and past 16 bits, the refusals, one context reused."""
import numpy as np
import pytest

import cluster_sets as CS
import dn_tables_sets as DT
from swarm_amd import SwaError, capi

pytestmark = pytest.mark.gpu

BROKEN = "a parent without a link to its child"


def _placeholders(ctx, n):
    """n placeholder amplicons as the resident database: one word each, abundances 1, 2, 3, 1, ... (singletons among them)"""
    seqs = np.arange(n, dtype=np.uint64)
    seq_off = np.arange(n + 1, dtype=np.uint64)
    seqlen = np.full(n, 32, dtype=np.uint32)
    ctx.upload_db(seqs, seq_off, seqlen, DT.abundances(n), 32)


def _make(ctx, csr, upload=True, details=False):
    """adopt, cluster, make the tables; returns the clustering's arrays and (nswarms, nlinks)"""
    offsets, neighbours, diffs = csr
    if upload:
        _placeholders(ctx, len(offsets) - 1)
    assert ctx.d1_network_adopt(offsets, neighbours, diffs) == len(neighbours)
    got = ctx.d1_cluster_device(details=details)
    return got, ctx.dn_tables_device()


def _check(ctx, csr, want=None, upload=True, details=False):
    """every array of the fetch, and the sizes, against the greedy loop"""
    want = DT.tables_of(csr) if want is None else want
    e = want.expected
    n = len(e.order)
    got, (nswarms, nlinks) = _make(ctx, csr, upload, details)
    assert nswarms == len(e.begins) - 1 and nlinks == n - nswarms == len(want.link_child)
    assert np.array_equal(got[3], e.order) and np.array_equal(got[4], e.begins)
    assert ctx.d1_cluster_maxgen() == e.maxgen
    t = ctx.dn_tables_fetch()
    assert list(t) == ["radius", "mass", "singletons", "maxgen", "maxradius", "link_parent", "link_child", "link_generation", "link_diff"]
    for name in t:
        assert t[name].dtype == getattr(want, name).dtype and np.array_equal(t[name], getattr(want, name)), name
    # (swarm s owns the links [begins[s] - s, begins[s + 1] - s - 1): every child of the range is a member of s)
    s_of_link = np.repeat(np.arange(nswarms), np.diff(e.begins.astype(np.int64)) - 1)
    assert np.array_equal(e.swarmid[t["link_child"]], s_of_link)
    return want


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 3001])
def test_random_graphs(gpu_ctx, n):
    """every density and share of ties of test_cluster_forms_gpu.py, links in arbitrary directions as well; density 0: no
    links at all"""
    rng = np.random.default_rng(2200 + n)
    _placeholders(gpu_ctx, n)
    cases = [(density, ties, False) for density in (0, 0.3, 1.5, 3) for ties in (0, 0.3, 0.7, 1)]
    cases += [(density, 0, True) for density in (0.3, 1.5, 3, 6)]
    for k, (density, ties, arbitrary) in enumerate(cases):
        csr, expected, radius = CS.random_graph(rng, n, density, ties, arbitrary)
        want = _check(gpu_ctx, csr, upload=False, details=k % 2 == 0)
        assert np.array_equal(want.radius, radius) and np.array_equal(want.expected.order, expected.order)
        if density == 0:
            assert len(want.link_child) == 0 and len(want.mass) == n and not want.maxgen.any()


@pytest.mark.parametrize("last_is_chain", [False, True])
@pytest.mark.parametrize("depth", [0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65])
def test_jumping_rounds(gpu_ctx, depth, last_is_chain):
    """deepest generations on either side of every change of bit_width(maxgen), the number of rounds launched (and of which
    of the two buffers holds the radii at the end), the last vertex on the chain or a swarm of its own"""
    csr, expected = CS.rising_chain(depth, 300, 3, last_is_chain)
    want = _check(gpu_ctx, csr)
    assert want.expected.maxgen == depth == expected.maxgen
    assert int(want.maxgen.max()) == depth and int(want.radius.max()) == int(want.maxradius.max()) >= depth


def test_falling_chain_and_layers(gpu_ctx):
    """ids falling along the chain (the children's positions ascend although their ids do not follow their parents'), and
    parents that are the smallest of several claimants with links back and into another swarm"""
    _check(gpu_ctx, CS.falling_chain(130)[0])
    _check(gpu_ctx, CS.layers(40, 9, np.random.default_rng(40))[0])


def test_one_wide_swarm_beside_small_ones(gpu_ctx):
    """a swarm of 2601 members (a star of 700, then layers) whose run in the member order spans 41 waves and 11 workgroups:
    one atomicMax per (wave, swarm); behind it swarms of one and two members (plain stores), one of them with its run from a
    wave's last lane into the next wave's first"""
    csr = DT.wide_swarm()
    want = _check(gpu_ctx, csr)
    e = want.expected
    sizes = np.diff(e.begins.astype(np.int64))
    assert sizes[0] == 2601 and set(sizes[1:]) == {1, 2}
    assert any(sizes[s] == 2 and e.begins[s] % 64 == 63 for s in range(1, len(sizes)))
    assert want.maxradius[0] == want.radius[:2601].max() > 0 and want.maxgen[0] > 2


@pytest.mark.parametrize("singles", [5, 6])
def test_radius_past_eight_and_sixteen_bits(gpu_ctx, singles):
    """a chain 65 deep with every difference 254: radius 16 510 (odd and even n); 259 deep: 65 786"""
    want = _check(gpu_ctx, DT.heavy_chain(65, singles))
    assert len(want.radius) == 66 + singles and int(want.radius.max()) == 16510
    want = _check(gpu_ctx, DT.heavy_chain(259, singles))
    assert int(want.maxradius.max()) == 65786


def test_refusals(gpu_ctx):
    csr, _, _ = CS.random_graph(np.random.default_rng(5), 500, 1.5, 0.3)
    offsets, neighbours, diffs = csr
    _placeholders(gpu_ctx, 500)
    # no clustering in place
    gpu_ctx.d1_network_adopt(offsets, neighbours, diffs)
    for call in (gpu_ctx.dn_tables_device, gpu_ctx.dn_tables_fetch):
        with pytest.raises(SwaError) as e:
            call()
        assert e.value.code == capi.SWA_E_ARG and "no clustering in place" in str(e.value)
    # the fetch before the tables are made
    gpu_ctx.d1_cluster_device()
    with pytest.raises(SwaError) as e:
        gpu_ctx.dn_tables_fetch()
    assert e.value.code == capi.SWA_E_ARG and "no tables in place" in str(e.value)
    nswarms, nlinks = gpu_ctx.dn_tables_device()
    assert nswarms + nlinks == 500 and len(gpu_ctx.dn_tables_fetch()["link_child"]) == nlinks
    # a new clustering of the same graph ends them
    gpu_ctx.d1_cluster_device()
    with pytest.raises(SwaError) as e:
        gpu_ctx.dn_tables_fetch()
    assert e.value.code == capi.SWA_E_ARG and "no tables in place" in str(e.value)
    gpu_ctx.dn_tables_device()
    # ... and so does a new adopt
    gpu_ctx.d1_network_adopt(offsets, neighbours, diffs)
    with pytest.raises(SwaError) as e:
        gpu_ctx.dn_tables_fetch()
    assert e.value.code == capi.SWA_E_ARG
    gpu_ctx.d1_cluster_device()
    with pytest.raises(SwaError) as e:
        gpu_ctx.dn_tables_fetch()
    assert e.value.code == capi.SWA_E_ARG and "no tables in place" in str(e.value)
    # a graph adopted without differences
    gpu_ctx.d1_network_adopt(offsets, neighbours, None)
    gpu_ctx.d1_cluster_device()
    for call in (gpu_ctx.dn_tables_device, gpu_ctx.dn_tables_fetch):
        with pytest.raises(SwaError) as e:
            call()
        assert e.value.code == capi.SWA_E_ARG and "carries no differences" in str(e.value)
    # a new upload ends everything
    _make(gpu_ctx, csr, upload=False)
    _placeholders(gpu_ctx, 500)
    with pytest.raises(SwaError) as e:
        gpu_ctx.dn_tables_fetch()
    assert e.value.code == capi.SWA_E_ARG


def test_a_link_of_255_differences_into_a_child(gpu_ctx):
    """swa_d1_network_adopt takes any byte; 255 is what says "no link" where the parent's row is searched, so a member whose
    parent's link carries it is reported — and no tables are left.  The same link into a vertex that another parent claims
    (a smaller id of the same generation) disturbs nothing."""
    rows = [[(1, 2), (2, 255)], [(3, 1)], [(3, 255)], [], []]        # 0 -> 1, 0 -(255)-> 2, 1 -> 3, 2 -(255)-> 3
    csr = CS.csr_from_rows(rows)
    _placeholders(gpu_ctx, 5)
    gpu_ctx.d1_network_adopt(*csr)
    gpu_ctx.d1_cluster_device()
    with pytest.raises(SwaError) as e:
        gpu_ctx.dn_tables_device()
    assert e.value.code == capi.SWA_E_DEVICE and BROKEN in str(e.value)
    with pytest.raises(SwaError) as e:
        gpu_ctx.dn_tables_fetch()
    assert e.value.code == capi.SWA_E_ARG and "no tables in place" in str(e.value)
    rows[0][1] = (2, 3)                                                # (2 is 0's child by 3 differences; 3 stays 1's child)
    want = _check(gpu_ctx, CS.csr_from_rows(rows), upload=False)
    assert list(want.link_parent) == [0, 0, 1] and list(want.link_diff) == [2, 3, 1]


def test_one_context_many_graphs(gpu_ctx):
    """3001 amplicons, then 2, then 1000: nothing of a run (control word, buffers of the larger run, which buffer held the
    radii) may reach the next"""
    rng = np.random.default_rng(12)
    _check(gpu_ctx, DT.wide_swarm())
    _check(gpu_ctx, CS.csr_from_rows([[(1, 3)], []]))
    _check(gpu_ctx, CS.random_graph(rng, 1000, 1.5, 0.3)[0])
    _check(gpu_ctx, CS.csr_from_rows([[], []]))
