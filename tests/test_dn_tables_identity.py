"""The identities swarm_amd/csrc/dn_tables.inc rests on, checked on the CPU against the reference's greedy loop restated
(tests/dn_tables_sets.py: walk_tables): the links in acceptance order as one stable sort of the non-seed positions of the
member order by their parent's position, every swarm's range of them, the radii by ping-pong pointer jumping in exactly
ceil(log2(deepest generation + 1)) rounds, and the swarms' deepest radius by the wave-wise segmented maximum.  No GPU."""
import numpy as np
import pytest

import cluster_sets as CS
import dn_tables_sets as DT


def _graphs():
    rng = np.random.default_rng(22)
    for n in (1, 2, 63, 64, 65, 257, 700):
        for density, ties, arbitrary in ((0, 0, False), (0.3, 0.3, False), (1.5, 0.7, False), (3, 1, False), (1.5, 0, True), (6, 0, True)):
            csr, _, _ = CS.random_graph(rng, n, density, ties, arbitrary)
            yield f"random n={n} density={density} ties={ties} arbitrary={arbitrary}", csr
    for depth in (0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65):
        for last_is_chain in (False, True):
            yield f"rising_chain depth={depth} last_is_chain={last_is_chain}", CS.rising_chain(depth, 300, 3, last_is_chain)[0]
    for m in (1, 2, 9, 64, 130):
        yield f"falling_chain m={m}", CS.falling_chain(m)[0]
    for width, depth in ((30, 12), (5, 70), (200, 3)):
        yield f"layers width={width} depth={depth}", CS.layers(width, depth, np.random.default_rng(width))[0]
    yield "wide swarm", DT.wide_swarm(1500, 300, 60, 300)
    yield "heavy chain", DT.heavy_chain(65, 5)


GRAPHS = list(_graphs())


@pytest.fixture(scope="module")
def tables():
    """the greedy loop over every graph, once"""
    return {name: (csr, DT.tables_of(csr)) for name, csr in GRAPHS}


def test_links_are_one_stable_sort_of_the_non_seed_positions(tables):
    multi_generation = 0
    for name, (csr, t) in tables.items():
        e = t.expected
        rows = CS.rows_from_csr(*csr)
        pdiff = DT.parent_diffs(rows, e.parent)
        assert 0xFF not in pdiff[e.generation != 0], name
        at = DT.links_by_stable_sort(e.order, e.begins, e.parent)
        child = e.order[at]
        assert np.array_equal(child, t.link_child), name
        assert np.array_equal(e.parent[child], t.link_parent), name
        assert np.array_equal(e.generation[child], t.link_generation), name
        assert np.array_equal(pdiff[child], t.link_diff), name
        assert len(at) == len(e.order) - (len(e.begins) - 1), name
        multi_generation += int((t.maxgen > 1).sum())
    assert multi_generation > 100


def test_every_swarm_owns_its_range_of_links(tables):
    for name, (_, t) in tables.items():
        begins = t.expected.begins.astype(np.int64)
        s = np.arange(len(begins) - 1)
        assert np.array_equal(t.link_begin, begins[:-1] - s), name
        assert np.array_equal(t.link_end, begins[1:] - s - 1), name
        for k in s:
            assert (t.link_swarm[t.link_begin[k]:t.link_end[k]] == k + 1).all(), name
            assert (t.expected.swarmid[t.link_child[t.link_begin[k]:t.link_end[k]]] == k).all(), name


def test_pointer_jumping_takes_bit_width_of_the_deepest_generation_rounds(tables):
    seen = set()
    for name, (csr, t) in tables.items():
        e = t.expected
        pdiff = DT.parent_diffs(CS.rows_from_csr(*csr), e.parent)
        radius, rounds = DT.jump_model(e.parent, pdiff)
        assert rounds == DT.jump_rounds(e.maxgen), name
        assert np.array_equal(radius, t.radius), name
        sequential = np.zeros(len(e.order), dtype=np.uint32)     # (a parent stands before its children in the order)
        for v in e.order:
            if e.parent[v] != CS.NO_AMPLICON:
                sequential[v] = sequential[e.parent[v]] + pdiff[v]
        assert np.array_equal(radius, sequential), name
        seen.add(rounds)
    assert seen >= set(range(8))                                  # 0 rounds (no links) up to 7 (depth 64, 65)
    assert [DT.jump_rounds(g) for g in (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65)] == [0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]


def test_a_radius_past_sixteen_bits():
    t = DT.tables_of(DT.heavy_chain(65, 5))
    assert int(t.radius.max()) == 65 * 254 == 16510 and int(t.maxradius.max()) == 16510
    t = DT.tables_of(DT.heavy_chain(259, 4))                       # (16 bits hold that one; a chain of 259 no longer)
    assert int(t.maxradius.max()) == 65786 > 0xFFFF


def test_segmented_maximum_by_waves(tables):
    plain = atomic = 0
    for name, (_, t) in tables.items():
        e = t.expected
        got, p, a = DT.segmented_max(e.order, e.swarmid, t.radius, e.begins)
        want = np.zeros(len(e.begins) - 1, dtype=np.uint32)
        for k, v in enumerate(e.order):                           # the plain loop
            want[e.swarmid[v]] = max(int(want[e.swarmid[v]]), int(t.radius[v]))
        assert np.array_equal(got, want), name
        assert np.array_equal(got, t.maxradius), name
        plain += p
        atomic += a
    assert plain > 1000 and atomic > 100


def test_the_wide_swarm_has_the_runs_it_is_made_for():
    csr = DT.wide_swarm()
    t = DT.tables_of(csr)
    e = t.expected
    assert len(e.order) == 3001 and e.begins[1] == 2601            # the wide swarm: 41 waves, 11 workgroups of 256
    assert int((e.generation == 1).sum()) >= 700
    sizes = np.diff(e.begins.astype(np.int64))
    assert (sizes[1:] <= 2).all() and (sizes == 1).sum() > 50 and (sizes == 2).sum() > 50
    straddling = [s for s in range(1, len(sizes)) if sizes[s] == 2 and e.begins[s] % 64 == 63]
    assert straddling, "a swarm whose run starts in a wave's last lane and ends in the next wave's first"
