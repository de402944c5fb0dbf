"""CPU checks behind tests/test_cluster_forms_gpu.py (no GPU):

1. the closed forms of tests/cluster_sets.py equal the reference's loop restated (_greedy_walk of test_walk_identity.py);
2. the sweep protocol of swarm_amd/csrc/cluster_gpu.hip as a model.  test_walk_identity.py proves "greedy walk = function of
   the graph" against a plain fixed point; the kernels reach that fixed point through stamps (only what changed in the sweep
   before hands its label on), pointer jumping, sweeps launched ahead in batches that return at once behind a sweep that
   changed nothing, and a restart of the sweep numbering when the flags run out.  Here k_label_sweep and k_level_sweep are
   restated memory access by memory access — every read, atomicMin and store of a lane is one micro-step —, a sweep runs its
   lanes under a random interleaving of those micro-steps (so a lane hands on a label it read before somebody lowered it,
   and reads gen[v] while another claimant writes it), and the host loops of swa_d1_cluster_device drive them, with small
   constants (a batch of 3, 8 flags) so that the restart is taken.  At the stop the labels must be "the smallest id that
   reaches v" and generations / parents the breadth-first ones: the stop never comes early."""
import numpy as np
import pytest

import cluster_sets as CS
from test_walk_identity import _graph

UNSET = CS.NO_AMPLICON


def _assert_expected(got, want):
    for name in ("swarmid", "generation", "parent", "order", "begins"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert got.maxgen == want.maxgen


def _check_builder(csr, want):
    offsets, neighbours, diffs = csr
    assert offsets[0] == 0 and offsets[-1] == len(neighbours) == len(diffs)
    rows = CS.rows_from_csr(offsets, neighbours, diffs)
    for u, r in enumerate(rows):                              # what swa_d1_network_adopt asks of a graph
        vs = [v for v, _ in r]
        assert vs == sorted(set(vs)) and u not in vs and all(0 <= v < len(rows) for v in vs)
    walked, _ = CS.expected_from_walk(rows)
    _assert_expected(want, walked)


@pytest.mark.parametrize("depth", [0, 1, 2, 31, 32, 33, 200])
@pytest.mark.parametrize("last_is_chain", [False, True])
def test_rising_chain_closed_form_is_the_walk(depth, last_is_chain):
    csr, want = CS.rising_chain(depth, 250 + 2 * depth, 3, last_is_chain)
    assert want.maxgen == depth and len(want.begins) - 1 == 250 + 2 * depth + 1
    n = len(csr[0]) - 1
    assert (want.parent[n - 1] != UNSET) == (last_is_chain and depth > 0)      # both values of "the last vertex is a seed"
    _check_builder(csr, want)


@pytest.mark.parametrize("m", [1, 2, 8, 13, 200])
def test_falling_chain_closed_form_is_the_walk(m):
    csr, want = CS.falling_chain(m)
    assert want.maxgen == m and len(want.begins) == 2
    assert list(want.order) == [0] + list(range(m, 0, -1))
    _check_builder(csr, want)


@pytest.mark.parametrize("width,depth,seed", [(40, 12, 1), (5, 60, 2), (1, 7, 3), (300, 3, 4)])
def test_layers_closed_form_is_the_walk(width, depth, seed):
    csr, want = CS.layers(width, depth, np.random.default_rng(seed))
    assert want.maxgen == depth and len(want.begins) == 3
    rows = CS.rows_from_csr(*csr)
    label = want.order[want.begins[:-1]][want.swarmid]
    assert any(label[v] != label[u] for u in range(len(rows)) for v, _ in rows[u])   # links into the other swarm exist
    assert any(want.generation[v] <= want.generation[u] and label[v] == label[u] for u in range(len(rows)) for v, _ in rows[u])
    _check_builder(csr, want)


def test_random_graph_variants():
    rng = np.random.default_rng(3)
    backward = 0
    for arbitrary in (False, True):
        for n in (1, 2, 65, 200):
            csr, want, radius = CS.random_graph(rng, n, 1.5, 0.3, arbitrary)
            rows = CS.rows_from_csr(*csr)
            assert len(rows) == n
            backward += sum(v < u for u in range(n) for v, _ in rows[u]) if arbitrary else 0
            for v in range(n):                                # radius(v) = radius(parent) + diff(parent, v)
                p = int(want.parent[v])
                assert radius[v] == (0 if p == UNSET else radius[p] + dict(rows[p])[v])
    assert backward > 50


# ---- the sweep protocol as a model ---------------------------------------------------------------------------------------

def _interleave(rng, lanes):
    """run generators to their ends, one micro-step of a random live lane at a time"""
    live = list(lanes)
    for lane in live:
        next(lane, None)                                      # (to the first yield: nothing is touched before it)
    while live:
        k = int(rng.integers(0, len(live)))
        try:
            next(live[k])
        except StopIteration:
            live[k] = live[-1]
            live.pop()


def _label_lane(rows, u, label, stamp, s, flags, active_rule):
    """one lane of k_label_sweep; a yield stands between any two accesses to memory"""
    yield
    any_ = False
    lu = label[u]
    yield
    active = active_rule(stamp[u], s)
    yield
    ll = label[lu]
    yield
    if ll < lu:
        label[u] = min(label[u], ll)                          # atomicMin
        lu = ll
        yield
        stamp[u] = s
        yield
        any_ = True
        active = True
    if active:
        for v, _ in rows[u]:
            lv = label[v]
            yield
            if lu < lv:
                label[v] = min(label[v], lu)                  # atomicMin
                yield
                stamp[v] = s
                yield
                any_ = True
    if any_:
        flags[s] = 1


def _label_sweep(rng, rows, label, stamp, s, flags, active_rule):
    if s > 1 and flags[s - 1] == 0:                           # behind the fixed point: returns at once
        return
    _interleave(rng, [_label_lane(rows, u, label, stamp, s, flags, active_rule) for u in range(len(rows))])


def _labels_by_protocol(rng, rows, batch=3, nflags=8, active_rule=lambda st, s: st + 1 >= s, clear_stamps=True):
    """the host loop of swa_d1_cluster_device (kSweepBatch = batch, kSweepFlags = nflags) -> labels, sweeps launched, restarts"""
    n = len(rows)
    label, stamp, flags = list(range(n)), [0] * n, [0] * nflags
    launched = restarts = 0
    s = 1
    while True:
        if s == 1:
            flags = [0] * nflags
        last = min(s + batch, nflags) - 1
        while s <= last:
            _label_sweep(rng, rows, label, stamp, s, flags, active_rule)
            launched += 1
            s += 1
        if flags[last] == 0:
            break
        if s == nflags:
            if clear_stamps:
                stamp = [0] * n
            s = 1
            restarts += 1
    return label, launched, restarts


def _smallest_id_that_reaches(rows):
    n = len(rows)
    label = list(range(n))
    for seed in range(n):                                     # ascending: the first seed to reach v is the smallest
        if label[seed] != seed:
            continue
        stack = [seed]
        seen = {seed}
        while stack:
            u = stack.pop()
            for v, _ in rows[u]:
                if v not in seen and label[v] > seed:
                    seen.add(v)
                    label[v] = seed
                    stack.append(v)
    return label


def _model_graphs(rng):
    for m in (1, 2, 5, 9, 17, 40):
        yield CS.rows_from_csr(*CS.falling_chain(m)[0])
    for t in range(40):
        n = int(rng.integers(1, 60))
        if t % 2:
            yield CS.rows_from_csr(*CS.random_graph(rng, n, float(rng.choice([0.3, 1.5, 3.0])), 0.0, arbitrary=True)[0])
        else:
            yield _graph(rng, n, float(rng.choice([0.3, 0.8, 1.5, 3.0])), float(rng.choice([0.0, 0.3, 0.7, 1.0])))
    yield CS.rows_from_csr(*CS.layers(6, 9, rng)[0])


def test_label_sweep_protocol_stops_at_the_fixed_point_and_never_before():
    rng = np.random.default_rng(41)
    most_restarts = 0
    for rows in _model_graphs(rng):
        want = _smallest_id_that_reaches(rows)
        for _ in range(3):
            label, launched, restarts = _labels_by_protocol(rng, rows)
            assert label == want, rows
            most_restarts = max(most_restarts, restarts)
    assert most_restarts >= 3                                 # the numbering was restarted, more than once in a run


def test_label_sweep_protocol_falling_chain_takes_a_sweep_a_hop():
    """why falling_chain defeats pointer jumping: in the model too the label 0 needs about a sweep a hop (a lucky interleaving
    carries it several hops in one sweep, never all the way)"""
    rng = np.random.default_rng(42)
    rows = CS.rows_from_csr(*CS.falling_chain(60)[0])
    label, launched, restarts = _labels_by_protocol(rng, rows)
    assert label == [0] * 61
    assert launched >= 15 and restarts >= 2


def test_label_sweep_protocol_without_clearing_the_stamps():
    """The restart clears `stamp`.  Sweep 1 of a numbering treats every vertex as active whatever its stamp says
    (stamp + 1 >= 1), and a stamp left over from the numbering before can only be too high: the vertex then hands its label on
    in sweeps where it need not.  So the clear spares work and the labels do not depend on it — stated here so that nobody
    looks for a failing test behind it."""
    rng = np.random.default_rng(43)
    for rows in _model_graphs(rng):
        label, _, _ = _labels_by_protocol(rng, rows, clear_stamps=False)
        assert label == _smallest_id_that_reaches(rows), rows


def test_label_sweep_model_tells_a_wrong_stamp_rule():
    """the model is no rubber stamp: with a stamp rule that forgets the sweep before (active = changed in THIS sweep), a change
    made to v after v's own lane went by is never handed on, and the loop stops early somewhere"""
    rng = np.random.default_rng(45)
    rows_list = list(_model_graphs(np.random.default_rng(44)))
    wrong = lambda st, s: s == 1 or st >= s
    assert any(_labels_by_protocol(rng, rows, active_rule=wrong)[0] != _smallest_id_that_reaches(rows) for rows in rows_list)


def _level_lane(rows, u, label, gen, parent, level, claimed):
    """one lane of k_level_sweep"""
    yield
    gu = gen[u]
    yield
    if gu != level - 1:
        return
    lu = label[u]
    yield
    for v, _ in rows[u]:
        lv = label[v]
        yield
        if lv != lu:
            continue
        gv = gen[v]
        yield
        if gv == UNSET or gv == level:
            if gv == UNSET:
                gen[v] = level
                yield
            parent[v] = min(parent[v], u)                     # atomicMin
            yield
            claimed[0] = True


def _levels_by_protocol(rng, rows, label, batch=3):
    """the second host loop (kLevelBatch = batch) -> gen, parent, maxgen, batches"""
    n = len(rows)
    gen = [0 if label[v] == v else UNSET for v in range(n)]   # k_level_init
    parent = [UNSET] * n
    maxgen = batches = 0
    level0 = 1
    while True:
        any_ = [0] * batch
        batches += 1
        for r in range(batch):
            if r > 0 and any_[r - 1] == 0:
                continue
            claimed = [False]
            _interleave(rng, [_level_lane(rows, u, label, gen, parent, level0 + r, claimed) for u in range(n)])
            if claimed[0]:
                any_[r] = 1
        for r in range(batch):
            if any_[r]:
                maxgen = level0 + r
        if any_[batch - 1] == 0:
            break
        level0 += batch
    return gen, parent, maxgen, batches


def test_level_sweep_protocol_gives_breadth_first_generations_and_smallest_parents():
    rng = np.random.default_rng(46)
    depths = set()
    for rows in list(_model_graphs(rng)) + [CS.rows_from_csr(*CS.rising_chain(d, 6 + 2 * d, 2, bool(d % 2))[0]) for d in range(0, 8)]:
        want, _ = CS.expected_from_walk(rows)
        label = _smallest_id_that_reaches(rows)
        gen, parent, maxgen, batches = _levels_by_protocol(rng, rows, label)
        assert gen == list(want.generation) and parent == list(want.parent), rows
        assert maxgen == want.maxgen and batches == want.maxgen // 3 + 1
        depths.add(want.maxgen % 3)
    assert depths == {0, 1, 2}                                # deepest generations on, before and behind a batch's last sweep
