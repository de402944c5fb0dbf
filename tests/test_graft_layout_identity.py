"""The grafted clustering as one layout, on the CPU: the closed form the device is held to (tests/graft_layout_sets.py:
closed_form_layout — two integer scans and a scatter) against a walk over the chains, and against what the host's walk
(D1Clusters.graft) makes the -o writer print: the ids of the file, in file order, are printed_order, and the lines' lengths
are grown of the printed swarms.  Random clusterings of tests/graft_sets.py (member orders that are no identity; no graft
at all; light swarms of several members; light swarms before their heavy swarm; chains of up to 15) and the hand-made sets
the GPU tests use.  No GPU."""
import numpy as np
import pytest

import graft_layout_sets as LS
import graft_sets as GS
from swarm_amd import D1Clusters, HostDb


def _id(token: bytes) -> int:
    return int(token.split(b"_")[0][1:])


def _check(tmp_path, records, csr, swarmid, begins, order, cand):
    g = GS.closed_form(swarmid, cand)
    grafts = (g.heavy, g.light)
    want = LS.closed_form_layout(begins, order, grafts)
    LS.same_layout(want, LS.walk_chains(begins, order, grafts))
    printed_order, new_begin, grown, attached, summary = want
    w = len(begins) - 1
    own = np.diff(np.asarray(begins, dtype=np.int64))
    # what the layout promises, stated once more: a permutation; every swarm's own members are where new_begin says
    assert np.array_equal(np.sort(printed_order), np.sort(np.asarray(order, dtype=np.uint32)))
    for s in range(w):
        assert np.array_equal(printed_order[int(new_begin[s]):int(new_begin[s]) + int(own[s])], order[int(begins[s]):int(begins[s + 1])]), s
    assert int(grown[attached == 0].sum()) == len(order) and np.array_equal(grown[attached != 0], own[attached != 0])
    # ... and the file of the host's walk
    fa = tmp_path / "in.fa"
    GS.write_fasta(fa, records)
    hdb = HostDb(fa)
    cl = D1Clusters(hdb, csr[0], csr[1])
    assert np.array_equal(cl.swarmid(), swarmid)
    assert cl.graft(cand) == summary[2] and cl.graft_route() == 1
    cl.write_swarms(tmp_path / "walk.o")
    lines = [[_id(t) for t in line.split()] for line in (tmp_path / "walk.o").read_bytes().splitlines()]
    assert [a for line in lines for a in line] == printed_order.tolist()
    assert [len(line) for line in lines] == grown[attached == 0].tolist()
    assert cl.summary()["swarms"] == summary[0] and cl.summary()["largest"] == summary[1]
    return g, want


@pytest.mark.parametrize("seed,n,share", GS.CASES)
def test_closed_form_is_the_walk_on_random_clusterings(tmp_path, seed, n, share):
    case = GS.make_case(seed, n, share)
    want = case.want
    g, layout = _check(tmp_path, case.records, case.csr, want.swarmid, want.begins, want.order, case.cand)
    assert not np.array_equal(want.order, np.arange(n))          # (member orders that are no identity)
    if len(g.heavy) == 0:                                        # no graft: the layout is the clustering's own
        assert np.array_equal(layout[0], want.order) and np.array_equal(layout[1], want.begins[:-1]) and not layout[3].any()


def test_the_random_cases_exercise_the_layout():
    """over the seeds: no graft at all, light swarms of more than one member, light swarms that precede their heavy swarm,
    a chain of several light swarms"""
    seen = {"none": 0, "wide_light": 0, "light_first": 0, "longest_chain": 0}
    for seed, n, share in GS.CASES:
        case = GS.make_case(seed, n, share)
        g = GS.closed_form(case.want.swarmid, case.cand)
        own = np.diff(case.want.begins.astype(np.int64))
        seen["none"] += len(g.heavy) == 0
        seen["wide_light"] += int((own[g.light.astype(np.int64)] > 1).sum())
        seen["light_first"] += int((g.light < g.heavy).sum())
        if len(g.heavy):
            seen["longest_chain"] = max(seen["longest_chain"], int(np.bincount(g.heavy.astype(np.int64)).max()))
    print(seen)
    assert seen["none"] >= 1 and seen["wide_light"] >= 4 and seen["light_first"] >= 1 and seen["longest_chain"] >= 5, seen


@pytest.mark.parametrize("name", list(LS.HAND_MADE))
def test_closed_form_is_the_walk_on_hand_made_sets(tmp_path, name):
    records, csr, swarmid, begins, cand = LS.hand_made(name)
    n = len(swarmid)
    g, layout = _check(tmp_path, records, csr, swarmid, begins, np.arange(n, dtype=np.uint32), cand)
    assert len(g.heavy) == len(LS.HAND_MADE[name][2])


def test_light_swarms_before_their_heavy_swarm(tmp_path):
    records, csr, swarmid, begins, cand, boundary = LS.lights_first()
    g, layout = _check(tmp_path, records, csr, swarmid, begins, np.arange(10, dtype=np.uint32), cand)
    assert g.light.tolist() == [1, 4, 7, 0, 3] and set(g.heavy.tolist()) == {5}     # chain order is not swarm order
    # swarm 2, then the heavy swarm with its chain, then swarm 6
    assert layout[0].tolist() == [2, 5, 6, 7, 1, 4, 9, 0, 3, 8]
    assert layout[1].tolist() == [7, 4, 0, 8, 5, 1, 9, 6] and layout[2].tolist() == [1, 1, 1, 1, 1, 8, 1, 1]
    assert layout[4] == [3, 8, 5]
