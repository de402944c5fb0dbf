"""What swarm_amd/csrc/dn_tables.inc makes of a clustering, on the CPU: plain numpy / Python, no GPU.

`walk_tables` is the reference's greedy loop restated (cluster_over_graph, swarm_amd/csrc/host/cluster_dn.cpp; the loop itself
is test_walk_identity._greedy_walk, which emits every member's radius and every accepted pair as it goes) turned into the
arrays swa_dn_tables_fetch returns.  The other functions are models of the device's steps, each checked against that loop in
tests/test_dn_tables_identity.py: the stable-sort identity behind the links, the ping-pong pointer jumping behind the radii,
and the segmented maximum along the member order with its two ways of writing."""
from collections import namedtuple

import numpy as np

import cluster_sets as CS
from test_walk_identity import _greedy_walk

NO_AMPLICON = CS.NO_AMPLICON

Tables = namedtuple("Tables", "expected radius mass singletons maxgen maxradius link_parent link_child link_generation link_diff "
                              "link_swarm link_begin link_end")


def abundances(n):
    """1, 2, 3, 1, 2, 3, ...: a third of the amplicons are singletons"""
    return (1 + np.arange(n) % 3).astype(np.uint64)


def walk_tables(rows, abundance=None):
    """rows[u] = sorted (v, diff) -> Tables by the greedy loop: Expected of cluster_sets, radius[n], the swarms' sums (maxgen
    = the deepest generation itself, 0 for a swarm of one), and the accepted pairs in acceptance order with every swarm's
    range of them"""
    n = len(rows)
    abundance = abundances(n) if abundance is None else np.asarray(abundance, dtype=np.uint64)
    swarms, links = _greedy_walk(rows)
    expected, radius = CS.expected_from_walk(rows)
    w = len(swarms)
    mass = np.zeros(w, dtype=np.uint64)
    singletons, maxgen, maxradius, link_begin, link_end = (np.zeros(w, dtype=np.uint32) for _ in range(5))
    for s, members in enumerate(swarms):
        ids = [v for v, _, _ in members]
        mass[s] = abundance[ids].sum()
        singletons[s] = int((abundance[ids] == 1).sum())
        maxgen[s] = max(g for _, g, _ in members)
        maxradius[s] = max(r for _, _, r in members)
    swarm_of_link = np.array([s for _, _, _, s, _ in links], dtype=np.int64)
    link_begin[:] = np.searchsorted(swarm_of_link, np.arange(1, w + 1), side="left")      # (the pairs come swarm after swarm)
    link_end[:] = np.searchsorted(swarm_of_link, np.arange(1, w + 1), side="right")
    col = lambda k, dtype: np.array([l[k] for l in links], dtype=dtype)
    return Tables(expected, radius, mass, singletons, maxgen, maxradius, col(0, np.uint32), col(1, np.uint32), col(4, np.uint32),
                  col(2, np.uint8), col(3, np.uint32), link_begin, link_end)


def tables_of(csr, abundance=None):
    return walk_tables(CS.rows_from_csr(*csr), abundance)


def parent_diffs(rows, parent):
    """diff(parent, v) per amplicon, 0 for seeds, 0xFF where the parent has no link to v: what k_dt_init looks up"""
    lookup = [dict(r) for r in rows]
    return np.array([0 if p == NO_AMPLICON else lookup[p].get(v, 0xFF) for v, p in enumerate(int(p) for p in parent)], dtype=np.uint8)


def links_by_stable_sort(order, begins, parent):
    """The identity behind k_dt_link_keys / the radix sort / k_dt_link_gather: the links of the whole clustering in acceptance
    order are the non-seed positions k of `order`, stably sorted by pos_of[parent[order[k]]], k ascending going in; position
    k of swarm s is non-seed entry k - s - 1.  Returns the sorted positions."""
    order = np.asarray(order, dtype=np.int64)
    n = len(order)
    pos_of = np.zeros(n, dtype=np.int64)
    pos_of[order] = np.arange(n)
    nswarms = len(begins) - 1
    swarm_at = np.repeat(np.arange(nswarms), np.diff(np.asarray(begins, dtype=np.int64)))      # swarm of position k
    keys = np.zeros(n - nswarms, dtype=np.int64)
    vals = np.zeros(n - nswarms, dtype=np.int64)
    written = np.zeros(n - nswarms, dtype=bool)
    for k in range(n):
        s = swarm_at[k]
        if k == begins[s]:
            continue
        j = k - s - 1
        assert 0 <= j < n - nswarms and not written[j]
        keys[j], vals[j], written[j] = pos_of[parent[order[k]]], k, True
    assert written.all() and (np.diff(vals) > 0).all()          # (every entry once, k ascending going in)
    return vals[np.argsort(keys, kind="stable")]


def jump_model(parent, pdiff):
    """k_dt_init's pairs and k_dt_jump's rounds, two buffers: a round reads only what the round before wrote.  Returns (radius,
    rounds until every ancestor has passed the seed)."""
    parent = np.asarray(parent, dtype=np.int64)
    n = len(parent)
    unset = int(NO_AMPLICON)
    anc = [parent.copy(), np.zeros(n, dtype=np.int64)]
    acc = [np.asarray(pdiff, dtype=np.int64).copy(), np.zeros(n, dtype=np.int64)]
    rounds = 0
    while (anc[rounds & 1] != unset).any():
        a_in, r_in = anc[rounds & 1], acc[rounds & 1]
        a_out, r_out = anc[(rounds + 1) & 1], acc[(rounds + 1) & 1]
        for v in range(n):
            a, r = a_in[v], r_in[v]
            if a != unset:
                r += r_in[a]
                a = a_in[a]
            a_out[v], r_out[v] = a, r
        rounds += 1
        assert rounds <= 64
    return acc[rounds & 1].astype(np.uint32), rounds


def jump_rounds(maxgen):
    """ceil(log2(maxgen + 1)) = bit_width(maxgen): the rounds the host launches"""
    return int(maxgen).bit_length()


def segmented_max(order, swarmid, radius, begins, wave=64):
    """k_dt_maxradius: waves of 64 positions of the member order; every run of equal swarms inside a wave is reduced, its
    result stored plainly when the run is the whole swarm and folded in with a maximum otherwise.  Returns (maxradius per
    swarm, plain stores, atomic maxima); a plain store onto an entry somebody wrote already is an error of the rule."""
    n = len(order)
    nswarms = len(begins) - 1
    out = np.zeros(nswarms, dtype=np.uint32)
    touched = np.zeros(nswarms, dtype=bool)
    plain = atomic = 0
    for w0 in range(0, n, wave):
        k = w0
        while k < min(n, w0 + wave):
            s = int(swarmid[order[k]])
            e = k
            while e + 1 < min(n, w0 + wave) and int(swarmid[order[e + 1]]) == s:
                e += 1
            m = max(int(radius[order[j]]) for j in range(k, e + 1))
            if k == begins[s] and e + 1 == begins[s + 1]:
                assert not touched[s]
                out[s] = m
                plain += 1
            else:
                out[s] = max(int(out[s]), m)
                atomic += 1
            touched[s] = True
            k = e + 1
    assert touched.all()
    return out, plain, atomic


# ---- graphs for tests/test_dn_tables_gpu.py ---------------------------------------------------------------------------------

def wide_swarm(n=3001, star=700, width=100, small=400, lane_gap=None):
    """One wide swarm around seed 0 — a star of `star` members, then layers of `width`, each member linked from one to three
    members of the layer before — whose run in the member order spans many waves and several workgroups (k_dt_maxradius'
    atomicMax path), and behind it `small` amplicons in swarms of one and two members (its plain stores).  The wide swarm
    takes the ids 0 .. n - small - 1, so its run ends at position n - small; lane_gap singles and then a swarm of two are
    placed so that the pair's run starts in a wave's last lane and ends in the next wave's first."""
    rng = np.random.default_rng(n)
    big = n - small
    rows = [dict() for _ in range(n)]
    layer = [np.array([0]), np.arange(1, 1 + star)]
    at = 1 + star
    while at < big:
        layer.append(np.arange(at, min(big, at + width)))
        at += width
    for k in range(1, len(layer)):
        for v in layer[k]:
            for u in rng.choice(layer[k - 1], size=min(len(layer[k - 1]), int(rng.integers(1, 4))), replace=False):
                rows[int(u)][int(v)] = CS.diff_of(int(u), int(v))
    # the small swarms: positions = ids from `big` on (they are their own swarms, in id order); singles up to the position
    # whose lane is 63, then a pair, then pairs and singles alternating
    v = big
    if lane_gap is None:
        lane_gap = (63 - big) % 64
    v += lane_gap
    assert v % 64 == 63 and v + 1 < n
    while v + 1 < n:
        rows[v][v + 1] = CS.diff_of(v, v + 1)                   # a swarm of two: v -> v + 1
        v += 3                                                 # ... and a single behind it
    return CS.csr_from_rows([sorted(r.items()) for r in rows])


def heavy_chain(depth, singles):
    """a chain of `depth` links whose every difference is 254 (radius of the last member = 254 depth), ids rising along it
    from id 1 on, then `singles` amplicons without links (id 0 is one of them)"""
    n = 1 + depth + 1 + singles - 1
    rows = [[] for _ in range(n)]
    for k in range(depth):
        rows[1 + k] = [(2 + k, 254)]
    return CS.csr_from_rows(rows)
