"""Graphs for the agglomeration kernels (swarm_amd/csrc/cluster_gpu.hip) with their expected result in closed form: plain
numpy / Python, no GPU.  Every builder returns

    (offsets u64[n + 1], neighbours u32[total], diffs u8[total]),  Expected(swarmid, generation, parent, order, begins, maxgen)

in the conventions of swa_d1_cluster_device: swarms numbered by their seed's id, parent = NO_AMPLICON for seeds, `order` = the
members swarm after swarm by (generation, id), swarm s = order[begins[s]:begins[s + 1]].  The builders state label (the seed's
id), generation and parent of every vertex from how the graph was made; `expected_from` only turns those into the five arrays.
tests/test_cluster_sets_identity.py checks every closed form against the reference's loop restated (_greedy_walk)."""
from collections import namedtuple

import numpy as np

from test_walk_identity import _graph, _greedy_walk

NO_AMPLICON = 0xFFFFFFFF

Expected = namedtuple("Expected", "swarmid generation parent order begins maxgen")


def diff_of(u, v):
    """the differences of the link u -> v in the made graphs: 1..3, the same both ways"""
    return 1 + (u + v) % 3


def csr_from_rows(rows):
    """rows[u] = sorted list of (v, diff) -> offsets, neighbours, diffs"""
    n = len(rows)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    neighbours = np.array([v for r in rows for v, _ in r], dtype=np.uint32)
    diffs = np.array([d for r in rows for _, d in r], dtype=np.uint8)
    return offsets, neighbours, diffs


def csr_from_links(n, src, dst):
    """links (src[k] -> dst[k]), no duplicates -> offsets, neighbours (rows ascending), diffs = diff_of"""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    at = np.lexsort((dst, src))
    src, dst = src[at], dst[at]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(np.bincount(src, minlength=n), dtype=np.uint64)
    return offsets, dst.astype(np.uint32), (1 + (src + dst) % 3).astype(np.uint8)


def rows_from_csr(offsets, neighbours, diffs):
    return [[(int(neighbours[e]), int(diffs[e])) for e in range(int(offsets[u]), int(offsets[u + 1]))] for u in range(len(offsets) - 1)]


def expected_from(label, generation, parent):
    """label[v] = id of v's seed, generation, parent (NO_AMPLICON for seeds) -> Expected"""
    label = np.asarray(label, dtype=np.int64)
    generation = np.asarray(generation, dtype=np.int64)
    n = len(label)
    is_seed = label == np.arange(n)
    rank = np.cumsum(is_seed) - is_seed                      # seeds before v
    swarmid = rank[label]
    order = np.lexsort((np.arange(n), generation, swarmid))
    nswarms = int(is_seed.sum())
    begins = np.zeros(nswarms + 1, dtype=np.uint32)
    begins[1:] = np.cumsum(np.bincount(swarmid, minlength=nswarms))
    return Expected(swarmid.astype(np.uint32), generation.astype(np.uint32), np.asarray(parent, dtype=np.uint32), order.astype(np.uint32),
                    begins, int(generation.max()) if n else 0)


def expected_from_walk(rows):
    """the same arrays from the reference's loop (_greedy_walk), and the radius of every vertex"""
    n = len(rows)
    swarms, links = _greedy_walk(rows)
    swarmid, generation, radius = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    parent = np.full(n, NO_AMPLICON, dtype=np.uint32)
    order, begins = [], [0]
    for s, members in enumerate(swarms):
        for v, g, r in members:
            swarmid[v], generation[v], radius[v] = s, g, r
            order.append(v)
        begins.append(len(order))
    for p, v, _, _, _ in links:
        parent[v] = p
    return Expected(swarmid, generation, parent, np.array(order, dtype=np.uint32), np.array(begins, dtype=np.uint32),
                    int(generation.max()) if n else 0), radius


def rising_chain(depth, singles, spread, last_is_chain=False):
    """One chain c_0 -> c_1 -> ... -> c_depth, links forward only, ids rising along it: c_k has id 1 + k * spread (the head
    is not id 0), the other `singles` vertices have no links.  last_is_chain: c_depth has the last id instead (the last
    vertex is then no seed when depth > 0); else the last id is a singleton."""
    n = singles + depth + 1
    ids = 1 + spread * np.arange(depth + 1, dtype=np.int64)
    if last_is_chain:
        ids[depth] = n - 1
    assert singles >= 2 and (depth == 0 or ids[depth - 1] < ids[depth]) and ids[depth] < n - (0 if last_is_chain else 1)
    label = np.arange(n, dtype=np.int64)
    generation = np.zeros(n, dtype=np.int64)
    parent = np.full(n, NO_AMPLICON, dtype=np.int64)
    label[ids] = ids[0]
    generation[ids] = np.arange(depth + 1)
    parent[ids[1:]] = ids[:-1]
    return csr_from_links(n, ids[:-1], ids[1:]), expected_from(label, generation, parent)


def falling_chain(m):
    """c_0 has id 0, c_k has id m + 1 - k (k = 1..m): the ids FALL along the chain, links both ways.  One swarm, generation
    of c_k = k.  Pointer jumping gives 1..m the label 1 within a few sweeps and cannot help the label 0 on its way down from
    id m to id 1: that takes about a sweep a hop."""
    n = m + 1
    chain = np.concatenate(([0], np.arange(m, 0, -1))).astype(np.int64)       # chain[k] = id of c_k
    label = np.zeros(n, dtype=np.int64)
    generation = np.zeros(n, dtype=np.int64)
    parent = np.full(n, NO_AMPLICON, dtype=np.int64)
    generation[chain] = np.arange(n)
    parent[chain[1:]] = chain[:-1]
    src = np.concatenate((chain[:-1], chain[1:]))
    dst = np.concatenate((chain[1:], chain[:-1]))
    return csr_from_links(n, src, dst), expected_from(label, generation, parent)


def layers(width, depth, rng):
    """Swarm A: seed id 1, then `depth` layers of `width` vertices with ids in random order; a vertex of layer k takes links
    from one to three vertices of layer k - 1 (its parent = the smallest of them), every vertex links back into its own and
    earlier layers (claimed already), and into swarm B: seed id 0 with a two-level family of its own whose ids lie among
    A's.  B reaches nothing of A, so A stays A — and the level sweep has to skip A's links into B (label[v] != lu)."""
    nb_members = max(2, width)                                # B: 0 -> half of them -> the other half
    n = 2 + width * depth + nb_members
    ids = 2 + rng.permutation(n - 2)
    b_ids, a_ids = np.sort(ids[:nb_members]), ids[nb_members:]
    layer = [np.array([1])] + [np.sort(a_ids[k * width:(k + 1) * width]) for k in range(depth)]
    label = np.zeros(n, dtype=np.int64)
    generation = np.zeros(n, dtype=np.int64)
    parent = np.full(n, NO_AMPLICON, dtype=np.int64)
    links = set()
    label[1] = 1
    for k in range(1, depth + 1):
        for v in layer[k]:
            claimants = rng.choice(layer[k - 1], size=min(len(layer[k - 1]), int(rng.integers(1, 4))), replace=False)
            links.update((int(u), int(v)) for u in claimants)
            label[v], generation[v], parent[v] = 1, k, claimants.min()
            for _ in range(int(rng.integers(0, 3))):         # back into a layer already claimed (its own included)
                w = int(rng.choice(layer[int(rng.integers(0, k + 1))]))
                if w != v:
                    links.add((int(v), w))
            if rng.random() < 0.5:                            # into the other swarm
                links.add((int(v), int(rng.choice(b_ids))))
    half = nb_members // 2
    first, second = b_ids[:half], b_ids[half:]
    for v in first:
        links.add((0, int(v)))
        generation[v], parent[v] = 1, 0
    for j, v in enumerate(second):
        claimants = {int(first[j % half]), int(first[(j * 7 + 3) % half])}
        links.update((u, int(v)) for u in claimants)
        generation[v], parent[v] = 2, min(claimants)
        links.add((int(v), int(first[(j + 1) % half])))       # back up, inside B
    src, dst = zip(*sorted(links))
    return csr_from_links(n, src, dst), expected_from(label, generation, parent)


def random_graph(rng, n, density, ties, arbitrary=False):
    """_graph of test_walk_identity.py (links from lower to higher ids, both ways where abundances tie), or — arbitrary — links
    in any direction; the expected result by the reference's loop.  Returns (csr, Expected, radius)."""
    if arbitrary:
        rows = [dict() for _ in range(n)]
        for _ in range(int(density * n)):
            u, v = (int(x) for x in rng.integers(0, n, 2))
            if u != v:
                rows[u][v] = diff_of(u, v)
        rows = [sorted(r.items()) for r in rows]
    else:
        rows = _graph(rng, n, density, ties)
    want, radius = expected_from_walk(rows)
    return csr_from_rows(rows), want, radius
