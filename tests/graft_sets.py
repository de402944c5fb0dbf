"""Small clusterings with graft candidates, and the grafting in closed form: plain numpy, no GPU.  Not product code.

What the reference's walk over the sorted (parent, child) pairs decides (src/algod1.cc:274-336, restated above
graft_sorted_pairs_in_parallel in swarm_amd/csrc/host/cluster_d1.cpp):

  * a light swarm hangs on the parent of the smallest packed pair `parent << 32 | child` among its members' candidates;
  * a heavy swarm's chain holds the light swarms it won in ascending order of those winning pairs;
  * every other candidate is withdrawn, and the heavy swarm's size, mass, length and singletons grow by its lights'.

`closed_form` states that; tests/test_graft_identity.py checks it against the sequential walk (D1Clusters.graft) and
tests/test_fastidious_resident_gpu.py hands the same cases to swa_d1_graft_device."""
from collections import namedtuple

import numpy as np

import cluster_sets as CS

NO = 0xFFFFFFFF
BOUNDARY = 8                      # light: mass < 8, so that light swarms of several members are common

Case = namedtuple("Case", "records csr want abundance seqlen light cand boundary")
Grafts = namedtuple("Grafts", "heavy light parent child kept")


def closed_form(swarmid, cand) -> Grafts:
    """the grafts in chain order — sorted by (heavy swarm, pair) — and the candidates with the losers' withdrawn"""
    swarmid = np.asarray(swarmid, dtype=np.int64)
    cand = np.asarray(cand, dtype=np.uint32)
    children = np.flatnonzero(cand != NO)
    pairs = (cand[children].astype(np.uint64) << np.uint64(32)) | children.astype(np.uint64)
    light = swarmid[children]
    at = np.lexsort((pairs, light))
    pairs, light = pairs[at], light[at]
    first = np.ones(len(at), dtype=bool)
    first[1:] = light[1:] != light[:-1]                       # the smallest pair of every light swarm
    pairs, light = pairs[first], light[first]
    parent = (pairs >> np.uint64(32)).astype(np.int64)
    child = (pairs & np.uint64(0xFFFFFFFF)).astype(np.int64)
    heavy = swarmid[parent]
    at = np.lexsort((pairs, heavy))
    kept = np.full(len(cand), NO, dtype=np.uint32)
    kept[child] = parent
    u32 = lambda a: a[at].astype(np.uint32)
    return Grafts(u32(heavy), u32(light), u32(parent), u32(child), kept)


def sums_of(swarmid, generation, abundance, seqlen, nswarms):
    """mass, total length, singletons, deepest generation of every swarm: the statement swa_d1_swarm_sums_device is held to"""
    swarmid = np.asarray(swarmid, dtype=np.int64)
    mass, sumlen = np.zeros(nswarms, dtype=np.uint64), np.zeros(nswarms, dtype=np.uint64)
    singles, maxgen = np.zeros(nswarms, dtype=np.uint32), np.zeros(nswarms, dtype=np.uint32)
    np.add.at(mass, swarmid, np.asarray(abundance, dtype=np.uint64))
    np.add.at(sumlen, swarmid, np.asarray(seqlen, dtype=np.uint64))
    np.add.at(singles, swarmid, (np.asarray(abundance) == 1).astype(np.uint32))
    np.maximum.at(maxgen, swarmid, np.asarray(generation, dtype=np.uint32))
    return mass, sumlen, singles, maxgen


def grown(sums, sizes, g: Grafts):
    """sums and sizes of the heavy swarms after the grafts (the deepest generation stays)"""
    mass, sumlen, singles, maxgen = (a.copy() for a in sums)
    sizes = np.asarray(sizes, dtype=np.uint32).copy()
    for a in (mass, sumlen, singles, sizes):
        np.add.at(a, g.heavy.astype(np.int64), a[g.light.astype(np.int64)])
    return (mass, sumlen, singles, maxgen), sizes


def properties(swarmid, cand) -> dict:
    """what a case exercises: a light swarm with several candidate children, one whose children name several parents,
    a heavy swarm that wins several light swarms, no candidate at all"""
    swarmid = np.asarray(swarmid, dtype=np.int64)
    children = np.flatnonzero(np.asarray(cand) != NO)
    per_light = {}
    for c in children:
        per_light.setdefault(int(swarmid[c]), []).append(int(cand[c]))
    g = closed_form(swarmid, cand)
    return {"several_children": any(len(v) > 1 for v in per_light.values()),
            "several_parents": any(len(set(v)) > 1 for v in per_light.values()),
            "several_lights_one_heavy": len(g.heavy) > len(set(g.heavy.tolist())),
            "withdrawn": len(children) > len(g.child),
            "no_candidates": len(children) == 0}


def make_case(seed: int, n: int = 300, share: float = 0.5, density: float = 0.8) -> Case:
    """a random clustering of n amplicons (tests/cluster_sets.py: random_graph, expected result by the reference's loop) with
    falling abundances of 1 .. 5 and lengths of 40 .. 70 nt; a `share` of the amplicons of light swarms name a random
    amplicon of a heavy swarm as their candidate.  Headers sort in id order, so the reader keeps the ids."""
    rng = np.random.default_rng(seed)
    csr, want, _ = CS.random_graph(rng, n, density, 0.3)
    abundance = np.sort(rng.integers(1, 6, n))[::-1].astype(np.uint64)
    seqlen = rng.integers(40, 71, n).astype(np.uint32)
    seen, records = set(), []
    for i in range(n):
        while True:
            s = "".join("ACGT"[v] for v in rng.integers(0, 4, int(seqlen[i])))
            if s not in seen:
                break
        seen.add(s)
        records.append((f"a{i:06d}_{int(abundance[i])}", s))
    nswarms = len(want.begins) - 1
    mass = sums_of(want.swarmid, want.generation, abundance, seqlen, nswarms)[0]
    light = (mass[want.swarmid.astype(np.int64)] < BOUNDARY).astype(np.uint8)
    heavy_ids = np.flatnonzero(light == 0)
    cand = np.full(n, NO, dtype=np.uint32)
    if len(heavy_ids):
        for c in np.flatnonzero(light != 0):
            if rng.random() < share:
                cand[c] = heavy_ids[int(rng.integers(0, len(heavy_ids)))]
    return Case(records, csr, want, abundance, seqlen, light, cand, BOUNDARY)


# (seed, amplicons, share of the light amplicons with a candidate): chosen on the CPU so that the properties above all occur
CASES = [(11, 300, 0.0), (12, 300, 0.1), (13, 320, 0.5), (14, 257, 0.9), (15, 400, 1.0), (16, 64, 0.6)]


def write_fasta(path, records) -> None:
    path.write_text("".join(f">{h}\n{s}\n" for h, s in records))
