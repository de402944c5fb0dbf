"""The grafted clustering as one layout (swa_d1_graft_layout_device, swarm_amd/csrc/fast_graft.inc), in plain numpy: no GPU.
Not product code.

A clustering of w swarms — bounds begins[w + 1] into the member order order[n] — and G grafts in chain order (heavy[i] wins
light[i]; sorted by heavy swarm, then by the winning pair: tests/graft_sets.py, closed_form).  The writers print the
unattached swarms in swarm order: a swarm's own members, then the members of each light swarm of its chain, in chain order.

  closed_form_layout   that order and where every swarm lies in it, by integer scans (the statement the device is held to)
  walk_chains          the same by building the chains and walking them, the way the reference's writers do

and the block graphs the GPU tests adopt: swarm k = the next sizes[k] ids, its first id linked to all the others."""
import numpy as np

import cluster_sets as CS


def closed_form_layout(begins, order, grafts):
    """grafts = (heavy, light) in chain order -> (printed_order u32[n], new_begin u32[w], grown u32[w], attached u8[w],
    summary3 [w - G, the largest grown among the printed swarms, G])"""
    begins = np.asarray(begins, dtype=np.int64)
    order = np.asarray(order, dtype=np.uint32)
    heavy, light = (np.asarray(a, dtype=np.int64) for a in grafts)
    w, n, G = len(begins) - 1, len(order), len(heavy)
    own = np.diff(begins)
    attached = np.zeros(w, dtype=np.uint8)
    attached[light] = 1
    ends = np.concatenate(([0], np.cumsum(own[light])))          # E: exclusive scan of the light swarms' sizes, E[G] the total
    first = np.ones(G, dtype=bool)
    first[1:] = heavy[1:] != heavy[:-1]
    last = np.ones(G, dtype=bool)
    last[:-1] = heavy[1:] != heavy[:-1]
    run_first, run_end = np.zeros(w, dtype=np.int64), np.zeros(w, dtype=np.int64)
    run_first[heavy[first]] = np.flatnonzero(first)
    run_end[heavy[last]] = np.flatnonzero(last) + 1
    grown = own + ends[run_end] - ends[run_first]
    printed = np.where(attached != 0, 0, grown)
    new_begin = np.concatenate(([0], np.cumsum(printed)))[:w]
    new_begin[light] = new_begin[heavy] + own[heavy] + ends[:G] - ends[run_first[heavy]]
    swarm_of_place = np.repeat(np.arange(w), own)                # the swarm of the member at position k of the order
    printed_order = np.zeros(n, dtype=np.uint32)
    printed_order[new_begin[swarm_of_place] + np.arange(n) - begins[swarm_of_place]] = order
    summary = [w - G, int(printed.max()) if w else 0, G]
    return printed_order, new_begin.astype(np.uint32), grown.astype(np.uint32), attached, summary


def walk_chains(begins, order, grafts):
    """the same five by linking every light swarm behind the tail of its heavy swarm's chain, in the order of the graft
    arrays, and walking the chains swarm by swarm; nothing shared with closed_form_layout but the inputs"""
    w, n = len(begins) - 1, len(order)
    head, tail, nxt = [None] * w, [None] * w, [None] * w
    attached = [0] * w
    for h, l in zip((int(v) for v in grafts[0]), (int(v) for v in grafts[1])):
        if head[h] is None:
            head[h] = l
        else:
            nxt[tail[h]] = l
        tail[h] = l
        attached[l] = 1
    printed_order, new_begin, grown = [], [0] * w, [0] * w
    for s in range(w):
        grown[s] = int(begins[s + 1]) - int(begins[s])
    for s in range(w):
        if attached[s]:
            continue
        new_begin[s] = len(printed_order)
        printed_order += [int(a) for a in order[int(begins[s]):int(begins[s + 1])]]
        g = head[s]
        while g is not None:
            new_begin[g] = len(printed_order)
            printed_order += [int(a) for a in order[int(begins[g]):int(begins[g + 1])]]
            grown[s] += int(begins[g + 1]) - int(begins[g])
            g = nxt[g]
    assert len(printed_order) == n
    largest = max((grown[s] for s in range(w) if not attached[s]), default=0)
    return (np.array(printed_order, dtype=np.uint32), np.array(new_begin, dtype=np.uint32), np.array(grown, dtype=np.uint32),
            np.array(attached, dtype=np.uint8), [w - len(grafts[0]), largest, len(grafts[0])])


def same_layout(got, want) -> None:
    for g, w, name in zip(got[:4], want[:4], ("printed_order", "new_begin", "grown", "attached")):
        assert np.asarray(g).dtype == np.asarray(w).dtype and np.array_equal(g, w), name
    assert [int(v) for v in got[4]] == [int(v) for v in want[4]], "summary3"


# ---- block graphs ---------------------------------------------------------------------------------------------------------
def blocks(sizes, abundance):
    """swarm k = the next sizes[k] ids: its first id is the seed and links to all the others, so the member order is
    0, 1, 2, ... and swarm k begins at member sum(sizes[:k]).  abundance: one value per amplicon, falling along the ids (the
    reader sorts by abundance: the ids must survive it).  Returns (records, csr, swarmid, begins)."""
    n = int(sum(sizes))
    abundance = np.asarray(abundance, dtype=np.uint64)
    assert len(abundance) == n and (np.diff(abundance.astype(np.int64)) <= 0).all()
    rng = np.random.default_rng(n)
    src, dst, swarmid = [], [], np.zeros(n, dtype=np.uint32)
    at = 0
    for k, size in enumerate(sizes):
        swarmid[at:at + size] = k
        src += [at] * (size - 1)
        dst += list(range(at + 1, at + size))
        at += size
    csr = CS.csr_from_links(n, src, dst) if src else (np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8))
    seen, records = set(), []
    for i in range(n):
        while True:
            s = "".join("ACGT"[v] for v in rng.integers(0, 4, 40))
            if s not in seen:
                break
        seen.add(s)
        records.append((f"a{i:06d}_{int(abundance[i])}", s))
    begins = np.concatenate(([0], np.cumsum(sizes))).astype(np.uint32)
    return records, csr, swarmid, begins


def block_abundance(sizes, heavy_swarms, high=9, low=1):
    """members of the swarms in heavy_swarms get `high`, all others `low`; asserts in blocks() that this falls along the ids"""
    return np.concatenate([np.full(size, high if k in heavy_swarms else low, dtype=np.uint64) for k, size in enumerate(sizes)])


# name -> (sizes, heavy swarms, {light swarm: heavy swarm}): the candidate of a light swarm's FIRST member is its heavy swarm's seed
HAND_MADE = {
    # 3 heavy + 257 one-member light swarms: runs of 86 / 86 / 85 cross waves, graft 257 sits in the second workgroup
    "257_grafts": ([1] * 260, {0, 1, 2}, {3 + i: i % 3 for i in range(257)}),
    # one heavy swarm wins 5000 one-member light swarms: one run across many workgroups and across the scan's tiles
    "one_run_of_5000": ([2] + [1] * 5000 + [3], {0}, {1 + i: 0 for i in range(5000)}),
    # light swarms of 1, 2, 63, 64, 65 and 300 members on one heavy swarm of 3000: blocks that start and end on both sides of
    # wave and workgroup edges in the move kernel; n = 3000 + 495 + 2 = 3497 is no multiple of 64
    "blocks_across_edges": ([3000, 1, 2, 63, 64, 65, 300, 2], {0}, {1: 0, 2: 0, 3: 0, 4: 0, 5: 0, 6: 0}),
    "one_swarm": ([777], set(), {}),
    "one_amplicon": ([1], set(), {}),
}


def hand_made(name):
    """(records, csr, swarmid, begins, cand): the candidates name the seed of the heavy swarm"""
    sizes, heavy_swarms, hang = HAND_MADE[name]
    records, csr, swarmid, begins = blocks(sizes, block_abundance(sizes, heavy_swarms))
    cand = np.full(int(sum(sizes)), 0xFFFFFFFF, dtype=np.uint32)
    for l, h in hang.items():
        cand[int(begins[l])] = begins[h]
    return records, csr, swarmid, begins, cand


def lights_first():
    """light swarms that PRECEDE their heavy swarm in swarm order: five light singletons of abundance 2, then a heavy swarm of
    three members of abundance 1 (mass 3: heavy at boundary 3), then two light singletons of abundance 1 behind it.
    (records, csr, swarmid, begins, cand, boundary)"""
    sizes = [1] * 5 + [3] + [1] * 2
    abundance = [2] * 5 + [1] * 3 + [1] * 2
    records, csr, swarmid, begins = blocks(sizes, abundance)
    cand = np.full(10, 0xFFFFFFFF, dtype=np.uint32)
    cand[[0, 1, 3, 4]] = [6, 5, 7, 5]                             # parents: members of the heavy swarm (ids 5, 6, 7)
    cand[9] = 5                                                   # ... and one light swarm behind it
    return records, csr, swarmid, begins, cand, 3
