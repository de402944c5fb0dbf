"""Inputs for the tests of the several-rank drivers (swarm_amd/csrc/multi.hip) at their edges, and what they are checked
with: sets whose window keys are shared by everybody, sets with fewer anchor groups or links than ranks, the d >= 2 graph
by alignment of all pairs, and lists for the merge kernel with numpy's stable sort as their closed form.  The properties
the GPU tests rely on are proven in tests/test_multi_sets_identity.py with numpy and the oracle only.  Not product code."""
from __future__ import annotations

import heapq

import numpy as np

import d1_sets
import support as S

WORLDS = (2, 3, 5, 8)
OTHER = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _rand(rng, length: int) -> str:
    return "".join("ACGT"[v] for v in rng.integers(0, 4, length))


def _one_edit(rng, s: str, lo: int, hi: int) -> str:
    """a substitution, deletion or insertion at a position in [lo, hi)"""
    p = int(rng.integers(lo, hi))
    how = int(rng.integers(0, 3))
    if how == 0:
        return s[:p] + OTHER[s[p]] + s[p + 1:]
    if how == 1:
        return s[:p] + s[p + 1:]
    return s[:p] + "ACGT"[int(rng.integers(0, 4))] + s[p:]


def from_records(records, path):
    """[(header str, sequence str)] -> (Db in the reference's order, the FASTA file the product's reader gets)"""
    path.write_text("".join(f">{h}\n{s}\n" for h, s in records))
    return S.build_db([(h.encode(), s.encode()) for h, s in records]), path


def from_db(db, path):
    """a database built in memory as a FASTA file (same headers: the same order once read)"""
    path.write_text("".join(f">{db.headers[i].decode()}\n{db.seq_str(i)}\n" for i in range(db.n)))
    return db, path


# ---- d = 1 ------------------------------------------------------------------------------------------------------------------
FLANK = 70


def shared_flanks(path, n: int = 9000, seed: int = 11):
    """About n amplicons of 149 .. 151 nt that all begin with the same 70 and end with the same 70 nucleotides (primers left
    on): n / 3 cores of 10 nt, each with two one-edit variants.  Every window key is the same for the whole set."""
    rng = np.random.default_rng(seed)
    head, tail = _rand(rng, FLANK), _rand(rng, FLANK)
    cores, recs = set(), []
    while len(recs) < n:
        core = _rand(rng, 10)
        if core in cores:
            continue
        cores.add(core)
        recs.append((f"c{len(recs)}_{int(rng.integers(5, 60))}", head + core + tail))
        for _ in range(2):
            v = _one_edit(rng, core, 0, 10)
            if v not in cores:
                cores.add(v)
                recs.append((f"v{len(recs)}_{int(rng.integers(1, 5))}", head + v + tail))
    return from_records(recs, path)


def shared_flanks_dense(path, seed: int = 12):
    """16 384 amplicons of 150 nt: the flanks of shared_flanks around every 7-mer (3 fixed nucleotides before it), so that
    every amplicon has 21 neighbours: 344 064 links without cluster breaking, more than two ranks' first link buffers
    (2 x 98 304) hold together"""
    rng = np.random.default_rng(seed)
    head, tail = _rand(rng, FLANK), _rand(rng, FLANK)
    recs = []
    for k in range(4 ** 7):
        core = "GAT" + "".join("ACGT"[(k >> (2 * p)) & 3] for p in range(7))
        recs.append((f"k{k}_{1 + (k * 7) % 31}", head + core + tail))
    return from_records(recs, path)


def link_cap(n: int, world: int) -> int:
    """a rank's first link buffer (multi.hip: d1_network_on_root)"""
    return 4 * n // world + 65536


def route_region(n: int, world: int) -> int:
    """records a region of a rank's outgoing lists holds (multi.hip: routed_index_build)"""
    return 3 * (n // world + 1) // (2 * world) + 1024


def longest_slice(n: int, world: int) -> int:
    return max(n * (r + 1) // world - n * r // world for r in range(world))


def few_groups(path, seed: int = 21):
    """two unrelated centroids of 150 nt, each with about 40 one-edit variants whose edit lies between the first and the
    last 64 nucleotides, and 5 unrelated singletons: 7 distinct windows at either end"""
    rng = np.random.default_rng(seed)
    recs, seen = [], set()
    for f in range(2):
        cent = _rand(rng, 150)
        seen.add(cent)
        recs.append((f"g{f}c_{30 + f}", cent))
        m = 0
        while m < 40:
            v = _one_edit(rng, cent, 64, 85)
            if v not in seen:
                seen.add(v)
                recs.append((f"g{f}v{m}_{1 + m % 4}", v))
                m += 1
    for k in range(5):
        recs.append((f"x{k}_{2 + k}", _rand(rng, 150)))
    return from_records(recs, path)


def tiny(path, n: int, seed: int = 31):
    """n sequences of 100 nt; the first two one substitution apart where there are two"""
    rng = np.random.default_rng(seed + n)
    first = _rand(rng, 100)
    recs = [("t0_9", first)]
    if n >= 2:
        recs.append(("t1_4", first[:50] + OTHER[first[50]] + first[51:]))
    while len(recs) < n:
        recs.append((f"t{len(recs)}_{1 + len(recs) % 3}", _rand(rng, 100)))
    return from_records(recs, path)


def mixed_lengths(path):
    return from_db(d1_sets.length_mix_db(), path)


def giant(path):
    return from_db(d1_sets.giant_group_db(), path)


def sorted_rows(off, nb):
    nb = nb.copy()
    for i in range(len(off) - 1):
        nb[int(off[i]):int(off[i + 1])].sort()
    return nb


def oracle_network(db, ncb: bool):
    """(offsets, neighbours ascending within every row) of the oracle; never changed afterwards"""
    off, nb, dup = S.oracle_d1_network(db, ncb)
    assert not dup
    nb = sorted_rows(off, nb)
    off.setflags(write=False)
    nb.setflags(write=False)
    return off, nb


def few_heavy(path, seed: int = 41):
    """3 heavy amplicons of 150 nt (abundance 10), five light ones (abundance 1) two substitutions away from each, and five
    light ones near nobody: fewer heavy amplicons than 5 or 8 ranks, and 15 grafts to find"""
    rng = np.random.default_rng(seed)
    recs = []
    for k in range(3):
        heavy = _rand(rng, 150)
        recs.append((f"h{k}_10", heavy))
        for v in range(5):
            t = list(heavy)
            for p in (10 + 10 * v, 80 + 5 * v):
                t[p] = OTHER[t[p]]
            recs.append((f"l{k}{v}_1", "".join(t)))
    recs += [(f"x{v}_1", _rand(rng, 150)) for v in range(5)]
    return from_records(recs, path)


# ---- d >= 2 -----------------------------------------------------------------------------------------------------------------
DN_DS = (2, 3, 9)
DN_VARIANTS = ("sparse", "no_pair", "with_short")


def _exact_edits(rng, s: str, k: int) -> str:
    """k substitutions at distinct positions 7 apart from each other: k differences in any alignment worth its score"""
    start = int(rng.integers(2, len(s) - 7 * k - 2))
    t = list(s)
    for j in range(k):
        t[start + 7 * j] = OTHER[t[start + 7 * j]]
    return "".join(t)


def dn_sparse(path, d: int, variant: str = "sparse", n: int = 130):
    """n unrelated sequences of 60 .. 120 nt and, by variant:
    sparse      a pair exactly d substitutions apart, a pair one substitution apart with tied abundances, and a pair d + 1
                substitutions apart (no link);
    no_pair     nothing else;
    with_short  the tied pair, 30 unrelated sequences below 16 (d + 1) nt, among them a pair one substitution apart, and
                a pair one insertion apart whose shorter member is the longest short sequence (16 (d + 1) - 1 nt; where that
                exceeds 120 nt — d = 9: every sequence is short — a second short pair d substitutions apart)."""
    assert variant in DN_VARIANTS
    rng = np.random.default_rng(1000 * d + 7 * DN_VARIANTS.index(variant))
    T = 16 * (d + 1)
    recs = [(f"r{k}_{1 + int(rng.integers(0, 40))}", _rand(rng, int(rng.integers(60, 121)))) for k in range(n)]
    if variant in ("sparse", "with_short"):
        a = _rand(rng, 100)
        recs += [("tie0_7", a), ("tie1_7", _exact_edits(rng, a, 1))]
    if variant == "sparse":
        a = _rand(rng, 110)
        recs += [("far0_50", a), ("far1_3", _exact_edits(rng, a, d))]
        a = _rand(rng, 120)
        recs += [("miss0_45", a), ("miss1_2", _exact_edits(rng, a, d + 1))]
    if variant == "with_short":
        lo, hi = (40, 60) if d >= 9 else (20, T)              # (random 20-mers can lie within 9 differences of each other)
        recs += [(f"s{k}_{1 + int(rng.integers(0, 9))}", _rand(rng, int(rng.integers(lo, hi)))) for k in range(30)]
        a = _rand(rng, hi - 4)
        recs += [("ss0_12", a), ("ss1_5", _exact_edits(rng, a, 1))]
        if T - 1 <= 120:
            a = _rand(rng, T - 1)
            recs += [("sl0_11", a), ("sl1_6", a[:T // 2] + OTHER[a[T // 2]] + a[T // 2:])]
        else:
            a = _rand(rng, 119)
            recs += [("sd0_11", a), ("sd1_6", _exact_edits(rng, a, d))]
    return from_records(recs, path)


_graphs: dict = {}


def brute_force_graph(db, d: int, ncb: bool):
    """(offsets u64, neighbours u32, diffs u8) of the d >= 2 graph by the oracle's nw() (orc_nw_diff, penalties 18 / 24 / 13)
    on all pairs: a link q -> t for every pair within d differences, towards the higher id always, towards the lower one
    when the abundances tie or with no cluster breaking.  (A gap column is a difference, so pairs whose lengths differ by
    more than d are beyond d and are not aligned.)"""
    key = (id(db), d)
    if key not in _graphs:
        lib = S.oracle()
        wp = [S._p(db.words(i), S.u64p) for i in range(db.n)]
        lens = db.seqlen.astype(np.int64)
        diffs = {}
        for q in range(db.n):
            for t in np.nonzero(np.abs(lens - lens[q]) <= d)[0].tolist():
                if t != q:
                    v = int(lib.orc_nw_diff(wp[t], int(lens[t]), wp[q], int(lens[q]), 18, 24, 13, None, None))
                    if v <= d:
                        diffs[q, t] = v
        _graphs[key] = (db, diffs)                           # (db: keeps the id alive)
    diffs = _graphs[key][1]
    rows = [[] for _ in range(db.n)]
    for (q, t), v in sorted(diffs.items()):
        if t > q or ncb or db.abundance[t] == db.abundance[q]:
            rows[q].append((t, v))
    off = np.zeros(db.n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    nb = np.array([t for r in rows for t, _ in r], dtype=np.uint32)
    df = np.array([v for r in rows for _, v in r], dtype=np.uint8)
    return off, nb, df


# ---- the merge kernel -------------------------------------------------------------------------------------------------------
MERGE_WORLDS = (1, 2, 3, 8, 64)
MERGE_LENGTHS = (0, 1, 2, 255, 256, 257, 1000)
MERGE_PATTERNS = ("ranges", "ranges_reversed", "interleaved", "high_bits", "ties")
MERGE_LAYOUTS = ("drawn", "all_but_one_empty", "empty_first", "empty_last", "empty_middle")


def merge_lengths(rng, world: int, layout: str) -> list:
    lens = [int(v) for v in rng.choice(MERGE_LENGTHS, world)]
    full = [v for v in MERGE_LENGTHS if v]
    if layout == "all_but_one_empty":
        keep = int(rng.integers(0, world))
        lens = [int(rng.choice(full)) if r == keep else 0 for r in range(world)]
    elif layout != "drawn":
        lens = [int(rng.choice(full)) for _ in range(world)]
        hole = (world + 2) // 3
        first = {"empty_first": 0, "empty_last": world - hole, "empty_middle": (world - hole) // 2}[layout]
        if world > 1:
            for r in range(first, first + hole):
                lens[r] = 0
        if layout == "empty_middle" and world >= 3:            # (an empty list BETWEEN two full ones)
            assert lens[first - 1] != 0 and lens[first + hole] != 0
    return lens


def merge_lists(rng, world: int, lens, pattern: str):
    """the lists [(keys u64 ascending, vals u32)] of one case; vals are distinct over all lists"""
    lists = []
    serial = 0
    for r, m in enumerate(lens):
        steps = rng.integers(1, 9, m).astype(np.uint64)
        run = np.cumsum(steps, dtype=np.uint64)              # strictly ascending, below 8000
        if pattern == "ranges":
            keys = run + np.uint64(10000 * r)
        elif pattern == "ranges_reversed":
            keys = run + np.uint64(10000 * (world - 1 - r))
        elif pattern == "interleaved":
            keys = run * np.uint64(world) + np.uint64(r)     # key % world == r
        elif pattern == "high_bits":                          # (source << 32 | target) with sources up to 2^32 - 1
            src = np.sort(rng.integers(0, 1 << 32, m, dtype=np.uint64) | np.uint64(1 << 31))
            keys = (src << np.uint64(32)) | ((run * np.uint64(world) + np.uint64(r)) & np.uint64(0xFFFFFFFF))
            keys = np.sort(keys)
        else:                                                 # ties: few distinct keys, the same in every list, runs of equal keys inside a list too
            keys = np.sort(rng.integers(0, 5, m).astype(np.uint64) * np.uint64(1 << 33) + np.uint64(3))
        vals = np.arange(serial, serial + m, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(r)
        serial += m
        lists.append((keys.astype(np.uint64), vals))
    return lists


def merge_flat(lists):
    """(keys, vals, at) as swa_merge_sorted_lists takes them"""
    at = np.zeros(len(lists) + 1, dtype=np.uint64)
    at[1:] = np.cumsum([len(k) for k, _ in lists])
    keys = np.concatenate([k for k, _ in lists]) if lists else np.zeros(0, dtype=np.uint64)
    vals = np.concatenate([v for _, v in lists]) if lists else np.zeros(0, dtype=np.uint32)
    return keys.astype(np.uint64), vals.astype(np.uint32), at


def merge_reference(lists):
    """numpy's stable sort of the concatenated lists: list order breaks ties — what upper bound below / lower bound above gives"""
    keys, vals, _ = merge_flat(lists)
    order = np.argsort(keys, kind="stable")
    return keys[order], vals[order]


def merge_by_heap(lists):
    """the same merge by the textbook: heapq.merge over (key, list, position)"""
    rows = heapq.merge(*[[(int(k), r, i) for i, k in enumerate(keys)] for r, (keys, _) in enumerate(lists)])
    rows = list(rows)
    return (np.array([k for k, _, _ in rows], dtype=np.uint64),
            np.array([lists[r][1][i] for _, r, i in rows], dtype=np.uint32))


def merge_cases():
    """(name, world, lists): every world x pattern with drawn lengths, every layout at every world, ties at every world"""
    for world in MERGE_WORLDS:
        for pattern in MERGE_PATTERNS:
            for layout in MERGE_LAYOUTS if pattern in ("interleaved", "ties") else ("drawn",):
                rng = np.random.default_rng(world * 1000 + MERGE_PATTERNS.index(pattern) * 10 + MERGE_LAYOUTS.index(layout))
                lens = merge_lengths(rng, world, layout)
                yield f"w{world}-{pattern}-{layout}", world, merge_lists(rng, world, lens, pattern)
        # lengths around the block of 256 side by side, and `all` of 1
        rng = np.random.default_rng(world)
        lens = [MERGE_LENGTHS[(r + 1) % len(MERGE_LENGTHS)] for r in range(world)]
        yield f"w{world}-interleaved-every-length", world, merge_lists(rng, world, lens, "interleaved")
        yield f"w{world}-one-element", world, merge_lists(rng, world, [1 if r == world - 1 else 0 for r in range(world)], "ranges")
