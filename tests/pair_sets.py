"""Sets that put every form of the d = 1 pair kernels (swarm_amd/csrc/d1_anchor.inc: k_d1_group_pairs and k_d1_pairs_tiled,
PASS 0 / 1 x record width W = 5, 8, 15, 21 words x window width NW = 1, 2, 4 words, and window mode) to work on purpose, and
the exact CPU models that say which form a set reaches and what the network has to be.  Shared by
tests/test_pair_sets_identity.py (no GPU) and tests/test_pair_forms_gpu.py (no test file imports another).

Everything is seeded and deterministic.  A builder returns a list of distinct sequences (strings over ACGT), some with a
dictionary of what was planted; `database` gives them abundances from a small set with many ties — the rank rule of the
kernels, m.rank <= prank, then decides in both directions — and packs them as the other d = 1 tests do.

Nothing here is product code: the key of a window (anchor_fold, mix64 >> 35), the width classes, the size kinds of the work
lists and the items of the tiled kernel are restated from the comments of d1_common.inc / key_ops.inc in numpy and Python."""
import functools

import numpy as np

import support as S

EDGES = {5: 160, 8: 256, 15: 480, 21: 672}         # longest sequence a record of W words holds: the width classes' upper edges
LOWER = {5: 1, 8: 161, 15: 257, 21: 481}           # shortest sequence of the class
CLASS_OF = {5: 0, 8: 1, 15: 2, 21: 3}
FORMS = [(5, 1), (5, 2), (8, 1), (8, 2), (15, 1), (15, 2), (15, 4), (21, 1), (21, 2), (21, 4)]   # SWA_PAIR_CASES of d1.hip, per PASS
KINDS = ("sub", "del", "ins")
ABUNDANCES = (1, 1, 1, 2, 2, 3, 7, 50)
GROUP_CAP = 4096                                   # kStreamGroupCap: larger groups go to the plain kernel
PAIR_BIG = 256                                     # kPairBigCap: groups of 65..256 take a workgroup of k_d1_group_pairs
TILED_COLS = 4                                     # kTiledCols
KIND_BIG, KIND_TILED = 5, 6                        # list kinds 0..4: bundles of groups up to 4, 8, 16, 32, 64 members
SIZES = (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 66, 128, 255, 256)     # both sides of every boundary between the kinds 0..5
SIZES_SMALL = (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)                   # the same up to the first 65..256 group
MAX_SEQUENCES = 4600
LETTERS = "ACGT"


def upper_centre(W: int) -> int:
    """centre length whose insertions are exactly as long as the class allows (160 / 256 / 480 / 672: nothing to shift)"""
    return EDGES[W] - 1


def lower_centre(W: int, NW: int) -> int:
    """centre length whose deletions are the shortest sequences of the class that still have two windows and a nucleotide;
    W = 5 with NW = 1: 80 nt — a centre much shorter has fewer than 256 single edits outside a window of 32 nt, so no group
    of the 65..256 or the tiled kind could be planted on it"""
    if (W, NW) == (5, 1):
        return 80
    return max(LOWER[W], 64 * NW + 1) + 1


def form_lengths(W: int, NW: int):
    return (upper_centre(W), lower_centre(W, NW))


# ---------------------------------------------------------------------------------------------- edits

def substitute(s: str, p: int, c: str) -> str:
    return s[:p] + c + s[p + 1:]


def delete(s: str, p: int) -> str:
    return s[:p] + s[p + 1:]


def insert(s: str, p: int, c: str) -> str:
    """c in front of position p (p = len(s): behind the end)"""
    return s[:p] + c + s[p:]


def random_sequence(rng, length: int) -> str:
    return "".join(rng.choice(list(LETTERS), size=length))


def runless_sequence(rng, length: int) -> str:
    """random, no two neighbouring nucleotides equal: a deletion or an insertion (of a letter its neighbours do not have) at p
    is then the edit at p and nowhere else, so which dword carries the difference is known"""
    steps = rng.integers(1, 4, size=length)
    steps[0] = rng.integers(0, 4)
    return "".join(LETTERS[int(v)] for v in np.cumsum(steps) % 4)


def edge_positions(W: int, L: int, NW=None) -> list:
    """Where a difference is the first or the last nucleotide of a dword of either chain of pair_near, for a sequence of L nt
    in a record of W words: 16 k and 16 k + 15 (forward dwords, k < 2 W), L - 1 - 16 k and L - 16 - 16 k (end-aligned dwords),
    and the four positions around the two window boundaries of 32 NW nt (NW = None: of every window width)."""
    out = set()
    for k in range(2 * W):
        out.update((16 * k, 16 * k + 15, L - 1 - 16 * k, L - 16 - 16 * k))
    for nw in ((1, 2, 4) if NW is None else (NW,)):
        out.update((32 * nw - 1, 32 * nw, L - 32 * nw - 1, L - 32 * nw))
    return sorted(p for p in out if 0 <= p < L)


def edit_place(p: int, kind: str, L: int, NW: int) -> str:
    """which window an edit at p of a run-less sequence of L nt changes: `first`, `last`, or neither (`interior`)"""
    w = 32 * NW
    if p < w:
        return "first"
    if kind == "ins":
        return "last" if p > L - w else "interior"
    return "last" if p >= L - w else "interior"


def edit_variants(s: str, p: int, kind: str) -> list:
    """the sequences one edit of `kind` at p makes of a run-less s, each different from any other edit's"""
    if kind == "sub":
        return [substitute(s, p, c) for c in LETTERS if c != s[p]]
    if kind == "del":
        return [delete(s, p)]
    shut = {s[p]} | ({s[p - 1]} if p > 0 else set())
    return [insert(s, p, c) for c in LETTERS if c not in shut]


def single_edit_sweep(centre: str, kinds=KINDS) -> list:
    """the centre and every substitution, deletion and insertion of it (those of `kinds`), each once"""
    out, seen = [centre], {centre}
    for p in range(len(centre) + 1):
        cand = []
        if p < len(centre) and "sub" in kinds:
            cand += [substitute(centre, p, c) for c in LETTERS if c != centre[p]]
        if p < len(centre) and "del" in kinds:
            cand.append(delete(centre, p))
        if "ins" in kinds:
            cand += [insert(centre, p, c) for c in LETTERS]
        for s in cand:
            if s not in seen:
                seen.add(s)
                out.append(s)
    return out


# ---------------------------------------------------------------------------------------------- databases

def database(seqs, seed: int = 0, twins=()):
    """(db, text): the packed database of `seqs` with tied abundances, and text[i] = the sequence of amplicon i.
    twins: numbers of sequences that the database holds a second time (abundance 1)"""
    rng = np.random.default_rng(1000 + seed)
    ab = rng.choice(ABUNDANCES, size=len(seqs))
    records = [(f"s{i}_{int(ab[i])}".encode(), s.encode()) for i, s in enumerate(seqs)]
    records += [(f"t{i}_1".encode(), seqs[i].encode()) for i in twins]
    db = S.build_db(records)
    order = [int(h[1:h.index(b"_")]) for h in db.headers]
    return db, [seqs[k] for k in order]


def codes_matrix(seqs):
    """(codes u8 [n, longest], lengths): what tests/index_prep_model.py's window model reads"""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    codes = np.zeros((len(seqs), int(lens.max())), dtype=np.uint8)
    lut = np.zeros(256, dtype=np.uint8)
    for k, c in enumerate(LETTERS):
        lut[ord(c)] = k
    for i, s in enumerate(seqs):
        codes[i, :len(s)] = lut[np.frombuffer(s.encode(), dtype=np.uint8)]
    return codes, lens


# ---------------------------------------------------------------------------------------------- keys and groups

_M1, _M2 = np.uint64(0xff51afd7ed558ccd), np.uint64(0xc4ceb9fe1a85ec53)
_SALT = np.uint64(0x9E3779B97F4A7C15)
_S33 = np.uint64(33)


def _mix64(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> _S33)
    x = x * _M1
    x = x ^ (x >> _S33)
    x = x * _M2
    return x ^ (x >> _S33)


def key29_model(windows, which: int) -> np.ndarray:
    """the 29 bits a group is keyed by: windows u64 [m, NW] (32 nt a word, the first in the lowest bits) -> u32 [m].
    anchor_fold: h = mix64(w0 ^ salt of the suffix side), h = mix64(h ^ wk) for the further words, the top bit dropped;
    the key is mix64(h) >> 35"""
    windows = np.atleast_2d(np.asarray(windows, dtype=np.uint64))
    h = _mix64(windows[:, 0] ^ (_SALT if which else np.uint64(0)))
    for k in range(1, windows.shape[1]):
        h = _mix64(h ^ windows[:, k])
    h = h & np.uint64(0x7FFFFFFFFFFFFFFF)
    return (_mix64(h) >> np.uint64(35)).astype(np.uint32)


def window_words(text: str) -> np.ndarray:
    assert len(text) % 32 == 0
    return S.pack_seq(text.encode())


def words_text(words) -> str:
    return "".join(LETTERS[(int(w) >> (2 * k)) & 3] for w in words for k in range(32))


def find_collision(NW: int, which: int, rng, draws: int = 300000):
    """two different windows of 32 NW nt with one key on side `which`: a birthday search (2^29 keys: 300 000 random windows
    hold about 80 colliding pairs)"""
    windows = rng.integers(0, 2 ** 64, size=(draws, NW), dtype=np.uint64)
    keys = key29_model(windows, which)
    order = np.argsort(keys, kind="stable")
    same = np.flatnonzero(keys[order][1:] == keys[order][:-1])
    for k in same:
        a, b = windows[order[k]], windows[order[k + 1]]
        if not np.array_equal(a, b):
            return words_text(a), words_text(b)
    raise AssertionError("no collision among the draws")


def width_class(length: int) -> int:
    return 0 if length <= 160 else (1 if length <= 256 else (2 if length <= 480 else (3 if length <= 672 else 4)))


def size_kind(g: int) -> int:
    """list kind of a group of g members (2 .. GROUP_CAP)"""
    if g <= 64:
        return 0 if g <= 4 else (1 if g <= 8 else (2 if g <= 16 else (3 if g <= 32 else 4)))
    return KIND_BIG if g <= PAIR_BIG else KIND_TILED


def tiled_item_count(members: int, cols: int = TILED_COLS) -> int:
    """items of k_d1_pairs_tiled for one group: every row tile of 64 members against its column tiles, `cols` an item"""
    tiles = (members + 63) // 64
    return sum((tiles - r + cols - 1) // cols for r in range(tiles))


def group_model(seqs, NW: int, offset: int = 0, merge: bool = True) -> dict:
    """The two anchor indexes of `seqs` under windows of 32 NW nt, `offset` nt from the ends: index 0 groups by
    [offset, offset + 32 NW), index 1 by the same from the end; a sequence shorter than offset + 32 NW is in neither.  Groups
    whose windows have one 29-bit key are one group (merge).  A group's width class is that of its longest member.
      groups[i]    [(members, class)] of index i, singletons included
      counts       u32 [2, 4, 8]: items of list (index, class, kind) — groups, and for kind 6 tiled_item_count of each group
      oversized    groups of more than GROUP_CAP members (left to the plain kernel, on no list)
      largest      members of the largest group"""
    w = 32 * NW
    groups = []
    for which in range(2):
        by_text = {}
        for s in seqs:
            if len(s) < offset + w:
                continue
            text = s[offset:offset + w] if which == 0 else s[len(s) - offset - w:len(s) - offset]
            by_text.setdefault(text, []).append(len(s))
        if merge:
            texts = list(by_text)
            keys = key29_model(np.stack([window_words(t) for t in texts]), which) if texts else []
            by_key = {}
            for t, k in zip(texts, keys):
                by_key.setdefault(int(k), []).extend(by_text[t])
            by_text = by_key
        groups.append([(len(v), width_class(max(v))) for v in by_text.values()])
    counts = np.zeros((2, 4, 8), dtype=np.uint32)
    oversized = 0
    for which in range(2):
        for g, cls in groups[which]:
            assert cls < 4, "a sequence beyond the pair kernels"
            if g > GROUP_CAP:
                oversized += 1
            elif g >= 2:
                kind = size_kind(g)
                counts[which, cls, kind] += tiled_item_count(g) if kind == KIND_TILED else 1
    return {"groups": groups, "counts": counts, "oversized": oversized,
            "largest": max(g for gs in groups for g, _ in gs)}


# ---------------------------------------------------------------------------------------------- the network, by definition

def one_edit(a: np.ndarray, b: np.ndarray) -> bool:
    """exactly one substitution, deletion or insertion turns a into b (arrays of letters)"""
    if len(a) == len(b):
        return int(np.count_nonzero(a != b)) == 1
    if len(a) > len(b):
        a, b = b, a
    if len(b) - len(a) != 1:
        return False
    differ = np.flatnonzero(a != b[:len(a)])
    p = int(differ[0]) if len(differ) else len(a)          # the nucleotide of b that a lacks
    return bool(np.array_equal(a[p:], b[p + 1:]))


def brute_network(text, abundance, ncb: bool, first: int = 0, count=None):
    """The d = 1 network from its definition: i and j are linked when one edit turns one into the other, and row i lists j
    when cluster breaking is off or j is not more abundant than i.  CSR (offsets u64, neighbours u32 ascending per row)
    over the seeds [first, first + count), as swa_d1_network returns it.  Quadratic: for a few hundred sequences."""
    n = len(text)
    count = n - first if count is None else count
    arr = [np.frombuffer(s.encode(), dtype=np.uint8) for s in text]
    rows = [[] for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            if abs(len(arr[i]) - len(arr[j])) <= 1 and one_edit(arr[i], arr[j]):
                if ncb or abundance[i] >= abundance[j]:
                    rows[i].append(j)
                if ncb or abundance[j] >= abundance[i]:
                    rows[j].append(i)
    off = np.zeros(count + 1, dtype=np.uint64)
    nb = []
    for k in range(count):
        nb += sorted(rows[first + k])
        off[k + 1] = len(nb)
    return off, np.array(nb, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------- families of planted edits

@functools.lru_cache(maxsize=None)
def families(W: int, NW: int, L: int, sizes=SIZES, where: str = "interior"):
    """One run-less centre of L nt per entry of `sizes`; its members are the centre and single edits of it.  The edits go
    through (position, kind) for the positions of edge_positions(W, L, NW) that `where` admits — `interior`: outside both
    windows (both indexes hold a group of that size), `first`: inside the first window (the suffix group has that size and
    PASS 1 has to emit), `last`: inside the last window (PASS 0, with its shortened suffix chain) — cyclically across the
    families of the call, so that together they use every such position with every kind of edit.  Where a family wants more
    members than those make, the other positions of the region follow, then those of the interior (`interior`: of the first
    window), so the group of the index named above still has its size.
    Returns (sequences, plan): plan["edits"] = [(family, position, kind)] as planted, plan["served"] = {index: sizes of the
    families that are one group of that index}."""
    assert where in ("interior", "first", "last") and L - 1 >= 64 * NW + 1 and L + 1 <= EDGES[W]
    rng = np.random.default_rng([W, NW, L, len(sizes)])
    centres = [runless_sequence(rng, L) for _ in sizes]
    combos = [(p, k) for p in edge_positions(W, L, NW) for k in KINDS if edit_place(p, k, L, NW) == where]
    region = [(p, k) for p in range(L) for k in KINDS if edit_place(p, k, L, NW) == where and p not in edge_positions(W, L, NW)]
    spill_to = "first" if where == "interior" else "interior"
    spill = [(p, k) for p in range(L) for k in KINDS if edit_place(p, k, L, NW) == spill_to]
    seqs, seen, edits, whole = [], set(), [], []
    cursor = 0
    for f, (size, centre) in enumerate(zip(sizes, centres)):
        fam = [centre]
        seen.add(centre)
        spilled = False

        def take(p, kind, turn):
            v = edit_variants(centre, p, kind)
            if turn < len(v) and v[turn] not in seen:
                seen.add(v[turn])
                fam.append(v[turn])
                edits.append((f, p, kind))

        for _ in range(3 * len(combos)):                     # the edge positions, on from where the last family stopped
            if len(fam) == size or not combos:
                break
            p, kind = combos[cursor % len(combos)]
            take(p, kind, cursor // len(combos) % 3)
            cursor += 1
        for pool in (region, spill):
            for turn in range(3):
                for p, kind in pool:
                    if len(fam) == size:
                        break
                    before = len(fam)
                    take(p, kind, turn)
                    spilled = spilled or (pool is spill and len(fam) != before)
        assert len(fam) == size, (W, NW, L, where, size)
        whole.append(not spilled)
        seqs += fam
    assert len(set(seqs)) == len(seqs)
    # the index whose window the edits leave alone holds every family as one group (what spills goes to the interior, or from
    # the interior into the first window: the last one is kept); `interior` families that did not spill are a group of both
    kept = [s for s, ok in zip(sizes, whole) if ok]
    served = {"interior": {0: kept, 1: list(sizes)}, "first": {0: [], 1: list(sizes)}, "last": {0: list(sizes), 1: []}}[where]
    return seqs, {"edits": edits, "served": served, "centres": centres}


# ---------------------------------------------------------------------------------------------- one centre, every edit

@functools.lru_cache(maxsize=None)
def tiled_sweep(W: int, NW: int, L: int):
    """The largest sweep of one run-less centre of L nt that the pair route admits: every kind of edit, unless a group
    would pass GROUP_CAP or the set MAX_SEQUENCES — then without the insertions (4 of the 8 edits of a position), then
    without the deletions.  Returns (sequences, kinds kept).  Kinds chosen, by this rule: all three up to 480 nt; 672 nt
    (any NW): substitutions and deletions."""
    rng = np.random.default_rng([W, NW, L, 7])
    centre = runless_sequence(rng, L)
    for kinds in (KINDS, ("sub", "del"), ("sub",)):
        seqs = single_edit_sweep(centre, kinds)
        if max(len(s) for s in seqs) > EDGES[W] or len(seqs) > MAX_SEQUENCES:
            continue
        if group_model(seqs, NW, merge=False)["largest"] <= GROUP_CAP:
            return seqs, kinds
    raise AssertionError("no sweep fits")


@functools.lru_cache(maxsize=None)
def capped_group(members: int, planted: int = 200, length: int = 150):
    """One prefix group of exactly `members` members: a shared head of 64 nt with random tails, `planted` of them with a
    neighbour (one edit behind the head, so it is a member too).  Returns (sequences, [(base, neighbour)])."""
    rng = np.random.default_rng(members)
    head = runless_sequence(rng, 64)
    seqs, seen, pairs = [], set(), []
    while len(seqs) < members - planted:
        s = head + random_sequence(rng, length - 64)
        if s not in seen:
            seen.add(s)
            seqs.append(s)
    for k in range(planted):
        base = seqs[(k * 19) % len(seqs)]
        p = 64 + (k * 7) % (length - 64)
        kind = KINDS[k % 3]
        c = LETTERS[(LETTERS.index(base[p]) + 1 + k % 3) % 4]
        s = substitute(base, p, c) if kind == "sub" else (delete(base, p) if kind == "del" else insert(base, p, c))
        assert s not in seen
        seen.add(s)
        seqs.append(s)
        pairs.append((base, s))
    return seqs, pairs


# ---------------------------------------------------------------------------------------------- the barrel shifter

def shifter_lengths(W: int, NW: int) -> list:
    """[(ws, bit shift, length)]: the lengths at which the whole-word shift of pair_stage_line, ws = (32 W - len) >> 5, is
    0, 1, 2, 3, 4, 5, 7, 8, 16 and W - 1 — as far as ws < W and the sub-family's deletion keeps 64 NW + 1 nt — each once with
    no bit shift between the words and once with one"""
    out = []
    for ws in sorted({0, 1, 2, 3, 4, 5, 7, 8, 16, W - 1}):
        if ws >= W:
            continue
        for r in (0, 5 + 2 * ws % 26):
            length = 32 * W - 32 * ws - r
            if length - 1 >= 64 * NW + 1:
                out.append((ws, r, length))
    return out


@functools.lru_cache(maxsize=None)
def mixed_lengths(W: int, NW: int):
    """One prefix group and one suffix group of width W whose members are far shorter than the record.  Prefix group: the
    longest member has 32 W nt, the others share its first 32 NW nt and have the lengths of shifter_lengths; each length is
    a sub-family of a centre, two substitutions, a deletion and an insertion outside both windows (the longest: no
    insertion), so its links are the prefix pass's and both ends of a link went through the shifter.  Suffix group: the
    same from the other end, the edits inside the first window, so the links are the suffix pass's.
    Returns (sequences, [(side, ws, bit shift, centre, neighbours)])."""
    rng = np.random.default_rng([W, NW, 11])
    w = 32 * NW
    seqs, seen, subs = [], set(), []
    for side in (0, 1):
        shared = runless_sequence(rng, w)
        for ws, r, length in shifter_lengths(W, NW):
            while True:
                body = runless_sequence(rng, length - w)
                centre = shared + body if side == 0 else body + shared
                if all(centre[k] != centre[k + 1] for k in range(length - 1)):
                    break
            lo, hi = (w, length - w) if side == 0 else (0, w)              # where the edits go
            span = hi - lo
            at = [lo + (span * k) // 5 for k in (1, 2, 3, 4)]
            nbs = [edit_variants(centre, at[0], "sub")[0], edit_variants(centre, at[1], "sub")[1], delete(centre, at[2])]
            if length + 1 <= EDGES[W]:
                nbs.append(edit_variants(centre, at[3], "ins")[0])
            for s in [centre] + nbs:
                assert s not in seen
                seen.add(s)
                seqs.append(s)
            subs.append((side, ws, r, centre, nbs))
    return seqs, subs


# ---------------------------------------------------------------------------------------------- key collisions

COLLISION_NEIGHBOURS = {"bundle": 3, "big": 49, "tiled": 149}      # per colliding sequence: merged groups of 8, 100 and 300


@functools.lru_cache(maxsize=None)
def collision_sets(W: int, NW: int, kind: str = "bundle"):
    """Two pairs of sequences that a 29-bit key puts in one group although their windows differ.
    Suffix side: windows A != B with one suffix key; P = X + mid + A and Q = X' + mid + B, X' = X with one deletion inside the
    first window.  The lengths are one apart, the first windows differ and everything above the last window agrees: without
    `ok = tail == 0` the chains of PASS 1 call P and Q neighbours.
    Prefix side: A + mid + Y and B + mid + Y', Y' = Y with one insertion outside the last window: without `same` PASS 0 does.
    Each of the four has COLLISION_NEIGHBOURS[kind] true neighbours that keep its window, so the merged group has links to
    find and lands in a bundle list (8 members), the 65..256 list (100) or the tiled list (300).
    Returns (sequences, {"suffix" | "prefix": {"windows", "pair", "neighbours": [(sequence, neighbour)]}})."""
    rng = np.random.default_rng([W, NW, len(kind)])
    w = 32 * NW
    n = EDGES[W] - 3                                          # the shorter of a pair; neighbours reach n + 3 at most
    per = COLLISION_NEIGHBOURS[kind]
    seqs, seen, info = [], set(), {}
    for side, which in (("suffix", 1), ("prefix", 0)):
        A, B = find_collision(NW, which, rng)
        rest = runless_sequence(rng, n + 1 - w)
        if which == 1:
            P = rest + A
            Q = delete(rest, w // 2) + B
            lo, hi = 0, n + 1 - w                             # neighbours: edits outside the last window
        else:
            P = A + rest
            Q = B + insert(rest, (n + 1 - w) // 3, [c for c in LETTERS if c not in rest[(n + 1 - w) // 3 - 1:(n + 1 - w) // 3 + 1]][0])
            lo, hi = w, n + 1                                 # edits outside the first window
        pair = (P, Q)
        nbs = []
        for s in pair:
            seen.add(s)
            seqs.append(s)
        for s in pair:
            span = min(hi, len(s) - (w if which == 1 else 0)) - lo
            made = 0
            for k in range(8 * per):
                if made == per:
                    break
                p = lo + (k * 37) % span
                kd = KINDS[k % 3]
                c = LETTERS[(LETTERS.index(s[p]) + 1 + (k // 3) % 3) % 4]
                t = substitute(s, p, c) if kd == "sub" else (delete(s, p) if kd == "del" else insert(s, p, c))
                keeps = t[-w:] == s[-w:] if which == 1 else t[:w] == s[:w]
                if keeps and t not in seen:
                    seen.add(t)
                    seqs.append(t)
                    nbs.append((s, t))
                    made += 1
            assert made == per
        info[side] = {"windows": (A, B), "pair": pair, "neighbours": nbs}
    return seqs, info


def chains_without_windows(a: str, b: str, W: int, NW: int, PASS: int) -> bool:
    """What pair_near<PASS, W, NW> answers when its window dwords are not looked at: lcp over the forward dwords its chain
    covers, lcs over the end-aligned ones, a dword the chain leaves out counted as equal; then the rule
    (equal lengths: lcp + lcs = n - 1; one apart: lcp + lcs >= n, both capped at n) and nothing else."""
    def dwords(s):
        v = 0
        for i, ch in enumerate(s):
            v |= LETTERS.index(ch) << (2 * i)
        t = (v << (2 * (32 * W - len(s)))) & ((1 << (64 * W)) - 1)
        cut = lambda x: [(x >> (32 * k)) & 0xFFFFFFFF for k in range(2 * W)]
        return cut(v), cut(t)
    wa, ta = dwords(a)
    wb, tb = dwords(b)
    fwd = range(2 * NW, 2 * W) if PASS == 0 else range(0, 2 * NW)
    bwd = range(2 * NW, 2 * W) if PASS == 0 else range(0, 2 * W - 2 * NW)
    f = min([32 * k + ((wa[k] ^ wb[k]) & -(wa[k] ^ wb[k])).bit_length() - 1 for k in fwd if wa[k] != wb[k]], default=1 << 32)
    l = min([32 * (2 * W - 1 - k) + 32 - (ta[k] ^ tb[k]).bit_length() for k in bwd if ta[k] != tb[k]], default=1 << 32)
    n = min(len(a), len(b))
    apart = max(len(a), len(b)) - n
    total = min(f >> 1, n) + min(l >> 1, n)
    return total + 1 == n if apart == 0 else (apart == 1 and total >= n)


# ---------------------------------------------------------------------------------------------- window mode

@functools.lru_cache(maxsize=None)
def flanked(W: int, L: int, n: int = 4300, flank: int = 40):
    """n sequences of about L nt that all share their first and their last `flank` nucleotides, in families (a centre and
    single edits between the flanks) of 2 .. 400 members: under windows of 32 nt at the ends everybody is in one group of
    each index, which moves the windows inwards (window mode)."""
    rng = np.random.default_rng([W, L, n, flank])
    head, tail = runless_sequence(rng, flank), runless_sequence(rng, flank)
    sizes = (400, 2, 300, 3, 130, 5, 70, 9, 40, 17, 33, 4, 65, 8, 257, 16)
    seqs, seen = [], set()
    f = big = 0
    while len(seqs) < n:
        centre = head + runless_sequence(rng, L - 2 * flank) + tail
        if centre in seen or len(centre) + 1 > EDGES[W]:
            continue
        want = min(sizes[f % len(sizes)], n - len(seqs))
        f += 1
        fam = [centre]
        seen.add(centre)
        # (a family that is to be one group of the tiled kind keeps its edits out of one of the moved windows: 32 nt further in)
        lo, hi = (flank, L - flank) if want < 257 else ((64, L - flank) if big % 2 else (flank, L - 64))
        big += want >= 257
        pool = [(turn, p, k) for turn in range(3) for p in range(lo, hi) for k in KINDS]
        for j in rng.permutation(len(pool)):
            if len(fam) == want:
                break
            turn, p, k = pool[j]
            v = edit_variants(centre, p, k)
            if turn < len(v) and v[turn] not in seen:
                seen.add(v[turn])
                fam.append(v[turn])
        seqs += fam
    return seqs
