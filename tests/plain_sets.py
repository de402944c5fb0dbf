"""Inputs for the tests of the d = 1 plain route (swarm_amd/csrc/d1_probe.inc: enumerate_variants, k_d1_probe; fastidious.hip: k_d1_flex,
fastidious_bloom_route), in closed form.  Not product code.

enumerate_variants deals the positions 0 .. len of a sequence to the 64 lanes of a wave: lane l owns [l K, (l + 1) K),
K = ceil((len + 1) / 64), and the rules "a deletion once per run" and "an insertion only where the base differs from the
previous one" read the previous lane's last nucleotide.  Random sets put an edit on a lane boundary inside a run by
chance; the sets here put one at every position:

  star(centre)          the centre and EVERY distinct sequence one edit away (3 L substitutions, one deletion per run,
                        3 L + 4 insertions: star_size), or only the edits at `positions`;
  shell2(centre, pairs) sequences exactly two edits away, one per pair of positions and kinds, and a few three edits away;
  lane_positions(L)     where lanes and packed words change hands;
  centres(L)            a random centre, one of homopolymer runs, one of period 2 and A * L.
"""
from __future__ import annotations

import functools

import numpy as np

import fastidious_sets as FS
import support as S

NO_GRAFT = FS.NO_GRAFT
CYCLE = (1, 2, 3, 3, 2, 1, 1)                                   # abundances of a star's members: ties and both sides of >=
CENTRE_ABUNDANCE = 9
KINDS = ("random", "runs", "period2", "single")
LANE_LENGTHS = (1, 2, 3, 31, 32, 33, 62, 63, 64, 65, 126, 127, 128, 129, 191, 192)
IDENTITY_LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129)
SHELL_LENGTHS = (2, 3, 31, 32, 33, 62, 63, 64, 65, 127, 128)
PAIR_KINDS = ("ss", "sd", "si", "ds", "dd", "di", "is", "id", "ii")


def lanes_k(length: int) -> int:
    return (length + 64) // 64                                  # ceil((length + 1) / 64)


def lane_positions(length: int) -> list:
    k = lanes_k(length)
    want = {0, 1, length - 1, length}
    for step in (k, 32):
        want |= {m + o for m in range(0, length + 1, step) for o in (-1, 0, 1)}
    return sorted(p for p in want if 0 <= p <= length)


def runs_of(s: str) -> list:
    """[(first position, length)] of the homopolymer runs"""
    out, p = [], 0
    while p < len(s):
        q = p
        while q < len(s) and s[q] == s[p]:
            q += 1
        out.append((p, q - p))
        p = q
    return out


def run_spans_lane_boundary(s: str) -> bool:
    """some run holds positions m K - 1 and m K: the lane that owns m K reads its previous base from another lane"""
    k = lanes_k(len(s))
    return any(s[b - 1] == s[b] for b in range(k, len(s), k))


def _runs_centre(length: int) -> str:
    for attempt in range(64):                                   # the seed is chosen so that a run spans a lane boundary
        rng = np.random.default_rng(7000 + 64 * length + attempt)
        s, last = "", ""
        while len(s) < length:
            b = "ACGT"[int(rng.integers(0, 4))]
            if b != last:
                s += b * int(rng.integers(3, 12))
                last = b
        s = s[:length]
        if lanes_k(length) < 2 or run_spans_lane_boundary(s):
            break
    assert lanes_k(length) < 2 or run_spans_lane_boundary(s), length
    return s


def centre(kind: str, length: int) -> str:
    if kind == "random":
        return FS._rand(np.random.default_rng(5000 + length), length)
    if kind == "runs":
        return _runs_centre(length)
    if kind == "period2":
        return ("AC" * length)[:length]
    assert kind == "single"
    return "A" * length


def centres(length: int) -> dict:
    return {kind: centre(kind, length) for kind in KINDS}


def single_edits(cent: str, positions=None) -> list:
    """every (kind, position, base) at the positions (default: all, the insertion at the end included)"""
    lc = len(cent)
    out = []
    for p in (range(lc + 1) if positions is None else positions):
        if p < lc:
            out += [("s", p, b) for b in "ACGT" if b != cent[p]]
            out.append(("d", p, ""))
        out += [("i", p, b) for b in "ACGT"]
    return out


def v1(s: str) -> set:
    """the microvariants of s: every distinct sequence one edit away, the empty one left out"""
    out = {FS.apply_edits(s, [e]) for e in single_edits(s)}
    out.discard("")
    out.discard(s)
    return out


def star_size(cent: str) -> int:
    """centre + 3 L substitutions + one deletion per run + 3 L + 4 insertions (the deletion of a 1-nt centre is empty)"""
    lc = len(cent)
    return 1 + 3 * lc + (len(runs_of(cent)) if lc > 1 else 0) + 3 * lc + 4


def star(cent: str, positions=None, tag: str = "") -> list:
    """[(header, sequence)] in db order: the centre first (abundance 9), then its one-edit sequences by abundance, header"""
    seen, members = {cent, ""}, []
    for kind, p, b in single_edits(cent, positions):
        s = FS.apply_edits(cent, [(kind, p, b)])
        if s not in seen:
            seen.add(s)
            members.append((f"{tag}{kind}{p:04d}{b}_{CYCLE[len(members) % len(CYCLE)]}", s))
    members.sort(key=lambda r: (-int(r[0].rsplit("_", 1)[1]), r[0]))
    return [(f"{tag}c_{CENTRE_ABUNDANCE}", cent)] + members


def merged(records_lists) -> list:
    """several record lists as one database: the centres (first of each list) first, a sequence met again is dropped"""
    seen, out = set(), []
    lists = [list(r) for r in records_lists]
    for h, s in [r[0] for r in lists] + [x for r in lists for x in r[1:]]:
        if s not in seen:
            seen.add(s)
            out.append((h, s))
    return out


def to_db(records) -> S.Db:
    return S.build_db([(h.encode(), s.encode()) for h, s in records])


@functools.lru_cache(maxsize=None)
def star_database(length: int, kinds: tuple = KINDS):
    """(db, {kind: (centre's id, star size)}): the full stars of the centres of `length` nt in one database"""
    cents = {kind: centre(kind, length) for kind in kinds}
    recs = merged([star(c, tag=kind[0]) for kind, c in cents.items()])
    db = to_db(recs)
    ids = {db.seq_str(i): i for i in range(db.n)}
    assert len(ids) == db.n == len({s for c in cents.values() for s in v1(c) | {c}})     # nothing lost, nothing twice
    return db, {kind: (ids[c], star_size(c)) for kind, c in cents.items()}


def with_star_of(db: S.Db, member: int, tag: str = "zstar") -> tuple:
    """(db', the member's sequence): the records of db and the full star of one of them (sequences db has are not added again)"""
    have = {db.seq_str(i) for i in range(db.n)}
    cent = db.seq_str(member)
    recs = [(db.headers[i], db.seq_str(i).encode()) for i in range(db.n)]
    recs += [(h.encode(), s.encode()) for h, s in star(cent, tag=tag)[1:] if s not in have]
    return S.build_db(recs), cent


# ---- long centres: the Zobrist table in LDS (longest <= 3070) and in memory ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def long_records(longest: int) -> tuple:
    """partial stars (lane_positions) of a random and a run-built centre of longest, longest - 1 and longest - 2 nt — an
    insertion that would pass `longest` is left out — and 200 unrelated sequences of 150 nt"""
    recs = []
    for back in range(3):
        for kind in ("random", "runs"):
            cent = centre(kind, longest - back)
            recs.append([r for r in star(cent, lane_positions(len(cent)), tag=f"{kind[0]}{back}") if len(r[1]) <= longest])
    rng = np.random.default_rng(longest)
    recs.append([(f"u{i:03d}_{1 + i % 4}", FS._rand(rng, 150)) for i in range(200)])
    out = merged(recs)
    assert max(len(s) for _, s in out) == longest
    return tuple(out)


# ---- shells: what lies two edits from a heavy centre ---------------------------------------------------------------------------

def position_pairs(length: int, limit: int = 150) -> list:
    """[(p1, p2, kinds)]: both edits on one lane, on neighbouring lanes (either side of every lane boundary), insertion +
    deletion and deletion + insertion (the light amplicon has the heavy's length), and lane_positions x lane_positions thinned"""
    k = lanes_k(length)
    out = []
    for b in range(k, length, k):
        out.append((b - 1, b, PAIR_KINDS[len(out) % 9]))          # neighbouring lanes
        if k >= 2 and b + 1 < length:
            out.append((b, b + 1, PAIR_KINDS[len(out) % 9]))      # one lane
    if length > 64:                                               # K = 1 has a lane a position: thin what is every pair of neighbours
        out = out[::max(len(out) // 40, 1)]
    lp = lane_positions(length)
    cross = [(p, q) for p in lp for q in lp if p < q]
    cross = cross[::max(len(cross) // limit, 1)]
    out += [(p, q, PAIR_KINDS[i % 9]) for i, (p, q) in enumerate(cross)]
    out += [(p, q, ("id", "di")[i % 2]) for i, (p, q) in enumerate(cross[::5])]
    return out


def one_edit_or_none(cent: str, s: str) -> bool:
    """s is the centre or one edit from it (cheap for long centres: common prefix + common suffix)"""
    if abs(len(cent) - len(s)) > 1:
        return False
    n = min(len(cent), len(s))
    lcp = next((i for i in range(n) if cent[i] != s[i]), n)
    lcs = next((i for i in range(n - lcp) if cent[-1 - i] != s[-1 - i]), n - lcp)
    return lcp + lcs >= max(len(cent), len(s)) - 1


def shell2(cent: str, pairs, tag: str = "", longest: int | None = None, avoid=()) -> tuple:
    """(two [(header, sequence)], three [(header, sequence)]): one sequence per (p1, p2, kinds) that is exactly two edits
    from the centre and no longer than `longest` (a pair of edits that undo each other or add up to one edit is left out), and up to four sequences
    three edits away, made as fastidious_sets.edit_atlas makes them: only where the three nucleotides around differ, the
    fourth base put in"""
    lc = len(cent)
    two, three, seen = [], [], {cent, ""}
    for p1, p2, kinds in pairs:
        edits = []
        for kind, p in zip(kinds, (p1, p2)):
            if kind != "i" and p >= lc:
                break
            b = "" if kind == "d" else (FS._other(cent[p], p1 + p2) if kind == "s" else "ACGT"[(p1 + p2 + p) % 4])
            edits.append((kind, p, b))
        if len(edits) < 2 or p1 == p2:
            continue
        s = FS.apply_edits(cent, edits)
        if s in seen or (longest is not None and len(s) > longest) or one_edit_or_none(cent, s):
            continue
        seen.add(s)
        two.append((f"{tag}p{kinds}{p1:04d}x{p2:04d}_2", s))
    taken = {q for p in avoid for q in (p - 1, p, p + 1)}       # (where single-edit heavy amplicons have their edit)
    free = [p for p in range(3, lc - 3) if p not in taken and len({cent[p - 1], cent[p], cent[p + 1]}) == 3]
    for i in range(4):
        ps = []
        for p in free[i:]:
            if len(ps) < 3 and (not ps or p - ps[-1] >= 3):
                ps.append(p)
        if len(ps) < 3:
            continue
        fourth = lambda p: next(b for b in "ACGT" if b not in cent[p - 1:p + 2])
        s = FS.apply_edits(cent, [(k, p, "" if k == "d" else fourth(p)) for k, p in zip(["sss", "sdi", "dsi", "ssd"][i], ps)])
        if s not in seen:
            seen.add(s)
            three.append((f"{tag}t{i}_1", s))
    return two, three


def _flags(db: S.Db, light_headers: set) -> np.ndarray:
    return np.array([h.decode() in light_headers for h in db.headers], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def shell_case(length: int) -> tuple:
    """(db, is_light, headers of the three-edit sequences).  Heavy: a random, a run-built and a period-2 centre of `length`
    nt and some single-edit sequences of the random one, half of them with a smaller id than it; light: the shells of the three centres."""
    heavy, light, three = [], [], []
    for c, kind in enumerate(KINDS[:3]):
        cent = centre(kind, length)
        heavy.append((f"h{c}_{90 - c}", cent))
        spots = lane_positions(length)[::11] if kind == "random" else []
        heavy += [(f"h{c}e{i:03d}_{(5, 95)[i % 2]}", FS.apply_edits(cent, [e])) for i, e in enumerate(single_edits(cent, spots)[::2])
                  if FS.apply_edits(cent, [e])]                 # (every other one sorts before its centre)
        two, far = shell2(cent, position_pairs(length), tag=f"x{c}", avoid=spots)
        light += two
        three += far
    recs = merged([heavy, light + three])
    db = to_db(recs)
    lights = {h for h, _ in light + three} & {h for h, _ in recs}
    return db, _flags(db, lights), [h for h, _ in three if h in lights]


@functools.lru_cache(maxsize=None)
def long_shell_case(longest: int) -> tuple:
    """the same around the long centres of long_records(longest).  Heavy: the six centres, some single-edit sequences of the
    random ones and the 200 unrelated sequences; light: shells of the six centres at lane_positions"""
    heavy, light, three = [], [], []
    for back in range(3):
        for kind in ("random", "runs"):
            cent = centre(kind, longest - back)
            heavy.append((f"h{kind[0]}{back}_{90 - back}", cent))
            spots = lane_positions(len(cent))[::40] if kind == "random" else []
            heavy += [(f"h{kind[0]}{back}e{i:03d}_5", FS.apply_edits(cent, [e])) for i, e in enumerate(single_edits(cent, spots))
                      if len(FS.apply_edits(cent, [e])) <= longest]
            two, far = shell2(cent, position_pairs(len(cent), 40), tag=f"x{kind[0]}{back}", longest=longest, avoid=spots)
            light += two
            three += far
    heavy += [r for r in long_records(longest) if r[0].startswith("u")]
    recs = merged([heavy, light + three])
    db = to_db(recs)
    lights = {h for h, _ in light + three} & {h for h, _ in recs}
    assert db.longest == longest
    return db, _flags(db, lights), [h for h, _ in three if h in lights]


# ---- the batch loop of the Bloom route ------------------------------------------------------------------------------------------

BATCH_LENGTH = 16


@functools.lru_cache(maxsize=None)
def batch_set() -> tuple:
    """(db, is_light, first dense heavy id, forced task cap): at most 64 amplicons, so that k_fast_band_lists lists the
    heavy ones in id order.  Ids 0, 1: heavy, nothing within two edits; then the dense heavies, a centre and every
    substitution at 8 of its positions; then light, sequences with two of those substitutions.  Nothing is longer than
    the centre, so the cap 7 longest + 4 is one heavy amplicon's worth of tasks."""
    rng = np.random.default_rng(16)
    cent = FS._rand(rng, BATCH_LENGTH)
    sparse = [(f"a{i}_{100 - i}", "GT"[i] * BATCH_LENGTH) for i in range(2)]
    spots = list(range(1, BATCH_LENGTH, 2))
    dense = [("b0_90", cent)] + [(f"b{p:02d}{b}_50", FS.apply_edits(cent, [("s", p, b)])) for p in spots for b in "ACGT" if b != cent[p]]
    others = lambda p: [b for b in "ACGT" if b != cent[p]]
    combos = [(p, bp, q, bq) for i, p in enumerate(spots) for q in spots[i + 1:] for bp in others(p) for bq in others(q)]
    light = [(f"x{i:02d}_1", FS.apply_edits(cent, [("s", p, bp), ("s", q, bq)])) for i, (p, bp, q, bq) in enumerate(combos[::7][:35])]
    recs = merged([sparse, dense, light])
    db = to_db(recs)
    assert db.n == len(sparse) + len(dense) + len(light) <= 64 and db.longest == BATCH_LENGTH
    assert "".join(h.decode()[0] for h in db.headers) == "a" * len(sparse) + "b" * len(dense) + "x" * len(light)   # db order is the layout above
    return db, _flags(db, {h for h, _ in light}), len(sparse), 7 * BATCH_LENGTH + 4
