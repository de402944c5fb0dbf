"""Inputs for the tests of the --fastidious pass (swarm_amd/csrc/d1_fast.inc, seam B2) across its kernel forms.  Not
product code.

`edit_atlas(L, seed)` builds, not draws, what lies around a few heavy centroids.  The longest record is exactly L nt:
the centroids are L, L - 1 and L - 2 nt long and an edit that would pass L is left out, so the centroid of L nt gets
substitutions and deletions, the one of L - 1 also single insertions (the one at the end included) and the one of
L - 2 every edit.  Around each centroid (abundance >= 3: heavy at boundary 3)

  s  every single edit (substitution, deletion, insertion) at the positions where the kernels change behaviour: 0, 1,
     30-33, 38-42, 62-65, 70-73, 79-81, every multiple of 32 and its two neighbours, Lc - 34 .. Lc - 31, Lc - 2, Lc - 1
     and Lc (the insertion at the end).  Abundance 1: the centroid's swarm takes them, they are HEAVY amplicons one
     nucleotide shorter or longer than their centroid;
  p  pairs of edits, one sequence per pair of positions: first 32 x last 32 with an insertion or deletion first (only
     the middle-window groups find those: the light amplicon's window sits at 41 or 39), both in the first 32, both in
     the last 32, two insertions, two deletions, and a sample of the rest.  Abundance 2: more than the single edits
     next to them, so no swarm takes them and each is a LIGHT swarm of mass 2, one edit from heavy amplicons (the
     single edits) and two from the centroid;
  t  three edits at positions no single edit uses: light, and no heavy amplicon within two edits: must not graft;
  d  distractors that share the first, the last or the middle 32 nt with the centroid and nothing else: light, in the
     centroid's groups, far away.

One more centroid is made of long homopolymer runs and one has period 2 (edits inside a run or a repeat coincide: what
is left after deduplication has many alignments).  `with_outlier` adds one unrelated sequence that sorts last."""
from __future__ import annotations

import numpy as np

NO_GRAFT = 0xFFFFFFFF
OUTLIER = "zz_outlier_1"


def _rand(rng, length: int) -> str:
    return "".join("ACGT"[v] for v in rng.integers(0, 4, length))


def _other(base: str, step: int) -> str:
    return "ACGT"[("ACGT".index(base) + 1 + step % 3) % 4]


def atlas_positions(lc: int, limit: int | None = None) -> list:
    """the positions of the module's docstring for a centroid of lc nt (lc itself: the insertion at the end); with a
    limit, the multiples of 32 in the middle are thinned, the fixed positions and the last three words stay"""
    fixed = {0, 1, *range(30, 34), *range(38, 43), *range(62, 66), *range(70, 74), *range(79, 82),
             *range(lc - 34, lc - 30), lc - 2, lc - 1, lc}
    words = [m + o for m in range(32, lc + 1, 32) for o in (-1, 0, 1)]
    tail = {p for p in words if p >= lc - 96}
    middle = sorted(set(words) - tail - fixed)
    keep = fixed | tail
    if limit is not None and len(keep) + len(middle) > limit:
        room = max(limit - len(keep), 0)
        middle = [middle[(i * len(middle)) // room] for i in range(room)] if room else []
    return sorted(p for p in keep | set(middle) if 0 <= p <= lc)


def apply_edits(s: str, edits) -> str:
    """edits [(kind, position of s, base)], kind 's' / 'd' / 'i' (insertion BEFORE the position), distinct positions"""
    for kind, p, b in sorted(edits, key=lambda e: -e[1]):
        s = s[:p] + b + s[p + 1:] if kind == "s" else (s[:p] + s[p + 1:] if kind == "d" else s[:p] + b + s[p:])
    return s


def _single_edits(cent: str, p: int, bases: int) -> list:
    lc = len(cent)
    out = []
    if p < lc:
        out += [("s", p, _other(cent[p], k)) for k in range(min(bases, 3))]
        out.append(("d", p, ""))
    out += [("i", p, "ACGT"[(k + p) % 4]) for k in range(bases)]
    return out


def _low_centroid(rng, length: int, periodic: bool) -> str:
    if periodic:
        return ("AC" if rng.integers(0, 2) else "GT") * (length // 2) + "A" * (length % 2)
    s = ""
    while len(s) < length:
        s += "ACGT"[int(rng.integers(0, 4))] * int(rng.integers(3, 12))
    return s[:length]


def edit_atlas(L: int, seed: int, small: bool = False) -> tuple:
    """(records [(header, sequence)], three [headers of the three-edit sequences]).  small: thinned positions and one base
    per substitution / insertion — several hundred records whatever L is."""
    rng = np.random.default_rng(seed)
    recs, three, seen = [], [], set()

    def add(header: str, s: str) -> bool:
        if s in seen or len(s) > L or len(s) < 34:
            return False
        seen.add(s)
        recs.append((header, s))
        return True

    plan = [(L, "r"), (L - 1, "r"), (L - 2, "r"), (L - 2, "h"), (L - 2, "p")]
    limit = 14 if small else 60
    bases = 1 if small else 4
    for c, (lc, kind) in enumerate(plan):
        cent = _rand(rng, lc) if kind == "r" else _low_centroid(rng, lc, kind == "p")
        if not add(f"c{c}_{100 - c}", cent):
            continue
        pos = atlas_positions(lc, limit)
        for p in pos:
            for e in _single_edits(cent, p, bases if kind == "r" else 2):
                add(f"c{c}s{e[0]}{p}{e[2]}_1", apply_edits(cent, [e]))
        first = [p for p in pos if p < 32]
        last = [p for p in pos if lc - 32 <= p < lc]
        used = set()

        def pair(e1, e2, tag):
            key = (min(e1[1], e2[1]), max(e1[1], e2[1]))
            if key in used or key[1] - key[0] < 2:
                return
            if add(f"c{c}p{tag}{e1[0]}{e1[1]}{e2[0]}{e2[1]}_2", apply_edits(cent, [e1, e2])):
                used.add(key)

        def edit(kind_, p, k):
            p = min(p, lc - 1) if kind_ != "i" else p
            return (kind_, p, "" if kind_ == "d" else (_other(cent[p], k) if kind_ == "s" else "ACGT"[(k + p) % 4]))

        # two insertions and two deletions first: they are what only the shortest centroid has room for
        spread = [pos[(i * len(pos)) // 6] for i in range(6)] + [lc - 1]
        for i, p1 in enumerate(spread[:-1]):
            pair(edit("i", p1, i), edit("i", spread[i + 1] + (1 if i == 5 else 0), i + 1), "ii")
        for i, p1 in enumerate(pos[1:-1:max(len(pos) // 6, 1)]):
            pair(edit("d", p1, i), edit("d", pos[(pos.index(p1) + 3) % len(pos)], i), "dd")
        pair(edit("d", 0, 0), edit("d", lc - 1, 0), "dd")
        pair(edit("i", 0, 0), edit("i", lc, 1), "ii")
        for i, p1 in enumerate(first):                            # first 32 x last 32, an indel first
            for j, k1 in enumerate("id"):
                p2 = last[(2 * i + j) % len(last)]
                pair(edit(k1, p1, i), edit("sdi"[(i + j) % 3], p2, i + j), "fl")
        for i in range(len(first) - 1):                           # both in the first 32, both in the last 32
            pair(edit("sdi"[i % 3], first[i], i), edit("ids"[i % 3], first[(i + 2) % len(first)], i + 1), "ff")
        for i in range(len(last) - 1):
            pair(edit("dis"[i % 3], last[i], i), edit("sid"[i % 3], last[(i + 2) % len(last)], i + 1), "ll")
        for i in range(12 if small else 60):                      # a sample of the rest
            p1, p2 = (int(v) for v in rng.choice(pos, 2, replace=False))
            pair(edit("sdi"[int(rng.integers(0, 3))], p1, i), edit("sdi"[int(rng.integers(0, 3))], p2, i + 1), "xx")
        if kind != "r":
            continue
        # three edits, none of them at or next to a position of the atlas (so no single edit is two edits away)
        taken = {q for p in pos for q in (p - 1, p, p + 1)}
        # ... and only where the three nucleotides around differ, with the fourth base inserted: no edit there can be
        # had by another one somewhere else
        free = [p for p in range(3, lc - 3) if p not in taken and len({cent[p - 1], cent[p], cent[p + 1]}) == 3]
        for i in range(4):
            ps = free[i::4][:3]
            kinds = ["sss", "sdi", "dsi", "ssd"][i]
            fourth = lambda p: next(b for b in "ACGT" if b not in cent[p - 1:p + 2])
            h = f"c{c}t{i}_1"
            if add(h, apply_edits(cent, [(k, p, "" if k == "d" else fourth(p)) for k, p in zip(kinds, ps)])):
                three.append(h)
        for i, (lo, hi) in enumerate([(0, 32), (lc - 32, lc), (40, 72)]):
            body = list(_rand(rng, lc + i - 1))
            body[lo:lo + 32] = cent[lo:hi]
            if i == 1:
                body[-32:] = cent[lo:hi]
            add(f"c{c}d{i}_1", "".join(body))
    assert max(len(s) for _, s in recs) == L
    return recs, three


def with_outlier(records: list, length: int, seed: int = 1) -> list:
    """the same records and one unrelated sequence of `length` nt whose header sorts behind every other: it moves the
    longest sequence of the database, and with it every kernel choice, and no amplicon's id"""
    rng = np.random.default_rng(1000 + seed)
    return list(records) + [(OUTLIER, _rand(rng, length))]


def write_fasta(path, recs) -> None:
    path.write_text("".join(f">{h}\n{s}\n" for h, s in recs))


def expected_plan(longest: int, bloom: bool = False, words: bool = False) -> list:
    """swa_d1_fastidious_plan restated from the kernels' limits, not from the library's code: the register kernels hold
    32 W nucleotides (the count kernel also a microvariant one longer), k_fast_count needs the Zobrist table of
    longest + 2 positions, two copies of the sequence (words + 3) and a set of >= 1.5 (7 longest + 4) slots (a power of
    two, at least 1024) per wave in 160 KB; the Bloom route keeps the Zobrist table in LDS up to 96 KB."""
    variants = 7 * longest + 4
    slots = 1024
    while slots < variants + variants // 2:
        slots *= 2
    words_of = (longest + 31) // 32
    lds = lambda waves: 8 * (4 * (longest + 2) + waves * (2 * (words_of + 3) + slots))
    waves = next((w for w in (4, 2, 1) if lds(w) <= 160 * 1024), 0)
    zobrist_lds = int(32 * (longest + 2) <= 96 * 1024)
    if bloom or longest < 112 or waves == 0:
        return [0, 0, 0, 0, 0, 0, zobrist_lds, 112]
    pair = 0 if words else next((w for w in (5, 8, 13) if longest <= 32 * w), 0)
    count = next((w for w in (5, 8) if longest + 1 <= 32 * w), 0)
    if count:
        return [1, pair, count, 0, 0, 0, zobrist_lds, 112]
    return [1, pair, 0, waves, slots, lds(waves), zobrist_lds, 112]



# natural cells: the longest record of edit_atlas(L) sits on every boundary of the dispatch and next to it
NATURAL = [112, 113, 114, 158, 159, 160, 161, 255, 256, 257, 389, 390, 415, 416, 417, 779, 780, 1003, 1004, 1005, 3071]


def is_small(L: int) -> bool:
    return L >= 1003


def cluster_records(recs: list, path):
    """the records written to `path` and clustered on the host from the oracle's network: (db, light flags)"""
    import support as S
    from swarm_amd import D1Clusters, HostDb
    write_fasta(path, recs)
    db = S.db_from_fasta(path)
    off, nb, dup = S.oracle_d1_network(db)
    assert not dup
    flags, _ = D1Clusters(HostDb(path), off, nb).light_flags(3)
    return db, flags


def build_case(L: int, path, outlier: int | None = None):
    """edit_atlas(L, seed L) (+ the outlier): (db, light flags, headers of the three-edit sequences)"""
    recs, three = edit_atlas(L, L, is_small(L))
    db, flags = cluster_records(recs if outlier is None else with_outlier(recs, outlier), path)
    return db, flags, three


# ---- one group larger than the items' stride -------------------------------------------------------------------------------
SHARED_HEAVY, SHARED_LIGHT = 500, 530


def shared_ends(seed: int = 64) -> tuple:
    """(records, three, planted): SHARED_HEAVY centroids (abundance 3) and 30 of their one-edit neighbours (abundance 1:
    their centroid's swarm takes them) are the ~530 heavy amplicons, SHARED_LIGHT amplicons of abundance 2 the light
    ones, all of 118 .. 122 nt with the same first 32 and the same last 32 nucleotides and random middles: the prefix
    group and the suffix group of the pair route each hold everybody, ceil(530 / 64)^2 = 81 tiles of 64 x 64, more than
    the 64 items a group's tiles are dealt to, so the tiles 64 .. 80 are somebody's SECOND turn.  The light amplicons
    are swarms of their own (abundance 2, as edit_atlas's: more than the abundance-1 neighbours some of them are one
    edit from, so nobody takes them; mass 2 < 3) and their headers put them in the order of k.  `planted` = k -> kind,
    spread over the whole order so that their places in the member list lie in every tile row:
      one   one edit from a centroid's neighbour (and two from the centroid), edits in the middle;
      two   two edits from a centroid, both in the middle;
      head  two edits from a centroid, one of them in the first 32 nt: out of the prefix group, so the suffix group's
            tiles must find the pair;
      three three substitutions in a centroid's middle: must not graft (`three`: their headers)."""
    rng = np.random.default_rng(seed)
    head, tail = _rand(rng, 32), _rand(rng, 32)
    seen, recs, three, planted = set(), [], [], {}

    def add(header: str, s: str) -> None:
        assert s not in seen and 118 <= len(s) <= 122 and s.endswith(tail), header
        seen.add(s)
        recs.append((header, s))

    def fresh(length: int) -> str:
        return head + _rand(rng, length - 64) + tail

    # the centroids edits are planted on have 120 nt: two insertions or two deletions stay within 118 .. 122
    cents = [fresh(120 if c % 5 == 0 else 118 + int(rng.integers(0, 5))) for c in range(SHARED_HEAVY)]
    for c, s in enumerate(cents):
        add(f"h{c:04d}_3", s)

    def edit(s: str, kind: str, p: int, step: int):
        return (kind, p, "" if kind == "d" else (_other(s[p], step) if kind == "s" else "ACGT"[(step + p) % 4]))

    neighbours = {}
    for j in range(30):                                           # heavy amplicons that are no centroids
        c = 5 * (3 * j + 1)
        neighbours[c] = apply_edits(cents[c], [edit(cents[c], "sdi"[j % 3], 40 + j, j)])
        add(f"m{c:04d}_1", neighbours[c])
    ones, twos = sorted(neighbours), [5 * (3 * j + 2) for j in range(33)]
    heads, threes = [15 * j for j in range(1, 9)], [15 * j for j in range(20, 26)]
    where = {}                                                    # k -> (kind, which of its kind): every kind all over the order
    for kind, every, first, count in (("one", 17, 1, len(ones)), ("two", 16, 3, len(twos)), ("head", 64, 7, len(heads)),
                                      ("three", 85, 10, len(threes))):
        for i in range(count):
            k = every * i + first
            while k in where:
                k += 1
            where[k] = (kind, i)
    assert max(where) < SHARED_LIGHT
    for k in range(SHARED_LIGHT):
        kind, i = where.get(k, ("", 0))
        if kind == "one":                                         # one edit from the neighbour, elsewhere in the middle
            s = apply_edits(neighbours[ones[i]], [edit(neighbours[ones[i]], "sid"[i % 3], 75 + i % 8, i)])
        elif kind == "two":
            c, kk = cents[twos[i]], ["ss", "sd", "si", "dd", "ii", "di"][i % 6]
            s = apply_edits(c, [edit(c, kk[0], 36 + i % 20, i), edit(c, kk[1], 70 + i % 15, i + 1)])
        elif kind == "head":
            s = apply_edits(cents[heads[i]], [edit(cents[heads[i]], "s", 3 * i + 2, i), edit(cents[heads[i]], "s", 50 + i, i)])
        elif kind == "three":
            s = apply_edits(cents[threes[i]], [edit(cents[threes[i]], "s", q, i) for q in (38, 59, 80)])
        else:
            s = fresh(118 + int(rng.integers(0, 5)))
        header = f"x{k:04d}{kind}_2"
        add(header, s)
        if kind:
            planted[k] = kind
        if kind == "three":
            three.append(header)
    return recs, three, planted


def assert_not_trivial(db, flags, graft, three) -> None:
    """on the ORACLE's graft candidates: at least 50 light amplicons get one, at least one for every length difference
    -2 .. 2 to its heavy amplicon, and no three-edit sequence (all of them light) gets any"""
    got = np.flatnonzero(graft != NO_GRAFT)
    assert len(got) >= 50 and all(flags[x] for x in got)
    assert {int(db.seqlen[x]) - int(db.seqlen[graft[x]]) for x in got} == {-2, -1, 0, 1, 2}
    ids = {h.decode(): i for i, h in enumerate(db.headers)}
    assert len(three) >= 4
    for h in three:
        assert flags[ids[h]] and graft[ids[h]] == NO_GRAFT, h
