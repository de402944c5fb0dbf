"""k_fast_count_sites_words (swarm_amd/csrc/d1_fast.inc), SWA_FAST_LONG=pairs and SWA_FAST_COUNT=sites without a GPU.

  * The kernel's arithmetic restated on Python integers as 64-bit words with a run-time word count — the staging with
    zero words behind the sequence, P and E word by word with the neighbour word of the end alignment, the positions in
    both forms, the microvariant's words on demand (swa_variant_word), the first mismatch of the forward words and the
    last mismatch of the shifted comparison, each loop ending at the word that holds its mismatch — checked against the
    brute-force |V1(h) & V1(x)| of tests/test_fastidious_identity.py.
  * The dispatch as a pure function (swa_d1_fastidious_plan_modes, host_tables.cpp) against its restatement here.
  * The sets of tests/test_fastidious_long_gpu.py on the oracle's result."""
import time

import numpy as np
import pytest

import fastidious_long_sets as LS
import fastidious_sets as FS
import fastidious_split_sets as SS
import support as S
from swarm_amd import capi
from test_fastidious_identity import v1

_M64 = (1 << 64) - 1


# ---- the kernel, word by word ------------------------------------------------------------------------------------------------
def _stage(s: str, words: int) -> list:
    """the sequence packed two bits a nucleotide, zero words behind it (`words` in all)"""
    w = [0] * words
    for p, c in enumerate(s):
        w[p >> 5] |= "ACGT".index(c) << ((p & 31) * 2)
    return w


def _nt(w, p):
    return (w[p >> 5] >> ((p & 31) * 2)) & 3


def _ctz(v):
    return (v & -v).bit_length() - 1


def _variant_word(seed, nw, kind, pos, base, w):
    """swa_variant_word (swa_internal.h): kind 0 substitution, 1 deletion, 2 insertion"""
    wp, sh = pos >> 5, (pos & 31) << 1
    cur = seed[w] if w < nw else 0
    if kind == 0:
        return cur if w != wp else (cur & ~(3 << sh) & _M64) | (base << sh)
    low = (1 << sh) - 1
    if kind == 1:
        nxt = seed[w + 1] if w + 1 < nw else 0
        shifted = ((cur >> 2) | (nxt << 62)) & _M64
        return cur if w < wp else (shifted if w > wp else (cur & low) | (shifted & ~low & _M64))
    prv = seed[w - 1] if (w >= 1 and w - 1 < nw) else 0
    shifted = ((cur << 2) | (prv >> 62)) & _M64
    return cur if w < wp else (shifted if w > wp else (cur & low) | (base << sh) | (shifted & ~(low | (3 << sh)) & _M64))


def _one_edit_from_x(swh, nwh, lh, swx, lx, kind, p, base, reads):
    lv = lh if kind == 0 else (lh - 1 if kind == 1 else lh + 1)
    dv = lv - lx
    if dv < -1 or dv > 1:
        return False
    v_longer, shifted = dv == 1, dv != 0
    nw = (max(lv, lx) + 31) >> 5
    lcp, hb = 0x7FFFFFFF, -1
    for w in range(nw):
        reads.append(w)
        d = _variant_word(swh, nwh, kind, p, base, w) ^ swx[w]
        if d:
            lcp = 32 * w + (_ctz(d) >> 1)
            break
    v_next = x_next = 0
    for w in range(nw - 1, -1, -1):
        reads.append(w)
        vw, xw = _variant_word(swh, nwh, kind, p, base, w), swx[w]
        lw, ln, sw = (vw, v_next, xw) if v_longer else (xw, x_next, vw)
        d = sw ^ ((((lw >> 2) | (ln << 62)) & _M64) if shifted else lw)
        if d:
            hb = 32 * w + ((d.bit_length() - 1) >> 1)
            break
        v_next, x_next = vw, xw
    return hb < lcp if shifted else hb == lcp


def sites_words_count(h: str, x: str, maxwords: int | None = None) -> int:
    """what a wave of k_fast_count_sites_words adds for the pair (h, x)"""
    lh, lx = len(h), len(x)
    nwh, nwx = (lh + 31) >> 5, (lx + 31) >> 5
    nmax = max(nwh, nwx)
    maxwords = nmax if maxwords is None else maxwords
    assert nmax <= maxwords
    # the kernel writes nmax + 3 <= maxwords + 3 words of each copy; what lies behind is the previous pair's: poisoned here
    swx = _stage(x, nmax + 3) + [_M64] * (maxwords - nmax)
    swh = _stage(h, nmax + 3) + [_M64] * (maxwords - nmax)
    dl = lx - lh
    assert -2 <= dl <= 2
    P, E = min(lh, lx), -1
    for i in range(nmax):
        hv, xv = swh[i], swx[i]
        d0 = hv ^ xv
        if d0:
            P = min(P, 32 * i + (_ctz(d0) >> 1))
        lo, hi = (swx[i - 1] if i > 0 else 0), swx[i + 1]
        xs = xv
        if dl == 1:
            xs = ((xv >> 2) | (hi << 62)) & _M64
        elif dl == 2:
            xs = ((xv >> 4) | (hi << 60)) & _M64
        elif dl == -1:
            xs = ((xv << 2) | (lo >> 62)) & _M64
        elif dl == -2:
            xs = ((xv << 4) | (lo >> 60)) & _M64
        d = hv ^ xs
        if i == 0 and dl < 0:
            d |= 3 if dl == -1 else 15
        if d:
            E = max(E, 32 * i + ((d.bit_length() - 1) >> 1))
    P = min(P, lh - 1)
    E = min(max(E, 0), lh - 1)
    first, last = min(P, E), max(P, E)

    def runstart(q):
        while q > 0 and _nt(swh, q - 1) == _nt(swh, q):
            q -= 1
        return q

    lo_pos, hi_pos = max(runstart(max(first - 1, 0)) - 1, 0), min(last + 1, lh)
    lo_b, hi_a = max(runstart(max(last - 1, 0)) - 1, 0), min(first + 1, lh)
    two = P <= E and lo_b > hi_a
    n_a = (hi_a if two else hi_pos) - lo_pos + 1
    slots = (n_a + (hi_pos - lo_b + 1 if two else 0)) * 8
    found = 0
    reads = []
    for t in range(slots):
        at, slot = t >> 3, t & 7
        p = lo_pos + at if at < n_a else lo_b + (at - n_a)
        prevc = _nt(swh, p - 1) if p >= 1 else 4
        c = _nt(swh, p) if p < lh else 4
        if slot < 4:
            kind, base, ok = 2, slot, (p == 0 or slot != prevc)
        elif slot < 7:
            t3 = slot - 4
            kind, base, ok = 0, (t3 if t3 < c else t3 + 1), p < lh
        else:
            kind, base, ok = 1, 0, p < lh and (p == 0 or c != prevc)
        if ok and _one_edit_from_x(swh, nwh, lh, swx, lx, kind, p, base, reads):
            found += 1
    assert all(w < nmax + 3 for w in reads)
    return found


_v1_memo = {}


def _brute(h: str, x: str) -> int:
    if h not in _v1_memo:
        if len(_v1_memo) > 8:
            _v1_memo.clear()
        _v1_memo[h] = v1(h)
    return len(_v1_memo[h] & v1(x))


def _make(rng, kind: int, L: int) -> str:
    if kind == 0:
        return "".join(rng.choice(list("ACGT"), L))
    if kind == 1:
        return "".join(rng.choice(list("AC"), L))
    if kind == 2:
        unit = "".join(rng.choice(list("ACGT"), int(rng.integers(1, 5))))
        return (unit * L)[:L]
    s = "".join(rng.choice(list("ACGT"), L))                     # random, ending in A's ('A' is 00: looks like padding)
    return s[:L - 5] + "AAAAA"


def _edit(rng, s: str, kind: str, p: int, alpha: str = "ACGT") -> str:
    p = min(p, len(s) - (0 if kind == "i" else 1))
    if kind == "s":
        b = str(rng.choice([c for c in alpha if c != s[p]] or ["G"]))
        return s[:p] + b + s[p + 1:]
    if kind == "d":
        return s[:p] + s[p + 1:]
    return s[:p] + str(rng.choice(list(alpha))) + s[p:]


COMBOS = ["", "s", "d", "i", "ss", "dd", "ii", "di", "sd", "si", "id", "sss", "sdi", "dds", "iis", "dis"]
LENGTHS = [31, 32, 33, 34, 63, 64, 65, 66, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 2050]


def _positions(rng, L: int, j: int) -> list:
    """three positions for the edits of case j: the first and the last position, the word boundaries, anywhere"""
    edge = [0, L - 1, L, 31, 32, 33, (L - 1) & ~31, ((L - 1) & ~31) - 1, L - 2, 1]
    anywhere = [int(v) for v in rng.integers(0, L + 1, 3)]
    pick = [edge[j % len(edge)], anywhere[0] if j % 3 else edge[(j + 1) % len(edge)], anywhere[1]]
    return [max(0, min(p, L)) for p in pick]


def test_word_model_counts_the_common_microvariants_across_word_boundaries():
    """lengths on both sides of 32, 64, 1024 and 2048; every length difference -2 .. 2; zero to three edits; random,
    two-letter and periodic sequences and sequences ending in A's; an edit at position 0 and at the last position"""
    rng = np.random.default_rng(41)
    seen_dl, seen_edits, nonzero = set(), set(), 0
    for li, L in enumerate(LENGTHS):
        for j, combo in enumerate(COMBOS):
            if combo == "" and L > 66 and L != 1025:
                continue                                          # (x = h expands every position of h: once at a long length)
            kind = (li + j) % 4
            h = _make(rng, kind, L)
            alpha = "AC" if kind == 1 else "ACGT"
            x = h
            for k, p in sorted(zip(combo, _positions(rng, L, j)), key=lambda e: -e[1]):
                x = _edit(rng, x, k, p, alpha)
            if abs(len(x) - L) > 2:
                continue
            want = _brute(h, x)
            got = sites_words_count(h, x, maxwords=max(len(h), len(x)) // 32 + 4)
            assert got == want, (L, combo, kind, want, got)
            seen_dl.add((L > 66, len(x) - L))
            seen_edits.add(len(combo))
            nonzero += want > 0
    assert seen_dl == {(long, d) for long in (False, True) for d in range(-2, 3)}
    assert seen_edits == {0, 1, 2, 3} and nonzero > 120


def test_word_model_on_many_short_pairs():
    """the same model on thousands of pairs of 28 .. 70 nt (words of 32 nt: one to three words), all alphabets, edits anywhere"""
    rng = np.random.default_rng(43)
    checked = 0
    for t in range(4000):
        L = int(rng.integers(28, 71))
        kind = t % 4
        h = _make(rng, kind, L)
        alpha = "AC" if kind == 1 else ("AAAC" if t % 8 == 2 else "ACGT")
        x = h
        for _ in range(int(rng.integers(1, 4))):
            x = _edit(rng, x, "sdi"[int(rng.integers(0, 3))], int(rng.integers(0, len(x) + 1)), alpha)
        if abs(len(x) - L) > 2 or x == h:
            continue
        assert sites_words_count(h, x) == _brute(h, x), (h, x)
        checked += 1
    assert checked > 3000


def test_word_model_with_runs_longer_than_a_word():
    """homopolymer runs of more than 64 nt that cross word boundaries and touch P or E: the walk back to the start of the
    run passes whole words; runs at the very start and the very end of the sequence"""
    rng = np.random.default_rng(47)
    checked = 0
    for L, run in ((200, 70), (200, 130), (230, 97), (1030, 150)):
        for start in (0, 17, 31, 33, L - run):
            base = "ACGT"[(start + run) % 4]
            left = "".join(rng.choice([c for c in "ACGT" if c != base], start))
            right = "".join(rng.choice([c for c in "ACGT" if c != base], L - start - run))
            h = left + base * run + right
            inside, end = start + run // 2, start + run - 1
            cases = [[("d", inside)], [("i", inside)], [("s", inside)], [("s", end)], [("s", start)], [("d", start), ("s", end)],
                     [("s", inside), ("s", min(end + 1, L - 1))], [("i", end + 1), ("d", max(start - 1, 0))],
                     [("s", start + 1), ("i", inside)], [("d", inside), ("d", inside + 1)]]
            for edits in cases[:(10 if L < 1000 else 5)]:
                x = h
                for k, p in sorted(edits, key=lambda e: -e[1]):
                    x = x[:p] + base + x[p:] if k == "i" else _edit(rng, x, k, p)     # the run's own base: a longer run
                if x == h:
                    continue
                assert sites_words_count(h, x) == _brute(h, x), (L, run, start, edits)
                checked += 1
    assert checked > 120


# ---- the plan ----------------------------------------------------------------------------------------------------------------
LDS = LS.LDS_BYTES
_sites_lds, _sites_waves, _sites_vector = LS.sites_lds, LS.sites_waves, LS.sites_plan


def test_sites_cap_and_wave_boundaries_restated_from_160_kb():
    words_1 = LDS // 16 - 3                                      # one wave: 16 (words + 3) <= 160 KB
    words_4 = LDS // 64 - 3
    words_2 = LDS // 32 - 3
    assert (words_1, words_2, words_4) == (10237, 5117, 2557)
    assert capi.fastidious_sites_cap() == 32 * words_1 == 327584 == LS.SITES_CAP and 32 * words_4 == 81824
    for longest, waves in ((1005, 4), (32 * words_4, 4), (32 * words_4 + 1, 2), (32 * words_2, 2), (32 * words_2 + 1, 1),
                           (32 * words_1, 1)):
        assert _sites_waves(longest) == waves
        assert capi.fastidious_plan_modes(longest, 0, long_mode=2) == _sites_vector(longest, longest), longest
    assert _sites_waves(32 * words_1 + 1) == 0
    # the hook counts within [1004, derived] only
    assert [capi.fastidious_sites_cap(n) for n in (1003, 1004, 5000, 327584, 327585)] == [327584, 1004, 5000, 327584, 327584]


def test_plan_modes_equals_plan_for_without_the_new_switches():
    for pair_longest in (0, 150, 1004):
        for longest in range(1, 4001):
            for split in (0, 1):
                assert capi.fastidious_plan_modes(longest, pair_longest, long_mode=split) == \
                    capi.fastidious_plan_for(longest, pair_longest, split=bool(split)), (longest, pair_longest, split)
            if longest % 97 == 0:
                for kw in ({"bloom": True}, {"words": True}):
                    assert capi.fastidious_plan_modes(longest, pair_longest, long_mode=1, **kw) == \
                        capi.fastidious_plan_for(longest, pair_longest, split=True, **kw)


def test_plan_under_pairs():
    cap = capi.fastidious_sites_cap()
    for pair_longest in (0, 150, 1004):
        for longest in range(1, 1005):                            # today's plan up to 1004
            assert capi.fastidious_plan_modes(longest, pair_longest, long_mode=2) == FS.expected_plan(longest), longest
        for longest in list(range(1005, 4001)) + [81824, 81825, 163744, 163745, cap]:
            assert capi.fastidious_plan_modes(longest, pair_longest, long_mode=2) == _sites_vector(longest, longest), longest
            assert capi.fastidious_plan_modes(longest, pair_longest, long_mode=2, bloom=True) == FS.expected_plan(longest, bloom=True)
    # above the cap, derived and overridden: the Bloom plan where no sequence is left for the pair route, else the
    # division at the cap with the staged-words kernel for the pairs that stay
    for longest, hook, C in ((cap + 1, 0, cap), (400000, 0, cap), (1005, 1004, 1004), (3071, 1004, 1004), (2049, 2000, 2000)):
        assert capi.fastidious_plan_modes(longest, 0, long_mode=2, sites_cap=hook) == FS.expected_plan(longest)
        assert capi.fastidious_plan_modes(longest, 111, long_mode=2, sites_cap=hook) == FS.expected_plan(longest)
        for served in (112, 150, 1004, C):
            assert capi.fastidious_plan_modes(longest, served, long_mode=2, sites_cap=hook) == _sites_vector(served, longest)
        assert capi.fastidious_plan_modes(longest, served, long_mode=2, sites_cap=hook, bloom=True) == FS.expected_plan(longest, bloom=True)
    # a hook outside [1004, derived] is ignored
    assert capi.fastidious_plan_modes(2049, 0, long_mode=2, sites_cap=1003) == _sites_vector(2049, 2049)
    assert capi.fastidious_plan_modes(2049, 0, long_mode=2, sites_cap=cap + 1) == _sites_vector(2049, 2049)


def test_plan_under_count_sites():
    for longest in range(1, 4001):
        today = FS.expected_plan(longest)
        got = capi.fastidious_plan_modes(longest, 0, count_sites=True)
        if today[0] == 1 and today[2] == 0:
            assert 256 <= longest <= 1004
            assert got == _sites_vector(longest, longest, pair_w=today[1]), longest
        else:
            assert got == today, longest
        assert capi.fastidious_plan_modes(longest, 0, count_sites=True, bloom=True) == FS.expected_plan(longest, bloom=True)
    # with the split: the row of pair_longest
    assert capi.fastidious_plan_modes(1500, 150, long_mode=1, count_sites=True) == capi.fastidious_plan_for(1500, 150, split=True)
    assert capi.fastidious_plan_modes(1500, 1004, long_mode=1, count_sites=True) == _sites_vector(1004, 1500)
    assert capi.fastidious_plan_modes(1500, 300, long_mode=1, count_sites=True) == _sites_vector(300, 1500)


# ---- the sets are worth running ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", LS.LONG_ATLASES)
def test_long_sets_have_pairs_on_every_side(tmp_path, L):
    db, flags, three = SS.build(str(L), tmp_path / "in.fa")
    assert db.longest == L and 300 <= db.n <= 3000
    t0 = time.perf_counter()
    graft, counters = S.oracle_fastidious(db, flags, 16)
    took = time.perf_counter() - t0
    print(f"edit_atlas({L}): n {db.n}, oracle {took:.2f} s, grafts {int((graft != FS.NO_GRAFT).sum())}")
    assert took < 10.0                                            # (measured: 0.6 s for the 1005 and 1025 sets, 2.0 s for the 2049 set)
    FS.assert_not_trivial(db, flags, graft, three)
    pairs = SS.graft_pair_lengths(db, graft)
    assert sum(1 for a, b in pairs if min(a, b) > SS.CAP) >= (5 if L == 1005 else 50)   # (1005: only the longest length is past the cap)
    edge = {1005: SS.CAP, 1025: 1024, 2049: 2048}[L]
    assert any(a <= edge < b for a, b in pairs) and any(b <= edge < a for a, b in pairs)
    if L > 1005:
        assert any(max(a, b) <= edge for a, b in pairs)         # and pairs wholly below the word boundary
