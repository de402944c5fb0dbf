"""What the d >= 2 graph route rests on at 9 <= d <= 16, checked on the host (no GPU): the window identity — a pair within
d edits shares one of d + 1 disjoint windows of the query, shifted by at most d in the target — and the count B of the
brute-force candidates from a histogram of 288 lengths (16 * 17 + 16: what a short sequence can pair with at d = 16)."""
import itertools

import numpy as np
import pytest

import dn_deep_sets as DS
import dn_short_sets as D


def _apply(s: str, script) -> str:
    """script: [(kind, position, base)] applied one after the other"""
    for kind, p, b in script:
        if kind == "s":
            s = s[:p] + b + s[p + 1:]
        elif kind == "d":
            s = s[:p] + s[p + 1:]
        else:
            s = s[:p] + b + s[p:]
    return s


@pytest.mark.parametrize("d,wlen,extra", [(1, 2, 2), (2, 2, 1), (2, 1, 2), (3, 1, 0)])
def test_window_identity_for_every_placement_on_toy_strings(d, wlen, extra):
    """every script of up to d edits (substitution, deletion, insertion at every place, every base of a two-letter
    alphabet) on a query of wlen (d + 1) + extra letters"""
    length = wlen * (d + 1) + extra
    rng = np.random.default_rng(d * 10 + wlen)
    checked = 0
    for _ in range(3):
        query = "".join(rng.choice(list("AC"), size=length))
        steps = [(k, p, b) for k in "sdi" for p in range(length + d + 1) for b in "AC"]
        for r in range(d + 1):
            for script in itertools.product(steps, repeat=r):
                t = query
                ok = True
                for kind, p, b in script:
                    if p > len(t) or (kind != "i" and p >= len(t)):
                        ok = False
                        break
                    t = _apply(t, [(kind, p, b)])
                if ok and len(t) >= 1:
                    assert DS.first_shared_window(query, t, d, wlen) is not None, (query, script, t)
                    checked += 1
    assert checked > 100


@pytest.mark.parametrize("d", list(range(9, 17)))
def test_window_identity_at_length_300(d):
    """random pairs d edits apart (and fewer), 16-nt windows: 16 (d + 1) <= 288 <= 300 for every d <= 16.  The shared
    window's shift is within -d .. +d, and both ends of that range are reached."""
    rng = np.random.default_rng(1600 + d)
    wlen = 16
    shifts = set()
    for trial in range(300):
        q = "".join(rng.choice(list("ACGT"), size=300))
        t = q
        for _ in range(d if trial % 3 else int(rng.integers(0, d + 1))):
            t = D.edit(rng, t)
        found = DS.first_shared_window(q, t, d, wlen)
        assert found is not None, (q, t)
        assert all(-d <= s <= d for s in found[1])
    # the built variants: the window they were built for is where they say
    for wl in (16, 32):
        cent = "".join(rng.choice(list("ACGT"), size=DS.centre_length(d, wl)))
        for kind, k, s in DS.variants(rng, cent, d, wl):
            if kind == "far":
                continue
            want = DS.wanted_shift(kind, k, d)
            assert DS.window_at(cent, s, k, want, wl), (kind, k)
            shifts.add(want)
            assert DS.first_shared_window(cent, s, d, wl)[0] <= k
    assert {0, d, -d, 1, -1} <= shifts


@pytest.mark.parametrize("d", [9, 12, 16])
def test_candidate_count_from_the_histogram_equals_the_direct_count(d):
    """B as window_length() computes it from the count of sequences per length (dn_short_sets.brute_candidates restates it)
    against the pairs counted one by one, with lengths up to 288 and beyond"""
    rng = np.random.default_rng(d)
    T = D.short_below(d)
    assert T + d <= 288
    for trial in range(4):
        hi = (T + d, 289, 400, T)[trial]
        lens = rng.integers(max(1, T - 40), hi, size=300)
        direct = sum(1 for i in range(len(lens)) for j in range(i + 1, len(lens))
                     if min(lens[i], lens[j]) < T and abs(int(lens[i]) - int(lens[j])) <= d)
        assert D.brute_candidates(lens, d) == direct
        assert direct > 0
