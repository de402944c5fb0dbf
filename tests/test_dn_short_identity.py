"""The identity the d >= 2 graph route's split rests on (dn_graph.hip), checked on the host with the oracle's nw()
(orc_nw_diff) as the truth.  A sequence is short when it has fewer than 16 (d + 1) nucleotides.  Every pair within d
differences is either a pair of two long sequences (the window groups find it) or has a short member and a length
difference of at most d (k_dg_brute compares exactly those); and B, which the library computes from the count of
sequences per length before it launches anything, is the number of the second kind's candidates."""
import numpy as np
import pytest

import dn_short_sets as D
import support as S


def _diff(a: str, b: str) -> int:
    aw, bw = S.pack_seq(a.encode()), S.pack_seq(b.encode())
    return int(S.oracle().orc_nw_diff(S._p(aw, S.u64p), len(a), S._p(bw, S.u64p), len(b), 18, 24, 13, None, None))


def _random_mixed(rng, d: int) -> list:
    """a few hundred sequences around and below 16 (d + 1): families, so that pairs within d exist on every side"""
    T = D.short_below(d)
    seen = set()
    recs = D.short_material(rng, d, seen, straddlers=8, below=4)
    recs += D.families(rng, "l", 6, 6, [T + d - 1, T + d, T + d + 1, T + 2 * d + 2, 2 * T], d, seen)
    return [s for _, s in recs]


@pytest.mark.parametrize("d", [2, 3, 5])
def test_pairs_within_d_are_long_long_or_short_with_a_close_length(d):
    rng = np.random.default_rng(1600 + d)
    seqs = _random_mixed(rng, d)
    T = D.short_below(d)
    lens = np.array([len(s) for s in seqs])
    assert (lens < T).any() and (lens >= T).any()
    candidates = 0
    linked = {"short-short": 0, "short-long": 0, "long-long": 0}
    for i in range(len(seqs)):
        for j in range(i + 1, len(seqs)):
            shorts = int(lens[i] < T) + int(lens[j] < T)
            close = abs(int(lens[i]) - int(lens[j])) <= d
            if shorts and close:
                candidates += 1
            # (pairs the brute-force pass never compares must be beyond d; long pairs are the windows' business)
            if shorts == 0 and not close:
                continue
            within = _diff(seqs[i], seqs[j]) <= d
            if within:
                assert close, (seqs[i], seqs[j])
                linked[("long-long", "short-long", "short-short")[shorts]] += 1
    assert all(v > 0 for v in linked.values()), linked
    assert D.brute_candidates(lens, d) == candidates


@pytest.mark.parametrize("d", [2, 3, 8])
def test_b_equals_the_enumerated_candidates_on_random_lengths(d):
    rng = np.random.default_rng(77 + d)
    T = D.short_below(d)
    for trial in range(20):
        lens = rng.integers(1, T + 3 * d + 2, int(rng.integers(1, 400)))
        if trial % 4 == 0:
            lens = np.concatenate((lens, rng.integers(150, 401, 50)))
        short = lens < T
        diff = np.abs(lens[:, None] - lens[None, :]) <= d
        pair = np.triu(diff & (short[:, None] | short[None, :]), 1)
        assert D.brute_candidates(lens, d) == int(pair.sum())


def test_the_trial_set_of_the_issue_is_within_the_cap():
    """2 000 x 150 nt, 20 families of 9 around 64 nt, 10 families of 6 at 20-40 nt, singletons of 1 / 4 / 5 / 6 nt, d = 3:
    B a few thousand against a cap of about a million"""
    rng = np.random.default_rng(5)
    recs = D.short_material(rng, 3, set())
    lens = np.array([150] * 2000 + [len(s) for _, s in recs])
    b = D.brute_candidates(lens, 3)
    assert 0 < b < 20_000 < D.default_cap(len(lens))
