"""The schedule of k_align_wide<K> (align_wide_model.wide_model: K offsets a lane, one parity live a step, two values
crossing the lanes, guards, the end cell's (lane, j)) with 4, 8 and 64 lanes against the plain row-by-row band
(generic_model, which restates k_align_generic) — bit-identical in (diff, score, length) on every pair — and against
the oracle's orc_nw_diff under the parity rule of tests/test_align_forms_gpu.py: where the oracle's diff <= d and its
score lies below the saturation value the three are identical, everywhere else the model's diff is > d.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import support as S
from align_wide_model import band_of, end_cell, generic_model, live_parity, wide_k, wide_model

UNIT, DEFAULT = (1, 0, 1), (18, 24, 13)
# (lanes, K, scoring, d): both parities of W for every (lanes, K); W = d + 1 at the unit scoring
CASES = [(4, 2, UNIT, 1), (4, 4, UNIT, 4), (4, 4, UNIT, 5), (4, 8, UNIT, 12), (4, 8, UNIT, 13),
         (8, 2, UNIT, 4), (8, 2, UNIT, 5), (8, 4, UNIT, 12), (8, 4, UNIT, 13), (8, 8, UNIT, 28), (8, 8, UNIT, 29),
         (8, 8, DEFAULT, 10),
         (64, 2, UNIT, 31), (64, 2, UNIT, 32), (64, 2, UNIT, 61), (64, 2, DEFAULT, 11), (64, 2, DEFAULT, 12),
         (64, 4, UNIT, 62), (64, 4, UNIT, 63), (64, 4, DEFAULT, 22), (64, 4, DEFAULT, 23),
         (64, 8, UNIT, 126), (64, 8, UNIT, 127), (64, 8, DEFAULT, 45), (64, 8, DEFAULT, 47)]
LENGTHS = [1, 2, 3, 5, 8, 13, 21, 31, 32, 33, 40, 64, 80]


def _codes(s) -> str:
    return "".join("ACGT"[v] for v in s)


def _oracle(dseq, qseq, mm, go, ge):
    dw, qw = S.pack_seq(_codes(dseq).encode()), S.pack_seq(_codes(qseq).encode())
    alen, score = C.c_uint64(0), C.c_uint64(0)
    d = S.oracle().orc_nw_diff(S._p(dw, S.u64p), len(dseq), S._p(qw, S.u64p), len(qseq), mm, go, ge,
                               C.byref(alen), C.byref(score))
    return int(d), int(score.value), int(alen.value)


def _base(rng, length, two):
    if not two:
        return [int(v) for v in rng.integers(0, 4, size=length)]
    out = []
    while len(out) < length:                                 # two letters in long runs: many equally good alignments
        out += [int(rng.integers(0, 2))] * int(rng.integers(1, 9))
    return out[:length]


def _mutate(rng, s, edits, letters):
    s = list(s)
    for _ in range(edits):
        p = int(rng.integers(0, len(s) + 1))
        u = rng.random()
        b = int(rng.integers(0, letters))
        if u < 0.5 and p < len(s):
            s[p] = b
        elif u < 0.75 and p < len(s) and len(s) > 1:
            del s[p]
        else:
            s.insert(p, b)
    return s


def _pairs(rng, d, W):
    """mutated pairs of 1 .. 80 nt over four and over two letters, and pairs whose lengths differ by 0, W - 1, W, W + 1"""
    out = []
    for k in range(10):
        two = k % 2 == 1
        a = _base(rng, int(rng.choice(LENGTHS)), two)
        out.append((a, _mutate(rng, a, int(rng.integers(0, min(d, 12) + 4)), 2 if two else 4)))
    for k, delta in enumerate((0, W - 1, W, W + 1)):
        two = k % 2 == 1
        short = int(rng.integers(1, 6)) if delta > 40 else int(rng.integers(1, 81 - delta))
        a = _base(rng, short + delta, two)
        b = list(a)
        for _ in range(delta):
            del b[int(rng.integers(0, len(b)))]
        out.append((a, b) if k < 2 else (b, a))
    return out


@pytest.mark.parametrize("lanes,K,scoring,d", CASES, ids=[f"{ln}x{k}-{s}-d{d}" for ln, k, s, d in CASES])
def test_schedule_equals_rows_and_oracle(lanes, K, scoring, d):
    W, sat = band_of(*scoring, d)
    assert wide_k(W, lanes) == K                             # the smallest K that holds the band on these lanes
    rng = np.random.default_rng(lanes * 1000 + K * 100 + d)
    accepted = infeasible = 0
    for dseq, qseq in _pairs(rng, d, W):
        rows = generic_model(dseq, qseq, *scoring, sat, W)
        assert wide_model(dseq, qseq, *scoring, sat, W, K, lanes) == rows, (dseq, qseq)
        od, osc, ol = _oracle(dseq, qseq, *scoring)
        if od <= d and osc < sat:
            accepted += 1
            assert rows == (od, osc, ol), (dseq, qseq)
        else:
            assert rows[0] > d, (dseq, qseq, rows, od, osc)
        infeasible += abs(len(dseq) - len(qseq)) > W
    assert accepted >= 1 and infeasible >= 1                 # (the identical pair; the W + 1 pair)


@pytest.mark.parametrize("lanes,K", [(4, 2), (4, 4), (8, 8), (64, 2)])
def test_any_band_the_lanes_hold(lanes, K):
    """every W from 1 to the widest the lanes hold (no d gives W = 1; the rows are the yardstick here), 8- and 16-bit"""
    rng = np.random.default_rng(lanes + K)
    for W in range(1, min((lanes * K - 3) // 2, 40) + 1):
        for sat, scoring in ((255, (4, 2, 3)), (65535, DEFAULT)):
            for dseq, qseq in _pairs(rng, W, W)[6:]:
                assert wide_model(dseq, qseq, *scoring, sat, W, K, lanes) == generic_model(dseq, qseq, *scoring, sat, W)


def test_schedule_facts():
    """One parity a step, alternating; the shuffle a step needs follows the parity; a step computes the cells of its
    anti-diagonal inside band and matrix; the end cell's (lane, j)."""
    rng = np.random.default_rng(9)
    for W, K in ((32, 2), (33, 2), (63, 4), (64, 4)):
        dseq, qseq = _base(rng, 50, False), _base(rng, 50 + W - 3, False)
        trace = []
        wide_model(dseq, qseq, 1, 0, 1, 255, W, K, 64, trace)
        assert len(trace) == len(dseq) + len(qseq) - 1
        for s, par, kind, cells in trace:
            assert par == live_parity(s, W) == (s + 1 + W) % 2 and kind == ("below", "above")[par]
            want = sum(1 for r in range(len(dseq)) if 0 <= s - r < len(qseq) and abs(s - 2 * r) <= W)
            assert cells == want
        ln, j = end_cell(len(dseq), len(qseq), W, K)
        assert ln * K + j == len(qseq) - len(dseq) + W + 1 and 0 <= j < K and 0 <= ln < 64
    # the end cell on j = 0 and on j = K - 1, on the first and the last in-band index
    assert end_cell(40, 40 - 32, 32, 2) == (0, 1) and end_cell(8, 40, 32, 2) == (32, 1)
    assert end_cell(40, 43, 32, 4) == (9, 0) and end_cell(40, 42, 32, 4) == (8, 3)
