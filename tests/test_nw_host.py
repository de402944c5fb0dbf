"""The uclust aligner of the host (swa_nw_align_host, the specification of seam B5) against the oracle's
nw() (orc_nw_diff, pinned to the reference by test_oracle_golden / test_oracle_vs_reference): differences and
alignment length on fuzzed pairs, and a CIGAR that spells out exactly that alignment."""
import ctypes as C
import re

import numpy as np
import pytest

import support as S
from swarm_amd import nw_align_host

SCORINGS = [(18, 24, 13), (4, 12, 1), (2, 3, 1), (7, 11, 3), (10, 1, 10)]   # tests/test_scan_gpu.py's


def fuzz_pairs(rng, count, max_len=700):
    """(member, seed) strings: identical pairs, a few edits, pure length differences, tie-heavy homopolymer
    runs, unrelated pairs"""
    out = []
    for k in range(count):
        kind = k % 6
        L = int(rng.integers(1, max_len + 1)) if k % 3 == 0 else int(rng.integers(1, 160))
        if kind == 2:          # homopolymer runs: many equal-cost paths
            seq = "".join(rng.choice(list("AT")) * int(rng.integers(1, 9)) for _ in range(L // 4 + 1))[:L]
        else:
            seq = "".join(rng.choice(list("ACGT"), L))
        if kind == 0:
            other = seq
        elif kind == 3:        # unrelated
            other = "".join(rng.choice(list("ACGT"), int(rng.integers(1, max_len + 1))))
        elif kind == 4:        # a pure length difference: a run inserted or cut
            n = int(rng.integers(1, 40))
            at = int(rng.integers(0, L + 1))
            other = seq[:at] + "".join(rng.choice(list("ACGT"), n)) + seq[at:] if rng.random() < 0.5 or L <= n \
                else seq[:at] + seq[at + n:]
        else:                  # a few substitutions / insertions / deletions
            s = list(seq)
            for _ in range(int(rng.integers(1, 12))):
                op = int(rng.integers(0, 3))
                if op == 0 and s:
                    s[int(rng.integers(0, len(s)))] = str(rng.choice(list("ACGT")))
                elif op == 1 and len(s) > 1:
                    del s[int(rng.integers(0, len(s)))]
                else:
                    s.insert(int(rng.integers(0, len(s) + 1)), str(rng.choice(list("ACGT"))))
            other = "".join(s)
        out.append((other or "A", seq))
    return out


def _oracle(d, q, mm, go, ge):
    dw, qw = S.pack_seq(d.encode()), S.pack_seq(q.encode())
    alen, score = C.c_uint64(0), C.c_uint64(0)
    diff = S.oracle().orc_nw_diff(S._p(dw, S.u64p), len(d), S._p(qw, S.u64p), len(q), mm, go, ge, C.byref(alen), C.byref(score))
    return int(diff), int(alen.value)


def _check_cigar(cigar, dlen, qlen, columns):
    runs = [(int(n) if n else 1, op) for n, op in re.findall(r"(\d*)([MID])", cigar)]
    assert "".join(f"{n if n > 1 else ''}{op}" for n, op in runs) == cigar
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])), cigar          # runs are maximal
    assert sum(n for n, _ in runs) == columns
    assert sum(n for n, op in runs if op in "MI") == dlen
    assert sum(n for n, op in runs if op in "MD") == qlen


@pytest.mark.parametrize("scoring", SCORINGS)
def test_host_aligner_equals_the_oracle(scoring):
    mm, go, ge = scoring
    rng = np.random.default_rng(sum(scoring))
    for d, q in fuzz_pairs(rng, 240):
        diffs, columns, cigar = nw_align_host(S.pack_seq(d.encode()), len(d), S.pack_seq(q.encode()), len(q), mm, go, ge)
        assert (diffs, columns) == _oracle(d, q, mm, go, ge), (d, q)
        _check_cigar(cigar, len(d), len(q), columns)


def test_host_aligner_edges():
    for d, q in [("A", "A"), ("A", "C"), ("A", "AAAA"), ("AAAA", "A"), ("ACGT" * 175, "ACGT" * 175),
                 ("T" * 700, "T" * 650), ("A" * 300, "C" * 300)]:
        diffs, columns, cigar = nw_align_host(S.pack_seq(d.encode()), len(d), S.pack_seq(q.encode()), len(q))
        assert (diffs, columns) == _oracle(d, q, 18, 24, 13)
        _check_cigar(cigar, len(d), len(q), columns)
    assert nw_align_host(S.pack_seq(b"ACGT"), 4, S.pack_seq(b"ACGT"), 4) == (0, 4, "4M")
    assert nw_align_host(S.pack_seq(b"ACGTT"), 5, S.pack_seq(b"ACGT"), 4) == (1, 5, "4MI")
