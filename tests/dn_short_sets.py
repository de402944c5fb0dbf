"""Inputs for the tests of the d >= 2 graph route on databases with SHORT sequences (fewer than 16 (d + 1) nucleotides:
no room for d + 1 windows), and the library's rule for them restated in numpy.  Not product code.

The rule (dn_graph.hip): short sequences stay out of the window groups; every pair with a short member is found by
comparing each short sequence with all sequences whose length differs by at most d.  B = the number of such (short,
partner) candidates, every pair once; the graph route serves a database when B <= 16 n + 2^20 (or SWA_DN_BRUTE_CAP)."""
from __future__ import annotations

import numpy as np

import support as S


def short_below(d: int) -> int:
    return 16 * (d + 1)


def default_cap(n: int) -> int:
    return 16 * n + (1 << 20)


def brute_candidates(lengths, d: int) -> int:
    """B from the count of sequences per length, as window_length() computes it"""
    lengths = np.asarray(lengths, dtype=np.int64)
    T = short_below(d)
    hist = np.bincount(lengths[lengths < T + d], minlength=T + d).astype(np.int64)
    total = 0
    for L in range(T):
        h = int(hist[L])
        if h:
            total += h * (h - 1) // 2 + h * int(hist[L + 1:L + d + 1].sum())
    return total


def _rand(rng, length: int) -> str:
    return "".join("ACGT"[v] for v in rng.integers(0, 4, length))


def edit(rng, s: str) -> str:
    """one substitution, deletion or insertion"""
    how = int(rng.integers(0, 3))
    b = "ACGT"[int(rng.integers(0, 4))]
    if how == 1 and len(s) > 1:
        p = int(rng.integers(0, len(s)))
        return s[:p] + s[p + 1:]
    if how == 2:
        p = int(rng.integers(0, len(s) + 1))
        return s[:p] + b + s[p:]
    p = int(rng.integers(0, len(s)))
    return s[:p] + b + s[p + 1:]


def families(rng, tag: str, count: int, members: int, lengths, d: int, seen: set) -> list:
    """`count` families: a centroid of a length drawn from `lengths` and `members` - 1 mutants 1..d edits away from it
    (substitutions and indels), with abundances above and below the centroid's; no sequence twice"""
    recs = []
    for f in range(count):
        cent = _rand(rng, int(lengths[f % len(lengths)]))
        if cent in seen:
            continue
        seen.add(cent)
        recs.append((f"{tag}{f}c_10", cent))
        for m in range(1, members):
            s = cent
            for _ in range(int(rng.integers(1, d + 1))):
                s = edit(rng, s)
            if s in seen:
                continue
            seen.add(s)
            recs.append((f"{tag}{f}m{m}_{int(rng.choice([1, 1, 2, 10, 25]))}", s))
    return recs


def short_material(rng, d: int, seen: set, straddlers: int = 20, below: int = 10) -> list:
    """families whose lengths straddle 16 (d + 1) (short-short, short-long and long-long pairs in one family), families
    well below it, and singletons without a q-gram (1, 4 nt) or with one or two (5, 6 nt)"""
    T = short_below(d)
    recs = families(rng, "x", straddlers, 9, [T - 2, T - 1, T, T + 1], d, seen)
    recs += families(rng, "y", below, 6, list(range(20, 41, 2)), d, seen)
    for k, s in enumerate(("G", "ACGT", "TTGCA", "CAGTCA")):
        assert s not in seen
        seen.add(s)
        recs.append((f"z{k}_{k + 1}", s))
    return recs


def mixed_set(path, d: int, seed: int, bulk=((2000, 150), (1000, 400))) -> list:
    """a bulk of generated amplicons (tools/gen_amplicons, up to d edits a member) plus short_material(); returns the
    records [(header, sequence)] as written"""
    recs = []
    seen = set()
    for k, (n, length) in enumerate(bulk):
        part = path.with_suffix(f".bulk{k}")
        S.gen_fasta(part, n, length, seed + k, d)
        for h, s in S.read_fasta(part):
            s = s.decode()
            if s not in seen:
                seen.add(s)
                recs.append((f"b{k}{h.decode()}", s))
        part.unlink()
    recs += short_material(np.random.default_rng(seed), d, seen)
    path.write_text("".join(f">{h}\n{s}\n" for h, s in recs))
    return recs
