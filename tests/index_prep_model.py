"""Plain models of the preparation stage of the d = 1 index build: what k_seqhash, the abundance-rank passes, k_db_lengths,
the window sample with choose_anchor_windows, and k_lines_build have to produce, written from the definitions (struct
swa_aux, the comments of d1_anchor.inc and d1_common.inc, the reference's zobrist.cc / variants.cc), not from the kernels.
numpy and Python only, exact 64-bit integers, no GPU and no product code: tests/test_index_prep_identity.py checks the
models against independent ground, tests/test_index_prep_gpu.py the kernels against the models.

A set of sequences is a matrix of nucleotide codes (0..3), one row an amplicon, zero behind its length, with the lengths
next to it: random_codes / pack_codes make the packed database the library takes from it without a loop over amplicons."""
import numpy as np

WIDTH_EDGES = (160, 256, 480, 672)        # upper edges of the width classes; beyond the last: too long for the pair kernels
GROUP_CAP = 2048                          # window sample: an estimated group size beyond this counts as stranded
CANDIDATES = (0, 32, 64, 96)              # candidate window offsets of the sample
MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------- sequences

def pack_codes(codes: np.ndarray, seqlen: np.ndarray):
    """(words u64, seq_off u64[n + 1]) of the rows of `codes` cut to `seqlen`: 32 nucleotides a word, the first in the
    lowest two bits, every sequence beginning a word"""
    codes = np.asarray(codes, dtype=np.uint8)
    seqlen = np.asarray(seqlen, dtype=np.int64)
    n, width = codes.shape
    wmax = (width + 31) // 32
    padded = np.zeros((n, 32 * wmax), dtype=np.uint8)
    padded[:, :width] = codes
    padded *= np.arange(32 * wmax)[None, :] < seqlen[:, None]
    shifts = np.arange(32, dtype=np.uint64) * np.uint64(2)
    words = np.zeros((n, wmax), dtype=np.uint64)
    for k in range(wmax):                                     # (a word at a time: the matrix never exists as 64-bit values)
        words[:, k] = np.bitwise_or.reduce(padded[:, 32 * k:32 * k + 32].astype(np.uint64) << shifts, axis=1)
    nw = (seqlen + 31) // 32
    used = np.arange(wmax)[None, :] < nw[:, None]
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(nw)
    flat = words[used]
    if flat.size == 0:
        flat = np.zeros(1, dtype=np.uint64)
    return np.ascontiguousarray(flat, dtype=np.uint64), off


def unpack_words(words, length: int) -> list:
    """the nucleotide codes of one packed sequence"""
    return [(int(words[p >> 5]) >> ((p & 31) * 2)) & 3 for p in range(length)]


def duplicate_rows(codes: np.ndarray, seqlen: np.ndarray) -> bool:
    """whether two amplicons of the set are the same sequence"""
    codes = np.asarray(codes, dtype=np.uint8)
    keep = np.arange(codes.shape[1])[None, :] < np.asarray(seqlen)[:, None]
    rows = np.concatenate([np.asarray(seqlen, dtype="<u4").view(np.uint8).reshape(-1, 4), codes * keep], axis=1)
    rows = np.ascontiguousarray(rows).view([("", np.void, rows.shape[1])]).ravel()
    return len(np.unique(rows)) != len(rows)


# ---------------------------------------------------------------------------------------------- k_seqhash

def aux_model(words, length: int, zobrist, anchor_w: int) -> dict:
    """struct swa_aux of one sequence.  zobrist[4 p + c] is Z[p][c].  h = XOR Z[p][s_p]; dall = XOR over p >= 1 of
    Z[p - 1][s_p] (the hash of the sequence behind a deleted position 0); iall = XOR Z[p + 1][s_p] (of the sequence behind
    a nucleotide inserted in front).  pb: first position of the run of equal nucleotides that contains position
    anchor_w - 1; a32 / d32 / i32: the same XORs over p < pb.  A sequence shorter than anchor_w has no such position:
    pb = anchor_w and the restricted streams are the full ones."""
    s = unpack_words(words, length)
    Z = lambda p, c: int(zobrist[4 * p + c])

    def streams(upto):
        h = d = i = 0
        for p in range(upto):
            h ^= Z(p, s[p])
            if p >= 1:
                d ^= Z(p - 1, s[p])
            i ^= Z(p + 1, s[p])
        return h, d, i

    h, dall, iall = streams(length)
    if length < anchor_w:
        pb = anchor_w
        a32, d32, i32 = h, dall, iall
    else:
        pb = anchor_w - 1
        while pb > 0 and s[pb - 1] == s[anchor_w - 1]:
            pb -= 1
        a32, d32, i32 = streams(pb)
    return {"h": h, "dall": dall, "iall": iall, "a32": a32, "d32": d32, "i32": i32, "pb": pb}


# ---------------------------------------------------------------------------------------------- abundance ranks

def ranks_model(abundance) -> np.ndarray:
    """rank[i] = index of the first amplicon with the abundance of amplicon i (the database is in descending order)"""
    neg = -np.asarray(abundance).astype(np.int64)
    return np.searchsorted(neg, neg, side="left").astype(np.uint32)


def ranks_brute(abundance) -> np.ndarray:
    """the same by walking the runs (for small n)"""
    out, start = [], 0
    for i in range(len(abundance)):
        if i > 0 and int(abundance[i]) != int(abundance[i - 1]):
            start = i
        out.append(start)
    return np.array(out, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------- k_db_lengths

def width_class(length: int) -> int:
    for c, edge in enumerate(WIDTH_EDGES):
        if length <= edge:
            return c
    return len(WIDTH_EDGES)


def lengths_model(seqlen):
    """(shortest length, [sequences of width class 0 .. 4]); class 4: longer than 672 nt"""
    seqlen = np.asarray(seqlen, dtype=np.int64)
    cls = np.searchsorted(np.array(WIDTH_EDGES), seqlen, side="left")          # first edge >= length
    return int(seqlen.min()), [int(v) for v in np.bincount(cls, minlength=len(WIDTH_EDGES) + 1)]


# ---------------------------------------------------------------------------------------------- the anchor windows

def anchor_nwin_model(shortest: int, offset: int, max_nwin: int) -> int:
    """words of 32 nt per anchor window: windows at the ends are as wide (32, 64 or 128 nt, at most max_nwin words) as
    leaves the shortest sequence two windows and a nucleotide; windows moved inwards keep one word"""
    if offset != 0:
        return 1
    nwin = 1
    for c in (2, 4):
        if c <= max_nwin and 2 * 32 * c + 1 <= shortest:
            nwin = c
    return nwin


def _group_counts(rows: np.ndarray) -> np.ndarray:
    """sizes of the groups of equal rows"""
    if rows.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    rows = np.ascontiguousarray(rows)
    keys = rows.view([("", np.void, rows.shape[1])]).ravel()
    return np.unique(keys, return_counts=True)[1].astype(np.int64)


def windows_model(seqs, seqlen, n: int, shortest: int, max_nwin: int) -> dict:
    """What the sample sees and what is chosen from it.  seqs: the matrix of codes.  Every stride-th amplicon is a sample,
    stride = max(1, n // 65536).  Per candidate offset w: the window width, the samples too short for two such windows
    and a nucleotide (they file no key), and the mass: the samples in groups — equal prefix-side window [w, w + W), or equal
    suffix-side window [len - w - W, len - w) — whose estimated size count * stride exceeds 2048, both sides added.
    The choice: the first candidate whose mass and whose too-short count are at most samples // 64 (candidate 0 is not
    asked about the short ones); the search ends at the first candidate with too many short samples; otherwise the ends."""
    seqs = np.asarray(seqs, dtype=np.uint8)
    seqlen = np.asarray(seqlen, dtype=np.int64)
    stride = max(1, n // 65536)
    picks = np.arange(0, n, stride)
    samples = len(picks)
    slen = seqlen[picks]
    too_short, mass = [], []
    for w in CANDIDATES:
        width = 32 * anchor_nwin_model(shortest, w, max_nwin)
        ok = slen >= 2 * w + 2 * width + 1
        too_short.append(int((~ok).sum()))
        rows, lens = picks[ok], slen[ok]
        total = 0
        for side in range(2):
            begin = np.full(len(rows), w, dtype=np.int64) if side == 0 else lens - w - width
            window = seqs[rows[:, None], begin[:, None] + np.arange(width)[None, :]]
            counts = _group_counts(window)
            total += int(counts[counts * stride > GROUP_CAP].sum())
        mass.append(total)
    limit = samples // 64
    offset, width = 0, 32 * anchor_nwin_model(shortest, 0, max_nwin)
    for c, w in enumerate(CANDIDATES):
        few_short = too_short[c] <= limit or c == 0
        if mass[c] <= limit and few_short:
            offset, width = w, 32 * anchor_nwin_model(shortest, w, max_nwin)
            break
        if not few_short:
            break
    return {"too_short": too_short, "mass": mass, "stride": stride, "samples": samples, "offset": offset, "width": width,
            "taken": True}


# ---------------------------------------------------------------------------------------------- k_lines_build

def line_quads_model(longest: int) -> int:
    return 4 if longest <= 160 else (8 if longest <= 480 else 16)


def lines_model(words, seq_off, seqlen, ranks, longest: int) -> np.ndarray:
    """u32[n, 4 quads]: dword 0 the length, dword 1 the abundance rank, then the packed words, zero up to the end of the
    line.  A line of q quads holds 2 q - 1 words; of a longer sequence it holds the first that many."""
    seqlen = np.asarray(seqlen, dtype=np.int64)
    n = len(seqlen)
    quads = line_quads_model(longest)
    cap = 2 * quads - 1
    body = np.zeros((n, cap), dtype=np.uint64)
    nw = np.minimum((seqlen + 31) // 32, cap)
    start = np.asarray(seq_off[:-1], dtype=np.int64)
    for k in range(cap):                                      # (a loop over the words of a line, not over amplicons)
        have = nw > k
        body[have, k] = np.asarray(words)[start[have] + k]
    out = np.zeros((n, 4 * quads), dtype=np.uint32)
    out[:, 0] = seqlen
    out[:, 1] = ranks
    out[:, 2:] = body.view(np.uint32).reshape(n, 2 * cap)
    return out
