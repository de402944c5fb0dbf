"""The flexible Bloom filter of the --fastidious Bloom route (the reference's src/bloomflex.cc; swarm_amd/csrc/fastidious.hip:
fastidious_bloom_route, k_d1_flex<., 0 | 1>, flex_word) as a model in plain integers over the oracle's microvariant hashes.
Not product code.

  m      = max(7 * bits * light_nt, 64)      bits of the filter
  fsize  = (((m - 1) // 8) + 1) >> 3         its 64-bit words: the bytes, truncated to whole words
  k      = max(int(0.4 * bits), 1)           bits of a pattern; the one float of the model, the reference's own expression
  pat    = orc_bloomflex_patterns(k)         65 536 patterns of k bits, mt19937_64(1)
  light pass:  words start all-ones; every microvariant hash h of every light amplicon does
               words[(h >> 16) % fsize] &= ~pat[h & 0xFFFF]
  heavy pass:  a microvariant h of a heavy amplicon is a task when (words[(h >> 16) % fsize] & pat[h & 0xFFFF]) == 0

Everything but k is np.uint64 or a Python integer; no value goes through a float (numpy turns uint64 combined with a
Python or a signed integer into float64, hence the typed constants).  flex_word_np restates the kernel's reciprocal form
of the word index, which does go through a double, for the identity test against the exact `%`."""
from __future__ import annotations

import ctypes as C

import numpy as np

import support as S

VAR_DTYPE = np.dtype([("hash", "<u8"), ("pos", "<u4"), ("type", "u1"), ("base", "u1"), ("pad", "<u2")])
assert VAR_DTYPE.itemsize == C.sizeof(S.OrcVar) == 16
TASK_DTYPE = np.dtype([("heavy", "<u4"), ("hash", "<u8"), ("pos", "<u4"), ("type", "u1"), ("base", "u1")])
_16, _MASK16 = np.uint64(16), np.uint64(0xFFFF)


def k_of(bits: int) -> int:
    """src/algod1.cc:1383-1385: the reference's expression, in double precision as there"""
    return max(int(0.4 * float(bits)), 1)


def sizes(light_nt: int, bits: int) -> tuple:
    """(m, n_bytes, fsize) in Python integers: algod1.cc:1386-1390, bloomflex.cc:91-101"""
    m = max(7 * int(bits) * int(light_nt), 64)
    n_bytes = (m - 1) // 8 + 1
    return m, n_bytes, n_bytes >> 3


def patterns(k: int) -> np.ndarray:
    pat = np.zeros(65536, dtype=np.uint64)
    S.oracle().orc_bloomflex_patterns(int(k), S._p(pat, S.u64p))
    return pat


def variants_of(db: S.Db, tab: np.ndarray, amp: int) -> np.ndarray:
    """the microvariants of one amplicon as the oracle enumerates them (VAR_DTYPE), straight out of its buffer"""
    lib = S.oracle()
    length = int(db.seqlen[amp])
    words = np.ascontiguousarray(db.words(amp))
    h = lib.orc_zobrist_hash(S._p(tab, S.u64p), S._p(words, S.u64p), length)
    buf = (S.OrcVar * (7 * length + 5))()
    n = lib.orc_generate_variants(S._p(tab, S.u64p), S._p(words, S.u64p), length, h, buf)
    return np.frombuffer(buf, dtype=VAR_DTYPE, count=n).copy()


def word_index(h: np.ndarray, fsize: int) -> np.ndarray:
    """(h >> 16) % fsize, exact in uint64"""
    return (h >> _16) % np.uint64(fsize)


def flex_model(db: S.Db, flags: np.ndarray, bits: int) -> dict:
    """{"light_nt", "k", "m", "fsize", "words" (u64[fsize]), "tasks" (how many heavy microvariants pass the filter),
    "heavy_variants", and beside what the issue of the filter needs: "light_variants", "task_list" (TASK_DTYPE: the tasks
    themselves, heavy amplicons ascending, a heavy amplicon's in the oracle's order)}"""
    flags = np.asarray(flags)
    light = np.flatnonzero(flags != 0)
    heavy = np.flatnonzero(flags == 0)
    light_nt = int(db.seqlen[light].astype(np.uint64).sum())
    k = k_of(bits)
    m, _, fsize = sizes(light_nt, bits)
    pat = patterns(k)
    tab = S.oracle_zobrist(db.longest + 2)
    words = np.full(fsize, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    light_variants = 0
    for a in light:
        h = variants_of(db, tab, int(a))["hash"]
        light_variants += len(h)
        np.bitwise_and.at(words, word_index(h, fsize).astype(np.intp), ~pat[(h & _MASK16).astype(np.intp)])
    heavy_variants, chunks = 0, []
    for s in heavy:
        v = variants_of(db, tab, int(s))
        heavy_variants += len(v)
        h = v["hash"]
        hit = (words[word_index(h, fsize).astype(np.intp)] & pat[(h & _MASK16).astype(np.intp)]) == np.uint64(0)
        t = np.zeros(int(hit.sum()), dtype=TASK_DTYPE)
        t["heavy"] = s
        for f in ("hash", "pos", "type", "base"):
            t[f] = v[f][hit]
        chunks.append(t)
    task_list = np.concatenate(chunks) if chunks else np.zeros(0, dtype=TASK_DTYPE)
    return {"light_nt": light_nt, "k": k, "m": m, "fsize": fsize, "words": words, "tasks": int(len(task_list)),
            "heavy_variants": heavy_variants, "light_variants": light_variants, "task_list": task_list}


def flex_word_np(x: np.ndarray, fsize: int) -> np.ndarray:
    """flex_word of fastidious.hip on x = h >> 16 (< 2^48), operation for operation in float64 / uint64 / int64: the
    quotient from a reciprocal in double precision, the remainder from it, one correction step either way"""
    x = np.asarray(x, dtype=np.uint64)
    f = np.uint64(fsize)
    finv = np.float64(1.0) / np.float64(fsize)
    q = (x.astype(np.float64) * finv).astype(np.uint64)          # (uint64_t)((double)x * finv): truncation
    r = (x - q * f).view(np.int64)                               # wraps like the kernel's unsigned arithmetic
    r = np.where(r < 0, r + np.int64(fsize), np.where(r >= np.int64(fsize), r - np.int64(fsize), r))
    return r.astype(np.uint64)


# the smallest filters: (heavy centre, light amplicon two edits away) by the light one's length.  7 * 2 bits * 2 nt = 28 bits are
# lifted to m = 64; 7 * 2 * 5 = 70 bits are 9 bytes, which the reference truncates to one word as well
HAND = {2: ("ACG", "TC"), 5: ("ACGT", "TCGTA")}


def hand_case(light_len: int) -> tuple:
    """(db, is_light): amplicon 0 the heavy centre, amplicon 1 the light one"""
    heavy, light = HAND[light_len]
    db = S.build_db([(b"h_9", heavy.encode()), (b"x_1", light.encode())])
    return db, np.array([0, 1], dtype=np.uint8)


def variant_string(db: S.Db, task) -> str:
    """the sequence of a task's microvariant (the oracle's generate_variant_sequence on the heavy amplicon)"""
    lib = S.oracle()
    s = int(task["heavy"])
    length = int(db.seqlen[s])
    words = np.ascontiguousarray(db.words(s))
    var = S.OrcVar(int(task["hash"]), int(task["pos"]), int(task["type"]), int(task["base"]), 0)
    out = np.zeros((length + 1 + 31) // 32 + 1, dtype=np.uint64)
    n = lib.orc_generate_variant_sequence(S._p(words, S.u64p), length, C.byref(var), S._p(out, S.u64p))
    return "".join("ACGT"[(int(out[p >> 5]) >> ((p & 31) * 2)) & 3] for p in range(n))
