"""The preparation stage of the d = 1 index build — the kernels that turn an uploaded database into the facts every later
kernel trusts — each in front of its exact model (tests/index_prep_model.py; the models themselves are checked on the CPU
by tests/test_index_prep_identity.py).  Every comparison is np.array_equal: integers, no tolerance.

  k_seqhash<true | false>     the per-amplicon record swa_aux (selector 3 of swa_d1_debug_read) against aux_model, at every
                              anchor width the build can choose and with the Zobrist table in LDS and in HBM
  k_abundance_rank, _carry,   the ranks as the amplicon lines carry them (selector 15, dword 1) against ranks_model, with run
  _fill                       boundaries on lane, wave, tile and turn edges
  k_lines_build<4 | 8 | 16>   the same reads, whole lines against lines_model
  k_db_lengths                the shortest sequence and the width-class populations (selector 4) against lengths_model
  k_anchor_sample,            the eight statistics, stride, samples and the choice made from them (selector 5) against
  k_sample_mass,              windows_model, on both sides of every threshold of the rule
  choose_anchor_windows

Databases are made from seeded generators and uploaded as arrays; each set is checked for identical sequences before it
is uploaded, and the index build's own answer must agree (none)."""
import numpy as np
import pytest

import index_prep_model as M
import support as S
from d1_sets import oracle_sorted_rows, upload

pytestmark = pytest.mark.gpu

WIDTH_HOOK = "SWA_D1_ANCHOR_W"
TURN = 256 * 8 * 256                      # amplicons per turn of k_abundance_rank_carry: 2048 tiles of 256


# ---------------------------------------------------------------------------------------------- making databases

def _db(codes, seqlen, abundance) -> S.Db:
    seqlen = np.ascontiguousarray(seqlen, dtype=np.uint32)
    assert not M.duplicate_rows(codes, seqlen)
    words, off = M.pack_codes(codes, seqlen)
    return S.Db(headers=[], seqs=words, seq_off=off, seqlen=seqlen, abundance=np.ascontiguousarray(abundance, dtype=np.uint64),
                longest=int(seqlen.max()))


def _matrix(rows) -> tuple:
    """rows of unequal length -> (matrix of codes, lengths)"""
    lens = np.array([len(r) for r in rows], dtype=np.uint32)
    codes = np.zeros((len(rows), int(lens.max())), dtype=np.uint8)
    for i, r in enumerate(rows):
        codes[i, :len(r)] = r
    return codes, lens


def _fixed_db(rng, n: int, length: int, abundance) -> S.Db:
    """n random sequences of one length, made as packed words (no matrix of codes: for the large sets)"""
    nw = (length + 31) // 32
    words = rng.integers(0, 1 << 64, (n, nw), dtype=np.uint64, endpoint=False)
    tail = length - 32 * (nw - 1)
    if tail < 32:
        words[:, -1] &= np.uint64((1 << (2 * tail)) - 1)
    assert len(np.unique(words.view([("", np.void, 8 * nw)]).ravel())) == n
    return S.Db(headers=[], seqs=np.ascontiguousarray(words.ravel()), seq_off=(np.arange(n + 1, dtype=np.uint64) * np.uint64(nw)),
                seqlen=np.full(n, length, dtype=np.uint32), abundance=np.ascontiguousarray(abundance, dtype=np.uint64), longest=length)


def _abundance(n: int, starts) -> np.ndarray:
    """descending abundances whose runs of equal values begin exactly at `starts` (0 among them)"""
    first = np.zeros(n, dtype=bool)
    first[np.asarray(starts, dtype=np.int64)] = True
    assert first[0]
    run = np.cumsum(first)
    return (int(run[-1]) - run + 1).astype(np.uint64)


def _build(ctx, db):
    upload(ctx, db)
    assert ctx.d1_index_build() is False                      # (_db / _fixed_db asserted that no two sequences are the same)


# ---------------------------------------------------------------------------------------------- k_seqhash

def _stream_rows(rng, lengths, W: int, n: int) -> list:
    """the set of the stream test for anchor width W: see test_hashes_and_streams"""
    rows, seen = [], set()

    def add(row):
        row = np.asarray(row, dtype=np.uint8)
        if row.tobytes() in seen:
            return
        seen.add(row.tobytes())
        rows.append(row)

    rand = lambda L, letters=4: rng.integers(0, letters, L).astype(np.uint8)
    for k, L in enumerate([lengths[0]] + list(lengths[-4:])):
        add(np.full(L, k % 4))                                # one run from end to end: pb = 0
    for L in [v for v in lengths if v >= W + 8][:4]:
        r = rand(L); c = int(r[W - 1]); r[W - 2] = (c + 1) & 3; r[W] = c
        add(r)                                                # a run that starts exactly at W - 1
        r = rand(L); c = int(r[W - 1]); r[W - 5:W] = c; r[W - 6] = (c + 1) & 3; r[W] = (c + 2) & 3
        add(r)                                                # ... one that ends there
        r = rand(L); c = int(r[W - 1]); r[W - 4:W + 5] = c; r[W - 5] = (c + 1) & 3
        add(r)                                                # ... one that holds it and crosses the word boundary behind it
        if W >= 64:
            r = rand(L); c = int(r[W - 1]); r[W - 36:W] = c; r[W - 37] = (c + 1) & 3
            add(r)                                            # ... one that comes into its word from the word before
        r = rand(L); r[:W] = r[W - 1]
        add(r)                                                # the whole window one run (pb = 0), the rest not
    k = 0
    while len(rows) < n:
        add(rand(lengths[k % len(lengths)], 2 if k % 3 == 0 else 4))      # every third from a two-letter alphabet
        k += 1
        assert k < 100 * n
    return [rows[i] for i in rng.permutation(len(rows))]


def _aux_want(db, W: int, zob) -> np.ndarray:
    from swarm_amd import capi
    out = np.zeros(db.n, dtype=capi.AUX_DTYPE)
    for i in range(db.n):
        for k, v in M.aux_model(db.words(i), int(db.seqlen[i]), zob, W).items():
            out[k][i] = v
    return out


def _same_aux(got, want, what):
    for k in ("h", "dall", "iall", "pb", "a32", "d32", "i32"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert bad.size == 0, (what, k, bad[:8].tolist(), got[k][bad[:4]].tolist(), want[k][bad[:4]].tolist())
    assert not got["pad"].any(), what


STREAM_SETS = {
    "short": [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160],         # shortest 1: 32-nt windows
    "mid": [129, 130, 159, 160, 161, 191, 192, 193, 255, 256],           # shortest 129: 64-nt windows
    "long": [257, 258, 287, 288, 289, 319, 320, 321, 383, 384, 385, 400],    # shortest 257: 128-nt windows
}


@pytest.mark.parametrize("name, hook, W", [("short", None, 32), ("mid", None, 64), ("long", None, 128), ("long", "64", 64),
                                           ("long", "32", 32), ("mid", "32", 32)])
def test_hashes_and_streams_at_every_anchor_width(gpu_ctx, monkeypatch, name, hook, W):
    """k_seqhash<true>: every field of swa_aux against aux_model.  The width comes from the shortest sequence of the set,
    or from the hook that caps it; 257 amplicons (a grid tail of one thread), then one alone.  The set holds one-run
    sequences, a run that starts exactly at W - 1, one that ends there, runs across the 32-nt word boundaries around it,
    a two-letter alphabet, and every length around the word boundaries (with W = 32 also sequences shorter than the
    window: pb = W, the restricted streams are the full ones)."""
    if hook is None:
        monkeypatch.delenv(WIDTH_HOOK, raising=False)
    else:
        monkeypatch.setenv(WIDTH_HOOK, hook)
    rng = np.random.default_rng(1000 + W + len(name))
    lengths = STREAM_SETS[name]
    rows = _stream_rows(rng, lengths, W, 257)
    assert len(rows) == 257
    codes, lens = _matrix(rows)
    db = _db(codes, lens, _abundance(257, range(0, 257, 5)))
    zob = S.oracle_zobrist(db.longest + 2)
    want = _aux_want(db, W, zob)
    # (the set is what it says it is)
    assert (want["pb"] == 0).sum() >= 5 and (want["pb"] == W - 1).sum() >= 3 and ((want["pb"] > 0) & (want["pb"] < W - 1)).sum() >= 8
    assert ((want["pb"] == W).sum() > 0) == (min(lengths) < W)
    _build(gpu_ctx, db)
    assert gpu_ctx.d1_anchor_width() == W
    got = gpu_ctx.d1_aux()
    assert gpu_ctx.d1_anchor_width() == W                     # (the reader built the database-wide index: under the same windows)
    _same_aux(got, want, (name, hook))
    assert np.array_equal(gpu_ctx.d1_debug(0, db.n), want["h"])
    # one amplicon alone, a single thread: the first of the set whose own length gives the same width
    cap = int(hook) // 32 if hook else 4
    one = next(i for i in range(db.n) if lens[i] >= 65 and 32 * M.anchor_nwin_model(int(lens[i]), 0, cap) == W and 0 < want["pb"][i] < W - 1)
    db1 = _db(codes[one:one + 1, :int(lens[one])], lens[one:one + 1], [3])
    _build(gpu_ctx, db1)
    assert gpu_ctx.d1_anchor_width() == W
    _same_aux(gpu_ctx.d1_aux(), _aux_want(db1, W, S.oracle_zobrist(db1.longest + 2)), (name, hook, "alone"))


def test_hashes_and_streams_with_the_zobrist_table_in_hbm(gpu_ctx, monkeypatch):
    """k_seqhash<false>: the longest sequence is the first whose Zobrist table, 4 (longest + 2) words of 8 bytes, no longer
    fits SWA_MAX_ZOBRIST_LDS (read from the build)."""
    monkeypatch.delenv(WIDTH_HOOK, raising=False)
    rng = np.random.default_rng(77)
    _build(gpu_ctx, _fixed_db(rng, 4, 70, [2, 2, 1, 1]))
    limit = gpu_ctx.d1_db_facts()["max_zobrist_lds"]
    assert limit >= 4 * 8 * 200
    longest = limit // 32 - 1
    assert 4 * (longest + 2) * 8 > limit >= 4 * (longest + 1) * 8         # the table of this set is the first one over the limit
    rows = [rng.integers(0, 4, L).astype(np.uint8) for L in (longest, longest - 1, longest - 71, 700, 65, 33, 40)]
    rows[1][:40] = 2                                          # (a run over the window's end: pb = 0)
    rows[2][20:32] = 1; rows[2][19] = 3
    codes, lens = _matrix(rows)
    db = _db(codes, lens, _abundance(len(rows), [0, 3]))
    zob = S.oracle_zobrist(db.longest + 2)
    want = _aux_want(db, 32, zob)
    lib = S.oracle()
    assert [int(v) for v in want["h"]] == [int(lib.orc_zobrist_hash(S._p(zob, S.u64p), S._p(db.words(i), S.u64p), int(db.seqlen[i])))
                                           for i in range(db.n)]
    _build(gpu_ctx, db)
    assert gpu_ctx.d1_anchor_width() == 32
    _same_aux(gpu_ctx.d1_aux(), want, "zobrist in HBM")
    assert np.array_equal(gpu_ctx.d1_debug(2, 4 * (db.longest + 2)), zob)


# ---------------------------------------------------------------------------------------------- ranks and lines

def _lines(ctx, n: int):
    quads = int(ctx.d1_debug(16, 4 * 8 + 2)[33])              # (selector 16: the list regions, their end, the quads a line)
    return quads, ctx.d1_debug(15, n * quads * 2).view(np.uint32).reshape(n, 4 * quads)


def _check_ranks_and_lines(ctx, db, what, want_ranks=None):
    _build(ctx, db)
    quads, got = _lines(ctx, db.n)
    ranks = M.ranks_model(db.abundance)
    if want_ranks is not None:
        assert np.array_equal(ranks, want_ranks), what        # (the model gives what the case was built to hold)
    want = M.lines_model(db.seqs, db.seq_off, db.seqlen, ranks, db.longest)
    assert quads == M.line_quads_model(db.longest), what
    bad = np.nonzero(got[:, 1] != want[:, 1])[0]
    assert bad.size == 0, (what, "ranks", bad.size, bad[:8].tolist(), got[bad[:8], 1].tolist(), want[bad[:8], 1].tolist())
    assert np.array_equal(got[:, 0], want[:, 0]), (what, "lengths")
    assert np.array_equal(got[:, 2:], want[:, 2:]), (what, "words and padding")


def _ranks_from_starts(n, starts):
    at = np.zeros(n, dtype=np.int64)
    at[np.asarray(starts, dtype=np.int64)] = np.asarray(starts, dtype=np.int64)
    return np.maximum.accumulate(at).astype(np.uint32)


RANK_CASES = [(f"equal_{n}", n, [0]) for n in (1, 63, 64, 65, 255, 256, 257, 513)] + [
    ("distinct", 513, list(range(513))),
    ("lane_0_and_tile_first", 700, [0, 64, 192, 256, 512]),
    ("lane_63_and_tile_last", 700, [0, 63, 255, 511]),
    ("neighbouring_edges", 700, [0, 63, 64, 255, 256, 511, 512]),
    ("one_run_over_tiles_1_to_3", 1300, [0, 200, 1100]),      # (the fill pass with a carry from more than two tiles back)
]


@pytest.mark.parametrize("name, n, starts", RANK_CASES, ids=[c[0] for c in RANK_CASES])
def test_ranks_with_runs_on_lane_wave_and_tile_edges(gpu_ctx, monkeypatch, name, n, starts):
    """k_abundance_rank / _carry / _fill, read through k_lines_build<4>: sequences of 65 nt, so that the anchored build runs"""
    monkeypatch.delenv(WIDTH_HOOK, raising=False)
    rng = np.random.default_rng(2000 + n + len(starts))
    db = _fixed_db(rng, n, 65, _abundance(n, starts))
    _check_ranks_and_lines(gpu_ctx, db, name, _ranks_from_starts(n, starts))


@pytest.mark.parametrize("name", ["runs_on_the_turn_edge", "one_run_across_the_turn_edge"])
def test_ranks_across_the_turns_of_the_carry_kernel(gpu_ctx, monkeypatch, name):
    """k_abundance_rank_carry takes 2048 tiles a turn: nothing below 524 288 amplicons enters its second turn.  Two
    databases of 524 288 + 600, because the two things to see exclude one another at the one edge there is: runs that
    begin at 524 287 (the last amplicon of turn 0) and at 524 288 (the first of turn 1), behind a run of 124 287 that
    ends at 524 286; and one run from 500 000 to 524 288 + 300, whose start the carry has to bring over the edge (and
    over a tile of turn 1).  In front: random runs of 40 on average; behind: 300 distinct abundances."""
    monkeypatch.delenv(WIDTH_HOOK, raising=False)
    rng = np.random.default_rng(31 + len(name))
    n = TURN + 600
    assert TURN == 524288
    body = np.nonzero(rng.random(400000) < 0.025)[0]
    tail = np.arange(n - 300, n)
    if name == "runs_on_the_turn_edge":
        starts = np.concatenate([[0], body, [400000, TURN - 1, TURN], tail])
    else:
        starts = np.concatenate([[0], body, [400000, 500000], tail])
    starts = np.unique(starts)
    db = _fixed_db(rng, n, 65, _abundance(n, starts))
    want = _ranks_from_starts(n, starts)
    assert want[TURN + 299] == (TURN if name == "runs_on_the_turn_edge" else 500000) and want[n - 1] == n - 1
    _check_ranks_and_lines(gpu_ctx, db, name, want)


@pytest.mark.parametrize("longest, quads", [(200, 8), (500, 16)])
def test_lines_of_eight_and_sixteen_quads(gpu_ctx, monkeypatch, longest, quads):
    """k_lines_build<8> / <16>: a few hundred amplicons of 65 .. longest nt: length, rank, words, zeros up to the line's end"""
    monkeypatch.delenv(WIDTH_HOOK, raising=False)
    rng = np.random.default_rng(longest)
    n = 300
    lens = rng.integers(65, longest + 1, n)
    lens[:4] = (longest, 65, longest - 8, 96)
    codes = rng.integers(0, 4, (n, longest), dtype=np.uint8)
    db = _db(codes, lens, _abundance(n, np.unique(np.concatenate([[0], rng.integers(1, n, 60)]))))
    assert M.line_quads_model(db.longest) == quads
    _check_ranks_and_lines(gpu_ctx, db, longest)


# ---------------------------------------------------------------------------------------------- k_db_lengths

EDGES = [160, 161, 256, 257, 480, 481, 672, 673]


def _census_small(rng, n: int) -> S.Db:
    """the eight lengths on the class edges, neighbours of them across the edges (so that there is a network), a random body"""
    rows = [rng.integers(0, 4, L).astype(np.uint8) for L in EDGES]
    long_one, at_160, at_672 = rows[7], rows[0], rows[6]
    sub = long_one.copy(); sub[400] = (sub[400] + 1) & 3
    rows += [sub, np.delete(long_one, 300), np.delete(rows[1], 50), np.insert(at_160, 80, (at_160[80] + 1) & 3),
             np.insert(at_672, 10, (at_672[10] + 2) & 3)]
    rows += [rng.integers(0, 4, int(L)).astype(np.uint8) for L in rng.integers(65, 701, n - len(rows))]
    codes, lens = _matrix(rows)
    return _db(codes, lens, _abundance(n, range(0, n, 3)))


@pytest.mark.parametrize("n", [1, 256, 257])
def test_length_census_on_the_class_edges(gpu_ctx, monkeypatch, n):
    """k_db_lengths: the shortest sequence and the five populations (selector 4); the members beyond 672 nt count in the
    last class, and the network is still the oracle's"""
    monkeypatch.delenv(WIDTH_HOOK, raising=False)
    rng = np.random.default_rng(4000 + n)
    if n == 1:
        db = _db(rng.integers(0, 4, (1, 673), dtype=np.uint8), [673], [1])
    else:
        db = _census_small(rng, n)
    shortest, pops = M.lengths_model(db.seqlen)
    assert pops[4] >= 1 and sum(pops) == n
    _build(gpu_ctx, db)
    facts = gpu_ctx.d1_db_facts()
    assert (facts["shortest"], facts["class_pop"]) == (shortest, pops)
    off, nb = gpu_ctx.d1_network()
    woff, wnb, _ = oracle_sorted_rows(db)
    assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
    assert n == 1 or len(nb) >= 5
    facts = gpu_ctx.d1_db_facts()
    assert (facts["shortest"], facts["class_pop"]) == (shortest, pops)


def test_length_census_when_a_thread_takes_two_amplicons(gpu_ctx, monkeypatch):
    """k_db_lengths runs at most eight workgroups of 256 a compute unit: a database of more amplicons than that many threads.
    Sequences of 65 .. 96 nt (three words each), the edge lengths three times over at the front and at the back."""
    monkeypatch.delenv(WIDTH_HOOK, raising=False)
    threads = 256 * 8 * 256                                   # an MI355X has 256 compute units (a partition of one has fewer)
    rng = np.random.default_rng(4999)
    edge_rows = [rng.integers(0, 4, L).astype(np.uint8) for L in EDGES * 3]
    ecodes, elens = _matrix(edge_rows)
    assert not M.duplicate_rows(ecodes, elens)
    ewords, eoff = M.pack_codes(ecodes, elens)
    split = int(eoff[12])
    nbody = threads + 300 - len(edge_rows)
    blens = rng.integers(65, 97, nbody).astype(np.uint32)
    bwords = rng.integers(0, 1 << 64, (nbody, 3), dtype=np.uint64, endpoint=False)
    third = blens.astype(np.uint64) - np.uint64(64)           # nucleotides in the third word: 1 .. 32
    bwords[:, 2] &= np.where(third == 32, np.uint64(M.MASK64), (np.uint64(1) << (np.uint64(2) * np.minimum(third, np.uint64(31)))) - np.uint64(1))
    assert len(np.unique(bwords.view([("", np.void, 24)]).ravel())) == nbody
    seqlen = np.concatenate([elens[:12], blens, elens[12:]]).astype(np.uint32)
    n = len(seqlen)
    assert n > threads
    nw = (seqlen.astype(np.int64) + 31) // 32
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(nw)
    db = S.Db(headers=[], seqs=np.ascontiguousarray(np.concatenate([ewords[:split], bwords.ravel(), ewords[split:]])), seq_off=off,
              seqlen=seqlen, abundance=np.ones(n, dtype=np.uint64), longest=673)
    assert len(db.seqs) == int(off[-1])
    shortest, pops = M.lengths_model(seqlen)
    assert pops == [n - 21, 6, 6, 6, 3] and shortest == int(blens.min())
    _build(gpu_ctx, db)
    facts = gpu_ctx.d1_db_facts()
    assert (facts["shortest"], facts["class_pop"]) == (shortest, pops)


# ---------------------------------------------------------------------------------------------- the window sample

def _window_set(rng, n: int, groups, short=()) -> tuple:
    """n unrelated sequences of 130 nt; groups: index arrays whose members get one 32-nt prefix each, every eighth member a
    neighbour (one substitution at position 70) of the member before it; short: indices cut to 100 nt"""
    codes = rng.integers(0, 4, (n, 130), dtype=np.uint8)
    for members in groups:
        members = np.asarray(members)
        codes[members, :32] = codes[members[0], :32]
        a, b = members[0:len(members) - 1:8], members[1:len(members):8]
        codes[b] = codes[a]
        codes[b, 70] ^= 1
    lens = np.full(n, 130, dtype=np.uint32)
    lens[np.asarray(short, dtype=np.int64)] = 100
    return codes, lens


def _check_windows(ctx, codes, lens, seeds: int, final: bool, expect):
    """the sample and its choice against the model; the final windows where the safety net's outcome is certain; the
    network of the first `seeds` amplicons against the oracle's"""
    n = len(lens)
    db = _db(codes, lens, 1 + (n - 1 - np.arange(n)) // 7)
    want = M.windows_model(codes, lens, n, int(lens.min()), 1)
    assert (want["stride"], want["samples"], want["mass"], want["too_short"], want["offset"]) == expect     # (what the case was built to hold)
    _build(ctx, db)
    got = ctx.d1_window_sample()
    assert got == want
    if final:
        assert ctx.d1_anchor_windows() == (want["offset"], want["offset"]) and ctx.d1_anchor_width() == want["width"]
    off, nb = ctx.d1_network(False, 0, seeds)
    woff, wnb, _ = oracle_sorted_rows(db, False, 0, seeds)
    assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
    assert ctx.d1_window_sample() == want                     # (the host's copy outlives the scratch it came from)
    return len(nb)


def test_window_sample_of_unrelated_sequences(gpu_ctx, monkeypatch):
    """k_anchor_sample / k_sample_mass: nothing repeats, every mass is 0, the windows stay at the ends.  (The final windows
    are certain here and in every case below that asserts them: no group of the set exceeds the 4096 members the pair
    kernels take, so the first build finds nothing stranded and its safety net does not act.)"""
    monkeypatch.setenv(WIDTH_HOOK, "32")
    rng = np.random.default_rng(51)
    codes, lens = _window_set(rng, 5000, [])
    _check_windows(gpu_ctx, codes, lens, 5000, True, (1, 5000, [0, 0, 0, 0], [0, 0, 5000, 5000], 0))


def test_window_sample_group_cap_edge_at_stride_one(gpu_ctx, monkeypatch):
    """k_sample_mass: 60 000 amplicons (stride 1) with a prefix group of exactly 2048 members — not stranded — and one of
    2049: the mass is 2049, more than 60 000 // 64 = 937, and the windows move to offset 32, where nothing repeats.
    The hook keeps the windows at 32 nt: at the 64 nt a shortest sequence of 130 nt would allow, a shared 32-nt prefix
    makes no group."""
    monkeypatch.setenv(WIDTH_HOOK, "32")
    rng = np.random.default_rng(52)
    codes, lens = _window_set(rng, 60000, [np.arange(0, 2048), np.arange(3000, 3000 + 2049)])
    links = _check_windows(gpu_ctx, codes, lens, 6000, True, (1, 60000, [2049, 0, 0, 0], [0, 0, 60000, 60000], 32))
    assert links >= 500


@pytest.mark.parametrize("members, short, offset", [(1536, 0, 0), (1537, 0, 32), (1537, 1537, 0), (1537, 1536, 32)])
def test_window_sample_share_edge_at_stride_two(gpu_ctx, monkeypatch, members, short, offset):
    """choose_anchor_windows: 196 607 amplicons are sampled at stride 2: 98 304 samples, and a candidate passes with at most
    98 304 // 64 = 1536 of them stranded and at most 1536 too short.  One 32-nt prefix on `members` amplicons at even
    indices (the odd ones unrelated: the sample sees every member): 1536 are stranded (1536 x 2 > 2048) yet few enough,
    the windows stay; 1537 move them.  Only from stride 2 on can this edge be met: at stride 1 a stranded group has more
    than 2048 members and no database sampled at stride 1 has 64 x 2048 amplicons.  With `short` sampled sequences of
    100 nt — too short for offset 32 — mixed in: 1537 of them end the search at candidate 1 (the ends stay, although
    candidate 0 failed), 1536 do not.  (Final windows: asserted except in the last case, where the short sequences go
    unserved under the moved windows and the first build is entitled to second thoughts.)"""
    monkeypatch.setenv(WIDTH_HOOK, "32")
    rng = np.random.default_rng(53 + members + short)
    n = 196607
    group = 2 * np.arange(members)
    shorts = 100000 + 2 * np.arange(short)
    codes, lens = _window_set(rng, n, [group], shorts)
    expect = (2, 98304, [members, 0, 0, 0], [0, short, 98304, 98304], offset)
    links = _check_windows(gpu_ctx, codes, lens, 4000, not (short == 1536), expect)
    assert links >= 150


def test_window_width_follows_the_shortest_sequence(gpu_ctx, monkeypatch):
    """anchor_nwin_for through choose_anchor_windows: 64 c + 1 <= shortest — 1, 2, 2 and 4 words at 128, 129, 256 and 257;
    and SWA_D1_WINDOWS=0 draws no sample"""
    monkeypatch.delenv(WIDTH_HOOK, raising=False)
    rng = np.random.default_rng(54)
    for shortest, words in ((128, 1), (129, 2), (256, 2), (257, 4)):
        codes = rng.integers(0, 4, (40, shortest + 9), dtype=np.uint8)
        lens = np.full(40, shortest + 9, dtype=np.uint32)
        lens[7] = shortest
        db = _db(codes, lens, _abundance(40, [0, 9, 30]))
        want = M.windows_model(codes, lens, 40, shortest, 4)
        assert want["width"] == 32 * words and want["offset"] == 0
        _build(gpu_ctx, db)
        assert gpu_ctx.d1_anchor_width() == 32 * words and gpu_ctx.d1_anchor_windows() == (0, 0)
        assert gpu_ctx.d1_window_sample() == want
        assert gpu_ctx.d1_db_facts()["shortest"] == shortest
    monkeypatch.setenv("SWA_D1_WINDOWS", "0")
    _build(gpu_ctx, db)
    assert gpu_ctx.d1_window_sample() == {"too_short": [0] * 4, "mass": [0] * 4, "stride": 0, "samples": 0, "offset": 0, "width": 32,
                                          "taken": False}
    assert gpu_ctx.d1_anchor_width() == 128 and gpu_ctx.d1_anchor_windows() == (0, 0)
