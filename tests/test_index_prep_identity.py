"""The models of tests/index_prep_model.py against independent ground, without a GPU: the hash and the two XOR streams
against the oracle's hash and microvariants (the reference's zobrist.cc / variants.cc), the rank model against a walk over
the runs, the length census against a loop, the window model on hand-built sets whose statistics can be counted by eye,
the line model against the database it was made from.  tests/test_index_prep_gpu.py then puts k_seqhash, the
k_abundance_rank passes, k_db_lengths, k_anchor_sample / k_sample_mass / choose_anchor_windows and k_lines_build in front
of these models."""
import numpy as np
import pytest

import index_prep_model as M
import support as S

ZLEN = 80


@pytest.fixture(scope="module")
def zob():
    tab = S.oracle_zobrist(ZLEN)
    tab.setflags(write=False)
    return tab


def _hash(zob, s: str) -> int:
    w = S.pack_seq(s.encode())
    return int(S.oracle().orc_zobrist_hash(S._p(zob, S.u64p), S._p(w, S.u64p), len(s)))


def _aux(zob, s: str, anchor_w: int) -> dict:
    w = S.pack_seq(s.encode()) if s else np.zeros(1, dtype=np.uint64)
    return M.aux_model(w, len(s), zob, anchor_w)


SHORT = ["A", "AC", "AAAA", "ACGTTTGCA", "GGGGGGCCCCCCAT", "ACACACACACACACACACACACACACACACACACAC",
         "TTGACCAGGTTTTTTTTTTTTTTTTTTTTTTTTTTTTTACGGA"]


def test_hash_is_the_oracles(zob):
    rng = np.random.default_rng(5)
    seqs = SHORT + ["".join(rng.choice(list("AC" if t % 3 == 0 else "ACGT"), int(rng.integers(1, 70)))) for t in range(60)]
    for s in seqs:
        assert _aux(zob, s, 32)["h"] == _hash(zob, s), s


@pytest.mark.parametrize("s", SHORT)
def test_streams_give_the_hash_behind_a_deletion_or_an_insertion_at_every_position(zob, s):
    """dall is the hash of everything behind a deleted position 0, iall of everything behind a nucleotide inserted in
    front: with the prefixes' own streams taken off, they give the hash of the sequence behind an edit anywhere.  Checked
    against the oracle's hash of the edited sequence at EVERY position, and against the oracle's microvariants where the
    reference lists one (deletions at the first position of a run, insertions that do not repeat the nucleotide before)."""
    L = len(s)
    full = _aux(zob, s, 32)
    listed = {(pos, typ, base): h for h, pos, typ, base in S.oracle_variants(zob, S.pack_seq(s.encode()), L, full["h"])}
    seen = 0
    for i in range(L):                                        # position i deleted
        head, upto = _aux(zob, s[:i], 32), _aux(zob, s[:i + 1], 32)
        got = head["h"] ^ full["dall"] ^ upto["dall"]
        if L > 1:
            assert got == _hash(zob, s[:i] + s[i + 1:]), (s, i)
        if (i, 1, 0) in listed:
            assert got == listed[(i, 1, 0)], (s, i)
            seen += 1
    for i in range(L + 1):                                    # base b inserted in front of position i
        head = _aux(zob, s[:i], 32)
        for b in range(4):
            got = head["h"] ^ int(zob[4 * i + b]) ^ full["iall"] ^ head["iall"]
            assert got == _hash(zob, s[:i] + "ACGT"[b] + s[i:]), (s, i, b)
            if (i, 2, b) in listed:
                assert got == listed[(i, 2, b)], (s, i, b)
                seen += 1
    runs = 1 + sum(1 for p in range(1, L) if s[p] != s[p - 1])
    assert seen == runs + 4 + 3 * L                           # every deletion and insertion the reference lists was met


@pytest.mark.parametrize("s", SHORT)
def test_restricted_streams_split_the_full_ones_at_the_run_start(zob, s):
    """for every window width 1 .. L + 2: pb by a direct search, the restricted streams are the streams of the prefix of
    pb nucleotides, and the deletion of the run around the window's end — which the reference lists at pb — is
    a32 ^ (dall ^ d32) with the run's first nucleotide taken off the deletion stream"""
    L = len(s)
    full = _aux(zob, s, 32)
    listed = {(pos, typ): h for h, pos, typ, base in S.oracle_variants(zob, S.pack_seq(s.encode()), L, full["h"])}
    for w in range(1, L + 3):
        a = _aux(zob, s, w)
        assert (a["h"], a["dall"], a["iall"]) == (full["h"], full["dall"], full["iall"])
        if L < w:
            assert a["pb"] == w and (a["a32"], a["d32"], a["i32"]) == (full["h"], full["dall"], full["iall"])
            continue
        starts = [p for p in range(w) if all(c == s[w - 1] for c in s[p:w])]
        assert a["pb"] == min(starts)
        assert a["pb"] == 0 or s[a["pb"] - 1] != s[w - 1]
        head = _aux(zob, s[:a["pb"]], 32)
        assert (a["a32"], a["d32"], a["i32"]) == (head["h"], head["dall"], head["iall"])
        code = "ACGT".index(s[a["pb"]])
        off = int(zob[4 * (a["pb"] - 1) + code]) if a["pb"] >= 1 else 0
        assert a["a32"] ^ a["dall"] ^ a["d32"] ^ off == listed[(a["pb"], 1)], (s, w)


def test_rank_model_is_the_walk_over_the_runs():
    rng = np.random.default_rng(11)
    for n in (1, 2, 63, 64, 65, 257, 1000):
        for style in range(3):
            if style == 0:
                ab = np.full(n, 7, dtype=np.uint64)
            elif style == 1:
                ab = np.arange(n, 0, -1).astype(np.uint64)
            else:
                ab = np.sort(rng.integers(1, max(2, n // 5), n).astype(np.uint64))[::-1].copy()
            assert np.array_equal(M.ranks_model(ab), M.ranks_brute(ab)), (n, style)
    assert M.ranks_model(np.array([9, 9, 5, 5, 5, 1], dtype=np.uint64)).tolist() == [0, 0, 2, 2, 2, 5]


def test_length_census_by_hand():
    lens = [160, 161, 256, 257, 480, 481, 672, 673, 1, 65]
    assert M.lengths_model(lens) == (1, [3, 2, 2, 2, 1])
    assert [M.width_class(v) for v in lens] == [0, 1, 1, 2, 2, 3, 3, 4, 0, 0]
    rng = np.random.default_rng(3)
    body = rng.integers(1, 900, 500)
    want = [0] * 5
    for v in body:
        want[M.width_class(int(v))] += 1
    assert M.lengths_model(body) == (int(body.min()), want)


def test_window_width_from_the_shortest_sequence():
    assert [M.anchor_nwin_model(s, 0, 4) for s in (64, 65, 128, 129, 256, 257, 1000)] == [1, 1, 1, 2, 2, 4, 4]
    assert [M.anchor_nwin_model(s, 0, 2) for s in (128, 129, 257)] == [1, 2, 2]
    assert [M.anchor_nwin_model(s, 0, 1) for s in (129, 257)] == [1, 1]
    assert M.anchor_nwin_model(1000, 32, 4) == 1              # moved windows keep one word


def _distinct(rng, n, length):
    codes = rng.integers(0, 4, (n, length), dtype=np.uint8)
    assert not M.duplicate_rows(codes, np.full(n, length))
    return codes


def test_window_model_counts_what_the_eye_counts(monkeypatch):
    """100 sequences of 130 nt, 40 of them with one 32-nt prefix; the cap lowered so that 40 x stride 1 is stranded and
    20 x stride 2 is judged by its estimate"""
    rng = np.random.default_rng(17)
    codes = _distinct(rng, 100, 130)
    codes[:40, :32] = codes[0, :32]
    lens = np.full(100, 130)
    monkeypatch.setattr(M, "GROUP_CAP", 39)
    got = M.windows_model(codes, lens, 100, 130, 1)
    assert got["stride"] == 1 and got["samples"] == 100
    assert got["too_short"] == [0, 0, 100, 100]               # 130 nt hold offsets 0 and 32 (129), not 64 (193)
    assert got["mass"] == [40, 0, 0, 0]                       # one prefix group of 40 > 39; nothing else repeats
    assert (got["offset"], got["width"]) == (32, 32)          # 40 > 100 // 64: the windows move to the first clean offset
    monkeypatch.setattr(M, "GROUP_CAP", 40)
    got = M.windows_model(codes, lens, 100, 130, 1)
    assert got["mass"] == [0, 0, 0, 0] and (got["offset"], got["width"]) == (0, 32)     # 40 is not more than 40
    got = M.windows_model(codes, lens, 100, 130, 4)
    assert got["mass"] == [0, 0, 0, 0] and (got["offset"], got["width"]) == (0, 64)     # 64-nt windows at the ends: no group
    # the same 40 as a suffix: counted on the suffix side; as both: both sides add up
    codes2 = _distinct(rng, 100, 130)
    codes2[:40, 98:] = codes2[0, 98:]
    monkeypatch.setattr(M, "GROUP_CAP", 39)
    assert M.windows_model(codes2, lens, 100, 130, 1)["mass"] == [40, 0, 0, 0]
    codes2[30:70, :32] = codes2[30, :32]
    assert M.windows_model(codes2, lens, 100, 130, 1)["mass"] == [80, 0, 0, 0]


def test_window_model_under_a_stride_and_with_short_sequences(monkeypatch):
    rng = np.random.default_rng(19)
    n = 2 * 65536 + 10                                        # stride 2: 65541 samples, the even indices
    codes = _distinct(rng, n, 130)
    lens = np.full(n, 130)
    codes[0:80:2, :32] = codes[0, :32]                        # 40 samples share a prefix ...
    codes[1:4001:2, :32] = codes[1, :32]                      # ... 2000 odd ones another: no sample sees them
    monkeypatch.setattr(M, "GROUP_CAP", 79)
    got = M.windows_model(codes, lens, n, 130, 1)
    assert got["stride"] == 2 and got["samples"] == 65541
    assert got["mass"] == [40, 0, 0, 0]                       # 40 x 2 = 80 > 79
    assert (got["offset"], got["width"]) == (0, 32)           # 40 <= 65541 // 64 = 1024: stranded, yet few: the ends stay
    monkeypatch.setattr(M, "GROUP_CAP", 80)
    assert M.windows_model(codes, lens, n, 130, 1)["mass"] == [0, 0, 0, 0]
    # a mass over the limit moves the windows — unless more than samples // 64 samples are too short for the next offset
    codes[0:2100:2, :32] = codes[0, :32]                      # 1050 samples > 1024
    monkeypatch.setattr(M, "GROUP_CAP", 2048)
    got = M.windows_model(codes, lens, n, 130, 1)
    assert got["mass"] == [1050, 0, 0, 0] and got["offset"] == 32
    lens2 = lens.copy()
    lens2[4000:6050:2] = 100                                  # 1025 samples of 100 nt: fine at the ends (65), short at 32 (129)
    got = M.windows_model(codes, lens2, n, 100, 1)
    assert got["too_short"][:2] == [0, 1025] and got["mass"][0] == 1050
    assert (got["offset"], got["width"]) == (0, 32)           # the search stops there: larger offsets only strand more
    lens2[4000] = 130                                         # 1024: few enough
    assert M.windows_model(codes, lens2, n, 100, 1)["offset"] == 32


def test_line_model_lays_out_length_rank_words_and_zeros():
    rng = np.random.default_rng(23)
    for longest, quads in ((65, 4), (160, 4), (161, 8), (480, 8), (481, 16), (1100, 16)):
        lens = np.array([1, 32, 33, longest], dtype=np.int64)
        codes = rng.integers(0, 4, (4, longest), dtype=np.uint8)
        words, off = M.pack_codes(codes, lens)
        ab = np.array([5, 5, 3, 3], dtype=np.uint64)
        lines = M.lines_model(words, off, lens, M.ranks_model(ab), longest)
        assert M.line_quads_model(longest) == quads and lines.shape == (4, 4 * quads)
        assert lines[:, 0].tolist() == lens.tolist() and lines[:, 1].tolist() == [0, 0, 2, 2]
        for i in range(4):
            own = words[int(off[i]):int(off[i + 1])][:2 * quads - 1]
            body = lines[i, 2:].copy().view(np.uint64)
            assert np.array_equal(body[:len(own)], own) and not body[len(own):].any()
            # ... and pack_codes is support.pack_seq
            assert np.array_equal(words[int(off[i]):int(off[i + 1])], S.pack_seq("".join("ACGT"[c] for c in codes[i, :lens[i]]).encode()))
