"""tests/bloom_model.py, the model that tests/test_bloom_params_gpu.py holds the Bloom route's filter against, checked
without a GPU: the reciprocal word index of flex_word against the exact remainder, the model against orc_d1_fastidious
(its counters, and no false negative: a pass that probes only the model's tasks finds every graft candidate of the oracle),
filters small enough to count by hand, and the rounding of k = int(0.4 bits)."""
import numpy as np
import pytest

import bloom_model as B
import plain_sets as P
import support as S

# the filter sizes of tests/test_bloom_params_gpu.py's grid (words), by shell_case length and bits
GRID_FSIZES = (2, 4, 7, 22, 91, 3687, 5530, 9218, 29498, 117992, 9382, 14074, 23457, 75062, 300251)
X_TOP = (1 << 48) - 1                                           # h >> 16 of a 64-bit hash


def _sizes() -> list:
    """255 sizes up to 2^40: every size to 64, the powers of two from 2^7 with their neighbours, 90 odd and even ones drawn"""
    out = list(range(1, 65))
    out += [(1 << e) + d for e in range(7, 41) for d in (-1, 0, 1) if (1 << e) + d <= 1 << 40]
    rng = np.random.default_rng(48)
    out += [int(rng.integers(65, 1 << int(rng.integers(8, 41)))) for _ in range(90)]
    assert len(out) == 255 and max(out) == 1 << 40
    return out


def _xs(fsize: int) -> np.ndarray:
    """x on, just above and just below multiples of fsize — the first ones, the last below 2^48, some between — and 2^48 - 1"""
    top_q = X_TOP // fsize
    rng = np.random.default_rng(fsize & 0xFFFFFFFF)
    qs = {0, 1, 2, 3, top_q - 1, top_q, top_q // 2, top_q // 3} | {int(rng.integers(0, top_q + 1)) for _ in range(56)}
    xs = {q * fsize + d for q in qs if q >= 0 for d in (-1, 0, 1)} | {X_TOP, X_TOP - 1, 0}
    return np.array(sorted(x for x in xs if 0 <= x <= X_TOP), dtype=np.uint64)


@pytest.mark.parametrize("sizes", [_sizes(), list(GRID_FSIZES)], ids=["255_sizes_to_2^40", "the_grid's_sizes"])
def test_reciprocal_word_index_is_the_exact_remainder(sizes):
    """flex_word's claim: x < 2^48 is exact in a double, so the quotient from the reciprocal is off by at most one and one
    correction step gives x % fsize.  A failure would be an index outside the filter."""
    wrong = []
    for fsize in sizes:
        xs = _xs(fsize)
        got = B.flex_word_np(xs, fsize)
        want = np.array([int(x) % fsize for x in xs], dtype=np.uint64)          # Python integers: exact
        assert np.array_equal(B.word_index(xs << np.uint64(16), fsize), want)   # the model's own index, too
        wrong += [(fsize, int(x)) for x in xs[got != want]]
    assert not wrong, wrong[:10]


def _probe(db, flags, task_list):
    """the second level on the tasks alone, in strings: every light amplicon one edit from a task's microvariant is a graft
    candidate of the task's heavy amplicon (check_heavy_var_2 / add_graft_candidate: the smallest heavy id wins)"""
    lights = {db.seq_str(int(a)): int(a) for a in np.flatnonzero(np.asarray(flags) != 0)}
    graft = np.full(db.n, P.NO_GRAFT, dtype=np.uint32)
    found = 0
    for t in task_list:
        for w in P.v1(B.variant_string(db, t)):
            amp = lights.get(w)
            if amp is not None:
                found += 1
                graft[amp] = min(int(graft[amp]), int(t["heavy"]))
    return graft, found


@pytest.mark.parametrize("bits", [2, 5, 16, 64])
@pytest.mark.parametrize("L", [2, 31])
def test_model_against_the_oracle(L, bits):
    db, flags, _ = P.shell_case(L)
    want_graft, c = S.oracle_fastidious(db, flags, bits)
    mo = B.flex_model(db, flags, bits)
    assert [mo["light_variants"], mo["heavy_variants"], mo["m"], mo["k"]] == [int(c[0]), int(c[1]), int(c[3]), int(c[4])]
    assert mo["fsize"] == len(mo["words"]) and 0 < mo["tasks"] < mo["heavy_variants"]
    graft, found = _probe(db, flags, mo["task_list"])
    print(f"shells {L} bits {bits}: fsize {mo['fsize']} tasks {mo['tasks']} of {mo['heavy_variants']} candidates {found}")
    assert np.array_equal(graft, want_graft)                     # no false negative among the tasks
    assert found == int(c[2])
    assert (graft != P.NO_GRAFT).sum() >= (100 if L >= 31 else 3)


def test_fewer_bits_never_pass_fewer_variants():
    """the table of the model on shell_case(2) / (31): what passes falls as the filter grows and stays away from all and none"""
    for L, want in ((2, [(2, 92), (4, 84), (7, 75), (22, 74), (91, 74)]), (31, [(3687, 1602), (5530, 1379), (9218, 948), (29498, 709), (117992, 704)])):
        db, flags, _ = P.shell_case(L)
        got = [(mo["fsize"], mo["tasks"]) for mo in (B.flex_model(db, flags, bits) for bits in (2, 3, 5, 16, 64))]
        assert got == want


@pytest.mark.parametrize("light_len,m,n_bytes", [(2, 64, 8), (5, 70, 9)])
def test_the_smallest_filter_by_hand(light_len, m, n_bytes):
    """bits 2: 7 * 2 * 2 = 28 bits are lifted to m = 64, one word; 7 * 2 * 5 = 70 bits are 9 bytes, and 9 >> 3 is still
    one word (the reference truncates).  k = 1, so every microvariant of the light amplicon clears exactly one bit."""
    db, flags = B.hand_case(light_len)
    assert B.sizes(light_len, 2) == (m, n_bytes, 1) and B.k_of(2) == 1
    mo = B.flex_model(db, flags, 2)
    assert [mo["light_nt"], mo["m"], mo["k"], mo["fsize"]] == [light_len, m, 1, 1]
    pat = B.patterns(1)
    assert all(bin(int(p)).count("1") == 1 for p in pat[:4096])
    tab = S.oracle_zobrist(db.longest + 2)
    hashes = [int(h) for h in B.variants_of(db, tab, 1)["hash"]]
    # L substitutions x 3, a deletion per run, an insertion x 4 at the front and x 3 behind every nucleotide
    assert len(hashes) == 3 * light_len + len(P.runs_of(B.HAND[light_len][1])) + 4 + 3 * light_len == mo["light_variants"]
    bit_of = lambda h: int(pat[h & 0xFFFF]).bit_length() - 1      # the one bit of the variant's pattern
    word = int(mo["words"][0])
    assert (word >> bit_of(hashes[0])) & 1 == 0                   # one variant by hand: its bit is cleared,
    cleared = {bit_of(h) for h in hashes}
    assert word == 0xFFFFFFFFFFFFFFFF & ~sum(1 << b for b in cleared)   # and all of them: these bits and no other
    assert 64 - bin(word).count("1") == len(cleared)
    # the graft is found through the filter
    graft, c = S.oracle_fastidious(db, flags, 2)
    assert graft.tolist() == [P.NO_GRAFT, 0] and [int(c[3]), int(c[4])] == [m, 1]
    assert np.array_equal(_probe(db, flags, mo["task_list"])[0], graft)
    assert 0 < mo["tasks"] <= mo["heavy_variants"]


def test_k_rounds_like_the_integer_quotient():
    """int(0.4 * bits) in double precision against floor(2 bits / 5) in integers: 0.4 is below 2/5 in binary, and at bits =
    5, 10, 15, ... the product could fall below the integer"""
    assert [B.k_of(bits) for bits in range(2, 65)] == [max(2 * bits // 5, 1) for bits in range(2, 65)]
    assert B.k_of(2) == 1 and B.k_of(5) == 2 and B.k_of(64) == 25
