"""How the -u alignments are divided among the ranks (no GPU): swa_multi_nw_bounds_for against a numpy model.

The rule (include/swarm_amd.h): w_k = seqlen[d_k] + seqlen[q_k], P(k) the sum of w_j over j < k, W = P(npairs);
bounds[0] = 0, bounds[world] = npairs, and for 0 < r < world bounds[r] is the smallest k with P(k) >= floor(r W / world).
The model takes the prefix sums from numpy and the targets in Python integers."""
import numpy as np
import pytest

from swarm_amd import SwaError, capi, nw_bounds_for

WORLDS = [1, 2, 3, 8, 64]


def weights(d, q, seqlen):
    return seqlen[np.asarray(d, dtype=np.int64)].astype(np.uint64) + seqlen[np.asarray(q, dtype=np.int64)].astype(np.uint64)


def model(d, q, seqlen, world):
    P = np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(weights(d, q, seqlen), dtype=np.uint64)))
    W = int(P[-1])
    bounds = [0] + [int(np.searchsorted(P, np.uint64(r * W // world), "left")) for r in range(1, world)] + [len(d)]
    return np.array(bounds, dtype=np.uint64)


def check(d, q, seqlen, world):
    got = nw_bounds_for(d, q, seqlen, world)
    assert got.dtype == np.uint64 and len(got) == world + 1
    assert np.array_equal(got, model(d, q, seqlen, world))
    assert got[0] == 0 and got[-1] == len(d)
    assert np.all(got[1:] >= got[:-1])
    return got


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_lists_follow_the_model(seed, world):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    seqlen = rng.integers(1, 3001, n).astype(np.uint32)
    npairs = int(rng.integers(1, 5000))
    d = rng.integers(0, n, npairs).astype(np.uint32)
    q = rng.integers(0, n, npairs).astype(np.uint32)
    got = check(d, q, seqlen, world)
    # no slice is heavier than its even share, the pair that crosses the boundary and the floor's rounding
    w = weights(d, q, seqlen)
    P = np.concatenate(([0], np.cumsum(w))).astype(np.uint64)
    W = int(P[-1])
    for r in range(world):
        assert int(P[int(got[r + 1])]) - int(P[int(got[r])]) <= W / world + int(w.max()) + 1


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("npairs", [1, 7, 64, 1000, 1001])
def test_equal_pairs_give_even_counts(npairs, world):
    seqlen = np.full(5, 150, dtype=np.uint32)
    d = np.arange(npairs, dtype=np.uint32) % 5
    q = (d + 1) % 5
    got = check(d, q, seqlen, world)
    counts = np.diff(got.astype(np.int64))
    assert counts.max() - counts.min() <= 1


@pytest.mark.parametrize("world", WORLDS)
def test_no_pairs_give_zeros(world):
    seqlen = np.array([10, 20], dtype=np.uint32)
    empty = np.zeros(0, dtype=np.uint32)
    assert np.array_equal(nw_bounds_for(empty, empty, seqlen, world), np.zeros(world + 1, dtype=np.uint64))
    # (no array is read then: null pointers are accepted)
    lib = capi.load_library()
    out = np.full(world + 1, 9, dtype=np.uint64)
    assert lib.swa_multi_nw_bounds_for(0, None, None, None, 0, world, out.ctypes.data) == capi.SWA_OK
    assert not out.any()


@pytest.mark.parametrize("world", [2, 3, 8, 64])
@pytest.mark.parametrize("npairs", [1, 2, 3])
def test_fewer_pairs_than_ranks_leave_slices_empty(npairs, world):
    rng = np.random.default_rng(10 * world + npairs)
    seqlen = rng.integers(1, 3001, 6).astype(np.uint32)
    d = rng.integers(0, 6, npairs).astype(np.uint32)
    q = rng.integers(0, 6, npairs).astype(np.uint32)
    got = check(d, q, seqlen, world)
    counts = np.diff(got.astype(np.int64))
    assert counts.sum() == npairs
    if npairs < world:
        assert (counts == 0).sum() >= world - npairs


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("where", [0, 17, 99])
def test_one_pair_heavier_than_all_the_others(where, world):
    seqlen = np.array([1, 3000], dtype=np.uint32)              # 99 pairs of weight 2, one of 6000
    d = np.zeros(100, dtype=np.uint32)
    q = np.zeros(100, dtype=np.uint32)
    d[where] = q[where] = 1
    got = check(d, q, seqlen, world)
    # the heavy pair is one rank's; nobody else's slice weighs more than the light pairs together
    w = weights(d, q, seqlen)
    for r in range(world):
        lo, hi = int(got[r]), int(got[r + 1])
        if not lo <= where < hi:
            assert int(w[lo:hi].sum()) <= 2 * 99


@pytest.mark.parametrize("world", [2, 3, 8, 64])
def test_large_weights_and_many_pairs(world):
    """2^20 pairs of weights near 2^28 + 2^28: W is near 2^49 and r W near 2^55 — past what a double holds exactly; the
    library forms floor(r W / world) from W / world and W % world, never the product."""
    rng = np.random.default_rng(5)
    seqlen = ((1 << 28) - rng.integers(0, 1000, 64)).astype(np.uint32)
    npairs = 1 << 20
    d = rng.integers(0, 64, npairs).astype(np.uint32)
    q = rng.integers(0, 64, npairs).astype(np.uint32)
    got = check(d, q, seqlen, world)
    counts = np.diff(got.astype(np.int64))
    assert counts.max() - counts.min() <= 2                    # (weights within 2000 of each other in 2^29)


def test_refusals():
    seqlen = np.array([10, 20, 30], dtype=np.uint32)
    d = np.array([0, 1, 2], dtype=np.uint32)
    q = np.array([2, 1, 0], dtype=np.uint32)
    assert len(nw_bounds_for(d, q, seqlen, 64)) == 65
    for world in (0, 65, 1 << 20):
        with pytest.raises(SwaError) as e:
            nw_bounds_for(d, q, seqlen, world)
        assert e.value.code == capi.SWA_E_ARG
    for bad in (3, 4, 0xFFFFFFFF):                             # an id >= n, in either list, at any place
        for lst in (0, 1):
            for at in range(3):
                ids = [d.copy(), q.copy()]
                ids[lst][at] = bad
                with pytest.raises(SwaError) as e:
                    nw_bounds_for(ids[0], ids[1], seqlen, 2)
                assert e.value.code == capi.SWA_E_ARG
    lib = capi.load_library()
    out = np.zeros(3, dtype=np.uint64)
    for args in ((3, None, q.ctypes.data, seqlen.ctypes.data), (3, d.ctypes.data, None, seqlen.ctypes.data),
                 (3, d.ctypes.data, q.ctypes.data, None)):
        assert lib.swa_multi_nw_bounds_for(*args, 3, 2, out.ctypes.data) == capi.SWA_E_ARG
    assert lib.swa_multi_nw_bounds_for(3, d.ctypes.data, q.ctypes.data, seqlen.ctypes.data, 3, 2, None) == capi.SWA_E_ARG
