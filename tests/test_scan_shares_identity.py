"""Ownership of the pool in the d >= 2 scan divided among several ranks (scan.hip: swa_scan_owner_for, swa_scan_share_for),
as pure functions — no device.  Amplicon i belongs to rank (i >> 5) % world; a rank numbers its amplicons 0, 1, 2, .. and
its kernels walk those local indices, j -> ((j >> 5) * world + rank) << 5 | (j & 31); swa_scan_share_for is what the
launches are sized and started from.  For every n <= 300, every world 1 .. 9 and every lowest_unswarmed 0 .. n + 1:
the shares are disjoint and complete, agree with swa_scan_owner_for, the local-to-global map is a bijection onto the
share, and world 1 is the identity."""
import ctypes as C

import numpy as np
import pytest

from swarm_amd import capi, scan_owner_for, scan_share_for

N_MAX = 300


def local_to_global(j: int, rank: int, world: int) -> int:
    return (((j >> 5) * world + rank) << 5) | (j & 31)


@pytest.mark.parametrize("world", range(1, 10))
def test_shares_partition_the_pool(world):
    lib = capi.load_library()
    capi._declare_multi_scan(lib)
    share_for = lib.swa_scan_share_for
    out = (C.c_uint32 * 2)()
    owner = np.array([scan_owner_for(i, world) for i in range(N_MAX + 2)])
    assert np.array_equal(owner, (np.arange(N_MAX + 2) >> 5) % world)
    # below[r][x] = amplicons with id < x that rank r owns
    below = [np.concatenate(([0], np.cumsum(owner == r))) for r in range(world)]
    for n in range(N_MAX + 1):
        for r in range(world):
            # the local indices 0 .. (share of [0, n)) - 1 map onto the rank's ids below n, in ascending order
            assert share_for(n, 0, r, world, out) == capi.SWA_OK
            mine = np.flatnonzero(owner[:n] == r)
            assert out[0] == len(mine), (n, r)
            assert [local_to_global(j, r, world) for j in range(len(mine))] == mine.tolist(), (n, r)
        for lo in range(n + 2):
            total, firsts = 0, []
            for r in range(world):
                assert share_for(n, lo, r, world, out) == capi.SWA_OK
                cut = min(lo, n)
                count = int(below[r][n] - below[r][cut])
                assert out[0] == count, (n, lo, r)
                # the share starts at local index (owned ids below lo) and that index maps to its first id
                first = local_to_global(int(below[r][cut]), r, world) if count else n
                assert out[1] == first, (n, lo, r, out[1], first)
                if count:
                    assert first >= lo and owner[first] == r and not np.any(owner[cut:first] == r)
                    firsts.append(first)
                total += count
            assert total == n - min(lo, n), (n, lo)                     # complete; disjoint: every id has one owner
            assert len(set(firsts)) == len(firsts)


def test_world_one_is_the_identity():
    for n in range(N_MAX + 1):
        for lo in range(n + 2):
            count, first = scan_share_for(n, lo, 0, 1)
            assert (count, first) == (n - min(lo, n), min(lo, n))
    assert all(scan_owner_for(i, 1) == 0 and local_to_global(i, 0, 1) == i for i in range(4096))


def test_share_for_refuses_a_rank_outside_the_world():
    for rank, world in ((0, 0), (1, 1), (9, 9)):
        with pytest.raises(capi.SwaError):
            scan_share_for(100, 0, rank, world)
    # ids near 2^32 stay in range
    n = 0xFFFFFFFF
    counts = [scan_share_for(n, n - 100, r, 8) for r in range(8)]
    assert sum(c for c, _ in counts) == 100
    assert all(first == n or (n - 100 <= first < n and scan_owner_for(first, 8) == r) for r, (_, first) in enumerate(counts))
