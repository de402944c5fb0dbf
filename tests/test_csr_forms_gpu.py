"""The link partition and the row kernels of the d = 1 step (csr_from_chunks: k_part_* with spanning tiles, k_csr_bucket<8>,
k_csr_bucket<9>, k_csr_bucket_big) through swa_d1_csr_from_lists on synthetic link lists, against numpy: neighbours by a
lexsort over (source, target), offsets by bincount + cumsum.  The lists are laid out so that rows and buckets fall on both
sides of every limit at which the kernels change their way:

  rows     4|5, 8|9, 16|17 (register networks), 64|65 (rank sort | odd-even sort in LDS) in a wave's bucket; 32|33 (insertion
           sort | a wave) in a workgroup's bucket; 2048|2049 (through a quarter of LDS | in place in the neighbour array)
  buckets  1024|1025 links (a wave | a workgroup), 8192|8193 (staged in LDS | placed in the neighbour array)
  targets  0, 2^31 - 1, 2^31, 0xFFFFFFFF (the padding of the register networks) and a repeated link, in every sorter
  count    2^17 | 2^17 + 1 (one | two levels), 2^26 | 2^26 + 1 (256 | 512 rows a bucket), 2^27 + 1 (three levels); the plan is
           checked with swa_d1_csr_plan_for
  lists    1 .. 20000 of 0 .. 3 links (tiles that span hundreds of lists; k_part_tiles<256> | <1024> at 2048 | 2049, its
           second round at 8192 | 8193), and lists of ~1000 links (a tile touches 4 | 5 of them)
  first    sources in the top of the 32-bit range"""
import time

import numpy as np
import pytest

import support as S
from swarm_amd import capi
from swarm_amd.capi import SWA_E_CAPACITY, SwaError

pytestmark = pytest.mark.gpu

GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD32 = np.uint32(0xA5A5A5A5)
SPECIAL = np.array([0, (1 << 31) - 1, 1 << 31, 0xFFFFFFFF], dtype=np.uint64)


def _lay_out(keys, counts, rng):
    """the lists one after the other in one buffer, 0 .. 2 foreign words in front of each: (buffer, starts)"""
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.sum() == len(keys)
    gaps = rng.integers(0, 3, size=len(counts))
    starts = np.cumsum(gaps + np.concatenate([[0], counts[:-1]]))
    buf = np.full(int(starts[-1] + counts[-1]) + 3 if len(counts) else 3, GUARD, dtype=np.uint64)
    before = np.cumsum(counts) - counts
    buf[np.repeat(starts - before, counts) + np.arange(len(keys))] = keys
    return buf, starts


def _check_csr(ctx, keys, counts, first, count, rng, sparse=False, caps=None):
    """swa_d1_csr_from_lists over the lists (keys in list order, counts per list) against numpy.  caps: the capacities to
    call with in turn (default: half the need, then room).  sparse: the offsets are compared where they rise — with the
    first and the last that fixes every one of them — instead of entry for entry (counts of 10^8 rows)."""
    keys = np.asarray(keys, dtype=np.uint64)
    total = len(keys)
    rows = (keys >> np.uint64(32)).astype(np.int64) - first
    assert total == 0 or (rows.min() >= 0 and rows.max() < count)
    tgt = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    order = np.lexsort((tgt, rows))
    want_nb, rows = tgt[order], rows[order]
    buf, starts = _lay_out(keys, counts, rng)
    d_links, d_off, d_nb = S.DeviceArray(len(buf), np.uint64), S.DeviceArray(count + 2, np.uint64), S.DeviceArray(total + 8, np.uint32)
    try:
        d_links.from_host(buf)
        for cap in caps if caps is not None else (total // 2, total + 3):
            d_off.from_host(np.full(count + 2, GUARD))
            d_nb.from_host(np.full(total + 8, GUARD32))
            if cap < total:
                with pytest.raises(SwaError) as e:
                    ctx.d1_csr_from_lists(d_links, starts, counts, first, count, d_off, d_nb, cap)
                assert e.value.code == SWA_E_CAPACITY and e.value.total == total
            else:
                assert ctx.d1_csr_from_lists(d_links, starts, counts, first, count, d_off, d_nb, cap) == total
            off, nb = d_off.to_host(), d_nb.to_host()
            assert off[count + 1] == GUARD and off[0] == 0 and off[count] == total, (first, count, cap)
            if sparse:
                rise = np.flatnonzero(np.diff(off[:count + 1]))
                have, per_row = np.unique(rows, return_counts=True)
                assert np.array_equal(rise, have), (first, count, cap)
                assert np.array_equal(off[rise + 1], np.cumsum(per_row).astype(np.uint64)), (first, count, cap)
            else:
                want_off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=count))]).astype(np.uint64)
                assert np.array_equal(off[:count + 1], want_off), (first, count, cap)
            assert np.all(nb[min(cap, total):] == GUARD32), (first, count, cap)
            if cap >= total:
                bad = np.flatnonzero(nb[:total] != want_nb)
                assert len(bad) == 0, (first, count, cap, len(bad), int(bad[0]), int(rows[bad[0]]))
    finally:
        d_links.free(); d_off.free(); d_nb.free()


def _links_of_rows(first, row_ids, row_lens, rng, low_bits=32):
    """row_lens[i] links from source first + row_ids[i], random targets of low_bits bits (repeats allowed)"""
    src = np.repeat(np.asarray(row_ids, dtype=np.uint64) + np.uint64(first), row_lens)
    return (src << np.uint64(32)) | rng.integers(0, 1 << low_bits, size=len(src), dtype=np.uint64)


def _in_order(keys, order, rng):
    return np.sort(keys)[::-1].copy() if order == "descending" else keys[rng.permutation(len(keys))]


def _split(keys, nlists, rng):
    cuts = np.sort(rng.integers(0, len(keys) + 1, size=nlists - 1))
    return np.diff(np.concatenate([[0], cuts, [len(keys)]]))


def _bucket_rows(bucket, lens, rng, rows=256):
    """rows of a bucket for the row lengths `lens`: its first and its last row among them"""
    ids = np.concatenate([[0, rows - 1], 1 + rng.permutation(rows - 2)])[:len(lens)]
    return bucket * rows + ids


WAVE_LENS = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65] * 2          # 750 links: one wave's bucket
FULL_WAVE_LENS = [100] + [4] * 231                                                        # exactly 1024, one row beyond 64
JUST_BIG_LENS = [32] * 16 + [33] * 15 + [18]                                              # exactly 1025: a workgroup's bucket
LAST_BUCKET = {"8192": [2, 32, 33, 64, 65, 2048, 2049, 3899],                             # exactly 8192: still staged in LDS
               "8193+": [0, 1, 2, 2048, 2049, 4097]}                                      # 8197: placed and sorted in the neighbour array


@pytest.mark.parametrize("order", ["descending", "shuffled"])
@pytest.mark.parametrize("last", ["8192", "8193+"])
def test_rows_and_buckets_on_both_sides_of_every_limit(gpu_ctx, last, order):
    rng = np.random.default_rng(len(last) * 2 + len(order))
    count = 1024
    assert capi.csr_plan_for(count) == [10, 8, 1, 2, 0, 0]     # four buckets of 256 rows
    assert sum(WAVE_LENS) < 1024 and sum(FULL_WAVE_LENS) == 1024 and sum(JUST_BIG_LENS) == 1025
    assert sum(LAST_BUCKET["8192"]) == 8192 and sum(LAST_BUCKET["8193+"]) >= 8193
    parts = [_links_of_rows(0, _bucket_rows(b, lens, rng), lens, rng)
             for b, lens in enumerate([WAVE_LENS, FULL_WAVE_LENS, JUST_BIG_LENS, LAST_BUCKET[last]])]
    keys = _in_order(np.concatenate(parts), order, rng)
    per_bucket = np.bincount((keys >> np.uint64(32 + 8)).astype(np.int64), minlength=4)
    assert per_bucket.tolist() == [750, 1024, 1025, sum(LAST_BUCKET[last])]
    _check_csr(gpu_ctx, keys, _split(keys, 3, rng), 0, count, rng)


def _special_row(length, rng, repeat):
    """a row of `length` targets with 0, 2^31 - 1, 2^31 and 0xFFFFFFFF among them; repeat: 0xFFFFFFFF (or, in a row of two,
    whatever comes first) twice"""
    row = np.concatenate([SPECIAL[[3, 2, 0, 1]][:length], rng.integers(0, 1 << 32, size=max(0, length - 4), dtype=np.uint64)])
    if repeat and length >= 2:
        row[-1] = row[0]
    return row[rng.permutation(length)]


def test_targets_at_the_ends_of_the_range_and_repeated_links(gpu_ctx):
    """unsigned order in every sorter; 0xFFFFFFFF is a target like any other although the register networks pad with it; a
    link that comes twice comes out twice"""
    rng = np.random.default_rng(31)
    count = 768                                                # (three of the four buckets of 256 rows exist)
    assert capi.csr_plan_for(count)[:2] == [10, 8]
    buckets = [[2, 3, 4, 5, 8, 13, 16, 17, 40, 64, 65, 100],                   # a wave: networks of 4, 8, 16; rank sort; odd-even sort
               [2, 20, 32, 33, 50, 1500],                                      # a workgroup, staged: insertion sort, a wave a row
               [2, 20, 1500, 2048, 2100, 2600]]                                # a workgroup, in the neighbour array: through LDS, in place
    assert sum(buckets[0]) <= 1024 < sum(buckets[1]) <= 8192 < sum(buckets[2])
    keys = []
    for b, lens in enumerate(buckets):
        for twice in (False, True):                            # every length once with and once without a repeated link
            ids = _bucket_rows(b, lens * 2, rng)[(len(lens) if twice else 0):][:len(lens)]
            for row, length in zip(ids, lens):
                keys.append((np.uint64(row) << np.uint64(32)) | _special_row(length, rng, twice))
    keys = np.concatenate(keys)
    assert len(np.unique(keys)) < len(keys)
    # (every length lies in a bucket twice: what was built, not the sums above, has to fall in the three classes of bucket)
    per_bucket = np.bincount((keys >> np.uint64(40)).astype(np.int64), minlength=3)
    assert per_bucket[0] <= 1024 < per_bucket[1] <= 8192 < per_bucket[2], per_bucket
    keys = keys[rng.permutation(len(keys))]
    _check_csr(gpu_ctx, keys, _split(keys, 4, rng), 0, count, rng)


@pytest.mark.parametrize("count,plan", [(1 << 17, [17, 8, 1, 9, 0, 0]), ((1 << 17) + 1, [18, 8, 2, 5, 5, 0]),
                                        (1 << 26, [26, 8, 2, 9, 9, 0]), ((1 << 26) + 1, [27, 9, 2, 9, 9, 0]),
                                        ((1 << 27) + 1, [28, 9, 3, 7, 6, 6])])
def test_levels_and_rows_per_bucket_by_the_number_of_rows(gpu_ctx, count, plan):
    """about 10^5 links over rows that include the first and the last, both sides of the edge of every first-level bin and of
    thousands of buckets, and random ones.  (The offsets of the two largest counts are 0.5 and 1 GB: compared where they rise.)"""
    assert capi.csr_plan_for(count) == plan
    nbits, r = plan[0], plan[1]
    rng = np.random.default_rng(count % 1000003)
    bin_edges = np.arange(1, 1 << plan[3], dtype=np.int64) << (nbits - plan[3])
    bucket_edges = rng.integers(1, (count + (1 << r) - 1) >> r, size=15000).astype(np.int64) << r
    edges = np.concatenate([bin_edges, bucket_edges])
    rows = np.unique(np.concatenate([[0, count - 1], edges - 1, edges, rng.integers(0, count, size=40000)]))
    rows = rows[rows < count]
    lens = rng.integers(1, 4, size=len(rows))
    lens[rng.integers(0, len(rows), size=3)] = [70, 300, 1500]
    lens[[0, -1]] = [5, 9]
    keys = _links_of_rows(0, rows, lens, rng)
    assert 60000 < len(keys) < 200000
    keys = keys[rng.permutation(len(keys))]
    t0 = time.perf_counter()
    big = count > (1 << 20)
    _check_csr(gpu_ctx, keys, _split(keys, 7, rng), 0, count, rng, sparse=big, caps=(len(keys) + 3,) if big else None)
    print(f"count {count}: {len(keys)} links, plan {plan}, {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("lists", [1, 5, 257, 2048, 2049, 8192, 8193, 20000])
def test_many_short_lists(gpu_ctx, lists):
    """0 .. 3 links a list, empty lists at both ends: one tile of the first level spans hundreds of lists"""
    rng = np.random.default_rng(lists)
    count = 5000
    counts = rng.integers(0, 4, size=lists)
    if lists >= 3:
        counts[[0, 1, -1]] = 0
        counts[2] = 3
    else:
        counts[:] = 3
    total = int(counts.sum())
    rows = rng.integers(0, count, size=total)
    rows[:2] = [0, count - 1]
    keys = (rows.astype(np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 32, size=total, dtype=np.uint64)
    _check_csr(gpu_ctx, keys, counts, 0, count, rng)


def test_tiles_that_touch_four_and_five_lists(gpu_ctx):
    rng = np.random.default_rng(45)
    counts = rng.integers(820, 1400, size=48)
    bounds = np.concatenate([[0], np.cumsum(counts)])
    touched = [int(np.searchsorted(bounds, min(t + 4096, bounds[-1]) - 1, side="right") - np.searchsorted(bounds, t, side="right")) + 1
               for t in range(0, int(bounds[-1]), 4096)]
    assert 4 in touched and 5 in touched and max(touched) <= 6 and len(touched) >= 10, touched   # (kSpanFast = 4: both ways)
    count = 70001
    total = int(counts.sum())
    keys = (rng.integers(0, count, size=total).astype(np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 32, size=total, dtype=np.uint64)
    _check_csr(gpu_ctx, keys, counts, 0, count, rng)


@pytest.mark.parametrize("count", [257, 65537])
@pytest.mark.parametrize("room", [0, 1])
def test_sources_in_the_top_of_the_range(gpu_ctx, count, room):
    """first = 2^32 - count (the last source is 2^32 - 1) and one less: source - first is formed modulo 2^32"""
    first = (1 << 32) - count - room
    rng = np.random.default_rng(count + room)
    lens = rng.integers(0, 5, size=count) * (rng.random(count) < 0.67)
    lens[[0, count - 1]] = [3, 6]
    picks = 1 + rng.permutation(count - 2)[:3]
    lens[picks] = [70, 300, 1500]
    keys = _links_of_rows(first, np.arange(count), lens, rng)
    assert int(keys.max() >> np.uint64(32)) == (1 << 32) - 1 - room and int(keys.min() >> np.uint64(32)) == first
    keys = _in_order(keys, "descending" if room else "shuffled", rng)
    _check_csr(gpu_ctx, keys, _split(keys, 5, rng), first, count, rng)
