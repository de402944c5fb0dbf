"""The forms of the two partitions of the d = 1 step as pure functions (swa_d1_part_plan_for, swa_d1_csr_plan_for:
host_tables.cpp, no device) at the record counts where the form changes.  The launches read the same functions, so what is
asserted here is what build_stream_index and csr_from_chunks run.  The expected values are worked out below from the rule
itself, not by asking the library twice.

Key partition.  bits = the smallest b >= 1 with (records >> b) <= 10240, at most 27; SWA_D1_PART_BITS replaces it; the
bits of a key-overflow retry are added; at most 27 in all.  Up to 10 bits are one level (10: the wide level of 1024 bins,
tiles of 8192 records, 4096 when the build is routed); more are ceil(bits / 9) levels of at most 9 bits, the earlier levels
one bit wider where the bits do not divide, in tiles of 2048.  k_keys takes the first histogram unless the build is routed.

Link side.  nbits = the smallest b >= 1 with 2^b >= count; r = min(8, nbits - 1), and 9 (never more than nbits - 18)
where r = 8 would need a third level; the nbits - r bits are spread over levels of at most 9 as above."""
import pytest

from swarm_amd import capi

TARGET = 10240          # records a bucket of the key partition holds at most, on average (k_group1)


def _levels(bits: int, most: int = 9) -> list:
    """bits over as few levels of at most `most` as hold them, the earlier ones wider: [levels, b0, b1, b2]"""
    n = -(-bits // most)
    split = [bits // n + (1 if l < bits % n else 0) for l in range(n)]
    assert sum(split) == bits and max(split) <= most and max(split) - min(split) <= 1 and split == sorted(split, reverse=True)
    return [n] + split + [0] * (3 - n)


def _expected_part(records: int, extra: int = 0, routed: bool = False, forced: int = 0) -> list:
    bits = forced
    if not forced:
        bits = 1
        while bits < 27 and (records >> bits) > TARGET:
            bits += 1
    bits = min(bits + extra, 27)
    wide = bits == 10
    tile = (4096 if routed else 8192) if wide else 2048
    return [bits] + _levels(bits, 10 if bits <= 10 else 9) + [tile, 0 if routed else 1, 1 if wide else 0]


def test_the_record_counts_where_the_key_partition_changes_its_form():
    # 512 buckets of 10240 records and one record more: the last size of 9 bits, the first of 10
    assert 5_243_391 >> 9 == TARGET and 5_243_392 >> 9 == TARGET + 1 and 10_486_783 >> 10 == TARGET and 10_486_784 >> 10 == TARGET + 1
    assert capi.part_plan_for(5_243_391) == [9, 1, 9, 0, 0, 2048, 1, 0]
    assert capi.part_plan_for(5_243_392) == [10, 1, 10, 0, 0, 8192, 1, 1]
    assert capi.part_plan_for(5_243_392, routed=True) == [10, 1, 10, 0, 0, 4096, 0, 1]
    assert capi.part_plan_for(10_486_783) == [10, 1, 10, 0, 0, 8192, 1, 1]
    assert capi.part_plan_for(10_486_783, routed=True) == [10, 1, 10, 0, 0, 4096, 0, 1]
    assert capi.part_plan_for(10_486_784) == [11, 2, 6, 5, 0, 2048, 1, 0]
    assert capi.part_plan_for(10_486_784, routed=True) == [11, 2, 6, 5, 0, 2048, 0, 0]
    assert capi.part_plan_for(10_000_000) == [10, 1, 10, 0, 0, 8192, 1, 1]          # the benchmark
    assert capi.part_plan_for(100_000_000) == [14, 2, 7, 7, 0, 2048, 1, 0]
    # a key-overflow retry at 10 M: 10 + 2 bits are two levels of 6
    assert capi.part_plan_for(10_000_000, extra_bits=2) == [12, 2, 6, 6, 0, 2048, 1, 0]
    for records in (0, 1, 20_000, 20_480, 20_481, 5_243_391, 5_243_392, 10_486_783, 10_486_784, 10_000_000, 100_000_000, 1 << 32, (1 << 40) + 5):
        for extra in (0, 2, 4, 8):
            for routed in (False, True):
                assert capi.part_plan_for(records, extra, routed) == _expected_part(records, extra, routed), (records, extra, routed)
    assert capi.part_plan_for(20_480)[0] == 1 and capi.part_plan_for(20_481)[0] == 1 and capi.part_plan_for(40_962)[0] == 2
    assert capi.part_plan_for((1 << 40) + 5)[:5] == [27, 3, 9, 9, 9]                 # (never more than three levels of 512 bins)


@pytest.mark.parametrize("forced,levels,split", [(1, 1, [1, 0, 0]), (9, 1, [9, 0, 0]), (10, 1, [10, 0, 0]), (11, 2, [6, 5, 0]),
                                                 (18, 2, [9, 9, 0]), (19, 3, [7, 6, 6]), (27, 3, [9, 9, 9])])
def test_forced_bits_stand_in_for_the_record_count(forced, levels, split):
    for records in (1, 20_000, 10_000_000, 100_000_000):
        for routed in (False, True):
            got = capi.part_plan_for(records, 0, routed, forced)
            assert got[:5] == [forced, levels] + split, (records, routed)
            assert got == _expected_part(records, 0, routed, forced)
            assert got[5] == (2048 if forced != 10 else (4096 if routed else 8192)) and got[6] == (0 if routed else 1) and got[7] == (forced == 10)
    # the retry's bits come on top of the forced ones, and the sum stops at 27
    assert capi.part_plan_for(20_000, 2, False, 1) == [3, 1, 3, 0, 0, 2048, 1, 0]
    assert capi.part_plan_for(20_000, 2, False, 8) == [10, 1, 10, 0, 0, 8192, 1, 1]
    assert capi.part_plan_for(20_000, 2, False, 10) == [12, 2, 6, 6, 0, 2048, 1, 0]
    assert capi.part_plan_for(20_000, 8, False, 27)[:5] == [27, 3, 9, 9, 9]
    for forced in range(1, 28):
        for extra in (0, 2, 8):
            assert capi.part_plan_for(12_345, extra, False, forced) == _expected_part(12_345, extra, False, forced)
    with pytest.raises(capi.SwaError):
        capi.part_plan_for(20_000, 0, False, 28)


def _expected_csr(count: int) -> list:
    nbits = 1
    while nbits < 32 and (1 << nbits) < count:
        nbits += 1
    r = min(8, nbits - 1)
    if nbits - r > 18:
        r = min(9, nbits - 18)
    return [nbits, r] + _levels(nbits - r)


def test_the_row_counts_where_the_link_partition_changes_its_form():
    assert capi.csr_plan_for(1) == [1, 0, 1, 1, 0, 0]
    assert capi.csr_plan_for(2) == [1, 0, 1, 1, 0, 0]
    assert capi.csr_plan_for(512) == [9, 8, 1, 1, 0, 0]
    assert capi.csr_plan_for(1 << 17) == [17, 8, 1, 9, 0, 0]                         # 512 buckets of 256 rows: the last one-level size
    assert capi.csr_plan_for((1 << 17) + 1) == [18, 8, 2, 5, 5, 0]
    assert capi.csr_plan_for(1 << 26) == [26, 8, 2, 9, 9, 0]                         # the last size with 256 rows a bucket
    assert capi.csr_plan_for((1 << 26) + 1) == [27, 9, 2, 9, 9, 0]                   # 512 rows a bucket instead of a third level
    assert capi.csr_plan_for(1 << 27) == [27, 9, 2, 9, 9, 0]
    assert capi.csr_plan_for((1 << 27) + 1) == [28, 9, 3, 7, 6, 6]
    assert capi.csr_plan_for((1 << 32) - 1) == [32, 9, 3, 8, 8, 7]
    for count in (1, 2, 3, 255, 256, 257, 511, 512, 513, 65537, 1 << 17, (1 << 17) + 1, 1 << 26, (1 << 26) + 1, 1 << 27, (1 << 27) + 1,
                  1 << 31, (1 << 31) + 1, (1 << 32) - 1):
        got = capi.csr_plan_for(count)
        assert got == _expected_csr(count), count
        nbits, r, levels = got[:3]
        assert (1 << nbits) >= count and sum(got[3:]) == nbits - r and r <= 9 and levels <= 3
    with pytest.raises(capi.SwaError):
        capi.csr_plan_for(0)
