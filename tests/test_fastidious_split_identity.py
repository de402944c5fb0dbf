"""SWA_FAST_LONG=split without a GPU: the dispatch as a pure function (swa_d1_fastidious_plan_for, host_tables.cpp)
against the plan restated in tests/fastidious_sets.py, the rule that divides the pairs between the two routes restated
in numpy, and the sets of tests/test_fastidious_split_gpu.py checked on the oracle's result.

The rule (include/swarm_amd.h): with cap the longest sequence k_fast_count's LDS set still serves, the pair route takes
the pairs whose two lengths lie in [112, cap], the Bloom route every other pair; the amplicons the Bloom route lists are
those of len <= 113 or len >= cap - 1.  Two sequences within two edits differ in length by at most 2.

The long set is edit_atlas(1005, 1005, small) (tests/fastidious_split_sets.py: LONG): chosen here, on the oracle's
graft pairs; 1006 is not needed."""
import ctypes as C
import struct

import numpy as np
import pytest

import fastidious_sets as FS
import fastidious_split_sets as SS
import support as S
from swarm_amd import capi


def test_cap_is_the_last_length_the_pair_route_serves():
    serves = [FS.expected_plan(L)[0] for L in range(112, 4001)]
    last = 112 + max(i for i, v in enumerate(serves) if v == 1)
    assert last == SS.CAP == 1004
    assert all(serves[:last - 112 + 1]) and not any(serves[last - 112 + 1:])


def test_plan_for_without_the_split_is_the_restated_plan():
    for longest in range(1, 4001):
        assert capi.fastidious_plan_for(longest) == FS.expected_plan(longest), longest
        assert capi.fastidious_plan_for(longest, bloom=True) == FS.expected_plan(longest, bloom=True), longest
        assert capi.fastidious_plan_for(longest, words=True) == FS.expected_plan(longest, words=True), longest
        # pair_longest is not read without the switch
        assert capi.fastidious_plan_for(longest, pair_longest=150) == FS.expected_plan(longest), longest


def test_plan_for_with_the_split_takes_the_row_of_pair_longest():
    """every longest in 1005 .. 4000 with every pair_longest in 112 .. 1004: expected_plan(pair_longest, words), entry
    [6] from the longest sequence (the raw entry point and one reused buffer: 2.7 M calls)"""
    lib = capi.load_library()
    buf = (C.c_uint32 * 8)()
    want = {}                                                   # (pair_longest, [6]) -> the plan's bytes
    for p in range(SS.MIN_LEN, SS.CAP + 1):
        plan = FS.expected_plan(p, words=True)
        assert plan[0] == 1 and plan[1] == 0
        for z in (0, 1):
            want[(p, z)] = struct.pack("8I", *(plan[:6] + [z] + plan[7:]))
    pairs = range(SS.MIN_LEN, SS.CAP + 1)
    for longest in range(SS.CAP + 1, 4001):
        z = FS.expected_plan(longest)[6]
        for p in pairs:
            assert lib.swa_d1_fastidious_plan_for(longest, p, 1, 0, 0, buf) == 0
            assert bytes(buf) == want[(p, z)], (longest, p, list(buf))
    assert {FS.expected_plan(L)[6] for L in range(SS.CAP + 1, 4001)} == {0, 1}
    # the binding gives the same
    assert capi.fastidious_plan_for(1500, 150, split=True) == FS.expected_plan(150, words=True)
    assert capi.fastidious_plan_for(3071, 1004, split=True) == FS.expected_plan(1004)[:6] + [0, 112]
    assert capi.fastidious_plan_for(3071, 1004, split=True)[3:5] == [1, 16384]


def test_plan_for_with_the_split_where_it_does_not_apply():
    for longest in (1005, 1500, 3070, 3071, 4000):
        for p in (0, 1, 34, 111):                               # nothing for the pair route: all Bloom, as today
            assert capi.fastidious_plan_for(longest, p, split=True) == FS.expected_plan(longest), (longest, p)
        for p in (0, 150, 1004):                                # SWA_FAST_BLOOM=1 wins
            assert capi.fastidious_plan_for(longest, p, split=True, bloom=True) == FS.expected_plan(longest, bloom=True)
    for longest in range(1, SS.CAP + 1):                        # longest <= cap: today's plan, lines kernels included
        for p in (0, 150, longest):
            assert capi.fastidious_plan_for(longest, p, split=True) == FS.expected_plan(longest), (longest, p)
            assert capi.fastidious_plan_for(longest, p, split=True, words=True) == FS.expected_plan(longest, words=True)
    assert capi.fastidious_plan_for(150, 150, split=True)[1] == 5 and capi.fastidious_plan_for(400, 0, split=True)[1] == 13


def test_every_pair_belongs_to_exactly_one_route():
    a, b = np.meshgrid(np.arange(100, 1101), np.arange(100, 1101), indexing="ij")
    near = np.abs(a - b) <= 2
    a, b = a[near], b[near]
    pair, bloom = SS.route_of(a, b)
    assert np.all(pair ^ bloom)
    assert pair.any() and bloom.any()
    # both members of a Bloom-route pair are in the listed bands, so the Bloom route sees the pair
    assert np.all(SS.in_bands(a[bloom]) & SS.in_bands(b[bloom]))
    # ... and the bands are no wider than that: each listed length is half of some Bloom-route pair
    listed = set(np.flatnonzero(SS.in_bands(np.arange(0, 1101))).tolist()) & set(range(100, 1101))
    assert listed == set(a[bloom].tolist()) | set(b[bloom].tolist())
    # without the switch (no upper bound) the rule is today's
    pair0, bloom0 = SS.route_of(a, b, cap=0xFFFFFFFF)
    assert np.array_equal(pair0, np.minimum(a, b) >= 112) and np.array_equal(bloom0, ~pair0)


@pytest.fixture(scope="module")
def oracle_of(tmp_path_factory):
    memo = {}

    def get(name):
        if name not in memo:
            db, flags, three = SS.build(name, tmp_path_factory.mktemp("set") / "in.fa")
            graft, counters = S.oracle_fastidious(db, flags, 16)
            memo[name] = (db, flags, three, graft)
        return memo[name]
    return get


@pytest.mark.parametrize("name", SS.NAMES)
def test_sets_are_worth_running(oracle_of, name):
    db, flags, three, graft = oracle_of(name)
    pairs = SS.graft_pair_lengths(db, graft)
    inside = [p for p in pairs if SS.MIN_LEN <= min(p) and max(p) <= SS.CAP]
    beyond = [p for p in pairs if max(p) > SS.CAP]
    print(name, "n", db.n, "longest", db.longest, "grafts", len(pairs), "inside", len(inside), "beyond", len(beyond))
    if name == "all_long":
        assert int(db.seqlen.min()) > SS.CAP and len(pairs) >= 5 and len(beyond) == len(pairs)
        return
    FS.assert_not_trivial(db, flags, graft, three)
    if name in ("long", "three"):
        assert len(inside) >= 10 and len(beyond) >= 10
        for want in ((1004, 1005), (1003, 1005)):
            assert want in beyond or want[::-1] in beyond, want
        assert db.longest == (SS.LONG if name == "long" else 3071)
        assert max(int(v) for v in db.seqlen if v <= SS.CAP) == SS.CAP          # pair_longest: the 1 wave x 16384 row
    if name == "three":
        short = [p for p in pairs if min(p) < SS.MIN_LEN]
        assert len(short) >= 10 and int((db.seqlen > SS.CAP).sum()) > 100
    if "+" in name:
        assert len(inside) == len(pairs) >= 50 and int((db.seqlen > SS.CAP).sum()) == 1
        assert max(int(v) for v in db.seqlen if v <= SS.CAP) == 150
