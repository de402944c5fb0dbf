"""Every form of the key partition of the d = 1 index build, and every bucket regime of k_group1, at small sizes.

Which form the partition takes is decided by the number of records alone (swa_d1_part_plan_for), so sets of a few ten
thousand sequences only ever run one level of a few bits.  SWA_D1_PART_BITS (a test hook, read at every build) sets the bit
count instead: 10 bits are the one wide level of the benchmark size (1024 bins, tiles of 8192 with the histogram taken by
k_keys, tiles of 4096 in a routed build), 11 .. 18 two levels, 19 three.  Every case sets the hook, reads the plan in place
back (Context.d1_part_plan) and compares it with the form it names — a case cannot pass on the default form — and then
compares the network for both cluster-breaking settings with the oracle.  One bit makes two buckets of half the records
each: that is how the four regimes of k_group1 (registers, tail registers, the loop over the records, the whole bucket to
the plain kernel) and the key-overflow retry are reached; the regime is asserted from the bucket starts (selectors 17 / 18
of swa_d1_debug_read)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import support as S
from d1_sets import (build_from_records, conserved_flank_set, giant_group_db, length_mix_db, link_keys, oracle_sorted_rows,
                     route_records, unrelated_db, upload)

pytestmark = pytest.mark.gpu

HOOK = "SWA_D1_PART_BITS"
# forced bits -> [levels, bits of level 0, 1, 2]: one level up to 10 bits, then as few levels of at most 9 as hold them
SPLIT = {1: [1, 1, 0, 0], 3: [1, 3, 0, 0], 9: [1, 9, 0, 0], 10: [1, 10, 0, 0], 11: [2, 6, 5, 0], 18: [2, 9, 9, 0], 19: [3, 7, 6, 6]}
G1_SLOTS, G1_REGISTERS, G1_TAIL, G1_RANKS = 8192, 8192, 10240, 65534      # k_group1: key slots; records in registers, with the tail, with 16-bit ranks


def _form(bits: int, routed: bool = False, extra: int = 0) -> list:
    """what d1_part_plan() reports for `bits` forced bits (extra: added by the key-overflow retry; the last entry)"""
    total = bits + extra
    tile = 2048 if total != 10 else (4096 if routed else 8192)
    return [total] + SPLIT[total] + [tile, 0 if routed else 1, extra]


@functools.lru_cache(maxsize=None)
def _generated(tmp, n=20000, seed=43):
    fa = os.path.join(tmp, f"gen_{n}_{seed}.fa")
    S.gen_fasta(fa, n, 150, seed)
    return S.db_from_fasta(fa)


@functools.lru_cache(maxsize=None)
def _flanks(tmp):
    from pathlib import Path
    fa = Path(tmp) / "flanks.fa"
    conserved_flank_set(fa, 30000, 71)
    return S.db_from_fasta(fa)


_length_mix = functools.lru_cache(maxsize=None)(length_mix_db)
_giant_group = functools.lru_cache(maxsize=None)(giant_group_db)
_unrelated = functools.lru_cache(maxsize=None)(unrelated_db)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("part_forms"))


_ORACLE = {}


def _oracle(name, db, ncb):
    """the oracle's network of a set, computed once and shared by the cases (read-only)"""
    if (name, ncb) not in _ORACLE:
        off, nb, _ = oracle_sorted_rows(db, ncb)
        off.setflags(write=False); nb.setflags(write=False)
        _ORACLE[(name, ncb)] = (off, nb)
    return _ORACLE[(name, ncb)]


def _run_form(ctx, name, db, bits, extra=0):
    """index build under the hook (set by the caller), the form in place, the network for both settings against the oracle"""
    upload(ctx, db)
    assert ctx.d1_index_build() is False
    plan = ctx.d1_part_plan()
    assert plan == _form(bits, extra=extra), (name, bits, plan)
    for which in range(2):
        starts = ctx.d1_bucket_starts(which)
        assert len(starts) == (1 << plan[0]) + 1 and starts[0] == 0 and (np.diff(starts.astype(np.int64)) >= 0).all() and starts[-1] <= db.n
    for ncb in (False, True):
        off, nb = ctx.d1_network(ncb)
        woff, wnb = _oracle(name, db, ncb)
        assert np.array_equal(off, woff), (name, bits, ncb)
        assert np.array_equal(nb, wnb), (name, bits, ncb)
    assert ctx.d1_part_plan() == plan                          # (no rebuild behind the check)
    return plan


@pytest.mark.parametrize("bits", [1, 9, 10, 11, 18, 19])
def test_generated_families_under_every_form(gpu_ctx, tmp, monkeypatch, bits):
    monkeypatch.setenv(HOOK, str(bits))
    _run_form(gpu_ctx, "generated", _generated(tmp), bits)


@pytest.mark.parametrize("bits", [10, 11, 19])
def test_absent_records_and_short_sequences_under_the_wide_and_deep_forms(gpu_ctx, monkeypatch, bits):
    """lengths 20 .. 200: amplicons too short for a window leave absent records in the partition's input"""
    db = _length_mix()
    assert int(db.seqlen.min()) < 32 and int(db.seqlen.max()) >= 200
    monkeypatch.setenv(HOOK, str(bits))
    _run_form(gpu_ctx, "length_mix", db, bits)


@pytest.mark.parametrize("bits", [1, 10])
def test_giant_groups_under_forced_forms(gpu_ctx, monkeypatch, bits):
    monkeypatch.setenv(HOOK, str(bits))
    _run_form(gpu_ctx, "giant_groups", _giant_group(), bits)


def test_conserved_flanks_in_window_mode_under_the_wide_form(tmp, monkeypatch):
    from swarm_amd import Context
    monkeypatch.setenv(HOOK, "10")
    monkeypatch.setenv("SWA_D1_ANCHOR_W", "32")
    ctx = Context(0)
    try:
        _run_form(ctx, "flanks", _flanks(tmp), 10)
        assert ctx.d1_anchor_windows()[0] >= 32                # the windows did move: every build on the way took the forced form
    finally:
        ctx.close()


def test_hook_unset_or_out_of_range_leaves_the_default_form(gpu_ctx, tmp, monkeypatch):
    db = _generated(tmp)
    for value in (None, "0", "28", "x"):
        if value is None:
            monkeypatch.delenv(HOOK, raising=False)
        else:
            monkeypatch.setenv(HOOK, value)
        upload(gpu_ctx, db)
        assert gpu_ctx.d1_index_build() is False
        assert gpu_ctx.d1_part_plan() == _form(1), value       # 20 000 records: one bit


@pytest.mark.parametrize("bits", [10, 11])
@pytest.mark.parametrize("by", ["ids", "records"])
def test_routed_builds_under_the_wide_and_the_two_level_form(tmp, monkeypatch, by, bits):
    """two ranks played in turn by one context; the partial networks of the ranks add up to the oracle's links.  A routed
    build keys from lists whose length the device knows: no histogram by k_keys, so the wide level takes tiles of 4096"""
    from swarm_amd import Context
    db = _generated(tmp)
    world, n = 2, db.n
    woff, wnb = _oracle("generated", db, False)
    whole = link_keys(woff, wnb)
    monkeypatch.setenv(HOOK, str(bits))
    want = _form(bits, routed=True)
    if bits == 10:
        assert want[5] == 4096 and want[6] == 0
    ctx = Context(0)
    try:
        upload(ctx, db)
        parts = []
        if by == "records":
            inbox = route_records(ctx, n, world)
            for rank in range(world):
                ctx.d1_set_ownership(rank, world)
                assert build_from_records(ctx, inbox[rank]) is False
                assert ctx.d1_part_plan() == want, (by, bits, rank)
                parts.append(link_keys(*ctx.d1_network()))
                assert ctx.d1_part_plan() == want
        else:
            cap = 3 * n // (2 * world) + 1024
            bounds = [n * r // world for r in range(world + 1)]
            inbox = [[[], []] for _ in range(world)]
            d_ids, d_counts = S.DeviceArray(2 * world * cap), S.DeviceArray(2 * world + 1)
            for r in range(world):
                ctx.d1_route_slice(bounds[r], bounds[r + 1] - bounds[r], world, d_ids, cap, d_counts)
                counts = d_counts.to_host()
                assert counts[2 * world] == 0
                ids = d_ids.to_host()
                for index in range(2):
                    for owner in range(world):
                        k = index * world + owner
                        inbox[owner][index].append(ids[k * cap: k * cap + counts[k]])
            d_ids.free(); d_counts.free()
            for rank in range(world):
                lists = [np.concatenate(inbox[rank][index]).astype(np.uint32) for index in range(2)]
                bufs = [S.DeviceArray(max(1, len(l))) for l in lists]
                for b, l in zip(bufs, lists):
                    b.from_host(l)
                ctx.d1_set_ownership(rank, world)
                assert ctx.d1_index_build_routed(bufs[0], len(lists[0]), bufs[1], len(lists[1])) is False
                assert ctx.d1_part_plan() == want, (by, bits, rank)
                parts.append(link_keys(*ctx.d1_network()))
                assert ctx.d1_part_plan() == want
                for b in bufs:
                    b.free()
        assert sum(len(p) > 0 for p in parts) == world
        assert np.array_equal(np.sort(np.concatenate(parts)), whole), (by, bits)
    finally:
        ctx.close()


def _bucket_sizes(ctx):
    return [np.diff(ctx.d1_bucket_starts(which).astype(np.int64)) for which in range(2)]


def test_key_overflow_retry_at_index_build(gpu_ctx, monkeypatch):
    """30 400 sequences with as many anchor keys in two buckets: about 15 200 distinct keys each for the 8192 slots of
    k_group1's table, so the build must come back with a finer partition — whichever way the keys fall, one bucket of the
    two holds at least half of them."""
    db = _unrelated()
    assert db.n > 2 * 2 * G1_SLOTS * 0.9
    monkeypatch.setenv(HOOK, "1")
    upload(gpu_ctx, db)
    assert gpu_ctx.d1_index_build() is False
    plan = gpu_ctx.d1_part_plan()
    extra = plan[7]
    assert extra >= 2 and extra % 2 == 0 and plan[0] == 1 + extra and plan[1] == 1 and plan[5] == 2048, plan
    for sizes in _bucket_sizes(gpu_ctx):                       # the buckets of the build that stood: within the table
        assert len(sizes) == 1 << (1 + extra) and sizes.max() <= G1_SLOTS and sizes.sum() <= db.n
    for ncb in (False, True):
        off, nb = gpu_ctx.d1_network(ncb)
        woff, wnb = _oracle("unrelated", db, ncb)
        assert np.array_equal(off, woff) and np.array_equal(nb, wnb), ncb
    assert len(nb) >= 400 and gpu_ctx.d1_part_plan() == plan


def test_key_overflow_retry_inside_the_network_call(monkeypatch):
    """The same overflow met by the index a network call builds for itself (the owner changed in between): the call
    partitions finer and runs again."""
    from swarm_amd import Context
    db = _unrelated()
    ctx = Context(0)
    try:
        monkeypatch.setenv(HOOK, "9")
        upload(ctx, db)
        assert ctx.d1_index_build() is False
        assert ctx.d1_part_plan() == _form(9)                  # 512 buckets of ~60 keys: no retry so far
        monkeypatch.setenv(HOOK, "1")
        ctx.d1_set_ownership(0, 2)
        ctx.d1_set_ownership(0, 1)                             # (the index in place is dropped; this owner's is built by the call)
        off, nb = ctx.d1_network()
        plan = ctx.d1_part_plan()
        assert plan[7] >= 2 and plan[0] == 1 + plan[7] and plan[1] == 1, plan
        woff, wnb = _oracle("unrelated", db, False)
        assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
    finally:
        ctx.close()


@pytest.mark.parametrize("n,lo,hi", [(12000, 0, G1_REGISTERS), (18000, G1_REGISTERS, G1_TAIL), (30000, G1_TAIL, G1_RANKS), (140000, G1_RANKS, 1 << 32)])
def test_group_kernel_bucket_regimes(gpu_ctx, tmp, monkeypatch, n, lo, hi):
    """Two buckets of half the records each: up to 8192 records stay in registers, up to 10240 take the tail registers, up
    to 65534 the loop that rewrites the records, and a bucket beyond 16-bit ranks goes to the plain kernel whole.  The
    larger bucket of each index, read from the bucket starts, names the regime; no retry may have changed the partition.
    (The generated families have about 0.43 n distinct 64-nt anchor windows: a bucket of the 30 000 holds ~15 000 records of
    ~6500 keys.  From ~38 000 sequences on a bucket has more keys than the table's 8192 slots and the build, rightly,
    partitions finer: that is the retry's test, not this one's.)"""
    db = _generated(tmp, n, 45)
    monkeypatch.setenv(HOOK, "1")
    upload(gpu_ctx, db)
    assert gpu_ctx.d1_index_build() is False
    assert gpu_ctx.d1_part_plan() == _form(1)                  # (extra bits 0)
    for which, sizes in enumerate(_bucket_sizes(gpu_ctx)):
        print(f"n {db.n} index {which}: buckets {sizes.tolist()}")
        assert len(sizes) == 2 and sizes.sum() == db.n and lo < sizes.max() <= hi, (which, sizes)
    rng = np.random.default_rng(n)
    for ncb in (False, True):
        off, nb = gpu_ctx.d1_network(ncb)
        if db.n <= 40000:
            woff, wnb = _oracle(("regime", n), db, ncb)
            assert np.array_equal(off, woff) and np.array_equal(nb, wnb), ncb
        else:                                                  # (a seeded sample of row ranges, as the 1 M test takes)
            assert len(off) == db.n + 1 and off[0] == 0 and off[-1] == len(nb) and len(nb) > db.n // 2
            for first in [0, db.n - 2000] + [int(f) for f in rng.integers(0, db.n - 2000, size=3)]:
                woff, wnb, _ = oracle_sorted_rows(db, ncb, first, 2000)
                assert np.array_equal(off[first:first + 2001] - off[first], woff), (ncb, first)
                assert np.array_equal(nb[int(off[first]):int(off[first + 2000])], wnb), (ncb, first)
    assert gpu_ctx.d1_part_plan() == _form(1)


@pytest.mark.parametrize("bits", [10, 19])
def test_indexes_in_hbm_are_consistent_under_forced_forms(bits):
    """tools/check_index.py in a child process: every amplicon once per member list, every work item a set of amplicons
    that share the window, every window group listed once — under the wide and under the three-level form"""
    r = subprocess.run([sys.executable, str(S.ROOT / "tools" / "check_index.py"), "30000"], capture_output=True, text=True,
                       env=dict(os.environ, **{HOOK: str(bits)}))
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert f"key partition: {_form(bits)}" in r.stdout, r.stdout[:400]
