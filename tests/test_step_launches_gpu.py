"""The bookkeeping of the d = 1 step that moved into neighbouring launches, at the smallest sizes where it can go wrong:

  starts     k_part_scatter writes the bucket starts of its level (the grid-stride tail behind the tiles): link lists that
             leave nearly every chunk empty, through swa_d1_csr_from_lists against numpy — one level, two levels, and two
             levels with more buckets than the grid has threads — and the key partition's starts under forced forms
  tile table k_keys<true> writes the tile table of a whole-database build: sizes around the tile of 2048 (and of 8192 under
             the wide form); a routed-records build still takes k_part_tiles
  work lists positions inside k_group_lists up to 1024 buckets, the two-launch scan above: both forms on one set with groups
             of every size kind, the form read back (Context.d1_lists_form)
  clears     the head of the status block and the CSR stage's heavy-bucket count cleared with the other counters, the
             count of fallback seeds in the one copy of the head: builds and networks repeated on one context"""
import functools
import os

import numpy as np
import pytest

import support as S
from d1_sets import build_from_records, giant_group_db, link_keys, oracle_sorted_rows, route_records, upload
from swarm_amd import capi

pytestmark = pytest.mark.gpu

HOOK = "SWA_D1_PART_BITS"
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD32 = np.uint32(0xA5A5A5A5)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("step_launches"))


@functools.lru_cache(maxsize=None)
def _records(tmp, n=9000, seed=47):
    """generated 150-nt families, as records: a prefix of them is a database of exactly that many sequences"""
    fa = os.path.join(tmp, f"gen_{n}_{seed}.fa")
    S.gen_fasta(fa, n, 150, seed)
    recs = S.read_fasta(fa)
    assert len(recs) >= 8193
    return recs


@functools.lru_cache(maxsize=None)
def _first(tmp, n):
    db = S.build_db(_records(tmp)[:n])
    assert db.n == n and int(db.seqlen.min()) >= 65            # (every sequence has both windows: n records per index)
    return db


_ORACLE = {}


def _oracle(name, db):
    """the oracle's network of a set, computed once and shared by the cases (read-only)"""
    if name not in _ORACLE:
        off, nb, _ = oracle_sorted_rows(db)
        off.setflags(write=False); nb.setflags(write=False)
        _ORACLE[name] = (off, nb)
    return _ORACLE[name]


def _same_network(ctx, name, db, what):
    off, nb = ctx.d1_network()
    woff, wnb = _oracle(name, db)
    assert np.array_equal(off, woff), what
    assert np.array_equal(nb, wnb), what


# ---- starts from the scatter ----------------------------------------------------------------------------------------

def _csr_against_numpy(ctx, rows, targets, counts, count, sparse=False):
    """swa_d1_csr_from_lists over the lists (links in list order, counts per list; a foreign word between the lists) against
    a CSR built with numpy"""
    rows = np.asarray(rows, dtype=np.int64)
    keys = (rows.astype(np.uint64) << np.uint64(32)) | np.asarray(targets, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.int64)
    total = len(keys)
    assert counts.sum() == total
    starts = np.cumsum(counts) - counts + np.arange(len(counts))
    buf = np.full(total + len(counts) + 3, GUARD, dtype=np.uint64)
    buf[np.repeat(starts - (np.cumsum(counts) - counts), counts) + np.arange(total)] = keys
    order = np.lexsort((np.asarray(targets, dtype=np.uint64), rows))
    want_nb = np.asarray(targets, dtype=np.uint32)[order]
    d_links, d_off, d_nb = S.DeviceArray(len(buf), np.uint64), S.DeviceArray(count + 2, np.uint64), S.DeviceArray(total + 8, np.uint32)
    try:
        d_links.from_host(buf)
        d_off.from_host(np.full(count + 2, GUARD))
        d_nb.from_host(np.full(total + 8, GUARD32))
        assert ctx.d1_csr_from_lists(d_links, starts, counts, 0, count, d_off, d_nb, total + 3) == total
        off, nb = d_off.to_host(), d_nb.to_host()
        assert off[count + 1] == GUARD and off[0] == 0 and off[count] == total
        if sparse:
            rise = np.flatnonzero(np.diff(off[:count + 1]))
            have, per_row = np.unique(rows, return_counts=True)
            assert np.array_equal(rise, have)
            assert np.array_equal(off[rise + 1], np.cumsum(per_row).astype(np.uint64))
        else:
            want_off = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=count))]).astype(np.uint64)
            assert np.array_equal(off[:count + 1], want_off)
        assert np.array_equal(nb[:total], want_nb) and np.all(nb[total:] == GUARD32)
    finally:
        d_links.free(); d_off.free(); d_nb.free()


def test_two_levels_with_three_links_in_the_first_the_middle_and_the_last_row(gpu_ctx):
    count = (1 << 17) + 1
    assert capi.csr_plan_for(count) == [18, 8, 2, 5, 5, 0]     # 32 chunks of 32 buckets: all but three of them empty
    _csr_against_numpy(gpu_ctx, [1 << 16, 1 << 17, 0], [7, 0xFFFFFFFF, 0], [2, 0, 1], count)


def test_two_levels_with_no_link_at_all(gpu_ctx):
    count = (1 << 17) + 1
    _csr_against_numpy(gpu_ctx, [], [], [0, 0], count)


def test_one_level_of_300_rows_with_links_in_the_first_and_the_last_row(gpu_ctx):
    count = 300
    assert capi.csr_plan_for(count) == [9, 8, 1, 1, 0, 0]      # two buckets, fewer than 512 rows
    _csr_against_numpy(gpu_ctx, [299, 0, 299], [5, 9, 1], [1, 2], count)


def test_more_buckets_than_the_grid_has_threads(gpu_ctx):
    """2^21 + 1 rows: the second level leaves 128 x 128 + 1 bucket starts, the grid of a handful of links is 8 workgroups of
    512 threads — every thread writes four or five of them"""
    count = (1 << 21) + 1
    plan = capi.csr_plan_for(count)
    assert plan == [22, 8, 2, 7, 7, 0] and (1 << (plan[3] + plan[4])) + 1 > 8 * 512
    rows = [0, 1 << 20, 1 << 21, (1 << 21) - 1, 255, 256, 257]
    _csr_against_numpy(gpu_ctx, rows, np.arange(len(rows)) * 3, [3, 0, 4], count, sparse=True)


@pytest.mark.parametrize("bits", [1, 10, 11])
def test_bucket_starts_of_the_key_partition_rise_to_the_records_made(gpu_ctx, tmp, monkeypatch, bits):
    db = _first(tmp, 4097)
    monkeypatch.setenv(HOOK, str(bits))
    upload(gpu_ctx, db)
    assert gpu_ctx.d1_index_build() is False
    plan = gpu_ctx.d1_part_plan()
    assert plan[0] == bits and plan[1] == (1 if bits <= 10 else 2), plan
    for which in range(2):
        starts = gpu_ctx.d1_bucket_starts(which).astype(np.int64)
        assert len(starts) == (1 << bits) + 1 and starts[0] == 0 and (np.diff(starts) >= 0).all()
        assert starts[-1] == db.n, (which, bits, starts[-1])   # (every sequence made a record for either index)
    _same_network(gpu_ctx, 4097, db, bits)


# ---- the tile table from k_keys -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,bits", [(2, None), (2047, None), (2048, None), (2049, None), (4097, None), (8193, 10)])
def test_whole_database_builds_around_the_tile(gpu_ctx, tmp, monkeypatch, n, bits):
    """one, one, one | two, three tiles of 2048 records; two of 8192 under the wide form"""
    db = _first(tmp, n)
    if bits is None:
        monkeypatch.delenv(HOOK, raising=False)
    else:
        monkeypatch.setenv(HOOK, str(bits))
    upload(gpu_ctx, db)
    assert gpu_ctx.d1_index_build() is False
    plan = gpu_ctx.d1_part_plan()
    assert plan[5] == (2048 if bits is None else 8192) and plan[6] == 1, plan     # (k_keys took the histogram — and the tile table)
    _same_network(gpu_ctx, n, db, plan)


def test_a_routed_records_build_keeps_k_part_tiles(tmp, monkeypatch):
    """two ranks played in turn by one context, each built from the key records routed to it: the ranks' partial networks add
    up to the links of the whole-database build"""
    from swarm_amd import Context
    db = _first(tmp, 4097)
    whole = link_keys(*_oracle(4097, db))
    monkeypatch.delenv(HOOK, raising=False)
    ctx = Context(0)
    try:
        upload(ctx, db)
        inbox = route_records(ctx, db.n, 2)
        parts = []
        for rank in range(2):
            ctx.d1_set_ownership(rank, 2)
            assert build_from_records(ctx, inbox[rank]) is False
            plan = ctx.d1_part_plan()
            assert plan[5] == 2048 and plan[6] == 0, plan      # (no histogram by k_keys: the partition makes its own tile table)
            parts.append(link_keys(*ctx.d1_network()))
        assert all(len(p) > 0 for p in parts)
        assert np.array_equal(np.sort(np.concatenate(parts)), whole)
    finally:
        ctx.close()


# ---- the work lists' two forms ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _every_size_kind():
    """giant_group_db (one group of 2600, clusters of ~75 and of a few) and 40 pairs: groups of 2, of 3 - 64, of 65 - 256 and
    of more than 256 members in either index"""
    base = giant_group_db()
    seqs = [base.seq_str(i) for i in range(base.n)]
    rng = np.random.default_rng(5)
    for _ in range(40):
        s = "".join(rng.choice(list("ACGT"), size=100))
        seqs += [s, s[:50] + "ACGT"[("ACGT".index(s[50]) + 1) % 4] + s[51:]]
    seqs = sorted(set(seqs))
    db = S.build_db([(f"s{i}_{1 + (i * 13) % 40}".encode(), s.encode()) for i, s in enumerate(seqs)])
    for window in (lambda s: s[:32], lambda s: s[-32:]):
        _, sizes = np.unique([window(db.seq_str(i)) for i in range(db.n)], return_counts=True)
        assert (sizes == 2).any() and ((sizes >= 3) & (sizes <= 64)).any() and ((sizes >= 65) & (sizes <= 256)).any() and (sizes > 256).any()
    return db


def test_work_list_positions_inside_the_kernel_and_by_the_scan(gpu_ctx, monkeypatch):
    db = _every_size_kind()
    assert capi.lists_form_for(1024) == 1 and capi.lists_form_for(1025) == 0 and capi.lists_form_for(2) == 1
    got = {}
    for bits, form in ((10, 1), (11, 0)):
        monkeypatch.setenv(HOOK, str(bits))
        upload(gpu_ctx, db)
        assert gpu_ctx.d1_index_build() is False
        assert gpu_ctx.d1_part_plan()[0] == bits and gpu_ctx.d1_lists_form() == form == capi.lists_form_for(1 << bits)
        counters = gpu_ctx.d1_debug(14, 128).view(np.uint32)
        got[bits] = (gpu_ctx.d1_network(), counters[64:].copy())
        woff, wnb = _oracle("kinds", db)
        assert np.array_equal(got[bits][0][0], woff) and np.array_equal(got[bits][0][1], wnb), bits
    assert np.array_equal(got[10][0][0], got[11][0][0]) and np.array_equal(got[10][0][1], got[11][0][1])
    # (the lists' lengths — the counters from kCounterBase on — do not depend on the number of buckets either)
    assert np.array_equal(got[10][1], got[11][1]) and got[10][1].sum() > 0


# ---- merged clears, one copy --------------------------------------------------------------------------------------------------

def test_builds_and_networks_repeated_on_one_context(tmp, monkeypatch):
    """three index builds + networks, then a network call after the owner changed and changed back (the call builds the index
    itself): the same CSR every time.  The set has buckets of 256 rows with more than 1024 links, so the count of buckets
    left to whole workgroups — cleared with the network call's other counters — is in use every time."""
    from swarm_amd import Context
    db = _every_size_kind()
    woff, wnb = _oracle("kinds", db)
    per_bucket = np.add.reduceat(np.diff(woff.astype(np.int64)), np.arange(0, db.n, 256))
    assert (per_bucket > 1024).any() and (per_bucket <= 1024).any()
    monkeypatch.delenv(HOOK, raising=False)
    ctx = Context(0)
    try:
        upload(ctx, db)
        for turn in range(3):
            assert ctx.d1_index_build() is False
            _same_network(ctx, "kinds", db, turn)
        ctx.d1_set_ownership(0, 2)
        ctx.d1_set_ownership(0, 1)
        _same_network(ctx, "kinds", db, "re-owned")
        _same_network(ctx, "kinds", db, "again")
        assert ctx.d1_guard_retries() == 0
    finally:
        ctx.close()


def test_a_sequence_too_short_for_two_windows_keeps_its_route(tmp, monkeypatch):
    """one sequence of 40 nt among 150-nt families: the index build raises kFlagUnserved and makes the member table, the
    network call lists that one seed for the plain kernel (counters[kCounterFallback], which also travels in the head of
    the status block) and serves it from the table — no retry, no database-wide table, the oracle's network"""
    from swarm_amd import Context
    recs = list(_records(tmp)[:3000]) + [(b"short_1", b"ACGTTGCAAGGCTTAACCGGATATCGCGTTAACTGACTGA")]
    db = S.build_db(recs)
    assert int(db.seqlen.min()) == 40 and int((db.seqlen < 65).sum()) == 1
    monkeypatch.delenv(HOOK, raising=False)
    ctx = Context(0)
    try:
        upload(ctx, db)
        for turn in range(2):
            assert ctx.d1_index_build() is False
            _same_network(ctx, "short", db, turn)
            assert int(ctx.d1_debug(14, 128).view(np.uint32)[2]) == 1, turn    # kCounterFallback: the short seed, once
        ctx.d1_set_ownership(0, 2)
        ctx.d1_set_ownership(0, 1)
        _same_network(ctx, "short", db, "re-owned")            # (this owner's index is built by the call: the database-wide table serves the seed)
        assert ctx.d1_guard_retries() == 0
    finally:
        ctx.close()
