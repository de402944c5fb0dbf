"""What tests/test_multi_edges_gpu.py takes for granted about the sets of tests/multi_sets.py, proven with numpy and the
oracle only (no GPU, no product code): that every admissible anchor window of shared_flanks gives one key for the whole
set, that few_groups has fewer windows than eight ranks, that the d >= 2 sets have fewer links than eight ranks, that the
dense set's links exceed two ranks' first link buffers, and that the merge kernel's closed form is the textbook merge."""
import numpy as np
import pytest

import multi_sets as MS
import support as S


def _seqs(db):
    return [db.seq_str(i) for i in range(db.n)]


def _same_order_as_the_file(db, fa):
    """the FASTA file holds the Db's records, and reading it back gives the same database"""
    again = S.db_from_fasta(fa)
    assert again.headers == db.headers and np.array_equal(again.seqs, db.seqs) and np.array_equal(again.abundance, db.abundance)


# ---- d = 1 ------------------------------------------------------------------------------------------------------------------
def test_shared_flanks_have_one_key_per_admissible_window(tmp_path):
    db, fa = MS.shared_flanks(tmp_path / "in.fa")
    _same_order_as_the_file(db, fa)
    seqs = _seqs(db)
    assert len(set(seqs)) == db.n >= 6500 and abs(db.n - 9000) <= 3
    shortest, longest = int(db.seqlen.min()), int(db.seqlen.max())
    assert shortest >= 149 and longest <= 151 and len(set(db.seqlen.tolist())) == 3
    # a window offset w is admissible when 2 w + 65 <= shortest (d1.hip: index_build): 0 and 32, not 64
    assert [w for w in (0, 32, 64, 96) if 2 * w + 65 <= shortest] == [0, 32]
    assert len({s[:64] for s in seqs}) == 1 and len({s[-64:] for s in seqs}) == 1
    for w in (0, 32):
        for width in (32, 64):
            if w + width <= 64:
                assert len({s[w:w + width] for s in seqs}) == 1 and len({s[len(s) - w - width:len(s) - w] for s in seqs}) == 1
    off, nb = MS.oracle_network(db, False)
    assert len(nb) > db.n // 2
    # all records of a slice go to one owner: the routed build overflows exactly where a slice exceeds a region
    overflow = {world: MS.longest_slice(db.n, world) > MS.route_region(db.n, world) for world in MS.WORLDS}
    assert overflow == {2: True, 3: True, 5: True, 8: False}


def test_the_dense_set_outgrows_two_ranks_first_link_buffers(tmp_path):
    db, fa = MS.shared_flanks_dense(tmp_path / "in.fa")
    assert db.n == 4 ** 7 <= 20000 and set(db.seqlen.tolist()) == {150}
    seqs = _seqs(db)
    assert len(set(seqs)) == db.n and len({s[:64] for s in seqs}) == 1 and len({s[-64:] for s in seqs}) == 1
    # without cluster breaking every amplicon lists its 21 neighbours (with it: only those that are not more abundant)
    off, nb = MS.oracle_network(db, True)
    assert np.array_equal(np.diff(off), np.full(db.n, 21, dtype=np.uint64))
    # two ranks: one of them finds at least half of the links, more than its first buffer holds
    assert len(nb) == 21 * db.n > 2 * MS.link_cap(db.n, 2)


def test_few_groups_has_fewer_windows_than_eight_ranks(tmp_path):
    db, fa = MS.few_groups(tmp_path / "in.fa")
    _same_order_as_the_file(db, fa)
    seqs = _seqs(db)
    assert db.n == 87 and len(set(seqs)) == db.n
    assert len({s[:64] for s in seqs}) == 7 < 8 and len({s[-64:] for s in seqs}) == 7 < 8
    assert int(db.seqlen.min()) >= 149 and int(db.seqlen.max()) <= 151
    off, nb = MS.oracle_network(db, False)
    # links inside the two families only: every variant next to its centroid, the singletons next to nobody
    fam = np.array([h[:2] for h in db.headers])
    rows = np.repeat(np.arange(db.n), np.diff(off).astype(np.int64))
    assert len(nb) >= db.n - 7 and (fam[rows] == fam[nb]).all()
    assert all(off[i] == off[i + 1] for i in range(db.n) if db.headers[i].startswith(b"x"))


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_tiny_sets(tmp_path, n):
    db, fa = MS.tiny(tmp_path / "in.fa", n)
    _same_order_as_the_file(db, fa)
    assert db.n == n and set(db.seqlen.tolist()) == {100}
    off, nb = MS.oracle_network(db, False)                        # the more abundant one lists the other ...
    assert nb.tolist() == ([1] if n >= 2 else []) and int(off[1]) == len(nb)
    off, nb = MS.oracle_network(db, True)                         # ... and both list each other without cluster breaking
    assert nb.tolist() == ([1, 0] if n >= 2 else [])


def test_mixed_lengths_and_giant_are_what_their_names_say(tmp_path):
    db, fa = MS.mixed_lengths(tmp_path / "mix.fa")
    _same_order_as_the_file(db, fa)
    assert 19 <= int(db.seqlen.min()) <= 21
    assert (db.seqlen < 65).any() and (db.seqlen >= 65).any() and int(db.seqlen.max()) >= 200
    assert len(MS.oracle_network(db, False)[1]) > db.n
    db, fa = MS.giant(tmp_path / "giant.fa")
    _same_order_as_the_file(db, fa)
    seqs = _seqs(db)
    heads = {}
    for s in seqs:
        heads[s[:32]] = heads.get(s[:32], 0) + 1
    assert max(heads.values()) == 2600 and len(heads) > 30      # one giant group beside ordinary ones


def test_few_heavy_has_fewer_heavy_amplicons_than_five_ranks(tmp_path):
    db, fa = MS.few_heavy(tmp_path / "in.fa")
    _same_order_as_the_file(db, fa)
    assert db.n == 23 and int((db.abundance >= 3).sum()) == 3 < 5
    assert len(MS.oracle_network(db, False)[1]) == 0              # every amplicon a swarm of its own: 3 heavy, 20 light
    flags = (db.abundance < 3).astype(np.uint8)
    graft, counters = S.oracle_fastidious(db, flags)
    assert int((graft != 0xFFFFFFFF).sum()) == 15


# ---- d >= 2 -----------------------------------------------------------------------------------------------------------------
WANT_LINKS = {"sparse": (3, 4), "no_pair": (0, 0), "with_short": (4, 6)}     # (with cluster breaking, without)


@pytest.mark.parametrize("variant", MS.DN_VARIANTS)
@pytest.mark.parametrize("d", MS.DN_DS)
def test_dn_sparse_sets_have_fewer_links_than_eight_ranks(tmp_path, d, variant):
    db, fa = MS.dn_sparse(tmp_path / "in.fa", d, variant)
    _same_order_as_the_file(db, fa)
    assert 120 <= db.n <= 300 and len(set(_seqs(db))) == db.n
    T = 16 * (d + 1)
    long_part = db.seqlen[[not h.startswith((b"s", b"ss", b"sl")) for h in db.headers]]
    assert int(long_part.min()) >= 60 and int(long_part.max()) <= 121
    if variant == "with_short":
        assert (db.seqlen < T).any() and ((db.seqlen >= T).any() or T > 121)
    for ncb in (False, True):
        off, nb, df = MS.brute_force_graph(db, d, ncb)
        assert len(nb) == WANT_LINKS[variant][int(ncb)] < 8
        assert len(df) == len(nb) and (df <= d).all() and (df >= 1).all()
        rows = np.repeat(np.arange(db.n), np.diff(off).astype(np.int64))
        assert ((rows[1:] > rows[:-1]) | (nb[1:] > nb[:-1])).all()                # rows strictly ascending
        names = {(db.headers[q].split(b"_")[0][:-1], db.headers[t].split(b"_")[0][:-1]) for q, t in zip(rows.tolist(), nb.tolist())}
        assert all(a == b and a in (b"tie", b"far", b"ss", b"sl", b"sd") for a, b in names), names   # links only inside the planted pairs
        if variant == "sparse":
            assert d in df.tolist() and 1 in df.tolist() and not any(a == b"miss" for a, _ in names)
        if variant == "with_short":
            short_member = (db.seqlen[rows] < T) | (db.seqlen[nb] < T)
            assert short_member.any() and ((~short_member).any() or T > 121)


# ---- the merge ---------------------------------------------------------------------------------------------------------------
def test_merge_reference_is_the_textbook_merge_and_the_cases_cover_the_issue():
    seen_worlds, seen_lengths, seen_patterns = set(), set(), set()
    gaps = {"first": False, "last": False, "middle": False, "all but one": False, "one element": False}
    for name, world, lists in MS.merge_cases():
        assert len(lists) == world
        for keys, vals in lists:
            assert keys.dtype == np.uint64 and vals.dtype == np.uint32 and len(keys) == len(vals)
            assert (keys[1:] >= keys[:-1]).all()                                  # what the kernel requires of a list
        lens = [len(k) for k, _ in lists]
        seen_worlds.add(world); seen_lengths.update(lens); seen_patterns.add(name.split("-")[1])
        keys, vals, at = MS.merge_flat(lists)
        assert len(set(vals.tolist())) == len(vals)                               # distinct values: the order of equal keys shows
        wk, wv = MS.merge_reference(lists)
        hk, hv = MS.merge_by_heap(lists)
        assert np.array_equal(wk, hk) and np.array_equal(wv, hv), name
        if world >= 3:
            gaps["first"] |= lens[0] == 0 and lens[-1] > 0
            gaps["last"] |= lens[-1] == 0 and lens[0] > 0
            gaps["middle"] |= any(lens[r] == 0 and lens[r - 1] > 0 and lens[r + 1] > 0 for r in range(1, world - 1))
            gaps["all but one"] |= sum(v > 0 for v in lens) == 1
        gaps["one element"] |= sum(lens) == 1
        if "ranges" in name and "reversed" not in name and "one-element" not in name:
            full = [k for k, _ in lists if len(k)]
            assert all(a[-1] < b[0] for a, b in zip(full, full[1:]))
        if "ranges_reversed" in name:
            full = [k for k, _ in lists if len(k)]
            assert all(a[0] > b[-1] for a, b in zip(full, full[1:]))
        if "interleaved" in name:
            assert all((k % np.uint64(world) == r).all() for r, (k, _) in enumerate(lists))
        if "high_bits" in name:
            assert all((k >> np.uint64(63) == 1).all() for k, _ in lists)
        if "ties" in name and world > 1 and sum(v > 2 for v in lens) >= 2:
            shared = set.intersection(*[set(k.tolist()) for k, _ in lists if len(k) > 2])
            assert shared                                                         # equal keys across lists
    assert seen_worlds == set(MS.MERGE_WORLDS) and seen_lengths >= set(MS.MERGE_LENGTHS)
    assert seen_patterns >= {"ranges", "ranges_reversed", "interleaved", "high_bits", "ties"}
    assert all(gaps.values()), gaps


def test_stable_order_is_upper_bound_below_and_lower_bound_above():
    """the kernel's placement rule worked through in numpy: element i of list r goes to i + (keys <= its key in the lists
    before r) + (keys < its key in the lists after r) — and that is the stable order"""
    rng = np.random.default_rng(5)
    lists = MS.merge_lists(rng, 3, [257, 0, 256], "ties") + MS.merge_lists(rng, 2, [2, 255], "ties")
    keys, vals, at = MS.merge_flat(lists)
    out_k, out_v = np.zeros_like(keys), np.zeros_like(vals)
    taken = np.zeros(len(keys), dtype=bool)
    for r, (k, v) in enumerate(lists):
        pos = np.arange(len(k))
        for s2, (k2, _) in enumerate(lists):
            if s2 != r:
                pos = pos + np.searchsorted(k2, k, side="right" if s2 < r else "left")
        assert not taken[pos].any()
        taken[pos] = True
        out_k[pos], out_v[pos] = k, v
    wk, wv = MS.merge_reference(lists)
    assert taken.all() and np.array_equal(out_k, wk) and np.array_equal(out_v, wv)
