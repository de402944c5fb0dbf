"""What makes tests/test_pair_forms_gpu.py mean what it says, checked without a GPU: the sets of tests/pair_sets.py reach
the list kinds, width classes and windows they are built for (group_model), nothing in them is left to the plain kernel,
the planted key collisions are collisions that only the window flags of pair_near reject, the oracle the GPU is compared
with equals the definition of the network (brute_network) on exactly these shapes, and every dword edge of both chains
carries a planted edit of every kind."""
import numpy as np
import pytest

import index_prep_model as M
import pair_sets as P
from d1_sets import oracle_sorted_rows

WHERES = ("interior", "first", "last")
BUNDLE_AND_BIG = [P.size_kind(g) for g in P.SIZES]


def _kinds_of(sizes):
    return sorted({P.size_kind(g) for g in sizes})


# ---------------------------------------------------------------------------------------------- models against independent ground

def test_key_model_against_plain_integers():
    """key29_model (numpy, wrapping 64-bit arithmetic) against the same in Python's unbounded integers"""
    mask = (1 << 64) - 1

    def mix(x):
        x ^= x >> 33
        x = x * 0xff51afd7ed558ccd & mask
        x ^= x >> 33
        x = x * 0xc4ceb9fe1a85ec53 & mask
        return x ^ (x >> 33)
    rng = np.random.default_rng(3)
    for NW in (1, 2, 4):
        wins = rng.integers(0, 2 ** 64, size=(50, NW), dtype=np.uint64)
        for which in (0, 1):
            got = P.key29_model(wins, which)
            for row, g in zip(wins, got):
                h = mix(int(row[0]) ^ (0x9E3779B97F4A7C15 if which else 0))
                for k in range(1, NW):
                    h = mix(h ^ int(row[k]))
                assert int(g) == mix(h & 0x7FFFFFFFFFFFFFFF) >> 35


def test_size_kinds_and_tiled_items():
    assert [P.size_kind(g) for g in (2, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 256, 257, 4096)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    # a group of g members: t = ceil(g / 64) row tiles, row tile r against the t - r column tiles from itself on, four an item
    assert P.tiled_item_count(257) == 2 + 1 + 1 + 1 + 1
    assert P.tiled_item_count(4096) == sum(-(-(64 - r) // 4) for r in range(64))
    assert [P.width_class(n) for n in (160, 161, 256, 257, 480, 481, 672, 673)] == [0, 1, 1, 2, 2, 3, 3, 4]


def test_edit_places_are_what_the_windows_see():
    """edit_place, the rule the builders sort edits by, against the windows of the edited sequence itself"""
    rng = np.random.default_rng(8)
    for NW, L in ((1, 80), (2, 130), (4, 300)):
        w = 32 * NW
        s = P.runless_sequence(rng, L)
        assert all(s[k] != s[k + 1] for k in range(L - 1))
        for p in range(L):
            for kind in P.KINDS:
                for t in P.edit_variants(s, p, kind):
                    place = "first" if t[:w] != s[:w] else ("last" if t[-w:] != s[-w:] else "interior")
                    assert place == P.edit_place(p, kind, L, NW), (NW, p, kind)


def test_one_edit_equals_the_definition_exhaustively():
    words = ["".join(P.LETTERS[(v >> (2 * k)) & 3] for k in range(n)) for n in range(1, 5) for v in range(4 ** n) if all((v >> (2 * k)) & 3 < 3 for k in range(n))]
    arr = {s: np.frombuffer(s.encode(), dtype=np.uint8) for s in words}
    for a in words:
        for b in words:
            want = a != b and ((len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1) or
                               (abs(len(a) - len(b)) == 1 and any((l := max(a, b, key=len))[:p] + l[p + 1:] == min(a, b, key=len) for p in range(max(len(a), len(b))))))
            assert P.one_edit(arr[a], arr[b]) == want, (a, b)


# ---------------------------------------------------------------------------------------------- reachability, group cap

def _no_plain_kernel(seqs, NW, model):
    assert model["oversized"] == 0 and model["largest"] <= P.GROUP_CAP
    assert min(len(s) for s in seqs) >= 64 * NW + 1
    assert len(set(seqs)) == len(seqs) <= P.MAX_SEQUENCES and sum(len(s) for s in seqs) <= 3_100_000


@pytest.mark.parametrize("W,NW", P.FORMS)
def test_families_reach_every_bundle_and_the_workgroup_list(W, NW):
    cls = P.CLASS_OF[W]
    for L in P.form_lengths(W, NW):
        for where in WHERES:
            seqs, plan = P.families(W, NW, L, P.SIZES, where)
            model = P.group_model(seqs, NW)
            _no_plain_kernel(seqs, NW, model)
            assert max(len(s) for s in seqs) == L + 1 and min(len(s) for s in seqs) == L - 1
            index = {"interior": 1, "first": 1, "last": 0}[where]
            assert sorted(plan["served"][index]) == sorted(P.SIZES)
            for i in (0, 1):                                      # the planted families are groups of that index, as large as planted
                sizes = sorted(g for g, c in model["groups"][i] if c == cls)
                for g in set(plan["served"][i]):
                    assert sizes.count(g) >= plan["served"][i].count(g), (W, NW, L, where, i, g)
                for kind in _kinds_of(plan["served"][i]):
                    assert model["counts"][i, cls, kind] != 0
            assert (model["counts"][index, cls, :6] != 0).all()
            if where == "interior" and L == P.upper_centre(W) and NW == 1:
                assert sorted(plan["served"][0]) == sorted(P.SIZES)    # (both indexes, every size)
            assert model["counts"][:, :, P.KIND_TILED].sum() == 0


@pytest.mark.parametrize("W,NW", P.FORMS)
def test_sweeps_reach_the_tiled_list_in_both_indexes(W, NW):
    cls = P.CLASS_OF[W]
    for L in P.form_lengths(W, NW):
        seqs, kinds = P.tiled_sweep(W, NW, L)
        model = P.group_model(seqs, NW)
        _no_plain_kernel(seqs, NW, model)
        for i in (0, 1):
            assert max(g for g, _ in model["groups"][i]) >= 257
            assert model["counts"][i, cls, P.KIND_TILED] != 0
        # the window sample leaves the windows at the ends (no candidate further in does better on one centre's sweep)
        codes, lens = P.codes_matrix(seqs)
        choice = M.windows_model(codes, lens, len(seqs), int(lens.min()), NW)
        assert (choice["offset"], choice["width"]) == (0, 32 * NW)


def test_the_widest_sweep_drops_edit_kinds_to_stay_under_the_caps():
    rng = np.random.default_rng(1)
    full = P.single_edit_sweep(P.runless_sequence(rng, 671))
    assert P.group_model(full, 1, merge=False)["largest"] > P.GROUP_CAP and len(full) > P.MAX_SEQUENCES
    seqs, kinds = P.tiled_sweep(21, 1, 671)
    assert kinds == ("sub", "del") and len(seqs) == 1 + 4 * 671
    assert P.tiled_sweep(15, 1, 479)[1] == P.KINDS


def test_capped_groups_sit_on_both_sides_of_the_cap():
    for members, oversized in ((4096, 0), (4097, 1)):
        seqs, pairs = P.capped_group(members)
        model = P.group_model(seqs, 2)
        assert len(seqs) == members and len(pairs) == 200 and model["largest"] == members and model["oversized"] == oversized
        assert 129 <= min(len(s) for s in seqs) and max(len(s) for s in seqs) <= 160
        assert (model["counts"][0, 0, P.KIND_TILED] == P.tiled_item_count(4096)) == (members == 4096)
        assert model["counts"][0, 0, P.KIND_TILED] in (0, P.tiled_item_count(4096))
        codes, lens = P.codes_matrix(seqs)
        choice = M.windows_model(codes, lens, len(seqs), int(lens.min()), 4)
        assert (choice["offset"], choice["width"]) == (0, 64)
    assert P.tiled_item_count(4096) > P.tiled_item_count(4095 - 63)      # (row tile 63 exists at 4096 members only above 4032)


@pytest.mark.parametrize("W,NW", P.FORMS)
def test_mixed_lengths_are_one_group_of_the_wide_class(W, NW):
    seqs, subs = P.mixed_lengths(W, NW)
    model = P.group_model(seqs, NW)
    _no_plain_kernel(seqs, NW, model)
    cls = P.CLASS_OF[W]
    for side in (0, 1):
        mine = [x for x in subs if x[0] == side]
        members = sum(1 + len(nbs) for _, _, _, _, nbs in mine)
        assert (members, cls) in model["groups"][side]           # one group, of the width of its longest member
        assert max(len(c) for _, _, _, c, _ in mine) == 32 * W
        for _, ws, r, centre, nbs in mine:
            assert (32 * W - len(centre)) >> 5 == ws and (32 * W - len(centre)) & 31 == r and len(nbs) >= 3
    want = [ws for ws in (0, 1, 2, 3, 4, 5, 7, 8, 16, W - 1) if ws < W and 32 * W - 32 * ws - 30 >= 64 * NW + 2]
    assert sorted({ws for _, ws, _, _, _ in subs}) == sorted(set(want))
    for ws in want:
        assert {r != 0 for _, w2, r, _, _ in subs if w2 == ws} == {False, True}


@pytest.mark.parametrize("W", [5, 8, 15, 21])
def test_flanked_sets_move_the_windows_and_reach_every_kind(W):
    L = {5: 150, 8: 250, 15: 470, 21: 660}[W]
    seqs = P.flanked(W, L)
    assert len(seqs) >= 4300 and len(set(seqs)) == len(seqs) and min(len(s) for s in seqs) >= 129
    assert len({s[:40] for s in seqs}) == 1 and len({s[-40:] for s in seqs}) == 1
    assert max(len(s) for s in seqs) <= P.EDGES[W] and P.width_class(max(len(s) for s in seqs)) == P.CLASS_OF[W]
    codes, lens = P.codes_matrix(seqs)
    choice = M.windows_model(codes, lens, len(seqs), int(lens.min()), 1)
    assert (choice["offset"], choice["width"]) == (32, 32)
    model = P.group_model(seqs, 1, offset=32)
    assert model["oversized"] == 0
    cls = P.CLASS_OF[W]
    for i in (0, 1):
        assert model["counts"][i, cls, :5].sum() != 0 and model["counts"][i, cls, P.KIND_BIG] != 0 and model["counts"][i, cls, P.KIND_TILED] != 0


# ---------------------------------------------------------------------------------------------- collisions

@pytest.mark.parametrize("W,NW", P.FORMS)
def test_collisions_are_rejected_by_the_window_flags_alone(W, NW):
    seqs, info = P.collision_sets(W, NW, "bundle")
    for side, which, PASS in (("suffix", 1, 1), ("prefix", 0, 0)):
        A, B = info[side]["windows"]
        a, b = info[side]["pair"]
        assert A != B and len(A) == len(B) == 32 * NW
        keys = P.key29_model(np.stack([P.window_words(A), P.window_words(B)]), which)
        assert keys[0] == keys[1]
        assert (a[-32 * NW:], b[-32 * NW:]) == (A, B) if which else (a[:32 * NW], b[:32 * NW]) == (A, B)
        arr = [np.frombuffer(s.encode(), dtype=np.uint8) for s in (a, b)]
        assert not P.one_edit(arr[0], arr[1])                       # not a link ...
        assert P.chains_without_windows(a, b, W, NW, PASS)          # ... but one to the chains without the window dwords
        assert P.chains_without_windows(b, a, W, NW, PASS)
        if PASS == 1:
            assert a[:32 * NW] != b[:32 * NW]                       # (PASS 1 emits only where the first windows differ)
        for s, t in info[side]["neighbours"]:
            assert P.one_edit(np.frombuffer(s.encode(), dtype=np.uint8), np.frombuffer(t.encode(), dtype=np.uint8))


@pytest.mark.parametrize("W,NW,kind", [(W, NW, "bundle") for W, NW in P.FORMS] +
                         [(W, NW, kind) for W, NW in ((8, 2), (21, 4)) for kind in ("big", "tiled")])
def test_collision_groups_merge_into_the_intended_kind(W, NW, kind):
    seqs, info = P.collision_sets(W, NW, kind)
    merged, apart = P.group_model(seqs, NW), P.group_model(seqs, NW, merge=False)
    _no_plain_kernel(seqs, NW, merged)
    cls = P.CLASS_OF[W]
    want_kind = {"bundle": 1, "big": P.KIND_BIG, "tiled": P.KIND_TILED}[kind]
    members = 2 * (1 + P.COLLISION_NEIGHBOURS[kind])
    for side, which in (("suffix", 1), ("prefix", 0)):
        assert merged["groups"][which].count((members, cls)) == apart["groups"][which].count((members, cls)) + 1
        assert merged["groups"][which].count((members // 2, cls)) == apart["groups"][which].count((members // 2, cls)) - 2
        assert len(merged["groups"][which]) == len(apart["groups"][which]) - 1
        assert merged["counts"][which, cls, want_kind] != 0
        assert not np.array_equal(merged["counts"][which], apart["counts"][which])


# ---------------------------------------------------------------------------------------------- the oracle against the definition

def _oracle_is_the_definition(seqs, seed=0):
    db, text = P.database(seqs, seed)
    assert len({int(a) for a in db.abundance}) >= 3 and len(seqs) <= 700
    for ncb in (False, True):
        off, nb, dup = oracle_sorted_rows(db, ncb)
        woff, wnb = P.brute_network(text, db.abundance, ncb)
        assert not dup
        assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
    return len(wnb)


@pytest.mark.parametrize("W", [5, 8, 15, 21])
def test_oracle_equals_the_definition_on_these_shapes(W):
    NW = 1
    for where in WHERES:
        seqs, _ = P.families(W, NW, P.upper_centre(W), P.SIZES_SMALL, where)
        assert _oracle_is_the_definition(seqs) > len(seqs) // 2
    NW = 4 if W >= 15 else 2
    assert _oracle_is_the_definition(P.mixed_lengths(W, NW)[0]) > 0
    assert _oracle_is_the_definition(P.mixed_lengths(W, 1)[0]) > 0
    assert _oracle_is_the_definition(P.collision_sets(W, NW, "bundle")[0]) >= 24
    assert _oracle_is_the_definition(P.collision_sets(W, NW, "big")[0]) > 0


def test_oracle_equals_the_definition_on_a_whole_sweep():
    rng = np.random.default_rng(70)
    seqs = P.single_edit_sweep(P.random_sequence(rng, 70))
    db, text = P.database(seqs)
    off, nb = P.brute_network(text, db.abundance, True)
    centre = text.index(seqs[0])
    assert int(off[centre + 1] - off[centre]) == len(seqs) - 1            # every member is a neighbour of the centre
    assert _oracle_is_the_definition(seqs) > len(seqs)
    for first, count in ((0, 1), (100, 200), (len(seqs) - 5, 5)):          # the rows of a range of seeds
        woff, wnb, _ = oracle_sorted_rows(db, False, first, count)
        boff, bnb = P.brute_network(text, db.abundance, False, first, count)
        assert np.array_equal(woff, boff) and np.array_equal(wnb, bnb)


# ---------------------------------------------------------------------------------------------- edge positions

@pytest.mark.parametrize("W,NW", P.FORMS)
def test_every_dword_edge_carries_every_kind_of_edit(W, NW):
    for L in P.form_lengths(W, NW):
        want = {(p, kind) for p in P.edge_positions(W, L, NW) for kind in P.KINDS}
        assert {0, 15, 16, L - 1, L - 16, L - 17, 32 * NW - 1, 32 * NW, L - 32 * NW - 1, L - 32 * NW} <= {p for p, _ in want}
        used = set()
        for where in WHERES:
            seqs, plan = P.families(W, NW, L, P.SIZES, where)
            at = 0
            for f, size in enumerate(P.SIZES):                   # the record of the edits against the sequences themselves
                centre, members = seqs[at], seqs[at + 1:at + size]
                at += size
                mine = [(p, kind) for g, p, kind in plan["edits"] if g == f]
                assert centre == plan["centres"][f] and len(mine) == len(members)
                for (p, kind), s in zip(mine, members):
                    assert s in P.edit_variants(centre, p, kind) and P.edit_place(p, kind, L, NW) in (where, "first" if where == "interior" else "interior")
            used |= {(p, kind) for _, p, kind in plan["edits"]}
        assert want <= used, sorted(want - used)[:5]
