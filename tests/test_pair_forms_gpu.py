"""Every form of the d = 1 pair kernels (swarm_amd/csrc/d1_anchor.inc) on planted edits and key collisions, at small sizes:
k_d1_group_pairs<PASS, W, NW> and k_d1_pairs_tiled<PASS, W, NW> for PASS 0 / 1, W = 5, 8, 15, 21 words a record and NW = 1, 2
(4 with W >= 15) words a window, and the window mode of each W.  The sets and the CPU models are tests/pair_sets.py's;
tests/test_pair_sets_identity.py shows without a GPU that the sets reach what they are built for and that the oracle equals
the definition of the network on them.

Which form ran is asserted, not assumed: before any network call the test reads the work-list counters the index build
left (status counters 64 + (index * 4 + class) * 8 + kind; index 0 = prefix groups = PASS 0, index 1 = suffix groups =
PASS 1; class 0..3 = W 5 / 8 / 15 / 21; kinds 0..4 = bundles of groups up to 4, 8, 16, 32, 64 members, 5 = groups of 65..256
in k_d1_group_pairs, 6 = row-tile items of k_d1_pairs_tiled) and compares them with group_model; the window width is
d1_anchor_width() = 32 NW (SWA_D1_ANCHOR_W caps it where the lengths would choose wider), and afterwards the fallback
counter (word 2) is 0 — no seed went to the plain kernel — and the guard repeated nothing during the test.  The network is the oracle's,
exactly, with and without cluster breaking.

form (PASS 0 and 1 each)        k_d1_group_pairs                                    k_d1_pairs_tiled
(W, NW) of FORMS, ends          test_families_at_every_dword_edge [interior|first|last x upper|lower length]
                                                                                    test_sweep_of_one_centre_is_tiled
                                test_mixed_lengths_go_through_the_shifter            (collisions, tiled kind: (8, 2), (21, 4))
                                test_key_collisions_are_not_links                    test_group_cap_boundary: (5, 2), row tile 63
                                test_identical_sequences_are_met_by_the_prefix_pass (every kind)
                                test_ranges_of_seeds
(15, 1) without the switch      test_one_short_sequence_narrows_the_windows
window mode, W = 5, 8, 15, 21   test_window_mode_of_every_width (bundles, 65..256 and tiled counters non-zero)
segment regrow                                                                      test_segments_regrow_under_a_wide_tiled_set
"""
import numpy as np
import pytest

import pair_sets as P
from d1_sets import oracle_sorted_rows, upload

pytestmark = pytest.mark.gpu

WHERES = ("interior", "first", "last")
COUNTER_FALLBACK = 2


def _list_counters(ctx) -> np.ndarray:
    """u32 [2, 4, 8]: items of work list (index, class, kind), as the index build left them"""
    return ctx.d1_debug(14, 128).view(np.uint32)[64:128].reshape(2, 4, 8).copy()


def _fallback(ctx) -> int:
    return int(ctx.d1_debug(14, 128).view(np.uint32)[COUNTER_FALLBACK])


def _build(ctx, monkeypatch, db, NW, seqs, windows=(0, 0), intended=()):
    """upload + index build under windows capped at 32 NW nt; the counters prove the form: equal to the model's, the
    intended lists non-empty.  Returns the model."""
    monkeypatch.setenv("SWA_D1_ANCHOR_W", str(32 * NW))
    retries = ctx.d1_guard_retries()                              # (a count over the context's life: this test's share is asserted)
    upload(ctx, db)
    assert ctx.d1_index_build() is False
    got = _list_counters(ctx)
    model = P.group_model(seqs, NW, offset=windows[0])
    model["guard_retries"] = retries
    assert ctx.d1_anchor_width() == 32 * NW and ctx.d1_anchor_windows() == windows
    assert np.array_equal(got[:, :, :7], model["counts"][:, :, :7]), (got[:, :, :7].tolist(), model["counts"][:, :, :7].tolist())
    for index, cls, kind in intended:
        assert got[index, cls, kind] != 0, (index, cls, kind)
    return model


def _network_is_the_oracles(ctx, db, retries_before, served_by_pairs=True):
    rows = {}
    for ncb in (False, True):
        off, nb = ctx.d1_network(ncb)
        woff, wnb, dup = oracle_sorted_rows(db, ncb)
        assert not dup
        assert np.array_equal(off, woff)
        assert np.array_equal(nb, wnb)
        if served_by_pairs:
            assert _fallback(ctx) == 0                            # nobody went to the plain kernel
        rows[ncb] = (off, nb)
    assert ctx.d1_guard_retries() == retries_before               # the guard repeated nothing
    return rows


def _check(ctx, monkeypatch, seqs, NW, seed=0, windows=(0, 0), intended=()):
    db, text = P.database(seqs, seed)
    model = _build(ctx, monkeypatch, db, NW, seqs, windows, intended)
    rows = _network_is_the_oracles(ctx, db, model["guard_retries"])
    return db, text, model, rows


def _has_link(rows, index_of, a: str, b: str) -> bool:
    """whether a and b are linked in the network without cluster breaking (rows[True]), in either row"""
    off, nb = rows[True]
    i, j = index_of[a], index_of[b]
    return j in nb[int(off[i]):int(off[i + 1])] and i in nb[int(off[j]):int(off[j + 1])]


# ---------------------------------------------------------------------------------------------- bundles and the workgroup list

@pytest.mark.parametrize("upper", [True, False], ids=["upper", "lower"])
@pytest.mark.parametrize("where", WHERES)
@pytest.mark.parametrize("W,NW", P.FORMS)
def test_families_at_every_dword_edge(gpu_ctx, monkeypatch, W, NW, where, upper):
    """Groups of 2 .. 256 members, both sides of every boundary between the list kinds, whose links are single edits at the
    first and last nucleotide of every dword of both chains.  interior: both passes' groups; first: the suffix groups, PASS 1
    emits; last: the prefix groups, PASS 0 emits with its shortened suffix chain.  upper: the longest member fills the
    record (no shift); lower: the shortest the class and the windows allow."""
    L = P.form_lengths(W, NW)[0 if upper else 1]
    seqs, plan = P.families(W, NW, L, P.SIZES, where)
    cls = P.CLASS_OF[W]
    intended = [(i, cls, P.size_kind(g)) for i in (0, 1) for g in plan["served"][i]]
    assert {(i, k) for i, _, k in intended} >= {({"interior": 1, "first": 1, "last": 0}[where], k) for k in range(6)}
    _, _, _, rows = _check(gpu_ctx, monkeypatch, seqs, NW, seed=L, intended=intended)
    assert len(rows[True][1]) >= 2 * (len(seqs) - len(P.SIZES))       # every member and its centre, both ways


def test_one_short_sequence_narrows_the_windows(gpu_ctx, monkeypatch):
    """(15, 1) without the switch: one 100-nt sequence in a file of 479-nt families leaves room for 32-nt windows only"""
    monkeypatch.delenv("SWA_D1_ANCHOR_W", raising=False)
    seqs, plan = P.families(15, 1, 479, P.SIZES, "interior")
    rng = np.random.default_rng(100)
    seqs = list(seqs) + [P.runless_sequence(rng, 100)]
    db, _ = P.database(seqs, 1)
    retries = gpu_ctx.d1_guard_retries()
    upload(gpu_ctx, db)
    assert gpu_ctx.d1_index_build() is False
    got = _list_counters(gpu_ctx)
    assert gpu_ctx.d1_anchor_width() == 32 and gpu_ctx.d1_anchor_windows() == (0, 0)
    assert np.array_equal(got[:, :, :7], P.group_model(seqs, 1)["counts"][:, :, :7])
    assert (got[:, 2, :6] != 0).all() and got[:, [0, 1, 3], :].sum() == 0
    _network_is_the_oracles(gpu_ctx, db, retries)


# ---------------------------------------------------------------------------------------------- the tiled kernel

@pytest.mark.parametrize("upper", [True, False], ids=["upper", "lower"])
@pytest.mark.parametrize("W,NW", P.FORMS)
def test_sweep_of_one_centre_is_tiled(gpu_ctx, monkeypatch, W, NW, upper):
    """every single edit of one centre (pair_sets.tiled_sweep: which kinds): one group of 257 .. 4096 members in each index,
    the centre linked with everybody, the members among each other where they differ at one position"""
    L = P.form_lengths(W, NW)[0 if upper else 1]
    seqs, kinds = P.tiled_sweep(W, NW, L)
    cls = P.CLASS_OF[W]
    db, text, model, rows = _check(gpu_ctx, monkeypatch, seqs, NW, seed=L, intended=[(0, cls, P.KIND_TILED), (1, cls, P.KIND_TILED)])
    off, nb = rows[True]
    centre = text.index(seqs[0])
    assert int(off[centre + 1] - off[centre]) == len(seqs) - 1


@pytest.mark.parametrize("members", [4096, 4097])
def test_group_cap_boundary(gpu_ctx, monkeypatch, members):
    """kStreamGroupCap: a prefix group of exactly 4096 members is the tiled kernel's — 64 row tiles, row tile 63 in the six
    bits of item.chunk, every column part — and one of 4097 is the plain kernel's: no tiled item, seeds on the fallback list.
    The oracle's network either way, the 200 planted neighbours in it."""
    seqs, pairs = P.capped_group(members)
    db, text = P.database(seqs, members)
    index_of = {s: i for i, s in enumerate(text)}
    monkeypatch.delenv("SWA_D1_ANCHOR_W", raising=False)
    retries = gpu_ctx.d1_guard_retries()
    upload(gpu_ctx, db)
    assert gpu_ctx.d1_index_build() is False
    got = _list_counters(gpu_ctx)
    assert gpu_ctx.d1_anchor_width() == 64 and gpu_ctx.d1_anchor_windows() == (0, 0)
    assert np.array_equal(got[:, :, :7], P.group_model(seqs, 2)["counts"][:, :, :7])
    assert got[0, 0, P.KIND_TILED] == (P.tiled_item_count(4096) if members == 4096 else 0)
    rows = _network_is_the_oracles(gpu_ctx, db, retries, served_by_pairs=members == 4096)
    assert (_fallback(gpu_ctx) > 0) == (members == 4097)
    for a, b in pairs:
        assert _has_link(rows, index_of, a, b)


# ---------------------------------------------------------------------------------------------- the shifter

@pytest.mark.parametrize("W,NW", P.FORMS)
def test_mixed_lengths_go_through_the_shifter(gpu_ctx, monkeypatch, W, NW):
    """pair_stage_line's barrel shifter: members of one prefix group and of one suffix group of width W that are 0, 1, 2, 3, 4,
    5, 7, 8, 16 words shorter than the record (as far as the form has them), with and without a bit shift.  The class
    counters prove that the groups were served at width W; the links of each short sub-family are asserted one by one, so a
    failure names the shift."""
    seqs, subs = P.mixed_lengths(W, NW)
    cls = P.CLASS_OF[W]
    sizes = [sum(1 + len(nbs) for side, _, _, _, nbs in subs if side == i) for i in (0, 1)]
    intended = [(i, cls, P.size_kind(sizes[i])) for i in (0, 1)]
    db, text, model, rows = _check(gpu_ctx, monkeypatch, seqs, NW, seed=W, intended=intended)
    for i in (0, 1):                                               # (the sub-families' own groups are of kind 0 or 1)
        assert sizes[i] >= 9 and (sizes[i], cls) in model["groups"][i]
    index_of = {s: i for i, s in enumerate(text)}
    for side, ws, r, centre, nbs in subs:
        for s in nbs:
            assert _has_link(rows, index_of, centre, s), f"pass {side}: word shift {ws}, bit shift {r}: a link is missing"


# ---------------------------------------------------------------------------------------------- key collisions

@pytest.mark.parametrize("W,NW,kind", [(W, NW, "bundle") for W, NW in P.FORMS] +
                         [(W, NW, kind) for W, NW in ((8, 2), (21, 4)) for kind in ("big", "tiled")])
def test_key_collisions_are_not_links(gpu_ctx, monkeypatch, W, NW, kind):
    """Two windows with one 29-bit key make one group of two: the counters show the merged group, the pair across the
    collision — one edit apart as far as the chains of pair_near see (`tail` / `same` alone reject it) — is not in the
    network, the true neighbours of both are."""
    seqs, info = P.collision_sets(W, NW, kind)
    cls = P.CLASS_OF[W]
    want_kind = {"bundle": 1, "big": P.KIND_BIG, "tiled": P.KIND_TILED}[kind]
    db, text, model, rows = _check(gpu_ctx, monkeypatch, seqs, NW, seed=NW, intended=[(0, cls, want_kind), (1, cls, want_kind)])
    assert not np.array_equal(model["counts"], P.group_model(seqs, NW, merge=False)["counts"])     # (two groups by their texts)
    index_of = {s: i for i, s in enumerate(text)}
    for side in ("suffix", "prefix"):
        a, b = info[side]["pair"]
        assert not _has_link(rows, index_of, a, b) and not _has_link(rows, index_of, b, a), f"{side} side: a key collision became a link"
        i, j = index_of[a], index_of[b]
        off, nb = rows[True]
        assert j not in nb[int(off[i]):int(off[i + 1])] and i not in nb[int(off[j]):int(off[j + 1])]
        for s, t in info[side]["neighbours"]:
            assert _has_link(rows, index_of, s, t), f"{side} side: a neighbour in a merged group is missing"


# ---------------------------------------------------------------------------------------------- identical sequences

@pytest.mark.parametrize("size", [4, 100, 300])
@pytest.mark.parametrize("W,NW", P.FORMS)
def test_identical_sequences_are_met_by_the_prefix_pass(gpu_ctx, monkeypatch, W, NW, size):
    """One member of a prefix group of each kind (a bundle, 65..256, tiled) a second time: the index build is clean, the
    network call whose seeds include a copy reports SWA_E_DUPLICATES, a call whose seeds include neither does not."""
    from swarm_amd.capi import SWA_E_DUPLICATES, SwaError
    L = P.upper_centre(W)
    seqs, plan = P.families(W, NW, L, (size, 3), "last")              # (edits in the last window: one prefix group)
    db, text = P.database(seqs, size, twins=(size // 2,))
    monkeypatch.setenv("SWA_D1_ANCHOR_W", str(32 * NW))
    upload(gpu_ctx, db)
    assert gpu_ctx.d1_index_build() is False
    got = _list_counters(gpu_ctx)
    kind = P.size_kind(size + 1)                                  # (the twin is a member: 5, 101 and 301)
    assert got[0, P.CLASS_OF[W], kind] == (P.tiled_item_count(size + 1) if kind == P.KIND_TILED else 1)
    assert gpu_ctx.d1_anchor_width() == 32 * NW
    copies = [i for i, s in enumerate(text) if s == seqs[size // 2]]
    assert len(copies) == 2
    gaps = [(0, copies[0]), (copies[0] + 1, copies[1] - copies[0] - 1), (copies[1] + 1, db.n - copies[1] - 1)]
    first, count = max(gaps, key=lambda g: g[1])
    assert count > 0
    # neither copy is a seed: nothing to report.  (The oracle's table holds one of two identical sequences: with a twin in
    # the database the yardstick is the definition itself — both copies are neighbours of their neighbours, not of each other.)
    off, nb = gpu_ctx.d1_network(False, first, count)
    woff, wnb = P.brute_network(text, db.abundance, False, first, count)
    assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
    for f, c in ((0, db.n), (copies[0], 1), (copies[1], 1)):
        with pytest.raises(SwaError) as e:
            gpu_ctx.d1_network(False, f, c)
        assert e.value.code == SWA_E_DUPLICATES


# ---------------------------------------------------------------------------------------------- ranges of seeds

@pytest.mark.parametrize("W,NW", [(5, 2), (8, 1), (15, 4), (21, 2)])
def test_ranges_of_seeds(gpu_ctx, monkeypatch, W, NW):
    """m.ok: members outside [first, first + count) are targets only.  The database is in abundance order, so any range
    cuts through the middle of the groups; a single seed; the last seeds only."""
    seqs, _ = P.families(W, NW, P.upper_centre(W), P.SIZES, "interior")
    db, _ = P.database(seqs, 5)
    model = _build(gpu_ctx, monkeypatch, db, NW, seqs)
    n = db.n
    for ncb in (False, True):
        for first, count in ((n // 3, n // 3), (n // 2, 1), (n - 5, 5)):
            off, nb = gpu_ctx.d1_network(ncb, first, count)
            woff, wnb, _ = oracle_sorted_rows(db, ncb, first, count)
            assert np.array_equal(off, woff) and np.array_equal(nb, wnb), (ncb, first, count)
            assert _fallback(gpu_ctx) == 0
    assert gpu_ctx.d1_guard_retries() == model["guard_retries"]


# ---------------------------------------------------------------------------------------------- window mode

@pytest.mark.parametrize("W,L", [(5, 150), (8, 250), (15, 470), (21, 660)])
def test_window_mode_of_every_width(gpu_ctx, monkeypatch, W, L):
    """Everybody shares the first and the last 40 nt: the windows move 32 nt inwards and the pair kernels run their
    window mode (`ends == false`: both chains in full, `same` on the window word of the record) at every record width, on
    bundles, on groups of 65..256 and on tiled groups."""
    seqs = P.flanked(W, L)
    cls = P.CLASS_OF[W]
    intended = [(i, cls, k) for i in (0, 1) for k in (P.KIND_BIG, P.KIND_TILED)]
    db, text, model, rows = _check(gpu_ctx, monkeypatch, seqs, 1, seed=W, windows=(32, 32), intended=intended)
    assert gpu_ctx.d1_anchor_windows()[0] >= 32 and gpu_ctx.d1_anchor_width() == 32
    got = _list_counters(gpu_ctx)
    for i in (0, 1):
        assert got[i, cls, :5].sum() != 0 and got[i, cls, P.KIND_BIG] != 0 and got[i, cls, P.KIND_TILED] != 0
    assert len(rows[True][1]) >= len(seqs)


# ---------------------------------------------------------------------------------------------- segment regrow

def test_segments_regrow_under_a_wide_tiled_set(monkeypatch):
    """SWA_D1_SEG_CAP (read once per context): per-wave link segments of one link under a tiled W = 15 sweep — the centre's
    wave alone has thousands of links — are regrown and the network is the same"""
    from swarm_amd import Context
    seqs, _ = P.tiled_sweep(15, 2, 479)
    db, _ = P.database(seqs, 15)
    monkeypatch.setenv("SWA_D1_SEG_CAP", "1")
    ctx = Context(0)
    try:
        model = _build(ctx, monkeypatch, db, 2, seqs, intended=[(0, 2, P.KIND_TILED), (1, 2, P.KIND_TILED)])
        _network_is_the_oracles(ctx, db, model["guard_retries"])
    finally:
        ctx.close()
