"""The d = 1 network on the plain route (swarm_amd/csrc/d1_probe.inc: enumerate_variants, k_d1_probe<ZLDS, MODE 0 / 2>;
d1.hip: k_seqhash, k_table_insert, the per-wave link segments) against the oracle at the places where that code changes
behaviour.  Every other route falls back on it; the other tests reach it through random sets only.

  lane edges   enumerate_variants deals positions [l K, (l + 1) K) to lane l, K = ceil((len + 1) / 64): full stars (every
               edit at every position) of a random, a run-built, a period-2 and a one-letter centre at the lengths where K
               or the number of packed words changes, under SWA_D1_PLAIN=1;
  ownership    the same seeds divided by id (swa_d1_set_ownership);
  Zobrist      longest sequence 3070 nt (the table in LDS: the largest launch there is) and 3071 (read from memory);
  MODE 2       the fallback seeds of the anchored route — oversized groups by position, moved windows by filter — with
               a full star planted on one of them;
  segments     SWA_D1_SEG_CAP: the per-wave link segments start too small and are regrown, for the CSR and the flat list.

The sets are tests/plain_sets.py's; tests/test_plain_identity.py ties the oracle to the definition on them.  Everything
is integer: compared exactly."""
import functools

import numpy as np
import pytest

import plain_sets as P
import support as S
from d1_sets import check_vs_oracle, conserved_flank_set, giant_group_db, link_keys, oracle_sorted_rows, upload
from swarm_amd import Context

pytestmark = pytest.mark.gpu

_oracle = functools.lru_cache(maxsize=None)(lambda L, ncb: oracle_sorted_rows(P.star_database(L)[0], ncb))


def _star_network(ctx, L, ncb):
    """the network of star_database(L) on ctx against the oracle, and every centre's row: its whole star"""
    db, info = P.star_database(L)
    off, nb = ctx.d1_network(ncb)
    woff, wnb, _ = _oracle(L, ncb)
    assert np.array_equal(off, woff), (L, ncb, np.flatnonzero(np.diff(off) != np.diff(woff))[:8])
    assert np.array_equal(nb, wnb), (L, ncb)
    for kind, (cid, size) in info.items():
        assert int(off[cid + 1] - off[cid]) == size - 1, (L, kind)
    return off, nb


@pytest.mark.parametrize("L", P.LANE_LENGTHS)
def test_lane_edges_full_stars(monkeypatch, L):
    """all four centre kinds at every length (the 192-nt database has 4993 sequences and takes no longer than the others)"""
    monkeypatch.setenv("SWA_D1_PLAIN", "1")
    db, _ = P.star_database(L)
    ctx = Context(0)
    try:
        upload(ctx, db)
        assert ctx.d1_index_build() is False
        for ncb in (False, True):
            _star_network(ctx, L, ncb)
    finally:
        ctx.close()


@pytest.mark.parametrize("plain", [True, False])
@pytest.mark.parametrize("L", [64, 128])
def test_ownership_partials_of_the_stars_add_up(monkeypatch, L, plain):
    """world 2 and 3: the ranks' partial rows hold every link of the network once (plain route: seeds by id mod world)"""
    if plain:
        monkeypatch.setenv("SWA_D1_PLAIN", "1")
    db, _ = P.star_database(L)
    woff, wnb, _ = _oracle(L, False)
    whole = link_keys(woff, wnb)
    ctx = Context(0)
    try:
        upload(ctx, db)
        assert ctx.d1_index_build() is False
        for world, rebuild in ((2, False), (2, True), (3, True)):
            parts = []
            for rank in range(world):
                ctx.d1_set_ownership(rank, world)
                if rebuild:
                    assert ctx.d1_index_build() is False
                poff, pnb = ctx.d1_network()
                keys = link_keys(poff, pnb)
                assert (np.diff(keys) > 0).all()
                parts.append(keys)
            assert np.array_equal(np.sort(np.concatenate(parts)), whole), (L, plain, world)
            assert all(len(p) > 0 for p in parts)
        ctx.d1_set_ownership(0, 1)
        assert ctx.d1_index_build() is False
        _star_network(ctx, L, False)
    finally:
        ctx.close()


_long_db = functools.lru_cache(maxsize=None)(lambda longest: P.to_db(P.long_records(longest)))
_long_oracle = functools.lru_cache(maxsize=None)(lambda longest, ncb: oracle_sorted_rows(_long_db(longest), ncb))


@pytest.mark.parametrize("plain", [True, False])
@pytest.mark.parametrize("longest,zobrist_lds", [(3070, 1), (3071, 0)])
def test_zobrist_table_in_lds_and_in_memory(monkeypatch, longest, zobrist_lds, plain):
    """partial stars (lane_positions) of centres of longest, longest - 1 and longest - 2 nt and 200 unrelated sequences of 150
    nt: 3070 is the launch with the most dynamic LDS that k_seqhash<true> and k_d1_probe<true, .> ever get"""
    if plain:
        monkeypatch.setenv("SWA_D1_PLAIN", "1")
    db = _long_db(longest)
    assert db.longest == longest
    ctx = Context(0)
    try:
        upload(ctx, db)
        assert ctx.d1_index_build() is False
        assert ctx.d1_fastidious_plan()[6] == zobrist_lds
        for ncb in (False, True):
            off, nb = ctx.d1_network(ncb)
            woff, wnb, _ = _long_oracle(longest, ncb)
            assert np.array_equal(off, woff) and np.array_equal(nb, wnb), (longest, plain, ncb)
        assert len(nb) > db.n
    finally:
        ctx.close()


def _giant_member(db):
    """a member of giant_group_db's one big group: the most frequent first 40 nucleotides"""
    heads = {}
    for i in range(db.n):
        heads.setdefault(db.seq_str(i)[:40], []).append(i)
    members = max(heads.values(), key=len)
    assert len(members) >= 2600
    return members[len(members) // 2]


@functools.lru_cache(maxsize=None)
def _giant_with_star():
    base = giant_group_db()
    return P.with_star_of(base, _giant_member(base))


def test_fallback_seeds_by_position():
    """giant_group_db and the full star of a member of its oversized group, on the default (anchored) route: the star's
    seeds are fallback seeds of k_d1_probe<., 2> with range 1 (positions from the prefix window on) and range 2 (positions
    inside it), an edit at every position among them — 31 / 32 and the run that holds the window's last position too"""
    db, cent = _giant_with_star()
    assert 85 <= len(cent) <= 87 and db.n > 3000 + P.star_size(cent) - 100
    ids = {db.seq_str(i): i for i in range(db.n)}
    ctx = Context(0)
    try:
        for ncb in (False, True):
            off, nb = check_vs_oracle(ctx, db, ncb)
            assert ctx.d1_anchor_width() != 0                       # the anchored route
            row = set(nb[int(off[ids[cent]]):int(off[ids[cent] + 1])].tolist())
            if ncb:
                assert row == {ids[s] for s in P.v1(cent)}          # every edit at every position found from the centre
    finally:
        ctx.close()


def test_fallback_seeds_in_window_mode(monkeypatch, tmp_path):
    """conserved flanks under 32-nt anchors: the windows move inwards and the oversized groups' seeds go through
    k_d1_probe<., 2> with every position enumerated and the hits filtered by window; one member has its full star"""
    monkeypatch.setenv("SWA_D1_ANCHOR_W", "32")
    fa = tmp_path / "in.fa"
    conserved_flank_set(fa, 30000, 72)
    db, cent = P.with_star_of(S.db_from_fasta(fa), 12345)
    ids = {db.seq_str(i): i for i in range(db.n)}
    ctx = Context(0)
    try:
        for ncb in (False, True):
            off, nb = check_vs_oracle(ctx, db, ncb)
            assert ctx.d1_anchor_windows()[0] >= 32                 # the windows did move
            if ncb:
                row = set(nb[int(off[ids[cent]]):int(off[ids[cent] + 1])].tolist())
                assert row == {ids[s] for s in P.v1(cent)}
    finally:
        ctx.close()


def _edges(ctx, want, ncb=False):
    """the flat link list of the whole database, sorted: (source << 32 | target) as link_keys gives them"""
    d_links = S.DeviceArray(len(want) + 16, np.uint64)
    try:
        total = ctx.d1_network_edges_device(d_links, len(want) + 16, ncb)
        assert total == len(want)
        return np.sort(d_links.to_host(total))
    finally:
        d_links.free()


@pytest.mark.parametrize("first_form", ["csr", "edges"])
@pytest.mark.parametrize("plain", [True, False])
@pytest.mark.parametrize("seg_cap", [1, 2, 63, 64, 65])
def test_segments_regrow(monkeypatch, seg_cap, plain, first_form):
    """SWA_D1_SEG_CAP (read once per context) on the 64-nt stars: a centre alone has more than 400 links, so the wave that
    serves it overflows its segment and the segments are regrown — in the first call, whichever form it has; the later
    calls start from the grown segments.  The oracle's network every time."""
    L = 64
    monkeypatch.setenv("SWA_D1_SEG_CAP", str(seg_cap))
    if plain:
        monkeypatch.setenv("SWA_D1_PLAIN", "1")
    db, info = P.star_database(L)
    assert min(size for _, size in info.values()) - 1 > 2 * 65
    woff, wnb, _ = _oracle(L, False)
    whole = link_keys(woff, wnb)
    ctx = Context(0)
    try:
        upload(ctx, db)
        assert ctx.d1_index_build() is False
        for form in (first_form, first_form, "edges" if first_form == "csr" else "csr"):
            if form == "csr":
                _star_network(ctx, L, False)
            else:
                assert np.array_equal(_edges(ctx, whole), whole), (seg_cap, plain, form)
    finally:
        ctx.close()
