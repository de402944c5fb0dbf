"""The yardstick of tests/test_plain_forms_gpu.py and tests/test_bloom_forms_gpu.py pinned on the CPU: the oracle against
the definition on the sets of tests/plain_sets.py, the closed forms of those sets, and the proofs that the sets are
worth running (a run across a lane boundary in every run-built centre; more true tasks in the batch set than the task
cap its test forces).  No GPU."""
import numpy as np
import pytest

import plain_sets as P
import support as S


def one_edit_apart(a: str, b: str) -> bool:
    """the definition, as tests/test_pair_identity.py states it"""
    if a == b or abs(len(a) - len(b)) > 1:
        return False
    if len(a) == len(b):
        return sum(x != y for x, y in zip(a, b)) == 1
    s, l = (a, b) if len(a) < len(b) else (b, a)
    return any(l[:p] + l[p + 1:] == s for p in range(len(l)))


def definition_links(seqs: list) -> set:
    """{(i, j), i != j: one_edit_apart(seqs[i], seqs[j])}, the same definition without the quadratic loop: equal lengths by
    counting the differing positions of all pairs at once; lengths n and n + 1 by looking every single deletion
    l[:p] + l[p + 1:] of the longer sequence up among the shorter ones"""
    by_len = {}
    for i, s in enumerate(seqs):
        by_len.setdefault(len(s), []).append(i)
    links = set()
    for n, ids in by_len.items():
        codes = np.array([np.frombuffer(seqs[i].encode(), dtype=np.uint8) for i in ids])
        for a, i in enumerate(ids):
            for b in np.flatnonzero((codes != codes[a]).sum(axis=1) == 1):
                links.add((i, ids[int(b)]))
        shorter = {seqs[j]: j for j in by_len.get(n - 1, [])}
        for i in ids:
            l = seqs[i]
            for j in {shorter[t] for t in (l[:p] + l[p + 1:] for p in range(n)) if t in shorter}:
                links |= {(i, j), (j, i)}
    return links


def definition_network(db: S.Db, links: set, ncb: bool):
    rows = [[] for _ in range(db.n)]
    for i, j in links:
        if ncb or db.abundance[i] >= db.abundance[j]:
            rows[i].append(j)
    off = np.zeros(db.n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.array([j for r in rows for j in sorted(r)], dtype=np.uint32)


def oracle_sorted(db: S.Db, ncb: bool):
    off, nb, dup = S.oracle_d1_network(db, ncb)
    assert not dup
    nb = nb.copy()
    for i in range(db.n):
        nb[int(off[i]):int(off[i + 1])].sort()
    return off, nb


@pytest.mark.parametrize("L", [1, 2, 3, 31])
def test_fast_definition_is_the_definition(L):
    """definition_links against one_edit_apart on every pair, where every pair is affordable"""
    db, _ = P.star_database(L)
    seqs = [db.seq_str(i) for i in range(db.n)]
    want = {(i, j) for i in range(db.n) for j in range(db.n) if one_edit_apart(seqs[i], seqs[j])}
    assert definition_links(seqs) == want and len(want) > 0


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("L", P.IDENTITY_LENGTHS)
def test_oracle_network_of_a_star_is_the_definition(L, kind):
    cent = P.centre(kind, L)
    recs = P.star(cent)
    db = P.to_db(recs)
    assert [h.decode() for h in db.headers] == [h for h, _ in recs]          # star() comes in db order
    assert db.n == len(recs) == len({s for _, s in recs}) == P.star_size(cent) == len(P.v1(cent)) + 1
    seqs = [db.seq_str(i) for i in range(db.n)]
    assert seqs[0] == cent and db.abundance[0] > db.abundance[1:].max(initial=0)
    assert db.n < 8 or set(db.abundance[1:].tolist()) == {1, 2, 3}        # ties and both sides of >=
    links = definition_links(seqs)
    for ncb in (False, True):
        off, nb = oracle_sorted(db, ncb)
        woff, wnb = definition_network(db, links, ncb)
        assert np.array_equal(off, woff) and np.array_equal(nb, wnb), (L, kind, ncb)
        assert int(off[1]) == len(recs) - 1                                  # the centre's row: everybody else


@pytest.mark.parametrize("L", P.IDENTITY_LENGTHS)
def test_closed_forms(L):
    """3 L substitutions, one deletion per run, 3 L + 4 insertions; the random centre's from its runs counted here"""
    cent = P.centre("random", L)
    runs = 1 + sum(a != b for a, b in zip(cent, cent[1:]))
    assert len(P.star(cent)) == 1 + 3 * L + (runs if L > 1 else 0) + 3 * L + 4
    assert len(P.star("A" * L)) == 1 + 3 * L + (1 if L > 1 else 0) + 3 * L + 4
    for kind in P.KINDS:
        c = P.centre(kind, L)
        assert len(c) == L and len(P.star(c)) == P.star_size(c)
        # a partial star is the part of the star whose edit can be made at one of the positions
        part = {s for _, s in P.star(c, P.lane_positions(L))}
        assert part <= {s for _, s in P.star(c)} and c in part
    assert all(3 <= n <= 11 for _, n in P.runs_of(P.centre("runs", L))[:-1]) or L < 3


@pytest.mark.parametrize("L", sorted(set(P.LANE_LENGTHS) | {3068, 3069, 3070, 3071}))
def test_run_built_centre_has_a_run_across_a_lane_boundary(L):
    c = P.centre("runs", L)
    assert len(c) == L
    if P.lanes_k(L) >= 2:
        assert P.run_spans_lane_boundary(c)


@pytest.mark.parametrize("L", P.LANE_LENGTHS)
def test_star_database_loses_no_member(L):
    """the four stars in one database: every sequence of every star is there once, each centre has the highest abundance"""
    db, info = P.star_database(L)
    seqs = {db.seq_str(i) for i in range(db.n)}
    assert len(seqs) == db.n
    for kind, (cid, size) in info.items():
        c = P.centre(kind, L)
        assert db.seq_str(cid) == c and int(db.abundance[cid]) == P.CENTRE_ABUNDANCE == int(db.abundance.max())
        assert P.v1(c) <= seqs and size == len(P.v1(c)) + 1
    if L >= 64:
        assert db.n == sum(size for _, size in info.values())                # long stars are disjoint
    assert db.n <= 6000


def test_lane_positions():
    for L in (1, 2, 63):
        assert P.lane_positions(L) == list(range(L + 1))                     # K = 1: every position
    for L, K in ((64, 2), (127, 2), (128, 3), (192, 4), (3070, 48), (3071, 48), (3072, 49)):
        lp = P.lane_positions(L)
        assert P.lanes_k(L) == K and lp[0] == 0 and lp[-1] == L and L - 1 in lp
        assert {m + o for m in range(K, L, K) for o in (-1, 0, 1)} <= set(lp)
        assert {m + o for m in range(32, L, 32) for o in (-1, 0, 1)} <= set(lp)
    assert 64 * P.lanes_k(64) > 64 and 64 * (P.lanes_k(64) - 1) <= 64       # K = ceil((len + 1) / 64)


def test_long_records_stay_within_the_longest():
    for longest in (3070, 3071):
        recs = P.long_records(longest)
        assert max(len(s) for _, s in recs) == longest and len({s for _, s in recs}) == len(recs)
        assert sum(len(s) == 150 for _, s in recs) == 200
        assert {len(s) for _, s in recs} == {150, *range(longest - 3, longest + 1)}
        # the Zobrist table of longest + 2 positions: in LDS up to 96 KiB
        assert (32 * (longest + 2) <= 96 * 1024) == (longest == 3070)


# ---- the shells ----------------------------------------------------------------------------------------------------------------

def _set_arithmetic(db, flags):
    """(graft candidates, candidate count) from the microvariant sets: a light x takes the smallest heavy h with a common
    microvariant; every common microvariant of every such pair is one candidate"""
    seqs = [db.seq_str(i) for i in range(db.n)]
    v1 = {i: P.v1(seqs[i]) for i in range(db.n)}
    graft = np.full(db.n, P.NO_GRAFT, dtype=np.uint32)
    count = 0
    for h in np.flatnonzero(flags == 0):
        for x in np.flatnonzero(flags != 0):
            if abs(len(seqs[h]) - len(seqs[x])) <= 2:
                common = len(v1[h] & v1[x])
                count += common
                if common:
                    graft[x] = min(int(graft[x]), int(h))
    return graft, count


@pytest.mark.parametrize("L", P.SHELL_LENGTHS)
def test_shells_graft_as_the_set_arithmetic_says(L):
    db, flags, three = P.shell_case(L)
    ids = {h.decode(): i for i, h in enumerate(db.headers)}
    graft, counters = S.oracle_fastidious(db, flags, 16)
    want, count = _set_arithmetic(db, flags)
    assert np.array_equal(graft, want) and int(counters[2]) == count
    assert (graft[flags == 0] == P.NO_GRAFT).all()
    # every two-edit sequence grafts, onto its centre (header x<c>...) or onto a heavy amplicon with a
    # smaller id; no three-edit sequence does
    cents = [ids.get(f"h{c}_{90 - c}") for c in range(3)]
    two = [i for h, i in ids.items() if h.startswith("x") and "t" not in h]
    assert len(two) >= (100 if L >= 31 else 3)
    for h, i in ids.items():
        if h.startswith("x") and "t" not in h and flags[i]:
            own = cents[int(h[1])]
            assert graft[i] != P.NO_GRAFT and (own is None or graft[i] <= own), h
    assert len(three) >= (1 if L >= 31 else 0)
    for h in three:
        assert flags[ids[h]] and graft[ids[h]] == P.NO_GRAFT, h
    if L >= 31:
        got = np.flatnonzero(graft != P.NO_GRAFT)
        assert {int(db.seqlen[x]) - int(db.seqlen[graft[x]]) for x in got} == {-2, -1, 0, 1, 2}
        assert int(counters[2]) > 2 * len(got)                               # pairs with several common microvariants


@pytest.mark.parametrize("longest", [3070, 3071])
def test_long_shells_graft_onto_their_centres(longest):
    """the set arithmetic is not affordable at 3 kb; the candidates are: the shell of a centre grafts onto that centre or a
    smaller heavy id, the three-edit sequences and the unrelated ones not at all"""
    db, flags, three = P.long_shell_case(longest)
    ids = {h.decode(): i for i, h in enumerate(db.headers)}
    graft, counters = S.oracle_fastidious(db, flags, 16)
    lights = [h for h, i in ids.items() if flags[i] and h not in three]
    assert len(lights) >= 200 and len(three) >= 4 and int(counters[2]) >= 2 * len(lights)
    for h in lights:
        own = ids[f"h{h[1:3]}_{90 - int(h[2])}"]
        assert graft[ids[h]] <= own, h
    for h in three:
        assert graft[ids[h]] == P.NO_GRAFT, h
    assert {int(db.seqlen[i]) for i in np.flatnonzero(flags)} >= set(range(longest - 4, longest + 1))


# ---- the batch set -------------------------------------------------------------------------------------------------------------

def test_batch_set_overflows_the_forced_cap():
    """the true surviving tasks of the dense heavy amplicons — microvariants of theirs that are microvariants of a light
    amplicon too, what the flexible Bloom filter must pass whatever its false positives add — exceed the cap of one heavy
    amplicon's worth that the test forces, so the batch that takes them all at once must be redone"""
    db, flags, first_dense, cap = P.batch_set()
    assert db.n <= 64 and cap == 7 * db.longest + 4
    seqs = [db.seq_str(i) for i in range(db.n)]
    light_variants = set().union(*(P.v1(seqs[x]) for x in np.flatnonzero(flags)))
    heavy = np.flatnonzero(flags == 0)
    assert list(heavy) == list(range(len(heavy)))                            # heavy first: the list is in id order
    true_tasks = [len(P.v1(seqs[h]) & light_variants) for h in heavy]
    assert true_tasks[:first_dense] == [0] * first_dense and first_dense >= 1
    assert sum(true_tasks[first_dense:]) > cap
    assert max(len(P.v1(seqs[h])) for h in heavy) <= cap                      # one heavy amplicon alone always fits
    graft, counters = S.oracle_fastidious(db, flags, 16)
    want, count = _set_arithmetic(db, flags)
    assert np.array_equal(graft, want) and int(counters[2]) == count and count > 0
    assert (graft[flags != 0] != P.NO_GRAFT).all() and (graft[flags != 0] >= first_dense).all()
