"""Inputs and the lock-step driver for the tests of the d >= 2 scan divided among several ranks
(tests/test_multi_scan_gpu.py): the sets and the model of tests/scan_sets.py and tests/scan_model.py, a MultiContext in
the place of the single context, and the bodies of the cases that need a process of their own (SWA_SCAN_PAIR_CAP is read
once per context).  Not product code."""
from __future__ import annotations

import numpy as np

import scan_model as M
import scan_sets as X
import support as S
from swarm_amd import scan_owner_for

WORLDS = (1, 2, 3, 8)


class MultiLockstep(X.Lockstep):
    """scan_sets.Lockstep over the ranks of a MultiContext (which answers scan_begin / scan_batch / scan_fetch /
    scan_totals as a Context does): every call compared exactly with the model — return code, nhits, the merged triples,
    and what the call added to the totals: comparisons and pairs summed over the ranks, one launch sequence."""

    def __init__(self, multi, db, d: int, ncb: bool = False, penalties=(18, 24, 13), model: M.ScanModel | None = None):
        self.ctx, self.db, self.d, self.ncb = multi, db, d, ncb
        multi.upload_db(db.seqs, db.seq_off, db.seqlen, db.abundance, db.longest)
        multi.dn_begin(d, *penalties)
        self.model = model or M.ScanModel(db, d, penalties)
        self.begin()


def rank_states(multi) -> list:
    return [multi.ctx(r).scan_debug_state() for r in range(multi.size())]


def rank_deltas(multi, before: list) -> list:
    return [X.state_delta(multi.ctx(r), before[r]) for r in range(multi.size())]


def cut(db, n: int):
    """the first n amplicons of db as a database of their own (the order stays: it is the abundance order already)"""
    out = S.build_db([(db.headers[i], db.seq_str(i).encode()) for i in range(n)])
    assert out.headers == db.headers[:n]
    return out


def wide_tie_set():
    """scan_sets.tie_set with enough families for 32 * 8 + 1 amplicons"""
    db, _ = X.tie_set(seed=23, families=26, members=12, length=90, d=3)
    assert db.n >= 257, db.n
    return db


# ------------------------------------------------------------------------------------------------ overflow on one rank

OVERFLOW_CAP = 64


def lopsided_set(seed: int = 5, length: int = 100, n: int = 256, strays: int = 3):
    """d = 2, for two ranks.  Amplicon 0 is a centre; strictly falling abundances fix the order.  Every other amplicon of
    rank 0's blocks (ids 32 k .. 32 k + 31, k even) is the centre with one substitution: 127 pairs for rank 0 in the
    first-generation batch.  Rank 1's blocks hold unrelated sequences, but for `strays` such variants in each."""
    rng = np.random.default_rng(seed)
    c = X._rand(rng, length)
    every = [X.sub(c, p, sh) for p in range(length) for sh in (1, 2, 3)]
    every = [every[k] for k in rng.permutation(len(every))]
    recs = []
    for i in range(n):
        near = (i >> 5) % 2 == 0 or (i & 31) < strays
        s = c if i == 0 else every.pop() if near else X._rand(rng, length)
        recs.append((f"a{i:04d}", 100000 - i, s))
    db, _ = X.make_db(recs)
    assert [h.decode() for h in db.headers] == [f"a{i:04d}_{100000 - i}" for i in range(n)]
    return db


def run_lopsided(multi, first_cap: int) -> list:
    """The overflow case on a fresh two-rank MultiContext whose pair arrays start at first_cap: -> the ranks' debug deltas"""
    d = 2
    db = lopsided_set()
    model = M.ScanModel(db, d)
    # the ranks' shares of the first batch's pairs, from the model and swa_scan_owner_for, before the GPU is asked anything
    pairs = [0, 0]
    for i in range(1, db.n):
        if model.qgram_diff(0, i) <= d:
            pairs[scan_owner_for(i, 2)] += 1
    assert pairs[0] > first_cap >= pairs[1] > 0, pairs
    before = rank_states(multi)
    assert all(b["pair_cap"] == 0 for b in before)
    want = M.model_greedy(model)
    lock = MultiLockstep(multi, db, d, model=model)
    first = lock.call([0], [0], 1, True)                 # (the totals of this call are exact: the repeated pass is not counted twice)
    assert lock.calls[0][2] == sum(pairs) and len(first) == sum(pairs)
    after_first = rank_deltas(multi, before)
    assert [x["redone"] for x in after_first] == [1, 0], after_first
    lock.begin()
    assert lock.walk() == want
    delta = rank_deltas(multi, before)
    assert [x["redone"] for x in delta] == [1, 0], delta  # (rank 0's arrays have grown: no second redo; rank 1 never needed one)
    caps = [s["pair_cap"] for s in rank_states(multi)]
    assert caps[0] > pairs[0] and caps[1] == first_cap, caps
    return delta


def child(case: str, first_cap: int) -> None:
    """what `python -c` runs under SWA_SCAN_PAIR_CAP=<first_cap>; prints `ok <debug deltas>`"""
    from swarm_amd import MultiContext
    multi = MultiContext([0, 0])
    try:
        if case == "lopsided":
            out = run_lopsided(multi, first_cap)
        else:
            raise ValueError(case)
    finally:
        multi.close()
    print("ok", out)
