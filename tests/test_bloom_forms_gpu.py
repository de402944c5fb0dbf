"""The Bloom route of the --fastidious pass (swarm_amd/csrc/fastidious.hip: fastidious_bloom_route, k_d1_flex<ZLDS, PASS 0 / 1>,
k_d1_probe<ZLDS, 1>) against S.oracle_fastidious, at the edges of enumerate_variants' lane partition and through every
branch of its batch loop.  It serves every pair with a member shorter than 112 nt and every pair of a database whose
longest sequence exceeds 1004 nt.

swa_d1_fastidious takes the light flags from the caller, so no clustering is needed: heavy = centres and some of their
single-edit sequences, light = sequences two edits from a centre, one per pair of positions (tests/plain_sets.py:
shell_case, position_pairs — both edits on one lane, on neighbouring lanes, insertion + deletion, ...), and a few three
edits away that must not graft.  A heavy amplicon of 63 nt has 64-nt microvariants that k_d1_probe<., 1> enumerates with
K = 2; one of 64 nt has 65-nt ones that need a third staged word.

The batch loop runs in a test only under SWA_FAST_TASK_CAP, which puts n tasks in the place of the list's 1 GiB;
swa_d1_fastidious_bloom_batches reports launches, redone batches, the cap and the fullest batch.
tests/test_plain_identity.py shows on the CPU what these sets hold.  Graft candidates and counters are integers:
compared exactly."""
import numpy as np
import pytest

import plain_sets as P
import support as S
from d1_sets import upload
from swarm_amd import D1Clusters, HostDb

pytestmark = pytest.mark.gpu
HOOK = "SWA_FAST_TASK_CAP"


def _resident(ctx, db):
    upload(ctx, db)
    assert ctx.d1_index_build() is False


def _pass(ctx, db, flags, shard=None):
    """one pass on the resident database (the pass re-purposes the table: the index is made again first)"""
    assert ctx.d1_index_build() is False
    light_nt = int(db.seqlen[flags != 0].astype(np.uint64).sum())
    graft, counters = ctx.d1_fastidious(flags, light_nt, 16, *(shard or ()))
    return graft, [int(x) for x in counters[:5]]


def _check(ctx, db, flags, label):
    graft, counters = _pass(ctx, db, flags)
    want_graft, want_counters = S.oracle_fastidious(db, flags, 16)
    print(f"{label}: n {db.n} light {int(flags.sum())} counters {counters} / {[int(x) for x in want_counters[:5]]} "
          f"grafts differ at {int((graft != want_graft).sum())} batches {ctx.d1_fastidious_bloom_batches()}")
    assert np.array_equal(graft, want_graft), label
    assert counters == [int(x) for x in want_counters[:5]], label
    return graft, counters


@pytest.mark.parametrize("L,forced", [(L, True) for L in P.SHELL_LENGTHS] + [(L, False) for L in P.SHELL_LENGTHS if L + 2 < 112])
def test_shells_on_the_bloom_route(gpu_ctx, monkeypatch, L, forced):
    """under SWA_FAST_BLOOM=1 and, where the Bloom route is the default (longest < 112), without it"""
    db, flags, three = P.shell_case(L)
    assert db.longest <= L + 2
    if forced:
        monkeypatch.setenv("SWA_FAST_BLOOM", "1")
    _resident(gpu_ctx, db)
    plan = gpu_ctx.d1_fastidious_plan()
    assert plan[0] == 0 and plan[6] == 1                            # no pair route; the Zobrist table in LDS
    graft, counters = _check(gpu_ctx, db, flags, f"shells {L} forced {forced}")
    totals, batches = gpu_ctx.d1_fastidious_totals(), gpu_ctx.d1_fastidious_bloom_batches()
    assert totals[0] == 0 and totals[1] == int(flags.sum()) and totals[2] == db.n - int(flags.sum())
    # the hook is off: one launch takes every heavy amplicon, nothing is redone
    assert batches[:2] == [1, 0] and batches[2] >= totals[2] * (7 * db.longest + 4) >= batches[3] > 0
    ids = {h.decode(): i for i, h in enumerate(db.headers)}
    assert all(graft[ids[h]] == P.NO_GRAFT for h in three)
    assert (graft[flags != 0] != P.NO_GRAFT).sum() >= (100 if L >= 31 else 3)


@pytest.mark.parametrize("longest,zobrist_lds", [(3070, 1), (3071, 0)])
def test_long_shells(gpu_ctx, longest, zobrist_lds):
    """the Bloom route as the default of a long database: k_d1_flex<true, .> and k_d1_probe<true, 1> at their largest LDS
    (3070), k_d1_flex<false, .> and k_d1_probe<false, 1> (3071); shells at lane_positions of centres of longest,
    longest - 1 and longest - 2 nt"""
    db, flags, three = P.long_shell_case(longest)
    _resident(gpu_ctx, db)
    plan = gpu_ctx.d1_fastidious_plan()
    assert plan[0] == 0 and plan[6] == zobrist_lds
    graft, _ = _check(gpu_ctx, db, flags, f"long shells {longest}")
    assert gpu_ctx.d1_fastidious_bloom_batches()[:2] == [1, 0]
    ids = {h.decode(): i for i, h in enumerate(db.headers)}
    assert all(graft[ids[h]] == P.NO_GRAFT for h in three) and (graft != P.NO_GRAFT).sum() >= 200


def test_two_shards_combine_to_the_whole(gpu_ctx):
    db, flags, _ = P.shell_case(64)
    _resident(gpu_ctx, db)
    whole, counters = _check(gpu_ctx, db, flags, "shells 64 unsharded")
    parts = [_pass(gpu_ctx, db, flags, (shard, 2)) for shard in range(2)]
    assert np.array_equal(np.minimum(parts[0][0], parts[1][0]), whole)
    assert not np.array_equal(parts[0][0], parts[1][0])
    assert [parts[0][1][0], parts[0][1][1] + parts[1][1][1], parts[0][1][2] + parts[1][1][2]] == counters[:3]
    assert parts[0][1][0] == parts[1][1][0]


# ---- the batch loop ------------------------------------------------------------------------------------------------------------

def test_an_overflowing_batch_is_redone(gpu_ctx, monkeypatch):
    """plain_sets.batch_set under a cap of one heavy amplicon's worth of tasks (7 longest + 4).  The first batch is heavy
    amplicon 0 alone, which has no light amplicon near and leaves (next to) no task; from that rate the loop takes all
    the others at once; the dense ones among them make more true tasks than the cap holds (test_plain_identity.py), so
    that batch is redone one amplicon at a time.  If no batch was redone, this test has not tested the redo."""
    db, flags, first_dense, cap = P.batch_set()
    _resident(gpu_ctx, db)
    free_graft, free_counters = _check(gpu_ctx, db, flags, "batch set, hook off")
    free = gpu_ctx.d1_fastidious_bloom_batches()
    assert free[:2] == [1, 0] and free[3] > cap                     # all at once, more tasks than the cap to come
    monkeypatch.setenv(HOOK, str(cap))
    graft, counters = _check(gpu_ctx, db, flags, "batch set, hook on")
    launches, redone, cap_used, fullest = gpu_ctx.d1_fastidious_bloom_batches()
    assert cap_used == cap and fullest <= cap
    assert redone >= 1 and launches >= 3
    assert np.array_equal(graft, free_graft) and counters == free_counters
    monkeypatch.delenv(HOOK)
    _check(gpu_ctx, db, flags, "batch set, hook off again")
    assert gpu_ctx.d1_fastidious_bloom_batches() == free


def _generated(tmp_path):
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 4000, 80, 61, 1, 0.3)
    hdb = HostDb(fa)
    db = S.db_from_fasta(fa)
    off, nb, dup = S.oracle_d1_network(db)
    assert not dup
    flags, stats = D1Clusters(hdb, off, nb).light_flags(3)
    return db, np.asarray(flags, dtype=np.uint8)


def test_many_batches(gpu_ctx, tmp_path, monkeypatch):
    """a few thousand amplicons of about 80 nt under SWA_FAST_BLOOM=1 with caps of exactly one heavy amplicon a batch, of
    all but one task of what all of them could make (two batches, the second tiny) and of a value in between: the offset
    into the heavy list, the optimistic sizing and the last partial batch.  (No exact batch counts: the order of the
    heavy list is not fixed beyond 64 consecutive ids.)"""
    monkeypatch.setenv("SWA_FAST_BLOOM", "1")
    db, flags = _generated(tmp_path)
    assert 60 <= int(db.seqlen.min()) and db.longest <= 100 and 2000 <= db.n
    _resident(gpu_ctx, db)
    free_graft, free_counters = _check(gpu_ctx, db, flags, "generated, hook off")
    free = gpu_ctx.d1_fastidious_bloom_batches()
    n_heavy, maxv = gpu_ctx.d1_fastidious_totals()[2], 7 * db.longest + 4
    assert n_heavy == db.n - int(flags.sum()) > 1000 and (free_graft != P.NO_GRAFT).sum() > 50
    assert free[:3] == [1, 0, n_heavy * maxv] and 0 < free[3] <= free[2]
    for cap in (maxv, n_heavy * maxv // 9, n_heavy * maxv - 1):
        monkeypatch.setenv(HOOK, str(cap))
        graft, counters = _check(gpu_ctx, db, flags, f"generated, cap {cap}")
        launches, redone, cap_used, fullest = gpu_ctx.d1_fastidious_bloom_batches()
        assert cap_used == cap and launches >= 2 and redone < launches
        assert 0 < fullest <= cap_used
        assert np.array_equal(graft, free_graft) and counters == free_counters
    # a cap below one heavy amplicon's worth is lifted to it; zero and a negative value are no hook at all
    for value, want_cap in (("1", maxv), ("0", n_heavy * maxv), ("-5", n_heavy * maxv)):
        monkeypatch.setenv(HOOK, value)
        graft, counters = _check(gpu_ctx, db, flags, f"generated, hook {value}")
        assert gpu_ctx.d1_fastidious_bloom_batches()[2] == want_cap
        assert np.array_equal(graft, free_graft) and counters == free_counters
    monkeypatch.delenv(HOOK)
    _check(gpu_ctx, db, flags, "generated, hook off again")
    assert gpu_ctx.d1_fastidious_bloom_batches() == free


def test_no_bloom_route_no_report(gpu_ctx, tmp_path):
    """a database of 150-nt amplicons: every pair is the pair route's, and the report is all zero"""
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 3000, 150, 62, 1, 0.3)
    db = S.db_from_fasta(fa)
    off, nb, _ = S.oracle_d1_network(db)
    flags = np.asarray(D1Clusters(HostDb(fa), off, nb).light_flags(3)[0], dtype=np.uint8)
    assert int(db.seqlen.min()) > 113                               # nobody in the short band
    _resident(gpu_ctx, db)
    _check(gpu_ctx, db, flags, "150 nt")
    assert gpu_ctx.d1_fastidious_plan()[0] == 1 and gpu_ctx.d1_fastidious_totals()[1:3] == [0, 0]
    assert gpu_ctx.d1_fastidious_bloom_batches() == [0, 0, 0, 0]
