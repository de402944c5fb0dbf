"""Seam B5 on several ranks: the -u alignments divided among the ranks of a MultiContext (swa_multi_nw_batch,
swarm_amd/csrc/multi.hip) give, bit for bit, what one context gives (swa_nw_batch) — differences, alignment lengths, CIGAR
ends and text — for every world, scoring and capacity, and the writers and the command line that use them print the same
files.  Every rank is on device 0.  What one context gives is itself compared with the host aligner on drawn pairs;
tests/test_multi_nw_identity.py proves the division (nw_bounds_for) on the CPU."""
import ctypes as C
import filecmp
import os
import subprocess

import numpy as np
import pytest

import support as S
from swarm_amd import Context, D1Clusters, DnClusters, HostDb, MultiContext, SwaError, capi, d1_write_uclust, nw_align_host, nw_bounds_for
from test_nw_host import fuzz_pairs
from test_uclust_gpu import BOUND, _mutate, _write_db

pytestmark = pytest.mark.gpu
G = S.GOLDEN
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
SCORINGS = [(18, 24, 13), (2, 3, 1)]
HOST_ONLY = 254                                  # include/swarm_amd.h: a pair with |dl - ql| above the widest band is the host's


@pytest.fixture(scope="module")
def multis():
    """one MultiContext per world, made when first asked for and reused by every test"""
    made = {}

    def get(world):
        if world not in made:
            made[world] = MultiContext([0] * world)
            assert made[world].uses_rccl() is False and made[world].size() == world
        return made[world]
    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def single():
    ctx = Context(0)
    yield ctx
    ctx.close()


def _random(rng, length):
    return "".join(rng.choice(list("ACGT"), length))


@pytest.fixture(scope="module")
def case(tmp_path_factory, single):
    """One small database and about 550 pairs over it, with what a single context makes of them at both scorings: computed
    once, never changed.  `split` names twelve more pairs: six that only the host can take, then six ordinary ones, each of
    weight 600."""
    rng = np.random.default_rng(32)
    seqs, pairs = [], []

    def add(d, q):
        seqs.extend([d, q])
        pairs.append((len(seqs) - 2, len(seqs) - 1))

    for d, q in fuzz_pairs(rng, 400, max_len=1000):
        add(d, q)
    for k in range(40):                                    # just inside / just outside each LDS tier's certificate
        seed = _random(rng, int(rng.integers(300, 400)))
        for bound in BOUND:
            add(_mutate(rng, seed, bound // 18 + k % 2), seed)
    for k in range(12):                                    # 700 .. 1 150 nt: the wide tiers' pairs
        seed = _random(rng, 700 + 41 * k - (k == 11))
        add(_mutate(rng, seed, 3), seed)
    for k in range(4):                                     # |dl - ql| > 254: the host's
        seed = _random(rng, 200 + 50 * k)
        add(seed + _random(rng, HOST_ONLY + 1 + 30 * k), seed)
    pairs += [(i, i) for i in range(0, 200, 15)]           # identical pairs: the same amplicon on both sides
    split = []
    for k in range(6):
        short = _random(rng, 100)
        seqs.extend([short + _random(rng, 400), short])
        split.append((len(seqs) - 2, len(seqs) - 1))
    for k in range(6):
        seed = _random(rng, 300)
        seqs.extend([_mutate(rng, seed, 1 + k), seed])
        split.append((len(seqs) - 2, len(seqs) - 1))
    fa = tmp_path_factory.mktemp("multi_nw") / "pairs.fa"
    _write_db(fa, seqs)
    hdb = HostDb(fa)
    assert hdb.n == len(seqs) and hdb.header(5).startswith(b"s000005")
    single.upload_hostdb(hdb)
    out = {"seqs": seqs, "hdb": hdb, "split": split, "pairs": pairs,
           "d": np.array([p[0] for p in pairs], dtype=np.uint32), "q": np.array([p[1] for p in pairs], dtype=np.uint32)}
    for scoring in SCORINGS:
        diffs, cols, cigars = single.nw_batch(out["d"], out["q"], *scoring)
        out[scoring] = {"diffs": diffs, "cols": cols, "cigars": cigars, "tiers": single.nw_batch_tiers(),
                        "text_full": single.nw_batch_text_full()}
    assert 520 <= len(pairs) <= 580
    return out


def _host(seqs, d, q, scoring):
    return nw_align_host(S.pack_seq(seqs[d].encode()), len(seqs[d]), S.pack_seq(seqs[q].encode()), len(seqs[q]), *scoring)


def _handle(multis, case, world):
    m = multis(world)
    m.upload_hostdb(case["hdb"])
    return m


# ---- 1. equals a single context ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_equals_a_single_context(multis, case, world, scoring):
    m = _handle(multis, case, world)
    want = case[scoring]
    diffs, cols, cigars = m.nw_batch(case["d"], case["q"], *scoring)
    assert np.array_equal(diffs, want["diffs"]) and np.array_equal(cols, want["cols"])
    assert cigars == want["cigars"]
    rng = np.random.default_rng(world)                     # ... and the single context equals the host aligner
    for k in rng.choice(len(case["pairs"]), 50, replace=False):
        d, q = case["pairs"][k]
        assert (int(diffs[k]), int(cols[k]), cigars[k]) == _host(case["seqs"], d, q, scoring), (k, d, q)
    # the counters: sums over the ranks, a rank's own through ctx(r)
    tiers = m.nw_batch_tiers()
    bounds = nw_bounds_for(case["d"], case["q"], case["hdb"].seqlen, world)
    per_rank = [m.ctx(r).nw_batch_tiers() for r in range(world)]
    assert [sum(t) for t in per_rank] == [int(b) for b in np.diff(bounds.astype(np.int64))]
    assert tiers == [sum(t[i] for t in per_rank) for i in range(8)] and sum(tiers) == len(case["pairs"])
    totals = m.nw_batch_totals()
    assert totals == tiers[:3] + [sum(tiers[3:])]
    assert m.nw_batch_text_full() == sum(m.ctx(r).nw_batch_text_full() for r in range(world))
    if m.nw_batch_text_full() == 0 and want["text_full"] == 0:
        assert tiers == want["tiers"]
    assert tiers[7] >= 4                                   # (the pairs too far apart in length)


# ---- 2. small counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npairs", [0, 1, 2, 3])
def test_small_counts(multis, case, npairs):
    m = _handle(multis, case, 3)
    scoring = SCORINGS[0]
    m.nw_batch(case["d"][:60], case["q"][:60], *scoring)   # every rank's counters stand at something
    assert all(sum(m.ctx(r).nw_batch_tiers()) > 0 for r in range(3))
    pick = np.array([401, 7, 530][:npairs], dtype=np.int64)      # a tier pair, a fuzz pair, a long one
    d, q = case["d"][pick], case["q"][pick]
    diffs, cols, cigars = m.nw_batch(d, q, *scoring)
    want = case[scoring]
    assert np.array_equal(diffs, want["diffs"][pick]) and np.array_equal(cols, want["cols"][pick])
    assert cigars == [want["cigars"][k] for k in pick]
    bounds = nw_bounds_for(d, q, case["hdb"].seqlen, 3)
    counts = np.diff(bounds.astype(np.int64))
    assert (counts == 0).sum() >= 3 - npairs
    for r in range(3):
        assert sum(m.ctx(r).nw_batch_tiers()) == counts[r]
        if counts[r] == 0:
            c = m.ctx(r)
            assert (c.nw_batch_tiers(), c.nw_batch_totals(), c.nw_batch_text_full()) == ([0] * 8, [0] * 4, 0)
    assert sum(m.nw_batch_tiers()) == npairs


# ---- 3. one rank all host ---------------------------------------------------------------------------------------------------------
def test_one_rank_all_host(multis, case, single):
    m = _handle(multis, case, 2)
    d = np.array([p[0] for p in case["split"]], dtype=np.uint32)
    q = np.array([p[1] for p in case["split"]], dtype=np.uint32)
    assert list(nw_bounds_for(d, q, case["hdb"].seqlen, 2)) == [0, 6, 12]
    got = m.nw_batch(d, q)
    assert m.ctx(0).nw_batch_tiers()[7] == 6
    assert m.ctx(1).nw_batch_tiers()[7] == 0
    assert sum(m.ctx(0).nw_batch_tiers()) == 6 and sum(m.ctx(1).nw_batch_tiers()) == 6
    for k, (a, b) in enumerate(case["split"]):
        assert (int(got[0][k]), int(got[1][k]), got[2][k]) == _host(case["seqs"], a, b, SCORINGS[0])
    single.upload_hostdb(case["hdb"])
    want = single.nw_batch(d, q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


# ---- 4. the capacity protocol, through the library handle ------------------------------------------------------------------------
def _raw_call(m, d, q, scoring, cap, with_buffer=True):
    n = len(d)
    diffs, cols, ends = np.full(n, 0xFFFFFFFF, dtype=np.uint32), np.full(n, 0xFFFFFFFF, dtype=np.uint32), np.zeros(n, dtype=np.uint64)
    buf = C.create_string_buffer(max(cap, 1)) if with_buffer else None
    total = C.c_uint64(0)
    rc = m.lib.swa_multi_nw_batch(m.h, *scoring, n, d.ctypes.data, q.ctypes.data, diffs.ctypes.data, cols.ctypes.data, ends.ctypes.data,
                                  buf, cap, C.byref(total))
    return rc, int(total.value), diffs, cols, ends, (buf.raw[:min(cap, int(total.value))] if with_buffer else b"")


@pytest.mark.parametrize("world", [3, 8])
def test_capacity_protocol(multis, case, world):
    m = _handle(multis, case, world)
    scoring = SCORINGS[0]
    want = case[scoring]
    text = "".join(want["cigars"]).encode()
    need = len(text)
    want_ends = np.cumsum([len(c) for c in want["cigars"]]).astype(np.uint64)
    weight = int(case["hdb"].seqlen[case["d"]].astype(np.int64).sum() + case["hdb"].seqlen[case["q"]].astype(np.int64).sum())
    assert 0 < need < weight
    for cap, with_buffer in ((need - 1, True), (0, True), (0, False), (need // 2, True)):
        rc, total, diffs, cols, ends, _ = _raw_call(m, case["d"], case["q"], scoring, cap, with_buffer)
        assert rc == capi.SWA_E_CAPACITY and total == need
        assert "CIGAR buffer too small" in m.lib.swa_multi_last_error(m.h).decode()
        assert np.array_equal(diffs, want["diffs"]) and np.array_equal(cols, want["cols"]) and np.array_equal(ends, want_ends)
    # with room: exactly the need (every rank but the lowest aligns into a buffer of its own), room for every slice's bound
    # (every rank writes into the caller's buffer), and in between
    for cap in (need, weight, (need + weight) // 2, weight + 1000):
        rc, total, diffs, cols, ends, raw = _raw_call(m, case["d"], case["q"], scoring, cap)
        assert rc == capi.SWA_OK and total == need and raw == text
        assert np.array_equal(diffs, want["diffs"]) and np.array_equal(cols, want["cols"]) and np.array_equal(ends, want_ends)


# ---- 5. penalties beyond 32 bits: every pair is the host's on every rank -----------------------------------------------------------
def test_overflowing_penalties(multis, case):
    m = _handle(multis, case, 3)
    scoring = (1 << 33, 1 << 32, 1 << 30)
    pick = np.arange(0, len(case["pairs"]), 9)
    d, q = case["d"][pick], case["q"][pick]
    diffs, cols, cigars = m.nw_batch(d, q, *scoring)
    assert m.nw_batch_totals() == [0, 0, 0, len(pick)] and m.nw_batch_tiers() == [0] * 7 + [len(pick)]
    counts = np.diff(nw_bounds_for(d, q, case["hdb"].seqlen, 3).astype(np.int64))
    assert [m.ctx(r).nw_batch_tiers() for r in range(3)] == [[0] * 7 + [int(c)] for c in counts]
    for k, at in enumerate(pick):
        a, b = case["pairs"][at]
        assert (int(diffs[k]), int(cols[k]), cigars[k]) == _host(case["seqs"], a, b, scoring), (k, a, b)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(multis, case):
    m = _handle(multis, case, 2)
    n = case["hdb"].n
    d, q = case["d"][:40].copy(), case["q"][:40].copy()
    seqlen = case["hdb"].seqlen.astype(np.int64)
    for at, bad in ((39, n), (0, n + 5), (30, 0xFFFFFFFF), (17, n)):
        w = seqlen[d] + seqlen[q]
        w[at] = 0                                           # (a pair that cannot be weighed weighs nothing: its rank refuses it)
        P = np.concatenate(([0], np.cumsum(w)))
        rank = int(at >= np.searchsorted(P, int(P[-1]) // 2, "left"))
        for ids in (d, q):
            kept = ids[at]
            ids[at] = bad
            with pytest.raises(SwaError) as e:
                m.nw_batch(d, q)
            ids[at] = kept
            assert e.value.code == capi.SWA_E_ARG and f"rank {rank}: " in str(e.value) and "out of range" in str(e.value)
    diffs, cols, cigars = m.nw_batch(d, q)                  # (and the handle works on)
    assert cigars == case[SCORINGS[0]]["cigars"][:40]
    ones = np.ones(2, dtype=np.uint32)
    ends = np.zeros(2, dtype=np.uint64)
    total = C.c_uint64(0)
    for args in ((None, ones.ctypes.data, ones.ctypes.data, ones.ctypes.data, ends.ctypes.data),
                 (ones.ctypes.data, ones.ctypes.data, None, ones.ctypes.data, ends.ctypes.data),
                 (ones.ctypes.data, ones.ctypes.data, ones.ctypes.data, ones.ctypes.data, None)):
        assert m.lib.swa_multi_nw_batch(m.h, 18, 24, 13, 2, *args, None, 0, C.byref(total)) == capi.SWA_E_ARG
    fresh = MultiContext([0, 0])
    try:
        with pytest.raises(SwaError) as e:
            fresh.nw_batch([0], [0])
        assert e.value.code == capi.SWA_E_ARG and "no database" in str(e.value)
    finally:
        fresh.close()


# ---- 7. the writers, in one process ----------------------------------------------------------------------------------------------
def test_writers_in_one_process(multis, single, tmp_path, monkeypatch):
    monkeypatch.setenv("SWA_NW_CHUNK", "5")
    m = multis(3)
    hdb = HostDb(G / "d1_uclust.fasta")
    single.upload_hostdb(hdb)
    m.upload_hostdb(hdb)
    assert single.d1_index_build() is False
    off, nb = single.d1_network()
    cl = D1Clusters(hdb, off, nb)
    d1_write_uclust(cl, tmp_path / "host.u")
    d1_write_uclust(cl, tmp_path / "one.u", ctx=single)
    d1_write_uclust(cl, tmp_path / "ranks.u", ctx=m)
    assert filecmp.cmp(tmp_path / "ranks.u", tmp_path / "one.u", shallow=False)
    assert filecmp.cmp(tmp_path / "ranks.u", tmp_path / "host.u", shallow=False)
    assert filecmp.cmp(tmp_path / "ranks.u", G / "d1_uclust.u", shallow=False)
    assert sum(m.nw_batch_tiers()) > 0                      # (the ranks aligned the last chunk)
    hdb = HostDb(G / "d3_400.fasta")
    single.upload_hostdb(hdb)
    m.upload_hostdb(hdb)
    cl = DnClusters(single, hdb, 3)
    cl.write_uclust(tmp_path / "host3.u")
    cl.write_uclust(tmp_path / "one3.u", ctx=single)
    cl.write_uclust(tmp_path / "ranks3.u", ctx=m)
    assert filecmp.cmp(tmp_path / "ranks3.u", tmp_path / "one3.u", shallow=False)
    assert filecmp.cmp(tmp_path / "ranks3.u", tmp_path / "host3.u", shallow=False)
    assert filecmp.cmp(tmp_path / "ranks3.u", G / "d3_400.u", shallow=False)


# ---- 8. the command line ---------------------------------------------------------------------------------------------------------
def _cli(args, fa, tmp_path, tag, env):
    u = tmp_path / f"{tag}.u"
    r = subprocess.run([str(BIN)] + args + ["-u", str(u), "-o", str(tmp_path / f"{tag}.o"), "-l", "/dev/null", str(fa)], capture_output=True,
                       text=True, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stderr
    return u, [line for line in r.stderr.splitlines() if line.startswith("multi: ")]


@pytest.mark.parametrize("name,args", [("d1_uclust", None), ("d1_fastidious", ["-d", "1", "-f"]), ("d3_400", ["-d", "3"])])
def test_cli_divides_the_alignments(tmp_path, name, args):
    fa = G / f"{name}.fasta"
    if args is None:
        args = (G / f"{name}.args").read_text().split()
        want = G / f"{name}.u"
    else:
        want, report = _cli(args, fa, tmp_path, "one", {"SWARM_AMD_MULTI_REPORT": "1"})
        assert report == []                                 # one GPU: nothing about ranks
    assert b"\nH\t" in want.read_bytes()
    for tag, env, line in (("two", {"SWARM_AMD_DEVICES": "0,0"}, "multi: -u alignments divided among 2 ranks"),
                           ("three", {"SWARM_AMD_DEVICES": "0,0,0"}, "multi: -u alignments divided among 3 ranks"),
                           ("root", {"SWARM_AMD_DEVICES": "0,0", "SWARM_AMD_MULTI_NW": "root"}, "multi: -u alignments on rank 0 alone")):
        u, report = _cli(args, fa, tmp_path, tag, dict(env, SWARM_AMD_MULTI_REPORT="1"))
        assert report[0].startswith(f"multi: {len(env['SWARM_AMD_DEVICES'].split(','))} ranks, exchange = ")
        assert report[-1] == line and sum("-u alignments" in x for x in report) == 1
        assert filecmp.cmp(u, want, shallow=False)


def test_cli_without_u_reports_what_it_did_before(tmp_path):
    fa = G / "d1_uclust.fasta"
    r = subprocess.run([str(BIN), "-d", "1", "-o", str(tmp_path / "o"), "-l", "/dev/null", str(fa)], capture_output=True, text=True,
                       env=dict(os.environ, SWARM_AMD_DEVICES="0,0", SWARM_AMD_MULTI_REPORT="1"))
    assert r.returncode == 0, r.stderr
    assert "-u alignments" not in r.stderr and "multi: 2 ranks" in r.stderr
