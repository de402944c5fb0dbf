"""Seam B5 past the LDS tiers: long amplicons (min(dl, ql) > 1024) and distant pairs (|dl - ql| > 30, or an end cost
past the 64-lane certificate) are aligned by the wide tiers of swa_nw_batch.  Every result is compared with the host
aligner (swarm_amd.nw_align_host, the specification) pair by pair, or with the compiled reference byte for byte."""
import filecmp
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import support as S

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
SCORINGS = [(18, 24, 13), (4, 12, 1), (2, 3, 1), (10, 1, 10)]
WIDE_W = [30, 62, 126, 254]                     # band half-width of the wide tiers (1, 2, 4, 8 offsets a lane)
LIMIT_SUM = 32768                               # include/swarm_amd.h: a pair with dl + ql above this is the host's
SUB = {"A": "C", "C": "G", "G": "T", "T": "A"}


def _rand(rng, n):
    return "".join(rng.choice(list("ACGT"), int(n)))


def _write_db(path, seqs):
    """every sequence once, abundances descending: db order = list order"""
    with open(path, "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(f">s{i:06d}_{len(seqs) - i}\n{s}\n")


def _mutate(seq, subs):
    """`subs` substitutions far apart (cost exactly subs * mismatch at 18/24/13)"""
    s = list(seq)
    for p in np.linspace(3, len(s) - 4, subs).astype(int):
        s[p] = SUB[s[p]]
    return "".join(s)


def _edits(rng, seq, subs, indels):
    """a few substitutions and indels of 1 to 3 nt, at random places"""
    s = list(seq)
    for _ in range(subs):
        p = int(rng.integers(0, len(s)))
        s[p] = SUB[s[p]]
    for _ in range(indels):
        p = int(rng.integers(1, len(s) - 4))
        n = int(rng.integers(1, 4))
        if rng.random() < 0.5:
            del s[p:p + n]
        else:
            s[p:p] = list(_rand(rng, n))
    return "".join(s)


def _host_all(seqs, pairs, scoring):
    from swarm_amd import nw_align_host
    packed = {}

    def pk(i):
        if i not in packed:
            packed[i] = S.pack_seq(seqs[i].encode())
        return packed[i]

    for d, q in pairs:
        pk(d), pk(q)
    with ThreadPoolExecutor(8) as ex:               # (the aligner runs outside the interpreter lock)
        return list(ex.map(lambda p: nw_align_host(pk(p[0]), len(seqs[p[0]]), pk(p[1]), len(seqs[p[1]]), *scoring), pairs))


def _check(ctx, seqs, pairs, scoring):
    d_ids = np.array([p[0] for p in pairs], dtype=np.uint32)
    q_ids = np.array([p[1] for p in pairs], dtype=np.uint32)
    diffs, cols, cigars = ctx.nw_batch(d_ids, q_ids, *scoring)
    want = _host_all(seqs, pairs, scoring)
    for k, (d, q) in enumerate(pairs):
        assert (int(diffs[k]), int(cols[k]), cigars[k]) == want[k], (k, d, q, len(seqs[d]), len(seqs[q]))
    tiers, totals = ctx.nw_batch_tiers(), ctx.nw_batch_totals()
    assert len(tiers) == 8 and sum(tiers) == len(pairs)
    assert totals[:3] == tiers[:3] and totals[3] == sum(tiers[3:])
    return tiers


class _Set:
    def __init__(self):
        self.seqs, self.pairs = [], []

    def add(self, d, q):
        self.seqs.extend([d, q])
        self.pairs.append((len(self.seqs) - 2, len(self.seqs) - 1))

    def upload(self, ctx, tmp_path):
        from swarm_amd import HostDb
        fa = tmp_path / "pairs.fa"
        _write_db(fa, self.seqs)
        ctx.upload_hostdb(HostDb(fa))


def _new_ground(rng):
    st = _Set()
    # lengths 1 025 to about 5 000 at mixed length differences, a few edits
    for k in range(120):
        L = int(1025 + (5000 - 1025) * rng.random() ** 2.5)
        seed = _rand(rng, L)
        delta = int(rng.choice([0, 0, 3, 17, 29, 31, 45, 62, 63, 90, 126, 127, 200, 254, 255, 300]))
        at = int(rng.integers(0, L - delta))
        member = _edits(rng, seed[:at] + seed[at + delta:], int(rng.integers(0, 6)), int(rng.integers(0, 4)))
        st.add(member, seed) if k % 2 else st.add(seed, member)
    # 8 192 nt, and one pair past the documented length limit
    for delta in (0, 40, 250):
        seed = _rand(rng, 8192)
        st.add(_edits(rng, seed[delta:], 4, 2), seed)
    seed = _rand(rng, LIMIT_SUM // 2 + 10)
    st.add(_edits(rng, seed, 3, 1), seed)
    # unrelated pairs: no tier certifies them
    for k in range(10):
        st.add(_rand(rng, rng.integers(1100, 2001)), _rand(rng, rng.integers(1100, 2001)))
    # just inside / just outside every wide tier's certificate (18/24/13: cost = 18 * subs against 24 + (W + 1) * 13), as
    # long pairs that enter at the narrowest wide tier and as short ones that come down from the 64-lane LDS tier
    for W in WIDE_W:
        bound = 24 + (W + 1) * 13
        for L in (1200, 1300, 1027, 700):
            seed = _rand(rng, L)
            for extra in (0, 1):
                st.add(_mutate(seed, bound // 18 + extra), seed)
    # a length difference of W and of W + 1: one long gap and nothing else, at either end and in the middle, in both
    # directions; and the same with two substitutions on top
    for W in WIDE_W:
        for gap in (W, W + 1):
            seed = _rand(rng, 1400)
            for cut in (seed[gap:], seed[:-gap], seed[:700] + seed[700 + gap:]):
                st.add(cut, seed)
                st.add(seed, cut)
            st.add(_mutate(seed[:500] + seed[500 + gap:], 2), seed)
    # a short member against a long seed
    seed = _rand(rng, 1500)
    st.add(seed[:300], seed)
    st.add(seed, seed[600:900])
    # identical long pairs: two copies, and the same amplicon on both sides
    for L in (1025, 1600, 4096, 8192):
        seed = _rand(rng, L)
        st.add(seed, seed)
    st.pairs += [(i, i) for i in range(0, 60, 7)]
    return st


@pytest.mark.parametrize("scoring", SCORINGS)
def test_wide_tiers_equal_the_host_aligner(gpu_ctx, tmp_path, scoring):
    rng = np.random.default_rng(90 + scoring[0])
    st = _new_ground(rng)
    st.upload(gpu_ctx, tmp_path)
    tiers = _check(gpu_ctx, st.seqs, st.pairs, scoring)
    assert tiers[7] >= 1                                   # the pair past the length limit at least
    if scoring == (18, 24, 13):
        assert all(t > 0 for t in tiers[3:]), tiers        # every wide tier and the host took pairs


def _cost(cigar, diffs, scoring):
    """the alignment's cost from its CIGAR: mismatches * mm + sum over gaps of (go + len * ge)"""
    mm, go, ge = scoring
    runs = [(int(n) if n else 1, op) for n, op in re.findall(r"(\d*)([MID])", cigar)]
    gapcols = sum(n for n, op in runs if op != "M")
    return (diffs - gapcols) * mm + sum(go + n * ge for n, op in runs if op != "M")


def test_the_gpu_serves_long_and_distant_pairs(gpu_ctx, tmp_path):
    """pairs the wide tiers must certify (checked on the CPU from the host aligner's own CIGAR): none may reach the host"""
    scoring = (18, 24, 13)
    rng = np.random.default_rng(11)
    st = _Set()
    for k in range(160):
        W = WIDE_W[k % 4]
        prev = 0 if k % 4 == 0 else WIDE_W[k % 4 - 1] + 4
        block = int(rng.integers(prev, W - 12))            # one block cut out: the length difference, give or take the indels
        L = int(rng.integers(1100 + block, 4001)) if k % 8 else int(rng.integers(1100, 1400))
        seed = _rand(rng, L)
        at = int(rng.integers(0, L - block))
        member = _edits(rng, seed[:at] + seed[at + block:], 2, 1)
        st.add(member, seed) if k % 2 else st.add(seed, member)
    want = _host_all(st.seqs, st.pairs, scoring)
    entered = [0] * 4
    for (d, q), (diffs, cols, cigar) in zip(st.pairs, want):
        delta = abs(len(st.seqs[d]) - len(st.seqs[q]))
        assert min(len(st.seqs[d]), len(st.seqs[q])) > 1024 and delta <= 254
        t = next(i for i, W in enumerate(WIDE_W) if delta <= W)
        assert _cost(cigar, diffs, scoring) < scoring[1] + (WIDE_W[t] + 1) * scoring[2], (d, q, cigar)
        entered[t] += 1
    assert all(n > 0 for n in entered), entered
    st.upload(gpu_ctx, tmp_path)
    tiers = _check(gpu_ctx, st.seqs, st.pairs, scoring)
    assert tiers[7] == 0 and gpu_ctx.nw_batch_text_full() == 0, tiers
    assert tiers[3:7] == entered, (tiers, entered)         # certified where they entered: every wide tier took pairs
    assert gpu_ctx.nw_batch_totals()[3] == sum(tiers[3:7])


def test_certificates_decide_the_tier(gpu_ctx, tmp_path):
    """costs of exactly 18 * subs just below and at or above every bound 24 + (W + 1) * 13: the tier that certifies each
    pair follows from its cost alone, for long pairs (they enter at K = 1) and for short ones (from the 64-lane LDS tier)"""
    scoring = (18, 24, 13)
    rng = np.random.default_rng(23)
    bounds = [24 + (W + 1) * 13 for W in WIDE_W]
    st = _Set()
    for L in (1100, 1200, 1300, 1500, 600, 700, 900):
        for bound in bounds:
            seed = _rand(rng, L)
            for extra in (0, 1):
                st.add(_mutate(seed, bound // 18 + extra), seed)
    want = _host_all(st.seqs, st.pairs, scoring)
    expect = [0] * 8
    for (d, q), (diffs, cols, cigar) in zip(st.pairs, want):
        cost = _cost(cigar, diffs, scoring)
        assert cigar == f"{len(st.seqs[q])}M" and cost == 18 * diffs      # substitutions only: the cost is what was planted
        t = next((i for i, b in enumerate(bounds) if cost < b), 4)         # narrowest certificate the cost is below
        # (a short pair certified at W = 30 stays in the 64-lane LDS tier; its failures continue at K = 2)
        expect[2 if t == 0 and len(st.seqs[q]) <= 1024 else 3 + t] += 1
    assert all(n > 0 for n in expect[2:]), expect
    st.upload(gpu_ctx, tmp_path)
    tiers = _check(gpu_ctx, st.seqs, st.pairs, scoring)
    assert tiers == expect, (tiers, expect)


def test_slice_boundary_with_long_pairs_on_both_sides(gpu_ctx, tmp_path):
    """more than 2^20 pairs in one call: short identical pairs, long ones around the boundary between the two slices"""
    scoring = (18, 24, 13)
    rng = np.random.default_rng(5)
    st = _Set()
    st.seqs.append(_rand(rng, 40))
    for k in range(12):
        seed = _rand(rng, int(rng.integers(1100, 2500)))
        st.add(_edits(rng, seed[k * 20:], 3, 2), seed)
    long_pairs = st.pairs
    n = (1 << 20) + 40
    d_ids = np.zeros(n, dtype=np.uint32)
    q_ids = np.zeros(n, dtype=np.uint32)
    where = list(range((1 << 20) - 6, (1 << 20) + 6))
    for pos, (d, q) in zip(where, long_pairs):
        d_ids[pos], q_ids[pos] = d, q
    st.upload(gpu_ctx, tmp_path)
    diffs, cols, cigars = gpu_ctx.nw_batch(d_ids, q_ids, *scoring)
    tiers = gpu_ctx.nw_batch_tiers()
    want = _host_all(st.seqs, long_pairs, scoring)
    for pos, w in zip(where, want):
        assert (int(diffs[pos]), int(cols[pos]), cigars[pos]) == w, pos
    rest = np.ones(n, dtype=bool)
    rest[where] = False
    assert not diffs[rest].any() and (cols[rest] == 40).all() and set(np.array(cigars, dtype=object)[rest]) == {"40M"}
    assert tiers[0] == n - 12 and sum(tiers[3:7]) == 12 and tiers[7] == 0, tiers


def test_a_full_text_buffer_sends_pairs_on_and_to_the_host(gpu_ctx, tmp_path):
    """one pair the 64-lane LDS tier certifies, 4 096 times, with a CIGAR longer than the packed text buffer has room for
    (48 bytes a pair + 64 KiB): the LDS tier passes the pairs it cannot store on, the wide tier that certifies them again
    finds the buffer still full, counts them and hands them to the host"""
    from swarm_amd import nw_align_host
    scoring = (10, 1, 10)
    n = 4096
    rng = np.random.default_rng(41)
    seed = _rand(rng, 600)
    s = list(seed)
    for i, p in enumerate(np.linspace(15, 585, 20).astype(int)[::-1]):     # single-nucleotide indels, evenly spread,
        if i % 2:                                                          # insertion and deletion in turn: |dl - ql| <= 1
            s[p:p] = [SUB[s[p]]]
        else:
            del s[p]
    st = _Set()
    st.add("".join(s), seed)
    want = nw_align_host(S.pack_seq(st.seqs[0].encode()), len(st.seqs[0]), S.pack_seq(seed.encode()), len(seed), *scoring)
    diffs, cols, cigar = want
    assert abs(len(st.seqs[0]) - len(seed)) <= 1
    assert 151 <= _cost(cigar, diffs, scoring) < 311                       # past the 32-lane certificate, inside the 64-lane one
    assert len(cigar) * n > 48 * n + 65536                                 # the batch's text cannot fit
    st.upload(gpu_ctx, tmp_path)
    d_ids = np.zeros(n, dtype=np.uint32)
    q_ids = np.ones(n, dtype=np.uint32)
    got_diffs, got_cols, got_cigars = gpu_ctx.nw_batch(d_ids, q_ids, *scoring)
    assert (got_diffs == diffs).all() and (got_cols == cols).all() and set(got_cigars) == {cigar}
    assert len(got_cigars) == n
    tiers, full = gpu_ctx.nw_batch_tiers(), gpu_ctx.nw_batch_text_full()
    assert sum(tiers) == n, tiers
    assert full > 0 and tiers[7] == full, (tiers, full)                    # the wide tier's text-full branch: the only way to the host
    assert tiers[2] > 0, tiers                                             # some pairs did get their text in


# ---- the writers and the command line on long amplicons -----------------------------------------------------------

@pytest.fixture(scope="module")
def long_fasta(tmp_path_factory):
    d = tmp_path_factory.mktemp("long")
    one, two = d / "d1.fa", d / "d3.fa"
    S.gen_fasta(one, 3000, 1500, 901, 1)
    S.gen_fasta(two, 3000, 1500, 902, 2)
    return one, two


def _d1(ctx, fa):
    from swarm_amd import D1Clusters, HostDb
    hdb = HostDb(fa)
    ctx.upload_hostdb(hdb)
    ctx.d1_index_build()
    off, nb = ctx.d1_network()
    return hdb, D1Clusters(hdb, off, nb)


def _writers_d1(ctx, tmp_path, fa):
    from swarm_amd import d1_write_uclust
    hdb, cl = _d1(ctx, fa)
    d1_write_uclust(cl, tmp_path / "host.u")
    d1_write_uclust(cl, tmp_path / "gpu.u", ctx=ctx)
    assert filecmp.cmp(tmp_path / "host.u", tmp_path / "gpu.u", shallow=False)
    return (tmp_path / "gpu.u").read_bytes()


def _writers_dn(ctx, tmp_path, fa, d):
    from swarm_amd import DnClusters, HostDb
    hdb = HostDb(fa)
    ctx.upload_hostdb(hdb)
    cl = DnClusters(ctx, hdb, d)
    cl.write_uclust(tmp_path / "hn.u")
    cl.write_uclust(tmp_path / "gn.u", ctx=ctx)
    assert filecmp.cmp(tmp_path / "hn.u", tmp_path / "gn.u", shallow=False)
    return (tmp_path / "gn.u").read_bytes()


def test_writers_on_long_amplicons(gpu_ctx, tmp_path, long_fasta, monkeypatch):
    one, two = long_fasta
    whole1 = _writers_d1(gpu_ctx, tmp_path, one)
    tiers = gpu_ctx.nw_batch_tiers()                       # (3 000 amplicons: a single chunk)
    assert whole1.count(b"\nH\t") > 100 and sum(tiers[3:7]) > 100 and tiers[7] == 0, tiers
    whole3 = _writers_dn(gpu_ctx, tmp_path, two, 3)
    tiers = gpu_ctx.nw_batch_tiers()
    assert whole3.count(b"\nH\t") > 100 and sum(tiers[3:7]) > 100 and tiers[7] == 0, tiers
    monkeypatch.setenv("SWA_NW_CHUNK", "97")
    assert _writers_d1(gpu_ctx, tmp_path, one) == whole1
    assert _writers_dn(gpu_ctx, tmp_path, two, 3) == whole3


def _cli(args, fa, tmp_path, tag, env=None):
    u, o = tmp_path / f"{tag}.u", tmp_path / f"{tag}.o"
    r = subprocess.run([str(BIN)] + args + ["-u", str(u), "-o", str(o), "-l", "/dev/null", str(fa)], capture_output=True,
                       text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return u, o, r.stderr


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("d", [1, 3])
def test_cli_long_amplicons_against_reference_binary(tmp_path, long_fasta, d):
    fa = long_fasta[0 if d == 1 else 1]
    args = ["-d", str(d)]
    r = S.run_ref_swarm(args + ["-u", str(tmp_path / "r.u"), "-o", str(tmp_path / "r.o"), "-l", "/dev/null", str(fa)])
    assert r.returncode == 0, r.stderr
    for tag, env in (("g", {"SWARM_AMD_TIMING": "1"}), ("c", {"SWA_NW_CHUNK": "97"}), ("m", {"SWARM_AMD_DEVICES": "0,0"})):
        u, o, err = _cli(args, fa, tmp_path, tag, env)
        assert filecmp.cmp(tmp_path / "r.u", u, shallow=False), tag
        assert filecmp.cmp(tmp_path / "r.o", o, shallow=False), tag
        if tag == "g":                                     # the second [nw] line: eight tiers, none of the pairs on the host
            line = [ln for ln in err.splitlines() if ln.startswith("[nw] pairs by tier")]
            assert len(line) == 1, err
            counts = [int(v) for v in re.search(r"host: ([\d ]+);", line[0]).group(1).split()]
            assert len(counts) == 8 and sum(counts[3:7]) > 100 and counts[7] == 0, line
