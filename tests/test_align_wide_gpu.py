"""k_align_wide<K, with lengths or not> (align.hip): the banded alignment kernel for bands wider than a wave, K = 2, 4, 8
band offsets a lane, chosen while the environment has SWA_ALIGN_WIDE=1.  Its yardsticks are k_align_generic — the same
launches with the switch unset, equal in all three arrays on EVERY pair — and the oracle's orc_nw_diff under the parity
rule of tests/test_align_forms_gpu.py (whose helpers are used here).  Which form runs is asked of the library."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import support as S
import test_align_forms_gpu as F
from align_wide_model import band_of, end_cell
from swarm_amd import reduced_penalties

pytestmark = pytest.mark.gpu

DEFAULT, UNIT = (18, 24, 13), (1, 0, 1)
SWITCH = "SWA_ALIGN_WIDE"


def _both(ctx, monkeypatch, q, targets, lengths=True):
    """search_do with the switch and without it: (wide, generic)"""
    monkeypatch.setenv(SWITCH, "1")
    assert ctx.search_form(lengths)[0].startswith("wide")
    wide = ctx.search_do(q, targets, lengths)
    monkeypatch.delenv(SWITCH)
    assert ctx.search_form(lengths)[0] == "generic"
    return wide, ctx.search_do(q, targets, lengths)


def _same(a, b, what=None):
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x, y), what


# ---- forms -----------------------------------------------------------------------------------------------------------

FORMS = [(DEFAULT, 11, "wide2", 65535), (DEFAULT, 21, "wide2", 65535), (DEFAULT, 22, "wide4", 65535),
         (DEFAULT, 44, "wide4", 65535), (DEFAULT, 45, "wide8", 65535), (DEFAULT, 89, "wide8", 65535),
         (DEFAULT, 90, "generic", 65535), ((4, 2, 1), 8, "wide2", 255), ((4, 0, 3), 255, "generic", 65535)]


def test_forms_follow_the_switch(gpu_ctx, monkeypatch):
    db = F._upload(gpu_ctx, F._families(np.random.default_rng(1), 2, [40, 150]))
    lds = 8 * ((db.longest + 31) // 32 + 1) * 2 * 4          # two sequences a pair, four pairs a workgroup
    for scoring, d, form, sat in FORMS:
        gpu_ctx.search_begin(*scoring, d)
        monkeypatch.delenv(SWITCH, raising=False)
        for value in (None, "0"):                            # unset, or switched off: the plan of before
            if value is not None:
                monkeypatch.setenv(SWITCH, value)
            assert gpu_ctx.search_form(True) == ("generic", sat, 0) == gpu_ctx.search_form(False), (scoring, d)
        monkeypatch.setenv(SWITCH, "1")
        with_len, without = gpu_ctx.search_form(True), gpu_ctx.search_form(False)
        if form == "generic":
            assert with_len == without == ("generic", sat, 0), (scoring, d)
        else:                                                # the lengths pick the template, nothing else
            assert with_len == (form + "_len", sat, lds) and without == (form, sat, lds), (scoring, d)
    # the forms of narrower bands do not look at the switch
    for scoring, d, cell in F.REPRESENTATIVES:
        if not cell.startswith("generic"):
            gpu_ctx.search_begin(*scoring, d)
            assert F._cell(gpu_ctx, True) == cell and F._cell(gpu_ctx, False) == cell


# ---- parity on short families ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scoring,d,form", [(UNIT, 31, "wide2"), (UNIT, 62, "wide4"), (UNIT, 126, "wide8"),
                                            ((4, 2, 1), 8, "wide2"), (DEFAULT, 11, "wide2"), (DEFAULT, 22, "wide4"),
                                            (DEFAULT, 45, "wide8")],
                         ids=lambda v: str(v))
def test_parity_on_short_families(gpu_ctx, monkeypatch, scoring, d, form):
    rng = np.random.default_rng(d * 100 + scoring[0])
    db = F._upload(gpu_ctx, F._families(rng, d, F.SHORT_LENGTHS))
    gpu_ctx.search_begin(*scoring, d)
    monkeypatch.setenv(SWITCH, "1")
    got_form, sat, _ = gpu_ctx.search_form(False)
    assert got_form == form and sat == (255 if scoring != DEFAULT else 65535)
    by_len = {}
    for i in range(db.n):
        by_len.setdefault(int(db.seqlen[i]), []).append(i)
    queries = [by_len[L][0] for L in F.SHORT_LENGTHS if L in by_len]
    assert len(queries) == len(F.SHORT_LENGTHS)
    targets = np.arange(db.n, dtype=np.uint64)
    accepted = 0
    for q in queries:
        rows = [F._oracle(db, q, int(t), *scoring) for t in targets]
        for lengths in (True, False):
            wide, generic = _both(gpu_ctx, monkeypatch, q, targets, lengths)
            _same(wide, generic, (q, lengths))
            n = F._check(db, q, targets, scoring, d, sat, wide, rows)
            accepted += n if lengths else 0
    assert accepted >= len(queries)                          # (each query at least finds itself)


# ---- band and lane edges -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [31, 32, 62, 63, 126, 127])
def test_band_and_lane_edges(gpu_ctx, monkeypatch, d):
    """(1, 0, 1): W = d + 1 of either parity.  Pairs whose length difference puts the end cell on every j of a lane,
    on the first and the last in-band index and one past it (infeasible: SAT), in both directions, among them a 1-nt
    sequence against one of 1 + W nt."""
    W, sat = band_of(*UNIT, d)
    K = {31: 2, 32: 2, 62: 4, 63: 4, 126: 8, 127: 8}[d]
    rng = np.random.default_rng(d)
    deltas = sorted({0, *range(1, 2 * K + 1), W - K - 1, *range(W - K, W + 2)})
    seqs, groups = [], []
    for L in (1, 37):
        base = F._centroid(rng, L, L == 37 and d % 2 == 0)
        group = [base]
        for delta in deltas:                                 # delta insertions
            s = list(base)
            for _ in range(delta):
                s.insert(int(rng.integers(0, len(s) + 1)), "ACGT"[int(rng.integers(0, 4))])
            group.append("".join(s))
        groups.append(group)
        seqs += group
    seqs = list(dict.fromkeys(seqs))
    db = F._upload(gpu_ctx, seqs)
    at = {db.seq_str(i): i for i in range(db.n)}
    gpu_ctx.search_begin(*UNIT, d)
    seen = set()
    for group in groups:
        ids = np.array([at[s] for s in group], dtype=np.uint64)
        for q in (int(ids[0]), int(ids[-1]), int(ids[-2]), int(ids[len(ids) // 2])):
            rows = [F._oracle(db, q, int(t), *UNIT) for t in ids]
            wide, generic = _both(gpu_ctx, monkeypatch, q, ids)
            wide_nolen, generic_nolen = _both(gpu_ctx, monkeypatch, q, ids, False)
            _same(wide, generic, q)
            _same(wide_nolen, generic_nolen, q)
            F._check(db, q, ids, UNIT, d, sat, wide, rows)
            F._check(db, q, ids, UNIT, d, sat, wide_nolen, rows)
            for k, t in enumerate(ids):
                dl, ql = int(db.seqlen[int(t)]), int(db.seqlen[q])
                if abs(ql - dl) <= W:
                    seen.add(("j", end_cell(dl, ql, W, K)[1]))
                    seen.add(("x", ql - dl + W + 1))
                else:
                    seen.add("past")
                    assert (int(wide[1][k]), int(wide[0][k]), int(wide[2][k])) == (sat, sat, 0)
                if {dl, ql} == {1, 1 + W}:
                    seen.add("one")
    assert {("j", j) for j in range(K)} <= seen and {("x", 1), ("x", 2 * W + 1), "past", "one"} <= seen


# ---- many pairs --------------------------------------------------------------------------------------------------------

def test_many_pairs(gpu_ctx, monkeypatch):
    """One query against 10 000 targets: past the 8 x CUs x 4 pairs of one grid stride; batches of 1 000 give the same."""
    scoring, d = DEFAULT, 11
    rng = np.random.default_rng(78)
    seqs = set()
    while len(seqs) < 10000:
        cent = F._centroid(rng, int(rng.integers(40, 91)), False)
        seqs.add(cent)
        for _ in range(40):
            seqs.add(F._mutate(rng, cent, int(rng.integers(0, d + 4)), "ACGT"))
    db = F._upload(gpu_ctx, sorted(seqs))
    gpu_ctx.search_begin(*scoring, d)
    q = int(rng.integers(0, db.n))
    targets = rng.permutation(db.n).astype(np.uint64)
    for lengths in (True, False):
        whole, generic = _both(gpu_ctx, monkeypatch, q, targets, lengths)
        _same(whole, generic, lengths)
        monkeypatch.setenv(SWITCH, "1")
        parts = [gpu_ctx.search_do(q, targets[i:i + 1000], lengths) for i in range(0, len(targets), 1000)]
        for k in range(3):
            if whole[k] is not None:
                assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k])
    sample = np.unique(np.concatenate([np.flatnonzero(whole[1] <= d), rng.integers(0, len(targets), size=500)]))
    monkeypatch.setenv(SWITCH, "1")
    got = gpu_ctx.search_do(q, targets[sample])
    assert F._check(db, q, targets[sample], scoring, d, 65535, got) >= 1


# ---- the staging boundary ----------------------------------------------------------------------------------------------

def test_staging_boundary(gpu_ctx, monkeypatch):
    """The longest-sequence length at which the wide form's staging stops fitting the LDS, asked of search_form.  Just
    below it a pair aligns in wide2 (more than 64 KB of dynamic LDS); at it the form is generic.  The oracle's direction
    matrix of such a pair would take gigabytes, so, as test_long_sequences does, the long pairs are copies with k
    substitutions far apart — diff = k, length = L, score = k * mismatch, the construction checked against the oracle
    at 2 000 nt — and the generic kernel's answers."""
    scoring, d = DEFAULT, 11
    mm = scoring[0]
    monkeypatch.setenv(SWITCH, "1")

    def form(L):
        F._upload(gpu_ctx, ["A" * L])
        gpu_ctx.search_begin(*scoring, d)
        return gpu_ctx.search_form(False)
    lo, hi = 1, 1 << 20
    assert form(lo)[0] == "wide2" and form(hi)[0] == "generic"
    while hi - lo > 1:                                       # first length that is generic
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if form(mid)[0] == "wide2" else (lo, mid)
    assert form(lo)[2] > 65536 and form(lo)[2] == 64 * ((lo + 31) // 32 + 1)
    rng = np.random.default_rng(5)
    for L in (2000, lo, hi):
        base = F._centroid(rng, L, False)
        longs = [base] + [F._substituted(rng, base, k) for k in (1, d, d + 1)]
        db = F._upload(gpu_ctx, longs)
        gpu_ctx.search_begin(*scoring, d)
        at = {db.seq_str(i): i for i in range(db.n)}
        ids = [at[s] for s in longs]
        targets = np.array(ids[1:], dtype=np.uint64)
        monkeypatch.setenv(SWITCH, "1")
        assert gpu_ctx.search_form(True)[0] == ("generic" if L == hi else "wide2_len")
        got = gpu_ctx.search_do(ids[0], targets)
        got_nolen = gpu_ctx.search_do(ids[0], targets, lengths=False)
        monkeypatch.delenv(SWITCH)
        _same(got, gpu_ctx.search_do(ids[0], targets), L)
        assert np.array_equal(got_nolen[1], got[1])
        for k, kk in enumerate((1, d, d + 1)):
            if kk <= d:
                assert (int(got[1][k]), int(got[2][k]), int(got[0][k])) == (kk, L, kk * mm), (L, kk)
            else:
                assert int(got[1][k]) > d
            if L == 2000:
                assert F._oracle(db, ids[0], ids[k + 1], *scoring) == (kk, L, kk * mm)


# ---- the routes --------------------------------------------------------------------------------------------------------

def _write(cl, where, ctx=None):
    where.mkdir()
    cl.write_swarms(where / "o")
    cl.write_structure(where / "i")
    cl.write_stats(where / "s")


@pytest.mark.parametrize("route", ["scan", "graph", "multi-scan"])
def test_routes_write_the_same_with_the_switch(gpu_ctx, tmp_path, monkeypatch, route):
    from swarm_amd import DnClusters, HostDb, MultiContext
    monkeypatch.delenv("SWARM_AMD_DN_WALK", raising=False)
    monkeypatch.setenv("SWARM_AMD_DN", route.split("-")[-1])
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 1200, 150, 1212, 12)
    hdb = HostDb(fa, check_duplicate_sequences=True)
    totals = {}
    for switch in ("off", "on"):
        if switch == "on":
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        if route == "multi-scan":
            m = MultiContext([0, 0])
            try:
                m.upload_hostdb(hdb)
                cl = m.dn_cluster(hdb, 12)
                assert cl.route() == ("scan", 2)
                totals[switch] = cl.scan_totals()
                _write(cl, tmp_path / switch)
                cl.close()
            finally:
                m.close()
        else:
            gpu_ctx.upload_hostdb(hdb)
            cl = DnClusters(gpu_ctx, hdb, 12)
            try:
                assert gpu_ctx.search_form(False)[0] == ("wide2" if switch == "on" else "generic")
                totals[switch] = cl.scan_totals()
                assert totals[switch]["route"] == route
                _write(cl, tmp_path / switch)
            finally:
                cl.close()
    assert totals["on"]["aligned_pairs"] == totals["off"]["aligned_pairs"] > 0
    for k in "ois":
        assert filecmp.cmp(tmp_path / "on" / k, tmp_path / "off" / k, shallow=False), k
    assert (tmp_path / "on" / "i").read_text().count("\n") > 100


def test_command_line_writes_the_same_with_the_switch(tmp_path):
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 1200, 150, 1213, 12)
    env = {k: v for k, v in os.environ.items() if k not in (SWITCH, "SWARM_AMD_DN", "SWARM_AMD_DN_WALK")}
    for tag, extra in (("off", {}), ("on", {SWITCH: "1"})):
        outs = []
        for k in "ois":
            outs += ["-" + k, str(tmp_path / f"{tag}.{k}")]
        r = subprocess.run([str(S.ROOT / "swarm_amd" / "bin" / "swarm"), "-d", "12"] + outs + ["-l", "/dev/null", str(fa)],
                           capture_output=True, text=True, env=dict(env, **extra))
        assert r.returncode == 0, (tag, r.stderr)
    for k in "ois":
        assert filecmp.cmp(tmp_path / f"on.{k}", tmp_path / f"off.{k}", shallow=False), k


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("route", ["auto", "scan"])
def test_wide2_8bit_against_reference_binary(gpu_ctx, tmp_path, monkeypatch, route):
    """-m 1 -p 1 -g 1 -e 0 -d 8: (4, 2, 1), W = 33, 8-bit — the set of test_align_forms_gpu's d8_generic_graph."""
    from swarm_amd import DnClusters, HostDb
    opts, d = ["-m", "1", "-p", "1", "-g", "1", "-e", "0"], 8
    assert reduced_penalties(1, 1, 1, 0) == (4, 2, 1)
    if route == "scan":
        monkeypatch.setenv("SWARM_AMD_DN", "scan")
    else:
        monkeypatch.delenv("SWARM_AMD_DN", raising=False)
    monkeypatch.delenv("SWARM_AMD_DN_WALK", raising=False)
    monkeypatch.setenv(SWITCH, "1")
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 1200, 160, 4000 + d, 8)
    F._ref_outputs(tmp_path, fa, d, opts)
    hdb = HostDb(fa, check_duplicate_sequences=True)
    gpu_ctx.upload_hostdb(hdb)
    cl = DnClusters(gpu_ctx, hdb, d, penalties=(4, 2, 1))
    try:
        assert gpu_ctx.search_form(False) == ("wide2", 255, 8 * ((hdb.longest + 31) // 32 + 1) * 8)
        assert cl.scan_totals()["route"] == ("scan" if route == "scan" else "graph")
        cl.write_swarms(tmp_path / "o")
        cl.write_structure(tmp_path / "i")
        cl.write_stats(tmp_path / "s")
        cl.write_uclust(tmp_path / "u", ctx=gpu_ctx)
    finally:
        cl.close()
    for suffix in "oisu":
        assert filecmp.cmp(tmp_path / suffix, tmp_path / ("r" + suffix), shallow=False), suffix
