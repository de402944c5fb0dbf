"""Every form of the d >= 2 alignment launch (swa_align_launch, align.hip) against the oracle's orc_nw_diff: which form
runs is asked of the library (swa_search_form), never restated here.  The forms: k_align_wfa<16> / <32> (wavefront),
k_align<32 | 64, with lengths or not> (banded), k_align_generic (any band, any length), each in the reference's 8- or
16-bit saturation.  Parity rule of every test: where the oracle's diff <= d and its score lies below the saturation
value, (diff, alignment length, score) are bit-identical; everywhere else the kernel's diff is > d."""
import ctypes as C
import filecmp
import subprocess

import numpy as np
import pytest

import support as S
from swarm_amd import reduced_penalties

pytestmark = pytest.mark.gpu

# (scoring, d) -> the cell (form without the lengths flag, saturation bits) it reaches on a short database
REPRESENTATIVES = [((4, 0, 3), 2, "wfa16-8"), ((8, 0, 9), 7, "wfa32-8"), ((4, 0, 3), 3, "banded32-8"),
                   ((12, 10, 19), 9, "banded32-16"), ((4, 0, 3), 11, "banded64-8"), ((4, 2, 15), 16, "banded64-16"),
                   ((4, 2, 1), 8, "generic-8"), ((18, 24, 13), 11, "generic-16"), ((4, 0, 3), 255, "generic-16")]
CELLS = {c for _, _, c in REPRESENTATIVES}
# edge systems: T = d * max(mm, go + ge) exactly 255 in 8-bit mode; room for one gap opening in 16-bit mode; a mismatch
# penalty of 255 (-m 2 -p 253 -g 1 -e 1), whose single mismatch saturates the 8-bit score at d = 1
EDGES = [((4, 14, 3), 15), ((18, 60000, 13), 2), ((255, 1, 2), 1), ((255, 1, 2), 2)]


def _cell(ctx, with_lengths=True) -> str:
    form, sat, _ = ctx.search_form(with_lengths)
    return f"{form.replace('_len', '')}-{8 if sat == 255 else 16}"


def _upload(ctx, seqs):
    db = S.build_db([(f"s{i}_1".encode(), s.encode()) for i, s in enumerate(seqs)])
    ctx.upload_db(db.seqs, db.seq_off, db.seqlen, db.abundance, db.longest)
    return db


def _oracle(db, q, t, mm, go, ge):
    alen, score = C.c_uint64(0), C.c_uint64(0)
    d = S.oracle().orc_nw_diff(S._p(db.words(t), S.u64p), int(db.seqlen[t]), S._p(db.words(q), S.u64p),
                               int(db.seqlen[q]), mm, go, ge, C.byref(alen), C.byref(score))
    return int(d), int(alen.value), int(score.value)


def _check(db, q, targets, scoring, d, sat, got, oracle_rows=None) -> int:
    """Parity of one search_do result with the oracle; returns the pairs accepted (diff <= d)."""
    scores, diffs, alens = got
    accepted = 0
    for k, t in enumerate(targets):
        od, ol, osc = oracle_rows[k] if oracle_rows is not None else _oracle(db, q, int(t), *scoring)
        if od <= d and osc < sat:
            accepted += 1
            assert int(diffs[k]) == od, (q, int(t), scoring, d, od, int(diffs[k]))
            if scores is not None:
                assert (int(scores[k]), int(alens[k])) == (osc, ol), (q, int(t), scoring, d)
        else:
            assert int(diffs[k]) > d, (q, int(t), scoring, d, od, osc, int(diffs[k]))
    return accepted


def _mutate(rng, s, edits, alphabet):
    s = list(s)
    for _ in range(edits):
        p = int(rng.integers(0, len(s) + 1))
        u = rng.random()
        b = alphabet[int(rng.integers(0, len(alphabet)))]
        if u < 0.5 and p < len(s):
            s[p] = b
        elif u < 0.75 and p < len(s) and len(s) > 1:
            del s[p]
        else:
            s.insert(p, b)
    return "".join(s)


def _centroid(rng, length, two_letter):
    if not two_letter:
        return "".join(rng.choice(list("ACGT"), size=length))
    out = []
    while len(out) < length:                                 # two letters in long runs: many equally good alignments
        out += [str(rng.choice(list("AC")))] * int(rng.integers(1, 9))
    return "".join(out[:length])


def _families(rng, d, lengths, members=6):
    """Families over ACGT and over two letters with long runs; members 0 .. d + 3 edits from their centroid."""
    seqs = set()
    for L in lengths:
        for two in (False, True):
            cent = _centroid(rng, L, two)
            seqs.add(cent)
            for _ in range(members):
                seqs.add(_mutate(rng, cent, int(rng.integers(0, d + 4)), "AC" if two else "ACGT"))
    return sorted(seqs, key=lambda s: (len(s), s))


SHORT_LENGTHS = [1, 2, 3, 5, 8, 31, 32, 33, 63, 64, 65, 150, 297]


def test_sweep_reaches_every_cell(gpu_ctx):
    """All legal command-line scorings (-m / -p 1..7, -g / -e 0..7, g + e >= 1, reduced as the reference does) at every d
    from 2 up to the reference's 16-bit limit (at most 255): the forms they select cover every cell, and the
    representatives above select theirs."""
    _upload(gpu_ctx, _families(np.random.default_rng(1), 2, [40, 150]))
    scorings = sorted({reduced_penalties(m, p, g, e) for m in range(1, 8) for p in range(1, 8) for g in range(8)
                       for e in range(8) if g + e >= 1})
    seen = set()
    for mm, go, ge in scorings:
        limit = min(255, 65535 // mm, (65535 - go) // ge)
        for d in range(2, limit + 1):
            gpu_ctx.search_begin(mm, go, ge, d)
            cell = _cell(gpu_ctx)
            seen.add(cell)
            if cell == "generic-16":                         # the band and the saturation only grow with d
                break
    assert CELLS <= seen, CELLS - seen
    for scoring, d, cell in REPRESENTATIVES:
        gpu_ctx.search_begin(*scoring, d)
        assert _cell(gpu_ctx, True) == cell and _cell(gpu_ctx, False) == cell, (scoring, d)
        form, _, _ = gpu_ctx.search_form(True)
        if form.startswith("banded"):                        # the lengths pick the template, nothing else
            assert form.endswith("_len") and not gpu_ctx.search_form(False)[0].endswith("_len")


@pytest.mark.parametrize("scoring,d", [(s, d) for s, d, _ in REPRESENTATIVES] + EDGES,
                         ids=[f"{c}-{s}-d{d}" for s, d, c in REPRESENTATIVES] + [f"edge-{s}-d{d}" for s, d in EDGES])
def test_form_parity_with_oracle(gpu_ctx, scoring, d):
    rng = np.random.default_rng(hash((scoring, d)) % (1 << 32))
    seqs = _families(rng, d, SHORT_LENGTHS + [int(x) for x in rng.integers(100, 301, size=3)])
    db = _upload(gpu_ctx, seqs)
    gpu_ctx.search_begin(*scoring, d)
    _, sat, _ = gpu_ctx.search_form()
    # queries from every length class
    by_len = {}
    for i in range(db.n):
        by_len.setdefault(int(db.seqlen[i]), []).append(i)
    queries = [by_len[L][0] for L in sorted(by_len) if L in (1, 5, 32, 33, 64, 65) or L > 150][:9]
    targets = np.arange(db.n, dtype=np.uint64)
    accepted = 0
    for q in queries:
        rows = [_oracle(db, q, int(t), *scoring) for t in targets]
        accepted += _check(db, q, targets, scoring, d, sat, gpu_ctx.search_do(q, targets), rows)
        _check(db, q, targets, scoring, d, sat, gpu_ctx.search_do(q, targets, lengths=False), rows)
    assert accepted >= len(queries)                          # (each query at least finds itself)


@pytest.mark.parametrize("scoring,d,cell", [((18, 24, 13), 11, "generic-16"), ((4, 2, 15), 16, "banded64-16")])
def test_many_targets(gpu_ctx, scoring, d, cell):
    """One query against 70 000+ targets: past the generic kernel's 65 536-thread grid stride and the banded kernels'
    block cap; the same targets in batches of 1 000 give the same answers, and a sample matches the oracle."""
    rng = np.random.default_rng(77)
    seqs = set()
    while len(seqs) < 70500:
        cent = _centroid(rng, int(rng.integers(40, 90)), False)
        seqs.add(cent)
        for _ in range(40):
            seqs.add(_mutate(rng, cent, int(rng.integers(0, d + 4)), "ACGT"))
    seqs = sorted(seqs)
    db = _upload(gpu_ctx, seqs)
    gpu_ctx.search_begin(*scoring, d)
    assert _cell(gpu_ctx) == cell
    _, sat, _ = gpu_ctx.search_form()
    q = int(rng.integers(0, db.n))
    targets = rng.permutation(db.n).astype(np.uint64)
    whole = gpu_ctx.search_do(q, targets)
    for lengths in (True, False):
        parts = [gpu_ctx.search_do(q, targets[i:i + 1000], lengths) for i in range(0, len(targets), 1000)]
        assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
        if lengths:
            assert np.array_equal(np.concatenate([p[0] for p in parts]), whole[0])
            assert np.array_equal(np.concatenate([p[2] for p in parts]), whole[2])
    sample = np.concatenate([np.flatnonzero(whole[1] <= d), rng.integers(0, len(targets), size=1500)])
    sample = np.unique(sample)
    got = tuple(x[sample] for x in whole)
    assert _check(db, q, targets[sample], scoring, d, sat, got) >= 1


def _substituted(rng, s, k, alphabet="ACGT"):
    """s with k substitutions at least len(s) // (k + 1) - 1 apart"""
    s = list(s)
    L = len(s)
    for j in range(k):
        p = (j + 1) * L // (k + 1)
        s[p] = alphabet[(alphabet.index(s[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return "".join(s)


def _long_boundaries(ctx, scoring, d):
    """The longest-sequence lengths where the launch's form or LDS opt-in changes, found by asking swa_search_form on
    one-sequence databases: the last length of each (form, staging <= 64 KB) class and the first of the next."""
    def key(L):
        _upload(ctx, ["A" * L])
        ctx.search_begin(*scoring, d)
        form, _, lds = ctx.search_form(False)
        return form, lds <= 65536
    out, L, k0 = [], 1, key(1)
    while L < 70000:
        hi = min(L * 2, 70000)
        if key(hi) == k0:
            L = hi
            continue
        lo = L
        while hi - lo > 1:                                   # first length with another key
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if key(mid) == k0 else (lo, mid)
        out += [lo, hi]
        L, k0 = hi, key(hi)
    return out


@pytest.mark.parametrize("d", [2, 4, 5, 11])
def test_long_sequences(gpu_ctx, d):
    """Databases of short families plus one long sequence and copies of it, the long one just below and just above each
    length where the launch changes form or needs more than 64 KB of LDS, at 64 999 / 65 000 (the wavefront kernels'
    cutoff) and at 70 000 nt.  Default scoring: d = 2 wfa16, d = 4 wfa32, d = 5 banded64, d = 11 generic on short
    databases.  The short pairs against the oracle (the longest sequence sizes every launch's staging); the long
    sequence against copies carrying k substitutions far apart: diff = k, length = L, score = k * mismatch (the only
    optimum while mismatch < 2 (gapopen + gapextend)), checked against the oracle itself at 2 000 and 12 000 nt."""
    scoring = (18, 24, 13)
    mm, go, ge = scoring
    assert mm < 2 * (go + ge)
    rng = np.random.default_rng(500 + d)
    bounds = _long_boundaries(gpu_ctx, scoring, d)
    lengths = sorted({2000, 12000, 64999, 65000, 70000, *[b for b in bounds if b > 12000]})
    short = _families(rng, d, [5, 33, 64, 150, 290], members=4)
    forms = set()
    for L in lengths:
        base = _centroid(rng, L, False)
        longs = [base] + [_substituted(rng, base, k) for k in (1, d, d + 1)]
        seqs = short + longs
        db = _upload(gpu_ctx, seqs)
        gpu_ctx.search_begin(*scoring, d)
        form, sat, lds = gpu_ctx.search_form()
        forms.add((form, lds > 65536))
        long_ids = [i for i in range(db.n) if int(db.seqlen[i]) == L]
        strs = {i: db.seq_str(i) for i in long_ids}              # (the database's order is not the list's)
        ids = [next(i for i in long_ids if strs[i] == s) for s in longs]
        # short pairs
        short_ids = np.array([i for i in range(db.n) if i not in long_ids], dtype=np.uint64)
        for q in rng.choice(short_ids, size=4, replace=False):
            for lengths_flag in (True, False):
                _check(db, int(q), short_ids, scoring, d, sat, gpu_ctx.search_do(int(q), short_ids, lengths_flag))
        # long pairs
        targets = np.array(ids[1:], dtype=np.uint64)
        scores, diffs, alens = gpu_ctx.search_do(ids[0], targets)
        _, diffs2, _ = gpu_ctx.search_do(ids[0], targets, lengths=False)
        for k, kk in enumerate((1, d, d + 1)):
            if kk <= d:
                assert (int(diffs[k]), int(alens[k]), int(scores[k])) == (kk, L, kk * mm), (L, d, kk, form)
                assert int(diffs2[k]) == kk, (L, d, kk, form)
            else:
                assert int(diffs[k]) > d and int(diffs2[k]) > d, (L, d, form)
            if L <= 12000:
                od, ol, osc = _oracle(db, ids[0], ids[k + 1], *scoring)
                assert (od, ol, osc) == (kk, L, kk * mm)
    assert len(forms) >= 2 or d == 11, forms


# ---- end to end against the compiled reference binary ----------------------------------------------------------------

def _isolated_indel_families(path, seed, families=40, length=420, d=15):
    """Members carry up to d + 1 single-nucleotide indels at least 24 nt apart: each costs gapopen + gapextend, so at
    -m 1 -p 1 -g 7 -e 1 (4, 14, 3) fifteen of them cost exactly 255, the 8-bit saturation value of d = 15."""
    rng = np.random.default_rng(seed)
    recs, seen = [], set()
    for f in range(families):
        cent = _centroid(rng, length, False)
        for m, k in enumerate([0, 1, 3, 14, 15, 15, 16, 2, 15]):
            slots = np.sort(rng.choice(np.arange(1, length // 24), size=k, replace=False)) * 24 if k else []
            s = list(cent)
            for p in slots[::-1]:
                if rng.random() < 0.5:
                    del s[p]
                else:
                    s.insert(p, "ACGT"[("ACGT".index(s[p]) + 2) % 4])   # (unlike the base it lands before)
            s = "".join(s)
            if s not in seen:
                seen.add(s)
                recs.append((f"f{f}m{m}_{int(rng.integers(1, 4)) if m else 5}", s))
    path.write_text("".join(f">{h}\n{s}\n" for h, s in recs))


def _long_family_set(path, seed):
    """A few hundred short amplicons and two families of ~18 000 nt (more than 64 KB of staging at d = 2)."""
    S.gen_fasta(path, 300, 150, seed, 2)
    rng = np.random.default_rng(seed)
    extra = []
    for f in range(2):
        cent = _centroid(rng, 18000 + 37 * f, False)
        extra.append((f"long{f}c_9", cent))
        for m in range(2):
            extra.append((f"long{f}m{m}_{m + 1}", _mutate(rng, cent, m + 1, "ACGT")))
    with open(path, "a") as fh:
        fh.write("".join(f">{h}\n{s}\n" for h, s in extra))


# Two known divergences, kept as strict xfails until the kernels follow them: the reference clusters these sets
# differently from both this library and its own nw().  At -g 30000 its 16-bit search starts each target with
# 2 (gapopen + gapextend) truncated to 16 bits (search16.cc, where a channel takes a new sequence), so a leading gap
# costs next to nothing.  At the default scoring in 16-bit mode it reports more differences than nw() for some pairs
# (a 152 / 153-nt pair of the d11 set: nw() 10, the search 15); the cause is not found yet.
_DIVERGES = pytest.mark.xfail(strict=True, reason="the reference's 16-bit search departs from its own nw() here")
E2E = [  # (id, CLI scoring options, d, input)
    pytest.param("d11_default", [], 11, ("gen", 1200, 150, 11), marks=_DIVERGES, id="d11_default"),
    pytest.param("d2_gapopen60000", ["-m", "5", "-p", "4", "-g", "30000", "-e", "4"], 2, ("gen", 1500, 150, 2),
                 marks=_DIVERGES, id="d2_gapopen60000"),
    ("d9_banded32_16", ["-m", "5", "-p", "1", "-g", "5", "-e", "7"], 9, ("gen", 1200, 150, 9)),
    ("d3_gapopen0", ["-m", "1", "-p", "1", "-g", "0", "-e", "1"], 3, ("gen", 1500, 100, 3)),
    ("d8_generic_graph", ["-m", "1", "-p", "1", "-g", "1", "-e", "0"], 8, ("gen", 1200, 160, 8)),
    ("d15_cost255", ["-m", "1", "-p", "1", "-g", "7", "-e", "1"], 15, ("indels",)),
    ("d2_long_families", [], 2, ("long",)),
]


def _e2e_input(path, spec, seed):
    if spec[0] == "gen":
        S.gen_fasta(path, spec[1], spec[2], seed, spec[3])
    elif spec[0] == "indels":
        _isolated_indel_families(path, seed)
    else:
        _long_family_set(path, seed)


def _ref_outputs(tmp_path, fa, d, opts):
    r = S.run_ref_swarm(["-d", d] + opts + ["-o", tmp_path / "ro", "-i", tmp_path / "ri", "-s", tmp_path / "rs",
                                            "-u", tmp_path / "ru", "-l", "/dev/null", fa])
    assert r.returncode == 0, r.stderr


def _penalties(opts):
    v = {"-m": 5, "-p": 4, "-g": 12, "-e": 4}
    for k in range(0, len(opts), 2):
        v[opts[k]] = int(opts[k + 1])
    return reduced_penalties(v["-m"], v["-p"], v["-g"], v["-e"])


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("route", ["auto", "scan"])
@pytest.mark.parametrize("name,opts,d,spec", E2E, ids=[c.id if hasattr(c, "id") else c[0] for c in E2E])
def test_scorings_against_reference_binary(gpu_ctx, tmp_path, monkeypatch, name, opts, d, spec, route):
    from swarm_amd import DnClusters, HostDb
    if route == "scan":
        monkeypatch.setenv("SWARM_AMD_DN", "scan")
    else:
        monkeypatch.delenv("SWARM_AMD_DN", raising=False)
    monkeypatch.delenv("SWARM_AMD_DN_WALK", raising=False)
    fa = tmp_path / "in.fa"
    _e2e_input(fa, spec, 4000 + d)
    _ref_outputs(tmp_path, fa, d, opts)
    hdb = HostDb(fa, check_duplicate_sequences=True)
    gpu_ctx.upload_hostdb(hdb)
    cl = DnClusters(gpu_ctx, hdb, d, penalties=_penalties(opts))
    if route == "scan":
        assert cl.scan_totals()["route"] == "scan"
    elif name in ("d3_gapopen0", "d8_generic_graph"):
        assert cl.scan_totals()["route"] == "graph"
    cl.write_swarms(tmp_path / "o")
    cl.write_structure(tmp_path / "i")
    cl.write_stats(tmp_path / "s")
    cl.write_uclust(tmp_path / "u", ctx=gpu_ctx)
    for suffix in "oisu":
        assert filecmp.cmp(tmp_path / suffix, tmp_path / ("r" + suffix), shallow=False), suffix
    if name == "d15_cost255":                                # pairs at exactly the saturation value were met
        gpu_ctx.search_begin(*_penalties(opts), d)
        assert _cell(gpu_ctx, False) == "generic-8"
        db = S.db_from_fasta(fa)
        at = {h.split(b"_")[0]: i for i, h in enumerate(db.headers)}
        exact = [_oracle(db, at[b"f%dm0" % f], at[b"f%dm%d" % (f, m)], *_penalties(opts))
                 for f in range(6) for m in (4, 5, 8) if b"f%dm%d" % (f, m) in at]
        assert (15, 255) in {(x[0], x[2]) for x in exact}, exact


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
def test_cli_banded32_16bit_against_reference_binary(tmp_path):
    fa = tmp_path / "in.fa"
    _, opts, d, spec = next(c for c in E2E if not hasattr(c, "id") and c[0] == "d9_banded32_16")
    _e2e_input(fa, spec, 4000 + d)
    _ref_outputs(tmp_path, fa, d, opts)
    outs = []
    for k in "oisu":
        outs += ["-" + k, str(tmp_path / k)]
    g = subprocess.run([str(S.ROOT / "swarm_amd" / "bin" / "swarm"), "-d", str(d)] + opts + outs + ["-l", "/dev/null", str(fa)],
                       capture_output=True, text=True)
    assert g.returncode == 0, g.stderr
    for suffix in "oisu":
        assert filecmp.cmp(tmp_path / suffix, tmp_path / ("r" + suffix), shallow=False), suffix


def test_generic_scratch_within_budget_and_unservable_length(gpu_ctx):
    """k_align_generic's scratch grows with the longest sequence: the launch cuts its threads to stay within 2 GiB, and
    a sequence so long that one thread's scratch exceeds that is refused with SWA_E_ARG, never a failed allocation or a
    wrong answer."""
    from swarm_amd import SwaError
    from swarm_amd.capi import SWA_E_ARG
    L = 90_000_000                                           # 6 x 4 B x (L + 1) > 2 GiB
    nw = (L + 31) // 32
    rng = np.random.default_rng(3)
    short = S.pack_seq(b"ACGTACGTAC")
    seqs = np.concatenate([rng.integers(0, 1 << 63, size=nw, dtype=np.uint64), short])
    off = np.array([0, nw, nw + len(short)], dtype=np.uint64)
    gpu_ctx.upload_db(seqs, off, np.array([L, 10], dtype=np.uint32), np.array([2, 1], dtype=np.uint64), L)
    for d in (2, 11):
        gpu_ctx.search_begin(18, 24, 13, d)
        with pytest.raises(SwaError) as e:
            gpu_ctx.search_form()
        assert e.value.code == SWA_E_ARG and "longest sequence" in str(e.value)
        with pytest.raises(SwaError) as e:
            gpu_ctx.search_do(1, np.array([0, 1], dtype=np.uint64))
        assert e.value.code == SWA_E_ARG


@pytest.mark.parametrize("route", ["auto", "scan"])
def test_generic_fallback_in_a_clustering_of_many_pairs(gpu_ctx, tmp_path, monkeypatch, route):
    """The default d = 2 with one sequence past the generic cutoff (its staging fits no LDS form) in a database whose
    launches hold more than 65 536 pairs: every alignment of the clustering runs in k_align_generic with its threads cut
    to the scratch budget, and the swarms are those of the same set without the long sequence, plus it alone."""
    from swarm_amd import DnClusters, HostDb
    monkeypatch.delenv("SWARM_AMD_DN_WALK", raising=False)
    if route == "scan":
        monkeypatch.setenv("SWARM_AMD_DN", "scan")
    else:
        monkeypatch.delenv("SWARM_AMD_DN", raising=False)
    short, both = tmp_path / "short.fa", tmp_path / "both.fa"
    S.gen_fasta(short, 80000, 150, 4242, 2)
    long_seq = _centroid(np.random.default_rng(5), 45000, False)
    both.write_text(short.read_text() + f">zzlong_1\n{long_seq}\n")
    outs = {}
    for name, fa in (("short", short), ("both", both)):
        hdb = HostDb(fa, check_duplicate_sequences=True)
        gpu_ctx.upload_hostdb(hdb)
        cl = DnClusters(gpu_ctx, hdb, 2)
        if name == "both":
            assert gpu_ctx.search_form(False)[0] == "generic"
            assert cl.scan_totals()["aligned_pairs"] > 65536
        cl.write_swarms(tmp_path / name)
        outs[name] = (tmp_path / name).read_text()
    assert outs["both"] == outs["short"] + "zzlong_1\n"
