"""Seam B5 on the GPU: the uclust alignments (swa_nw_batch) equal the host aligner pair by pair — differences,
alignment length and CIGAR — in every band tier and in the host fallback, and the -u writers that use them print
the same bytes as the host writers and as the compiled reference."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import support as S
from test_nw_host import fuzz_pairs

pytestmark = pytest.mark.gpu
G = S.GOLDEN
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
BOUND = [24 + 7 * 13, 24 + 15 * 13, 24 + 31 * 13]      # certificate of each tier at 18/24/13: cost < go + (W + 1) ge


def _write_db(path, seqs):
    """every sequence once, abundances descending: db order = list order"""
    with open(path, "w") as fh:
        for i, s in enumerate(seqs):
            fh.write(f">s{i:06d}_{len(seqs) - i}\n{s}\n")


def _mutate(rng, seq, subs):
    """`subs` substitutions far apart (cost exactly subs * mismatch at 18/24/13)"""
    s = list(seq)
    for p in np.linspace(3, len(s) - 4, subs).astype(int):
        s[p] = {"A": "C", "C": "G", "G": "T", "T": "A"}[s[p]]
    return "".join(s)


def _pairs_db(tmp_path, rng):
    seqs, pairs = [], []

    def add(d, q):
        seqs.extend([d, q])
        pairs.append((len(seqs) - 2, len(seqs) - 1))

    for d, q in fuzz_pairs(rng, 2400, max_len=1000):
        add(d, q)
    for k in range(240):                                   # just inside / just outside each tier's certificate
        seed = "".join(rng.choice(list("ACGT"), int(rng.integers(300, 400))))
        for bound in BOUND:
            subs = bound // 18 + k % 2                     # inside: 18 * subs < bound; outside: >= bound
            add(_mutate(rng, seed, subs), seed)
    for k in range(40):                                    # longer than 672 nt, and too long for a lane's LDS column
        seed = "".join(rng.choice(list("ACGT"), 700 + 13 * k if k < 30 else 1100 + k))
        add(_mutate(rng, seed, 3), seed)
    # identical pairs: the same amplicon on both sides
    pairs += [(i, i) for i in range(0, 200, 7)]
    fa = tmp_path / "pairs.fa"
    _write_db(fa, seqs)
    return fa, seqs, pairs


def _host(seqs, d, q, scoring):
    from swarm_amd import nw_align_host
    return nw_align_host(S.pack_seq(seqs[d].encode()), len(seqs[d]), S.pack_seq(seqs[q].encode()), len(seqs[q]), *scoring)


@pytest.mark.parametrize("scoring", [(18, 24, 13), (4, 12, 1), (2, 3, 1), (10, 1, 10)])
def test_nw_batch_equals_the_host_aligner(gpu_ctx, tmp_path, scoring):
    from swarm_amd import HostDb
    rng = np.random.default_rng(7 + scoring[0])
    fa, seqs, pairs = _pairs_db(tmp_path, rng)
    hdb = HostDb(fa)
    assert hdb.header(5).startswith(b"s000005")
    gpu_ctx.upload_hostdb(hdb)
    d_ids = np.array([p[0] for p in pairs], dtype=np.uint32)
    q_ids = np.array([p[1] for p in pairs], dtype=np.uint32)
    diffs, cols, cigars = gpu_ctx.nw_batch(d_ids, q_ids, *scoring)
    totals = gpu_ctx.nw_batch_totals()
    assert sum(totals) == len(pairs)
    for k, (d, q) in enumerate(pairs):
        assert (int(diffs[k]), int(cols[k]), cigars[k]) == _host(seqs, d, q, scoring), (k, d, q)
    if scoring == (18, 24, 13):
        assert all(t > 0 for t in totals), totals          # every tier and the host fallback took pairs


def test_nw_batch_overflowing_penalties_go_to_the_host(gpu_ctx, tmp_path):
    from swarm_amd import HostDb
    rng = np.random.default_rng(3)
    fa, seqs, pairs = _pairs_db(tmp_path, rng)
    pairs = pairs[:300]
    hdb = HostDb(fa)
    gpu_ctx.upload_hostdb(hdb)
    scoring = (1 << 33, 1 << 32, 1 << 30)                  # costs beyond 32 bits
    diffs, cols, cigars = gpu_ctx.nw_batch([p[0] for p in pairs], [p[1] for p in pairs], *scoring)
    assert gpu_ctx.nw_batch_totals() == [0, 0, 0, len(pairs)]
    for k, (d, q) in enumerate(pairs):
        assert (int(diffs[k]), int(cols[k]), cigars[k]) == _host(seqs, d, q, scoring)
    diffs, cols, cigars = gpu_ctx.nw_batch([], [], 18, 24, 13)
    assert len(diffs) == len(cols) == len(cigars) == 0 and gpu_ctx.nw_batch_totals() == [0, 0, 0, 0]


# ---- the writers: GPU against host, same process ---------------------------------------------------------------

def _d1(ctx, fa, fastidious=False):
    from swarm_amd import D1Clusters, HostDb
    hdb = HostDb(fa)
    ctx.upload_hostdb(hdb)
    assert ctx.d1_index_build() is False
    off, nb = ctx.d1_network()
    cl = D1Clusters(hdb, off, nb)
    if fastidious:
        flags, stats = cl.light_flags(3)
        graft, _ = ctx.d1_fastidious(flags, stats[2], 16)
        cl.graft(graft)
    return hdb, cl


def _same_uclust_d1(ctx, tmp_path, fa, fastidious=False, **kw):
    from swarm_amd import d1_write_uclust
    hdb, cl = _d1(ctx, fa, fastidious)
    d1_write_uclust(cl, tmp_path / "host.u", **kw)
    d1_write_uclust(cl, tmp_path / "gpu.u", ctx=ctx, **kw)
    assert filecmp.cmp(tmp_path / "host.u", tmp_path / "gpu.u", shallow=False)
    return (tmp_path / "gpu.u").read_bytes()


@pytest.mark.parametrize("name", ["tiny_one", "tiny_mix"])
def test_writers_on_tiny_fixtures(gpu_ctx, tmp_path, name):
    from swarm_amd import DnClusters, HostDb
    _same_uclust_d1(gpu_ctx, tmp_path, G / f"{name}.fasta")
    hdb = HostDb(G / f"{name}.fasta")
    gpu_ctx.upload_hostdb(hdb)
    cl = DnClusters(gpu_ctx, hdb, 2)
    cl.write_uclust(tmp_path / "h2.u")
    cl.write_uclust(tmp_path / "g2.u", ctx=gpu_ctx)
    assert filecmp.cmp(tmp_path / "h2.u", tmp_path / "g2.u", shallow=False)


def test_writers_on_singletons_and_one_nt(gpu_ctx, tmp_path):
    fa = tmp_path / "single.fa"
    _write_db(fa, ["ACGT" * 10 + "A" * k + "C" * 6 for k in range(0, 60, 3)])     # >= 2 differences apart: no H line
    out = _same_uclust_d1(gpu_ctx, tmp_path, fa)
    assert b"\nH\t" not in out and out.count(b"\nC\t") + out.startswith(b"C\t") == 20
    fa = tmp_path / "one.fa"
    _write_db(fa, ["A", "C", "G", "T", "AC", "CA", "ACG"])
    out = _same_uclust_d1(gpu_ctx, tmp_path, fa, usearch=False, append_abundance=0)
    assert b"H\t" in out


def test_writer_many_chunks_and_user_scoring(gpu_ctx, tmp_path, monkeypatch):
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 8000, 150, 41, 1, 0.3)
    whole = _same_uclust_d1(gpu_ctx, tmp_path, fa, fastidious=True)
    monkeypatch.setenv("SWA_NW_CHUNK", "97")
    assert _same_uclust_d1(gpu_ctx, tmp_path, fa, fastidious=True) == whole
    assert _same_uclust_d1(gpu_ctx, tmp_path, fa, penalties=(4, 12, 1)) != b""
    from swarm_amd import DnClusters, HostDb
    hdb = HostDb(fa)
    gpu_ctx.upload_hostdb(hdb)
    cl = DnClusters(gpu_ctx, hdb, 3, penalties=(7, 11, 3))
    cl.write_uclust(tmp_path / "h3.u", usearch=True)
    cl.write_uclust(tmp_path / "g3.u", usearch=True, ctx=gpu_ctx)
    assert filecmp.cmp(tmp_path / "h3.u", tmp_path / "g3.u", shallow=False)


@pytest.mark.parametrize("light", [0.0, 0.3])
def test_writer_full_size(gpu_ctx, tmp_path, light):
    """the 1 M x 150 bench sets (tests/golden/fullsize.json), with and without --fastidious"""
    import bench
    fa = bench.gen_fasta(1_000_000, 150, 1, 1, light)
    _same_uclust_d1(gpu_ctx, tmp_path, fa, fastidious=light > 0)


# ---- the command line --------------------------------------------------------------------------------------------

def _cli(args, fa, tmp_path, tag, env=None):
    u, o = tmp_path / f"{tag}.u", tmp_path / f"{tag}.o"
    r = subprocess.run([str(BIN)] + args + ["-u", str(u), "-o", str(o), "-l", "/dev/null", str(fa)], capture_output=True,
                       text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr
    return u, o


@pytest.mark.parametrize("env", [{}, {"SWA_NW_CHUNK": "1000"}, {"SWARM_AMD_READ_CHUNK_KB": "1"}, {"SWARM_AMD_DEVICES": "0,0"}])
@pytest.mark.parametrize("name", ["d1_uclust", "d3_400"])
def test_cli_uclust_fixtures(tmp_path, name, env):
    args = (G / f"{name}.args").read_text().split()
    u, o = _cli(args, G / f"{name}.fasta", tmp_path, "g", env)
    assert filecmp.cmp(u, G / f"{name}.u", shallow=False)
    assert filecmp.cmp(o, G / f"{name}.o", shallow=False)


def test_cli_uclust_empty_input(tmp_path):
    for d in ("1", "2"):
        u, _ = _cli(["-d", d], G / "tiny_empty.fasta", tmp_path, f"e{d}")
        assert u.read_bytes() == b""


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("n,length,seed,light,args,env", [
    (60000, 150, 401, 0.0, ["-d", "1"], {}),
    (60000, 150, 402, 0.3, ["-d", "1", "-f"], {}),
    (60000, 150, 402, 0.3, ["-d", "1", "-f"], {"SWA_NW_CHUNK": "1000"}),
    (60000, 150, 402, 0.3, ["-d", "1", "-f"], {"SWARM_AMD_READ_CHUNK_KB": "1"}),
    (60000, 150, 402, 0.3, ["-d", "1", "-f"], {"SWARM_AMD_DEVICES": "0,0"}),
    (30000, 250, 403, 0.0, ["-d", "1", "-n"], {}),
    (20000, 400, 404, 0.0, ["-d", "3"], {}),
    (20000, 150, 405, 0.0, ["-d", "2", "-m", "3", "-p", "5", "-g", "9", "-e", "2"], {}),
])
def test_cli_uclust_against_reference_binary(tmp_path, n, length, seed, light, args, env):
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, n, length, seed, 2 if "-d" in args and args[args.index("-d") + 1] != "1" else 1, light)
    r = S.run_ref_swarm(list(args) + ["-u", str(tmp_path / "r.u"), "-o", str(tmp_path / "r.o"), "-l", "/dev/null", str(fa)])
    assert r.returncode == 0, r.stderr
    u, o = _cli(list(args), fa, tmp_path, "g", env)
    assert filecmp.cmp(tmp_path / "r.u", u, shallow=False)
    assert filecmp.cmp(tmp_path / "r.o", o, shallow=False)
