"""Several ranks, everything behind the exchange on rank 0's GPU (swarm_amd/csrc/multi.hip: swa_multi_d1_network_resident,
swa_multi_d1_fastidious_resident, swa_multi_dn_graph_resident; fast_graft.inc: the shard-owner kernels; the command line
under SWARM_AMD_MULTI_CLUSTER).  A one-GPU box lists device 0 several times (device-to-device copies) and runs ONE rank
through RCCL (the ncclBroadcast / ncclAllReduce calls themselves).  Whatever the device list and the route, the result is
the single-GPU result, entry for entry and byte for byte."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import graft_sets as GS
import support as S
from swarm_amd import Context, HostDb, MultiContext, SwaError, capi

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
G = S.GOLDEN

# (devices, SWARM_AMD_FORCE_RCCL, SWARM_AMD_MULTI_BUILD)
# (one rank with and without RCCL: a communicator of size 1, and no exchange at all)
CONFIGS = [([0, 0], False, "records"), ([0, 0, 0], False, "records"), ([0, 0, 0], False, "streamed"), ([0], True, "records"),
           ([0], False, "records")]


def _multi(monkeypatch, devices, rccl, build):
    if rccl:
        monkeypatch.setenv("SWARM_AMD_FORCE_RCCL", "1")
    monkeypatch.setenv("SWARM_AMD_MULTI_BUILD", build)
    m = MultiContext(devices)
    assert m.uses_rccl() is rccl
    return m


def _same(got, want, names):
    for a, b, name in zip(got, want, names):
        assert a.dtype == b.dtype and np.array_equal(a, b), name


FIVE = ("swarm id", "generation", "parent", "order", "bounds")
FOUR = ("heavy swarm", "light swarm", "parent", "child")


# ---- 1. the owner kernels at their edges ----------------------------------------------------------------------------------
TILE, TURN = capi.shard_owner_plan()
OWNER_N = [1, 2, 3, 4, 5, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3] + ([TILE * TURN + 1] if TURN else [])
BOUNDARY = 3


def _singletons(ctx, heavy):
    """n amplicons of 32 nt, every one a swarm of its own (a network without links), heavy[a] deciding the abundance on
    either side of the boundary; clustered, not flagged yet"""
    n = len(heavy)
    seqs = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(n)     # distinct words
    abundance = np.where(heavy, BOUNDARY, BOUNDARY - 1).astype(np.uint64)
    ctx.upload_db(seqs, np.arange(n + 1, dtype=np.uint64), np.full(n, 32, dtype=np.uint32), abundance, 32)
    ctx.d1_network_adopt(np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32))
    begins = ctx.d1_cluster_device(details=False)[4]
    assert len(begins) == n + 1


def _want_owners(heavy, nshards):
    h = np.cumsum(heavy, dtype=np.uint64) - heavy.astype(np.uint64)
    total = int(heavy.sum())
    owner = ((h + np.uint64(1)) * np.uint64(nshards) - np.uint64(1)) // np.uint64(max(total, 1))
    return np.where(heavy, owner, 255).astype(np.uint8), total


@pytest.mark.parametrize("n", OWNER_N)
def test_owner_bytes_at_the_kernels_edges(gpu_ctx, n):
    rng = np.random.default_rng(n)
    patterns = {"all light": np.zeros(n, dtype=bool), "all heavy": np.ones(n, dtype=bool), "first heavy": np.arange(n) == 0,
                "last heavy": np.arange(n) == n - 1, "alternating": np.arange(n) % 2 == 1, "random": rng.random(n) < 0.4}
    for name, heavy in patterns.items():
        _singletons(gpu_ctx, heavy)
        flags, stats = gpu_ctx.d1_light_flags_device(BOUNDARY)
        assert np.array_equal(flags, (~heavy).astype(np.uint8)), name
        for nshards in (1, 2, 3, 64):
            want, total = _want_owners(heavy, nshards)
            got, counted = gpu_ctx.d1_shard_owners_device(nshards)
            assert counted == total == stats[4], (name, nshards)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (name, nshards, np.flatnonzero(got != want)[:8])
            assert gpu_ctx.d1_shard_owners_device(nshards, fetch=False) == (None, total)


def test_owner_bytes_need_flags_and_a_shard_count(gpu_ctx):
    _singletons(gpu_ctx, np.arange(10) < 4)
    with pytest.raises(SwaError) as e:                            # clustered, not flagged
        gpu_ctx.d1_shard_owners_device(2)
    assert e.value.code == capi.SWA_E_ARG and "swa_d1_light_flags_device first" in str(e.value)
    gpu_ctx.d1_light_flags_device(BOUNDARY)
    for nshards in (0, 65):
        with pytest.raises(SwaError) as e:
            gpu_ctx.d1_shard_owners_device(nshards)
        assert e.value.code == capi.SWA_E_ARG
    assert gpu_ctx.d1_shard_owners_device(2)[1] == 4
    gpu_ctx.d1_cluster_device(details=False)                      # a new clustering ends the flags
    with pytest.raises(SwaError) as e:
        gpu_ctx.d1_shard_owners_device(2)
    assert e.value.code == capi.SWA_E_ARG


# ---- 2. / 3. the network, its clustering and the fastidious pass on rank 0 ------------------------------------------------
def _single_reference(fa):
    """what one context makes of the set: networks with and without cluster breaking, the clustering, flags, candidates,
    counters and grafts — computed once, never changed"""
    hdb = HostDb(fa)
    ctx = Context(0)
    ctx.upload_hostdb(hdb)
    ref = {"hdb": hdb, "fa": fa}
    for ncb in (True, False):                                      # (False last: its clustering is the one that goes on)
        assert ctx.d1_index_build() is False
        total = ctx.d1_network_resident(ncb)
        ref["net", ncb] = ctx.d1_network_fetch(total)
        ref["cluster", ncb] = ctx.d1_cluster_device()
    ref["flags"], ref["stats"] = ctx.d1_light_flags_device(3)
    ref["cand"], ref["counters"] = ctx.d1_fastidious_resident(ref["stats"][2], 16)
    ref["grafts"] = ctx.d1_graft_device(None)
    ref["kept"] = ctx.d1_graft_candidates()
    ctx.close()
    for a in list(ref["net", True]) + list(ref["net", False]) + list(ref["cluster", False]) + [ref["cand"], ref["kept"]] + list(ref["grafts"]):
        a.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def light_set(tmp_path_factory):
    fa = tmp_path_factory.mktemp("multi_resident") / "in.fa"
    S.gen_fasta(fa, 60000, 150, 61, 1, 0.3)
    ref = _single_reference(fa)
    assert len(ref["net", False][1]) > 1000 and len(ref["grafts"][0]) >= 1
    return ref


@pytest.fixture(scope="module")
def golden_fastidious():
    return _single_reference(G / "d1_fastidious.fasta")


@pytest.mark.parametrize("devices,rccl,build", CONFIGS)
def test_network_resident_on_rank_0(light_set, monkeypatch, devices, rccl, build):
    ref = light_set
    m = _multi(monkeypatch, devices, rccl, build)
    try:
        m.upload_hostdb(ref["hdb"])
        c0 = m.ctx(0)
        for ncb in (False, True, False):
            total = m.d1_network_resident(ncb)
            assert total == len(ref["net", ncb][1])
            _same(c0.d1_network_fetch(total), ref["net", ncb], ("offsets", "neighbours"))
            _same(c0.d1_cluster_device(), ref["cluster", ncb], FIVE)
        c0.close()                                                # (a view: the handle lives on)
        assert m.ctx(0).d1_cluster_maxgen() == int(ref["cluster", False][1].max())
    finally:
        m.close()


def test_a_failed_network_call_leaves_no_resident_network(light_set, tmp_path):
    fa = tmp_path / "dup.fa"
    seq = "ACGTTGCAAGCTTAGCGATCGGATCCATGCAAGTCTAGCTAGGCTAACGTACGATCGATCGTAGCTAGCTAGCATCGATCAGCTACGACTAGCATCAGCTAC"
    fa.write_text(f">a_3\n{seq}\n>b_2\n{seq}\n>c_1\n{seq[:-1]}G\n")
    m = MultiContext([0, 0])
    try:
        m.upload_hostdb(light_set["hdb"])
        total = m.d1_network_resident()
        assert len(m.ctx(0).d1_network_fetch(total)[1]) == total   # a network in place ...
        m.upload_hostdb(HostDb(fa))
        with pytest.raises(SwaError) as e:
            m.d1_network_resident()
        assert e.value.code == capi.SWA_E_DUPLICATES
        with pytest.raises(SwaError) as e:                        # ... and none after the call that failed
            m.ctx(0).d1_network_fetch(0)
        assert e.value.code == capi.SWA_E_ARG and "no resident network" in str(e.value)
    finally:
        m.close()


def _whole_pass(m, ref, fetch):
    c0 = m.ctx(0)
    m.d1_network_resident(False)                                  # (the pass before may have taken the index's table: a new index, a new clustering)
    _same(c0.d1_cluster_device(), ref["cluster", False], FIVE)
    flags, stats = c0.d1_light_flags_device(3, flags=fetch)
    assert stats == ref["stats"] and (flags is None or np.array_equal(flags, ref["flags"]))
    cand, counters = m.d1_fastidious_resident(stats[2], 16, fetch=fetch)
    assert [int(x) for x in counters[:5]] == [int(x) for x in ref["counters"][:5]]
    if fetch:
        assert np.array_equal(cand, ref["cand"])
    else:
        assert cand is None
    four = c0.d1_graft_device(None)
    _same(four, ref["grafts"], FOUR)
    _same(four, GS.closed_form(ref["cluster", False][0], ref["cand"])[:4], FOUR)
    assert np.array_equal(c0.d1_graft_candidates(), ref["kept"])


@pytest.mark.parametrize("devices,rccl,build", CONFIGS)
def test_fastidious_pass_from_rank_0s_flags(light_set, golden_fastidious, monkeypatch, devices, rccl, build):
    m = _multi(monkeypatch, devices, rccl, build)
    try:
        for ref in (light_set, golden_fastidious):
            m.upload_hostdb(ref["hdb"])
            _whole_pass(m, ref, fetch=True)
            _whole_pass(m, ref, fetch=False)
    finally:
        m.close()


def test_fastidious_pass_needs_rank_0s_clustering_and_flags(light_set):
    m = MultiContext([0, 0])
    try:
        m.upload_hostdb(light_set["hdb"])
        m.d1_network_resident()
        for prepare in (lambda: None, lambda: m.ctx(0).d1_cluster_device(details=False)):
            prepare()
            with pytest.raises(SwaError) as e:
                m.d1_fastidious_resident(100)
            assert e.value.code == capi.SWA_E_ARG
    finally:
        m.close()


def test_fewer_heavy_amplicons_than_ranks(tmp_path):
    """two heavy amplicons, three ranks: rank 0's slice of the heavy ones is empty (floor(2 * 1 / 3) = 0), and it still
    counts the light variants; ten light amplicons two substitutions away from a heavy one, five near nobody"""
    rng = np.random.default_rng(7)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    records = []
    for k in range(2):
        heavy = "".join("ACGT"[v] for v in rng.integers(0, 4, 150))
        records.append((f"h{k}_10", heavy))
        for v in range(5):
            s = list(heavy)
            for p in (10 + 10 * v, 80 + 5 * v):
                s[p] = other[s[p]]
            records.append((f"l{k}{v}_1", "".join(s)))
    for v in range(5):
        records.append((f"x{v}_1", "".join("ACGT"[c] for c in rng.integers(0, 4, 150))))
    fa = tmp_path / "few.fa"
    GS.write_fasta(fa, records)
    ref = _single_reference(fa)
    assert ref["stats"][4] == 2 and len(ref["grafts"][0]) == 10
    m = MultiContext([0, 0, 0])
    try:
        m.upload_hostdb(ref["hdb"])
        _whole_pass(m, ref, fetch=True)
        owners, heavy = m.ctx(0).d1_shard_owners_device(3)
        assert heavy == 2 and sorted(owners[owners != 255].tolist()) == [1, 2]
    finally:
        m.close()


# ---- 4. d >= 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d2_small", "d3_400", "d5_ties"])
def test_dn_graph_resident_on_rank_0(name):
    d = int((G / f"{name}.args").read_text().split()[1])
    hdb = HostDb(G / f"{name}.fasta")
    mm, go, ge = capi.reduced_penalties()

    def everything(c, total):
        out = list(c.d1_network_fetch(total)) + [c.d1_network_fetch_diffs(total)]
        out += list(c.d1_cluster_device()) + [c.dn_parent_diffs()]
        sizes = c.dn_tables_device()
        tables = c.dn_tables_fetch()
        return out + [np.array(sizes, dtype=np.uint64)] + [tables[k] for k in sorted(tables)]

    ctx = Context(0)
    ctx.upload_hostdb(hdb)
    ctx.qgram_build()
    ctx.search_begin(mm, go, ge, d)
    assert ctx.dn_graph_supported()
    want = {ncb: everything(ctx, ctx.dn_graph_resident(ncb)) for ncb in (False, True)}
    ctx.close()
    assert len(want[False][1]) > 0
    m = MultiContext([0, 0, 0])
    try:
        m.upload_hostdb(hdb)
        for ncb in (False, True, False):
            total = m.dn_graph_resident(d, ncb, mm, go, ge)
            assert total == len(want[ncb][1])
            got = everything(m.ctx(0), total)
            _same(got, want[ncb], [f"array {k}" for k in range(len(got))])
        # the entry point that downloads still does, and leaves nothing resident
        off, nb, df = m.dn_graph(d, False, mm, go, ge)
        _same((off, nb, df), want[False][:3], ("offsets", "neighbours", "diffs"))
        with pytest.raises(SwaError) as e:
            m.ctx(0).d1_network_fetch(0)
        assert e.value.code == capi.SWA_E_ARG
    finally:
        m.close()


# ---- 5. the command line --------------------------------------------------------------------------------------------------
FLAG = {"o": "-o", "s": "-s", "i": "-i", "j": "-j", "w": "-w", "u": "-u"}
KEEP = ("Number", "Largest", "Max", "Got", "Made", "Heavy var", "Generated")


def _cli(args, kinds, fa, cwd, env_extra):
    """one run in a directory of its own (the log names the output files: the same relative names everywhere)"""
    cwd.mkdir()
    env = dict(os.environ, **env_extra)
    if "SWARM_AMD_DEVICES" not in env_extra:
        env.pop("SWARM_AMD_DEVICES", None)
    cmd = [str(BIN)] + args
    for k in kinds:
        cmd += [FLAG[k], f"out.{k}"]
    r = subprocess.run(cmd + ["-l", "out.l", str(fa)], capture_output=True, text=True, env=env, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r


def _kept(path):
    return [ln for ln in path.read_text().splitlines() if ln.startswith(KEEP)]


def _routes(tmp_path, args, kinds, fa, golden=None):
    _cli(args, kinds, fa, tmp_path / "one", {})
    for devices in ("0,0", "0,0,0"):
        for route, line in (("device", "multi: clustering on rank 0's GPU"), ("host", "multi: clustering on the host")):
            tag = f"{route}{devices.count(',') + 1}"
            r = _cli(args, kinds, fa, tmp_path / tag, {"SWARM_AMD_DEVICES": devices, "SWARM_AMD_MULTI_CLUSTER": route, "SWARM_AMD_MULTI_REPORT": "1"})
            lines = r.stderr.splitlines()
            assert line in lines and lines.index(line) == 1 + next(i for i, ln in enumerate(lines) if ln.startswith("multi: ") and "ranks, exchange" in ln)
            for k in kinds:
                assert filecmp.cmp(tmp_path / "one" / f"out.{k}", tmp_path / tag / f"out.{k}", shallow=False), (tag, k)
                if golden is not None and (G / f"{golden}.{k}").exists():
                    assert filecmp.cmp(tmp_path / tag / f"out.{k}", G / f"{golden}.{k}", shallow=False), (tag, k, "golden")
            assert _kept(tmp_path / "one" / "out.l") == _kept(tmp_path / tag / "out.l"), tag


@pytest.mark.parametrize("args", [["-d", "1"], ["-d", "1", "-f"], ["-d", "1", "-n"], ["-d", "1", "-f", "-b", "10", "-y", "8"]])
def test_cli_d1_routes_are_byte_identical(light_set, tmp_path, args):
    _routes(tmp_path, args, "osijwu", light_set["fa"])


@pytest.mark.parametrize("name", ["d1_1k", "d1_fastidious", "d1_nobreak", "d1_fastidious_b10_y8"])
def test_cli_d1_routes_write_the_reference_files(tmp_path, name):
    _routes(tmp_path, (G / f"{name}.args").read_text().split(), "osijwu", G / f"{name}.fasta", golden=name)


@pytest.mark.parametrize("name", ["d2_small", "d3_400", "d5_ties", "d8_16bit"])
def test_cli_dn_routes_are_byte_identical(tmp_path, name):
    _routes(tmp_path, (G / f"{name}.args").read_text().split(), "osiuw", G / f"{name}.fasta", golden=name)


def test_cli_plain_fastidious_run_downloads_no_details(tmp_path):
    r = _cli(["-d", "1", "-f"], "o", G / "d1_fastidious.fasta", tmp_path / "device",
             {"SWARM_AMD_DEVICES": "0,0", "SWARM_AMD_MULTI_CLUSTER": "device", "SWARM_AMD_TIMING": "1"})
    assert "[details] swarm id, generation and parent downloaded 0 time(s)" in r.stderr
    r = _cli(["-d", "1", "-f"], "o", G / "d1_fastidious.fasta", tmp_path / "host",
             {"SWARM_AMD_DEVICES": "0,0", "SWARM_AMD_MULTI_CLUSTER": "host", "SWARM_AMD_TIMING": "1"})
    assert "[details] swarm id, generation and parent downloaded" in r.stderr
    assert filecmp.cmp(tmp_path / "device" / "out.o", tmp_path / "host" / "out.o", shallow=False)
