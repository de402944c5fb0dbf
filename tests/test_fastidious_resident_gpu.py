"""--fastidious on the clustering that is still in HBM (swarm_amd/csrc/fast_graft.inc): swa_d1_swarm_sums_device,
swa_d1_light_flags_device, swa_d1_fastidious_resident, swa_d1_graft_device and the install step, against numpy statements
(tests/graft_sets.py), against the host's bookkeeping on the same result, and — whole pass and command line — against the
host route byte for byte.  Everything is integer equality.

The sums and flags run on adopted synthetic graphs (swa_d1_network_adopt) over small databases with chosen abundances and
lengths: swarms laid out so that they begin and end on either side of a wave's and a workgroup's last position in the
member order, one swarm of everybody, nobody with anybody, one amplicon, an abundance above 2^32."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import cluster_sets as CS
import fastidious_sets as FS
import graft_sets as GS
import support as S
from swarm_amd import Context, D1Clusters, HostDb, SwaError, capi

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"


# ---- adopted graphs -----------------------------------------------------------------------------------------------------
def _blocks(sizes, abundance=None, deep=()):
    """swarm k = the next sizes[k] ids: its first id is the seed and links to all the others (generation 1), or — k in
    `deep` — the ids form a chain (generation = place in it).  The member order is then 0, 1, 2, ...: swarm k begins at
    member sum(sizes[:k]).  Returns (records, csr, swarmid, generation, abundance, seqlen)."""
    n = int(sum(sizes))
    rng = np.random.default_rng(n)
    src, dst, swarmid, generation = [], [], np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    at = 0
    for k, size in enumerate(sizes):
        ids = np.arange(at, at + size)
        swarmid[ids] = k
        if k in deep:
            src += ids[:-1].tolist(); dst += ids[1:].tolist()
            generation[ids] = np.arange(size)
        else:
            src += [at] * (size - 1); dst += ids[1:].tolist()
            generation[ids[1:]] = 1
        at += size
    csr = CS.csr_from_links(n, src, dst) if src else (np.zeros(n + 1, dtype=np.uint64), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint8))
    if abundance is None:
        abundance = np.sort(rng.integers(1, 4, n))[::-1]
    abundance = np.asarray(abundance, dtype=np.uint64)
    assert (np.diff(abundance.astype(np.int64)) <= 0).all()       # (the reader sorts by abundance: the ids must survive it)
    seqlen = rng.integers(33, 100, n).astype(np.uint32)
    seen, records = set(), []
    for i in range(n):
        while True:
            s = "".join("ACGT"[v] for v in rng.integers(0, 4, int(seqlen[i])))
            if s not in seen:
                break
        seen.add(s)
        records.append((f"a{i:06d}_{int(abundance[i])}", s))
    return records, csr, swarmid, generation, abundance, seqlen


def _adopt(ctx, tmp_path, records, csr):
    """the database uploaded, the graph adopted and clustered on the device: (hdb, lazy result, swarmid, generation, begins)"""
    fa = tmp_path / "in.fa"
    GS.write_fasta(fa, records)
    hdb = HostDb(fa)
    ctx.upload_hostdb(hdb)
    ctx.d1_network_adopt(csr[0], csr[1])
    cl = D1Clusters.from_resident(ctx, hdb, lazy=True)
    swarmid, generation, _ = ctx.d1_cluster_fetch()
    return hdb, cl, swarmid, generation


def _same_sums(got, want):
    for g, w, name in zip(got, want, ("mass", "sumlen", "singletons", "maxgen")):
        assert g.dtype == w.dtype and np.array_equal(g, w), name


LAYOUTS = {
    "one_swarm": ([777], ()),
    "singletons": ([1] * 333, ()),
    "one_amplicon": ([1], ()),
    # swarms that begin at members 63, 64, 255, 256 (and end at 63, 64, 255, 256) of the order; 301 amplicons
    "wave_and_block_edges": ([63, 1, 191, 1, 45], (2,)),
    # 3000 members across a dozen workgroups of 256, one-member swarms on both sides; n = 3005 is no multiple of 64
    "across_workgroups": ([1, 1, 3000, 1, 1, 1], ()),
    "deep_and_flat": ([70, 5, 130, 2, 64, 64, 1, 1, 129], (0, 4)),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_sums_and_flags_on_laid_out_swarms(gpu_ctx, tmp_path, name):
    sizes, deep = LAYOUTS[name]
    n = sum(sizes)
    abundance = None
    if name == "wave_and_block_edges":                           # the first swarm's mass passes 2^32 twice over
        abundance = np.sort(np.random.default_rng(5).integers(1, 4, n))[::-1].astype(np.uint64)
        abundance[0], abundance[1] = (1 << 33) + 5, (1 << 32) + 1
    records, csr, swarmid, generation, abundance, seqlen = _blocks(sizes, abundance, deep)
    hdb, cl, got_sid, got_gen = _adopt(gpu_ctx, tmp_path, records, csr)
    assert np.array_equal(hdb.abundance, abundance) and np.array_equal(hdb.seqlen, seqlen)
    assert np.array_equal(got_sid, swarmid) and np.array_equal(got_gen, generation)
    w = len(sizes)
    want = GS.sums_of(swarmid, generation, abundance, seqlen, w)
    _same_sums(gpu_ctx.d1_swarm_sums_device(w), want)
    if name == "wave_and_block_edges":
        assert int(want[0][0]) > 1 << 33 and int(want[0][0]) % (1 << 32) != int(want[0][0])
    with pytest.raises(SwaError) as e:                           # arrays one entry short
        gpu_ctx.d1_swarm_sums_device(w - 1)
    assert e.value.code == capi.SWA_E_CAPACITY
    # every boundary at which some swarm changes sides: mass == boundary is heavy, mass == boundary - 1 light; 1: all heavy;
    # one past the largest mass: all light
    mass = want[0]
    boundaries = sorted({1, int(mass.max()) + 1} | {int(m) + d for m in np.unique(mass)[:6] for d in (0, 1)})
    seen = set()
    for boundary in boundaries:
        flags, stats = gpu_ctx.d1_light_flags_device(boundary)
        light_swarm = mass < np.uint64(boundary)
        assert np.array_equal(flags, light_swarm[swarmid].astype(np.uint8))
        assert stats == [int(light_swarm.sum()), int(flags.sum()), int(seqlen[flags != 0].sum()), int((~light_swarm).sum()), int(n - flags.sum())]
        assert gpu_ctx.d1_light_flags_device(boundary, flags=False) == (None, stats)
        seen.add((stats[0] == 0, stats[3] == 0))
    assert (True, False) in seen and (False, True) in seen       # all heavy, all light
    # ... and the host's bookkeeping on the same result (it downloads the details and sums on the CPU)
    assert cl.detail_fetches() == 0
    for boundary in boundaries[:3] + boundaries[-1:]:
        flags, stats = gpu_ctx.d1_light_flags_device(boundary)
        host_flags, host_stats = cl.light_flags(boundary)
        assert np.array_equal(flags, host_flags) and stats == host_stats
    assert cl.detail_fetches() == 1


@pytest.mark.parametrize("seed,n,share", GS.CASES)
def test_sums_flags_and_grafting_on_random_clusterings(gpu_ctx, tmp_path, seed, n, share):
    """the cases of tests/test_graft_identity.py: member orders that are no identity, generations of any depth; the four
    arrays, the withdrawn candidates and the grown sums against the closed form; a lazy result with the grafts installed
    writes what the host's walk writes"""
    case = GS.make_case(seed, n, share)
    want = case.want
    hdb, cl, swarmid, generation = _adopt(gpu_ctx, tmp_path, case.records, case.csr)
    assert np.array_equal(swarmid, want.swarmid) and np.array_equal(generation, want.generation)
    w = len(want.begins) - 1
    sums = GS.sums_of(swarmid, generation, case.abundance, case.seqlen, w)
    _same_sums(gpu_ctx.d1_swarm_sums_device(w), sums)
    flags, stats = gpu_ctx.d1_light_flags_device(case.boundary)
    assert np.array_equal(flags, case.light)
    g = GS.closed_form(swarmid, case.cand)
    got = gpu_ctx.d1_graft_device(case.cand)
    for a, b, what in zip(got, g[:4], ("heavy swarm", "light swarm", "parent", "child")):
        assert a.dtype == np.uint32 and np.array_equal(a, b), what
    assert np.array_equal(gpu_ctx.d1_graft_candidates(), g.kept)
    grown, sizes = GS.grown(sums, np.diff(want.begins), g)
    _same_sums(gpu_ctx.d1_swarm_sums_device(w), grown)
    # a second call starts from the swarms' own sums and the candidates in HBM (the winners'): the same grafts, sums grown once
    again = gpu_ctx.d1_graft_device(None)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    _same_sums(gpu_ctx.d1_swarm_sums_device(w), grown)
    # installed into the lazy result: nothing is downloaded for it or for -o; -s / -i / -w then fold the grafts in
    cl.install_graft(*got)
    assert cl.summary()["swarms"] == w - len(g.heavy) and cl.summary()["largest"] == int(sizes.max())
    cl.write_swarms(tmp_path / "d.o")
    assert cl.detail_fetches() == 0
    for k, write in (("s", cl.write_stats), ("i", cl.write_structure), ("w", cl.write_seeds)):
        write(tmp_path / f"d.{k}")
    assert cl.detail_fetches() == 1
    host = D1Clusters(hdb, case.csr[0], case.csr[1])
    assert host.graft(case.cand) == len(g.heavy)
    for k, write in (("o", host.write_swarms), ("s", host.write_stats), ("i", host.write_structure), ("w", host.write_seeds)):
        write(tmp_path / f"h.{k}")
        assert filecmp.cmp(tmp_path / f"h.{k}", tmp_path / f"d.{k}", shallow=False), k


def test_grafts_one_past_a_workgroup_and_a_table_one_short(gpu_ctx, tmp_path):
    """257 grafts: the second workgroup of k_graft_apply holds one; three heavy swarms win 86, 86 and 85 light ones, runs
    that cross the waves.  cap = 256: SWA_E_CAPACITY with the need, nothing grown; then the call with room."""
    heavy, lights = 3, 257
    abundance = [9] * heavy + [1] * lights
    records, csr, swarmid, generation, abundance, seqlen = _blocks([1] * (heavy + lights), abundance)
    hdb, cl, got_sid, _ = _adopt(gpu_ctx, tmp_path, records, csr)
    cand = np.full(heavy + lights, GS.NO, dtype=np.uint32)
    cand[heavy:] = np.arange(lights) % heavy
    g = GS.closed_form(swarmid, cand)
    assert len(g.heavy) == 257
    w = heavy + lights
    sums = GS.sums_of(swarmid, generation, abundance, seqlen, w)
    with pytest.raises(SwaError) as e:
        gpu_ctx.d1_graft_device(cand, cap=256)
    assert e.value.code == capi.SWA_E_CAPACITY and e.value.grafts == 257
    _same_sums(gpu_ctx.d1_swarm_sums_device(w), sums)
    got = gpu_ctx.d1_graft_device(cand, cap=257)
    assert all(np.array_equal(a, b) for a, b in zip(got, g[:4]))
    _same_sums(gpu_ctx.d1_swarm_sums_device(w), GS.grown(sums, np.ones(w), g)[0])
    with pytest.raises(SwaError) as e:                           # a candidate that is no amplicon never reaches the device
        gpu_ctx.d1_graft_device(np.where(cand == 1, w, cand).astype(np.uint32))
    assert e.value.code == capi.SWA_E_ARG


# ---- the whole pass -----------------------------------------------------------------------------------------------------
def _cluster_again(ctx, hdb):
    """(the Bloom route of the pass re-purposes the index's table, and an index build ends the clustering)"""
    assert ctx.d1_index_build() is False
    ctx.d1_network_resident()
    return D1Clusters.from_resident(ctx, hdb, lazy=True)


@pytest.mark.parametrize("L", [112, 150, 257])
def test_whole_pass_equals_the_host_route(gpu_ctx, tmp_path, L):
    """sets of tests/fastidious_sets.py: 110 .. 112 nt (both routes of the pass), 150 (register forms), 257 (k_fast_count)"""
    fa = tmp_path / "in.fa"
    db, want_flags, three = FS.build_case(L, fa)
    hdb = HostDb(fa)
    gpu_ctx.upload_hostdb(hdb)
    # the host route, as the command line takes it under SWARM_AMD_FASTIDIOUS=host
    host = _cluster_again(gpu_ctx, hdb)
    flags_h, stats_h = host.light_flags(3)
    assert np.array_equal(flags_h, want_flags)
    graft_h, counters_h = gpu_ctx.d1_fastidious(flags_h, stats_h[2], 16)
    made = host.graft(graft_h)
    assert made >= 1                                              # (a set without a graft would show nothing)
    # the device route
    dev = _cluster_again(gpu_ctx, hdb)
    flags_d, stats_d = gpu_ctx.d1_light_flags_device(3)
    assert np.array_equal(flags_d, flags_h) and stats_d == stats_h
    graft_d, counters_d = gpu_ctx.d1_fastidious_resident(stats_d[2], 16)
    assert np.array_equal(graft_d, graft_h) and [int(x) for x in counters_d[:5]] == [int(x) for x in counters_h[:5]]
    four = gpu_ctx.d1_graft_device(None)
    assert len(four[0]) == made
    swarmid = gpu_ctx.d1_cluster_fetch()[0]
    g = GS.closed_form(swarmid, graft_h)
    assert all(np.array_equal(a, b) for a, b in zip(four, g[:4])) and np.array_equal(gpu_ctx.d1_graft_candidates(), g.kept)
    dev.install_graft(*four)
    assert dev.summary() == host.summary()
    dev.write_swarms(tmp_path / "d.o")
    assert dev.detail_fetches() == 0
    host.write_swarms(tmp_path / "h.o")
    for k in "siw":
        for tag, cl in (("d", dev), ("h", host)):
            {"s": cl.write_stats, "i": cl.write_structure, "w": cl.write_seeds}[k](tmp_path / f"{tag}.{k}")
    for k in "osiw":
        assert filecmp.cmp(tmp_path / f"h.{k}", tmp_path / f"d.{k}", shallow=False), k
    # ... and without the download of the candidates: the same grafts
    dev2 = _cluster_again(gpu_ctx, hdb)
    gpu_ctx.d1_light_flags_device(3, flags=False)
    none, counters_n = gpu_ctx.d1_fastidious_resident(stats_d[2], 16, fetch=False)
    assert none is None and [int(x) for x in counters_n[:5]] == [int(x) for x in counters_h[:5]]
    assert all(np.array_equal(a, b) for a, b in zip(gpu_ctx.d1_graft_device(None), four))
    print(f"L {L}: n {db.n}, {stats_h[0]} light swarms, {int(counters_h[2])} candidates, {made} grafts")


# ---- the command line ---------------------------------------------------------------------------------------------------
def _run(args, env_extra, cwd=None):
    env = dict(os.environ, **env_extra)
    env.pop("SWARM_AMD_DEVICES", None)
    r = subprocess.run([str(BIN)] + args, capture_output=True, text=True, env=env, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_routes_write_the_same_files(tmp_path):
    fa = S.GOLDEN / "d1_fastidious.fasta"
    # (the log names the output file: each route writes the same relative names in a directory of its own)
    for tag, env in (("device", {}), ("host", {"SWARM_AMD_FASTIDIOUS": "host"})):
        (tmp_path / tag).mkdir()
        args = ["-d", "1", "-f"]
        for k in "osiwul":
            args += [f"-{k}", f"out.{k}"]
        _run(args + [str(fa)], env, cwd=tmp_path / tag)
    for k in "osiwul":
        assert filecmp.cmp(tmp_path / "device" / f"out.{k}", tmp_path / "host" / f"out.{k}", shallow=False), k
    log = (tmp_path / "device" / "out.l").read_text()
    assert "Made " in log and "Made 0 grafts" not in log
    for k in "osiw":                                             # ... and the reference's, where the fixture is at hand
        if (S.GOLDEN / f"d1_fastidious.{k}").exists():
            assert filecmp.cmp(tmp_path / "device" / f"out.{k}", S.GOLDEN / f"d1_fastidious.{k}", shallow=False), k


def test_cli_plain_fastidious_run_downloads_no_details(tmp_path):
    """-f -o alone: the closing line of SWARM_AMD_TIMING counts the downloads of swarm id / generation / parent"""
    fa = S.GOLDEN / "d1_fastidious.fasta"
    line = "[details] swarm id, generation and parent downloaded {} time(s)"
    args = ["-d", "1", "-f", "-l", "/dev/null"]
    r = _run(args + ["-o", str(tmp_path / "device.o"), str(fa)], {"SWARM_AMD_TIMING": "1"})
    assert line.format(0) in r.stderr
    r = _run(args + ["-o", str(tmp_path / "host.o"), str(fa)], {"SWARM_AMD_TIMING": "1", "SWARM_AMD_FASTIDIOUS": "host"})
    assert line.format(1) in r.stderr                            # (the line is live: the host route fetches them)
    assert filecmp.cmp(tmp_path / "device.o", tmp_path / "host.o", shallow=False)


# ---- call order -----------------------------------------------------------------------------------------------------------
def test_calls_before_a_clustering_are_refused(tmp_path):
    ctx = Context(0)
    try:
        records, csr, *_ = _blocks([3, 2, 1])
        n = 6

        def refused(call, needle="no clustering in place"):
            with pytest.raises(SwaError) as e:
                call()
            assert e.value.code == capi.SWA_E_ARG and needle in str(e.value), str(e.value)

        ctx.n = n
        calls = [lambda: ctx.d1_swarm_sums_device(3), lambda: ctx.d1_light_flags_device(3), lambda: ctx.d1_fastidious_resident(100),
                 lambda: ctx.d1_graft_device(np.full(n, GS.NO, dtype=np.uint32)), lambda: ctx.d1_graft_device(None),
                 lambda: ctx.d1_graft_candidates()]
        for call in calls:                                        # no database at all
            refused(call)
        fa = tmp_path / "in.fa"
        GS.write_fasta(fa, records)
        hdb = HostDb(fa)
        ctx.upload_hostdb(hdb)
        for call in calls:                                        # a database
            refused(call)
        ctx.d1_network_adopt(csr[0], csr[1])
        for call in calls:                                        # ... and a network, not clustered yet
            refused(call)
        D1Clusters.from_resident(ctx, hdb)
        refused(lambda: ctx.d1_fastidious_resident(100), "swa_d1_light_flags_device first")
        refused(lambda: ctx.d1_graft_device(None), "no candidates in place")
        flags, stats = ctx.d1_light_flags_device(3)
        refused(lambda: ctx.d1_fastidious_resident(stats[2]), "swa_d1_index_build first")   # (an adopted graph has no index)
        assert ctx.d1_graft_device(np.full(n, GS.NO, dtype=np.uint32))[0].size == 0
        # a new clustering ends the flags and the candidates of the one before
        D1Clusters.from_resident(ctx, hdb)
        refused(lambda: ctx.d1_fastidious_resident(stats[2]), "swa_d1_light_flags_device first")
        refused(lambda: ctx.d1_graft_device(None), "no candidates in place")
        ctx.d1_network_adopt(csr[0], csr[1])                      # ... and so does a new network
        refused(lambda: ctx.d1_light_flags_device(3))
    finally:
        ctx.close()
