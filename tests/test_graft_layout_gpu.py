"""The grafted clustering laid out on the device (swa_d1_graft_layout_device, swarm_amd/csrc/fast_graft.inc) and adopted by
the result (swa_d1_result_adopt_layout): the four arrays and the summary against the closed form of
tests/graft_layout_sets.py (which tests/test_graft_layout_identity.py holds to a walk over the chains), and every file of the
adopted result against the host walk's, byte for byte.  Everything is integer equality.

Adopted synthetic graphs (swa_d1_network_adopt) with host candidates: the random clusterings of tests/graft_sets.py, grafts
one past a workgroup, one run across many workgroups and the scans' tiles, light swarms whose blocks start and end on both
sides of wave and workgroup edges of the move kernel, light swarms before their heavy swarm, one swarm, one amplicon; the
refusals; the whole pass on sets of tests/fastidious_sets.py; the command line under SWARM_AMD_FASTIDIOUS=layout."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import fastidious_sets as FS
import graft_layout_sets as LS
import graft_sets as GS
import support as S
from swarm_amd import Context, D1Clusters, HostDb, SwaError, capi

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
KINDS = (("o", "write_swarms"), ("s", "write_stats"), ("i", "write_structure"), ("w", "write_seeds"))


def _adopt(ctx, tmp_path, records, csr):
    """the database uploaded, the graph adopted and clustered on the device: (hdb, lazy result)"""
    fa = tmp_path / "in.fa"
    GS.write_fasta(fa, records)
    hdb = HostDb(fa)
    ctx.upload_hostdb(hdb)
    ctx.d1_network_adopt(csr[0], csr[1])
    return hdb, D1Clusters.from_resident(ctx, hdb, lazy=True)


def _layout(d) -> tuple:
    return d["printed_order"], d["new_begin"], d["grown"], d["attached"], d["summary"]


def _files_equal_the_walk(ctx, cl, host, tmp_path):
    """the adopted lazy result `cl` against the host's walk `host`: -o without a download of the details, -s -i -w after one"""
    assert cl.graft_route() == 3 and host.graft_route() == 1
    assert cl.summary() == host.summary()
    cl.write_swarms(tmp_path / "d.o")
    assert cl.detail_fetches() == 0
    for k, write in KINDS[1:]:
        getattr(cl, write)(tmp_path / f"d.{k}")
        assert cl.detail_fetches() == 1
    for k, write in KINDS:
        getattr(host, write)(tmp_path / f"h.{k}")
        assert filecmp.cmp(tmp_path / f"h.{k}", tmp_path / f"d.{k}", shallow=False), k


def _graft_lay_adopt(ctx, tmp_path, records, csr, swarmid, begins, order, cand):
    hdb, cl = _adopt(ctx, tmp_path, records, csr)
    got_sid = ctx.d1_cluster_fetch()[0]
    assert np.array_equal(got_sid, swarmid)
    g = GS.closed_form(swarmid, cand)
    four = ctx.d1_graft_device(cand)
    assert np.array_equal(four[0], g.heavy) and np.array_equal(four[1], g.light)
    want = LS.closed_form_layout(begins, order, (g.heavy, g.light))
    LS.same_layout(_layout(ctx.d1_graft_layout_device()), want)
    info = ctx.d1_graft_layout_info()
    assert info == {"in_place": True, "n": len(swarmid), "swarms": len(begins) - 1, "grafts": len(g.heavy)}
    LS.same_layout(_layout(ctx.d1_graft_layout_device()), want)  # a second call: the same arrays
    assert ctx.d1_graft_layout_device(fetch=False)["summary"] == want[4]
    cl.adopt_layout(ctx)
    host = D1Clusters(hdb, csr[0], csr[1])
    assert host.graft(cand) == len(g.heavy)
    _files_equal_the_walk(ctx, cl, host, tmp_path)
    return g, want


@pytest.mark.parametrize("seed,n,share", GS.CASES)
def test_layout_on_random_clusterings(gpu_ctx, tmp_path, seed, n, share):
    """member orders that are no identity; seed 11 has no graft: the layout is the clustering's own"""
    case = GS.make_case(seed, n, share)
    want = case.want
    g, layout = _graft_lay_adopt(gpu_ctx, tmp_path, case.records, case.csr, want.swarmid, want.begins, want.order, case.cand)
    if share == 0.0:
        assert len(g.heavy) == 0 and np.array_equal(layout[0], want.order) and np.array_equal(layout[1], want.begins[:-1])


@pytest.mark.parametrize("name", list(LS.HAND_MADE))
def test_layout_on_hand_made_sets(gpu_ctx, tmp_path, name):
    """257 grafts (the second workgroup holds one; runs of 86 / 86 / 85 cross the waves); one run of 5000 grafts; light swarms
    of 1, 2, 63, 64, 65 and 300 members behind 3000 own members, n no multiple of 64; one swarm; one amplicon"""
    records, csr, swarmid, begins, cand = LS.hand_made(name)
    n = len(swarmid)
    g, layout = _graft_lay_adopt(gpu_ctx, tmp_path, records, csr, swarmid, begins, np.arange(n, dtype=np.uint32), cand)
    assert len(g.heavy) == len(LS.HAND_MADE[name][2])
    if len(g.heavy) == 0:
        assert np.array_equal(layout[0], np.arange(n)) and layout[4] == [len(begins) - 1, int(np.diff(begins).max()), 0]
    if name == "blocks_across_edges":
        assert n % 64 != 0 and layout[1][1:7].tolist() == [3000, 3001, 3003, 3066, 3130, 3195]


def test_light_swarms_before_their_heavy_swarm(gpu_ctx, tmp_path):
    records, csr, swarmid, begins, cand, boundary = LS.lights_first()
    g, layout = _graft_lay_adopt(gpu_ctx, tmp_path, records, csr, swarmid, begins, np.arange(10, dtype=np.uint32), cand)
    assert (g.light < g.heavy).sum() == 4 and layout[0].tolist() == [2, 5, 6, 7, 1, 4, 9, 0, 3, 8]
    # the flags of the device at this boundary agree that the parents are heavy and the children light
    flags, stats = gpu_ctx.d1_light_flags_device(boundary)
    assert flags.tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 1, 1] and stats[3] == 1


def test_refusals(tmp_path):
    ctx = Context(0)
    try:
        case = GS.make_case(*GS.CASES[2])
        want = case.want
        n, w = len(want.swarmid), len(want.begins) - 1

        def refused(call, needle, code=capi.SWA_E_ARG):
            with pytest.raises(SwaError) as e:
                call()
            assert e.value.code == code and needle in str(e.value), str(e.value)

        ctx.n = n
        refused(lambda: ctx.d1_graft_layout_device(), "no clustering in place")          # no database at all
        hdb, cl = _adopt(ctx, tmp_path, case.records, case.csr)
        refused(lambda: ctx.d1_graft_layout_device(), "no grafts in place")              # a clustering, no graft call yet
        refused(lambda: cl.adopt_layout(ctx), "holds no layout")
        assert not ctx.d1_graft_layout_info()["in_place"]
        g = GS.closed_form(want.swarmid, case.cand)
        with pytest.raises(SwaError) as e:                                               # a graft call that did not complete
            ctx.d1_graft_device(case.cand, cap=len(g.heavy) - 1)
        assert e.value.code == capi.SWA_E_CAPACITY
        refused(lambda: ctx.d1_graft_layout_device(), "no grafts in place")
        four = ctx.d1_graft_device(case.cand)
        layout = LS.closed_form_layout(want.begins, want.order, (g.heavy, g.light))
        refused(lambda: ctx.d1_graft_layout_device(nswarms=w - 1), "fewer entries", capi.SWA_E_CAPACITY)
        assert not ctx.d1_graft_layout_info()["in_place"]                                # ... with nothing changed
        LS.same_layout(_layout(ctx.d1_graft_layout_device(nswarms=w)), layout)
        refused(lambda: ctx.d1_graft_layout_device(nswarms=w - 1), "fewer entries", capi.SWA_E_CAPACITY)
        # a result with grafts installed: refused, untouched, and still writing the right -o
        cl.install_graft(*four)
        before = cl.summary()
        refused(lambda: cl.adopt_layout(ctx), "holds grafts already")
        assert cl.summary() == before and cl.graft_route() == 2
        host = D1Clusters(hdb, case.csr[0], case.csr[1])
        host.graft(case.cand)
        cl.write_swarms(tmp_path / "d.o")
        host.write_swarms(tmp_path / "h.o")
        assert filecmp.cmp(tmp_path / "h.o", tmp_path / "d.o", shallow=False)
        # a result of another n
        other = GS.make_case(*GS.CASES[5])
        (tmp_path / "other").mkdir()
        GS.write_fasta(tmp_path / "other" / "in.fa", other.records)
        hdb2 = HostDb(tmp_path / "other" / "in.fa")
        cl2 = D1Clusters(hdb2, other.csr[0], other.csr[1])
        refused(lambda: cl2.adopt_layout(ctx), "another clustering")
        assert cl2.graft_route() == 0
        # the next graft call ends the layout (and makes the grafts again); a caller's candidates end it too
        ctx.d1_graft_device(None, cap=0)
        assert not ctx.d1_graft_layout_info()["in_place"]
        LS.same_layout(_layout(ctx.d1_graft_layout_device()), layout)
        # a new network ends everything
        ctx.d1_network_adopt(case.csr[0], case.csr[1])
        refused(lambda: ctx.d1_graft_layout_device(), "no clustering in place")
        assert not ctx.d1_graft_layout_info()["in_place"]
        D1Clusters.from_resident(ctx, hdb)
        refused(lambda: ctx.d1_graft_layout_device(), "no grafts in place")
    finally:
        ctx.close()


# ---- the whole pass -----------------------------------------------------------------------------------------------------
def _cluster_again(ctx, hdb):
    """(the Bloom route of the pass re-purposes the index's table, and an index build ends the clustering)"""
    assert ctx.d1_index_build() is False
    ctx.d1_network_resident()
    return D1Clusters.from_resident(ctx, hdb, lazy=True)


def _order_of(swarmid, generation):
    """members by (generation, id), swarms by seed id: (begins, order) of the clustering"""
    order = np.lexsort((np.arange(len(swarmid)), generation, swarmid)).astype(np.uint32)
    begins = np.concatenate(([0], np.cumsum(np.bincount(swarmid.astype(np.int64))))).astype(np.uint32)
    return begins, order


@pytest.mark.parametrize("L", [112, 150, 257])
def test_whole_pass_equals_the_host_route(gpu_ctx, tmp_path, L):
    fa = tmp_path / "in.fa"
    db, want_flags, three = FS.build_case(L, fa)
    hdb = HostDb(fa)
    gpu_ctx.upload_hostdb(hdb)
    host = _cluster_again(gpu_ctx, hdb)
    flags_h, stats_h = host.light_flags(3)
    graft_h, counters_h = gpu_ctx.d1_fastidious(flags_h, stats_h[2], 16)
    made = host.graft(graft_h)
    assert made >= 1
    # flags, the pass, the grafts, the layout: nothing but counters comes home
    dev = _cluster_again(gpu_ctx, hdb)
    assert gpu_ctx.d1_light_flags_device(3, flags=False)[1] == stats_h
    none, counters_d = gpu_ctx.d1_fastidious_resident(stats_h[2], 16, fetch=False)
    assert none is None and [int(x) for x in counters_d[:5]] == [int(x) for x in counters_h[:5]]
    assert all(len(a) == 0 for a in gpu_ctx.d1_graft_device(None, cap=0))
    assert gpu_ctx.d1_graft_layout_device(fetch=False)["summary"][2] == made
    swarmid, generation, _ = gpu_ctx.d1_cluster_fetch()
    begins, order = _order_of(swarmid, generation)
    g = GS.closed_form(swarmid, graft_h)
    LS.same_layout(_layout(gpu_ctx.d1_graft_layout_device()), LS.closed_form_layout(begins, order, (g.heavy, g.light)))
    dev.adopt_layout(gpu_ctx)
    _files_equal_the_walk(gpu_ctx, dev, host, tmp_path)


# ---- the command line ---------------------------------------------------------------------------------------------------
def _run(args, env_extra, cwd=None):
    env = dict(os.environ)
    for name in ("SWARM_AMD_DEVICES", "SWARM_AMD_FASTIDIOUS", "SWARM_AMD_MULTI_CLUSTER"):
        env.pop(name, None)
    env.update(env_extra)
    r = subprocess.run([str(BIN)] + args, capture_output=True, text=True, env=env, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_routes_write_the_same_files(tmp_path):
    fa = S.GOLDEN / "d1_fastidious.fasta"
    kinds = "osiwul"
    runs = (("layout", {"SWARM_AMD_FASTIDIOUS": "layout"}, []), ("default", {}, []), ("install", {"SWARM_AMD_FASTIDIOUS": "install"}, []),
            ("host", {"SWARM_AMD_FASTIDIOUS": "host"}, []),
            ("two", {"SWARM_AMD_FASTIDIOUS": "layout", "SWARM_AMD_DEVICES": "0,0"}, []),
            ("layout_r", {"SWARM_AMD_FASTIDIOUS": "layout"}, ["-r"]), ("host_r", {"SWARM_AMD_FASTIDIOUS": "host"}, ["-r"]))
    for tag, env, more in runs:
        (tmp_path / tag).mkdir()
        args = ["-d", "1", "-f"] + more
        for k in kinds:
            args += [f"-{k}", f"out.{k}"]
        _run(args + [str(fa)], env, cwd=tmp_path / tag)
    for tag in ("default", "install", "host", "two"):
        for k in kinds.replace("l", "") if tag == "two" else kinds:    # (several ranks say more in their log)
            assert filecmp.cmp(tmp_path / "layout" / f"out.{k}", tmp_path / tag / f"out.{k}", shallow=False), (tag, k)
    for k in kinds:
        assert filecmp.cmp(tmp_path / "layout_r" / f"out.{k}", tmp_path / "host_r" / f"out.{k}", shallow=False), k
    log = (tmp_path / "layout" / "out.l").read_text()
    assert "Made " in log and "Made 0 grafts" not in log
    for k in "osiw":                                             # ... and the reference's, where the fixture is at hand
        if (S.GOLDEN / f"d1_fastidious.{k}").exists():
            assert filecmp.cmp(tmp_path / "layout" / f"out.{k}", S.GOLDEN / f"d1_fastidious.{k}", shallow=False), k


def test_cli_layout_run_downloads_no_details(tmp_path):
    fa = S.GOLDEN / "d1_fastidious.fasta"
    args = ["-d", "1", "-f", "-l", "/dev/null"]
    r = _run(args + ["-o", str(tmp_path / "layout.o"), str(fa)], {"SWARM_AMD_TIMING": "1", "SWARM_AMD_FASTIDIOUS": "layout"})
    assert "grafts laid out on the device" in r.stderr
    assert "[details] swarm id, generation and parent downloaded 0 time(s)" in r.stderr
    r = _run(args + ["-o", str(tmp_path / "install.o"), str(fa)], {"SWARM_AMD_TIMING": "1", "SWARM_AMD_FASTIDIOUS": "install"})
    assert "grafts laid out on the device" not in r.stderr      # (the switch is live: the route before has no such milestone)
    assert "[details] swarm id, generation and parent downloaded 0 time(s)" in r.stderr
    assert filecmp.cmp(tmp_path / "layout.o", tmp_path / "install.o", shallow=False)
