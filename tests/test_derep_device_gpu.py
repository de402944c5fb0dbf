"""d = 0 with the clusters made on the GPU (derep.hip: swa_derep_resident, swa_d0_cluster_device, swa_d0_cluster_fetch):
the six arrays and the summary against the closed form of tests/derep_sets.py, every writer's file against the host
route's, the command line's two routes against each other, the re-key rounds, and what ends the resident state."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import derep_sets as DS
import support as S
from swarm_amd import Context, D0Clusters, HostDb, SwaError

pytestmark = pytest.mark.gpu
G = S.GOLDEN
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
NAMES = sorted(DS.SETS) + ["golden"]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """name -> (fasta path, expected tables, first_identical by the oracle): made once, shared, left unchanged"""
    root = tmp_path_factory.mktemp("derep_sets")
    out = {}
    for name in NAMES:
        fa = G / "d0_derep.fasta" if name == "golden" else root / f"{name}.fa"
        if name != "golden":
            DS.SETS[name](fa)
        db = S.db_from_fasta(fa)
        first = S.oracle_derep(db)
        out[name] = (fa, DS.expected_tables(first, db.abundance), first)
    return out


def _write_all(cl, d, tag):
    cl.write_swarms(d / f"{tag}.o")
    cl.write_swarms(d / f"{tag}.or", mothur=True, append_abundance=1)
    cl.write_seeds(d / f"{tag}.w")
    cl.write_stats(d / f"{tag}.s")
    cl.write_structure(d / f"{tag}.i")
    cl.write_uclust(d / f"{tag}.u")
    return ("o", "or", "w", "s", "i", "u")


@pytest.mark.parametrize("name", NAMES)
def test_device_tables_are_the_closed_form(gpu_ctx, sets, name):
    fa, want, _ = sets[name]
    hdb = HostDb(fa)
    gpu_ctx.upload_hostdb(hdb)
    gpu_ctx.derep_resident()
    DS.assert_tables_equal(gpu_ctx.d0_cluster_device(), want, name)


@pytest.mark.parametrize("name", NAMES)
def test_device_route_writes_the_host_routes_files(gpu_ctx, sets, tmp_path, name):
    fa, want, first = sets[name]
    hdb = HostDb(fa)
    gpu_ctx.upload_hostdb(hdb)
    gpu_ctx.derep_resident()
    dev = D0Clusters.from_device(gpu_ctx, hdb)
    DS.assert_tables_equal(dev.tables(), want, name)
    assert dev.summary() == {k: want[k] for k in DS.SUMMARY}
    kinds = _write_all(dev, tmp_path, "dev")
    _write_all(D0Clusters(hdb, first), tmp_path, "host")
    for k in kinds:
        assert filecmp.cmp(tmp_path / f"dev.{k}", tmp_path / f"host.{k}", shallow=False), k
    if name == "golden":
        for k in [k for k in "owsiu" if (G / f"d0_derep.{k}").exists()]:   # (as tests/test_cli_gpu.py takes the fixtures)
            assert filecmp.cmp(tmp_path / f"dev.{k}", G / f"d0_derep.{k}", shallow=False), k


def test_device_route_after_the_rekey_rounds(sets, tmp_path):
    """SWA_DEREP_KEY_BITS=4: different sequences share table slots, the dereplication goes round again with longer keys —
    the tables made from what the rounds leave are the same (own process: the hook is read from the environment)."""
    names = ["random_long", "random_short"]
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {str(S.ROOT)!r})\n"
        "from swarm_amd import Context, HostDb\n"
        "ctx = Context(0)\n"
        f"for name, fa in {[(n, str(sets[n][0])) for n in names]!r}:\n"
        "    hdb = HostDb(fa); ctx.upload_hostdb(hdb); ctx.derep_resident()\n"
        f"    np.savez({str(tmp_path)!r} + '/' + name + '.npz', **ctx.d0_cluster_device())\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(os.environ, SWA_DEREP_KEY_BITS="4"), timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    for name in names:
        DS.assert_tables_equal(dict(np.load(tmp_path / f"{name}.npz")), sets[name][1], name)


def test_command_line_routes_agree(sets, tmp_path):
    """`swarm -d 0 -o -s -w -i -u -l`: the default and SWARM_AMD_D0=host write identical files and identical logs (the
    opposite switch, SWARM_AMD_D0=device, likewise: whichever of the two is the default, both routes run here)."""
    for name in ("wave_edges", "random_long", "random_short"):
        fa = sets[name][0]
        for route in ("default", "host", "device"):
            d = tmp_path / f"{name}_{route}"
            d.mkdir()
            env = dict(os.environ)
            env.pop("SWARM_AMD_D0", None)
            if route != "default":
                env["SWARM_AMD_D0"] = route
            r = subprocess.run([str(BIN), "-d", "0", "-o", "o", "-s", "s", "-w", "w", "-i", "i", "-u", "u", "-l", "l", str(fa)],
                               cwd=d, env=env, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
        for route in ("host", "device"):
            for k in "oswiul":
                assert filecmp.cmp(tmp_path / f"{name}_default" / k, tmp_path / f"{name}_{route}" / k, shallow=False), (name, route, k)
        want = sets[name][1]
        log = (tmp_path / f"{name}_device" / "l").read_text()
        assert f"Number of swarms:  {want['swarms']}\nLargest swarm:     {want['largest']}\nHeaviest swarm:    {want['heaviest']}\n" in log


# ---- what ends what (swa_internal.h: swa_derep_facts) ---------------------------------------------------------------------

def test_tables_need_a_resident_dereplication(sets):
    ctx = Context(0)
    try:
        ctx.upload_hostdb(HostDb(sets["wave_edges"][0]))
        with pytest.raises(SwaError, match="swa_derep_resident"):
            ctx.d0_cluster_device()
        with pytest.raises(SwaError, match="swa_d0_cluster_device"):
            ctx.d0_cluster_fetch()
    finally:
        ctx.close()


def test_an_upload_ends_the_tables(sets):
    ctx = Context(0)
    try:
        hdb = HostDb(sets["wave_edges"][0])
        ctx.upload_hostdb(hdb)
        ctx.derep_resident()
        DS.assert_tables_equal(ctx.d0_cluster_device(), sets["wave_edges"][1])
        ctx.upload_hostdb(hdb)
        with pytest.raises(SwaError, match="no cluster tables in place"):
            ctx.d0_cluster_fetch()
        with pytest.raises(SwaError, match="swa_derep_resident"):
            ctx.d0_cluster_device()
    finally:
        ctx.close()


def test_a_small_cluster_array_is_a_capacity_error(sets):
    ctx = Context(0)
    try:
        ctx.upload_hostdb(HostDb(sets["wave_edges"][0]))
        ctx.derep_resident()
        want = sets["wave_edges"][1]
        ctx.d0_cluster_device()
        with pytest.raises(SwaError, match="too small") as e:
            ctx.d0_cluster_fetch(cluster_cap=want["swarms"] - 1)
        assert e.value.code == 4                                # SWA_E_CAPACITY
        DS.assert_tables_equal(dict(ctx.d0_cluster_fetch(), **{k: want[k] for k in DS.SUMMARY}), want)
    finally:
        ctx.close()


def test_the_d1_index_after_the_tables_and_the_tables_again(sets):
    ctx = Context(0)
    try:
        fa, want, _ = sets["random_short"]
        ctx.upload_hostdb(HostDb(fa))
        ctx.derep_resident()
        DS.assert_tables_equal(ctx.d0_cluster_device(), want)
        ctx.d1_index_build()
        assert ctx.d1_has_duplicates() is True                  # (as after swa_derep: tests/test_derep.py)
        ctx.derep_resident()
        DS.assert_tables_equal(ctx.d0_cluster_device(), want)
        DS.assert_tables_equal(ctx.d0_cluster_device(), want)   # (made again from the same resident array)
    finally:
        ctx.close()
