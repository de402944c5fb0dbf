"""SWARM_AMD_DN_TABLES=host|device end to end: the d >= 2 graph route with its swarm tables made on the host (five downloaded
arrays, an OpenMP loop over the swarms) or in HBM (swarm_amd/csrc/dn_tables.inc) writes the same bytes — the golden files of
the reference where they exist —, the links are downloaded once and only for a writer that reads them, and the routes the
switch does not concern (the host walk, the scan) do not notice it."""
import os
import subprocess

import pytest

import support as S
from swarm_amd import DnClusters, HostDb

pytestmark = pytest.mark.gpu
G = S.GOLDEN
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
OUTS = "osiwu"
SWITCHES = ("SWARM_AMD_DN", "SWARM_AMD_DN_WALK", "SWARM_AMD_DN_TABLES", "SWA_DN_BRUTE_CAP")


def _cli(tmp_path, name, tag, **switches):
    """one run of the command line over a golden set with all five writers; returns the files' bytes and stderr"""
    args = (G / f"{name}.args").read_text().split()
    d = args[args.index("-d") + 1]
    cmd = [str(BIN), "-d", d]
    for k in OUTS:
        cmd += [f"-{k}", str(tmp_path / f"{tag}.{k}")]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run(cmd + ["-l", "/dev/null", str(G / f"{name}.fasta")], capture_output=True, text=True, timeout=300,
                       env=dict(env, SWARM_AMD_TIMING="1", **switches))
    assert r.returncode == 0, r.stderr
    return {k: (tmp_path / f"{tag}.{k}").read_bytes() for k in OUTS}, r.stderr


@pytest.mark.parametrize("name", ["d2_small", "d3_400", "d5_ties", "d8_16bit"])
def test_both_routes_write_the_golden_files(tmp_path, name):
    host, host_log = _cli(tmp_path, name, "host", SWARM_AMD_DN_TABLES="host")
    device, device_log = _cli(tmp_path, name, "device", SWARM_AMD_DN_TABLES="device")
    for k in OUTS:
        assert device[k] == host[k], k
        if (G / f"{name}.{k}").exists():
            assert device[k] == (G / f"{name}.{k}").read_bytes(), k
    if "graph: resident" in host_log:                              # (the graph route with the device walk served the set)
        assert "swarm tables on the host" in host_log and "swarm tables on the device" not in host_log
        assert "swarm tables on the device" in device_log and "swarm tables on the host" not in device_log
    else:
        assert "swarm tables on the" not in host_log + device_log
    if name in ("d2_small", "d3_400"):                             # 60 nt, d = 2 / 120 nt, d = 3: room for d + 1 windows of 16
        assert "graph: resident" in host_log and "graph: resident" in device_log


@pytest.mark.parametrize("name", ["d2_small", "d3_400"])
def test_links_are_fetched_once_and_only_for_a_writer_that_reads_them(gpu_ctx, tmp_path, monkeypatch, name):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    args = (G / f"{name}.args").read_text().split()
    d = int(args[args.index("-d") + 1])
    hdb = HostDb(G / f"{name}.fasta", check_duplicate_sequences=True)
    gpu_ctx.upload_hostdb(hdb)
    monkeypatch.setenv("SWARM_AMD_DN_TABLES", "host")
    host = DnClusters(gpu_ctx, hdb, d)
    for k, writer in zip("osiw", (host.write_swarms, host.write_stats, host.write_structure, host.write_seeds)):
        writer(tmp_path / f"host.{k}")
    host.write_uclust(tmp_path / "host.u")
    assert host.link_fetches() == 0                               # (made on the host: nothing to fetch)
    monkeypatch.setenv("SWARM_AMD_DN_TABLES", "device")
    cl = DnClusters(gpu_ctx, hdb, d)
    assert cl.scan_totals()["route"] == "graph" and cl.summary() == host.summary()
    cl.write_swarms(tmp_path / "device.o")
    cl.write_stats(tmp_path / "device.s")
    cl.write_seeds(tmp_path / "device.w")
    assert cl.link_fetches() == 0
    cl.write_structure(tmp_path / "device.i")
    assert cl.link_fetches() == 1
    cl.write_uclust(tmp_path / "device.u")
    cl.write_uclust(tmp_path / "device.ug", ctx=gpu_ctx)
    cl.write_structure(tmp_path / "device.i2")
    assert cl.link_fetches() == 1
    for k in OUTS:
        assert (tmp_path / f"device.{k}").read_bytes() == (tmp_path / f"host.{k}").read_bytes(), k
        if (G / f"{name}.{k}").exists():
            assert (tmp_path / f"device.{k}").read_bytes() == (G / f"{name}.{k}").read_bytes(), k
    assert (tmp_path / "device.ug").read_bytes() == (tmp_path / "device.u").read_bytes()
    assert (tmp_path / "device.i2").read_bytes() == (tmp_path / "device.i").read_bytes()
    # the -u writer on the GPU as the first reader of the links: fetched at its entry, once
    first = DnClusters(gpu_ctx, hdb, d)
    first.write_swarms(tmp_path / "first.o")
    assert first.link_fetches() == 0
    first.write_uclust(tmp_path / "first.u", ctx=gpu_ctx)
    assert first.link_fetches() == 1
    assert (tmp_path / "first.u").read_bytes() == (tmp_path / "host.u").read_bytes()
    for r in (host, cl, first):
        r.close()


def test_links_left_on_a_context_that_has_moved_on_are_refused(gpu_ctx, tmp_path, monkeypatch):
    """a result whose links wait in HBM, and a second clustering on the same context before a writer asked for them: -o, -s, -w
    still come out, -i and -u fail (with a message) instead of writing the other clustering's links"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SWARM_AMD_DN_TABLES", "device")
    hdb = HostDb(G / "d3_400.fasta", check_duplicate_sequences=True)
    gpu_ctx.upload_hostdb(hdb)
    stale = DnClusters(gpu_ctx, hdb, 3)
    assert gpu_ctx.dn_tables_serial() > 0
    fresh = DnClusters(gpu_ctx, hdb, 2)
    assert stale.summary() != fresh.summary()
    stale.write_swarms(tmp_path / "o")
    stale.write_stats(tmp_path / "s")
    assert (tmp_path / "o").read_bytes() == (G / "d3_400.o").read_bytes() and (tmp_path / "s").read_bytes() == (G / "d3_400.s").read_bytes()
    with pytest.raises(AssertionError):
        stale.write_structure(tmp_path / "i")
    assert stale.link_fetches() == 0
    assert "has since been given other work" in stale.lib.swa_dn_result_error(stale.h).decode()
    fresh.write_structure(tmp_path / "i2")
    assert fresh.link_fetches() == 1
    stale.close()
    fresh.close()


@pytest.mark.parametrize("other", [{"SWARM_AMD_DN_WALK": "host"}, {"SWARM_AMD_DN": "scan"}])
def test_the_host_walk_and_the_scan_do_not_notice_the_switch(tmp_path, other):
    plain, _ = _cli(tmp_path, "d3_400", "plain", **other)
    for where in ("host", "device"):
        got, log = _cli(tmp_path, "d3_400", where, SWARM_AMD_DN_TABLES=where, **other)
        assert "swarm tables on the" not in log
        for k in OUTS:
            assert got[k] == plain[k], (where, k)
            if (G / f"d3_400.{k}").exists():
                assert got[k] == (G / f"d3_400.{k}").read_bytes(), k
