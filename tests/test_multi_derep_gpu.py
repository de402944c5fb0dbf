"""d = 0 on several GPUs (multi.hip: swa_multi_derep_resident, swa_multi_derep; derep.hip: k_derep_hash_slice, k_derep_route,
the owners' rounds): several ranks on one device, and one rank over RCCL, against the oracle's dereplication, the closed
form of the cluster tables and the host route's files on every read set of tests/derep_sets.py; the owners' shares against
swa_multi_derep_owner_for on the hashes a single context reports; the re-key rounds at the owners; what the call ends on
every rank; and the command line under SWARM_AMD_DEVICES."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import derep_sets as DS
import multi_derep_sets as MD
import support as S
from swarm_amd import D0Clusters, HostDb, MultiContext, SwaError
from swarm_amd.capi import derep_owner_for

pytestmark = pytest.mark.gpu
G = S.GOLDEN
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
# (device list, SWARM_AMD_FORCE_RCCL): ranks that share a device exchange by device-to-device copies; one rank under the
# variable runs the same path through ncclSend / ncclRecv
LISTS = {"two": ([0, 0], False), "three": ([0, 0, 0], False), "eight": ([0] * 8, False), "one_rccl": ([0], True)}


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """name -> (fasta path, db, first_identical by the oracle, expected tables): made once, shared, left unchanged"""
    made = MD.make_sets(tmp_path_factory.mktemp("multi_derep_sets"))
    return {name: (fa, db, first, DS.expected_tables(first, db.abundance)) for name, (fa, db, first, _) in made.items()}


@pytest.fixture(scope="module")
def multis():
    """key of LISTS -> its MultiContext, created when first asked for and kept for the module"""
    made = {}

    def get(key):
        if key not in made:
            devices, rccl = LISTS[key]
            before = os.environ.get("SWARM_AMD_FORCE_RCCL")
            if rccl:
                os.environ["SWARM_AMD_FORCE_RCCL"] = "1"
            else:
                os.environ.pop("SWARM_AMD_FORCE_RCCL", None)
            try:
                made[key] = MultiContext(devices)
            finally:
                os.environ.pop("SWARM_AMD_FORCE_RCCL", None)
                if before is not None:
                    os.environ["SWARM_AMD_FORCE_RCCL"] = before
            assert made[key].uses_rccl() is rccl
        return made[key]

    yield get
    for m in made.values():
        m.close()


def _write_all(cl, d, tag):
    cl.write_swarms(d / f"{tag}.o")
    cl.write_seeds(d / f"{tag}.w")
    cl.write_stats(d / f"{tag}.s")
    cl.write_structure(d / f"{tag}.i")
    cl.write_uclust(d / f"{tag}.u")
    return ("o", "w", "s", "i", "u")


@pytest.mark.parametrize("name", MD.NAMES)
@pytest.mark.parametrize("key", list(LISTS))
def test_derep_is_the_oracles(multis, sets, key, name):
    fa, db, first, _ = sets[name]
    m = multis(key)
    m.upload_hostdb(HostDb(fa))
    got = m.derep()
    assert got.dtype == first.dtype and np.array_equal(got, first)
    t = m.derep_totals()
    assert int(t["received"].sum()) == db.n and t["routed"] == db.n and t["rounds"] >= 1


@pytest.mark.parametrize("name", MD.NAMES)
@pytest.mark.parametrize("key", list(LISTS))
def test_resident_tables_and_files(multis, sets, tmp_path, key, name):
    fa, db, first, want = sets[name]
    m = multis(key)
    hdb = HostDb(fa)
    m.upload_hostdb(hdb)
    m.derep_resident()
    DS.assert_tables_equal(m.ctx(0).d0_cluster_device(), want, name)
    dev = D0Clusters.from_device(m.ctx(0), hdb)
    DS.assert_tables_equal(dev.tables(), want, name)
    kinds = _write_all(dev, tmp_path, "dev")
    _write_all(D0Clusters(hdb, first), tmp_path, "host")
    for k in kinds:
        assert filecmp.cmp(tmp_path / f"dev.{k}", tmp_path / f"host.{k}", shallow=False), k


# ---- shares -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["wave_edges", "random_long", "random_short", "all_different_257", "golden"])
@pytest.mark.parametrize("key", ["two", "three", "eight"])
def test_shares_are_the_owner_functions(gpu_ctx, multis, sets, key, name):
    """what every owner received = the reads whose hash — as a single context computes it — the owner function gives it"""
    fa, db, _, _ = sets[name]
    hdb = HostDb(fa)
    gpu_ctx.upload_hostdb(hdb)
    gpu_ctx.d1_index_build()                                 # (reports the duplicates; the hashes are made either way)
    hashes = gpu_ctx.d1_debug(0, db.n)
    m = multis(key)
    world = len(LISTS[key][0])
    m.upload_hostdb(hdb)
    m.derep_resident()
    received = m.derep_totals()["received"]
    want = np.bincount([derep_owner_for(int(h), world) for h in hashes], minlength=world)
    assert int(received.sum()) == db.n
    assert np.array_equal(received, want.astype(np.uint64)), (received, want)


def test_one_sequence_goes_to_one_owner(multis, sets):
    """5000 copies of one sequence at 8 ranks: one inbox of 5000 records, seven empty ones"""
    fa, db, first, want = sets["one_sequence_5000"]
    m = multis("eight")
    m.upload_hostdb(HostDb(fa))
    assert np.array_equal(m.derep(), first)
    assert sorted(int(x) for x in m.derep_totals()["received"]) == [0] * 7 + [5000]
    DS.assert_tables_equal(m.ctx(0).d0_cluster_device(), want)


@pytest.mark.parametrize("name", ["one_read", "two_different"])
def test_empty_slices(multis, sets, name):
    """fewer reads than ranks: most slices are empty, and so are most inboxes"""
    fa, db, first, want = sets[name]
    m = multis("eight")
    m.upload_hostdb(HostDb(fa))
    assert np.array_equal(m.derep(), first)
    received = m.derep_totals()["received"]
    assert int(received.sum()) == db.n and int((received == 0).sum()) >= 8 - db.n
    DS.assert_tables_equal(m.ctx(0).d0_cluster_device(), want)


# ---- the re-key rounds at the owners --------------------------------------------------------------------------------------

def test_rekey_rounds_at_the_owners(sets, tmp_path):
    """SWA_DEREP_KEY_BITS=4: different sequences share table slots at their owner, which goes round again with longer keys;
    the owner of a read does not move with the round (own process: the hook is read from the environment)"""
    names = ["random_long", "random_short"]
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {str(S.ROOT)!r})\n"
        "from swarm_amd import HostDb, MultiContext\n"
        "m = MultiContext([0, 0, 0])\n"
        f"for name, fa in {[(n, str(sets[n][0])) for n in names]!r}:\n"
        "    hdb = HostDb(fa); m.upload_hostdb(hdb); first = m.derep(); t = m.derep_totals()\n"
        "    m.derep_resident()\n"
        f"    np.savez({str(tmp_path)!r} + '/' + name + '.npz', first=first, rounds=t['rounds'], received=t['received'], **m.ctx(0).d0_cluster_device())\n"
        "m.close()\n"
        "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True,
                       env=dict(os.environ, SWA_DEREP_KEY_BITS="4"), timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    for name in names:
        got = dict(np.load(tmp_path / f"{name}.npz"))
        assert np.array_equal(got.pop("first"), sets[name][2]), name
        assert int(got.pop("rounds")) > 1, name
        assert int(got.pop("received").sum()) == sets[name][1].n
        DS.assert_tables_equal(got, sets[name][3], name)


# ---- what the call ends, and what may follow it ------------------------------------------------------------------------------

def test_only_rank_0_holds_the_resident_array(multis, sets):
    fa, _, _, want = sets["wave_edges"]
    m = multis("three")
    m.upload_hostdb(HostDb(fa))
    m.derep_resident()
    for rank in (1, 2):
        with pytest.raises(SwaError, match="swa_derep_resident"):
            m.ctx(rank).d0_cluster_device()
    DS.assert_tables_equal(m.ctx(0).d0_cluster_device(), want)
    m.derep_resident()                                       # (a second call: the same tables)
    DS.assert_tables_equal(m.ctx(0).d0_cluster_device(), want)


def test_a_single_context_call_on_a_rank_ends_with_the_next_multi_call(multis, sets):
    """rank 1 dereplicates on its own (it may: it holds the database), then the ranks do: rank 1's array ends there"""
    fa, _, _, want = sets["mass_ties"]
    m = multis("two")
    m.upload_hostdb(HostDb(fa))
    m.ctx(1).derep_resident()
    DS.assert_tables_equal(m.ctx(1).d0_cluster_device(), want)
    m.derep_resident()
    with pytest.raises(SwaError, match="swa_derep_resident"):
        m.ctx(1).d0_cluster_device()
    DS.assert_tables_equal(m.ctx(0).d0_cluster_device(), want)


def test_the_d1_network_after_the_dereplication_and_back(multis, gpu_ctx, sets, tmp_path):
    """a duplicate-free set: d = 1 on the ranks after d = 0 on them (no rank takes its partly filled hash array for the
    database's), and d = 0 again after that"""
    fa = tmp_path / "unique.fa"
    S.gen_fasta(fa, 3000, 150, 31)
    hdb = HostDb(fa)
    db = S.db_from_fasta(fa)
    gpu_ctx.upload_hostdb(hdb)
    assert gpu_ctx.d1_index_build() is False
    woff, wnb = gpu_ctx.d1_network()
    for key in ("two", "three"):
        m = multis(key)
        m.upload_hostdb(hdb)
        identity = np.arange(db.n, dtype=np.uint32)
        assert np.array_equal(m.derep(), identity)
        off, nb = m.d1_network()
        assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
        m.derep_resident()
        DS.assert_tables_equal(m.ctx(0).d0_cluster_device(), DS.expected_tables(identity, db.abundance))
        off, nb = m.d1_network()
        assert np.array_equal(off, woff) and np.array_equal(nb, wnb)


# ---- the command line -----------------------------------------------------------------------------------------------------

CLI_SETS = ("wave_edges", "random_long", "random_short")
CLI_ARGS = ["-d", "0", "-o", "o", "-s", "s", "-w", "w", "-i", "i", "-u", "u", "-l", "l"]
SUMMARY_LINES = ("Number of swarms:", "Largest swarm:", "Heaviest swarm:")


def _run(d, fa, devices=None, route=None, report=False, args=CLI_ARGS):
    d.mkdir()
    env = dict(os.environ)
    for k in ("SWARM_AMD_DEVICES", "SWARM_AMD_D0", "SWARM_AMD_MULTI_REPORT"):
        env.pop(k, None)
    if devices is not None:
        env["SWARM_AMD_DEVICES"] = devices
    if route is not None:
        env["SWARM_AMD_D0"] = route
    if report:
        env["SWARM_AMD_MULTI_REPORT"] = "1"
    r = subprocess.run([str(BIN)] + list(args) + [str(fa)], cwd=d, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r


@pytest.fixture(scope="module")
def cli_single(sets, tmp_path_factory):
    """name -> the directory of the run without SWARM_AMD_DEVICES, default route"""
    root = tmp_path_factory.mktemp("cli_single")
    out = {}
    for name in CLI_SETS:
        out[name] = root / name
        _run(out[name], sets[name][0])
    return out


@pytest.mark.parametrize("route", [None, "host"])
@pytest.mark.parametrize("devices", [None, "0,0", "0,0,0"])
@pytest.mark.parametrize("name", CLI_SETS)
def test_command_line_on_several_ranks(sets, cli_single, tmp_path, name, devices, route):
    """`swarm -d 0 -o -s -w -i -u -l`: with and without SWARM_AMD_DEVICES, on either route, the files and the log are those
    of the single-GPU run; SWARM_AMD_MULTI_REPORT=1 names the ranks on stderr"""
    fa, _, _, want = sets[name]
    r = _run(tmp_path / "run", fa, devices, route, report=True)
    for k in "oswiul":
        assert filecmp.cmp(cli_single[name] / k, tmp_path / "run" / k, shallow=False), (name, devices, route, k)
    log = (tmp_path / "run" / "l").read_text()
    assert f"Number of swarms:  {want['swarms']}\nLargest swarm:     {want['largest']}\nHeaviest swarm:    {want['heaviest']}\n" in log
    single = (cli_single[name] / "l").read_text()
    for prefix in SUMMARY_LINES:
        assert [x for x in log.splitlines() if x.startswith(prefix)] == [x for x in single.splitlines() if x.startswith(prefix)]
    if devices is None:
        assert "multi:" not in r.stderr
    else:
        ranks = devices.count(",") + 1
        assert f"multi: {ranks} ranks, exchange = device-to-device copies" in r.stderr, r.stderr


@pytest.mark.parametrize("tiny", ["tiny_empty", "tiny_one"])
def test_command_line_tiny_inputs(tmp_path, tiny):
    """no read, and one read for two ranks: as without the variable"""
    fa = G / f"{tiny}.fasta"
    args = ["-d", "0", "-o", "o", "-s", "s", "-i", "i", "-l", "l"]
    a = _run(tmp_path / "single", fa, args=args)
    b = _run(tmp_path / "multi", fa, "0,0", args=args)
    for k in "osil":
        assert filecmp.cmp(tmp_path / "single" / k, tmp_path / "multi" / k, shallow=False), k
    assert a.stdout == b.stdout
    for k in [k for k in "osi" if (G / f"{tiny}_d0.{k}").exists()]:
        assert filecmp.cmp(tmp_path / "multi" / k, G / f"{tiny}_d0.{k}", shallow=False), k


@pytest.mark.parametrize("name", ["d0_derep", "d0_mothur"])
def test_command_line_reproduces_the_golden_files(tmp_path, name):
    flag = {"o": "-o", "s": "-s", "i": "-i", "w": "-w", "u": "-u"}
    kept = [k for k in flag if (G / f"{name}.{k}").exists()]   # (as tests/test_cli_gpu.py takes the fixtures)
    args = (G / f"{name}.args").read_text().split()
    for k in kept:
        args += [flag[k], k]
    _run(tmp_path / "run", G / "d0_derep.fasta", "0,0", args=args + ["-l", "l"])
    for k in kept:
        assert filecmp.cmp(tmp_path / "run" / k, G / f"{name}.{k}", shallow=False), k
    log = (tmp_path / "run" / "l").read_text()
    for line in (G / f"{name}.log").read_text().splitlines():
        assert line in log, line
