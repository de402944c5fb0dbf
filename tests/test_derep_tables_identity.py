"""d = 0 cluster tables on the CPU: the closed form of tests/derep_sets.py against a brute-force grouping, against the
host route (swa_d0_cluster through D0Clusters.tables()) and — where the compiled reference is present — the host route's
files against the reference's own, so that the closed form the GPU tests compare with is tied to src/derep.cc itself."""
import filecmp

import numpy as np
import pytest

import derep_sets as DS
import support as S
from swarm_amd import D0Clusters, HostDb

G = S.GOLDEN
NAMES = sorted(DS.SETS) + ["golden"]


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """name -> (fasta path, first_identical by the oracle, abundance in db order): made once, shared, left unchanged"""
    root = tmp_path_factory.mktemp("derep_sets")
    out = {}
    for name in NAMES:
        fa = G / "d0_derep.fasta" if name == "golden" else root / f"{name}.fa"
        if name != "golden":
            DS.SETS[name](fa)
        db = S.db_from_fasta(fa)
        out[name] = (fa, S.oracle_derep(db), db.abundance.copy())
    return out


def _brute_force(first, abundance) -> dict:
    groups = {}
    for i, f in enumerate(first.tolist()):
        groups.setdefault(f, []).append(i)                     # (ascending i: db order inside a cluster)
    begin, at = {}, 0
    for f in sorted(groups):                                   # members[] grouped in seed order
        begin[f] = at
        at += len(groups[f])
    mass = {f: sum(int(abundance[i]) for i in m) for f, m in groups.items()}
    order = sorted(groups, key=lambda f: (-mass[f], f))
    return {"seed": np.array(order, dtype=np.uint32), "mass": np.array([mass[f] for f in order], dtype=np.uint64),
            "size": np.array([len(groups[f]) for f in order], dtype=np.uint32),
            "singletons": np.array([sum(1 for i in groups[f] if int(abundance[i]) == 1) for f in order], dtype=np.uint32),
            "begin": np.array([begin[f] for f in order], dtype=np.uint32),
            "members": np.array([i for f in sorted(groups) for i in groups[f]], dtype=np.uint32),
            "swarms": len(groups), "largest": max(len(m) for m in groups.values()), "heaviest": max(mass.values())}


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_is_the_brute_force_grouping(sets, name):
    _, first, abundance = sets[name]
    DS.assert_tables_equal(DS.expected_tables(first, abundance), _brute_force(first, abundance), name)


def test_the_sets_have_the_shapes_they_are_meant_to(sets):
    t = {name: DS.expected_tables(first, abundance) for name, (_, first, abundance) in sets.items()}
    assert t["all_different_257"]["swarms"] == 257 and t["all_different_257"]["largest"] == 1
    assert np.array_equal(t["all_different_257"]["seed"], np.arange(257))           # every mass ties: purely by seed
    for c in DS.COPIES:
        assert t[f"one_sequence_{c}"]["swarms"] == 1 and t[f"one_sequence_{c}"]["largest"] == c
    assert sorted(t["wave_edges"]["size"].tolist()) == sorted([1, 63, 1, 64, 1, 65, 127, 129, 255, 257, 1])
    assert (t["wave_edges"]["singletons"] != t["wave_edges"]["size"]).any()
    ties = t["mass_ties"]
    assert ties["mass"].tolist() == [20, 20, 20, 6, 6, 6, 4, 1]
    assert ties["size"].tolist() == [6, 3, 2, 1, 3, 6, 1, 1]                        # by seed, not by size, either way
    assert (np.diff(ties["seed"][:3].astype(np.int64)) > 0).all() and (np.diff(ties["seed"][3:6].astype(np.int64)) > 0).all()
    # the reader takes abundances beyond 32 bits as they are: the masses asked for are there
    assert set(DS.BIG_MASSES) <= set(t["big_masses"]["mass"].tolist())
    assert t["big_masses"]["heaviest"] == 6 * 10**9


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_is_the_host_route(sets, name):
    fa, first, abundance = sets[name]
    hdb = HostDb(fa)
    assert np.array_equal(hdb.abundance, abundance)
    DS.assert_tables_equal(D0Clusters(hdb, first).tables(), DS.expected_tables(first, abundance), name)


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("name", ["wave_edges", "mass_ties", "big_masses"])
def test_host_route_files_are_the_references(sets, tmp_path, name):
    fa, first, _ = sets[name]
    r = S.run_ref_swarm(["-d", 0, "-o", tmp_path / "ro", "-s", tmp_path / "rs", "-w", tmp_path / "rw", "-l", "/dev/null", fa])
    assert r.returncode == 0, r.stderr
    cl = D0Clusters(HostDb(fa), first)
    cl.write_swarms(tmp_path / "go")
    cl.write_stats(tmp_path / "gs")
    cl.write_seeds(tmp_path / "gw")
    for k in "osw":
        assert filecmp.cmp(tmp_path / f"r{k}", tmp_path / f"g{k}", shallow=False), k
