"""The several-rank drivers (swarm_amd/csrc/multi.hip) where the uniform sets of test_multi_gpu.py never take them: worlds of
5 and 8 ranks, sets whose window keys everybody shares (the routed build overflows and the ranks stream), sets with fewer
anchor groups, links or heavy amplicons than ranks (empty shares in the gather, the CSR assembly and the merge), databases
smaller than the world, link lists that regrow — and the merge kernel on its own.  Every rank is on device 0 (the exchange
then uses device-to-device copies).  Expected values come from the oracle (d = 1, fastidious), from alignments of all pairs
by the oracle's nw() (d >= 2) and from numpy's stable sort (the merge); tests/test_multi_sets_identity.py proves on the CPU
what is assumed of the sets.  What happens on rank 0 after the exchange is compared with a single context's."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import multi_sets as MS
import support as S
from swarm_amd import Context, D1Clusters, HostDb, MultiContext, SwaError, capi

pytestmark = pytest.mark.gpu
BIN = S.ROOT / "swarm_amd" / "bin" / "swarm"
G = S.GOLDEN
WORLDS = MS.WORLDS
ROUTED, STREAMED, OVERFLOWED = capi.MULTI_BUILD_NAMES[1:]
FIVE = ("swarm id", "generation", "parent", "order", "bounds")


@pytest.fixture(scope="module")
def multis():
    """one MultiContext per world, made when first asked for and reused by every test (making one costs more than these
    sets do)"""
    made = {}

    def get(world):
        if world not in made:
            made[world] = MultiContext([0] * world)
            assert made[world].uses_rccl() is False
        return made[world]
    yield get
    for m in made.values():
        m.close()


@pytest.fixture(scope="module")
def single():
    ctx = Context(0)
    yield ctx
    ctx.close()


D1_SETS = ("shared_flanks", "few_groups", "tiny1", "tiny2", "tiny3", "tiny7", "mixed_lengths", "giant", "uniform", "few_heavy", "light")


@pytest.fixture(scope="module")
def d1_sets(tmp_path_factory, single):
    """name -> the set, the oracle's networks and what one context makes of it; computed once, never changed"""
    root = tmp_path_factory.mktemp("multi_edges")
    memo = {}

    def get(name):
        if name in memo:
            return memo[name]
        fa = root / f"{name}.fa"
        if name.startswith("tiny"):
            db, fa = MS.tiny(fa, int(name[4:]))
        elif name == "uniform":
            S.gen_fasta(fa, 6000, 150, 61)
            db = S.db_from_fasta(fa)
        elif name == "light":
            S.gen_fasta(fa, 3000, 150, 62, 1, 0.3)
            db = S.db_from_fasta(fa)
        else:
            db, fa = getattr(MS, name)(fa)
        hdb = HostDb(fa)
        assert hdb.n == db.n and all(hdb.header(i) == db.headers[i] for i in (0, db.n // 2, db.n - 1))
        assert np.array_equal(np.asarray(hdb.seqlen), db.seqlen) and np.array_equal(np.asarray(hdb.abundance), db.abundance)
        case = {"name": name, "db": db, "fa": fa, "hdb": hdb}
        single.upload_hostdb(hdb)
        for ncb in (True, False):
            case["net", ncb] = MS.oracle_network(db, ncb)
            assert single.d1_index_build() is False
            total = single.d1_network_resident(ncb)
            got = single.d1_network_fetch(total)
            _same(got, case["net", ncb], ("offsets", "neighbours"))        # (the single context itself, against the oracle)
            case["cluster", ncb] = single.d1_cluster_device()
            for a in case["cluster", ncb]:
                a.setflags(write=False)
        memo[name] = case
        return case
    return get


def _same(got, want, names):
    for a, b, name in zip(got, want, names):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name


def _expected_build(case, world, build):
    """what swa_multi_d1_last_build must say, where it follows from the sizes: a slice no longer than a region cannot
    overflow it; in shared_flanks every record of a slice goes to one region"""
    n = case["db"].n
    if build == "streamed":
        return STREAMED
    if MS.longest_slice(n, world) <= MS.route_region(n, world):
        return ROUTED
    return OVERFLOWED if case["name"] == "shared_flanks" else None


# ---- 1. the d = 1 network ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["default", "streamed"])
@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", D1_SETS[:9])
def test_d1_network_equals_the_oracle(multis, d1_sets, monkeypatch, name, world, build):
    """swa_multi_d1_network for both settings of cluster breaking against the oracle, row by row; the resident entry's
    network against the oracle too, and the clustering of it on rank 0 against a single context's"""
    case = d1_sets(name)
    if build == "streamed":
        monkeypatch.setenv("SWARM_AMD_MULTI_BUILD", "streamed")
    else:
        monkeypatch.delenv("SWARM_AMD_MULTI_BUILD", raising=False)
    m = multis(world)
    m.upload_hostdb(case["hdb"])
    want_build = _expected_build(case, world, build)
    for ncb in (False, True):
        _same(m.d1_network(ncb), case["net", ncb], ("offsets", "neighbours"))
        print(f"last_build {name} world {world} {build}: {m.last_build()}")
        assert want_build is None or m.last_build() == want_build
    if name == "shared_flanks" and build == "default" and world in (2, 3):
        assert m.last_build() == OVERFLOWED
    if name == "uniform" and build == "default":
        assert m.last_build() == ROUTED
    c0 = m.ctx(0)
    for ncb in (True, False):
        total = m.d1_network_resident(ncb)
        assert total == len(case["net", ncb][1])
        assert want_build is None or m.last_build() == want_build
        _same(c0.d1_network_fetch(total), case["net", ncb], ("offsets", "neighbours"))
        _same(c0.d1_cluster_device(), case["cluster", ncb], FIVE)


@pytest.mark.parametrize("world", [2, 3])
def test_an_overflowed_attempt_leaves_nothing_behind(multis, d1_sets, monkeypatch, world):
    """shared_flanks twice on one MultiContext (both attempts overflow), then the uniform set (routed), then shared_flanks
    again: region buffers, counts and ownership of an abandoned attempt must not reach the next call"""
    monkeypatch.delenv("SWARM_AMD_MULTI_BUILD", raising=False)
    flanks, uniform = d1_sets("shared_flanks"), d1_sets("uniform")
    m = multis(world)
    m.upload_hostdb(flanks["hdb"])
    for ncb in (False, True):                                    # (the second call finds what the first attempt left)
        _same(m.d1_network(ncb), flanks["net", ncb], ("offsets", "neighbours"))
        assert m.last_build() == OVERFLOWED
    for case, want in ((uniform, ROUTED), (flanks, OVERFLOWED), (uniform, ROUTED)):
        m.upload_hostdb(case["hdb"])
        for ncb in (False, True):
            _same(m.d1_network(ncb), case["net", ncb], ("offsets", "neighbours"))
            assert m.last_build() == want
        total = m.d1_network_resident(False)
        _same(m.ctx(0).d1_network_fetch(total), case["net", False], ("offsets", "neighbours"))
        assert m.last_build() == want


def test_some_rank_of_eight_owns_nothing_of_few_groups(multis, d1_sets, monkeypatch):
    """the ranks' shares one by one (a context under ownership returns partial rows): they add up to the oracle's network,
    no link twice, and at least one of the eight is empty — so the calls above ran a zero-length chunk in the middle of
    the gather and of the CSR assembly"""
    monkeypatch.delenv("SWARM_AMD_MULTI_BUILD", raising=False)
    case = d1_sets("few_groups")
    m = multis(8)
    m.upload_hostdb(case["hdb"])
    want_off, want_nb = case["net", False]
    shares = []
    for r in range(8):
        c = m.ctx(r)
        c.d1_set_ownership(r, 8)
        assert c.d1_index_build() is False
        off, nb = c.d1_network(False)
        rows = np.repeat(np.arange(case["db"].n, dtype=np.uint64), np.diff(off).astype(np.int64))
        shares.append((rows << np.uint64(32)) | nb.astype(np.uint64))
    sizes = [len(s) for s in shares]
    print(f"few_groups, links per rank of 8: {sizes}")
    assert 0 in sizes and sum(sizes) == len(want_nb) > 0
    every = np.sort(np.concatenate(shares))
    rows = np.repeat(np.arange(case["db"].n, dtype=np.uint64), np.diff(want_off).astype(np.int64))
    assert np.array_equal(every, np.sort((rows << np.uint64(32)) | want_nb.astype(np.uint64)))
    # ... and the driver on the same contexts, after they were used one by one
    _same(m.d1_network(False), case["net", False], ("offsets", "neighbours"))


def test_no_database_is_an_argument_error(multis, d1_sets):
    m = multis(2)
    case = d1_sets("tiny3")
    m.upload_hostdb(case["hdb"])
    empty = HostDb(G / "tiny_empty.fasta")
    assert empty.n == 0
    with pytest.raises(SwaError) as e:                           # (refused: the database before it stays)
        m.upload_hostdb(empty)
    assert e.value.code == capi.SWA_E_ARG
    _same(m.d1_network(False), case["net", False], ("offsets", "neighbours"))
    fresh = MultiContext([0, 0])
    try:
        for call in (fresh.d1_network, fresh.d1_network_resident):
            with pytest.raises(SwaError) as e:
                call(False)
            assert e.value.code == capi.SWA_E_ARG and "no database" in str(e.value)
            assert fresh.last_build() == "none"
    finally:
        fresh.close()


# ---- 2. link lists that regrow -------------------------------------------------------------------------------------------------
def test_link_lists_regrow(tmp_path):
    """the dense set without cluster breaking has 21 n links (the oracle's count; test_multi_sets_identity), more than two
    first buffers of 4 n / 2 + 65536 hold together: whichever way the two ranks divide them, one list regrows.  A new
    MultiContext, so that the buffers are the first ones."""
    db, fa = MS.shared_flanks_dense(tmp_path / "in.fa")
    want_off, want_nb = MS.oracle_network(db, True)
    assert len(want_nb) == 21 * db.n > 2 * MS.link_cap(db.n, 2)
    hdb = HostDb(fa)
    m = MultiContext([0, 0])
    try:
        m.upload_hostdb(hdb)
        off, nb = m.d1_network(True)
        assert len(nb) == len(want_nb)
        _same((off, nb), (want_off, want_nb), ("offsets", "neighbours"))
        print(f"last_build dense world 2: {m.last_build()}")
        # ... and with the buffers grown
        _same(m.d1_network(False), MS.oracle_network(db, False), ("offsets", "neighbours"))
    finally:
        m.close()


# ---- 3. the fastidious pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [5, 8])
@pytest.mark.parametrize("name", ["few_groups", "few_heavy", "light"])
def test_fastidious_pass_equals_the_oracle(multis, d1_sets, monkeypatch, name, world):
    """both entries — flags from the host, flags in rank 0's HBM — against the oracle's pass over the same flags; the flags
    themselves (host clustering of the oracle's network) against those rank 0 makes"""
    monkeypatch.delenv("SWARM_AMD_MULTI_BUILD", raising=False)
    case = d1_sets(name)
    db = case["db"]
    off, nb = case["net", False]
    cl = D1Clusters(case["hdb"], off, nb)
    flags, stats = cl.light_flags(3)
    cl.close()
    want_graft, want_counters = S.oracle_fastidious(db, flags, 16)
    heavy = int((flags == 0).sum())
    print(f"{name}: {db.n} amplicons, {heavy} heavy, {int((want_graft != capi.NO_AMPLICON).sum())} graft candidates")
    if name == "few_heavy":
        assert 0 < heavy < world and (want_graft != capi.NO_AMPLICON).sum() == 15
    if name == "light":
        assert (want_graft != capi.NO_AMPLICON).sum() > 10
    m = multis(world)
    m.upload_hostdb(case["hdb"])
    _same(m.d1_network(False), case["net", False], ("offsets", "neighbours"))
    graft, counters = m.d1_fastidious(flags, stats[2], 16)
    assert np.array_equal(graft, want_graft)
    assert [int(x) for x in counters[:5]] == [int(x) for x in want_counters[:5]]
    c0 = m.ctx(0)
    for fetch in (True, False):
        m.d1_network_resident(False)
        _same(c0.d1_cluster_device(), case["cluster", False], FIVE)
        got_flags, got_stats = c0.d1_light_flags_device(3)
        assert np.array_equal(got_flags, flags) and got_stats[2] == stats[2]
        cand, counters = m.d1_fastidious_resident(got_stats[2], 16, fetch=fetch)
        assert [int(x) for x in counters[:5]] == [int(x) for x in want_counters[:5]]
        if fetch:
            assert np.array_equal(cand, want_graft)
        else:
            assert cand is None


# ---- 4. d >= 2 -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dn_sets(tmp_path_factory, single):
    root = tmp_path_factory.mktemp("multi_edges_dn")
    memo = {}
    mm, go, ge = 18, 24, 13

    def everything(c, total):
        out = list(c.d1_network_fetch(total)) + [c.d1_network_fetch_diffs(total)]
        out += list(c.d1_cluster_device()) + [c.dn_parent_diffs()]
        sizes = c.dn_tables_device()
        tables = c.dn_tables_fetch()
        return out + [np.array(sizes, dtype=np.uint64)] + [tables[k] for k in sorted(tables)]

    def get(d, variant):
        if (d, variant) not in memo:
            db, fa = MS.dn_sparse(root / f"d{d}_{variant}.fa", d, variant)
            hdb = HostDb(fa)
            assert hdb.n == db.n and all(hdb.header(i) == db.headers[i] for i in (0, db.n // 2, db.n - 1))
            case = {"db": db, "hdb": hdb, "everything": everything}
            single.upload_hostdb(hdb)
            single.qgram_build()
            single.search_begin(mm, go, ge, d)
            assert single.dn_graph_supported()
            for ncb in (False, True):
                case["graph", ncb] = MS.brute_force_graph(db, d, ncb)
                case["single", ncb] = everything(single, single.dn_graph_resident(ncb))
                _same(case["single", ncb][:3], case["graph", ncb], ("offsets", "neighbours", "diffs"))
            memo[d, variant] = case
        return memo[d, variant]
    return get


def _strictly_ascending_rows(off, nb):
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))
    return bool(((rows[1:] > rows[:-1]) | (nb[1:] > nb[:-1])).all())


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("variant", MS.DN_VARIANTS)
@pytest.mark.parametrize("d", MS.DN_DS)
def test_dn_graph_equals_alignments_of_all_pairs(multis, dn_sets, d, variant, world):
    """fewer links than ranks (none at all in no_pair): some ranks send nothing.  The downloaded graph against the brute
    force, no pair from two ranks; the resident one and everything made of it on rank 0 against a single context's"""
    case = dn_sets(d, variant)
    m = multis(world)
    m.upload_hostdb(case["hdb"])
    for ncb in (False, True, False):
        want = case["graph", ncb]
        got = m.dn_graph(d, ncb)
        assert got is not None
        assert _strictly_ascending_rows(got[0], got[1])
        _same(got, want, ("offsets", "neighbours", "diffs"))
        assert len(want[1]) < 8
        if variant == "no_pair":
            assert not got[0].any() and len(got[1]) == 0
    for ncb in (True, False):
        total = m.dn_graph_resident(d, ncb)
        assert total == len(case["graph", ncb][1])
        got = case["everything"](m.ctx(0), total)
        _same(got[:3], case["graph", ncb], ("offsets", "neighbours", "diffs"))
        _same(got, case["single", ncb], [f"array {k}" for k in range(len(got))])


@pytest.mark.parametrize("world", WORLDS)
def test_a_graph_with_links_after_one_without(multis, dn_sets, world):
    m = multis(world)
    for variant in ("no_pair", "sparse", "no_pair", "with_short"):
        case = dn_sets(3, variant)
        m.upload_hostdb(case["hdb"])
        for resident in (False, True):
            if resident:
                total = m.dn_graph_resident(3, True)
                got = list(m.ctx(0).d1_network_fetch(total)) + [m.ctx(0).d1_network_fetch_diffs(total)]
            else:
                got = m.dn_graph(3, True)
            _same(got, case["graph", True], ("offsets", "neighbours", "diffs"))
            assert (len(got[1]) == 0) == (variant == "no_pair")


# ---- 5. the merge kernel -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", MS.MERGE_WORLDS)
def test_merge_kernel_equals_the_stable_sort(single, world):
    ran = 0
    for name, w, lists in MS.merge_cases():
        if w != world:
            continue
        keys, vals, at = MS.merge_flat(lists)
        want_keys, want_vals = MS.merge_reference(lists)
        got_keys, got_vals = single.merge_sorted_lists(keys, vals, at)
        assert np.array_equal(got_keys, want_keys), name
        assert np.array_equal(got_vals, want_vals), name
        ran += 1
    assert ran >= 14


def test_merge_kernel_keeps_equal_keys_in_list_order(single):
    """the same three keys in every one of eight lists, values that name list and place: upper bound below, lower bound above"""
    lists = [(np.array([5, 5, 9, 1 << 40], dtype=np.uint64), np.arange(4, dtype=np.uint32) + np.uint32(100 * r)) for r in range(8)]
    keys, vals, at = MS.merge_flat(lists)
    got_keys, got_vals = single.merge_sorted_lists(keys, vals, at)
    assert got_keys.tolist() == [5] * 16 + [9] * 8 + [1 << 40] * 8
    assert got_vals.tolist() == [100 * r + i for r in range(8) for i in (0, 1)] + [100 * r + 2 for r in range(8)] + [100 * r + 3 for r in range(8)]
    _same((got_keys, got_vals), MS.merge_reference(lists), ("keys", "values"))


@pytest.mark.parametrize("world", MS.MERGE_WORLDS)
def test_merge_of_nothing_touches_nothing(single, world):
    at = np.zeros(world + 1, dtype=np.uint64)
    out_keys, out_vals = np.full(4, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.full(4, 0x5A5A5A5A, dtype=np.uint32)
    got = single.merge_sorted_lists(np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32), at, out_keys=out_keys, out_vals=out_vals)
    assert got[0] is out_keys and (out_keys == 0xA5A5A5A5A5A5A5A5).all() and (out_vals == 0x5A5A5A5A).all()
    # ... nor does the C entry look at the arrays (null pointers)
    assert single.lib.swa_merge_sorted_lists(single.h, None, None, at.ctypes.data, world, None, None) == capi.SWA_OK


def test_merge_rejects_a_world_outside_1_to_64(single):
    at = np.zeros(70, dtype=np.uint64)
    for world in (0, 65):
        with pytest.raises(SwaError) as e:
            single.merge_sorted_lists(np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32), at, world=world)
        assert e.value.code == capi.SWA_E_ARG
    at[:3] = (0, 2, 1)                                            # a list that ends before it begins
    with pytest.raises(SwaError) as e:
        single.merge_sorted_lists(np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.uint32), at, world=2)
    assert e.value.code == capi.SWA_E_ARG


# ---- 6. the command line -------------------------------------------------------------------------------------------------------
FLAG = {"o": "-o", "s": "-s", "i": "-i", "j": "-j", "w": "-w", "u": "-u"}


def _cli(cwd, fa, env_extra):
    cwd.mkdir()
    env = dict(os.environ, **env_extra)
    for name in ("SWARM_AMD_DEVICES", "SWARM_AMD_MULTI_CLUSTER", "SWARM_AMD_MULTI_BUILD"):
        if name not in env_extra:
            env.pop(name, None)
    cmd = [str(BIN), "-d", "1", "-f"]
    for k in FLAG:
        cmd += [FLAG[k], f"out.{k}"]
    r = subprocess.run(cmd + ["-l", "out.l", str(fa)], capture_output=True, text=True, env=env, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r


@pytest.mark.parametrize("name", ["shared_flanks", "few_groups"])
def test_cli_with_three_and_eight_ranks_is_byte_identical(d1_sets, tmp_path, name):
    fa = d1_sets(name)["fa"]
    _cli(tmp_path / "one", fa, {})
    for k in FLAG:
        assert (tmp_path / "one" / f"out.{k}").stat().st_size > 0, k
    for devices in ("0,0,0", "0,0,0,0,0,0,0,0"):
        for route, line in (("device", "multi: clustering on rank 0's GPU"), ("host", "multi: clustering on the host")):
            tag = f"{route}{devices.count(',') + 1}"
            r = _cli(tmp_path / tag, fa, {"SWARM_AMD_DEVICES": devices, "SWARM_AMD_MULTI_CLUSTER": route, "SWARM_AMD_MULTI_REPORT": "1"})
            assert line in r.stderr.splitlines(), r.stderr
            for k in FLAG:
                assert filecmp.cmp(tmp_path / "one" / f"out.{k}", tmp_path / tag / f"out.{k}", shallow=False), (tag, k)
    if S.have_reference():
        cmd = ["-d", "1", "-f"]
        for k in FLAG:
            cmd += [FLAG[k], tmp_path / f"ref.{k}"]
        r = S.run_ref_swarm(cmd + ["-l", "/dev/null", fa])
        assert r.returncode == 0, r.stderr
        for k in FLAG:
            assert filecmp.cmp(tmp_path / "one" / f"out.{k}", tmp_path / f"ref.{k}", shallow=False), ("reference", k)
