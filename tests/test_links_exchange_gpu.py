"""The link exchange of a multi-GPU d = 1 job on the device: swa_d1_links_split (a rank's flat link list grouped by the rank
that owns each source) and swa_d1_csr_from_lists (runs of links -> the CSR of a slice), each against numpy on synthetic
link lists, both together against the whole network of an unsharded context, and sharding.exchange_owned_links on GPU
tensors against the same call on CPU copies (two processes on GPU 0, collectives over gloo)."""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import support as S
from swarm_amd import Context, sharding
from swarm_amd.capi import SWA_E_ARG, SWA_E_CAPACITY, SwaError

pytestmark = pytest.mark.gpu

GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
IDS = 70001                                   # sources of the synthetic lists lie in [0, IDS)
SPLIT_M = (0, 1, 63, 64, 65, 4095, 4096, 4097, 100003)


def _bounds_of(kind: str, world: int) -> list:
    """bound arrays (world + 1 ascending ids from 0) of one kind"""
    if kind == "even":
        return [[0] + [f + c for f, c in sharding.partition_even(IDS, world)]]
    if kind == "uneven":                      # what partition_by_length makes of sequences of very different lengths
        lens = (np.arange(IDS, dtype=np.uint32)[::-1] // 40 + 1) ** 2 % 65521 + 1
        return [[0] + [f + c for f, c in sharding.partition_by_length(lens, world)]]
    assert kind == "empty"
    if world == 1:
        return [[0, 0]]                       # (the one rank owns nothing: only the empty list can be split)
    out = []
    for empty in ({0}, {world // 2}, {world - 1}, {0, world // 2, world - 1}):
        live = [r for r in range(world) if r not in empty]
        if not live:
            continue
        cuts = [0] + [f + c for f, c in sharding.partition_even(IDS, len(live))]
        b, k = [0], 0
        for r in range(world):
            if r in live:
                k += 1
            b.append(cuts[k])
        out.append(b)
    return out


def _sources(rng, m: int, bounds: list, lo: int, hi: int) -> np.ndarray:
    """m sources in [lo, hi): first the ids next to every bound (bounds[r] - 1 and bounds[r]), then random ones"""
    edge = [v for b in bounds for v in (b - 1, b) if lo <= v < hi]
    edge = np.array(edge, dtype=np.uint64)[rng.permutation(len(edge))] if edge else np.zeros(0, dtype=np.uint64)
    src = np.concatenate([edge, rng.integers(lo, max(hi, lo + 1), size=m).astype(np.uint64)])[:m]
    return src[rng.permutation(m)]


def _check_split(ctx, links: np.ndarray, bounds: list, unaligned: bool = False):
    world, m = len(bounds) - 1, len(links)
    d_in = S.DeviceArray(m + 1, np.uint64)
    d_out = S.DeviceArray(m + 8, np.uint64)
    d_cnt = S.DeviceArray(world + 2, np.uint64)
    try:
        # (unaligned: the list begins 8 bytes into a 16-byte line, and is handed over as a raw device pointer)
        d_in.from_host(np.concatenate([np.full(1, GUARD), links]) if unaligned else links)
        d_out.from_host(np.full(m + 8, GUARD))
        d_cnt.from_host(np.full(world + 2, GUARD))
        ctx.d1_links_split(d_in.data_ptr() + 8 if unaligned else d_in, m, bounds, d_out, d_cnt)
        cnt, out = d_cnt.to_host(), d_out.to_host()
        dest = np.searchsorted(np.array(bounds[1:], dtype=np.uint64), links >> np.uint64(32), side="right")
        assert np.array_equal(cnt[:world], np.bincount(dest, minlength=world).astype(np.uint64)), (m, bounds)
        assert cnt[world] == 0 and cnt[world + 1] == GUARD
        assert int(cnt[:world].sum()) == m                        # the runs are contiguous and cover d_out[:m]
        at = 0
        for r in range(world):
            run = out[at: at + int(cnt[r])]
            assert np.array_equal(np.sort(run), np.sort(links[dest == r])), (m, bounds, r)
            at += int(cnt[r])
        assert np.all(out[m:] == GUARD)
    finally:
        d_in.free(); d_out.free(); d_cnt.free()


@pytest.mark.parametrize("world", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("kind", ["even", "uneven", "empty", "one"])
def test_split_groups_the_links_by_owner(gpu_ctx, world, kind):
    rng = np.random.default_rng(1000 * world + len(kind))
    if kind == "one":                          # every link goes to one rank, here the middle one
        bounds_list = _bounds_of("even", world)
    else:
        bounds_list = _bounds_of(kind, world)
    for bounds in bounds_list:
        lo, hi = (bounds[world // 2], bounds[world // 2 + 1]) if kind == "one" else (0, bounds[world])
        for m in SPLIT_M if hi > lo else (0,):
            src = _sources(rng, m, bounds, lo, hi)
            links = (src << np.uint64(32)) | rng.integers(0, 1 << 31, size=m).astype(np.uint64)
            _check_split(gpu_ctx, links, bounds)
    # the same with a list that does not begin on a 16-byte line
    bounds = bounds_list[-1]
    lo, hi = (bounds[world // 2], bounds[world // 2 + 1]) if kind == "one" else (0, bounds[world])
    for m in (1, 2, 4097) if hi > lo else ():
        src = _sources(rng, m, bounds, lo, hi)
        _check_split(gpu_ctx, (src << np.uint64(32)) | rng.integers(0, 1 << 31, size=m).astype(np.uint64), bounds, unaligned=True)


def test_split_reports_a_source_nobody_owns(gpu_ctx):
    rng = np.random.default_rng(7)
    world, m = 3, 5000
    bounds = [0, 100, 100, 40000]
    src = _sources(rng, m, bounds, 0, 40000)
    src[1234] = 40000                          # = bounds[world]: the first id no rank owns
    links = (src << np.uint64(32)) | rng.integers(0, 1 << 31, size=m).astype(np.uint64)
    d_in, d_out, d_cnt = S.DeviceArray(m, np.uint64), S.DeviceArray(m + 8, np.uint64), S.DeviceArray(world + 1, np.uint64)
    try:
        d_in.from_host(links)
        d_out.from_host(np.full(m + 8, GUARD))
        with pytest.raises(SwaError) as e:
            gpu_ctx.d1_links_split(d_in, m, bounds, d_out, d_cnt)
        assert e.value.code == SWA_E_ARG and "beyond" in str(e.value)
        cnt, out = d_cnt.to_host(), d_out.to_host()
        dest = np.searchsorted(np.array(bounds[1:], dtype=np.uint64), src, side="right")
        assert np.array_equal(cnt, np.bincount(dest, minlength=world + 1).astype(np.uint64)) and cnt[world] == 1
        assert np.all(out[m - 1:] == GUARD)    # (the link nobody owns is written nowhere: one place of d_out stays as it was)
        assert np.array_equal(np.sort(out[:m - 1]), np.sort(np.delete(links, 1234)))
        # buffers that are not 8-byte aligned (raw pointers)
        for shift in ((4, 0, 0), (0, 4, 0), (0, 0, 4)):
            with pytest.raises(SwaError) as e:
                gpu_ctx.d1_links_split(d_in.data_ptr() + shift[0], m - 1, bounds, d_out.data_ptr() + shift[1], d_cnt.data_ptr() + shift[2])
            assert e.value.code == SWA_E_ARG
        # bounds that do not begin at 0, descend, name no rank, name more than 64
        for bad in ([1, 5], [0, 9, 3], [0], list(range(67))):
            with pytest.raises(SwaError) as e:
                gpu_ctx.d1_links_split(d_in, m, bad, d_out, d_cnt)
            assert e.value.code == SWA_E_ARG
    finally:
        d_in.free(); d_out.free(); d_cnt.free()


def _csr_reference(keys: np.ndarray, first: int, count: int):
    """rows ascending, neighbours ascending within a row (lexsort by source, then target)"""
    src, tgt = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    order = np.lexsort((tgt, src))
    offsets = np.searchsorted(src[order], np.arange(first, first + count + 1)).astype(np.uint64)
    return offsets, tgt[order]


def _csr_from_runs(ctx, runs: list, first: int, count: int, rng, caps=None):
    """runs laid into one buffer with gaps of foreign words between them; the CSR call with every cap of `caps` in turn
    (default: too small, then with room); returns (offsets, neighbours) of the last call"""
    pieces, starts, at = [], [], 0
    for run in runs:
        gap = int(rng.integers(0, 5))
        pieces.append(np.full(gap, GUARD)); at += gap
        starts.append(at); pieces.append(run); at += len(run)
    pieces.append(np.full(3, GUARD))
    buf = np.concatenate(pieces).astype(np.uint64)
    total = sum(len(r) for r in runs)
    want_off, want_nb = _csr_reference(np.concatenate(runs) if runs else np.zeros(0, dtype=np.uint64), first, count)
    d_links = S.DeviceArray(len(buf), np.uint64)
    d_off = S.DeviceArray(count + 2, np.uint64)
    d_nb = S.DeviceArray(total + 8, np.uint32)
    try:
        d_links.from_host(buf)
        for cap in caps if caps is not None else (total // 2, total + 3):
            d_off.from_host(np.full(count + 2, GUARD))
            d_nb.from_host(np.full(total + 8, 0xA5A5A5A5, dtype=np.uint32))
            if cap < total:
                with pytest.raises(SwaError) as e:
                    ctx.d1_csr_from_lists(d_links, starts, [len(r) for r in runs], first, count, d_off, d_nb, cap)
                assert e.value.code == SWA_E_CAPACITY and e.value.total == total
            else:
                assert ctx.d1_csr_from_lists(d_links, starts, [len(r) for r in runs], first, count, d_off, d_nb, cap) == total
            off, nb = d_off.to_host(), d_nb.to_host()
            assert np.array_equal(off[:count + 1], want_off) and off[count + 1] == GUARD, (first, count, cap)
            assert np.all(nb[min(cap, total):] == 0xA5A5A5A5), (first, count, cap)
            if cap >= total:
                assert np.array_equal(nb[:total], want_nb), (first, count, cap)
        return off[:count + 1], nb[:total]
    finally:
        d_links.free(); d_off.free(); d_nb.free()


@pytest.mark.parametrize("first", [0, 1, 70001])
@pytest.mark.parametrize("count", [1, 255, 256, 257, 65537])
def test_csr_of_a_slice_from_runs(gpu_ctx, first, count):
    rng = np.random.default_rng(first * 7 + count)
    # links per row: about two, a third of the rows none; one row beyond 255 and one beyond 4096 links (a whole workgroup
    # takes their buckets: k_csr_bucket_big)
    per_row = rng.integers(0, 5, size=count) * (rng.random(count) < 0.67)
    per_row[int(rng.integers(0, count))] = 5000
    if count > 1:
        rows = np.flatnonzero(per_row != 5000)
        per_row[rows[int(rng.integers(0, len(rows)))]] = 300
    src = np.repeat(np.arange(first, first + count, dtype=np.uint64), per_row)
    tgt = rng.integers(0, 1 << 31, size=len(src)).astype(np.uint64)
    keys = np.unique((src << np.uint64(32)) | tgt)[::-1].copy()          # each link once; rows and neighbours in descending order
    assert np.bincount((keys >> np.uint64(32)).astype(np.int64) - first).max() > 4096
    nlists = 1 + (first + count) % 9
    cuts = np.sort(rng.integers(0, len(keys) + 1, size=nlists - 1))
    if nlists >= 3:
        cuts[1] = cuts[0]                      # an empty list
    runs = np.split(keys, cuts)
    assert len(runs) == nlists
    _csr_from_runs(gpu_ctx, runs, first, count, rng)
    # no list at all, and lists without a link: every row empty
    off, nb = _csr_from_runs(gpu_ctx, [], first, count, rng, caps=(0,))
    assert not off.any() and len(nb) == 0
    _csr_from_runs(gpu_ctx, [np.zeros(0, dtype=np.uint64)] * 2, first, count, rng, caps=(0,))


def test_exchange_on_one_gpu_equals_the_whole_network(tmp_path):
    """Every rank of a world in turn on one context: its links under ownership, split by the bounds of the final partition;
    then, for every destination, the ranks' runs side by side -> the CSR of its slice = those rows of the whole network."""
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, 20000, 150, 43)
    db = S.db_from_fasta(fa)
    rng = np.random.default_rng(43)
    ctx = Context(0)
    bufs = []
    try:
        ctx.upload_db(db.seqs, db.seq_off, db.seqlen, db.abundance, db.longest)
        assert ctx.d1_index_build() is False
        whole_off, whole_nb = ctx.d1_network()
        cap = len(whole_nb) + 16
        d_links, d_out = S.DeviceArray(cap, np.uint64), S.DeviceArray(cap, np.uint64)
        bufs += [d_links, d_out]
        for world in (2, 3, 8):
            parts = sharding.partition_even(db.n, world)
            bounds = [0] + [f + c for f, c in parts]
            d_cnt = S.DeviceArray(world + 1, np.uint64)
            bufs.append(d_cnt)
            sent = []                          # [rank][destination]: the run
            for rank in range(world):
                ctx.d1_set_ownership(rank, world)
                assert ctx.d1_index_build() is False
                total = ctx.d1_network_edges_device(d_links, cap)
                ctx.d1_links_split(d_links, total, bounds, d_out, d_cnt)
                cnt, out = d_cnt.to_host(), d_out.to_host(total)
                assert cnt[world] == 0 and int(cnt[:world].sum()) == total
                ends = np.cumsum(cnt[:world]).astype(np.int64)
                sent.append([out[e - int(c): e] for e, c in zip(ends, cnt[:world])])
            assert sum(len(run) for row in sent for run in row) == len(whole_nb)
            ctx.d1_set_ownership(0, 1)
            for dest, (first, count) in enumerate(parts):
                off, nb = _csr_from_runs(ctx, [sent[rank][dest] for rank in range(world)], first, count, rng,
                                         caps=(int(whole_off[first + count] - whole_off[first]),))
                lo, hi = int(whole_off[first]), int(whole_off[first + count])
                assert np.array_equal(off, whole_off[first: first + count + 1] - whole_off[first]), (world, dest)
                assert np.array_equal(nb, whole_nb[lo:hi]), (world, dest)
    finally:
        for b in bufs:
            b.free()
        ctx.close()


EXCHANGE_WORKER = textwrap.dedent('''
    import sys
    import numpy as np
    import torch
    import torch.distributed as dist
    torch.zeros(1, device="cuda:0")            # torch initialises the GPU first (as in bench.py)
    sys.path.insert(0, sys.argv[1])
    from swarm_amd import sharding
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    sorts = [0]
    torch_sort = torch.sort
    def counted_sort(*a, **k):
        sorts[0] += 1
        return torch_sort(*a, **k)
    torch.sort = counted_sort
    n = 50001
    full = 150000 + 7 * rank
    # (counts, links this rank holds, their sources below): the last two have a rank that holds no link at all — in the
    # first of them it owns rows and receives nothing either, in the second it receives everything
    cases = [([25001, 25000], full, n), ([50001, 0], full, n), ([123, 49878], full, n),
             ([25001, 25000], full if rank == 0 else 0, 25001), ([25001, 25000], 0 if rank == 0 else full, n)]
    for counts, m, below in cases:
        rng = np.random.default_rng(17 + rank)
        links = (rng.integers(0, below, size=m).astype(np.int64) << 32) | rng.permutation(1 << 20)[:m].astype(np.int64)
        on_cpu = torch.from_numpy(links)
        on_gpu = on_cpu.to("cuda:0")
        sorts[0] = 0
        g_off, g_nb = sharding.exchange_owned_links(on_gpu, counts)
        g_host = (g_off.cpu(), g_nb.cpu())     # (on torch's stream, with nothing waited for in between: the results must be there)
        assert sorts[0] == 0, "torch.sort ran on the GPU path"
        assert len(sharding._helper_contexts) == 1
        c_off, c_nb = sharding.exchange_owned_links(on_cpu, counts)
        assert sorts[0] == 2                   # (the wrapper does count: the torch path sorts twice)
        assert g_off.device.type == "cuda" and g_off.dtype == torch.int64 and g_nb.dtype == torch.int32
        assert g_off.shape == c_off.shape and torch.equal(g_host[0], c_off), "offsets differ"
        assert g_nb.shape == c_nb.shape and torch.equal(g_host[1], c_nb), "neighbours differ"
        assert torch.equal(on_gpu.cpu(), on_cpu), "the caller's links were changed"
    dist.all_reduce(torch.zeros(1))
    dist.destroy_process_group()
    print("rank", rank, "ok")
''')


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_exchange_owned_links_on_gpu_tensors_equals_cpu(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(EXCHANGE_WORKER)
    port = str(_free_port())
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   LOCAL_WORLD_SIZE="2", GROUP_RANK="0")
        procs.append(subprocess.Popen([sys.executable, str(script), str(S.ROOT)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True, env=env))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    for p, (out, err) in zip(procs, outs):
        assert p.returncode == 0, out[-2000:] + err[-3000:]
    assert sum(out.count("ok") for out, _ in outs) == 2
