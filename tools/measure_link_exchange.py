#!/usr/bin/env python3
"""tools/measure_link_exchange.py [--per-gpu 10000000] [--world 8] [--length 150] [--reps 9] [--out FILE]

The LOCAL cost of the link exchange of a d = 1 job on several GPUs (sharding.exchange_owned_links), on one GPU that
plays rank 0 of `world`: the set-up of `bench.py --simulate-world` up to rank 0's flat link list (database of
world x per-gpu amplicons resident, ownership of rank 0, swa_d1_network_edges_device), plus — once, outside the timed
region — what the other ranks would send to rank 0 (every rank played in turn, its links with a source in rank 0's
slice kept).  Two cases on the same input, the collectives replaced by identity copies of the right sizes:

  (a) glue    the torch operations of the exchange as it was before the library had kernels for it: 64-bit sort,
              searchsorted, two host reads, [copy], 64-bit sort, bincount, cumsum, shift and mask;
  (b) library swa_d1_links_split, one host read, [copy], swa_d1_csr_from_lists.

Both are warmed up, then timed alternately `reps` times with a host clock around work that ends in a device
synchronise; median and [min, max] per case, the results compared with each other.  One JSON line on stdout.
Nothing here crosses a link between GPUs: the figure at N > 1 over RCCL is not measured on hardware by this tool."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-gpu", type=int, default=10_000_000)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args()
    assert args.reps >= 7 and args.world >= 2

    import numpy as np
    import torch

    import bench
    from swarm_amd import Context, HostDb, sharding

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    world, n_total = args.world, args.per_gpu * args.world
    with tempfile.TemporaryDirectory(prefix="swa_measure_") as tmp:
        bench.DATA_DIR = Path(tmp)
        hdb = HostDb(bench.gen_fasta(n_total, args.length, args.seed))
    assert hdb.n == n_total

    def to_dev(a, as_dtype):
        return torch.from_numpy(np.ascontiguousarray(a).view(as_dtype)).to(dev)

    t_seqs = to_dev(np.concatenate([hdb.seqs, np.zeros(2, dtype=np.uint64)]), np.int64)
    t_off, t_len, t_ab = to_dev(hdb.seq_off, np.int64), to_dev(hdb.seqlen, np.int32), to_dev(hdb.abundance, np.int64)
    ctx = Context(0, torch.cuda.current_stream(dev).cuda_stream)
    ctx.attach_db(t_seqs, t_off, t_len, t_ab, hdb.longest)
    parts = sharding.partition_even(n_total, world)
    counts = [c for _, c in parts]
    bounds = [0] + [f + c for f, c in parts]
    first, mine = parts[0]
    cap = 8 * mine
    helper = sharding._helper_context(dev)     # (what exchange_owned_links uses when it is given no context)

    # every rank in turn: its links; rank 0's are the input, of each the run for rank 0 is what rank 0 receives
    d_links = torch.zeros(cap, dtype=torch.int64, device=dev)
    d_runs = torch.empty(cap, dtype=torch.int64, device=dev)
    d_sizes = torch.empty(world + 1, dtype=torch.int64, device=dev)
    links, inbox = None, []
    for rank in range(world):
        ctx.d1_set_ownership(rank, world)
        assert ctx.d1_index_build() is False
        total = ctx.d1_network_edges_device(d_links, cap)
        helper.d1_links_split(d_links, total, bounds, d_runs, d_sizes)
        inbox.append(d_runs[: int(d_sizes[0])].clone())
        if rank == 0:
            links = d_links[:total].clone()
        torch.cuda.synchronize(dev)
    recv_list = [int(p.numel()) for p in inbox]
    arriving = torch.cat(inbox)
    del d_links, d_runs, inbox
    m, received = int(links.numel()), int(arriving.numel())

    def glue():
        keys, _ = torch.sort(links)
        cuts = torch.searchsorted(keys, torch.tensor(bounds, dtype=torch.int64, device=dev) << 32)
        send_sizes = cuts[1:] - cuts[:-1]
        recv_sizes = send_sizes.clone()                          # (the all-to-all of the sizes)
        send_list = [int(x) for x in send_sizes.tolist()]
        _ = [int(x) for x in recv_sizes.tolist()]
        assert sum(send_list) == m
        got = torch.empty(received, dtype=torch.int64, device=dev)
        got.copy_(arriving)                                      # (the all-to-all of the links)
        got, _ = torch.sort(got)
        rows = (got >> 32) - first
        offsets = torch.zeros(mine + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(rows, minlength=mine), dim=0, out=offsets[1:])
        return offsets, (got & 0xFFFFFFFF).to(torch.int32)

    def library():
        runs = torch.empty(m, dtype=torch.int64, device=dev)
        sizes = torch.empty(2 * world + 1, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()           # (as exchange_owned_links joins torch's stream and the context's)
        helper.d1_links_split(links, m, bounds, runs, sizes[:world + 1])
        sizes[world + 1:].copy_(sizes[:world])                   # (the all-to-all of the sizes)
        sizes_host = sizes.tolist()
        assert sum(sizes_host[:world]) == m
        got = torch.empty(received, dtype=torch.int64, device=dev)
        got.copy_(arriving)                                      # (the all-to-all of the links)
        offsets = torch.empty(mine + 1, dtype=torch.int64, device=dev)
        neighbours = torch.empty(received, dtype=torch.int32, device=dev)
        starts = [sum(recv_list[:r]) for r in range(world)]
        torch.cuda.current_stream(dev).synchronize()
        helper.d1_csr_from_lists(got, starts, recv_list, first, mine, offsets, neighbours, received)
        helper.synchronize()
        return offsets, neighbours

    def timed(fn) -> float:
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0)
        del out
        return ms

    a_out, b_out = glue(), library()
    torch.cuda.synchronize(dev)
    same = bool(torch.equal(a_out[0], b_out[0]) and torch.equal(a_out[1], b_out[1]))
    del a_out, b_out
    for _ in range(args.warmup):
        timed(glue); timed(library)
    ms = {"glue": [], "library": []}
    for _ in range(args.reps):
        ms["glue"].append(timed(glue)); ms["library"].append(timed(library))

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}

    result = {"what": "local work of the d=1 link exchange on rank 0 of a simulated job, one GPU, collectives = identity copies",
              "world": world, "amplicons": n_total, "length": args.length, "links_held": m, "links_received": received,
              "glue_torch": summary(ms["glue"]), "library": summary(ms["library"]), "results_equal": same,
              "library_median_below_glue_min": statistics.median(ms["library"]) < min(ms["glue"]),
              "several_gpus_over_rccl": "not measured on hardware"}
    line = json.dumps(result)
    print(line)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(line + "\n")
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
