"""The link exchange without a GPU: its two entry points are part of the library's C ABI and of the binding, and
sharding.exchange_owned_links on CPU tensors stays plain torch: it makes no helper context."""
import os
import socket
import subprocess
import sys
import textwrap

from swarm_amd import Context, capi

NEW_CALLS = ("swa_d1_links_split", "swa_d1_csr_from_lists")


def test_new_calls_are_declared_and_exported():
    lib = capi.load_library()
    for name in NEW_CALLS:
        assert name in capi.EXPORTS
        fn = getattr(lib, name)               # (AttributeError: the built library does not export it)
        assert fn.argtypes is not None and len(fn.argtypes) == {"swa_d1_links_split": 7, "swa_d1_csr_from_lists": 11}[name]
    assert callable(Context.d1_links_split) and callable(Context.d1_csr_from_lists)
    header = (capi.PKG.parent / "include" / "swarm_amd.h").read_text()
    internal = (capi.PKG / "csrc" / "swa_internal.h").read_text()
    for name in NEW_CALLS:
        assert f"int {name}(" in header
        assert name + "(" not in internal     # (one declaration: the public one)


CPU_WORKER = textwrap.dedent('''
    import sys
    import numpy as np
    import torch
    import torch.distributed as dist
    sys.path.insert(0, sys.argv[1])
    from swarm_amd import sharding
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    n, m = 1001, 5000
    rng = np.random.default_rng(3 + rank)
    links = (rng.integers(0, n, size=m).astype(np.int64) << 32) | rng.permutation(1 << 16)[:m].astype(np.int64)
    counts = [c for _, c in sharding.partition_even(n, world)]
    off, nb = sharding.exchange_owned_links(torch.from_numpy(links), counts)
    assert off.device.type == "cpu" and off.numel() == counts[rank] + 1 and int(off[-1]) == nb.numel()
    gathered = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(gathered, torch.tensor([nb.numel()]))
    assert sum(int(g) for g in gathered) == world * m          # every link arrived somewhere
    assert sharding._helper_contexts == {}, "the CPU path made a helper context"
    dist.destroy_process_group()
    print("rank", rank, "ok")
''')


def test_cpu_tensors_make_no_helper_context(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(CPU_WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    root = str(capi.PKG.parent)
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   LOCAL_WORLD_SIZE="2", GROUP_RANK="0")
        procs.append(subprocess.Popen([sys.executable, str(script), root], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
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
