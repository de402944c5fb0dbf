"""tools/measure_fast_long.py — the numbers of profiles/r16/NOTES.md, by the method of profiles/r11/NOTES.md part A: in one
process, a case on a resident database, the swa_d1_fastidious call alone, 2 warm-up calls and 7 timed ones; wall ms of
the call (median, min, max) and the kernel laps of swa_timing_read (pair kernels, count kernel).

  set 1   V4-like 1 M x 250 and one 1500-nt record: default (the Bloom route for every pair), SWA_FAST_LONG=split,
          SWA_FAST_LONG=pairs
  set 2   the same without the record: default (k_fast_count) against SWA_FAST_COUNT=sites (k_fast_count_sites_words)
  set 3   full-length: gen_amplicons 200000 1500 16 1 0.3, default (all Bloom) against SWA_FAST_LONG=pairs, and the
          command line's -o file under both

usage: measure_fast_long.py [1] [2] [3]   (no argument: all three).  Prints one JSON record; fails if a switch changes a
graft candidate, a counter or the -o file."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from swarm_amd import Context, D1Clusters, HostDb  # noqa: E402

SWITCHES = ("SWA_FAST_LONG", "SWA_FAST_COUNT", "SWA_FAST_PAIRS", "SWA_FAST_SITES_CAP")
want = set(sys.argv[1:]) or {"1", "2", "3"}
work = Path(tempfile.mkdtemp(prefix="fast_long_"))
gen_bin = str(ROOT / "tools" / "gen_amplicons")
result = {"sets": {}}


def generate(path, args, conserved=None):
    env = dict(os.environ, GEN_CONSERVED=conserved) if conserved else dict(os.environ)
    subprocess.run([gen_bin, *args, str(path)], check=True, env=env)
    return ("GEN_CONSERVED=" + conserved + " " if conserved else "") + " ".join(args)


def measure(fasta, env):
    for name in SWITCHES:
        os.environ.pop(name, None)
    os.environ.update(env)
    hdb = HostDb(fasta)
    ctx = Context(0)
    ctx.upload_hostdb(hdb)
    assert ctx.d1_index_build() is False
    off, nb = ctx.d1_network()
    flags, stats = D1Clusters(hdb, off, nb).light_flags(3)
    ctx.timing_enable(True)
    wall, laps = [], []
    for i in range(9):
        ctx.d1_index_build()
        t = time.perf_counter()
        graft, counters = ctx.d1_fastidious(flags, stats[2], 16)
        dt = 1e3 * (time.perf_counter() - t)
        if i >= 2:
            wall.append(dt)
            laps.append(ctx.timing_read())
    run = {"n": hdb.n, "longest": hdb.longest, "light": int(flags.sum()), "plan": ctx.d1_fastidious_plan(),
           "split": ctx.d1_fastidious_split(), "totals": ctx.d1_fastidious_totals(), "counters": [int(c) for c in counters[:5]],
           "wall_ms": [round(v, 2) for v in wall], "wall_ms_median": round(statistics.median(wall), 2),
           "wall_ms_min_max": [round(min(wall), 2), round(max(wall), 2)],
           "pair_kernels_ms_median": round(statistics.median(l[5] for l in laps), 3),
           "count_kernel_ms_median": round(statistics.median(l[6] for l in laps), 3)}
    ctx.close()
    for name in SWITCHES:
        os.environ.pop(name, None)
    return run, graft, [int(c) for c in counters[:5]]


def compare(tag, fasta, cases):
    """every case of a set must give the first case's graft candidates and counters"""
    runs, first = {}, None
    for label, env in cases:
        run, graft, counters = measure(fasta, env)
        print(tag, label, json.dumps(run), flush=True)
        runs[label] = run
        if first is None:
            first = (graft, counters)
        run["equals_default"] = bool(np.array_equal(graft, first[0]) and counters == first[1])
        assert run["equals_default"], (tag, label)
    return runs


v4 = work / "v4_1m.fa"
if want & {"1", "2"}:
    result["v4_generator"] = generate(v4, ["1000000", "250", "11", "1", "0.3"], "60")
if "1" in want:
    rng = np.random.default_rng(7)
    outlier = "".join("ACGT"[v] for v in rng.integers(0, 4, 1500))
    with_out = work / "v4_1m_outlier.fa"
    with_out.write_bytes(v4.read_bytes() + f">zz_outlier_1\n{outlier}\n".encode())
    result["sets"]["1: V4-like 1 M x 250 + one 1500-nt record"] = compare("set1", with_out, (
        ("default (all Bloom)", {}), ("SWA_FAST_LONG=split", {"SWA_FAST_LONG": "split"}), ("SWA_FAST_LONG=pairs", {"SWA_FAST_LONG": "pairs"})))
if "2" in want:
    result["sets"]["2: V4-like 1 M x 250"] = compare("set2", v4, (
        ("default (k_fast_count)", {}), ("SWA_FAST_COUNT=sites", {"SWA_FAST_COUNT": "sites"})))
if "3" in want:
    full = work / "full_200k.fa"
    result["full_generator"] = generate(full, ["200000", "1500", "16", "1", "0.3"])
    result["sets"]["3: full-length 200 k x 1500"] = compare("set3", full, (
        ("default (all Bloom)", {}), ("SWA_FAST_LONG=pairs", {"SWA_FAST_LONG": "pairs"})))
    swarm, outputs = str(ROOT / "swarm_amd" / "bin" / "swarm"), []
    for env in ({}, {"SWA_FAST_LONG": "pairs"}):
        out = work / "cli.out"
        subprocess.run([swarm, "-d", "1", "-f", "-o", str(out), "-l", os.devnull, str(full)], check=True, timeout=300,
                       capture_output=True, text=True, env=dict(os.environ, **env))
        outputs.append(out.read_bytes())
    result["cli_o_file_identical"] = outputs[0] == outputs[1] and len(outputs[0]) > 0
    assert result["cli_o_file_identical"]
print(json.dumps(result))
