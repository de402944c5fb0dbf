"""tools/measure_fast_split.py — the numbers of profiles/r11/NOTES.md.  The fastidious phase of `swarm -d 1 -f` on a
V4-like 1 M x 250 set: without the 1500-nt outlier (by default and under SWA_FAST_PAIRS=words, the pair kernel that the
split uses), with it by default (the Bloom route for every pair) and with it under SWA_FAST_LONG=split.  Measured twice:
in one process a case on a resident database (the swa_d1_fastidious call alone, 2 warm-up calls and 7 timed ones: wall
ms of the call and the kernel laps of swa_timing_read), and as the command line itself (1 + 7 fresh processes a case
under SWARM_AMD_TIMING: the time between the milestones before and after the call).  Prints one JSON record; fails if
the split's result differs from the default's."""
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

work = Path(tempfile.mkdtemp(prefix="fast_split_"))
base = work / "v4_1m.fa"
gen = [str(ROOT / "tools" / "gen_amplicons"), "1000000", "250", "11", "1", "0.3", str(base)]
subprocess.run(gen, check=True, env=dict(os.environ, GEN_CONSERVED="60"))
rng = np.random.default_rng(7)
outlier = "".join("ACGT"[v] for v in rng.integers(0, 4, 1500))
with_out = work / "v4_1m_outlier.fa"
with_out.write_bytes(base.read_bytes() + f">zz_outlier_1\n{outlier}\n".encode())

result = {"generator": "GEN_CONSERVED=60 " + " ".join(gen[1:6]), "runs": {}}
grafts = {}
CASES = (("floor: no outlier", base, {}), ("floor: no outlier, SWA_FAST_PAIRS=words", base, {"SWA_FAST_PAIRS": "words"}),
         ("outlier, default (all Bloom)", with_out, {}), ("outlier, SWA_FAST_LONG=split", with_out, {"SWA_FAST_LONG": "split"}))
for label, fasta, env in CASES:
    for name in ("SWA_FAST_LONG", "SWA_FAST_PAIRS"):
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
    grafts[label] = (graft, [int(c) for c in counters[:3]])
    run = {"n": hdb.n, "longest": hdb.longest, "light": int(flags.sum()), "plan": ctx.d1_fastidious_plan(),
           "split": ctx.d1_fastidious_split(), "totals": ctx.d1_fastidious_totals(), "counters": [int(c) for c in counters[:5]],
           "wall_ms": [round(v, 2) for v in wall], "wall_ms_median": round(statistics.median(wall), 2),
           "wall_ms_min_max": [round(min(wall), 2), round(max(wall), 2)],
           "pair_kernels_ms_median": round(statistics.median(l[5] for l in laps), 3),
           "count_kernel_ms_median": round(statistics.median(l[6] for l in laps), 3)}
    result["runs"][label] = run
    print(label, json.dumps(run), flush=True)
    ctx.close()
for name in ("SWA_FAST_LONG", "SWA_FAST_PAIRS"):
    os.environ.pop(name, None)

# the command line: `swarm -d 1 -f` in fresh processes; the phase is what lies between the two milestones around the call
BEFORE, AFTER = "Counting amplicons in heavy and light swarms", "Adding light swarm amplicons to Bloom filter"
swarm = str(ROOT / "swarm_amd" / "bin" / "swarm")
result["cli"] = {}
outputs = {}
for label, fasta, env in CASES:
    phase = []
    out = work / "cli.out"
    for i in range(8):
        r = subprocess.run([swarm, "-d", "1", "-f", "-o", str(out), "-l", os.devnull, str(fasta)], check=True, timeout=120,
                           capture_output=True, text=True, env=dict(os.environ, SWARM_AMD_TIMING="1", **env))
        at = {line.split("] ", 1)[1]: float(line[2:].split("]")[0]) for line in r.stderr.splitlines() if line.startswith("[t ")}
        if i >= 1:
            phase.append(1e3 * (at[AFTER] - at[BEFORE]))
    outputs[label] = out.read_bytes()
    run = {"phase_ms": [round(v, 1) for v in phase], "phase_ms_median": round(statistics.median(phase), 1),
           "phase_ms_min_max": [round(min(phase), 1), round(max(phase), 1)]}
    result["cli"][label] = run
    print("cli", label, json.dumps(run), flush=True)
result["cli_split_equals_default"] = outputs["outlier, default (all Bloom)"] == outputs["outlier, SWA_FAST_LONG=split"]
assert result["cli_split_equals_default"]
a, b = grafts["outlier, default (all Bloom)"], grafts["outlier, SWA_FAST_LONG=split"]
result["split_equals_default"] = bool(np.array_equal(a[0], b[0]) and a[1] == b[1])
print("split equals default:", result["split_equals_default"])
print(json.dumps(result))
assert result["split_equals_default"]
