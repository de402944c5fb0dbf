#!/usr/bin/env python3
"""tools/measure_graft_layout.py <parent's swarm binary> <out.json> [n] [runs]: `swarm -d 1 -o` on gen_amplicons <n> 150 1 1 0.3
(default 10 M: BASELINE configs[2]), the parent build and this build four ways each — `-f` by default, `-f` under
SWARM_AMD_FASTIDIOUS=install and =host, and plain without `-f` —, alternated, <runs> (7) fresh processes each, every process
under its own time limit; stops at the first failure.  Spans between the milestones of SWARM_AMD_TIMING and the md5 of every
-o file (profiles/r25/NOTES.md, profiles/r26/NOTES.md)."""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

import tempfile

ROOT = Path(__file__).resolve().parent.parent
PARENT, OUT = Path(sys.argv[1]), Path(sys.argv[2])
N = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
RUNS = int(sys.argv[4]) if len(sys.argv) > 4 else 7
TMP = Path(tempfile.mkdtemp(prefix="graft_layout_"))
fa = TMP / f"layout_{N}.fa"
t0 = time.time()
subprocess.run([str(ROOT / "tools" / "gen_amplicons"), str(N), "150", "1", "1", "0.3", str(fa)], check=True, timeout=300)
print(f"set made in {time.time() - t0:.1f} s", flush=True)

WAYS = {"default": (["-f"], {}), "install": (["-f"], {"SWARM_AMD_FASTIDIOUS": "install"}),
        "host": (["-f"], {"SWARM_AMD_FASTIDIOUS": "host"}), "plain": ([], {})}
BUILDS = {f"{who}_{way}": (binary, flags, extra) for way, (flags, extra) in WAYS.items()
          for who, binary in (("parent", PARENT), ("branch", ROOT / "swarm_amd" / "bin" / "swarm"))}
GRAFTING = "Grafting light swarms on heavy swarms"
STAMP = re.compile(r"^\[t\s+([0-9.]+)\] (.*)$")


def run(tag, k):
    binary, flags, extra = BUILDS[tag]
    env = dict(os.environ, SWARM_AMD_TIMING="1", **extra)
    for name in ("SWARM_AMD_DEVICES",):
        env.pop(name, None)
    out = TMP / f"layout_{tag}.o"
    t = time.time()
    r = subprocess.run([str(binary), "-d", "1", *flags, "-o", str(out), "-l", "/dev/null", str(fa)], capture_output=True, text=True, env=env, timeout=120)
    wall = time.time() - t
    if r.returncode != 0:
        print(tag, k, "FAILED", r.returncode, r.stderr[-2000:], flush=True)
        sys.exit(1)
    stamps = {}
    for line in r.stderr.splitlines():
        m = STAMP.match(line)
        if m:
            stamps[m.group(2).strip()] = float(m.group(1))
    md5 = hashlib.md5(out.read_bytes()).hexdigest()
    rec = {"tag": tag, "run": k, "wall_s": round(wall, 3), "md5": md5,
           "clustering_to_grafting_ms": round(1e3 * (stamps[GRAFTING] - stamps["Clustering:"]), 1) if flags else None,
           "grafting_to_written_ms": round(1e3 * (stamps["Writing swarms:"] - stamps[GRAFTING]), 1) if flags else None,
           "clustering_to_written_ms": round(1e3 * (stamps["Writing swarms:"] - stamps["Clustering:"]), 1),
           "results_written_s": stamps.get("results written"),
           "details": [ln for ln in r.stderr.splitlines() if ln.startswith("[details]")],
           "stamps": stamps}
    print(json.dumps({k_: v for k_, v in rec.items() if k_ != "stamps"}), flush=True)
    return rec


records = []
run("branch_install", -1)                                             # (unmeasured: the file into the page cache)
for k in range(RUNS):
    for tag in BUILDS:
        records.append(run(tag, k))
summary = {}
for tag in BUILDS:
    mine = [r for r in records if r["tag"] == tag]
    summary[tag] = {"md5": sorted({r["md5"] for r in mine})}
    for span in ("clustering_to_grafting_ms", "grafting_to_written_ms", "clustering_to_written_ms"):
        v = [r[span] for r in mine if r[span] is not None]
        if not v:
            continue
        summary[tag][span] = {"median": statistics.median(v), "min": min(v), "max": max(v), "all": v}
print(json.dumps(summary, indent=1), flush=True)
OUT.write_text(json.dumps({"n": N, "summary": summary, "runs": records}, indent=1))
import shutil
shutil.rmtree(TMP)
