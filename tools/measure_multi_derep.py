#!/usr/bin/env python3
"""tools/measure_multi_derep.py <reads.fasta> <out.json> [device lists, default "0,0"]: `swarm -d 0 -o -w -s` on one GPU
against the same run under SWARM_AMD_DEVICES (several ranks on one device: what the run shows is the local cost of the
route, not a speed-up).  One unmeasured run, then seven fresh processes per configuration, the configurations alternating,
every process under its own time limit; the first failure ends the script.  Spans between the milestones of
SWARM_AMD_TIMING: "database uploaded" -> "dereplicated", -> "clusters made", and the whole run; md5 of the three files.
profiles/r28/NOTES.md has the numbers; the read sets are those of tools/derep_run.sh (tools/make_reads.py)."""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "swarm_amd" / "bin" / "swarm"
TMP = Path(os.environ.get("TMPDIR", "/tmp")) / f"measure.{os.getpid()}"
TMP.mkdir(parents=True, exist_ok=True)
KINDS = "ows"


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def run(fa, devices, tag):
    cmd = [str(BIN), "-d", "0"]
    for k in KINDS:
        cmd += [f"-{k}", str(TMP / f"{tag}.{k}")]
    cmd += ["-l", str(TMP / f"{tag}.log"), str(fa)]
    env = dict(os.environ, SWARM_AMD_TIMING="1")
    env.pop("SWARM_AMD_DEVICES", None)
    if devices:
        env["SWARM_AMD_DEVICES"] = devices
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=240)
    wall = time.time() - t0
    if r.returncode != 0:
        print(r.stderr[-3000:])
        raise SystemExit(f"{tag}: exit status {r.returncode}")
    t = {}
    for m in re.finditer(r"^\[t\s+([0-9.]+)\] (.*)$", r.stderr, re.M):
        t.setdefault(m.group(2).strip(), 1e3 * float(m.group(1)))
    up = t.get("database uploaded (all ranks)", t.get("database uploaded"))
    rec = {"wall_ms": 1e3 * wall, "whole_ms": t.get("results written"), "derep_ms": t["dereplicated"] - up,
           "clusters_ms": t["clusters made"] - t["dereplicated"], "md5": {k: md5(TMP / f"{tag}.{k}") for k in KINDS}}
    for k in KINDS:
        (TMP / f"{tag}.{k}").unlink()
    return rec


def summary(recs, key):
    vals = [r[key] for r in recs]
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals), "n": len(vals)}


def main():
    fa, out = sys.argv[1], sys.argv[2]
    configs = ["single"] + (sys.argv[3:] or ["0,0"])
    result = {"fasta": Path(fa).name, "runs": {c: [] for c in configs}}
    run(fa, None, "warm")                                      # (unmeasured: the file into the page cache)
    for k in range(7):
        for c in configs if k % 2 == 0 else configs[::-1]:
            rec = run(fa, None if c == "single" else c, f"run{k}")
            result["runs"][c].append(rec)
            print(c, k, {x: round(v, 3) for x, v in rec.items() if x.endswith("_ms")}, flush=True)
    result["summary"] = {c: {key: summary(recs, key) for key in ("derep_ms", "clusters_ms", "whole_ms", "wall_ms")}
                         for c, recs in result["runs"].items()}
    md5s = {json.dumps(r["md5"], sort_keys=True) for recs in result["runs"].values() for r in recs}
    result["md5_all_equal"] = len(md5s) == 1
    result["md5"] = json.loads(sorted(md5s)[0])
    Path(out).write_text(json.dumps(result, indent=1))
    print(json.dumps(result["summary"], indent=1))
    print("md5 all equal:", result["md5_all_equal"], result["md5"])


if __name__ == "__main__":
    main()
