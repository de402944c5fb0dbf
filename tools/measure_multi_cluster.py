#!/usr/bin/env python3
"""tools/measure_multi_cluster.py <d1|d1f|d3> <out.json> [parent's swarm binary]: SWARM_AMD_MULTI_CLUSTER=device against
=host with two ranks on one GPU (SWARM_AMD_DEVICES=0,0: what changes between the routes lies behind the exchange, on rank
0).  One unmeasured run, then seven fresh processes per route, the routes alternating, every process under its own time
limit; the first failure ends the script.  Intervals between the milestones of SWARM_AMD_TIMING: from the network or graph
assembled (on the host route: and downloaded) to "Clustering" (with -f: "Grafting") done, the same from the upload, and the
whole run; md5 of every file.  With a third argument the d1 workload is run once more with that binary (the parent
commit's: the host route is its code path).  profiles/r23/NOTES.md has the numbers."""
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
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402  (the generator and its cache of sets)

BIN = ROOT / "swarm_amd" / "bin" / "swarm"
PARENT = Path(sys.argv[3]) if len(sys.argv) > 3 else None
TMP = Path(os.environ.get("TMPDIR", "/tmp")) / f"measure.{os.getpid()}"
TMP.mkdir(parents=True, exist_ok=True)

WORKLOADS = {
    "d1": (lambda: bench.gen_fasta(10_000_000, 150, 1), ["-d", "1"], "o"),
    "d1f": (lambda: bench.gen_fasta(10_000_000, 150, 1, 1, 0.3), ["-d", "1", "-f"], "o"),
    "d3": (lambda: bench.gen_fasta(1_000_000, 400, 1, 3, 0.0), ["-d", "3"], "osiw"),
}


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def run(binary, args, kinds, fa, env_extra, tag):
    cmd = [str(binary)] + args
    for k in kinds:
        cmd += [f"-{k}", str(TMP / f"{tag}.{k}")]
    cmd += ["-l", str(TMP / f"{tag}.log"), str(fa)]
    env = dict(os.environ, SWARM_AMD_TIMING="1", SWARM_AMD_DEVICES="0,0", **env_extra)
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=240)
    wall = time.time() - t0
    if r.returncode != 0:
        print(r.stderr[-3000:])
        raise SystemExit(f"{tag}: exit status {r.returncode}")
    t = {}
    for m in re.finditer(r"^\[t\s+([0-9.]+)\] (.*)$", r.stderr, re.M):
        t.setdefault(m.group(2).strip(), 1e3 * float(m.group(1)))
    dn = {}
    for m in re.finditer(r"^\[dn\s+([0-9.]+) ms\] (.*)$", r.stderr, re.M):
        dn.setdefault(m.group(2).strip(), float(m.group(1)))
    rec = {"wall_ms": 1e3 * wall, "whole_ms": t.get("results written"), "md5": {k: md5(TMP / f"{tag}.{k}") for k in kinds}}
    up = t.get("database uploaded (all ranks)")
    asm = t.get("network resident on rank 0", t.get("network assembled and downloaded"))
    end = t.get("Grafting light swarms on heavy swarms") if "-f" in args else t.get("Clustering:")
    if up is not None and end is not None:
        rec["from_upload_ms"] = end - up
    if asm is not None and end is not None:
        rec["from_assembled_ms"] = end - asm
        rec["network_ms"] = asm - up
    if dn:
        start = dn.get("graph: start")
        asm = dn.get("graph: resident", dn.get("graph: downloaded"))
        end = dn.get("swarm tables on the device", dn.get("swarm tables on the host", dn.get("host walk: swarms made")))
        if asm is not None and end is not None:
            rec["from_assembled_ms"] = end - asm
        if start is not None and end is not None:
            rec["from_upload_ms"] = end - start
            rec["network_ms"] = asm - start
    rec["stamps"] = {**t, **{f"dn: {k}": v for k, v in dn.items()}}
    for k in kinds:
        (TMP / f"{tag}.{k}").unlink()
    return rec


def summary(recs, key):
    vals = [r[key] for r in recs if r.get(key) is not None]
    return None if not vals else {"median": statistics.median(vals), "min": min(vals), "max": max(vals), "n": len(vals)}


def main():
    name = sys.argv[1]
    make, args, kinds = WORKLOADS[name]
    fa = make()
    result = {"workload": name, "args": args, "fasta": fa.name, "runs": {"device": [], "host": []}}
    run(BIN, args, kinds, fa, {"SWARM_AMD_MULTI_CLUSTER": "host"}, "warm")      # (unmeasured: the file into the page cache)
    for k in range(7):
        for route in ("device", "host") if k % 2 == 0 else ("host", "device"):
            rec = run(BIN, args, kinds, fa, {"SWARM_AMD_MULTI_CLUSTER": route}, f"{route}{k}")
            result["runs"][route].append(rec)
            print(route, k, {x: round(v, 3) for x, v in rec.items() if x.endswith("_ms") and v is not None}, flush=True)
    if name == "d1" and PARENT is not None:
        rec = run(PARENT, args, kinds, fa, {}, "parent")
        result["parent"] = rec
        print("parent", {x: round(v, 3) for x, v in rec.items() if x.endswith("_ms") and v is not None}, flush=True)
    result["summary"] = {route: {key: summary(recs, key) for key in ("from_assembled_ms", "from_upload_ms", "network_ms", "whole_ms", "wall_ms")}
                         for route, recs in result["runs"].items()}
    md5s = {json.dumps(r["md5"], sort_keys=True) for recs in result["runs"].values() for r in recs}
    if "parent" in result:
        md5s.add(json.dumps(result["parent"]["md5"], sort_keys=True))
    result["md5_all_equal"] = len(md5s) == 1
    result["md5"] = json.loads(sorted(md5s)[0])
    Path(sys.argv[2]).write_text(json.dumps(result, indent=1))
    print(json.dumps(result["summary"], indent=1))
    print("md5 all equal:", result["md5_all_equal"], result["md5"])


if __name__ == "__main__":
    main()
