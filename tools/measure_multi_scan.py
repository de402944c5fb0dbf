#!/usr/bin/env python3
"""tools/measure_multi_scan.py <amplicons.fasta> <out.json> [-d N] [--only a+b] [--repeats K] [--compare-bin path/to/swarm]:
`swarm -d N -o` under SWARM_AMD_DN=scan on one GPU against the same run under SWARM_AMD_DEVICES — the scan left to rank 0
(SWARM_AMD_MULTI_SCAN=root), divided among two ranks, divided among eight.  All ranks share device 0: what the run shows
is the local cost of the route, not a speed-up.  One unmeasured run, then seven fresh processes per configuration, the
configurations alternating, every process under its own time limit; the first failure ends the script.  The span is
"search / scan begin" -> "scan: swarms made" of SWARM_AMD_TIMING; md5 of the -o file.  --compare-bin adds the
configuration "single, other build": the same run of another build's executable, alternating with the rest (a build
without the second stamp has no span: its whole run and wall time are what compares).
profiles/r29/NOTES.md has the numbers; the set there is `tools/gen_amplicons 100000 400 77 12` at -d 12."""
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
TMP = Path(os.environ.get("TMPDIR", "/tmp")) / f"measure.{os.getpid()}"
TMP.mkdir(parents=True, exist_ok=True)
CONFIGS = {
    "single": {},
    "0,0 root": {"SWARM_AMD_DEVICES": "0,0", "SWARM_AMD_MULTI_SCAN": "root"},
    "0,0 divided": {"SWARM_AMD_DEVICES": "0,0"},
    "8 ranks divided": {"SWARM_AMD_DEVICES": ",".join(["0"] * 8)},
}


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def run(binary, fa, d, extra, tag, limit):
    extra = dict(extra)
    binary = extra.pop("bin", binary)
    out = TMP / f"{tag}.o"
    cmd = [str(binary), "-d", str(d), "-o", str(out), "-l", str(TMP / f"{tag}.log"), str(fa)]
    env = {k: v for k, v in os.environ.items() if k not in ("SWARM_AMD_DEVICES", "SWARM_AMD_MULTI_SCAN")}
    env.update(SWARM_AMD_TIMING="1", SWARM_AMD_DN="scan", SWARM_AMD_MULTI_REPORT="1", **extra)
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=limit)
    wall = time.time() - t0
    if r.returncode != 0:
        print(r.stderr[-3000:])
        raise SystemExit(f"{tag}: exit status {r.returncode}")
    t, dn = {}, {}
    for m in re.finditer(r"^\[t\s+([0-9.]+)\] (.*)$", r.stderr, re.M):
        t.setdefault(m.group(2).strip(), 1e3 * float(m.group(1)))
    for m in re.finditer(r"^\[dn\s+([0-9.]+) ms\] (.*)$", r.stderr, re.M):
        dn.setdefault(m.group(2).strip(), float(m.group(1)))
    rec = {"wall_ms": 1e3 * wall, "whole_ms": t.get("results written"),
           "scan_ms": dn["scan: swarms made"] - dn["search / scan begin"] if "scan: swarms made" in dn else None,
           "route": [ln for ln in r.stderr.splitlines() if ln.startswith("multi: scan")], "md5": md5(out)}
    out.unlink()
    return rec


def summary(recs, key):
    vals = [r[key] for r in recs if r[key] is not None]
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals), "n": len(vals)} if vals else None


def main():
    args = sys.argv[1:]
    d, binary, only, limit, repeats = 12, ROOT / "swarm_amd" / "bin" / "swarm", None, 240, 7
    while len(args) > 2:
        flag, value = args[2], args[3]
        args = args[:2] + args[4:]
        if flag == "-d":
            d = int(value)
        elif flag == "--compare-bin":
            CONFIGS["single, other build"] = {"bin": str(Path(value).resolve())}
        elif flag == "--repeats":
            repeats = int(value)
        elif flag == "--only":                                 # configuration names joined by '+'
            only = value.split("+")
        elif flag == "--limit":
            limit = int(value)
        else:
            raise SystemExit(f"unknown option {flag}")
    fa, out = args
    configs = [c for c in CONFIGS if only is None or c in only]
    result = {"fasta": Path(fa).name, "d": d, "binary": str(binary), "runs": {c: [] for c in configs}}
    run(binary, fa, d, {}, "warm", limit)                      # (unmeasured: the file into the page cache)
    for k in range(repeats):
        for c in configs if k % 2 == 0 else configs[::-1]:
            rec = run(binary, fa, d, CONFIGS[c], f"run{k}", limit)
            result["runs"][c].append(rec)
            print(c, k, {x: round(v, 3) for x, v in rec.items() if x.endswith("_ms") and v is not None}, rec["route"], flush=True)
    result["summary"] = {c: {key: summary(recs, key) for key in ("scan_ms", "whole_ms", "wall_ms")} for c, recs in result["runs"].items()}
    md5s = {r["md5"] for recs in result["runs"].values() for r in recs}
    result["md5_all_equal"] = len(md5s) == 1
    result["md5"] = sorted(md5s)[0]
    Path(out).write_text(json.dumps(result, indent=1))
    print(json.dumps(result["summary"], indent=1))
    print("md5 all equal:", result["md5_all_equal"], result["md5"])


if __name__ == "__main__":
    main()
