#!/usr/bin/env python3
"""tools/measure_multi_nw.py <amplicons.fasta> <out.json> [runs, default 5] [seconds a process may take, default 240]:
the -u phase of `swarm -d 1 -o -u` — "Writing UCLUST" minus the milestone before it, of SWARM_AMD_TIMING — with the
alignments on one context and divided among ranks that share one GPU (what the run shows is the local cost of the route,
not a speed-up).  Configurations: SWARM_AMD_DEVICES unset; 0,0 under SWARM_AMD_MULTI_NW=root (rank 0 alone); 0,0 divided;
eight ranks divided.  One unmeasured run, then fresh processes that alternate between the configurations, one at a time,
each under its own `timeout`; the first failure ends the script.  Per configuration: median and range of the phase and of
the whole run, the [nw] tier lines, md5 of the -u file.  profiles/r32/NOTES.md has the numbers; the sets are the bench's
10 M x 150 (bench.gen_fasta(10_000_000, 150, 1)) and `tools/gen_amplicons 200000 1500 16 1 0.3`."""
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "swarm_amd" / "bin" / "swarm"
TMP = Path(os.environ.get("TMPDIR", "/tmp")) / f"measure_nw.{os.getpid()}"
TMP.mkdir(parents=True, exist_ok=True)
CONFIGS = {"single": {}, "0,0 root": {"SWARM_AMD_DEVICES": "0,0", "SWARM_AMD_MULTI_NW": "root"}, "0,0 divided": {"SWARM_AMD_DEVICES": "0,0"},
           "8 ranks divided": {"SWARM_AMD_DEVICES": ",".join(["0"] * 8)}}
PHASE = "Writing UCLUST:"


def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()


def run(fa, extra, tag, limit):
    u = TMP / f"{tag}.u"
    cmd = ["timeout", "-k", "10", str(limit), str(BIN), "-d", "1", "-o", str(TMP / f"{tag}.o"), "-u", str(u), "-l", str(TMP / f"{tag}.log"), str(fa)]
    env = dict(os.environ, SWARM_AMD_TIMING="1", SWARM_AMD_MULTI_REPORT="1")
    for k in ("SWARM_AMD_DEVICES", "SWARM_AMD_MULTI_NW"):
        env.pop(k, None)
    env.update(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        print(r.stderr[-3000:])
        raise SystemExit(f"{tag}: exit status {r.returncode}")
    stamps = [(m.group(2).strip(), 1e3 * float(m.group(1))) for m in re.finditer(r"^\[t\s+([0-9.]+)\] (.*)$", r.stderr, re.M)]
    main_thread = [s for s in stamps if "helper thread" not in s[0]]
    at = next(i for i, s in enumerate(main_thread) if s[0].startswith(PHASE))
    rec = {"uclust_ms": main_thread[at][1] - main_thread[at - 1][1], "after": main_thread[at - 1][0],
           "whole_ms": dict(stamps).get("results written"), "nw": re.findall(r"^\[nw\] .*$", r.stderr, re.M),
           "report": re.findall(r"^multi: -u .*$", r.stderr, re.M), "md5": md5(u)}
    u.unlink()
    (TMP / f"{tag}.o").unlink()
    return rec


def summary(recs, key):
    vals = [r[key] for r in recs]
    return {"median": statistics.median(vals), "min": min(vals), "max": max(vals), "n": len(vals)}


def main():
    fa, out = sys.argv[1], sys.argv[2]
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    limit = int(sys.argv[4]) if len(sys.argv) > 4 else 240
    names = list(CONFIGS)
    result = {"fasta": Path(fa).name, "runs": {c: [] for c in names}}
    run(fa, {}, "warm", limit)                                 # (unmeasured: the file into the page cache)
    for k in range(runs):
        for c in names if k % 2 == 0 else names[::-1]:
            rec = run(fa, CONFIGS[c], f"run{k}", limit)
            result["runs"][c].append(rec)
            print(c, k, round(rec["uclust_ms"], 1), round(rec["whole_ms"], 1), rec["report"], flush=True)
    result["summary"] = {c: {key: summary(recs, key) for key in ("uclust_ms", "whole_ms")} for c, recs in result["runs"].items()}
    result["nw_lines"] = {c: recs[-1]["nw"] for c, recs in result["runs"].items()}
    result["md5_all_equal"] = len({r["md5"] for recs in result["runs"].values() for r in recs}) == 1
    Path(out).write_text(json.dumps(result, indent=1))
    print(json.dumps(result["summary"], indent=1))
    print(json.dumps(result["nw_lines"], indent=1))
    print("md5 all equal:", result["md5_all_equal"])


if __name__ == "__main__":
    main()
