#!/usr/bin/env python3
"""Regenerates tests/golden/reference_vectors.json: the UNMODIFIED reference's answers on the seeded inputs of
tests/test_oracle_vs_reference.py and on the defective files of tests/test_host_logic.py
(test_hostdb_errors_in_the_reference_order), so that those tests run where the compiled reference is not available.
Needs oracle/_ref (`make -C oracle ref`, where the reference's sources are).

    python tests/golden/make_reference_vectors.py
"""
from __future__ import annotations

import hashlib
import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE.parent), str(HERE.parent.parent)]      # tests/ and the repository (as tests/conftest.py sets them)
import support as S  # noqa: E402
import test_host_logic as H  # noqa: E402
import test_oracle_vs_reference as T  # noqa: E402


def params(test, names: str) -> list:
    return next(m.args[1] for m in test.pytestmark if m.name == "parametrize" and m.args[0] == names)


def main() -> None:
    if not S.have_reference():
        raise SystemExit("the compiled reference (oracle/_ref) is not available")
    out = {"function_fuzz_sha256": {}, "network_j": {}, "hostdb_errors": {}}
    for seed in params(T.test_function_level_fuzz, "seed"):
        # (live: every answer of the oracle is compared with the reference's before it enters the digest)
        out["function_fuzz_sha256"][str(seed)] = T.fuzz_digest(seed, True)
    with tempfile.TemporaryDirectory() as tmp:
        for n, length, seed, ncb in params(T.test_network_against_reference_binary, "n,length,seed,ncb"):
            fa, net = Path(tmp) / "in.fa", Path(tmp) / "net.txt"
            S.gen_fasta(fa, n, length, seed)
            r = S.run_ref_swarm(["-d", "1", "-j", net, "-o", "/dev/null", "-l", "/dev/null"] + (["-n"] if ncb else []) + [fa])
            assert r.returncode == 0, r.stderr
            data = net.read_bytes()
            out["network_j"][f"{n},{length},{seed},{int(ncb)}"] = {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()}
        for text, d in params(H.test_hostdb_errors_in_the_reference_order, "text,d"):
            fa = Path(tmp) / "bad.fa"
            fa.write_text(text)
            r = S.run_ref_swarm(["-d", d, "-o", "/dev/null", "-l", "/dev/null", fa])
            errors = [ln.strip() for ln in r.stderr.splitlines() if ln.startswith("Error:")]
            assert r.returncode != 0 and errors, r.stderr
            out["hostdb_errors"][f"{d}:{text}"] = errors[0]
    (HERE / "reference_vectors.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
