"""The streaming index build and CSR assembly (swarm_amd/csrc/d1_stream.inc, d1_part.hip) on the GPU, stage by stage: in fresh
processes (first use of the device, fresh allocations) the d=1 network under the streaming index with either CSR
assembly equals the oracle's — whole database, a sub-range, no-cluster-breaking — the amplicon
lines equal the database they were made from, and the anchor indexes as they lie in HBM are consistent (every amplicon
once per member list, every work item a set of amplicons sharing the window, every window group listed once)."""
import subprocess
import sys

import pytest

import support as S

pytestmark = pytest.mark.gpu


def test_network_by_stage_equals_the_oracle():
    r = subprocess.run([sys.executable, str(S.ROOT / "tools" / "check_stream.py"), "200000", "stream"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "DIFFERENT" not in r.stdout
    assert "lines: wrong words 0, wrong length 0, wrong rank 0" in r.stdout


def test_indexes_in_hbm_are_consistent():
    r = subprocess.run([sys.executable, str(S.ROOT / "tools" / "check_index.py"), "200000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def _heavy_tail_db(tmp_path, env, seed):
    import os
    fa = tmp_path / "in.fa"
    subprocess.run([str(S.gen_bin()), "200000", "150", str(seed), "1", "0", str(fa)], check=True, env=dict(os.environ, **env))
    return S.db_from_fasta(fa)


@pytest.mark.parametrize("name,env,lib_env", [
    ("zipf", {"GEN_ZIPF": "0.1"}, {}),                       # families of 10^4 members: prefix groups of thousands -> the tiled pair kernel
    ("core", {"GEN_CORE": "60"}, {}),                        # conserved everywhere but a 60-nt core: anchor windows move inwards
    ("core_no_window_mode", {"GEN_CORE": "60"}, {"SWA_D1_WINDOWS": "0"}),   # ... or not: a prefix group of 87 k members -> plain kernel,
])                                                                            # identical sequences checked through the table
def test_heavy_tailed_sets_equal_the_oracle(tmp_path, monkeypatch, name, env, lib_env):
    """Real amplicon sets are not the generator's friendly case: swarms of 10^4-10^5 members that
    share their first 32 nt, and sets conserved everywhere except a hypervariable core.  The network must equal the
    oracle's whatever route the group sizes select."""
    import numpy as np
    from swarm_amd import Context
    db = _heavy_tail_db(tmp_path, env, 41)
    for k, v in lib_env.items():
        monkeypatch.setenv(k, v)
    woff, wnb, _ = S.oracle_d1_network(db)
    wnb = wnb.copy()
    for i in range(db.n):
        wnb[int(woff[i]):int(woff[i + 1])].sort()
    ctx = Context(0)
    ctx.upload_db(db.seqs, db.seq_off, db.seqlen, db.abundance, db.longest)
    assert ctx.d1_index_build() is False
    off, nb = ctx.d1_network()
    assert np.array_equal(off, woff) and np.array_equal(nb, wnb)
    if name == "core":
        # conserved flanks are answered by wider windows at the ends (round 4) or by 32-nt windows moved inwards
        assert ctx.d1_anchor_windows() != (0, 0) or ctx.d1_anchor_width() > 32
    ctx.close()


