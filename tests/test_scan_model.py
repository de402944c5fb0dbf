"""The plain model of the d >= 2 scan step (tests/scan_model.py) checked against the reference's recorded outputs and,
where it is compiled, the reference itself: the member order of -o and the links of -i.  This tests the model, not the
library — tests/test_scan_step_gpu.py then holds the library's scan step against the model, call by call."""
import pytest

import scan_model as M
import support as S

G = S.GOLDEN


@pytest.mark.parametrize("name", ["d2_small", "d3_400", "d5_ties", "d8_16bit"])
def test_model_reproduces_golden_fixture(name):
    args = (G / f"{name}.args").read_text().split()
    d = int(args[args.index("-d") + 1])
    assert set(args) - {"-d", str(d)} == set(), "a fixture with its own scoring: pass it to the model"
    db = S.db_from_fasta(G / f"{name}.fasta")
    model = M.ScanModel(db, d)                                  # (default scoring; d8_16bit: d = 8 saturates at 65535)
    assert model.sat == (65535 if name == "d8_16bit" else 255)
    swarms, links = M.model_greedy(model)
    checked = 0
    if (G / f"{name}.o").exists():
        assert M.swarms_text(db, swarms) == (G / f"{name}.o").read_text()
        checked += 1
    if (G / f"{name}.i").exists():
        assert M.structure_text(db, links) == (G / f"{name}.i").read_text()
        checked += 1
    assert checked > 0


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("n,length,d,edits,extra", [(500, 80, 3, 3, []), (400, 60, 2, 3, ["-n"])])
def test_model_reproduces_reference_binary(tmp_path, n, length, d, edits, extra):
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, n, length, 4100 + d, edits)
    r = S.run_ref_swarm(["-d", d, "-o", tmp_path / "ro", "-i", tmp_path / "ri", "-l", "/dev/null"] + extra + [fa])
    assert r.returncode == 0, r.stderr
    db = S.db_from_fasta(fa)
    swarms, links = M.model_greedy(M.ScanModel(db, d), ncb="-n" in extra)
    assert len(swarms) < db.n and max(m[1] for sw in swarms for m in sw) >= 2      # (real swarms, later generations)
    assert M.swarms_text(db, swarms) == (tmp_path / "ro").read_text()
    assert M.structure_text(db, links) == (tmp_path / "ri").read_text()
