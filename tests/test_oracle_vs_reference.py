"""Fuzz the oracle against the compiled, unmodified reference (oracle/_ref, built by oracle/Makefile where the
reference's sources are).  The reference's answers on the same seeded inputs are also kept in
tests/golden/reference_vectors.json (tests/golden/make_reference_vectors.py): the oracle is checked against them
everywhere, and against the live reference where it is available."""
import ctypes as C
import hashlib
import json
import subprocess
import sys

import numpy as np
import pytest

import support as S

def gold() -> dict:
    return json.loads((S.GOLDEN / "reference_vectors.json").read_text())


_FUZZ = r'''
import ctypes as C, hashlib, sys
import numpy as np
sys.path.insert(0, %r)
import support as S
live = %r                       # compare with the compiled reference as well (else: only the digest, checked by the caller)
lib = S.oracle()
digest = hashlib.sha256()
def note(*values):              # everything the oracle answered, in order: the caller compares the digest with the reference's
    digest.update(repr(tuple(v if isinstance(v, (bytes, list)) else int(v) for v in values)).encode())
if live:
    ref = C.CDLL(str(S.REF_DIR / "libswarmref.so"))
    for f in ("ref_zobrist_table", "ref_zobrist_hash", "ref_zobrist_hash_delete_first", "ref_zobrist_hash_insert_first", "ref_nw"):
        getattr(ref, f).restype = C.c_uint64
ZL = 700
ot = S.oracle_zobrist(ZL)
note(ot.tobytes())
if live:
    assert ref.ref_zobrist_init(ZL) == 0
    rt = np.zeros(4 * ZL, dtype=np.uint64)
    ref.ref_zobrist_table(rt.ctypes.data_as(S.u64p), C.c_uint64(4 * ZL))
    assert np.array_equal(rt, ot)
rng = np.random.default_rng(int(sys.argv[1]))
for trial in range(250):
    L = int(rng.integers(1, 600))
    alpha = [b"ACGT", b"AC", b"A", b"ACGT"][trial %% 4]
    s = bytes(rng.choice(list(alpha), size=L).tolist())
    w = S.pack_seq(s)
    wp = w.ctypes.data_as(S.u64p); cp = w.ctypes.data_as(C.c_char_p); tp = ot.ctypes.data_as(S.u64p)
    h = lib.orc_zobrist_hash(tp, wp, L)
    h_del = lib.orc_zobrist_hash_delete_first(tp, wp, L)
    h_ins = lib.orc_zobrist_hash_insert_first(tp, wp, L)
    variants = S.oracle_variants(ot, w, L, h)
    qb = np.zeros(128, dtype=np.uint8)
    lib.orc_findqgrams(wp, L, qb.ctypes.data_as(S.u8p))
    note(h, h_del, h_ins, [tuple(int(x) for x in v) for v in variants], qb.tobytes())
    if not live:
        continue
    assert h == ref.ref_zobrist_hash(cp, L)
    assert h_del == ref.ref_zobrist_hash_delete_first(cp, L)
    assert h_ins == ref.ref_zobrist_hash_insert_first(cp, L)
    N = 7 * L + 5
    oh = np.zeros(N, dtype=np.uint64); op = np.zeros(N, dtype=np.uint32); oty = np.zeros(N, dtype=np.uint8); ob = np.zeros(N, dtype=np.uint8)
    n = ref.ref_generate_variants(cp, L, C.c_uint64(h), oh.ctypes.data_as(S.u64p), op.ctypes.data_as(S.u32p),
                                  oty.ctypes.data_as(S.u8p), ob.ctypes.data_as(S.u8p))
    assert [(int(oh[i]), int(op[i]), int(oty[i]), int(ob[i])) for i in range(n)] == variants
    qa = np.zeros(128, dtype=np.uint8)
    ref.ref_findqgrams(cp, C.c_uint64(L), qa.ctypes.data_as(S.u8p))
    assert np.array_equal(qa, qb)
for trial in range(300):
    L = int(rng.integers(1, 120))
    alpha = list("ACGT" if trial %% 2 else "AC")
    a = "".join(rng.choice(alpha, size=L))
    b = list(a)
    for _ in range(int(rng.integers(0, 6))):
        p = int(rng.integers(0, len(b))) if b else 0
        u = rng.random()
        if u < 0.5 and b: b[p] = alpha[int(rng.integers(0, len(alpha)))]
        elif u < 0.75 and len(b) > 1: del b[p]
        else: b.insert(p, alpha[int(rng.integers(0, len(alpha)))])
    b = "".join(b)
    wa = S.pack_seq(a.encode()); wb = S.pack_seq(b.encode())
    mm, go, ge = [(18, 24, 13), (4, 12, 1), (2, 3, 1)][trial %% 3]
    al2 = C.c_uint64(0)
    got = lib.orc_nw_diff(wb.ctypes.data_as(S.u64p), len(b), wa.ctypes.data_as(S.u64p), len(a), mm, go, ge, C.byref(al2), None)
    note(got, al2.value)
    if not live:
        continue
    al = C.c_uint64(0); buf = C.create_string_buffer(len(a) + len(b) + 8)
    want = ref.ref_nw(wb.ctypes.data_as(C.c_char_p), C.c_uint64(len(b)), wa.ctypes.data_as(C.c_char_p), C.c_uint64(len(a)),
                      C.c_int64(mm), C.c_uint64(go), C.c_uint64(ge), buf, C.byref(al))
    assert (got, al2.value) == (want, al.value), (a, b, mm, go, ge)
print("ok", digest.hexdigest())
'''


def fuzz_digest(seed: int, live: bool) -> str:
    """The oracle's answers on the fuzz inputs of `seed`, as a digest; with `live`, every answer is first compared with the
    compiled reference's.  Own process: the reference's generators are only valid on their first call per process."""
    r = subprocess.run([sys.executable, "-c", _FUZZ % (str(S.ROOT / "tests"), live), str(seed)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"], r.stderr[-2000:]
    return r.stdout.split()[1]


def oracle_network_lines(fa, ncb: bool) -> bytes:
    """What the reference's -j writes for the d = 1 network of `fa`, as the oracle computes it."""
    db = S.db_from_fasta(fa)
    off, nb, _ = S.oracle_d1_network(db, ncb)
    lines = []
    for i in range(db.n):
        for j in sorted(nb[int(off[i]):int(off[i + 1])].tolist()):
            lines.append(db.headers[i] + b"\t" + db.headers[j] + b"\n")
    return b"".join(lines)


@pytest.mark.parametrize("seed", [1, 2])
def test_function_level_fuzz(seed):
    assert fuzz_digest(seed, S.have_reference()) == gold()["function_fuzz_sha256"][str(seed)]


@pytest.mark.parametrize("n,length,seed,ncb", [(2500, 150, 101, False), (1500, 64, 102, True), (800, 300, 103, False)])
def test_network_against_reference_binary(tmp_path, n, length, seed, ncb):
    fa = tmp_path / "in.fa"
    S.gen_fasta(fa, n, length, seed)
    got = oracle_network_lines(fa, ncb)
    want = gold()["network_j"][f"{n},{length},{seed},{int(ncb)}"]
    assert (len(got), hashlib.sha256(got).hexdigest()) == (want["bytes"], want["sha256"])
    if S.have_reference():
        net = tmp_path / "net.txt"
        r = S.run_ref_swarm(["-d", "1", "-j", net, "-o", "/dev/null", "-l", "/dev/null"] + (["-n"] if ncb else []) + [fa])
        assert r.returncode == 0, r.stderr
        assert got == net.read_bytes()


# the scorings the alignment-form tests (test_align_forms_gpu.py) take the oracle as ground truth at: gapopen = 0, one
# gap opening at most in 16 bits, T = 255 exactly, a mismatch penalty of 255 and a representative of every kernel form
_NEW_SCORINGS = [(4, 0, 3), (8, 0, 9), (2, 0, 1), (18, 60000, 13), (4, 14, 3), (12, 10, 19), (4, 2, 15), (4, 2, 1),
                 (18, 24, 13), (255, 1, 2)]


@pytest.mark.skipif(not S.have_reference(), reason="compiled reference not available on this box")
@pytest.mark.parametrize("scoring", _NEW_SCORINGS, ids=[f"{m}-{o}-{e}" for m, o, e in _NEW_SCORINGS])
def test_oracle_nw_at_new_scorings(scoring):
    """orc_nw_diff against the reference's own nw() (ref_nw): differences and alignment length, on related pairs over
    ACGT and over two letters, 1 to ~2 000 nt."""
    ref = C.CDLL(str(S.REF_DIR / "libswarmref.so"))
    ref.ref_nw.restype = C.c_uint64
    lib = S.oracle()
    mm, go, ge = scoring
    rng = np.random.default_rng(sum(scoring))
    for trial in range(60):
        L = int(rng.integers(1, 2100)) if trial % 6 == 0 else int(rng.integers(1, 320))
        alpha = list("ACGT" if trial % 2 else "AC")
        a = "".join(rng.choice(alpha, size=L))
        b = list(a)
        for _ in range(int(rng.integers(0, 12))):
            p = int(rng.integers(0, len(b) + 1))
            u = rng.random()
            if u < 0.5 and p < len(b):
                b[p] = alpha[int(rng.integers(0, len(alpha)))]
            elif u < 0.75 and p < len(b) and len(b) > 1:
                del b[p]
            else:
                b.insert(p, alpha[int(rng.integers(0, len(alpha)))])
        b = "".join(b)
        wa, wb = S.pack_seq(a.encode()), S.pack_seq(b.encode())
        alen, score = C.c_uint64(0), C.c_uint64(0)
        got = lib.orc_nw_diff(wb.ctypes.data_as(S.u64p), len(b), wa.ctypes.data_as(S.u64p), len(a), mm, go, ge,
                              C.byref(alen), C.byref(score))
        ral, buf = C.c_uint64(0), C.create_string_buffer(len(a) + len(b) + 8)
        want = ref.ref_nw(wb.ctypes.data_as(C.c_char_p), C.c_uint64(len(b)), wa.ctypes.data_as(C.c_char_p),
                          C.c_uint64(len(a)), C.c_int64(mm), C.c_uint64(go), C.c_uint64(ge), buf, C.byref(ral))
        assert (got, alen.value) == (want, ral.value), (scoring, a, b)
        assert score.value == _path_cost(buf.raw[:ral.value][::-1], b, a, mm, go, ge), (scoring, a, b)


def _path_cost(ops: bytes, d: str, q: str, mm: int, go: int, ge: int) -> int:
    """The cost of the reference's own alignment path (ref_nw's operations, first column first): mismatches, and
    gapopen + length * gapextend per gap run.  'I' consumes a nucleotide of d, 'D' one of q, 'M' one of each."""
    cost, i, j, prev = 0, 0, 0, None
    for op in ops:
        if op == ord("M"):
            cost += mm if d[i] != q[j] else 0
            i, j = i + 1, j + 1
        else:
            cost += ge + (go if op != prev else 0)
            i, j = (i + 1, j) if op == ord("I") else (i, j + 1)
        prev = op
    assert (i, j) == (len(d), len(q))
    return cost
