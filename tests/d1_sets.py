"""The hard sets of the d = 1 tests and what they are checked with: shared by tests/test_d1_gpu.py and
tests/test_part_forms_gpu.py (no test file imports another)."""
import numpy as np

import support as S


def upload(ctx, db):
    ctx.upload_db(db.seqs, db.seq_off, db.seqlen, db.abundance, db.longest)


def oracle_sorted_rows(db, ncb=False, first=0, count=None):
    off, nb, dup = S.oracle_d1_network(db, ncb, first, count)
    nb = nb.copy()
    for i in range(len(off) - 1):
        nb[int(off[i]):int(off[i + 1])].sort()
    return off, nb, dup


def check_vs_oracle(ctx, db, ncb=False):
    upload(ctx, db)
    assert ctx.d1_index_build() is False
    off, nb = ctx.d1_network(ncb)
    woff, wnb, _ = oracle_sorted_rows(db, ncb)
    assert np.array_equal(off, woff)
    assert np.array_equal(nb, wnb)
    return off, nb


def giant_group_db():
    rng = np.random.default_rng(99)
    head = "".join(rng.choice(list("ACGT"), size=40))
    tail = "".join(rng.choice(list("ACGT"), size=40))
    mids = set()
    while len(mids) < 2600:
        mids.add("".join(rng.choice(list("ACGT"), size=int(rng.integers(5, 8)))))
    seqs = [head + m + tail for m in sorted(mids)]
    # plus a few ordinary clusters so that small and big groups coexist
    for k in range(30):
        base = "".join(rng.choice(list("ACGT"), size=120))
        seqs.append(base)
        for j in range(100):
            p = int(rng.integers(0, 120))
            seqs.append(base[:p] + "ACGT"[(("ACGT".index(base[p])) + 1 + j % 3) % 4] + base[p + 1:])
    seqs = sorted(set(seqs))
    db = S.build_db([(f"s{i}_{1 + (i * 13) % 40}".encode(), s.encode()) for i, s in enumerate(seqs)])
    return db


def length_mix_db():
    rng = np.random.default_rng(7)
    seqs = set()
    for L in (20, 31, 32, 33, 40, 63, 64, 65, 66, 70, 96, 97, 128, 129, 200):
        for k in range(6):
            base = "".join(rng.choice(list("ACGT"), size=L))
            seqs.add(base)
            for j in range(25):
                u = rng.random()
                p = int(rng.integers(0, L))
                if u < 0.4:
                    seqs.add(base[:p] + "ACGT"[int(rng.integers(0, 4))] + base[p + 1:])
                elif u < 0.7:
                    seqs.add(base[:p] + base[p + 1:])
                else:
                    seqs.add(base[:p] + "ACGT"[int(rng.integers(0, 4))] + base[p:])
    seqs = sorted(seqs)
    db = S.build_db([(f"s{i}_{1 + (i * 7) % 9}".encode(), s.encode()) for i, s in enumerate(seqs)])
    return db


def link_keys(off, nb):
    rows = np.repeat(np.arange(len(off) - 1, dtype=np.uint64), np.diff(off).astype(np.int64))
    return (rows << np.uint64(32)) | nb.astype(np.uint64)


def conserved_flank_set(path, n, seed, flank=40):
    """Every amplicon starts and ends with the same `flank` nucleotides (primers / conserved regions left on): with the
    default anchors (first / last 32 nt) everybody lands in one prefix and one suffix group."""
    src = path.with_suffix(".src.fa")
    S.gen_fasta(src, n, 150, seed)
    rng = np.random.default_rng(seed)
    head = "".join(rng.choice(list("ACGT"), flank))
    tail = "".join(rng.choice(list("ACGT"), flank))
    seen, out = set(), []
    for h, s in S.read_fasta(src):
        s = s.decode().upper()
        t = head + s[flank:len(s) - flank] + tail
        if t not in seen:
            seen.add(t)
            out.append(b">" + h + b"\n" + t.encode() + b"\n")
    path.write_bytes(b"".join(out))


def route_records(ctx, n, world):
    """steps 1 + 2 through the host: every slice routed, the record lists collected per owner: inbox[owner][index]"""
    cap = 3 * n // (2 * world) + 1024
    bounds = [n * r // world for r in range(world + 1)]
    inbox = [[[], []] for _ in range(world)]
    d_rec, d_counts = S.DeviceArray(2 * world * cap, np.uint64), S.DeviceArray(2 * world + 1)
    for r in range(world):
        ctx.d1_route_slice_records(bounds[r], bounds[r + 1] - bounds[r], world, d_rec, cap, d_counts)
        counts = d_counts.to_host()
        assert counts[2 * world] == 0
        rec = d_rec.to_host()
        for owner in range(world):
            for index in range(2):
                k = index * world + owner
                got = rec[k * cap: k * cap + counts[k]]
                assert ((got & np.uint64(0xFFFFFFFF)) >= bounds[r]).all() and ((got & np.uint64(0xFFFFFFFF)) < bounds[r + 1]).all()
                inbox[owner][index].append(got)
    d_rec.free(); d_counts.free()
    return inbox


def build_from_records(ctx, lists) -> bool:
    recs = [np.concatenate(lists[index]).astype(np.uint64) for index in range(2)]
    bufs = [S.DeviceArray(len(r), np.uint64) for r in recs]
    for b, r in zip(bufs, recs):
        if len(r):
            b.from_host(r)
    try:
        return ctx.d1_index_build_records(bufs[0], bufs[1])
    finally:
        for b in bufs:
            b.free()


def unrelated_db():
    """30 000 unrelated sequences of 90 .. 129 nt plus 400 neighbours (so that there is a network): as many anchor groups as
    amplicons, the fullest the key tables get"""
    rng = np.random.default_rng(808)
    seqs = set()
    while len(seqs) < 30000:
        seqs.add("".join(rng.choice(list("ACGT"), size=int(rng.integers(90, 130)))))
    seqs = sorted(seqs)
    extra = set()
    for s in seqs[:400]:
        p = int(rng.integers(0, len(s)))
        extra.add(s[:p] + s[p + 1:])
    seqs = sorted(set(seqs) | extra)
    return S.build_db([(f"s{i}_{1 + (i * 7) % 23}".encode(), s.encode()) for i, s in enumerate(seqs)])
