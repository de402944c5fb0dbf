"""d = 0 on several GPUs: the scheme of swa_multi_derep_resident as a model on the host, and its owner function restated.

owner(hash, world) restates swa_multi_derep_owner_for: the 64-bit finaliser of MurmurHash3 over the full hash, then the high
word of the 128-bit product with world — [0, world) without a division, from bits the table slot of k_derep_claim does not use.

model_derep(seqs, world, owner_for) walks the scheme: rank r takes the slice [n r / world, n (r + 1) / world) of the reads,
sends (hash, id) of each to owner_for(hash, world); an owner keeps, per identical sequence among what it received, the
smallest id; every id comes home with the smallest id of its sequence.  Any hash of the sequence serves the model (identical
sequences must share it, nothing else matters): seq_hash is 64 bits of blake2b over the sequence."""
import hashlib

import numpy as np

import derep_sets as DS
import support as S

MASK = (1 << 64) - 1
WORLDS = (1, 2, 3, 8, 64)
NAMES = sorted(DS.SETS) + ["golden"]


def owner(h: int, world: int) -> int:
    h &= MASK
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & MASK
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & MASK
    h ^= h >> 33
    return (h * world) >> 64


def seq_hash(seq: str) -> int:
    return int.from_bytes(hashlib.blake2b(seq.encode(), digest_size=8).digest(), "little")


def make_sets(root) -> dict:
    """name -> (fasta path, db, first_identical by the oracle, the reads' sequences): made once by a module fixture, shared,
    left unchanged"""
    out = {}
    for name in NAMES:
        fa = S.GOLDEN / "d0_derep.fasta" if name == "golden" else root / f"{name}.fa"
        if name != "golden":
            DS.SETS[name](fa)
        db = S.db_from_fasta(fa)
        out[name] = (fa, db, S.oracle_derep(db), [db.seq_str(i) for i in range(db.n)])
    return out


def model_derep(seqs: list, world: int, owner_for=owner):
    """(first_identical u32[n], received per rank) of the routed scheme over the reads `seqs`, in db order"""
    n = len(seqs)
    hashes = [seq_hash(s) for s in seqs]
    inbox = [[] for _ in range(world)]
    for r in range(world):                                   # every rank routes its slice
        for i in range(n * r // world, n * (r + 1) // world):
            inbox[owner_for(hashes[i], world)].append(i)
    first = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    arrived = 0
    for got in inbox:                                        # every owner dereplicates what it received
        smallest = {}
        for i in got:
            smallest[seqs[i]] = min(i, smallest.get(seqs[i], i))
        for i in got:                                        # ... and sends (first, id) home
            assert first[i] == 0xFFFFFFFF
            first[i] = smallest[seqs[i]]
            arrived += 1
    assert arrived == n
    return first, np.array([len(g) for g in inbox], dtype=np.uint64)
