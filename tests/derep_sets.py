"""Read sets for the d = 0 cluster tables, and their closed form.

Every set is a small FASTA writer: the smallest shapes at which the grouping, the per-run sums and the two sorts of
derep.hip can go wrong (runs that end on, before and after a wave of 64 and a workgroup of 256; one cluster — no key
bits —; as many clusters as reads; equal masses of different sizes; masses beyond 32 bits).  Headers are distinct and the
entries are written in a shuffled order with a fixed seed; db order (abundance descending, then header) scatters a
cluster's members further.

expected_tables(first_identical, abundance) is the closed form of src/derep.cc:276-354 and 67-90 in numpy, integers only:
clusters in output order (mass descending, ties by seed index ascending) with seed, mass, size, singletons and begin,
and members[n] — grouped by cluster in SEED order (the layout of swa_d0_result: `begin` points into it), ascending db
index inside a cluster, so that the seed comes first."""
import numpy as np

_NT = np.array(list("ACGT"))


def _seq(rng, length: int) -> str:
    return "".join(rng.choice(_NT, size=length))


def _distinct(rng, count: int, lo: int, hi: int) -> list:
    seen, out = set(), []
    while len(out) < count:
        s = _seq(rng, int(rng.integers(lo, hi + 1)))
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def _write(path, entries, seed: int) -> None:
    """entries: (sequence, abundance); headers e<k>_<abundance>, shuffled with a fixed seed"""
    rng = np.random.default_rng(seed)
    named = [(f"e{k}_{int(a)}", s) for k, (s, a) in enumerate(entries)]
    with open(path, "w") as fh:
        for j in rng.permutation(len(named)):
            fh.write(f">{named[j][0]}\n{named[j][1]}\n")


def _clusters(path, sizes_and_abundances, seed: int, lo: int = 60, hi: int = 70) -> None:
    """one distinct sequence per item; an item is the list of its reads' abundances"""
    rng = np.random.default_rng(seed)
    seqs = _distinct(rng, len(sizes_and_abundances), lo, hi)
    entries = [(s, a) for s, abund in zip(seqs, sizes_and_abundances) for a in abund]
    _write(path, entries, seed + 1)


# ---- 1: one read, two identical reads, two different reads
def one_read(path):
    _write(path, [("ACGTACGTTGCA", 3)], 1)


def two_identical(path):
    _write(path, [("ACGTACGTTGCA", 3), ("ACGTACGTTGCA", 1)], 2)


def two_different(path):
    _write(path, [("ACGTACGTTGCA", 2), ("ACGTACGTTGCC", 2)], 3)


# ---- 2: 257 different reads of abundance 1: every mass ties, the order is purely by seed; crosses one workgroup
def all_different_257(path):
    _clusters(path, [[1]] * 257, 20)


# ---- 3: one sequence in `copies` copies: one cluster, zero key bits, a run that spans waves and workgroups
COPIES = [63, 64, 65, 255, 256, 257, 5000]


def one_sequence(copies: int):
    def write(path):
        rng = np.random.default_rng(30 + copies)
        _clusters(path, [[int(a) for a in rng.integers(1, 4, size=copies)]], 31 + copies)
    return write


# ---- 4: clusters whose runs begin and end on every side of the wave edges; abundances mix 1 and larger values
def wave_edges(path):
    rng = np.random.default_rng(40)
    sizes = [1, 63, 1, 64, 1, 65, 127, 129, 255, 257, 1]
    _clusters(path, [[int(a) for a in rng.choice([1, 1, 2, 5, 9], size=s)] for s in sizes], 41)


# ---- 5: equal masses of different sizes, twice, the second triple with its seeds in the opposite db order
def mass_ties(path):
    # db order is abundance descending, then header.  First triple, mass 6: the seeds come as sizes 1, 3, 6 (the read of
    # abundance 6, the three of 2, the six of 1).  Second triple, mass 20: the seeds (abundances 15, 12, 10) come as
    # sizes 6, 3, 2.  An order that looked at the size, either way, would get one of them wrong.
    first = [[2, 2, 2], [1] * 6, [6]]
    second = [[10, 10], [12, 4, 4], [15, 1, 1, 1, 1, 1]]
    _clusters(path, first + second + [[1], [4]], 50)


# ---- 6: masses beyond 32 bits, beside small ones
BIG_MASSES = [2**32 - 1, 2**32, 2**32 + 3, 2**32 + 5, 6 * 10**9]


def big_masses(path):
    _clusters(path, [[2**32 - 2, 1], [2**31, 2**31], [2**32, 1, 1, 1], [2**32 + 5], [3 * 10**9, 3 * 10**9],
                     [1], [2, 1], [5], [1, 1, 1]], 60)


# ---- 7: random sets
def random_long(path):
    _random(path, 3000, 147, 153, 6, 70)


def random_short(path):
    _random(path, 500, 17, 23, 40, 71)


def _random(path, n_unique, lo, hi, max_copies, seed):
    rng = np.random.default_rng(seed)
    uniq = _distinct(rng, n_unique, lo, hi)
    _write(path, [(s, int(rng.integers(1, 50))) for s in uniq for _ in range(int(rng.integers(1, max_copies + 1)))], seed + 1)


SETS = {"one_read": one_read, "two_identical": two_identical, "two_different": two_different,
        "all_different_257": all_different_257, "wave_edges": wave_edges, "mass_ties": mass_ties, "big_masses": big_masses,
        "random_long": random_long, "random_short": random_short}
SETS.update({f"one_sequence_{c}": one_sequence(c) for c in COPIES})

KEYS = ("seed", "mass", "size", "singletons", "begin", "members")
SUMMARY = ("swarms", "largest", "heaviest")


def expected_tables(first_identical, abundance) -> dict:
    first = np.asarray(first_identical, dtype=np.int64)
    ab = np.asarray(abundance, dtype=np.uint64)
    n = first.shape[0]
    seeds = np.flatnonzero(first == np.arange(n))
    c = seeds.shape[0]
    number = np.full(n, -1, dtype=np.int64)
    number[seeds] = np.arange(c)
    cluster = number[first]                                   # cluster number (seed order) of every read
    assert (cluster >= 0).all()
    mass = np.zeros(c, dtype=np.uint64)
    np.add.at(mass, cluster, ab)
    size = np.zeros(c, dtype=np.uint32)
    np.add.at(size, cluster, np.uint32(1))
    singles = np.zeros(c, dtype=np.uint32)
    np.add.at(singles, cluster, (ab == 1).astype(np.uint32))
    members = np.argsort(cluster, kind="stable").astype(np.uint32)
    begin = np.zeros(c, dtype=np.uint32)
    if c > 1:
        begin[1:] = np.cumsum(size.astype(np.uint64))[:-1].astype(np.uint32)
    heaviest = mass.max() if c else np.uint64(0)
    order = np.lexsort((seeds, heaviest - mass))             # mass descending (integers: no negation of a u64), then seed
    return {"seed": seeds[order].astype(np.uint32), "mass": mass[order], "size": size[order], "singletons": singles[order],
            "begin": begin[order], "members": members, "swarms": int(c), "largest": int(size.max()) if c else 0,
            "heaviest": int(heaviest)}


def assert_tables_equal(got: dict, want: dict, what: str = "") -> None:
    for k in SUMMARY:
        assert int(got[k]) == int(want[k]), (what, k, got[k], want[k])
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), (what, k)
