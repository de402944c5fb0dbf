"""Inputs and the expected graph for the tests of the d >= 2 graph route at 9 <= d <= 16 (dn_graph.hip: up to 17 windows at
up to 33 shifts, k_dg_pairs_deep).  Not product code.

The variants are built, not drawn: around a centre of wlen (d + 1) + 40 nucleotides (wlen = 16 or 32: the window
length the library chooses for such lengths), for every window index k = 0 .. d

  sub     d substitutions, one in every window except k            -> window k is the only one left, unshifted
  ins     d nucleotides inserted in one piece just before window k -> window k (and all behind it) at shift +d
  del     the d nucleotides before window k deleted (k >= 1)       -> ... at shift -d
  mixins  substitutions in the windows 0 .. k - 2, then d - k + 1 nucleotides inserted in one piece inside window k - 1
                                                                    -> window k is the FIRST one left, at shift +(d - k + 1)
  mixdel  the same with a deletion (where window k - 1 has room)   -> ... at shift -(d - k + 1)
  far     d + 1 substitutions: every window except k and the tail  -> shares window k with the centre and must not appear

(The indels come in one piece because the default scoring prices a gap of one at more than two mismatches: d scattered
indels are not an alignment of d differences.  With d edits a window cannot be both the first one left and d away, except
window 0 after an insertion in front and window 1 after a deletion that takes window 0's end; `mix*` go as far as the
budget allows.)  The centre has the highest abundance of its family, so it is the QUERY of its pairs (the lower id) and the
variant the target: `first_shared_window` restates, on strings, through which window and at which shifts the library must
find a pair.  Every `ins` / `del` pair beyond its first window also sits in the groups of the later windows, at the extreme
shift: there it must be recognised as found already, or the graph holds it twice."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

from swarm_amd import nw_align_host

TAIL = 40


def centre_length(d: int, wlen: int) -> int:
    return wlen * (d + 1) + TAIL


def _rand(rng, length: int) -> str:
    return "".join("ACGT"[v] for v in rng.integers(0, 4, length))


def _other(base: str, step: int) -> str:
    return "ACGT"[("ACGT".index(base) + 1 + step % 3) % 4]


def variants(rng, cent: str, d: int, wlen: int) -> list:
    """[(kind, k, sequence)] as the module's docstring lists them"""
    out = []

    def subs(s, windows, step, at):
        for j in windows:
            p = j * wlen + at
            s[p] = _other(s[p], step)

    for k in range(d + 1):
        s = list(cent)
        subs(s, [j for j in range(d + 1) if j != k], k, wlen // 2 + (k % 3) - 1)
        out.append(("sub", k, "".join(s)))
        piece = _rand(rng, d)
        out.append(("ins", k, cent[:k * wlen] + piece + cent[k * wlen:]))
        if k >= 1:
            out.append(("del", k, cent[:k * wlen - d] + cent[k * wlen:]))
            g = d - k + 1                                         # what the budget leaves after k - 1 substitutions
            s = list(cent)
            subs(s, range(k - 1), k, wlen // 2)
            s = "".join(s)
            p = (k - 1) * wlen + 1
            m = p - 1 + wlen // 2                                 # (mid-window: a piece behind the first nucleotide can restore the window)
            out.append(("mixins", k, s[:m] + _rand(rng, g) + s[m:]))
            if g <= wlen - 2:
                out.append(("mixdel", k, s[:p] + s[p + g:]))
        s = list(cent)
        subs(s, [j for j in range(d + 1) if j != k], k + 1, wlen // 2 + 2)
        p = (d + 1) * wlen + 3 + k
        s[p] = _other(s[p], k)
        out.append(("far", k, "".join(s)))
    return out


def wanted_shift(kind: str, k: int, d: int) -> int:
    return {"sub": 0, "ins": d, "del": -d, "mixins": d - k + 1, "mixdel": -(d - k + 1)}[kind]


def window_at(query: str, target: str, k: int, s: int, wlen: int) -> bool:
    """window k of the query lies in the target at k wlen + s"""
    p = k * wlen + s
    return p >= 0 and p + wlen <= len(target) and target[p:p + wlen] == query[k * wlen:(k + 1) * wlen]


def family_set(seed: int, d: int, wlen: int, centres: int) -> tuple:
    """(records [(header, sequence)], built [(header of the centre, kind, k, header of the variant)]).  The centres'
    lengths lie 2 d + 2 apart, so that two families never pass the length test together."""
    rng = np.random.default_rng(seed)
    recs, built, seen = [], [], set()
    for c in range(centres):
        cent = _rand(rng, centre_length(d, wlen) + c * (2 * d + 2))
        assert cent not in seen
        seen.add(cent)
        ch = f"c{c}_100"
        recs.append((ch, cent))
        for kind, k, s in variants(rng, cent, d, wlen):
            if s in seen:
                continue
            seen.add(s)
            h = f"c{c}{kind}{k}_{int(rng.choice([1, 1, 2, 5]))}"
            recs.append((h, s))
            built.append((ch, kind, k, h))
    return recs, built


def write_fasta(path, recs) -> None:
    path.write_text("".join(f">{h}\n{s}\n" for h, s in recs))


def first_shared_window(query: str, target: str, d: int, wlen: int):
    """(k, shifts): the first window of the query that occurs in the target at k wlen + s, |s| <= d, and every such s;
    None when no window does"""
    for k in range(d + 1):
        w = query[k * wlen:(k + 1) * wlen]
        if len(w) < wlen:
            break
        shifts = [s for s in range(-d, d + 1)
                  if k * wlen + s >= 0 and k * wlen + s + wlen <= len(target) and target[k * wlen + s:k * wlen + s + wlen] == w]
        if shifts:
            return k, shifts
    return None


def expected_graph(hdb, d: int, penalties, no_cluster_breaking: bool):
    """The CSR swa_dn_graph must return, from the host's nw() alone: row q = every t != q with nw(query q, target t) <= d
    that the abundance rule allows, ascending, with that number.  Pairs are passed over by their length difference only."""
    return graph_from_diffs(hdb, all_pair_diffs(hdb, d, penalties), d, no_cluster_breaking)


def all_pair_diffs(hdb, d: int, penalties) -> dict:
    """{(q, t): nw differences of query q against target t} for every ordered pair whose lengths differ by at most d"""
    n = hdb.n
    off = np.asarray(hdb.seq_off)
    lens = np.asarray(hdb.seqlen).astype(np.int64)
    seqs = np.asarray(hdb.seqs)
    words = [np.ascontiguousarray(seqs[int(off[i]):int(off[i + 1])]) for i in range(n)]
    mm, go, ge = penalties
    pairs = [(q, t) for q in range(n) for t in range(n) if t != q and abs(int(lens[q] - lens[t])) <= d]
    # (the aligner keeps its state on its own stack and ctypes releases the interpreter lock: a few threads)
    with ThreadPoolExecutor(8) as pool:
        got = pool.map(lambda p: nw_align_host(words[p[1]], int(lens[p[1]]), words[p[0]], int(lens[p[0]]), mm, go, ge)[0], pairs,
                       chunksize=64)
        return dict(zip(pairs, got))


def graph_from_diffs(hdb, diffs: dict, d: int, no_cluster_breaking: bool):
    n = hdb.n
    ab = np.asarray(hdb.abundance)
    off, nb, df = [0], [], []
    rows = [[] for _ in range(n)]
    for (q, t), v in diffs.items():
        if v <= d and (t > q or no_cluster_breaking or ab[t] == ab[q]):
            rows[q].append((t, v))
    for q in range(n):
        for t, v in sorted(rows[q]):
            nb.append(t)
            df.append(v)
        off.append(len(nb))
    return np.array(off, dtype=np.uint64), np.array(nb, dtype=np.uint32), np.array(df, dtype=np.uint8)


def ids_by_header(hdb_path_records, hdb) -> dict:
    """header (without the abundance) -> id in the HostDb's order; hdb_path_records = the records as written"""
    seqs = np.asarray(hdb.seqs)
    off = np.asarray(hdb.seq_off)
    lens = np.asarray(hdb.seqlen)
    by_seq = {}
    for i in range(hdb.n):
        w = seqs[int(off[i]):int(off[i + 1])]
        s = "".join("ACGT"[(int(w[p >> 5]) >> (2 * (p & 31))) & 3] for p in range(int(lens[i])))
        by_seq[s] = i
    return {h: by_seq[s] for h, s in hdb_path_records}


def chain_set(seed: int, d: int, length: int, chains: int, links: int) -> list:
    """chains of sequences d // 2 substitutions apart, abundances falling along the chain: a member is within d of its two
    predecessors only, so a swarm's generations run as deep as the chain is long"""
    rng = np.random.default_rng(seed)
    recs, seen = [], set()
    for c in range(chains):
        s = _rand(rng, length + c)
        for m in range(links):
            assert s not in seen
            seen.add(s)
            recs.append((f"h{c}m{m}_{1000 - m}", s))
            t = list(s)
            for p in rng.choice(len(t), size=d // 2, replace=False):
                t[p] = _other(t[p], int(p))
            s = "".join(t)
    return recs


def low_complexity_set(seed: int, d: int, length: int) -> list:
    """homopolymers, dinucleotide repeats and two-letter run sequences with members 0 .. d + 3 edits away: one window at
    many shifts of the same target (one membership a group), many equally good alignments"""
    import test_align_forms_gpu as AF
    rng = np.random.default_rng(seed)
    cents = ["A" * length, "C" * (length + 3), "AC" * (length // 2), "GT" * (length // 2 + 2), "AAC" * (length // 3)]
    cents += [AF._centroid(rng, length + int(rng.integers(-3, 4)), True) for _ in range(4)]
    seen, recs = set(), []
    for f, cent in enumerate(cents):
        for m in range(12):
            letters = "ACGT" if m % 2 else "AC"
            s = AF._mutate(rng, cent, int(rng.integers(0, d + 4)) if m else 0, letters)
            if s not in seen:
                seen.add(s)
                recs.append((f"f{f}m{m}_{int(rng.choice([1, 1, 1, 2, 3]))}", s))
    return recs
