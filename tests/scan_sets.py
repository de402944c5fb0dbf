"""Inputs for the direct tests of the d >= 2 scan step (tests/test_scan_step_gpu.py), the driver that walks the library's
swa_scan_batch and the plain model (tests/scan_model.py) side by side, and the bodies of the cases that need a process
of their own (SWA_SCAN_PAIR_CAP is read once per context).  Not product code."""
from __future__ import annotations

import numpy as np

import scan_model as M
import support as S

SWA_OK, SWA_E_ARG, SWA_E_CAPACITY = 0, 2, 4
MIRROR_HITS = 16384            # scan.hip's kMirrorHits: more hits than this in one batch are fetched by copy
DEFAULT_PAIR_CAP = 65536       # scan.hip: first capacity of the pair arrays = max(65536, n)
LIST_BOUND = 8                 # scan.hip: the first candidate list holds est <= 8 d


def _rand(rng, length: int) -> str:
    return "".join("ACGT"[v] for v in rng.integers(0, 4, length))


def sub(s: str, p: int, shift: int) -> str:
    """s with the base at p replaced by the one `shift` (1..3) further on in ACGT"""
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + shift) % 4] + s[p + 1:]


def subs(s: str, edits) -> str:
    for p, shift in edits:
        s = sub(s, p, shift)
    return s


def make_db(recs):
    """[(name, abundance, sequence)] -> (Db, {name: id}); no sequence and no name twice"""
    assert len({s for _, _, s in recs}) == len(recs) and len({h for h, _, _ in recs}) == len(recs)
    db = S.build_db([(f"{h}_{a}".encode(), s.encode()) for h, a, s in recs])
    return db, {h.decode().rsplit("_", 1)[0]: i for i, h in enumerate(db.headers)}


# ------------------------------------------------------------------------------------------------ driver

class Lockstep:
    """One context and one model fed with the same calls.  call() compares, exactly: the return code, nhits, the sorted
    (seed index, id, diff) triples, and what the call added to swa_scan_totals (q-gram comparisons, aligned pairs, one
    launch sequence) with the model's comparison and pair counts."""

    def __init__(self, ctx, db, d: int, ncb: bool = False, penalties=(18, 24, 13), model: M.ScanModel | None = None):
        self.ctx, self.db, self.d, self.ncb = ctx, db, d, ncb
        ctx.upload_db(db.seqs, db.seq_off, db.seqlen, db.abundance, db.longest)
        ctx.qgram_build()
        ctx.search_begin(*penalties, d)
        self.model = model or M.ScanModel(db, d, penalties)
        self.begin()

    def begin(self) -> None:
        self.ctx.scan_begin()
        self.model.begin()
        self.calls = []                     # (hits, comparisons, pairs) of every call since begin()
        t = self.ctx.scan_totals()
        assert (t["qgram_comparisons"], t["aligned_pairs"], t["launch_sequences"]) == (0, 0, 0), t

    def call(self, seeds, radii, lo: int, first: bool, cap: int | None = None):
        want, comparisons, pairs = self.model.batch(seeds, radii, lo, first, self.ncb)
        t0 = self.ctx.scan_totals()
        rc, nh, sidx, ids, diffs = self.ctx.scan_batch(seeds, radii, lo, first, self.ncb, cap)
        t1 = self.ctx.scan_totals()
        where = f"call {len(self.calls)}: {len(seeds)} seeds from {int(seeds[0])}, lo {lo}, first {first}, cap {cap}"
        assert nh == len(want), (where, nh, len(want))
        room = self.db.n if cap is None else cap        # (None: the host loop's buffers, one place an amplicon)
        if nh > room:
            assert rc == SWA_E_CAPACITY, (where, rc)
            sidx, ids, diffs = self.ctx.scan_fetch(nh)
        else:
            assert rc == SWA_OK, (where, rc)
        got = list(zip(sidx.tolist(), ids.tolist(), diffs.tolist()))
        if got != want:
            raise AssertionError((where, sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5]))
        delta = tuple(t1[k] - t0[k] for k in ("qgram_comparisons", "aligned_pairs", "launch_sequences"))
        assert delta == (comparisons, pairs, 1), (where, delta, (comparisons, pairs, 1))
        self.calls.append((want, comparisons, pairs))
        return want

    def refused(self, seeds, radii, lo: int, first: bool) -> None:
        """a call the library must refuse with SWA_E_ARG, leaving the statistics alone"""
        t0 = self.ctx.scan_totals()
        rc, nh, *_ = self.ctx.scan_batch(seeds, radii, lo, first, self.ncb)
        assert rc == SWA_E_ARG, rc
        assert self.ctx.scan_totals() == t0

    def walk(self, lo_of=None):
        """the host's whole greedy loop, every call in lockstep; lo_of(generation of the sub-seeds, lowest_unswarmed) may
        raise lowest_unswarmed of a later-generation batch"""
        def step(seeds, radii, lo, first, gen):
            if lo_of is not None and not first:
                lo = lo_of(gen, lo)
            return self.call(seeds, radii, lo, first)
        return M.greedy(step, self.db.n)


def model_walk(model: M.ScanModel, ncb: bool = False, lo_of=None):
    """the same walk over the model alone -> [(generation of the seeds, seeds, hits, comparisons, pairs, est before)]"""
    model.begin()
    log = []

    def step(seeds, radii, lo, first, gen):
        if lo_of is not None and not first:
            lo = lo_of(gen, lo)
        est = model.est.copy()
        hits, comparisons, pairs = model.batch(seeds, radii, lo, first, ncb)
        log.append((gen, list(seeds), hits, comparisons, pairs, est))
        return hits
    M.greedy(step, model.db.n)
    return log


def state_delta(ctx, before: dict) -> dict:
    now = ctx.scan_debug_state()
    return {k: now[k] - before[k] for k in ("redone", "relists", "by_copy")}


# ------------------------------------------------------------------------------------------------ case A

def two_shell_set(seed: int, length: int, n_a: int, n_b: int):
    """d = 8.  A centre c; a0 = c + 4 substitutions; b0 = a0 + 5 more; shell A = a0 + 0..2 substitutions in a region of
    its own, shell B = b0 + 0..1 in another; abundances c > every A > every B.  Every A is within 8 of c, every B is
    9 or more from c, every (A, B) pair is 5..8 apart: the second-generation batch has n_a seeds, n_a n_b hits."""
    rng = np.random.default_rng(seed)
    c = _rand(rng, length)
    x = [1 + 2 * k for k in range(9)]                       # 1, 3, .. 17
    a0 = subs(c, [(p, 1) for p in x[:4]])
    b0 = subs(a0, [(p, 2) for p in x[4:]])
    reg_a, reg_b = range(20, 50), range(52, length)
    assert 1 + 3 * len(reg_b) >= n_b
    shell_a, shell_b = [a0], [b0]
    seen = {a0}
    while len(shell_a) < n_a:
        ps = rng.choice(list(reg_a), size=int(rng.integers(1, 3)), replace=False)
        s = subs(a0, [(int(p), int(rng.integers(1, 4))) for p in ps])
        if s not in seen:
            seen.add(s)
            shell_a.append(s)
    every_b = [sub(b0, p, sh) for p in reg_b for sh in (1, 2, 3)]
    shell_b += [every_b[k] for k in rng.permutation(len(every_b))[:n_b - 1]]
    recs = [("c", 100000, c)]
    recs += [(f"a{k}", 50000 - k, s) for k, s in enumerate(shell_a)]
    recs += [(f"b{k}", 1000 - (k % 7), s) for k, s in enumerate(shell_b)]
    return make_db(recs)


def run_two_shell(ctx, seed: int, length: int, n_a: int, n_b: int, first_cap: int, small_cap: int | None = 100) -> dict:
    """Case A on `ctx`, which must not have run a scan before (first_cap = the capacity its pair arrays start with)."""
    d = 8
    db, _ = two_shell_set(seed, length, n_a, n_b)
    model = M.ScanModel(db, d)
    log = model_walk(model)
    gen, seeds, hits, comparisons, pairs, _ = log[1]
    # the batch this set is built for, from the model, before the GPU is asked anything
    assert gen == 1 and len(seeds) == n_a and len(log[0][2]) == n_a
    assert pairs > (4 * first_cap if first_cap < DEFAULT_PAIR_CAP else first_cap), (pairs, first_cap)
    assert len(hits) == n_a * n_b and (len(hits) > MIRROR_HITS), len(hits)
    before = ctx.scan_debug_state()
    assert before["pair_cap"] == 0, "a context that scanned before: its pair arrays have grown already"
    lock = Lockstep(ctx, db, d, model=model)
    swarms, _ = lock.walk()
    assert len(swarms) == 1 and len(swarms[0]) == db.n
    delta = state_delta(ctx, before)
    assert delta["redone"] >= 1 and delta["by_copy"] >= 1, delta
    assert ctx.scan_debug_state()["pair_cap"] > pairs >= first_cap
    if small_cap is not None:
        # once more, with room for `small_cap` hits: SWA_E_CAPACITY and the whole count, then swa_scan_fetch
        lock.begin()
        first = lock.call([0], [0], 1, True)
        assert len(first) == n_a > small_cap
        lock.call([i for _, i, _ in first], [df for _, _, df in first], 1, False, cap=small_cap)
        assert state_delta(ctx, before)["redone"] == delta["redone"]       # (grown arrays: no second redo)
    return delta


# ------------------------------------------------------------------------------------------------ case B

def chain_set(seed: int = 33, links: int = 11, crowd: int = 80):
    """d = 2.  A chain c0 .. c<links>, neighbours exactly 2 substitutions apart at positions of their own (6 apart: every
    substitution changes 10 q-grams of its own), abundances falling: c<j> is j generations deep with radius 2 j and a
    q-gram estimate of about 2 j against c0.  The first candidate list holds est <= 16; the sub-seed c8 (limit 18) makes
    the library list again.  Around the chain:
      w*  c2 + 1 substitution, more abundant than c3: ids between c2 and c3 (for the walk with lowest_unswarmed raised)
      x   c2 + one of the two substitutions towards c3: taken by c2 beside c3, and within d of c3, a sub-seed of the next
          batch, which must not get it again
      z   c3 + 1 substitution: within d of both c3 and x, sub-seeds of one batch
      y   c3 + one substitution towards c4
      m*  `crowd` variants of c8, 1..2 substitutions away: est 16..18 (the seed is one whose chain loses no q-gram to a
          collision up to c8), most of them absent from the first list, found by c8 in the batch that lists again
          (more than 64 pairs)
      e*  variants of c9 and c10: est 19..22, present only in the second list"""
    rng = np.random.default_rng(seed)
    slots = [4 + 6 * k for k in range(34)]
    length = slots[-1] + 4
    c = [_rand(rng, length)]
    for j in range(links):
        c.append(subs(c[-1], [(slots[2 * j], 1), (slots[2 * j + 1], 2)]))
    free = slots[2 * links:]
    assert len(free) >= 10
    recs = [(f"c{j}", 10000 - 500 * j, s) for j, s in enumerate(c)]
    recs += [(f"w{k}", 9000 - 10 * (k + 1), sub(c[2], free[k], 1)) for k in range(3)]
    x = sub(c[2], slots[4], 1)
    recs += [("x", 5, x), ("z", 4, sub(c[3], free[4], 3)), ("y", 3, sub(c[3], slots[6], 1))]
    crowd_set = []
    for p in free:
        crowd_set += [sub(c[8], p, sh) for sh in (1, 2, 3)]
    for a in range(len(free)):
        for b in range(a + 1, len(free)):
            crowd_set.append(subs(c[8], [(free[a], 1), (free[b], 2)]))
    assert len(crowd_set) >= crowd
    recs += [(f"m{k}", 100 - (k % 5), s) for k, s in enumerate(crowd_set[:crowd])]
    recs += [(f"e{j}_{k}", 50 - k, subs(c[j], [(free[k], 3), (free[k + 1], 1)][:1 + k % 2])) for j in (9, 10) for k in range(6)]
    return make_db(recs)


def run_chain(ctx, first_cap: int | None = None, raised: bool = False, model: M.ScanModel | None = None) -> dict:
    """Case B on `ctx`; first_cap: the capacity a fresh context's pair arrays start with (SWA_SCAN_PAIR_CAP)"""
    d = 2
    db, ids = chain_set()
    model = model or M.ScanModel(db, d)
    assert [ids[f"c{j}"] for j in range(4)] + [ids[f"w{k}"] for k in range(3)] == [0, 1, 2, 6, 3, 4, 5]
    lo_of = (lambda gen, lo: max(lo, ids["c3"]) if gen >= 2 else lo) if raised else None
    log = model_walk(model, lo_of=lo_of)
    assert len(log) >= 10 and log[0][1] == [0]                                # one swarm, 9 or more generations deep
    swarm0 = log[:next((k for k in range(1, len(log)) if log[k][0] == 0), len(log))]      # the calls of the first swarm
    found = {i: gen + 1 for gen, _, hits, _, _, _ in swarm0 for _, i, _ in hits}
    assert all(found[ids[f"c{j}"]] == j for j in range(1, 12))
    gen, seeds, hits, comparisons, pairs, est = next(e for e in log if e[0] == 8)
    late = [i for _, i, _ in hits if est[i] > LIST_BOUND * d]
    assert ids["c8"] in seeds and len(late) >= 40 and all(LIST_BOUND * d < est[i] <= 12 * d for i in late), (len(late),)
    if first_cap is not None:
        assert pairs > first_cap
    # x, y: taken beside a chain member that is a sub-seed of the next batch and within d of them; z: under two sub-seeds
    assert model.nw_diff(ids["c3"], ids["x"]) <= d and found[ids["x"]] == found[ids["c3"]] == 3
    z_hits = [k for e in log if e[0] == 3 for k, i, _ in e[2] if i == ids["z"]]
    assert len(z_hits) == 2
    for k in range(3):                                      # the w: within d of c2 alone (raised: left to a later swarm)
        assert (ids[f"w{k}"] in found) == (not raised)
        assert model.nw_diff(ids["c2"], ids[f"w{k}"]) <= d
    before = ctx.scan_debug_state()
    if first_cap is not None:
        assert before["pair_cap"] == 0
    lock = Lockstep(ctx, db, d, model=model)
    swarms, _ = lock.walk(lo_of=lo_of)
    assert (len(swarms) > 1) == raised
    delta = state_delta(ctx, before)
    assert delta["relists"] >= 1, delta
    if first_cap is not None:
        assert delta["redone"] >= 1, delta
    return {"delta": delta, "calls": lock.calls}


# ------------------------------------------------------------------------------------------------ case C

def star_set(seed: int = 9, length: int = 120, ones: int = 300, twos: int = 1960, targets: int = 30):
    """d = 2.  A centre with `ones` 1-substitution and `twos` 2-substitution variants (all taken by the centre: one batch
    of ones + twos sub-seeds) and `targets` variants 3 or 4 substitutions from the centre, each within 2 of a sub-seed
    (most of them of several)."""
    rng = np.random.default_rng(seed)
    c = _rand(rng, length)
    every = [(p, sh) for p in range(length) for sh in (1, 2, 3)]
    star = {frozenset([every[k]]) for k in rng.permutation(len(every))[:ones]}
    while len(star) < ones + twos:
        a, b = (every[int(k)] for k in rng.integers(0, len(every), 2))
        if a[0] != b[0]:
            star.add(frozenset([a, b]))
    star = sorted(star, key=lambda e: sorted(e))
    star = [star[k] for k in rng.permutation(len(star))]
    far = set()
    while len(far) < targets:
        base = star[int(rng.integers(0, len(star)))]
        extra = [every[int(k)] for k in rng.integers(0, len(every), 1 + len(far) % 2)]
        e = frozenset(list(base) + extra)
        if len({p for p, _ in e}) == len(base) + len(extra) and len(e) >= 3:
            far.add(e)
    recs = [("c", 100000, c)]
    recs += [(f"s{k}", 50000 - (k % 40), subs(c, sorted(e))) for k, e in enumerate(star)]
    recs += [(f"t{k}", 1 + k % 3, subs(c, sorted(e))) for k, e in enumerate(sorted(far, key=lambda e: sorted(e)))]
    return make_db(recs)


# ------------------------------------------------------------------------------------------------ case E / F

def tie_set(seed: int = 21, families: int = 12, members: int = 12, length: int = 90, d: int = 3):
    """families of variants 0..d + 1 substitutions from a centroid with abundances from {1, 1, 2, 2, 3}: most pairs tie,
    and a member may be more abundant than its centroid (the abundance rule decides, unless -n)"""
    rng = np.random.default_rng(seed)
    recs, seen = [], set()
    for f in range(families):
        cent = _rand(rng, length)
        for m in range(members):
            s = cent
            for _ in range(int(rng.integers(0, d + 2)) if m else 0):
                s = sub(s, int(rng.integers(0, length)), int(rng.integers(1, 4)))
            if s not in seen:
                seen.add(s)
                recs.append((f"f{f}m{m}", int(rng.choice([1, 1, 2, 2, 3])), s))
    return make_db(recs)


# ------------------------------------------------------------------------------------------------ child processes

def child(case: str, first_cap: int) -> None:
    """what `python -c` runs under SWA_SCAN_PAIR_CAP=<first_cap>; prints `ok <debug deltas>`"""
    from swarm_amd import Context
    ctx = Context(0)
    try:
        if case == "two_shell":
            out = run_two_shell(ctx, 3, 120, 150, 150, first_cap)
        elif case == "chain":
            out = run_chain(ctx, first_cap)["delta"]
        else:
            raise ValueError(case)
    finally:
        ctx.close()
    print("ok", out)


# ------------------------------------------------------------------------------------------------ case D

SPLIT = 65535                  # cluster_dn.cpp: sub-seeds a batch (grid.y of the filter kernels)


def split_star_fasta(path, seed: int = 13, length: int = 150, star: int = 70000, both: int = 12, single: int = 12):
    """d = 2.  A centre and `star` 2-substitution variants s<k> with strictly falling abundances (id = k + 1: one
    generation of `star` sub-seeds, split after the first 65535), and members 3 substitutions from the centre:
      both<k>   = centre + {u, v, w} where s<40 + k> = {u, v} and s<65535 + 10 + k> = {u, w}: one parent in either half
      twin<k>   = the same with s<500 + k> and s<700 + k>: two parents in one batch
      early<k>  = s<300 + k> + 2 substitutions, late<k> = s<66000 + k> + 2 substitutions, within d of no other member
    -> {name of a hanging member: [names of the star members within d of it, in queue order]}"""
    rng = np.random.default_rng(seed)
    c = _rand(rng, length)
    every = [(p, sh) for p in range(length) for sh in (1, 2, 3)]
    chosen = set()
    while len(chosen) < star:
        a = rng.integers(0, len(every), 4096)
        b = rng.integers(0, len(every), 4096)
        for x, y in zip(a.tolist(), b.tolist()):
            if every[x][0] != every[y][0] and len(chosen) < star:
                chosen.add(frozenset((every[x], every[y])))
    order = sorted(chosen, key=lambda e: sorted(e))
    order = [order[k] for k in rng.permutation(len(order))]
    hang = {}
    for name, first_at, second_at in (("both", 40, SPLIT + 10), ("twin", 500, 700)):
        for k in range(both):
            u, v = sorted(order[first_at + k])
            w = next(e for e in every if e[0] not in (u[0], v[0]) and frozenset((u, e)) not in chosen
                     and frozenset((v, e)) not in chosen)
            second = frozenset((u, w))
            chosen.discard(order[second_at + k])
            chosen.add(second)
            order[second_at + k] = second
            hang[f"{name}{k}"] = frozenset((u, v, w))
    def lone(e) -> bool:                      # no star member is a pair of these substitutions
        return all(frozenset((a, b)) not in chosen for a in e for b in e if a < b)
    for name, at in (("early", 300), ("late", 66000)):
        for k in range(single):
            # 4 substitutions from the centre, 2 from s<at + k> and more than 2 from every other star member
            u, v = sorted(order[at + k])
            ws = [e for e in every if e[0] not in (u[0], v[0]) and lone((u, e)) and lone((v, e))]
            w, x = next((w, x) for w in ws for x in ws if w[0] < x[0] and lone((w, x)))
            hang[f"{name}{k}"] = frozenset((u, v, w, x))
    assert len(set(order)) == star
    index = {e: k for k, e in enumerate(order)}
    parents = {}
    for name, e in hang.items():
        near = sorted(index[frozenset((a, b))] for a in e for b in e if a < b and frozenset((a, b)) in index)
        parents[name] = [f"s{k}" for k in near]
    with open(path, "w") as fh:
        fh.write(f">c_{10 * star}\n{c}\n")
        for k, e in enumerate(order):
            fh.write(f">s{k}_{2 * star - k}\n{subs(c, sorted(e))}\n")
        for name, e in hang.items():
            fh.write(f">{name}_1\n{subs(c, sorted(e))}\n")
    return parents
