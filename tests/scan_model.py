"""A plain model of the fused d >= 2 scan step (scan.hip) and of the host's greedy loop over it (swa_dn_cluster), built on
the oracle alone: orc_findqgrams, orc_qgram_diff, orc_nw_diff.  Not product code.

One batch is the reference's candidate rule (src/algo.cc:423-442, 515-531) for every seed k of the batch against every
pool amplicon i:  i >= lowest_unswarmed, i is not the seed, i is not swarmed, in a later generation
est[i] <= radius_k + d, and unless -n abundance[i] <= abundance[seed].  A pair that passes is a COMPARISON (in a first
generation it stores est[i] = the q-gram bound); a comparison whose q-gram bound is <= d is a PAIR; a pair whose
alignment has <= d differences is a HIT (k, i, diff), and i is swarmed once the batch is over.  All seeds of a batch see
the pool as it was when the batch started."""
from __future__ import annotations

import ctypes as C

import numpy as np

import support as S


def saturation(d: int, mm: int, go: int, ge: int) -> int:
    """the score at which the reference's search saturates for this scoring and d: 8-bit mode where d mismatches and d
    gaps of one fit a byte, else 16-bit (src/scan.cc; the rule tests/test_scan_gpu.py uses)"""
    return 65535 if d > min(255 // mm, 255 // (go + ge)) else 255


class ScanModel:
    def __init__(self, db: S.Db, d: int, penalties=(18, 24, 13)):
        self.db, self.d = db, int(d)
        self.mm, self.go, self.ge = (int(v) for v in penalties)
        self.sat = saturation(self.d, self.mm, self.go, self.ge)
        self.lib = S.oracle()
        n = db.n
        self.sigs = np.zeros((n, 128), dtype=np.uint8)
        self._words = [np.ascontiguousarray(db.words(i)) for i in range(n)]
        self._wp = [S._p(w, S.u64p) for w in self._words]
        self._len = [int(v) for v in db.seqlen]
        for i in range(n):
            self.lib.orc_findqgrams(self._wp[i], self._len[i], S._p(self.sigs[i], S.u8p))
        self._sp = [S._p(self.sigs[i], S.u8p) for i in range(n)]
        self.ab = db.abundance.astype(np.uint64)
        self._ids = np.arange(n, dtype=np.int64)
        self._qcache, self._ncache = {}, {}
        self.begin()

    def begin(self) -> None:
        """swa_scan_begin: every amplicon unswarmed, no estimates"""
        self.est = np.zeros(self.db.n, dtype=np.int64)
        self.swarmed = np.zeros(self.db.n, dtype=bool)

    def qgram_diff(self, a: int, b: int) -> int:
        key = (a, b) if a < b else (b, a)
        v = self._qcache.get(key)
        if v is None:
            v = self._qcache[key] = int(self.lib.orc_qgram_diff(self._sp[a], self._sp[b]))
        return v

    def nw_diff(self, query: int, target: int) -> int:
        """differences of the alignment search_do(query, [target]) reports; above d where the score saturates"""
        v = self._ncache.get((query, target))
        if v is None:
            alen, score = C.c_uint64(0), C.c_uint64(0)
            v = int(self.lib.orc_nw_diff(self._wp[target], self._len[target], self._wp[query], self._len[query],
                                         self.mm, self.go, self.ge, C.byref(alen), C.byref(score)))
            if int(score.value) >= self.sat:
                v = max(v, self.d + 1)
            self._ncache[(query, target)] = v
        return v

    def batch(self, seeds, radii, lowest_unswarmed: int, first_generation: bool, ncb: bool):
        """-> (hits [(k, i, diff)] sorted by (k, i), comparisons, pairs); est[] and swarmed[] move on"""
        assert not first_generation or len(seeds) == 1
        lo = min(int(lowest_unswarmed), self.db.n)
        pool = (self._ids >= lo) & ~self.swarmed
        hits, comparisons, pairs = [], 0, 0
        new_est = self.est.copy()
        for k, (seed, radius) in enumerate(zip(seeds, radii) if pool.any() else ()):
            seed = int(seed)
            cand = pool & (self._ids != seed)
            if not first_generation:
                cand &= self.est <= int(radius) + self.d
            if not ncb:
                cand &= self.ab <= self.ab[seed]
            for i in np.flatnonzero(cand):
                i = int(i)
                comparisons += 1
                q = self.qgram_diff(seed, i)
                if first_generation:
                    new_est[i] = q
                if q <= self.d:
                    pairs += 1
                    df = self.nw_diff(seed, i)
                    if df <= self.d:
                        hits.append((k, i, df))
        self.est = new_est
        if first_generation:
            self.swarmed[int(seeds[0])] = True
        for _, i, _ in hits:
            self.swarmed[i] = True
        return hits, comparisons, pairs


def greedy(step, n: int):
    """The host's loop (swa_dn_cluster, after src/algo.cc:384-602) over `step(seeds, radii, lowest_unswarmed,
    first_generation, generation of the seeds) -> hits [(k, i, diff)] sorted by (k, i)`: a first-generation step per
    initial seed, then one batch per generation (at most 65535 sub-seeds a batch), a target found by several sub-seeds
    kept for the first in queue order.
    -> (swarms: one list of (id, generation, radius) each, in output order; links [(parent, child, diff, swarm number,
    generation)] in the order they are made)"""
    swarmed = np.zeros(n, dtype=bool)
    swarms, links = [], []
    for seed in range(n):
        if swarmed[seed]:
            continue
        no = len(swarms) + 1
        swarmed[seed] = True
        queue = [(seed, 0, 0)]
        for _, i, df in step([seed], [0], seed + 1, True, 0):
            swarmed[i] = True
            queue.append((i, 1, df))
            links.append((seed, i, df, no, 1))
        nxt = 1
        while nxt < len(queue):
            gen = queue[nxt][1]
            end = nxt
            while end < len(queue) and queue[end][1] == gen and end - nxt < 65535:
                end += 1
            subs = queue[nxt:end]
            hits = step([m[0] for m in subs], [m[2] for m in subs], seed + 1, False, gen)
            nxt = end
            for k, i, df in hits:
                if swarmed[i]:
                    continue
                swarmed[i] = True
                # the unseeded part of the queue stays ordered by generation, then id (src/algo.cc:205-219)
                pos = len(queue)
                while pos > nxt and queue[pos - 1][0] > i and queue[pos - 1][1] > gen:
                    pos -= 1
                queue.insert(pos, (i, gen + 1, subs[k][2] + df))
                links.append((subs[k][0], i, df, no, gen + 1))
        swarms.append(queue)
    return swarms, links


def model_greedy(model: ScanModel, ncb: bool = False):
    model.begin()
    return greedy(lambda seeds, radii, lo, first, gen: model.batch(seeds, radii, lo, first, ncb)[0], model.db.n)


def _plain(header: bytes) -> str:
    return header.decode().rsplit("_", 1)[0]


def swarms_text(db: S.Db, swarms) -> str:
    """-o"""
    return "".join(" ".join(db.headers[m[0]].decode() for m in sw) + "\n" for sw in swarms)


def structure_text(db: S.Db, links) -> str:
    """-i"""
    return "".join(f"{_plain(db.headers[p])}\t{_plain(db.headers[c])}\t{df}\t{no}\t{gen}\n" for p, c, df, no, gen in links)
