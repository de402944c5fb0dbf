"""Integer models of the d >= 2 alignment kernels for bands wider than a wave (align.hip).

generic_model restates k_align_generic: the band walked row by row, a cell's inputs taken from the previous row and the
previous column, unpacked values and plain branches.

wide_model restates the SCHEDULE of k_align_wide<K>: offset index x = lane * K + j stands for band offset x - 1 - W
(column - row); x = 0 and x > 2 W + 1 are guards that never compute; on anti-diagonal step s the offsets with
j & 1 == (s + 1 + W) & 1 are live and update in place; inside a lane the neighbours are the lane's own j - 1 / j + 1, and
two values cross the lanes: j = 0 takes the horizontal state of the lane below's j = K - 1 (live parity even), j = K - 1
the vertical state of the lane above's j = 0 (live parity odd); the first and the last lane have no such neighbour and
receive 0, which only a guard ever sees.  What travels between offsets is packed (score | counter << 16) as in the kernel.
The number of lanes is a parameter (the kernel has 64): a form needs 2 W + 3 <= lanes * K.

Sequences are strings or lists of small integers; both models return (diff, score, length) as swa_search_do reports
them: an infeasible pair (|length difference| > W) gives (sat, sat, 0), a saturated end score (sat, score, 0)."""

BIG = 0xFFFF


def band_of(mm: int, go: int, ge: int, d: int) -> tuple:
    """(W, saturation) as align_plan computes them"""
    sat = 65535 if d > min(255 // mm, 255 // (go + ge)) else 255
    return d * max(mm, go + ge) // ge + 1, sat


def wide_k(W: int, lanes: int = 64) -> int:
    """offsets a lane of the wide form: the smallest of 2, 4, 8 that holds band and guards; 0 when one offset a lane
    does, or none"""
    if 2 * W + 3 <= lanes:
        return 0
    return next((k for k in (2, 4, 8) if 2 * W + 3 <= lanes * k), 0)


def _sat_add(a, b, sat):
    return min(a + b, sat)


def generic_model(dseq, qseq, mm, go, ge, sat, W):
    dl, ql = len(dseq), len(qseq)
    delta = ql - dl
    if delta > W or -delta > W:
        return sat, sat, 0
    pH, pE, pAM, pAI, pLM, pLI = ([0] * ql for _ in range(6))
    endH, endAM, endLM = sat, BIG, 0
    for r in range(dl):
        c0, c1 = max(r - W, 0), min(r + W, ql - 1)
        if c0 == 0:
            top, adh, ldh = _sat_add(2 * go, (r + 2) * ge, sat), r + 1, r + 1
            hd, amd, lmd = (0 if r == 0 else _sat_add(go, r * ge, sat)), r, r
        else:
            top, adh, ldh = sat, BIG, 0
            hd, amd, lmd = pH[c0 - 1], pAM[c0 - 1], pLM[c0 - 1]
        for c in range(c0, c1 + 1):
            if r == 0:
                left, aiv, liv = _sat_add(2 * go, (c + 2) * ge, sat), c + 1, c + 1
                nhd, namd, nlmd = _sat_add(go, (c + 1) * ge, sat), c + 1, c + 1
            else:
                if c <= r - 1 + W:
                    left, aiv, liv = pE[c], pAI[c], pLI[c]
                else:
                    left, aiv, liv = sat, BIG, 0
                nhd, namd, nlmd = pH[c], pAM[c], pLM[c]
            mis = 1 if dseq[r] != qseq[c] else 0
            dp = _sat_add(hd, mm if mis else 0, sat)
            up = top < dp
            h = min(dp, top, left)
            lb = left == h
            d2, l2, t2 = _sat_add(h, go + ge, sat), _sat_add(left, ge, sat), _sat_add(top, ge, sat)
            eu, el = t2 < d2, l2 < d2
            if lb:
                am, lm = aiv + 1, liv + 1
            elif up:
                am, lm = adh + 1, ldh + 1
            else:
                am, lm = amd + mis, lmd + 1
            am = min(am, BIG)
            ai = min(aiv + 1 if el else am, BIG)
            ad = min(adh + 1 if eu else am, BIG)
            pH[c], pAM[c], pLM[c] = h, am, lm
            pE[c], pAI[c], pLI[c] = min(d2, l2), ai, (liv + 1 if el else lm)
            top, adh, ldh = min(d2, t2), ad, (ldh + 1 if eu else lm)
            hd, amd, lmd = nhd, namd, nlmd
            if r == dl - 1 and c == ql - 1:
                endH, endAM, endLM = h, am, lm
    if endH >= sat:
        return sat, endH, 0
    return endAM, endH, endLM


def live_parity(s: int, W: int) -> int:
    """the parity of j (= of the offset index) whose offsets compute a cell on step s"""
    return (s + 1 + W) & 1


def end_cell(dl: int, ql: int, W: int, K: int) -> tuple:
    """(lane, j) that holds the cell (dl - 1, ql - 1) of a feasible pair"""
    xe = ql - dl + W + 1
    return xe // K, xe % K


def wide_model(dseq, qseq, mm, go, ge, sat, W, K, lanes=64, trace=None):
    """trace (a list, optional) receives (s, parity, shuffle kind, cells computed) a step"""
    assert K in (2, 4, 8) and 2 * W + 3 <= lanes * K
    dl, ql = len(dseq), len(qseq)
    delta = ql - dl
    if delta > W or -delta > W or dl == 0 or ql == 0:
        return sat, sat, 0
    outside = sat | (BIG << 16)
    n = lanes * K
    H, AM, LM = [0] * n, [0] * n, [0] * n
    dn_pk, rt_pk, dn_len, rt_len = [outside] * n, [outside] * n, [0] * n, [0] * n
    last = dl + ql - 2
    for s in range(last + 1):
        par = live_parity(s, W)
        edge_h = 0 if s == 0 else _sat_add(go, s * ge, sat)
        edge_pk = _sat_add(2 * go, (s + 2) * ge, sat) | ((s + 1) << 16)
        # the two values that cross lanes (taken before the step writes anything)
        if par == 0:
            in_pk = [0] + [rt_pk[(ln - 1) * K + K - 1] for ln in range(1, lanes)]
            in_len = [0] + [rt_len[(ln - 1) * K + K - 1] for ln in range(1, lanes)]
        else:
            in_pk = [dn_pk[(ln + 1) * K] for ln in range(lanes - 1)] + [0]
            in_len = [dn_len[(ln + 1) * K] for ln in range(lanes - 1)] + [0]
        cells = 0
        for ln in range(lanes):
            for j in range(par, K, 2):
                x = ln * K + j
                if x < 1 or x > 2 * W + 1:                   # a guard
                    continue
                rs = s - (x - 1 - W)
                assert rs & 1 == 0
                r = rs >> 1
                c = s - r
                if not (0 <= r < dl and 0 <= c < ql):
                    continue
                cells += 1
                above_pk, above_len = (in_pk[ln], in_len[ln]) if j == K - 1 else (dn_pk[x + 1], dn_len[x + 1])
                below_pk, below_len = (in_pk[ln], in_len[ln]) if j == 0 else (rt_pk[x - 1], rt_len[x - 1])
                row0, col0 = r == 0, c == 0
                mis = 1 if dseq[r] != qseq[c] else 0
                hd = edge_h if row0 or col0 else H[x]
                amd = s if row0 or col0 else AM[x]
                lmd = s if row0 or col0 else LM[x]
                left_pk = edge_pk if row0 else above_pk
                top_pk = edge_pk if col0 else below_pk
                liv = s + 1 if row0 else above_len
                ldh = s + 1 if col0 else below_len
                left, aiv = left_pk & 0xFFFF, left_pk >> 16
                top, adh = top_pk & 0xFFFF, top_pk >> 16
                dp = _sat_add(hd, mm if mis else 0, sat)
                up = top < dp
                h = min(dp, top, left)
                lb = left == h
                d2, l2, t2 = _sat_add(h, go + ge, sat), _sat_add(left, ge, sat), _sat_add(top, ge, sat)
                eu, el = t2 < d2, l2 < d2
                am = aiv + 1 if lb else (adh + 1 if up else amd + mis)
                am = min(am, BIG)
                ai = min(aiv + 1 if el else am, BIG)
                ad = min(adh + 1 if eu else am, BIG)
                lm = liv + 1 if lb else (ldh + 1 if up else lmd + 1)
                H[x], AM[x], LM[x] = h, am, lm
                dn_pk[x], dn_len[x] = min(d2, l2) | (ai << 16), (liv + 1 if el else lm)
                rt_pk[x], rt_len[x] = min(d2, t2) | (ad << 16), (ldh + 1 if eu else lm)
        if trace is not None:
            trace.append((s, par, "below" if par == 0 else "above", cells))
    # the guards still hold the outside value
    for x in [0] + list(range(2 * W + 2, n)):
        assert dn_pk[x] == outside and rt_pk[x] == outside and dn_len[x] == 0 and rt_len[x] == 0
    ln, j = end_cell(dl, ql, W, K)
    xe = ln * K + j
    assert 1 <= xe <= 2 * W + 1
    if H[xe] >= sat:
        return sat, H[xe], 0
    return AM[xe], H[xe], LM[xe]
