// d1_fast.inc — seam B2 (--fastidious) by PAIRS (included once, by fastidious.hip alone, inside its anonymous namespace after
// group_join.inc, d1_common.inc and d1_probe.inc).
//
// What the reference computes (src/algod1.cc:339-552): for every heavy amplicon h, every
// microvariant v of h that the Bloom filter of the light microvariants lets through is
// materialised, every microvariant w of v is looked up among the light amplicons, and each verified
// light amplicon x is a graft candidate of h:  graft_cand[x] = min h, candidates += 1 per (h, v, x).
// generate_variants (src/variants.cc:184-249) lists DISTINCT sequences (tests/test_oracle_golden.py
// checks that), a Bloom false positive can never lead to a verified x, and "x is a microvariant of
// v" is symmetric — so with V1(s) = the set of microvariants of s
//
//     candidates    = sum over (h heavy, x light) of | V1(h) ∩ V1(x) |
//     graft_cand[x] = min { h heavy : V1(h) ∩ V1(x) not empty }          (non-empty <=> edit distance <= 2)
//     light / heavy variants = sum of |V1(s)| = 6 L + 4 + (number of homopolymer runs of s)
//
// The round-1 route followed the reference literally: 3 G random 8-byte atomics and 7 G random
// 8-byte reads over a 6 GB Bloom filter — TLB / latency bound at 1.5 % of the HBM roofline
// (profiles/r01).  Here the problem is turned into a JOIN:
//   1. groups: two sequences within two edits of each other share their first 32 nucleotides, or
//      their last 32, or — one edit in the first 32 nt, the other in the last 32 — the 32 nt at
//      positions 40..71 up to a shift of one (both at least kFastMinLen long).  Light amplicons are
//      grouped by those keys (the middle window at offsets 39, 40, 41), heavy amplicons join the
//      groups that exist (k_fg_light, k_fg_heavy; the table, the member lists and the work items are
//      the grouped join of group_join.inc);
//   2. k_fast_pairs: all (light, heavy) pairs of a group, each lane one pair: exact "edit distance
//      <= 2" by furthest-reaching diagonals with 32-nucleotide XOR + count-trailing-zeros extension
//      (Landau-Vishkin, 9 extensions at most); a pair that shares its prefix is only taken in the
//      prefix groups, one that shares its suffix not in the middle groups: every pair once;
//   3. k_fast_count: one wave per surviving pair: V1(x) into a wave-private LDS hash set, V1(h)
//      probed against it, matches verified on the materialised microvariants: |V1(h) ∩ V1(x)| exactly.
// Pairs with a sequence shorter than kFastMinLen keep the Bloom route (k_d1_flex / k_d1_probe<MODE 1>,
// restricted to them).  HBM traffic: the members' packed sequences, a few times, from L2.
// SWA_FAST_LONG=split adds the same division at the long end: k_fast_count's LDS set holds the microvariants of a
// sequence of up to cap = 1004 nt (swa_fast_cap), so where longer sequences exist the groups are made of the amplicons
// of kFastMinLen .. cap nt only (FastGroupArgs.max_len) and the pairs with a longer member keep the Bloom route too.
// SWA_FAST_LONG=pairs serves those sequences on the pair route instead: neither the join (k_fg_light / k_fg_heavy key 32-nt
// windows) nor k_fast_pairs (which walks packed words) has a length bound, and k_fast_count_sites_words counts a pair from
// two staged copies alone, so its cap is 327 584 nt (swa_fast_sites_cap); SWA_FAST_COUNT=sites runs that kernel in
// k_fast_count's place on 256 .. 1004 nt, for comparison.

constexpr uint32_t kFastMinLen = SWA_FAST_MIN_LEN;   // (112) both sequences at least this long => the pair route is complete
constexpr uint32_t kFastMid = 40;         // middle window of a heavy amplicon: [40, 72); light: 39, 40, 41
constexpr uint32_t kFastStride = 64;      // a group's tiles are dealt round-robin to at most this many items
using FastTiles = JoinBlocks<64, 64, kFastStride>;   // the join's work items (group_join.inc): 64 lights x 64 heavies a tile

// group key: TYPE 0 first 32 nt, 1 last 32 nt, 2 the 32 nt at `offset`
template <int TYPE>
__device__ __forceinline__ uint64_t fast_key(const uint64_t * seq, uint32_t len, uint32_t offset) {
  if (TYPE == 0) { return anchor_key(seq, len, 0, 0u, 0u); }
  if (TYPE == 1) { return anchor_key(seq, len, 1, 0u, 0u); }
  return mix64(window32(seq, offset) ^ 0xD1B54A32D192ED03ull) & 0x7FFFFFFFFFFFFFFFull;
}

struct FastGroupArgs {
  const uint64_t * seqs;
  const uint64_t * seq_off;
  const uint32_t * seqlen;
  const uint8_t * role;          // 0 light, 1 heavy (this shard), 2 not taking part
  uint32_t n;
  uint32_t max_len;              // longer amplicons join no group (0xFFFFFFFF: no bound)
  unsigned long long * keys;     // [asize]
  uint32_t * cnt_l, * cnt_h;     // [asize]
  uint64_t amask;
  uint32_t * lslot;              // [n * 3] (TYPE 2) / [n]
  uint32_t * hslot;              // [n]
  uint32_t * overflow;
};

// light amplicons create the groups
template <int TYPE>
__global__ __launch_bounds__(256) void k_fg_light(const FastGroupArgs a) {
  constexpr uint32_t NK = TYPE == 2 ? 3u : 1u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    uint32_t slots[NK];
#pragma unroll
    for (uint32_t j = 0; j < NK; ++j) { slots[j] = kEmpty; }
    const uint32_t len = a.seqlen[i];
    if (a.role[i] == 0u && len >= kFastMinLen && len <= a.max_len) {
      const uint64_t * s = a.seqs + a.seq_off[i];
      uint64_t key[NK];
#pragma unroll
      for (uint32_t j = 0; j < NK; ++j) {
        key[j] = fast_key<TYPE>(s, len, kFastMid - 1u + j);
        bool repeat = false;                                 // a window that reads the same at two offsets: one membership
        for (uint32_t q = 0; q < j; ++q) { repeat = repeat || key[q] == key[j]; }
        if (repeat) { continue; }
        slots[j] = join_claim(a.keys, a.amask, key[j]);
        if (slots[j] != kEmpty) { atomicAdd(&a.cnt_l[slots[j]], 1u); }
        else { *a.overflow = 1u; }
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < NK; ++j) { a.lslot[(uint64_t)i * NK + j] = slots[j]; }
  }
}

// heavy amplicons join the groups that exist
template <int TYPE>
__global__ __launch_bounds__(256) void k_fg_heavy(const FastGroupArgs a) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    uint32_t slot = kEmpty;
    const uint32_t len = a.seqlen[i];
    if (a.role[i] == 1u && len >= kFastMinLen && len <= a.max_len) {
      slot = join_find(a.keys, a.amask, fast_key<TYPE>(a.seqs + a.seq_off[i], len, kFastMid));
      if (slot != kEmpty) { atomicAdd(&a.cnt_h[slot], 1u); }
    }
    a.hslot[i] = slot;
  }
}

// ---- exact "edit distance <= 2" ---------------------------------------------------------------
// longest common extension of A[i..m) and B[j..n), 32 nucleotides per step
__device__ __forceinline__ int fast_lce(const uint64_t * A, int i, int m, const uint64_t * B, int j, int n) {
  const int lim = min(m - i, n - j);
  int t = 0;
  while (t < lim) {
    const uint64_t d = window32(A, (uint32_t)(i + t)) ^ window32(B, (uint32_t)(j + t));
    if (d != 0ull) { return min(t + (__builtin_ctzll(d) >> 1), lim); }
    t += 32;
  }
  return lim;
}

// furthest-reaching rows on the diagonals j - i = k after e = 0, 1, 2 edits (Landau-Vishkin); only the
// diagonal n - m matters in the end.  -1 = unreachable.
__device__ __forceinline__ bool within_two_edits(const uint64_t * A, int m, const uint64_t * B, int n) {
  const int dk = n - m;
  if (dk > 2 || dk < -2) { return false; }
  const int l0 = fast_lce(A, 0, m, B, 0, n);                  // e = 0, diagonal 0
  if (dk == 0 && l0 >= m) { return true; }
  int l1[5];                                                  // e = 1, diagonals -2 .. 2 (index k + 2)
  l1[0] = -1; l1[4] = -1;
  // substitution on 0; insertion 0 -> +1 (row stays); deletion 0 -> -1 (row advances)
  l1[2] = (l0 + 1 <= m && l0 + 1 <= n) ? l0 + 1 + fast_lce(A, l0 + 1, m, B, l0 + 1, n) : -1;
  l1[3] = (l0 + 1 <= n) ? l0 + fast_lce(A, l0, m, B, l0 + 1, n) : -1;
  l1[1] = (l0 + 1 <= m) ? l0 + 1 + fast_lce(A, l0 + 1, m, B, l0, n) : -1;
  if (dk >= -1 && dk <= 1 && l1[dk + 2] >= m) { return true; }
  // e = 2 on diagonal dk
  int best = -1;
  const int same = l1[dk + 2];
  if (same >= 0 && same + 1 <= m && same + 1 + dk <= n) { best = same + 1; }
  if (dk - 1 >= -2) { const int below = l1[dk + 1]; if (below >= 0 && below + dk <= n && below > best) { best = below; } }
  if (dk + 1 <= 2) { const int above = l1[dk + 3]; if (above >= 0 && above + 1 <= m && above + 1 > best) { best = above + 1; } }
  if (best < 0) { return false; }
  return best + fast_lce(A, best, m, B, best + dk, n) >= m;
}

struct FastPairArgs {
  const uint64_t * seqs;
  const uint64_t * seq_off;
  const uint32_t * seqlen;
  const uint32_t * members;
  const join_item * items;
  const uint32_t * item_count;
  uint32_t item_cap;
  unsigned long long * pairs;          // (heavy << 32) | light
  unsigned long long * pair_counter;
  uint64_t pair_cap;
  const uint4 * lines;                 // k_fast_pairs_lines: the amplicon lines (d1_stream.inc),
  uint32_t line_quads;                 // 16-byte quads each
};

// all (light, heavy) pairs of a group, one pair per lane and turn
template <int TYPE>
__global__ __launch_bounds__(kThreads) void k_fast_pairs(const FastPairArgs a) {
  __shared__ unsigned long long stage_rows[kWaves][kPairStage];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  PairStage stage(stage_rows, a.pairs, a.pair_counter, a.pair_cap);
  const uint32_t nitems = min(*a.item_count, a.item_cap);
  const uint32_t nwaves = gridDim.x * kWaves;
  for (uint32_t it = blockIdx.x * kWaves + wave; it < nitems; it += nwaves) {
    const join_item item = a.items[it];
    const uint64_t tiles_h = ((uint64_t)item.nb + 63) / 64;
    const uint64_t ntiles = (((uint64_t)item.na + 63) / 64) * tiles_h;
    const uint32_t * lights = a.members + item.begin;
    const uint32_t * heavies = lights + item.na;
    for (uint64_t tile = item.tile; tile < ntiles; tile += kFastStride) {
      const uint32_t l0 = (uint32_t)(tile / tiles_h) * 64u, h0 = (uint32_t)(tile % tiles_h) * 64u;
      const uint32_t ih = h0 + (uint32_t)lane;
      const bool have_h = ih < item.nb;
      const uint32_t h = have_h ? heavies[ih] : 0u;
      const int lh = have_h ? (int)a.seqlen[h] : 0;
      const uint64_t * sh = a.seqs + (have_h ? a.seq_off[h] : 0ull);
      for (uint32_t il = l0; il < min(l0 + 64u, item.na); ++il) {
        bool take = false;
        const uint32_t x = lights[il];
        if (have_h) {
          const int lx = (int)a.seqlen[x];
          const int dl = lx - lh;
          if (dl >= -2 && dl <= 2) {
            const uint64_t * sx = a.seqs + a.seq_off[x];
            // every pair in exactly one kind of group: prefix groups take all their pairs, suffix groups
            // the pairs whose first 32 nt differ, middle groups those that share neither end
            // (decided on the nucleotides themselves, not on the group keys, so that a key collision cannot
            // put a pair into two classes)
            const bool same_prefix = sx[0] == sh[0];
            bool mine = TYPE == 0 ? same_prefix : !same_prefix;
            if (TYPE >= 1 && mine) {
              const bool same_suffix = window32(sx, (uint32_t)lx - 32u) == window32(sh, (uint32_t)lh - 32u);
              mine = TYPE == 1 ? same_suffix : !same_suffix;
            }
            take = mine && within_two_edits(sh, lh, sx, lx);
          }
        }
        stage.push(take, ((unsigned long long)h << 32) | x);
      }
    }
  }
  stage.finish();
}

// ---- the same on amplicon lines (round 3) -------------------------------------------------------------------------------
// k_fast_pairs above walks the packed sequences in HBM word by word, one lane per heavy amplicon of a 64 x 64 tile: most
// groups hold one to three light and one to three heavy amplicons, so a wave ran with a few lanes, each chasing pointers.
// Here (sequences up to 32 W nucleotides, the amplicon lines of d1_stream.inc) both sequences of a pair sit in registers,
// the five diagonals of Landau-Vishkin are difference masks (A xor B shifted by k nucleotides) searched with
// count-trailing-zeros, and the pairs of 64 consecutive groups are dealt to the lanes one pair per lane (prefix sums of
// nl x nh in LDS, a 6-step search per lane): every lane works whatever the group sizes.
template <int W>
__device__ __forceinline__ uint64_t reg_window(const uint64_t (&w)[W], uint32_t pos) {
  const uint32_t k = pos >> 5, sh = (pos & 31u) << 1;
  uint64_t lo = 0ull, hi = 0ull;
#pragma unroll
  for (int j = 0; j < W; ++j) { lo = (uint32_t)j == k ? w[j] : lo; hi = (uint32_t)j == k + 1u ? w[j] : hi; }
  return sh != 0u ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

// D[p] != 0  <=>  A[p] != B[p + k]   (k = -2 .. 2; positions of A; beyond the ends: whatever the zero padding gives)
template <int W>
__device__ __forceinline__ void diagonal_mask(const uint64_t (&A)[W], const uint64_t (&B)[W], int k, uint64_t (&D)[W]) {
  const uint32_t s = 2u * (uint32_t)(k < 0 ? -k : k);
#pragma unroll
  for (int w = 0; w < W; ++w) {
    uint64_t b = B[w];
    if (k > 0) { b = (B[w] >> s) | ((w + 1 < W ? B[w + 1 < W ? w + 1 : w] : 0ull) << (64u - s)); }
    else if (k < 0) { b = (B[w] << s) | ((w > 0 ? B[w > 0 ? w - 1 : 0] : 0ull) >> (64u - s)); }
    D[w] = A[w] ^ b;
  }
}

// first position >= from with a set difference, 32 W if none
template <int W>
__device__ __forceinline__ int first_difference(const uint64_t (&D)[W], int from) {
  int pos = 32 * W;
#pragma unroll
  for (int w = W - 1; w >= 0; --w) {
    const int rel = from - 32 * w;
    const uint64_t mask = rel <= 0 ? ~0ull : (rel >= 32 ? 0ull : ~0ull << (2 * rel));
    const uint64_t t = D[w] & mask;
    pos = t != 0ull ? 32 * w + (__builtin_ctzll(t) >> 1) : pos;
  }
  return pos;
}

// rows common to A[i..m) and B[i + k..n) from row i on
template <int W>
__device__ __forceinline__ int reg_lce(const uint64_t (&D)[W], int i, int k, int m, int n) {
  const int lim = min(m - i, n - i - k);
  return min(first_difference<W>(D, i) - i, lim);
}

// = within_two_edits(A, m, B, n) with both sequences in registers (zero padded to W words)
template <int W>
__device__ __forceinline__ bool within_two_edits_reg(const uint64_t (&A)[W], int m, const uint64_t (&B)[W], int n) {
  const int dk = n - m;
  if (dk > 2 || dk < -2) { return false; }
  uint64_t D0[W], Dp[W], Dm[W];
  diagonal_mask<W>(A, B, 0, D0);
  diagonal_mask<W>(A, B, 1, Dp);
  diagonal_mask<W>(A, B, -1, Dm);
  const int l0 = reg_lce<W>(D0, 0, 0, m, n);
  if (dk == 0 && l0 >= m) { return true; }
  int l1[5];
  l1[0] = -1; l1[4] = -1;
  l1[2] = (l0 + 1 <= m && l0 + 1 <= n) ? l0 + 1 + reg_lce<W>(D0, l0 + 1, 0, m, n) : -1;
  l1[3] = (l0 + 1 <= n) ? l0 + reg_lce<W>(Dp, l0, 1, m, n) : -1;
  l1[1] = (l0 + 1 <= m) ? l0 + 1 + reg_lce<W>(Dm, l0 + 1, -1, m, n) : -1;
  if (dk >= -1 && dk <= 1 && l1[dk + 2] >= m) { return true; }
  int best = -1;
  const int same = dk == 0 ? l1[2] : (dk == 1 ? l1[3] : (dk == -1 ? l1[1] : -1));
  const int below = dk == 1 ? l1[2] : (dk == 0 ? l1[1] : (dk == 2 ? l1[3] : -1));      // diagonal dk - 1
  const int above = dk == -1 ? l1[2] : (dk == 0 ? l1[3] : (dk == -2 ? l1[1] : -1));    // diagonal dk + 1
  if (same >= 0 && same + 1 <= m && same + 1 + dk <= n) { best = same + 1; }
  if (below >= 0 && below + dk <= n && below > best) { best = below; }
  if (above >= 0 && above + 1 <= m && above + 1 > best) { best = above + 1; }
  if (best < 0) { return false; }
  if (dk == 0) { return best + reg_lce<W>(D0, best, 0, m, n) >= m; }
  if (dk == 1) { return best + reg_lce<W>(Dp, best, 1, m, n) >= m; }
  if (dk == -1) { return best + reg_lce<W>(Dm, best, -1, m, n) >= m; }
  uint64_t D2[W];
  diagonal_mask<W>(A, B, dk, D2);
  return best + reg_lce<W>(D2, best, dk, m, n) >= m;
}

// is this pair (heavy H, light X) the business of the groups of this TYPE, and within two edits?
template <int TYPE, int W>
__device__ __forceinline__ bool fast_pair_test(const uint64_t (&Hw)[W], int lh, const uint64_t (&Xw)[W], int lx) {
  const int dl = lx - lh;
  if (dl < -2 || dl > 2) { return false; }
  const bool same_prefix = Xw[0] == Hw[0];
  bool mine = TYPE == 0 ? same_prefix : !same_prefix;
  if (TYPE >= 1 && mine) {
    const bool same_suffix = reg_window<W>(Xw, (uint32_t)lx - 32u) == reg_window<W>(Hw, (uint32_t)lh - 32u);
    mine = TYPE == 1 ? same_suffix : !same_suffix;
  }
  return mine && within_two_edits_reg<W>(Hw, lh, Xw, lx);
}

template <int TYPE, int W>
__global__ __launch_bounds__(kThreads) void k_fast_pairs_lines(const FastPairArgs a) {
  __shared__ unsigned long long stage_rows[kWaves][kPairStage];
  __shared__ uint32_t psum_all[kWaves][64], begin_all[kWaves][64], nl_all[kWaves][64], nh_all[kWaves][64], tile_all[kWaves][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t * psum = psum_all[wave], * ibegin = begin_all[wave], * inl = nl_all[wave], * inh = nh_all[wave], * itile = tile_all[wave];
  PairStage stage(stage_rows, a.pairs, a.pair_counter, a.pair_cap);
  const uint32_t nitems = min(*a.item_count, a.item_cap);
  const uint32_t nwaves = gridDim.x * kWaves;
  for (uint32_t chunk = (blockIdx.x * kWaves + wave) * 64u; chunk < nitems; chunk += nwaves * 64u) {
    const uint32_t idx = chunk + (uint32_t)lane;
    join_item item{0u, 0u, 0u, 0u};
    if (idx < nitems) { item = a.items[idx]; }
    const bool small = idx < nitems && item.na <= 64u && item.nb <= 64u;      // one tile: all its pairs dealt to lanes
    const bool large = idx < nitems && !small;
    uint32_t incl = small ? item.na * item.nb : 0u;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, (unsigned)d, 64); if (lane >= d) { incl += up; } }
    wave_lds_sync();                                            // (the previous chunk's tables are no longer read)
    psum[lane] = incl; ibegin[lane] = item.begin; inl[lane] = item.na; inh[lane] = item.nb; itile[lane] = item.tile;
    wave_lds_sync();
    const uint32_t total = psum[63];
    for (uint32_t r = 0; r < total; r += 64u) {
      const uint32_t slot = r + (uint32_t)lane;
      const bool valid = slot < total;
      uint32_t j = 0;                                           // first group whose inclusive sum exceeds the slot
#pragma unroll
      for (uint32_t step = 32u; step != 0u; step >>= 1) { if (psum[j + step - 1u] <= slot) { j += step; } }
      j = valid ? j : 0u;
      const uint32_t local = valid ? slot - (j != 0u ? psum[j - 1u] : 0u) : 0u;
      const uint32_t nh = max(inh[j], 1u), nl = inl[j];
      const uint32_t il = local / nh, ih = local - il * nh;
      bool take = false;
      uint32_t x = 0, h = 0;
      if (valid) {
        x = a.members[ibegin[j] + il];
        h = a.members[ibegin[j] + nl + ih];
        uint64_t Xw[W], Hw[W];
        uint32_t lx, lh, rank;
        line_fetch<W>(a.lines, a.line_quads, x, Xw, lx, rank);
        line_fetch<W>(a.lines, a.line_quads, h, Hw, lh, rank);
        take = fast_pair_test<TYPE, W>(Hw, (int)lh, Xw, (int)lx);
      }
      stage.push(take, ((unsigned long long)h << 32) | x);
    }
    // groups of more than one tile: lane = heavy amplicon of the tile, the light ones in turn (as k_fast_pairs)
    uint64_t todo = __ballot(large);
    while (todo != 0ull) {
      const int j = __builtin_ctzll(todo);
      todo &= todo - 1ull;
      const uint32_t nl = inl[j], nh = inh[j], begin = ibegin[j];
      const uint64_t tiles_h = ((uint64_t)nh + 63) / 64;
      const uint64_t ntiles = (((uint64_t)nl + 63) / 64) * tiles_h;
      const uint32_t * lights = a.members + begin;
      const uint32_t * heavies = lights + nl;
      for (uint64_t tile = itile[j]; tile < ntiles; tile += kFastStride) {
        const uint32_t l0 = (uint32_t)(tile / tiles_h) * 64u, h0 = (uint32_t)(tile % tiles_h) * 64u;
        const uint32_t ih = h0 + (uint32_t)lane;
        const bool have_h = ih < nh;
        const uint32_t h = have_h ? heavies[ih] : 0u;
        uint64_t Hw[W];
        uint32_t lh = 0, rank;
        if (have_h) { line_fetch<W>(a.lines, a.line_quads, h, Hw, lh, rank); }
        else {
#pragma unroll
          for (int w = 0; w < W; ++w) { Hw[w] = 0ull; }
        }
        for (uint32_t il = l0; il < min(l0 + 64u, nl); ++il) {
          const uint32_t x = lights[il];
          uint64_t Xw[W];
          uint32_t lx;
          line_fetch<W>(a.lines, a.line_quads, x, Xw, lx, rank);
          const bool take = have_h && fast_pair_test<TYPE, W>(Hw, (int)lh, Xw, (int)lx);
          stage.push(take, ((unsigned long long)h << 32) | x);
        }
      }
    }
  }
  stage.finish();
}

// ---- |V1(h) ∩ V1(x)| of every pair -------------------------------------------------------------
struct FastCountArgs {
  const uint64_t * seqs;
  const uint64_t * seq_off;
  const uint32_t * seqlen;
  const uint64_t * zobrist;
  uint32_t zlen, maxwords;
  uint32_t slots;                      // per-wave LDS set, power of two >= 1.5 * (7 * longest + 4)
  const unsigned long long * pairs;
  uint64_t npairs;
  uint32_t * graft;
  unsigned long long * cand_counter;
};

// One wave per pair.  Set entry = upper 44 bits of the microvariant's hash | 20-bit edit code (type |
// base << 2 | position << 4), addressed by the low hash bits; a tag match is confirmed on the two
// materialised microvariants (swa_variant_word), so the count never depends on the hash function.
__global__ void k_fast_count(const FastCountArgs a) {
  extern __shared__ uint64_t lds[];
  const int waves = (int)(blockDim.x >> 6);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint64_t * zob = lds;
  const uint32_t seed_words = a.maxwords + 3u;
  uint64_t * wbase = lds + 4u * a.zlen + (size_t)wave * (2u * seed_words + a.slots);
  uint64_t * swx = wbase;
  uint64_t * swh = wbase + seed_words;
  unsigned long long * set = reinterpret_cast<unsigned long long *>(wbase + 2u * seed_words);
  for (uint32_t i = threadIdx.x; i < 4u * a.zlen; i += blockDim.x) { zob[i] = a.zobrist[i]; }
  __syncthreads();
  const uint32_t mask = a.slots - 1u;
  unsigned long long total = 0;
  const uint64_t nwaves = (uint64_t)gridDim.x * waves;
  for (uint64_t k = (uint64_t)blockIdx.x * waves + wave; k < a.npairs; k += nwaves) {
    const unsigned long long pr = a.pairs[k];
    const uint32_t h = (uint32_t)(pr >> 32), x = (uint32_t)pr;
    const uint32_t lx = a.seqlen[x], lh = a.seqlen[h];
    const uint32_t nwx = (lx + 31u) >> 5, nwh = (lh + 31u) >> 5;
    const uint64_t * gx = a.seqs + a.seq_off[x];
    const uint64_t * gh = a.seqs + a.seq_off[h];
    for (uint32_t w = lane; w < seed_words; w += 64u) { swx[w] = (w < nwx) ? gx[w] : 0ull; swh[w] = (w < nwh) ? gh[w] : 0ull; }
    for (uint32_t i = lane; i < a.slots; i += 64u) { set[i] = kKeyEmpty; }
    wave_lds_sync();
    (void)enumerate_variants(swx, lx, zob, lane, [&](const Slots & s) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (s.ok[i]) {
          const unsigned long long entry = (s.hs[i] & ~0xFFFFFull) | s.code[i];
          uint32_t idx = (uint32_t)s.hs[i] & mask;
          while (atomicCAS(&set[idx], kKeyEmpty, entry) != kKeyEmpty) { idx = (idx + 1u) & mask; }
        }
      }
    });
    wave_lds_sync();
    uint32_t found = 0;
    (void)enumerate_variants(swh, lh, zob, lane, [&](const Slots & s) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (s.ok[i]) {
          uint32_t idx = (uint32_t)s.hs[i] & mask;
          for (;;) {
            const unsigned long long e = set[idx];
            if (e == kKeyEmpty) { break; }
            if (((e ^ s.hs[i]) >> 20) == 0ull) {
              // the same sequence?  (microvariant of x by edit e, microvariant of h by edit s.code[i])
              const uint32_t cx = (uint32_t)e & 0xFFFFFu, ch = s.code[i];
              const uint32_t tx = cx & 3u, th = ch & 3u;
              const uint32_t vlx = tx == 0u ? lx : (tx == 1u ? lx - 1u : lx + 1u);
              const uint32_t vlh = th == 0u ? lh : (th == 1u ? lh - 1u : lh + 1u);
              bool same = vlx == vlh;
              const uint32_t vnw = (vlx + 31u) >> 5;
              for (uint32_t w = 0; same && w < vnw; ++w) {
                same = swa_variant_word(swx, nwx, tx, cx >> 4, (cx >> 2) & 3u, w) == swa_variant_word(swh, nwh, th, ch >> 4, (ch >> 2) & 3u, w);
              }
              if (same) { ++found; }
            }
            idx = (idx + 1u) & mask;
          }
        }
      }
    });
    for (int o = 32; o > 0; o >>= 1) { found += (uint32_t)__shfl_xor((int)found, o, 64); }
    if (found != 0u) {
      if (lane == 0) { atomicMin(&a.graft[x], h); }
      total += found;
    }
    wave_lds_sync();
  }
  if (lane == 0 && total != 0ull) { atomicAdd(a.cand_counter, total); }
}

// ---- |V1(h) ∩ V1(x)| without enumerating everything (sequences up to 32 W nucleotides) ---------------------
// A microvariant v of h can only be a microvariant of x as well if its edit acts where h and x differ: between
// the first mismatch of the two (P) and the last mismatch of the end-aligned comparison (E) — and, because
// generate_variants files an edit inside a homopolymer run under the run's FIRST position, from the start of the run
// that touches that interval.  (Checked by brute force against the set intersection, random and low-complexity
// and periodic sequences: tests/test_fastidious_identity.py.)  So only the canonical positions
//     [ runstart(h, min(P, E) - 1) - 1 ,  max(P, E) + 1 ]
// of h are expanded: lane = (position, slot), the microvariant is materialised in registers (swa_variant_word) and
// compared with x by an exact one-edit test on registers (one_edit_apart).  No hashes, no LDS set.

// exactly one edit apart, on packed 64-bit words held in registers (a microvariant built in registers against a sequence;
// the pair kernels of the d = 1 step, d1_anchor.inc, use lcp + lcs on staged records instead)
template <int W>
__device__ __forceinline__ bool one_edit_apart(const uint64_t (&sw)[W], uint32_t slen, const uint64_t (&w)[W], uint32_t len) {
  // L = the longer of the two (either, when the lengths are equal), S = the other (n nucleotides).
  //   lengths differ by one: one edit apart <=> there is a p with S[0, p) = L[0, p) and S[p, n) = L[p + 1, n + 1).  The
  //     largest candidate p is the first mismatch of S against L (lcp); it works iff the last mismatch of S against L
  //     shifted down by one nucleotide (hb) lies below it.  Zero padding behind both sequences makes positions >= n
  //     compare equal in the shifted comparison.
  //   equal lengths: one substitution <=> the first and the last mismatch of S against L are the same position.
  // One code path for both (the shift is a per-lane select): lanes of a wave hold members of different lengths.
  const int dl = (int)len - (int)slen;
  const bool mine_longer = dl == 1, shifted = dl != 0;
  auto longer = [&](int k) { return mine_longer ? w[k] : sw[k]; };
  auto shorter = [&](int k) { return mine_longer ? sw[k] : w[k]; };
  int lcp = 0x7fffffff, hb = -1;
#pragma unroll
  for (int k = W - 1; k >= 0; --k) {
    const uint64_t a = shorter(k) ^ longer(k);
    lcp = a != 0ull ? 32 * k + (__builtin_ctzll(a) >> 1) : lcp;
  }
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const uint64_t next = k + 1 < W ? longer(k + 1 < W ? k + 1 : k) : 0ull;
    const uint64_t other = shifted ? ((longer(k) >> 2) | (next << 62)) : longer(k);
    const uint64_t b = shorter(k) ^ other;
    hb = b != 0ull ? 32 * k + ((63 - __builtin_clzll(b)) >> 1) : hb;
  }
  return (dl >= -1 && dl <= 1) && (shifted ? hb < lcp : hb == lcp);
}

template <int W>
__global__ __launch_bounds__(kThreads) void k_fast_count_sites(const FastCountArgs a) {
  __shared__ uint64_t hw_all[kWaves][W + 2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint64_t * hw = hw_all[wave];
  unsigned long long total = 0;
  const uint64_t nwaves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t k = (uint64_t)blockIdx.x * kWaves + wave; k < a.npairs; k += nwaves) {
    const unsigned long long pr = a.pairs[k];
    const uint32_t h = (uint32_t)(pr >> 32), x = (uint32_t)pr;
    const int lh = (int)a.seqlen[h], lx = (int)a.seqlen[x];
    const uint32_t nwh = ((uint32_t)lh + 31u) >> 5, nwx = ((uint32_t)lx + 31u) >> 5;
    const uint64_t hv = (uint32_t)lane < nwh && lane < W ? a.seqs[a.seq_off[h] + (uint32_t)lane] : 0ull;
    const uint64_t xv = (uint32_t)lane < nwx && lane < W ? a.seqs[a.seq_off[x] + (uint32_t)lane] : 0ull;
    uint64_t Hw[W], Xw[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { Hw[i] = lane_value64(hv, i); Xw[i] = lane_value64(xv, i); }
    wave_lds_sync();                                          // (the previous pair's words are no longer read)
    if (lane < W + 2) { hw[lane] = lane < W ? hv : 0ull; }
    wave_lds_sync();
    // P: first position where h and x differ;  E: last position of h that differs from x aligned at the ends
    const int dl = lx - lh;                                   // -2 .. 2
    int P = min(lh, lx), E = -1;
#pragma unroll
    for (int i = W - 1; i >= 0; --i) {
      const uint64_t d = Hw[i] ^ Xw[i];
      P = d != 0ull ? min(32 * i + (__builtin_ctzll(d) >> 1), P) : P;
    }
#pragma unroll
    for (int i = 0; i < W; ++i) {
      // x moved by dl nucleotides so that its end meets h's end: xs[q] = x[q + dl]
      const uint64_t lo = i > 0 ? Xw[i - 1] : 0ull, hi = i + 1 < W ? Xw[i + 1 < W ? i + 1 : i] : 0ull;
      uint64_t xs = Xw[i];
      if (dl == 1) { xs = (Xw[i] >> 2) | (hi << 62); }
      else if (dl == 2) { xs = (Xw[i] >> 4) | (hi << 60); }
      else if (dl == -1) { xs = (Xw[i] << 2) | (lo >> 62); }
      else if (dl == -2) { xs = (Xw[i] << 4) | (lo >> 60); }
      uint64_t d = Hw[i] ^ xs;
      if (i == 0 && dl < 0) { d |= dl == -1 ? 3ull : 15ull; }            // positions of h before x's first nucleotide: differences
      E = d != 0ull ? 32 * i + ((63 - __builtin_clzll(d)) >> 1) : E;
    }
    P = min(P, lh - 1);
    E = min(max(E, 0), lh - 1);
    const int first = min(P, E), last = max(P, E);
    int q = max(first - 1, 0);                                // start of the run that touches the interval
    while (q > 0 && swa_nt(hw, (uint32_t)q - 1u) == swa_nt(hw, (uint32_t)q)) { --q; }
    const int lo_pos = max(q - 1, 0), hi_pos = min(last + 1, lh);
    // Two edits far apart (P < E and the two neighbourhoods do not touch): a common microvariant undoes one of them, so its
    // edit sits next to P or next to E — [lo_pos, P + 1] and [runstart(E - 1) - 1, hi_pos] — never in between
    // (tests/test_fastidious_identity.py checks both forms by brute force).  Typically 8 positions instead of E - P.
    int q2 = max(last - 1, 0);
    while (q2 > 0 && swa_nt(hw, (uint32_t)q2 - 1u) == swa_nt(hw, (uint32_t)q2)) { --q2; }
    const int lo_b = max(q2 - 1, 0), hi_a = min(first + 1, lh);
    const bool two_windows = P <= E && lo_b > hi_a;
    const int n_a = two_windows ? hi_a - lo_pos + 1 : hi_pos - lo_pos + 1;
    const int slots = (n_a + (two_windows ? hi_pos - lo_b + 1 : 0)) * 8;
    uint32_t found = 0;
    for (int t0 = 0; t0 < slots; t0 += 64) {
      const int t = t0 + lane;
      const int at = t >> 3;
      const uint32_t p = (uint32_t)(at < n_a ? lo_pos + at : lo_b + (at - n_a));
      const uint32_t slot = (uint32_t)t & 7u;
      bool ok = t < slots;
      const uint32_t prevc = (ok && p >= 1u) ? swa_nt(hw, p - 1u) : 4u;
      const uint32_t c = (ok && p < (uint32_t)lh) ? swa_nt(hw, p) : 4u;
      uint32_t type, base;
      if (slot < 4u) { type = 2u; base = slot; ok = ok && (p == 0u || base != prevc); }                       // insertion before p
      else if (slot < 7u) { type = 0u; const uint32_t t3 = slot - 4u; base = t3 < c ? t3 : t3 + 1u; ok = ok && p < (uint32_t)lh; }
      else { type = 1u; base = 0u; ok = ok && p < (uint32_t)lh && (p == 0u || c != prevc); }                  // deletion, once per run
      bool near = false;
      if (ok) {
        uint64_t v[W];
#pragma unroll
        for (int w = 0; w < W; ++w) { v[w] = swa_variant_word(hw, nwh, type, p, base, (uint32_t)w); }
        const uint32_t lv = type == 0u ? (uint32_t)lh : (type == 1u ? (uint32_t)lh - 1u : (uint32_t)lh + 1u);
        near = one_edit_apart<W>(Xw, (uint32_t)lx, v, lv);
      }
      found += (uint32_t)__popcll(__ballot(near));
    }
    if (found != 0u) {
      if (lane == 0) { atomicMin(&a.graft[x], h); }
      total += found;
    }
  }
  if (lane == 0 && total != 0ull) { atomicAdd(a.cand_counter, total); }
}

// ---- the same rule on words staged in LDS, any length (SWA_FAST_LONG=pairs, SWA_FAST_COUNT=sites) ---------------------------
// k_fast_count_sites keeps both sequences in W register words and so ends at 255 nt; k_fast_count's set ends at 1004.  Here
// h and x are staged per wave in dynamic LDS (maxwords + 3 words each, zero behind the sequence: no set, no Zobrist table),
// the word count is a run-time value and nothing is materialised:
//   P, E      the words dealt to the lanes in strides of 64, min / max over the wave; the end alignment's shifted word of x
//             takes its neighbour word from LDS;
//   positions exactly those of k_fast_count_sites, both forms; a homopolymer run may span many words: the walk back is
//             uniform over the wave and ends at position 0 at the latest;
//   the test  lane = (position, slot); the microvariant's words come from swa_variant_word as the loops ask for them, and
//             "v is one edit from x" is one_edit_apart (above) with a run-time word count: lcp = the first mismatch
//             of the forward words, hb = the last mismatch of the shorter against the longer moved down by one nucleotide
//             (equal lengths: unmoved); one edit apart <=> hb < lcp (lengths n, n + 1), hb == lcp (equal lengths).  Each loop
//             stops at the word that holds its mismatch, which IS lcp / hb: no word is skipped on an assumption.
// tests/test_fastidious_long_identity.py restates all of it on 64-bit words and checks it against the set intersection.
template <int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_fast_count_sites_words(const FastCountArgs a) {
  extern __shared__ uint64_t lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t seed_words = a.maxwords + 3u;
  uint64_t * swx = lds + (size_t)wave * 2u * seed_words;
  uint64_t * swh = swx + seed_words;
  unsigned long long total = 0;
  const uint64_t nwaves = (uint64_t)gridDim.x * WAVES;
  for (uint64_t k = (uint64_t)blockIdx.x * WAVES + wave; k < a.npairs; k += nwaves) {
    const unsigned long long pr = a.pairs[k];
    const uint32_t h = (uint32_t)(pr >> 32), x = (uint32_t)pr;
    const int lh = (int)a.seqlen[h], lx = (int)a.seqlen[x];
    const uint32_t nwh = ((uint32_t)lh + 31u) >> 5, nwx = ((uint32_t)lx + 31u) >> 5;
    const uint32_t nmax = max(nwh, nwx);                      // <= maxwords
    const uint64_t * gx = a.seqs + a.seq_off[x];
    const uint64_t * gh = a.seqs + a.seq_off[h];
    wave_lds_sync();                                          // (the previous pair's words are no longer read)
    // every index read below is < nmax + 3 <= seed_words
    for (uint32_t w = (uint32_t)lane; w < nmax + 3u; w += 64u) { swx[w] = w < nwx ? gx[w] : 0ull; swh[w] = w < nwh ? gh[w] : 0ull; }
    wave_lds_sync();
    // P: first position where h and x differ;  E: last position of h that differs from x aligned at the ends
    const int dl = lx - lh;                                   // -2 .. 2
    int P = min(lh, lx), E = -1;
    for (uint32_t i = (uint32_t)lane; i < nmax; i += 64u) {
      const uint64_t hv = swh[i], xv = swx[i];
      const uint64_t d0 = hv ^ xv;
      if (d0 != 0ull) { P = min(P, (int)(32u * i) + (__builtin_ctzll(d0) >> 1)); }
      // x moved by dl nucleotides so that its end meets h's end: xs[q] = x[q + dl]
      const uint64_t lo = i > 0u ? swx[i - 1u] : 0ull, hi = swx[i + 1u];
      uint64_t xs = xv;
      if (dl == 1) { xs = (xv >> 2) | (hi << 62); }
      else if (dl == 2) { xs = (xv >> 4) | (hi << 60); }
      else if (dl == -1) { xs = (xv << 2) | (lo >> 62); }
      else if (dl == -2) { xs = (xv << 4) | (lo >> 60); }
      uint64_t d = hv ^ xs;
      if (i == 0u && dl < 0) { d |= dl == -1 ? 3ull : 15ull; }             // positions of h before x's first nucleotide: differences
      if (d != 0ull) { E = max(E, (int)(32u * i) + ((63 - __builtin_clzll(d)) >> 1)); }
    }
    for (int o = 32; o > 0; o >>= 1) { P = min(P, __shfl_xor(P, o, 64)); E = max(E, __shfl_xor(E, o, 64)); }
    P = min(P, lh - 1);
    E = min(max(E, 0), lh - 1);
    const int first = min(P, E), last = max(P, E);
    int q = max(first - 1, 0);                                // start of the run that touches the interval
    while (q > 0 && swa_nt(swh, (uint32_t)q - 1u) == swa_nt(swh, (uint32_t)q)) { --q; }
    const int lo_pos = max(q - 1, 0), hi_pos = min(last + 1, lh);
    // two edits far apart: the two neighbourhoods only (k_fast_count_sites has the argument)
    int q2 = max(last - 1, 0);
    while (q2 > 0 && swa_nt(swh, (uint32_t)q2 - 1u) == swa_nt(swh, (uint32_t)q2)) { --q2; }
    const int lo_b = max(q2 - 1, 0), hi_a = min(first + 1, lh);
    const bool two_windows = P <= E && lo_b > hi_a;
    const int n_a = two_windows ? hi_a - lo_pos + 1 : hi_pos - lo_pos + 1;
    const int slots = (n_a + (two_windows ? hi_pos - lo_b + 1 : 0)) * 8;
    uint32_t found = 0;
    for (int t0 = 0; t0 < slots; t0 += 64) {
      const int t = t0 + lane;
      const int at = t >> 3;
      const uint32_t p = (uint32_t)(at < n_a ? lo_pos + at : lo_b + (at - n_a));
      const uint32_t slot = (uint32_t)t & 7u;
      bool ok = t < slots;
      const uint32_t prevc = (ok && p >= 1u) ? swa_nt(swh, p - 1u) : 4u;
      const uint32_t c = (ok && p < (uint32_t)lh) ? swa_nt(swh, p) : 4u;
      uint32_t type, base;
      if (slot < 4u) { type = 2u; base = slot; ok = ok && (p == 0u || base != prevc); }                       // insertion before p
      else if (slot < 7u) { type = 0u; const uint32_t t3 = slot - 4u; base = t3 < c ? t3 : t3 + 1u; ok = ok && p < (uint32_t)lh; }
      else { type = 1u; base = 0u; ok = ok && p < (uint32_t)lh && (p == 0u || c != prevc); }                  // deletion, once per run
      const int lv = type == 0u ? lh : (type == 1u ? lh - 1 : lh + 1);
      const int dv = lv - lx;                                 // v against x: one edit apart needs -1 .. 1
      bool near = false;
      if (ok && dv >= -1 && dv <= 1) {
        const bool v_longer = dv == 1, shifted = dv != 0;
        const uint32_t nw = ((uint32_t)max(lv, lx) + 31u) >> 5;   // words of the longer one: <= nmax + 1
        int lcp = 0x7fffffff, hb = -1;
        for (uint32_t w = 0; w < nw; ++w) {
          const uint64_t d = swa_variant_word(swh, nwh, type, p, base, w) ^ swx[w];
          if (d != 0ull) { lcp = (int)(32u * w) + (__builtin_ctzll(d) >> 1); break; }
        }
        uint64_t v_next = 0ull, x_next = 0ull;                // word nw of either is zero
        for (uint32_t w = nw; w-- > 0u; ) {
          const uint64_t vw = swa_variant_word(swh, nwh, type, p, base, w), xw = swx[w];
          const uint64_t lw = v_longer ? vw : xw, ln = v_longer ? v_next : x_next, sw = v_longer ? xw : vw;
          const uint64_t d = sw ^ (shifted ? ((lw >> 2) | (ln << 62)) : lw);
          if (d != 0ull) { hb = (int)(32u * w) + ((63 - __builtin_clzll(d)) >> 1); break; }
          v_next = vw; x_next = xw;
        }
        near = shifted ? hb < lcp : hb == lcp;
      }
      found += (uint32_t)__popcll(__ballot(near));
    }
    if (found != 0u) {
      if (lane == 0) { atomicMin(&a.graft[x], h); }
      total += found;
    }
  }
  if (lane == 0 && total != 0ull) { atomicAdd(a.cand_counter, total); }
}

// Amplicons that can be half of a pair the pair route does not take — with a sequence shorter than kFastMinLen
// (len <= short_cut) or, under the split, longer than the cap (len >= long_cut; 0xFFFFFFFF: no such band): flags for the
// light-only table, id lists for the Bloom route; out[0] lights, out[1] heavies, out[2] nucleotides of the lights
__global__ __launch_bounds__(256) void k_fast_band_lists(const uint32_t * __restrict__ seqlen, const uint8_t * __restrict__ role,
                                                         uint32_t n, uint32_t short_cut, uint32_t long_cut, uint8_t * __restrict__ is_member,
                                                         uint32_t * __restrict__ light_list, uint32_t * __restrict__ heavy_list,
                                                         unsigned long long * out) {
  const int lane = threadIdx.x & 63;
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i0 = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
    const uint32_t i = i0 + (uint32_t)lane;
    bool is_l = false, is_h = false;
    uint32_t len = 0;
    if (i < n) {
      len = seqlen[i];
      const uint32_t r = role[i];
      const bool band = len <= short_cut || len >= long_cut;
      is_l = r == 0u && band;
      is_h = r == 1u && band;
      is_member[i] = is_l ? 1 : 0;
    }
    const uint64_t ml = __ballot(is_l), mh = __ballot(is_h);
    if (ml != 0ull) {
      unsigned long long base = 0, nt = is_l ? len : 0u;
      for (int o = 32; o > 0; o >>= 1) { nt += swa_shfl_u64(nt, lane ^ o); }
      if (lane == 0) { base = atomicAdd(out + 0, (unsigned long long)__popcll(ml)); atomicAdd(out + 2, nt); }
      base = swa_shfl_u64(base, 0);
      if (is_l) { light_list[base + (uint64_t)__popcll(ml & lane_lt)] = i; }
    }
    if (mh != 0ull) {
      unsigned long long base = 0;
      if (lane == 0) { base = atomicAdd(out + 1, (unsigned long long)__popcll(mh)); }
      base = swa_shfl_u64(base, 0);
      if (is_h) { heavy_list[base + (uint64_t)__popcll(mh & lane_lt)] = i; }
    }
  }
}

// The lengths of the database against the pair route's cap: out[0] the longest sequence <= cap (0: none), out[1] the
// amplicons longer than cap, out[2] those of cap - 1 nt or more (which can be half of a pair with a longer one).  One
// atomic per wave and value.
__global__ __launch_bounds__(256) void k_fast_length_classes(const uint32_t * __restrict__ seqlen, uint32_t n, uint32_t cap,
                                                             uint32_t * out) {
  uint32_t best = 0, n_long = 0, n_band = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t len = seqlen[i];
    if (len <= cap) { best = max(best, len); } else { ++n_long; }
    if (len + 1u >= cap) { ++n_band; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
    n_long += (uint32_t)__shfl_xor((int)n_long, o, 64);
    n_band += (uint32_t)__shfl_xor((int)n_band, o, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (best != 0u) { atomicMax(out + 0, best); }
    if (n_long != 0u) { atomicAdd(out + 1, n_long); }
    if (n_band != 0u) { atomicAdd(out + 2, n_band); }
  }
}

// |V1(s)| = 6 L + 4 + runs(s) summed over the light (counters[0]) and this shard's heavy (counters[1]) amplicons
__global__ __launch_bounds__(256) void k_fast_variant_totals(const uint64_t * __restrict__ seqs, const uint64_t * __restrict__ seq_off,
                                                             const uint32_t * __restrict__ seqlen, const uint8_t * __restrict__ role,
                                                             uint32_t n, unsigned long long * counters) {
  unsigned long long mine[2] = {0ull, 0ull};
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t r = role[i];
    if (r > 1u) { continue; }
    const uint32_t len = seqlen[i];
    const uint64_t * s = seqs + seq_off[i];
    uint32_t runs = len != 0u ? 1u : 0u;
    const uint32_t nw = (len + 31u) >> 5;
    for (uint32_t w = 0; w < nw; ++w) {
      // positions p in this word (p >= 1, p < len) whose nucleotide differs from the one before
      const uint64_t cur = s[w];
      const uint64_t prev = (cur << 2) | (w != 0u ? s[w - 1] >> 62 : (cur & 3ull));   // position 0 compared with itself
      uint64_t d = cur ^ prev;
      d = (d | (d >> 1)) & 0x5555555555555555ull;
      const uint32_t valid = len - 32u * w >= 32u ? 32u : len - 32u * w;
      if (valid < 32u) { d &= (1ull << (2u * valid)) - 1ull; }
      runs += (uint32_t)__popcll(d);
    }
    mine[r] += 6ull * len + 4ull + runs;
  }
  for (int r = 0; r < 2; ++r) {
    unsigned long long v = mine[r];
    for (int o = 32; o > 0; o >>= 1) { v += swa_shfl_u64(v, (int)((threadIdx.x & 63) ^ o)); }
    if ((threadIdx.x & 63u) == 0u && v != 0ull) { atomicAdd(&counters[r], v); }
  }
}
