// d1_anchor.inc — device code of the ANCHORED d=1 network (included once, by d1.hip alone, inside its anonymous namespace
// after d1_common.inc).
//
// Why: the plain kernel (k_d1_probe<MODE 0>) issues one divergent 8-byte Bloom read per microvariant — ~1000 random L2
// requests per query amplicon — and rocprofv3 shows it bound by exactly that request rate (profiles/r01).  The fix is
// locality, which the reference's layout cannot offer but the problem does: two sequences of at least 2 w + 1 nucleotides
// one edit apart share their first w or their last w nucleotides.  So
//
//   * two anchor indexes group all amplicons by (a 29-bit key of) their first / last w nucleotides, w = 32, 64 or 128
//     chosen per database (or, when those are the same for everybody, by 32-nt windows further in: anchor_key);
//   * inside a group the question "which members are one edit from which" is answered on the sequences themselves,
//     pair by pair (k_d1_group_pairs, k_d1_pairs_tiled), exactly, with no hash at all;
//   * the prefix pass takes the pairs that share the prefix-side window, the suffix pass the others; together every
//     link is found exactly once.
//
// Singleton groups have no candidates and cost nothing.  Groups too large for pairs (> 4096 members), groups with a
// sequence too long for the widest pair kernel (> 672 nt) and sequences shorter than 2 w + 1 nt fall back to the plain
// kernel (restricted to the same share of the seed, against a table of those members only), so the result is identical
// for any input; only speed depends on the data.
//
// Rounds 1-3 also carried an enumerating kernel per group (LDS hash table, microvariants by wave-wide XOR scans) and the
// hash-table index build it read (k_anchor_place / k_anchor_scatter): retired in round 4 — the streaming build
// (d1_stream.inc) and the pair kernels serve every length now.
//
// In this file, in order: routing and the window sample; abundance ranks; the pair machinery (records, pair_stage,
// pair_near, pair_emit, the guard) and its two kernels.  The types, the amplicon lines and the anchor keys are in
// d1_common.inc (the --fastidious pass reads them too), the plain kernel's restricted enumeration (enumerate_range) is
// with that kernel in d1_probe.inc.

#ifndef SWA_PAIR_WG
#define SWA_PAIR_WG 5
#endif

// which rank of a multi-GPU job serves the group of this anchor key: bits of the MIXED key that neither the table index
// (its low bits) nor the slot tag (its high half) depend on alone; multiply-shift, no division
__device__ __forceinline__ uint32_t anchor_owner(uint64_t mixed, uint32_t world) {
  return (uint32_t)((((mixed >> 24) & 0xFFFFFFull) * world) >> 24);
}

constexpr uint32_t kRoutePerThread = 8;

__global__ __launch_bounds__(256) void k_anchor_route(const uint64_t * __restrict__ seqs, const uint64_t * __restrict__ seq_off,
                                                      const uint32_t * __restrict__ seqlen, uint32_t first, uint32_t count,
                                                      uint32_t world, uint32_t win_a, uint32_t win_b, uint32_t nwin,
                                                      uint32_t * __restrict__ out, uint64_t cap, uint32_t * counts) {
  __shared__ uint32_t hist[2 * kRouteMaxWorld], base[2 * kRouteMaxWorld];
  const uint32_t tile = 256u * kRoutePerThread;
  for (uint32_t t0 = blockIdx.x * tile; t0 < count; t0 += gridDim.x * tile) {
    if (threadIdx.x < 2u * world) { hist[threadIdx.x] = 0u; }
    __syncthreads();
    uint32_t dest[kRoutePerThread][2], place[kRoutePerThread][2];
#pragma unroll
    for (uint32_t k = 0; k < kRoutePerThread; ++k) {
      const uint32_t e = t0 + k * 256u + threadIdx.x;
      dest[k][0] = dest[k][1] = 0xFFFFFFFFu;
      if (e < count) {
        const uint32_t i = first + e;
        const uint32_t len = seqlen[i];
        const uint64_t * s = seqs + seq_off[i];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
          if (len >= (which == 0 ? win_a : win_b) + kAnchor * nwin) {
            const uint32_t d = (uint32_t)which * world + anchor_owner(mix64(anchor_key(s, len, which, win_a, win_b, nwin)), world);
            dest[k][which] = d;
            place[k][which] = atomicAdd(&hist[d], 1u);
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 2u * world) { base[threadIdx.x] = hist[threadIdx.x] != 0u ? atomicAdd(&counts[threadIdx.x], hist[threadIdx.x]) : 0u; }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kRoutePerThread; ++k) {
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        const uint32_t d = dest[k][which];
        if (d == 0xFFFFFFFFu) { continue; }
        const uint64_t at = (uint64_t)base[d] + place[k][which];
        if (at < cap) { out[(uint64_t)d * cap + at] = first + t0 + k * 256u + threadIdx.x; }
        else { counts[2u * world] = 1u; }
      }
    }
    __syncthreads();
  }
}

// ---- choosing the anchor windows from a sample --------------------------------------------------
// Every `stride`-th amplicon files its prefix- and suffix-side keys for the candidate window offsets 0, 32, 64, 96 in
// eight small tables; k_sample_mass then estimates, per candidate, how many amplicons of the database would sit in
// groups too large for LDS (a sample count c stands for c * stride members) and how many are too short to be anchored
// seeds at that offset.  Costs microseconds; a full index build under the wrong windows costs 100+ ms on a database
// with conserved flanks (ten million atomics on one slot).
constexpr uint32_t kSampleSlots = 1u << 17;
constexpr uint32_t kSampleCandidates = 4;
// words per anchor window for a database whose shortest sequence has `shortest` nt, windows `offset` nt from the ends:
// the widest of 32 / 64 / 128 nt that leaves every sequence two windows and a nucleotide (2 offset + 2 w + 1 <= shortest),
// at most max_nwin words; moved windows (offset > 0, "window mode") stay at 32 nt — the pair kernels keep one window word
__host__ __device__ inline uint32_t anchor_nwin_for(uint32_t shortest, uint32_t offset, uint32_t max_nwin) {
  uint32_t nwin = 1u;
  if (offset != 0u) { return nwin; }
  for (uint32_t c = 2u; c <= max_nwin && c <= 4u; c <<= 1) { if (64u * c + 1u <= shortest) { nwin = c; } }
  return nwin;
}
// out[0] = 0xFFFFFFFF - the shortest sequence, out[1 + c] = sequences of width class c (c = kTooLong: beyond the pair kernels)
__global__ __launch_bounds__(256) void k_db_lengths(const uint32_t * __restrict__ seqlen, uint32_t n, uint32_t * out) {
  __shared__ uint32_t pop[kWidthClasses + 1];
  if (threadIdx.x <= kWidthClasses) { pop[threadIdx.x] = 0u; }
  __syncthreads();
  uint32_t shortest = 0xFFFFFFFFu, mine[kWidthClasses + 1] = {};
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t len = seqlen[i];
    shortest = min(shortest, len);
    const uint32_t c = width_class(len);
#pragma unroll
    for (uint32_t k = 0; k <= kWidthClasses; ++k) { mine[k] += c == k ? 1u : 0u; }
  }
  for (int o = 32; o > 0; o >>= 1) { shortest = min(shortest, (uint32_t)__shfl_xor((int)shortest, o, 64)); }
#pragma unroll
  for (uint32_t k = 0; k <= kWidthClasses; ++k) {
    uint32_t v = mine[k];
    for (int o = 32; o > 0; o >>= 1) { v += (uint32_t)__shfl_xor((int)v, o, 64); }
    if ((threadIdx.x & 63u) == 0u && v != 0u) { atomicAdd(&pop[k], v); }
  }
  if ((threadIdx.x & 63u) == 0u && shortest != 0xFFFFFFFFu) { atomicMax(out, 0xFFFFFFFFu - shortest); }
  __syncthreads();
  if (threadIdx.x <= kWidthClasses && pop[threadIdx.x] != 0u) { atomicAdd(out + 1u + threadIdx.x, pop[threadIdx.x]); }
}
__global__ __launch_bounds__(256) void k_anchor_sample(const uint64_t * __restrict__ seqs, const uint64_t * __restrict__ seq_off,
                                                       const uint32_t * __restrict__ seqlen, uint32_t n, uint32_t stride,
                                                       unsigned long long * keys, uint32_t * counts, uint32_t * too_short,
                                                       uint32_t shortest, uint32_t max_nwin) {
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; (uint64_t)k * stride < n; k += gridDim.x * blockDim.x) {
    const uint32_t i = k * stride;
    const uint32_t len = seqlen[i];
    const uint64_t * s = seqs + seq_off[i];
    for (uint32_t c = 0; c < kSampleCandidates; ++c) {
      const uint32_t w = 32u * c, nwin = anchor_nwin_for(shortest, w, max_nwin);   // (offset from either end, words per window)
      if (len < 2u * w + 2u * kAnchor * nwin + 1u) { atomicAdd(&too_short[c], 1u); continue; }
      for (int which = 0; which < 2; ++which) {
        const uint64_t key = anchor_key(s, len, which, w, w, nwin);
        unsigned long long * tk = keys + (size_t)(2u * c + (uint32_t)which) * kSampleSlots;
        uint32_t * tc = counts + (size_t)(2u * c + (uint32_t)which) * kSampleSlots;
        uint32_t idx = (uint32_t)mix64(key) & (kSampleSlots - 1u);
        for (uint32_t probes = 0; probes < kSampleSlots; ++probes) {
          const unsigned long long old = atomicCAS(&tk[idx], kKeyEmpty, (unsigned long long)key);
          if (old == kKeyEmpty || old == key) { atomicAdd(&tc[idx], 1u); break; }
          idx = (idx + 1u) & (kSampleSlots - 1u);
        }
      }
    }
  }
}

// mass[c] = sample amplicons in groups whose estimated size (count * stride) exceeds kGroupCap, both sides added
__global__ __launch_bounds__(256) void k_sample_mass(const uint32_t * __restrict__ counts, uint32_t stride, uint32_t * mass) {
  const uint32_t total = 2u * kSampleCandidates * kSampleSlots;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const uint32_t c = counts[i];
    if ((uint64_t)c * stride > kGroupCap) { atomicAdd(&mass[i / (2u * kSampleSlots)], c); }
  }
}

// Work lists for the pair kernels, made by k_group1 / k_group_lists (d1_stream.inc).  Per width class: one list per size
// class — a group of g members goes to the class of the smallest S in {4, 8, 16, 32, 64} with g <= S, 64 / S groups of a
// class share a wave —, one list of the groups of 65..pair_big members (a workgroup each), and one of 64-member row tiles
// of the groups beyond that (k_d1_pairs_tiled).  Regions of the item buffer: ListRegions (host: list_regions).
struct PairLists {
  swa_item * items;                 // base of the index's item buffer
  ListRegions region;
  uint32_t * counters;              // [kWidthClasses][8] device counters: items in list (class, kind)
  uint32_t pair_big;
};

__device__ __forceinline__ uint32_t pair_class(uint32_t g) {        // g in 2..64
  return g <= 4u ? 0u : (g <= 8u ? 1u : (g <= 16u ? 2u : (g <= 32u ? 3u : 4u)));
}

// rank[i] = index of the first amplicon with the same abundance as amplicon i.  The db order is
// abundance descending (src/db.cc:388-413), so abundance[x] >= abundance[y] <=> rank[x] <= rank[y]
// and the abundance rule of the network (algod1.cc:576-580) becomes a 32-bit compare that fits
// next to the group table in LDS.  flags[kFlagUnordered] is raised when the order does not hold (a caller
// that uploaded some other order): the anchored passes are then not used.
// Three streaming passes over tiles of 256 amplicons (a max-scan of "where did the current run of equal abundances
// start"): the runs that start inside a tile, the tiles' last starts carried forward, the amplicons whose run
// started before their tile.
__global__ __launch_bounds__(256) void k_abundance_rank(const uint64_t * __restrict__ abundance, uint32_t n,
                                                        uint32_t * __restrict__ rank, uint32_t * flags,
                                                        uint32_t * __restrict__ tile_last) {
  __shared__ uint32_t wave_max[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
    const uint32_t i = base + threadIdx.x;
    const bool have = i < n;
    const uint64_t ab = have ? abundance[i] : 0ull;
    const uint64_t before = (have && i > 0u) ? abundance[i - 1u] : ~0ull;
    if (have && before < ab) { atomicOr(flags + kFlagUnordered, 1u); }
    uint32_t start = (have && before != ab) ? i + 1u : 0u;     // 1 + position where a run starts, else 0
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)start, (unsigned)d, 64);
      if ((int)lane >= d) { start = max(start, up); }
    }
    if (lane == 63u) { wave_max[wave] = start; }
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) { start = max(start, wave_max[w]); }
    if (have) { rank[i] = start != 0u ? start - 1u : 0xFFFFFFFFu; }      // (0xFFFFFFFF: the run began before this tile)
    if (threadIdx.x == 255u) { tile_last[base >> 8] = start; }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_abundance_rank_carry(uint32_t * tile_last, uint32_t tiles) {
  // one workgroup: exclusive running maximum over the tiles, 2048 per turn (eight consecutive ones per thread)
  constexpr uint32_t kPer = 8;
  __shared__ uint32_t wave_max[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < tiles; base += 256u * kPer) {
    const uint32_t t0 = base + threadIdx.x * kPer;
    uint32_t v[kPer], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) { v[k] = t0 + k < tiles ? tile_last[t0 + k] : 0u; mine = max(mine, v[k]); }
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, (unsigned)d, 64);
      if ((int)lane >= d) { incl = max(incl, up); }
    }
    if (lane == 63u) { wave_max[wave] = incl; }
    __syncthreads();
    uint32_t before = carry;
    for (uint32_t w = 0; w < wave; ++w) { before = max(before, wave_max[w]); }
    const uint32_t up1 = (uint32_t)__shfl_up((int)incl, 1u, 64);
    uint32_t run = max(before, lane > 0u ? up1 : 0u);
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      if (t0 + k < tiles) { tile_last[t0 + k] = run; }
      run = max(run, v[k]);
    }
    carry = max(carry, max(max(wave_max[0], wave_max[1]), max(wave_max[2], wave_max[3])));
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_abundance_rank_fill(uint32_t n, uint32_t * __restrict__ rank, const uint32_t * __restrict__ tile_last) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    if (rank[i] == 0xFFFFFFFFu) { rank[i] = tile_last[i >> 8] - 1u; }   // (amplicon 0 starts a run: the carry is never 0 here)
  }
}

// ---- a rank of a multi-GPU job that serves only the anchor groups it owns (ownership) ---------
// What such a rank can do without the database-wide hash table: identical sequences share their
// first 32 nucleotides, hence their prefix group, and a group lives whole on ONE rank — so
// "is there a pair of identical sequences" is answered inside the owned prefix groups.
__device__ __forceinline__ bool identical_sequences(const uint64_t * seqs, const uint64_t * seq_off, uint32_t len,
                                                    uint32_t x, uint32_t y) {
  const uint64_t * p = seqs + seq_off[x];
  const uint64_t * q = seqs + seq_off[y];
  bool same = true;
  for (uint32_t w = 0; w < ((len + 31u) >> 5); ++w) { same = same && (p[w] == q[w]); }
  return same;
}

struct AnchorArgs {
  const swa_item * items;           // row tiles of the groups beyond pair_big (k_d1_pairs_tiled): this launch's class
  const uint32_t * item_count;      // device counter
  int pass;                         // 0 = prefix groups: pairs that share the prefix-side window, 1 = suffix groups: the others
  int no_cluster_breaking;
  uint32_t first, count;            // seeds outside [first, first+count) are only targets
  uint64_t * edges;
  uint64_t seg_cap;                 // per-wave output segments (see NetArgs)
  uint32_t * seg_fill;
  uint32_t * sched_big;             // work counter of the 65..pair_big groups of k_d1_group_pairs (zeroed per network call)
  uint32_t * sched_tiled;           // work counter of k_d1_pairs_tiled (zeroed per network call)
  uint32_t batch;                   // bundles a wave of k_d1_group_pairs takes per visit of the work counter
  uint32_t * sched_wide;            // k_d1_group_pairs: 2^shard_bits work counters, kSchedStride entries apart
  uint32_t shard_bits;
  uint32_t minlen;                  // seeds at least this long are served by the anchored passes (win_a + win_b + 2 w + 1)
  uint32_t win_word;                // window mode: the prefix-side window is word win_a / 32 of a sequence
  uint32_t window_mode;             // anchor windows moved inwards (anchor_key)
  const uint32_t * ids;             // the members' ids in group order and
  const uint4 * lines;              // the amplicon lines (d1_stream.inc): length | rank | words of every amplicon,
  uint32_t line_quads;              // 16-byte quads per line
  const swa_item * pair_items;      // work lists of k_d1_group_pairs (k_group_lists), this launch's width class: base,
  uint64_t pair_region[kPairClasses + 1];   // first item of each list,
  const uint32_t * pair_counters;   // items in each list
  uint32_t win_word_b;              // the suffix-side window ends win_b / 32 words before the end of the end-aligned words
  // the guard (round 4): members staged per wave, this pass (one writer per entry, like seg_fill) and — kGuardMisfiled — members found
  // in a group whose key is not theirs
  uint32_t * seg_staged;
  unsigned long long * guard;
  // identical sequences (round 6): two members of a prefix group whose every word agrees are the reference's "identical
  // sequences" (src/algod1.cc:1131-1150: fatal while it inserts) — seen by PASS 0 for two instructions a pair, where
  // k_group1 ran a second hash table over fingerprints for them.  flags[kFlagDuplicates] |= 1 when one of the two is a seed of this call.
  uint32_t * flags;
};

// ---- groups by PAIRS ----------------------------------------------------------------------------------
// Enumerating ~7 L microvariants per seed and probing an LDS table costs about 600 wave-instructions per seed;
// comparing two members directly costs less than two.  No hashes, no Bloom filter, no table, no separate
// verification: the test is exact.  Each unordered pair is looked at once and yields the links the abundance
// rule allows in either direction.
// PASS 0 (prefix groups): pairs that share the prefix-side window; PASS 1 (suffix groups): pairs that do not — the
// same division the plain kernel applies to the seeds it serves (k_d1_probe<MODE 2>: window_filter).

// ---- groups up to pair_big members by pairs, every lane a pair -------------------------------------------------------
// k_d1_group_pairs.  Each member of a group is staged once in LDS as a record: its packed words, the same words
// END-ALIGNED (the sequence shifted up so that its last nucleotide is the top 2-bit group of word W - 1), the
// prefix-side window, id, length, abundance rank, "may be a source of links".  A lane then holds one member in
// registers and meets partner after partner from LDS (7 ds_read_b128 for W = 5): member j of a group of g meets
// members j + 1 .. j + g / 2 (mod g), so every unordered pair is looked at once and every lane of the group works in
// every turn.  Groups of 2..64: 64 / S groups of size class S share a wave (k_scan_apply_lists), the wave's own
// quarter of the record array, no workgroup barrier; groups of 65..pair_big: one workgroup, its waves take turns t.
//   one edit apart  <=>  lcp + lcs >= n - 1 = the one mismatch          (equal lengths n; identical: never)
//                        lcp + lcs >= n, lengths n and n + 1            (lcp, lcs capped at n)
// lcp = first differing bit of the forward words (v_ffbl per dword, OR 32 k, v_min3), lcs = first differing bit from
// the top of the end-aligned words (v_ffbh): 32-bit full-rate instructions only, no shifts, no selects, no
// cross-lane traffic in the loop.  About 110 VALU instructions per 64 pairs (round 2's first pair kernel — lane =
// member, seed words through v_readlane, shifted comparison chosen per lane — spent ~170 per turn with g of 64 lanes busy).
typedef uint4 __attribute__((may_alias)) uint4_alias;
typedef uint64_t __attribute__((may_alias)) u64_alias;

template <int W> struct PairLayout {
  static constexpr uint32_t kMeta = 4 * W;                        // dwords: [0, 2W) forward | [2W, 4W) end-aligned | meta
  static constexpr uint32_t kDwords = (4 * W + 6 + 3) / 4 * 4;    // meta: window (2) id len | rank ok (pad)
  static constexpr bool kDynamicLds = 256u * kDwords * 4u > 48u * 1024u;   // k_d1_group_pairs: a record per thread
  static constexpr uint32_t kDynamicBytes = kDynamicLds ? 256u * kDwords * 4u : 0u;
};
template <int W> struct PairMember {
  uint32_t w[2 * W], t[2 * W];
  uint32_t pw_lo, pw_hi, id, len, rank, ok;
};

// (0xFFFFFFFF for x = 0: what the OR / min chains below rely on; the builtins are undefined there)
__device__ __forceinline__ uint32_t first_set_bit(uint32_t x) { uint32_t r; asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x)); return r; }
__device__ __forceinline__ uint32_t leading_zero_bits(uint32_t x) { uint32_t r; asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x)); return r; }

// the amplicon line of member `id` (abundance rank, length, packed words): ONE aligned fetch; nothing for a lane without a member
template <int W>
__device__ __forceinline__ void pair_fetch_line(const AnchorArgs & a, bool have, uint32_t id, uint32_t & rank, uint32_t & len, uint64_t (&w64)[W]) {
  rank = 0u; len = 0u;
#pragma unroll
  for (int k = 0; k < W; ++k) { w64[k] = 0ull; }
  if (!have) { return; }
  line_fetch<W>(a.lines, a.line_quads, id, w64, len, rank);
}

// a member whose line has been fetched (pair_fetch_line): end-aligned words, meta; into registers (m) and into its LDS record (rec).
// FULL = false: the member is only wanted in registers (a column member of the tiled kernel): rec is not touched.
// End-aligned = the sequence shifted up by 32 W - len nucleotides: by (that mod 32) nucleotides between neighbouring
// words, then by whole words — a member as long as its group's width needs none; the others (a 150-nt read in the group of
// a 460-nt one) take a barrel shifter over the word array, log2 W steps of selects: no indexed register access, no LDS.
template <int W, bool FULL = true>
__device__ __forceinline__ void pair_stage_line(const AnchorArgs & a, bool have, uint32_t id, uint32_t rank, uint32_t len, const uint64_t (&w64)[W],
                                                uint32_t * rec, PairMember<W> & m) {
  uint64_t t64[W];
  m.id = id; m.rank = rank; m.len = len;
  const uint32_t sh = have ? 32u * W - m.len : 0u;              // nucleotides to shift up by (len <= 32 W: the group's width class)
  const uint32_t ws = sh >> 5, b = (sh & 31u) << 1;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const uint64_t below = k > 0 ? w64[k > 0 ? k - 1 : 0] : 0ull;
    t64[k] = b != 0u ? (w64[k] << b) | (below >> (64u - b)) : w64[k];
  }
  if (__ballot(ws != 0u) != 0ull) {                             // (not the usual case: everybody longer than 32 (W - 1))
#pragma unroll
    for (int step = 1; step < W; step <<= 1) {
      const bool take = (ws & (uint32_t)step) != 0u;
#pragma unroll
      for (int k = W - 1; k >= 0; --k) {
        const uint64_t from = k >= step ? t64[k >= step ? k - step : 0] : 0ull;
        t64[k] = take ? from : t64[k];
      }
    }
  }
  uint64_t pw = w64[0];                                          // the prefix-side window's word (window mode: word win_word, wave-uniform)
  if (a.win_word != 0u) {
#pragma unroll
    for (int k = 1; k < W; ++k) { pw = a.win_word == (uint32_t)k ? w64[k] : pw; }
  }
  m.pw_lo = (uint32_t)pw; m.pw_hi = (uint32_t)(pw >> 32);
  // a member is a SOURCE of links when it is a seed of this call that the anchored passes serve (not too short: those go
  // to the plain kernel, k_stream_fallback)
  m.ok = (have && m.id >= a.first && m.id - a.first < a.count && m.len >= a.minlen) ? 1u : 0u;
  u64_alias * r64 = reinterpret_cast<u64_alias *>(rec);
#pragma unroll
  for (int k = 0; k < W; ++k) {
    m.w[2 * k] = (uint32_t)w64[k]; m.w[2 * k + 1] = (uint32_t)(w64[k] >> 32);
    m.t[2 * k] = (uint32_t)t64[k]; m.t[2 * k + 1] = (uint32_t)(t64[k] >> 32);
    if (FULL) { r64[k] = w64[k]; r64[W + k] = t64[k]; }
  }
  if (FULL) {
    r64[2 * W] = pw;
    rec[4 * W + 2] = m.id; rec[4 * W + 3] = m.len; rec[4 * W + 4] = m.rank; rec[4 * W + 5] = m.ok;
  }
}

// member number `index` of the group-order member list: its id, then its line, then the above
template <int W, bool FULL = true>
__device__ __forceinline__ void pair_stage(const AnchorArgs & a, bool have, uint64_t index, uint32_t * rec, PairMember<W> & m) {
  uint64_t w64[W];
  uint32_t rank, len;
  const uint32_t id = have ? a.ids[index] : 0u;
  pair_fetch_line<W>(a, have, id, rank, len, w64);
  pair_stage_line<W, FULL>(a, have, id, rank, len, w64, rec, m);
}

// (volatile: 16 bytes a read, as written.  A pass that leaves some dwords of a record unread — the shortened chains of
// pair_near — had the compiler take the reads apart and put them together again as twenty 4-byte pairs for W = 8: the
// prefix pass of a 200-nt set ran 2.1 x longer, bound by LDS instructions)
typedef uint32_t swa_u32x4 __attribute__((ext_vector_type(4), may_alias));
template <int W>
__device__ __forceinline__ void pair_load_record(const uint32_t * rec, uint32_t (&p)[PairLayout<W>::kDwords]) {
  // (rec lies in LDS; said so, or a volatile read through a generic pointer becomes a flat load)
  typedef const volatile __attribute__((address_space(3))) swa_u32x4 * lds_quads;
  lds_quads q = (lds_quads)rec;
#pragma unroll
  for (uint32_t i = 0; i < PairLayout<W>::kDwords / 4u; ++i) {
    const swa_u32x4 v = q[i];
    p[4 * i] = v.x; p[4 * i + 1] = v.y; p[4 * i + 2] = v.z; p[4 * i + 3] = v.w;
  }
}

template <int W>
__device__ __forceinline__ void pair_member_from(const uint32_t * rec, PairMember<W> & m) {
  uint32_t p[PairLayout<W>::kDwords];
  pair_load_record<W>(rec, p);
#pragma unroll
  for (int k = 0; k < 2 * W; ++k) { m.w[k] = p[k]; m.t[k] = p[2 * W + k]; }
  m.pw_lo = p[4 * W]; m.pw_hi = p[4 * W + 1]; m.id = p[4 * W + 2]; m.len = p[4 * W + 3]; m.rank = p[4 * W + 4]; m.ok = p[4 * W + 5];
}

// member m against the partner whose record is p: exactly one edit apart, and on this pass's side of the division.
// ends = the anchor windows are the first / last 32 NW nucleotides (no window mode; wave-uniform).  Then neither chain runs
// over all 2 W dwords (round 6; tests/test_pair_identity.py pins each step on the CPU):
//   PASS 0 — a pair only counts when the two share their first window: the first 2 NW forward dwords are compared for
//     equality only (that IS `same`), the forward chain covers the rest.  The suffix chain leaves out the LOWEST 2 NW
//     end-aligned dwords: when every dword above them agrees the common suffix has min(n, 32 W - 32 NW) nucleotides and
//     the common prefix 32 NW (same), so lcp + lcs >= n whatever the dwords left out hold — near for lengths one apart,
//     not near (one substitution needs lcp + lcs = n - 1) for equal lengths — which is what an empty chain (lcs capped at
//     n) answers; when a dword above them differs, that is the topmost difference and the chain has it.
//   PASS 1 — the members of a group share their last window unless two window keys collide, so the top 2 NW end-aligned
//     dwords are compared for equality only (a collision: not a pair of this group at all — its true groups, if any, find
//     it); a pair only counts when the first windows DIFFER (the prefix pass has the others), and then the first
//     difference lies in the first 2 NW forward dwords: the forward chain covers those and nothing else (empty chain =
//     equal first windows = `same` = not this pass's pair).
// Window mode (NW = 1): both chains in full, `same` on the window word kept in the record.
template <int PASS, int W, int NW>
__device__ __forceinline__ bool pair_near(const PairMember<W> & m, const uint32_t (&p)[PairLayout<W>::kDwords], bool ends, bool & identical) {
  uint32_t f = 0xFFFFFFFFu, l = 0xFFFFFFFFu;
  bool ok = true, same;
  if (ends) {
    uint32_t head = 0u, tail = 0u;
#pragma unroll
    for (int k = 0; k < 2 * W; ++k) {
      if (PASS == 0) {
        if (k < 2 * NW) { head |= m.w[k] ^ p[k]; }
        else {
          f = min(f, first_set_bit(m.w[k] ^ p[k]) | (uint32_t)(32 * k));
          l = min(l, leading_zero_bits(m.t[k] ^ p[2 * W + k]) | (uint32_t)(32 * (2 * W - 1 - k)));
        }
      } else {
        if (k < 2 * NW) { f = min(f, first_set_bit(m.w[k] ^ p[k]) | (uint32_t)(32 * k)); }
        if (k >= 2 * W - 2 * NW) { tail |= m.t[k] ^ p[2 * W + k]; }
        else { l = min(l, leading_zero_bits(m.t[k] ^ p[2 * W + k]) | (uint32_t)(32 * (2 * W - 1 - k))); }
      }
    }
    // (kept as OR chains: told that only `== 0` is asked, the compiler compares dword by dword and packs the answers)
    if (PASS == 0) { asm("" : "+v"(head)); } else { asm("" : "+v"(tail)); }
    if (PASS == 1) { ok = tail == 0u; }
    same = PASS == 0 ? head == 0u : f == 0xFFFFFFFFu;
  } else {
#pragma unroll
    for (int k = 0; k < 2 * W; ++k) {
      f = min(f, first_set_bit(m.w[k] ^ p[k]) | (uint32_t)(32 * k));
      l = min(l, leading_zero_bits(m.t[k] ^ p[2 * W + k]) | (uint32_t)(32 * (2 * W - 1 - k)));
    }
    same = m.pw_lo == p[4 * W] && m.pw_hi == p[4 * W + 1];
  }
  const uint32_t plen = p[4 * W + 3];
  const uint32_t n = min(m.len, plen), apart = max(m.len, plen) - n;
  const uint32_t sum = min(f >> 1, n) + min(l >> 1, n);
  const bool near = apart == 0u ? sum + 1u == n : (apart == 1u && sum >= n);
  // (no differing bit anywhere in the forward words, equal lengths: the same sequence.  PASS 0 only: identical sequences share
  // their prefix-side window, hence a prefix group — ends: the window dwords are in `head`, the chain covers the rest)
  identical = PASS == 0 && apart == 0u && f == 0xFFFFFFFFu && same;
  return ok && near && (PASS == 0 ? same : !same);
}

// The guard (round 4).  A member of a group must carry the group's 32-bit window key.  Its window (the record's dwords
// [at, at + 2 NW): forward words for PASS 0, end-aligned words for PASS 1) is compared with the window of the group's
// first member; a difference is a key collision — two windows, one 32-bit key: harmless, every pair test is exact — or
// a member that was filed under a key that is not its own, which loses its links silently (the round-1 / round-3
// anomaly's signature).  Only then are the two keys recomputed: returns true for a misfiled member.
template <int NW>
__device__ __forceinline__ bool pair_misfiled(const uint32_t * mine, const uint32_t * first, uint32_t at, int which) {
  uint32_t diff = 0u;
#pragma unroll
  for (int k = 0; k < 2 * NW; ++k) { diff |= mine[at + k] ^ first[at + k]; }
  if (diff == 0u) { return false; }
  uint64_t wa[NW], wb[NW];
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    wa[k] = (uint64_t)mine[at + 2 * k] | ((uint64_t)mine[at + 2 * k + 1] << 32);
    wb[k] = (uint64_t)first[at + 2 * k] | ((uint64_t)first[at + 2 * k + 1] << 32);
  }
  return anchor_key29(wa, NW, which) != anchor_key29(wb, NW, which);
}
// where the window of this pass lies in a record (dword index)
template <int PASS, int W, int NW>
__device__ __forceinline__ uint32_t pair_window_at(const AnchorArgs & a) {
  return PASS == 0 ? 2u * a.win_word : 2u * (uint32_t)W + 2u * ((uint32_t)(W - NW) - a.win_word_b);
}

// two members with the same sequence: reported when one of them is a seed of this call (the reference's duplicate check is
// per inserted amplicon, src/algod1.cc:1131-1150; a rank of a multi-GPU job answers for the groups it owns: first = 0, count = n)
__device__ __forceinline__ void pair_twin(const AnchorArgs & a, uint32_t ida, uint32_t idb) {
  if (ida != idb && ((ida - a.first < a.count) || (idb - a.first < a.count))) { atomicOr(a.flags + kFlagDuplicates, 1u); }
}

// set bits of a ballot below this lane (v_mbcnt_lo / _hi: two instructions)
__device__ __forceinline__ uint32_t lanes_below(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// links of one turn: e1 = member -> partner, e2 = partner -> member; into the wave's output segment `seg` (room for cap
// links; what does not fit is counted, not written: the caller repeats the call with larger segments).  Round 6: one branch
// a turn instead of six (emission was 45 of a pass's 270 us at 10 M: profiles/r06/NOTES.md section 10).
__device__ __forceinline__ void pair_emit(bool e1, bool e2, uint32_t id, uint32_t pid, unsigned long long * seg, uint32_t cap,
                                          uint32_t & seg_at) {
  const uint64_t m1 = __ballot(e1), m2 = __ballot(e2);
  if ((m1 | m2) == 0ull) { return; }
  const uint32_t n1 = (uint32_t)__popcll(m1);
  const uint32_t at1 = seg_at + lanes_below(m1), at2 = seg_at + n1 + lanes_below(m2);
  if (e1 && at1 < cap) { seg[at1] = ((unsigned long long)id << 32) | pid; }
  if (e2 && at2 < cap) { seg[at2] = ((unsigned long long)pid << 32) | id; }
  seg_at += n1 + (uint32_t)__popcll(m2);
}

// Groups beyond pair_big (up to kGroupCap = 2048 members) by pairs, in 64 x 64 tiles: work item = (group, row tile r, part:
// up to kTiledCols of the column tiles C >= r); the workgroup stages the row tile's records in LDS, its waves take the item's
// column tiles in turn: lane j keeps
// member 64 C + j in registers and meets every member of the row tile (all lanes read the same record: broadcast).
// Quadratic — 1.7 VALU instructions per pair, so a member of a group of g costs 0.9 g against the ~600 of the
// enumerating kernel — but it needs no hashes at all, and it is the only kind of kernel window mode has (the
// enumerating kernel divides a seed's microvariants by position, the pair kernels by the window itself).
template <int PASS, int W, int NW>
__global__ __launch_bounds__(kThreads) void k_d1_pairs_tiled(const AnchorArgs a) {
  constexpr uint32_t RD = PairLayout<W>::kDwords;
  __shared__ __attribute__((aligned(16))) uint32_t row_recs[kSeedsPerItem * RD];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nitems = *a.item_count;
  const uint32_t gwave = blockIdx.x * kWaves + wave;
  uint32_t seg_at = a.seg_fill[gwave];
  unsigned long long * const seg = reinterpret_cast<unsigned long long *>(a.edges) + (uint64_t)gwave * a.seg_cap;
  const uint32_t seg_room = (uint32_t)min(a.seg_cap, (uint64_t)0xFFFFFFFFu);
  uint32_t staged_members = a.seg_staged[gwave], misfiled = 0u;   // (the guard: pair_misfiled)
  const uint32_t win_at = pair_window_at<PASS, W, NW>(a);
  const bool ncb = a.no_cluster_breaking != 0;
  const bool ends = a.window_mode == 0u;                          // (anchor windows = the first / last 32 NW nt)
  // A row tile of a group of g members meets g / 64 - r column tiles, kTiledCols of them an item.  Items are
  // handed out through a counter (a workgroup's first item is a fixed one; the visit for the next is issued once the row
  // tile is staged and read when the item is done), not dealt round-robin: the list is in decreasing order of cost inside
  // every group, and a fixed deal left workgroups idle for a third of the kernel on sets with groups of thousands.
  __shared__ uint32_t sh_it;
  uint32_t it = blockIdx.x, it_next = 0;
  while (it < nitems) {
    const swa_item item = a.items[it];
    const uint32_t g = item.size, r = item.chunk & 63u, part = item.chunk >> 6;
    const uint32_t all_tiles = (g + kSeedsPerItem - 1u) / kSeedsPerItem;
    const uint32_t c_first = r + part * kTiledCols;              // this item's column tiles: [c_first, tiles)
    const uint32_t tiles = min(all_tiles, c_first + kTiledCols);
    const uint32_t nrow = min(kSeedsPerItem, g - r * kSeedsPerItem);
    if (threadIdx.x < kSeedsPerItem) {
      const bool have = threadIdx.x < nrow;
      PairMember<W> staged;
      pair_stage<W>(a, have, (uint64_t)item.begin + r * kSeedsPerItem + threadIdx.x, row_recs + threadIdx.x * RD, staged);
      if (part == 0u) { staged_members += (uint32_t)__popcll(__ballot(have)); }   // (wave 0: every member of a group is a row member of ONE first part)
    }
    if (threadIdx.x == 0) { it_next = atomicInc(a.sched_tiled, 0xFFFFFFFFu); }   // (atomicInc, and nothing computed from it here: see `advance` in k_d1_group_pairs)
    __syncthreads();
    // (the guard: every member of the row tile against the tile's first; the tiles of a group hang together through the
    // column members below, which are all compared with row 0's window when r = 0)
    if (threadIdx.x < nrow && pair_misfiled<NW>(row_recs + threadIdx.x * RD, row_recs, win_at, PASS)) { ++misfiled; }
    // the wave's column tiles: the lines of its next tile and the ids of the one after are fetched while this one is
    // compared (round 6: a tile's fetches depend on each other — ids, then lines — and the kernel waited for them tile by tile;
    // made of many short items, it is bound by those waits, not by its comparisons: profiles/r06/NOTES.md section 10)
    auto column_id = [&](uint32_t c2) -> uint32_t {
      const uint32_t col2 = c2 * kSeedsPerItem + lane;
      return (c2 < tiles && col2 < g) ? a.ids[(uint64_t)item.begin + col2] : 0u;
    };
    uint32_t id_here = column_id(c_first + wave), id_next = column_id(c_first + wave + (uint32_t)kWaves);
    uint64_t w64[W];
    uint32_t rank = 0, len = 0;
    if (c_first + wave < tiles) { pair_fetch_line<W>(a, (c_first + wave) * kSeedsPerItem + lane < g, id_here, rank, len, w64); }
    for (uint32_t c = c_first + wave; c < tiles; c += (uint32_t)kWaves) {
      const uint32_t col = c * kSeedsPerItem + lane;
      const bool have = col < g;
      PairMember<W> m;
      pair_stage_line<W, false>(a, have, id_here, rank, len, w64, nullptr, m);
      {
        const uint32_t cn = c + (uint32_t)kWaves;
        id_here = id_next;
        if (cn < tiles) { pair_fetch_line<W>(a, cn * kSeedsPerItem + lane < g, id_here, rank, len, w64); }
        id_next = column_id(cn + (uint32_t)kWaves);
      }
      if (r == 0u && c != 0u && have) {
        // the column member's window, from its registers (PASS 0: forward dwords, PASS 1: end-aligned dwords; the place is
        // wave-uniform: a chain of selects)
        const uint32_t off = PASS == 0 ? win_at : win_at - 2u * (uint32_t)W;
        uint32_t mine[2 * NW], first_win[2 * NW];
#pragma unroll
        for (int q = 0; q < 2 * NW; ++q) {
          mine[q] = 0u;
#pragma unroll
          for (int k = 0; k < 2 * W; ++k) { mine[q] = off + (uint32_t)q == (uint32_t)k ? (PASS == 0 ? m.w[k] : m.t[k]) : mine[q]; }
          first_win[q] = row_recs[win_at + q];
        }
        if (pair_misfiled<NW>(mine, first_win, 0u, PASS)) { ++misfiled; }
      }
      for (uint32_t i = 0; i < nrow; ++i) {
        uint32_t p[RD];
        pair_load_record<W>(row_recs + i * RD, p);
        // the diagonal tile looks at each unordered pair once
        bool twin = false;
        const bool near = have && (c != r || lane > i) && pair_near<PASS, W, NW>(m, p, ends, twin);
        if (PASS == 0 && twin && have && (c != r || lane > i)) { pair_twin(a, m.id, p[4 * W + 2]); }
        const uint32_t pid = p[4 * W + 2], prank = p[4 * W + 4];
        const bool e1 = near && m.ok != 0u && (ncb || m.rank <= prank);
        const bool e2 = near && p[4 * W + 5] != 0u && (ncb || prank <= m.rank);
        pair_emit(e1, e2, m.id, pid, seg, seg_room, seg_at);
      }
    }
    if (threadIdx.x == 0) { sh_it = gridDim.x + it_next; }
    __syncthreads();                                          // (also: this item's row tile is no longer read)
    it = sh_it;
  }
  if (lane == 0u) { a.seg_fill[gwave] = seg_at; a.seg_staged[gwave] = staged_members; }
  if (misfiled != 0u) { atomicAdd(a.guard + kGuardMisfiled, (unsigned long long)misfiled); }
}

// (W = 5: five workgroups per CU — 96 registers a lane; the prefix pass came out at 98 without being told)
template <int PASS, int W, int NW>
__global__ __launch_bounds__(kThreads, W == 5 ? SWA_PAIR_WG : 1) void k_d1_group_pairs(const AnchorArgs a) {
  constexpr uint32_t RD = PairLayout<W>::kDwords;
  // (a record per thread: 28 KB for W = 5, 41 KB for W = 8 — static; 70 / 94 KB for W = 15 / 21: beyond what a kernel gets
  // unasked, so those take it as dynamic LDS — pair_dynamic_lds, opted in by the launcher)
  constexpr bool kDynamic = PairLayout<W>::kDynamicLds;
  __shared__ __attribute__((aligned(16))) uint32_t recs_static[kDynamic ? 4 : kThreads * RD];
  extern __shared__ __attribute__((aligned(16))) uint32_t recs_dynamic[];
  uint32_t * const recs = kDynamic ? recs_dynamic : recs_static;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (told to the compiler: the same in every lane)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t gwave = blockIdx.x * kWaves + wave;
  uint32_t seg_at = a.seg_fill[gwave];
  unsigned long long * const seg = reinterpret_cast<unsigned long long *>(a.edges) + (uint64_t)gwave * a.seg_cap;
  const uint32_t seg_room = (uint32_t)min(a.seg_cap, (uint64_t)0xFFFFFFFFu);
  uint32_t staged_members = a.seg_staged[gwave], misfiled = 0u;   // (the guard: pair_misfiled)
  const uint32_t win_at = pair_window_at<PASS, W, NW>(a);
  const bool ncb = a.no_cluster_breaking != 0;
  const bool ends = a.window_mode == 0u;                          // (anchor windows = the first / last 32 NW nt)

  // ---- groups of 65..pair_big members: one workgroup per group ----
  const uint32_t nbig = a.pair_counters[kPairClasses];
  const swa_item * big = a.pair_items + a.pair_region[kPairClasses];
  // (handed out through a counter: the launch holds exactly the workgroups that are resident together — with a static
  // share, workgroups of a second round would start on their big groups when everybody else has finished the bundles)
  // (a workgroup's first group is a fixed one; the visit of the counter for the next is issued once the current group is
  // staged and read when it is finished — see the bundles below)
  __shared__ uint32_t sh_big;
  uint32_t it = blockIdx.x, it_next = 0;
  while (it < nbig) {
    const swa_item item = big[it];
    const uint32_t g = item.size, half = g >> 1;
    {
      const bool have = threadIdx.x < g;
      PairMember<W> staged;
      pair_stage<W>(a, have, (uint64_t)item.begin + threadIdx.x, recs + threadIdx.x * RD, staged);
      staged_members += (uint32_t)__popcll(__ballot(have));
    }
    if (threadIdx.x == 0) { it_next = atomicInc(a.sched_big, 0xFFFFFFFFu); }
    __syncthreads();
    if (threadIdx.x < g && pair_misfiled<NW>(recs + threadIdx.x * RD, recs, win_at, PASS)) { ++misfiled; }
    for (uint32_t mbase = 0; mbase < g; mbase += 64u) {
      const uint32_t mslot = mbase + lane;
      const bool have = mslot < g;
      PairMember<W> m;
      pair_member_from<W>(recs + (have ? mslot : 0u) * RD, m);
      for (uint32_t t = 1u + wave; t <= half; t += (uint32_t)kWaves) {
        const bool active = have && !(2u * t == g && mslot >= half);      // g even: the opposite member is met by one of the two
        uint32_t pj = mslot + t;
        pj -= pj >= g ? g : 0u;
        pj = have ? pj : 0u;
        uint32_t p[RD];
        pair_load_record<W>(recs + pj * RD, p);
        bool twin = false;
        const bool near = active && pair_near<PASS, W, NW>(m, p, ends, twin);
        if (PASS == 0 && twin && active) { pair_twin(a, m.id, p[4 * W + 2]); }
        const uint32_t pid = p[4 * W + 2], prank = p[4 * W + 4];
        const bool e1 = near && m.ok != 0u && (ncb || m.rank <= prank);
        const bool e2 = near && p[4 * W + 5] != 0u && (ncb || prank <= m.rank);
        pair_emit(e1, e2, m.id, pid, seg, seg_room, seg_at);
      }
    }
    if (threadIdx.x == 0) { sh_big = gridDim.x + it_next; }
    __syncthreads();                                            // (also: this group's records are no longer read)
    it = sh_big;
  }
  __syncthreads();

  // ---- groups of 2..64 members: bundles of 64 / S groups of size class S, one wave per bundle ----
  // bundle numbering: the large classes first (their bundles take the most turns); upto[k] = bundles of the classes
  // 4, 3, .., 4 - k; the lists' sizes and places stay in registers (round 6: a bundle used to read its class's counter
  // from memory — the first of four dependent fetches a bundle)
  uint32_t upto[kPairClasses], cls_count[kPairClasses];
  uint64_t cls_region[kPairClasses];
  {
    uint32_t acc = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPairClasses; ++k) {
      const uint32_t c = kPairClasses - 1u - k;
      cls_count[k] = a.pair_counters[c];
      cls_region[k] = a.pair_region[c];
      acc += (cls_count[k] + (16u >> c) - 1u) >> (4u - c);
      upto[k] = acc;
    }
  }
  const uint32_t nbundles = upto[kPairClasses - 1u];
  uint32_t * const myrec = recs + (wave * 64u + lane) * RD;
  // Bundles are handed out in batches through 2^shard_bits counters (bundle numbers base << shard_bits | shard).  A visit of
  // a counter is a device-scope atomic with a return value: counters that share a cache line serve ~125 M visits a second
  // between them (measured at 10 M amplicons: pair kernels 0.78 / 1.21 / 2.2 ms with 4 / 2 / 1 bundles per visit and 8
  // adjacent counters), so (1) the counters lie kSchedStride entries apart, (2) a wave's first batch is a fixed one — the
  // counters start behind those — and (3) the visit for the NEXT batch is issued by the first bundle of the current
  // one, behind its line fetches, and is awaited only when that batch is finished: the compute of the batch hides it.
  const uint32_t kBatch = a.batch;
  const uint32_t nshards = 1u << a.shard_bits;
  const uint32_t shard = blockIdx.x & (nshards - 1u);
  uint32_t * const my_sched = a.sched_wide + (uint64_t)shard * kSchedStride;
  const uint32_t shard_waves = ((gridDim.x + nshards - 1u - shard) >> a.shard_bits) * (uint32_t)kWaves;
  uint32_t bi = 0, batch_left = 0;
  const uint32_t fixed_base = ((blockIdx.x >> a.shard_bits) * (uint32_t)kWaves + wave) * kBatch;
  bool fixed_next = true;
  uint32_t visit = 0;                                             // lane 0: what the last visit of the counter returned
  // the wave's next bundle (bi); false: none left (the counters only grow: a batch beyond the end ends the walk).  Opening
  // a batch issues the visit for the one after it; nothing touches what it returns before that batch opens (anything
  // computed from it right behind the atomic would make the wave wait for it — and for every fetch issued before it — on the spot).
  auto advance = [&]() -> bool {
    if (batch_left == 0u) {
      const uint32_t base = fixed_next ? fixed_base : (shard_waves + lane_value(visit, 0)) * kBatch;
      fixed_next = false;
      bi = (base << a.shard_bits) + shard;
      if (bi >= nbundles) { return false; }
      batch_left = kBatch;
      if (lane == 0u) { visit = atomicInc(my_sched, 0xFFFFFFFFu); }   // (counts batches.  Not atomicAdd: the compiler's wave-level
      // reduction of uniform-address additions reads the result back — a wait — right behind the atomic)
    } else {
      bi += nshards;
    }
    --batch_left;
    return bi < nbundles;                                         // (beyond the end: so is every later batch)
  };
  // bundle number -> its class (as the shift of the group size) and this lane's group: the item is fetched here
  auto describe = [&](uint32_t number, uint32_t & shift, swa_item & item) {
    uint32_t k = 0, before = 0;
#pragma unroll
    for (uint32_t q = 0; q + 1u < kPairClasses; ++q) {
      const bool past = number >= upto[q];
      k += past ? 1u : 0u;
      before = past ? upto[q] : before;
    }
    uint32_t count_c = cls_count[0];
    uint64_t region = cls_region[0];
#pragma unroll
    for (uint32_t q = 1; q < kPairClasses; ++q) {
      count_c = k == q ? cls_count[q] : count_c;
      region = k == q ? cls_region[q] : region;
    }
    shift = 2u + (kPairClasses - 1u - k);
    const uint32_t gi = (number - before) * (64u >> shift) + (lane >> shift);
    item = swa_item{0u, 0u, 0u};
    if (gi < count_c) { item = a.pair_items[region + gi]; }
  };
  // this lane's member of a described bundle: its id (0 without one)
  auto member_id = [&](uint32_t shift, const swa_item & item) -> uint32_t {
    const uint32_t jj = lane & ((1u << shift) - 1u);
    return jj < item.size ? a.ids[(uint64_t)item.begin + jj] : 0u;
  };
  // A bundle's fetches depend on each other — item, then the members' ids, then their lines — and a wave that walks that
  // chain bundle by bundle waits three times before it computes; the memory system delivers random 64-byte lines at 55 G a
  // second (tools/ubench_lines: 0.18 ms for the 10 M of a pass) when it is kept full.  So the wave runs three bundles deep
  // (round 6): while bundle i is compared, the lines of bundle i + 1, the ids of i + 2 and the item of i + 3 are on their way.
  uint32_t shift0 = 0, shift1 = 0, shift2 = 0, id0 = 0, id1 = 0, g0 = 0, g1 = 0;
  swa_item item2{0u, 0u, 0u};
  uint64_t w64[W];
  uint32_t rank = 0, len = 0;
  bool more0 = advance(), more1 = false, more2 = false;
  if (more0) {
    swa_item item0{0u, 0u, 0u}, item1{0u, 0u, 0u};
    describe(bi, shift0, item0);
    more1 = advance();
    if (more1) { describe(bi, shift1, item1); }
    id0 = member_id(shift0, item0); g0 = item0.size;
    more2 = more1 && advance();
    if (more2) { describe(bi, shift2, item2); }
    if (more1) { id1 = member_id(shift1, item1); g1 = item1.size; }
    pair_fetch_line<W>(a, (lane & ((1u << shift0) - 1u)) < g0, id0, rank, len, w64);
  }
  while (more0) {
    const uint32_t shift = shift0, S = 1u << shift;
    const uint32_t sub = lane >> shift, j = lane & (S - 1u);
    const uint32_t g = g0, half = g >> 1;
    const bool have = j < g;
    PairMember<W> m;
    pair_stage_line<W>(a, have, id0, rank, len, w64, myrec, m);
    staged_members += (uint32_t)__popcll(__ballot(have));
    // the fetches of the bundles behind this one, each a step further along its chain
    if (more1) { pair_fetch_line<W>(a, (lane & ((1u << shift1) - 1u)) < g1, id1, rank, len, w64); }
    uint32_t id2 = 0;
    if (more2) { id2 = member_id(shift2, item2); }
    const uint32_t g2 = item2.size;
    const bool more3 = more2 && advance();
    uint32_t shift3 = 0;
    swa_item item3{0u, 0u, 0u};
    if (more3) { describe(bi, shift3, item3); }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (have && pair_misfiled<NW>(myrec, recs + (wave * 64u + (sub << shift)) * RD, win_at, PASS)) { ++misfiled; }
    for (uint32_t t = 1u; t <= 32u; ++t) {
      const bool active = have && t <= half && !(2u * t == g && j >= half);
      if (__ballot(active) == 0ull) { break; }
      uint32_t pj = j + t;
      pj -= pj >= g ? g : 0u;
      pj = active ? pj : j;
      const uint32_t pslot = (sub << shift) + pj;
      uint32_t p[RD];
      pair_load_record<W>(recs + (wave * 64u + pslot) * RD, p);
      bool twin = false;
      const bool near = active && pair_near<PASS, W, NW>(m, p, ends, twin);
      if (PASS == 0 && twin && active) { pair_twin(a, m.id, p[4 * W + 2]); }
      const uint32_t pid = p[4 * W + 2], prank = p[4 * W + 4];
      const bool e1 = near && m.ok != 0u && (ncb || m.rank <= prank);
      const bool e2 = near && p[4 * W + 5] != 0u && (ncb || prank <= m.rank);
      pair_emit(e1, e2, m.id, pid, seg, seg_room, seg_at);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // (the next bundle overwrites the records)
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    more0 = more1; shift0 = shift1; id0 = id1; g0 = g1;
    more1 = more2; shift1 = shift2; id1 = id2; g1 = g2;
    more2 = more3; shift2 = shift3; item2 = item3;
  }
  if (lane == 0u) { a.seg_fill[gwave] = seg_at; a.seg_staged[gwave] = staged_members; }
  if (misfiled != 0u) { atomicAdd(a.guard + kGuardMisfiled, (unsigned long long)misfiled); }
}
