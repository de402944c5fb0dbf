// d1_common.inc — what the d = 1 network (d1.hip) and the --fastidious pass (fastidious.hip) both build on: the launch
// shape of the wave-per-amplicon kernels, the per-amplicon records of the anchored index, the amplicon lines and the
// anchor keys.  Included once by each of the two, inside its anonymous namespace, after key_ops.inc (mix64, window32).
// Types, constants and __device__ helpers only: NO KERNEL is defined here — every kernel lives in the code object of
// exactly one of the two units (d1_anchor.inc, d1_stream.inc: d1.hip; d1_fast.inc: fastidious.hip; k_d1_probe, by MODE:
// d1_probe.inc).

constexpr int kWaves = 4;                 // waves per workgroup
constexpr int kThreads = kWaves * 64;
constexpr int kQueueCap = 128;            // per-wave candidate queue (>= 64 + 63)

// value of lane `src` when src is wave-uniform: v_readlane_b32 (no LDS crossbar round trip,
// unlike ds_bpermute behind __shfl), and the result lives in an SGPR
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int src) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(src));
}
__device__ __forceinline__ uint64_t lane_value64(uint64_t v, int src) {
  return ((uint64_t)lane_value((uint32_t)(v >> 32), src) << 32) | lane_value((uint32_t)v, src);
}

struct alignas(16) swa_aux {     // per amplicon, written by k_seqhash
  uint64_t h;                    // Zobrist hash of the sequence           (XOR of Z[p][s_p])
  uint64_t dall, iall;           // XOR of Z[p-1][s_p] (p >= 1) / of Z[p+1][s_p] over all p
  uint64_t a32, d32, i32;        // the same three streams restricted to p < pb
  // pb = first position of the homopolymer run that contains position 31 (<= 31).  The passes divide a seed's
  // microvariants by what they SHARE with the seed: the prefix pass takes those that keep the first 32 nucleotides —
  // every edit at a canonical position >= 32, and the run edits (deletion of / insertion into the run around
  // position 31, listed at the run's first position by generate_variants) — so it enumerates positions >= pb against
  // the prefix group; the suffix pass takes the microvariants whose first 32 nucleotides differ (positions < 32,
  // a hit that shares the prefix is dropped).  pb = 0 (first 32 nt one run): the seed goes to the plain kernel.
  uint32_t pb;
  uint32_t pad[3];
};
static_assert(sizeof(swa_aux) == 64, "swa_aux: the record swa_d1_debug_read 3 hands out (capi.py: AUX_DTYPE)");

struct swa_item { uint32_t begin, size, chunk; };      // members [begin, begin + size) of the group-order id list; chunk (tiled kernel): row tile | column part << 6
struct swa_fallback { uint32_t seed, range; };         // range: 0 all positions, 1 the neighbours that share the prefix-side window, 2 the others

constexpr uint32_t kAnchor = 32;            // one word of an anchor window, in nucleotides
constexpr uint32_t kMinAnchoredLen = 65;    // no database whose longest sequence is shorter has anchored passes
constexpr uint32_t kGroupCap = 2048;        // (window sample: a group this large counts as stranded)
constexpr uint32_t kSeedsPerItem = 64;
// An item of the tiled kernel: a row tile of a group against up to kTiledCols of its column tiles — one a wave (round 6: it
// was the row tile against ALL its column tiles — items of 1 to 64 tiles of work; the kernel's time was its few longest items')
#ifndef SWA_TILED_COLS
#define SWA_TILED_COLS 4            // (pair passes of the Zipf set with 4 / 8 / 16: 0.60 + 0.58 / 0.63 + 0.60 / 0.67 + 0.64 ms, lease z33)
#endif
constexpr uint32_t kTiledCols = SWA_TILED_COLS;
__host__ __device__ constexpr inline uint32_t tiled_item_count(uint32_t members) {
  const uint32_t tiles = (members + kSeedsPerItem - 1u) / kSeedsPerItem;
  uint32_t items = 0;
  for (uint32_t r = 0; r < tiles; ++r) { items += (tiles - r + kTiledCols - 1u) / kTiledCols; }
  return items;
}
constexpr uint32_t kPrefetchWords = 2;      // (anchor_applicable: sequences up to 64 * 2 * 32 - 64 nt)
constexpr uint32_t kPairClasses = 5;        // size classes of the groups served by pairs in one wave: up to 4, 8, 16, 32, 64 members
constexpr uint32_t kPairBigCap = 256;       // groups of 65..this many members: by pairs in one workgroup (k_d1_group_pairs)
// Width classes (round 4; VERDICT r03 item 2).  The pair kernels keep a member's packed words in registers, W words each,
// and W is chosen per GROUP — by its longest member — not per database: one 460-nt read in a file of 150-nt reads puts its
// own groups on the 15-word kernels and nobody else's.  Class of a sequence: the smallest W in {5, 8, 15, 21} that holds it;
// kTooLong: beyond the widest kernel — its groups go to the plain kernel, like oversized ones.
constexpr uint32_t kWidthClasses = 4;
constexpr uint32_t kTooLong = kWidthClasses;
__host__ __device__ inline uint32_t width_class(uint32_t len) { return len <= 160u ? 0u : (len <= 256u ? 1u : (len <= 480u ? 2u : (len <= 672u ? 3u : kTooLong))); }
__host__ __device__ inline int width_words(uint32_t cls) { return cls == 0u ? 5 : (cls == 1u ? 8 : (cls == 2u ? 15 : 21)); }
// work lists of an index: per width class the groups by size kind — kPairClasses lists of small groups (bundles), one of
// the groups of 65..pair_big (a workgroup each), one of 64-member row tiles of the larger ones (k_d1_pairs_tiled)
constexpr uint32_t kListKinds = kPairClasses + 2;
constexpr uint32_t kListsPerIndex = kWidthClasses * kListKinds;
struct ListRegions { uint64_t at[kWidthClasses][kListKinds + 1]; };   // first item of list (class, kind) in an index's item buffer; [.][kListKinds] = end
constexpr uint32_t kSchedStride = 64;       // entries between two work counters of k_d1_group_pairs (own cache lines / channels)

// ---- amplicon lines (streaming build, d1_stream.inc): every amplicon as ONE aligned line of 64, 128 or 256 bytes (one
// stride per database, by its longest sequence: up to 160 / 480 / beyond) ---------------------------------------------------------
// dword [0] length | [1] abundance rank | [2, 2 + 2 C) packed sequence, zero padded; C = 2 quads - 1 words fit (7 / 15 / 31).
// A sequence longer than 32 C nt has its first C words there (nobody reads them: its groups go to the plain kernel).
// A reader takes the quads its own width needs: 3 of a line for W = 5, 5 for 8, 8 for 15, 11 for 21.
__host__ __device__ inline uint32_t line_capacity_words(uint32_t quads) { return 2u * quads - 1u; }

// words + length + rank of amplicon `id` from its line (W <= the line's capacity)
template <int W>
__device__ __forceinline__ void line_fetch(const uint4 * __restrict__ lines, uint32_t quads, uint32_t id, uint64_t (&w64)[W], uint32_t & len, uint32_t & rank) {
  constexpr uint32_t used = (2 * W + 2 + 3) / 4;                  // quads that carry anything
  const uint4 * L = lines + (uint64_t)id * quads;
  uint32_t d[4 * used + 2];
#pragma unroll
  for (uint32_t q = 0; q < used; ++q) { const uint4 v = L[q]; d[4 * q] = v.x; d[4 * q + 1] = v.y; d[4 * q + 2] = v.z; d[4 * q + 3] = v.w; }
  len = d[0]; rank = d[1];
#pragma unroll
  for (int k = 0; k < W; ++k) { w64[k] = (uint64_t)d[2 + 2 * k] | ((uint64_t)d[3 + 2 * k] << 32); }
}

// key of the prefix-side (which = 0) or suffix-side (which = 1) anchor window.  Normally the first / last 32 * nwin
// nucleotides (win_a = win_b = 0).  When those are (nearly) the same for everybody — conserved flanks — the windows
// move inwards: [win_a, win_a + 32 nwin) from the start, [len - win_b - 32 nwin, len - win_b) from the end ("window
// mode", chosen per database at index build).  len >= win_a + 32 nwin resp. win_b + 32 nwin.
// Width (round 4): two sequences of >= 2 w + 1 nucleotides one edit apart share their first w or their last w nucleotides
// for ANY w, and a wider window keeps a family member in its parent's group only if its edit misses the window: at w = 64
// a 150-nt family leaves (86 / 150)^2 of its pairs to each pass where w = 32 left (118 / 150)^2.  nwin = w / 32 words
// (1, 2 or 4: chosen per database from its shortest sequence, anchor_width_for); one word: the key of rounds 1-3.
constexpr uint64_t kSuffixSalt = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ uint64_t anchor_fold(const uint64_t * win, uint32_t nwin, int which) {
  uint64_t h = mix64(win[0] ^ (which ? kSuffixSalt : 0ull));
  for (uint32_t k = 1; k < nwin; ++k) { h = mix64(h ^ win[k]); }
  return h & 0x7FFFFFFFFFFFFFFFull;
}
// the 32 bits of a key record (k_keys): the top 29 bits of the mixed key — what a group is — and, below them, the width
// class of the amplicon, which k_group1 gathers into the class of the group
__device__ __forceinline__ uint32_t record_key(uint64_t mixed, uint32_t len) { return ((uint32_t)(mixed >> 32) & ~7u) | width_class(len); }
// the 29 bits a window stands for (the guard of the pair kernels)
__device__ __forceinline__ uint32_t anchor_key29(const uint64_t * win, uint32_t nwin, int which) {
  return (uint32_t)(mix64(anchor_fold(win, nwin, which)) >> 35);
}
__device__ __forceinline__ uint64_t anchor_key(const uint64_t * seq, uint32_t len, int which, uint32_t win_a, uint32_t win_b, uint32_t nwin = 1u) {
  const uint32_t pos = which == 0 ? win_a : len - win_b - kAnchor * nwin;
  uint64_t win[4] = {0ull, 0ull, 0ull, 0ull};
  for (uint32_t k = 0; k < nwin; ++k) { win[k] = window32(seq, pos + kAnchor * k); }
  return anchor_fold(win, nwin, which);
}
