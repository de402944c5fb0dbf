// dn_graph.hip — d >= 2 in BULK: every ordered pair (query, target) of amplicons whose alignment has at
// most d differences, as one CSR, without the greedy loop.
//
// The reference (src/algo.cc:384-602) interleaves the search with the clustering: one q-gram scan +
// alignment call per seed and sub-seed, against the shrinking pool — ~120 k dependent steps for 1 M
// amplicons, each a few kernels and a host round trip, which is what bounded the fused scan of
// scan.hip at 3 % of the HBM roofline.  But which pairs are within d differences does not depend on
// the pool (scan.hip's batching already relies on that), the abundance rule is a property of the
// pair, and the triangle-inequality prune (src/algo.cc:521-522) only skips pairs that cannot match.
// So the whole search is a function of the database:  G = { (q, t, diff(q, t)) : diff <= d }  —
// the same object as the d = 1 network, and the clustering becomes the host walk over it
// (cluster_dn.cpp), exactly like d = 1.
//
// Finding the pairs without comparing everything with everything: an alignment with <= d
// non-identical columns is <= d edits, so of d + 1 disjoint windows of the query (W nucleotides at
// offsets 0, W, 2W, ...) at least one is untouched, and it reappears in the target shifted by the net
// indels before it, -d .. +d.  Every amplicon is filed as a TARGET under its windows at all those
// shifts and looks itself up as a QUERY under its unshifted windows ("groups", one window at a
// time: the grouped join of group_join.inc, targets creating and queries joining); inside a group every (query < target) pair goes through: length difference, "not already
// found through an earlier window", the q-gram bound (src/qgram.cc:68-96, B3) — survivors are
// aligned by the B4 kernels (align.hip) in the direction(s) the abundance rule allows, and the
// accepted (query, target, diff) triples are sorted into a CSR (rocPRIM radix sort).
//
// The windows need room: a sequence is SHORT when it has fewer than 16 (d + 1) nucleotides.  Short sequences stay
// out of the groups, as targets and as queries, and the window length (32 or 16) is chosen from the shortest LONG
// sequence.  A pair with a short member has a length difference of at most d like every other pair, so the partner of
// a short sequence of length L has L - d .. L + d nucleotides: k_dg_brute compares every short sequence with all of
// those (the sequences below 16 (d + 1) + d, sorted by length once), the same q-gram bound, into the same pair list.
// The two parts are disjoint (a pair has a short member or it has none) and together complete; everything behind the
// pair list does not know which part a pair came from.  The brute-force part is quadratic in the short sequences, so
// the number B of its (short, partner) candidates — known from the count of sequences per length before anything is
// launched — is capped (brute_cap): beyond it, and for d > 16, the fused scan of scan.hip serves
// (swa_dn_graph_supported).  Nothing in the method depends on d; 16 is where the constants stop (kMaxShifts, SWA_DN_HIST_LEN,
// the unrolled windows of k_dg_pairs_deep).  HBM traffic: group bookkeeping (a few tens of bytes per amplicon and window) + the
// members' sequences and signatures, mostly from L2.
#include "swa_internal.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <vector>

int swa_align_launch(swa_ctx * ctx, uint32_t query, const uint32_t * d_queries, const uint32_t * d_targets,
                     const uint32_t * d_count, uint32_t max_count, uint32_t * d_diffs, uint32_t * d_scores,
                     uint32_t * d_alnlens);

namespace {

#include "wave_ops.inc"     // wave_lds_sync
#include "key_ops.inc"      // kEmpty, kKeyEmpty, mix64, window32
#include "group_join.inc"   // the window groups are a grouped join: targets create, queries join

constexpr uint32_t kTile = 4096;          // (query, target) pairs per turn of a wave
constexpr uint32_t kStride = 64;          // a group's tiles are dealt round-robin to at most this many items
constexpr int kMaxD = 16;                 // the graph route serves d <= kMaxD
constexpr int kMaxShifts = 2 * kMaxD + 1; // 2 d + 1 for d <= 16
constexpr int kSmallShifts = 17;          // ... and for d <= 8: k_dg_targets<kSmallShifts> is the kernel those d have always run

// `wlen` (<= 32) nucleotides from position pos on: window32, masked
__device__ __forceinline__ uint64_t window(const uint64_t * seq, uint32_t pos, uint32_t wlen) {
  const uint64_t v = window32(seq, pos);
  return wlen >= 32u ? v : (v & ((1ull << (2u * wlen)) - 1ull));
}

__device__ __forceinline__ uint64_t window_key(uint64_t w, uint32_t k) {
  return mix64(w ^ (0xA24BAED4963EE407ull * (uint64_t)(k + 1u))) & 0x7FFFFFFFFFFFFFFFull;
}

struct GroupArgs {
  const uint64_t * seqs;
  const uint64_t * seq_off;
  const uint32_t * seqlen;
  uint32_t n, d, k, wlen;        // window k at offset k * wlen
  uint32_t short_below;          // sequences with fewer nucleotides join no group (k_dg_brute finds their pairs)
  unsigned long long * keys;
  uint32_t * cnt_t, * cnt_q;
  uint64_t amask;
  uint32_t * tslot;              // [n * (2 d + 1)]
  uint32_t * qslot;              // [n]
  uint32_t * overflow;
  uint32_t owner_rank, owner_world;   // world > 1: only the window keys this rank owns make groups here (swa_dn_set_ownership)
};

// every amplicon (that is not short) is a target under its window k at the shifts -d .. +d (MAXS >= 2 d + 1)
template <int MAXS>
__global__ __launch_bounds__(256) void k_dg_targets(const GroupArgs a) {
  const uint32_t ns = 2u * a.d + 1u;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    const uint32_t len = a.seqlen[i];
    const bool is_short = len < a.short_below;
    const uint64_t * s = a.seqs + a.seq_off[i];
    uint64_t seen[MAXS];
    for (uint32_t j = 0; j < ns; ++j) {
      uint32_t slot = kEmpty;
      const int64_t pos = (int64_t)a.k * a.wlen + (int64_t)j - (int64_t)a.d;
      seen[j] = kKeyEmpty;
      if (!is_short && pos >= 0 && (uint64_t)pos + a.wlen <= len) {
        const uint64_t key = window_key(window(s, (uint32_t)pos, a.wlen), a.k);
        bool repeat = false;                                  // (low complexity: the same window at two shifts — one membership)
        for (uint32_t q = 0; q < j; ++q) { repeat = repeat || seen[q] == key; }
        seen[j] = key;
        // (ownership by bits of the mixed key that the table index — its low bits — does not use alone)
        const bool owned = a.owner_world == 1u || (uint32_t)((((mix64(key) >> 40) & 0xFFFFFFull) * a.owner_world) >> 24) == a.owner_rank;
        if (!repeat && owned) {
          slot = join_claim(a.keys, a.amask, key);
          if (slot != kEmpty) { atomicAdd(&a.cnt_t[slot], 1u); }
          else { *a.overflow = 1u; }
        }
      }
      a.tslot[(uint64_t)i * ns + j] = slot;
    }
  }
}

// ... and a query under the unshifted window (its own target entry at shift 0 made the group)
__global__ __launch_bounds__(256) void k_dg_queries(const GroupArgs a) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += gridDim.x * blockDim.x) {
    if (a.seqlen[i] < a.short_below) { a.qslot[i] = kEmpty; continue; }      // (a short sequence has no window k to look up)
    const uint64_t key = window_key(window(a.seqs + a.seq_off[i], a.k * a.wlen, a.wlen), a.k);
    const uint32_t slot = join_find(a.keys, a.amask, key);
    if (slot != kEmpty) { atomicAdd(&a.cnt_q[slot], 1u); }
    a.qslot[i] = slot;
  }
}

// The work items of a group (k_join_items): DnTiles, the tiles of k_dg_pairs (4096 pairs, at most kStride items a group), or
// DnBlocks, the blocks of k_dg_pairs_lds
// (kBlockT targets x kBlockQ queries each, block b = target block + target blocks x query chunk), dealt round-robin to at most
// kBlockStride items a group (item.tile = its first block).  Either way a group's items are bounded, and so is their sum:
// min(S, x y) <= 1 + sqrt(S) (x - 1 + y - 1) for x, y >= 1, so a group of t targets and q >= 1 queries makes at most
// 1 + t / 4 + q / 16 blocked items (S = 256, x = ceil(t / 64), y = ceil(q / 256)) and at most 1 + t / 8 + q / 8 tiles
// (S = 64, 4096-pair tiles); over all groups t sums to <= n (2 d + 1), q to <= n, and the groups with items number <= n
// (every one holds a query): the host's item_cap = n + n (2 d + 2) / 2 + 64 holds them (tests/test_pair_identity.py).
// Items past the cap are not dropped quietly: the join raises its flag and the search fails.
constexpr uint32_t kBlockT = 64;          // targets of a block: one per lane
constexpr uint32_t kBlockQ = 256;         // queries of a block, staged kStageQ at a time
constexpr uint32_t kStageQ = 16;
constexpr uint32_t kBlockStride = 256;    // a group's blocks are dealt round-robin to at most this many items
using DnBlocks = JoinBlocks<kBlockT, kBlockQ, kBlockStride>;
using DnTiles = JoinPairTiles<kTile, kStride>;

struct PairArgs {
  const uint64_t * seqs;
  const uint64_t * seq_off;
  const uint32_t * seqlen;
  const ulonglong2 * sigs;       // q-gram signatures, 8 x 16 bytes per amplicon
  const uint32_t * members;
  const join_item * items;
  const uint32_t * item_count;
  uint32_t item_cap;
  uint32_t d, k, wlen;
  unsigned long long * pairs;    // (query << 32) | target, query < target
  unsigned long long * counters; // [0] pairs [1] q-gram comparisons
  uint64_t pair_cap;
};

// all (query, target) pairs of a group with query < target, one pair per lane and turn
__global__ __launch_bounds__(256) void k_dg_pairs(const PairArgs a) {
  __shared__ unsigned long long stage_rows[4][kPairStage];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  PairStage stage(stage_rows, a.pairs, &a.counters[0], a.pair_cap);
  unsigned long long compared = 0;
  const uint32_t nitems = min(*a.item_count, a.item_cap);
  const uint32_t nwaves = gridDim.x * 4u;
  const int d = (int)a.d;
  for (uint32_t it = blockIdx.x * 4u + wave; it < nitems; it += nwaves) {
    const join_item item = a.items[it];
    const uint64_t npairs = (uint64_t)item.na * item.nb;
    const uint64_t ntiles = (npairs + kTile - 1) / kTile;
    const uint32_t * targets = a.members + item.begin;
    const uint32_t * queries = targets + item.na;
    for (uint64_t tile = item.tile; tile < ntiles; tile += kStride) {
      const uint64_t q0 = tile * kTile;
      const uint64_t q1 = min(q0 + (uint64_t)kTile, npairs);
      for (uint64_t qb = q0; qb < q1; qb += 64u) {
        const uint64_t p = qb + (uint64_t)lane;
        bool take = false;
        uint32_t q = 0, t = 0;
        if (p < q1) {
          const uint32_t iq = (uint32_t)(p / item.na);
          const uint32_t itg = (uint32_t)(p - (uint64_t)iq * item.na);
          q = queries[iq];
          t = targets[itg];
          if (q < t) {
            const int lq = (int)a.seqlen[q], lt = (int)a.seqlen[t];
            const int dl = lq - lt;
            if (dl >= -d && dl <= d) {
              const uint64_t * sq = a.seqs + a.seq_off[q];
              const uint64_t * st = a.seqs + a.seq_off[t];
              // the pair belongs to the FIRST window of the query that reappears (shifted) in the target
              bool earlier = false;
              for (uint32_t k2 = 0; k2 < a.k && !earlier; ++k2) {
                const uint64_t wq = window(sq, k2 * a.wlen, a.wlen);
                for (int s = -d; s <= d && !earlier; ++s) {
                  const int pos = (int)(k2 * a.wlen) + s;
                  earlier = pos >= 0 && pos + (int)a.wlen <= lt && window(st, (uint32_t)pos, a.wlen) == wq;
                }
              }
              if (!earlier) {
                // (the group key may collide: make sure window k really reappears)
                bool here = false;
                const uint64_t wq = window(sq, a.k * a.wlen, a.wlen);
                for (int s = -d; s <= d && !here; ++s) {
                  const int pos = (int)(a.k * a.wlen) + s;
                  here = pos >= 0 && pos + (int)a.wlen <= lt && window(st, (uint32_t)pos, a.wlen) == wq;
                }
                if (here) {
                  // q-gram bound (qgram_diff, src/qgram.cc:68-96): ceil(popcount(sig_q ^ sig_t) / 10) <= d
                  const ulonglong2 * gq = a.sigs + (uint64_t)q * 8u;
                  const ulonglong2 * gt = a.sigs + (uint64_t)t * 8u;
                  uint32_t pop = 0;
#pragma unroll
                  for (int w = 0; w < 8; ++w) {
                    const ulonglong2 x = gq[w], y = gt[w];
                    pop += (uint32_t)__popcll(x.x ^ y.x) + (uint32_t)__popcll(x.y ^ y.y);
                  }
                  ++compared;
                  take = (pop + 9u) / 10u <= a.d;
                }
              }
            }
          }
        }
        stage.push(take, ((unsigned long long)q << 32) | t);
      }
    }
  }
  stage.finish();
  for (int o = 32; o > 0; o >>= 1) { compared += swa_shfl_u64(compared, lane ^ o); }
  if (lane == 0 && compared != 0ull) { atomicAdd(&a.counters[1], compared); }
}

// The same pairs, block by block (r05).  k_dg_pairs computes every pair from global memory: two lengths, two offsets, up
// to (k + 1)(2 d + 1) windows cut out of the target's words and two 128-byte signatures PER PAIR — 16 ms of 57 at
// 1 M x 400, d = 3, 0.07 of the HBM roofline on bytes that mostly came from L2.  Here a wave takes a
// block of a group: 64 targets, one per lane, each with its windows at every shift (cut out once), its validity bits and
// its signature in registers; the queries pass by in LDS, kStageQ at a time — their windows, lengths, ids and
// signatures are read by all lanes at the same address (a broadcast) — so a pair costs ~2 instructions of a wave, and
// the global reads are one signature and a few words per MEMBER of the block.  D = the template's d (<= 3: 28 window
// registers); other d: k_dg_pairs.
template <int D>
__global__ __launch_bounds__(256) void k_dg_pairs_lds(const PairArgs a) {
  constexpr int NS = 2 * D + 1;
  struct QRec { uint64_t sig[16]; uint64_t win[D + 1]; uint32_t id, len; };
  __shared__ unsigned long long stage_rows[4][kPairStage];
  __shared__ QRec qrec_all[4][kStageQ];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  QRec * qrec = qrec_all[wave];
  PairStage stage(stage_rows, a.pairs, &a.counters[0], a.pair_cap);
  unsigned long long compared = 0;
  const uint32_t nitems = min(*a.item_count, a.item_cap);
  const uint32_t nwaves = gridDim.x * 4u;
  const uint32_t K = a.k;                                     // this launch's window (<= D), wave-uniform
  for (uint32_t it = blockIdx.x * 4u + wave; it < nitems; it += nwaves) {
    const join_item item = a.items[it];
    const uint32_t * targets = a.members + item.begin;
    const uint32_t * queries = targets + item.na;
    const uint32_t ntb = (item.na + kBlockT - 1u) / kBlockT;
    const uint64_t nblocks = (uint64_t)ntb * ((item.nb + kBlockQ - 1u) / kBlockQ);
    for (uint64_t blk = item.tile; blk < nblocks; blk += kBlockStride) {
      const uint32_t tb = (uint32_t)(blk % ntb), qc = (uint32_t)(blk / ntb);
      // ---- my target: windows at every shift of the windows 0 .. K, validity, signature
      const uint32_t ti = tb * kBlockT + (uint32_t)lane;
      const bool have_t = ti < item.na;
      const uint32_t t = have_t ? targets[ti] : 0u;
      const int lt = have_t ? (int)a.seqlen[t] : 0;
      const uint64_t * st = a.seqs + a.seq_off[t];
      uint64_t twin[D + 1][NS];
      uint32_t valid = 0u;
#pragma unroll
      for (int k2 = 0; k2 <= D; ++k2) {
#pragma unroll
        for (int s2 = 0; s2 < NS; ++s2) {
          const int pos = k2 * (int)a.wlen + s2 - D;
          const bool ok = have_t && (uint32_t)k2 <= K && pos >= 0 && pos + (int)a.wlen <= lt;
          twin[k2][s2] = ok ? window(st, (uint32_t)pos, a.wlen) : 0ull;
          valid |= ok ? 1u << (k2 * NS + s2) : 0u;
        }
      }
      uint64_t tsig[16];
      {
        const ulonglong2 * gt = a.sigs + (uint64_t)t * 8u;
#pragma unroll
        for (int w = 0; w < 8; ++w) { const ulonglong2 y = have_t ? gt[w] : make_ulonglong2(0ull, 0ull); tsig[2 * w] = y.x; tsig[2 * w + 1] = y.y; }
      }
      const uint32_t q_begin = qc * kBlockQ, q_end = min(item.nb, q_begin + kBlockQ);
      for (uint32_t qs = q_begin; qs < q_end; qs += kStageQ) {
        const uint32_t nq_here = min(kStageQ, q_end - qs);
        wave_lds_sync();
        // ---- the next queries into LDS: lanes [16 j', 16 j' + 16) carry the signature words of query 4 r + j'
        for (uint32_t r = 0; r < kStageQ / 4u; ++r) {
          const uint32_t j = 4u * r + ((uint32_t)lane >> 4), w = (uint32_t)lane & 15u;
          if (j < nq_here) {
            const uint32_t q = queries[qs + j];
            qrec[j].sig[w] = reinterpret_cast<const uint64_t *>(a.sigs + (uint64_t)q * 8u)[w];
          }
        }
        if ((uint32_t)lane < nq_here) {
          const uint32_t q = queries[qs + (uint32_t)lane];
          const uint64_t * sq = a.seqs + a.seq_off[q];
          qrec[lane].id = q; qrec[lane].len = a.seqlen[q];
#pragma unroll
          for (int k2 = 0; k2 <= D; ++k2) { qrec[lane].win[k2] = (uint32_t)k2 <= K ? window(sq, (uint32_t)k2 * a.wlen, a.wlen) : 0ull; }
        }
        wave_lds_sync();
        for (uint32_t j = 0; j < nq_here; ++j) {
          const uint32_t q = qrec[j].id;
          const int dl = (int)qrec[j].len - lt;
          bool take = have_t && q < t && dl >= -D && dl <= D;
          // the pair belongs to the FIRST window of the query that reappears (shifted) in the target
          bool earlier = false, here = false;
#pragma unroll
          for (int k2 = 0; k2 <= D; ++k2) {
            if ((uint32_t)k2 > K) { continue; }                  // (wave-uniform: the windows behind this launch's are nobody's business here)
            const uint64_t wq = qrec[j].win[k2];
            bool hit = false;
#pragma unroll
            for (int s2 = 0; s2 < NS; ++s2) { hit = hit || (((valid >> (k2 * NS + s2)) & 1u) != 0u && twin[k2][s2] == wq); }
            earlier = earlier || ((uint32_t)k2 < K && hit);
            here = here || ((uint32_t)k2 == K && hit);        // (the group key may collide: window K must really reappear)
          }
          take = take && !earlier && here;
          if (__ballot(take) != 0ull) {
            // q-gram bound (qgram_diff, src/qgram.cc:68-96): ceil(popcount(sig_q ^ sig_t) / 10) <= d
            uint32_t pop = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) { pop += (uint32_t)__popcll(qrec[j].sig[w] ^ tsig[w]); }
            if (take) { ++compared; }
            take = take && (pop + 9u) / 10u <= (uint32_t)D;
          }
          stage.push(take, ((unsigned long long)q << 32) | t);
        }
      }
    }
  }
  stage.finish();
  for (int o = 32; o > 0; o >>= 1) { compared += swa_shfl_u64(compared, lane ^ o); }
  if (lane == 0 && compared != 0ull) { atomicAdd(&a.counters[1], compared); }
}

// The same blocks for 9 <= d <= 16 (runtime d).  A target's windows at every shift are up to 17 x 33 words here: they fit
// neither registers nor LDS (64 targets x 561 x 8 bytes a wave).  But the windows 0 .. K at the shifts -d .. +d all lie in
// the target's first (K + 1) WLEN + d nucleotides — at most 560 (WLEN = 32) or 288 (WLEN = 16), 18 or 10 words — and those
// stay in the lane's registers.  Window k2 at all its shifts is one REGION of WLEN + 2 d <= 64 nucleotides from position
// k2 WLEN - d on: three of the words funnelled into 128 bits (which words is known at compile time: k2 is unrolled and
// 32 - d or 16 - d of the offset is a shift), and the 2 d + 1 candidates are that region moved down two bits a step — a
// few register instructions a shift, nothing from memory.  The queries pass by in LDS as in k_dg_pairs_lds (id, length,
// signature, windows 0 .. K: read by all lanes at one address).  "Not already found through an earlier window" stops as
// soon as no lane of the wave is still undecided: in a family nearly every pair shares window 0.
// Registers, not LDS, for the words (figures of the compiler for gfx950 in DESIGN.md 3.5): as an LDS column a lane they
// would add 36 KiB (WLEN = 32) to a workgroup's 25 KiB and leave two workgroups a CU.
constexpr int kDeepWindows = kMaxD + 1;
template <int WLEN>
struct DeepWords { static constexpr int value = (kDeepWindows * WLEN + kMaxD + 31) / 32; };

// does `wq` (WLEN nucleotides) occur in the target at k2 WLEN + s - d for one of the shifts s = 0 .. 2 d the target has
// room for?  tw: the target's first words; 1 <= d <= 16.
template <int WLEN, int K2, int NW>
__device__ __forceinline__ bool deep_hit(const uint64_t (&tw)[NW], uint64_t wq, int d, int lt) {
  // the region starts at nucleotide K2 WLEN - d = 32 (base - 1) + off of the target: word `base - 1` (none: zeros)
  constexpr int at = K2 * WLEN;
  constexpr int base = at / 32 + (at % 32 != 0 ? 1 : 0);
  static_assert(base + 1 < NW + 1, "the target's words end before the region does");
  const uint32_t sh = 2u * (uint32_t)((at % 32 != 0 ? 16 : 32) - d);          // 0 .. 62
  const uint64_t w0 = base >= 1 ? tw[base >= 1 ? base - 1 : 0] : 0ull;
  const uint64_t w1 = tw[base];
  const uint64_t w2 = base + 1 < NW ? tw[base + 1 < NW ? base + 1 : 0] : 0ull;
  uint64_t r0 = sh != 0u ? (w0 >> sh) | (w1 << (64u - sh)) : w0;
  uint64_t r1 = sh != 0u ? (w1 >> sh) | (w2 << (64u - sh)) : w1;
  // the shifts with the whole window inside the target: s >= d - K2 WLEN, s <= lt - (K2 + 1) WLEN + d
  const int smin = max(0, d - at), smax = min(2 * d, lt - (at + WLEN) + d);
  const uint32_t room = smax >= smin ? (uint32_t)(smax - smin + 1) : 0u;
  bool hit = false;
  for (int s = 0; s <= 2 * d; ++s) {
    const uint64_t c = WLEN >= 32 ? r0 : (r0 & ((1ull << (2 * (WLEN & 31))) - 1ull));
    hit = hit || ((uint32_t)(s - smin) < room && c == wq);
    r0 = (r0 >> 2) | (r1 << 62);
    r1 >>= 2;
  }
  return hit;
}

template <int WLEN, int K2, int NW>
struct DeepEarlier {
  // earlier |= window k2 reappears, for k2 = K2 .. K - 1, until no lane with `open` set is left without it
  static __device__ __forceinline__ void run(const uint64_t (&tw)[NW], const uint64_t * qwin, uint32_t K, int d, int lt, bool open, bool & earlier) {
    if constexpr (K2 < kDeepWindows - 1) {
      if ((uint32_t)K2 >= K || __ballot(open && !earlier) == 0ull) { return; }
      earlier = earlier || deep_hit<WLEN, K2, NW>(tw, qwin[K2], d, lt);
      DeepEarlier<WLEN, K2 + 1, NW>::run(tw, qwin, K, d, lt, open, earlier);
    }
  }
};

template <int WLEN, int K2, int NW>
struct DeepHere {
  // window K itself (wave-uniform K picks the instance)
  static __device__ __forceinline__ bool run(const uint64_t (&tw)[NW], const uint64_t * qwin, uint32_t K, int d, int lt) {
    if constexpr (K2 < kDeepWindows) {
      if ((uint32_t)K2 == K) { return deep_hit<WLEN, K2, NW>(tw, qwin[K2], d, lt); }
      return DeepHere<WLEN, K2 + 1, NW>::run(tw, qwin, K, d, lt);
    } else {
      return false;
    }
  }
};

template <int WLEN>
__global__ __launch_bounds__(256) void k_dg_pairs_deep(const PairArgs a) {
  constexpr int NW = DeepWords<WLEN>::value;
  struct QRec { uint64_t sig[16]; uint64_t win[kDeepWindows]; uint32_t id, len; };
  __shared__ unsigned long long stage_rows[4][kPairStage];
  __shared__ QRec qrec_all[4][kStageQ];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  QRec * qrec = qrec_all[wave];
  PairStage stage(stage_rows, a.pairs, &a.counters[0], a.pair_cap);
  unsigned long long compared = 0;
  const uint32_t nitems = min(*a.item_count, a.item_cap);
  const uint32_t nwaves = gridDim.x * 4u;
  const uint32_t K = a.k;                                     // this launch's window (<= d), wave-uniform
  const int d = (int)a.d;
  for (uint32_t it = blockIdx.x * 4u + wave; it < nitems; it += nwaves) {
    const join_item item = a.items[it];
    const uint32_t * targets = a.members + item.begin;
    const uint32_t * queries = targets + item.na;
    const uint32_t ntb = (item.na + kBlockT - 1u) / kBlockT;
    const uint64_t nblocks = (uint64_t)ntb * ((item.nb + kBlockQ - 1u) / kBlockQ);
    for (uint64_t blk = item.tile; blk < nblocks; blk += kBlockStride) {
      const uint32_t tb = (uint32_t)(blk % ntb), qc = (uint32_t)(blk / ntb);
      // ---- my target: its first words (only its own: what lies behind them is not read), signature
      const uint32_t ti = tb * kBlockT + (uint32_t)lane;
      const bool have_t = ti < item.na;
      const uint32_t t = have_t ? targets[ti] : 0u;
      const int lt = have_t ? (int)a.seqlen[t] : 0;
      const uint64_t * st = a.seqs + a.seq_off[t];
      uint64_t tw[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) { tw[w] = 32 * w < lt ? st[w] : 0ull; }
      uint64_t tsig[16];
      {
        const ulonglong2 * gt = a.sigs + (uint64_t)t * 8u;
#pragma unroll
        for (int w = 0; w < 8; ++w) { const ulonglong2 y = have_t ? gt[w] : make_ulonglong2(0ull, 0ull); tsig[2 * w] = y.x; tsig[2 * w + 1] = y.y; }
      }
      const uint32_t q_begin = qc * kBlockQ, q_end = min(item.nb, q_begin + kBlockQ);
      for (uint32_t qs = q_begin; qs < q_end; qs += kStageQ) {
        const uint32_t nq_here = min(kStageQ, q_end - qs);
        wave_lds_sync();
        // ---- the next queries into LDS: lanes [16 j', 16 j' + 16) carry the signature words of query 4 r + j'
        for (uint32_t r = 0; r < kStageQ / 4u; ++r) {
          const uint32_t j = 4u * r + ((uint32_t)lane >> 4), w = (uint32_t)lane & 15u;
          if (j < nq_here) {
            const uint32_t q = queries[qs + j];
            qrec[j].sig[w] = reinterpret_cast<const uint64_t *>(a.sigs + (uint64_t)q * 8u)[w];
          }
        }
        if ((uint32_t)lane < nq_here) {
          const uint32_t q = queries[qs + (uint32_t)lane];
          const uint64_t * sq = a.seqs + a.seq_off[q];
          qrec[lane].id = q; qrec[lane].len = a.seqlen[q];
          // (a query is long: it has all d + 1 windows)
          for (uint32_t k2 = 0; k2 <= K; ++k2) { qrec[lane].win[k2] = window(sq, k2 * (uint32_t)WLEN, (uint32_t)WLEN); }
        }
        wave_lds_sync();
        for (uint32_t j = 0; j < nq_here; ++j) {
          const uint32_t q = qrec[j].id;
          const int dl = (int)qrec[j].len - lt;
          bool take = have_t && q < t && dl >= -d && dl <= d;
          if (__ballot(take) == 0ull) { continue; }
          // the pair belongs to the FIRST window of the query that reappears (shifted) in the target
          bool earlier = false;
          DeepEarlier<WLEN, 0, NW>::run(tw, qrec[j].win, K, d, lt, take, earlier);
          take = take && !earlier;
          if (__ballot(take) == 0ull) { continue; }
          // (the group key may collide: window K must really reappear)
          take = take && DeepHere<WLEN, 0, NW>::run(tw, qrec[j].win, K, d, lt);
          if (__ballot(take) != 0ull) {
            // q-gram bound (qgram_diff, src/qgram.cc:68-96): ceil(popcount(sig_q ^ sig_t) / 10) <= d
            uint32_t pop = 0;
#pragma unroll
            for (int w = 0; w < 16; ++w) { pop += (uint32_t)__popcll(qrec[j].sig[w] ^ tsig[w]); }
            if (take) { ++compared; }
            take = take && (pop + 9u) / 10u <= a.d;
          }
          stage.push(take, ((unsigned long long)q << 32) | t);
        }
      }
    }
  }
  stage.finish();
  for (int o = 32; o > 0; o >>= 1) { compared += swa_shfl_u64(compared, lane ^ o); }
  if (lane == 0 && compared != 0ull) { atomicAdd(&a.counters[1], compared); }
}

// ---- the pairs with a short member -------------------------------------------------------------------------------
// The ids of all sequences below `below` nucleotides (16 (d + 1) + d: the short ones and what they can pair with) in
// the order of their lengths: start[L] = first entry of length L (from the host's counts), cursor[L] = entries placed.
// The lanes of a wave that hold the same length share one atomic.
__global__ __launch_bounds__(256) void k_dg_short_sort(const uint32_t * __restrict__ seqlen, uint32_t n, uint32_t below,
                                                       const uint32_t * __restrict__ start, uint32_t * cursor,
                                                       uint32_t * __restrict__ sorted, uint32_t cap) {
  const int lane = threadIdx.x & 63;
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  const uint64_t first = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~63ull;     // wave-uniform
  for (uint64_t i0 = first; i0 < n; i0 += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = i0 + (uint64_t)lane;
    const uint32_t len = i < n ? seqlen[i] : below;
    const bool near = len < below;
    uint64_t todo = __ballot(near);
    while (todo != 0ull) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t L = (uint32_t)__shfl((int)len, leader, 64);
      const uint64_t m = __ballot(near && len == L);
      uint32_t base = 0;
      if (lane == leader) { base = atomicAdd(&cursor[L], (uint32_t)__popcll(m)); }
      base = (uint32_t)__shfl((int)base, leader, 64);
      if (near && len == L) {
        const uint32_t at = start[L] + base + (uint32_t)__popcll(m & lane_lt);
        if (at < cap) { sorted[at] = (uint32_t)i; }
      }
      todo &= ~m;
    }
  }
}

struct BruteArgs {
  const uint32_t * seqlen;
  const ulonglong2 * sigs;       // q-gram signatures, 8 x 16 bytes per amplicon
  const uint32_t * sorted;       // k_dg_short_sort's list: entries [0, nshort) are the short sequences
  const uint32_t * start;        // [short_below + d + 1]
  uint32_t nshort, short_below, d;
  uint32_t tile, ntiles;         // a short sequence's partners are dealt to ntiles waves, `tile` (a multiple of 64) each
  uint32_t owner_rank, owner_world;   // world > 1: only the short sequences with id % world == rank emit here
  unsigned long long * pairs;    // (lower id << 32) | higher id, as k_dg_pairs
  unsigned long long * counters; // [0] pairs [1] q-gram comparisons
  uint64_t pair_cap;
};

// One wave per short sequence s and tile of its partners — the sequences of len(s) - d .. len(s) + d nucleotides, a
// contiguous range of the sorted list: the signature of s in (scalar) registers, one partner per lane and turn.  A pair
// of two short sequences is emitted by the one with the lower id.  The q-gram bound and the staging of the survivors
// are k_dg_pairs'.
__global__ __launch_bounds__(256) void k_dg_brute(const BruteArgs a) {
  __shared__ unsigned long long stage_rows[4][kPairStage];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  PairStage stage(stage_rows, a.pairs, &a.counters[0], a.pair_cap);
  unsigned long long compared = 0;
  const uint64_t nitems = (uint64_t)a.nshort * a.ntiles;
  const uint64_t nwaves = (uint64_t)gridDim.x * 4u;
  const uint32_t top = a.short_below + a.d;                  // start[] has top + 1 entries
  for (uint64_t it = (uint64_t)blockIdx.x * 4u + (uint64_t)wave; it < nitems; it += nwaves) {
    const uint32_t si = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(it / a.ntiles));
    const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(it % a.ntiles));
    const uint32_t s = a.sorted[si];
    if (a.owner_world != 1u && s % a.owner_world != a.owner_rank) { continue; }
    const uint32_t len = a.seqlen[s];
    const uint32_t lo = len > a.d ? len - a.d : 0u, hi = min(len + a.d + 1u, top);
    const uint64_t r0 = (uint64_t)a.start[lo] + (uint64_t)tile * a.tile;
    const uint64_t r1 = min((uint64_t)a.start[hi], r0 + a.tile);
    if (r0 >= r1) { continue; }
    uint64_t ssig[16];
    {
      const ulonglong2 * gs = a.sigs + (uint64_t)s * 8u;
#pragma unroll
      for (int w = 0; w < 8; ++w) { const ulonglong2 x = gs[w]; ssig[2 * w] = x.x; ssig[2 * w + 1] = x.y; }
    }
    for (uint64_t r = r0; r < r1; r += 64u) {
      const uint64_t at = r + (uint64_t)lane;
      bool take = false;
      uint32_t p = 0;
      if (at < r1) {
        p = a.sorted[at];
        // (entries below nshort are short themselves: that pair belongs to the lower id of the two)
        if (p != s && !(at < a.nshort && p < s)) {
          // q-gram bound (qgram_diff, src/qgram.cc:68-96): ceil(popcount(sig_s ^ sig_p) / 10) <= d
          const ulonglong2 * gp = a.sigs + (uint64_t)p * 8u;
          uint32_t pop = 0;
#pragma unroll
          for (int w = 0; w < 8; ++w) {
            const ulonglong2 y = gp[w];
            pop += (uint32_t)__popcll(ssig[2 * w] ^ y.x) + (uint32_t)__popcll(ssig[2 * w + 1] ^ y.y);
          }
          ++compared;
          take = (pop + 9u) / 10u <= a.d;
        }
      }
      stage.push(take, ((unsigned long long)min(s, p) << 32) | max(s, p));
    }
  }
  stage.finish();
  for (int o = 32; o > 0; o >>= 1) { compared += swa_shfl_u64(compared, lane ^ o); }
  if (lane == 0 && compared != 0ull) { atomicAdd(&a.counters[1], compared); }
}

// the alignments a pair needs: (a, b) with a < b always (db order is abundance-descending, so b's
// abundance is not the larger one); (b, a) as well when the abundance rule allows it: equal abundances,
// or no rule (-n).  Queries / targets of the second kind are appended behind the first npairs entries.
__global__ __launch_bounds__(256) void k_dg_worklist(const unsigned long long * __restrict__ pairs, uint64_t npairs,
                                                     const uint64_t * __restrict__ abundance, int ncb, uint32_t * __restrict__ wq,
                                                     uint32_t * __restrict__ wt, unsigned long long * extra_counter) {
  // (2048 pairs a workgroup and turn, ONE atomic for the second directions it adds — see k_dg_edges)
  constexpr uint32_t kPer = 8;
  __shared__ uint32_t wave_sum[4];
  __shared__ unsigned long long block_base;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t p0 = (uint64_t)blockIdx.x * (256u * kPer); p0 < npairs; p0 += (uint64_t)gridDim.x * (256u * kPer)) {
    uint32_t qa[kPer], tb[kPer];
    uint32_t both = 0u, mine = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint64_t p = p0 + (uint64_t)k * 256u + threadIdx.x;
      qa[k] = 0u; tb[k] = 0u;
      if (p < npairs) {
        const unsigned long long pr = pairs[p];
        qa[k] = (uint32_t)(pr >> 32); tb[k] = (uint32_t)pr;
        wq[p] = qa[k]; wt[p] = tb[k];
        if (ncb != 0 || abundance[qa[k]] == abundance[tb[k]]) { both |= 1u << k; ++mine; }
      }
    }
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, (unsigned)o, 64); if ((int)lane >= o) { incl += up; } }
    if (lane == 63u) { wave_sum[wave] = incl; }
    __syncthreads();
    uint32_t before = incl - mine, total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) { before += w < wave ? wave_sum[w] : 0u; total += wave_sum[w]; }
    if (threadIdx.x == 0 && total != 0u) { block_base = atomicAdd(extra_counter, (unsigned long long)total); }
    __syncthreads();
    if (both != 0u) {
      uint64_t at = npairs + block_base + before;
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) {
        if ((both >> k & 1u) != 0u) { wq[at] = tb[k]; wt[at] = qa[k]; ++at; }
      }
    }
    __syncthreads();
  }
}

// Round 6: the work list in the order of the alignments' expected length.  k_align_wfa runs a wave — four pairs — until its
// LAST pair is done: a pair within d stops at its score, a pair beyond d takes every step; in the order the pair kernels
// found them nearly every wave holds one of the latter.  Ordered by the q-gram distance of the two signatures (what the
// filter measured: 0..30 differing bits for the pairs it let through) plus ten a nucleotide of length difference (a gap
// costs more than a mismatch), pairs that stop early share their waves.
// key[i] for the work list's item i (both directions carry their pair's key).
__global__ __launch_bounds__(256) void k_dg_work_keys(const uint32_t * __restrict__ wq, const uint32_t * __restrict__ wt, uint64_t nwork,
                                                      const ulonglong2 * __restrict__ sigs, const uint32_t * __restrict__ seqlen, uint32_t len_weight,
                                                      unsigned char * __restrict__ key, unsigned long long * __restrict__ packed) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwork; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t q = wq[i], t = wt[i];
    const ulonglong2 * sq = sigs + (uint64_t)q * 8u;
    const ulonglong2 * st = sigs + (uint64_t)t * 8u;
    uint32_t pop = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) { const ulonglong2 x = sq[w], y = st[w]; pop += (uint32_t)__popcll(x.x ^ y.x) + (uint32_t)__popcll(x.y ^ y.y); }
    const uint32_t lq = seqlen[q], lt = seqlen[t];
    key[i] = (unsigned char)min(pop + len_weight * (max(lq, lt) - min(lq, lt)), 63u);
    packed[i] = ((unsigned long long)q << 32) | t;
  }
}
__global__ __launch_bounds__(256) void k_dg_work_unpack(const unsigned long long * __restrict__ packed, uint64_t nwork, uint32_t * __restrict__ wq,
                                                        uint32_t * __restrict__ wt) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwork; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long v = packed[i];
    wq[i] = (uint32_t)(v >> 32); wt[i] = (uint32_t)v;
  }
}

// accepted alignments -> (query << 32 | target) keys + diffs, compacted.  A workgroup takes 2048 work items a turn — eight a
// thread — and appends what it keeps with ONE atomic on the counter (a single address takes ~90 atomics a microsecond: one
// per wave of 64 items was 50 000 of them, 0.55 of this kernel's 0.60 ms at 3.2 M items; round 6)
__global__ __launch_bounds__(256) void k_dg_edges(const uint32_t * __restrict__ wq, const uint32_t * __restrict__ wt,
                                                  const uint32_t * __restrict__ diffs, uint64_t count, uint32_t d,
                                                  unsigned long long * __restrict__ keys, uint32_t * __restrict__ vals,
                                                  unsigned long long * edge_counter) {
  constexpr uint32_t kPer = 8;
  __shared__ uint32_t wave_sum[4];
  __shared__ unsigned long long block_base;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint64_t e0 = (uint64_t)blockIdx.x * (256u * kPer); e0 < count; e0 += (uint64_t)gridDim.x * (256u * kPer)) {
    uint32_t dv[kPer];
    uint32_t keep = 0u, mine = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint64_t e = e0 + (uint64_t)k * 256u + threadIdx.x;
      dv[k] = e < count ? diffs[e] : 0xFFFFFFFFu;
      if (e < count && dv[k] <= d) { keep |= 1u << k; ++mine; }
    }
    // the thread's place among the workgroup's kept items: a wave scan + the waves before
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, (unsigned)o, 64); if ((int)lane >= o) { incl += up; } }
    if (lane == 63u) { wave_sum[wave] = incl; }
    __syncthreads();
    uint32_t before = incl - mine, total = 0u;
#pragma unroll
    for (uint32_t w = 0; w < 4u; ++w) { before += w < wave ? wave_sum[w] : 0u; total += wave_sum[w]; }
    if (threadIdx.x == 0 && total != 0u) { block_base = atomicAdd(edge_counter, (unsigned long long)total); }
    __syncthreads();
    if (keep != 0u) {
      uint64_t at = block_base + before;
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) {
        if ((keep >> k & 1u) != 0u) {
          const uint64_t e = e0 + (uint64_t)k * 256u + threadIdx.x;
          keys[at] = ((unsigned long long)wq[e] << 32) | wt[e];
          vals[at] = dv[k];
          ++at;
        }
      }
    }
    __syncthreads();
  }
}

// sorted keys -> CSR: offsets[i] = first key >= i << 32; neighbours / diffs split out of the sorted arrays
__global__ __launch_bounds__(256) void k_dg_offsets(const unsigned long long * __restrict__ keys, uint64_t count, uint32_t n,
                                                    uint64_t * __restrict__ offsets) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long want = (unsigned long long)i << 32;
    uint64_t lo = 0, hi = count;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (keys[mid] < want) { lo = mid + 1; } else { hi = mid; } }
    offsets[i] = lo;
  }
}

__global__ __launch_bounds__(256) void k_dg_split(const unsigned long long * __restrict__ keys, const uint32_t * __restrict__ vals,
                                                  uint64_t count, uint32_t * __restrict__ neighbours, uint8_t * __restrict__ diffs) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x) {
    neighbours[i] = (uint32_t)keys[i];
    diffs[i] = (uint8_t)vals[i];
  }
}

// diff of the link parent[v] -> v (rows ascending: binary search), 0 for a seed
__global__ __launch_bounds__(256) void k_dg_parent_diffs(const uint64_t * __restrict__ offsets, const uint32_t * __restrict__ nb,
                                                         const uint8_t * __restrict__ df, const uint32_t * __restrict__ parent, uint32_t n,
                                                         uint8_t * __restrict__ out) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) {
    const uint32_t p = parent[v];
    uint8_t d = 0;
    if (p != SWA_NO_AMPLICON) {
      uint64_t at;
      d = swa_row_find(offsets, nb, p, v, at) ? df[at] : (uint8_t)0xFF;
    }
    out[v] = d;
  }
}

// how many sequences have each length below SWA_DN_HIST_LEN (out[L]) and the shortest of the others (out[SWA_DN_HIST_LEN])
__global__ __launch_bounds__(256) void k_dg_lengths(const uint32_t * __restrict__ seqlen, uint32_t n, uint32_t * out) {
  __shared__ uint32_t hist[SWA_DN_HIST_LEN];
  for (uint32_t i = threadIdx.x; i < SWA_DN_HIST_LEN; i += blockDim.x) { hist[i] = 0u; }
  __syncthreads();
  uint32_t mn = 0xFFFFFFFFu;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t len = seqlen[i];
    if (len < SWA_DN_HIST_LEN) { atomicAdd(&hist[len], 1u); } else { mn = min(mn, len); }
  }
  for (int o = 32; o > 0; o >>= 1) { mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64)); }
  if ((threadIdx.x & 63u) == 0u && mn != 0xFFFFFFFFu) { atomicMin(out + SWA_DN_HIST_LEN, mn); }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < SWA_DN_HIST_LEN; i += blockDim.x) { if (hist[i] != 0u) { atomicAdd(out + i, hist[i]); } }
}

struct widen_u32 {
  __host__ __device__ uint64_t operator()(uint32_t v) const { return (uint64_t)v; }
};

// d_frole (the fastidious pair route's buffer, idle at d >= 2) in u32 words: the length counts as k_dg_lengths leaves
// them, then what the brute-force part reads — start[] and cursor[] per length and the ids sorted by length
constexpr uint32_t kShortStart = 320, kShortCursor = 640, kShortSorted = 960;
static_assert(kShortStart >= SWA_DN_HIST_LEN + 1u && kShortCursor >= kShortStart + SWA_DN_HIST_LEN + 1u && kShortSorted >= kShortCursor + SWA_DN_HIST_LEN, "d_frole layout");

// what the database's lengths decide for this d
struct dn_plan {
  uint32_t wlen = 0;             // window length: 32, 16, or 0 (the graph route does not serve this database)
  uint32_t short_below = 0;      // 16 (d + 1): sequences below it are short
  uint32_t nshort = 0, nnear = 0;   // short sequences; sequences below short_below + d (what a short one can pair with)
  uint32_t max_range = 0;        // most partners of one short sequence
  uint64_t brute = 0;            // B: (short, partner) candidates, every pair once
};

// the cap on B: the size the pair list starts with (every candidate may survive the q-gram bound), or SWA_DN_BRUTE_CAP
uint64_t brute_cap(uint32_t n) {
  const char * env = std::getenv("SWA_DN_BRUTE_CAP");
  if (env != nullptr && env[0] != '\0') { return std::strtoull(env, nullptr, 10); }
  return 16ull * n + (1ull << 20);
}

int window_length(swa_ctx * ctx, uint32_t d, dn_plan * out) {
  if (ctx->up.dn_shortest == 0) {
    SWA_TRY(swa_reserve(ctx, ctx->d_frole, (uint64_t)kShortSorted * sizeof(uint32_t)));
    auto * slot = static_cast<uint32_t *>(ctx->d_frole.ptr);
    SWA_HIP(ctx, hipMemsetAsync(slot, 0, SWA_DN_HIST_LEN * sizeof(uint32_t), ctx->stream));
    SWA_HIP(ctx, hipMemsetAsync(slot + SWA_DN_HIST_LEN, 0xFF, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_dg_lengths, dim3(swa_grid256(ctx, ctx->db.n)), dim3(256), 0, ctx->stream, ctx->db.seqlen, ctx->db.n, slot);
    uint32_t got[SWA_DN_HIST_LEN + 1];
    SWA_HIP(ctx, hipMemcpyAsync(got, slot, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t mn = got[SWA_DN_HIST_LEN];
    for (uint32_t L = SWA_DN_HIST_LEN; L-- > 0;) { ctx->up.dn_len_hist[L] = got[L]; if (got[L] != 0u) { mn = L; } }
    ctx->up.dn_shortest_rest = got[SWA_DN_HIST_LEN];
    ctx->up.dn_shortest = mn;
  }
  *out = dn_plan();
  if (d > (uint32_t)kMaxD) { return SWA_OK; }
  const uint32_t * hist = ctx->up.dn_len_hist;
  const uint32_t T = 16u * (d + 1u), top = T + d;              // (d <= 16: top <= SWA_DN_HIST_LEN)
  out->short_below = T;
  uint32_t shortest_long = ctx->up.dn_shortest_rest;
  for (uint32_t L = SWA_DN_HIST_LEN; L-- > T;) { if (hist[L] != 0u) { shortest_long = L; } }
  // (no long sequence at all: the windows find nothing whatever their length)
  out->wlen = shortest_long >= 32u * (d + 1u) && shortest_long != 0xFFFFFFFFu ? 32u : 16u;
  for (uint32_t L = 0; L < top; ++L) { out->nnear += hist[L]; if (L < T) { out->nshort += hist[L]; } }
  if (out->nshort == 0) { return SWA_OK; }
  // B: a short sequence of length L meets every other sequence of L - d .. L + d nucleotides; two short ones meet once
  for (uint32_t L = 0; L < T; ++L) {
    if (hist[L] == 0u) { continue; }
    uint64_t range = 0, later = 0;
    for (uint32_t M = L > d ? L - d : 0u; M <= L + d; ++M) {
      range += hist[M];
      if (M > L) { later += hist[M]; }
    }
    out->max_range = (uint32_t)std::max<uint64_t>(out->max_range, range);
    out->brute += (uint64_t)hist[L] * (hist[L] - 1u) / 2u + (uint64_t)hist[L] * later;
  }
  if (out->brute > brute_cap(ctx->db.n)) { out->wlen = 0; }
  return SWA_OK;
}

}  // namespace

extern "C" int swa_dn_graph_supported(swa_ctx * ctx) {
  if (ctx == nullptr || !ctx->search_ready || ctx->db.n == 0) { return 0; }
  dn_plan plan;
  if (window_length(ctx, (uint32_t)ctx->resolution, &plan) != SWA_OK) { return 0; }
  return plan.wlen != 0 ? 1 : 0;
}

// the search itself: the sorted (query << 32 | target, diff) list of this context's share of the graph, left in HBM
int swa_dn_graph_compute(swa_ctx * ctx, int no_cluster_breaking) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (!ctx->up.qgram_ready || !ctx->search_ready) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_dn_graph: call swa_qgram_build and swa_search_begin first");
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->db.n;
  const uint32_t d = (uint32_t)ctx->resolution;
  dn_plan plan;
  SWA_TRY(window_length(ctx, d, &plan));
  const uint32_t wlen = plan.wlen;
  if (wlen == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_dn_graph: a sequence is too short for d + 1 windows (use the scan)"); }

  if (!ctx->up.dn_graph_ready || ctx->up.dn_graph_ncb != (no_cluster_breaking != 0)) {
    const uint32_t ns = 2u * d + 1u;
    uint64_t asize = 64;
    while (asize < 2ull * n * ns) { asize <<= 1; }
    const uint64_t member_cap = (uint64_t)n * (ns + 1u);
    const uint64_t item_cap64 = (uint64_t)n + member_cap / 2 + 64;
    const uint32_t item_cap = item_cap64 > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)item_cap64;
    SWA_TRY(join_reserve(ctx, asize, n, ns, member_cap, item_cap));
    SWA_TRY(swa_reserve(ctx, ctx->d_fcounters, 16 * sizeof(uint64_t)));
    const JoinTable jt = join_table(ctx, asize, n, ns);
    auto tot64 = rocprim::make_transform_iterator(jt.tot, widen_u32());
    size_t scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, scan_bytes, tot64, jt.offsets, (uint64_t)0, asize + 1, rocprim::plus<uint64_t>(), ctx->stream);
    SWA_TRY(swa_reserve(ctx, ctx->d_scan_tmp, scan_bytes + 16));
    auto scan = [&](const JoinTable &) -> int {
      SWA_HIP(ctx, rocprim::exclusive_scan(ctx->d_scan_tmp.ptr, scan_bytes, tot64, jt.offsets, (uint64_t)0, asize + 1, rocprim::plus<uint64_t>(),
                                           ctx->stream));
      return SWA_OK;
    };
    auto * fc = static_cast<unsigned long long *>(ctx->d_fcounters.ptr);   // [0] pairs [1] comparisons [2] extra directions [3] edges
    if (ctx->dn_pair_cap == 0) { ctx->dn_pair_cap = 16ull * n + (1ull << 20); }
    uint64_t npairs = 0;
    uint64_t launches = 0;
    for (int slot : {kTimePairs, kTimeAlign}) { ctx->ev_used[slot] = false; }
    swa_t0(ctx, kTimePairs);                                            // (groups + pairs; kTimeAlign: alignments + CSR)
    // the short sequences and what they can pair with, by length (once: a regrow repeats only the search)
    BruteArgs br{};
    if (plan.nshort != 0) {
      const uint32_t top = plan.short_below + d;
      SWA_TRY(swa_reserve(ctx, ctx->d_frole, ((uint64_t)kShortSorted + plan.nnear) * sizeof(uint32_t)));
      auto * words = static_cast<uint32_t *>(ctx->d_frole.ptr);
      uint32_t start[SWA_DN_HIST_LEN + 1];
      start[0] = 0;
      for (uint32_t L = 0; L < top; ++L) { start[L + 1] = start[L] + ctx->up.dn_len_hist[L]; }
      SWA_HIP(ctx, hipMemcpyAsync(words + kShortStart, start, (top + 1u) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
      SWA_HIP(ctx, hipMemsetAsync(words + kShortCursor, 0, top * sizeof(uint32_t), ctx->stream));
      hipLaunchKernelGGL(k_dg_short_sort, dim3(swa_grid256(ctx, n)), dim3(256), 0, ctx->stream, ctx->db.seqlen, n, top, words + kShortStart,
                         words + kShortCursor, words + kShortSorted, plan.nnear);
      SWA_HIP(ctx, hipGetLastError());
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (start[] is on this stack)
      ++launches;
      br.seqlen = ctx->db.seqlen; br.sigs = static_cast<const ulonglong2 *>(ctx->d_qgrams.ptr);
      br.sorted = words + kShortSorted; br.start = words + kShortStart;
      br.nshort = plan.nshort; br.short_below = plan.short_below; br.d = d;
      // enough waves to fill the device when the short sequences are few, one wave each when they are many
      const uint32_t want_tiles = std::max<uint32_t>(1u, 16384u / plan.nshort);
      br.ntiles = std::min<uint32_t>(want_tiles, (plan.max_range + 255u) / 256u);
      br.ntiles = std::max<uint32_t>(1u, br.ntiles);
      br.tile = ((plan.max_range + br.ntiles - 1u) / br.ntiles + 63u) & ~63u;
      br.owner_rank = ctx->dn_owner_rank; br.owner_world = ctx->dn_owner_world;
      br.counters = fc;
    }
    for (int attempt = 0; attempt < 6; ++attempt) {
      SWA_TRY(swa_reserve(ctx, ctx->d_fpairs, ctx->dn_pair_cap * sizeof(uint64_t)));
      SWA_HIP(ctx, hipMemsetAsync(fc, 0, 8 * sizeof(uint64_t), ctx->stream));
      SWA_HIP(ctx, hipMemsetAsync(jt.flags, 0, kJoinItemCount * sizeof(uint32_t), ctx->stream));
      for (uint32_t k = 0; k <= d; ++k) {
        GroupArgs g{};
        g.seqs = ctx->db.seqs; g.seq_off = ctx->db.seq_off; g.seqlen = ctx->db.seqlen; g.n = n; g.d = d; g.k = k; g.wlen = wlen; g.short_below = plan.short_below;
        g.keys = jt.keys; g.cnt_t = jt.cnt_a; g.cnt_q = jt.cnt_b; g.amask = asize - 1; g.tslot = jt.aslot; g.qslot = jt.bslot; g.overflow = jt.flags + kJoinKeyOverflow;
        g.owner_rank = ctx->dn_owner_rank; g.owner_world = ctx->dn_owner_world;
        auto key_kernels = [&](dim3 gn, dim3 b) {
          if (ns <= (uint32_t)kSmallShifts) { hipLaunchKernelGGL(k_dg_targets<kSmallShifts>, gn, b, 0, ctx->stream, g); }
          else { hipLaunchKernelGGL(k_dg_targets<kMaxShifts>, gn, b, 0, ctx->stream, g); }
          hipLaunchKernelGGL(k_dg_queries, gn, b, 0, ctx->stream, g);
        };
        uint32_t * item_count = jt.flags + kJoinItemCount;
        SWA_HIP(ctx, hipMemsetAsync(item_count, 0, sizeof(uint32_t), ctx->stream));
        // blocks of 64 targets x 256 queries for the LDS kernels (d = 2, 3 and 9 .. 16; the per-pair kernel for other d);
        // a group needs a pair of DIFFERENT amplicons (an amplicon alone is its own target): t q >= 2
        const bool deep = d >= 9u;
        const bool blocked = d == 2u || d == 3u || deep;
        if (blocked) { SWA_TRY(join_run<DnBlocks>(ctx, jt, 2u, item_count, item_cap, key_kernels, scan)); }
        else { SWA_TRY(join_run<DnTiles>(ctx, jt, 2u, item_count, item_cap, key_kernels, scan)); }
        PairArgs p{};
        p.seqs = ctx->db.seqs; p.seq_off = ctx->db.seq_off; p.seqlen = ctx->db.seqlen;
        p.sigs = static_cast<const ulonglong2 *>(ctx->d_qgrams.ptr);
        p.members = jt.members; p.items = jt.items; p.item_count = item_count; p.item_cap = item_cap; p.d = d; p.k = k; p.wlen = wlen;
        p.pairs = static_cast<unsigned long long *>(ctx->d_fpairs.ptr); p.counters = fc; p.pair_cap = ctx->dn_pair_cap;
        if (deep && wlen == 32u) { hipLaunchKernelGGL(k_dg_pairs_deep<32>, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, p); }
        else if (deep) { hipLaunchKernelGGL(k_dg_pairs_deep<16>, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, p); }
        else if (blocked && d == 2u) { hipLaunchKernelGGL(k_dg_pairs_lds<2>, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, p); }
        else if (blocked) { hipLaunchKernelGGL(k_dg_pairs_lds<3>, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, p); }
        else { hipLaunchKernelGGL(k_dg_pairs, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, p); }
        SWA_HIP(ctx, hipGetLastError());
        launches += 9;
      }
      if (plan.nshort != 0) {
        br.pairs = static_cast<unsigned long long *>(ctx->d_fpairs.ptr); br.pair_cap = ctx->dn_pair_cap;
        const uint64_t blocks = ((uint64_t)br.nshort * br.ntiles + 3u) / 4u;
        hipLaunchKernelGGL(k_dg_brute, dim3((unsigned)std::min<uint64_t>(blocks, (uint64_t)ctx->num_cus * 8u)), dim3(256), 0, ctx->stream, br);
        SWA_HIP(ctx, hipGetLastError());
        ++launches;
      }
      uint64_t got[2] = {0, 0};
      SWA_TRY(join_status(ctx, jt, fc, 2, got, "swa_dn_graph: group key table overflow",
                          "swa_dn_graph: the work items of a window outgrew item_cap"));
      ctx->dn_comparisons = got[1];
      if (got[0] <= ctx->dn_pair_cap) { npairs = got[0]; break; }
      if (attempt == 5) { return swa_fail_msg(ctx, SWA_E_NOMEM, "swa_dn_graph: pair list keeps overflowing"); }
      ctx->dn_pair_cap = got[0] + 1024;
    }
    swa_t1(ctx, kTimePairs);
    // alignments in the direction(s) the abundance rule allows
    swa_t0(ctx, kTimeAlign);
    uint64_t nedges = 0;
    if (npairs != 0) {
      SWA_TRY(swa_reserve(ctx, ctx->d_scan_targets, 4 * npairs * sizeof(uint32_t)));        // queries | targets, both directions
      SWA_TRY(swa_reserve(ctx, ctx->d_scan_diffs, 2 * npairs * sizeof(uint32_t)));
      auto * wq = static_cast<uint32_t *>(ctx->d_scan_targets.ptr);
      auto * wt = wq + 2 * npairs;
      auto * wd = static_cast<uint32_t *>(ctx->d_scan_diffs.ptr);
      hipLaunchKernelGGL(k_dg_worklist, dim3(swa_grid256(ctx, npairs)), dim3(256), 0, ctx->stream,
                         static_cast<const unsigned long long *>(ctx->d_fpairs.ptr), npairs, ctx->db.abundance, no_cluster_breaking,
                         wq, wt, fc + 2);
      uint64_t extra = 0;
      SWA_HIP(ctx, hipMemcpyAsync(&extra, fc + 2, sizeof(extra), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      const uint64_t nwork = npairs + extra;
      ctx->dn_aligned = nwork;
      // the wavefront kernel's work in the order of its expected length (k_dg_work_keys)
      constexpr uint32_t kAlignLenWeight = 10;   // (a nucleotide of length difference counts as ten signature bits: alignments + CSR 6.9-7.1 -> 6.5-6.6 ms against 0; 5 and 20: 7.0 / 6.8)
      if (nwork > 1 && ctx->d_qgrams.ptr != nullptr) {
        SWA_TRY(swa_reserve(ctx, ctx->d_dn_keys, 2 * nwork * sizeof(uint64_t)));          // packed items: in | out (the edges' keys later)
        SWA_TRY(swa_reserve(ctx, ctx->d_dn_vals, 2 * nwork * sizeof(uint32_t)));          // keys: in | out (bytes; the edges' values later)
        auto * packed = static_cast<unsigned long long *>(ctx->d_dn_keys.ptr);
        auto * wkey = static_cast<unsigned char *>(ctx->d_dn_vals.ptr);
        hipLaunchKernelGGL(k_dg_work_keys, dim3(swa_grid256(ctx, nwork)), dim3(256), 0, ctx->stream, wq, wt, nwork,
                           static_cast<const ulonglong2 *>(ctx->d_qgrams.ptr), ctx->db.seqlen, kAlignLenWeight, wkey, packed);
        size_t order_bytes = 0;
        (void)rocprim::radix_sort_pairs(nullptr, order_bytes, wkey, wkey + nwork, packed, packed + nwork, nwork, 0, 6, ctx->stream);
        SWA_TRY(swa_reserve(ctx, ctx->d_scan_hits, order_bytes + 16));
        SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, order_bytes, wkey, wkey + nwork, packed, packed + nwork, nwork, 0, 6, ctx->stream));
        hipLaunchKernelGGL(k_dg_work_unpack, dim3(swa_grid256(ctx, nwork)), dim3(256), 0, ctx->stream, packed + nwork, nwork, wq, wt);
        launches += 4;
      }
      // (the launcher takes 32-bit counts: in slices)
      for (uint64_t at = 0; at < nwork; at += 0x40000000ull) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(0x40000000ull, nwork - at);
        SWA_TRY(swa_align_launch(ctx, 0, wq + at, wt + at, nullptr, cnt, wd + at, nullptr, nullptr));
        ++launches;
      }
      SWA_TRY(swa_reserve(ctx, ctx->d_dn_keys, 2 * nwork * sizeof(uint64_t)));
      SWA_TRY(swa_reserve(ctx, ctx->d_dn_vals, 2 * nwork * sizeof(uint32_t)));
      auto * ekeys = static_cast<unsigned long long *>(ctx->d_dn_keys.ptr);
      auto * evals = static_cast<uint32_t *>(ctx->d_dn_vals.ptr);
      hipLaunchKernelGGL(k_dg_edges, dim3(swa_grid256(ctx, nwork)), dim3(256), 0, ctx->stream, wq, wt, wd, nwork, d, ekeys, evals, fc + 3);
      SWA_HIP(ctx, hipMemcpyAsync(&nedges, fc + 3, sizeof(nedges), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (nedges != 0) {
        size_t sort_bytes = 0;
        (void)rocprim::radix_sort_pairs(nullptr, sort_bytes, ekeys, ekeys + nwork, evals, evals + nwork, nedges, 0, 64, ctx->stream);
        SWA_TRY(swa_reserve(ctx, ctx->d_scan_hits, sort_bytes + 16));
        SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, sort_bytes, ekeys, ekeys + nwork, evals, evals + nwork, nedges, 0, 64,
                                               ctx->stream));
        launches += 6;
      }
    }
    swa_t1(ctx, kTimeAlign);
    ctx->dn_edges = nedges;
    ctx->dn_work = npairs != 0 ? ctx->dn_aligned : 0;
    ctx->dn_launches = launches + 4;
    ctx->up.dn_graph_ready = true;
    ctx->up.dn_graph_ncb = no_cluster_breaking != 0;
  }
  return SWA_OK;
}

// a sorted link list -> offsets / neighbours / diffs on the host (buffers and capacity protocol of swa_dn_graph)
int swa_dn_graph_emit(swa_ctx * ctx, const unsigned long long * sorted, const uint32_t * svals, uint64_t nedges, uint64_t * offsets,
                      uint32_t * neighbours, uint8_t * diffs, uint64_t cap, uint64_t * total) {
  const uint32_t n = ctx->db.n;
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  *total = nedges;
  ctx->res.csr_ready = false;                                   // (d_offsets_tmp / d_nb_tmp now hold this graph)
  SWA_TRY(swa_reserve(ctx, ctx->d_offsets_tmp, ((uint64_t)n + 1) * sizeof(uint64_t)));
  hipLaunchKernelGGL(k_dg_offsets, dim3(swa_grid256(ctx, (uint64_t)n + 1)), dim3(256), 0, ctx->stream, sorted, nedges, n,
                     static_cast<uint64_t *>(ctx->d_offsets_tmp.ptr));
  SWA_HIP(ctx, hipMemcpyAsync(offsets, ctx->d_offsets_tmp.ptr, ((uint64_t)n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (nedges > cap) {
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_dn_graph: neighbour buffer too small");
  }
  if (nedges != 0) {
    SWA_TRY(swa_reserve(ctx, ctx->d_nb_tmp, nedges * (sizeof(uint32_t) + 1)));
    auto * nb32 = static_cast<uint32_t *>(ctx->d_nb_tmp.ptr);
    auto * df8 = reinterpret_cast<uint8_t *>(nb32 + nedges);
    hipLaunchKernelGGL(k_dg_split, dim3(swa_grid256(ctx, nedges)), dim3(256), 0, ctx->stream, sorted, svals, nedges, nb32, df8);
    SWA_HIP(ctx, hipMemcpyAsync(neighbours, nb32, nedges * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipMemcpyAsync(diffs, df8, nedges, hipMemcpyDeviceToHost, ctx->stream));
  }
  SWA_HIP(ctx, hipGetLastError());
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

extern "C" int swa_dn_graph(swa_ctx * ctx, int no_cluster_breaking, uint64_t * offsets, uint32_t * neighbours, uint8_t * diffs,
                            uint64_t cap, uint64_t * total) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (offsets == nullptr || total == nullptr || (cap != 0 && (neighbours == nullptr || diffs == nullptr))) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_dn_graph: null buffer");
  }
  SWA_TRY(swa_dn_graph_compute(ctx, no_cluster_breaking));
  const unsigned long long * sorted = ctx->dn_work != 0 ? static_cast<const unsigned long long *>(ctx->d_dn_keys.ptr) + ctx->dn_work : nullptr;
  const uint32_t * svals = ctx->dn_work != 0 ? static_cast<const uint32_t *>(ctx->d_dn_vals.ptr) + ctx->dn_work : nullptr;
  return swa_dn_graph_emit(ctx, sorted, svals, ctx->dn_edges, offsets, neighbours, diffs, cap, total);
}

// The graph left in HBM as the resident network (offsets | neighbours | diffs in the buffers swa_d1_network_resident uses):
// swa_d1_cluster_device then evaluates the agglomeration of src/algo.cc:384-602 on it where it lies — the same pure
// function of the directed graph as for d = 1 (seeds by lowest id, generations by distance, members by generation then
// id: find_correct_position_in_list, src/algo.cc:205-219) — and swa_dn_parent_diffs adds what the radius needs.
// swa_dn_graph_install: from a sorted link list in HBM — this context's own (swa_dn_graph_resident), or the ranks' shares
// merged on rank 0 (multi.hip: swa_multi_dn_graph_resident).
int swa_dn_graph_install(swa_ctx * ctx, const unsigned long long * sorted, const uint32_t * svals, uint64_t nedges) {
  const uint32_t n = ctx->db.n;
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  ctx->res.csr_ready = false;
  ctx->res.tables = {};                                     // (radii and links of the graph that is replaced here: dn_tables.inc)
  SWA_TRY(swa_reserve(ctx, ctx->d_offsets_tmp, ((uint64_t)n + 1) * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_nb_tmp, (nedges + 1) * (sizeof(uint32_t) + 1)));
  hipLaunchKernelGGL(k_dg_offsets, dim3(swa_grid256(ctx, (uint64_t)n + 1)), dim3(256), 0, ctx->stream, sorted, nedges, n,
                     static_cast<uint64_t *>(ctx->d_offsets_tmp.ptr));
  if (nedges != 0) {
    auto * nb32 = static_cast<uint32_t *>(ctx->d_nb_tmp.ptr);
    hipLaunchKernelGGL(k_dg_split, dim3(swa_grid256(ctx, nedges)), dim3(256), 0, ctx->stream, sorted, svals, nedges, nb32,
                       reinterpret_cast<uint8_t *>(nb32 + nedges));
  }
  SWA_HIP(ctx, hipGetLastError());
  ctx->res.csr_ready = true;
  ctx->res.csr_total = nedges;
  ctx->res.csr_has_diffs = true;
  return SWA_OK;
}

extern "C" int swa_dn_graph_resident(swa_ctx * ctx, int no_cluster_breaking, uint64_t * total) {
  if (ctx == nullptr || total == nullptr) { return SWA_E_ARG; }
  SWA_TRY(swa_dn_graph_compute(ctx, no_cluster_breaking));
  const uint64_t nedges = ctx->dn_edges;
  const unsigned long long * sorted = ctx->dn_work != 0 ? static_cast<const unsigned long long *>(ctx->d_dn_keys.ptr) + ctx->dn_work : nullptr;
  const uint32_t * svals = ctx->dn_work != 0 ? static_cast<const uint32_t *>(ctx->d_dn_vals.ptr) + ctx->dn_work : nullptr;
  SWA_TRY(swa_dn_graph_install(ctx, sorted, svals, nedges));
  *total = nedges;
  return SWA_OK;
}

// pdiff[v] = differences between v and its parent in the clustering swa_d1_cluster_device has just made of the graph
// (0 for seeds); n bytes on the host.  radius(v) = radius(parent) + pdiff[v] (src/algo.cc:560-574).
extern "C" int swa_dn_parent_diffs(swa_ctx * ctx, uint8_t * pdiff) {
  if (ctx == nullptr || pdiff == nullptr) { return SWA_E_ARG; }
  if (!ctx->res.csr_ready || !ctx->res.csr_has_diffs || ctx->d_cluster.ptr == nullptr) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_dn_parent_diffs: call swa_dn_graph_resident and swa_d1_cluster_device first");
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->db.n;
  const auto * nb32 = static_cast<const uint32_t *>(ctx->d_nb_tmp.ptr);
  swa_cluster_arrays cl;
  SWA_TRY(swa_carve(ctx, ctx->d_cluster, n, false, cl));
  SWA_TRY(swa_reserve(ctx, ctx->d_scan_diffs, (uint64_t)n + 16));
  auto * out = static_cast<uint8_t *>(ctx->d_scan_diffs.ptr);
  hipLaunchKernelGGL(k_dg_parent_diffs, dim3(swa_grid256(ctx, n)), dim3(256), 0, ctx->stream, static_cast<const uint64_t *>(ctx->d_offsets_tmp.ptr),
                     nb32, reinterpret_cast<const uint8_t *>(nb32 + ctx->res.csr_total), cl.parent, n, out);
  SWA_HIP(ctx, hipGetLastError());
  SWA_HIP(ctx, hipMemcpyAsync(pdiff, out, n, hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

// Multi-GPU by ownership of window groups (as swa_d1_set_ownership): with world > 1 this context makes only the groups
// whose window key maps to `rank`.  A pair is reported through the FIRST window it shares ("not already found through
// an earlier window" is decided on the two sequences), and that window's group lives on one rank; a pair with a short
// member comes from the rank with id % world of the short sequence that emits it (k_dg_brute): over all ranks every
// pair of the graph is found exactly once.  world = 1 restores the complete graph.
extern "C" int swa_dn_set_ownership(swa_ctx * ctx, uint32_t rank, uint32_t world) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (world == 0 || rank >= world) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_dn_set_ownership: bad rank / world"); }
  if (rank != ctx->dn_owner_rank || world != ctx->dn_owner_world) {
    ctx->dn_owner_rank = rank; ctx->dn_owner_world = world;
    ctx->up.dn_graph_ready = false;
  }
  return SWA_OK;
}

// out3 = {q-gram comparisons, aligned pairs, kernel launches} of the last swa_dn_graph
extern "C" int swa_dn_graph_totals(swa_ctx * ctx, uint64_t * out3) {
  if (ctx == nullptr || out3 == nullptr) { return SWA_E_ARG; }
  out3[0] = ctx->dn_comparisons; out3[1] = ctx->dn_aligned; out3[2] = ctx->dn_launches;
  return SWA_OK;
}

// loads this translation unit's code object (see swa_ctx_warmup): an empty launch
__global__ void k_warm_dn() {}
void swa_warm_dn(swa_ctx * ctx) { hipLaunchKernelGGL(k_warm_dn, dim3(1), dim3(64), 0, ctx->stream); }
