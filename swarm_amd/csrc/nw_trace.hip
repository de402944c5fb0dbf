// nw_trace.hip — seam B5: the uclust alignments (-u) on gfx950, with their traceback.
//
// Replaces the nw() call per H line of the reference's uclust writers (src/algod1.cc:896-925, src/algo.cc:620-655,
// src/nw.cc:237-255): for pairs (d, q) = (member, seed) of the resident database, the reference's tie-broken
// minimum-cost global alignment with affine gaps, returned as the difference count (columns - matches), the alignment
// length and the CIGAR text.  host/nw_host.cpp (swa_nw_align) is the specification: same comparisons, same direction
// bits (src/nw.cc:91-103), same walk-back priority and state machine (src/nw.cc:139-172), so the result is equal bit for
// bit, not merely equally optimal.
//
//   * banded: a group of G lanes aligns one pair, lane <-> band offset (column - row), one anti-diagonal per step, one DPP
//     shift each way per step (as k_align in align.hip).  Lane 0 and the lanes above 2W + 1 are guards that hold the
//     "outside the band" value for ever, so W = (G - 3) / 2: 6, 14, 30 for G = 16, 32, 64.
//   * direction bits: 4 per cell, kept in LDS, one u32 column per lane (8 cells of its diagonal per word; cell (r, c)
//     is cell min(r, c) of diagonal c - r).  One lane then walks back exactly as swa_nw_align does and writes the
//     run-length CIGAR right to left into LDS; the group copies it out to a packed text buffer.
//   * certificate: the result is accepted only when the band's end cost C satisfies C < gapopen + (W + 1) * gapextend.
//     Any path that touches a cell outside the band has paid one gap opening and W + 1 gap columns by then; every value
//     the walk-back compares has its smaller side <= C; so each comparison it reads — and each direction bit — is the
//     full matrix's.  The argument uses neither where the bits are kept nor how many offsets a lane
//     holds, so it covers the wide tiers below word for word.  Pairs that fail go to the next wider tier.
//   * wide tiers (k_nw_trace_wide<K>, K = 1, 2, 4, 8): one wave aligns one pair, each of its 64 lanes owns K adjacent band
//     offsets in registers (offset index x = lane * K + j; x = 0 and x > 2W + 1 are the guards), so W = (64 K - 3) / 2:
//     30, 62, 126, 254.  Only a lane's outermost offsets cross to its neighbours, one DPP shift each way per anti-
//     diagonal; for K > 1 the offsets of one parity are live on a step, so a step touches K / 2 cells per lane.  The
//     direction bits go to a global scratch slot per wave, laid out [word][j][lane] (one word per lane = one 256-byte
//     line); the walking lane reads them back through L2 with the last word kept in a register (8 cells of a diagonal
//     run share it).  They take what the LDS tiers cannot: min(dl, ql) > 1024, |dl - ql| > 30, and what the 64-lane LDS
//     tier failed to certify.  Slots are sized by the slice's longest min(dl, ql) and the grid is cut until they fit
//     kBitsBudget.
//   * the host (swa_nw_align, inside the same call) aligns what is left: pairs the widest tier cannot certify (|dl - ql|
//     > 254 or an end cost of at least gapopen + 255 gapextend), pairs with dl + ql > kWideMaxSum, pairs whose costs
//     could overflow 32 bits, and pairs that found the text buffer full (sent there at once, and counted).
#include "swa_internal.h"
#include "host/nw_host.h"
#include "host/pool.h"

#include <algorithm>
#include <cstdlib>

namespace {

constexpr uint32_t kUp = 1, kLeft = 2, kExtUp = 4, kExtLeft = 8;   // host/nw_host.cpp, src/nw.cc:91-103
constexpr uint32_t kInf = 0x40000000u;            // "outside the band": every finite value stays below 2^30 (host check)
constexpr uint32_t kMaxCells = 1024;              // longest diagonal a lane stores (LDS: 128 words x 64 lanes)
constexpr uint32_t kTiers = 3;                    // the LDS tiers: G = 16, 32, 64
constexpr uint32_t kWide = 4;                     // the wide tiers: K = 1, 2, 4, 8 offsets a lane
constexpr uint32_t kLists = kTiers + kWide;       // device lists; list kLists is the host's
constexpr uint32_t kWideMaxSum = 32768;           // longest dl + ql of a wide tier (sequences and CIGAR text in 64 KB of LDS)
constexpr uint64_t kBitsBudget = 1ull << 31;      // the wide tiers' direction bits: 2 GiB of slots at most (as k_align_generic)
constexpr uint32_t kPassedWaves = 256;             // waves (and slots) a wide tier gets for what the LDS tiers pass down
constexpr uint64_t kTextPerWidePair = 256;        // more CIGAR room for a pair that enters a wide tier
constexpr uint64_t kSlice = 1u << 20;             // pairs per device pass: device memory does not grow with the batch
constexpr uint64_t kTextPerPair = 48;             // packed CIGAR room per pair (a pair that finds it full goes to the host)
constexpr int kBlock = 64;                        // one wave per workgroup

struct NwArgs {
  const uint64_t * seqs;
  const uint64_t * seq_off;
  const uint32_t * seqlen;
  const uint32_t * d_ids;          // [pairs of the slice]
  const uint32_t * q_ids;
  const uint32_t * list;           // this tier's pairs (indices into the slice) ...
  const uint32_t * list_count;     // ... how many (read on the device: earlier tiers append)
  uint32_t list_room;              // an upper bound of *list_count (the grid is sized on it)
  uint32_t * next_list;            // pairs this tier could not certify: the next tier's list, or the host's
  uint32_t * next_count;
  uint4 * res;                     // per pair: diffs, columns, CIGAR length, tier + 1 (0: not done on the device)
  unsigned long long * text_off;   // per pair: where its CIGAR starts in `text`
  char * text;
  unsigned long long * text_used;
  unsigned long long text_cap;
  uint32_t mismatch, gapopen, gapextend;
  uint32_t maxwords;               // u64 words per staged sequence
  uint32_t bitwords;               // u32 direction words per lane
  uint32_t textcap;                // LDS text bytes per group (>= the longest dl + ql, multiple of 8)
  uint32_t tier;
  uint32_t * bits;                 // wide tiers: the direction bits, one slot per workgroup ...
  unsigned long long slot_words;   // ... of bitwords * K * 64 words
  uint32_t * text_full;            // pairs a wide tier certified but could not store: they go to the host's list
  uint32_t * host_list;
  uint32_t * host_count;
};

__device__ __forceinline__ uint32_t from_lane_below(uint32_t v) {   // lane i <- lane i-1
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t from_lane_above(uint32_t v) {   // lane i <- lane i+1
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ uint32_t nt_at(const uint64_t * w, int p) { return (uint32_t)(w[p >> 5] >> ((p & 31) << 1)) & 3u; }

template <int G>
__global__ __launch_bounds__(kBlock) void k_nw_trace(const NwArgs a) {
  extern __shared__ uint64_t lds[];
  constexpr int kGroups = kBlock / G;
  constexpr int W = (G - 3) / 2;
  const int group = threadIdx.x / G;
  const int t = threadIdx.x % G;
  const int lane = threadIdx.x;
  uint64_t * dw = lds + (size_t)(2 * group) * a.maxwords;                        // member words
  uint64_t * qw = dw + a.maxwords;                                               // seed words
  uint32_t * bitmem = reinterpret_cast<uint32_t *>(lds + (size_t)2 * kGroups * a.maxwords);   // [word][64 lanes]
  char * tx = reinterpret_cast<char *>(bitmem + (size_t)a.bitwords * kBlock) + (size_t)group * a.textcap;

  const int o = t - 1 - W;                                     // band offset = column - row
  const bool in_band = t >= 1 && t <= 2 * W + 1;
  const uint32_t mm = a.mismatch, go = a.gapopen, ge = a.gapextend;
  const uint32_t bound = go + (uint32_t)(W + 1) * ge;          // the certificate: end cost < bound
  const uint32_t count = min(*a.list_count, a.list_room);

  for (uint32_t i = blockIdx.x * kGroups + group; i < count; i += gridDim.x * kGroups) {
    const uint32_t k = a.list[i];
    const uint32_t did = a.d_ids[k], qid = a.q_ids[k];
    const int dl = (int)a.seqlen[did], ql = (int)a.seqlen[qid];
    wave_lds_sync();                                           // the previous pair's LDS readers are done
    {
      const uint64_t * gd = a.seqs + a.seq_off[did];
      const uint64_t * gq = a.seqs + a.seq_off[qid];
      for (int w = t; w < ((dl + 31) >> 5); w += G) { dw[w] = gd[w]; }
      for (int w = t; w < ((ql + 31) >> 5); w += G) { qw[w] = gq[w]; }
    }
    wave_lds_sync();
    const int delta = ql - dl;
    const bool feasible = delta <= W && -delta <= W;
    uint32_t h_own = 0, e_out = kInf, f_out = kInf, acc = 0;
    if (feasible) {
      const int last = dl + ql - 2;
#pragma unroll 1
      for (int s = 0; s <= last; ++s) {
        const uint32_t e_nb = from_lane_below(e_out);          // horizontal gap state of (r, c - 1)
        const uint32_t f_nb = from_lane_above(f_out);          // vertical gap state of (r - 1, c)
        const int rs = s - o;
        const int r = rs >> 1;
        const int c = s - r;
        const bool act = in_band && (rs & 1) == 0 && r >= 0 && r < dl && c >= 0 && c < ql;
        const int rc_ = r < 0 ? 0 : (r >= dl ? dl - 1 : r);
        const int cc_ = c < 0 ? 0 : (c >= ql ? ql - 1 : c);
        const bool mis = nt_at(dw, rc_) != nt_at(qw, cc_);
        // borders (host/nw_host.cpp): H(-1, c) = go + (c + 1) ge, H(r, -1) = go + (r + 1) ge, H(-1, -1) = 0;
        // horizontal state entering column 0 = 2 go + (r + 2) ge, vertical state entering row 0 = 2 go + (c + 2) ge
        const uint32_t across = c == 0 ? 2u * go + (uint32_t)(r + 2) * ge : e_nb;
        const uint32_t down = r == 0 ? 2u * go + (uint32_t)(c + 2) * ge : f_nb;
        const uint32_t diag = (r == 0 || c == 0) ? ((r | c) == 0 ? 0u : go + (uint32_t)(r + c) * ge) : h_own;
        uint32_t h = diag + (mis ? mm : 0u);
        uint32_t bits = 0;
        if (across < h) { bits |= kUp; h = across; }
        if (down < h) { h = down; }
        if (down == h) { bits |= kLeft; }
        const uint32_t opened = h + go + ge;
        const uint32_t across_n = across + ge, down_n = down + ge;
        if (across_n < opened) { bits |= kExtUp; }
        if (down_n < opened) { bits |= kExtLeft; }
        if (act) {
          h_own = h;
          e_out = min(across_n, opened);
          f_out = min(down_n, opened);
          const int cell = r < c ? r : c;
          acc |= bits << ((cell & 7) << 2);
          if ((cell & 7) == 7 || r == dl - 1 || c == ql - 1) {   // a full word, or the last cell of the diagonal
            bitmem[(cell >> 3) * kBlock + lane] = acc;
            acc = 0;
          }
        }
      }
    }
    // the end cell (dl - 1, ql - 1) lies on offset delta, in lane delta + W + 1 of the group
    const uint32_t cost = (uint32_t)__shfl((int)h_own, group * G + (feasible ? delta + W + 1 : 0), kBlock);
    const bool certified = feasible && cost < bound;
    wave_lds_sync();
    int start = 0;
    uint32_t diffs = 0, columns = 0;
    if (certified && t == 0) {
      // walk back from the last cell: host/nw_host.cpp, src/nw.cc:139-172
      int pos = (int)a.textcap;
      char run_op = 0;
      uint32_t run_len = 0, matches = 0;
      auto flush = [&]() {                                     // one run, written right to left: count (if > 1), then op
        if (run_len == 0) { return; }
        tx[--pos] = run_op;
        if (run_len > 1) { for (uint32_t v = run_len; v != 0; v /= 10) { tx[--pos] = (char)('0' + v % 10); } }
      };
      auto push = [&](char op, uint32_t n) {
        if (op == run_op) { run_len += n; return; }
        flush();
        run_op = op;
        run_len = n;
      };
      int row = dl, col = ql;
      char op = 0;
      while (row > 0 && col > 0) {
        const int r = row - 1, c = col - 1;
        const int cell = r < c ? r : c;
        const uint32_t bits = (bitmem[(cell >> 3) * kBlock + group * G + (c - r) + W + 1] >> ((cell & 7) << 2)) & 15u;
        if (op == 'I' && (bits & kExtLeft)) { --row; op = 'I'; }
        else if (op == 'D' && (bits & kExtUp)) { --col; op = 'D'; }
        else if (bits & kLeft) { --row; op = 'I'; }
        else if (bits & kUp) { --col; op = 'D'; }
        else {
          if (nt_at(dw, r) == nt_at(qw, c)) { ++matches; }
          --row; --col; op = 'M';
        }
        ++columns;
        push(op, 1);
      }
      if (col > 0) { push('D', (uint32_t)col); }
      if (row > 0) { push('I', (uint32_t)row); }
      flush();
      columns += (uint32_t)(col + row);
      diffs = columns - matches;
      start = pos;
    }
    wave_lds_sync();
    start = __shfl(start, group * G, kBlock);
    bool done = certified;
    unsigned long long off = 0;
    if (certified) {
      const uint32_t len = a.textcap - (uint32_t)start;
      if (t == 0) { off = atomicAdd(a.text_used, (unsigned long long)len); }
      off = (unsigned long long)__shfl((long long)off, group * G, kBlock);
      done = off + len <= a.text_cap;
      if (done) {
        for (uint32_t b = (uint32_t)t; b < len; b += G) { a.text[off + b] = tx[start + (int)b]; }
        if (t == 0) {
          a.res[k] = make_uint4(diffs, columns, len, a.tier + 1);
          a.text_off[k] = off;
        }
      }
    }
    if (!done && t == 0) { a.next_list[atomicAdd(a.next_count, 1u)] = k; }
  }
}

// One wave, one pair, K band offsets a lane: offset index x = lane * K + j <-> band offset x - 1 - W.  The same recurrence,
// direction bits, certificate and walk-back as k_nw_trace; the bits live in the wave's global slot.
template <int K>
__global__ __launch_bounds__(kBlock) void k_nw_trace_wide(const NwArgs a) {
  extern __shared__ uint64_t lds[];
  constexpr int W = (kBlock * K - 3) / 2;
  constexpr int kShift = K == 1 ? 0 : K == 2 ? 1 : K == 4 ? 2 : 3;
  static_assert(K == 1 || (W & 1) == 0, "the parity of the live offsets is a compile-time fact only for even W");
  const int lane = threadIdx.x;
  uint64_t * dw = lds;                                                           // member words
  uint64_t * qw = dw + a.maxwords;                                               // seed words
  char * tx = reinterpret_cast<char *>(qw + a.maxwords);
  uint32_t * bitmem = a.bits + (size_t)blockIdx.x * a.slot_words;                // [word][j][64 lanes]

  const uint32_t mm = a.mismatch, go = a.gapopen, ge = a.gapextend;
  const uint32_t bound = go + (uint32_t)(W + 1) * ge;          // the certificate: end cost < bound
  const uint32_t count = min(*a.list_count, a.list_room);

  for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
    const uint32_t k = a.list[i];
    const uint32_t did = a.d_ids[k], qid = a.q_ids[k];
    const int dl = (int)a.seqlen[did], ql = (int)a.seqlen[qid];
    const int delta = ql - dl;
    // (the launch sized LDS and the slot for every pair of the list; a pair outside them is passed on, never written)
    const bool feasible = delta <= W && -delta <= W && (uint32_t)(dl + ql) <= a.textcap &&
                          (uint32_t)((max(dl, ql) + 31) >> 5) <= a.maxwords && (uint32_t)((min(dl, ql) + 7) >> 3) <= a.bitwords;
    wave_lds_sync();                                           // the previous pair's LDS readers are done
    if (feasible) {
      const uint64_t * gd = a.seqs + a.seq_off[did];
      const uint64_t * gq = a.seqs + a.seq_off[qid];
      for (int w = lane; w < ((dl + 31) >> 5); w += kBlock) { dw[w] = gd[w]; }
      for (int w = lane; w < ((ql + 31) >> 5); w += kBlock) { qw[w] = gq[w]; }
    }
    wave_lds_sync();
    uint32_t h_own[K], e_out[K], f_out[K], acc[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { h_own[j] = 0; e_out[j] = kInf; f_out[j] = kInf; acc[j] = 0; }
    // one anti-diagonal: the offsets j of parity `par` (every j when K = 1, where the parity is the lane's)
    auto step = [&](const int s, const int par) {
      const uint32_t e_in = from_lane_below(e_out[K - 1]);     // horizontal gap state of (r, c - 1) for j = 0
      const uint32_t f_in = from_lane_above(f_out[0]);         // vertical gap state of (r - 1, c) for j = K - 1
#pragma unroll
      for (int j = 0; j < K; ++j) {
        if (K > 1 && (j & 1) != par) { continue; }
        const int x = lane * K + j;
        const int rs = s - (x - 1 - W);
        const int r = rs >> 1;
        const int c = s - r;
        const bool act = x >= 1 && x <= 2 * W + 1 && (K > 1 || (rs & 1) == 0) && r >= 0 && r < dl && c >= 0 && c < ql;
        const int rc_ = r < 0 ? 0 : (r >= dl ? dl - 1 : r);
        const int cc_ = c < 0 ? 0 : (c >= ql ? ql - 1 : c);
        const bool mis = nt_at(dw, rc_) != nt_at(qw, cc_);
        const uint32_t e_nb = j == 0 ? e_in : e_out[j == 0 ? 0 : j - 1];
        const uint32_t f_nb = j == K - 1 ? f_in : f_out[j == K - 1 ? j : j + 1];
        // borders and recurrence: exactly k_nw_trace's (host/nw_host.cpp)
        const uint32_t across = c == 0 ? 2u * go + (uint32_t)(r + 2) * ge : e_nb;
        const uint32_t down = r == 0 ? 2u * go + (uint32_t)(c + 2) * ge : f_nb;
        const uint32_t diag = (r == 0 || c == 0) ? ((r | c) == 0 ? 0u : go + (uint32_t)(r + c) * ge) : h_own[j];
        uint32_t h = diag + (mis ? mm : 0u);
        uint32_t bits = 0;
        if (across < h) { bits |= kUp; h = across; }
        if (down < h) { h = down; }
        if (down == h) { bits |= kLeft; }
        const uint32_t opened = h + go + ge;
        const uint32_t across_n = across + ge, down_n = down + ge;
        if (across_n < opened) { bits |= kExtUp; }
        if (down_n < opened) { bits |= kExtLeft; }
        if (act) {
          h_own[j] = h;
          e_out[j] = min(across_n, opened);
          f_out[j] = min(down_n, opened);
          const int cell = r < c ? r : c;
          acc[j] |= bits << ((cell & 7) << 2);
          if ((cell & 7) == 7 || r == dl - 1 || c == ql - 1) {   // a full word, or the last cell of the diagonal
            bitmem[((size_t)(cell >> 3) * K + j) * kBlock + lane] = acc[j];
            acc[j] = 0;
          }
        }
      }
    };
    if (feasible) {
      const int last = dl + ql - 2;
      if constexpr (K == 1) {
#pragma unroll 1
        for (int s = 0; s <= last; ++s) { step(s, 0); }
      } else {
        // x = lane * K + j has j's parity; offset x is live on step s when s - (x - 1 - W) is even: j odd on even steps
#pragma unroll 1
        for (int s = 0; s <= last; s += 2) {
          step(s, 1);
          if (s < last) { step(s + 1, 0); }
        }
      }
    }
    // the end cell (dl - 1, ql - 1) lies on offset delta: index x = delta + W + 1
    const int xe = feasible ? delta + W + 1 : 0;
    uint32_t h_end = h_own[0];
#pragma unroll
    for (int j = 1; j < K; ++j) { if ((xe & (K - 1)) == j) { h_end = h_own[j]; } }
    const uint32_t cost = (uint32_t)__shfl((int)h_end, xe >> kShift, kBlock);
    const bool certified = feasible && cost < bound;
    // the walking lane reads what its own wave stored: producer and consumer share the CU's write-through L1, so the
    // workgroup-scope release / acquire around a wave barrier orders them without touching L2
    wave_lds_sync();
    int start = 0;
    uint32_t diffs = 0, columns = 0;
    if (certified && lane == 0) {
      // walk back from the last cell: host/nw_host.cpp, src/nw.cc:139-172
      int pos = (int)a.textcap;
      char run_op = 0;
      uint32_t run_len = 0, matches = 0;
      auto flush = [&]() {                                     // one run, written right to left: count (if > 1), then op
        if (run_len == 0) { return; }
        tx[--pos] = run_op;
        if (run_len > 1) { for (uint32_t v = run_len; v != 0; v /= 10) { tx[--pos] = (char)('0' + v % 10); } }
      };
      auto push = [&](char op, uint32_t n) {
        if (op == run_op) { run_len += n; return; }
        flush();
        run_op = op;
        run_len = n;
      };
      int row = dl, col = ql;
      char op = 0;
      size_t have = ~size_t(0);                                // the word held in `word`
      uint32_t word = 0;
      while (row > 0 && col > 0) {
        const int r = row - 1, c = col - 1;
        const int cell = r < c ? r : c;
        const int x = (c - r) + W + 1;
        const size_t at = ((size_t)(cell >> 3) * K + (x & (K - 1))) * kBlock + (x >> kShift);
        if (at != have) { word = bitmem[at]; have = at; }
        const uint32_t bits = (word >> ((cell & 7) << 2)) & 15u;
        if (op == 'I' && (bits & kExtLeft)) { --row; op = 'I'; }
        else if (op == 'D' && (bits & kExtUp)) { --col; op = 'D'; }
        else if (bits & kLeft) { --row; op = 'I'; }
        else if (bits & kUp) { --col; op = 'D'; }
        else {
          if (nt_at(dw, r) == nt_at(qw, c)) { ++matches; }
          --row; --col; op = 'M';
        }
        ++columns;
        push(op, 1);
      }
      if (col > 0) { push('D', (uint32_t)col); }
      if (row > 0) { push('I', (uint32_t)row); }
      flush();
      columns += (uint32_t)(col + row);
      diffs = columns - matches;
      start = pos;
    }
    wave_lds_sync();
    start = __shfl(start, 0, kBlock);
    bool done = certified;
    unsigned long long off = 0;
    if (certified) {
      const uint32_t len = a.textcap - (uint32_t)start;
      if (lane == 0) { off = atomicAdd(a.text_used, (unsigned long long)len); }
      off = (unsigned long long)__shfl((long long)off, 0, kBlock);
      done = off + len <= a.text_cap;
      if (done) {
        for (uint32_t b = (uint32_t)lane; b < len; b += kBlock) { a.text[off + b] = tx[start + (int)b]; }
        if (lane == 0) {
          a.res[k] = make_uint4(diffs, columns, len, a.tier + 1);
          a.text_off[k] = off;
        }
      } else if (lane == 0) {                                  // text buffer full: a wider band would find it full again
        atomicAdd(a.text_full, 1u);
        a.host_list[atomicAdd(a.host_count, 1u)] = k;
      }
    }
    if (!certified && lane == 0) { a.next_list[atomicAdd(a.next_count, 1u)] = k; }
  }
}

// the words of amplicons ids[j] to dst + dst_off[j] (the host's fallback pairs)
__global__ __launch_bounds__(256) void k_nw_gather(const uint64_t * seqs, const uint64_t * seq_off, const uint32_t * seqlen,
                                                   const uint32_t * ids, const uint64_t * dst_off, uint32_t nids, uint64_t * dst) {
  for (uint32_t j = blockIdx.x; j < nids; j += gridDim.x) {
    const uint32_t id = ids[j];
    const uint32_t nw = (seqlen[id] + 31u) >> 5;
    for (uint32_t w = threadIdx.x; w < nw; w += blockDim.x) { dst[dst_off[j] + w] = seqs[seq_off[id] + w]; }
  }
}

template <int G>
size_t lds_bytes(const NwArgs & a) {
  return (size_t)2 * (kBlock / G) * a.maxwords * 8 + (size_t)a.bitwords * kBlock * 4 + (size_t)(kBlock / G) * a.textcap;
}

template <int G>
int launch_tier(swa_ctx * ctx, NwArgs a, uint32_t room) {
  if (room == 0) { return SWA_OK; }
  a.list_room = room;
  constexpr uint32_t kGroups = kBlock / G;
  const uint32_t grid = std::max<uint32_t>(1, std::min<uint32_t>((room + kGroups - 1) / kGroups, (uint32_t)ctx->num_cus * 32u));
  hipLaunchKernelGGL(k_nw_trace<G>, dim3(grid), dim3(kBlock), lds_bytes<G>(a), ctx->stream, a);
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}

size_t wide_lds_bytes(const NwArgs & a) { return (size_t)2 * a.maxwords * 8 + a.textcap; }

// waves of a wide tier: one a pair (`room` of them expected), at most 16 a CU, and no more slots than kBitsBudget holds
template <int K>
uint32_t wide_grid(const swa_ctx * ctx, uint32_t room, uint32_t bitwords) {
  const uint64_t slot_bytes = (uint64_t)bitwords * K * kBlock * 4;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(room, (uint64_t)ctx->num_cus * 16u), kBitsBudget / slot_bytes));
}

template <int K>
int launch_wide(swa_ctx * ctx, NwArgs a, uint32_t room, uint32_t waves) {
  if (room == 0) { return SWA_OK; }
  a.list_room = room;
  a.slot_words = (unsigned long long)a.bitwords * K * kBlock;
  hipLaunchKernelGGL(k_nw_trace_wide<K>, dim3(wide_grid<K>(ctx, waves, a.bitwords)), dim3(kBlock), wide_lds_bytes(a), ctx->stream, a);
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}

// lengths of the resident database on the host: the batch sorts its pairs into tiers and sizes LDS by them
int host_seqlen(swa_ctx * ctx) {
  if (ctx->nw_seqlen.size() == ctx->db.n) { return SWA_OK; }
  ctx->nw_seqlen.resize(ctx->db.n);
  if (ctx->db.n == 0) { return SWA_OK; }
  SWA_HIP(ctx, hipMemcpyAsync(ctx->nw_seqlen.data(), ctx->db.seqlen, (size_t)ctx->db.n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

template <class T>
T * buf(swa_dbuf & b) { return static_cast<T *>(b.ptr); }

}  // namespace

extern "C" int swa_nw_batch(swa_ctx * ctx, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t npairs,
                            const uint32_t * d_ids, const uint32_t * q_ids, uint32_t * diffs, uint32_t * columns,
                            uint64_t * cigar_end, char * cigar, uint64_t cigar_cap, uint64_t * cigar_total) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (npairs > 0 && (d_ids == nullptr || q_ids == nullptr || diffs == nullptr || columns == nullptr || cigar_end == nullptr)) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_nw_batch: null result array");
  }
  if (ctx->db.seqs == nullptr && npairs > 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_nw_batch: no database resident"); }
  for (uint64_t k = 0; k < npairs; ++k) {
    if (d_ids[k] >= ctx->db.n || q_ids[k] >= ctx->db.n) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_nw_batch: amplicon id out of range"); }
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(host_seqlen(ctx));
  for (auto & v : ctx->nw_totals) { v = 0; }
  ctx->nw_text_full = 0;
  const uint32_t * len = ctx->nw_seqlen.data();
  // 32-bit costs: every finite value the kernels form is below mm + 3 go + (dl + ql + 4) ge; it must stay below kInf
  auto fits = [&](uint32_t dl, uint32_t ql) {
    const unsigned __int128 top = (unsigned __int128)mismatch + 3 * (unsigned __int128)gapopen + (unsigned __int128)(dl + ql + 4) * gapextend;
    return top < kInf;
  };
  // half-widths: the LDS tiers, then the wide tiers.  A wide tier takes a pair whose slot fits the budget at K = 8 (so
  // that every later tier can take it too) and whose sequences and CIGAR text fit LDS.
  static constexpr uint32_t kW[kLists] = {6, 14, 30, 30, 62, 126, 254};
  auto wide_fits = [&](uint32_t dl, uint32_t ql) {
    return (uint64_t)dl + ql <= kWideMaxSum && (uint64_t)((std::min(dl, ql) + 7) / 8) * 8 * kBlock * 4 <= kBitsBudget;
  };
  struct Extent {                                              // what a launch sizes LDS and slots by
    uint32_t maxlen = 1, maxmin = 1, maxsum = 1;
    void add(uint32_t dl, uint32_t ql) {
      maxlen = std::max(maxlen, std::max(dl, ql));
      maxmin = std::max(maxmin, std::min(dl, ql));
      maxsum = std::max(maxsum, dl + ql);
    }
    void add(const Extent & o) { maxlen = std::max(maxlen, o.maxlen); maxmin = std::max(maxmin, o.maxmin); maxsum = std::max(maxsum, o.maxsum); }
  };

  std::vector<uint4> res;
  std::vector<unsigned long long> toff;
  std::string text;
  std::vector<std::string> host_cigar;
  std::vector<uint32_t> lists[kLists + 1];
  std::vector<uint32_t> tmp, host_slot;
  uint64_t total = 0;
  for (uint64_t base = 0; base < npairs; base += kSlice) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(kSlice, npairs - base);
    const uint32_t * sd = d_ids + base, * sq = q_ids + base;
    for (auto & l : lists) { l.clear(); }
    Extent lds_ext, wide_ext[kWide];                           // the LDS tiers' pairs; each wide tier's own pairs
    for (uint32_t k = 0; k < m; ++k) {
      const uint32_t dl = len[sd[k]], ql = len[sq[k]];
      const uint32_t delta = dl > ql ? dl - ql : ql - dl;
      uint32_t tier = kLists;
      if (fits(dl, ql)) {
        if (std::min(dl, ql) <= kMaxCells && delta <= kW[kTiers - 1]) {
          for (uint32_t t = 0; t < kTiers; ++t) { if (delta <= kW[t]) { tier = t; break; } }
        } else if (wide_fits(dl, ql)) {
          for (uint32_t t = kTiers; t < kLists; ++t) { if (delta <= kW[t]) { tier = t; break; } }
        }
      }
      lists[tier].push_back(k);
      if (tier < kTiers) { lds_ext.add(dl, ql); }
      else if (tier < kLists) { wide_ext[tier - kTiers].add(dl, ql); }
    }
    res.assign(m, make_uint4(0, 0, 0, 0));
    toff.assign(m, 0);
    const uint32_t on_device = m - (uint32_t)lists[kLists].size();
    if (on_device > 0) {
      uint32_t hcounts[16] = {};
      uint32_t wide_own = 0;
      for (uint32_t t = 0; t < kLists; ++t) { hcounts[t] = (uint32_t)lists[t].size(); if (t >= kTiers) { wide_own += hcounts[t]; } }
      const unsigned long long text_cap = (unsigned long long)kTextPerPair * on_device + (unsigned long long)kTextPerWidePair * wide_own + (1u << 16);
      // a wide tier aligns its own pairs and whatever came down to it: the pairs of the narrower wide tiers, and from
      // K = 2 on what the 64-lane LDS tier passed on.  How many that will be is known only on the device: wroom bounds the
      // list, wwaves sizes the grid and the slots, and counts the LDS tiers' pairs as kPassedWaves at most (they are rare:
      // 1 and 10 of 10 M in profiles/r07; the kernel's loop strides by the grid)
      Extent ext[kWide];
      uint32_t wroom[kWide], wwaves[kWide];
      size_t bits_bytes = 0;
      {
        Extent e;
        uint32_t room = 0, waves = 0;
        for (uint32_t w = 0; w < kWide; ++w) {
          if (w == 1) {
            const uint32_t passed = hcounts[0] + hcounts[1] + hcounts[2];
            e.add(lds_ext); room += passed; waves += std::min(passed, kPassedWaves);
          }
          e.add(wide_ext[w]);
          room += hcounts[kTiers + w];
          waves += hcounts[kTiers + w];
          ext[w] = e;
          wroom[w] = room;
          wwaves[w] = waves;
          if (room == 0) { continue; }
          const uint32_t bw = (e.maxmin + 7) / 8;
          const uint64_t slot = (uint64_t)bw * (1u << w) * kBlock * 4;
          const uint32_t grid = w == 0 ? wide_grid<1>(ctx, waves, bw) : w == 1 ? wide_grid<2>(ctx, waves, bw) : w == 2 ? wide_grid<4>(ctx, waves, bw)
                                                                                                                    : wide_grid<8>(ctx, waves, bw);
          bits_bytes = std::max<size_t>(bits_bytes, (size_t)(slot * grid));
        }
      }
      // one u32 block behind the lists: [0, kLists] list counts, [8] text used (u64), [10] text-full pairs
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_ids, (size_t)2 * m * sizeof(uint32_t)));
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_lists, (size_t)(kLists + 1) * m * sizeof(uint32_t) + 64));
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_res, (size_t)m * (sizeof(uint4) + sizeof(unsigned long long))));
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_text, (size_t)text_cap));
      if (bits_bytes > 0) { SWA_TRY(swa_reserve(ctx, ctx->d_nw_bits, bits_bytes)); }
      uint32_t * ids = buf<uint32_t>(ctx->d_nw_ids);
      uint32_t * dl_ = buf<uint32_t>(ctx->d_nw_lists);
      uint32_t * counts = dl_ + (size_t)(kLists + 1) * m;
      uint4 * d_res = buf<uint4>(ctx->d_nw_res);
      unsigned long long * d_toff = reinterpret_cast<unsigned long long *>(d_res + m);
      SWA_HIP(ctx, hipMemcpyAsync(ids, sd, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
      SWA_HIP(ctx, hipMemcpyAsync(ids + m, sq, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
      for (uint32_t t = 0; t < kLists; ++t) {
        if (!lists[t].empty()) {
          SWA_HIP(ctx, hipMemcpyAsync(dl_ + (size_t)t * m, lists[t].data(), lists[t].size() * 4, hipMemcpyHostToDevice, ctx->stream));
        }
      }
      SWA_HIP(ctx, hipMemcpyAsync(counts, hcounts, sizeof(hcounts), hipMemcpyHostToDevice, ctx->stream));
      SWA_HIP(ctx, hipMemsetAsync(d_res, 0, (size_t)m * sizeof(uint4), ctx->stream));
      NwArgs a{};
      a.seqs = ctx->db.seqs; a.seq_off = ctx->db.seq_off; a.seqlen = ctx->db.seqlen;
      a.d_ids = ids; a.q_ids = ids + m;
      a.res = d_res; a.text_off = d_toff; a.text = buf<char>(ctx->d_nw_text);
      a.text_used = reinterpret_cast<unsigned long long *>(counts + 8);
      a.text_full = counts + 10;
      a.host_list = dl_ + (size_t)kLists * m; a.host_count = counts + kLists;
      a.text_cap = text_cap;
      a.bits = buf<uint32_t>(ctx->d_nw_bits);
      a.mismatch = (uint32_t)mismatch; a.gapopen = (uint32_t)gapopen; a.gapextend = (uint32_t)gapextend;
      a.maxwords = (lds_ext.maxlen + 31) / 32 + 1;
      a.bitwords = (lds_ext.maxmin + 7) / 8;
      a.textcap = (lds_ext.maxsum + 7) & ~7u;
      uint32_t room = 0;
      for (uint32_t t = 0; t < kTiers; ++t) {
        a.list = dl_ + (size_t)t * m; a.list_count = counts + t;
        // (the 64-lane tier's failures skip the K = 1 wide tier, whose band is no wider)
        const uint32_t next = t + 1 < kTiers ? t + 1 : kTiers + 1;
        a.next_list = dl_ + (size_t)next * m; a.next_count = counts + next;
        a.tier = t;
        room += hcounts[t];                                    // this tier's own pairs + whatever the tiers before it passed on
        if (t == 0) { SWA_TRY(launch_tier<16>(ctx, a, room)); }
        else if (t == 1) { SWA_TRY(launch_tier<32>(ctx, a, room)); }
        else { SWA_TRY(launch_tier<64>(ctx, a, room)); }
      }
      for (uint32_t w = 0; w < kWide; ++w) {
        const uint32_t t = kTiers + w;
        a.list = dl_ + (size_t)t * m; a.list_count = counts + t;
        a.next_list = dl_ + (size_t)(t + 1) * m; a.next_count = counts + t + 1;
        a.tier = t;
        a.maxwords = (ext[w].maxlen + 31) / 32 + 1;
        a.bitwords = (ext[w].maxmin + 7) / 8;
        a.textcap = (ext[w].maxsum + 7) & ~7u;
        if (w == 0) { SWA_TRY(launch_wide<1>(ctx, a, wroom[w], wwaves[w])); }
        else if (w == 1) { SWA_TRY(launch_wide<2>(ctx, a, wroom[w], wwaves[w])); }
        else if (w == 2) { SWA_TRY(launch_wide<4>(ctx, a, wroom[w], wwaves[w])); }
        else { SWA_TRY(launch_wide<8>(ctx, a, wroom[w], wwaves[w])); }
      }
      SWA_HIP(ctx, hipMemcpyAsync(hcounts, counts, sizeof(hcounts), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipMemcpyAsync(res.data(), d_res, (size_t)m * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipMemcpyAsync(toff.data(), d_toff, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      // the widest tier appended what it could not certify to the host's list (from entry 0 on: counts[kLists] began at 0)
      const uint32_t appended = hcounts[kLists];
      ctx->nw_text_full += hcounts[10];
      const unsigned long long used = std::min<unsigned long long>(*reinterpret_cast<unsigned long long *>(hcounts + 8), text_cap);
      text.resize(used);
      if (used > 0) { SWA_HIP(ctx, hipMemcpyAsync(text.data(), a.text, used, hipMemcpyDeviceToHost, ctx->stream)); }
      if (appended > 0) {
        tmp.resize(appended);
        SWA_HIP(ctx, hipMemcpyAsync(tmp.data(), dl_ + (size_t)kLists * m, (size_t)appended * 4, hipMemcpyDeviceToHost, ctx->stream));
      }
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (appended > 0) { lists[kLists].insert(lists[kLists].end(), tmp.begin(), tmp.begin() + appended); }
    }
    // pairs for the host: their words fetched from the device in one gather, aligned by the host's workers
    const std::vector<uint32_t> & hl = lists[kLists];
    host_cigar.assign(hl.size(), std::string());
    if (!hl.empty()) {
      std::vector<uint32_t> gids(2 * hl.size());
      std::vector<uint64_t> goff(2 * hl.size() + 1, 0);
      for (size_t j = 0; j < hl.size(); ++j) { gids[2 * j] = sd[hl[j]]; gids[2 * j + 1] = sq[hl[j]]; }
      for (size_t j = 0; j < gids.size(); ++j) { goff[j + 1] = goff[j] + (len[gids[j]] + 31u) / 32u; }
      std::vector<uint64_t> words(std::max<uint64_t>(goff.back(), 1));
      const size_t ids_bytes = (gids.size() * 4 + 7) & ~size_t(7);
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_gather, ids_bytes + gids.size() * 8 + words.size() * 8));
      uint32_t * g_ids = buf<uint32_t>(ctx->d_nw_gather);
      uint64_t * g_off = reinterpret_cast<uint64_t *>(buf<char>(ctx->d_nw_gather) + ids_bytes);
      uint64_t * g_words = g_off + gids.size();
      SWA_HIP(ctx, hipMemcpyAsync(g_ids, gids.data(), gids.size() * 4, hipMemcpyHostToDevice, ctx->stream));
      SWA_HIP(ctx, hipMemcpyAsync(g_off, goff.data(), gids.size() * 8, hipMemcpyHostToDevice, ctx->stream));
      const uint32_t grid = (uint32_t)std::min<size_t>(gids.size(), 4096);
      hipLaunchKernelGGL(k_nw_gather, dim3(grid), dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen, g_ids, g_off,
                         (uint32_t)gids.size(), g_words);
      SWA_HIP(ctx, hipGetLastError());
      SWA_HIP(ctx, hipMemcpyAsync(words.data(), g_words, goff.back() * 8, hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      const unsigned parts = (unsigned)std::max<size_t>(1, std::min<size_t>(hl.size() / 16 + 1, std::min<unsigned>(swa_pool::get().size(), 16u)));
      swa_pool::get().run(parts, [&](unsigned p) {
        swa_nw_scratch sc;
        for (size_t j = hl.size() * p / parts; j < hl.size() * (p + 1) / parts; ++j) {
          const uint32_t k = hl[j];
          const uint64_t nd = swa_nw_align(words.data() + goff[2 * j], len[sd[k]], words.data() + goff[2 * j + 1], len[sq[k]],
                                           mismatch, gapopen, gapextend, sc);
          res[k] = make_uint4((uint32_t)nd, (uint32_t)sc.ops.size(), 0, 0);
          host_cigar[j] = swa_cigar(sc.ops);
        }
      });
    }
    // results in pair order; the CIGARs back to back
    for (uint32_t k = 0; k < m; ++k) {
      const uint32_t tier = res[k].w;
      if (tier > 0) { ctx->nw_totals[tier - 1] += 1; }
    }
    ctx->nw_totals[kLists] += hl.size();
    host_slot.assign(m, UINT32_MAX);                           // pair -> its entry of host_cigar
    for (size_t j = 0; j < hl.size(); ++j) { host_slot[hl[j]] = (uint32_t)j; }
    for (uint32_t k = 0; k < m; ++k) {
      diffs[base + k] = res[k].x;
      columns[base + k] = res[k].y;
      const char * src;
      size_t n;
      if (host_slot[k] != UINT32_MAX) { src = host_cigar[host_slot[k]].data(); n = host_cigar[host_slot[k]].size(); }
      else { src = text.data() + toff[k]; n = res[k].z; }
      if (cigar != nullptr && total + n <= cigar_cap) { std::memcpy(cigar + total, src, n); }
      total += n;
      cigar_end[base + k] = total;
    }
  }
  if (cigar_total != nullptr) { *cigar_total = total; }
  if (total > cigar_cap || (cigar == nullptr && total > 0)) {
    return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_nw_batch: CIGAR buffer too small (*cigar_total = need)");
  }
  return SWA_OK;
}

extern "C" int swa_nw_batch_totals(const swa_ctx * ctx, uint64_t * out4) {
  if (ctx == nullptr || out4 == nullptr) { return SWA_E_ARG; }
  for (uint32_t t = 0; t < kTiers; ++t) { out4[t] = ctx->nw_totals[t]; }
  out4[kTiers] = 0;                                            // left by the LDS tiers: the wide tiers and the host
  for (uint32_t t = kTiers; t <= kLists; ++t) { out4[kTiers] += ctx->nw_totals[t]; }
  return SWA_OK;
}

extern "C" int swa_nw_batch_tiers(const swa_ctx * ctx, uint64_t * out8) {
  if (ctx == nullptr || out8 == nullptr) { return SWA_E_ARG; }
  for (uint32_t t = 0; t <= kLists; ++t) { out8[t] = ctx->nw_totals[t]; }
  return SWA_OK;
}

extern "C" int swa_nw_batch_text_full(const swa_ctx * ctx, uint64_t * out1) {
  if (ctx == nullptr || out1 == nullptr) { return SWA_E_ARG; }
  *out1 = ctx->nw_text_full;
  return SWA_OK;
}
