// nw_trace.hip — seam B5: the uclust alignments (-u) on gfx950, with their traceback.
//
// Replaces the nw() call per H line of the reference's uclust writers (src/algod1.cc:896-925, src/algo.cc:620-655,
// src/nw.cc:237-255): for pairs (d, q) = (member, seed) of the resident database, the reference's tie-broken
// minimum-cost global alignment with affine gaps, returned as the difference count (columns - matches), the alignment
// length and the CIGAR text.  host/nw_host.cpp (swa_nw_align) is the specification: same comparisons, same direction
// bits (src/nw.cc:91-103), same walk-back priority and state machine (src/nw.cc:139-172), so the result is equal bit for
// bit, not merely equally optimal.
//
// What carries that equality is written once and both kernel templates call it: nw_cell (one cell of the recurrence),
// nw_walk_back (one lane walks back and writes the run-length CIGAR into LDS) and nw_store_text (room in the packed text
// buffer, the copy out of LDS, the pair's result; or "full").  The kernels differ in where a band offset (column - row)
// lives, where the direction bits are kept and what a full text buffer means:
//   * LDS tiers (k_nw_trace<G>, G = 16, 32, 64): a group of G lanes aligns one pair, lane <-> band offset, one anti-
//     diagonal and one DPP shift each way per step (as k_align in align.hip).  Lane 0 and the lanes above 2W + 1 are guards
//     that hold the "outside the band" value for ever, so W = (G - 3) / 2: 6, 14, 30.  Direction bits: LDS, one u32 column
//     per lane.  A pair that finds the text buffer full goes to the next list, like one that is not certified.
//   * wide tiers (k_nw_trace_wide<K>, K = 1, 2, 4, 8): one wave aligns one pair, each lane owns K adjacent band offsets in
//     registers (offset index x = lane * K + j; x = 0 and x > 2W + 1 are the guards), so W = (64 K - 3) / 2: 30, 62, 126,
//     254.  Only a lane's outermost offsets cross to its neighbours; for K > 1 the offsets of one parity are live on a
//     step, K / 2 cells per lane.  Direction bits: a global scratch slot per wave, laid out [word][j][lane] (a word per
//     lane = one 256-byte line), read back through L2 by the walking lane.  They take what the LDS tiers cannot: min(dl,
//     ql) > 1024, |dl - ql| > 30, and what the 64-lane tier failed to certify.  Slots are sized by the slice's longest
//     min(dl, ql) and the grid is cut until they fit kBitsBudget.  A pair that finds the text buffer full goes to the
//     host at once, and is counted.
//   * certificate: a result is accepted only when the band's end cost C satisfies C < gapopen + (W + 1) * gapextend.  A
//     path that leaves the band has paid one gap opening and W + 1 gap columns by then, and every value the walk-back
//     compares has its smaller side <= C; so each direction bit it reads is the full matrix's, wherever
//     the bits are kept.  Pairs that fail go to a wider tier (kTier says which).
//   * the host (swa_nw_align, inside the same call) aligns what is left: pairs the widest tier cannot certify, pairs with
//     dl + ql > kWideMaxSum, pairs whose costs could overflow 32 bits, and the pairs a wide tier could not store.
#include "swa_internal.h"
#include "host/nw_host.h"
#include "host/pool.h"

#include <algorithm>
#include <cstddef>
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

constexpr int lds_half_width(int G) { return (G - 3) / 2; }              // G lanes, one band offset each, two guards
constexpr int wide_half_width(int K) { return (kBlock * K - 3) / 2; }    // 64 lanes, K band offsets each

// the device's status block behind the lists
struct NwStatus {
  uint32_t count[kLists + 1];      // entries of each list (the tiers append to later ones; list kLists is the host's)
  unsigned long long text_used;    // bytes asked of the packed text buffer (may pass its size)
  uint32_t text_full;              // pairs a wide tier certified but could not store
};
constexpr size_t kStatusRoom = 64;   // bytes kept for it
static_assert(sizeof(NwStatus) <= kStatusRoom && offsetof(NwStatus, count) == 0 && offsetof(NwStatus, text_used) == 4 * (kLists + 1) &&
              offsetof(NwStatus, text_used) % 8 == 0 && offsetof(NwStatus, text_full) == offsetof(NwStatus, text_used) + 8, "NwStatus layout");

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

#include "wave_ops.inc"   // from_lane_below, from_lane_above, wave_mem_sync

__device__ __forceinline__ uint32_t nt_at(const uint64_t * w, int p) { return (uint32_t)(w[p >> 5] >> ((p & 31) << 1)) & 3u; }

struct NwCell { uint32_t h, bits, e, f; };   // cost, direction bits, the horizontal / vertical gap state handed on

// A cell from the horizontal gap state of (r, c - 1), the vertical gap state of (r - 1, c) and H(r - 1, c - 1).  The callers
// put the borders in (host/nw_host.cpp): H(-1, c) = go + (c + 1) ge, H(r, -1) = go + (r + 1) ge, H(-1, -1) = 0; horizontal
// state entering column 0 = 2 go + (r + 2) ge, vertical state entering row 0 = 2 go + (c + 2) ge.  (Taking r and c in here
// changes the induction variables the compiler picks for the anti-diagonal loops: profiles/r11/NOTES.md.)
__device__ __forceinline__ NwCell nw_cell(uint32_t across, uint32_t down, uint32_t diag, bool mis, uint32_t mm,
                                          uint32_t go, uint32_t ge) {
  uint32_t h = diag + (mis ? mm : 0u);
  uint32_t bits = 0;
  if (across < h) { bits |= kUp; h = across; }
  if (down < h) { h = down; }
  if (down == h) { bits |= kLeft; }
  const uint32_t opened = h + go + ge;
  const uint32_t across_n = across + ge, down_n = down + ge;
  if (across_n < opened) { bits |= kExtUp; }
  if (down_n < opened) { bits |= kExtLeft; }
  return {h, bits, min(across_n, opened), min(down_n, opened)};
}

struct NwWalk { int start; uint32_t diffs, columns; };   // the CIGAR is tx[start, textcap)

// Walk back from the last cell (host/nw_host.cpp, src/nw.cc:139-172), one lane; the run-length CIGAR is written right
// to left.  Direction bits: 4 a cell, 8 cells of a diagonal a u32, cell (r, c) being cell min(r, c) of diagonal c - r;
// word_at(cell, offset) is the u32 that holds those of cell `cell` of diagonal `offset`.
template <class WordAt>
__device__ __forceinline__ NwWalk nw_walk_back(const uint64_t * dw, const uint64_t * qw, int dl, int ql, char * tx, uint32_t textcap,
                                               WordAt word_at) {
  int pos = (int)textcap;
  char run_op = 0;
  uint32_t run_len = 0, matches = 0, columns = 0;
  auto flush = [&]() {                                         // one run, written right to left: count (if > 1), then op
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
    const uint32_t bits = (word_at(cell, c - r) >> ((cell & 7) << 2)) & 15u;
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
  return {pos, columns - matches, columns};
}

// The G lanes of a pair's group (t = 0 .. G - 1, the first of them lane `lead` of the wave) move its CIGAR tx[start,
// textcap) to the packed text buffer and write the pair's result.  False: the buffer is full, nothing was written.
template <int G>
__device__ __forceinline__ bool nw_store_text(const NwArgs & a, uint32_t k, const char * tx, int start, uint32_t diffs, uint32_t columns,
                                              int t, int lead) {
  const uint32_t len = a.textcap - (uint32_t)start;
  unsigned long long off = 0;
  if (t == 0) { off = atomicAdd(a.text_used, (unsigned long long)len); }
  off = (unsigned long long)__shfl((long long)off, lead, kBlock);
  if (off + len > a.text_cap) { return false; }
  for (uint32_t b = (uint32_t)t; b < len; b += G) { a.text[off + b] = tx[start + (int)b]; }
  if (t == 0) {
    a.res[k] = make_uint4(diffs, columns, len, a.tier + 1);
    a.text_off[k] = off;
  }
  return true;
}

template <int G>
__global__ __launch_bounds__(kBlock) void k_nw_trace(const NwArgs a) {
  extern __shared__ uint64_t lds[];
  constexpr int kGroups = kBlock / G;
  constexpr int W = lds_half_width(G);
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
    wave_mem_sync();                                           // the previous pair's LDS readers are done
    {
      const uint64_t * gd = a.seqs + a.seq_off[did];
      const uint64_t * gq = a.seqs + a.seq_off[qid];
      for (int w = t; w < ((dl + 31) >> 5); w += G) { dw[w] = gd[w]; }
      for (int w = t; w < ((ql + 31) >> 5); w += G) { qw[w] = gq[w]; }
    }
    wave_mem_sync();
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
        const uint32_t across = c == 0 ? 2u * go + (uint32_t)(r + 2) * ge : e_nb;
        const uint32_t down = r == 0 ? 2u * go + (uint32_t)(c + 2) * ge : f_nb;
        const uint32_t diag = (r == 0 || c == 0) ? ((r | c) == 0 ? 0u : go + (uint32_t)(r + c) * ge) : h_own;
        const NwCell x = nw_cell(across, down, diag, mis, mm, go, ge);
        if (act) {
          h_own = x.h;
          e_out = x.e;
          f_out = x.f;
          const int cell = r < c ? r : c;
          acc |= x.bits << ((cell & 7) << 2);
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
    wave_mem_sync();
    NwWalk w{0, 0, 0};
    if (certified && t == 0) {
      w = nw_walk_back(dw, qw, dl, ql, tx, a.textcap,
                       [&](int cell, int offset) { return bitmem[(cell >> 3) * kBlock + group * G + offset + W + 1]; });
    }
    wave_mem_sync();
    const int start = __shfl(w.start, group * G, kBlock);
    const bool done = certified && nw_store_text<G>(a, k, tx, start, w.diffs, w.columns, t, group * G);
    if (!done && t == 0) { a.next_list[atomicAdd(a.next_count, 1u)] = k; }   // not certified, or no room for its text
  }
}

// One wave, one pair, K band offsets a lane: offset index x = lane * K + j <-> band offset x - 1 - W.
template <int K>
__global__ __launch_bounds__(kBlock) void k_nw_trace_wide(const NwArgs a) {
  extern __shared__ uint64_t lds[];
  constexpr int W = wide_half_width(K);
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
    wave_mem_sync();                                           // the previous pair's LDS readers are done
    if (feasible) {
      const uint64_t * gd = a.seqs + a.seq_off[did];
      const uint64_t * gq = a.seqs + a.seq_off[qid];
      for (int w = lane; w < ((dl + 31) >> 5); w += kBlock) { dw[w] = gd[w]; }
      for (int w = lane; w < ((ql + 31) >> 5); w += kBlock) { qw[w] = gq[w]; }
    }
    wave_mem_sync();
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
        const uint32_t e_nb = j == 0 ? e_in : e_out[j == 0 ? 0 : j - 1];
        const uint32_t f_nb = j == K - 1 ? f_in : f_out[j == K - 1 ? j : j + 1];
        const bool mis = nt_at(dw, rc_) != nt_at(qw, cc_);
        const uint32_t across = c == 0 ? 2u * go + (uint32_t)(r + 2) * ge : e_nb;
        const uint32_t down = r == 0 ? 2u * go + (uint32_t)(c + 2) * ge : f_nb;
        const uint32_t diag = (r == 0 || c == 0) ? ((r | c) == 0 ? 0u : go + (uint32_t)(r + c) * ge) : h_own[j];
        const NwCell y = nw_cell(across, down, diag, mis, mm, go, ge);
        if (act) {
          h_own[j] = y.h;
          e_out[j] = y.e;
          f_out[j] = y.f;
          const int cell = r < c ? r : c;
          acc[j] |= y.bits << ((cell & 7) << 2);
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
    wave_mem_sync();
    NwWalk w{0, 0, 0};
    if (certified && lane == 0) {
      size_t have = ~size_t(0);                                // the word held in `word`
      uint32_t word = 0;
      w = nw_walk_back(dw, qw, dl, ql, tx, a.textcap, [&](int cell, int offset) {
        const int x = offset + W + 1;
        const size_t at = ((size_t)(cell >> 3) * K + (x & (K - 1))) * kBlock + (x >> kShift);
        if (at != have) { word = bitmem[at]; have = at; }
        return word;
      });
    }
    wave_mem_sync();
    const int start = __shfl(w.start, 0, kBlock);
    if (certified) {
      if (!nw_store_text<kBlock>(a, k, tx, start, w.diffs, w.columns, lane, 0) && lane == 0) {
        atomicAdd(a.text_full, 1u);                            // text buffer full: a wider band would find it full again
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

// ---- the host side ----------------------------------------------------------------------------------------------------

// The device tiers in the order they run.  A tier takes a pair with |dl - ql| <= W; what it cannot certify it appends to
// list `fail_to` (kLists: the host's).  The 64-lane LDS tier skips the K = 1 wide tier, whose band is no wider.
struct Tier { bool wide; int n; uint32_t W, fail_to; void (*kernel)(const NwArgs); };   // n: G lanes a pair, or K offsets a lane
const Tier kTier[kLists] = {
    {false, 16, lds_half_width(16), 1, k_nw_trace<16>},      {false, 32, lds_half_width(32), 2, k_nw_trace<32>},
    {false, 64, lds_half_width(64), 4, k_nw_trace<64>},      {true, 1, wide_half_width(1), 4, k_nw_trace_wide<1>},
    {true, 2, wide_half_width(2), 5, k_nw_trace_wide<2>},    {true, 4, wide_half_width(4), 6, k_nw_trace_wide<4>},
    {true, 8, wide_half_width(8), kLists, k_nw_trace_wide<8>}};

struct Scoring { uint64_t mismatch, gapopen, gapextend; };

// 32-bit costs: every finite value the kernels form is below mm + 3 go + (dl + ql + 4) ge; it must stay below kInf
bool fits(const Scoring & sc, uint32_t dl, uint32_t ql) {
  const unsigned __int128 top = (unsigned __int128)sc.mismatch + 3 * (unsigned __int128)sc.gapopen + (unsigned __int128)(dl + ql + 4) * sc.gapextend;
  return top < kInf;
}
// A wide tier takes a pair whose slot fits the budget at K = 8 (so that every later tier can take it too) and whose
// sequences and CIGAR text fit LDS.
bool wide_fits(uint32_t dl, uint32_t ql) {
  return (uint64_t)dl + ql <= kWideMaxSum && (uint64_t)((std::min(dl, ql) + 7) / 8) * 8 * kBlock * 4 <= kBitsBudget;
}

struct Extent {                                                // what a launch sizes LDS and slots by
  uint32_t maxlen = 1, maxmin = 1, maxsum = 1;
  void add(uint32_t dl, uint32_t ql) { add(Extent{std::max(dl, ql), std::min(dl, ql), dl + ql}); }
  void add(const Extent & o) { maxlen = std::max(maxlen, o.maxlen); maxmin = std::max(maxmin, o.maxmin); maxsum = std::max(maxsum, o.maxsum); }
  uint32_t maxwords() const { return (maxlen + 31) / 32 + 1; }
  uint32_t bitwords() const { return (maxmin + 7) / 8; }
  uint32_t textcap() const { return (maxsum + 7) & ~7u; }
};

struct Pairs { uint32_t m; const uint32_t * d, * q; };         // one slice of the batch: kSlice pairs at most

struct Plan {                                                  // the device pass of a slice
  std::vector<uint32_t> lists[kLists + 1];                     // pairs by the tier they enter at (kLists: the host)
  struct { Extent ext; uint32_t room, grid; } tier[kLists];    // every pair that can reach the tier; a bound of its list (0: no launch)
  unsigned long long text_cap;
  size_t bits_bytes;                                           // the wide tiers' slots: the largest grid * slot of any of them
};

struct Results {                                               // of a slice
  std::vector<uint4> res;                                      // per pair: diffs, columns, CIGAR length, tier + 1 (0: the host's)
  std::vector<unsigned long long> toff;
  std::string text;
  std::vector<std::string> host_cigar;                         // of the host's list, entry by entry
};

// lengths of the resident database on the host: the batch sorts its pairs into tiers and sizes LDS by them
int host_seqlen(swa_ctx * ctx) {
  if (ctx->up.nw_seqlen.size() == ctx->db.n) { return SWA_OK; }
  ctx->up.nw_seqlen.resize(ctx->db.n);
  if (ctx->db.n == 0) { return SWA_OK; }
  SWA_HIP(ctx, hipMemcpyAsync(ctx->up.nw_seqlen.data(), ctx->db.seqlen, (size_t)ctx->db.n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

template <class T>
T * buf(swa_dbuf & b) { return static_cast<T *>(b.ptr); }

int check_args(swa_ctx * ctx, uint64_t npairs, const uint32_t * d_ids, const uint32_t * q_ids, const uint32_t * diffs,
               const uint32_t * columns, const uint64_t * cigar_end) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (npairs > 0 && (d_ids == nullptr || q_ids == nullptr || diffs == nullptr || columns == nullptr || cigar_end == nullptr)) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_nw_batch: null result array");
  }
  if (ctx->db.seqs == nullptr && npairs > 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_nw_batch: no database resident"); }
  for (uint64_t k = 0; k < npairs; ++k) {
    if (d_ids[k] >= ctx->db.n || q_ids[k] >= ctx->db.n) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_nw_batch: amplicon id out of range"); }
  }
  return SWA_OK;
}

// Host only: every pair to the list of the narrowest tier that may take it, and what each launch is sized by.
Plan plan_slice(const Pairs & s, const uint32_t * len, const Scoring & sc, uint32_t num_cus) {
  Plan p{};
  for (uint32_t k = 0; k < s.m; ++k) {
    const uint32_t dl = len[s.d[k]], ql = len[s.q[k]];
    const uint32_t delta = dl > ql ? dl - ql : ql - dl;
    uint32_t first = kLists, end = kLists;                     // the tiers the pair may enter at
    if (fits(sc, dl, ql)) {
      if (std::min(dl, ql) <= kMaxCells && delta <= kTier[kTiers - 1].W) { first = 0; end = kTiers; }
      else if (wide_fits(dl, ql)) { first = kTiers; }
    }
    uint32_t tier = kLists;
    for (uint32_t t = first; t < end; ++t) { if (delta <= kTier[t].W) { tier = t; break; } }
    p.lists[tier].push_back(k);
    if (tier < kLists) { p.tier[tier].ext.add(dl, ql); }
  }
  // Tier t's list holds the pairs that enter there and whatever the tiers that fail to it pass on.  How many that will
  // be is known only on the device: room bounds the list; waves sizes a wide tier's grid and slots, and counts what an LDS
  // tier passes on as kPassedWaves at most (such pairs are rare: 1 and 10 of 10 M in profiles/r07; the kernel's loop
  // strides by the grid)
  uint32_t waves[kLists], wide_own = 0;
  for (uint32_t t = 0; t < kLists; ++t) {
    p.tier[t].room = waves[t] = (uint32_t)p.lists[t].size();
    if (kTier[t].wide) { wide_own += waves[t]; }
  }
  p.text_cap = kTextPerPair * (s.m - p.lists[kLists].size()) + kTextPerWidePair * wide_own + (1u << 16);
  for (uint32_t t = 0; t < kLists; ++t) {
    const uint32_t to = kTier[t].fail_to;                      // a later tier: its figures are still open
    if (to == kLists) { continue; }
    p.tier[to].ext.add(p.tier[t].ext);
    p.tier[to].room += p.tier[t].room;
    waves[to] += kTier[t].wide ? waves[t] : std::min(p.tier[t].room, kPassedWaves);
  }
  p.tier[0].ext = p.tier[1].ext = p.tier[kTiers - 1].ext;      // the LDS tiers are sized alike, by all their pairs
  for (uint32_t t = 0; t < kLists; ++t) {
    const uint32_t n = (uint32_t)kTier[t].n, room = p.tier[t].room;
    if (!kTier[t].wide) {                                      // kBlock / G pairs a workgroup, 32 workgroups a CU at most
      p.tier[t].grid = std::max(1u, std::min((room + kBlock / n - 1) / (kBlock / n), num_cus * 32u));
    } else if (room > 0) {             // a wave a pair, 16 a CU at most, and no more slots than kBitsBudget holds
      const uint64_t slot_bytes = (uint64_t)p.tier[t].ext.bitwords() * n * kBlock * 4;
      p.tier[t].grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint64_t>(waves[t], (uint64_t)num_cus * 16u), kBitsBudget / slot_bytes));
      p.bits_bytes = std::max<size_t>(p.bits_bytes, slot_bytes * p.tier[t].grid);
    }
  }
  return p;
}

// The device pass of a planned slice: upload, the tiers in order, results and text back.  What the tiers left to the host
// is appended to the plan's host list.
int run_device_tiers(swa_ctx * ctx, const Pairs & s, Plan & p, const Scoring & sc, Results & out) {
  const uint32_t m = s.m;
  NwStatus st{};
  for (uint32_t t = 0; t < kLists; ++t) { st.count[t] = (uint32_t)p.lists[t].size(); }
  SWA_TRY(swa_reserve(ctx, ctx->d_nw_ids, (size_t)2 * m * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_nw_lists, (size_t)(kLists + 1) * m * sizeof(uint32_t) + kStatusRoom));
  SWA_TRY(swa_reserve(ctx, ctx->d_nw_res, (size_t)m * (sizeof(uint4) + sizeof(unsigned long long))));
  SWA_TRY(swa_reserve(ctx, ctx->d_nw_text, (size_t)p.text_cap));
  if (p.bits_bytes > 0) { SWA_TRY(swa_reserve(ctx, ctx->d_nw_bits, p.bits_bytes)); }
  uint32_t * ids = buf<uint32_t>(ctx->d_nw_ids);
  uint32_t * d_lists = buf<uint32_t>(ctx->d_nw_lists);         // list t at d_lists + t * m, the status block behind them
  NwStatus * d_st = reinterpret_cast<NwStatus *>(d_lists + (size_t)(kLists + 1) * m);
  uint4 * d_res = buf<uint4>(ctx->d_nw_res);
  unsigned long long * d_toff = reinterpret_cast<unsigned long long *>(d_res + m);
  SWA_HIP(ctx, hipMemcpyAsync(ids, s.d, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
  SWA_HIP(ctx, hipMemcpyAsync(ids + m, s.q, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
  for (uint32_t t = 0; t < kLists; ++t) {
    if (!p.lists[t].empty()) {
      SWA_HIP(ctx, hipMemcpyAsync(d_lists + (size_t)t * m, p.lists[t].data(), p.lists[t].size() * 4, hipMemcpyHostToDevice, ctx->stream));
    }
  }
  SWA_HIP(ctx, hipMemcpyAsync(d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(d_res, 0, (size_t)m * sizeof(uint4), ctx->stream));
  NwArgs a{};
  a.seqs = ctx->db.seqs; a.seq_off = ctx->db.seq_off; a.seqlen = ctx->db.seqlen;
  a.d_ids = ids; a.q_ids = ids + m;
  a.res = d_res; a.text_off = d_toff; a.text = buf<char>(ctx->d_nw_text);
  a.text_used = &d_st->text_used; a.text_full = &d_st->text_full; a.text_cap = p.text_cap;
  a.host_list = d_lists + (size_t)kLists * m; a.host_count = &d_st->count[kLists];
  a.bits = buf<uint32_t>(ctx->d_nw_bits);
  a.mismatch = (uint32_t)sc.mismatch; a.gapopen = (uint32_t)sc.gapopen; a.gapextend = (uint32_t)sc.gapextend;
  for (uint32_t t = 0; t < kLists; ++t) {
    const Tier & tier = kTier[t];
    if (p.tier[t].room == 0) { continue; }
    a.list = d_lists + (size_t)t * m; a.list_count = &d_st->count[t]; a.list_room = p.tier[t].room;
    a.next_list = d_lists + (size_t)tier.fail_to * m; a.next_count = &d_st->count[tier.fail_to];
    a.tier = t;
    a.maxwords = p.tier[t].ext.maxwords(); a.bitwords = p.tier[t].ext.bitwords(); a.textcap = p.tier[t].ext.textcap();
    a.slot_words = tier.wide ? (unsigned long long)a.bitwords * tier.n * kBlock : 0;
    // LDS: member and seed words and the CIGAR text of each pair of the workgroup; an LDS tier's direction bits
    const size_t groups = tier.wide ? 1 : kBlock / tier.n;
    const size_t lds = groups * (2 * a.maxwords * 8 + a.textcap) + (tier.wide ? 0 : (size_t)a.bitwords * kBlock * 4);
    hipLaunchKernelGGL(tier.kernel, dim3(p.tier[t].grid), dim3(kBlock), lds, ctx->stream, a);
    SWA_HIP(ctx, hipGetLastError());
  }
  SWA_HIP(ctx, hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipMemcpyAsync(out.res.data(), d_res, (size_t)m * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipMemcpyAsync(out.toff.data(), d_toff, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->nw_text_full += st.text_full;
  out.text.resize(std::min<unsigned long long>(st.text_used, p.text_cap));
  if (!out.text.empty()) { SWA_HIP(ctx, hipMemcpyAsync(out.text.data(), a.text, out.text.size(), hipMemcpyDeviceToHost, ctx->stream)); }
  std::vector<uint32_t> & hl = p.lists[kLists];                // the tiers' list of what is the host's began at 0
  const size_t classified = hl.size();
  hl.resize(classified + st.count[kLists]);
  if (hl.size() > classified) {
    SWA_HIP(ctx, hipMemcpyAsync(hl.data() + classified, a.host_list, (size_t)st.count[kLists] * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

// The host's list hl: the pairs' words fetched from the device in one gather, aligned by the host's workers.
int align_on_host(swa_ctx * ctx, const Pairs & s, const std::vector<uint32_t> & hl, const uint32_t * len, const Scoring & sc, Results & out) {
  out.host_cigar.assign(hl.size(), std::string());
  if (hl.empty()) { return SWA_OK; }
  std::vector<uint32_t> gids(2 * hl.size());
  std::vector<uint64_t> goff(2 * hl.size() + 1, 0);
  for (size_t j = 0; j < hl.size(); ++j) { gids[2 * j] = s.d[hl[j]]; gids[2 * j + 1] = s.q[hl[j]]; }
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
  swa_pool::get().run(parts, [&](unsigned part) {
    swa_nw_scratch scratch;
    for (size_t j = hl.size() * part / parts; j < hl.size() * (part + 1) / parts; ++j) {
      const uint32_t k = hl[j];
      const uint64_t nd = swa_nw_align(words.data() + goff[2 * j], len[s.d[k]], words.data() + goff[2 * j + 1], len[s.q[k]],
                                       sc.mismatch, sc.gapopen, sc.gapextend, scratch);
      out.res[k] = make_uint4((uint32_t)nd, (uint32_t)scratch.ops.size(), 0, 0);
      out.host_cigar[j] = swa_cigar(scratch.ops);
    }
  });
  return SWA_OK;
}

// The slice's results in pair order, its CIGARs back to back from cigar + total on; the tier counters.
void assemble(swa_ctx * ctx, uint32_t m, const std::vector<uint32_t> & hl, const Results & r, uint32_t * diffs, uint32_t * columns,
              uint64_t * cigar_end, char * cigar, uint64_t cigar_cap, uint64_t & total) {
  ctx->nw_totals[kLists] += hl.size();
  std::vector<uint32_t> host_slot(m, UINT32_MAX);              // pair -> its entry of host_cigar
  for (size_t j = 0; j < hl.size(); ++j) { host_slot[hl[j]] = (uint32_t)j; }
  for (uint32_t k = 0; k < m; ++k) {
    if (r.res[k].w > 0) { ctx->nw_totals[r.res[k].w - 1] += 1; }   // the tier that certified it
    diffs[k] = r.res[k].x;
    columns[k] = r.res[k].y;
    const bool host = host_slot[k] != UINT32_MAX;
    const char * src = host ? r.host_cigar[host_slot[k]].data() : r.text.data() + r.toff[k];
    const size_t n = host ? r.host_cigar[host_slot[k]].size() : r.res[k].z;
    if (cigar != nullptr && total + n <= cigar_cap) { std::memcpy(cigar + total, src, n); }
    total += n;
    cigar_end[k] = total;
  }
}

}  // namespace

int swa_nw_host_seqlen(swa_ctx * ctx) {
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  return host_seqlen(ctx);
}

extern "C" int swa_nw_batch(swa_ctx * ctx, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t npairs,
                            const uint32_t * d_ids, const uint32_t * q_ids, uint32_t * diffs, uint32_t * columns,
                            uint64_t * cigar_end, char * cigar, uint64_t cigar_cap, uint64_t * cigar_total) {
  if (const int rc = check_args(ctx, npairs, d_ids, q_ids, diffs, columns, cigar_end); rc != SWA_OK) { return rc; }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(host_seqlen(ctx));
  for (auto & v : ctx->nw_totals) { v = 0; }
  ctx->nw_text_full = 0;
  const uint32_t * len = ctx->up.nw_seqlen.data();
  const Scoring sc{mismatch, gapopen, gapextend};
  uint64_t total = 0;
  for (uint64_t base = 0; base < npairs; base += kSlice) {
    const Pairs s{(uint32_t)std::min<uint64_t>(kSlice, npairs - base), d_ids + base, q_ids + base};
    Plan p = plan_slice(s, len, sc, (uint32_t)ctx->num_cus);
    const std::vector<uint32_t> & hl = p.lists[kLists];        // the host's pairs: the device pass may add to them
    Results r{std::vector<uint4>(s.m, make_uint4(0, 0, 0, 0)), std::vector<unsigned long long>(s.m, 0), {}, {}};
    if (hl.size() < s.m) { SWA_TRY(run_device_tiers(ctx, s, p, sc, r)); }
    SWA_TRY(align_on_host(ctx, s, hl, len, sc, r));
    assemble(ctx, s.m, hl, r, diffs + base, columns + base, cigar_end + base, cigar, cigar_cap, total);
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
