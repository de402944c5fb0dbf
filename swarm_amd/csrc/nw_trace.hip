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
//     full matrix's.  Pairs that fail go to the next wider tier; pairs that fail the widest, that are
//     too long for the LDS budget, or whose costs could overflow 32 bits are aligned by swa_nw_align on the host inside
//     the same call.
#include "swa_internal.h"
#include "host/nw_host.h"
#include "host/pool.h"

#include <algorithm>
#include <cstdlib>

namespace {

constexpr uint32_t kUp = 1, kLeft = 2, kExtUp = 4, kExtLeft = 8;   // host/nw_host.cpp, src/nw.cc:91-103
constexpr uint32_t kInf = 0x40000000u;            // "outside the band": every finite value stays below 2^30 (host check)
constexpr uint32_t kMaxCells = 1024;              // longest diagonal a lane stores (LDS: 128 words x 64 lanes)
constexpr uint32_t kTiers = 3;                    // G = 16, 32, 64
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
  const uint32_t * len = ctx->nw_seqlen.data();
  // 32-bit costs: every finite value the kernel forms is below mm + 3 go + (dl + ql + 4) ge; it must stay below kInf
  auto fits = [&](uint32_t dl, uint32_t ql) {
    const unsigned __int128 top = (unsigned __int128)mismatch + 3 * (unsigned __int128)gapopen + (unsigned __int128)(dl + ql + 4) * gapextend;
    return top < kInf && std::min(dl, ql) <= kMaxCells;
  };
  static constexpr int kW[kTiers] = {6, 14, 30};

  std::vector<uint4> res;
  std::vector<unsigned long long> toff;
  std::string text;
  std::vector<std::string> host_cigar;
  std::vector<uint32_t> lists[kTiers + 1];
  std::vector<uint32_t> tmp, host_slot;
  uint64_t total = 0;
  for (uint64_t base = 0; base < npairs; base += kSlice) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(kSlice, npairs - base);
    const uint32_t * sd = d_ids + base, * sq = q_ids + base;
    for (auto & l : lists) { l.clear(); }
    uint32_t maxlen = 1, maxmin = 1, maxsum = 1;
    for (uint32_t k = 0; k < m; ++k) {
      const uint32_t dl = len[sd[k]], ql = len[sq[k]];
      const uint32_t delta = dl > ql ? dl - ql : ql - dl;
      uint32_t tier = kTiers;
      if (fits(dl, ql)) {
        for (uint32_t t = 0; t < kTiers; ++t) { if (delta <= (uint32_t)kW[t]) { tier = t; break; } }
      }
      lists[tier].push_back(k);
      if (tier < kTiers) {
        maxlen = std::max(maxlen, std::max(dl, ql));
        maxmin = std::max(maxmin, std::min(dl, ql));
        maxsum = std::max(maxsum, dl + ql);
      }
    }
    res.assign(m, make_uint4(0, 0, 0, 0));
    toff.assign(m, 0);
    const uint32_t on_device = m - (uint32_t)lists[kTiers].size();
    if (on_device > 0) {
      const unsigned long long text_cap = (unsigned long long)kTextPerPair * on_device + (1u << 16);
      // one u32 block: [0, kTiers + 1) list counts, [kTiers + 1] text used (u64, 8-aligned at 8 words)
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_ids, (size_t)2 * m * sizeof(uint32_t)));
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_lists, (size_t)(kTiers + 1) * m * sizeof(uint32_t) + 64));
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_res, (size_t)m * (sizeof(uint4) + sizeof(unsigned long long))));
      SWA_TRY(swa_reserve(ctx, ctx->d_nw_text, (size_t)text_cap));
      uint32_t * ids = buf<uint32_t>(ctx->d_nw_ids);
      uint32_t * dl_ = buf<uint32_t>(ctx->d_nw_lists);
      uint32_t * counts = dl_ + (size_t)(kTiers + 1) * m;
      uint4 * d_res = buf<uint4>(ctx->d_nw_res);
      unsigned long long * d_toff = reinterpret_cast<unsigned long long *>(d_res + m);
      SWA_HIP(ctx, hipMemcpyAsync(ids, sd, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
      SWA_HIP(ctx, hipMemcpyAsync(ids + m, sq, (size_t)m * 4, hipMemcpyHostToDevice, ctx->stream));
      uint32_t hcounts[16] = {};
      for (uint32_t t = 0; t < kTiers; ++t) {
        hcounts[t] = (uint32_t)lists[t].size();
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
      a.text_cap = text_cap;
      a.mismatch = (uint32_t)mismatch; a.gapopen = (uint32_t)gapopen; a.gapextend = (uint32_t)gapextend;
      a.maxwords = (maxlen + 31) / 32 + 1;
      a.bitwords = (maxmin + 7) / 8;
      a.textcap = (maxsum + 7) & ~7u;
      uint32_t room = 0;
      for (uint32_t t = 0; t < kTiers; ++t) {
        a.list = dl_ + (size_t)t * m; a.list_count = counts + t;
        a.next_list = dl_ + (size_t)(t + 1) * m; a.next_count = counts + t + 1;
        a.tier = t;
        room += hcounts[t];                                    // this tier's own pairs + whatever the tiers before it passed on
        if (t == 0) { SWA_TRY(launch_tier<16>(ctx, a, room)); }
        else if (t == 1) { SWA_TRY(launch_tier<32>(ctx, a, room)); }
        else { SWA_TRY(launch_tier<64>(ctx, a, room)); }
      }
      SWA_HIP(ctx, hipMemcpyAsync(hcounts, counts, sizeof(hcounts), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipMemcpyAsync(res.data(), d_res, (size_t)m * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipMemcpyAsync(toff.data(), d_toff, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      // the widest tier appended what it could not certify to the host's list (from entry 0 on: counts[kTiers] began at 0)
      const uint32_t appended = hcounts[kTiers];
      const unsigned long long used = std::min<unsigned long long>(*reinterpret_cast<unsigned long long *>(hcounts + 8), text_cap);
      text.resize(used);
      if (used > 0) { SWA_HIP(ctx, hipMemcpyAsync(text.data(), a.text, used, hipMemcpyDeviceToHost, ctx->stream)); }
      if (appended > 0) {
        tmp.resize(appended);
        SWA_HIP(ctx, hipMemcpyAsync(tmp.data(), dl_ + (size_t)kTiers * m, (size_t)appended * 4, hipMemcpyDeviceToHost, ctx->stream));
      }
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      if (appended > 0) { lists[kTiers].insert(lists[kTiers].end(), tmp.begin(), tmp.begin() + appended); }
    }
    // pairs for the host: their words fetched from the device in one gather, aligned by the host's workers
    const std::vector<uint32_t> & hl = lists[kTiers];
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
    ctx->nw_totals[kTiers] += hl.size();
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
  for (uint32_t t = 0; t <= kTiers; ++t) { out4[t] = ctx->nw_totals[t]; }
  return SWA_OK;
}
