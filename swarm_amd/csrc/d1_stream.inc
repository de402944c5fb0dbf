// d1_stream.inc — the STREAMING index build of the d=1 step (included by d1.hip inside its anonymous namespace, after
// d1_anchor.inc); the partition and the CSR assembly it speaks of are a unit of their own, d1_part.hip.
//
// Round 2 grouped the amplicons with hash tables in HBM: one device-scope atomic per amplicon and index
// (k_anchor_place), one random 8-byte offset read + one random 16-byte record write per member (k_anchor_scatter),
// one random offset read + cursor atomic + random 4-byte write per link (a scatter of the links into counted rows).  rocprofv3 showed what that
// costs on this memory system: an atomic drops its line from L2 and goes to the fabric, every 8- or 16-byte random
// access moves 64-128 bytes — 3.2 of the step's 5.9 ms at 10 M amplicons, 4.4 x the bytes the algorithm needs.
//
// Here nothing is random but the one line per member that the pair kernels fetch anyway:
//
//   amplicon lines   per upload: every amplicon as ONE aligned line of 64 bytes (sequences up to 160 nt) or 128 bytes
//                    (up to 416 nt): packed words | length | abundance rank.  A member fetch is one line, not a record
//                    plus 40 bytes that straddle two.
//   keys             one streaming pass over the lines: 32-bit key of the prefix-side and of the suffix-side anchor
//                    window (the high half of the mixed 64-bit key the tables of round 2 used); records key << 32 | id —
//                    and, on the way, the first partition level's histogram.
//   partition        records grouped by the top bits of the key in LDS-staged, coalesced radix levels (k_part_hist /
//                    flat scan / k_part_scatter: counting sort by digit, tile by tile; no atomics in HBM).  The bucket
//                    starts a level leaves for the next one (or for k_group1 / k_csr_bucket) are written by the
//                    scatter launch itself, from the scanned counts (part_write_starts).  Default:
//                    ONE level of up to 1024 bins until a bucket holds ~10 000 records (k_group1).  Runs of 16 consecutive
//                    tiles go to one XCD (xcd_tile), whose L2 merges their partial lines.  (Round 3 also carried buckets of
//                    ~600 records — k_group — and one-pass first levels with decoupled look-back — k_sweep_*: both measured
//                    slower, profiles/r03/late_experiments.md, and removed in round 4.)
//   groups           one workgroup per bucket: the bucket's groups found in an LDS table, members written in group
//                    order (ids only), the work lists of the pair kernels by size class, identical sequences detected
//                    on the fingerprints inside the prefix groups (the separate duplicate kernels are gone);
//   CSR              the links leave the pair kernels as before (per-wave segments); the same partition primitive sorts
//                    them by the top bits of their source (two levels at 10 M amplicons) until a bucket holds the links
//                    of 256 consecutive sources, k_csr_bucket — a wave per bucket — counts, places and sorts the rows:
//                    no cursor atomics, no per-amplicon count atomics in the pair kernels.
//
// Two keys with equal 32-bit values share a group (about n^2 / 2^33 group pairs): harmless — every pair test is exact.

// Largest group the pair kernels take (k_d1_pairs_tiled: 64 x 64 tiles, any size; quadratic — 0.9 g instructions per
// member — so beyond this the enumerating plain kernel, ~600 per member plus its random probes, is the cheaper one)
constexpr uint32_t kStreamGroupCap = 4096;

// ---- amplicon lines ------------------------------------------------------------------------------------------
// LQ quads per line (4, 8 or 16: d1_anchor.inc); dword [0] length | [1] abundance rank | [2, ..) packed words, zero padded
template <int LQ>
__global__ __launch_bounds__(256) void k_lines_build(const uint64_t * __restrict__ seqs, const uint64_t * __restrict__ seq_off,
                                                     const uint32_t * __restrict__ seqlen, const uint32_t * __restrict__ rank, uint32_t n,
                                                     uint4 * __restrict__ lines) {
  constexpr uint32_t C = 2u * LQ - 1u;                          // words a line holds
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t len = seqlen[i];
    const uint64_t * s = seqs + seq_off[i];
    const uint32_t nw = (len + 31u) >> 5;
    uint32_t d[4 * LQ];
    d[0] = len; d[1] = rank[i];
#pragma unroll
    for (uint32_t k = 0; k < C; ++k) {
      const uint64_t w = k < nw ? s[k] : 0ull;
      d[2 + 2 * k] = (uint32_t)w; d[3 + 2 * k] = (uint32_t)(w >> 32);
    }
    // (only the quads that carry something are written — and the first one always: a line's zero padding is never read
    // beyond the width class of its amplicon, but the readers of a group take the group's width: zeros up to there)
#pragma unroll
    for (uint32_t q = 0; q < (uint32_t)LQ; ++q) { lines[(uint64_t)i * LQ + q] = make_uint4(d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]); }
  }
}

// ---- keys ------------------------------------------------------------------------------------------------------
// 32 nucleotides from position pos of a packed sequence in memory (reads the word after the window's first when the
// window straddles two: the lines end in zero padding or in their neighbour's first quad, the database in two zero words)
__device__ __forceinline__ uint64_t window_at(const uint64_t * words, uint32_t pos) {
  const uint32_t k = pos >> 5, sh = (pos & 31u) << 1;
  const uint64_t lo = words[k];
  return sh != 0u ? (lo >> sh) | (words[k + 1u] << (64u - sh)) : lo;
}

// 32 nucleotides from position pos of a sequence whose first 7 words are in registers (zero padded; pos + 32 <= 224)
__device__ __forceinline__ uint64_t window_of7(const uint64_t (&w)[7], uint32_t pos) {
  const uint32_t k = pos >> 5, sh = (pos & 31u) << 1;
  uint64_t lo = 0ull, hi = 0ull;
#pragma unroll
  for (int j = 0; j < 7; ++j) { lo = (uint32_t)j == k ? w[j] : lo; hi = (uint32_t)j == k + 1u ? w[j] : hi; }
  return sh != 0u ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

// ---- routed index build of a multi-GPU job: the KEY RECORDS travel ----------------------------------------------------------
// Every rank keys the amplicons of its own contiguous slice — a streaming pass over its share of the packed database — and
// files, per index and per OWNING rank, the finished key record (record key << 32 | id): 8 bytes per amplicon and index
// through the exchange instead of the 4 of a bare id (rounds 4-5), and the owner starts at the partition: no k_keys pass of
// random 64-byte line fetches out of a replicated line array N times its share (0.55 ms of the 2.5 a rank's share of an
// 8 x 10 M job took, VERDICT r05 next 2).  out_rec[(which * world + owner) * cap + ..], counts[which * world + owner];
// counts[2 * world] != 0: a region overflowed.
__global__ __launch_bounds__(256) void k_anchor_route_records(const uint64_t * __restrict__ seqs, const uint64_t * __restrict__ seq_off,
                                                              const uint32_t * __restrict__ seqlen, uint32_t first, uint32_t count,
                                                              uint32_t world, uint32_t win_a, uint32_t win_b, uint32_t nwin,
                                                              unsigned long long * __restrict__ out_rec, uint64_t cap, uint32_t * counts) {
  __shared__ uint32_t hist[2 * kRouteMaxWorld], base[2 * kRouteMaxWorld];
  constexpr uint32_t kPer = 4;
  const uint32_t tile = 256u * kPer;
  for (uint32_t t0 = blockIdx.x * tile; t0 < count; t0 += gridDim.x * tile) {
    if (threadIdx.x < 2u * world) { hist[threadIdx.x] = 0u; }
    __syncthreads();
    uint32_t dest[kPer][2], place[kPer][2], key[kPer][2];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const uint32_t e = t0 + k * 256u + threadIdx.x;
      dest[k][0] = dest[k][1] = 0xFFFFFFFFu;
      if (e < count) {
        const uint32_t i = first + e;
        const uint32_t len = seqlen[i];
        const uint64_t * s = seqs + seq_off[i];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
          if (len >= (which == 0 ? win_a : win_b) + kAnchor * nwin) {
            const uint64_t mixed = mix64(anchor_key(s, len, which, win_a, win_b, nwin));
            const uint32_t d = (uint32_t)which * world + anchor_owner(mixed, world);
            dest[k][which] = d;
            key[k][which] = record_key(mixed, len);
            place[k][which] = atomicAdd(&hist[d], 1u);
          }
        }
      }
    }
    __syncthreads();
    if (threadIdx.x < 2u * world) { base[threadIdx.x] = hist[threadIdx.x] != 0u ? atomicAdd(&counts[threadIdx.x], hist[threadIdx.x]) : 0u; }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        const uint32_t d = dest[k][which];
        if (d == 0xFFFFFFFFu) { continue; }
        const uint64_t at = (uint64_t)base[d] + place[k][which];
        if (at < cap) {
          out_rec[(uint64_t)d * cap + at] = ((unsigned long long)key[k][which] << 32) | (first + t0 + k * 256u + threadIdx.x);
        } else { counts[2u * world] = 1u; }
      }
    }
    __syncthreads();
  }
}

struct KeyArgs {
  const uint4 * lines;               // line_quads quads per line
  uint32_t line_quads;
  const uint64_t * seqs; const uint64_t * seq_off;   // the packed database: for the few sequences longer than a line holds
  uint32_t n;
  const uint32_t * list[kMaxIdx];    // routed build: the amplicons to key for index i (else nullptr: all of [0, n))
  uint32_t list_count[kMaxIdx];
  unsigned long long * rec[kMaxIdx]; // out: record_key << 32 | id, or kRecAbsent; position = amplicon id (list position when routed)
  uint32_t owner_rank, owner_world;
  uint32_t win_a, win_b, minlen, window_mode;
  uint32_t nwin;                     // words (32 nt) per anchor window: 1, 2 or 4 (anchor_key)
  uint32_t * flags;                  // the status block's: kFlagUnserved, kFlagOverMass, kFlagShortest
  unsigned long long * guard;        // the status block's: [kGuardMade + which] records made for index `which` (what the groups must add up to)
  uint32_t fault;                    // test hook (SWA_D1_GUARD_TEST): 1 = a few suffix-side keys are wrong, 2 = a few records get lost
  // The too-short seeds (len < minlen) go to the enumerating kernel, and whatever is one edit from one of them is at most
  // minlen long: those amplicons are marked (bit 2 of their `over` byte) and counted (kFlagOverMass) as members of the table that
  // kernel probes — build_member_index — so that a few short reads do not cost the database-wide table (r05).  nullptr: off.
  uint8_t * mark_short;
  // k_keys<LQ, true>: the first partition level's histogram on the way (the flat count arrays of both indexes, layout of
  // part_flat for one segment: digit * tiles + tile); a workgroup then takes whole tiles of hist_tile amplicons
  uint32_t * hist_cnt[kMaxIdx];
  uint32_t hist_bits, hist_tile, hist_ntiles, hist_run_bits;
  // ... and that level's tile table (what k_part_tiles makes of ONE chunk whose size the host knows: first tile 0, the
  // number of tiles, the entry behind the last count — the scan's total); nullptr: k_part_tiles runs
  uint32_t * hist_ctile[kMaxIdx];
};

// One pass over the lines: per index the key record of every amplicon (the 29-bit key of its window | its width class |
// its id) and, for the prefix index, the fingerprint of its sequence.  A lane reads the first 64 bytes of its line — a
// whole line of a database of short reads, the first seven words of any other — and works from those registers; what a
// longer sequence has beyond them (fingerprint, suffix-side window) it reads word by word from the line again, or, when the
// line could not hold it, from the packed database: loops of the few lanes that have long sequences.
template <bool HIST>
__global__ __launch_bounds__(256) void k_keys(const KeyArgs a) {
  const uint32_t LQ = a.line_quads, C = 2u * LQ - 1u;           // words a line holds
  const int which_only = a.list[0] != nullptr || a.list[1] != nullptr ? (int)blockIdx.y : -1;   // routed: one index per y
  const uint32_t total = which_only < 0 ? a.n : a.list_count[which_only];
  bool unserved = false;
  uint32_t shortest = 0xFFFFFFFFu, marked = 0u;
  uint32_t made[2] = {0u, 0u};
  __shared__ uint32_t hist[HIST ? 2 : 1][HIST ? 1024 : 1];
  const uint32_t hbins = 1u << a.hist_bits, hshift = 32u - a.hist_bits;
  // HIST: turns over tiles (xcd_tile), inside a tile hist_tile / 256 amplicons per thread; else a plain grid-stride walk
  const uint32_t per_turn = HIST ? a.hist_tile / 256u : 1u;
  const uint32_t turns = HIST ? (a.hist_ntiles + (8u << a.hist_run_bits) - 1u) & ~((8u << a.hist_run_bits) - 1u) : 0u;
  for (uint32_t v = blockIdx.x; HIST ? v < turns : v * blockDim.x + threadIdx.x < total; v += gridDim.x) {
    const uint32_t t = HIST ? xcd_tile(v, a.hist_run_bits) : v;
    if (HIST) {
      if (t >= a.hist_ntiles) { continue; }
      for (uint32_t b = threadIdx.x; b < hbins; b += 256u) { hist[0][b] = 0u; hist[HIST ? 1 : 0][b] = 0u; }
      __syncthreads();
    }
   for (uint32_t k = 0; k < per_turn; ++k) {
    const uint32_t e = HIST ? t * a.hist_tile + k * 256u + threadIdx.x : v * blockDim.x + threadIdx.x;
    if (e >= total) { break; }
    const uint32_t i = which_only < 0 ? e : a.list[which_only][e];
    const uint4 * L = a.lines + (uint64_t)i * LQ;
    uint32_t d[16];
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) { const uint4 x = L[q]; d[4 * q] = x.x; d[4 * q + 1] = x.y; d[4 * q + 2] = x.z; d[4 * q + 3] = x.w; }
    const uint32_t len = d[0], nw = (len + 31u) >> 5;
    const bool fits = nw <= C;                                  // (else: nothing but the length comes from the line)
    uint64_t w7[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) { w7[q] = (uint64_t)d[2 + 2 * q] | ((uint64_t)d[3 + 2 * q] << 32); }
    const uint64_t * words = fits ? reinterpret_cast<const uint64_t *>(L) + 1 : a.seqs + a.seq_off[i];
    if (which_only < 0) {
      shortest = min(shortest, len);
      unserved |= len < a.minlen;     // (no run rule here: the pair kernels divide a seed's links by the window itself)
      if (a.mark_short != nullptr && len <= a.minlen) {
        atomicOr(reinterpret_cast<unsigned int *>(a.mark_short + (i & ~3u)), 4u << (8u * (i & 3u)));
        ++marked;
      }
    }
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      if (which_only >= 0 && which != which_only) { continue; }
      unsigned long long rec = kRecAbsent;
      if (len >= (which == 0 ? a.win_a : a.win_b) + kAnchor * a.nwin) {
        const uint32_t pos = which == 0 ? a.win_a : len - a.win_b - kAnchor * a.nwin;
        uint64_t win[4] = {0ull, 0ull, 0ull, 0ull};
        if (which == 0 && fits && a.win_a == 0u) {              // (the usual prefix window: the first words, in registers)
#pragma unroll
          for (uint32_t q = 0; q < 4u; ++q) { if (q < a.nwin) { win[q] = w7[q]; } }
        } else if (fits && nw <= 7u) {                           // (a window anywhere in a sequence the registers hold whole)
#pragma unroll
          for (uint32_t q = 0; q < 4u; ++q) { if (q < a.nwin) { win[q] = window_of7(w7, pos + kAnchor * q); } }
        } else {
#pragma unroll
          for (uint32_t q = 0; q < 4u; ++q) { if (q < a.nwin) { win[q] = window_at(words, pos + kAnchor * q); } }
        }
        const uint64_t mixed = mix64(anchor_fold(win, a.nwin, which));   // = mix64(anchor_key())
        // (routed lists hold exactly what this rank owns)
        if (which_only >= 0 || a.owner_world == 1u || anchor_owner(mixed, a.owner_world) == a.owner_rank) {
          rec = ((unsigned long long)record_key(mixed, len) << 32) | i;
          // (what the anomaly looked like, on purpose: the guard's regression test, tests/test_guard_gpu.py)
          if (a.fault == 1u && which == 1 && i % 5021u == 7u) { rec ^= 0x0000A5A000000000ull; }
        }
      }
      made[which] += rec != kRecAbsent ? 1u : 0u;
      if (a.fault == 2u && which == 0 && i % 5021u == 7u) { rec = kRecAbsent; }
      a.rec[which][e] = rec;
      if (HIST && rec != kRecAbsent) { atomicAdd(&hist[HIST ? which : 0][((uint32_t)(rec >> 32) >> hshift) & (hbins - 1u)], 1u); }
    }
   }
    if (HIST) {
      __syncthreads();
      for (uint32_t b = threadIdx.x; b < hbins; b += 256u) {
        a.hist_cnt[0][(uint64_t)b * a.hist_ntiles + t] = hist[0][b];
        a.hist_cnt[1][(uint64_t)b * a.hist_ntiles + t] = hist[HIST ? 1 : 0][b];
      }
      __syncthreads();
    }
  }
  if (HIST && blockIdx.x == 0 && threadIdx.x < kMaxIdx && a.hist_ctile[threadIdx.x] != nullptr) {
    uint32_t * ctile = a.hist_ctile[threadIdx.x];
    ctile[0] = 0u; ctile[1] = a.hist_ntiles;
    a.hist_cnt[threadIdx.x][(uint64_t)a.hist_ntiles << a.hist_bits] = 0u;
  }
  if (which_only < 0) {
    if (unserved) { a.flags[kFlagUnserved] = 1u; }
    if (a.mark_short != nullptr) {
      for (int o = 32; o > 0; o >>= 1) { marked += (uint32_t)__shfl_xor((int)marked, o, 64); }
      if ((threadIdx.x & 63u) == 0u && marked != 0u) { atomicAdd(a.flags + kFlagOverMass, marked); }
    }
    // shortest sequence: one atomic per workgroup, and only if it can still raise the flag (a single address takes
    // ~88 atomics per microsecond: one per wave was 0.1 ms of nothing but that)
    __shared__ uint32_t sh_short[4];
    for (int o = 32; o > 0; o >>= 1) { shortest = min(shortest, (uint32_t)__shfl_xor((int)shortest, o, 64)); }
    if ((threadIdx.x & 63u) == 0u) { sh_short[threadIdx.x >> 6] = shortest; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t s4 = min(min(sh_short[0], sh_short[1]), min(sh_short[2], sh_short[3]));
      if (s4 != 0xFFFFFFFFu && 0xFFFFFFFFu - s4 > a.flags[kFlagShortest]) { atomicMax(a.flags + kFlagShortest, 0xFFFFFFFFu - s4); }
    }
  }
  // the guard: records made, per index (one atomic per workgroup and index)
  {
    __shared__ uint32_t sh_made[2];
    if (threadIdx.x < 2u) { sh_made[threadIdx.x] = 0u; }
    __syncthreads();
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      uint32_t v = made[which];
      for (int o = 32; o > 0; o >>= 1) { v += (uint32_t)__shfl_xor((int)v, o, 64); }
      if ((threadIdx.x & 63u) == 0u && v != 0u) { atomicAdd(&sh_made[which], v); }
    }
    __syncthreads();
    if (threadIdx.x < 2u && sh_made[threadIdx.x] != 0u) { atomicAdd(a.guard + kGuardMade + threadIdx.x, (unsigned long long)sh_made[threadIdx.x]); }
  }
}

// ---- the guard's second opinion on the key records (once per uploaded database) ----------------------------------------
// k_keys derives the records from the amplicon LINES, with the sequence in registers (window_of).  These two kernels say
// the same thing from the PACKED DATABASE, word by word from memory (anchor_key, the function the routing and the window
// sample use), and about what the partition left of the records: wrapped sums of mix64(record) per index — and of
// mix64(fingerprint << 32 | id) for the fingerprints that travel with the prefix index — which must agree.  A key
// computed wrongly, a line that is not its amplicon, a record lost or invented between k_keys and the groups: all show,
// whether or not the victim ends up in a group the pair kernels look at (a wrong key usually makes a singleton, which
// nobody looks at again: the signature of the round-1 anomaly).  out: [0, 1] record sums, [2] fingerprint sum.
struct GuardDbArgs {
  const uint64_t * seqs; const uint64_t * seq_off; const uint32_t * seqlen;
  uint32_t n;
  const uint32_t * list[kMaxIdx]; uint32_t list_count[kMaxIdx];
  const unsigned long long * list_rec[kMaxIdx];   // routed by records: the ids are the records' low halves
  uint32_t owner_rank, owner_world, win_a, win_b, nwin;
  unsigned long long * out;
};
__device__ __forceinline__ void guard_reduce(unsigned long long v, unsigned long long * out) {
  for (int o = 32; o > 0; o >>= 1) { v += swa_shfl_xor_u64(v, o); }
  if ((threadIdx.x & 63u) == 0u && v != 0ull) { atomicAdd(out, v); }
}
__global__ __launch_bounds__(256) void k_guard_db(const GuardDbArgs a) {
  const bool by_rec = a.list_rec[0] != nullptr || a.list_rec[1] != nullptr;
  const int which_only = by_rec || a.list[0] != nullptr || a.list[1] != nullptr ? (int)blockIdx.y : -1;
  const uint32_t total = which_only < 0 ? a.n : a.list_count[which_only];
  unsigned long long sum[2] = {0ull, 0ull};
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const uint32_t i = which_only < 0 ? e : (by_rec ? (uint32_t)a.list_rec[which_only][e] : a.list[which_only][e]);
    const uint32_t len = a.seqlen[i];
    const uint64_t * s = a.seqs + a.seq_off[i];
    for (int which = 0; which < 2; ++which) {
      if (which_only >= 0 && which != which_only) { continue; }
      if (len >= (which == 0 ? a.win_a : a.win_b) + kAnchor * a.nwin) {
        const uint64_t mixed = mix64(anchor_key(s, len, which, a.win_a, a.win_b, a.nwin));
        if (which_only >= 0 || a.owner_world == 1u || anchor_owner(mixed, a.owner_world) == a.owner_rank) {
          sum[which] += mix64(((unsigned long long)record_key(mixed, len) << 32) | i);
        }
      }
    }
  }
  guard_reduce(sum[0], a.out + 0); guard_reduce(sum[1], a.out + 1);
}
// the same sums over the partitioned records of index blockIdx.y (and the fingerprints of index 0): out [0, 1], [2]
struct GuardRecArgs { const unsigned long long * rec[kMaxIdx]; const uint32_t * total[kMaxIdx]; unsigned long long * out; };
__global__ __launch_bounds__(256) void k_guard_records(const GuardRecArgs a) {
  const uint32_t which = blockIdx.y, m = *a.total[which];
  unsigned long long sum = 0ull;
  for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < m; e += gridDim.x * blockDim.x) { sum += mix64(a.rec[which][e]); }
  guard_reduce(sum, a.out + which);
}

// ---- groups of one bucket -----------------------------------------------------------------------------------------
// One workgroup per bucket and index.  The bucket's distinct keys go into an LDS table (slot = key << 32 | members so
// far), an exclusive scan of the counts gives every group its place, a second walk over the records drops every id into
// its group.  Out: the ids in group order (members), per bucket the groups as work items sorted by kind (k_group_lists
// moves them into the lists the pair kernels read), flags; index 0 also looks for identical sequences: two members of a
// prefix group with equal fingerprints are compared word for word.
struct GroupIdx {
  unsigned long long * rec;          // partitioned records (k_group1 keeps rank and slot of a bucket's last records in their key halves)
  const uint64_t * bstart;           // [buckets + 1]
  uint32_t buckets;
  uint32_t * members;                // out: ids in group order, [records]
  unsigned long long * items_tmp;    // out: per bucket, at the bucket's first record: begin | size << 32 (chunk items: | chunk << 48)
  uint32_t * kind_cnt;               // out: [kListsPerIndex][buckets] items of each list (width class x size kind)
};
struct GroupArgs {
  GroupIdx g[kMaxIdx];
  uint32_t pair_big, group_cap;
  uint32_t * flags;                  // the status block's: kFlagKeyOverflow, kFlagOversized, kFlagOverMass
  unsigned long long * guard;        // the status block's: kGuardListed / kGuardSingleton / kGuardOversized + which, kGuardBucketTotal
  uint8_t * over;                    // per amplicon: bit `which` = member of an oversized group of that index
};

// ---- groups of one LARGE bucket ------------------------------------------------------------------------------------------
// k_group1 takes buckets of ~10 000 records — ONE partition level of 10 bits at 10 M — with 1024 threads and 128 KB of
// dynamic LDS per workgroup:
//   tkey[8192]   the distinct keys of the bucket, open addressing (key | 1: a live slot is never 0)
//   tcnt[8192]   per slot: members [0, 16), one bit per width class seen among them [16, 21)
//   (16384 more entries: the groups' first places and the staging area of the members in group order.  Rounds 3-5 also
//   kept a table of 16-bit fingerprint tags there — the search for identical sequences, 0.07 ms of the kernel's 0.28 at
//   10 M; round 6: the prefix pass of the pair kernels sees them on the sequences themselves, d1_anchor.inc pair_twin)
// Round 4, second form.  The kernel is bound by LDS instruction issue, not by HBM (stage by stage, profiles/r04/NOTES.md:
// counting 0.17 ms, identical sequences 0.07, places and work items 0.12, placing 0.055 of 0.46 ms at 10 M): a 64-bit
// LDS atomic over 64 random addresses is >= 4 passes through the 32 banks before conflicts.  So the table is two 32-bit
// arrays, the counting atomic RETURNS the record's rank among its group's members (stage 3 then needs no cursor atomics:
// place = first place of the group + rank), and the per-list counters — ~1000 groups of a bucket on five addresses, which
// the LDS serialises lane by lane — are bumped once per wave and list.
constexpr uint32_t kG1Threads = 1024;
constexpr uint32_t kG1SlotBits = 13, kG1Slots = 1u << kG1SlotBits;      // (a bucket holds ~2200 distinct keys: load ~0.3 — the probe loops run as long as the slowest of 64 lanes)
constexpr uint32_t kG1DupBits = 14, kG1DupSlots = 1u << kG1DupBits;
constexpr uint32_t kG1Target = SWA_G1_TARGET;           // records per bucket the partition aims at (on average, at most)
constexpr size_t kG1LdsBytes = kG1Slots * 4 * 2 + kG1DupSlots * 4;
static_assert(kG1Slots * 4 <= kG1DupSlots * 4, "the groups' places lie in the area behind the two tables");
constexpr uint32_t kG1OverBit = 0x80000000u;     // toff: the group is left to the plain kernel

constexpr uint32_t kG1Per = 8;                    // records per thread held in registers (10 or 12, batches of 2..8 walked together: all slower —
                                                  // the kernel is bound by the instructions it issues, profiles/r04/NOTES.md)
constexpr uint32_t kG1Tail = 2;                   // ... and asked for at the start of a stage, worked on at its end (not kept between stages)

// A count word: [0, 16) the number of members (a bucket holds at most 65 534 records), [16, 21) one bit per width class
// seen among the members (class 0 — the usual one — is not recorded: it is what no bit means).
__device__ __forceinline__ uint32_t g1_size(uint32_t w) { return w & 0xFFFFu; }
__device__ __forceinline__ uint32_t g1_class(uint32_t w) {       // widest class among the members; kTooLong: one is too long
  const uint32_t bits = (w >> 16) & 0x1Fu;
  return bits == 0u ? 0u : 31u - (uint32_t)__clz((int)bits);
}
// a group the pair kernels do not take: more members than they serve, or a member longer than their widest records
// (a singleton has no candidates whatever its length)
__device__ __forceinline__ bool g1_over(uint32_t w, uint32_t cap) { return g1_size(w) > 1u && (g1_size(w) > cap || g1_class(w) >= kTooLong); }
// list of a group: class * kListKinds + size kind, or kListsPerIndex: none (singletons, groups left to the plain kernel)
__device__ __forceinline__ uint32_t g1_list(uint32_t w, uint32_t pair_big, uint32_t cap) {
  const uint32_t g = g1_size(w);
  if (g < 2u || g1_over(w, cap)) { return kListsPerIndex; }
  const uint32_t kind = g <= kSeedsPerItem ? pair_class(g) : (g <= pair_big ? kPairClasses : kPairClasses + 1u);
  return g1_class(w) * kListKinds + kind;
}
// Both tables are LINES of four 32-bit entries: one ds_read_b128 shows a key's whole neighbourhood, so that nearly every
// record is done after one read and one atomic.  (What the kernel pays for is the NUMBER of LDS instructions its waves
// issue — SQ counters, profiles/r04/NOTES.md: the LDS pipeline is busy ~80 % of the kernel, ~14 cycles an instruction
// however few lanes are left in it — and a probe loop over single entries runs for every wave as long as the unluckiest
// of its 256 lane-records needs: six rounds of read / swap / add at load 0.3.)  A line fills from its first entry on and
// entries never change once set; a key lives in the first line from its home line on that was not full when it came.
constexpr uint32_t kG1LineBits = kG1SlotBits - 2u, kG1Lines = 1u << kG1LineBits;
__device__ __forceinline__ uint32_t g1_home_line(uint32_t kk) { return (kk * 0x9E3779B1u) >> (32u - kG1LineBits); }   // (the key's top bits are the bucket's)

// a record into the slot of its key: its rank among the group's members << kG1SlotBits | slot
__device__ __forceinline__ uint32_t g1_enter(uint32_t * tcnt, uint32_t idx, uint32_t cls) {
  const uint32_t old = atomicAdd(&tcnt[idx], 1u);
  if (cls != 0u && (old >> (16u + cls) & 1u) == 0u) { atomicOr(&tcnt[idx], 1u << (16u + cls)); }
  return (old & 0xFFFFu) << kG1SlotBits | idx;
}
__device__ __forceinline__ uint32_t g1_find4(const uint4 & q, uint32_t v) {     // first entry of the line equal to v (4: none)
  return q.x == v ? 0u : q.y == v ? 1u : q.z == v ? 2u : q.w == v ? 3u : 4u;
}

// Counts N keys in, their probe sequences walked together (all reads issued, then all swaps, then all adds: the LDS round
// trips of a thread's records overlap).  valid: bit k = key[k] is to be counted; sr[k] = its rank and slot; returns false
// when the table is full.
template <uint32_t N>
__device__ __forceinline__ bool g1_count_keys(uint32_t * tkey, uint32_t * tcnt, const uint32_t (&key)[N], uint32_t valid, uint32_t (&sr)[N]) {
  uint32_t line[N];
#pragma unroll
  for (uint32_t k = 0; k < N; ++k) { line[k] = g1_home_line(key[k] & ~7u); sr[k] = 0u; }
  uint32_t pend = valid;
  // (a round either enters a record, moves it one line on, or loses a swap against an entry that is set from then on)
  for (uint32_t rounds = 0; pend != 0u; ++rounds) {
    if (rounds > kG1Slots + kG1Lines) { return false; }
    uint4 q[N];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) { if ((pend >> k & 1u) != 0u) { q[k] = *reinterpret_cast<const uint4 *>(tkey + 4u * line[k]); } }
    uint32_t at[N];
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
      at[k] = 4u;
      if ((pend >> k & 1u) == 0u) { continue; }
      const uint32_t want = (key[k] & ~7u) | 1u;
      at[k] = g1_find4(q[k], want);
      if (at[k] == 4u) {
        const uint32_t e = g1_find4(q[k], 0u);
        if (e == 4u) {
          line[k] = (line[k] + 1u) & (kG1Lines - 1u);                       // a full line without the key
        } else {
          const uint32_t old = atomicCAS(&tkey[4u * line[k] + e], 0u, want);
          if (old == 0u || old == want) { at[k] = e; }                       // (else: another key came first — the line again)
        }
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < N; ++k) {
      if ((pend >> k & 1u) != 0u && at[k] < 4u) { sr[k] = g1_enter(tcnt, 4u * line[k] + at[k], key[k] & 7u); pend &= ~(1u << k); }
    }
  }
  return true;
}

// a record whose rank and slot stage 1 found into its group: first place of the group + rank.  STAGED: the bucket's members
// are put in order in LDS and leave in whole lines (10 000 stores of 4 bytes to 10 000 places of a 40 KB region are 64 cache
// lines an instruction); buckets larger than the staging area go straight to memory.
constexpr uint32_t kG1Staged = kG1Slots + (kG1DupSlots - kG1Slots);
template <bool STAGED>
__device__ __forceinline__ void g1_place(const GroupArgs & a, const GroupIdx & g, const uint32_t * toff, uint32_t * staged, uint64_t start, uint32_t id, uint32_t sr, uint32_t which) {
  const uint32_t t = toff[sr & (kG1Slots - 1u)];
  const uint32_t at = (t & ~kG1OverBit) + (sr >> kG1SlotBits);
  if (STAGED) { staged[at] = id; } else { g.members[start + at] = id; }
  if ((t & kG1OverBit) != 0u) { atomicOr(reinterpret_cast<unsigned int *>(a.over + (id & ~3u)), (1u << which) << (8u * (id & 3u))); }
}

__device__ __forceinline__ uint32_t lanes_below(unsigned long long mask) {      // set bits of `mask` below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ONE attempt at a key, no loop: the home line holds the key or has room for it (~98 % of the records at load 0.3).  The
// kernel is bound by the instructions its waves issue, and a loop runs for a whole wave as long as its unluckiest lane
// needs — so the usual case is straight-line code and the rest is collected and looped over once (k_group1, stage 1).
__device__ __forceinline__ bool g1_count_once(uint32_t * tkey, uint32_t * tcnt, uint32_t key, uint32_t & sr) {
  const uint32_t want = (key & ~7u) | 1u, first = 4u * g1_home_line(key & ~7u);
  const uint4 q = *reinterpret_cast<const uint4 *>(tkey + first);
  uint32_t at = g1_find4(q, want);
  if (at == 4u) {
    const uint32_t e = g1_find4(q, 0u);
    if (e < 4u) {
      const uint32_t old = atomicCAS(&tkey[first + e], 0u, want);
      if (old == 0u || old == want) { at = e; }
    }
  }
  if (at == 4u) { return false; }
  sr = g1_enter(tcnt, first + at, key & 7u);
  return true;
}
// exclusive scan of a 64-bit value over the 1024 threads of a workgroup
__device__ __forceinline__ unsigned long long block_exclusive_scan64_1024(unsigned long long v, unsigned long long * smem16, unsigned long long & total, uint32_t tid) {
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = (unsigned long long)(uint32_t)__shfl_up((int)(uint32_t)incl, (unsigned)d, 64)
                                | (unsigned long long)(uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), (unsigned)d, 64) << 32;
    if ((int)lane >= d) { incl += up; }
  }
  if (lane == 63u) { smem16[wave] = incl; }
  __syncthreads();
  // (the sixteen wave sums: lane w of every wave reads one and the wave scans them — not sixteen reads a thread)
  unsigned long long x = lane < 16u ? smem16[lane] : 0ull;
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) {
    const unsigned long long up = (unsigned long long)(uint32_t)__shfl_up((int)(uint32_t)x, (unsigned)d, 64)
                                | (unsigned long long)(uint32_t)__shfl_up((int)(uint32_t)(x >> 32), (unsigned)d, 64) << 32;
    if ((int)lane >= d) { x += up; }
  }
  const unsigned long long tot = lane_value64(x, 15);
  const unsigned long long before = wave == 0u ? 0ull : lane_value64(x, (int)wave - 1);
  __syncthreads();
  total = tot;
  return before + incl - v;
}

__global__ __launch_bounds__(kG1Threads) void k_group1(const GroupArgs a) {
  extern __shared__ uint32_t g1_lds[];
  uint32_t * tcnt = g1_lds;                                                 // [kG1Slots] members, class bits
  uint32_t * tkey = tcnt + kG1Slots;                                        // [kG1Slots] key | 1
  uint32_t * toff = tkey + kG1Slots + (kG1DupSlots - kG1Slots);             // [kG1Slots] first place of the group | kG1OverBit (step 2 on)
  uint32_t * staged = tkey;                                                 // [kG1Staged] step 3: the members in group order, over the keys and
                                                                            // the area behind them up to the places
  __shared__ uint32_t kcnt[kListsPerIndex], kbase[kListsPerIndex];
  __shared__ unsigned long long smem16[16];
  __shared__ uint32_t sh_fail;
  __shared__ uint32_t gsum[3];                                  // the guard: members of all / singleton / oversized groups of the bucket
  uint32_t * glist = tkey;                                                  // [<= kG1Slots] the slots of the listed groups (step 2 on: the keys are done with)
  const uint32_t which = blockIdx.y;
  const GroupIdx & g = a.g[which];
  if (threadIdx.x < 3u) { gsum[threadIdx.x] = 0u; }
  for (uint32_t b = blockIdx.x; b < g.buckets; b += gridDim.x) {
    // (the thread's number as something the compiler takes for new in every round: what it derives from it — record numbers,
    // table addresses, the scan's sixteen wave comparisons — would otherwise be kept from before the loop on, and spill)
    uint32_t tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const uint32_t lane = tid & 63u;
    const uint64_t start = g.bstart[b];
    const uint32_t c = (uint32_t)(g.bstart[b + 1] - start);
    if (c == 0u) {
      if (tid < kListsPerIndex) { g.kind_cnt[tid * g.buckets + b] = 0u; }
      continue;
    }
    // A bucket beyond 16-bit ranks and record numbers (one enormous group — 10^5 amplicons behind one 64-nt window happen in
    // real sets — or many large ones behind one key prefix): every member is left to the plain kernel, as the members of an
    // oversized group are; its table finds identical sequences as well.  Nothing is grouped, nothing listed.
    if (c > 0xFFFEu) {
      for (uint32_t r = tid; r < c; r += kG1Threads) {
        const uint32_t id = (uint32_t)g.rec[start + r];
        g.members[start + r] = id;
        atomicOr(reinterpret_cast<unsigned int *>(a.over + (id & ~3u)), (1u << which) << (8u * (id & 3u)));
      }
      if (tid < kListsPerIndex) { g.kind_cnt[tid * g.buckets + b] = 0u; }
      if (tid == 0) { atomicOr(a.flags + kFlagOversized, 1u); atomicAdd(a.flags + kFlagOverMass, c); atomicAdd(a.guard + kGuardOversized + which, (unsigned long long)c); }
      continue;
    }
    const uint32_t cap = a.group_cap;
    // the bucket's records into registers: every load in flight at once, read once for all three stages
    uint32_t rkey[kG1Per], rid[kG1Per];                         // (key, then — stage 1 on — rank and slot; id)
    uint32_t here = 0u;                                         // bit k: the thread's k-th record exists (k < kG1Per + kG1Tail)
#pragma unroll
    for (uint32_t k = 0; k < kG1Per + kG1Tail; ++k) { here |= (k * kG1Threads + tid < c ? 1u : 0u) << k; }
#pragma unroll
    for (uint32_t k = 0; k < kG1Per; ++k) {
      const uint32_t r = k * kG1Threads + tid;
      const unsigned long long rec = (here >> k & 1u) != 0u ? g.rec[start + r] : 0ull;
      rkey[k] = (uint32_t)(rec >> 32); rid[k] = (uint32_t)rec;
    }
    {
      uint4 * t4 = reinterpret_cast<uint4 *>(tcnt);
      for (uint32_t i = tid; i < (2u * kG1Slots) / 4u; i += kG1Threads) { t4[i] = make_uint4(0u, 0u, 0u, 0u); }      // (tcnt and tkey)
    }
    if (tid < kListsPerIndex) { kcnt[tid] = 0u; }
    if (tid == 0) { sh_fail = 0u; }
    __syncthreads();
    // ---- 1. distinct keys, their counts, every record's rank in its group
    {
      bool ok = true;
      uint32_t left = 0u;                                       // records of this thread the one attempt did not enter
      // (the next kG1Tail records of the thread — the usual bucket is a little larger than the registers — are asked for now
      // and worked on after the others: their way from memory is not waited for)
      unsigned long long trec[kG1Tail];
#pragma unroll
      for (uint32_t t = 0; t < kG1Tail; ++t) {
        const uint32_t r = (kG1Per + t) * kG1Threads + tid;
        trec[t] = (here >> (kG1Per + t) & 1u) != 0u ? g.rec[start + r] : 0ull;
      }
#pragma unroll
      for (uint32_t k = 0; k < kG1Per; ++k) {
        if ((here >> k & 1u) != 0u && !g1_count_once(tkey, tcnt, rkey[k], rkey[k])) { left |= 1u << k; }
        __builtin_amdgcn_sched_barrier(0);                      // (one record after the other: eight reads of 16 bytes hoisted to the front spill)
      }
#pragma unroll
      for (uint32_t t = 0; t < kG1Tail; ++t) {
        if ((here >> (kG1Per + t) & 1u) != 0u) {
          const uint32_t r = (kG1Per + t) * kG1Threads + tid;
          const uint32_t key[1] = {(uint32_t)(trec[t] >> 32)};
          uint32_t sr[1];
          if (!g1_count_once(tkey, tcnt, key[0], sr[0])) { ok = g1_count_keys<1>(tkey, tcnt, key, 1u, sr) && ok; }
          g.rec[start + r] = (unsigned long long)sr[0] << 32 | (uint32_t)trec[t];
        }
      }
      while (left != 0u) {                                      // (the key out of and the result into the registers by constant indices)
        const uint32_t k = (uint32_t)__ffs((int)left) - 1u;
        left &= left - 1u;
        uint32_t key[1] = {0u}, sr[1];
#pragma unroll
        for (uint32_t j = 0; j < kG1Per; ++j) { key[0] = j == k ? rkey[j] : key[0]; }
        ok = g1_count_keys<1>(tkey, tcnt, key, 1u, sr) && ok;
#pragma unroll
        for (uint32_t j = 0; j < kG1Per; ++j) { rkey[j] = j == k ? sr[0] : rkey[j]; }
      }
      // (records beyond the registers: rank and slot go back into the key half of the record, which no one needs again)
      for (uint32_t r = (kG1Per + kG1Tail) * kG1Threads + tid; r < c; r += kG1Threads) {
        const unsigned long long rec = g.rec[start + r];
        const uint32_t key[1] = {(uint32_t)(rec >> 32)};
        uint32_t sr[1];
        ok = g1_count_keys<1>(tkey, tcnt, key, 1u, sr) && ok;
        g.rec[start + r] = (unsigned long long)sr[0] << 32 | (uint32_t)rec;
      }
      if (!ok) { sh_fail = 1u; }
    }
    __syncthreads();                                            // (every count is in)
    if (sh_fail != 0u) {                                        // more distinct keys than slots: the host partitions finer
      if (tid == 0) { a.flags[kFlagKeyOverflow] = 1u; }
      if (tid < kListsPerIndex) { g.kind_cnt[tid * g.buckets + b] = 0u; }
      __syncthreads();
      continue;
    }
    // ---- 2. places of the groups (slot order); the listed groups' slots side by side, so that what follows — their kinds,
    // their work items — is one dense pass of ~1000 lanes, not eight sparse ones over the table
    uint32_t n_listed;
    {
      constexpr uint32_t kPer = kG1Slots / kG1Threads;
      static_assert(kPer == 8u, "two 16-byte reads per thread");
      uint32_t slot[kPer];
      {
        const uint4 lo = *reinterpret_cast<const uint4 *>(tcnt + tid * kPer), hi = *reinterpret_cast<const uint4 *>(tcnt + tid * kPer + 4u);
        slot[0] = lo.x; slot[1] = lo.y; slot[2] = lo.z; slot[3] = lo.w; slot[4] = hi.x; slot[5] = hi.y; slot[6] = hi.z; slot[7] = hi.w;
      }
      // one scan sums three things: members [0, 17), singleton groups [17, 32), listed groups [32, 48)
      unsigned long long s = 0;
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t sz = g1_size(slot[k]);
        s += (unsigned long long)(sz + (sz == 1u ? 1u << 17 : 0u)) | (unsigned long long)(sz >= 2u && !g1_over(slot[k], cap) ? 1u : 0u) << 32;
      }
      unsigned long long total;
      const unsigned long long before = block_exclusive_scan64_1024(s, smem16, total, tid);
      uint32_t run = (uint32_t)before & 0x1FFFFu, lrun = (uint32_t)(before >> 32);
      uint32_t mass = 0;
      uint32_t off[kPer];
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t sz = g1_size(slot[k]);
        const bool over = g1_over(slot[k], cap);
        off[k] = run | (over ? kG1OverBit : 0u);
        run += sz;
        if (sz >= 2u && !over) { glist[lrun++] = tid * kPer + k; }
        if (over) { mass += sz; }
      }
      *reinterpret_cast<uint4 *>(toff + tid * kPer) = make_uint4(off[0], off[1], off[2], off[3]);
      *reinterpret_cast<uint4 *>(toff + tid * kPer + 4u) = make_uint4(off[4], off[5], off[6], off[7]);
      if (mass != 0u) { atomicOr(a.flags + kFlagOversized, 1u); atomicAdd(a.flags + kFlagOverMass, mass); atomicAdd(&gsum[2], mass); }
      // the guard: what became of the bucket's records — members of singleton groups, of groups left to the plain kernel, the rest listed
      n_listed = (uint32_t)(total >> 32);
      if (tid == 0) {
        gsum[0] = (uint32_t)total & 0x1FFFFu; gsum[1] = ((uint32_t)total >> 17) & 0x7FFFu;
        if (((uint32_t)total & 0x1FFFFu) != c) { atomicAdd(a.guard + kGuardBucketTotal, 1ull); }   // (never read: swa_internal.h)
      }
    }
    __syncthreads();
    // (how many items each list gets: one atomic per wave and list — a thousand groups of a bucket share five counters)
    for (uint32_t i0 = 0; i0 < n_listed; i0 += kG1Threads) {
      const uint32_t i = i0 + tid;
      const uint32_t w = i < n_listed ? tcnt[glist[i]] : 0u;
      const uint32_t list = i < n_listed ? g1_list(w, a.pair_big, cap) : kListsPerIndex;
      unsigned long long todo = __ballot(list < kListsPerIndex);
      while (todo != 0ull) {
        const uint32_t l = lane_value(list, __ffsll((long long)todo) - 1);
        const unsigned long long same = __ballot(list == l);
        if (l % kListKinds == kPairClasses + 1u) {
          if (list == l) { atomicAdd(&kcnt[l], tiled_item_count(g1_size(w))); }
        } else if (lane == (uint32_t)(__ffsll((long long)same) - 1)) {
          atomicAdd(&kcnt[l], (uint32_t)__popcll(same));
        }
        todo &= ~same;
      }
    }
    __syncthreads();
    if (tid < 64u) {                                    // (each list's first place: the items of the lists before it — wave 0 scans the counts)
      const uint32_t mine = tid < kListsPerIndex ? kcnt[tid] : 0u;
      uint32_t incl = mine;
#pragma unroll
      for (int d = 1; d < 32; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, (unsigned)d, 64); if ((int)lane >= d) { incl += up; } }
      if (tid < kListsPerIndex) { kbase[tid] = incl - mine; g.kind_cnt[tid * g.buckets + b] = mine; kcnt[tid] = 0u; }
    }
    if (tid >= 64u && tid < 67u) {
      const uint32_t j = tid - 64u;
      const uint32_t sum = j == 0u ? gsum[0] - gsum[1] - gsum[2] : gsum[j];
      if (sum != 0u) { atomicAdd(a.guard + kGuardListed + 2u * j + which, (unsigned long long)sum); }   // (j: listed, singleton, oversized)
    }
    __syncthreads();
    if (tid == 64u) { gsum[2] = 0u; }
    for (uint32_t i0 = 0; i0 < n_listed; i0 += kG1Threads) {
      const uint32_t i = i0 + tid;
      const uint32_t sl = i < n_listed ? glist[i] : 0u;
      const uint32_t w = i < n_listed ? tcnt[sl] : 0u;
      const uint32_t sz = g1_size(w);
      const uint32_t list = i < n_listed ? g1_list(w, a.pair_big, cap) : kListsPerIndex;
      const unsigned long long item = (unsigned long long)(uint32_t)(start + (toff[sl] & ~kG1OverBit)) | ((unsigned long long)sz << 32);
      unsigned long long todo = __ballot(list < kListsPerIndex);
      while (todo != 0ull) {
        const uint32_t l = lane_value(list, __ffsll((long long)todo) - 1);
        const unsigned long long same = __ballot(list == l);
        if (l % kListKinds == kPairClasses + 1u) {
          if (list == l) {
            // (row tile by row tile, each against its column tiles kTiledCols at a time: chunk = row tile | part << 6)
            const uint32_t tiles = (sz + kSeedsPerItem - 1u) / kSeedsPerItem;
            uint32_t at = kbase[l] + atomicAdd(&kcnt[l], tiled_item_count(sz));
            for (uint32_t r2 = 0; r2 < tiles; ++r2) {
              const uint32_t parts = (tiles - r2 + kTiledCols - 1u) / kTiledCols;
              for (uint32_t q = 0; q < parts; ++q) { g.items_tmp[start + at++] = item | ((unsigned long long)(r2 | (q << 6)) << 48); }
            }
          }
        } else {
          const int first = __ffsll((long long)same) - 1;
          uint32_t at = 0;
          if ((int)lane == first) { at = atomicAdd(&kcnt[l], (uint32_t)__popcll(same)); }
          at = lane_value(at, first);
          if (list == l) { g.items_tmp[start + kbase[l] + at + lanes_below(same)] = item; }
        }
        todo &= ~same;
      }
    }
    // ---- 3. every record into its group
    auto place_all = [&](auto staged_c) {
      constexpr bool STAGED = decltype(staged_c)::value;
      unsigned long long trec[kG1Tail];
#pragma unroll
      for (uint32_t t = 0; t < kG1Tail; ++t) {
        const uint32_t r = (kG1Per + t) * kG1Threads + tid;
        trec[t] = (here >> (kG1Per + t) & 1u) != 0u ? g.rec[start + r] : 0ull;
      }
#pragma unroll
      for (uint32_t k = 0; k < kG1Per; ++k) {
        if ((here >> k & 1u) != 0u) { g1_place<STAGED>(a, g, toff, staged, start, rid[k], rkey[k], which); }
      }
#pragma unroll
      for (uint32_t t = 0; t < kG1Tail; ++t) {
        if ((here >> (kG1Per + t) & 1u) != 0u) { g1_place<STAGED>(a, g, toff, staged, start, (uint32_t)trec[t], (uint32_t)(trec[t] >> 32), which); }
      }
      for (uint32_t r = (kG1Per + kG1Tail) * kG1Threads + tid; r < c; r += kG1Threads) {
        const unsigned long long rec = g.rec[start + r];
        g1_place<STAGED>(a, g, toff, staged, start, (uint32_t)rec, (uint32_t)(rec >> 32), which);
      }
    };
    if (c <= kG1Staged) {
      __syncthreads();                                          // (the listed groups' slots lie where the members are staged)
      place_all(std::true_type{});
      __syncthreads();
      for (uint32_t i = tid; i < c; i += kG1Threads) { g.members[start + i] = staged[i]; }
    } else {
      place_all(std::false_type{});
    }
    __syncthreads();
  }
}

// ---- work lists ----------------------------------------------------------------------------------------------------
// kind_cnt (list-major: entry [l][b] = items of list l in bucket b) -> every bucket's items into the lists the pair kernels
// read (PairLists: one region per width class and size kind), the lists' lengths into their counters.  One wave per bucket.
// Where a bucket's items go in list l is the number of items of that list in the buckets before it.  Two forms
// (swa_lists_inline: by the number of buckets alone):
//   INLINE   up to 1024 buckets: every workgroup adds up, list by list, the counts of the buckets before its own — at most
//            28 x 1024 values out of L2, and only the lists of width classes the database has —, and the wave of the last
//            bucket, which then knows the lists' lengths, writes the counters.  No launch but this one.
//   else     kind_cnt arrives scanned in place by k_flat_sums / k_flat_apply (entry [l][b] = items of all lists < l plus
//            those of list l in buckets < b, + a closing entry), two launches more.
struct ListIdx {
  const unsigned long long * items_tmp;
  const uint64_t * bstart;
  const uint32_t * kind_pos;         // kind_cnt [kListsPerIndex][buckets]: as k_group1 left it (INLINE), or scanned + closing entry
  uint32_t buckets;
  uint32_t list_mask;                // (INLINE) bit l: list l may hold items (its width class has sequences)
  PairLists l;
};
struct ListArgs { ListIdx x[kMaxIdx]; };
static_assert(kListsPerIndex <= 32u, "k_group_lists: a bit per list");

template <bool INLINE>
__global__ __launch_bounds__(256) void k_group_lists(const ListArgs a) {
  const ListIdx & x = a.x[blockIdx.y];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t nwaves = gridDim.x * 4u;
  const uint64_t entries = (uint64_t)kListsPerIndex * x.buckets;
  // (INLINE) lbase[l]: items of list l in the buckets before the workgroup's first bucket of this round
  __shared__ uint32_t lbase[kListsPerIndex], wsum[4][kListsPerIndex];
  uint32_t summed = 0;                                          // (INLINE) lbase covers the buckets [0, summed)
  if (INLINE && threadIdx.x < kListsPerIndex) { lbase[threadIdx.x] = 0u; }
  // (b0: the same for the whole workgroup, so that its barriers are met by every wave)
  for (uint32_t b0 = blockIdx.x * 4u; b0 < x.buckets; b0 += nwaves) {
    const uint32_t b = b0 + wave;
    if constexpr (INLINE) {
#pragma unroll 1
      for (uint32_t l = 0; l < kListsPerIndex; ++l) {
        if ((x.list_mask >> l & 1u) == 0u) { continue; }
        uint32_t part = 0;
        for (uint32_t q = summed + threadIdx.x; q < b0; q += 256u) { part += x.kind_pos[(uint64_t)l * x.buckets + q]; }
        for (int o = 32; o > 0; o >>= 1) { part += (uint32_t)__shfl_xor((int)part, o, 64); }
        if (lane == 0u) { wsum[wave][l] = part; }
      }
      __syncthreads();
      if (threadIdx.x < kListsPerIndex && (x.list_mask >> threadIdx.x & 1u) != 0u) {
        lbase[threadIdx.x] += wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
      }
      __syncthreads();
      summed = b0;
    }
    if (b >= x.buckets) { continue; }
    const uint64_t start = x.bstart[b];
    // lane l < kListsPerIndex: where in list l this bucket's items go and how many they are (all loads at once, not one list
    // after the other: 28 dependent round trips per bucket were 0.05 ms of the step)
    uint32_t my_at = 0, my_cnt = 0;
    if (lane < kListsPerIndex) {
      const uint64_t e = (uint64_t)lane * x.buckets + b;
      if constexpr (INLINE) {
        my_cnt = x.kind_pos[e];
        my_at = lbase[lane];
        for (uint32_t w = 0; w < wave; ++w) { my_at += x.kind_pos[(uint64_t)lane * x.buckets + b0 + w]; }
      } else {
        const uint32_t my_pos = x.kind_pos[e];
        my_cnt = x.kind_pos[e + 1] - my_pos;                                     // (e + 1 <= entries: the closing entry)
        my_at = my_pos - x.kind_pos[(uint64_t)lane * x.buckets];
      }
    }
    uint32_t local = 0;
    unsigned long long todo = __ballot(my_cnt != 0u);
    while (todo != 0ull) {
      const int l = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      // (lists before l that are empty add nothing to `local`: the items of a bucket lie list after list)
      const uint32_t cnt = lane_value(my_cnt, l), at = lane_value(my_at, l);
      const uint64_t base = x.l.region.at[(uint32_t)l / kListKinds][(uint32_t)l % kListKinds];
      const uint64_t room = x.l.region.at[(uint32_t)l / kListKinds][(uint32_t)l % kListKinds + 1u] - base;
      for (uint32_t j = lane; j < cnt; j += 64u) {
        const unsigned long long it = x.items_tmp[start + local + j];
        swa_item item;
        item.begin = (uint32_t)it; item.size = (uint32_t)(it >> 32) & 0xFFFFu; item.chunk = (uint32_t)(it >> 48);
        if ((uint64_t)at + j < room) { x.l.items[base + at + j] = item; }    // (the regions hold every possible list: list_regions)
      }
      local += cnt;
    }
    // (never more items than the list's region holds: the copy above drops what does not fit, the guard's member
    // counts then fail to balance and the step ends in SWA_E_INTERNAL instead of a kernel reading its neighbour's list)
    if (INLINE && b + 1u == x.buckets && lane < kListsPerIndex) {             // (the last bucket: what lies before it + its own)
      const uint32_t l = lane;
      const uint64_t room = x.l.region.at[l / kListKinds][l % kListKinds + 1u] - x.l.region.at[l / kListKinds][l % kListKinds];
      x.l.counters[(l / kListKinds) * 8u + l % kListKinds] = (uint32_t)min((uint64_t)(my_at + my_cnt), room);
    }
  }
  if (!INLINE && blockIdx.x == 0 && threadIdx.x < kListsPerIndex) {
    const uint32_t l = threadIdx.x;
    const uint32_t len = x.kind_pos[l + 1u < kListsPerIndex ? (uint64_t)(l + 1u) * x.buckets : entries] - x.kind_pos[(uint64_t)l * x.buckets];
    const uint64_t room = x.l.region.at[l / kListKinds][l % kListKinds + 1u] - x.l.region.at[l / kListKinds][l % kListKinds];
    x.l.counters[(l / kListKinds) * 8u + l % kListKinds] = (uint32_t)min((uint64_t)len, room);
  }
}

// seeds the anchored passes cannot serve, from the per-amplicon bits of k_group1 (members of groups left to the plain
// kernel: oversized, or with a sequence too long for the pair kernels) and the sequences themselves (too short)
__global__ __launch_bounds__(256) void k_stream_fallback(const uint32_t * __restrict__ seqlen, uint32_t first, uint32_t count,
                                                         const uint8_t * __restrict__ over, swa_fallback * list, uint32_t * list_counter,
                                                         uint32_t owner_rank, uint32_t owner_world, const uint64_t * __restrict__ seqs,
                                                         const uint64_t * __restrict__ seq_off, uint32_t minlen) {
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
    const uint32_t seed = first + k;
    const bool plain = seqlen[seed] < minlen;                  // (too short for two windows: every position, against the table)
    if (plain) {
      if (owner_world == 1u || seed % owner_world == owner_rank) { list[atomicAdd(list_counter, 1u)] = swa_fallback{seed, 0u}; }
      continue;
    }
    const uint32_t bits = over[seed];
    if ((bits & 1u) != 0u) { list[atomicAdd(list_counter, 1u)] = swa_fallback{seed, 1u}; }
    if ((bits & 2u) != 0u) { list[atomicAdd(list_counter, 1u)] = swa_fallback{seed, 2u}; }
  }
}
