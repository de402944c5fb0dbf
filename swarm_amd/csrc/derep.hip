// derep.hip — d = 0: dereplication on the GPU.
//
// The reference walks the amplicons in db order and, for each, finds the bucket of the
// identical sequence in an open-addressing table keyed by the Zobrist hash, comparing the
// packed sequences on a hash match (src/derep.cc:276-354).  What the clustering needs from
// that loop is, per amplicon, the FIRST amplicon (smallest db index) with the identical
// sequence; cluster order, mass and the member chains follow from it on the host.
//
// Here every amplicon claims the table slot of its key with one atomicCAS (identical
// sequences share a key, hence a slot — a sequence with 10^6 copies costs 10^6 atomics on one
// slot, not a 10^6-long probe chain), the slot keeps the minimum claimant index, and a second
// kernel verifies each amplicon against its slot's minimum.  Two different sequences with the
// same 64-bit key (astronomically rare; forced in the tests with a narrowed key) share a slot:
// the group that does not own the minimum fails verification and goes round again with a
// re-mixed key until nobody is left.
#include "swa_internal.h"

#include <rocprim/rocprim.hpp>

#include <algorithm>

namespace {

// key of hash h in round `round`: the hash itself first, a splitmix64 re-mix of it afterwards.
// keybits = 64 in production; the tests narrow it (6 more bits every round, so the rounds end)
__device__ __forceinline__ uint64_t derep_key(uint64_t h, uint32_t keybits, uint32_t round) {
  uint64_t k = h;
  if (round != 0) {
    k += 0x9E3779B97F4A7C15ull * round;
    k = (k ^ (k >> 30)) * 0xBF58476D1CE4E5B9ull;
    k = (k ^ (k >> 27)) * 0x94D049BB133111EBull;
    k ^= k >> 31;
  }
  const uint32_t bits = keybits + 6u * round;
  if (bits < 64u) { k &= (1ull << bits) - 1ull; }
  return k == 0 ? 1ull : k;                          // 0 marks a free slot
}

__global__ __launch_bounds__(256) void k_derep_claim(const uint64_t * __restrict__ seqhash,
                                                     const uint32_t * __restrict__ list, uint32_t count,
                                                     uint32_t keybits, uint32_t round, unsigned long long * keys,
                                                     uint32_t * rep, uint64_t tmask, uint32_t * slot_of) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
    const uint32_t i = list != nullptr ? list[t] : t;
    const uint64_t key = derep_key(seqhash[i], keybits, round);
    uint64_t idx = (key ^ (key >> 32)) & tmask;
    for (;;) {
      const unsigned long long old = atomicCAS(&keys[idx], 0ull, (unsigned long long)key);
      if (old == 0ull || old == key) { break; }
      idx = (idx + 1) & tmask;
    }
    atomicMin(&rep[idx], i);
    slot_of[i] = (uint32_t)idx;
  }
}

__global__ __launch_bounds__(256) void k_derep_resolve(const uint64_t * __restrict__ seqs,
                                                       const uint64_t * __restrict__ seq_off,
                                                       const uint32_t * __restrict__ seqlen,
                                                       const uint32_t * __restrict__ list, uint32_t count,
                                                       const uint32_t * __restrict__ rep,
                                                       const uint32_t * __restrict__ slot_of, uint32_t * first_identical,
                                                       uint32_t * next_list, uint32_t * next_count) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
    const uint32_t i = list != nullptr ? list[t] : t;
    const uint32_t r = rep[slot_of[i]];
    bool same = r == i;
    if (!same && seqlen[r] == seqlen[i]) {
      const uint64_t * x = seqs + seq_off[i];
      const uint64_t * y = seqs + seq_off[r];
      same = true;
      for (uint32_t w = 0; w < ((seqlen[i] + 31u) >> 5); ++w) { same = same && (x[w] == y[w]); }
    }
    if (same) { first_identical[i] = r; }
    else { next_list[atomicAdd(next_count, 1u)] = i; }
  }
}

// ---- several GPUs: the reads of a rank's slice travel to the rank that owns their hash -----------------------------------
// (swa_multi_derep_resident, multi.hip.)  Rank r hashes the slice [n r / world, n (r + 1) / world) only — k_derep_hash_slice,
// the hash stream of k_seqhash without the XOR streams and the anchor metadata that only d = 1 reads —, and
// k_derep_route<false / true> groups the (hash, id) records by owner in the count-then-place form of k_links_split
// (d1_part.hip).  The owner is a function of the full 64-bit hash, re-mixed so that it shares no bits with the slot
// k_derep_claim takes from it and never changes with the round: all copies of a sequence meet on one rank in every round.

// fmix64 of MurmurHash3, then the high word of the product with world: [0, world) without a division
__host__ __device__ __forceinline__ uint32_t derep_owner(uint64_t h, uint32_t world) {
  h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
#ifdef __HIP_DEVICE_COMPILE__
  return (uint32_t)__umul64hi(h, (uint64_t)world);
#else
  return (uint32_t)(((unsigned __int128)h * world) >> 64);
#endif
}

template <bool ZLDS>
__global__ __launch_bounds__(256) void k_derep_hash_slice(const uint64_t * __restrict__ seqs, const uint64_t * __restrict__ seq_off,
                                                          const uint32_t * __restrict__ seqlen, const uint64_t * __restrict__ zobrist,
                                                          uint32_t zlen, uint32_t first, uint32_t count, uint64_t * __restrict__ out) {
  extern __shared__ uint64_t lds[];
  const uint64_t * zob = zobrist;
  if (ZLDS) {
    for (uint32_t i = threadIdx.x; i < 4u * zlen; i += blockDim.x) { lds[i] = zobrist[i]; }
    __syncthreads();
    zob = lds;
  }
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
    const uint64_t * s = seqs + seq_off[first + k];
    const uint32_t len = seqlen[first + k];
    uint64_t h = 0, word = 0;
    for (uint32_t p = 0; p < len; ++p) {
      if ((p & 31u) == 0u) { word = s[p >> 5]; }
      h ^= zob[4u * p + (uint32_t)(word & 3u)];
      word >>= 2;
    }
    out[k] = h;
  }
}

// Record k of the slice is (hash[k], first + k).  Two launches over tiles of 2048 records, a lane reading two hashes at a
// time (16 bytes; `hash` is 16-byte aligned):
//   <false>  counts: a histogram per workgroup in LDS over all its tiles, then ONE global atomic per destination it met;
//   <true>   places: every workgroup turns the counts into the runs' first places (a scan over at most 64 values by one
//            wave), and per tile: the histogram in LDS, whose atomic returns the record's rank among the tile's records
//            for its owner, one global atomic per owner the tile met to reserve room in that run, the tile's records put
//            in owner order in LDS and written as one contiguous piece per owner — hashes to out_hash, ids to out_id, at
//            the same position.
// The runs are exactly as long as the counts say: a read with 10^6 copies sends 10^6 records to one owner, and nothing
// overflows.  The order inside a run depends on scheduling; what the owner makes of it, a minimum, does not.
constexpr uint32_t kDerepMaxWorld = 64, kRouteTile = 2048, kRouteThreads = 256;
constexpr uint32_t kRoutePairs = kRouteTile / (2u * kRouteThreads);
struct RouteArgs {
  const unsigned long long * hash;
  uint32_t first, count, world;
  uint32_t * counts;                 // [world] records per owner
  uint32_t * cursor;                 // [world] (places) records of every run that have their place so far
  unsigned long long * out_hash;     // [count]
  uint32_t * out_id;                 // [count]
};

template <bool PLACE>
__global__ __launch_bounds__(kRouteThreads) void k_derep_route(const RouteArgs a) {
  __shared__ uint32_t hist[kDerepMaxWorld], lstart[kDerepMaxWorld], gbase[kDerepMaxWorld];
  __shared__ uint32_t present;
  __shared__ __attribute__((aligned(16))) unsigned long long stage_h[PLACE ? kRouteTile : 1];
  __shared__ uint32_t stage_i[PLACE ? kRouteTile : 1];
  const uint32_t tid = threadIdx.x, world = a.world;
  if (tid < kDerepMaxWorld) { hist[tid] = 0u; }
  // (places) first place of run `tid`: the counts before it — lane d of the first wave keeps it
  uint32_t run_start = 0u;
  if (PLACE && tid < 64u) {
    const uint32_t mine = tid < world ? a.counts[tid] : 0u;
    uint32_t incl = mine;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64); if (tid >= d) { incl += up; } }
    run_start = incl - mine;
  }
  __syncthreads();
  const uint64_t tiles = ((uint64_t)a.count + kRouteTile - 1u) / kRouteTile;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    unsigned long long rec[2u * kRoutePairs];
    uint32_t valid = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kRoutePairs; ++k) {
      const uint64_t j = t * kRouteTile + (uint64_t)k * (2u * kRouteThreads) + 2u * tid;
      const bool v0 = j < a.count, v1 = j + 1u < a.count;
      rec[2u * k] = rec[2u * k + 1u] = 0ull;
      if (v1) {
        const uint4 q = *reinterpret_cast<const uint4 *>(a.hash + j);
        rec[2u * k] = (unsigned long long)q.x | (unsigned long long)q.y << 32;
        rec[2u * k + 1u] = (unsigned long long)q.z | (unsigned long long)q.w << 32;
      } else if (v0) { rec[2u * k] = a.hash[j]; }
      valid |= (v0 ? 1u : 0u) << (2u * k) | (v1 ? 1u : 0u) << (2u * k + 1u);
    }
    uint32_t pos[2u * kRoutePairs];                              // owner << 16 | rank among the tile's records for it
#pragma unroll
    for (uint32_t k = 0; k < 2u * kRoutePairs; ++k) {
      pos[k] = 0u;
      if ((valid >> k & 1u) != 0u) {
        const uint32_t d = derep_owner(rec[k], world);
        pos[k] = d << 16 | atomicAdd(&hist[d], 1u);
      }
    }
    if (!PLACE) { continue; }                                    // (the histogram runs on over the workgroup's tiles)
    __syncthreads();
    if (tid < 64u) {
      // the tile's records per owner, where each owner's piece begins in the staging area, and the room reserved for it
      const uint32_t h = tid < world ? hist[tid] : 0u;
      uint32_t incl = h;
#pragma unroll
      for (unsigned d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64); if (tid >= d) { incl += up; } }
      lstart[tid] = incl - h;
      if (h != 0u) { gbase[tid] = run_start + atomicAdd(&a.cursor[tid], h); }
      if (tid == 63u) { present = incl; }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 2u * kRoutePairs; ++k) {
      if ((valid >> k & 1u) != 0u) {
        const uint32_t at = lstart[pos[k] >> 16] + (pos[k] & 0xFFFFu);
        stage_h[at] = rec[k];
        stage_i[at] = a.first + (uint32_t)(t * kRouteTile) + (k >> 1) * (2u * kRouteThreads) + 2u * tid + (k & 1u);
      }
    }
    __syncthreads();
    const uint32_t staged = present;
#pragma unroll
    for (uint32_t k = 0; k < kRouteTile / kRouteThreads; ++k) {
      const uint32_t j = k * kRouteThreads + tid;
      if (j < staged) {
        // the owner whose piece holds place j: the last d with lstart[d] <= j (an owner the tile did not meet begins where
        // the next one does; behind the last rank every lstart is `staged`)
        uint32_t d = 0;
#pragma unroll
        for (uint32_t step = kDerepMaxWorld / 2u; step != 0u; step >>= 1) { if (lstart[d + step] <= j) { d += step; } }
        const uint32_t g = gbase[d] + (j - lstart[d]);
        if (g < a.count) { a.out_hash[g] = stage_h[j]; a.out_id[g] = stage_i[j]; }   // (always, when the slice is what the counting launch saw)
      }
    }
    if (tid < kDerepMaxWorld) { hist[tid] = 0u; }
    __syncthreads();
  }
  if (!PLACE) {
    __syncthreads();
    if (tid < world && hist[tid] != 0u) { atomicAdd(&a.counts[tid], hist[tid]); }
  }
}

// an owner: the hashes it received into its own d_seqhash, where k_derep_claim looks them up by id
__global__ __launch_bounds__(256) void k_derep_scatter(const uint64_t * __restrict__ in_hash, const uint32_t * __restrict__ in_id, uint32_t count,
                                                       uint32_t n, uint64_t * __restrict__ seqhash) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
    const uint32_t i = in_id[t];
    if (i < n) { seqhash[i] = in_hash[t]; }
  }
}

// ... and what it found, for the way home: first_identical[id] << 32 | id
__global__ __launch_bounds__(256) void k_derep_pack(const uint32_t * __restrict__ in_id, uint32_t count, uint32_t n,
                                                    const uint32_t * __restrict__ first_identical, unsigned long long * __restrict__ packed) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
    const uint32_t i = in_id[t];
    packed[t] = (unsigned long long)(i < n ? first_identical[i] : SWA_NO_AMPLICON) << 32 | i;
  }
}

// rank 0: the owners' packed words into first_identical[]
__global__ __launch_bounds__(256) void k_derep_home(const unsigned long long * __restrict__ packed, uint32_t count, uint32_t n,
                                                    uint32_t * __restrict__ first_identical) {
  for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < count; t += gridDim.x * blockDim.x) {
    const unsigned long long w = packed[t];
    if ((uint32_t)w < n) { first_identical[(uint32_t)w] = (uint32_t)(w >> 32); }
  }
}

// The rounds of the search over the amplicons of `list` (nullptr: all n of the database) against a table of `tsize` slots:
// claim, resolve, and again with a re-mixed key over whoever failed verification, until nobody is left.  d_seqhash holds the
// hash of every listed amplicon; first_identical[i] of every listed i is left in d_graft.  Serves swa_derep_resident (every
// amplicon, swa_hashtable_size(n)) and an owner of swa_multi_derep_resident (its inbox, swa_hashtable_size(received)).
// *rounds (may be null): how many rounds ran.
int derep_rounds(swa_ctx * ctx, const uint32_t * list, uint32_t count, uint64_t tsize, uint32_t * rounds) {
  const uint32_t n = ctx->db.n;
  // test hook: narrow the key so that distinct sequences collide (exercises the re-key rounds)
  uint32_t keybits = 64;
  if (const char * bits = std::getenv("SWA_DEREP_KEY_BITS")) {
    const int b = std::atoi(bits);
    if (b >= 1 && b < 64) { keybits = (uint32_t)b; }
  }
  SWA_TRY(swa_reserve(ctx, ctx->d_table, tsize * sizeof(unsigned long long)));        // keys
  SWA_TRY(swa_reserve(ctx, ctx->d_counts, tsize * sizeof(uint32_t)));                 // minimum claimant per slot
  SWA_TRY(swa_reserve(ctx, ctx->d_cursor, uint64_t(n) * sizeof(uint32_t)));           // slot of every amplicon
  SWA_TRY(swa_reserve(ctx, ctx->d_graft, uint64_t(n) * sizeof(uint32_t)));            // result
  ctx->res.fast.candidates_end();                           // (d_graft no longer holds graft candidates)
  SWA_TRY(swa_reserve(ctx, ctx->d_list_a, uint64_t(count) * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_list_b, uint64_t(count) * sizeof(uint32_t)));
  ctx->ix.table_repurposed();                             // d_table becomes the key table
  SWA_HIP(ctx, hipMemsetAsync(ctx->d_table.ptr, 0, tsize * sizeof(unsigned long long), ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(ctx->d_counts.ptr, 0xFF, tsize * sizeof(uint32_t), ctx->stream));

  auto * keys = static_cast<unsigned long long *>(ctx->d_table.ptr);
  auto * rep = static_cast<uint32_t *>(ctx->d_counts.ptr);
  auto * slot_of = static_cast<uint32_t *>(ctx->d_cursor.ptr);
  auto * result = static_cast<uint32_t *>(ctx->d_graft.ptr);
  uint32_t * next_count = swa_status(ctx)->flags + kFlagDerepLeft;
  uint32_t * lists[2] = {static_cast<uint32_t *>(ctx->d_list_a.ptr), static_cast<uint32_t *>(ctx->d_list_b.ptr)};
  const uint32_t * active = list;                          // round 0: every amplicon (of the list)
  uint32_t round = 0;
  for (; count > 0; ++round) {
    if (round > 64) { return swa_fail_msg(ctx, SWA_E_DEVICE, "swa_derep: key collisions did not resolve"); }
    uint32_t * next = lists[round & 1u];
    const int grid = (int)std::min<uint64_t>((uint64_t(count) + 255) / 256, (uint64_t)ctx->num_cus * 16);
    SWA_HIP(ctx, hipMemsetAsync(next_count, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_derep_claim, dim3(grid), dim3(256), 0, ctx->stream,
                       static_cast<const uint64_t *>(ctx->d_seqhash.ptr), active, count, keybits, round, keys, rep,
                       tsize - 1, slot_of);
    hipLaunchKernelGGL(k_derep_resolve, dim3(grid), dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off,
                       ctx->db.seqlen, active, count, rep, slot_of, result, next, next_count);
    SWA_HIP(ctx, hipGetLastError());
    uint32_t left = 0;
    SWA_HIP(ctx, hipMemcpyAsync(&left, next_count, sizeof(left), hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    active = next;
    count = left;
  }
  if (rounds != nullptr) { *rounds = round; }
  return SWA_OK;
}

}  // namespace

// What swa_derep does up to the download: first_identical stays in HBM (d_graft) for swa_d0_cluster_device.
extern "C" int swa_derep_resident(swa_ctx * ctx) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  ctx->dr = {};                                             // the previous dereplication and its tables end here
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_derep: no database"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->db.n;
  SWA_TRY(swa_hash_sequences(ctx));
  SWA_TRY(derep_rounds(ctx, nullptr, n, swa_hashtable_size(n), nullptr));
  ctx->dr.first_ready = true;
  return SWA_OK;
}

extern "C" int swa_derep(swa_ctx * ctx, uint32_t * first_identical) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_derep: no database"); }
  if (first_identical == nullptr) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_derep: bad argument"); }
  SWA_TRY(swa_derep_resident(ctx));
  return swa_download(ctx, {{first_identical, ctx->d_graft.ptr, uint64_t(ctx->db.n) * sizeof(uint32_t)}});
}

// ---- several GPUs: one rank's steps of swa_multi_derep_resident (multi.hip runs the exchange between them) -------------------
uint32_t swa_derep_owner_of(uint64_t hash, uint32_t world) { return derep_owner(hash, world); }

extern "C" int swa_multi_derep_owner_for(uint64_t hash, uint32_t world, uint32_t * owner) {
  if (owner == nullptr || world < 1 || world > kDerepMaxWorld) { return SWA_E_ARG; }
  *owner = derep_owner(hash, world);
  return SWA_OK;
}

int swa_derep_route_slice(swa_ctx * ctx, uint32_t first, uint32_t count, uint32_t world, swa_dbuf & work, uint32_t * counts) {
  if (ctx == nullptr || counts == nullptr || world < 1 || world > kDerepMaxWorld) { return SWA_E_ARG; }
  // On every rank the previous dereplication ends, and neither d_table nor the partly filled d_seqhash serves a later d = 1 call
  ctx->dr = {};
  ctx->ix.table_repurposed();
  const uint32_t n = ctx->db.n;
  if (n == 0 || first > n || count > n - first) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_multi_derep: no database, or a slice beyond it"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(swa_prepare_hashing(ctx));
  SWA_TRY(swa_reserve(ctx, work, swa_derep_routed::bytes(count)));
  const swa_derep_routed w(work.ptr, count);
  // counts and run cursors: the status block's cursor words, as 32-bit ones
  static_assert(2 * kDerepMaxWorld * sizeof(uint32_t) <= sizeof(swa_status_block::cursors), "a count and a run cursor for every rank");
  auto * d_counts = reinterpret_cast<uint32_t *>(swa_status(ctx)->cursors);
  SWA_HIP(ctx, hipMemsetAsync(d_counts, 0, 2 * kDerepMaxWorld * sizeof(uint32_t), ctx->stream));
  if (count != 0) {
    const size_t zbytes = 4ull * ctx->zobrist_len * sizeof(uint64_t);
    const int hgrid = swa_grid256(ctx, count);
    const auto * zob = static_cast<const uint64_t *>(ctx->d_zobrist.ptr);
    if (zbytes <= 48u * 1024u) {
      hipLaunchKernelGGL(k_derep_hash_slice<true>, dim3(hgrid), dim3(256), zbytes, ctx->stream, ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen,
                         zob, ctx->zobrist_len, first, count, w.slice_hash);
    } else {
      hipLaunchKernelGGL(k_derep_hash_slice<false>, dim3(hgrid), dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen,
                         zob, ctx->zobrist_len, first, count, w.slice_hash);
    }
    RouteArgs a{};
    a.hash = reinterpret_cast<const unsigned long long *>(w.slice_hash);
    a.first = first; a.count = count; a.world = world;
    a.counts = d_counts; a.cursor = d_counts + kDerepMaxWorld;
    a.out_hash = reinterpret_cast<unsigned long long *>(w.hash); a.out_id = w.id;
    const uint64_t tiles = ((uint64_t)count + kRouteTile - 1) / kRouteTile;
    const dim3 grid((unsigned)std::min<uint64_t>(tiles, (uint64_t)ctx->num_cus * 8));
    hipLaunchKernelGGL(k_derep_route<false>, grid, dim3(kRouteThreads), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_derep_route<true>, grid, dim3(kRouteThreads), 0, ctx->stream, a);
    SWA_HIP(ctx, hipGetLastError());
  }
  // ONE read of the counts, into the pinned mirror of the status block
  auto * h_counts = reinterpret_cast<uint32_t *>(ctx->h_status->cursors);
  SWA_HIP(ctx, hipMemcpyAsync(h_counts, d_counts, kDerepMaxWorld * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t sum = 0;
  for (uint32_t r = 0; r < world; ++r) { counts[r] = h_counts[r]; sum += h_counts[r]; }
  if (sum != count) { return swa_fail_msg(ctx, SWA_E_INTERNAL, "swa_multi_derep: the routed records do not add up to the slice"); }
  return SWA_OK;
}

int swa_derep_owner_rounds(swa_ctx * ctx, const uint64_t * in_hash, const uint32_t * in_id, uint32_t received, uint64_t * packed, uint32_t * rounds) {
  if (ctx == nullptr || rounds == nullptr) { return SWA_E_ARG; }
  *rounds = 0;
  if (received == 0) { return SWA_OK; }                        // (an empty inbox: a slice of nothing, or hashes that all live elsewhere)
  const uint32_t n = ctx->db.n;
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const dim3 g((unsigned)swa_grid256(ctx, received)), b(256);
  hipLaunchKernelGGL(k_derep_scatter, g, b, 0, ctx->stream, in_hash, in_id, received, n, static_cast<uint64_t *>(ctx->d_seqhash.ptr));
  SWA_TRY(derep_rounds(ctx, in_id, received, swa_hashtable_size(received), rounds));
  hipLaunchKernelGGL(k_derep_pack, g, b, 0, ctx->stream, in_id, received, n, static_cast<const uint32_t *>(ctx->d_graft.ptr),
                     reinterpret_cast<unsigned long long *>(packed));
  SWA_HIP(ctx, hipGetLastError());
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

int swa_derep_home(swa_ctx * ctx, const uint64_t * packed) {
  if (ctx == nullptr || packed == nullptr) { return SWA_E_ARG; }
  const uint32_t n = ctx->db.n;
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(swa_reserve(ctx, ctx->d_graft, uint64_t(n) * sizeof(uint32_t)));
  ctx->res.fast.candidates_end();
  hipLaunchKernelGGL(k_derep_home, dim3((unsigned)swa_grid256(ctx, n)), dim3(256), 0, ctx->stream, reinterpret_cast<const unsigned long long *>(packed),
                     n, n, static_cast<uint32_t *>(ctx->d_graft.ptr));
  SWA_HIP(ctx, hipGetLastError());
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->dr.first_ready = true;
  return SWA_OK;
}

// ---- the clusters, their sums and their order, from the resident array (src/derep.cc:276-354, 67-90) --------------------
// swa_d0_cluster (host/cluster_d0.cpp) walks first_identical[] twice with one thread and sorts the clusters; everything it
// makes is integer sums, a stable grouping and a stable order, all of it a function of first_identical[] and abundance[],
// which are both in HBM.  Here:
//
//   k_d0_seed_flags   flag[i] = first[i] == i; rocPRIM's exclusive scan of the flags numbers the clusters in db order (=
//                     seed order) and counts them
//   k_d0_keys         (cluster number of first[i], i); one stable radix sort over the bits the cluster count needs groups
//                     the members, ascending db index inside every cluster: the layout of swa_d0_result::members
//   k_d0_sums         one position per lane over the grouped order: the cluster number never falls along it, so mass, size
//                     and singletons come from the run reduction of swa_internal.h (swa_wave_run_reduce; a sequence with
//                     10^6 copies: 15 625 atomics on its words); the first position of a cluster writes its seed and begin
//   k_d0_maxima       largest size and heaviest mass, a wave's maximum per atomic
//   k_d0_order_keys   heaviest - mass: one stable radix sort of the cluster numbers over the bits the heaviest mass needs
//                     leaves them by mass descending, ties in seed order as they went in
//   k_d0_gather       the five tables in that order
// Nothing depends on scheduling: sums, maxima and stable sorts of integers.
namespace {

// d_d0, n amplicons: rank (cluster number of a seed), the grouping sort's keys and ids, the members in grouped order
struct D0Work {
  uint32_t * rank, * keys_in, * keys_out, * ids_in, * members;  void lay(swa_carver & c, uint64_t n) { c.take(n, rank, keys_in, keys_out, ids_in, members); }
};

// d_d0_tab, c clusters: maxima (heaviest, largest); the tables in seed order (*_s), the order sort's keys and cluster numbers, the tables
// in output order.  k_d0_sums and k_d0_maxima add into what two fills clear: maxima with mass_s (`cleared64`), size_s with singles_s (`cleared32`)
struct D0Tables {
  unsigned long long * maxima, * mass_s, * okeys_in, * okeys_out, * mass;
  uint32_t * seed_s, * size_s, * singles_s, * begin_s, * num_in, * num_out, * seed, * size, * singles, * begin;
  swa_extent cleared64, cleared32;
  void lay(swa_carver & at, uint64_t c) {
    at.take(2, maxima); at.take(c, mass_s);
    cleared64 = at.extent(maxima);
    at.take(c, okeys_in, okeys_out, mass, seed_s, size_s, singles_s);
    cleared32 = at.extent(size_s);
    at.take(c, begin_s, num_in, num_out, seed, size, singles, begin);
  }
};

__global__ __launch_bounds__(256) void k_d0_seed_flags(const uint32_t * __restrict__ first, uint32_t n, uint32_t * __restrict__ flag) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    flag[i] = first[i] == (uint32_t)i ? 1u : 0u;
  }
}

__global__ __launch_bounds__(256) void k_d0_keys(const uint32_t * __restrict__ first, const uint32_t * __restrict__ rank, uint32_t n,
                                                 uint32_t * __restrict__ keys, uint32_t * __restrict__ ids) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    keys[i] = rank[first[i]];
    ids[i] = (uint32_t)i;
  }
}

// mass and singletons of a run of one cluster (swa_wave_run_reduce, swa_internal.h; the run's length is its size)
struct D0Run {
  unsigned long long mass; uint32_t singles;
  __device__ __forceinline__ D0Run shfl_up(uint32_t d) const { return D0Run{swa_shfl_up_u64(mass, d), __shfl_up(singles, d, 64)}; }
  __device__ __forceinline__ void absorb(const D0Run & o) { mass += o.mass; singles += o.singles; }
};

// cluster[k] = the cluster number of position k of the grouped order (never falls along k), members[k] the amplicon there.
// mass / size / singles were cleared before the launch.
__global__ __launch_bounds__(256) void k_d0_sums(const uint32_t * __restrict__ cluster, const uint32_t * __restrict__ members,
                                                 const uint64_t * __restrict__ abundance, uint32_t n, unsigned long long * mass,
                                                 uint32_t * size, uint32_t * singles, uint32_t * __restrict__ seed, uint32_t * __restrict__ begin) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < swa_wave_span(n); k += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t c = SWA_NO_AMPLICON;                                     // (beyond the order: a run of its own that writes nothing)
    D0Run r{0, 0};
    if (k < n) {
      c = cluster[k];
      const uint32_t a = members[k];
      r.mass = abundance[a]; r.singles = r.mass == 1ull ? 1u : 0u;
      if (k == 0 || cluster[k - 1] != c) { seed[c] = a; begin[c] = (uint32_t)k; }   // the cluster's first position: its seed
    }
    const swa_run run = swa_wave_run_reduce(c, r);
    if (k >= n || !run.last) { continue; }
    // the run [k + 1 - length, k]: the whole cluster when nothing of it lies in front of or behind it — nobody else writes its sums
    const uint64_t start = k + 1 - run.length;
    const bool whole = (start == 0 || cluster[start - 1] != c) && (k + 1 == n || cluster[k + 1] != c);
    if (whole) { mass[c] = r.mass; size[c] = run.length; singles[c] = r.singles; }
    else { atomicAdd(&mass[c], r.mass); atomicAdd(&size[c], run.length); atomicAdd(&singles[c], r.singles); }
  }
}

// maxima[0] = heaviest mass, maxima[1] = largest size (cleared before the launch): a wave's maxima per atomic
__global__ __launch_bounds__(256) void k_d0_maxima(const unsigned long long * __restrict__ mass, const uint32_t * __restrict__ size,
                                                   uint32_t clusters, unsigned long long * maxima) {
  unsigned long long heavy = 0, large = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < clusters; c += (uint64_t)gridDim.x * blockDim.x) {
    heavy = mass[c] > heavy ? mass[c] : heavy;
    large = size[c] > large ? size[c] : large;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long h2 = swa_shfl_xor_u64(heavy, d), l2 = swa_shfl_xor_u64(large, d);
    heavy = h2 > heavy ? h2 : heavy;
    large = l2 > large ? l2 : large;
  }
  if ((threadIdx.x & 63u) == 0u && large != 0ull) { atomicMax(&maxima[0], heavy); atomicMax(&maxima[1], large); }
}

__global__ __launch_bounds__(256) void k_d0_order_keys(const unsigned long long * __restrict__ mass, unsigned long long heaviest,
                                                       uint32_t clusters, unsigned long long * __restrict__ keys, uint32_t * __restrict__ num) {
  for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < clusters; c += (uint64_t)gridDim.x * blockDim.x) {
    keys[c] = heaviest - mass[c];
    num[c] = (uint32_t)c;
  }
}

__global__ __launch_bounds__(256) void k_d0_gather(D0Tables t, uint32_t clusters) {
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < clusters; r += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t c = t.num_out[r];
    t.mass[r] = t.mass_s[c]; t.seed[r] = t.seed_s[c]; t.size[r] = t.size_s[c]; t.singles[r] = t.singles_s[c]; t.begin[r] = t.begin_s[c];
  }
}

}  // namespace

extern "C" int swa_d0_cluster_device(swa_ctx * ctx, uint64_t * summary3) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (!ctx->dr.first_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d0_cluster_device: no resident first_identical array (call swa_derep_resident first)"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  ctx->dr.tables_ready = false;
  const uint32_t n = ctx->db.n;
  const auto * first = static_cast<const uint32_t *>(ctx->d_graft.ptr);
  D0Work w;
  SWA_TRY(swa_carve(ctx, ctx->d_d0, n, true, w));
  const dim3 g((unsigned)swa_grid256(ctx, n)), b(256);
  // rocPRIM's scratch: the most any of the three calls asks for at n items (the clusters are never more)
  size_t asked[3] = {}, need = 0;
  auto * k64 = static_cast<unsigned long long *>(nullptr);
  (void)rocprim::exclusive_scan(nullptr, asked[0], w.keys_in, w.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->stream);
  (void)rocprim::radix_sort_pairs(nullptr, asked[1], w.keys_in, w.keys_out, w.ids_in, w.members, (size_t)n, 0, 32, ctx->stream);
  (void)rocprim::radix_sort_pairs(nullptr, asked[2], k64, k64, w.ids_in, w.members, (size_t)n, 0, 64, ctx->stream);
  const size_t tmp_bytes = *std::max_element(asked, asked + 3);
  SWA_TRY(swa_reserve(ctx, ctx->d_scan_hits, tmp_bytes + 16));
  // ---- cluster numbers in seed order, and how many
  hipLaunchKernelGGL(k_d0_seed_flags, g, b, 0, ctx->stream, first, n, w.keys_in);
  need = tmp_bytes;
  SWA_HIP(ctx, rocprim::exclusive_scan(ctx->d_scan_hits.ptr, need, w.keys_in, w.rank, 0u, (size_t)n, rocprim::plus<uint32_t>(), ctx->stream));
  uint32_t last_rank = 0, last_first = 0;
  SWA_HIP(ctx, hipMemcpyAsync(&last_rank, w.rank + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipMemcpyAsync(&last_first, first + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  hipLaunchKernelGGL(k_d0_keys, g, b, 0, ctx->stream, first, w.rank, n, w.keys_in, w.ids_in);     // (needs no count: queued in front of the wait)
  SWA_HIP(ctx, hipGetLastError());
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const uint32_t clusters = last_rank + (last_first == n - 1 ? 1u : 0u);
  if (clusters == 0 || clusters > n) { return swa_fail_msg(ctx, SWA_E_INTERNAL, "swa_d0_cluster_device: the resident array has no seed"); }
  // ---- members grouped by cluster, db order inside (zero key bits — one cluster — sort on one bit that is 0 everywhere)
  need = tmp_bytes;
  SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, need, w.keys_in, w.keys_out, w.ids_in, w.members, (size_t)n, 0,
                                         std::max(1u, swa_bit_width(clusters - 1u)), ctx->stream));
  // ---- sums over the runs, seeds, begins; the maxima
  D0Tables t;
  SWA_TRY(swa_carve(ctx, ctx->d_d0_tab, clusters, true, t));
  const dim3 gc((unsigned)swa_grid256(ctx, clusters));
  SWA_HIP(ctx, hipMemsetAsync(t.cleared64.ptr, 0, t.cleared64.bytes, ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(t.cleared32.ptr, 0, t.cleared32.bytes, ctx->stream));
  hipLaunchKernelGGL(k_d0_sums, g, b, 0, ctx->stream, w.keys_out, w.members, ctx->db.abundance, n, t.mass_s, t.size_s, t.singles_s, t.seed_s, t.begin_s);
  hipLaunchKernelGGL(k_d0_maxima, gc, b, 0, ctx->stream, t.mass_s, t.size_s, clusters, t.maxima);
  SWA_HIP(ctx, hipGetLastError());
  unsigned long long maxima[2] = {0, 0};
  SWA_HIP(ctx, hipMemcpyAsync(maxima, t.maxima, sizeof(maxima), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // ---- output order: mass descending, seed order among equals (the numbers go in ascending: the sort is stable)
  hipLaunchKernelGGL(k_d0_order_keys, gc, b, 0, ctx->stream, t.mass_s, maxima[0], clusters, t.okeys_in, t.num_in);
  need = tmp_bytes;
  SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, need, t.okeys_in, t.okeys_out, t.num_in, t.num_out, (size_t)clusters, 0,
                                         std::max(1u, swa_bit_width(maxima[0])), ctx->stream));
  hipLaunchKernelGGL(k_d0_gather, gc, b, 0, ctx->stream, t, clusters);
  SWA_HIP(ctx, hipGetLastError());
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->dr.tables_ready = true;
  ctx->dr.clusters = clusters;
  ctx->dr.largest = (uint32_t)maxima[1];
  ctx->dr.heaviest = maxima[0];
  if (summary3 != nullptr) { summary3[0] = clusters; summary3[1] = maxima[1]; summary3[2] = maxima[0]; }
  return SWA_OK;
}

extern "C" int swa_d0_cluster_fetch(swa_ctx * ctx, uint32_t * seed, uint64_t * mass, uint32_t * size, uint32_t * singletons, uint32_t * begin,
                                    uint32_t cluster_cap, uint32_t * members, uint32_t * clusters) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (!ctx->dr.tables_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d0_cluster_fetch: no cluster tables in place (call swa_d0_cluster_device first)"); }
  const uint32_t c = ctx->dr.clusters, n = ctx->db.n;
  if (clusters != nullptr) { *clusters = c; }
  const bool wants_tables = seed != nullptr || mass != nullptr || size != nullptr || singletons != nullptr || begin != nullptr;
  if (wants_tables && cluster_cap < c) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d0_cluster_fetch: cluster arrays too small"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  D0Work w;
  SWA_TRY(swa_carve(ctx, ctx->d_d0, n, false, w));
  D0Tables t;
  SWA_TRY(swa_carve(ctx, ctx->d_d0_tab, c, false, t));
  const uint64_t c4 = (uint64_t)c * sizeof(uint32_t);
  return swa_download(ctx, {{members, w.members, (uint64_t)n * sizeof(uint32_t)}, {mass, t.mass, (uint64_t)c * sizeof(uint64_t)},
                            {seed, t.seed, c4}, {size, t.size, c4}, {singletons, t.singles, c4}, {begin, t.begin, c4}});
}
