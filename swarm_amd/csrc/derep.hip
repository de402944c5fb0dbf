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

}  // namespace

// What swa_derep does up to the download: first_identical stays in HBM (d_graft) for swa_d0_cluster_device.
extern "C" int swa_derep_resident(swa_ctx * ctx) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  ctx->dr = {};                                             // the previous dereplication and its tables end here
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_derep: no database"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->db.n;
  SWA_TRY(swa_hash_sequences(ctx));
  // test hook: narrow the key so that distinct sequences collide (exercises the re-key rounds)
  uint32_t keybits = 64;
  if (const char * bits = std::getenv("SWA_DEREP_KEY_BITS")) {
    const int b = std::atoi(bits);
    if (b >= 1 && b < 64) { keybits = (uint32_t)b; }
  }
  const uint64_t tsize = swa_hashtable_size(n);
  SWA_TRY(swa_reserve(ctx, ctx->d_table, tsize * sizeof(unsigned long long)));        // keys
  SWA_TRY(swa_reserve(ctx, ctx->d_counts, tsize * sizeof(uint32_t)));                 // minimum claimant per slot
  SWA_TRY(swa_reserve(ctx, ctx->d_cursor, uint64_t(n) * sizeof(uint32_t)));           // slot of every amplicon
  SWA_TRY(swa_reserve(ctx, ctx->d_graft, uint64_t(n) * sizeof(uint32_t)));            // result
  ctx->res.fast.candidates_end();                           // (d_graft no longer holds graft candidates)
  SWA_TRY(swa_reserve(ctx, ctx->d_list_a, uint64_t(n) * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_list_b, uint64_t(n) * sizeof(uint32_t)));
  ctx->ix.table_repurposed();                             // d_table becomes the key table
  SWA_HIP(ctx, hipMemsetAsync(ctx->d_table.ptr, 0, tsize * sizeof(unsigned long long), ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(ctx->d_counts.ptr, 0xFF, tsize * sizeof(uint32_t), ctx->stream));

  auto * keys = static_cast<unsigned long long *>(ctx->d_table.ptr);
  auto * rep = static_cast<uint32_t *>(ctx->d_counts.ptr);
  auto * slot_of = static_cast<uint32_t *>(ctx->d_cursor.ptr);
  auto * result = static_cast<uint32_t *>(ctx->d_graft.ptr);
  uint32_t * next_count = swa_status(ctx)->flags + kFlagDerepLeft;
  uint32_t * lists[2] = {static_cast<uint32_t *>(ctx->d_list_a.ptr), static_cast<uint32_t *>(ctx->d_list_b.ptr)};
  const uint32_t * active = nullptr;                       // round 0: every amplicon
  uint32_t count = n;
  for (uint32_t round = 0; count > 0; ++round) {
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
