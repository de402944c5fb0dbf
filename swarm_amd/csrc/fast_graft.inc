// fast_graft.inc — the bookkeeping of --fastidious on the clustering that swa_d1_cluster_device left in HBM; included at the
// end of cluster_gpu.hip (one code object with the agglomeration: nothing more to load for a run that takes this route).
//
// The reference keeps this on the host, between and after its two fastidious passes (src/algod1.cc:1291-1328: mass per
// swarm, light / heavy; :214-336: attach_candidates).  Everything it reads is in HBM already — d_cluster (swarm of every
// amplicon, generation, member order, bounds), the database (abundance, length), d_graft (the candidates) — so it is done
// there, and a plain `-f -o` run downloads none of those arrays:
//
//   k_swarm_sums      one pass over the member order: position k belongs to swarm sid[order[k]], which never falls along
//                     k, so a wave sums its runs of equal swarms with a segmented scan over the lanes and the last lane of
//                     a run writes — a plain store when the run is the whole swarm (most swarms have one to three
//                     members), one atomic per (wave, swarm) otherwise (a swarm of millions spans thousands of waves)
//   k_light_roles     role[a] = mass[sid[a]] < boundary ? 0 : 1, the byte the fastidious pass reads; k_light_stats the five
//                     numbers of the log, reduced per wave
//   k_owner_counts, k_owner_scan, k_owner_write   the owner byte of every amplicon (255 light, else the shard of a run on several
//                     GPUs that expands this heavy amplicon) from the role bytes: an exclusive count of the heavy ones
//   k_graft_min       slot[swarm of the child] = min(parent << 32 | child) over the candidates: what the sequential walk
//                     over the sorted pairs decides (cluster_d1.cpp: graft_sorted_pairs_in_parallel) without the walk
//   k_graft_winners   the winners compacted, the losers' candidates withdrawn
//   rocPRIM           winners by (heavy swarm, pair): a radix sort on the pair, a stable one on the heavy swarm's bits
//   k_graft_apply     light swarm / parent / child of every graft in chain order; the heavy swarms' sums grown by their
//                     lights', a wave's run of one heavy swarm reduced first as above
// Integer sums, minima and maxima only: every result is independent of scheduling.

namespace {

// d_cluster as swa_d1_cluster_device lays it out: label | gen | parent | swarmid | ids_in | ids_out (the order) | seed_rank | begins
struct ClusterView { const uint32_t * gen, * sid, * order, * begins; };
ClusterView cluster_view(const swa_ctx * ctx) {
  const uint64_t n = ctx->db.n;
  const auto * label = static_cast<const uint32_t *>(ctx->d_cluster.ptr);
  return ClusterView{label + n, label + 3 * n, label + 5 * n, label + 7 * n};
}

// d_swarm_sums: mass u64[w] | sumlen u64[w] | singletons u32[w] | maxgen u32[w], w = swarms of the clustering in place
struct SwarmSums { unsigned long long * mass, * sumlen; uint32_t * singles, * maxgen; };
SwarmSums swarm_sums(const swa_ctx * ctx) {
  const uint64_t w = ctx->res.cluster_nswarms;
  auto * mass = static_cast<unsigned long long *>(ctx->d_swarm_sums.ptr);
  auto * singles = reinterpret_cast<uint32_t *>(mass + 2 * w);
  return SwarmSums{mass, mass + w, singles, singles + w};
}

// d_graft_work: eight control words (kCtl*), then slot u64[w] | pairs u64[2][w] | heavy u32[2][w]
constexpr uint32_t kCtlLightSwarms = 0, kCtlLightAmps = 1, kCtlLightNt = 2, kCtlWinners = 3, kCtlWords = 8;

// The lanes of a wave hold keys that never fall from lane to lane: every run of equal keys is summed (a, b, c, count) and
// its maximum taken (m) into its LAST lane — a segmented inclusive scan, six steps.  Every lane of the wave takes part.
__device__ __forceinline__ void wave_run_reduce(uint32_t key, unsigned long long & a, unsigned long long & b, uint32_t & c, uint32_t & m,
                                                uint32_t & count) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t key2 = __shfl_up(key, d, 64);
    const unsigned long long a2 = swa_shfl_up_u64(a, d), b2 = swa_shfl_up_u64(b, d);
    const uint32_t c2 = __shfl_up(c, d, 64), m2 = __shfl_up(m, d, 64), count2 = __shfl_up(count, d, 64);
    if (lane >= d && key2 == key) { a += a2; b += b2; c += c2; m = m2 > m ? m2 : m; count += count2; }
  }
}

// positions of a grid-stride loop in which whole waves take part: the count rounded up to the wave
__device__ __forceinline__ uint64_t wave_span(uint64_t count) { return (count + 63u) & ~uint64_t(63); }

__global__ __launch_bounds__(256) void k_swarm_sums(const uint32_t * __restrict__ order, const uint32_t * __restrict__ sid,
                                                    const uint32_t * __restrict__ gen, const uint32_t * __restrict__ begins,
                                                    const uint64_t * __restrict__ abundance, const uint32_t * __restrict__ seqlen, uint32_t n,
                                                    SwarmSums out) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < wave_span(n); k += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t s = kUnset, single = 0, g = 0, members = 0;       // (beyond the order: a run of its own that writes nothing)
    unsigned long long mass = 0, len = 0;
    if (k < n) {
      const uint32_t a = order[k];
      s = sid[a]; mass = abundance[a]; len = seqlen[a]; single = mass == 1ull ? 1u : 0u; g = gen[a]; members = 1;
    }
    wave_run_reduce(s, mass, len, single, g, members);
    const uint32_t next = __shfl_down(s, 1, 64);
    if (k >= n || (lane != 63u && next == s)) { continue; }   // (not the last lane of its run)
    // the run [k + 1 - members, k] is the whole swarm: nobody else writes its sums (they were cleared before the launch)
    if ((uint32_t)k + 1u - members == begins[s] && (uint32_t)k + 1u == begins[s + 1u]) {
      out.mass[s] = mass; out.sumlen[s] = len; out.singles[s] = single; out.maxgen[s] = g;
    } else {
      atomicAdd(&out.mass[s], mass); atomicAdd(&out.sumlen[s], len); atomicAdd(&out.singles[s], single); atomicMax(&out.maxgen[s], g);
    }
  }
}

// four amplicons a thread: one 32-bit store of four role bytes (the tail one by one)
__global__ __launch_bounds__(256) void k_light_roles(const uint32_t * __restrict__ sid, const unsigned long long * __restrict__ mass,
                                                     unsigned long long boundary, uint32_t n, uint8_t * __restrict__ role) {
  const uint64_t quads = (uint64_t)n / 4u;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t four = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) { four |= (mass[sid[4u * q + j]] < boundary ? 0u : 1u) << (8u * j); }
    reinterpret_cast<uint32_t *>(role)[q] = four;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) {
    const uint64_t a = 4u * quads + threadIdx.x;
    role[a] = mass[sid[a]] < boundary ? 0 : 1;
  }
}

// ctl[kCtlLightSwarms .. kCtlLightNt] += light swarms, their amplicons (sizes from the bounds), their nucleotides
__global__ __launch_bounds__(256) void k_light_stats(const unsigned long long * __restrict__ mass, const unsigned long long * __restrict__ sumlen,
                                                     const uint32_t * __restrict__ begins, unsigned long long boundary, uint32_t nswarms,
                                                     unsigned long long * ctl) {
  unsigned long long swarms = 0, amps = 0, nt = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nswarms; s += (uint64_t)gridDim.x * blockDim.x) {
    if (mass[s] < boundary) { ++swarms; amps += begins[s + 1u] - begins[s]; nt += sumlen[s]; }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    swarms += swa_shfl_xor_u64(swarms, d); amps += swa_shfl_xor_u64(amps, d); nt += swa_shfl_xor_u64(nt, d);
  }
  if ((threadIdx.x & 63u) == 0u && swarms != 0ull) {
    atomicAdd(&ctl[kCtlLightSwarms], swarms); atomicAdd(&ctl[kCtlLightAmps], amps); atomicAdd(&ctl[kCtlLightNt], nt);
  }
}

__global__ __launch_bounds__(256) void k_graft_min(const uint32_t * __restrict__ cand, const uint32_t * __restrict__ sid, uint32_t n,
                                                   unsigned long long * slot) {
  for (uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; a < n; a += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = cand[a];
    if (p != kUnset) { atomicMin(&slot[sid[a]], ((unsigned long long)p << 32) | a); }
  }
}

// a candidate that holds its swarm's slot wins (one a swarm: the pairs are distinct, so there are never more winners than
// swarms); every other candidate is withdrawn.  Winners are appended a wave at a time, in no particular order: the sort fixes it.
__global__ __launch_bounds__(256) void k_graft_winners(uint32_t * __restrict__ cand, const uint32_t * __restrict__ sid, uint32_t n,
                                                       const unsigned long long * __restrict__ slot, unsigned long long * __restrict__ pairs,
                                                       uint32_t * __restrict__ heavy, unsigned long long * ctl) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; a < wave_span(n); a += (uint64_t)gridDim.x * blockDim.x) {
    bool win = false;
    unsigned long long pair = 0;
    uint32_t p = kUnset;
    if (a < n) { p = cand[a]; }
    if (p != kUnset) {
      pair = ((unsigned long long)p << 32) | a;
      win = slot[sid[a]] == pair;
      if (!win) { cand[a] = kUnset; }
    }
    const unsigned long long mask = __ballot(win);
    if (mask == 0ull) { continue; }
    unsigned long long base = 0;
    if (lane == 0u) { base = atomicAdd(&ctl[kCtlWinners], (unsigned long long)__popcll(mask)); }
    base = swa_shfl_u64(base, 0);
    if (win) {
      const uint64_t at = base + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
      pairs[at] = pair;
      heavy[at] = sid[p];
    }
  }
}

// the winners sorted by (heavy swarm, pair): graft i hangs light swarm sid[child] on heavy[i]
__global__ __launch_bounds__(256) void k_graft_apply(const uint32_t * __restrict__ heavy, const unsigned long long * __restrict__ pairs,
                                                     const uint32_t * __restrict__ sid, uint32_t grafts, uint32_t * __restrict__ light_out,
                                                     uint32_t * __restrict__ parent_out, uint32_t * __restrict__ child_out, SwarmSums sums) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < wave_span(grafts); i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t h = kUnset, single = 0, unused = 0, count = 0;
    unsigned long long mass = 0, len = 0;
    if (i < grafts) {
      const unsigned long long pair = pairs[i];
      const uint32_t child = (uint32_t)pair, l = sid[child];
      h = heavy[i];
      light_out[i] = l; parent_out[i] = (uint32_t)(pair >> 32); child_out[i] = child;
      mass = sums.mass[l]; len = sums.sumlen[l]; single = sums.singles[l]; count = 1;   // (a light swarm is nobody's heavy swarm: its sums stand still)
    }
    wave_run_reduce(h, mass, len, single, unused, count);
    const uint32_t next = __shfl_down(h, 1, 64);
    if (i >= grafts || (lane != 63u && next == h)) { continue; }
    atomicAdd(&sums.mass[h], mass); atomicAdd(&sums.sumlen[h], len); atomicAdd(&sums.singles[h], single);   // (maxgen untouched, like the reference)
  }
}

// ---- shard owners: which of S shards expands a heavy amplicon (swa_d1_fastidious_shard's slices, made where the flags lie) ----
// The h-th heavy amplicon (amplicon order, H in all) belongs to the shard s with floor(H s / S) <= h < floor(H (s + 1) / S), which is
// floor(((h + 1) S - 1) / H): h needs the number of heavy bytes in front of it, an exclusive count.  Three launches, none of
// which waits for another workgroup: the heavy bytes of every tile (k_owner_counts), the tiles' counts scanned by one
// workgroup in turns of kOwnerTurn tiles (k_owner_scan), then every tile scans its own words again from its base and writes
// the owner bytes (k_owner_write).  A thread takes four role bytes as one 32-bit load (k_light_roles stores them so); the
// word that holds the last n & 3 bytes is masked when counted and written byte by byte (both buffers are reserved with four
// bytes to spare).  Integer sums only.
constexpr uint32_t kOwnerBlock = 256, kOwnerTile = 4 * kOwnerBlock, kOwnerTurn = 256;
constexpr uint8_t kOwnerLight = 255;

// the role word q of n bytes, bytes beyond n as light
__device__ __forceinline__ uint32_t owner_role_word(const uint8_t * __restrict__ role, uint64_t q, uint32_t n) {
  const uint32_t w = reinterpret_cast<const uint32_t *>(role)[q];
  const uint64_t left = (uint64_t)n - 4u * q;                // (> 0: q < ceil(n / 4))
  return left >= 4u ? w : w & ((1u << (8u * (uint32_t)left)) - 1u);
}

// inclusive scan of v over the 256 threads of the workgroup; *total = the sum.  lds: four words
__device__ __forceinline__ uint32_t owner_block_scan(uint32_t v, uint32_t * lds, uint32_t * total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t up = __shfl_up(v, d, 64);
    if (lane >= d) { v += up; }
  }
  __syncthreads();                                          // (the previous turn's readers are done with lds)
  if (lane == 63u) { lds[wave] = v; }
  __syncthreads();
  const uint32_t w0 = lds[0], w1 = lds[1], w2 = lds[2], w3 = lds[3];
  *total = w0 + w1 + w2 + w3;
  return v + (wave > 0u ? w0 : 0u) + (wave > 1u ? w1 : 0u) + (wave > 2u ? w2 : 0u);
}

// counts[b] = heavy bytes of tile b; one workgroup a tile
__global__ __launch_bounds__(kOwnerBlock) void k_owner_counts(const uint8_t * __restrict__ role, uint32_t n, uint32_t * __restrict__ counts) {
  __shared__ uint32_t lds[4];
  const uint64_t words = ((uint64_t)n + 3u) / 4u, q = (uint64_t)blockIdx.x * kOwnerBlock + threadIdx.x;
  const uint32_t mine = q < words ? (uint32_t)__popc(owner_role_word(role, q, n) & 0x01010101u) : 0u;
  uint32_t total = 0;
  (void)owner_block_scan(mine, lds, &total);
  if (threadIdx.x == 0) { counts[blockIdx.x] = total; }
}

// base[t] = heavy bytes in front of tile t, base[tiles] = H; one workgroup, a carry from turn to turn
__global__ __launch_bounds__(kOwnerTurn) void k_owner_scan(const uint32_t * __restrict__ counts, uint32_t tiles, unsigned long long * __restrict__ base) {
  static_assert(kOwnerTurn == kOwnerBlock, "owner_block_scan: 256 threads");
  __shared__ uint32_t lds[4];
  unsigned long long carry = 0;
  for (uint32_t first = 0; first < tiles; first += kOwnerTurn) {
    const uint32_t t = first + threadIdx.x;
    const uint32_t mine = t < tiles ? counts[t] : 0u;
    uint32_t total = 0;
    const uint32_t incl = owner_block_scan(mine, lds, &total);   // (a turn holds 256 * 1024 bytes at most: 32 bits)
    if (t < tiles) { base[t] = carry + (incl - mine); }
    carry += total;
  }
  if (threadIdx.x == 0) { base[tiles] = carry; }
}

__global__ __launch_bounds__(kOwnerBlock) void k_owner_write(const uint8_t * __restrict__ role, uint32_t n, const unsigned long long * __restrict__ base,
                                                             uint32_t tiles, uint32_t nshards, uint8_t * __restrict__ owner) {
  __shared__ uint32_t lds[4];
  const uint64_t words = ((uint64_t)n + 3u) / 4u, q = (uint64_t)blockIdx.x * kOwnerBlock + threadIdx.x;
  const uint32_t w = q < words ? owner_role_word(role, q, n) : 0u;
  const uint32_t mine = (uint32_t)__popc(w & 0x01010101u);
  uint32_t total = 0;
  const uint32_t incl = owner_block_scan(mine, lds, &total);
  if (q >= words) { return; }
  const unsigned long long heavy = base[tiles];
  unsigned long long h = base[blockIdx.x] + (incl - mine);
  uint32_t four = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) {
    uint32_t o = kOwnerLight;
    if (((w >> (8u * j)) & 1u) != 0u) { o = (uint32_t)(((h + 1ull) * nshards - 1ull) / heavy); ++h; }
    four |= o << (8u * j);
  }
  const uint64_t left = (uint64_t)n - 4u * q;
  if (left >= 4u) { reinterpret_cast<uint32_t *>(owner)[q] = four; }
  else { for (uint32_t j = 0; j < (uint32_t)left; ++j) { owner[4u * q + j] = (uint8_t)(four >> (8u * j)); } }
}

// four amplicons a thread, the tail one by one (as k_light_roles)
__device__ __forceinline__ uint32_t role_of_owner(uint32_t o, uint32_t shard) { return o == kOwnerLight ? 0u : (o == shard ? 1u : 2u); }
__global__ __launch_bounds__(256) void k_roles_from_owners(const uint8_t * __restrict__ owner, uint32_t shard, uint32_t n, uint8_t * __restrict__ role) {
  const uint64_t quads = (uint64_t)n / 4u;
  for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t w = reinterpret_cast<const uint32_t *>(owner)[q];
    uint32_t four = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) { four |= role_of_owner((w >> (8u * j)) & 0xFFu, shard) << (8u * j); }
    reinterpret_cast<uint32_t *>(role)[q] = four;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3u)) {
    const uint64_t a = 4u * quads + threadIdx.x;
    role[a] = (uint8_t)role_of_owner(owner[a], shard);
  }
}

int need_clustering(swa_ctx * ctx, const char * who) {
  if (ctx->res.cluster_ready && ctx->res.csr_ready) { return SWA_OK; }
  return swa_fail_msg(ctx, SWA_E_ARG, std::string(who) + ": no clustering in place (swa_d1_cluster_device)");
}

int ensure_swarm_sums(swa_ctx * ctx) {
  if (ctx->res.fast.sums_ready) { return SWA_OK; }
  const uint32_t n = ctx->db.n, w = ctx->res.cluster_nswarms;
  SWA_TRY(swa_reserve(ctx, ctx->d_swarm_sums, (uint64_t)w * 24 + 64));
  SWA_HIP(ctx, hipMemsetAsync(ctx->d_swarm_sums.ptr, 0, (uint64_t)w * 24, ctx->stream));
  const ClusterView cv = cluster_view(ctx);
  hipLaunchKernelGGL(k_swarm_sums, dim3(blocks_for(ctx, n)), dim3(256), 0, ctx->stream, cv.order, cv.sid, cv.gen, cv.begins,
                     ctx->db.abundance, ctx->db.seqlen, n, swarm_sums(ctx));
  SWA_HIP(ctx, hipGetLastError());
  ctx->res.fast.sums_ready = true;
  return SWA_OK;
}

}  // namespace

// mass, total length, singletons and deepest generation of every swarm of the clustering in place (src/algod1.cc:1232-1257
// keeps them while it clusters), left in HBM; any output may be null
extern "C" int swa_d1_swarm_sums_device(swa_ctx * ctx, uint64_t * mass, uint64_t * sumlen, uint32_t * singletons, uint32_t * maxgen,
                                        uint32_t nswarms) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  SWA_TRY(need_clustering(ctx, "swa_d1_swarm_sums_device"));
  const uint32_t w = ctx->res.cluster_nswarms;
  const bool wanted = mass != nullptr || sumlen != nullptr || singletons != nullptr || maxgen != nullptr;
  if (wanted && nswarms < w) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_swarm_sums_device: the arrays hold fewer entries than there are swarms"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(ensure_swarm_sums(ctx));
  if (!wanted) { return SWA_OK; }
  const SwarmSums s = swarm_sums(ctx);
  if (mass != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(mass, s.mass, (uint64_t)w * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream)); }
  if (sumlen != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(sumlen, s.sumlen, (uint64_t)w * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream)); }
  if (singletons != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(singletons, s.singles, (uint64_t)w * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream)); }
  if (maxgen != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(maxgen, s.maxgen, (uint64_t)w * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream)); }
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

// src/algod1.cc:1291-1328 on the device: the role byte of every amplicon stays in HBM for swa_d1_fastidious_resident
extern "C" int swa_d1_light_flags_device(swa_ctx * ctx, uint64_t boundary, uint8_t * is_light, uint64_t stats5[5]) {
  if (ctx == nullptr || stats5 == nullptr) { return SWA_E_ARG; }
  SWA_TRY(need_clustering(ctx, "swa_d1_light_flags_device"));
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  ctx->res.fast.roles_ready = false;
  ctx->res.fast.owners_ready = false;                       // (owner bytes are made from the role bytes that are replaced here)
  SWA_TRY(ensure_swarm_sums(ctx));
  const uint32_t n = ctx->db.n, w = ctx->res.cluster_nswarms;
  SWA_TRY(swa_reserve(ctx, ctx->d_swarm_role, (uint64_t)n + 4));
  SWA_TRY(swa_reserve(ctx, ctx->d_graft_work, kCtlWords * sizeof(uint64_t)));
  auto * ctl = static_cast<unsigned long long *>(ctx->d_graft_work.ptr);
  auto * role = static_cast<uint8_t *>(ctx->d_swarm_role.ptr);
  const ClusterView cv = cluster_view(ctx);
  const SwarmSums s = swarm_sums(ctx);
  SWA_HIP(ctx, hipMemsetAsync(ctl, 0, kCtlWords * sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(k_light_roles, dim3(blocks_for(ctx, n / 4u + 1u)), dim3(256), 0, ctx->stream, cv.sid, s.mass, (unsigned long long)boundary, n, role);
  hipLaunchKernelGGL(k_light_stats, dim3(blocks_for(ctx, w)), dim3(256), 0, ctx->stream, s.mass, s.sumlen, cv.begins, (unsigned long long)boundary, w, ctl);
  SWA_HIP(ctx, hipGetLastError());
  uint64_t host[3] = {};
  SWA_HIP(ctx, hipMemcpyAsync(host, ctl, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
  if (is_light != nullptr) {
    swa_touch_pages(is_light, n);
    SWA_HIP(ctx, hipMemcpyAsync(is_light, role, n, hipMemcpyDeviceToHost, ctx->stream));
  }
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (is_light != nullptr) { for (uint32_t a = 0; a < n; ++a) { is_light[a] ^= 1; } }   // (the role byte is 0 for light: the caller's flag is the other way round)
  stats5[0] = host[kCtlLightSwarms]; stats5[1] = host[kCtlLightAmps]; stats5[2] = host[kCtlLightNt];
  stats5[3] = w - host[kCtlLightSwarms]; stats5[4] = n - host[kCtlLightAmps];
  ctx->res.fast.roles_ready = true;
  ctx->res.fast.light_amps = host[kCtlLightAmps];
  return SWA_OK;
}

// the candidates in HBM (after swa_d1_graft_device: with the losers' withdrawn), n entries
extern "C" int swa_d1_graft_candidates_fetch(swa_ctx * ctx, uint32_t * graft_cand) {
  if (ctx == nullptr || graft_cand == nullptr) { return SWA_E_ARG; }
  SWA_TRY(need_clustering(ctx, "swa_d1_graft_candidates_fetch"));
  if (!ctx->res.fast.cand_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_graft_candidates_fetch: no candidates in place (swa_d1_fastidious*, swa_d1_graft_device)"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  swa_touch_pages(graft_cand, (uint64_t)ctx->db.n * sizeof(uint32_t));
  SWA_HIP(ctx, hipMemcpyAsync(graft_cand, ctx->d_graft.ptr, (uint64_t)ctx->db.n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

// attach_candidates (src/algod1.cc:214-336) on the device: G grafts in chain order
extern "C" int swa_d1_graft_device(swa_ctx * ctx, const uint32_t * graft_cand, uint32_t * heavy_swarm, uint32_t * light_swarm,
                                   uint32_t * parent, uint32_t * child, uint32_t cap, uint32_t * grafts) {
  if (ctx == nullptr || grafts == nullptr) { return SWA_E_ARG; }
  *grafts = 0;
  SWA_TRY(need_clustering(ctx, "swa_d1_graft_device"));
  const uint32_t n = ctx->db.n, w = ctx->res.cluster_nswarms;
  if (graft_cand == nullptr && !ctx->res.fast.cand_ready) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_graft_device: no candidates in place (swa_d1_fastidious_resident, swa_d1_fastidious)");
  }
  if (graft_cand != nullptr) {                               // (a caller's candidates index the kernels' arrays: checked before anything is copied)
    for (uint32_t a = 0; a < n; ++a) {
      if (graft_cand[a] != SWA_NO_AMPLICON && graft_cand[a] >= n) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_graft_device: a candidate is not an amplicon of the database"); }
    }
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  if (ctx->res.fast.sums_grafted) { ctx->res.fast.sums_ready = false; ctx->res.fast.sums_grafted = false; }   // (every call grows the swarms' own sums)
  SWA_TRY(ensure_swarm_sums(ctx));
  SWA_TRY(swa_reserve(ctx, ctx->d_graft, (uint64_t)n * sizeof(uint32_t)));
  ctx->dr = {};                                             // (d_graft: candidates from here on, no dereplication's array)
  SWA_TRY(swa_reserve(ctx, ctx->d_graft_work, kCtlWords * sizeof(uint64_t) + (uint64_t)w * 32));
  auto * ctl = static_cast<unsigned long long *>(ctx->d_graft_work.ptr);
  auto * slot = ctl + kCtlWords, * pairs0 = slot + w, * pairs1 = pairs0 + w;
  auto * heavy0 = reinterpret_cast<uint32_t *>(pairs1 + w), * heavy1 = heavy0 + w;
  auto * cand = static_cast<uint32_t *>(ctx->d_graft.ptr);
  const uint32_t pair_bits = 32u + std::max(1u, bit_width_u32(n - 1u)), heavy_bits = std::max(1u, bit_width_u32(w - 1u));
  size_t tmp_bytes = 0, need = 0;
  (void)rocprim::radix_sort_pairs(nullptr, need, pairs0, pairs1, heavy0, heavy1, (size_t)w, 0, pair_bits, ctx->stream);
  tmp_bytes = std::max(tmp_bytes, need);
  (void)rocprim::radix_sort_pairs(nullptr, need, heavy1, heavy0, pairs1, pairs0, (size_t)w, 0, heavy_bits, ctx->stream);
  tmp_bytes = std::max(tmp_bytes, need);
  SWA_TRY(swa_reserve(ctx, ctx->d_scan_hits, tmp_bytes + 16));
  if (graft_cand != nullptr) {
    ctx->res.fast.cand_ready = false;
    SWA_HIP(ctx, hipMemcpyAsync(cand, graft_cand, (uint64_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  const ClusterView cv = cluster_view(ctx);
  const dim3 g(blocks_for(ctx, n)), b(256);
  SWA_HIP(ctx, hipMemsetAsync(ctl + kCtlWinners, 0, sizeof(uint64_t), ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(slot, 0xFF, (uint64_t)w * sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(k_graft_min, g, b, 0, ctx->stream, cand, cv.sid, n, slot);
  hipLaunchKernelGGL(k_graft_winners, g, b, 0, ctx->stream, cand, cv.sid, n, slot, pairs0, heavy0, ctl);
  SWA_HIP(ctx, hipGetLastError());
  uint64_t winners = 0;
  SWA_HIP(ctx, hipMemcpyAsync(&winners, ctl + kCtlWinners, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));           // (the caller's candidates are free again, too)
  ctx->res.fast.cand_ready = true;
  const uint32_t made = (uint32_t)winners;
  *grafts = made;
  if (made == 0) { return SWA_OK; }
  const bool wanted = heavy_swarm != nullptr || light_swarm != nullptr || parent != nullptr || child != nullptr;
  // (before the sums grow: the call with room starts from the same candidates — the winners keep theirs — and the same sums)
  if (wanted && made > cap) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_graft_device: result arrays too small"); }
  need = tmp_bytes;
  SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, need, pairs0, pairs1, heavy0, heavy1, (size_t)made, 0, pair_bits, ctx->stream));
  need = tmp_bytes;
  SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, need, heavy1, heavy0, pairs1, pairs0, (size_t)made, 0, heavy_bits, ctx->stream));
  // the sorted winners lie in heavy0 / pairs0; light swarm -> heavy1, parent | child -> the two halves of pairs1
  auto * light_d = heavy1, * parent_d = reinterpret_cast<uint32_t *>(pairs1), * child_d = parent_d + w;
  hipLaunchKernelGGL(k_graft_apply, dim3(blocks_for(ctx, made)), b, 0, ctx->stream, heavy0, pairs0, cv.sid, made, light_d, parent_d, child_d, swarm_sums(ctx));
  SWA_HIP(ctx, hipGetLastError());
  ctx->res.fast.sums_grafted = true;
  const uint64_t bytes = (uint64_t)made * sizeof(uint32_t);
  if (heavy_swarm != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(heavy_swarm, heavy0, bytes, hipMemcpyDeviceToHost, ctx->stream)); }
  if (light_swarm != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(light_swarm, light_d, bytes, hipMemcpyDeviceToHost, ctx->stream)); }
  if (parent != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(parent, parent_d, bytes, hipMemcpyDeviceToHost, ctx->stream)); }
  if (child != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(child, child_d, bytes, hipMemcpyDeviceToHost, ctx->stream)); }
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

// ---- shard owners ------------------------------------------------------------------------------------------------------
// owner(h) of the h-th of `heavy` heavy amplicons among nshards shards: the shard whose slice [floor(heavy s / nshards),
// floor(heavy (s + 1) / nshards)) holds h — the slices of swa_d1_fastidious_shard — in closed form; no device
extern "C" int swa_d1_shard_owner_for(uint64_t heavy, uint32_t nshards, uint64_t h, uint32_t * owner) {
  if (owner == nullptr || nshards < 1 || nshards > 64 || heavy > 0xFFFFFFFFull || h >= heavy) { return SWA_E_ARG; }
  *owner = (uint32_t)(((h + 1ull) * nshards - 1ull) / heavy);
  return SWA_OK;
}

// {amplicons per tile of the owner kernels, tiles per turn of the scan of their counts}
extern "C" int swa_d1_shard_owner_plan(uint32_t out[2]) {
  if (out == nullptr) { return SWA_E_ARG; }
  out[0] = kOwnerTile; out[1] = kOwnerTurn;
  return SWA_OK;
}

// The owner byte of every amplicon — 255 light, else the shard (of nshards) that expands it — from the role bytes of the last
// swa_d1_light_flags_device call; left in HBM (d_shard_owner).  owners: n bytes on the host, or null; *heavy = H.
extern "C" int swa_d1_shard_owners_device(swa_ctx * ctx, uint32_t nshards, uint8_t * owners, uint64_t * heavy) {
  if (ctx == nullptr || heavy == nullptr) { return SWA_E_ARG; }
  SWA_TRY(need_clustering(ctx, "swa_d1_shard_owners_device"));
  if (!ctx->res.fast.roles_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_shard_owners_device: call swa_d1_light_flags_device first"); }
  if (nshards < 1 || nshards > 64) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_shard_owners_device: 1 to 64 shards"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  ctx->res.fast.owners_ready = false;
  const uint32_t n = ctx->db.n;
  const uint64_t words = ((uint64_t)n + 3u) / 4u, tiles = (words + kOwnerBlock - 1u) / kOwnerBlock;
  const uint64_t owner_bytes = ((uint64_t)n + 4u + 7u) & ~uint64_t(7);
  SWA_TRY(swa_reserve(ctx, ctx->d_shard_owner, owner_bytes + (tiles + 1u) * sizeof(uint64_t) + tiles * sizeof(uint32_t)));
  auto * owner = static_cast<uint8_t *>(ctx->d_shard_owner.ptr);
  auto * base = reinterpret_cast<unsigned long long *>(owner + owner_bytes);
  auto * counts = reinterpret_cast<uint32_t *>(base + tiles + 1u);
  const auto * role = static_cast<const uint8_t *>(ctx->d_swarm_role.ptr);
  hipLaunchKernelGGL(k_owner_counts, dim3((uint32_t)tiles), dim3(kOwnerBlock), 0, ctx->stream, role, n, counts);
  hipLaunchKernelGGL(k_owner_scan, dim3(1), dim3(kOwnerTurn), 0, ctx->stream, counts, (uint32_t)tiles, base);
  hipLaunchKernelGGL(k_owner_write, dim3((uint32_t)tiles), dim3(kOwnerBlock), 0, ctx->stream, role, n, base, (uint32_t)tiles, nshards, owner);
  SWA_HIP(ctx, hipGetLastError());
  uint64_t h = 0;
  SWA_HIP(ctx, hipMemcpyAsync(&h, base + tiles, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  if (owners != nullptr) {
    swa_touch_pages(owners, n);
    SWA_HIP(ctx, hipMemcpyAsync(owners, owner, n, hipMemcpyDeviceToHost, ctx->stream));
  }
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *heavy = h;
  ctx->res.fast.owners_ready = true;
  ctx->res.fast.owners_shards = nshards;
  ctx->res.fast.owners_heavy = h;
  return SWA_OK;
}

int swa_d1_roles_from_owners(swa_ctx * ctx, const uint8_t * d_owner, uint32_t shard, uint8_t * d_role) {
  const uint32_t n = ctx->db.n;
  hipLaunchKernelGGL(k_roles_from_owners, dim3(blocks_for(ctx, n / 4u + 1u)), dim3(256), 0, ctx->stream, d_owner, shard, n, d_role);
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}
