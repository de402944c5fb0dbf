// fast_graft.inc — the bookkeeping of --fastidious on the clustering that swa_d1_cluster_device left in HBM; included at the
// end of cluster_gpu.hip (one code object with the agglomeration: nothing more to load for a run that takes this route).
//
// The reference keeps this on the host, between and after its two fastidious passes (src/algod1.cc:1291-1328: mass per
// swarm, light / heavy; :214-336: attach_candidates).  Everything it reads is in HBM already — d_cluster (swarm of every
// amplicon, generation, member order, bounds), the database (abundance, length), d_graft (the candidates) — so it is done
// there, and a plain `-f -o` run downloads none of those arrays:
//
//   k_swarm_sums      mass, length, singletons, deepest generation of every swarm: swa_wave_run_reduce over the member order
//   k_light_roles     role[a] = mass[sid[a]] < boundary ? 0 : 1, the byte the fastidious pass reads; k_light_stats the five
//                     numbers of the log, reduced per wave
//   k_owner_counts, k_owner_scan, k_owner_write   the owner byte of every amplicon (255 light, else the shard of a run on several
//                     GPUs that expands this heavy amplicon) from the role bytes: an exclusive count of the heavy ones
//   k_graft_min       slot[swarm of the child] = min(parent << 32 | child) over the candidates: what the sequential walk
//                     over the sorted pairs decides (cluster_d1.cpp: graft_sorted_pairs_in_parallel) without the walk
//   k_graft_winners   the winners compacted, the losers' candidates withdrawn
//   rocPRIM           winners by (heavy swarm, pair): a radix sort on the pair, a stable one on the heavy swarm's bits
//   k_graft_apply     light swarm / parent / child of every graft in chain order; the heavy swarms' sums grown by their
//                     lights', a wave's run of one heavy swarm reduced first in the same way
//   k_layout_grafts   the grafted clustering as one layout (swa_d1_graft_layout_device), from those arrays: the light swarms
//                     marked attached, their sizes in chain order, where every heavy swarm's run of grafts begins and ends
//   rocPRIM           an exclusive scan of those sizes (E)
//   k_layout_grown    grown[s] = own[s] + E[end of its run] - E[start of it]; the largest printed swarm
//   rocPRIM           an exclusive scan of the printed swarms' grown sizes: where each begins in the printed order
//   k_layout_lights   where every light swarm begins: behind its heavy swarm's own members and the lights before it in the chain
//   k_layout_move     printed_order[new_begin[swarm] + place in the swarm] = member, one thread a member position
// Integer sums, minima and maxima only: every result is independent of scheduling.

namespace {

// d_swarm_sums, w = swarms of the clustering in place; one fill clears all four arrays (`all`)
struct SwarmSums {
  unsigned long long * mass, * sumlen; uint32_t * singles, * maxgen; swa_extent all;
  void lay(swa_carver & c, uint64_t w) { c.take(w, mass, sumlen, singles, maxgen); all = c.extent(mass); c.spare(64); }
};

// d_graft_work: the control words, then — w entries each — the slot of every swarm and the winners' (pair, heavy swarm) lists twice
// over, for the sorts; k_graft_apply's results go where the sorts are done with: light swarms -> heavy[1], parents | children -> pairs[1]
struct GraftCounters { unsigned long long light_swarms, light_amps, light_nt, winners, pad[4]; };
struct GraftWork {
  GraftCounters * ctl;
  unsigned long long * slot, * pairs[2];
  uint32_t * heavy[2], * light_out, * parent_out, * child_out;
  void lay(swa_carver & c, uint64_t w) {
    c.take(1, ctl);
    c.take(w, slot, pairs[0], pairs[1], heavy[0], heavy[1]);
    light_out = heavy[1]; parent_out = reinterpret_cast<uint32_t *>(pairs[1]); child_out = parent_out + w;
  }
};

// the sums of a run of one swarm (swa_wave_run_reduce, swa_internal.h): k_graft_apply leaves the deepest generation alone
struct GraftRun {
  unsigned long long mass, len; uint32_t singles;
  __device__ __forceinline__ GraftRun shfl_up(uint32_t d) const { return GraftRun{swa_shfl_up_u64(mass, d), swa_shfl_up_u64(len, d), __shfl_up(singles, d, 64)}; }
  __device__ __forceinline__ void absorb(const GraftRun & o) { mass += o.mass; len += o.len; singles += o.singles; }
};
struct SumsRun {
  GraftRun sums; uint32_t maxgen;
  __device__ __forceinline__ SumsRun shfl_up(uint32_t d) const { return SumsRun{sums.shfl_up(d), __shfl_up(maxgen, d, 64)}; }
  __device__ __forceinline__ void absorb(const SumsRun & o) { sums.absorb(o.sums); maxgen = o.maxgen > maxgen ? o.maxgen : maxgen; }
};

__global__ __launch_bounds__(256) void k_swarm_sums(const uint32_t * __restrict__ order, const uint32_t * __restrict__ sid,
                                                    const uint32_t * __restrict__ gen, const uint32_t * __restrict__ begins,
                                                    const uint64_t * __restrict__ abundance, const uint32_t * __restrict__ seqlen, uint32_t n,
                                                    SwarmSums out) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < swa_wave_span(n); k += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t s = kUnset;                                      // (beyond the order: a run of its own that writes nothing)
    SumsRun r{{0, 0, 0}, 0};
    if (k < n) {
      const uint32_t a = order[k];
      s = sid[a]; r.sums.mass = abundance[a]; r.sums.len = seqlen[a]; r.sums.singles = r.sums.mass == 1ull ? 1u : 0u; r.maxgen = gen[a];
    }
    const swa_run run = swa_wave_run_reduce(s, r);
    if (k >= n || !run.last) { continue; }
    // the run [k + 1 - length, k] is the whole swarm: nobody else writes its sums (they were cleared before the launch)
    if ((uint32_t)k + 1u - run.length == begins[s] && (uint32_t)k + 1u == begins[s + 1u]) {
      out.mass[s] = r.sums.mass; out.sumlen[s] = r.sums.len; out.singles[s] = r.sums.singles; out.maxgen[s] = r.maxgen;
    } else {
      atomicAdd(&out.mass[s], r.sums.mass); atomicAdd(&out.sumlen[s], r.sums.len); atomicAdd(&out.singles[s], r.sums.singles); atomicMax(&out.maxgen[s], r.maxgen);
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

// ctl->light_swarms, light_amps, light_nt += light swarms, their amplicons (sizes from the bounds), their nucleotides
__global__ __launch_bounds__(256) void k_light_stats(const unsigned long long * __restrict__ mass, const unsigned long long * __restrict__ sumlen,
                                                     const uint32_t * __restrict__ begins, unsigned long long boundary, uint32_t nswarms,
                                                     GraftCounters * ctl) {
  unsigned long long swarms = 0, amps = 0, nt = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nswarms; s += (uint64_t)gridDim.x * blockDim.x) {
    if (mass[s] < boundary) { ++swarms; amps += begins[s + 1u] - begins[s]; nt += sumlen[s]; }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    swarms += swa_shfl_xor_u64(swarms, d); amps += swa_shfl_xor_u64(amps, d); nt += swa_shfl_xor_u64(nt, d);
  }
  if ((threadIdx.x & 63u) == 0u && swarms != 0ull) {
    atomicAdd(&ctl->light_swarms, swarms); atomicAdd(&ctl->light_amps, amps); atomicAdd(&ctl->light_nt, nt);
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
                                                       uint32_t * __restrict__ heavy, GraftCounters * ctl) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; a < swa_wave_span(n); a += (uint64_t)gridDim.x * blockDim.x) {
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
    if (lane == 0u) { base = atomicAdd(&ctl->winners, (unsigned long long)__popcll(mask)); }
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
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < swa_wave_span(grafts); i += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t h = kUnset;
    GraftRun r{0, 0, 0};
    if (i < grafts) {
      const unsigned long long pair = pairs[i];
      const uint32_t child = (uint32_t)pair, l = sid[child];
      h = heavy[i];
      light_out[i] = l; parent_out[i] = (uint32_t)(pair >> 32); child_out[i] = child;
      r.mass = sums.mass[l]; r.len = sums.sumlen[l]; r.singles = sums.singles[l];   // (a light swarm is nobody's heavy swarm: its sums stand still)
    }
    const swa_run run = swa_wave_run_reduce(h, r);            // (every lane takes part)
    if (i >= grafts || !run.last) { continue; }
    atomicAdd(&sums.mass[h], r.mass); atomicAdd(&sums.sumlen[h], r.len); atomicAdd(&sums.singles[h], r.singles);   // (maxgen untouched, like the reference)
  }
}

// ---- the grafted clustering as one layout -----------------------------------------------------------------------------------
// The chain a heavy swarm's light swarms form says in which order the members are printed: a permutation of the member order,
// fixed by the grafts in chain order (heavy[0], light_out).  With own[s] = begins[s + 1] - begins[s] and E the exclusive scan of
// own[light[i]] over the grafts (E[G] = their total):
//   grown[h]            = own[h] + E[end of h's run of grafts] - E[start of it]       (a swarm without grafts: own[h])
//   new_begin[printed]  = the exclusive scan over the swarms of (attached ? 0 : grown)
//   new_begin[light[i]] = new_begin[h] + own[h] + E[i] - E[start of h's run]          (h = heavy[i])
//   printed_order[new_begin[s] + k - begins[s]] = order[k]                            (s = swarm of the member at position k)
// d_graft_layout, w swarms of n amplicons; n and the scans' room are set before lay() runs.  rocPRIM's room comes first (it has
// the buffer's own alignment); one fill clears the runs' bounds, the largest printed swarm and the attached bytes (`cleared`).
struct GraftLayout {
  uint64_t n = 0, tmp_bytes = 0;
  unsigned long long * tmp = nullptr;
  uint32_t * printed_order = nullptr, * new_begin = nullptr, * grown = nullptr, * scan_in = nullptr, * sizes = nullptr, * ends = nullptr;
  uint32_t * run_first = nullptr, * run_end = nullptr, * largest = nullptr;
  uint8_t * attached = nullptr;
  swa_extent cleared{nullptr, 0};
  void lay(swa_carver & c, uint64_t w) {
    c.take((tmp_bytes + 7u) / 8u, tmp);
    c.take(n, printed_order);
    c.take(w, new_begin, grown, scan_in);
    c.take(w + 1u, sizes, ends);                             // (entry G of the sizes is 0: ends[G] = the total)
    c.take(w, run_first, run_end);
    c.take(1, largest);
    c.take(w, attached);
    cleared = c.extent(run_first);
    c.spare(64);
  }
};

// graft i hangs light swarm light[i] on heavy[i]; the grafts of one heavy swarm are a run [run_first, run_end) of the arrays
// (both 0 for a swarm without one: cleared before the launch).  Position G closes the sizes.
__global__ __launch_bounds__(256) void k_layout_grafts(const uint32_t * __restrict__ heavy, const uint32_t * __restrict__ light,
                                                       const uint32_t * __restrict__ begins, uint32_t grafts, GraftLayout out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= grafts; i += (uint64_t)gridDim.x * blockDim.x) {
    if (i == grafts) { out.sizes[i] = 0; continue; }
    const uint32_t h = heavy[i], l = light[i];
    out.attached[l] = 1;
    out.sizes[i] = begins[l + 1u] - begins[l];
    if (i == 0 || heavy[i - 1u] != h) { out.run_first[h] = (uint32_t)i; }
    if (i + 1u == grafts || heavy[i + 1u] != h) { out.run_end[h] = (uint32_t)i + 1u; }
  }
}

// grown[s], what the scan over the printed swarms adds up, and *largest = the most members a printed swarm has (a maximum a wave)
__global__ __launch_bounds__(256) void k_layout_grown(const uint32_t * __restrict__ begins, uint32_t nswarms, GraftLayout out) {
  uint32_t most = 0;
  for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < nswarms; s += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t g = begins[s + 1u] - begins[s] + out.ends[out.run_end[s]] - out.ends[out.run_first[s]];
    const uint32_t printed = out.attached[s] != 0 ? 0u : g;
    out.grown[s] = g;
    out.scan_in[s] = printed;
    most = printed > most ? printed : most;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t other = __shfl_xor(most, d, 64);
    most = other > most ? other : most;
  }
  if ((threadIdx.x & 63u) == 0u && most != 0u) { atomicMax(out.largest, most); }
}

// (new_begin of a heavy swarm is read, that of its light swarms written: no light swarm is anybody's heavy swarm)
__global__ __launch_bounds__(256) void k_layout_lights(const uint32_t * __restrict__ heavy, const uint32_t * __restrict__ light,
                                                       const uint32_t * __restrict__ begins, uint32_t grafts, GraftLayout out) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < grafts; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t h = heavy[i];
    out.new_begin[light[i]] = out.new_begin[h] + (begins[h + 1u] - begins[h]) + out.ends[i] - out.ends[out.run_first[h]];
  }
}

// one thread a member position: coalesced reads of the order, an even load whatever the swarms' sizes
__global__ __launch_bounds__(256) void k_layout_move(const uint32_t * __restrict__ order, const uint32_t * __restrict__ sid,
                                                     const uint32_t * __restrict__ begins, const uint32_t * __restrict__ new_begin, uint32_t n,
                                                     uint32_t * __restrict__ printed_order) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = order[k], s = sid[a];
    const uint32_t at = new_begin[s] + ((uint32_t)k - begins[s]);
    // (always so for grafts as swa_d1_graft_device makes them from light children and heavy parents; a caller's candidates
    // that hang a swarm on a swarm that hangs itself lay nothing sensible out, and write nowhere else)
    if (at < n) { printed_order[at] = a; }
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

// d_shard_owner on the rank that makes the owners, n amplicons: the owner bytes (four to spare: the kernels store whole
// words), the bases of the tiles and of the end, the tiles' counts.  The other ranks of a swa_multi hold the owner bytes alone.
uint64_t owner_tiles(uint64_t n) { return ((n + 3u) / 4u + kOwnerBlock - 1u) / kOwnerBlock; }
struct ShardOwners {
  uint8_t * owner; unsigned long long * base; uint32_t * counts;
  void lay(swa_carver & c, uint64_t n) { c.take(n + 4u, owner); c.take(owner_tiles(n) + 1u, base); c.take(owner_tiles(n), counts); }
};

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

// the arrays of the clustering in place / the sums of its swarms (made on first use: `s` is valid on return)
int cluster_arrays(swa_ctx * ctx, swa_cluster_arrays & cl) { return swa_carve(ctx, ctx->d_cluster, ctx->db.n, false, cl); }

int ensure_swarm_sums(swa_ctx * ctx, SwarmSums & s) {
  const uint32_t n = ctx->db.n, w = ctx->res.cluster_nswarms;
  SWA_TRY(swa_carve(ctx, ctx->d_swarm_sums, w, !ctx->res.fast.sums_ready, s));
  if (ctx->res.fast.sums_ready) { return SWA_OK; }
  swa_cluster_arrays cl;
  SWA_TRY(cluster_arrays(ctx, cl));
  SWA_HIP(ctx, hipMemsetAsync(s.all.ptr, 0, s.all.bytes, ctx->stream));
  hipLaunchKernelGGL(k_swarm_sums, dim3(swa_grid256(ctx, n)), dim3(256), 0, ctx->stream, cl.order, cl.swarmid, cl.gen, cl.begins,
                     ctx->db.abundance, ctx->db.seqlen, n, s);
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
  SwarmSums s;
  SWA_TRY(ensure_swarm_sums(ctx, s));
  if (!wanted) { return SWA_OK; }
  const uint64_t w8 = (uint64_t)w * sizeof(uint64_t), w4 = (uint64_t)w * sizeof(uint32_t);
  return swa_download(ctx, {{mass, s.mass, w8}, {sumlen, s.sumlen, w8}, {singletons, s.singles, w4}, {maxgen, s.maxgen, w4}});
}

// src/algod1.cc:1291-1328 on the device: the role byte of every amplicon stays in HBM for swa_d1_fastidious_resident
extern "C" int swa_d1_light_flags_device(swa_ctx * ctx, uint64_t boundary, uint8_t * is_light, uint64_t stats5[5]) {
  if (ctx == nullptr || stats5 == nullptr) { return SWA_E_ARG; }
  SWA_TRY(need_clustering(ctx, "swa_d1_light_flags_device"));
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  ctx->res.fast.roles_ready = false;
  ctx->res.fast.owners_ready = false;                       // (owner bytes are made from the role bytes that are replaced here)
  SwarmSums s;
  SWA_TRY(ensure_swarm_sums(ctx, s));
  const uint32_t n = ctx->db.n, w = ctx->res.cluster_nswarms;
  SWA_TRY(swa_reserve(ctx, ctx->d_swarm_role, (uint64_t)n + 4));
  GraftWork gw;                                             // (the control words alone: no array of it is used here)
  SWA_TRY(swa_carve(ctx, ctx->d_graft_work, 0, true, gw));
  auto * role = static_cast<uint8_t *>(ctx->d_swarm_role.ptr);
  swa_cluster_arrays cl;
  SWA_TRY(cluster_arrays(ctx, cl));
  SWA_HIP(ctx, hipMemsetAsync(gw.ctl, 0, sizeof(GraftCounters), ctx->stream));
  hipLaunchKernelGGL(k_light_roles, dim3(swa_grid256(ctx, n / 4u + 1u)), dim3(256), 0, ctx->stream, cl.swarmid, s.mass, (unsigned long long)boundary, n, role);
  hipLaunchKernelGGL(k_light_stats, dim3(swa_grid256(ctx, w)), dim3(256), 0, ctx->stream, s.mass, s.sumlen, cl.begins, (unsigned long long)boundary, w, gw.ctl);
  SWA_HIP(ctx, hipGetLastError());
  GraftCounters host = {};
  SWA_TRY(swa_download(ctx, {{&host, gw.ctl, offsetof(GraftCounters, winners)}, {is_light, role, n}}));
  if (is_light != nullptr) { for (uint32_t a = 0; a < n; ++a) { is_light[a] ^= 1; } }   // (the role byte is 0 for light: the caller's flag is the other way round)
  stats5[0] = host.light_swarms; stats5[1] = host.light_amps; stats5[2] = host.light_nt;
  stats5[3] = w - host.light_swarms; stats5[4] = n - host.light_amps;
  ctx->res.fast.roles_ready = true;
  ctx->res.fast.light_amps = host.light_amps;
  return SWA_OK;
}

// the candidates in HBM (after swa_d1_graft_device: with the losers' withdrawn), n entries
extern "C" int swa_d1_graft_candidates_fetch(swa_ctx * ctx, uint32_t * graft_cand) {
  if (ctx == nullptr || graft_cand == nullptr) { return SWA_E_ARG; }
  SWA_TRY(need_clustering(ctx, "swa_d1_graft_candidates_fetch"));
  if (!ctx->res.fast.cand_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_graft_candidates_fetch: no candidates in place (swa_d1_fastidious*, swa_d1_graft_device)"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  return swa_download(ctx, {{graft_cand, ctx->d_graft.ptr, (uint64_t)ctx->db.n * sizeof(uint32_t)}});
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
  ctx->res.fast.grafts_ready = false;                       // (the grafts of the call before, and their layout, end here)
  ctx->res.fast.layout_ready = false;
  if (ctx->res.fast.sums_grafted) { ctx->res.fast.sums_ready = false; ctx->res.fast.sums_grafted = false; }   // (every call grows the swarms' own sums)
  SwarmSums sums;
  SWA_TRY(ensure_swarm_sums(ctx, sums));
  SWA_TRY(swa_reserve(ctx, ctx->d_graft, (uint64_t)n * sizeof(uint32_t)));
  ctx->dr = {};                                             // (d_graft: candidates from here on, no dereplication's array)
  GraftWork gw;
  SWA_TRY(swa_carve(ctx, ctx->d_graft_work, w, true, gw));
  auto * cand = static_cast<uint32_t *>(ctx->d_graft.ptr);
  const uint32_t pair_bits = 32u + std::max(1u, swa_bit_width(n - 1u)), heavy_bits = std::max(1u, swa_bit_width(w - 1u));
  size_t asked[2] = {}, need = 0;
  (void)rocprim::radix_sort_pairs(nullptr, asked[0], gw.pairs[0], gw.pairs[1], gw.heavy[0], gw.heavy[1], (size_t)w, 0, pair_bits, ctx->stream);
  (void)rocprim::radix_sort_pairs(nullptr, asked[1], gw.heavy[1], gw.heavy[0], gw.pairs[1], gw.pairs[0], (size_t)w, 0, heavy_bits, ctx->stream);
  const size_t tmp_bytes = std::max(asked[0], asked[1]);
  SWA_TRY(swa_reserve(ctx, ctx->d_scan_hits, tmp_bytes + 16));
  if (graft_cand != nullptr) {
    ctx->res.fast.candidates_end();
    SWA_HIP(ctx, hipMemcpyAsync(cand, graft_cand, (uint64_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  swa_cluster_arrays cl;
  SWA_TRY(cluster_arrays(ctx, cl));
  const dim3 g(swa_grid256(ctx, n)), b(256);
  SWA_HIP(ctx, hipMemsetAsync(&gw.ctl->winners, 0, sizeof(uint64_t), ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(gw.slot, 0xFF, (uint64_t)w * sizeof(uint64_t), ctx->stream));
  hipLaunchKernelGGL(k_graft_min, g, b, 0, ctx->stream, cand, cl.swarmid, n, gw.slot);
  hipLaunchKernelGGL(k_graft_winners, g, b, 0, ctx->stream, cand, cl.swarmid, n, gw.slot, gw.pairs[0], gw.heavy[0], gw.ctl);
  SWA_HIP(ctx, hipGetLastError());
  uint64_t winners = 0;
  SWA_HIP(ctx, hipMemcpyAsync(&winners, &gw.ctl->winners, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));           // (the caller's candidates are free again, too)
  ctx->res.fast.cand_ready = true;
  const uint32_t made = (uint32_t)winners;
  *grafts = made;
  ctx->res.fast.grafts = made;
  if (made == 0) { ctx->res.fast.grafts_ready = true; return SWA_OK; }
  const bool wanted = heavy_swarm != nullptr || light_swarm != nullptr || parent != nullptr || child != nullptr;
  // (before the sums grow: the call with room starts from the same candidates — the winners keep theirs — and the same sums)
  if (wanted && made > cap) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_graft_device: result arrays too small"); }
  need = tmp_bytes;
  SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, need, gw.pairs[0], gw.pairs[1], gw.heavy[0], gw.heavy[1], (size_t)made, 0, pair_bits, ctx->stream));
  need = tmp_bytes;
  SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, need, gw.heavy[1], gw.heavy[0], gw.pairs[1], gw.pairs[0], (size_t)made, 0, heavy_bits, ctx->stream));
  // the sorted winners lie in gw.heavy[0] / gw.pairs[0]; the results go where GraftWork says
  hipLaunchKernelGGL(k_graft_apply, dim3(swa_grid256(ctx, made)), b, 0, ctx->stream, gw.heavy[0], gw.pairs[0], cl.swarmid, made, gw.light_out, gw.parent_out,
                     gw.child_out, sums);
  SWA_HIP(ctx, hipGetLastError());
  ctx->res.fast.sums_grafted = true;
  ctx->res.fast.grafts_ready = true;                        // (in chain order in d_graft_work: swa_d1_graft_layout_device)
  const uint64_t bytes = (uint64_t)made * sizeof(uint32_t);
  return swa_download(ctx, {{heavy_swarm, gw.heavy[0], bytes}, {light_swarm, gw.light_out, bytes}, {parent, gw.parent_out, bytes}, {child, gw.child_out, bytes}});
}

// The grafted clustering laid out in HBM (GraftLayout above): the member order as the writers print it — every printed swarm's
// own members, then those of the light swarms of its chain, in chain order —, where every swarm's own members begin in it,
// how many members it has with everything grafted, whether it hangs on another.  Needs a completed swa_d1_graft_device (G = 0:
// the layout is the clustering's own); made once, a second call downloads the same arrays.  Any output may be null.
extern "C" int swa_d1_graft_layout_device(swa_ctx * ctx, uint32_t * printed_order, uint32_t * new_begin, uint32_t * grown, uint8_t * attached,
                                          uint32_t nswarms, uint64_t summary3[3]) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  SWA_TRY(need_clustering(ctx, "swa_d1_graft_layout_device"));
  if (!ctx->res.fast.grafts_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_graft_layout_device: no grafts in place (a completed swa_d1_graft_device)"); }
  const uint32_t n = ctx->db.n, w = ctx->res.cluster_nswarms, made = ctx->res.fast.grafts;
  if (nswarms < w) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_graft_layout_device: the arrays hold fewer entries than there are swarms"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  GraftLayout gl;
  gl.n = n;
  size_t asked = 0;                                         // (both scans are of w + 1 entries at most)
  (void)rocprim::exclusive_scan(nullptr, asked, gl.sizes, gl.ends, 0u, (size_t)w + 1u, rocprim::plus<uint32_t>(), ctx->stream);
  gl.tmp_bytes = asked;
  if (!ctx->res.fast.layout_ready) {
    SWA_TRY(swa_carve(ctx, ctx->d_graft_layout, w, true, gl));
    GraftWork gw;
    SWA_TRY(swa_carve(ctx, ctx->d_graft_work, w, false, gw));
    swa_cluster_arrays cl;
    SWA_TRY(cluster_arrays(ctx, cl));
    const dim3 b(256);
    SWA_HIP(ctx, hipMemsetAsync(gl.cleared.ptr, 0, gl.cleared.bytes, ctx->stream));
    hipLaunchKernelGGL(k_layout_grafts, dim3(swa_grid256(ctx, (uint64_t)made + 1u)), b, 0, ctx->stream, gw.heavy[0], gw.light_out, cl.begins, made, gl);
    size_t need = asked;
    SWA_HIP(ctx, rocprim::exclusive_scan(gl.tmp, need, gl.sizes, gl.ends, 0u, (size_t)made + 1u, rocprim::plus<uint32_t>(), ctx->stream));
    hipLaunchKernelGGL(k_layout_grown, dim3(swa_grid256(ctx, w)), b, 0, ctx->stream, cl.begins, w, gl);
    need = asked;
    SWA_HIP(ctx, rocprim::exclusive_scan(gl.tmp, need, gl.scan_in, gl.new_begin, 0u, (size_t)w, rocprim::plus<uint32_t>(), ctx->stream));
    if (made != 0) {
      hipLaunchKernelGGL(k_layout_lights, dim3(swa_grid256(ctx, made)), b, 0, ctx->stream, gw.heavy[0], gw.light_out, cl.begins, made, gl);
    }
    hipLaunchKernelGGL(k_layout_move, dim3(swa_grid256(ctx, n)), b, 0, ctx->stream, cl.order, cl.swarmid, cl.begins, gl.new_begin, n, gl.printed_order);
    SWA_HIP(ctx, hipGetLastError());
    uint32_t largest = 0;
    SWA_TRY(swa_download(ctx, {{&largest, gl.largest, sizeof(largest)}}));
    ctx->res.fast.layout_largest = largest;
    ctx->res.fast.layout_ready = true;
  } else {
    SWA_TRY(swa_carve(ctx, ctx->d_graft_layout, w, false, gl));
  }
  if (summary3 != nullptr) { summary3[0] = w - made; summary3[1] = ctx->res.fast.layout_largest; summary3[2] = made; }
  const uint64_t w4 = (uint64_t)w * sizeof(uint32_t);
  return swa_download(ctx, {{printed_order, gl.printed_order, (uint64_t)n * sizeof(uint32_t)}, {new_begin, gl.new_begin, w4}, {grown, gl.grown, w4}, {attached, gl.attached, w}});
}

// {whether a layout is in place, amplicons and swarms of the clustering it lays out, grafts}; no device
extern "C" int swa_d1_graft_layout_info(const swa_ctx * ctx, uint64_t out4[4]) {
  if (ctx == nullptr || out4 == nullptr) { return SWA_E_ARG; }
  const bool there = ctx->res.cluster_ready && ctx->res.csr_ready && ctx->res.fast.layout_ready;
  out4[0] = there ? 1u : 0u; out4[1] = there ? ctx->db.n : 0u; out4[2] = there ? ctx->res.cluster_nswarms : 0u; out4[3] = there ? ctx->res.fast.grafts : 0u;
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
  ShardOwners so;
  SWA_TRY(swa_carve(ctx, ctx->d_shard_owner, n, true, so));
  const uint64_t tiles = owner_tiles(n);
  const auto * role = static_cast<const uint8_t *>(ctx->d_swarm_role.ptr);
  hipLaunchKernelGGL(k_owner_counts, dim3((uint32_t)tiles), dim3(kOwnerBlock), 0, ctx->stream, role, n, so.counts);
  hipLaunchKernelGGL(k_owner_scan, dim3(1), dim3(kOwnerTurn), 0, ctx->stream, so.counts, (uint32_t)tiles, so.base);
  hipLaunchKernelGGL(k_owner_write, dim3((uint32_t)tiles), dim3(kOwnerBlock), 0, ctx->stream, role, n, so.base, (uint32_t)tiles, nshards, so.owner);
  SWA_HIP(ctx, hipGetLastError());
  uint64_t h = 0;
  SWA_TRY(swa_download(ctx, {{&h, so.base + tiles, sizeof(h)}, {owners, so.owner, n}}));
  *heavy = h;
  ctx->res.fast.owners_ready = true;
  ctx->res.fast.owners_shards = nshards;
  ctx->res.fast.owners_heavy = h;
  return SWA_OK;
}

int swa_d1_roles_from_owners(swa_ctx * ctx, const uint8_t * d_owner, uint32_t shard, uint8_t * d_role) {
  const uint32_t n = ctx->db.n;
  hipLaunchKernelGGL(k_roles_from_owners, dim3(swa_grid256(ctx, n / 4u + 1u)), dim3(256), 0, ctx->stream, d_owner, shard, n, d_role);
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}
