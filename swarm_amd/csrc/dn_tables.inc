// dn_tables.inc — the bookkeeping of the d >= 2 graph route on the clustering that swa_d1_cluster_device left in HBM; included
// at the end of cluster_gpu.hip, behind fast_graft.inc (one code object with the agglomeration: nothing more to load).
//
// cluster_dn.cpp made these tables on the host from five downloaded arrays of n entries (cluster_on_device: radii, per-swarm
// sums, the -i / -u links in acceptance order).  Everything they are made of lies in HBM — d_cluster (generation, parent,
// swarm, member order, bounds), the differences behind the resident graph's links, the abundances — so they are made there,
// and a run that writes the swarms alone downloads the member order, the bounds and four numbers a swarm:
//
//   k_dt_init         diff(parent, v) looked up in the parent's row (swa_row_find, as k_dg_parent_diffs of dn_graph.hip), the
//                     first (ancestor, accumulated differences) pair of every amplicon = (parent, that difference), members
//                     without a link from their parent counted into a control word, pos_of[order[k]] = k
//   k_dt_jump         pointer jumping: (a, r) -> (ancestor of a, r + accumulated of a), from one buffer into the other — a
//                     round reads only what the round before wrote, nobody waits for anybody; a pair whose ancestor has passed
//                     the seed stands still.  bit_width(deepest generation) rounds: radius(v) = the differences summed along
//                     the parent chain up to the seed (src/algo.cc:560-574)
//   k_dt_maxradius    the deepest radius of every swarm: swa_wave_run_reduce (swa_internal.h) along the member order with
//                     k_swarm_sums' rule for the whole swarm; mass, singletons and deepest generation are k_swarm_sums' own
//   k_dt_link_keys    the links of the whole clustering in acceptance order = the non-seed positions k of the member order,
//   rocPRIM           stably sorted by pos_of[parent[order[k]]], k ascending going in (the host's counting sort per swarm:
//   k_dt_link_gather  swarms are contiguous in the order, so one sort groups by swarm; children of one parent share a
//                     generation, so their positions ascend with their ids — tests/test_dn_tables_identity.py); position k of
//                     swarm s is non-seed entry k - s - 1, swarm s owns the links [begins[s] - s, begins[s + 1] - s - 1)
// Integer sums and maxima only: every result is independent of scheduling.

namespace {

constexpr uint32_t kDtCtlBroken = 0, kDtCtlWords = 16;

// d_dn_tables, n amplicons: the control words, then n entries each — the two jumping buffers (ancestor, accumulated), pos_of, sort
// keys and values in / out, the links' parent / child / generation, the swarms' deepest radius, the parents' and the links' differences
struct DnTables {
  uint32_t * ctl, * anc[2], * acc[2], * pos_of, * keys[2], * vals[2], * link_parent, * link_child, * link_gen, * maxradius;
  uint8_t * pdiff, * link_diff;
  void lay(swa_carver & c, uint64_t n) {
    c.take(kDtCtlWords, ctl);
    c.take(n, anc[0], anc[1], acc[0], acc[1], pos_of, keys[0], keys[1], vals[0], vals[1], link_parent, link_child, link_gen, maxradius,
           pdiff, link_diff);
    c.spare(64);
  }
};

// the deepest radius of a run of one swarm (swa_wave_run_reduce, swa_internal.h)
struct RadiusRun {
  uint32_t deepest;
  __device__ __forceinline__ RadiusRun shfl_up(uint32_t d) const { return RadiusRun{__shfl_up(deepest, d, 64)}; }
  __device__ __forceinline__ void absorb(const RadiusRun & o) { deepest = o.deepest > deepest ? o.deepest : deepest; }
};

__global__ __launch_bounds__(256) void k_dt_init(const uint64_t * __restrict__ offsets, const uint32_t * __restrict__ nb,
                                                 const uint8_t * __restrict__ df, const uint32_t * __restrict__ parent,
                                                 const uint32_t * __restrict__ gen, const uint32_t * __restrict__ order, uint32_t n,
                                                 uint32_t * __restrict__ anc, uint32_t * __restrict__ acc, uint8_t * __restrict__ pdiff,
                                                 uint32_t * __restrict__ pos_of, uint32_t * ctl) {
  const uint32_t lane = threadIdx.x & 63u;
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < swa_wave_span(n); k += (uint64_t)gridDim.x * blockDim.x) {
    bool broken = false;
    if (k < n) {
      const uint32_t v = (uint32_t)k, p = parent[v];
      uint32_t d = 0;
      if (p != kUnset) {                                    // (rows ascend strictly: swa_d1_network_adopt, k_dg_split)
        uint64_t at;
        d = swa_row_find(offsets, nb, p, v, at) ? (uint32_t)df[at] : 0xFFu;
      }
      broken = gen[v] != 0u && d == 0xFFu;
      pdiff[v] = (uint8_t)d;
      anc[v] = p;
      acc[v] = d;
      pos_of[order[k]] = (uint32_t)k;
    }
    const unsigned long long mask = __ballot(broken);
    if (mask != 0ull && lane == 0u) { atomicAdd(&ctl[kDtCtlBroken], (uint32_t)__popcll(mask)); }
  }
}

__global__ __launch_bounds__(256) void k_dt_jump(const uint32_t * __restrict__ anc_in, const uint32_t * __restrict__ acc_in, uint32_t n,
                                                 uint32_t * __restrict__ anc_out, uint32_t * __restrict__ acc_out) {
  for (uint64_t v = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n; v += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t a = anc_in[v], r = acc_in[v];
    if (a != kUnset) { r += acc_in[a]; a = anc_in[a]; }
    anc_out[v] = a;
    acc_out[v] = r;
  }
}

__global__ __launch_bounds__(256) void k_dt_maxradius(const uint32_t * __restrict__ order, const uint32_t * __restrict__ sid,
                                                      const uint32_t * __restrict__ radius, const uint32_t * __restrict__ begins, uint32_t n,
                                                      uint32_t * out) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < swa_wave_span(n); k += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t s = kUnset;                                      // (beyond the order: a run of its own that writes nothing)
    RadiusRun r{0};
    if (k < n) {
      const uint32_t a = order[k];
      s = sid[a]; r.deepest = radius[a];
    }
    const swa_run run = swa_wave_run_reduce(s, r);
    if (k >= n || !run.last) { continue; }
    if ((uint32_t)k + 1u - run.length == begins[s] && (uint32_t)k + 1u == begins[s + 1u]) { out[s] = r.deepest; }   // (cleared before the launch)
    else { atomicMax(&out[s], r.deepest); }
  }
}

__global__ __launch_bounds__(256) void k_dt_link_keys(const uint32_t * __restrict__ order, const uint32_t * __restrict__ sid,
                                                      const uint32_t * __restrict__ parent, const uint32_t * __restrict__ pos_of,
                                                      const uint32_t * __restrict__ begins, uint32_t n, uint32_t * __restrict__ keys,
                                                      uint32_t * __restrict__ vals) {
  for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = order[k], s = sid[a];
    if ((uint32_t)k == begins[s]) { continue; }               // (the seed: nobody's child)
    const uint32_t j = (uint32_t)k - s - 1u, p = parent[a];   // (s + 1 seeds stand at or before k)
    keys[j] = p != kUnset ? pos_of[p] : 0u;
    vals[j] = (uint32_t)k;
  }
}

__global__ __launch_bounds__(256) void k_dt_link_gather(const uint32_t * __restrict__ sorted, const uint32_t * __restrict__ order,
                                                        const uint32_t * __restrict__ parent, const uint32_t * __restrict__ gen,
                                                        const uint8_t * __restrict__ pdiff, uint64_t nlinks, uint32_t * __restrict__ link_parent,
                                                        uint32_t * __restrict__ link_child, uint32_t * __restrict__ link_gen,
                                                        uint8_t * __restrict__ link_diff) {
  for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nlinks; j += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = order[sorted[j]];
    link_parent[j] = parent[a]; link_child[j] = a; link_gen[j] = gen[a]; link_diff[j] = pdiff[a];
  }
}

int need_graph_clustering(swa_ctx * ctx, const char * who) {
  SWA_TRY(need_clustering(ctx, who));
  if (ctx->res.csr_has_diffs) { return SWA_OK; }
  return swa_fail_msg(ctx, SWA_E_ARG, std::string(who) + ": the resident network carries no differences (swa_dn_graph_resident, swa_d1_network_adopt with diffs)");
}

}  // namespace

// Radii, the swarms' sums and deepest radii, and the links in acceptance order of the clustering in place, made and left in
// HBM (swa_dn_tables_fetch).  *nswarms / *nlinks (= n - swarms) size the caller's arrays.
extern "C" int swa_dn_tables_device(swa_ctx * ctx, uint32_t * nswarms, uint64_t * nlinks) {
  if (ctx == nullptr || nswarms == nullptr || nlinks == nullptr) { return SWA_E_ARG; }
  *nswarms = 0; *nlinks = 0;
  ctx->res.tables = {};
  if (ctx->db.n == 0) { return SWA_OK; }                      // (nothing to make)
  SWA_TRY(need_graph_clustering(ctx, "swa_dn_tables_device"));
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->db.n, w = ctx->res.cluster_nswarms;
  const uint64_t links = (uint64_t)n - w;
  const uint32_t rounds = swa_bit_width(ctx->res.cluster_maxgen), key_bits = std::max(1u, swa_bit_width(n - 1u));
  SwarmSums sums;
  SWA_TRY(ensure_swarm_sums(ctx, sums));
  DnTables t;
  SWA_TRY(swa_carve(ctx, ctx->d_dn_tables, n, true, t));
  size_t tmp_bytes = 0;
  if (links != 0) {
    (void)rocprim::radix_sort_pairs(nullptr, tmp_bytes, t.keys[0], t.keys[1], t.vals[0], t.vals[1], (size_t)links, 0, key_bits, ctx->stream);
    SWA_TRY(swa_reserve(ctx, ctx->d_scan_hits, tmp_bytes + 16));
  }
  const auto * offsets = static_cast<const uint64_t *>(ctx->d_offsets_tmp.ptr);
  const auto * nb = static_cast<const uint32_t *>(ctx->d_nb_tmp.ptr);
  const auto * df = reinterpret_cast<const uint8_t *>(nb + ctx->res.csr_total);
  swa_cluster_arrays cv;
  SWA_TRY(cluster_arrays(ctx, cv));
  const dim3 g(swa_grid256(ctx, n)), b(256);
  SWA_HIP(ctx, hipMemsetAsync(t.ctl, 0, kDtCtlWords * sizeof(uint32_t), ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(t.maxradius, 0, (uint64_t)w * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_dt_init, g, b, 0, ctx->stream, offsets, nb, df, cv.parent, cv.gen, cv.order, n, t.anc[0], t.acc[0], t.pdiff, t.pos_of, t.ctl);
  for (uint32_t r = 0; r < rounds; ++r) {
    hipLaunchKernelGGL(k_dt_jump, g, b, 0, ctx->stream, t.anc[r & 1u], t.acc[r & 1u], n, t.anc[(r + 1u) & 1u], t.acc[(r + 1u) & 1u]);
  }
  const uint32_t radius_at = rounds & 1u;
  hipLaunchKernelGGL(k_dt_maxradius, g, b, 0, ctx->stream, cv.order, cv.swarmid, t.acc[radius_at], cv.begins, n, t.maxradius);
  if (links != 0) {
    hipLaunchKernelGGL(k_dt_link_keys, g, b, 0, ctx->stream, cv.order, cv.swarmid, cv.parent, t.pos_of, cv.begins, n, t.keys[0], t.vals[0]);
    SWA_HIP(ctx, rocprim::radix_sort_pairs(ctx->d_scan_hits.ptr, tmp_bytes, t.keys[0], t.keys[1], t.vals[0], t.vals[1], (size_t)links, 0, key_bits, ctx->stream));
    hipLaunchKernelGGL(k_dt_link_gather, dim3(swa_grid256(ctx, links)), b, 0, ctx->stream, t.vals[1], cv.order, cv.parent, cv.gen, t.pdiff, links,
                       t.link_parent, t.link_child, t.link_gen, t.link_diff);
  }
  SWA_HIP(ctx, hipGetLastError());
  uint32_t broken = 0;
  SWA_HIP(ctx, hipMemcpyAsync(&broken, t.ctl + kDtCtlBroken, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (broken != 0u) { return swa_fail_msg(ctx, SWA_E_DEVICE, "d >= 2 clustering on the GPU: a parent without a link to its child"); }
  ctx->res.tables.ready = true;
  ctx->res.tables.nlinks = links;
  ctx->res.tables.radius_at = radius_at;
  ctx->res.tables.serial = ++ctx->dn_tables_made;
  *nswarms = w; *nlinks = links;
  return SWA_OK;
}

// which of this context's swa_dn_tables_device calls made the tables in place (counted from 1), 0 when none are: a caller that
// fetches later can tell whether they are still its own
extern "C" uint64_t swa_dn_tables_serial(const swa_ctx * ctx) {
  return ctx != nullptr && ctx->res.cluster_ready && ctx->res.csr_ready && ctx->res.tables.ready ? ctx->res.tables.serial : 0u;
}

// what swa_dn_tables_device left in HBM: the radius of every amplicon (n), mass / singletons / deepest generation / deepest
// radius of every swarm, parent / child / generation / differences of every link; any output may be null
extern "C" int swa_dn_tables_fetch(swa_ctx * ctx, uint32_t * radius, uint64_t * mass, uint32_t * singletons, uint32_t * maxgen, uint32_t * maxradius,
                                   uint32_t * link_parent, uint32_t * link_child, uint32_t * link_generation, uint8_t * link_diff) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return SWA_OK; }
  SWA_TRY(need_graph_clustering(ctx, "swa_dn_tables_fetch"));
  if (!ctx->res.tables.ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_dn_tables_fetch: no tables in place (swa_dn_tables_device)"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t n = ctx->db.n, w = ctx->res.cluster_nswarms, links = ctx->res.tables.nlinks;
  DnTables t;
  SWA_TRY(swa_carve(ctx, ctx->d_dn_tables, n, false, t));
  SwarmSums s;
  SWA_TRY(swa_carve(ctx, ctx->d_swarm_sums, w, false, s));
  return swa_download(ctx, {{radius, t.acc[ctx->res.tables.radius_at], n * sizeof(uint32_t)},
                            {mass, s.mass, w * sizeof(uint64_t)}, {singletons, s.singles, w * sizeof(uint32_t)},
                            {maxgen, s.maxgen, w * sizeof(uint32_t)}, {maxradius, t.maxradius, w * sizeof(uint32_t)},
                            {link_parent, t.link_parent, links * sizeof(uint32_t)}, {link_child, t.link_child, links * sizeof(uint32_t)},
                            {link_generation, t.link_gen, links * sizeof(uint32_t)}, {link_diff, t.link_diff, links}});
}
