// multi.hip — the d = 1 path on several GPUs of one node, from C++ (no Python, no torch): one context, one
// stream and one host thread per GPU inside this process, RCCL over xGMI for the exchange.
//
// The reference fans its probe loop out over pthreads that share one hash table
// (src/algod1.cc:641-669, 1166-1167; src/utils/threads.h:145-162).  Here the database is replicated
// (288 GB per GPU is never the limit) and the PROBING is divided by ownership of anchor groups
// (swa_d1_set_ownership: rank r serves the groups whose key maps to r, with all their members), so every
// link of the network is found by exactly one rank.  Exchange, as SURVEY 8e / the north star name it: the
// per-rank hit counts are known on the host when the kernels return, then every rank's flat link list is
// gathered on rank 0 — the one consumer: grouped ncclSend / ncclRecv (round 2 all-gathered the whole network into every
// GPU) —, and the CSR is made there by the partition + row kernels of the single-GPU step (swa_d1_csr_from_lists).  It is
// then downloaded for the host (swa_multi_d1_network) or left as rank 0's resident network (swa_multi_d1_network_resident):
// agglomeration, swarm sums, light flags and grafting then run on rank 0's GPU as they do on a single one.  Fastidious: the
// heavy amplicons are split — by the host from host flags (swa_d1_fastidious_shard), or by owner bytes that rank 0 makes
// from its flags in HBM and broadcasts (swa_multi_d1_fastidious_resident) —, graft_cand is combined with
// swa_rccl().AllReduce(min) (src/algod1.cc:244-258 keeps the smallest heavy id), the two heavy-side counters add up.
//
// d = 0 (derep_on_root below): the reads of a rank's slice travel to the rank that owns their hash, the owners dereplicate,
// first_identical[] is assembled on rank 0.  d >= 2: the bulk graph divided by ownership of window groups (further below),
// and the fused scan divided by ownership of the pool (swa_multi_scan_*, at the end: no exchange at all, every rank's hits
// come to the host through its own pinned mirror and are merged there).  The -u alignments (seam B5): every batch cut into a
// contiguous run of pairs a rank, aligned by swa_nw_batch on a host thread a rank (swa_multi_nw_batch, near the end).
//
// The same code runs with several contexts on ONE device (SWARM_AMD_DEVICES=0,0: what a one-GPU box can
// test); RCCL refuses two ranks on one GPU, so that configuration moves the same bytes with device-to-
// device copies instead.  Results are identical to a single GPU by construction and by test
// (tests/test_multi_gpu.py).
#include "swa_internal.h"

#include "rccl_late.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <set>
#include <thread>
#include <vector>

struct swa_multi {
  std::vector<swa_ctx *> ctx;
  std::vector<int> devices;
  std::vector<ncclComm_t> comms;       // empty: in-process copies (several ranks on one device)
  std::vector<swa_dbuf> links;
  swa_dbuf gathered;                   // on rank 0: what the ranks send there (their link lists, graft candidates, graph shares)
  std::vector<swa_dbuf> routed, routed_counts, inbox;   // routed index build: a rank's outgoing id lists, their counts, what it received
  std::vector<uint64_t> link_cap;
  int last_build = SWA_MULTI_BUILD_NONE;   // of the last swa_multi_d1_network* call (swa_multi_d1_last_build)
  std::vector<uint64_t> derep_received;    // of the last swa_multi_derep* call (swa_multi_derep_totals): records every owner received,
  uint64_t derep_rounds = 0, derep_routed = 0;   // the rounds of the slowest owner, the records routed
  bool scan_ready = false;                 // swa_multi_scan_begin has run
  uint64_t scan_batches = 0;               // swa_multi_scan_batch calls since then (swa_multi_scan_totals)
  struct ScanHit { uint32_t sidx, id, diff; };
  std::vector<ScanHit> scan_hits;          // the merged hits of the last swa_multi_scan_batch (swa_multi_scan_fetch)
  std::string err;
};

namespace {

// The ranks' shares of the d >= 2 graph arrive SORTED (swa_dn_graph_compute ends with a sort of its own share) and no key
// occurs in two of them (a pair is found through the first window it shares, and that window's group lives on one rank),
// so the whole is a merge, not a sort: element i of list r goes to i + (the number of smaller keys in every other list) —
// `world - 1` binary searches per element over lists that lie in L2 — where round 3 ran a 64-bit radix sort (8 passes).
// Equal keys across lists (which cannot happen) would still land in distinct places: upper bound below r, lower bound above.
struct MergeArgs {
  const unsigned long long * keys; const uint32_t * vals;     // the gathered lists, list r = [at[r], at[r + 1])
  uint64_t at[65];
  uint32_t world;
  unsigned long long * out_keys; uint32_t * out_vals;
};
__global__ __launch_bounds__(256) void k_merge_sorted_lists(const MergeArgs a) {
  const uint64_t all = a.at[a.world];
  for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < all; idx += (uint64_t)gridDim.x * blockDim.x) {
    uint32_t r = 0;
    while (idx >= a.at[r + 1]) { ++r; }
    const unsigned long long key = a.keys[idx];
    uint64_t pos = idx - a.at[r];
    for (uint32_t s2 = 0; s2 < a.world; ++s2) {
      if (s2 == r) { continue; }
      uint64_t lo = a.at[s2], hi = a.at[s2 + 1];
      while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const unsigned long long k2 = a.keys[mid];
        if (s2 < r ? k2 <= key : k2 < key) { lo = mid + 1; } else { hi = mid; }
      }
      pos += lo - a.at[s2];
    }
    a.out_keys[pos] = key; a.out_vals[pos] = a.vals[idx];
  }
}

// the one launch of the merge (dn_graph_on_root, swa_merge_sorted_lists): a.at[a.world] != 0
int launch_merge(swa_ctx * c, const MergeArgs & a) {
  hipLaunchKernelGGL(k_merge_sorted_lists, dim3(swa_grid256(c, a.at[a.world])), dim3(256), 0, c->stream, a);
  SWA_HIP(c, hipGetLastError());
  return SWA_OK;
}

__global__ __launch_bounds__(256) void k_min_u32(uint32_t * __restrict__ acc, const uint32_t * __restrict__ other, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    acc[i] = min(acc[i], other[i]);
  }
}

// runs f(rank) on one host thread per rank; first non-zero status wins
int on_all(swa_multi * m, const std::function<int(int)> & f) {
  const int world = (int)m->ctx.size();
  std::vector<int> rc((size_t)world, SWA_OK);
  if (world == 1) { rc[0] = f(0); }
  else {
    std::vector<std::thread> threads;
    for (int r = 0; r < world; ++r) { threads.emplace_back([&, r]() { rc[(size_t)r] = f(r); }); }
    for (auto & t : threads) { t.join(); }
  }
  for (int r = 0; r < world; ++r) {
    if (rc[(size_t)r] != SWA_OK) { m->err = "rank " + std::to_string(r) + ": " + swa_last_error(m->ctx[(size_t)r]); return rc[(size_t)r]; }
  }
  return SWA_OK;
}

int fail(swa_multi * m, int code, const std::string & msg) { m->err = msg; return code; }

#define NCCL_OK(m, expr)                                                                               \
  do {                                                                                                 \
    ncclResult_t r_ = (expr);                                                                          \
    if (r_ != ncclSuccess) { return fail((m), SWA_E_DEVICE, std::string(#expr) + ": " + swa_rccl().GetErrorString(r_)); } \
  } while (0)

// every rank's buffer src[r] (count[r] elements of `bytes_per` bytes) into dst + prefix(r) on rank 0 ONLY: the consumer
// of the gathered lists is the rank that builds the CSR, so nothing is sent to the others (an all-gather moved the
// whole network into every GPU: 0.9 GB per rank at 8 x 10 M amplicons).  RCCL: one ncclSend per rank, the matching
// ncclRecv on rank 0, all in one group; ranks sharing a device: device-to-device copies.
int gather_to_root_v(swa_multi * m, const std::vector<const void *> & src, void * dst, const std::vector<uint64_t> & count, size_t bytes_per) {
  const int world = (int)m->ctx.size();
  swa_ctx * c0 = m->ctx[0];
  std::vector<uint64_t> at((size_t)world + 1, 0);
  for (int r = 0; r < world; ++r) { at[(size_t)r + 1] = at[(size_t)r] + count[(size_t)r]; }
  if (!m->comms.empty()) { NCCL_OK(m, swa_rccl().GroupStart()); }
  for (int r = 0; r < world; ++r) {
    if (count[(size_t)r] == 0) { continue; }
    char * recv = static_cast<char *>(dst) + at[(size_t)r] * bytes_per;
    if (!m->comms.empty() && r != 0) {
      NCCL_OK(m, swa_rccl().Send(src[(size_t)r], count[(size_t)r] * bytes_per, ncclUint8, 0, m->comms[(size_t)r], m->ctx[(size_t)r]->stream));
      NCCL_OK(m, swa_rccl().Recv(recv, count[(size_t)r] * bytes_per, ncclUint8, r, m->comms[0], c0->stream));
    } else {
      if (hipSetDevice(c0->device) != hipSuccess ||
          hipMemcpyAsync(recv, src[(size_t)r], count[(size_t)r] * bytes_per, hipMemcpyDefault, c0->stream) != hipSuccess) {
        return fail(m, SWA_E_DEVICE, "device-to-device copy of a rank's list failed");
      }
    }
  }
  if (!m->comms.empty()) { NCCL_OK(m, swa_rccl().GroupEnd()); }
  for (int k = 0; k < world; ++k) {
    if (hipSetDevice(m->devices[(size_t)k]) != hipSuccess || hipStreamSynchronize(m->ctx[(size_t)k]->stream) != hipSuccess) {
      return fail(m, SWA_E_DEVICE, "synchronising the exchange failed");
    }
  }
  return SWA_OK;
}

}  // namespace

extern "C" int swa_multi_create(const int * devices, int ndevices, swa_multi ** out) {
  if (out == nullptr || devices == nullptr || ndevices < 1 || ndevices > 64) { return SWA_E_ARG; }
  auto * m = new swa_multi();
  *out = m;
  m->devices.assign(devices, devices + ndevices);
  // (per-rank buffers first: swa_multi_destroy walks them for every context that exists, also after a failure below)
  m->links.resize((size_t)ndevices);
  m->routed.resize((size_t)ndevices);
  m->routed_counts.resize((size_t)ndevices);
  m->inbox.resize((size_t)ndevices);
  m->link_cap.assign((size_t)ndevices, 0);
  for (int r = 0; r < ndevices; ++r) {
    swa_ctx * c = nullptr;
    const int rc = swa_ctx_create(devices[r], nullptr, &c);
    if (rc != SWA_OK) { m->err = "no usable gfx950 GPU with index " + std::to_string(devices[r]); return rc; }
    m->ctx.push_back(c);
  }
  const std::set<int> distinct(m->devices.begin(), m->devices.end());
  const char * force = getenv("SWARM_AMD_FORCE_RCCL");       // test hook: RCCL even for a single rank
  if ((int)distinct.size() == ndevices && (ndevices > 1 || (force != nullptr && force[0] == '1'))) {
    if (!swa_rccl().error.empty()) { m->err = swa_rccl().error; return SWA_E_DEVICE; }
    m->comms.resize((size_t)ndevices);
    const ncclResult_t r = swa_rccl().CommInitAll(m->comms.data(), ndevices, m->devices.data());
    if (r != ncclSuccess) { m->comms.clear(); m->err = std::string("ncclCommInitAll: ") + swa_rccl().GetErrorString(r); return SWA_E_DEVICE; }
  }
  return SWA_OK;
}

extern "C" void swa_multi_destroy(swa_multi * m) {
  if (m == nullptr) { return; }
  for (size_t r = 0; r < m->ctx.size(); ++r) {
    (void)hipSetDevice(m->devices[r]);
    swa_release(m->links[r]);
    if (r == 0) { swa_release(m->gathered); }
    swa_release(m->routed[r]);
    swa_release(m->routed_counts[r]);
    swa_release(m->inbox[r]);
  }
  for (auto & c : m->comms) { (void)swa_rccl().CommDestroy(c); }
  for (auto * c : m->ctx) { swa_ctx_destroy(c); }
  delete m;
}

extern "C" int swa_multi_size(const swa_multi * m) { return m != nullptr ? (int)m->ctx.size() : 0; }
extern "C" int swa_multi_uses_rccl(const swa_multi * m) { return m != nullptr && !m->comms.empty() ? 1 : 0; }
extern "C" swa_ctx * swa_multi_ctx(swa_multi * m, int rank) {
  return (m != nullptr && rank >= 0 && rank < (int)m->ctx.size()) ? m->ctx[(size_t)rank] : nullptr;
}
extern "C" const char * swa_multi_last_error(const swa_multi * m) { return m != nullptr ? m->err.c_str() : "null handle"; }

extern "C" int swa_multi_db_upload(swa_multi * m, const swa_db_view * host) {
  if (m == nullptr) { return SWA_E_ARG; }
  return on_all(m, [&](int r) { return swa_db_upload(m->ctx[(size_t)r], host); });
}

// Index build of all ranks WITHOUT any of them walking the whole database (swa_d1_route_slice_records /
// swa_d1_index_build_records): every rank keys its own slice, the finished key records travel all-to-all — grouped
// ncclSend / ncclRecv over RCCL, device-to-device copies when the ranks share a device —, every rank builds its indexes
// from what it received, starting at the partition (round 6: rounds 4-5 sent the ids and keyed them again at the owner,
// one random line fetch each).
// *routed = false when a destination region overflowed: the caller builds the other way.  Hashed ownership spreads DISTINCT
// keys evenly, so a region — 1.5 x its even share + 1024 records — holds what a slice sends one owner; amplicons that share
// a window key (primers or conserved flanks left on: one key for the whole database) all go to that key's owner, and a
// slice of more than the region's records then overflows it (n > 8192 at two ranks, > 6144 at three).  Nothing of the
// attempt is used afterwards: the counts are on this stack, m->routed is written anew by the next attempt, and the
// streamed build starts from a cleared index under the same ownership and the same sampled windows.
static int routed_index_build(swa_multi * m, std::vector<int> & dup, bool * routed) {
  const int world = (int)m->ctx.size();
  const uint32_t n = m->ctx[0]->db.n;
  *routed = false;
  std::vector<uint32_t> first((size_t)world + 1, 0);
  for (int r = 0; r <= world; ++r) { first[(size_t)r] = (uint32_t)((uint64_t)n * (uint64_t)r / (uint64_t)world); }
  const uint64_t cap = 3ull * ((uint64_t)n / (uint64_t)world + 1) / (2ull * (uint64_t)world) + 1024;
  const size_t lists = 2 * (size_t)world;
  std::vector<std::vector<uint32_t>> cnt((size_t)world, std::vector<uint32_t>(lists + 1, 0));
  int rc = on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    SWA_HIP(c, hipSetDevice(c->device));
    SWA_TRY(swa_d1_set_ownership(c, (uint32_t)r, (uint32_t)world));
    SWA_TRY(swa_reserve(c, m->routed[(size_t)r], lists * cap * sizeof(uint64_t)));
    SWA_TRY(swa_reserve(c, m->routed_counts[(size_t)r], (lists + 1) * sizeof(uint32_t)));
    SWA_TRY(swa_d1_route_slice_records(c, first[(size_t)r], first[(size_t)r + 1] - first[(size_t)r], (uint32_t)world,
                                       static_cast<uint64_t *>(m->routed[(size_t)r].ptr), cap, static_cast<uint32_t *>(m->routed_counts[(size_t)r].ptr)));
    SWA_HIP(c, hipMemcpy(cnt[(size_t)r].data(), m->routed_counts[(size_t)r].ptr, (lists + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return (int)SWA_OK;
  });
  if (rc != SWA_OK) { return rc; }
  for (int r = 0; r < world; ++r) { if (cnt[(size_t)r][lists] != 0) { m->last_build = SWA_MULTI_BUILD_OVERFLOWED; return SWA_OK; } }
  // rank r receives, per index, the lists of the sources in rank order: inbox[r] = [index 0: s = 0, 1, ..][index 1: ..]
  std::vector<uint32_t> m0((size_t)world, 0), m1((size_t)world, 0);
  for (int r = 0; r < world; ++r) {
    for (int s2 = 0; s2 < world; ++s2) { m0[(size_t)r] += cnt[(size_t)s2][(size_t)r]; m1[(size_t)r] += cnt[(size_t)s2][(size_t)world + (size_t)r]; }
    swa_ctx * c = m->ctx[(size_t)r];
    if (hipSetDevice(c->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
    rc = swa_reserve(c, m->inbox[(size_t)r], ((uint64_t)m0[(size_t)r] + m1[(size_t)r] + 1) * sizeof(uint64_t));
    if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c)); }
  }
  if (!m->comms.empty()) { NCCL_OK(m, swa_rccl().GroupStart()); }
  for (int r = 0; r < world; ++r) {
    uint64_t at[2] = {0, m0[(size_t)r]};
    for (int s2 = 0; s2 < world; ++s2) {
      for (int index = 0; index < 2; ++index) {
        const size_t list = (size_t)index * (size_t)world + (size_t)r;
        const uint32_t count = cnt[(size_t)s2][list];
        if (count == 0) { continue; }
        const uint64_t * src = static_cast<const uint64_t *>(m->routed[(size_t)s2].ptr) + list * cap;
        uint64_t * dst = static_cast<uint64_t *>(m->inbox[(size_t)r].ptr) + at[index];
        at[index] += count;
        if (!m->comms.empty()) {
          NCCL_OK(m, swa_rccl().Send(src, count, ncclUint64, r, m->comms[(size_t)s2], m->ctx[(size_t)s2]->stream));
          NCCL_OK(m, swa_rccl().Recv(dst, count, ncclUint64, s2, m->comms[(size_t)r], m->ctx[(size_t)r]->stream));
        } else {
          if (hipSetDevice(m->devices[(size_t)r]) != hipSuccess ||
              hipMemcpyAsync(dst, src, (size_t)count * sizeof(uint64_t), hipMemcpyDefault, m->ctx[(size_t)r]->stream) != hipSuccess) {
            return fail(m, SWA_E_DEVICE, "device-to-device copy of a routed record list failed");
          }
        }
      }
    }
  }
  if (!m->comms.empty()) { NCCL_OK(m, swa_rccl().GroupEnd()); }
  for (int k = 0; k < world; ++k) {
    if (hipSetDevice(m->devices[(size_t)k]) != hipSuccess || hipStreamSynchronize(m->ctx[(size_t)k]->stream) != hipSuccess) {
      return fail(m, SWA_E_DEVICE, "synchronising the exchange of the routed record lists failed");
    }
  }
  *routed = true;
  m->last_build = SWA_MULTI_BUILD_ROUTED;
  return on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    const uint64_t * in = static_cast<const uint64_t *>(m->inbox[(size_t)r].ptr);
    return swa_d1_index_build_records(c, in, m0[(size_t)r], in + m0[(size_t)r], m1[(size_t)r], &dup[(size_t)r]);
  });
}

// The whole network of the database assembled as a CSR on rank 0's device, and then either downloaded (resident = false:
// swa_multi_d1_network) or left there as rank 0's resident network (swa_multi_d1_network_resident: offsets and neighbours unused).
static int d1_network_on_root(swa_multi * m, int no_cluster_breaking, bool resident, uint64_t * offsets, uint32_t * neighbours, uint64_t cap,
                              uint64_t * total, int * has_duplicates) {
  const int world = (int)m->ctx.size();
  const uint32_t n = m->ctx[0]->db.n;
  m->last_build = SWA_MULTI_BUILD_NONE;
  if (n == 0) { return fail(m, SWA_E_ARG, "swa_multi_d1_network: no database"); }
  m->ctx[0]->res.csr_ready = false;                            // (whatever fails below: no resident network on rank 0)
  m->ctx[0]->res.cluster_ready = false;
  m->ctx[0]->res.tables = {};
  // 1. every rank indexes and probes the anchor groups it owns
  std::vector<int> dup((size_t)world, 0);
  std::vector<uint64_t> count((size_t)world, 0);
  // (SWARM_AMD_MULTI_BUILD=streamed: every rank walks the whole database for the keys it owns, as before the routed build)
  const char * env_build = getenv("SWARM_AMD_MULTI_BUILD");
  bool routed = false;
  int rc = SWA_OK;
  if (world > 1 && !(env_build != nullptr && env_build[0] == 's')) {
    rc = routed_index_build(m, dup, &routed);
    if (rc != SWA_OK) {
      if (has_duplicates != nullptr) { *has_duplicates = 0; for (int d : dup) { *has_duplicates |= d; } }
      return rc;
    }
  } else {
    m->last_build = SWA_MULTI_BUILD_STREAMED;
  }
  rc = on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    SWA_TRY(swa_d1_set_ownership(c, (uint32_t)r, (uint32_t)world));
    int rc2 = routed ? (int)SWA_OK : swa_d1_index_build(c, &dup[(size_t)r]);
    if (rc2 != SWA_OK) { return rc2; }
    if (m->link_cap[(size_t)r] == 0) { m->link_cap[(size_t)r] = 4ull * n / (uint64_t)world + 65536; }
    for (;;) {
      SWA_HIP(c, hipSetDevice(c->device));
      SWA_TRY(swa_reserve(c, m->links[(size_t)r], m->link_cap[(size_t)r] * sizeof(uint64_t)));
      rc2 = swa_d1_network_edges_device(c, no_cluster_breaking, 0, n, static_cast<uint64_t *>(m->links[(size_t)r].ptr),
                                        m->link_cap[(size_t)r], &count[(size_t)r]);
      if (rc2 == SWA_E_CAPACITY) { m->link_cap[(size_t)r] = count[(size_t)r] + 1024; continue; }
      if (rc2 == SWA_E_DUPLICATES) { dup[(size_t)r] = 1; }     // (identical sequences inside a prefix group this rank owns: the pair pass met them)
      return rc2;
    }
  });
  if (has_duplicates != nullptr) { *has_duplicates = 0; for (int d : dup) { *has_duplicates |= d; } }
  if (rc != SWA_OK) { return rc; }
  // 2. the link lists to rank 0, which builds the CSR (counts are on the host already)
  uint64_t all = 0;
  for (uint64_t c : count) { all += c; }
  *total = all;
  std::vector<const void *> src((size_t)world);
  for (int r = 0; r < world; ++r) { src[(size_t)r] = m->links[(size_t)r].ptr; }
  {
    swa_ctx * c = m->ctx[0];
    if (hipSetDevice(c->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
    rc = swa_reserve(c, m->gathered, (all + 2) * sizeof(uint64_t));
    if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c)); }
  }
  if (all != 0) {
    rc = gather_to_root_v(m, src, m->gathered.ptr, count, sizeof(uint64_t));
    if (rc != SWA_OK) { return rc; }
  }
  // 3. rank 0: the gathered lists -> CSR (-> host).  The partition + row kernels of the single-GPU step (d1_part.hip: csr_from_chunks,
  // the ranks' lists as the chunks of its first level) where round 3 ran a 64-bit radix sort over all links.
  swa_ctx * c0 = m->ctx[0];
  if (hipSetDevice(c0->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
  auto * keys_in = static_cast<unsigned long long *>(m->gathered.ptr);
  auto stage = [&]() -> int {
    c0->res.csr_ready = false;                                   // (d_offsets_tmp / d_nb_tmp now hold the gathered network)
    SWA_TRY(swa_reserve(c0, c0->d_offsets_tmp, ((uint64_t)n + 1) * sizeof(uint64_t)));
    SWA_TRY(swa_reserve(c0, c0->d_nb_tmp, (all + 1) * sizeof(uint32_t)));
    std::vector<uint64_t> starts((size_t)world, 0);
    for (int r = 1; r < world; ++r) { starts[(size_t)r] = starts[(size_t)r - 1] + count[(size_t)r - 1]; }
    uint64_t need = 0;                                       // (= all: the buffer was sized for it, so SWA_E_CAPACITY cannot come back)
    SWA_TRY(swa_d1_csr_from_lists(c0, reinterpret_cast<const uint64_t *>(keys_in), starts.data(), count.data(), (uint32_t)world, 0, n,
                                  static_cast<uint64_t *>(c0->d_offsets_tmp.ptr), static_cast<uint32_t *>(c0->d_nb_tmp.ptr), all + 1, &need));
    (void)need;
    if (!resident) {
      SWA_HIP(c0, hipMemcpyAsync(offsets, c0->d_offsets_tmp.ptr, ((uint64_t)n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c0->stream));
      if (all != 0 && all <= cap) {
        SWA_HIP(c0, hipMemcpyAsync(neighbours, c0->d_nb_tmp.ptr, all * sizeof(uint32_t), hipMemcpyDeviceToHost, c0->stream));
      }
    }
    SWA_HIP(c0, hipGetLastError());
    SWA_HIP(c0, hipStreamSynchronize(c0->stream));           // (m->gathered, which the row kernels read, is free for the next exchange)
    if (resident) {                                            // the state swa_d1_network_resident leaves
      c0->res.csr_ready = true;
      c0->res.csr_has_diffs = false;
      c0->res.csr_total = all;
    }
    return SWA_OK;
  };
  rc = stage();
  if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c0)); }
  if (!resident && all > cap) { return fail(m, SWA_E_CAPACITY, "swa_multi_d1_network: neighbour buffer too small"); }
  return SWA_OK;
}

// the whole network of the database as a CSR on the host (buffers and capacity protocol of swa_d1_network)
extern "C" int swa_multi_d1_network(swa_multi * m, int no_cluster_breaking, uint64_t * offsets, uint32_t * neighbours, uint64_t cap,
                                    uint64_t * total, int * has_duplicates) {
  if (m == nullptr || offsets == nullptr || total == nullptr || (neighbours == nullptr && cap != 0)) { return SWA_E_ARG; }
  return d1_network_on_root(m, no_cluster_breaking, false, offsets, neighbours, cap, total, has_duplicates);
}

// ... or left where it was assembled: rank 0's context holds it as swa_d1_network_resident would (swa_d1_network_fetch,
// swa_d1_cluster_device and everything behind it work on swa_multi_ctx(m, 0)); nothing comes to the host
extern "C" int swa_multi_d1_network_resident(swa_multi * m, int no_cluster_breaking, uint64_t * total, int * has_duplicates) {
  if (m == nullptr || total == nullptr) { return SWA_E_ARG; }
  return d1_network_on_root(m, no_cluster_breaking, true, nullptr, nullptr, 0, total, has_duplicates);
}

extern "C" int swa_multi_d1_last_build(const swa_multi * m) { return m != nullptr ? m->last_build : SWA_MULTI_BUILD_NONE; }

// B2 on all GPUs: heavy amplicons split over the ranks, graft_cand combined with MIN, heavy counters summed
extern "C" int swa_multi_d1_fastidious(swa_multi * m, const uint8_t * is_light, uint64_t light_nt, uint32_t bloom_bits,
                                       uint32_t * graft_cand, uint64_t * counters) {
  if (m == nullptr || is_light == nullptr || graft_cand == nullptr || counters == nullptr) { return SWA_E_ARG; }
  const int world = (int)m->ctx.size();
  const uint32_t n = m->ctx[0]->db.n;
  std::vector<std::vector<uint32_t>> scratch((size_t)world);
  std::vector<std::vector<uint64_t>> cnt((size_t)world, std::vector<uint64_t>(8, 0));
  int rc = on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    if (!c->ix.d1_ready) { int dup = 0; SWA_TRY(swa_d1_index_build(c, &dup)); }
    uint32_t * host = graft_cand;
    if (r != 0) { scratch[(size_t)r].resize(n); host = scratch[(size_t)r].data(); }   // (the per-rank host copy is not the result)
    return swa_d1_fastidious_shard(c, is_light, light_nt, bloom_bits, (uint32_t)r, (uint32_t)world, host, cnt[(size_t)r].data());
  });
  if (rc != SWA_OK) { return rc; }
  for (int k = 0; k < 5; ++k) { counters[k] = cnt[0][(size_t)k]; }
  for (int r = 1; r < world; ++r) { counters[1] += cnt[(size_t)r][1]; counters[2] += cnt[(size_t)r][2]; }
  if (world == 1 && m->comms.empty()) { return SWA_OK; }
  // element-wise minimum of the ranks' graft_cand arrays, which are still in HBM (d_graft)
  if (!m->comms.empty()) {
    NCCL_OK(m, swa_rccl().GroupStart());
    for (int r = 0; r < world; ++r) {
      NCCL_OK(m, swa_rccl().AllReduce(m->ctx[(size_t)r]->d_graft.ptr, m->ctx[(size_t)r]->d_graft.ptr, n, ncclUint32, ncclMin, m->comms[(size_t)r],
                               m->ctx[(size_t)r]->stream));
    }
    NCCL_OK(m, swa_rccl().GroupEnd());
  } else {
    swa_ctx * c0 = m->ctx[0];
    if (hipSetDevice(c0->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
    rc = swa_reserve(c0, m->gathered, (uint64_t)n * sizeof(uint32_t));
    if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c0)); }
    for (int r = 1; r < world; ++r) {
      if (hipMemcpyAsync(m->gathered.ptr, m->ctx[(size_t)r]->d_graft.ptr, (uint64_t)n * sizeof(uint32_t), hipMemcpyDefault, c0->stream) != hipSuccess) {
        return fail(m, SWA_E_DEVICE, "device-to-device copy of graft candidates failed");
      }
      hipLaunchKernelGGL(k_min_u32, dim3(swa_grid256(c0, n)), dim3(256), 0, c0->stream, static_cast<uint32_t *>(c0->d_graft.ptr),
                         static_cast<const uint32_t *>(m->gathered.ptr), (uint64_t)n);
    }
  }
  swa_ctx * c0 = m->ctx[0];
  if (hipSetDevice(c0->device) != hipSuccess ||
      hipMemcpyAsync(graft_cand, c0->d_graft.ptr, (uint64_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c0->stream) != hipSuccess ||
      hipStreamSynchronize(c0->stream) != hipSuccess) {
    return fail(m, SWA_E_DEVICE, "download of the combined graft candidates failed");
  }
  return SWA_OK;
}

// B2 on all GPUs from the flags in rank 0's HBM (swa_d1_light_flags_device on swa_multi_ctx(m, 0)): rank 0 makes the owner byte
// of every amplicon (swa_d1_shard_owners_device, S = world), the bytes travel to every rank — ncclBroadcast, or device-to-
// device copies when ranks share a device —, every rank maps them to its roles on its own GPU and runs its shard of the pass,
// and the candidates are combined into rank 0's d_graft, where swa_d1_graft_device(ctx0, NULL, ...) reads them.  No flag, role
// or candidate array crosses the host (the candidates only when graft_cand is not null).
extern "C" int swa_multi_d1_fastidious_resident(swa_multi * m, uint64_t light_nt, uint32_t bloom_bits, uint32_t * graft_cand, uint64_t * counters) {
  if (m == nullptr || counters == nullptr) { return SWA_E_ARG; }
  const int world = (int)m->ctx.size();
  swa_ctx * c0 = m->ctx[0];
  const uint32_t n = c0->db.n;
  if (!c0->res.cluster_ready || !c0->res.csr_ready || !c0->res.fast.roles_ready) {
    return fail(m, SWA_E_ARG, "swa_multi_d1_fastidious_resident: rank 0 holds no clustering with flags (swa_d1_cluster_device, swa_d1_light_flags_device)");
  }
  if (!c0->ix.d1_ready) { return fail(m, SWA_E_ARG, "swa_multi_d1_fastidious_resident: rank 0's index has been given up (its clustering would end with a new one)"); }
  uint64_t heavy = 0;
  // (returns with rank 0's stream synchronised: the other ranks' streams, which do not order against it, may read the bytes)
  int rc = swa_d1_shard_owners_device(c0, (uint32_t)world, nullptr, &heavy);
  if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c0)); }
  const uint64_t n_light = c0->res.fast.light_amps;
  for (int r = 1; r < world; ++r) {
    swa_ctx * c = m->ctx[(size_t)r];
    if (hipSetDevice(c->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
    rc = swa_reserve(c, c->d_shard_owner, (uint64_t)n + 4);
    if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c)); }
  }
  if (!m->comms.empty()) {
    NCCL_OK(m, swa_rccl().GroupStart());
    for (int r = 0; r < world; ++r) {
      swa_ctx * c = m->ctx[(size_t)r];
      NCCL_OK(m, swa_rccl().Broadcast(c->d_shard_owner.ptr, c->d_shard_owner.ptr, n, ncclUint8, 0, m->comms[(size_t)r], c->stream));
    }
    NCCL_OK(m, swa_rccl().GroupEnd());
  } else {
    for (int r = 1; r < world; ++r) {
      swa_ctx * c = m->ctx[(size_t)r];
      if (hipSetDevice(c->device) != hipSuccess ||
          hipMemcpyAsync(c->d_shard_owner.ptr, c0->d_shard_owner.ptr, n, hipMemcpyDefault, c->stream) != hipSuccess) {
        return fail(m, SWA_E_DEVICE, "device-to-device copy of the owner bytes failed");
      }
    }
  }
  std::vector<std::vector<uint64_t>> cnt((size_t)world, std::vector<uint64_t>(8, 0));
  rc = on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    if (r != 0 && !c->ix.d1_ready) { int dup = 0; SWA_TRY(swa_d1_index_build(c, &dup)); }
    const uint64_t lo = heavy * (uint64_t)r / (uint64_t)world, hi = heavy * ((uint64_t)r + 1) / (uint64_t)world;
    return swa_d1_fastidious_owned(c, static_cast<const uint8_t *>(c->d_shard_owner.ptr), (uint32_t)r, n_light, hi - lo, light_nt, bloom_bits,
                                   nullptr, cnt[(size_t)r].data());
  });
  if (rc != SWA_OK) { return rc; }                           // (every rank's pass ends with its stream synchronised)
  for (int k = 0; k < 5; ++k) { counters[k] = cnt[0][(size_t)k]; }
  for (int r = 1; r < world; ++r) { counters[1] += cnt[(size_t)r][1]; counters[2] += cnt[(size_t)r][2]; }
  // element-wise minimum of the ranks' candidates into rank 0's d_graft
  if (!m->comms.empty()) {
    NCCL_OK(m, swa_rccl().GroupStart());
    for (int r = 0; r < world; ++r) {
      swa_ctx * c = m->ctx[(size_t)r];
      NCCL_OK(m, swa_rccl().AllReduce(c->d_graft.ptr, c->d_graft.ptr, n, ncclUint32, ncclMin, m->comms[(size_t)r], c->stream));
    }
    NCCL_OK(m, swa_rccl().GroupEnd());
    for (int r = 1; r < world; ++r) {
      if (hipSetDevice(m->devices[(size_t)r]) != hipSuccess || hipStreamSynchronize(m->ctx[(size_t)r]->stream) != hipSuccess) {
        return fail(m, SWA_E_DEVICE, "synchronising the exchange of the graft candidates failed");
      }
    }
    if (hipSetDevice(c0->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
  } else if (world > 1) {
    if (hipSetDevice(c0->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
    rc = swa_reserve(c0, m->gathered, (uint64_t)n * sizeof(uint32_t));
    if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c0)); }
    for (int r = 1; r < world; ++r) {
      if (hipMemcpyAsync(m->gathered.ptr, m->ctx[(size_t)r]->d_graft.ptr, (uint64_t)n * sizeof(uint32_t), hipMemcpyDefault, c0->stream) != hipSuccess) {
        return fail(m, SWA_E_DEVICE, "device-to-device copy of graft candidates failed");
      }
      hipLaunchKernelGGL(k_min_u32, dim3(swa_grid256(c0, n)), dim3(256), 0, c0->stream, static_cast<uint32_t *>(c0->d_graft.ptr),
                         static_cast<const uint32_t *>(m->gathered.ptr), (uint64_t)n);
    }
  }
  if (graft_cand != nullptr) {
    swa_touch_pages(graft_cand, (uint64_t)n * sizeof(uint32_t));
    if (hipMemcpyAsync(graft_cand, c0->d_graft.ptr, (uint64_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c0->stream) != hipSuccess) {
      return fail(m, SWA_E_DEVICE, "download of the combined graft candidates failed");
    }
  }
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c0->stream) != hipSuccess) { return fail(m, SWA_E_DEVICE, "combining the graft candidates failed"); }
  c0->res.fast.cand_ready = true;                              // (d_graft on rank 0: the candidates of the whole pass)
  return SWA_OK;
}

// ---- d = 0 on several GPUs: the reads travel to the owner of their hash (src/derep.cc:276-354) ------------------------------
// The routed build of d = 1, applied to hashes.  Every rank hashes its slice of the replicated database and groups the
// (hash, id) records by owner (swa_derep_route_slice: k_derep_hash_slice, k_derep_route); the counts come to the host once,
// the inboxes are reserved from them — exactly: a read with 10^6 copies sends 10^6 records to one owner, so there is no
// region cap, no overflow and no other build —, and the records travel all-to-all: grouped ncclSend / ncclRecv, device-to-
// device copies when the ranks share a device; one rank takes the same path.  Every owner dereplicates what it received
// (swa_derep_owner_rounds: the re-key rounds stay local, all copies of a sequence are there) and packs first << 32 | id;
// rank 0 gathers the packed words and writes first_identical[] into its d_graft (swa_derep_home): from there on
// swa_multi_ctx(m, 0) is a context after swa_derep_resident.
static int derep_on_root(swa_multi * m) {
  const int world = (int)m->ctx.size();
  const uint32_t n = m->ctx[0]->db.n;
  m->derep_received.assign((size_t)world, 0);
  m->derep_rounds = m->derep_routed = 0;
  for (swa_ctx * c : m->ctx) { c->dr = {}; }                   // (whatever fails below: no rank holds a resident array)
  if (n == 0) { return fail(m, SWA_E_ARG, "swa_multi_derep: no database"); }
  // 1. every rank hashes and routes its slice
  std::vector<uint32_t> first((size_t)world + 1, 0);
  for (int r = 0; r <= world; ++r) { first[(size_t)r] = (uint32_t)((uint64_t)n * (uint64_t)r / (uint64_t)world); }
  std::vector<std::vector<uint32_t>> cnt((size_t)world, std::vector<uint32_t>((size_t)world, 0));
  int rc = on_all(m, [&](int r) {
    return swa_derep_route_slice(m->ctx[(size_t)r], first[(size_t)r], first[(size_t)r + 1] - first[(size_t)r], (uint32_t)world, m->routed[(size_t)r],
                                 cnt[(size_t)r].data());
  });
  if (rc != SWA_OK) { return rc; }
  // 2. the exchange: rank r receives the runs for it of the sources in rank order
  std::vector<uint64_t> received((size_t)world, 0);
  for (int r = 0; r < world; ++r) {
    for (int s2 = 0; s2 < world; ++s2) { received[(size_t)r] += cnt[(size_t)s2][(size_t)r]; }
    swa_ctx * c = m->ctx[(size_t)r];
    if (hipSetDevice(c->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
    rc = swa_reserve(c, m->inbox[(size_t)r], swa_derep_inbox::bytes(received[(size_t)r]));
    if (rc == SWA_OK) { rc = swa_reserve(c, m->links[(size_t)r], (received[(size_t)r] + 2) * sizeof(uint64_t)); }
    if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c)); }
  }
  if (!m->comms.empty()) { NCCL_OK(m, swa_rccl().GroupStart()); }
  for (int r = 0; r < world; ++r) {
    const swa_derep_inbox in(m->inbox[(size_t)r].ptr, received[(size_t)r]);
    uint64_t at = 0;
    for (int s2 = 0; s2 < world; ++s2) {
      const uint32_t count = cnt[(size_t)s2][(size_t)r];
      if (count == 0) { continue; }
      const swa_derep_routed out(m->routed[(size_t)s2].ptr, first[(size_t)s2 + 1] - first[(size_t)s2]);
      uint64_t run = 0;                                        // where the run for r begins in the source's arrays
      for (int d = 0; d < r; ++d) { run += cnt[(size_t)s2][(size_t)d]; }
      if (!m->comms.empty()) {
        NCCL_OK(m, swa_rccl().Send(out.hash + run, count, ncclUint64, r, m->comms[(size_t)s2], m->ctx[(size_t)s2]->stream));
        NCCL_OK(m, swa_rccl().Recv(in.hash + at, count, ncclUint64, s2, m->comms[(size_t)r], m->ctx[(size_t)r]->stream));
        NCCL_OK(m, swa_rccl().Send(out.id + run, count, ncclUint32, r, m->comms[(size_t)s2], m->ctx[(size_t)s2]->stream));
        NCCL_OK(m, swa_rccl().Recv(in.id + at, count, ncclUint32, s2, m->comms[(size_t)r], m->ctx[(size_t)r]->stream));
      } else {
        if (hipSetDevice(m->devices[(size_t)r]) != hipSuccess ||
            hipMemcpyAsync(in.hash + at, out.hash + run, (size_t)count * sizeof(uint64_t), hipMemcpyDefault, m->ctx[(size_t)r]->stream) != hipSuccess ||
            hipMemcpyAsync(in.id + at, out.id + run, (size_t)count * sizeof(uint32_t), hipMemcpyDefault, m->ctx[(size_t)r]->stream) != hipSuccess) {
          return fail(m, SWA_E_DEVICE, "device-to-device copy of routed dereplication records failed");
        }
      }
      at += count;
    }
  }
  if (!m->comms.empty()) { NCCL_OK(m, swa_rccl().GroupEnd()); }
  for (int k = 0; k < world; ++k) {
    if (hipSetDevice(m->devices[(size_t)k]) != hipSuccess || hipStreamSynchronize(m->ctx[(size_t)k]->stream) != hipSuccess) {
      return fail(m, SWA_E_DEVICE, "synchronising the exchange of the dereplication records failed");
    }
  }
  // 3. every owner dereplicates what it received
  std::vector<uint32_t> rounds((size_t)world, 0);
  rc = on_all(m, [&](int r) {
    const swa_derep_inbox in(m->inbox[(size_t)r].ptr, received[(size_t)r]);
    return swa_derep_owner_rounds(m->ctx[(size_t)r], in.hash, in.id, (uint32_t)received[(size_t)r], static_cast<uint64_t *>(m->links[(size_t)r].ptr),
                                  &rounds[(size_t)r]);
  });
  if (rc != SWA_OK) { return rc; }
  // 4. home: every id exactly once
  uint64_t all = 0;
  for (int r = 0; r < world; ++r) { all += received[(size_t)r]; m->derep_rounds = std::max<uint64_t>(m->derep_rounds, rounds[(size_t)r]); }
  m->derep_received = received;
  m->derep_routed = all;
  if (all != n) { return fail(m, SWA_E_INTERNAL, "swa_multi_derep: the owners hold " + std::to_string(all) + " records of " + std::to_string(n) + " reads"); }
  swa_ctx * c0 = m->ctx[0];
  if (hipSetDevice(c0->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
  rc = swa_reserve(c0, m->gathered, (all + 2) * sizeof(uint64_t));
  if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c0)); }
  std::vector<const void *> src((size_t)world);
  for (int r = 0; r < world; ++r) { src[(size_t)r] = m->links[(size_t)r].ptr; }
  rc = gather_to_root_v(m, src, m->gathered.ptr, received, sizeof(uint64_t));
  if (rc != SWA_OK) { return rc; }
  rc = swa_derep_home(c0, static_cast<const uint64_t *>(m->gathered.ptr));
  if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c0)); }
  return SWA_OK;
}

// = swa_derep_resident on swa_multi_ctx(m, 0), the search divided among the ranks by ownership of the hashes
extern "C" int swa_multi_derep_resident(swa_multi * m) {
  if (m == nullptr) { return SWA_E_ARG; }
  return derep_on_root(m);
}

// ... plus the download: swa_derep's array
extern "C" int swa_multi_derep(swa_multi * m, uint32_t * first_identical) {
  if (m == nullptr) { return SWA_E_ARG; }
  if (first_identical == nullptr) { return fail(m, SWA_E_ARG, "swa_multi_derep: bad argument"); }
  SWA_TRY(derep_on_root(m));
  swa_ctx * c0 = m->ctx[0];
  const int rc = swa_download(c0, {{first_identical, c0->d_graft.ptr, uint64_t(c0->db.n) * sizeof(uint32_t)}});
  return rc != SWA_OK ? fail(m, rc, swa_last_error(c0)) : (int)SWA_OK;
}

// received[world]: the records every owner got in the last call; out2 = {rounds of the slowest owner, records routed}
extern "C" int swa_multi_derep_totals(swa_multi * m, uint64_t * received, uint64_t * out2) {
  if (m == nullptr || received == nullptr || out2 == nullptr) { return SWA_E_ARG; }
  for (size_t r = 0; r < m->ctx.size(); ++r) { received[r] = r < m->derep_received.size() ? m->derep_received[r] : 0; }
  out2[0] = m->derep_rounds; out2[1] = m->derep_routed;
  return SWA_OK;
}

// ---- d >= 2 on several GPUs: the bulk graph (dn_graph.hip) divided by ownership of window groups ------------------
// Replaces the scan fan-out of src/scan.cc:221-256 under the loop of src/algo.cc:505-602: every rank finds the pairs of
// the window groups it owns (swa_dn_set_ownership) and aligns them; the accepted (query, target, diff) triples travel
// to rank 0 — ncclSend / ncclRecv over RCCL, device-to-device copies when ranks share a device —, which sorts them
// into the CSR of swa_dn_graph — downloaded for the host's greedy walk (swa_multi_dn_graph), or left as rank 0's resident
// network, where swa_d1_cluster_device walks it and dn_tables.inc makes radii and links (swa_multi_dn_graph_resident).
extern "C" int swa_multi_dn_begin(swa_multi * m, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t d) {
  if (m == nullptr) { return SWA_E_ARG; }
  return on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    SWA_TRY(swa_qgram_build(c));
    return swa_search_begin(c, mismatch, gapopen, gapextend, d);
  });
}

extern "C" int swa_multi_dn_graph_supported(swa_multi * m) {
  if (m == nullptr) { return 0; }
  for (swa_ctx * c : m->ctx) { if (swa_dn_graph_supported(c) == 0) { return 0; } }
  return 1;
}

static int dn_graph_on_root(swa_multi * m, int no_cluster_breaking, bool resident, uint64_t * offsets, uint32_t * neighbours, uint8_t * diffs,
                            uint64_t cap, uint64_t * total) {
  const int world = (int)m->ctx.size();
  if (resident) {                                              // (whatever fails below: no resident network on rank 0)
    m->ctx[0]->res.csr_ready = false;
    m->ctx[0]->res.tables = {};
  }
  int rc = on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    SWA_TRY(swa_dn_set_ownership(c, (uint32_t)r, (uint32_t)world));
    SWA_TRY(swa_dn_graph_compute(c, no_cluster_breaking));
    // (the share's final sort is still queued on this rank's stream, and the streams of the contexts do not order against
    // each other: the copies below run on rank 0's stream when the ranks share a device — ADVICE r03)
    SWA_HIP(c, hipStreamSynchronize(c->stream));
    return (int)SWA_OK;
  });
  // the shares are computed: a later single-context call on any of these contexts sees the whole database again
  for (swa_ctx * c : m->ctx) { (void)swa_dn_set_ownership(c, 0, 1); }
  if (rc != SWA_OK) { return rc; }
  swa_ctx * c0 = m->ctx[0];
  uint64_t all = 0;
  std::vector<uint64_t> at((size_t)world + 1, 0);
  for (int r = 0; r < world; ++r) { at[(size_t)r] = all; all += m->ctx[(size_t)r]->dn_edges; }
  at[(size_t)world] = all;
  if (hipSetDevice(c0->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
  // rank 0's buffers: [all keys | sorted keys] and [all diffs | sorted diffs]
  rc = swa_reserve(c0, m->gathered, (2 * all + 2) * sizeof(uint64_t));
  if (rc == SWA_OK) { rc = swa_reserve(c0, m->links[0], (2 * all + 2) * sizeof(uint32_t)); }
  if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c0)); }
  auto * keys = static_cast<unsigned long long *>(m->gathered.ptr);
  auto * vals = static_cast<uint32_t *>(m->links[0].ptr);
  if (!m->comms.empty()) { NCCL_OK(m, swa_rccl().GroupStart()); }
  for (int r = 0; r < world; ++r) {
    swa_ctx * c = m->ctx[(size_t)r];
    const uint64_t cnt = c->dn_edges;
    if (cnt == 0) { continue; }
    const auto * k_src = static_cast<const unsigned long long *>(c->d_dn_keys.ptr) + c->dn_work;
    const auto * v_src = static_cast<const uint32_t *>(c->d_dn_vals.ptr) + c->dn_work;
    if (!m->comms.empty() && r != 0) {
      NCCL_OK(m, swa_rccl().Send(k_src, cnt, ncclUint64, 0, m->comms[(size_t)r], c->stream));
      NCCL_OK(m, swa_rccl().Recv(keys + at[(size_t)r], cnt, ncclUint64, r, m->comms[0], c0->stream));
      NCCL_OK(m, swa_rccl().Send(v_src, cnt, ncclUint32, 0, m->comms[(size_t)r], c->stream));
      NCCL_OK(m, swa_rccl().Recv(vals + at[(size_t)r], cnt, ncclUint32, r, m->comms[0], c0->stream));
    } else {
      if (hipSetDevice(c0->device) != hipSuccess ||
          hipMemcpyAsync(keys + at[(size_t)r], k_src, cnt * sizeof(uint64_t), hipMemcpyDefault, c0->stream) != hipSuccess ||
          hipMemcpyAsync(vals + at[(size_t)r], v_src, cnt * sizeof(uint32_t), hipMemcpyDefault, c0->stream) != hipSuccess) {
        return fail(m, SWA_E_DEVICE, "device-to-device copy of a rank's share of the graph failed");
      }
    }
  }
  if (!m->comms.empty()) { NCCL_OK(m, swa_rccl().GroupEnd()); }
  for (int k = 0; k < world; ++k) {
    if (hipSetDevice(m->devices[(size_t)k]) != hipSuccess || hipStreamSynchronize(m->ctx[(size_t)k]->stream) != hipSuccess) {
      return fail(m, SWA_E_DEVICE, "synchronising the exchange of the graph failed");
    }
  }
  if (hipSetDevice(c0->device) != hipSuccess) { return fail(m, SWA_E_DEVICE, "hipSetDevice"); }
  auto stage = [&]() -> int {
    if (all != 0) {
      MergeArgs ma{};
      ma.keys = keys; ma.vals = vals; ma.world = (uint32_t)world;
      for (int r = 0; r <= world; ++r) { ma.at[r] = at[(size_t)r]; }
      ma.out_keys = keys + all + 1; ma.out_vals = vals + all + 1;
      SWA_TRY(launch_merge(c0, ma));
    }
    const unsigned long long * sorted = all != 0 ? keys + all + 1 : nullptr;
    const uint32_t * svals = all != 0 ? vals + all + 1 : nullptr;
    if (!resident) { return swa_dn_graph_emit(c0, sorted, svals, all, offsets, neighbours, diffs, cap, total); }
    SWA_TRY(swa_dn_graph_install(c0, sorted, svals, all));
    *total = all;
    // (m->gathered and m->links[0], which the split reads, are free for the next exchange once it has run)
    if (hipStreamSynchronize(c0->stream) != hipSuccess) { c0->res.csr_ready = false; return swa_fail_msg(c0, SWA_E_DEVICE, "swa_multi_dn_graph_resident: the split of the merged graph failed"); }
    return SWA_OK;
  };
  rc = stage();
  if (rc != SWA_OK) { return fail(m, rc, swa_last_error(c0)); }
  return SWA_OK;
}

extern "C" int swa_multi_dn_graph(swa_multi * m, int no_cluster_breaking, uint64_t * offsets, uint32_t * neighbours, uint8_t * diffs,
                                  uint64_t cap, uint64_t * total) {
  if (m == nullptr || offsets == nullptr || total == nullptr || (cap != 0 && (neighbours == nullptr || diffs == nullptr))) { return SWA_E_ARG; }
  return dn_graph_on_root(m, no_cluster_breaking, false, offsets, neighbours, diffs, cap, total);
}

// ... or left on rank 0 as its resident network, as swa_dn_graph_resident leaves a single context's (csr_has_diffs)
extern "C" int swa_multi_dn_graph_resident(swa_multi * m, int no_cluster_breaking, uint64_t * total) {
  if (m == nullptr || total == nullptr) { return SWA_E_ARG; }
  return dn_graph_on_root(m, no_cluster_breaking, true, nullptr, nullptr, nullptr, 0, total);
}

// out3 = {q-gram comparisons, aligned pairs, kernel launches} over all ranks
extern "C" int swa_multi_dn_graph_totals(swa_multi * m, uint64_t * out3) {
  if (m == nullptr || out3 == nullptr) { return SWA_E_ARG; }
  out3[0] = out3[1] = out3[2] = 0;
  for (swa_ctx * c : m->ctx) {
    uint64_t t[3] = {0, 0, 0};
    (void)swa_dn_graph_totals(c, t);
    out3[0] += t[0]; out3[1] += t[1]; out3[2] = std::max(out3[2], t[2]);
  }
  return SWA_OK;
}

// ---- d >= 2 on several GPUs: the fused scan (scan.hip) divided by ownership of the pool --------------------------------
// What src/scan.cc:221-256 does with threads: the targets of one search shared out.  Rank r scans the amplicons i with
// (i >> 5) % world == r (swa_scan_set_ownership) against every seed of the batch.  One host thread enqueues the launch
// sequence on every rank's stream first and then finishes rank by rank (no thread per generation: starting and joining
// `world` threads costs more than a late generation's kernels); a rank whose pair arrays overflowed is redone alone, a rank
// with no amplicon of its own at or above lowest_unswarmed launches nothing.  Every rank's hits arrive sorted through its
// pinned mirror; they are merged here by (seed index, id).  No RCCL call: the same code serves ranks on one device and
// ranks on distinct devices.
extern "C" int swa_multi_scan_begin(swa_multi * m) {
  if (m == nullptr) { return SWA_E_ARG; }
  m->scan_ready = false;
  const int world = (int)m->ctx.size();
  const int rc = on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    SWA_TRY(swa_scan_set_ownership(c, (uint32_t)r, (uint32_t)world));
    return swa_scan_begin(c);
  });
  if (rc != SWA_OK) { return rc; }
  m->scan_ready = true;
  m->scan_batches = 0;
  m->scan_hits.clear();
  return SWA_OK;
}

extern "C" int swa_multi_scan_fetch(swa_multi * m, uint32_t * hit_seedidx, uint32_t * hit_ids, uint32_t * hit_diffs, uint32_t cap) {
  if (m == nullptr) { return SWA_E_ARG; }
  const size_t got = m->scan_hits.size();
  if (got > cap) { return fail(m, SWA_E_CAPACITY, "swa_multi_scan_fetch: hit buffer too small"); }
  if (got != 0 && (hit_ids == nullptr || hit_diffs == nullptr)) { return fail(m, SWA_E_ARG, "swa_multi_scan_fetch: null buffer"); }
  for (size_t k = 0; k < got; ++k) {
    if (hit_seedidx != nullptr) { hit_seedidx[k] = m->scan_hits[k].sidx; }
    hit_ids[k] = m->scan_hits[k].id;
    hit_diffs[k] = m->scan_hits[k].diff;
  }
  return SWA_OK;
}

extern "C" int swa_multi_scan_batch(swa_multi * m, uint32_t nseeds, const uint32_t * seeds, const uint32_t * radii, uint32_t lowest_unswarmed,
                                    int first_generation, int no_cluster_breaking, uint32_t * hit_seedidx, uint32_t * hit_ids,
                                    uint32_t * hit_diffs, uint32_t cap, uint32_t * nhits) {
  if (m == nullptr) { return SWA_E_ARG; }
  if (!m->scan_ready) { return fail(m, SWA_E_ARG, "swa_multi_scan_batch: call swa_multi_scan_begin first"); }
  const int world = (int)m->ctx.size();
  const swa_scan_call call{nseeds, seeds, radii, lowest_unswarmed, first_generation, no_cluster_breaking};
  if (const char * why = swa_scan_check_call(m->ctx[0], call, hit_seedidx, hit_ids, hit_diffs, cap, nhits)) {
    return fail(m, SWA_E_ARG, std::string("swa_multi_scan_batch: ") + why);
  }
  for (int r = 0; r < world; ++r) {                            // (a rank that was given other work since swa_multi_scan_begin)
    swa_ctx * c = m->ctx[(size_t)r];
    if (!c->up.scan_ready || c->scan_world != (uint32_t)world || c->scan_rank != (uint32_t)r) {
      return fail(m, SWA_E_ARG, "swa_multi_scan_batch: rank " + std::to_string(r) + " has left the scan, call swa_multi_scan_begin again");
    }
  }
  ++m->scan_batches;
  m->scan_hits.clear();
  const uint32_t n = m->ctx[0]->db.n;
  std::vector<char> active((size_t)world, 0);
  auto failed = [&](int r, int rc) { return fail(m, rc, "rank " + std::to_string(r) + ": " + swa_last_error(m->ctx[(size_t)r])); };
  // 1. every rank with a share: its launch sequence on its stream
  for (int r = 0; r < world; ++r) {
    swa_ctx * c = m->ctx[(size_t)r];
    uint32_t share[2] = {0, 0};
    (void)swa_scan_share_for(n, lowest_unswarmed, (uint32_t)r, (uint32_t)world, share);
    c->scan_perm.clear();
    if (share[0] == 0 && world > 1) {
      if (first_generation != 0) { c->scan_cand_bound = 0; }   // (as swa_scan_enqueue leaves a rank that launches nothing)
      continue;
    }
    active[(size_t)r] = 1;
    ++c->scan_launches;
    const int rc = swa_scan_enqueue(c, call);
    if (rc != SWA_OK) {
      for (int k = 0; k < r; ++k) { if (active[(size_t)k]) { (void)hipSetDevice(m->devices[(size_t)k]); (void)hipStreamSynchronize(m->ctx[(size_t)k]->stream); } }
      return failed(r, rc);
    }
  }
  // 2. rank by rank: wait, read its mirror (a rank that overflowed its pair arrays repeats its sequence alone)
  int bad_rank = -1, bad_rc = SWA_OK;
  uint64_t total = 0;
  for (int r = 0; r < world; ++r) {
    if (!active[(size_t)r]) { continue; }
    uint32_t got = 0;
    const int rc = swa_scan_finish(m->ctx[(size_t)r], call, &got);
    if (rc != SWA_OK && bad_rank < 0) { bad_rank = r; bad_rc = rc; }     // (the others are still waited for)
    total += got;
  }
  if (bad_rank >= 0) { return failed(bad_rank, bad_rc); }
  // 3. the ranks' sorted lists merged by (seed index, id)
  m->scan_hits.reserve(total);
  for (int r = 0; r < world; ++r) {
    if (!active[(size_t)r]) { continue; }
    swa_ctx * c = m->ctx[(size_t)r];
    const auto * triples = reinterpret_cast<const swa_multi::ScanHit *>(c->scan_host.data() + 4);
    const size_t before = m->scan_hits.size();
    for (uint32_t at : c->scan_perm) { m->scan_hits.push_back(triples[at]); }
    std::inplace_merge(m->scan_hits.begin(), m->scan_hits.begin() + (std::ptrdiff_t)before, m->scan_hits.end(),
                       [](const swa_multi::ScanHit & x, const swa_multi::ScanHit & y) { return x.sidx != y.sidx ? x.sidx < y.sidx : x.id < y.id; });
  }
  *nhits = (uint32_t)total;
  if (total > cap) { return fail(m, SWA_E_CAPACITY, "swa_multi_scan_batch: hit buffer too small, use swa_multi_scan_fetch"); }
  return swa_multi_scan_fetch(m, hit_seedidx, hit_ids, hit_diffs, cap);
}

// single (sub)seed convenience form
extern "C" int swa_multi_scan_step(swa_multi * m, uint32_t seed, uint32_t lowest_unswarmed, int first_generation, uint32_t radius,
                                   int no_cluster_breaking, uint32_t * hit_ids, uint32_t * hit_diffs, uint32_t cap, uint32_t * nhits) {
  if (m == nullptr) { return SWA_E_ARG; }
  std::vector<uint32_t> idx(cap > 0 ? cap : 1);
  return swa_multi_scan_batch(m, 1, &seed, &radius, lowest_unswarmed, first_generation, no_cluster_breaking, idx.data(), hit_ids, hit_diffs, cap, nhits);
}

// out3 = {q-gram comparisons and aligned pairs, summed over the ranks (the shares partition the candidates: the numbers of
// a single context), launch sequences = batches since swa_multi_scan_begin (not a sum)}
extern "C" int swa_multi_scan_totals(swa_multi * m, uint64_t * out3) {
  if (m == nullptr || out3 == nullptr) { return SWA_E_ARG; }
  if (!m->scan_ready) { return fail(m, SWA_E_ARG, "swa_multi_scan_totals: no scan state"); }
  out3[0] = out3[1] = 0;
  out3[2] = m->scan_batches;
  for (size_t r = 0; r < m->ctx.size(); ++r) {
    uint64_t t[3] = {0, 0, 0};
    const int rc = swa_scan_totals(m->ctx[r], t);
    if (rc != SWA_OK) { return fail(m, rc, "rank " + std::to_string(r) + ": " + swa_last_error(m->ctx[r])); }
    out3[0] += t[0]; out3[1] += t[1];
  }
  return SWA_OK;
}

// ---- B5 on several GPUs: the -u alignments divided among the ranks -------------------------------------------------------
// Whether (member, seed) aligns with some CIGAR depends on the pair alone, and every rank holds the whole database: rank r
// aligns the contiguous pairs [bounds[r], bounds[r + 1]) with swa_nw_batch on its own context, one host thread a rank, so the
// one-thread host parts of a batch (planning a slice, assembling it) overlap as well as the kernels — also between ranks that
// share a device.  No collective, no kernel of its own: the tier kernels of nw_trace.hip on every rank's stream.
namespace {

// floor(r * W / world) without the 64-bit product: r * (W / world) <= W, and r, W % world < 64
uint64_t nw_share_target(uint64_t W, uint32_t r, uint32_t world) { return (W / world) * r + (W % world) * r / world; }

// bounds[0 .. world] of swa_multi_nw_bounds_for and at[r] = P(bounds[r]), the weight below every boundary.  strict: an id
// >= n is refused; else such a pair weighs nothing (the rank that gets it refuses it, and so names itself).
int nw_bounds(uint64_t npairs, const uint32_t * d_ids, const uint32_t * q_ids, const uint32_t * seqlen, uint32_t n, uint32_t world,
              bool strict, uint64_t * bounds, uint64_t * at) {
  auto weight = [&](uint64_t k) -> uint64_t {
    return d_ids[k] < n && q_ids[k] < n ? (uint64_t)seqlen[d_ids[k]] + seqlen[q_ids[k]] : 0;
  };
  uint64_t W = 0;
  for (uint64_t k = 0; k < npairs; ++k) {
    if (strict && (d_ids[k] >= n || q_ids[k] >= n)) { return SWA_E_ARG; }
    W += weight(k);
  }
  bounds[0] = 0;
  if (at != nullptr) { at[0] = 0; }
  uint32_t r = 1;
  uint64_t P = 0;
  for (uint64_t k = 0; k <= npairs && r < world; ++k) {      // P = P(k)
    while (r < world && P >= nw_share_target(W, r, world)) { bounds[r] = k; if (at != nullptr) { at[r] = P; } ++r; }
    if (k < npairs) { P += weight(k); }
  }
  bounds[world] = npairs;
  if (at != nullptr) { at[world] = W; }
  return SWA_OK;
}

}  // namespace

extern "C" int swa_multi_nw_bounds_for(uint64_t npairs, const uint32_t * d_ids, const uint32_t * q_ids, const uint32_t * seqlen, uint32_t n,
                                       uint32_t world, uint64_t * bounds) {
  if (world < 1 || world > 64 || bounds == nullptr) { return SWA_E_ARG; }
  if (npairs > 0 && (d_ids == nullptr || q_ids == nullptr || seqlen == nullptr)) { return SWA_E_ARG; }
  return nw_bounds(npairs, d_ids, q_ids, seqlen, n, world, true, bounds, nullptr);
}

extern "C" int swa_multi_nw_batch(swa_multi * m, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t npairs,
                                  const uint32_t * d_ids, const uint32_t * q_ids, uint32_t * diffs, uint32_t * columns,
                                  uint64_t * cigar_end, char * cigar, uint64_t cigar_cap, uint64_t * cigar_total) {
  if (m == nullptr) { return SWA_E_ARG; }
  const int world = (int)m->ctx.size();
  if (npairs > 0 && (d_ids == nullptr || q_ids == nullptr || diffs == nullptr || columns == nullptr || cigar_end == nullptr)) {
    return fail(m, SWA_E_ARG, "swa_multi_nw_batch: null result array");
  }
  swa_ctx * c0 = m->ctx[0];
  if (npairs > 0 && c0->db.seqs == nullptr) { return fail(m, SWA_E_ARG, "swa_multi_nw_batch: no database resident"); }
  int rc = swa_nw_host_seqlen(c0);
  if (rc != SWA_OK) { return fail(m, rc, std::string("rank 0: ") + swa_last_error(c0)); }
  std::vector<uint64_t> bounds((size_t)world + 1, 0), at((size_t)world + 1, 0), total((size_t)world, 0);
  (void)nw_bounds(npairs, d_ids, q_ids, c0->up.nw_seqlen.data(), c0->db.n, (uint32_t)world, false, bounds.data(), at.data());
  // A rank's text goes where no other rank writes: into the caller's buffer at the weight of the lower slices — a pair's
  // weight bounds its CIGAR — where the slice's whole bound fits there, else into a buffer of the rank's own.
  std::vector<std::unique_ptr<char[]>> own((size_t)world);
  rc = on_all(m, [&](int r) {
    swa_ctx * c = m->ctx[(size_t)r];
    const uint64_t lo = bounds[(size_t)r], count = bounds[(size_t)r + 1] - lo;
    if (count == 0) {                                          // nothing launched: the counters of a batch without pairs
      for (auto & v : c->nw_totals) { v = 0; }
      c->nw_text_full = 0;
      return (int)SWA_OK;
    }
    const uint64_t room = at[(size_t)r + 1] - at[(size_t)r];
    char * text = nullptr;
    if (cigar != nullptr && at[(size_t)r + 1] <= cigar_cap) { text = cigar + at[(size_t)r]; }
    else {
      own[(size_t)r].reset(new (std::nothrow) char[std::max<uint64_t>(room, 1)]);
      if (!own[(size_t)r]) { return swa_fail_msg(c, SWA_E_NOMEM, "swa_multi_nw_batch: no memory for the slice's CIGAR text"); }
      text = own[(size_t)r].get();
    }
    return swa_nw_batch(c, mismatch, gapopen, gapextend, count, d_ids + lo, q_ids + lo, diffs + lo, columns + lo, cigar_end + lo, text, room,
                        &total[(size_t)r]);
  });
  if (rc != SWA_OK) { return rc; }
  // the texts together in rank order (a slice only ever moves down: its text is no longer than its bound), every rank's
  // ends raised by the totals of the ranks below it
  uint64_t sum = 0;
  for (int r = 0; r < world; ++r) {
    const uint64_t lo = bounds[(size_t)r], hi = bounds[(size_t)r + 1], bytes = total[(size_t)r];
    if (lo == hi) { continue; }
    if (sum != 0) { for (uint64_t k = lo; k < hi; ++k) { cigar_end[k] += sum; } }
    const char * src = own[(size_t)r] ? own[(size_t)r].get() : cigar + at[(size_t)r];
    if (cigar != nullptr && bytes != 0 && sum < cigar_cap && src != cigar + sum) {
      std::memmove(cigar + sum, src, (size_t)std::min<uint64_t>(bytes, cigar_cap - sum));
    }
    sum += bytes;
  }
  if (cigar_total != nullptr) { *cigar_total = sum; }
  if (sum > cigar_cap || (cigar == nullptr && sum > 0)) {
    return fail(m, SWA_E_CAPACITY, "swa_multi_nw_batch: CIGAR buffer too small (*cigar_total = need)");
  }
  return SWA_OK;
}

// the counters of the last swa_multi_nw_batch summed over the ranks (a rank's own: swa_nw_batch_* on swa_multi_ctx(m, r))
extern "C" int swa_multi_nw_batch_totals(swa_multi * m, uint64_t * out4) {
  if (m == nullptr || out4 == nullptr) { return SWA_E_ARG; }
  for (int i = 0; i < 4; ++i) { out4[i] = 0; }
  for (swa_ctx * c : m->ctx) { uint64_t t[4] = {}; (void)swa_nw_batch_totals(c, t); for (int i = 0; i < 4; ++i) { out4[i] += t[i]; } }
  return SWA_OK;
}

extern "C" int swa_multi_nw_batch_tiers(swa_multi * m, uint64_t * out8) {
  if (m == nullptr || out8 == nullptr) { return SWA_E_ARG; }
  for (int i = 0; i < 8; ++i) { out8[i] = 0; }
  for (swa_ctx * c : m->ctx) { uint64_t t[8] = {}; (void)swa_nw_batch_tiers(c, t); for (int i = 0; i < 8; ++i) { out8[i] += t[i]; } }
  return SWA_OK;
}

extern "C" int swa_multi_nw_batch_text_full(swa_multi * m, uint64_t * out1) {
  if (m == nullptr || out1 == nullptr) { return SWA_E_ARG; }
  *out1 = 0;
  for (swa_ctx * c : m->ctx) { uint64_t t = 0; (void)swa_nw_batch_text_full(c, &t); *out1 += t; }
  return SWA_OK;
}

// debug entry: k_merge_sorted_lists on lists from the host, launched as dn_graph_on_root launches it
extern "C" int swa_merge_sorted_lists(swa_ctx * ctx, const uint64_t * keys, const uint32_t * vals, const uint64_t * at, uint32_t world,
                                      uint64_t * out_keys, uint32_t * out_vals) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (world < 1 || world > 64) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_merge_sorted_lists: world outside 1 .. 64"); }
  if (at == nullptr || at[0] != 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_merge_sorted_lists: at[0] must be 0"); }
  for (uint32_t r = 0; r < world; ++r) {
    if (at[r + 1] < at[r]) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_merge_sorted_lists: at[] descends"); }
  }
  const uint64_t all = at[world];
  if (all == 0) { return SWA_OK; }
  if (keys == nullptr || vals == nullptr || out_keys == nullptr || out_vals == nullptr) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_merge_sorted_lists: null buffer");
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  // [all keys | merged keys] and [all values | merged values], as rank 0 lays them out
  swa_dbuf kbuf, vbuf;
  auto run = [&]() -> int {
    SWA_TRY(swa_reserve(ctx, kbuf, (2 * all + 2) * sizeof(uint64_t)));
    SWA_TRY(swa_reserve(ctx, vbuf, (2 * all + 2) * sizeof(uint32_t)));
    auto * dk = static_cast<unsigned long long *>(kbuf.ptr);
    auto * dv = static_cast<uint32_t *>(vbuf.ptr);
    SWA_HIP(ctx, hipMemcpyAsync(dk, keys, all * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    SWA_HIP(ctx, hipMemcpyAsync(dv, vals, all * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    MergeArgs ma{};
    ma.keys = dk; ma.vals = dv; ma.world = world;
    for (uint32_t r = 0; r <= world; ++r) { ma.at[r] = at[r]; }
    ma.out_keys = dk + all + 1; ma.out_vals = dv + all + 1;
    SWA_TRY(launch_merge(ctx, ma));
    SWA_HIP(ctx, hipMemcpyAsync(out_keys, ma.out_keys, all * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipMemcpyAsync(out_vals, ma.out_vals, all * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWA_OK;
  };
  const int rc = run();
  if (rc != SWA_OK) { (void)hipStreamSynchronize(ctx->stream); }
  swa_release(kbuf);
  swa_release(vbuf);
  return rc;
}
