// cluster_d1.cpp — host side of the d = 1 path: greedy single-linkage agglomeration
// over the GPU-returned neighbour lists, fastidious bookkeeping and grafting, writers.
//
// Behaviour mirrors algo_d1_run's host part (src/algod1.cc:1185-1280 clustering,
// 214-336 grafting, 755-1095 writers) so that every output file is byte-identical.
// Shape is this repo's own: swarms are contiguous ranges of one member array (the reference threads a
// linked list through ampinfo[].next); grafting moves the members of the light swarms behind those of
// the heavy swarm that won them, so a printed swarm stays one range (lay_out_grafts).
#include "hostdb.h"
#include "nw_host.h"
#include "out.h"
#include "uclust_gpu.h"

#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <omp.h>
#include <parallel/algorithm>
#include <string>
#include <vector>

struct swa_d1_result {
  uint32_t n = 0;
  swa_vec<uint32_t> swarmid, parent, generation;   // (swa_vec: sized without a serial fill, see hostdb.h)
  swa_vec<uint32_t> order;                  // amplicons in printed order: discovery order, swarm after swarm, until grafts are laid out
  struct Swarm {                            // plain data: the table of 1.6 M swarms (10 M amplicons) is filled by all threads
    uint64_t mass, sumlen;
    uint32_t seed, size, singletons, maxgen;
    // printed members = order[begin, end): the swarm's own, order[begin, own_end), then those of the light swarms grafted
    // onto it, in graft order (own_end == end without grafts).  An attached swarm keeps its bounds, inside its heavy swarm's.
    uint32_t begin, own_end, end;
    uint32_t attached;                      // this (light) swarm hangs on another one: it prints nothing itself
  };
  static constexpr Swarm empty_swarm() { return Swarm{0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; }
  swa_vec<Swarm> swarms;
  swa_vec<uint32_t> graft_cand;             // per amplicon, after swa_d1_graft
  uint64_t swarmcount_adjusted = 0;
  uint32_t largest = 0, maxgen = 0;
  std::string error;
  // The clustering made on the GPU (swa_d1_cluster_resident) brings home only what the swarms file needs — the member
  // order and the swarms' bounds.  swarmid / parent / generation / graft_cand and the per-swarm sums (mass, length,
  // singletons, deepest generation) are fetched and computed when somebody asks: -i, -s, -u, -w, --fastidious and the
  // accessors (need_details).  A plain `swarm -d 1 -o` never does.
  swa_ctx * lazy_ctx = nullptr;
  const swa_hostdb * lazy_db = nullptr;
  bool details = true;
  uint32_t detail_fetches = 0;              // downloads of swarm id / generation / parent made for this result (swa_d1_result_detail_fetches)
  // the winning (child << 32 | parent) pairs of swa_d1_graft / swa_d1_result_install_graft, until they are written into
  // graft_cand: at once, or when the details of a lazy result are made after all (keep_winners)
  swa_vec<uint64_t> winners;
  // how the grafts came (swa_d1_result_graft_route): 0 none, 1 decided on the host, 2 installed, 3 an adopted layout
  uint32_t graft_route = 0;
  // swa_d1_result_prepare: order and the download area of the swarms' bounds sized ahead — and pinned, when the runtime agreed
  swa_vec<uint32_t> begin_tmp;
  bool prepared = false, pinned_order = false, pinned_begin = false;
  ~swa_d1_result() {
    if (pinned_order) { swa_host_unpin(order.data()); }
    if (pinned_begin) { swa_host_unpin(begin_tmp.data()); }
  }
};

namespace {

// v[i] = value for all i, by all threads (first touch of a freshly sized array included)
template <class V, class T>
void fill_parallel(V & v, size_t n, T value) {
  v.resize(n);
  auto * p = v.data();
#pragma omp parallel for schedule(static) if (n >= 100000) num_threads(swa_host_team())
  for (int64_t i = 0; i < (int64_t)n; ++i) { p[i] = value; }
}

template <typename F>
void for_each_member(const swa_d1_result * r, const swa_d1_result::Swarm & s, F && f) {
  for (uint32_t k = s.begin; k < s.end; ++k) { f(r->order[k]); }
}

// what a swarm costs a writer that walks its members: its own and those of the light swarms grafted onto it (which print
// nothing themselves) — swa_format_in_weighted_pieces
inline uint64_t printed_members(const swa_d1_result * r, size_t k) {
  const auto & s = r->swarms[k];
  return s.attached != 0 ? 0u : 1u + (s.end - s.begin);
}

// SWARM_AMD_CLUSTER_TIMING: what a phase took since the one before it
struct Laps {
  const bool on = std::getenv("SWARM_AMD_CLUSTER_TIMING") != nullptr;
  double last = omp_get_wtime();
  void operator()(const char * what) {
    if (!on) { return; }
    const double now = omp_get_wtime();
    std::fprintf(stderr, "[cluster] %-24s %8.3f ms\n", what, 1000.0 * (now - last));
    last = now;
  }
};

// order[first, last) added to a swarm's mass, length and singletons; its deepest generation raised to that of
// order[first, own_last) — a heavy swarm's stays its own, like the reference
void add_members(const swa_d1_result * r, swa_d1_result::Swarm & sw, uint32_t first, uint32_t last, uint32_t own_last) {
  const swa_hostdb * db = r->lazy_db;
  const auto & gen = r->generation;
  for (uint32_t k = first; k < last; ++k) {
    // (members of consecutive swarms are consecutive in `order`: what the sums read 16 members ahead is asked for now)
    if (k + 16u < r->n) { const uint32_t f = r->order[k + 16u]; __builtin_prefetch(&db->abundance[f]); __builtin_prefetch(&db->seqlen[f]); __builtin_prefetch(&gen[f]); }
    const uint32_t a = r->order[k];
    sw.mass += db->abundance[a];
    sw.sumlen += db->seqlen[a];
    if (db->abundance[a] == 1) { ++sw.singletons; }
    if (k < own_last) { sw.maxgen = std::max(sw.maxgen, gen[a]); }
  }
}

// graft_cand = the winners' candidates and nobody else's (the losers' are withdrawn)
void keep_winners(swa_d1_result * r) {
  fill_parallel(r->graft_cand, r->n, (uint32_t)SWA_NO_AMPLICON);
  const int64_t g64 = (int64_t)r->winners.size();
#pragma omp parallel for schedule(static) if (g64 >= 100000) num_threads(swa_host_team())
  for (int64_t i = 0; i < g64; ++i) { r->graft_cand[(uint32_t)(r->winners[(size_t)i] >> 32)] = (uint32_t)r->winners[(size_t)i]; }
  swa_vec<uint64_t>().swap(r->winners);
}

constexpr uint32_t kParallelOutputFrom = 200000;   // amplicons from which the writers format on several threads
constexpr uint32_t kParallelUclustFrom = 200;      // -u aligns every member against its seed: worth it much earlier

// number of every swarm in the output files (attached = grafted swarms have none: they are printed
// with the swarm they were grafted to)
std::vector<uint32_t> output_numbers(const swa_d1_result * r) {
  std::vector<uint32_t> number(r->swarms.size());
  uint32_t next = 0;
  for (size_t k = 0; k < r->swarms.size(); ++k) { number[k] = next; if (r->swarms[k].attached == 0) { ++next; } }
  return number;
}

// swarmid / parent / generation from HBM and the sums of every swarm (see swa_d1_result); false when the context that holds
// them has moved on
bool need_details(const swa_d1_result * cr) {
  if (cr->details) { return true; }
  if (cr->lazy_ctx == nullptr) { return false; }
  auto * r = const_cast<swa_d1_result *>(cr);
  const uint32_t n = r->n;
  r->swarmid.resize(n); r->parent.resize(n); r->generation.resize(n);
  // (the fetch faults the arrays' pages in on the library's worker threads before the copies land: swa_touch_pages)
  if (swa_d1_cluster_fetch(r->lazy_ctx, r->swarmid.data(), r->generation.data(), r->parent.data()) != SWA_OK) {
    r->error = swa_last_error(r->lazy_ctx);
    return false;
  }
  // the winners' candidates (the losers' withdrawn): in HBM behind an adopted layout, else the pairs that were installed
  if (r->graft_route == 3) {
    r->graft_cand.resize(n);
    if (swa_d1_graft_candidates_fetch(r->lazy_ctx, r->graft_cand.data()) != SWA_OK) { r->error = swa_last_error(r->lazy_ctx); return false; }
  } else { keep_winners(r); }
  // (an attached swarm's sums are its own: its range lies inside its heavy swarm's, which counts those members too)
#pragma omp parallel for schedule(dynamic, 1024) num_threads(swa_host_team())
  for (int64_t s = 0; s < (int64_t)r->swarms.size(); ++s) {
    auto & sw = r->swarms[(size_t)s];
    add_members(r, sw, sw.begin, sw.end, sw.own_end);
  }
  ++r->detail_fetches;
  r->details = true;
  r->lazy_ctx = nullptr;                                    // (nothing of the context is needed from here on)
  return true;
}

// what an entry point returns when the details could not be had: the fetch's own failure (SWA_E_DEVICE, text in
// swa_d1_result_error) — never SWA_E_ARG, which the command line reports as "Unable to open ... file" 
int details_failed(const swa_d1_result * r) { return r->error.empty() ? SWA_E_ARG : SWA_E_DEVICE; }

}  // namespace

// ---- the same clustering, computed without the serial walk --------------------------------
// The greedy loop above is equivalent to three order-free statements (i -> j = "j is in i's
// neighbour list"; ids are db order):
//   swarm(v)      = seed(v) = the smallest id among v and everything that reaches v.
//                   (That id m is a seed: anything claiming m earlier would reach v and be smaller.
//                   When m's turn comes nothing on a path m -> ... -> v is taken, for the same
//                   reason, so m's walk claims v.)
//   generation(v) = the distance from seed(v) to v (every path from the seed to v stays inside
//                   the swarm, again because a node taken earlier would make v's seed smaller).
//   parent(v)     = the smallest id u with u -> v and generation(u) = generation(v) - 1 (a
//                   generation is expanded in ascending id order and the first to reach v keeps it).
// Members are listed by (generation, id), swarms by seed id.  Each statement is a data-parallel
// fixed point / sweep over the CSR, which is what the many cores of a GPU host are for: used for
// large inputs, and checked against the serial walk in tests/test_host_logic.py.
namespace {

inline void atomic_min_u32(uint32_t * addr, uint32_t value) {
  uint32_t seen = __atomic_load_n(addr, __ATOMIC_RELAXED);
  while (value < seen && !__atomic_compare_exchange_n(addr, &seen, value, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
}

void cluster_by_fixed_points(const swa_hostdb * db, const uint64_t * offsets, const uint32_t * neighbours,
                             swa_d1_result * r) {
  const uint32_t n = db->n;
  const int64_t n64 = (int64_t)n;
  constexpr uint32_t kUnset = SWA_NO_AMPLICON;
  Laps lap;
  // 1. seed(v): push the smaller label along every edge until nothing changes
  swa_vec<uint32_t> label(n);
  swa_vec<uint8_t> active, next_active;
  fill_parallel(active, n, (uint8_t)1);
  fill_parallel(next_active, n, (uint8_t)0);
#pragma omp parallel for schedule(static) num_threads(swa_host_team())
  for (int64_t v = 0; v < n64; ++v) { label[(size_t)v] = (uint32_t)v; }
  for (bool changed = true; changed;) {
    changed = false;
#pragma omp parallel for schedule(dynamic, 8192) reduction(|| : changed) num_threads(swa_host_team())
    for (int64_t u = 0; u < n64; ++u) {
      if (active[(size_t)u] == 0) { continue; }
      active[(size_t)u] = 0;
      const uint32_t lu = __atomic_load_n(&label[(size_t)u], __ATOMIC_RELAXED);
      for (uint64_t e = offsets[u]; e < offsets[u + 1]; ++e) {
        const uint32_t v = neighbours[e];
        if (lu < __atomic_load_n(&label[v], __ATOMIC_RELAXED)) {
          atomic_min_u32(&label[v], lu);
          __atomic_store_n(&next_active[v], (uint8_t)1, __ATOMIC_RELAXED);
          changed = true;
        }
      }
    }
    active.swap(next_active);              // (next_active is all zero again: every visited flag was cleared)
  }
  lap("labels");
  // 2. generation(v): level-synchronous distances from the seeds inside their swarms;
  //    parent(v): smallest id of the previous level that points at v
  auto & gen = r->generation;
  auto & parent = r->parent;
#pragma omp parallel for schedule(static) num_threads(swa_host_team())
  for (int64_t v = 0; v < n64; ++v) { gen[(size_t)v] = label[(size_t)v] == (uint32_t)v ? 0u : kUnset; parent[(size_t)v] = kUnset; }
  // Frontier by frontier (not a sweep over all amplicons per level: swarms can be hundreds of generations
  // deep): the nodes of level - 1 are a list; a node is claimed for `level` by exactly one thread (compare and
  // swap on its generation), which appends it to that thread's piece of the next list; parents are the
  // smallest claiming or co-claiming id, by atomic minimum.
  {
    const int nthreads = std::max(1, swa_host_team());
    std::vector<std::vector<uint32_t>> piece((size_t)nthreads);
    std::vector<uint32_t> frontier, next;
    // level 0 = the seeds
#pragma omp parallel num_threads(swa_host_team())
    {
      auto & mine = piece[(size_t)omp_get_thread_num()];
      mine.clear();
#pragma omp for schedule(static) nowait
      for (int64_t v = 0; v < n64; ++v) { if (label[(size_t)v] == (uint32_t)v) { mine.push_back((uint32_t)v); } }
    }
    auto gather_pieces = [&](std::vector<uint32_t> & into) {
      std::vector<size_t> at((size_t)nthreads + 1, 0);
      for (int t = 0; t < nthreads; ++t) { at[(size_t)t + 1] = at[(size_t)t] + piece[(size_t)t].size(); }
      into.resize(at[(size_t)nthreads]);
#pragma omp parallel for schedule(static, 1) num_threads(swa_host_team())
      for (int t = 0; t < nthreads; ++t) { std::copy(piece[(size_t)t].begin(), piece[(size_t)t].end(), into.begin() + (std::ptrdiff_t)at[(size_t)t]); }
    };
    gather_pieces(frontier);
    for (uint32_t level = 1; !frontier.empty(); ++level) {
      const int64_t fsize = (int64_t)frontier.size();
#pragma omp parallel num_threads(swa_host_team())
      {
        auto & mine = piece[(size_t)omp_get_thread_num()];
        mine.clear();
#pragma omp for schedule(dynamic, 2048) nowait
        for (int64_t k = 0; k < fsize; ++k) {
          const uint32_t u = frontier[(size_t)k];
          const uint32_t lu = label[u];
          for (uint64_t e = offsets[u]; e < offsets[u + 1]; ++e) {
            const uint32_t v = neighbours[e];
            if (label[v] != lu) { continue; }
            uint32_t gv = __atomic_load_n(&gen[v], __ATOMIC_RELAXED);
            if (gv == kUnset) {
              if (__atomic_compare_exchange_n(&gen[v], &gv, level, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { mine.push_back(v); gv = level; }
            }
            if (gv == level) { atomic_min_u32(&parent[v], u); }   // (gv holds the winner's value after a lost exchange)
          }
        }
      }
      gather_pieces(next);
      frontier.swap(next);
    }
  }
  lap("generations + parents");
  // 3. swarms in seed order, members by (generation, id)
  // swarm number of every seed = number of seeds before it: per-block counts, prefix, numbering
  swa_vec<uint32_t> sid_of_seed(n);
  const int blocks = std::max(1, swa_host_team());
  std::vector<uint32_t> seeds_before((size_t)blocks + 1, 0);
#pragma omp parallel for schedule(static, 1) num_threads(swa_host_team())
  for (int b = 0; b < blocks; ++b) {
    uint32_t c = 0;
    for (int64_t v = n64 * b / blocks; v < n64 * (b + 1) / blocks; ++v) { c += label[(size_t)v] == (uint32_t)v ? 1u : 0u; }
    seeds_before[(size_t)b + 1] = c;
  }
  for (int b = 0; b < blocks; ++b) { seeds_before[(size_t)b + 1] += seeds_before[(size_t)b]; }
  const uint32_t nswarms = seeds_before[(size_t)blocks];
#pragma omp parallel for schedule(static, 1) num_threads(swa_host_team())
  for (int b = 0; b < blocks; ++b) {
    uint32_t next = seeds_before[(size_t)b];
    for (int64_t v = n64 * b / blocks; v < n64 * (b + 1) / blocks; ++v) {
      if (label[(size_t)v] == (uint32_t)v) { sid_of_seed[(size_t)v] = next++; }
    }
  }
  fill_parallel(r->swarms, nswarms, swa_d1_result::empty_swarm());
  std::vector<uint32_t> size(nswarms, 0);
#pragma omp parallel for schedule(static) num_threads(swa_host_team())
  for (int64_t v = 0; v < n64; ++v) {
    const uint32_t sid = sid_of_seed[label[(size_t)v]];
    r->swarmid[(size_t)v] = sid;
    __atomic_fetch_add(&size[sid], 1u, __ATOMIC_RELAXED);
  }
  uint32_t at = 0;
  for (uint32_t s = 0; s < nswarms; ++s) {
    auto & sw = r->swarms[s];
    sw.begin = at;
    at += size[s];
    sw.end = sw.begin;                      // filled below (used as the cursor)
  }
  lap("swarm table");
  r->order.resize(n);
#pragma omp parallel for schedule(static) num_threads(swa_host_team())
  for (int64_t v = 0; v < n64; ++v) {
    auto & sw = r->swarms[r->swarmid[(size_t)v]];
    r->order[__atomic_fetch_add(&sw.end, 1u, __ATOMIC_RELAXED)] = (uint32_t)v;
  }
  lap("placement");
  uint32_t largest = 0, maxgen = 0;
#pragma omp parallel for schedule(dynamic, 1024) num_threads(swa_host_team())
  for (int64_t s = 0; s < (int64_t)nswarms; ++s) {
    const auto & sw = r->swarms[(size_t)s];
    std::sort(r->order.begin() + sw.begin, r->order.begin() + sw.end, [&](uint32_t x, uint32_t y) {
      return gen[x] != gen[y] ? gen[x] < gen[y] : x < y;
    });
  }
  // (the sums read ahead in `order`, into the next swarms' members: after the sorts)
#pragma omp parallel for schedule(dynamic, 1024) reduction(max : largest) reduction(max : maxgen) num_threads(swa_host_team())
  for (int64_t s = 0; s < (int64_t)nswarms; ++s) {
    auto & sw = r->swarms[(size_t)s];
    sw.seed = r->order[sw.begin];
    sw.own_end = sw.end;
    sw.size = sw.end - sw.begin;
    add_members(r, sw, sw.begin, sw.end, sw.end);
    largest = std::max(largest, sw.size);
    maxgen = std::max(maxgen, sw.maxgen);
  }
  r->largest = largest;
  r->maxgen = maxgen;
  lap("member order + sums");
}

}  // namespace

// ---- the same result from the network that is still in HBM (cluster_gpu.hip) ------------------
// swa_d1_network_resident left the CSR on the device; the three order-free statements above are evaluated
// there and only swarm / generation / parent / member order come back.  The per-swarm sums stay here.
static int cluster_resident(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result ** out, swa_d1_result * prepared = nullptr);

extern "C" int swa_d1_result_prepare(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result ** out) {
  if (ctx == nullptr || db == nullptr || out == nullptr) { return SWA_E_ARG; }
  auto * r = new swa_d1_result();
  *out = r;
  r->n = db->n;
  r->prepared = true;
  if (db->n == 0) { return SWA_OK; }
  r->order.resize(db->n);
  r->begin_tmp.resize((size_t)db->n + 1);
  // (pinning faults the pages in and maps them for the device; when it is refused the downloads are staged copies as before)
  r->pinned_order = swa_host_pin(ctx, r->order.data(), (size_t)db->n * sizeof(uint32_t)) == SWA_OK;
  // (the swarms' bounds are a few hundred kilobytes of an array sized for the worst case: not pinned, not touched — 40 MB of
  // pages this process would otherwise fault in and take apart again)
  if (std::getenv("SWARM_AMD_CLUSTER_TIMING") != nullptr) { std::fprintf(stderr, "[cluster] result arrays pinned: order %d, bounds %d\n", (int)r->pinned_order, (int)r->pinned_begin); }
  return SWA_OK;
}

extern "C" int swa_d1_cluster_resident_prepared(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result * prepared) {
  if (prepared == nullptr || !prepared->prepared || db == nullptr || prepared->n != db->n) { return SWA_E_ARG; }
  swa_d1_result * same = prepared;
  return cluster_resident(ctx, db, &same, prepared);
}

// The result owns everything it returns: swarm / generation / parent are fetched and the sums made before this returns, and
// the context may be destroyed or used for the next database afterwards.
extern "C" int swa_d1_cluster_resident(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result ** out) {
  const int rc = cluster_resident(ctx, db, out);
  if (rc != SWA_OK) { return rc; }
  return swa_d1_result_detach(*out);
}

// The command line's form: the details stay in HBM until an accessor, the grafting or one of -i -s -u -w asks for them (a
// plain `swarm -d 1 -o` never does: 160 MB of downloads and a pass over all members less).  The CALLER keeps `ctx` alive and
// its clustering untouched until swa_d1_result_detach (or the result's release).
extern "C" int swa_d1_cluster_resident_lazy(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result ** out) {
  return cluster_resident(ctx, db, out);
}

extern "C" int swa_d1_result_detach(swa_d1_result * r) {
  if (r == nullptr) { return SWA_E_ARG; }
  if (r->n == 0) { r->lazy_ctx = nullptr; return SWA_OK; }
  return need_details(r) ? SWA_OK : details_failed(r);
}

extern "C" const char * swa_d1_result_error(const swa_d1_result * r) { return r == nullptr ? "" : r->error.c_str(); }

static int cluster_resident(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result ** out, swa_d1_result * prepared) {
  if (ctx == nullptr || db == nullptr || out == nullptr) { return SWA_E_ARG; }
  auto * r = prepared != nullptr ? prepared : new swa_d1_result();
  *out = r;
  const uint32_t n = db->n;
  r->n = n;
  Laps lap;
  if (n == 0) { return SWA_OK; }
  if (prepared == nullptr) {
    r->order.resize(n);                                     // (every entry is written by the download below)
    r->begin_tmp.resize((size_t)n + 1);
  }
  swa_vec<uint32_t> & begin = r->begin_tmp;
  lap("result arrays");
  uint32_t nswarms = 0;
  const int rc = swa_d1_cluster_device(ctx, nullptr, nullptr, nullptr, r->order.data(), begin.data(), n, &nswarms);
  if (rc != SWA_OK) { r->error = swa_last_error(ctx); return rc; }
  lap("device + download");
  r->lazy_ctx = ctx;
  r->lazy_db = db;
  r->details = false;
  r->swarms.resize(nswarms);
  uint32_t largest = 0;
#pragma omp parallel for schedule(static) reduction(max : largest) num_threads(swa_host_team())
  for (int64_t s = 0; s < (int64_t)nswarms; ++s) {
    auto & sw = r->swarms[(size_t)s];
    sw = swa_d1_result::empty_swarm();
    sw.begin = begin[(size_t)s];
    sw.own_end = sw.end = begin[(size_t)s + 1];
    sw.seed = r->order[sw.begin];
    sw.size = sw.end - sw.begin;
    largest = std::max(largest, sw.size);
  }
  r->largest = largest;
  r->maxgen = swa_d1_cluster_maxgen(ctx);
  r->swarmcount_adjusted = r->swarms.size();
  lap("swarm table");
  return SWA_OK;
}

// ---- clustering (src/algod1.cc:1185-1280, process_seed 673-718) ------------------------
extern "C" int swa_d1_cluster(const swa_hostdb * db, const uint64_t * offsets, const uint32_t * neighbours,
                              swa_d1_result ** out) {
  if (db == nullptr || out == nullptr || (db->n > 0 && (offsets == nullptr))) { return SWA_E_ARG; }
  auto * r = new swa_d1_result();
  *out = r;
  const uint32_t n = db->n;
  r->n = n;
  r->lazy_db = db;
  fill_parallel(r->swarmid, n, (uint32_t)SWA_NO_AMPLICON);
  fill_parallel(r->parent, n, (uint32_t)SWA_NO_AMPLICON);
  fill_parallel(r->generation, n, 0u);
  fill_parallel(r->graft_cand, n, (uint32_t)SWA_NO_AMPLICON);
  // large inputs on a many-core host: the order-free formulation (SWARM_AMD_CLUSTER=serial|parallel
  // overrides the choice)
  {
    const char * mode = std::getenv("SWARM_AMD_CLUSTER");
    const bool force_parallel = mode != nullptr && std::strcmp(mode, "parallel") == 0;
    const bool force_serial = mode != nullptr && std::strcmp(mode, "serial") == 0;
    if (force_parallel || (!force_serial && n >= 500000 && swa_host_team() >= 8)) {
      cluster_by_fixed_points(db, offsets, neighbours, r);
      r->swarmcount_adjusted = r->swarms.size();
      return SWA_OK;
    }
  }
  r->order.reserve(n);
  // The walk is a chain of dependent random reads (row of s -> ids -> swarmid of each id), so the
  // loop touches as little as possible per amplicon: the visited test reads swarmid[] only,
  // parent / generation go to arrays aligned with `order` (sequential writes) and are scattered
  // afterwards in one pass of independent writes, and the rows of the next generation are
  // prefetched while the current one is expanded.
  std::vector<uint32_t> order_parent, order_generation;
  order_parent.reserve(n);
  order_generation.reserve(n);
  std::vector<uint64_t> fresh;                // (id << 32 | parent): sorting it sorts by id
  for (uint32_t seed = 0; seed < n; ++seed) {
    if (r->swarmid[seed] != SWA_NO_AMPLICON) { continue; }
    const uint32_t sid = (uint32_t)r->swarms.size();
    swa_d1_result::Swarm sw = swa_d1_result::empty_swarm();
    sw.seed = seed;
    sw.begin = (uint32_t)r->order.size();
    r->swarmid[seed] = sid;
    r->order.push_back(seed);
    order_parent.push_back(SWA_NO_AMPLICON);
    order_generation.push_back(0);
    uint32_t gen_begin = sw.begin;            // current generation = order[gen_begin, gen_end)
    uint32_t gen_end = gen_begin + 1;
    uint32_t gen = 0;
    while (gen_begin < gen_end) {
      fresh.clear();
      for (uint32_t k = gen_begin; k < gen_end; ++k) {
        const uint32_t s = r->order[k];
        const uint64_t row_end = offsets[s + 1];
        for (uint64_t e = offsets[s]; e < row_end; ++e) {
          if (e + 8 < row_end) { __builtin_prefetch(&r->swarmid[neighbours[e + 8]]); }
          const uint32_t amp = neighbours[e];
          if (r->swarmid[amp] == SWA_NO_AMPLICON) {
            r->swarmid[amp] = sid;
            __builtin_prefetch(&offsets[amp]);
            fresh.push_back(((uint64_t)amp << 32) | s);
          }
        }
      }
      // each generation joins the swarm sorted by db index (= abundance, then header)
      std::sort(fresh.begin(), fresh.end());
      for (const uint64_t f : fresh) {
        r->order.push_back((uint32_t)(f >> 32));
        order_parent.push_back((uint32_t)f);
        order_generation.push_back(gen + 1);
      }
      gen_begin = gen_end;
      gen_end = (uint32_t)r->order.size();
      if (!fresh.empty()) { ++gen; }
    }
    sw.own_end = sw.end = (uint32_t)r->order.size();
    sw.size = sw.end - sw.begin;
    r->largest = std::max(r->largest, sw.size);
    r->maxgen = std::max(r->maxgen, gen);
    r->swarms.push_back(sw);
  }
  // per-amplicon results and per-swarm sums: independent gathers / scatters over `order`
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t a = r->order[k];
    r->parent[a] = order_parent[k];
    r->generation[a] = order_generation[k];
  }
  for (auto & sw : r->swarms) { add_members(r, sw, sw.begin, sw.end, sw.end); }   // (the deepest generation with them)
  r->swarmcount_adjusted = r->swarms.size();
  return SWA_OK;
}

extern "C" void swa_d1_result_free(swa_d1_result * r) { delete r; }

extern "C" void swa_d1_result_summary(const swa_d1_result * r, uint64_t * out4) {
  out4[0] = r->swarmcount_adjusted;
  out4[1] = r->largest;
  out4[2] = r->maxgen;
  out4[3] = r->swarms.size();
}

extern "C" const uint32_t * swa_d1_result_swarmid(const swa_d1_result * r) { return need_details(r) ? r->swarmid.data() : nullptr; }
extern "C" const uint32_t * swa_d1_result_parent(const swa_d1_result * r) { return need_details(r) ? r->parent.data() : nullptr; }
extern "C" const uint32_t * swa_d1_result_generation(const swa_d1_result * r) { return need_details(r) ? r->generation.data() : nullptr; }

// ---- fastidious bookkeeping (src/algod1.cc:1291-1328) -----------------------------------
extern "C" int swa_d1_light_flags(const swa_d1_result * r, int64_t boundary, uint8_t * is_light, uint64_t * stats5) {
  if (!need_details(r) && r->n != 0) { return details_failed(r); }      // (without the masses every swarm would look light)
  uint64_t light_swarms = 0, light_amps = 0, light_nt = 0;
  const int64_t nswarms = (int64_t)r->swarms.size();
  // (every amplicon belongs to one swarm: the flags are independent writes; 3 M swarms at 10 M amplicons with 30 % light ones)
#pragma omp parallel for schedule(static) reduction(+ : light_swarms, light_amps, light_nt) if (r->n >= kParallelOutputFrom) num_threads(swa_host_team())
  for (int64_t i = 0; i < nswarms; ++i) {
    const auto & s = r->swarms[(size_t)i];
    const bool light = s.mass < (uint64_t)boundary;
    if (light) { ++light_swarms; light_amps += s.size; light_nt += s.sumlen; }
    for (uint32_t k = s.begin; k < s.end; ++k) { is_light[r->order[k]] = light ? 1 : 0; }
  }
  stats5[0] = light_swarms;
  stats5[1] = light_amps;
  stats5[2] = light_nt;
  stats5[3] = r->swarms.size() - light_swarms;
  stats5[4] = r->n - light_amps;
  return SWA_OK;
}

// ---- grafting (src/algod1.cc:214-241 attach, 274-336 attach_candidates) -----------------
// The reference hangs a light swarm's member list behind its heavy swarm's.  Here a printed swarm is one range of `order`, so
// G grafts in chain order — heavy[i] wins light[i]; by heavy swarm, a heavy swarm's in the order it won them — are a new
// layout of the swarms in `order`, in closed form (own[s] = end - begin before the grafts):
//   grown[s]            = own[s] + own[] of the light swarms s won
//   new_begin[printed]  = exclusive scan, in swarm order, of (attached ? 0 : grown)
//   new_begin[light[i]] = new_begin[h] + own[h] + own[] of the light swarms h = heavy[i] won before light[i]
//   every swarm's members move as one block: order'[new_begin[s] + k] = order[begin[s] + k]
// Whoever decided the grafts — swa_d1_graft here, swa_d1_graft_device on the GPU — ends in this form (the GPU can make the
// layout as well: swa_d1_result_adopt_layout).
namespace {

// Every swarm's bounds, size and `attached` from a layout whose member order is in place; where the details are on the host
// the grafted members join their heavy swarm's mass, length and singletons (else need_details sums over [begin, end)).
void set_layout(swa_d1_result * r, const uint32_t * new_begin, const uint32_t * grown, const uint8_t * attached) {
  const int64_t w64 = (int64_t)r->swarms.size();
  // (the heavy swarms come first and hold all the grafted members: not one thread's share)
#pragma omp parallel for schedule(dynamic, 1024) if (r->n >= kParallelOutputFrom) num_threads(swa_host_team())
  for (int64_t s = 0; s < w64; ++s) {
    auto & sw = r->swarms[(size_t)s];
    const uint32_t own = sw.end - sw.begin;
    sw.begin = new_begin[s];
    sw.own_end = sw.begin + own;
    sw.end = sw.begin + grown[s];
    sw.size = grown[s];
    sw.attached = attached[s];
    if (r->details) { add_members(r, sw, sw.own_end, sw.end, sw.own_end); }
  }
}

// The layout of `grafts` grafts in chain order, made and taken over.  SWA_E_ARG, a text in r->error and nothing changed for
// what is no graft of this result: grafts on top of grafts, a swarm it does not have, heavy swarms that do not ascend, a light
// swarm listed twice, a heavy swarm that is somebody's light swarm.
int lay_out_grafts(swa_d1_result * r, const uint32_t * heavy, const uint32_t * light, uint32_t grafts) {
  auto refuse = [&](const char * why) { r->error = std::string("not a graft of this clustering: ") + why; return SWA_E_ARG; };
  if (r->graft_route != 0) { return refuse("the result holds grafts already"); }
  const size_t w = r->swarms.size();
  const int64_t w64 = (int64_t)w, g64 = (int64_t)grafts;
  const bool wide = r->n >= kParallelOutputFrom;
  swa_vec<uint8_t> attached;
  fill_parallel(attached, w, (uint8_t)0);
  bool fits = true;
#pragma omp parallel for schedule(static) reduction(&& : fits) if (wide) num_threads(swa_host_team())
  for (int64_t i = 0; i < g64; ++i) {
    fits = fits && heavy[i] < w && light[i] < w && (i == 0 || heavy[i - 1] <= heavy[i]) &&
           __atomic_exchange_n(&attached[light[i]], (uint8_t)1, __ATOMIC_RELAXED) == 0;
  }
  if (!fits) { return refuse("a swarm it does not have, heavy swarms out of order or a light swarm twice"); }
#pragma omp parallel for schedule(static) reduction(&& : fits) if (wide) num_threads(swa_host_team())
  for (int64_t i = 0; i < g64; ++i) { fits = fits && attached[heavy[i]] == 0; }
  if (!fits) { return refuse("a swarm hangs on a swarm that is attached itself"); }
  // grown, and how far behind its heavy swarm's begin every light swarm lies: a heavy swarm's run of grafts by one thread
  swa_vec<uint32_t> grown(w), new_begin(w), behind(grafts);
#pragma omp parallel for schedule(static) if (wide) num_threads(swa_host_team())
  for (int64_t s = 0; s < w64; ++s) { grown[(size_t)s] = r->swarms[(size_t)s].end - r->swarms[(size_t)s].begin; }
#pragma omp parallel for schedule(dynamic, 4096) if (wide) num_threads(swa_host_team())
  for (int64_t i = 0; i < g64; ++i) {
    const uint32_t h = heavy[i];
    if (i > 0 && heavy[i - 1] == h) { continue; }           // (not the first of its run)
    uint32_t at = grown[h];
    for (int64_t j = i; j < g64 && heavy[j] == h; ++j) { behind[(size_t)j] = at; at += grown[light[j]]; }   // (no light swarm grows)
    grown[h] = at;
  }
  // where the printed swarms begin: a block's share goes behind the shares of the blocks before it
  const int blocks = wide ? std::max(1, swa_host_team()) : 1;
  std::vector<uint32_t> before((size_t)blocks + 1, 0);
#pragma omp parallel for schedule(static, 1) if (wide) num_threads(swa_host_team())
  for (int b = 0; b < blocks; ++b) {
    uint32_t c = 0;
    for (int64_t s = w64 * b / blocks; s < w64 * (b + 1) / blocks; ++s) { c += attached[(size_t)s] != 0 ? 0u : grown[(size_t)s]; }
    before[(size_t)b + 1] = c;
  }
  for (int b = 0; b < blocks; ++b) { before[(size_t)b + 1] += before[(size_t)b]; }
  uint32_t largest = 0;
#pragma omp parallel for schedule(static, 1) reduction(max : largest) if (wide) num_threads(swa_host_team())
  for (int b = 0; b < blocks; ++b) {
    uint32_t at = before[(size_t)b];
    for (int64_t s = w64 * b / blocks; s < w64 * (b + 1) / blocks; ++s) {
      if (attached[(size_t)s] != 0) { continue; }
      new_begin[(size_t)s] = at;
      at += grown[(size_t)s];
      largest = std::max(largest, grown[(size_t)s]);
    }
  }
#pragma omp parallel for schedule(static) if (wide) num_threads(swa_host_team())
  for (int64_t i = 0; i < g64; ++i) { new_begin[light[i]] = new_begin[heavy[i]] + behind[(size_t)i]; }
  // the move, swarm by swarm, and back into the result's own array (which may be pinned: it stays the one it was)
  if (grafts != 0) {
    swa_vec<uint32_t> moved(r->n);
#pragma omp parallel for schedule(dynamic, 1024) if (wide) num_threads(swa_host_team())
    for (int64_t s = 0; s < w64; ++s) {
      const auto & sw = r->swarms[(size_t)s];
      std::copy(r->order.begin() + sw.begin, r->order.begin() + sw.end, moved.begin() + new_begin[(size_t)s]);
    }
#pragma omp parallel for schedule(static) if (wide) num_threads(swa_host_team())
    for (int64_t k = 0; k < (int64_t)r->n; ++k) { r->order[(size_t)k] = moved[(size_t)k]; }
  }
  set_layout(r, new_begin.data(), grown.data(), attached.data());
  r->largest = largest;
  r->swarmcount_adjusted = w - grafts;
  return SWA_OK;
}

// grafts in chain order and the pairs that won them: laid out, the winners' candidates kept — now, or with the details
int install(swa_d1_result * r, const uint32_t * heavy, const uint32_t * light, const uint32_t * parent, const uint32_t * child,
            uint32_t grafts, uint32_t route) {
  const int64_t g64 = (int64_t)grafts;
  bool ours = true;
#pragma omp parallel for schedule(static) reduction(&& : ours) if (g64 >= 100000) num_threads(swa_host_team())
  for (int64_t i = 0; i < g64; ++i) { ours = ours && parent[i] < r->n && child[i] < r->n; }
  if (!ours) { r->error = "not a graft of this clustering: an amplicon it does not have"; return SWA_E_ARG; }
  const int rc = lay_out_grafts(r, heavy, light, grafts);
  if (rc != SWA_OK) { return rc; }
  r->winners.resize(grafts);
#pragma omp parallel for schedule(static) if (g64 >= 100000) num_threads(swa_host_team())
  for (int64_t i = 0; i < g64; ++i) { r->winners[(size_t)i] = ((uint64_t)child[i] << 32) | parent[i]; }
  if (r->details) { keep_winners(r); }
  r->graft_route = route;
  return SWA_OK;
}

}  // namespace

// What the reference's walk over the sorted (parent, child) pairs decides (src/algod1.cc:263-336), restated without the walk:
//   * a light swarm hangs on the parent of the FIRST pair, in sorted order, whose child is one of its members (later pairs
//     find it attached: their child's candidate is withdrawn) — a minimum over pair numbers, per light swarm;
//   * a heavy swarm prints the light swarms it won in the order of those winning pairs.
// So: the winning pair of every light swarm by an atomic minimum; the winners keyed (heavy swarm, number of the pair) and
// sorted — the grafts in chain order.  (3.2 M pairs, 1.5 M grafts at 10 M amplicons with 30 % light ones.)
extern "C" uint32_t swa_d1_graft(swa_d1_result * r, const uint32_t * graft_cand) {
  if (!need_details(r)) { return 0; }
  // (parent << 32 | child): sorting the packed pairs is the (parent, child) order of
  // src/algod1.cc:263-271, and a plain integer sort runs on all cores
  const int64_t n64 = (int64_t)r->n;
  const int blocks = std::max(1, swa_host_team());
  std::vector<uint64_t> before((size_t)blocks + 1, 0);        // candidates in the blocks before each block
  bool strays = false;
#pragma omp parallel for schedule(static, 1) reduction(|| : strays) num_threads(swa_host_team())
  for (int b = 0; b < blocks; ++b) {
    uint64_t c = 0;
    for (int64_t i = n64 * b / blocks; i < n64 * (b + 1) / blocks; ++i) {
      c += graft_cand[i] != SWA_NO_AMPLICON ? 1u : 0u;
      strays = strays || (graft_cand[i] != SWA_NO_AMPLICON && graft_cand[i] >= r->n);
    }
    before[(size_t)b + 1] = c;
  }
  if (strays) { r->error = "swa_d1_graft: a candidate that is no amplicon of this result"; return 0; }
  for (int b = 0; b < blocks; ++b) { before[(size_t)b + 1] += before[(size_t)b]; }
  swa_vec<uint64_t> pairs(before[(size_t)blocks]);
#pragma omp parallel for schedule(static, 1) num_threads(swa_host_team())
  for (int b = 0; b < blocks; ++b) {
    uint64_t at = before[(size_t)b];
    for (int64_t i = n64 * b / blocks; i < n64 * (b + 1) / blocks; ++i) {
      if (graft_cand[i] != SWA_NO_AMPLICON) { pairs[at++] = ((uint64_t)graft_cand[i] << 32) | (uint64_t)i; }
    }
  }
  __gnu_parallel::sort(pairs.begin(), pairs.end());
  const int64_t np64 = (int64_t)pairs.size();
  const bool wide = np64 >= 50000;
  swa_vec<uint32_t> first_pair;
  fill_parallel(first_pair, r->swarms.size(), 0xFFFFFFFFu);              // (pairs <= n < 2^32 - 1)
#pragma omp parallel for schedule(static) if (wide) num_threads(swa_host_team())
  for (int64_t at = 0; at < np64; ++at) {
    if (at + 16 < np64) { __builtin_prefetch(&r->swarmid[(uint32_t)pairs[at + 16]]); }
    uint32_t * slot = &first_pair[r->swarmid[(uint32_t)pairs[at]]];
    uint32_t seen = __atomic_load_n(slot, __ATOMIC_RELAXED);
    while ((uint32_t)at < seen && !__atomic_compare_exchange_n(slot, &seen, (uint32_t)at, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) { }
  }
  // the winners in pair order (a block's share goes behind the shares of the blocks before it)
  auto wins = [&](int64_t at) { return first_pair[r->swarmid[(uint32_t)pairs[at]]] == (uint32_t)at; };
#pragma omp parallel for schedule(static, 1) if (wide) num_threads(swa_host_team())
  for (int b = 0; b < blocks; ++b) {
    uint64_t c = 0;
    for (int64_t at = np64 * b / blocks; at < np64 * (b + 1) / blocks; ++at) { c += wins(at) ? 1u : 0u; }
    before[(size_t)b + 1] = c;
  }
  for (int b = 0; b < blocks; ++b) { before[(size_t)b + 1] += before[(size_t)b]; }
  const int64_t nwin = (int64_t)before[(size_t)blocks];
  swa_vec<uint64_t> keyed(nwin);                                        // heavy swarm << 32 | number of the winning pair
#pragma omp parallel for schedule(static, 1) if (wide) num_threads(swa_host_team())
  for (int b = 0; b < blocks; ++b) {
    uint64_t rank = before[(size_t)b];
    for (int64_t at = np64 * b / blocks; at < np64 * (b + 1) / blocks; ++at) {
      if (wins(at)) { keyed[rank++] = ((uint64_t)r->swarmid[(uint32_t)(pairs[at] >> 32)] << 32) | (uint64_t)at; }
    }
  }
  __gnu_parallel::sort(keyed.begin(), keyed.end());
  swa_vec<uint32_t> four((size_t)nwin * 4);
  uint32_t * heavy = four.data(), * light = heavy + nwin, * parent = light + nwin, * child = parent + nwin;
#pragma omp parallel for schedule(static) if (wide) num_threads(swa_host_team())
  for (int64_t i = 0; i < nwin; ++i) {
    const uint64_t pair = pairs[(uint32_t)keyed[(size_t)i]];
    heavy[i] = (uint32_t)(keyed[(size_t)i] >> 32);
    parent[i] = (uint32_t)(pair >> 32);
    child[i] = (uint32_t)pair;
    light[i] = r->swarmid[child[i]];
  }
  return install(r, heavy, light, parent, child, (uint32_t)nwin, 1) == SWA_OK ? (uint32_t)nwin : 0u;
}

// The grafts swa_d1_graft_device made (chain order), with the pairs that won them: what swa_d1_graft leaves.  On a result
// whose details are still on the device nothing is fetched: the sums and graft_cand are settled when somebody asks for the
// details (need_details); a plain -o never does.
extern "C" int swa_d1_result_install_graft(swa_d1_result * r, const uint32_t * heavy_swarm, const uint32_t * light_swarm,
                                           const uint32_t * parent, const uint32_t * child, uint32_t grafts) {
  if (r == nullptr || (grafts != 0 && (heavy_swarm == nullptr || light_swarm == nullptr || parent == nullptr || child == nullptr))) { return SWA_E_ARG; }
  return install(r, heavy_swarm, light_swarm, parent, child, grafts, 2);
}

// The layout swa_d1_graft_layout_device left in HBM adopted as the result's own: the printed member order into `order` (one
// DMA where swa_d1_result_prepare pinned it) and the three per-swarm arrays; nothing to decide, check or move here.
extern "C" int swa_d1_result_adopt_layout(swa_d1_result * r, swa_ctx * ctx) {
  if (r == nullptr || ctx == nullptr) { return SWA_E_ARG; }
  auto refuse = [&](const char * why) { r->error = std::string("swa_d1_result_adopt_layout: ") + why; return SWA_E_ARG; };
  uint64_t info[4] = {};
  if (swa_d1_graft_layout_info(ctx, info) != SWA_OK || info[0] == 0) { return refuse("the context holds no layout (swa_d1_graft_layout_device)"); }
  if (info[1] != r->n || info[2] != r->swarms.size()) { return refuse("the layout is of another clustering than this result"); }
  if (r->graft_route != 0) { return refuse("the result holds grafts already"); }
  const size_t w = r->swarms.size();
  swa_vec<uint32_t> new_begin(w), grown(w);
  swa_vec<uint8_t> attached(w);
  // (a result with its details on the host has its sums: the candidates are needed before anything is changed)
  swa_vec<uint32_t> kept;
  if (r->details) {
    kept.resize(r->n);
    if (swa_d1_graft_candidates_fetch(ctx, kept.data()) != SWA_OK) { r->error = swa_last_error(ctx); return SWA_E_DEVICE; }
  }
  uint64_t summary[3] = {};
  if (swa_d1_graft_layout_device(ctx, r->order.data(), new_begin.data(), grown.data(), attached.data(), (uint32_t)w, summary) != SWA_OK) {
    r->error = swa_last_error(ctx);
    return SWA_E_DEVICE;
  }
  set_layout(r, new_begin.data(), grown.data(), attached.data());
  if (r->details) { r->graft_cand.swap(kept); }
  r->largest = (uint32_t)summary[1];
  r->swarmcount_adjusted = summary[0];
  r->graft_route = 3;
  return SWA_OK;
}

extern "C" uint32_t swa_d1_result_graft_route(const swa_d1_result * r) { return r == nullptr ? 0u : r->graft_route; }

extern "C" uint32_t swa_d1_result_detail_fetches(const swa_d1_result * r) { return r == nullptr ? 0u : r->detail_fetches; }

// ---- writers ------------------------------------------------------------------------------
// -o / -r  (src/algod1.cc:790-846)
extern "C" int swa_d1_write_swarms(const swa_d1_result * r, const swa_hostdb * db, const char * path, int mothur,
                                   int usearch, int64_t append_abundance, int64_t differences) {
  BufOut o(path);
  if (!o.ok()) { return SWA_E_ARG; }
  if (mothur) { o.str("swarm_"); o.u64((uint64_t)differences); o.put('\t'); o.u64(r->swarmcount_adjusted); }
  // A member's identifier is three dependent random reads away — order[k] -> its entry pointer -> the entry -> the
  // header text — and the members of consecutive swarms are consecutive in `order`: what the walk will need 24, 16 and 8
  // members ahead is asked for now (without that: ~100 ms of cache misses at 10 M amplicons on 16 threads, lease r5f).
  const uint32_t * order = r->order.data();
  auto format_range = [&](BufOut & sink, size_t begin, size_t end) {
    // pass 1: where every printed swarm of this piece ends.  The printed swarms of a piece are one run of `order`, grafted
    // members included (lay_out_grafts).
    std::vector<uint32_t> ends;
    const uint32_t * ids = nullptr;
    if (begin < end) { ends.reserve(end - begin); }
    for (size_t k = begin; k < end; ++k) {
      const auto & s = r->swarms[k];
      if (s.attached != 0) { continue; }
      if (ids == nullptr) { ids = order + s.begin; }
      ends.push_back((uint32_t)(order + s.end - ids));
    }
    const size_t total = ends.empty() ? 0 : ends.back();
    // pass 2: a member's identifier is three dependent random reads away — its entry pointer, the entry, the header
    // text: what the walk needs 24, 16 and 8 members ahead is asked for now (without that: ~100 ms of cache misses at
    // 10 M amplicons on 16 threads, lease r5f)
    sink.reserve(std::min<size_t>(total * (db->longest_header + 2u) + 64, (size_t)8 << 20));
    size_t at = 0;
    for (const uint32_t stop : ends) {
      bool first = true;
      for (; at < stop; ++at) {
        if (at + 24 < total) { __builtin_prefetch(&db->ent[ids[at + 24]]); }
        if (at + 16 < total) { __builtin_prefetch(db->ent[ids[at + 16]]); }
        if (at + 8 < total) { __builtin_prefetch(db->hdr(ids[at + 8])); }
        if (mothur) { sink.put(first ? '\t' : ','); }
        else if (!first) { sink.put(' '); }
        first = false;
        swa_out::id(sink, db, ids[at], usearch != 0, append_abundance);
      }
      if (!mothur) { sink.put('\n'); }
    }
  };
  swa_format_in_weighted_pieces(o, r->swarms.size(), r->n >= kParallelOutputFrom, [&](size_t k) { return printed_members(r, k); }, format_range);
  if (mothur) { o.put('\n'); }
  return SWA_OK;
}

// -s  (src/algod1.cc:1040-1062): maxgen is printed twice for d = 1
extern "C" int swa_d1_write_stats(const swa_d1_result * r, const swa_hostdb * db, const char * path, int usearch) {
  if (!need_details(r)) { return details_failed(r); }
  BufOut o(path);
  if (!o.ok()) { return SWA_E_ARG; }
  for (const auto & s : r->swarms) {
    if (s.attached != 0) { continue; }
    o.u64(s.size); o.put('\t'); o.u64(s.mass); o.put('\t');
    swa_out::id_noabundance(o, db, s.seed, usearch != 0);
    o.put('\t'); o.u64(db->abundance[s.seed]); o.put('\t'); o.u64(s.singletons);
    o.put('\t'); o.u64(s.maxgen); o.put('\t'); o.u64(s.maxgen); o.put('\n');
  }
  return SWA_OK;
}

// -i  (src/algod1.cc:985-1037)
extern "C" int swa_d1_write_structure(const swa_d1_result * r, const swa_hostdb * db, const char * path, int usearch) {
  if (!need_details(r)) { return details_failed(r); }
  BufOut o(path);
  if (!o.ok()) { return SWA_E_ARG; }
  const std::vector<uint32_t> number = output_numbers(r);
  swa_format_in_weighted_pieces(o, r->swarms.size(), r->n >= kParallelOutputFrom, [&](size_t k) { return printed_members(r, k); }, [&](BufOut & sink, size_t begin, size_t end) {
    for (size_t k = begin; k < end; ++k) {
      const auto & s = r->swarms[k];
      if (s.attached != 0) { continue; }
      const uint32_t cluster_no = number[k];
      for_each_member(r, s, [&](uint32_t a) {
        if (a == s.seed) { return; }
        const uint32_t gp = r->graft_cand[a];
        if (gp != SWA_NO_AMPLICON) {
          swa_out::id_noabundance(sink, db, gp, usearch != 0);
          sink.put('\t');
          swa_out::id_noabundance(sink, db, a, usearch != 0);
          sink.put('\t'); sink.u64(2); sink.put('\t'); sink.u64(cluster_no + 1); sink.put('\t'); sink.u64(r->generation[gp] + 1);
          sink.put('\n');
        }
        const uint32_t p = r->parent[a];
        if (p != SWA_NO_AMPLICON) {
          swa_out::id_noabundance(sink, db, p, usearch != 0);
          sink.put('\t');
          swa_out::id_noabundance(sink, db, a, usearch != 0);
          sink.put('\t'); sink.u64(1); sink.put('\t'); sink.u64(cluster_no + 1); sink.put('\t'); sink.u64(r->generation[a]);
          sink.put('\n');
        }
      });
    }
  });
  return SWA_OK;
}

// -w  (src/algod1.cc:935-982 + db_fprintseq src/db.cc:925-943)
extern "C" int swa_d1_write_seeds(const swa_d1_result * r, const swa_hostdb * db, const char * path, int usearch) {
  if (!need_details(r)) { return details_failed(r); }
  BufOut o(path);
  if (!o.ok()) { return SWA_E_ARG; }
  std::vector<uint32_t> idx(r->swarms.size());
  std::iota(idx.begin(), idx.end(), 0u);
  std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
    const auto & a = r->swarms[x];
    const auto & b = r->swarms[y];
    if (a.mass != b.mass) { return a.mass > b.mass; }
    return std::strcmp(swa_out::hdr(db, a.seed), swa_out::hdr(db, b.seed)) < 0;
  });
  swa_format_in_pieces(o, idx.size(), r->n >= kParallelOutputFrom, [&](BufOut & sink, size_t begin, size_t end) {
    std::string line;
    for (size_t i = begin; i < end; ++i) {
      const auto & s = r->swarms[idx[i]];
      if (s.attached != 0) { continue; }
      sink.put('>');
      swa_out::id_new_abundance(sink, db, s.seed, s.mass, usearch != 0);
      sink.put('\n');
      swa_out::sequence(sink, db, s.seed, line);
    }
  });
  return SWA_OK;
}

// -j  (src/algod1.cc:755-788): rows ascending by target id (the C ABI already sorts them)
extern "C" int swa_d1_write_network(const swa_hostdb * db, const uint64_t * offsets, const uint32_t * neighbours,
                                    const char * path, int usearch, int64_t append_abundance) {
  BufOut o(path);
  if (!o.ok()) { return SWA_E_ARG; }
  std::vector<uint32_t> row;
  for (uint32_t i = 0; i < db->n; ++i) {
    row.assign(neighbours + offsets[i], neighbours + offsets[i + 1]);
    std::sort(row.begin(), row.end());
    for (uint32_t j : row) {
      swa_out::id(o, db, i, usearch != 0, append_abundance);
      o.put('\t');
      swa_out::id(o, db, j, usearch != 0, append_abundance);
      o.put('\n');
    }
  }
  return SWA_OK;
}

// -u  (src/algod1.cc:849-932): members in swarm order, each aligned against the seed
extern "C" int swa_d1_write_uclust(const swa_d1_result * r, const swa_hostdb * db, const char * path, int usearch,
                                   int64_t append_abundance, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend) {
  if (!need_details(r)) { return details_failed(r); }
  BufOut o(path);
  if (!o.ok()) { return SWA_E_ARG; }
  const std::vector<uint32_t> number = output_numbers(r);
  // one alignment per member: by far the most expensive writer, and every swarm is independent
  swa_format_in_weighted_pieces(o, r->swarms.size(), r->n >= kParallelUclustFrom, [&](size_t k) { return printed_members(r, k); }, [&](BufOut & sink, size_t begin, size_t end) {
    swa_nw_scratch scratch;
    for (size_t k = begin; k < end; ++k) {
      const auto & s = r->swarms[k];
      if (s.attached != 0) { continue; }
      const uint32_t cluster_no = number[k];
      swa_out::uclust_cluster(sink, db, cluster_no, s.size, s.seed, usearch != 0, append_abundance);
      for_each_member(r, s, [&](uint32_t a) {
        if (a == s.seed) { return; }
        const uint64_t nwdiff = swa_nw_align(db->words(a), db->seqlen[a],
                                             db->words(s.seed), db->seqlen[s.seed], mismatch, gapopen,
                                             gapextend, scratch);
        const std::string cigar = nwdiff > 0 ? swa_cigar(scratch.ops) : std::string();
        swa_out::uclust_hit(sink, db, cluster_no, a, s.seed, nwdiff, scratch.ops.size(), cigar.data(), cigar.size(), usearch != 0,
                            append_abundance);
      });
    }
  });
  return SWA_OK;
}

// -u with the alignments on the GPU (seam B5): the same lines as swa_d1_write_uclust, the pairs aligned by swa_nw_batch
extern "C" int swa_d1_write_uclust_gpu(swa_ctx * ctx, const swa_d1_result * r, const swa_hostdb * db, const char * path, int usearch,
                                       int64_t append_abundance, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend) {
  return swa_d1_write_uclust_with(swa_uclust_on_ctx(ctx), r, db, path, usearch, append_abundance, mismatch, gapopen, gapextend);
}

// ... by whoever the aligner names: that context, or the ranks of a swa_multi (uclust_multi.cpp)
int swa_d1_write_uclust_with(const swa_uclust_aligner & aligner, const swa_d1_result * r, const swa_hostdb * db, const char * path, int usearch,
                             int64_t append_abundance, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend) {
  if (!need_details(r)) { return details_failed(r); }
  BufOut o(path);
  if (!o.ok()) { return SWA_E_ARG; }
  const std::vector<uint32_t> number = output_numbers(r);
  return swa_uclust_gpu(aligner, db, o, r->swarms.size(), r->n >= kParallelUclustFrom, mismatch, gapopen, gapextend,
    [&](size_t k, auto && push) {
      const auto & s = r->swarms[k];
      if (s.attached != 0) { return; }
      for_each_member(r, s, [&](uint32_t a) { if (a != s.seed) { push(a, s.seed); } });
    },
    [&](size_t k) { return printed_members(r, k); },
    [&](BufOut & sink, size_t k, const swa_uclust_chunk & c, uint64_t p) {
      const auto & s = r->swarms[k];
      if (s.attached != 0) { return; }
      swa_out::uclust_cluster(sink, db, number[k], s.size, s.seed, usearch != 0, append_abundance);
      for_each_member(r, s, [&](uint32_t a) {
        if (a == s.seed) { return; }
        size_t len = 0;
        const char * cigar = swa_uclust_cigar(c, p, &len);
        swa_out::uclust_hit(sink, db, number[k], a, s.seed, c.diffs[p], c.columns[p], cigar, len, usearch != 0, append_abundance);
        ++p;
      });
    });
}
