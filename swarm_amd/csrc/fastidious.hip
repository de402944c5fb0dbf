// fastidious.hip — seam B2: the --fastidious second pass on gfx950 (algo_d1_run's fastidious branch,
// src/algod1.cc:1337-1467), a translation unit and a code object of its own.
//
// In this unit: the first level of the Bloom route (k_d1_flex), every kernel of the pair route (d1_fast.inc, on the grouped
// join of group_join.inc), MODE 1 of k_d1_probe (d1_probe.inc: the Bloom route's second level), the two routes, the plan
// and its reports, and the three entry points swa_d1_fastidious, _shard and _resident.  What it needs of the d = 1 step —
// the Zobrist table, the database-wide index, the abundance ranks, the amplicon lines, a grid size, an exclusive scan and the
// table rebuild — it calls in d1.hip through the block "what fastidious.hip takes from d1.hip" of swa_internal.h; the device
// code both units compile (no kernel among it) is d1_common.inc, and d1_probe.inc by MODE.  The grafting on the clustering
// in place (fast_graft.inc) is with cluster_gpu.hip.
#include "swa_internal.h"

#include <algorithm>
#include <cstdlib>
#include <memory>
#include <thread>
#include <type_traits>

namespace {

#include "wave_ops.inc"     // wave_lds_sync
#include "key_ops.inc"      // kEmpty, kKeyEmpty, mix64, window32
#include "group_join.inc"   // the grouped join of the pair route
#include "d1_common.inc"    // kWaves / kThreads / kQueueCap, line_fetch, anchor_key
#include "d1_probe.inc"     // swa_task, NetArgs, Slots, enumerate_variants, k_d1_probe: MODE 1 is launched (and instantiated) here

// ---- fastidious first level (algod1.cc:495-518 mark_light_var, 398-450 check_heavy_var) ---
struct FlexArgs {
  const uint64_t * seqs;
  const uint64_t * seq_off;
  const uint32_t * seqlen;
  const uint64_t * zobrist;
  uint32_t zlen;
  uint32_t maxwords;
  unsigned long long * fbits;     // the flexible Bloom, inverted polarity (bloomflex.cc:61-70)
  uint64_t fsize;                 // words
  double finv;                    // 1.0 / fsize
  const uint64_t * fpat;          // 65536 patterns with k bits
  const uint32_t * list;          // amplicon ids to process
  uint32_t count;
  swa_task * tasks;               // PASS 1: surviving (heavy, variant) pairs
  unsigned long long * task_counter;
  uint64_t task_cap;
  unsigned long long * variant_counter;
};

// (h >> 16) % fsize for an arbitrary (non power-of-two) fsize: bloomflex.cc:43-49.
// x < 2^48 is exact in a double, so the quotient estimate is off by at most one.
__device__ __forceinline__ uint64_t flex_word(uint64_t h, uint64_t fsize, double finv) {
  const uint64_t x = h >> 16;
  uint64_t q = (uint64_t)((double)x * finv);
  int64_t r = (int64_t)(x - q * fsize);
  if (r < 0) { r += (int64_t)fsize; }
  else if ((uint64_t)r >= fsize) { r -= (int64_t)fsize; }
  return (uint64_t)r;
}

// PASS 0: clear the pattern bits of every microvariant of a light amplicon.
// PASS 1: test every microvariant of a heavy amplicon, emit the survivors as tasks.
template <bool ZLDS, int PASS>
__global__ __launch_bounds__(kThreads) void k_d1_flex(const FlexArgs a) {
  extern __shared__ uint64_t lds[];
  uint64_t * zob_lds = lds;
  uint64_t * wave_base = lds + (ZLDS ? 4u * a.zlen : 0u);
  const uint32_t seed_words = a.maxwords + 2u;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  uint64_t * sw = wave_base + (size_t)wave * seed_words;
  // PASS 1 stages its surviving tasks in LDS and reserves space in the global task list in
  // bulk: one returning atomic per ~200 tasks instead of one per ballot (a single address
  // sustains only ~88 atomics/us, which bound this kernel)
  constexpr uint32_t kStage = 256;
  swa_task * stage = reinterpret_cast<swa_task *>(wave_base + (size_t)kWaves * seed_words) + (size_t)wave * kStage;
  uint32_t nstage = 0;
  if (ZLDS) {
    for (uint32_t i = threadIdx.x; i < 4u * a.zlen; i += kThreads) { zob_lds[i] = a.zobrist[i]; }
    __syncthreads();
  }
  const uint64_t * zob = ZLDS ? zob_lds : a.zobrist;
  const uint64_t lane_lt = (1ull << lane) - 1ull;
  unsigned long long nvar = 0;
  auto flush = [&]() {
    wave_lds_sync();
    unsigned long long base = 0;
    if (lane == 0) { base = atomicAdd(a.task_counter, (unsigned long long)nstage); }
    base = swa_shfl_u64(base, 0);
    for (uint32_t i = lane; i < nstage; i += 64u) {
      if (base + i < a.task_cap) { a.tasks[base + i] = stage[i]; }
    }
    nstage = 0;
    wave_lds_sync();
  };
  const uint32_t nwaves = gridDim.x * kWaves;
  for (uint32_t k = blockIdx.x * kWaves + wave; k < a.count; k += nwaves) {
    const uint32_t amp = a.list[k];
    const uint32_t len = a.seqlen[amp];
    const uint32_t nw = (len + 31u) >> 5;
    const uint64_t * gs = a.seqs + a.seq_off[amp];
    for (uint32_t w = lane; w < nw + 2u; w += 64u) { sw[w] = (w < nw) ? gs[w] : 0ull; }
    wave_lds_sync();
    (void)enumerate_variants(sw, len, zob, lane, [&](const Slots & s) {
      if (PASS == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (s.ok[i]) {
            atomicAnd(&a.fbits[flex_word(s.hs[i], a.fsize, a.finv)], ~(unsigned long long)a.fpat[s.hs[i] & 0xFFFFu]);
          }
          nvar += (unsigned long long)__popcll(__ballot(s.ok[i]));
        }
      } else {
        uint64_t word[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          word[i] = s.ok[i] ? (uint64_t)a.fbits[flex_word(s.hs[i], a.fsize, a.finv)] : ~0ull;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const bool pass = s.ok[i] && ((word[i] & a.fpat[s.hs[i] & 0xFFFFu]) == 0ull);   // bloomflex_get
          nvar += (unsigned long long)__popcll(__ballot(s.ok[i]));
          const uint64_t m = __ballot(pass);
          if (m != 0ull) {
            if (pass) {
              swa_task t;
              t.hash = s.hs[i]; t.heavy = amp; t.code = s.code[i];
              stage[nstage + (uint32_t)__popcll(m & lane_lt)] = t;
            }
            nstage += (uint32_t)__popcll(m);
            if (nstage > kStage - 64u) { flush(); }
          }
        }
      }
    });
    __builtin_amdgcn_wave_barrier();
  }
  if (PASS == 1 && nstage != 0u) { flush(); }
  if (lane == 0 && nvar != 0ull) { atomicAdd(a.variant_counter, nvar); }
}

#include "d1_fast.inc"

// the pass's device counters: an address for taking the addresses of members (kernel arguments, copies, fills), never to
// be dereferenced on the host
inline swa_fast_counters * fast_counters(const swa_ctx * ctx) { return static_cast<swa_fast_counters *>(ctx->d_fcounters.ptr); }

// the group type of the pair route (0 prefix, 1 suffix, 2 middle groups) as a template argument: f(std::integral_constant<int, type>{})
template <class F>
void with_group_type(int type, F && f) {
  if (type == 0) { f(std::integral_constant<int, 0>{}); }
  else if (type == 1) { f(std::integral_constant<int, 1>{}); }
  else { f(std::integral_constant<int, 2>{}); }
}

}  // namespace

// loads this translation unit's code object (see swa_ctx_warmup): an empty launch
void swa_warm_fastidious(swa_ctx * ctx) {
  hipLaunchKernelGGL(k_fast_length_classes, dim3(1), dim3(64), 0, ctx->stream, static_cast<const uint32_t *>(nullptr), 0u, 0u,
                     static_cast<uint32_t *>(nullptr));
}

// ---- the two routes -------------------------------------------------------------------------
// Chosen per PAIR of (heavy, light) amplicons by the shorter of the two lengths (and, under SWA_FAST_LONG=split or =pairs,
// the longer):
//   pair route  (both >= kFastMinLen, and both <= the cap under the split / pairs; d1_fast.inc): groups by shared
//               32-nt windows, exact "within two edits" test per pair, exact |V1(h) ∩ V1(x)| per surviving pair;
//   Bloom route (every other pair; the reference's own scheme): light-only table + Bloom,
//               every microvariant of every light amplicon clears its k pattern bits in the flexible
//               Bloom (atomicAnd: the reference's plain `&=` from many threads can lose a bit; -t 1 is
//               the specification), every microvariant of every heavy amplicon is tested, survivors
//               become 16-byte tasks, one wave per task re-runs the d=1 probe (k_d1_probe<MODE 1>).
// Both end in atomicMin on graft_cand = add_graft_candidate (src/algod1.cc:244-258) and one counter
// (swa_fast_counters::candidates; the layout of the pass's device counters: swa_internal.h).
static int fastidious_bloom_route(swa_ctx * ctx, uint32_t n_light, uint32_t n_heavy, uint64_t light_nt, uint32_t bloom_bits,
                                  uint32_t pair_route_min_len, uint32_t pair_route_max_len, bool zlds) {
  SWA_TRY(swa_ensure_full_index(ctx));                       // hashes of every amplicon, room for the table
  uint32_t k = static_cast<uint32_t>(0.4 * static_cast<double>(bloom_bits));
  if (k < 1) { k = 1; }
  uint64_t m = light_nt * 7ull * bloom_bits;
  if (m < 64) { m = 64; }
  const uint64_t n_bytes = ((m - 1) / 8) + 1;
  const uint64_t fsize = n_bytes >> 3;
  std::vector<uint64_t> fpat;
  swa_bloom_patterns(65536, k, fpat);
  SWA_TRY(swa_reserve(ctx, ctx->d_bloomflex, fsize * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_fpatterns, fpat.size() * sizeof(uint64_t)));
  const uint64_t maxv = 7ull * ctx->db.longest + 4ull;
  uint64_t task_cap = uint64_t(n_heavy) * maxv;
  uint64_t cap_limit = (1ull << 30) / sizeof(swa_task);                  // 1 GiB of tasks
  const char * env_cap = getenv("SWA_FAST_TASK_CAP");         // test hook: so many tasks instead (the floor below stays), exercise the batch loop
  if (env_cap != nullptr && atoll(env_cap) > 0) { cap_limit = (uint64_t)atoll(env_cap); }
  if (task_cap > cap_limit) { task_cap = cap_limit; }
  if (task_cap < maxv) { task_cap = maxv; }                  // (what makes a batch of task_cap / maxv heavy amplicons unable to overflow)
  ctx->fast_batches[2] = task_cap;
  SWA_TRY(swa_reserve(ctx, ctx->d_queue, task_cap * sizeof(swa_task)));
  SWA_HIP(ctx, hipMemcpyAsync(ctx->d_fpatterns.ptr, fpat.data(), fpat.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(ctx->d_bloomflex.ptr, 0xFF, fsize * sizeof(uint64_t), ctx->stream));
  ctx->ix.table_repurposed();                                // the table now holds the light amplicons of the bands only
  SWA_TRY(swa_d1_rebuild_table(ctx, static_cast<const uint8_t *>(ctx->d_light.ptr)));

  swa_fast_counters * fc = fast_counters(ctx);
  FlexArgs f{};
  f.seqs = ctx->db.seqs; f.seq_off = ctx->db.seq_off; f.seqlen = ctx->db.seqlen;
  f.zobrist = static_cast<const uint64_t *>(ctx->d_zobrist.ptr);
  f.zlen = ctx->zobrist_len;
  f.maxwords = (ctx->db.longest + 1u + 31u) >> 5;
  f.fbits = static_cast<unsigned long long *>(ctx->d_bloomflex.ptr);
  f.fsize = fsize;
  f.finv = 1.0 / static_cast<double>(fsize);
  f.fpat = static_cast<const uint64_t *>(ctx->d_fpatterns.ptr);
  f.tasks = static_cast<swa_task *>(ctx->d_queue.ptr);
  f.task_counter = &fc->batch_tasks;
  f.task_cap = task_cap;
  const size_t flex_lds = sizeof(uint64_t) * ((zlds ? 4ull * ctx->zobrist_len : 0ull) + kWaves * (size_t)(f.maxwords + 2u)) +
                          kWaves * 256 * sizeof(swa_task);
  // light side
  f.list = static_cast<const uint32_t *>(ctx->d_list_a.ptr);
  f.count = n_light;
  f.variant_counter = &fc->scratch;                          // (the reported totals are computed for all amplicons, not here)
  {
    const int grid = swa_grid_for(ctx, f.count, kWaves, 8);
    if (zlds) { hipLaunchKernelGGL((k_d1_flex<true, 0>), dim3(grid), dim3(kThreads), flex_lds, ctx->stream, f); }
    else { hipLaunchKernelGGL((k_d1_flex<false, 0>), dim3(grid), dim3(kThreads), flex_lds, ctx->stream, f); }
    SWA_HIP(ctx, hipGetLastError());
  }
  // heavy side
  NetArgs a{};
  a.seqs = ctx->db.seqs; a.seq_off = ctx->db.seq_off; a.seqlen = ctx->db.seqlen; a.abundance = ctx->db.abundance;
  a.zobrist = f.zobrist; a.zlen = ctx->zobrist_len;
  a.maxwords = f.maxwords;                                   // a microvariant can be one nt longer
  a.table = static_cast<const swa_slot *>(ctx->d_table.ptr);
  a.tmask = ctx->ix.table_size - 1;
  a.bloom = static_cast<const uint64_t *>(ctx->d_bloom.ptr);
  a.bmask = ctx->ix.bloom_words - 1;
  a.patterns = static_cast<const uint64_t *>(ctx->d_patterns.ptr);
  a.tasks = f.tasks;
  a.graft = static_cast<uint32_t *>(ctx->d_graft.ptr);
  a.cand_counter = &fc->candidates;
  a.fast_min_len = pair_route_min_len;
  a.fast_max_len = pair_route_max_len;
  const size_t probe_lds = sizeof(uint64_t) * ((zlds ? 4ull * ctx->zobrist_len : 0ull) + 1024ull +
                                               kWaves * ((size_t)(a.maxwords + 2u) + kQueueCap + kQueueCap / 2));
  // (the two words of a batch, cleared and read with one call each)
  static_assert(offsetof(swa_fast_counters, batch_variants) == offsetof(swa_fast_counters, batch_tasks) + sizeof(uint64_t), "batch_tasks, batch_variants: neighbours");
  uint64_t done = 0;
  uint64_t tasks_run = 0;                                    // tasks of the batches that ran to the end (a redone batch is counted once, as it ran)
  uint64_t batch = task_cap / maxv;                          // cannot overflow
  double rate = -1.0;                                        // observed tasks per heavy amplicon
  while (done < n_heavy) {
    uint64_t want = batch;
    if (rate >= 0.0) {                                       // optimistic sizing, overflow is detected below
      const double est = static_cast<double>(task_cap) / (4.0 * rate + 1.0);
      want = est > 4.0e9 ? 4000000000ull : static_cast<uint64_t>(est);
      if (want < batch) { want = batch; }
    }
    if (want > n_heavy - done) { want = n_heavy - done; }
    SWA_HIP(ctx, hipMemsetAsync(&fc->batch_tasks, 0, 2 * sizeof(uint64_t), ctx->stream));    // tasks + batch variants
    f.list = static_cast<const uint32_t *>(ctx->d_list_b.ptr) + done;
    f.count = static_cast<uint32_t>(want);
    f.variant_counter = &fc->batch_variants;
    const int grid = swa_grid_for(ctx, f.count, kWaves, 8);
    if (zlds) { hipLaunchKernelGGL((k_d1_flex<true, 1>), dim3(grid), dim3(kThreads), flex_lds, ctx->stream, f); }
    else { hipLaunchKernelGGL((k_d1_flex<false, 1>), dim3(grid), dim3(kThreads), flex_lds, ctx->stream, f); }
    SWA_HIP(ctx, hipGetLastError());
    uint64_t got[2] = {0, 0};
    SWA_HIP(ctx, hipMemcpyAsync(got, &fc->batch_tasks, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    rate = static_cast<double>(got[0]) / static_cast<double>(want);
    ++ctx->fast_batches[0];
    if (got[0] > task_cap) { ++ctx->fast_batches[1]; continue; }   // optimistic batch did not fit: redo it smaller
    if (got[0] > ctx->fast_batches[3]) { ctx->fast_batches[3] = got[0]; }
    tasks_run += got[0];
    if (got[0] > 0) {
      a.count = static_cast<uint32_t>(got[0]);
      const int pgrid = swa_grid_for(ctx, a.count, kWaves, 8);
      if (zlds) { hipLaunchKernelGGL((k_d1_probe<true, 1>), dim3(pgrid), dim3(kThreads), probe_lds, ctx->stream, a); }
      else { hipLaunchKernelGGL((k_d1_probe<false, 1>), dim3(pgrid), dim3(kThreads), probe_lds, ctx->stream, a); }
      SWA_HIP(ctx, hipGetLastError());
    }
    done += want;
  }
  // what swa_d1_fastidious_bloom_read reports: written once the route has run to its end
  ctx->fast_bloom[0] = fsize; ctx->fast_bloom[1] = m; ctx->fast_bloom[2] = k; ctx->fast_bloom[3] = bloom_bits; ctx->fast_bloom[4] = tasks_run;
  return SWA_OK;
}

// Every choice of the pass, from the longest sequence of the database alone (and the switches): what
// swa_d1_fastidious_shard launches and what swa_d1_fastidious_plan reports (host_tables.cpp: swa_fast_plan_for).
//   longest      pair kernel             count kernel
//   < 112        none: every pair on the Bloom route
//   112 .. 159   k_fast_pairs_lines<5>   k_fast_count_sites<5>   (a microvariant of 160 nt still fits 5 words)
//   160          k_fast_pairs_lines<5>   k_fast_count_sites<8>
//   161 .. 255   k_fast_pairs_lines<8>   k_fast_count_sites<8>
//   256          k_fast_pairs_lines<8>   k_fast_count, 4 waves x 4096 slots
//   257 .. 389   k_fast_pairs_lines<13>  k_fast_count, 4 waves x 4096
//   390 .. 416   k_fast_pairs_lines<13>  k_fast_count, 2 waves x 8192
//   417 .. 779   k_fast_pairs            k_fast_count, 2 waves x 8192
//   780 .. 1004  k_fast_pairs            k_fast_count, 1 wave x 16384
//   >= 1005      none: k_fast_count's set no longer fits 160 KB; Bloom route, Zobrist table in LDS up to 3070 nt
// SWA_FAST_LONG=split, longest > cap (= 1004, swa_fast_cap): the row of pair_longest, the longest sequence <= cap, with
// k_fast_pairs as the pair kernel, for the pairs whose two lengths lie in [112, cap]; the Bloom route for every other pair.
// SWA_FAST_LONG=pairs, longest > 1004: k_fast_pairs and k_fast_count_sites_words (4 / 2 / 1 waves, two staged sequences a
// wave and nothing else in LDS) for the pairs whose two lengths lie in [112, C], C = swa_fast_sites_cap() = 327 584 nt (or
// SWA_FAST_SITES_CAP, a test hook); where longer sequences exist, the split's division at C.
// SWA_FAST_COUNT=sites: k_fast_count_sites_words on the rows of k_fast_count (256 .. 1004), a comparison switch.
using FastPlan = swa_fast_plan;

// pair_longest, and how many amplicons are longer than the cap / can be half of a pair with one that is: a fact of the
// uploaded database and the cap (the split's, or the one of SWA_FAST_LONG=pairs: the environment is read at every call),
// read once for each
static int ensure_length_classes(swa_ctx * ctx, uint32_t cap) {
  if (ctx->up.d1.fast_classes_ready && ctx->up.d1.fast_classes_cap == cap) { return SWA_OK; }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(swa_reserve(ctx, ctx->d_fcounters, sizeof(swa_fast_counters)));
  uint32_t * out = fast_counters(ctx)->length_classes;
  SWA_HIP(ctx, hipMemsetAsync(out, 0, 4 * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_fast_length_classes, dim3(swa_grid_for(ctx, ctx->db.n, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.seqlen, ctx->db.n,
                     cap, out);
  SWA_HIP(ctx, hipGetLastError());
  uint32_t host[4] = {};
  SWA_HIP(ctx, hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->up.d1.fast_pair_longest = host[0]; ctx->up.d1.fast_n_long = host[1]; ctx->up.d1.fast_n_band = host[2];
  ctx->up.d1.fast_classes_ready = true;
  ctx->up.d1.fast_classes_cap = cap;
  return SWA_OK;
}

// SWA_FAST_SITES_CAP=n, a test hook: the cap of SWA_FAST_LONG=pairs (swa_fast_sites_cap_in_effect decides whether it counts)
static uint32_t fast_sites_cap_hook() {
  const char * env = getenv("SWA_FAST_SITES_CAP");
  const long long v = env != nullptr ? atoll(env) : 0;
  return v > 0 && v <= 0xFFFFFFFFll ? (uint32_t)v : 0u;
}

// long_cap: the cap of the division at the long end that the switches ask for (SWA_FAST_LONG=pairs: C; else the split's)
static int fast_plan(swa_ctx * ctx, FastPlan & p, uint32_t * long_cap = nullptr) {
  const char * env_route = getenv("SWA_FAST_BLOOM");          // test hook: the reference's scheme for every pair
  const char * env_fp = getenv("SWA_FAST_PAIRS");             // =words: the round-2 pair kernel, which walks the packed sequences — comparison switch
  const char * env_long = getenv("SWA_FAST_LONG");            // =split: keep the pair route for the pairs up to the cap when longer sequences exist
  const bool bloom = env_route != nullptr && env_route[0] == '1';
  const char * env_count = getenv("SWA_FAST_COUNT");          // =sites: k_fast_count_sites_words where k_fast_count would run — comparison switch
  const bool past_cap = !bloom && ctx->db.longest > swa_fast_cap();
  const bool split = env_long != nullptr && strcmp(env_long, "split") == 0 && past_cap;
  const bool pairs = env_long != nullptr && strcmp(env_long, "pairs") == 0 && past_cap;   // =pairs: the pair route serves the long sequences
  const uint32_t sites_cap = fast_sites_cap_hook();
  const uint32_t cap = pairs ? swa_fast_sites_cap_in_effect(sites_cap) : swa_fast_cap();
  if (long_cap != nullptr) { *long_cap = cap; }
  uint32_t pair_longest = 0;
  if ((split || pairs) && ctx->db.longest > cap) { SWA_TRY(ensure_length_classes(ctx, cap)); pair_longest = ctx->up.d1.fast_pair_longest; }
  p = swa_fast_plan_modes(ctx->db.longest, pair_longest, pairs ? 2 : (split ? 1 : 0), bloom, env_fp != nullptr && env_fp[0] == 'w',
                          env_count != nullptr && strcmp(env_count, "sites") == 0, sites_cap);
  return SWA_OK;
}

extern "C" int swa_d1_fastidious_plan(swa_ctx * ctx, uint32_t out[8]) {
  if (ctx == nullptr || out == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious_plan: no database is resident"); }
  FastPlan p{};
  SWA_TRY(fast_plan(ctx, p));
  swa_fast_plan_report(p, out);
  return SWA_OK;
}

// The report reads the length classes whenever the longest sequence exceeds the cap, with or without the switch: its
// first call after an upload then launches k_fast_length_classes and waits for it; later calls read the cached values.
extern "C" int swa_d1_fastidious_split(swa_ctx * ctx, uint32_t out[4]) {
  if (ctx == nullptr || out == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious_split: no database is resident"); }
  FastPlan p{};
  uint32_t cap = 0;
  SWA_TRY(fast_plan(ctx, p, &cap));
  const bool longer = ctx->db.longest > cap;
  if (longer) { SWA_TRY(ensure_length_classes(ctx, cap)); }
  out[0] = (uint32_t)p.long_mode;
  out[1] = cap;
  out[2] = longer ? ctx->up.d1.fast_pair_longest : ctx->db.longest;
  out[3] = longer ? ctx->up.d1.fast_n_long : 0u;
  return SWA_OK;
}

extern "C" int swa_d1_fastidious_totals(swa_ctx * ctx, uint64_t out[4]) {
  if (ctx == nullptr || out == nullptr) { return SWA_E_ARG; }
  for (int i = 0; i < 4; ++i) { out[i] = ctx->fast_totals[i]; }
  return SWA_OK;
}

extern "C" int swa_d1_fastidious_bloom_batches(swa_ctx * ctx, uint64_t out[4]) {
  if (ctx == nullptr || out == nullptr) { return SWA_E_ARG; }
  for (int i = 0; i < 4; ++i) { out[i] = ctx->fast_batches[i]; }
  return SWA_OK;
}

// copies: no kernel runs, nothing of the pass changes (the pass ended with the stream idle, so the words are settled)
extern "C" int swa_d1_fastidious_bloom_read(swa_ctx * ctx, uint64_t facts[8], uint64_t * words, uint64_t cap_words) {
  if (ctx == nullptr || facts == nullptr) { return SWA_E_ARG; }
  for (int i = 0; i < 8; ++i) { facts[i] = i < 5 ? ctx->fast_bloom[i] : 0; }
  const uint64_t fsize = ctx->fast_bloom[0];
  if (words == nullptr || fsize == 0) { return SWA_OK; }
  if (cap_words < fsize) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_fastidious_bloom_read: the filter has more words than the buffer"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_HIP(ctx, hipMemcpyAsync(words, ctx->d_bloomflex.ptr, fsize * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

static int fastidious_pair_route(swa_ctx * ctx, uint32_t n_light, uint32_t n_heavy, const FastPlan & plan) {
  const uint32_t slots = plan.slots;
  const int count_waves = plan.count_waves;
  const uint32_t n = ctx->db.n;
  swa_fast_counters * fc = fast_counters(ctx);
  if (n_light == 0 || n_heavy == 0) { return SWA_OK; }
  uint64_t asize_max = 64, asize_ends = 64;
  while (asize_max < 6ull * n_light) { asize_max <<= 1; }    // load <= 0.5 with three memberships per light amplicon (middle windows)
  while (asize_ends < 2ull * n_light) { asize_ends <<= 1; }  // one membership (prefix / suffix groups): a smaller table to clear and scan
  const uint64_t member_cap = 3ull * n_light + n_heavy;
  const uint64_t item_cap64 = 3ull * n_light + (3ull * n_light + n_heavy) / 2 + 64;
  const uint32_t item_cap = item_cap64 > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)item_cap64;
  SWA_TRY(join_reserve(ctx, asize_max, n, 3u, member_cap, item_cap));
  SWA_TRY(swa_reserve(ctx, ctx->d_scan_tmp, ((asize_max + kScanOffsetsTile - 1) / kScanOffsetsTile) * sizeof(uint64_t)));
  // (the offsets by the three-launch scan of d1_part.hip, not rocPRIM's as at d >= 2: DESIGN.md 3.5 has the measurement)
  auto scan = [&](const JoinTable & t) -> int { return swa_scan_offsets(ctx, t.tot, (uint32_t)t.asize, t.offsets); };
  if (ctx->fast_pair_cap == 0) {
    ctx->fast_pair_cap = 4ull * n_light + (1ull << 20);
    const char * env_cap = getenv("SWA_FAST_PAIR_CAP");       // test hook: start small, exercise the regrow path
    if (env_cap != nullptr && atoll(env_cap) > 0) { ctx->fast_pair_cap = (uint64_t)atoll(env_cap); }
  }
  uint64_t npairs = 0;
  const int pair_w = plan.pair_w;
  if (pair_w != 0) {
    SWA_TRY(swa_launch_abundance_rank(ctx));
    SWA_TRY(swa_ensure_lines(ctx));
  }
  JoinTable jt = join_table(ctx, asize_max, n, 3u);
  swa_t0(ctx, kTimePairs);
  for (int attempt = 0; attempt < 6; ++attempt) {
    SWA_TRY(swa_reserve(ctx, ctx->d_fpairs, ctx->fast_pair_cap * sizeof(uint64_t)));
    SWA_HIP(ctx, hipMemsetAsync(&fc->pairs, 0, sizeof(uint64_t), ctx->stream));
    SWA_HIP(ctx, hipMemsetAsync(jt.flags, 0, kJoinFlagWords * sizeof(uint32_t), ctx->stream));
    ctx->fast_totals[3] = (uint64_t)attempt + 1u;
    for (int type = 0; type < 3; ++type) {
      // one membership a light amplicon in the prefix / suffix groups, three (the middle window at 39, 40, 41) in the middle ones
      jt = join_table(ctx, type == 2 ? asize_max : asize_ends, n, type == 2 ? 3u : 1u);
      uint32_t * item_counter = jt.flags + kJoinItemCount + type;   // (one a type: the pair kernel of the type before still reads its own)
      FastGroupArgs g{};
      g.seqs = ctx->db.seqs; g.seq_off = ctx->db.seq_off; g.seqlen = ctx->db.seqlen;
      g.role = static_cast<const uint8_t *>(ctx->d_frole.ptr); g.n = n; g.max_len = plan.max_len;
      g.keys = jt.keys; g.cnt_l = jt.cnt_a; g.cnt_h = jt.cnt_b; g.amask = jt.asize - 1; g.lslot = jt.aslot; g.hslot = jt.bslot; g.overflow = jt.flags + kJoinKeyOverflow;
      // a group needs a light and a heavy amplicon: l h >= 1
      SWA_TRY(join_run<FastTiles>(ctx, jt, 1u, item_counter, item_cap, [&](dim3 gn, dim3 b) {
        with_group_type(type, [&](auto t) {
          constexpr int T = decltype(t)::value;
          hipLaunchKernelGGL(k_fg_light<T>, gn, b, 0, ctx->stream, g); hipLaunchKernelGGL(k_fg_heavy<T>, gn, b, 0, ctx->stream, g);
        });
      }, scan));
      FastPairArgs p{};
      p.seqs = ctx->db.seqs; p.seq_off = ctx->db.seq_off; p.seqlen = ctx->db.seqlen; p.members = jt.members;
      p.items = jt.items; p.item_count = item_counter; p.item_cap = item_cap;
      p.pairs = static_cast<unsigned long long *>(ctx->d_fpairs.ptr); p.pair_counter = &fc->pairs; p.pair_cap = ctx->fast_pair_cap;
      const dim3 gp(ctx->num_cus * 8);
      p.lines = static_cast<const uint4 *>(ctx->d_stream[kSbLines].ptr);
      p.line_quads = ctx->up.d1.lines_quads;
      with_group_type(type, [&](auto t) {
        constexpr int T = decltype(t)::value;
        if (pair_w == 5) { hipLaunchKernelGGL((k_fast_pairs_lines<T, 5>), gp, dim3(kThreads), 0, ctx->stream, p); }
        else if (pair_w == 8) { hipLaunchKernelGGL((k_fast_pairs_lines<T, 8>), gp, dim3(kThreads), 0, ctx->stream, p); }
        else if (pair_w == 13) { hipLaunchKernelGGL((k_fast_pairs_lines<T, 13>), gp, dim3(kThreads), 0, ctx->stream, p); }
        else { hipLaunchKernelGGL(k_fast_pairs<T>, gp, dim3(kThreads), 0, ctx->stream, p); }
      });
      SWA_HIP(ctx, hipGetLastError());
    }
    uint64_t got = 0;
    // (a group of l light and h heavy amplicons makes at most l + h / 2 items: tests/test_fastidious_identity.py)
    SWA_TRY(join_status(ctx, jt, &fc->pairs, 1, &got, "swa_d1_fastidious: group key table overflow", "swa_d1_fastidious: work item list overflow"));
    if (got <= ctx->fast_pair_cap) { npairs = got; break; }
    if (attempt == 5) { return swa_fail_msg(ctx, SWA_E_NOMEM, "swa_d1_fastidious: pair list keeps overflowing"); }
    ctx->fast_pair_cap = got + got / 8 + 1024;               // the count of a complete run: size for it (+ slack: none needed, it is exact)
  }
  swa_t1(ctx, kTimePairs);
  swa_t0(ctx, kTimeAlign);
  if (npairs != 0) {
    FastCountArgs c{};
    c.seqs = ctx->db.seqs; c.seq_off = ctx->db.seq_off; c.seqlen = ctx->db.seqlen;
    c.zobrist = static_cast<const uint64_t *>(ctx->d_zobrist.ptr);
    // the longest sequence a pair can hold: the database's, under the split pair_longest (k_fg_light / k_fg_heavy keep longer
    // ones out of every group).  swa_prepare_hashing lays the Zobrist table out by position, four values each, drawn in that
    // order (host_tables.cpp: swa_zobrist_table): its first 4 * zlen words ARE the table of a database whose longest sequence
    // is plan.served, so k_fast_count stages a prefix.
    c.zlen = plan.served + 2u; c.maxwords = (plan.served + 31u) >> 5; c.slots = slots;
    c.pairs = static_cast<const unsigned long long *>(ctx->d_fpairs.ptr); c.npairs = npairs;
    c.graft = static_cast<uint32_t *>(ctx->d_graft.ptr); c.cand_counter = &fc->candidates;
    if (plan.count_words) {
      // two staged sequences a wave: no set, no Zobrist table (c.zobrist, c.zlen and c.slots are not read)
      uint64_t blocks = (npairs + count_waves - 1) / count_waves;
      const uint64_t max_blocks = (uint64_t)ctx->num_cus * 8;
      if (blocks > max_blocks) { blocks = max_blocks; }
      const dim3 gc((uint32_t)blocks);
      if (count_waves == 4) { hipLaunchKernelGGL(k_fast_count_sites_words<4>, gc, dim3(256), plan.count_lds, ctx->stream, c); }
      else if (count_waves == 2) { hipLaunchKernelGGL(k_fast_count_sites_words<2>, gc, dim3(128), plan.count_lds, ctx->stream, c); }
      else { hipLaunchKernelGGL(k_fast_count_sites_words<1>, gc, dim3(64), plan.count_lds, ctx->stream, c); }
    } else if (plan.count_w != 0) {
      uint64_t blocks = (npairs + kWaves - 1) / kWaves;
      const uint64_t max_blocks = (uint64_t)ctx->num_cus * 8;
      if (blocks > max_blocks) { blocks = max_blocks; }
      if (plan.count_w == 5) { hipLaunchKernelGGL(k_fast_count_sites<5>, dim3((uint32_t)blocks), dim3(kThreads), 0, ctx->stream, c); }
      else { hipLaunchKernelGGL(k_fast_count_sites<8>, dim3((uint32_t)blocks), dim3(kThreads), 0, ctx->stream, c); }
    } else {
    const size_t lds = plan.count_lds;
    uint64_t blocks = (npairs + count_waves - 1) / count_waves;
    const uint64_t max_blocks = (uint64_t)ctx->num_cus * 8;
    if (blocks > max_blocks) { blocks = max_blocks; }
    hipLaunchKernelGGL(k_fast_count, dim3((uint32_t)blocks), dim3(64 * count_waves), lds, ctx->stream, c);
    }
    SWA_HIP(ctx, hipGetLastError());
  }
  swa_t1(ctx, kTimeAlign);
  return SWA_OK;
}

// The pass from the roles on (0 light, 1 heavy and to be expanded here, 2 neither): what swa_d1_fastidious_shard and
// swa_d1_fastidious_resident share.  host_role: the shard form's array, uploaded into d_frole; d_owner: owner bytes in this
// context's HBM (swa_d1_shard_owners_device, on rank 0 or as it sent them), mapped for `shard` on the device; neither: the bytes
// swa_d1_light_flags_device left in d_swarm_role, copied on the device.  Reservations, copies and launches come in the order
// swa_d1_fastidious_shard has always made them.  graft_cand may be null: the candidates then stay in HBM (d_graft) only.
static int fastidious_with_roles(swa_ctx * ctx, const uint8_t * host_role, const uint8_t * d_owner, uint32_t shard, uint64_t n_light, uint64_t n_heavy, uint64_t light_nt,
                                 uint32_t bloom_bits, uint32_t * graft_cand, uint64_t * counters) {
  SWA_TRY(swa_prepare_hashing(ctx));                         // the Zobrist table
  const uint32_t n = ctx->db.n;
  ctx->res.fast.candidates_end();
  // the numbers of the reference's log line (src/algod1.cc:1337-1357, 1383-1403; bloomflex.cc:91-115)
  uint32_t k = static_cast<uint32_t>(0.4 * static_cast<double>(bloom_bits));
  if (k < 1) { k = 1; }
  uint64_t m = light_nt * 7ull * bloom_bits;
  if (m < 64) { m = 64; }

  FastPlan plan{};
  SWA_TRY(fast_plan(ctx, plan));
  const bool pair_route = plan.pair_route;
  for (uint64_t & t : ctx->fast_totals) { t = 0; }
  for (uint64_t & t : ctx->fast_batches) { t = 0; }
  for (uint64_t & t : ctx->fast_bloom) { t = 0; }
  const uint32_t min_len = pair_route ? kFastMinLen : 0xFFFFFFFFu;
  const uint32_t max_len = plan.max_len;                     // (0xFFFFFFFF without a division at the long end)

  SWA_TRY(swa_reserve(ctx, ctx->d_frole, n));
  SWA_TRY(swa_reserve(ctx, ctx->d_light, n));
  SWA_TRY(swa_reserve(ctx, ctx->d_graft, uint64_t(n) * sizeof(uint32_t)));
  ctx->dr = {};                                             // (d_graft no longer holds a dereplication's array)
  SWA_TRY(swa_reserve(ctx, ctx->d_list_a, (uint64_t(n) + 1) * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_list_b, (uint64_t(n) + 1) * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_fcounters, sizeof(swa_fast_counters)));
  if (host_role != nullptr) { SWA_HIP(ctx, hipMemcpyAsync(ctx->d_frole.ptr, host_role, n, hipMemcpyHostToDevice, ctx->stream)); }
  else if (d_owner != nullptr) { SWA_TRY(swa_d1_roles_from_owners(ctx, d_owner, shard, static_cast<uint8_t *>(ctx->d_frole.ptr))); }
  else { SWA_HIP(ctx, hipMemcpyAsync(ctx->d_frole.ptr, ctx->d_swarm_role.ptr, n, hipMemcpyDeviceToDevice, ctx->stream)); }
  SWA_HIP(ctx, hipMemsetAsync(ctx->d_graft.ptr, 0xFF, uint64_t(n) * sizeof(uint32_t), ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(ctx->d_fcounters.ptr, 0, sizeof(swa_fast_counters), ctx->stream));
  swa_fast_counters * fc = fast_counters(ctx);
  for (int slot : {kTimePairs, kTimeAlign}) { ctx->ev_used[slot] = false; }

  // the log's variant totals (light_variants and, behind it, heavy_variants), and the amplicons that can be part of a pair
  // the pair route does not take
  static_assert(offsetof(swa_fast_counters, heavy_variants) == offsetof(swa_fast_counters, light_variants) + sizeof(uint64_t), "light_variants, heavy_variants: neighbours");
  hipLaunchKernelGGL(k_fast_variant_totals, dim3(swa_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off,
                     ctx->db.seqlen, static_cast<const uint8_t *>(ctx->d_frole.ptr), n, &fc->light_variants);
  const uint32_t short_cut = pair_route ? kFastMinLen + 1u : 0xFFFFFFFFu;   // len <= cut: may pair with a sequence < kFastMinLen
  const uint32_t long_cut = max_len != 0xFFFFFFFFu ? max_len - 1u : 0xFFFFFFFFu;   // len >= cut: may pair with a sequence > the cap (split, pairs)
  hipLaunchKernelGGL(k_fast_band_lists, dim3(swa_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.seqlen,
                     static_cast<const uint8_t *>(ctx->d_frole.ptr), n, short_cut, long_cut, static_cast<uint8_t *>(ctx->d_light.ptr),
                     static_cast<uint32_t *>(ctx->d_list_a.ptr), static_cast<uint32_t *>(ctx->d_list_b.ptr), fc->bands);
  SWA_HIP(ctx, hipGetLastError());
  uint64_t bands[3] = {0, 0, 0};                             // light / heavy amplicons of the two bands, the lights' nucleotides
  static_assert(sizeof(bands) == sizeof(fc->bands), "the bands: one copy");
  SWA_HIP(ctx, hipMemcpyAsync(bands, fc->bands, sizeof(bands), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));           // (role is a host temporary, too)

  if (pair_route) { SWA_TRY(fastidious_pair_route(ctx, (uint32_t)n_light, (uint32_t)n_heavy, plan)); }
  if (bands[0] != 0 && bands[1] != 0) {
    SWA_TRY(fastidious_bloom_route(ctx, (uint32_t)bands[0], (uint32_t)bands[1], bands[2], bloom_bits, min_len, max_len, plan.zobrist_lds));
  }

  // the head of the counters, up to the bands' two amplicon counts, with one copy (eight words)
  swa_fast_counters host_fc{};
  constexpr size_t head = offsetof(swa_fast_counters, bands) + 2 * sizeof(uint64_t);
  SWA_HIP(ctx, hipMemcpyAsync(&host_fc, fc, head, hipMemcpyDeviceToHost, ctx->stream));
  if (graft_cand != nullptr) {
    swa_touch_pages(graft_cand, uint64_t(n) * sizeof(uint32_t));
    SWA_HIP(ctx, hipMemcpyAsync(graft_cand, ctx->d_graft.ptr, uint64_t(n) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  counters[0] = host_fc.light_variants;
  counters[1] = host_fc.heavy_variants;
  counters[2] = host_fc.candidates;
  counters[3] = m;
  counters[4] = k;
  ctx->fast_totals[0] = host_fc.pairs; ctx->fast_totals[1] = host_fc.bands[0]; ctx->fast_totals[2] = host_fc.bands[1];
  return SWA_OK;
}

extern "C" int swa_d1_fastidious_shard(swa_ctx * ctx, const uint8_t * is_light, uint64_t light_nt, uint32_t bloom_bits,
                                       uint32_t shard, uint32_t nshards, uint32_t * graft_cand, uint64_t * counters) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (nshards == 0 || shard >= nshards) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious_shard: bad shard"); }
  if (!ctx->ix.d1_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious: call swa_d1_index_build first"); }
  if (is_light == nullptr || graft_cand == nullptr || counters == nullptr || bloom_bits < 2 || bloom_bits > 64) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious: bad argument");
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->db.n;

  // role of every amplicon: 0 light, 1 heavy and in this shard's contiguous slice of the heavy ones, 2 neither
  // (by blocks on a few threads: two serial passes over 10 M flags were 15 ms of this call, lease r6j)
  std::unique_ptr<uint8_t[]> role(new uint8_t[n]);
  uint64_t n_light = 0, n_heavy_all = 0;
  const unsigned blocks = n >= (1u << 20) ? std::min(16u, std::max(1u, std::thread::hardware_concurrency())) : 1u;
  std::vector<uint64_t> heavy_before(blocks + 1, 0);
  auto in_blocks = [&](auto && body) {
    std::vector<std::thread> team;
    for (unsigned b = 1; b < blocks; ++b) { team.emplace_back([&, b] { body(b); }); }
    body(0u);
    for (auto & t : team) { t.join(); }
  };
  in_blocks([&](unsigned b) {
    uint64_t heavy = 0;
    for (uint64_t i = (uint64_t)n * b / blocks; i < (uint64_t)n * (b + 1) / blocks; ++i) { heavy += is_light[i] == 0 ? 1u : 0u; }
    heavy_before[b + 1] = heavy;
  });
  for (unsigned b = 0; b < blocks; ++b) { heavy_before[b + 1] += heavy_before[b]; }
  n_heavy_all = heavy_before[blocks];
  n_light = n - n_heavy_all;
  const uint64_t lo = n_heavy_all * shard / nshards, hi = n_heavy_all * (shard + 1ull) / nshards;
  in_blocks([&](unsigned b) {
    uint64_t seen = heavy_before[b];
    for (uint64_t i = (uint64_t)n * b / blocks; i < (uint64_t)n * (b + 1) / blocks; ++i) {
      if (is_light[i] != 0) { role[i] = 0; }
      else { role[i] = (seen >= lo && seen < hi) ? 1 : 2; ++seen; }
    }
  });
  const uint64_t n_heavy = hi - lo;
  const int rc = fastidious_with_roles(ctx, role.get(), nullptr, 0, n_light, n_heavy, light_nt, bloom_bits, graft_cand, counters);
  if (rc != SWA_OK) { (void)hipStreamSynchronize(ctx->stream); }     // (role is a host temporary)
  ctx->res.fast.cand_ready = rc == SWA_OK && nshards == 1u;   // (d_graft: the candidates of the whole pass, for swa_d1_graft_device)
  return rc;
}

extern "C" int swa_d1_fastidious(swa_ctx * ctx, const uint8_t * is_light, uint64_t light_nt, uint32_t bloom_bits,
                                 uint32_t * graft_cand, uint64_t * counters) {
  return swa_d1_fastidious_shard(ctx, is_light, light_nt, bloom_bits, 0, 1, graft_cand, counters);
}

// The same pass fed from the device: the roles are the bytes swa_d1_light_flags_device left in HBM for the clustering in
// place (no host flags, no role passes on the host, no upload), and the candidates come home only when the caller hands
// over a buffer — swa_d1_graft_device reads them where they lie.
extern "C" int swa_d1_fastidious_resident(swa_ctx * ctx, uint64_t light_nt, uint32_t bloom_bits, uint32_t * graft_cand, uint64_t * counters) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (!ctx->res.cluster_ready || !ctx->res.csr_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious_resident: no clustering in place (swa_d1_cluster_device)"); }
  if (!ctx->res.fast.roles_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious_resident: call swa_d1_light_flags_device first"); }
  if (!ctx->ix.d1_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious: call swa_d1_index_build first"); }
  if (counters == nullptr || bloom_bits < 2 || bloom_bits > 64) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious: bad argument"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->db.n;
  const uint64_t n_light = ctx->res.fast.light_amps;
  SWA_TRY(fastidious_with_roles(ctx, nullptr, nullptr, 0, n_light, n - n_light, light_nt, bloom_bits, graft_cand, counters));
  ctx->res.fast.cand_ready = true;
  return SWA_OK;
}

// One shard of the pass with its roles from owner bytes in HBM: what a rank of swa_multi_d1_fastidious_resident runs.  The
// candidates of this shard alone are left in d_graft (cand_ready stays false: the caller combines the shards first).
int swa_d1_fastidious_owned(swa_ctx * ctx, const uint8_t * d_owner, uint32_t shard, uint64_t n_light, uint64_t n_heavy, uint64_t light_nt,
                            uint32_t bloom_bits, uint32_t * graft_cand, uint64_t * counters) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (!ctx->ix.d1_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious: call swa_d1_index_build first"); }
  if (d_owner == nullptr || counters == nullptr || bloom_bits < 2 || bloom_bits > 64) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_fastidious: bad argument"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  return fastidious_with_roles(ctx, nullptr, d_owner, shard, n_light, n_heavy, light_nt, bloom_bits, graft_cand, counters);
}
