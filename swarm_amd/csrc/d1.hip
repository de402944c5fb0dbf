// d1.hip — seam B1: the d = 1 amplicon network on gfx950.
//
// Replaces (behaviourally) the reference's per-thread loop
//   network_thread -> check_variants -> generate_variants + find_variant_matches
// (src/algod1.cc:558-670, src/variants.cc:184-249) and the serial table build
// (src/algod1.cc:188-208, 1122-1150).  Nothing here is a translation of that code:
//
//   * one 64-lane wavefront owns one query amplicon; lane l owns the K = ceil((L+1)/64)
//     consecutive sequence positions [l*K, (l+1)*K).  The reference's serially
//     incremental deletion / insertion hashes become three wave-wide XOR scans
//     (exclusive prefix of Z[p][s_p], suffixes of Z[p-1][s_p] and Z[p+1][s_p]);
//   * default route (d1_anchor.inc): amplicons grouped by their first / last 32 nucleotides,
//     a group's members in an LDS table + LDS Bloom, every probe answered from LDS;
//   * plain route (k_d1_probe, d1_probe.inc: statistics, sequences the anchored passes cannot
//     serve; its MODE 1, the fastidious second level, belongs to fastidious.hip): the 2-bit packed query, the Zobrist table and the
//     1024 Bloom patterns in LDS, Bloom-word loads issued 8 at a time per lane, survivors
//     compacted with __ballot/__popcll into a per-wave LDS queue and drained 64 at a time so
//     that table walk, abundance rule and exact verification run with full lanes;
//   * the hash table is one 16-byte slot per entry (hash, amplicon id): one transaction
//     per probe step instead of the reference's three arrays;
//   * hits leave a wave through its own segment of the edge buffer (one writer per segment,
//     no atomics); the partition of d1_part.hip sorts the segments' links into the canonical CSR.
//
// All arithmetic is 64-bit integer XOR/shift/compare; results are bit-exact.
//
// In this unit: hashing, the table, the plain probe (MODE 0 / 2), the anchored passes (d1_anchor.inc), the streaming index
// build (d1_stream.inc), the guard, the multi-GPU route entry points, the debug readers.  The partition engine, the CSR
// assembly and the link exchange are a unit of their own (d1_part.hip), called through the six functions of
// d1_internal.h.  The --fastidious pass is a unit of its own (fastidious.hip); the few host functions it calls here are
// declared in one block of swa_internal.h ("what fastidious.hip takes from d1.hip"), the device code both compile is in
// d1_common.inc and d1_probe.inc.
#include "d1_internal.h"
using namespace swa_d1;

#include <algorithm>
#include <type_traits>   // (d1_stream.inc: std::conditional, std::true_type)
#include <cstdlib>

namespace {

constexpr size_t kMaxZobristLds = SWA_MAX_ZOBRIST_LDS;

#include "wave_ops.inc"     // wave_lds_sync
#include "key_ops.inc"      // kEmpty, kKeyEmpty, mix64, window32
#include "d1_common.inc"    // kWaves / kThreads / kQueueCap, swa_aux, swa_item, the width classes, the amplicon lines, the anchor keys

// ---- sequence hashes (db.cc:761 zobrist_hash) --------------------------------------
template <bool ZLDS>
__global__ __launch_bounds__(256) void k_seqhash(const uint64_t * __restrict__ seqs,
                                                 const uint64_t * __restrict__ seq_off,
                                                 const uint32_t * __restrict__ seqlen,
                                                 const uint64_t * __restrict__ zobrist, uint32_t zlen,
                                                 uint32_t n, uint64_t * __restrict__ seqhash,
                                                 swa_aux * __restrict__ aux, uint32_t anchor_w, const uint8_t * __restrict__ only) {
  extern __shared__ uint64_t lds[];
  const uint64_t * zob = zobrist;
  if (ZLDS) {
    for (uint32_t i = threadIdx.x; i < 4u * zlen; i += blockDim.x) { lds[i] = zobrist[i]; }
    __syncthreads();
    zob = lds;
  }
  for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < n; a += gridDim.x * blockDim.x) {
    if (only != nullptr && only[a] == 0) { continue; }         // (the member table of the groups left to the plain kernel: only those)
    const uint64_t * s = seqs + seq_off[a];
    const uint32_t len = seqlen[a];
    uint64_t h = 0, dall = 0, iall = 0;
    uint64_t word = 0;
    swa_aux ax{};
    // pb: first position of the run that contains position anchor_w - 1 (see swa_aux; 31 for the 32-nt windows of rounds
    // 1-3), and the three streams below it: kept as of the start of the current run until that position is reached
    uint32_t run_start = 0, prev = 4u;
    uint64_t rh = 0, rd = 0, ri = 0;
    ax.pb = anchor_w;
    for (uint32_t p = 0; p < len; ++p) {
      if ((p & 31u) == 0u) { word = s[p >> 5]; }
      const uint32_t c = (uint32_t)(word & 3u);
      if (c != prev) { run_start = p; rh = h; rd = dall; ri = iall; prev = c; }
      if (p + 1u == anchor_w) { ax.pb = run_start; ax.a32 = rh; ax.d32 = rd; ax.i32 = ri; }
      h ^= zob[4u * p + c];
      if (p >= 1u) { dall ^= zob[4u * (p - 1u) + c]; }
      iall ^= zob[4u * (p + 1u) + c];
      word >>= 2;
    }
    if (len < anchor_w) { ax.a32 = h; ax.d32 = dall; ax.i32 = iall; }
    ax.h = h; ax.dall = dall; ax.iall = iall;
    seqhash[a] = h;
    aux[a] = ax;
  }
}

// ---- table + Bloom build (algod1.cc:188-208; insertion order is free) ---------------
__global__ __launch_bounds__(256) void k_table_clear(swa_slot * table, uint64_t slots, uint64_t * bloom,
                                                     uint64_t bloom_words) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += stride) {
    swa_slot s;
    s.hash = 0; s.amp = kEmpty; s.pad = 0;
    table[i] = s;
  }
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < bloom_words; i += stride) {
    bloom[i] = ~0ull;          // inverted polarity, bloompat.cc:93-97
  }
}

// inserts amplicons for which (is_member == nullptr || is_member[a] != 0)
__global__ __launch_bounds__(256) void k_table_insert(const uint64_t * __restrict__ seqhash, uint32_t n,
                                                      const uint8_t * __restrict__ is_member,
                                                      swa_slot * table, uint64_t tmask,
                                                      unsigned long long * bloom, uint64_t bmask,
                                                      const uint64_t * __restrict__ patterns) {
  for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < n; a += gridDim.x * blockDim.x) {
    if (is_member != nullptr && is_member[a] == 0) { continue; }
    const uint64_t h = seqhash[a];
    uint64_t idx = (h >> 32) & tmask;                          // hashtable.cc:47-53
    for (;;) {
      const uint32_t old = atomicCAS(&table[idx].amp, kEmpty, a);
      if (old == kEmpty) { break; }
      idx = (idx + 1) & tmask;
    }
    table[idx].hash = h;
    atomicAnd(&bloom[(h >> 10) & bmask], ~(unsigned long long)patterns[h & 1023u]);   // bloompat.cc:62-65
  }
}

// identical sequences => flag (algod1.cc:174-208 detects this while inserting)
__global__ __launch_bounds__(256) void k_dup_check(const uint64_t * __restrict__ seqs,
                                                   const uint64_t * __restrict__ seq_off,
                                                   const uint32_t * __restrict__ seqlen,
                                                   const uint64_t * __restrict__ seqhash, uint32_t first,
                                                   uint32_t count, const swa_slot * __restrict__ table, uint64_t tmask,
                                                   uint32_t * flag) {
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
    const uint32_t a = first + k;
    const uint64_t h = seqhash[a];
    const uint32_t len = seqlen[a];
    uint64_t idx = (h >> 32) & tmask;
    for (;;) {
      const swa_slot s = table[idx];
      if (s.amp == kEmpty) { break; }
      if (s.hash == h && s.amp != a && seqlen[s.amp] == len) {
        const uint64_t * x = seqs + seq_off[a];
        const uint64_t * y = seqs + seq_off[s.amp];
        bool same = true;
        for (uint32_t w = 0; w < ((len + 31u) >> 5); ++w) { same = same && (x[w] == y[w]); }
        if (same) { atomicOr(flag, 1u); }
      }
      idx = (idx + 1) & tmask;
    }
  }
}

#include "d1_probe.inc"   // enumerate_variants / enumerate_range, k_d1_probe: MODE 0 and MODE 2 are launched (and instantiated) here

#include "d1_anchor.inc"

#include "d1_stream.inc"

}  // namespace

int swa_grid_for(const swa_ctx * ctx, uint64_t items, int per_block, int max_per_cu) {
  uint64_t blocks = (items + per_block - 1) / per_block;
  const uint64_t cap = (uint64_t)ctx->num_cus * max_per_cu;
  if (blocks > cap) { blocks = cap; }
  if (blocks < 1) { blocks = 1; }
  return (int)blocks;
}

// loads this translation unit's code object (see swa_ctx_warmup): an empty launch
void swa_warm_d1(swa_ctx * ctx) {
  hipLaunchKernelGGL(k_table_clear, dim3(1), dim3(64), 0, ctx->stream, static_cast<swa_slot *>(nullptr), (uint64_t)0,
                     static_cast<uint64_t *>(nullptr), (uint64_t)0);
}

// d_table and d_bloom cleared and filled again: with all amplicons (swa_ensure_full_index) or with those a byte array marks
// (the light amplicons of the Bloom route's bands: fastidious.hip)
int swa_d1_rebuild_table(swa_ctx * ctx, const uint8_t * d_is_member) {
  const uint32_t n = ctx->db.n;
  hipLaunchKernelGGL(k_table_clear, dim3(swa_grid_for(ctx, ctx->ix.table_size, 256, 8)), dim3(256), 0, ctx->stream,
                     static_cast<swa_slot *>(ctx->d_table.ptr), ctx->ix.table_size,
                     static_cast<uint64_t *>(ctx->d_bloom.ptr), ctx->ix.bloom_words);
  hipLaunchKernelGGL(k_table_insert, dim3(swa_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream,
                     static_cast<const uint64_t *>(ctx->d_seqhash.ptr), n, d_is_member,
                     static_cast<swa_slot *>(ctx->d_table.ptr), ctx->ix.table_size - 1,
                     static_cast<unsigned long long *>(ctx->d_bloom.ptr), ctx->ix.bloom_words - 1,
                     static_cast<const uint64_t *>(ctx->d_patterns.ptr));
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}


// ---- the anchored index (see d1_anchor.inc, d1_stream.inc) ----------------------------------------------------------
static bool anchored_enabled() {
  const char * e = getenv("SWA_D1_PLAIN");
  return !(e != nullptr && e[0] == '1');
}

// shortest seed the anchored passes serve: two windows and a nucleotide (65 with the 32-nt windows of rounds 1-3)
static uint32_t anchor_minlen(const swa_ctx * ctx) { return ctx->ix.anchor_a + ctx->ix.anchor_b + 2u * ctx->ix.anchor_w + 1u; }

// whether the anchored passes may be used at all for this database (decided at index build)
static bool anchor_applicable(const swa_ctx * ctx) {
  return anchored_enabled() && ctx->db.longest >= kMinAnchoredLen && ctx->db.longest <= 64u * kPrefetchWords * 32u - 64u;
}

// 16-byte quads per amplicon line: by the longest sequence of the database (64 bytes hold 7 words, 128 hold 15, 256 hold 31;
// longer sequences are cut off in their lines and served by the plain kernel)
static uint32_t line_quads_for(const swa_ctx * ctx) { return ctx->db.longest <= 160u ? 4u : (ctx->db.longest <= 480u ? 8u : 16u); }

// widest anchor windows, in words of 32 nt (anchor_nwin_for).  SWA_D1_ANCHOR_W=32 / 64 / 128 caps it (comparison switch).
static uint32_t anchor_max_nwin(const swa_ctx *) {
  uint32_t cap = 4u;
  if (const char * e = getenv("SWA_D1_ANCHOR_W")) { cap = std::min(4u, std::max(1u, (uint32_t)atoi(e) / 32u)); }
  return cap;
}
// SWA_D1_WINDOWS=0: the anchor windows stay at the ends (no sample, no search for windows moved inwards)
static bool windows_search_off() {
  const char * e = getenv("SWA_D1_WINDOWS");
  return e != nullptr && e[0] == '0';
}

// Shortest sequence and the population of every width class: facts of the uploaded database (k_db_lengths), read once per
// upload.  The work lists of an index are laid out from the populations (list_regions).
static int ensure_db_lengths(swa_ctx * ctx) {
  if (ctx->up.d1.props_ready) { return SWA_OK; }
  SWA_TRY(swa_reserve(ctx, ctx->d_rank_tmp, std::max<size_t>(ctx->d_rank_tmp.bytes, 64)));
  auto * out = static_cast<uint32_t *>(ctx->d_rank_tmp.ptr);
  SWA_HIP(ctx, hipMemsetAsync(out, 0, 8 * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_db_lengths, dim3(swa_grid_for(ctx, ctx->db.n, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.seqlen, ctx->db.n, out);
  uint32_t host[8] = {};
  SWA_HIP(ctx, hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->up.d1.db_shortest = 0xFFFFFFFFu - host[0];
  for (uint32_t c = 0; c <= kWidthClasses; ++c) { ctx->up.d1.class_pop[c] = host[1 + c]; }
  ctx->up.d1.props_ready = true;
  return SWA_OK;
}

// Where the work lists of an index lie in its item buffer.  A group of width class c has a member of that class, and all
// its members are of classes <= c; a group on size list k has at least least[k] members: so list (c, k) holds at most
// min(pop[c], pop[<= c] / least[k]) groups, and the row tiles of class c (64 members each, of groups of more than 256)
// number at most pop[<= c] / 64 + pop[<= c] / (kPairBigCap + 1), kPairBigCap = the largest group a workgroup takes by
// pairs.  A database of one class — the usual one — pays for one class.
static ListRegions list_regions(const swa_ctx * ctx, uint64_t * total_items) {
  const uint32_t least[kListKinds] = {2, 5, 9, 17, 33, 65, kPairBigCap + 1u};
  ListRegions r{};
  uint64_t at = 0, upto = 0;
  for (uint32_t c = 0; c < kWidthClasses; ++c) {
    upto += ctx->up.d1.class_pop[c];
    for (uint32_t k = 0; k < kListKinds; ++k) {
      r.at[c][k] = at;
      uint64_t room = 64;
      // (the tiled kernel's items: a row tile against kTiledCols column tiles — per row tile at most what the largest group has)
      constexpr uint64_t per_row_tile = (tiled_item_count(kStreamGroupCap) + kStreamGroupCap / 64u - 1u) / (kStreamGroupCap / 64u);
      if (ctx->up.d1.class_pop[c] != 0) { room += k + 1 < kListKinds ? std::min<uint64_t>(ctx->up.d1.class_pop[c], upto / least[k]) : per_row_tile * (upto / 64 + upto / least[k]); }
      at += room;
    }
    r.at[c][kListKinds] = at;
  }
  *total_items = at;
  return r;
}

// abundance rank of every amplicon (k_abundance_rank: three streaming passes); kFlagUnordered is raised when the database is
// not in abundance order
int swa_launch_abundance_rank(swa_ctx * ctx) {
  if (ctx->up.d1.rank_ready) {                                    // (a fact of the uploaded database: once per upload)
    if (ctx->up.d1.db_unordered) { SWA_HIP(ctx, hipMemsetAsync(swa_status(ctx)->flags + kFlagUnordered, 1, sizeof(uint32_t), ctx->stream)); }
    return SWA_OK;
  }
  ctx->up.d1.rank_ready = true;
  // (the flag is this database's from here on: the index build's clear leaves it alone)
  SWA_HIP(ctx, hipMemsetAsync(swa_status(ctx)->flags + kFlagUnordered, 0, sizeof(uint32_t), ctx->stream));
  const uint32_t n = ctx->db.n;
  const uint32_t tiles = (n + 255u) / 256u;
  SWA_TRY(swa_reserve(ctx, ctx->d_arank, uint64_t(n) * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_rank_tmp, uint64_t(tiles) * sizeof(uint32_t)));
  auto * rank = static_cast<uint32_t *>(ctx->d_arank.ptr);
  auto * tile_last = static_cast<uint32_t *>(ctx->d_rank_tmp.ptr);
  hipLaunchKernelGGL(k_abundance_rank, dim3(swa_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.abundance, n, rank,
                     swa_status(ctx)->flags, tile_last);
  hipLaunchKernelGGL(k_abundance_rank_carry, dim3(1), dim3(256), 0, ctx->stream, tile_last, tiles);
  hipLaunchKernelGGL(k_abundance_rank_fill, dim3(swa_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, n, rank, tile_last);
  return SWA_OK;
}

__global__ void k_set_flags(uint32_t * flags, uint32_t unserved, uint32_t shortest_code) { flags[kFlagUnserved] = unserved; flags[kFlagShortest] = shortest_code; }
__global__ void k_set_guard_made(unsigned long long * guard, uint32_t made0, uint32_t made1) { guard[kGuardMade] = made0; guard[kGuardMade + 1] = made1; }

// ---- the streaming build (d1_stream.inc) ------------------------------------------------------

// the amplicon lines of the uploaded database (once per upload; needs the abundance ranks)
int swa_ensure_lines(swa_ctx * ctx) {
  const uint32_t lq = line_quads_for(ctx);
  if (ctx->up.d1.lines_ready && ctx->up.d1.lines_quads == lq) { return SWA_OK; }
  const uint32_t n = ctx->db.n;
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbLines], (uint64_t)n * lq * 16u + 64u));   // (+ what window_at may read behind the last line)
  auto * lines = static_cast<uint4 *>(ctx->d_stream[kSbLines].ptr);
  const auto * rank = static_cast<const uint32_t *>(ctx->d_arank.ptr);
  SWA_HIP(ctx, hipMemsetAsync(reinterpret_cast<uint8_t *>(lines) + (uint64_t)n * lq * 16u, 0, 64, ctx->stream));
  swa_t0(ctx, kTimeLines);
  const dim3 grid(swa_grid_for(ctx, n, 256, 8));
  if (lq == 4u) { hipLaunchKernelGGL(k_lines_build<4>, grid, dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen, rank, n, lines); }
  else if (lq == 8u) { hipLaunchKernelGGL(k_lines_build<8>, grid, dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen, rank, n, lines); }
  else { hipLaunchKernelGGL(k_lines_build<16>, grid, dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen, rank, n, lines); }
  swa_t1(ctx, kTimeLines);
  SWA_HIP(ctx, hipGetLastError());
  ctx->up.d1.lines_ready = true;
  ctx->up.d1.lines_quads = lq;
  return SWA_OK;
}

// The two anchor indexes of the whole database (or of the routed id lists) by the streaming build: members in group
// order (d_stream[kSbMembers + which]: ids), the work lists of the pair kernels, the flags build_owned_index reads
// (kFlagDuplicates, kFlagKeyOverflow, kFlagUnserved, kFlagOversized / kFlagOverMass, kFlagShortest).
// What a routed build is given (swa_d1_index_build_routed / _records): the members of this rank's groups as two id lists,
// or — the key records themselves travelled: no k_keys pass — as two record lists; [0] prefix side, [1] suffix side.  The
// lists are the caller's, for the one call.  A default one: not routed (every build the library starts on its own); an
// empty list still counts as routed (the entry points pass a pointer to nothing then, and so do the kernels' arguments).
struct RouteLists {
  const uint32_t * ids[2] = {nullptr, nullptr};
  const unsigned long long * rec[2] = {nullptr, nullptr};
  uint32_t m[2] = {0, 0};
  bool routed() const { return ids[0] != nullptr || rec[0] != nullptr; }
  bool by_rec() const { return rec[0] != nullptr; }
};

static int build_stream_index(swa_ctx * ctx, const RouteLists & route) {
  const bool clear_head = ctx->ix.head_clear_pending;            // (index_build: the first build of the call)
  ctx->ix.head_clear_pending = false;
  ctx->ix.anchor_ready = false;
  ctx->ix.stream_index = false;
  ctx->ix.list_counts_ready = false;
  const uint32_t n = ctx->db.n;
  swa_status_block * st = swa_status(ctx);
  swa_lap(ctx, "(build starts)");
  SWA_TRY(ensure_db_lengths(ctx));
  swa_lap(ctx, "db lengths");
  SWA_TRY(swa_ensure_lines(ctx));
  swa_lap(ctx, "amplicon lines");
  const uint32_t lq = ctx->up.d1.lines_quads;
  uint64_t item_room = 0;
  const ListRegions regions = list_regions(ctx, &item_room);
  const bool by_rec = route.by_rec();                         // routed, and the key records themselves arrived: no k_keys pass
  const bool routed = route.routed();
  const uint64_t records = routed ? std::max<uint64_t>(std::max(route.m[0], route.m[1]), 1) : n;
  // buckets of ~10 000 records for k_group1, the levels, the tile and who takes the first histogram: swa_part_plan_for
  // (host_tables.cpp).  SWA_D1_PART_BITS=1..27 (test hook, read at every build): that many bits instead of what the number
  // of records gives; the bits of the key-overflow retry still come on top
  uint32_t forced_bits = 0;
  if (const char * e = getenv("SWA_D1_PART_BITS")) {
    const int b = atoi(e);
    if (b >= 1 && b <= (int)(3 * kPartMaxBits)) { forced_bits = (uint32_t)b; }
  }
  const swa_part_plan plan = swa_part_plan_for(records, ctx->up.d1.stream_extra_bits, routed, forced_bits);
  const uint32_t total_bits = plan.lv.total;
  const bool keys_hist = plan.keys_hist;
  PartJob j;
  j.nidx = 2;
  j.plan = plan.lv;
  j.max_records = records;
  j.out_cap = records + 1;
  j.tile = plan.tile;
  swa_part_plan_report(plan, ctx->ix.part_plan);
  ctx->ix.part_plan[7] = ctx->up.d1.stream_extra_bits;                 // (swa_d1_part_plan: the retry's bits in place of `wide`)
  ctx->ix.part_starts_valid = false;
  j.max_tiles0 = records / j.tile + 2;
  j.chunks0 = 1; j.single0 = true; j.top_bit = 32; j.bias = 0;
  uint64_t e_cnt, e_tile, e_start, e_partial;
  swa_part_scratch(j, &e_cnt, &e_tile, &e_start, &e_partial);
  const uint64_t buckets = 1ull << total_bits;
  e_partial = std::max<uint64_t>(e_partial, ((uint64_t)kListsPerIndex * buckets + 1) / kFlatChunk + 2);
  for (int i = 0; i < 2; ++i) {
    for (int h = 0; h < 2; ++h) { SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbRec + 2 * i + h], (records + 1) * sizeof(uint64_t))); }
    SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbCnt + i], e_cnt * sizeof(uint32_t)));
    SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbTile + i], e_tile * sizeof(uint32_t)));
    SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbStart + i], (2 * e_start + 4) * sizeof(uint64_t)));
    SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbPartial + i], e_partial * sizeof(uint32_t)));
    SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbMembers + i], (records + 1) * sizeof(uint32_t)));
    SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbKind + i], ((uint64_t)kListsPerIndex * buckets + 2) * sizeof(uint32_t)));
    SWA_TRY(swa_reserve(ctx, ctx->d_aitems[i], (item_room + 1) * sizeof(swa_item)));
  }
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbScal], 64 * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbOver], ((uint64_t)n + 8) & ~3ull));
  {
    ClearList c{};
    clear_add(c, st->counters, sizeof(st->counters));
    if (clear_head) {
      // the head of the status block for a new index: the flags — but kFlagUnordered, which the abundance ranks in front of
      // this build have just set or left at 0 (swa_launch_abundance_rank) —, the stats, the guard's counters up to its second
      // opinion.  (A retry, or the build of a network call, comes with its flags cleared by its caller and clears the
      // guard's index counters alone.)
      static_assert(kFlagDuplicates == 0 && kFlagUnordered == 1, "status block: the flags around kFlagUnordered");
      clear_add(c, st->flags + kFlagDuplicates, sizeof(uint32_t));
      clear_add(c, st->flags + kFlagUnordered + 1, offsetof(swa_status_block, guard) + kGuardKeys * sizeof(uint64_t) - (kFlagUnordered + 1) * sizeof(uint32_t));
    } else {
      clear_add(c, st->guard, kGuardCall * sizeof(uint64_t));  // the guard's index counters: this build's
    }
    clear_add(c, ctx->d_stream[kSbOver].ptr, ((uint64_t)n + 8) & ~3ull);
    // (the entry behind the last bucket's counts of each index: the scan of the counts reads one past the end)
    for (int i = 0; i < 2; ++i) { clear_add(c, static_cast<uint32_t *>(ctx->d_stream[kSbKind + i].ptr) + (uint64_t)kListsPerIndex * buckets, sizeof(uint32_t)); }
    SWA_TRY(swa_clear_launch(ctx, c));
  }
  swa_lap(ctx, "buffers reserved, counters cleared");
  uint32_t * dflags = st->flags;                            // (cleared above — a new index — or by the caller: a retry, a network call's build)
  auto * scal = static_cast<uint64_t *>(ctx->d_stream[kSbScal].ptr);      // [0..3] level-0 chunk tables, [8 + i] totals (u32)
  const uint32_t win_a = ctx->ix.anchor_a, win_b = ctx->ix.anchor_b;
  const uint32_t minlen = anchor_minlen(ctx), window_mode = (win_a != 0 || win_b != 0) ? 1u : 0u;

  // ---- keys: records into the PONG halves (level 0 reads them from there), fingerprints likewise
  KeyArgs k{};
  k.lines = static_cast<const uint4 *>(ctx->d_stream[kSbLines].ptr);
  k.line_quads = lq;
  k.seqs = ctx->db.seqs; k.seq_off = ctx->db.seq_off;
  k.n = n;
  for (int i = 0; i < 2; ++i) {
    k.list[i] = routed && !by_rec ? route.ids[i] : nullptr;
    k.list_count[i] = routed ? route.m[i] : 0;
    k.rec[i] = static_cast<unsigned long long *>(ctx->d_stream[kSbRec + 2 * i + 1].ptr);
  }
  k.owner_rank = ctx->owner_rank; k.owner_world = ctx->owner_world;
  k.win_a = win_a; k.win_b = win_b; k.minlen = minlen; k.window_mode = window_mode;
  k.nwin = ctx->ix.anchor_w / 32u;
  k.flags = dflags;
  k.guard = reinterpret_cast<unsigned long long *>(st->guard);
  // (single GPU, the whole database keyed: the short sequences and their possible neighbours become members of the plain
  // kernel's table; a rank of a multi-GPU job keeps the database-wide table for them)
  k.mark_short = (!routed && ctx->owner_world == 1u) ? static_cast<uint8_t *>(ctx->d_stream[kSbOver].ptr) : nullptr;
  if (const char * e = getenv("SWA_D1_GUARD_TEST")) {         // (test hook: a wrong index, on purpose; "...-once": only the first build)
    static int builds = 0;
    const bool once = strstr(e, "-once") != nullptr;
    if (!once || builds++ == 0) { k.fault = e[0] == 'm' ? 1u : (e[0] == 'd' ? 2u : 0u); }
  }
  if (routed) {
    hipLaunchKernelGGL(k_set_flags, dim3(1), dim3(1), 0, ctx->stream, dflags,
                       ctx->up.d1.db_shortest < minlen ? 1u : 0u, 0xFFFFFFFFu - ctx->up.d1.db_shortest);
  }
  if (by_rec) {   // (the records were made by the ranks that hold the amplicons' slices: what k_keys would have counted)
    hipLaunchKernelGGL(k_set_guard_made, dim3(1), dim3(1), 0, ctx->stream, k.guard, route.m[0], route.m[1]);
  }
  swa_t0(ctx, kTimeKeys);
  if (by_rec) { /* nothing to key */ }
  else if (keys_hist) {
    const uint32_t ntiles = (uint32_t)((records + j.tile - 1) / j.tile);
    for (int i = 0; i < 2; ++i) {
      k.hist_cnt[i] = static_cast<uint32_t *>(ctx->d_stream[kSbCnt + i].ptr);
      k.hist_ctile[i] = static_cast<uint32_t *>(ctx->d_stream[kSbTile + i].ptr);
    }
    k.hist_bits = j.plan.bits[0]; k.hist_tile = j.tile; k.hist_ntiles = ntiles;
    k.hist_run_bits = j.max_tiles0 >= (uint64_t)ctx->num_cus * 8 ? 4u : 0u;
    const dim3 hgrid((unsigned)((std::min<uint64_t>(ntiles, (uint64_t)ctx->num_cus * 8) + 7) & ~7ull), 1u);
    hipLaunchKernelGGL(k_keys<true>, hgrid, dim3(256), 0, ctx->stream, k);
    j.hist0_done = true;
    j.tiles0_done = true;
  } else {
    const dim3 kgrid((unsigned)swa_grid_for(ctx, records, 256, 8), routed ? 2u : 1u);
    hipLaunchKernelGGL(k_keys<false>, kgrid, dim3(256), 0, ctx->stream, k);
  }
  swa_t1(ctx, kTimeKeys);
  swa_lap(ctx, "k_keys");

  // ---- partition by the top bits of the key
  for (int i = 0; i < 2; ++i) {
    j.buf[i][0] = static_cast<unsigned long long *>(ctx->d_stream[kSbRec + 2 * i].ptr);
    j.buf[i][1] = static_cast<unsigned long long *>(ctx->d_stream[kSbRec + 2 * i + 1].ptr);
    j.in[i] = by_rec ? route.rec[i] : j.buf[i][1];
    j.cstart0[i] = nullptr; j.cstride0[i] = routed ? route.m[i] : n;   // (one chunk: [0, records of this index))
    j.cnt[i] = static_cast<uint32_t *>(ctx->d_stream[kSbCnt + i].ptr);
    j.ctile[i] = static_cast<uint32_t *>(ctx->d_stream[kSbTile + i].ptr);
    j.starts[i] = static_cast<uint64_t *>(ctx->d_stream[kSbStart + i].ptr);
    j.partial[i] = static_cast<uint32_t *>(ctx->d_stream[kSbPartial + i].ptr);
    j.total[i] = reinterpret_cast<uint32_t *>(scal + 8 + i);
  }
  // (no second array travels with the records: the fingerprints of rounds 3-5 served k_group1's search for identical
  // sequences, which the prefix pass of the pair kernels now does on the sequences themselves)
  j.starts_stride = e_start + 2;
  swa_t0(ctx, kTimeKeyPartition);
  SWA_TRY(swa_part_run(ctx, j));
  swa_t1(ctx, kTimeKeyPartition);
  swa_lap(ctx, "key partition");
  ctx->ix.part_starts_at = (uint64_t)(j.bstart[0] - j.starts[0]);   // (the same place in both indexes' buffers)
  ctx->ix.part_buckets = j.buckets;
  ctx->ix.part_starts_valid = true;
  if (!ctx->up.d1.guard_keys_done) {
    // the guard's second opinion on the key records, once per uploaded database: from the packed database against what the
    // partition holds (k_guard_db / k_guard_records); compared at the next guard_check
    auto * guard = reinterpret_cast<unsigned long long *>(st->guard);
    SWA_HIP(ctx, hipMemsetAsync(guard + kGuardKeys, 0, sizeof(st->guard) - kGuardKeys * sizeof(uint64_t), ctx->stream));
    GuardDbArgs gd{};
    gd.seqs = ctx->db.seqs; gd.seq_off = ctx->db.seq_off; gd.seqlen = ctx->db.seqlen; gd.n = n;
    for (int i = 0; i < 2; ++i) { gd.list[i] = k.list[i]; gd.list_count[i] = routed ? route.m[i] : 0; gd.list_rec[i] = by_rec ? route.rec[i] : nullptr; }
    gd.owner_rank = k.owner_rank; gd.owner_world = k.owner_world; gd.win_a = win_a; gd.win_b = win_b; gd.nwin = k.nwin;
    gd.out = guard + kGuardKeysDb;
    hipLaunchKernelGGL(k_guard_db, dim3((unsigned)swa_grid_for(ctx, records, 256, 8), routed ? 2u : 1u), dim3(256), 0, ctx->stream, gd);
    GuardRecArgs gr{};
    for (int i = 0; i < 2; ++i) { gr.rec[i] = j.out[i]; gr.total[i] = j.total[i]; }
    gr.out = guard + kGuardKeysRec;
    hipLaunchKernelGGL(k_guard_records, dim3((unsigned)swa_grid_for(ctx, records, 256, 8), 2u), dim3(256), 0, ctx->stream, gr);
    ctx->up.d1.guard_keys_pending = true;
  }

  swa_lap(ctx, "guard: second opinion");
  // ---- groups
  GroupArgs g{};
  for (int i = 0; i < 2; ++i) {
    GroupIdx & x = g.g[i];
    x.rec = const_cast<unsigned long long *>(j.out[i]);
    x.bstart = j.bstart[i];
    x.buckets = j.buckets;
    x.members = static_cast<uint32_t *>(ctx->d_stream[kSbMembers + i].ptr);
    x.items_tmp = j.buf[i][j.last ^ 1];
    x.kind_cnt = static_cast<uint32_t *>(ctx->d_stream[kSbKind + i].ptr);
  }
  g.pair_big = kPairBigCap; g.group_cap = kStreamGroupCap;   // (the tiled pair kernel serves every group up to that)
  g.flags = dflags;
  g.guard = k.guard;
  g.over = static_cast<uint8_t *>(ctx->d_stream[kSbOver].ptr);
  swa_t0(ctx, kTimeGroups);
  {
    if (!ctx->g1_lds_opt_in) {
      // (128 KB of dynamic LDS: above the 64 KB a kernel gets unasked.  The attribute belongs to the function ON A DEVICE:
      // once per context, not once per process — swa_multi_* runs a context per GPU in one process)
      SWA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_group1), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kG1LdsBytes));
      ctx->g1_lds_opt_in = true;
    }
    hipLaunchKernelGGL(k_group1, dim3((unsigned)std::min<uint64_t>(buckets, (uint64_t)ctx->num_cus), 2), dim3(kG1Threads), kG1LdsBytes, ctx->stream, g);
  }
  swa_t1(ctx, kTimeGroups);                                   // (k_group1 alone; the work lists below count in kTimeIndex, the whole build)

  // ---- work lists
  FlatScanArgs f{};
  ListArgs la{};
  for (int i = 0; i < 2; ++i) {
    f.v[i] = g.g[i].kind_cnt; f.units[i] = nullptr; f.fixed[i] = (uint64_t)kListsPerIndex * buckets + 1;
    f.partial[i] = j.partial[i]; f.total[i] = reinterpret_cast<uint32_t *>(scal + 10 + i);
    ListIdx & x = la.x[i];
    x.items_tmp = g.g[i].items_tmp; x.bstart = g.g[i].bstart; x.kind_pos = g.g[i].kind_cnt; x.buckets = (uint32_t)buckets;
    x.l.items = static_cast<swa_item *>(ctx->d_aitems[i].ptr);
    x.l.region = regions;
    x.l.counters = st->counters + kCounterBase + (uint32_t)i * kWidthClasses * 8u;
    x.l.pair_big = g.pair_big;
  }
  const dim3 grid_l((unsigned)std::min<uint64_t>((buckets + 3) / 4, (uint64_t)ctx->num_cus * 8), 2);
  if (plan.lists_inline) {
    // (every workgroup adds up the counts before its buckets itself — only the lists of width classes this database has)
    uint32_t mask = 0;
    for (uint32_t c = 0; c < kWidthClasses; ++c) { if (ctx->up.d1.class_pop[c] != 0) { mask |= ((1u << kListKinds) - 1u) << (c * kListKinds); } }
    for (int i = 0; i < 2; ++i) { la.x[i].list_mask = mask; }
    hipLaunchKernelGGL(k_group_lists<true>, grid_l, dim3(256), 0, ctx->stream, la);
  } else {
    const dim3 grid_k((unsigned)std::min<uint64_t>(((uint64_t)kListsPerIndex * buckets + kFlatChunk) / kFlatChunk, (uint64_t)ctx->num_cus * 8), 2);
    swa_flat_scan(ctx, grid_k, f);
    hipLaunchKernelGGL(k_group_lists<false>, grid_l, dim3(256), 0, ctx->stream, la);
  }
  ctx->ix.lists_form = plan.lists_inline ? 1 : 0;
  SWA_HIP(ctx, hipGetLastError());
  swa_lap(ctx, "groups + work lists");
  ctx->ix.list_regions_items = item_room;
  ctx->ix.anchor_ready = true;
  ctx->ix.stream_index = true;
  ctx->ix.guard_index = true;
  return SWA_OK;
}

// the pair kernels by (pass, record width W in words, window width NW in words): W = 5 / 8 / 15 / 21 (width_words), NW = 1 / 2
// — and 4 with W >= 15: 128-nt windows need sequences of 257 nt
#define SWA_PAIR_CASE(KERNEL, P, WW, NN) \
  if (pass == P && width == WW && nwin == NN) { hipLaunchKernelGGL((KERNEL<P, WW, NN>), dim3(grid), dim3(kThreads), 0, ctx->stream, a); return SWA_OK; }
#define SWA_PAIR_WIDTH(KERNEL, WW) \
  SWA_PAIR_CASE(KERNEL, 0, WW, 1) SWA_PAIR_CASE(KERNEL, 1, WW, 1) SWA_PAIR_CASE(KERNEL, 0, WW, 2) SWA_PAIR_CASE(KERNEL, 1, WW, 2)
#define SWA_PAIR_CASES(KERNEL) \
  SWA_PAIR_WIDTH(KERNEL, 5) SWA_PAIR_WIDTH(KERNEL, 8) SWA_PAIR_WIDTH(KERNEL, 15) SWA_PAIR_WIDTH(KERNEL, 21) \
  SWA_PAIR_CASE(KERNEL, 0, 15, 4) SWA_PAIR_CASE(KERNEL, 1, 15, 4) SWA_PAIR_CASE(KERNEL, 0, 21, 4) SWA_PAIR_CASE(KERNEL, 1, 21, 4)
// (k_d1_group_pairs keeps a record per thread in LDS: static up to W = 8, dynamic — opted in per launch: the attribute belongs
// to the function on a device — for W = 15 / 21)
#define SWA_PAIR_CASE_DYN(KERNEL, P, WW, NN) \
  if (pass == P && width == WW && nwin == NN) { \
    const int bytes = (int)PairLayout<WW>::kDynamicBytes; \
    constexpr uint32_t bit_ = 1u << (P + (WW == 21 ? 2 : 0) + (NN == 2 ? 4 : (NN == 4 ? 8 : 0))); \
    if (bytes != 0 && (ctx->pair_lds_opt_in & bit_) == 0u) {     /* (once per context: the call costs tens of microseconds now and then) */ \
      SWA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&KERNEL<P, WW, NN>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes)); \
      ctx->pair_lds_opt_in |= bit_; \
    } \
    hipLaunchKernelGGL((KERNEL<P, WW, NN>), dim3(grid), dim3(kThreads), (size_t)bytes, ctx->stream, a); return SWA_OK; }
#define SWA_PAIR_WIDTH_DYN(KERNEL, WW) \
  SWA_PAIR_CASE_DYN(KERNEL, 0, WW, 1) SWA_PAIR_CASE_DYN(KERNEL, 1, WW, 1) SWA_PAIR_CASE_DYN(KERNEL, 0, WW, 2) SWA_PAIR_CASE_DYN(KERNEL, 1, WW, 2)
static int launch_group_pairs(swa_ctx * ctx, int pass, int width, int nwin, int grid, const AnchorArgs & a) {
  SWA_PAIR_WIDTH_DYN(k_d1_group_pairs, 5) SWA_PAIR_WIDTH_DYN(k_d1_group_pairs, 8) SWA_PAIR_WIDTH_DYN(k_d1_group_pairs, 15) SWA_PAIR_WIDTH_DYN(k_d1_group_pairs, 21)
  SWA_PAIR_CASE_DYN(k_d1_group_pairs, 0, 15, 4) SWA_PAIR_CASE_DYN(k_d1_group_pairs, 1, 15, 4) SWA_PAIR_CASE_DYN(k_d1_group_pairs, 0, 21, 4) SWA_PAIR_CASE_DYN(k_d1_group_pairs, 1, 21, 4)
  return swa_fail_msg(ctx, SWA_E_ARG, "pair kernels: no kernel for this record / window width");
}
static int launch_pairs_tiled(swa_ctx * ctx, int pass, int width, int nwin, int grid, const AnchorArgs & a) {
  SWA_PAIR_CASES(k_d1_pairs_tiled)
  return swa_fail_msg(ctx, SWA_E_ARG, "pair kernels: no kernel for this record / window width");
}

// workgroups of k_d1_group_pairs<*, W, *> that one CU holds at a time (registers and LDS: the occupancy API; 1..8)
static int pair_blocks_per_cu(swa_ctx * ctx, uint32_t cls) {
  int & c = ctx->pair_blocks[cls];                        // (per context: swa_multi runs one context per GPU on its own host thread)
  if (c == 0) {
    int nb = 0;
    const hipError_t e = cls == 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_d1_group_pairs<0, 5, 1>, kThreads, 0)
                       : cls == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_d1_group_pairs<0, 8, 1>, kThreads, 0)
                       : cls == 2 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_d1_group_pairs<0, 15, 1>, kThreads, PairLayout<15>::kDynamicBytes)
                                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_d1_group_pairs<0, 21, 1>, kThreads, PairLayout<21>::kDynamicBytes);
    c = (e == hipSuccess && nb >= 1) ? std::min(nb, 8) : (cls <= 1u ? 4 : (cls == 2u ? 2 : 1));
  }
  return c;
}

// per-wave link segments: one per wave of the largest launch (d_seg_fill: [fills | members staged, pass 0 | pass 1])
static uint32_t seg_count(const swa_ctx * ctx) { return (uint32_t)ctx->num_cus * 8u * kWaves; }

// anchored network over [first, first+count): per pass and width class the pair kernels over that class's work lists,
// then the seeds (or halves of seeds) left to the plain kernel; links in the per-wave segments
static int launch_network_anchored(swa_ctx * ctx, int ncb, uint32_t first, uint32_t count) {
  // (the status block's counters from kCounterBase on — the lists of k_group_lists — were made at index build: not cleared here)
  swa_status_block * st = swa_status(ctx);
  uint32_t * acounters = st->counters;
  SWA_TRY(swa_reserve(ctx, ctx->d_afallback, (2ull * count + 16) * sizeof(swa_fallback)));
  ClearList clears{};
  clear_add(clears, st->stats, sizeof(st->stats));
  // the guard's counters of this network call — and with kGuardMisfiled what k_group1 counted into the same word
  // (kGuardBucketTotal) while the index was built: that count lives from the build to this clear and is never read
  clear_add(clears, st->guard + kGuardCall, (kGuardKeys - kGuardCall) * sizeof(uint64_t));
  clear_add(clears, acounters, kCounterBase * sizeof(uint32_t));
  clear_add(clears, ctx->d_seg_fill.ptr, 3ull * seg_count(ctx) * sizeof(uint32_t));   // segment fills | members staged, per pass
  // work counters of k_d1_group_pairs (per pass and class): 2^shard_bits of them, kSchedStride entries apart
  // (a workgroup serves the bundles of shard blockIdx.x mod 2^shard_bits: every shard needs a workgroup — ADVICE r03)
  uint32_t shard_bits = 6;
  while (shard_bits > 0 && (1u << shard_bits) > (uint32_t)ctx->num_cus) { --shard_bits; }
  {
    const uint64_t bytes = ((2ull * kWidthClasses) << shard_bits) * kSchedStride * sizeof(uint32_t);
    SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbSched], bytes));
    clear_add(clears, ctx->d_stream[kSbSched].ptr, bytes);
  }
  // (the CSR stage's count of buckets left to whole workgroups: csr_from_chunks)
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbHeavy], csr_heavy_bytes(count)));
  clear_add(clears, ctx->d_stream[kSbHeavy].ptr, sizeof(uint32_t));
  SWA_TRY(swa_clear_launch(ctx, clears));
  const bool zlds = 4ull * ctx->zobrist_len * sizeof(uint64_t) <= kMaxZobristLds;
  const uint32_t maxwords = (ctx->db.longest + 31u) >> 5;
  swa_t0(ctx, kTimeNetwork);
  const bool window_mode = ctx->ix.anchor_a != 0 || ctx->ix.anchor_b != 0;
  uint64_t item_room = 0;
  const ListRegions regions = list_regions(ctx, &item_room);
  if (item_room != ctx->ix.list_regions_items) { return swa_fail_msg(ctx, SWA_E_ARG, "d=1 network: the work lists in place were laid out for another database"); }
  const int nwin = (int)(ctx->ix.anchor_w / 32u);
  for (int pass = 0; pass < 2; ++pass) {
    swa_t0(ctx, kTimePass + pass);
    AnchorArgs a{};
    a.pass = pass;
    a.no_cluster_breaking = ncb;
    a.first = first; a.count = count;
    a.edges = static_cast<uint64_t *>(ctx->d_edges.ptr);
    a.seg_cap = ctx->seg_cap;
    a.seg_fill = static_cast<uint32_t *>(ctx->d_seg_fill.ptr);
    a.minlen = anchor_minlen(ctx);
    a.win_word = ctx->ix.anchor_a / 32u;
    a.win_word_b = ctx->ix.anchor_b / 32u;
    a.window_mode = window_mode ? 1u : 0u;
    a.seg_staged = static_cast<uint32_t *>(ctx->d_seg_fill.ptr) + (uint64_t)(1 + pass) * seg_count(ctx);
    a.guard = reinterpret_cast<unsigned long long *>(st->guard);
    a.flags = st->flags;
    a.shard_bits = shard_bits;
    a.ids = static_cast<const uint32_t *>(ctx->d_stream[kSbMembers + pass].ptr);
    a.lines = static_cast<const uint4 *>(ctx->d_stream[kSbLines].ptr);
    a.line_quads = ctx->up.d1.lines_quads;
    a.pair_items = static_cast<const swa_item *>(ctx->d_aitems[pass].ptr);
    for (uint32_t cls = 0; cls < kWidthClasses; ++cls) {
      // (a group of class c has a member of class c: no such sequences, no such groups.  Lines too narrow for the class's
      // records cannot occur: the lines are as wide as the longest sequence needs)
      if (ctx->up.d1.class_pop[cls] == 0) { continue; }
      const int width = width_words(cls);
      if (nwin == 4 && width < 15) { return swa_fail_msg(ctx, SWA_E_ARG, "pair kernels: 128-nt windows with sequences of 256 nt or less"); }
      const uint32_t pc = (uint32_t)pass * kWidthClasses + cls;
      for (uint32_t k = 0; k <= kPairClasses; ++k) { a.pair_region[k] = regions.at[cls][k]; }
      a.pair_counters = acounters + kCounterBase + pc * 8u;
      a.items = a.pair_items + regions.at[cls][kPairClasses + 1u];
      a.item_count = a.pair_counters + kPairClasses + 1u;
      a.sched_big = acounters + kCounterSchedBig + 2 * pc;
      a.sched_tiled = acounters + kCounterSchedTiled + 2 * pc;
      a.sched_wide = static_cast<uint32_t *>(ctx->d_stream[kSbSched].ptr) + ((uint64_t)pc << shard_bits) * kSchedStride;
      // (the pair kernel hands its work out through counters: exactly the workgroups that are resident together, no second round;
      // no launch over lists the index build found empty)
      const uint32_t * have = ctx->ix.list_counts_ready ? ctx->ix.list_counts + pc * 8u : nullptr;
      bool any_pairs = have == nullptr;
      for (uint32_t k = 0; k <= kPairClasses && have != nullptr; ++k) { any_pairs = any_pairs || have[k] != 0u; }
      // Bundles per visit of a work counter: 4 where every wave has dozens of bundles to go through (10 M amplicons: the counters
      // are what limits then — 0.78 / 1.21 / 2.2 ms with 4 / 2 / 1), fewer where the waves' shares are what limits (1 M: 2.4
      // bundles a wave — 0.072 / 0.049 / 0.037 ms a pass with 4 / 2 / 1)
      const int pgrid = ctx->num_cus * pair_blocks_per_cu(ctx, cls);
      {
        uint64_t bundles = 0;
        for (uint32_t k = 0; k < kPairClasses && have != nullptr; ++k) { bundles += ((uint64_t)have[k] + (16u >> k) - 1u) >> (4u - k); }
        const uint64_t waves = (uint64_t)pgrid * 4u;
        a.batch = have == nullptr || bundles >= 16u * waves ? 4u : (bundles >= 8u * waves ? 2u : 1u);
      }
      if (any_pairs) { SWA_TRY(launch_group_pairs(ctx, pass, width, nwin, pgrid, a)); }
      if (have == nullptr || have[kPairClasses + 1u] != 0u) { SWA_TRY(launch_pairs_tiled(ctx, pass, width, nwin, ctx->num_cus * (cls <= 1u ? 8 : 4), a)); }
    }
    swa_t1(ctx, kTimePass + pass);
    SWA_HIP(ctx, hipGetLastError());
  }
  // seeds (or halves of seeds) the anchored passes skipped (a lean build has made sure there are none: no sequence
  // too short, no oversized group — and what holds for the whole database holds for every part of it)
  const bool use_member_table = ctx->ix.member_index && !ctx->ix.full_index;
  if (ctx->ix.full_index || ctx->ix.member_index) {
    hipLaunchKernelGGL(k_stream_fallback, dim3(swa_grid_for(ctx, count, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.seqlen, first, count,
                       static_cast<const uint8_t *>(ctx->d_stream[kSbOver].ptr), static_cast<swa_fallback *>(ctx->d_afallback.ptr), acounters + kCounterFallback,
                       ctx->owner_rank, ctx->owner_world, ctx->db.seqs, ctx->db.seq_off, anchor_minlen(ctx));
  }
  NetArgs f{};
  f.seqs = ctx->db.seqs; f.seq_off = ctx->db.seq_off; f.seqlen = ctx->db.seqlen; f.abundance = ctx->db.abundance;
  f.zobrist = static_cast<const uint64_t *>(ctx->d_zobrist.ptr);
  f.zlen = ctx->zobrist_len; f.maxwords = maxwords;
  f.table = static_cast<const swa_slot *>(use_member_table ? ctx->d_stream[kSbMTable].ptr : ctx->d_table.ptr);
  f.tmask = (use_member_table ? ctx->ix.mtable_size : ctx->ix.table_size) - 1;
  f.bloom = static_cast<const uint64_t *>(use_member_table ? ctx->d_stream[kSbMBloom].ptr : ctx->d_bloom.ptr);
  f.bmask = (use_member_table ? ctx->ix.mbloom_words : ctx->ix.bloom_words) - 1;
  f.patterns = static_cast<const uint64_t *>(ctx->d_patterns.ptr);
  f.no_cluster_breaking = ncb;
  f.first = first; f.count = count;
  f.edges = static_cast<uint64_t *>(ctx->d_edges.ptr);
  f.seg_cap = ctx->seg_cap;
  f.seg_fill = static_cast<uint32_t *>(ctx->d_seg_fill.ptr);
  f.fallback = static_cast<const swa_fallback *>(ctx->d_afallback.ptr);
  f.fallback_count = acounters + kCounterFallback;
  f.aux = static_cast<const swa_aux *>(ctx->d_aux.ptr);
  f.owner_rank = 0; f.owner_world = 1;                       // the list already is this rank's share
  f.window_mode = window_mode ? 1u : 0u; f.win_word = ctx->ix.anchor_a / 32u; f.anchor_w = ctx->ix.anchor_w;
  const size_t flds = sizeof(uint64_t) * ((zlds ? 4ull * ctx->zobrist_len : 0ull) + 1024ull +
                                          kWaves * ((size_t)(maxwords + 2u) + kQueueCap + kQueueCap / 2));
  const int fgrid = swa_grid_for(ctx, count, kWaves, 8);
  // (a rank that built only its owned groups has no table: by construction its fallback list is
  // empty — network_run checks the count and builds the full index if that ever fails to hold)
  if (!ctx->ix.full_index && !ctx->ix.member_index) { /* nothing to probe against */ }
  else if (zlds) { hipLaunchKernelGGL((k_d1_probe<true, 2>), dim3(fgrid), dim3(kThreads), flds, ctx->stream, f); }
  else { hipLaunchKernelGGL((k_d1_probe<false, 2>), dim3(fgrid), dim3(kThreads), flds, ctx->stream, f); }
  swa_t1(ctx, kTimeNetwork);
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}

// Zobrist table in HBM (it only depends on its length: uploaded once) + room for the hashes
int swa_prepare_hashing(swa_ctx * ctx) {
  const uint32_t n = ctx->db.n;
  ctx->zobrist_len = ctx->db.longest + 2;                  // db.cc:652-653 (sequence part)
  SWA_TRY(swa_reserve(ctx, ctx->d_seqhash, uint64_t(n) * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_aux, uint64_t(n) * sizeof(swa_aux)));
  if (ctx->zobrist_resident != ctx->zobrist_len) {
    std::vector<uint64_t> zob;
    swa_zobrist_table(ctx->zobrist_len, zob);
    SWA_TRY(swa_reserve(ctx, ctx->d_zobrist, zob.size() * sizeof(uint64_t)));
    SWA_HIP(ctx, hipMemcpyAsync(ctx->d_zobrist.ptr, zob.data(), zob.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));      // zob is a host temporary
    ctx->zobrist_resident = ctx->zobrist_len;
  }
  return SWA_OK;
}

// sequence hashes + the XOR streams the plain kernel's restricted enumeration reads (swa_aux)
static int launch_seqhash(swa_ctx * ctx, const uint8_t * only = nullptr) {
  const uint32_t n = ctx->db.n;
  const size_t zbytes = 4ull * ctx->zobrist_len * sizeof(uint64_t);
  const bool zlds = zbytes <= kMaxZobristLds;
  swa_t0(ctx, kTimeSeqhash);
  const int hgrid = swa_grid_for(ctx, n, 256, 8);
  if (zlds) {
    hipLaunchKernelGGL(k_seqhash<true>, dim3(hgrid), dim3(256), zbytes, ctx->stream, ctx->db.seqs, ctx->db.seq_off,
                       ctx->db.seqlen, static_cast<const uint64_t *>(ctx->d_zobrist.ptr), ctx->zobrist_len, n,
                       static_cast<uint64_t *>(ctx->d_seqhash.ptr), static_cast<swa_aux *>(ctx->d_aux.ptr), ctx->ix.anchor_w, only);
  } else {
    hipLaunchKernelGGL(k_seqhash<false>, dim3(hgrid), dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off,
                       ctx->db.seqlen, static_cast<const uint64_t *>(ctx->d_zobrist.ptr), ctx->zobrist_len, n,
                       static_cast<uint64_t *>(ctx->d_seqhash.ptr), static_cast<swa_aux *>(ctx->d_aux.ptr), ctx->ix.anchor_w, only);
  }
  SWA_HIP(ctx, hipGetLastError());
  swa_t1(ctx, kTimeSeqhash);
  return SWA_OK;
}

// Zobrist table + per-amplicon sequence hashes (src/db.cc:761, src/zobrist.cc:89-112) and the
// anchored-index metadata; shared by the d = 1 index and the d = 0 dereplication
int swa_hash_sequences(swa_ctx * ctx) {
  SWA_TRY(swa_prepare_hashing(ctx));
  return launch_seqhash(ctx);
}

// hashes of ALL amplicons + the database-wide table and Bloom filter (src/algod1.cc:188-208,
// src/bloompat.cc): what the plain kernel, the fastidious pass and the debug readers work on.
// Always built by a single-GPU index build; a rank that serves only the anchor groups it owns
// builds it on demand (rarely: see build_owned_index).
int swa_ensure_full_index(swa_ctx * ctx) {
  if (ctx->ix.full_index) { return SWA_OK; }
  SWA_TRY(swa_reserve(ctx, ctx->d_table, ctx->ix.table_size * sizeof(swa_slot)));
  SWA_TRY(swa_reserve(ctx, ctx->d_bloom, ctx->ix.bloom_words * sizeof(uint64_t)));
  SWA_TRY(swa_hash_sequences(ctx));
  swa_t0(ctx, kTimeTable);
  SWA_TRY(swa_d1_rebuild_table(ctx, nullptr));
  swa_t1(ctx, kTimeTable);
  ctx->ix.full_index = true;
  return SWA_OK;
}

// Anchor windows for this database, from a sample (k_anchor_sample): the smallest offset whose estimated share of
// amplicons in oversized groups and of too-short seeds is below 1 / 64 each; (0, 0) when nothing is skewed, which is
// the normal case.  Window mode needs the pair kernels (sequences up to 416 nt).
static int choose_anchor_windows(swa_ctx * ctx) {
  ctx->ix.anchor_a = ctx->ix.anchor_b = 0;
  ctx->ix.anchor_w = 32;
  SWA_TRY(ensure_db_lengths(ctx));
  const uint32_t shortest = ctx->up.d1.db_shortest;
  const uint32_t n = ctx->db.n;
  const uint32_t max_nwin = anchor_max_nwin(ctx);
  // the ends, as wide as the shortest sequence allows — unless the sample finds them skewed (conserved flanks), then 32-nt
  // windows moved inwards
  ctx->ix.anchor_w = 32u * anchor_nwin_for(shortest, 0u, max_nwin);
  if (windows_search_off()) { return SWA_OK; }
  const uint32_t stride = std::max<uint32_t>(1u, n / 65536u);
  const uint32_t samples = (n + stride - 1) / stride;
  const size_t slots = (size_t)2 * kSampleCandidates * kSampleSlots;
  SWA_TRY(swa_reserve(ctx, ctx->d_akeys[0], std::max<size_t>(ctx->d_akeys[0].bytes, slots * sizeof(uint64_t))));
  SWA_TRY(swa_reserve(ctx, ctx->d_acounts[0], std::max<size_t>(ctx->d_acounts[0].bytes, (slots + 16) * sizeof(uint32_t))));
  auto * keys = static_cast<unsigned long long *>(ctx->d_akeys[0].ptr);
  auto * counts = static_cast<uint32_t *>(ctx->d_acounts[0].ptr);
  uint32_t * stats = counts + slots;                         // [0..4) too short, [4..8) mass
  SWA_HIP(ctx, hipMemsetAsync(keys, 0xFF, slots * sizeof(uint64_t), ctx->stream));
  SWA_HIP(ctx, hipMemsetAsync(counts, 0, (slots + 16) * sizeof(uint32_t), ctx->stream));
  hipLaunchKernelGGL(k_anchor_sample, dim3(swa_grid_for(ctx, samples, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off,
                     ctx->db.seqlen, n, stride, keys, counts, stats, shortest, max_nwin);
  hipLaunchKernelGGL(k_sample_mass, dim3(swa_grid_for(ctx, slots, 256, 8)), dim3(256), 0, ctx->stream, counts, stride, stats + 4);
  uint32_t host[8] = {};
  SWA_HIP(ctx, hipMemcpyAsync(host, stats, sizeof(host), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // (kept for swa_d1_debug_read 5; sample_offset / sample_w: the ends, unless a candidate below qualifies)
  swa_db_facts::d1_facts & facts = ctx->up.d1;
  memcpy(facts.sample_stats, host, sizeof(host));
  facts.sample_stride = stride; facts.sample_count = samples;
  facts.sample_offset = 0; facts.sample_w = ctx->ix.anchor_w;
  facts.sample_taken = true;
  for (uint32_t c = 0; c < kSampleCandidates; ++c) {
    const bool few_short = host[c] <= samples / 64u || c == 0;
    if (host[4 + c] <= samples / 64u && few_short) {
      ctx->ix.anchor_a = ctx->ix.anchor_b = 32u * c;
      ctx->ix.anchor_w = 32u * anchor_nwin_for(shortest, 32u * c, max_nwin);
      facts.sample_offset = ctx->ix.anchor_a; facts.sample_w = ctx->ix.anchor_w;
      return SWA_OK;
    }
    if (!few_short) { break; }                               // (larger offsets only strand more seeds)
  }
  return SWA_OK;                                             // nothing qualifies: the ends it is (and the plain kernel for the giants)
}

// the anchor windows of this database: chosen from a sample once per upload (and corrected by the safety net of the
// first build if the sample misjudged), then reused
static int ensure_anchor_windows(swa_ctx * ctx) {
  if (!ctx->up.d1.windows_ready) {
    SWA_TRY(choose_anchor_windows(ctx));
    ctx->up.d1.windows_chosen = ctx->ix.anchor_a;
    ctx->up.d1.windows_w = ctx->ix.anchor_w;
    ctx->up.d1.windows_ready = true;
  }
  ctx->ix.anchor_a = ctx->ix.anchor_b = ctx->up.d1.windows_chosen;
  ctx->ix.anchor_w = ctx->up.d1.windows_w;
  return SWA_OK;
}

// Hash table + Bloom filter of the members of oversized groups ONLY (the streaming build marks them: one byte per
// amplicon), for the plain kernel that serves their halves: a neighbour that shares the window of an oversized group is
// a member of that group, so nothing else needs to be in the table — and a Bloom filter of a few megabytes stays in L2
// where the database-wide one (one byte per table slot: 33 MB at 10 M) is a random HBM / Infinity-Cache line per probe.
// Identical sequences among the members are found through the same table (k_dup_check), as the reference finds them
// while it inserts (src/algod1.cc:1131-1150).

static int build_member_index(swa_ctx * ctx, uint32_t dup_first, uint32_t dup_count) {
  ctx->ix.member_index = false;
  const uint32_t n = ctx->db.n;
  // Zobrist hashes + the XOR streams of the members (k_seqhash: nobody else is inserted, probed for or enumerated)
  SWA_TRY(swa_prepare_hashing(ctx));
  SWA_TRY(launch_seqhash(ctx, static_cast<const uint8_t *>(ctx->d_stream[kSbOver].ptr)));
  uint64_t slots = 1024;
  while (slots < 2ull * ctx->ix.over_mass) { slots <<= 1; }
  const uint64_t words = std::max<uint64_t>(slots >> 3, 1);  // one byte of filter per slot, as the reference sizes it
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbMTable], slots * sizeof(swa_slot)));
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbMBloom], words * sizeof(uint64_t)));
  auto * table = static_cast<swa_slot *>(ctx->d_stream[kSbMTable].ptr);
  auto * bloom = static_cast<uint64_t *>(ctx->d_stream[kSbMBloom].ptr);
  swa_t0(ctx, kTimeTable);
  hipLaunchKernelGGL(k_table_clear, dim3(swa_grid_for(ctx, slots, 256, 8)), dim3(256), 0, ctx->stream, table, slots, bloom, words);
  hipLaunchKernelGGL(k_table_insert, dim3(swa_grid_for(ctx, n, 256, 8)), dim3(256), 0, ctx->stream, static_cast<const uint64_t *>(ctx->d_seqhash.ptr), n,
                     static_cast<const uint8_t *>(ctx->d_stream[kSbOver].ptr), table, slots - 1, reinterpret_cast<unsigned long long *>(bloom), words - 1,
                     static_cast<const uint64_t *>(ctx->d_patterns.ptr));
  swa_t1(ctx, kTimeTable);
  swa_t0(ctx, kTimeDupCheck);
  if (dup_count != 0) {
    hipLaunchKernelGGL(k_dup_check, dim3(swa_grid_for(ctx, dup_count, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen,
                       static_cast<const uint64_t *>(ctx->d_seqhash.ptr), dup_first, dup_count, table, slots - 1, swa_status(ctx)->flags + kFlagDuplicates);
  }
  swa_t1(ctx, kTimeDupCheck);
  SWA_HIP(ctx, hipGetLastError());
  ctx->ix.mtable_size = slots;
  ctx->ix.mbloom_words = words;
  ctx->ix.member_index = true;
  return SWA_OK;
}

// Index build of a rank that serves only the anchor groups it owns (swa_d1_set_ownership,
// world > 1), without anything proportional to the database except streaming passes: abundance
// ranks, the anchor indexes of the owned groups (all their members), hashes and XOR streams of
// those members only, duplicates inside the owned prefix groups.  *needs_table is set when some
// seed can only be served by the plain kernel (a sequence shorter than 65 nt anywhere, a group
// too large for LDS) or the db order does not hold: the caller then builds the full index.
static int build_owned_index(swa_ctx * ctx, const RouteLists & route, bool * needs_table, uint32_t * dups, uint32_t * oversized_mass = nullptr,
                             uint32_t * shortest = nullptr) {
  swa_lap(ctx, "(owned index starts)");
  // (no Zobrist table, no hash / XOR-stream arrays here: the pair route needs none of them — 240 MB of HBM at 10 M and an
  // upload with its synchronisation per build; the member table and the database-wide table prepare them when they are built)
  SWA_TRY(swa_launch_abundance_rank(ctx));
  swa_lap(ctx, "abundance ranks");
  // streaming build (d1_stream.inc): keys, partition, groups + work lists + identical sequences, all in one go
  swa_t0(ctx, kTimeIndex);
  SWA_TRY(build_stream_index(ctx, route));
  swa_t1(ctx, kTimeIndex);
  // (ONE copy of the status block up to the split cursors: the flags, and how long the work lists are — the network call
  // then launches no kernel over an empty one)
  // (into the context's pinned mirror: a copy to pageable memory is staged by the runtime, ~15 us more per look)
  const swa_status_block * status = ctx->h_status;
  SWA_HIP(ctx, hipMemcpyAsync(ctx->h_status, ctx->d_status.ptr, offsetof(swa_status_block, cursors), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const uint32_t * flags = status->flags;
  *dups = flags[kFlagDuplicates];
  memcpy(ctx->ix.list_counts, status->counters + kCounterBase, sizeof(ctx->ix.list_counts));
  ctx->ix.list_counts_ready = true;
  if (oversized_mass != nullptr) { *oversized_mass = flags[kFlagOverMass]; }
  if (shortest != nullptr) { *shortest = 0xFFFFFFFFu - flags[kFlagShortest]; }
  if (flags[kFlagKeyOverflow] != 0) {                       // a bucket with more distinct keys than the group kernel's table: finer
    if (ctx->up.d1.stream_extra_bits >= 8) { return swa_fail_msg(ctx, SWA_E_DEVICE, "streaming index build: partition still too coarse"); }
    ctx->up.d1.stream_extra_bits += 2;
    SWA_HIP(ctx, hipMemsetAsync(swa_status(ctx)->flags, 0, sizeof(status->flags), ctx->stream));
    return build_owned_index(ctx, route, needs_table, dups, oversized_mass, shortest);
  }
  const bool unordered = flags[kFlagUnordered] != 0, unserved = flags[kFlagUnserved] != 0, oversized = flags[kFlagOversized] != 0;
  if (unordered) { ctx->up.d1.db_unordered = true; }
  *needs_table = unordered || unserved || oversized;
  // (groups left to the plain kernel — and, on a single GPU, sequences too short for two windows — are the ONLY reason: a
  // table of their members alone serves it — build_member_index)
  ctx->ix.only_oversized = !unordered && (oversized || unserved) &&
                        (!unserved || (ctx->owner_world == 1u && !route.routed()));
  ctx->ix.over_mass = flags[kFlagOverMass];
  return SWA_OK;
}

// The index build behind swa_d1_index_build, _range, _routed and _records, and the guard's rebuild
static int index_build(swa_ctx * ctx, uint32_t first, uint32_t count, const RouteLists & route, int * has_duplicates) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_index_build: no database"); }
  if (first > ctx->db.n || count > ctx->db.n - first) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_index_build_range: bad range"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t n = ctx->db.n;
  ctx->ix = {};                                             // the index in place ends here ...
  ctx->res = {};                                            // ... and a resident network belongs to the index it was made from
  const bool routed = route.routed();
  ctx->ix.index_first = first; ctx->ix.index_count = count; ctx->ix.index_routed = routed;   // (network_run_guarded repeats it)
  for (int slot : {kTimeSeqhash, kTimeTable, kTimeDupCheck, kTimeIndex, kTimeKeys, kTimeKeyPartition, kTimeGroups, kTimeLines}) { ctx->ev_used[slot] = false; }   // phases this build does not run report 0
  ctx->ix.table_size = swa_hashtable_size(n);
  const uint64_t bloom_bytes = ctx->ix.table_size < 8 ? 8 : ctx->ix.table_size;   // bloompat.cc:100-113
  ctx->ix.bloom_words = bloom_bytes >> 3;

  if (!ctx->patterns_resident) {                            // the 1024 Bloom patterns are constants: upload once
    std::vector<uint64_t> pat;
    swa_bloom_patterns(1024, 8, pat);
    SWA_TRY(swa_reserve(ctx, ctx->d_patterns, pat.size() * sizeof(uint64_t)));
    SWA_HIP(ctx, hipMemcpyAsync(ctx->d_patterns.ptr, pat.data(), pat.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));       // pat is a host temporary
    ctx->patterns_resident = true;
  }
  // (flags, stats and the guard's index / network counters lie together at the head of the status block: one fill, up to
  // the guard's second opinion)
  swa_status_block * st = swa_status(ctx);
  ctx->ix.anchor_usable = anchor_applicable(ctx);
  // (the streaming build clears this head with its own counters, one launch: nothing before its clear writes there but the
  // abundance ranks' kFlagUnordered, which that clear leaves alone; the other route fills it here)
  ctx->ix.head_clear_pending = ctx->ix.anchor_usable;
  if (!ctx->ix.anchor_usable) { SWA_HIP(ctx, hipMemsetAsync(st, 0, offsetof(swa_status_block, guard) + kGuardKeys * sizeof(uint64_t), ctx->stream)); }

  bool owned_ok = false;                                    // served without the database-wide table
  uint32_t group_dups = 0;
  // The lean build (no database-wide table / Bloom / table-based duplicate check) serves a single GPU as well
  // as a rank of a multi-GPU job: with world = 1 this GPU owns every anchor group.
  if (ctx->ix.anchor_usable) {
    bool needs_table = false;
    uint32_t mass = 0, shortest = 0;
    swa_lap(ctx, "(index build: before the windows)");
    SWA_TRY(ensure_anchor_windows(ctx));
    swa_lap(ctx, "anchor windows");
    const uint32_t sampled = ctx->ix.anchor_a;
    SWA_TRY(build_owned_index(ctx, route, &needs_table, &group_dups, &mass, &shortest));
    // Conserved flanks: when a noticeable part of the database sits in groups too large for LDS (everybody shares
    // the first or last 32 nt), the anchor windows move inwards, 32 nt at a time, as far as the shortest sequence
    // allows (every seed needs win_a + win_b + 65 nt), and the setting with the fewest stranded members wins.
    // (safety net behind the sample: the real build still found too many stranded members — try the next offsets.
    // Single GPU only: under ownership `mass` counts the oversized groups THIS rank owns, the ranks would settle on
    // different windows and divide the pairs differently; there the sampled choice — the same on every rank — stands
    // and oversized groups take the plain kernel)
    // (a routed build's lists were made under the sampled windows: no second thoughts)
    if (!routed && ctx->owner_world == 1 && needs_table && mass > n / 64u && !windows_search_off()) {
      uint32_t best = sampled, best_mass = mass;
      for (uint32_t w = sampled + 32u; 2u * w + kMinAnchoredLen <= shortest && w <= 96u; w += 32u) {
        ctx->ix.anchor_a = ctx->ix.anchor_b = w;
        ctx->ix.anchor_w = 32;                                     // (moved windows: anchor_nwin_for)
        SWA_HIP(ctx, hipMemsetAsync(st->flags, 0, sizeof(st->flags), ctx->stream));
        uint32_t m = 0;
        SWA_TRY(build_owned_index(ctx, route, &needs_table, &group_dups, &m));
        if (m < best_mass) { best_mass = m; best = w; }
        if (m <= n / 64u) { break; }
      }
      if (ctx->ix.anchor_a != best) {                            // (the last one tried was not the best: build that one again)
        ctx->ix.anchor_a = ctx->ix.anchor_b = best;
        ctx->ix.anchor_w = best == sampled ? ctx->up.d1.windows_w : 32u;
        SWA_HIP(ctx, hipMemsetAsync(st->flags, 0, sizeof(st->flags), ctx->stream));
        SWA_TRY(build_owned_index(ctx, route, &needs_table, &group_dups));
      }
    }
    ctx->up.d1.windows_chosen = ctx->ix.anchor_a;                     // (what the safety net settled on, for the next build)
    ctx->up.d1.windows_w = ctx->ix.anchor_w;
    owned_ok = !needs_table;
    if (!owned_ok && ctx->ix.only_oversized) {
      // nothing but groups too large for the pair kernels stands in the way: a table of their members is all the plain kernel needs.  Their
      // twins: a rank of a multi-GPU job answers for the groups it owns, whichever slice the members lie in; a single GPU honours the slice asked about
      SWA_TRY(build_member_index(ctx, ctx->owner_world > 1 ? 0u : first, ctx->owner_world > 1 ? n : count));
      owned_ok = true;
      // (the member table's own search for identical sequences may have raised the flag since the build looked at it)
      uint32_t * mirror = &ctx->h_status->flags[kFlagDuplicates];
      SWA_HIP(ctx, hipMemcpyAsync(mirror, st->flags + kFlagDuplicates, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
      SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
      group_dups = *mirror;
    }
    if (!owned_ok) { SWA_HIP(ctx, hipMemsetAsync(st->flags, 0, sizeof(st->flags), ctx->stream)); }
  }
  uint32_t flag = group_dups;
  if (!owned_ok) {
    SWA_TRY(swa_ensure_full_index(ctx));
    swa_t0(ctx, kTimeDupCheck);
    if (count > 0) {
      hipLaunchKernelGGL(k_dup_check, dim3(swa_grid_for(ctx, count, 256, 8)), dim3(256), 0, ctx->stream, ctx->db.seqs, ctx->db.seq_off,
                         ctx->db.seqlen, static_cast<const uint64_t *>(ctx->d_seqhash.ptr), first, count,
                         static_cast<const swa_slot *>(ctx->d_table.ptr), ctx->ix.table_size - 1,
                         swa_status(ctx)->flags + kFlagDuplicates);
    }
    SWA_HIP(ctx, hipGetLastError());
    swa_t1(ctx, kTimeDupCheck);
    if (ctx->ix.anchor_usable) {
      SWA_TRY(swa_launch_abundance_rank(ctx));
      SWA_HIP(ctx, hipGetLastError());
    }
    uint32_t flags[kFlagUnordered + 1] = {};                // duplicates, abundances not in descending order
    SWA_HIP(ctx, hipMemcpyAsync(flags, st->flags, sizeof(flags), hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    flag |= flags[kFlagDuplicates];
    if (flags[kFlagUnordered] != 0) { ctx->ix.anchor_usable = false; ctx->up.d1.db_unordered = true; }   // the anchored passes rely on the db order
  }
  ctx->ix.d1_ready = true;
  if (has_duplicates != nullptr) { *has_duplicates = flag != 0 ? 1 : 0; }
  if (flag != 0) {
    return swa_fail_msg(ctx, SWA_E_DUPLICATES, "some fasta entries have identical sequences");
  }
  return SWA_OK;
}

extern "C" int swa_d1_index_build_range(swa_ctx * ctx, uint32_t first, uint32_t count, int * has_duplicates) {
  return index_build(ctx, first, count, RouteLists{}, has_duplicates);
}
extern "C" int swa_d1_index_build(swa_ctx * ctx, int * has_duplicates) { return swa_d1_index_build_range(ctx, 0, ctx != nullptr ? ctx->db.n : 0, has_duplicates); }

// width of the anchor windows the last index build chose, in nucleotides (32, 64 or 128)
extern "C" uint32_t swa_d1_anchor_width(const swa_ctx * ctx) { return ctx != nullptr ? ctx->ix.anchor_w : 0; }

extern "C" uint64_t swa_d1_table_size(const swa_ctx * ctx) { return ctx != nullptr ? ctx->ix.table_size : 0; }

// the anchor windows the last index build chose: out2 = {nt from the start, nt from the end} (0, 0 = the first / last 32 nt)
extern "C" int swa_d1_anchor_windows(const swa_ctx * ctx, uint32_t * out2) {
  if (ctx == nullptr || out2 == nullptr) { return SWA_E_ARG; }
  out2[0] = ctx->ix.anchor_a; out2[1] = ctx->ix.anchor_b;
  return SWA_OK;
}

static size_t network_lds_bytes(const swa_ctx * ctx, bool zlds) {
  const uint32_t maxwords = (ctx->db.longest + 31u) >> 5;
  const size_t per_wave = (size_t)(maxwords + 2u) + kQueueCap + kQueueCap / 2;
  return sizeof(uint64_t) * ((zlds ? 4ull * ctx->zobrist_len : 0ull) + 1024ull + kWaves * per_wave);
}

// launches the network kernel for [first, first+count); leaves the links in the per-wave segments
static int launch_network(swa_ctx * ctx, int ncb, uint32_t first, uint32_t count) {
  NetArgs a{};
  a.seqs = ctx->db.seqs; a.seq_off = ctx->db.seq_off; a.seqlen = ctx->db.seqlen; a.abundance = ctx->db.abundance;
  a.zobrist = static_cast<const uint64_t *>(ctx->d_zobrist.ptr);
  a.zlen = ctx->zobrist_len;
  a.maxwords = (ctx->db.longest + 31u) >> 5;
  a.table = static_cast<const swa_slot *>(ctx->d_table.ptr);
  a.tmask = ctx->ix.table_size - 1;
  a.bloom = static_cast<const uint64_t *>(ctx->d_bloom.ptr);
  a.bmask = ctx->ix.bloom_words - 1;
  a.patterns = static_cast<const uint64_t *>(ctx->d_patterns.ptr);
  a.no_cluster_breaking = ncb;
  a.first = first; a.count = count;
  a.edges = static_cast<uint64_t *>(ctx->d_edges.ptr);
  a.seg_cap = ctx->seg_cap;
  a.seg_fill = static_cast<uint32_t *>(ctx->d_seg_fill.ptr);
  a.owner_rank = ctx->owner_rank; a.owner_world = ctx->owner_world;
  a.anchor_w = 32;
  SWA_HIP(ctx, hipMemsetAsync(swa_status(ctx)->stats, 0, sizeof(swa_status_block::stats), ctx->stream));
  const bool zlds = 4ull * ctx->zobrist_len * sizeof(uint64_t) <= kMaxZobristLds;
  const size_t lds = network_lds_bytes(ctx, zlds);
  const int grid = swa_grid_for(ctx, count, kWaves, 8);
  swa_t0(ctx, kTimeNetwork);
  if (zlds) { hipLaunchKernelGGL((k_d1_probe<true, 0>), dim3(grid), dim3(kThreads), lds, ctx->stream, a); }
  else { hipLaunchKernelGGL((k_d1_probe<false, 0>), dim3(grid), dim3(kThreads), lds, ctx->stream, a); }
  swa_t1(ctx, kTimeNetwork);
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}

// The guard (round 4).  The reference's network thread is serialised by a mutex and cannot return a partial
// network (src/algod1.cc:630-670); this pipeline is twenty kernels handing records to one another, and twice in three
// rounds a run lost the links of a few wavefronts' worth of amplicons without any error (DESIGN: the anomaly).  So the
// counts that must balance are kept and compared before a network leaves this file:
//   records keyed per index (k_keys)  =  members of listed + singleton + oversized groups (k_group1)
//   members of listed groups          =  members the pair kernels staged, per pass
//   no member sits in a group whose window key is not its own (pair_misfiled; key collisions excepted, exactly)
// and, for every CSR result whatever the route (csr_check),
//   links in the wave segments        =  links the partition sorted  =  the last CSR offset
// A mismatch is SWA_E_INTERNAL — never a short network.
static int guard_check(swa_ctx * ctx, const swa_status_block & status) {
  const uint64_t * g = status.guard, * staged = status.stats + kStatSeg + kSegStaged;
  const uint64_t * made = g + kGuardMade, * listed = g + kGuardListed, * single = g + kGuardSingleton, * over = g + kGuardOversized;
  char msg[256];
  if (g[kGuardMisfiled] != 0) {
    snprintf(msg, sizeof(msg), "d=1 guard: %llu member(s) filed under an anchor key that is not theirs", (unsigned long long)g[kGuardMisfiled]);
    return swa_fail_msg(ctx, SWA_E_INTERNAL, msg);
  }
  if (ctx->ix.stream_index && ctx->up.d1.guard_keys_pending) {
    ctx->up.d1.guard_keys_pending = false;
    for (int i = 0; i < 2; ++i) {
      const uint64_t from_db = g[kGuardKeysDb + i], from_records = g[kGuardKeysRec + i];
      if (from_db != from_records) {
        snprintf(msg, sizeof(msg), "d=1 guard: the %s derived from the amplicon lines are not the ones the packed database gives (%016llx / %016llx)",
                 i == 0 ? "prefix-side key records" : "suffix-side key records", (unsigned long long)from_records,
                 (unsigned long long)from_db);
        return swa_fail_msg(ctx, SWA_E_INTERNAL, msg);
      }
    }
    ctx->up.d1.guard_keys_done = true;
  }
  if (ctx->ix.stream_index && ctx->ix.guard_index) {
    for (int i = 0; i < 2; ++i) {
      if (made[i] != listed[i] + single[i] + over[i]) {
        snprintf(msg, sizeof(msg), "d=1 guard: index %d has %llu key records but %llu + %llu + %llu grouped members", i, (unsigned long long)made[i],
                 (unsigned long long)listed[i], (unsigned long long)single[i], (unsigned long long)over[i]);
        return swa_fail_msg(ctx, SWA_E_INTERNAL, msg);
      }
      if (staged[i] != listed[i]) {
        snprintf(msg, sizeof(msg), "d=1 guard: pass %d staged %llu members of %llu listed", i, (unsigned long long)staged[i], (unsigned long long)listed[i]);
        return swa_fail_msg(ctx, SWA_E_INTERNAL, msg);
      }
    }
  }
  return SWA_OK;
}
static int csr_check(swa_ctx * ctx, uint64_t csr_end, uint32_t links_sorted, uint64_t n_edges) {
  if (csr_end != n_edges || (uint64_t)links_sorted != (n_edges & 0xFFFFFFFFull)) {
    char msg[256];
    snprintf(msg, sizeof(msg), "d=1 guard: %llu links found, %u sorted, CSR ends at %llu", (unsigned long long)n_edges, links_sorted, (unsigned long long)csr_end);
    return swa_fail_msg(ctx, SWA_E_INTERNAL, msg);
  }
  return SWA_OK;
}

// The network over [first, first + count), left in HBM either as CSR (d_offsets / d_neighbours)
// or, when d_edge_list != nullptr, as one flat list of (source << 32 | target) links.
static int network_run(swa_ctx * ctx, int no_cluster_breaking, uint32_t first, uint32_t count, uint64_t * d_offsets,
                       uint32_t * d_neighbours, uint64_t * d_edge_list, uint64_t cap, uint64_t * total) {
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  swa_status_block * st = swa_status(ctx);
  // hits leave the kernels through per-wave segments of the edge buffer (no shared counter)
  const uint32_t nseg = seg_count(ctx);                       // >= waves of any launch below
  SWA_TRY(swa_reserve(ctx, ctx->d_seg_fill, 3ull * nseg * sizeof(uint32_t)));   // fills | members staged, pass 0 | pass 1
  if (ctx->seg_cap == 0) {
    ctx->seg_cap = 512;
    while (ctx->seg_cap < 8ull * count / nseg) { ctx->seg_cap <<= 1; }
    const char * env_cap = getenv("SWA_D1_SEG_CAP");          // test hook: start small, exercise the regrow path
    if (env_cap != nullptr && atoi(env_cap) > 0) { ctx->seg_cap = (uint64_t)atoi(env_cap); }
  }
  uint64_t n_edges = 0;
  uint64_t stream_link_cap = 0;
  bool clean = false;                                        // the last attempt ran to the end without a retry condition
  bool twins = false;                                        // the prefix pass of the pair kernels met identical sequences
  for (int attempt = 0; attempt < 8 && !clean; ++attempt) {
    SWA_TRY(swa_reserve(ctx, ctx->d_edges, uint64_t(nseg) * ctx->seg_cap * sizeof(uint64_t)));
    // (the segment fills start at zero: the anchored route clears them with its other counters — one launch —, the plain one here)
    if (!ctx->ix.anchor_usable) { SWA_HIP(ctx, hipMemsetAsync(ctx->d_seg_fill.ptr, 0, 3ull * nseg * sizeof(uint32_t), ctx->stream)); }
    if (ctx->ix.anchor_usable) {
      if (!(ctx->ix.anchor_ready && ctx->ix.stream_index)) {
        // (the streaming index serves any query range; it is rebuilt when the owner changed)
        swa_t0(ctx, kTimeIndex);
        SWA_TRY(swa_launch_abundance_rank(ctx));
        // (kFlagKeyOverflow .. kFlagShortest, what the streaming build raises: the previous owner's values must not survive
        // into this owner's build — kFlagUnserved is only ever set, kFlagOversized / kFlagOverMass accumulate)
        SWA_HIP(ctx, hipMemsetAsync(st->flags + kFlagKeyOverflow, 0, (kFlagsD1 - kFlagKeyOverflow) * sizeof(uint32_t), ctx->stream));
        SWA_TRY(build_stream_index(ctx, RouteLists{}));
        swa_t1(ctx, kTimeIndex);
        // The index of another owner (swa_d1_set_ownership after the build): the member table and its Bloom filter hold the
        // previous owner's oversized groups, so they are dropped, and whatever this owner's groups leave to the plain kernel
        // (kFlagUnserved, kFlagOversized) gets the database-wide table
        if (!ctx->ix.full_index) {
          uint32_t fl[kFlagOverMass + 1] = {};
          SWA_HIP(ctx, hipMemcpyAsync(fl, st->flags, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
          SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
          ctx->ix.member_index = false;
          if (fl[kFlagUnserved] != 0 || fl[kFlagOversized] != 0) { SWA_TRY(swa_ensure_full_index(ctx)); }
        }
      }
      SWA_TRY(launch_network_anchored(ctx, no_cluster_breaking, first, count));
    }
    else {
      SWA_TRY(swa_ensure_full_index(ctx));
      SWA_TRY(launch_network(ctx, no_cluster_breaking, first, count));
    }
    const bool check_unserved = ctx->ix.anchor_usable && !ctx->ix.full_index && !ctx->ix.member_index;
    // CSR assembly is enqueued right behind, before the host looks at the totals: every kernel
    // below guards its writes with `cap` / the segment capacity, so a run that turns out to
    // need bigger segments or a bigger neighbour buffer has only wasted these launches.
    // Offsets are always complete; neighbours only if they fit.
    swa_t0(ctx, kTimeCsr);
    if (d_edge_list != nullptr) {
      SWA_TRY(swa_d1_seg_compact(ctx, nseg, d_edge_list, cap));
    } else {
      // CSR: the links sorted by source with the partition primitive
      stream_link_cap = std::max<uint64_t>(std::max<uint64_t>(cap, stream_link_cap), 2ull * count + 1024);
      SWA_TRY(swa_d1_csr_stream(ctx, first, count, nseg, stream_link_cap, d_offsets, d_neighbours, cap, ctx->ix.anchor_usable));
    }
    SWA_HIP(ctx, hipGetLastError());
    swa_t1(ctx, kTimeCsr);
    // ONE copy of the status block's head: flags | stats (links, fullest segment, members staged) | the guard's counters |
    // last CSR offset, links sorted, fallback seeds listed
    swa_status_block * status = ctx->h_status;               // (the pinned mirror)
    SWA_HIP(ctx, hipMemcpyAsync(status, st, offsetof(swa_status_block, host_unserved), hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t unserved = check_unserved ? status->fallback_copy : 0u;   // fallback seeds listed while there is no table to serve them
    const uint64_t * seg = status->stats + kStatSeg;          // what was made of the segments (SegArgs / k_seg_reduce)
    const uint64_t fullest = seg[kSegFullest];
    const uint32_t anchor_overflow = status->flags[kFlagKeyOverflow];
    const bool guarded = ctx->ix.anchor_usable;
    n_edges = seg[kSegLinks];
    if (guarded && anchor_overflow != 0) {
      // a bucket of the index rebuilt above held more distinct keys than the group kernel's table: partition finer, again
      ctx->up.d1.stream_extra_bits = std::min<uint32_t>(ctx->up.d1.stream_extra_bits + 2, 8);
      ctx->ix.anchor_ready = false;
      continue;
    }
    if (check_unserved && unserved != 0) {                   // should not happen (build_owned_index looks for such seeds)
      SWA_TRY(swa_ensure_full_index(ctx));
      continue;
    }
    if (d_edge_list == nullptr && fullest <= ctx->seg_cap && n_edges > stream_link_cap) {
      // more links than the internal link buffers of the CSR stage hold (a first call with a small `cap`): bigger, again
      stream_link_cap = n_edges + 1024;
      continue;
    }
    if (fullest <= ctx->seg_cap) {
      clean = true;
      if (guarded) { SWA_TRY(guard_check(ctx, *status)); }
      if (d_edge_list == nullptr) { SWA_TRY(csr_check(ctx, status->csr_end, status->links_sorted, n_edges)); }
      twins = guarded && status->flags[kFlagDuplicates] != 0u;   // (the prefix pass met two identical sequences)
      break;
    }
    // one wave found more hits than its segment holds: grow the segments and run again (rare).
    // The small-group passes hand out work dynamically, so a wave's fill differs from run to run:
    // twice the observed maximum, not just the maximum
    while (ctx->seg_cap < 2 * fullest) { ctx->seg_cap <<= 1; }
  }
  if (!clean) {
    // counts[] / offsets include links the segment guards dropped: never hand that out as a result
    return swa_fail_msg(ctx, SWA_E_DEVICE, "swa_d1_network: per-wave link segments still overflowed after 8 attempts");
  }
  *total = n_edges;
  // Identical sequences (the reference: fatal while it fills its table, src/algod1.cc:1131-1150).  On the pair route they are
  // met here — two members of a prefix group whose sequences agree word for word — not by the index build (round 6).
  if (twins) { return swa_fail_msg(ctx, SWA_E_DUPLICATES, "some fasta entries have identical sequences"); }
  if (n_edges > cap) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_network: neighbour buffer too small"); }
  return SWA_OK;
}

// The reference cannot fail here (src/algod1.cc:630-670), so a drop-in must not exit where the reference would not: when
// the guard finds counts that do not balance, everything derived from the uploaded database (lines, lengths, ranks,
// windows, indexes) is made again and the step repeated — once; which count disagreed goes to stderr.  Only a second
// disagreement is SWA_E_INTERNAL.  (A routed build's id lists belong to the caller: multi.hip repeats its own exchange.)
static int network_run_guarded(swa_ctx * ctx, int no_cluster_breaking, uint32_t first, uint32_t count, uint64_t * d_offsets,
                               uint32_t * d_neighbours, uint64_t * d_edge_list, uint64_t cap, uint64_t * total) {
  const int rc = network_run(ctx, no_cluster_breaking, first, count, d_offsets, d_neighbours, d_edge_list, cap, total);
  if (rc != SWA_E_INTERNAL || ctx->ix.index_routed) { return rc; }
  const std::string first_msg = ctx->err;
  fprintf(stderr, "swarm-amd: %s; rebuilding the index from the packed database and repeating the step\n", first_msg.c_str());
  ++ctx->guard_retries;
  const uint32_t index_first = ctx->ix.index_first, index_count = ctx->ix.index_count;
  ctx->up.d1 = {};
  ctx->ix = {};
  int dup = 0;
  const int rb = index_build(ctx, index_first, index_count, RouteLists{}, &dup);
  if (rb != SWA_OK && rb != SWA_E_DUPLICATES) { return rb; }
  const int again = network_run(ctx, no_cluster_breaking, first, count, d_offsets, d_neighbours, d_edge_list, cap, total);
  if (again == SWA_E_INTERNAL) { ctx->err = first_msg + "; after a rebuild: " + ctx->err; }
  return again;
}

extern "C" int swa_d1_guard_retries(const swa_ctx * ctx) { return ctx != nullptr ? (int)ctx->guard_retries : 0; }

extern "C" int swa_d1_network_device(swa_ctx * ctx, int no_cluster_breaking, uint32_t first, uint32_t count,
                                     uint64_t * d_offsets, uint32_t * d_neighbours, uint64_t cap, uint64_t * total) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (!ctx->ix.d1_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_network: call swa_d1_index_build first"); }
  if (count == 0 || (uint64_t)first + count > ctx->db.n || d_offsets == nullptr || total == nullptr ||
      (d_neighbours == nullptr && cap != 0)) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_network: bad range or null buffer");
  }
  return network_run_guarded(ctx, no_cluster_breaking, first, count, d_offsets, d_neighbours, nullptr, cap, total);
}

extern "C" int swa_d1_network_edges_device(swa_ctx * ctx, int no_cluster_breaking, uint32_t first, uint32_t count,
                                           uint64_t * d_edge_list, uint64_t cap, uint64_t * total) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (!ctx->ix.d1_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_network: call swa_d1_index_build first"); }
  if (count == 0 || (uint64_t)first + count > ctx->db.n || d_edge_list == nullptr || total == nullptr) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_network_edges: bad range or null buffer");
  }
  return network_run_guarded(ctx, no_cluster_breaking, first, count, nullptr, nullptr, d_edge_list, cap, total);
}

extern "C" int swa_d1_route_slice(swa_ctx * ctx, uint32_t first, uint32_t count, uint32_t world, uint32_t * d_ids, uint64_t cap,
                                  uint32_t * d_counts) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_route_slice: no database"); }
  if (first > ctx->db.n || count > ctx->db.n - first) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_route_slice: bad range"); }
  if (world == 0 || world > kRouteMaxWorld || d_ids == nullptr || d_counts == nullptr || cap == 0) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_route_slice: bad argument (1..64 ranks)");
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(ensure_anchor_windows(ctx));
  SWA_HIP(ctx, hipMemsetAsync(d_counts, 0, (2ull * world + 1) * sizeof(uint32_t), ctx->stream));
  if (count != 0) {
    hipLaunchKernelGGL(k_anchor_route, dim3(swa_grid_for(ctx, (count + kRoutePerThread - 1) / kRoutePerThread, 256, 8)), dim3(256), 0, ctx->stream,
                       ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen, first, count, world, ctx->ix.anchor_a, ctx->ix.anchor_b, ctx->ix.anchor_w / 32u, d_ids, cap,
                       d_counts);
  }
  SWA_HIP(ctx, hipGetLastError());
  // the caller reads the counts next (and may do so from another stream: a context without a caller's stream works on
  // its own): they are final when this returns
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

extern "C" int swa_d1_index_build_routed(swa_ctx * ctx, const uint32_t * d_ids_prefix, uint32_t n_prefix, const uint32_t * d_ids_suffix,
                                         uint32_t n_suffix, int * has_duplicates) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_index_build_routed: no database"); }
  if (ctx->owner_world <= 1) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_index_build_routed: call swa_d1_set_ownership(rank, world > 1) first"); }
  if ((n_prefix != 0 && d_ids_prefix == nullptr) || (n_suffix != 0 && d_ids_suffix == nullptr)) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_index_build_routed: null list"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(ensure_db_lengths(ctx));
  static const uint32_t nothing = 0;                         // (an empty list still marks the build as routed)
  RouteLists route;
  route.ids[0] = n_prefix != 0 ? d_ids_prefix : &nothing; route.m[0] = n_prefix;
  route.ids[1] = n_suffix != 0 ? d_ids_suffix : &nothing; route.m[1] = n_suffix;
  return index_build(ctx, 0, ctx->db.n, route, has_duplicates);
}

// The same exchange with the KEY RECORDS travelling (d1_stream.inc: k_anchor_route_records): 8 bytes per amplicon and index;
// the owner's build starts at the partition.
extern "C" int swa_d1_route_slice_records(swa_ctx * ctx, uint32_t first, uint32_t count, uint32_t world, uint64_t * d_records, uint64_t cap,
                                          uint32_t * d_counts) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_route_slice_records: no database"); }
  if (first > ctx->db.n || count > ctx->db.n - first) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_route_slice_records: bad range"); }
  if (world == 0 || world > kRouteMaxWorld || d_records == nullptr || d_counts == nullptr || cap == 0) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_route_slice_records: bad argument (1..64 ranks)");
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(ensure_anchor_windows(ctx));
  SWA_HIP(ctx, hipMemsetAsync(d_counts, 0, (2ull * world + 1) * sizeof(uint32_t), ctx->stream));
  if (count != 0) {
    hipLaunchKernelGGL(k_anchor_route_records, dim3(swa_grid_for(ctx, (count + 3) / 4, 256, 8)), dim3(256), 0, ctx->stream,
                       ctx->db.seqs, ctx->db.seq_off, ctx->db.seqlen, first, count, world, ctx->ix.anchor_a, ctx->ix.anchor_b, ctx->ix.anchor_w / 32u,
                       reinterpret_cast<unsigned long long *>(d_records), cap, d_counts);
  }
  SWA_HIP(ctx, hipGetLastError());
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));           // (the caller reads the counts next, maybe from another stream)
  return SWA_OK;
}

extern "C" int swa_d1_index_build_records(swa_ctx * ctx, const uint64_t * d_rec_prefix, uint32_t n_prefix, const uint64_t * d_rec_suffix, uint32_t n_suffix,
                                          int * has_duplicates) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (ctx->db.n == 0) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_index_build_records: no database"); }
  if (ctx->owner_world <= 1) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_index_build_records: call swa_d1_set_ownership(rank, world > 1) first"); }
  if ((n_prefix != 0 && d_rec_prefix == nullptr) || (n_suffix != 0 && d_rec_suffix == nullptr)) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_index_build_records: null list");
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_TRY(ensure_db_lengths(ctx));
  static const unsigned long long nothing = 0;               // (an empty list still marks the build as routed)
  RouteLists route;
  route.rec[0] = n_prefix != 0 ? reinterpret_cast<const unsigned long long *>(d_rec_prefix) : &nothing; route.m[0] = n_prefix;
  route.rec[1] = n_suffix != 0 ? reinterpret_cast<const unsigned long long *>(d_rec_suffix) : &nothing; route.m[1] = n_suffix;
  return index_build(ctx, 0, ctx->db.n, route, has_duplicates);
}

extern "C" int swa_d1_set_ownership(swa_ctx * ctx, uint32_t rank, uint32_t world) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (world == 0 || rank >= world) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_set_ownership: bad rank / world"); }
  if (rank != ctx->owner_rank || world != ctx->owner_world) {
    ctx->owner_rank = rank;
    ctx->owner_world = world;
    ctx->ix.owner_changed();                                 // the next network call indexes this rank's groups
    ctx->res = {};
  }
  return SWA_OK;
}

extern "C" int swa_d1_network(swa_ctx * ctx, int no_cluster_breaking, uint32_t first, uint32_t count,
                              uint64_t * offsets, uint32_t * neighbours, uint64_t cap, uint64_t * total) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (offsets == nullptr || total == nullptr) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_network: null buffer"); }
  ctx->res.csr_ready = false;                                   // (d_offsets_tmp / d_nb_tmp are about to hold this call's rows)
  SWA_TRY(swa_reserve(ctx, ctx->d_offsets_tmp, (uint64_t(count) + 1) * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_nb_tmp, (cap > 0 ? cap : 1) * sizeof(uint32_t)));
  const int rc = swa_d1_network_device(ctx, no_cluster_breaking, first, count,
                                       static_cast<uint64_t *>(ctx->d_offsets_tmp.ptr),
                                       static_cast<uint32_t *>(ctx->d_nb_tmp.ptr), cap, total);
  if (rc != SWA_OK && rc != SWA_E_CAPACITY) { return rc; }
  swa_touch_pages(offsets, (uint64_t(count) + 1) * sizeof(uint64_t));
  if (rc == SWA_OK) { swa_touch_pages(neighbours, *total * sizeof(uint32_t)); }
  SWA_HIP(ctx, hipMemcpyAsync(offsets, ctx->d_offsets_tmp.ptr, (uint64_t(count) + 1) * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, ctx->stream));
  if (rc == SWA_OK && *total > 0) {
    SWA_HIP(ctx, hipMemcpyAsync(neighbours, ctx->d_nb_tmp.ptr, *total * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                ctx->stream));
  }
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return rc;
}

extern "C" int swa_d1_debug_read(swa_ctx * ctx, int what, void * out, size_t out_bytes) {
  if (ctx == nullptr || out == nullptr) { return SWA_E_ARG; }
  if (!ctx->ix.d1_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_debug_read: no index"); }
  if (what >= 10) {
    // the streaming index as it lies in HBM (tools/check_stream.py validates it on the host): 10 + i: ids in group order of
    // index i, u32[n] · 12 + i: its item buffer, swa_item[regions' end] · 14: the counters, u32[kCounterWords] · 15: the amplicon lines,
    // lines_quads x 16 bytes each · 16: u64[kWidthClasses][kListKinds + 1] first items of the lists (ListRegions) + [.][0] = line quads behind
    if (!ctx->ix.stream_index) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_debug_read: no streaming index in place"); }
    const void * from = nullptr;
    size_t need = 0;
    if (what == 10 || what == 11) { from = ctx->d_stream[kSbMembers + (what - 10)].ptr; need = uint64_t(ctx->db.n) * sizeof(uint32_t); }
    else if (what == 12 || what == 13) { from = ctx->d_aitems[what - 12].ptr; need = ctx->ix.list_regions_items * sizeof(swa_item); }
    else if (what == 14) { from = swa_status(ctx)->counters; need = kCounterWords * sizeof(uint32_t); }
    else if (what == 15) { from = ctx->d_stream[kSbLines].ptr; need = uint64_t(ctx->db.n) * ctx->up.d1.lines_quads * 16u; }
    else if (what == 17 || what == 18) {
      // the bucket starts of the key partition, u64[buckets + 1]: as the index build left them — a network call sorts its
      // links in the same scratch, so they are there between the build and the first network call only
      if (!ctx->ix.part_starts_valid) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_debug_read: the bucket starts are there only between the index build and the next network call"); }
      const swa_dbuf & b = ctx->d_stream[kSbStart + (what - 17)];
      need = ((uint64_t)ctx->ix.part_buckets + 1) * sizeof(uint64_t);
      if (b.ptr == nullptr || (ctx->ix.part_starts_at + ctx->ix.part_buckets + 1) * sizeof(uint64_t) > b.bytes) { return swa_fail_msg(ctx, SWA_E_INTERNAL, "swa_d1_debug_read: bucket starts outside their buffer"); }
      from = static_cast<const uint64_t *>(b.ptr) + ctx->ix.part_starts_at;
    }
    else if (what == 16) {                                    // (host-side facts: where the lists lie, how wide a line is)
      uint64_t total = 0;
      const ListRegions r = list_regions(ctx, &total);
      const size_t bytes = sizeof(r) + 2 * sizeof(uint64_t);
      if (out_bytes < bytes) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_debug_read: buffer too small"); }
      memcpy(out, &r, sizeof(r));
      const uint64_t tail[2] = {total, ctx->up.d1.lines_quads};
      memcpy(static_cast<char *>(out) + sizeof(r), tail, sizeof(tail));
      return SWA_OK;
    }
    else { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_debug_read: unknown selector"); }
    if (out_bytes < need) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_debug_read: buffer too small"); }
    SWA_HIP(ctx, hipSetDevice(ctx->device));
    SWA_HIP(ctx, hipMemcpyAsync(out, from, need, hipMemcpyDeviceToHost, ctx->stream));
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWA_OK;
  }
  if (what == 4 || what == 5) {
    // host-side facts of the uploaded database, copied as they stand (no kernel, no index touched).  4: u32[8] = the shortest
    // sequence, the populations of the width classes [0 .. kWidthClasses] (the last: beyond the pair kernels), SWA_MAX_ZOBRIST_LDS
    // of this build, 0 (ensure_db_lengths).  5: u32[16] = the window sample choose_anchor_windows drew for this upload:
    // too short [4], stranded mass [4] per candidate offset 0 / 32 / 64 / 96, stride, samples, the offset and the width chosen
    // from the sample (the safety net of the first build may since have moved swa_d1_anchor_windows), 1 if a sample was drawn
    // (0 under SWA_D1_WINDOWS=0: the words before it are 0 then), 0, 0, 0
    const swa_db_facts::d1_facts & facts = ctx->up.d1;
    uint32_t words[16] = {};
    size_t bytes = 0;
    if (what == 4) {
      if (!facts.props_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_debug_read: the lengths of this database were never read"); }
      words[0] = facts.db_shortest;
      for (uint32_t c = 0; c <= kWidthClasses; ++c) { words[1 + c] = facts.class_pop[c]; }
      words[2 + kWidthClasses] = SWA_MAX_ZOBRIST_LDS;
      bytes = 8 * sizeof(uint32_t);
    } else {
      if (!facts.windows_ready) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_debug_read: no anchor windows were chosen for this database"); }
      memcpy(words, facts.sample_stats, sizeof(facts.sample_stats));
      words[8] = facts.sample_stride; words[9] = facts.sample_count;
      words[10] = facts.sample_offset; words[11] = facts.sample_w;
      words[12] = facts.sample_taken ? 1u : 0u;
      bytes = 16 * sizeof(uint32_t);
    }
    if (out_bytes < bytes) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_debug_read: buffer too small"); }
    memcpy(out, words, bytes);
    return SWA_OK;
  }
  SWA_TRY(swa_ensure_full_index(ctx));
  const void * src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case 0: src = ctx->d_seqhash.ptr; bytes = uint64_t(ctx->db.n) * sizeof(uint64_t); break;
    case 1: src = ctx->d_bloom.ptr; bytes = ctx->ix.bloom_words * sizeof(uint64_t); break;
    case 2: src = ctx->d_zobrist.ptr; bytes = 4ull * ctx->zobrist_len * sizeof(uint64_t); break;
    case 3: src = ctx->d_aux.ptr; bytes = uint64_t(ctx->db.n) * sizeof(swa_aux); break;
    default: return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_debug_read: unknown selector");
  }
  if (out_bytes < bytes) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_debug_read: buffer too small"); }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_HIP(ctx, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWA_OK;
}

// How the work lists of the streaming index in place got their positions: 1 inside k_group_lists, 0 by the two-launch scan
// (swa_lists_inline); -1 without such an index
extern "C" int swa_d1_lists_form(const swa_ctx * ctx) {
  return ctx != nullptr && ctx->ix.stream_index && ctx->ix.anchor_ready ? ctx->ix.lists_form : -1;
}

// The key partition of the streaming index in place: the layout of swa_d1_part_plan_for, with the bits the key-overflow
// retry added in [7]
extern "C" int swa_d1_part_plan(const swa_ctx * ctx, uint32_t out[8]) {
  if (ctx == nullptr || out == nullptr) { return SWA_E_ARG; }
  if (!ctx->ix.d1_ready || !ctx->ix.stream_index) { return SWA_E_ARG; }
  memcpy(out, ctx->ix.part_plan, sizeof(ctx->ix.part_plan));
  return SWA_OK;
}
