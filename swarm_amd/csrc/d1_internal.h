// d1_internal.h — the seam between the d = 1 step (d1.hip: index build and network) and its partition unit (d1_part.hip:
// the partition engine and the rows built on it).  Constants, types, a __device__ __forceinline__ helper, inline host
// functions and declarations only: NO KERNEL is defined here or in anything else that more than one unit includes — every
// kernel lives in the code object of exactly one unit, and whatever takes a kernel's address (a launch, an occupancy query,
// a dynamic-LDS opt-in) is in that unit.  A type that crosses the seam is defined here, once, outside any anonymous namespace:
// in namespace swa_d1, which the two units open with a using-directive — no other unit's names can meet these.
#pragma once

#include "swa_internal.h"

namespace swa_d1 {

// ---- the partition's layout -----------------------------------------------------------------------------------------------
// k_keys<true> (d1_stream.inc) takes level 0's histogram of the key partition on its way and writes the flat counts and the
// tile table where k_part_scatter (d1_part.hip) reads them: what fixes that layout is here, for both.  The flat counts of a
// level lie (segment, digit, tile) — part_flat in d1_part.hip; k_keys spells its one-chunk case, digit * tiles + tile —,
// tiles are dealt to the XCDs by xcd_tile, and a chunk's tile table is first tile | tiles | the scan's closing entry.
constexpr uint32_t kPartTileMax = 4096;           // records per tile of k_part_hist (PartArgs::tile: 2048 or 4096; the one-level key
                                                  // partition scatters tiles of 8192, its histogram taken by k_keys)
constexpr uint32_t kPartMaxBits = SWA_PART_MAX_BITS;              // bits per level (512 bins) — 10 for the one-level key partition in front of k_group1;
                                                  // 2048 bins were tried: the flat count array — bins x tiles — grows with them and costs more than a level
constexpr unsigned long long kRecAbsent = ~0ull;  // a record slot that holds nothing (amplicon without this window / not owned)
constexpr uint32_t kMaxIdx = 2;                   // indexes handled per launch (blockIdx.y)
constexpr uint32_t kFlatChunk = 4096;             // entries of a flat array a workgroup of k_flat_sums / k_flat_apply scans at a time
constexpr uint32_t kRouteMaxWorld = 64;            // ranks of a multi-GPU job (k_anchor_route*, k_links_split)

// Which tile a workgroup takes in turn `v` (v = blockIdx.x + k * gridDim.x).  Workgroups go to the 8 XCDs round-robin, and
// every XCD has its own L2.  Tiles t .. t + 15 of one digit are neighbours everywhere — their counts share a 64-byte line
// of the flat array, their output runs are adjacent in the bucket — so runs of 2^run_bits consecutive tiles (16) are given to ONE XCD
// (the workgroups v, v + 8, .. v + 120): its L2 then merges their partial writes into whole lines, and fetches a line of
// counts once instead of once per XCD.  v runs to the tile count rounded up to 128; tiles beyond the end do not exist.
__device__ __forceinline__ uint32_t xcd_tile(uint32_t v, uint32_t run_bits) {
  const uint32_t xcd = v & 7u, w = v >> 3;
  return ((((w >> run_bits) << 3) + xcd) << run_bits) + (w & ((1u << run_bits) - 1u));
}

// ---- types that cross the seam --------------------------------------------------------------------------------------------
// what the first level of a network call's link partition makes of the per-wave segments on its way (k_part_tiles<., true>)
struct SegArgs {
  const uint32_t * staged;           // [2][chunks] members the pair kernels staged, per pass (behind the fills)
  unsigned long long * out;          // the status block's stats + kStatSeg: kSegLinks, kSegFullest, kSegStaged + pass
  const uint32_t * fallback;         // the status block's counters + kCounterFallback ...
  uint32_t * fallback_copy;          // ... and where the head of the block carries it to the host
};

// an exclusive scan of flat u32 arrays in place (swa_flat_scan)
// length of array i: (*units[i] << unit_bits) + 1 (the flat counts of a partition level: tiles << bits, + the closing entry),
// or fixed[i] when units[i] == nullptr
struct FlatScanArgs { uint32_t * v[kMaxIdx]; const uint32_t * units[kMaxIdx]; uint32_t unit_bits; uint64_t fixed[kMaxIdx]; uint32_t * partial[kMaxIdx]; uint32_t * total[kMaxIdx]; };

using PartPlan = swa_part_levels;                  // (host_tables.cpp: swa_plan_levels, swa_part_plan_for, swa_csr_plan_for)

// One multi-level partition (d1_part.hip: swa_part_run) over up to kMaxIdx record sets.  Level l reads what level l - 1 wrote
// (ping / pong) and leaves, in starts[], the first record of every bucket; the last level's buckets are the result.
struct PartJob {
  uint32_t nidx = 1;
  const unsigned long long * in[kMaxIdx] = {};      // level-0 input (may be buf[i][1])
  unsigned long long * buf[kMaxIdx][2] = {};
  const uint64_t * cstart0[kMaxIdx] = {};           // level-0 chunks (nullptr: regular, PartIdx::cstride)
  uint64_t cstride0[kMaxIdx] = {};
  const uint32_t * csize0[kMaxIdx] = {};
  uint32_t csize_cap = 0, chunks0 = 1;
  bool single0 = true;
  uint64_t max_records = 0, max_tiles0 = 0;         // host-side upper bounds (per set)
  uint64_t out_cap = 0;                             // entries every buf[][] holds
  uint32_t bias = 0, top_bit = 32;
  uint32_t tile = 4096;                             // records per tile: 4096 (links), 2048 / 4096 / 8192 (key records: swa_part_run)
  bool hist0_done = false;                          // the flat counts of level 0 are there already (k_keys<W, true>)
  bool tiles0_done = false;                         // ... and its tile table (one chunk of a size the host knows)
  const SegArgs * seg = nullptr;                    // level 0's chunks are the per-wave link segments: k_part_tiles reduces their fills on the way
  PartPlan plan{};
  // scratch, per set
  uint32_t * cnt[kMaxIdx] = {}; uint32_t * ctile[kMaxIdx] = {}; uint64_t * starts[kMaxIdx] = {}; uint32_t * partial[kMaxIdx] = {};
  uint32_t * total[kMaxIdx] = {};
  uint64_t starts_stride = 0;
  // results
  const unsigned long long * out[kMaxIdx] = {}; const uint64_t * bstart[kMaxIdx] = {};
  uint32_t buckets = 0;
  int last = 0;                                     // buf[i][last] holds the result, buf[i][last ^ 1] is free
};

// several small buffers zeroed by ONE launch (a step clears about ten; each hipMemsetAsync is a launch of 4-5 us)
struct ClearList { uint32_t * p[8]; uint64_t words[8]; uint32_t n; };
inline void clear_add(ClearList & c, void * p, uint64_t bytes) {          // (bytes: a multiple of 4)
  c.p[c.n] = static_cast<uint32_t *>(p); c.words[c.n] = bytes / 4; ++c.n;
}

// the list of the buckets k_csr_bucket leaves to whole workgroups, its count in front: a word per bucket of the CSR over `count` sources
inline uint64_t csr_heavy_bytes(uint32_t count) { return ((1ull << swa_csr_plan_for(count).lv.total) + 2) * sizeof(uint32_t); }

}  // namespace swa_d1

// ---- d1_part.hip: the partition engine, the flat scan, the clears, the rows -------------------------------------------------
// All enqueue on ctx->stream and return SWA_OK or the error they recorded.
void swa_part_scratch(const swa_d1::PartJob & j, uint64_t * cnt, uint64_t * ctile, uint64_t * starts_half, uint64_t * partial);   // entries of a job's scratch arrays, per set
int swa_part_run(swa_ctx * ctx, swa_d1::PartJob & j);                                  // every level of the job; fills its results
void swa_flat_scan(swa_ctx * ctx, dim3 grid, const swa_d1::FlatScanArgs & f);          // k_flat_sums, k_flat_apply over grid.y arrays
int swa_clear_launch(swa_ctx * ctx, const swa_d1::ClearList & c);                      // the list's buffers zeroed by one launch (none when empty)
// the CSR of [first, first + count) from the per-wave link segments: link partition, then the row kernels.  heavy_cleared: the
// caller has zeroed the word in front of d_stream[kSbHeavy] with its own clears (launch_network_anchored does, having
// reserved the buffer at csr_heavy_bytes(count)) — else, or when the buffer grew since, it is zeroed here
int swa_d1_csr_stream(swa_ctx * ctx, uint32_t first, uint32_t count, uint32_t nseg, uint64_t link_cap, uint64_t * d_offsets,
                      uint32_t * d_neighbours, uint64_t cap, bool heavy_cleared);
// the per-wave link segments as one flat list of at most cap links in d_edge_list: k_seg_reduce, k_seg_bases, k_seg_compact
int swa_d1_seg_compact(swa_ctx * ctx, uint32_t nseg, uint64_t * d_edge_list, uint64_t cap);
