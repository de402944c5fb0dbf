// d1_part.hip — the partition engine of the d = 1 step and what is built on it, a translation unit and a code object of
// its own.
//
// In this unit: the segmented radix partition (k_part_tiles / k_part_hist / k_flat_sums + k_flat_apply / k_part_scatter) that
// sorts the key records of the index build and the links of a network call; the CSR rows made of the partitioned links
// (k_csr_bucket, k_csr_bucket_big); the per-wave link segments reduced and compacted into a flat list (k_seg_*); the link
// exchange of a multi-GPU job (k_links_split, swa_d1_csr_from_lists); the exclusive scan of the --fastidious groups
// (swa_scan_offsets) and the one-launch clear of several small buffers (k_clear_many).  d1.hip calls it through the six
// functions of d1_internal.h; the layout k_keys<true> shares with k_part_scatter is fixed there too.
#include "d1_internal.h"
using namespace swa_d1;

#include <algorithm>
#include <type_traits>   // (std::conditional: k_part_hist, k_part_scatter)

namespace {

#include "wave_ops.inc"     // wave_lds_sync
#include "key_ops.inc"      // (mix64, window32: d1_common.inc)
#include "d1_common.inc"    // lane_value

// ---- exclusive scans (a workgroup's: the flat scan and k_csr_bucket_big too; the fastidious pass's offsets), the per-wave segments' totals and flat list ------
constexpr int kScanItems = 8;
constexpr int kScanBlock = 256;
constexpr int kScanTile = kScanItems * kScanBlock;

__device__ __forceinline__ uint64_t block_exclusive_scan(uint64_t v, uint64_t * smem, uint64_t & total) {
  // v: per-thread value; returns exclusive prefix within the block (256 threads)
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  uint64_t incl = v;
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) {
    const uint64_t t = swa_shfl_up_u64(incl, d);
    if (lane >= (int)d) { incl += t; }
  }
  if (lane == 63) { smem[wave] = incl; }
  __syncthreads();
  uint64_t wave_off = 0;
  uint64_t tot = 0;
  for (int w = 0; w < kScanBlock / 64; ++w) {
    if (w < wave) { wave_off += smem[w]; }
    tot += smem[w];
  }
  __syncthreads();
  total = tot;
  return wave_off + incl - v;
}

// swa_scan_offsets (the fastidious groups' member offsets): exclusive scan of counts[0, n) into 64-bit offsets[0, n], three launches
__global__ __launch_bounds__(kScanBlock) void k_scan_tiles(const uint32_t * __restrict__ counts, uint32_t n,
                                                           uint64_t * __restrict__ tile_sums) {
  __shared__ uint64_t smem[4];
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
  uint64_t v = 0;
  for (int i = 0; i < kScanItems; ++i) { if (base + i < n) { v += counts[base + i]; } }
  uint64_t total;
  (void)block_exclusive_scan(v, smem, total);
  if (threadIdx.x == 0) { tile_sums[blockIdx.x] = total; }
}

__global__ __launch_bounds__(kScanBlock) void k_scan_sums(uint64_t * tile_sums, uint32_t tiles) {
  __shared__ uint64_t smem[4];
  uint64_t carry = 0;
  for (uint32_t base = 0; base < tiles; base += kScanBlock) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t v = (i < tiles) ? tile_sums[i] : 0;
    uint64_t total;
    const uint64_t ex = block_exclusive_scan(v, smem, total);
    if (i < tiles) { tile_sums[i] = carry + ex; }
    carry += total;
  }
}

__global__ __launch_bounds__(kScanBlock) void k_scan_apply(const uint32_t * __restrict__ counts, uint32_t n,
                                                           const uint64_t * __restrict__ tile_sums,
                                                           uint64_t * __restrict__ offsets) {
  __shared__ uint64_t smem[4];
  const uint32_t base = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
  uint32_t c[kScanItems];
  uint64_t v = 0;
  for (int i = 0; i < kScanItems; ++i) {
    c[i] = (base + i < n) ? counts[base + i] : 0u;
    v += c[i];
  }
  uint64_t total;
  uint64_t run = tile_sums[blockIdx.x] + block_exclusive_scan(v, smem, total);
  for (int i = 0; i < kScanItems; ++i) {
    if (base + i < n) { offsets[base + i] = run; }
    run += c[i];
    if (base + i + 1 == n) { offsets[n] = run; }
  }
}

// total and largest fill of the per-wave edge segments -> out[0], out[1]; the members the pair kernels staged (the
// guard; seg_fill + nseg, + 2 nseg: pass 0, pass 1) -> out[2], out[3]
// (one workgroup of 1024 threads, eight loads in flight per thread: the 8192 fills of an MI355X in one round — with 256
// threads and a load per turn this single workgroup took 11 us of every step)
// ... and the count of fallback seeds next to them in the head of the status block (fallback_copy: the host's one copy).
// The CSR route takes all of this in the first k_part_tiles of its link partition (SegArgs); this kernel
// serves the edge-list route.
__global__ __launch_bounds__(1024) void k_seg_reduce(const uint32_t * __restrict__ seg_fill, uint32_t nseg,
                                                     unsigned long long * out, const uint32_t * fallback, uint32_t * fallback_copy) {
  __shared__ unsigned long long ssum[16], smax[16], sst0[16], sst1[16];
  unsigned long long sum = 0, mx = 0, st0 = 0, st1 = 0;
  for (uint32_t base = 0; base < nseg; base += 8192u) {
    uint32_t v[8], s0[8], s1[8];
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
      const uint32_t i = base + k * 1024u + threadIdx.x;
      v[k] = i < nseg ? seg_fill[i] : 0u;
      s0[k] = i < nseg ? seg_fill[(uint64_t)nseg + i] : 0u;
      s1[k] = i < nseg ? seg_fill[2ull * nseg + i] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) { sum += v[k]; mx = mx > v[k] ? mx : v[k]; st0 += s0[k]; st1 += s1[k]; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long s2 = swa_shfl_xor_u64(sum, o), m2 = swa_shfl_xor_u64(mx, o);
    sum += s2; mx = mx > m2 ? mx : m2;
    st0 += swa_shfl_xor_u64(st0, o); st1 += swa_shfl_xor_u64(st1, o);
  }
  if ((threadIdx.x & 63u) == 0u) { ssum[threadIdx.x >> 6] = sum; smax[threadIdx.x >> 6] = mx; sst0[threadIdx.x >> 6] = st0; sst1[threadIdx.x >> 6] = st1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0, m = 0, a0 = 0, a1 = 0;
    for (int w = 0; w < 16; ++w) { s += ssum[w]; m = m > smax[w] ? m : smax[w]; a0 += sst0[w]; a1 += sst1[w]; }
    out[0] = s; out[1] = m; out[2] = a0; out[3] = a1;
    *fallback_copy = *fallback;
  }
}

// start of every segment in the compacted edge list: exclusive prefix sum of the fills
__global__ __launch_bounds__(256) void k_seg_bases(const uint32_t * __restrict__ seg_fill, uint32_t nseg,
                                                   unsigned long long * __restrict__ bases) {
  __shared__ unsigned long long part[256];
  const uint32_t chunk = (nseg + 255u) / 256u;
  const uint32_t lo = threadIdx.x * chunk, hi = min(nseg, lo + chunk);
  unsigned long long sum = 0;
  for (uint32_t i = lo; i < hi; ++i) { sum += seg_fill[i]; }
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int t = 0; t < 256; ++t) { const unsigned long long v = part[t]; part[t] = run; run += v; }
  }
  __syncthreads();
  unsigned long long at = part[threadIdx.x];
  for (uint32_t i = lo; i < hi; ++i) { bases[i] = at; at += seg_fill[i]; }
}

// per-wave segments -> one flat list of (source << 32 | target) links, in no particular order
__global__ __launch_bounds__(256) void k_seg_compact(const uint64_t * __restrict__ edges,
                                                     const uint32_t * __restrict__ seg_fill, uint32_t nseg, uint64_t seg_cap,
                                                     const unsigned long long * __restrict__ bases,
                                                     uint64_t * __restrict__ out, uint64_t cap) {
  for (uint32_t s = blockIdx.x; s < nseg; s += gridDim.x) {
    const uint64_t fill = min((uint64_t)seg_fill[s], seg_cap);
    const uint64_t base = bases[s];
    for (uint64_t i = threadIdx.x; i < fill; i += blockDim.x) {
      if (base + i < cap) { out[base + i] = edges[(uint64_t)s * seg_cap + i]; }
    }
  }
}

// ---- link exchange of a multi-GPU job: a rank's flat link list split by the rank that owns each source -----------------------
// (swa_d1_links_split.)  The owners' ranges are contiguous but arbitrary (sharding.partition_by_length), so the destination
// of a link is found by a binary search of its source in the ranges' first ids, kept in LDS: six steps for up to 64 ranks —
// where a 64-bit sort of the whole list used to make the destinations contiguous.  Two launches over tiles of 4096 links,
// a lane reading two links at a time (16 bytes):
//   <false>  counts: a histogram per workgroup in LDS over all its tiles, then ONE global atomic per destination it met;
//   <true>   places: every workgroup turns the counts into the runs' first places (a scan over at most 64 values by one
//            wave), and per tile: histogram in LDS whose atomic returns the link's rank among the tile's links of its
//            destination, one global atomic per destination the tile met to reserve room in that run, the tile's links put
//            in destination order in LDS and written as one contiguous piece per destination.
// No global atomic per link.  A source >= bounds[world] is counted in counts[world] and written nowhere.
struct SplitArgs {
  const unsigned long long * links;  // 16-byte aligned: the caller's list begins `head` (0 or 1) entries behind it
  uint32_t head;
  uint64_t end;                      // head + links in the list
  uint32_t world;
  uint32_t bounds[kRouteMaxWorld + 1];   // rank r owns the sources [bounds[r], bounds[r + 1]); bounds[0] = 0
  unsigned long long * counts;       // [world + 1] links per destination; [world]: sources beyond the last range
  unsigned long long * cursor;       // [world] (places) links of every run that have their place so far
  unsigned long long * out;          // [links]
};
constexpr uint32_t kSplitTile = 4096, kSplitThreads = 512;
constexpr uint32_t kSplitPairs = kSplitTile / (2u * kSplitThreads);          // pairs of links a lane takes from a tile

// the r with sb[r] <= src < sb[r + 1] (sb: the ranges' first ids, 0xFFFFFFFF behind the last rank; of equal ones — ranks that
// own nothing — the last, whose range is the one that is not empty); `world` when no rank owns src
__device__ __forceinline__ uint32_t split_dest(const uint32_t * sb, uint32_t beyond, uint32_t world, uint32_t src) {
  if (src >= beyond) { return world; }
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t step = kRouteMaxWorld / 2u; step != 0u; step >>= 1) { if (sb[pos + step] <= src) { pos += step; } }
  return pos;
}

template <bool PLACE>
__global__ __launch_bounds__(kSplitThreads) void k_links_split(const SplitArgs a) {
  __shared__ uint32_t sb[kRouteMaxWorld], hist[kRouteMaxWorld + 1], lstart[kRouteMaxWorld];
  __shared__ unsigned long long gbase[kRouteMaxWorld];
  __shared__ uint32_t present;
  __shared__ __attribute__((aligned(16))) unsigned long long stage[PLACE ? kSplitTile : 1];
  const uint32_t tid = threadIdx.x, world = a.world, beyond = a.bounds[world];
  if (tid < kRouteMaxWorld) { sb[tid] = tid < world ? a.bounds[tid] : 0xFFFFFFFFu; }
  if (tid <= kRouteMaxWorld) { hist[tid] = 0u; }
  // (places) first place of run `tid`: the counts before it — lane d of the first wave keeps it
  unsigned long long run_start = 0ull;
  if (PLACE && tid < 64u) {
    const unsigned long long mine = tid < world ? a.counts[tid] : 0ull;
    unsigned long long incl = mine;
#pragma unroll
    for (unsigned d = 1; d < 64; d <<= 1) { const unsigned long long up = swa_shfl_up_u64(incl, d); if (tid >= d) { incl += up; } }
    run_start = incl - mine;
  }
  __syncthreads();
  const uint64_t links = a.end - a.head;
  const uint64_t tiles = (a.end + kSplitTile - 1u) / kSplitTile;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    // the tile's links: pair k of the lane = entries j, j + 1 behind the aligned pointer, j even (one 16-byte load when both
    // belong to the list; the list's first or last entry alone is read alone: nothing outside the list is touched)
    unsigned long long rec[2u * kSplitPairs];
    uint32_t valid = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kSplitPairs; ++k) {
      const uint64_t j = t * kSplitTile + (uint64_t)k * (2u * kSplitThreads) + 2u * tid;
      const bool v0 = j >= a.head && j < a.end, v1 = j + 1u < a.end;   // (j + 1 >= 1 >= head)
      rec[2u * k] = rec[2u * k + 1u] = 0ull;
      if (v0 && v1) {
        const uint4 q = *reinterpret_cast<const uint4 *>(a.links + j);
        rec[2u * k] = (unsigned long long)q.x | (unsigned long long)q.y << 32;
        rec[2u * k + 1u] = (unsigned long long)q.z | (unsigned long long)q.w << 32;
      } else if (v0) { rec[2u * k] = a.links[j]; }
      else if (v1) { rec[2u * k + 1u] = a.links[j + 1u]; }
      valid |= (v0 ? 1u : 0u) << (2u * k) | (v1 ? 1u : 0u) << (2u * k + 1u);
    }
    uint32_t pos[2u * kSplitPairs];                              // destination << 16 | rank among the tile's links for it
#pragma unroll
    for (uint32_t k = 0; k < 2u * kSplitPairs; ++k) {
      pos[k] = 0u;
      if ((valid >> k & 1u) != 0u) {
        const uint32_t d = split_dest(sb, beyond, world, (uint32_t)(rec[k] >> 32));
        pos[k] = d << 16 | atomicAdd(&hist[d], 1u);
        if (d == world) { valid &= ~(1u << k); }               // (counted, not placed)
      }
    }
    if (!PLACE) { continue; }                                    // (the histogram runs on over the workgroup's tiles)
    __syncthreads();
    if (tid < 64u) {
      // the tile's links per destination, where each destination's piece begins in the staging area, and the room
      // reserved for it in its run
      const uint32_t h = tid < world ? hist[tid] : 0u;
      uint32_t incl = h;
#pragma unroll
      for (unsigned d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64); if (tid >= d) { incl += up; } }
      lstart[tid] = incl - h;
      if (h != 0u) { gbase[tid] = run_start + atomicAdd(&a.cursor[tid], (unsigned long long)h); }
      if (tid == 63u) { present = incl; }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < 2u * kSplitPairs; ++k) {
      if ((valid >> k & 1u) != 0u) { stage[lstart[pos[k] >> 16] + (pos[k] & 0xFFFFu)] = rec[k]; }
    }
    __syncthreads();
    const uint32_t staged = present;
#pragma unroll
    for (uint32_t k = 0; k < kSplitTile / kSplitThreads; ++k) {
      const uint32_t j = k * kSplitThreads + tid;
      if (j < staged) {
        const unsigned long long r = stage[j];
        const uint32_t d = split_dest(sb, beyond, world, (uint32_t)(r >> 32));
        const uint64_t g = gbase[d] + (j - lstart[d]);
        if (g < links) { a.out[g] = r; }                       // (always, when the list is what the counting launch saw)
      }
    }
    if (tid <= kRouteMaxWorld) { hist[tid] = 0u; }
    __syncthreads();
  }
  if (!PLACE) {
    __syncthreads();
    if (tid <= world && hist[tid] != 0u) { atomicAdd(&a.counts[tid], (unsigned long long)hist[tid]); }
  }
}

// ---- segmented radix partition ------------------------------------------------------------------------------------
// One level: the records of every input chunk are grouped by a digit of their key (high 32 bits), chunk by chunk
// (a chunk = a bucket of the level before; the first level has one chunk, or — the links — the per-wave segments
// of the pair kernels, which all feed ONE bucket space: single_seg).  Counting sort in three steps: per tile
// (4096 records) a histogram of the digit into a flat array ordered (segment, digit, tile) — so that ONE exclusive
// scan over the flat array yields every tile's first output position for every digit; then the scatter, staged
// through LDS so that a tile's records for one digit leave as one contiguous run.
struct PartIdx {
  const unsigned long long * in;
  unsigned long long * out;
  uint64_t out_cap;                  // entries the output buffers hold (writes beyond are dropped: the caller grows and repeats)
  const uint64_t * cstart;           // [chunks + 1] first record of chunk c (or [chunks] when csize is given); nullptr: chunk c
  uint64_t cstride;                  // ... begins at c * cstride (the per-wave link segments; with csize), or — ONE chunk, no csize — is [0, cstride)
  const uint32_t * csize;            // nullptr: cstart[c + 1] - cstart[c]
  uint32_t csize_cap;                // (csize given) sizes are clamped to this: a wave segment may have overflowed
  uint32_t chunks;
  uint32_t * ctile;                  // [chunks + 1] first tile of chunk c; [chunks] = tiles in all
  uint32_t * tchunk;                 // [tchunk_cap] the chunk of tile t, where k_part_tiles wrote it (a hint: checked by its readers)
  uint32_t tchunk_cap;
  uint32_t * cnt;                    // flat counts -> offsets [bins * max_tiles + 1]
  uint64_t * next_start;             // out: [out_buckets + 1] chunk starts of the next level / of the consumer
  uint32_t * total;                  // out: records in all (after the scan)
};
struct PartArgs {
  PartIdx p[kMaxIdx];
  uint32_t single_seg;               // all chunks feed one bucket space
  uint32_t shift, bits;              // digit = ((high half - bias) >> shift) & (2^bits - 1)
  uint32_t bias;
  uint32_t tile;                     // records per tile (a multiple of 256, at most kPartTileMax)
  uint32_t run_bits;                 // xcd_tile: 2^run_bits consecutive tiles per XCD
  uint32_t span;                     // (single_seg) tiles are cut from the chunks laid end to end, not chunk by chunk: see part_span
};

__device__ __forceinline__ uint32_t part_chunk_size(const PartIdx & p, uint32_t c) {
  if (p.csize != nullptr) { return min(p.csize[c], p.csize_cap); }
  return p.cstart != nullptr ? (uint32_t)(p.cstart[c + 1] - p.cstart[c]) : (uint32_t)p.cstride;
}

// exclusive scan over the THREADS threads of a workgroup
template <uint32_t THREADS>
__device__ __forceinline__ uint64_t block_exclusive_scan_of(uint64_t v, uint64_t * smem, uint64_t & total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t incl = v;
#pragma unroll
  for (unsigned d = 1; d < 64; d <<= 1) { const uint64_t t = swa_shfl_up_u64(incl, d); if (lane >= d) { incl += t; } }
  if (lane == 63u) { smem[wave] = incl; }
  __syncthreads();
  uint64_t wave_off = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < THREADS / 64u; ++w) { const uint64_t x = smem[w]; wave_off += w < wave ? x : 0ull; tot += x; }
  __syncthreads();
  total = tot;
  return wave_off + incl - v;
}

// first tile of every chunk (one workgroup per index)
// (THREADS = 1024 for the thousands of link segments: one round of the scan instead of three dependent ones)
// SEG — the first level of the link partition of a network call, whose chunks are the per-wave segments of the pair kernels:
// the same pass over the segment fills yields what k_seg_reduce makes of them (links in all — the fills as they are, not
// clamped to a segment's capacity —, the fullest segment, the members staged per pass) and leaves, next to it in the head
// of the status block, the count of fallback seeds: one single-workgroup launch and one copy to the host instead of two each.
template <uint32_t THREADS, bool SEG = false>
__global__ __launch_bounds__(THREADS) void k_part_tiles(const PartArgs a, const SegArgs sg) {
  __shared__ uint64_t smem[THREADS / 64u];
  const PartIdx & p = a.p[blockIdx.y];
  uint64_t carry = 0;
  unsigned long long seg_sum = 0, seg_max = 0, seg_st0 = 0, seg_st1 = 0;
  const bool tile_pow2 = (a.tile & (a.tile - 1u)) == 0u;
  const uint32_t tile_shift = 31u - (uint32_t)__clz((int)a.tile);
  // (rounds of 8 THREADS chunks, eight per thread with their loads in flight together: the 8192 wave segments of the link
  // partition took 32 dependent rounds — 10 us of a single workgroup — with one chunk per thread)
  for (uint32_t base = 0; base < p.chunks; base += 8u * THREADS) {
    uint32_t v[8];
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
      const uint32_t c = base + threadIdx.x * 8u + k;
      if constexpr (SEG) {
        const uint32_t fill = c < p.chunks ? p.csize[c] : 0u, size = min(fill, p.csize_cap);
        v[k] = a.span != 0u ? size : (size + a.tile - 1u) / a.tile;
        seg_sum += fill; seg_max = seg_max > fill ? seg_max : fill;
        if (c < p.chunks) { seg_st0 += sg.staged[c]; seg_st1 += sg.staged[(uint64_t)p.chunks + c]; }
      } else {
        v[k] = c < p.chunks ? (a.span != 0u ? part_chunk_size(p, c) : (part_chunk_size(p, c) + a.tile - 1u) / a.tile) : 0u;
      }
    }
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) { mine += v[k]; }
    uint64_t total;
    uint64_t run = carry + block_exclusive_scan_of<THREADS>(mine, smem, total);
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
      const uint32_t c = base + threadIdx.x * 8u + k;
      if (c < p.chunks) {
        p.ctile[c] = (uint32_t)run;
        // the tiles that begin in this chunk name it (a spanning tile would find its chunks by two binary searches of one
        // thread — 13 dependent fetches each with the workgroup waiting).  A chunk of many tiles is left out: its tiles
        // search (the table is a hint; whoever reads it checks it).
        if (v[k] != 0u && a.span != 0u) {
          // (32-bit, and a shift for the tile sizes in use — powers of two: a 64-bit division is a subroutine here.  Only
          // the spanning level, whose chunks begin a tile or two each: this kernel is ONE workgroup, and the 8-tile
          // buckets of the later levels cost it more than their tiles' searches cost the others — 7 -> 18 us, measured)
          const uint32_t r32 = (uint32_t)run;
          const uint32_t first = tile_pow2 ? (r32 + a.tile - 1u) >> tile_shift : (r32 + a.tile - 1u) / a.tile;
          const uint32_t n = (tile_pow2 ? (r32 + v[k] + a.tile - 1u) >> tile_shift : (r32 + v[k] + a.tile - 1u) / a.tile) - first;
          if (n <= 4u) {
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) { if (i < n && first + i < p.tchunk_cap) { p.tchunk[first + i] = c; } }
          }
        }
      }
      run += v[k];
    }
    carry += total;
  }
  if (threadIdx.x == 0) {
    // (span: ctile[c] = RECORDS before chunk c; the closing entry is the number of tiles either way)
    if (a.span != 0u) { carry = ((uint32_t)carry + a.tile - 1u) / a.tile; }
    p.ctile[p.chunks] = (uint32_t)carry;
    p.cnt[carry << a.bits] = 0u;                              // the entry behind the last count: after the scan, the total
  }
  if constexpr (SEG) {
    __shared__ unsigned long long ssum[THREADS / 64u], smax[THREADS / 64u], sst0[THREADS / 64u], sst1[THREADS / 64u];
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long m2 = swa_shfl_xor_u64(seg_max, o);
      seg_sum += swa_shfl_xor_u64(seg_sum, o); seg_max = seg_max > m2 ? seg_max : m2;
      seg_st0 += swa_shfl_xor_u64(seg_st0, o); seg_st1 += swa_shfl_xor_u64(seg_st1, o);
    }
    if ((threadIdx.x & 63u) == 0u) { ssum[threadIdx.x >> 6] = seg_sum; smax[threadIdx.x >> 6] = seg_max; sst0[threadIdx.x >> 6] = seg_st0; sst1[threadIdx.x >> 6] = seg_st1; }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long s = 0, m = 0, a0 = 0, a1 = 0;
      for (uint32_t w = 0; w < THREADS / 64u; ++w) { s += ssum[w]; m = m > smax[w] ? m : smax[w]; a0 += sst0[w]; a1 += sst1[w]; }
      sg.out[0] = s; sg.out[1] = m; sg.out[2] = a0; sg.out[3] = a1;
      *sg.fallback_copy = *sg.fallback;
    }
  }
}

// chunk of tile t: the last c with ctile[c] <= t (chunks without records own no tile and are skipped)
__device__ __forceinline__ uint32_t part_chunk_of(const uint32_t * ctile, uint32_t chunks, uint32_t t) {
  uint32_t lo = 0, hi = chunks;                               // first index with ctile[index] > t, in (0, chunks]
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ctile[mid] <= t) { lo = mid + 1u; } else { hi = mid; } }
  return lo - 1u;
}

__device__ __forceinline__ uint64_t part_flat(const PartArgs & a, const PartIdx & p, uint32_t c, uint32_t t, uint32_t b) {
  if (a.single_seg != 0u) { return (uint64_t)b * p.ctile[p.chunks] + t; }
  const uint32_t t0 = p.ctile[c], nt = p.ctile[c + 1] - t0;
  return ((uint64_t)t0 << a.bits) + (uint64_t)b * nt + (t - t0);
}

struct PartTile { uint32_t c, count; uint64_t first; };

__device__ __forceinline__ PartTile part_tile(const PartIdx & p, uint32_t tile_records, uint32_t t, uint32_t * sh) {
  if (threadIdx.x == 0) {
    sh[0] = part_chunk_of(p.ctile, p.chunks, t);
  }
  __syncthreads();
  PartTile r;
  r.c = sh[0];
  const uint32_t within = (t - p.ctile[r.c]) * tile_records;
  r.first = (p.cstart != nullptr ? p.cstart[r.c] : (p.csize != nullptr ? (uint64_t)r.c * p.cstride : 0ull)) + within;
  r.count = min(tile_records, part_chunk_size(p, r.c) - within);
  return r;
}

// Spanning tiles (round 6; the first level of the link partition).  The per-wave link segments of the pair kernels hold
// ~3300 links each at 10 M amplicons — less than a tile, and close enough to one that a little more spread between the
// waves gives many of them a second, nearly empty tile (the level took 15 % longer behind pair kernels that ran 7 %
// faster).  With `span` a tile is 4096 consecutive records of the chunks laid end to end: ctile[c] holds the RECORDS
// before chunk c; a tile learns the chunk it begins in from the table k_part_tiles leaves (a hint it checks; a binary
// search by one thread otherwise), keeps the bounds of the up to four chunks it usually touches in every thread's
// registers, and — tiles over many small chunks: small inputs — looks its records up in rounds of kSpanRound bounds in
// LDS.  Same output order as chunk-by-chunk tiles: by position.
constexpr uint32_t kSpanFast = 4;        // chunks a tile usually touches at most: their bounds stay in registers
constexpr uint32_t kSpanRound = 256;     // otherwise: the bounds of this many chunks at a time in LDS
// before[i]: records before chunk i of the round (one more: the bound behind the round); shift[i] (the first kSpanFast chunks of
// the tile): what turns a position into a place in the input — first record of the chunk - records before it, modulo 2^64
// (1 KB: the scatter kernels keep their four workgroups a CU)
struct SpanLds { uint32_t c_lo, n, count, q0; uint64_t shift[kSpanFast]; uint32_t before[kSpanRound + 1]; };
__device__ __forceinline__ uint64_t part_chunk_base(const PartIdx & p, uint32_t c) {
  return p.cstart != nullptr ? p.cstart[c] : (p.csize != nullptr ? (uint64_t)c * p.cstride : 0ull);
}
// tile t of the chunks laid end to end: take(k, place) for every record k * THREADS + threadIdx.x of the thread inside the
// tile (k < PER), place = where it lies in the input; returns the tile's count.  All threads; barriers inside — the first
// covers what the caller cleared before.  (No array of places: the kernels' occupancy hangs on their registers.)
template <uint32_t PER, uint32_t THREADS, typename Take>
__device__ __forceinline__ uint32_t part_span(const PartIdx & p, uint32_t tile_records, uint32_t t, SpanLds & s, Take take) {
  if (threadIdx.x == 0) {
    const uint32_t last = p.chunks - 1u;
    const uint32_t total = p.ctile[last] + part_chunk_size(p, last);
    const uint32_t q0 = t * tile_records, q1 = min(q0 + tile_records, total) - 1u;       // (t < tiles: q0 < total)
    // the chunk that holds position q: the table's word for tile `tile` if it stands the test, a search otherwise
    const auto chunk_at = [&](uint32_t tile, uint32_t q) -> uint32_t {
      const uint32_t c = tile < p.tchunk_cap ? p.tchunk[tile] : 0xFFFFFFFFu;
      if (c < p.chunks && p.ctile[c] <= q && q < (c + 1u < p.chunks ? p.ctile[c + 1u] : total)) { return c; }
      return part_chunk_of(p.ctile, p.chunks, q);
    };
    const uint32_t c_lo = chunk_at(t, q0);
    // (the last chunk of the tile: no later than where the next tile begins)
    const uint32_t c_hi = q1 + 1u < total ? chunk_at(t + 1u, q1 + 1u) : part_chunk_of(p.ctile, p.chunks, q1);
    s.c_lo = c_lo; s.n = c_hi - c_lo + 1u; s.count = q1 - q0 + 1u; s.q0 = q0;
  }
  __syncthreads();
  const uint32_t n = s.n, count = s.count, q0 = s.q0, c_lo = s.c_lo;
  if (n <= kSpanFast) {
    // the usual tile: every thread keeps the bounds (a bound that is not there is never reached)
    if (threadIdx.x < n) {
      const uint32_t before = p.ctile[c_lo + threadIdx.x];
      s.before[threadIdx.x] = before;
      s.shift[threadIdx.x] = part_chunk_base(p, c_lo + threadIdx.x) - before;
    }
    __syncthreads();
    const uint32_t b1 = n > 1u ? s.before[1] : 0xFFFFFFFFu, b2 = n > 2u ? s.before[2] : 0xFFFFFFFFu, b3 = n > 3u ? s.before[3] : 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
      const uint32_t j = k * THREADS + threadIdx.x, q = q0 + j;
      // (bounds rise: the bounds at or below q are the first i of them — with chunks without records between, equal bounds,
      // that is the last chunk that starts at or below q: the one that has it.  Its shift comes from LDS: registers are
      // what the scatter kernel's four workgroups a CU hang on)
      const uint32_t i = (q >= b1 ? 1u : 0u) + (q >= b2 ? 1u : 0u) + (q >= b3 ? 1u : 0u);
      if (j < count) { take(k, s.shift[i] + q); }
    }
    return count;
  }
  // small segments (small inputs): rounds of kSpanRound chunks, every record looks itself up in the round that has it
  for (uint32_t r0 = 0; r0 < n; r0 += kSpanRound) {
    const uint32_t m = min(kSpanRound, n - r0);
    if (r0 != 0u) { __syncthreads(); }                           // (the round before is no longer read)
    for (uint32_t i = threadIdx.x; i <= m; i += THREADS) { s.before[i] = r0 + i < n ? p.ctile[c_lo + r0 + i] : 0xFFFFFFFFu; }
    __syncthreads();
    const uint32_t from = s.before[0], upto = s.before[m];
#pragma unroll
    for (uint32_t k = 0; k < PER; ++k) {
      const uint32_t j = k * THREADS + threadIdx.x, q = q0 + j;
      if (j < count && q >= from && q < upto) {
        uint32_t lo = 0, hi = m;                                 // first index with before[index] > q, in (0, m]
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (s.before[mid] <= q) { lo = mid + 1u; } else { hi = mid; } }
        take(k, part_chunk_base(p, c_lo + r0 + lo - 1u) + (q - s.before[lo - 1u]));
      }
    }
  }
  return count;
}

// SPAN: the tiles are cut from the chunks laid end to end (part_span; its own instantiation: the other keeps its registers)
template <uint32_t BINS, uint32_t TILE, uint32_t THREADS, bool SPAN = false>
__global__ __launch_bounds__(THREADS) void k_part_hist(const PartArgs a) {
  __shared__ uint32_t hist[BINS];
  __shared__ uint32_t sh[1];
  __shared__ typename std::conditional<SPAN, SpanLds, uint32_t>::type span;
  const PartIdx & p = a.p[blockIdx.y];
  const uint32_t bins = 1u << a.bits;
  const uint32_t ntiles = p.ctile[p.chunks];
  for (uint32_t v = blockIdx.x; v < ((ntiles + (8u << a.run_bits) - 1u) & ~((8u << a.run_bits) - 1u)); v += gridDim.x) {
    const uint32_t t = xcd_tile(v, a.run_bits);
    if (t >= ntiles) { continue; }
    for (uint32_t b = threadIdx.x; b < bins; b += THREADS) { hist[b] = 0u; }
    PartTile tile{0u, 0u, 0ull};
    const auto count_one = [&](unsigned long long r) {
      if (r != kRecAbsent) { atomicAdd(&hist[(((uint32_t)(r >> 32) - a.bias) >> a.shift) & (bins - 1u)], 1u); }
    };
    if constexpr (SPAN) {
      (void)part_span<TILE / THREADS, THREADS>(p, a.tile, t, span, [&](uint32_t, uint64_t place) { count_one(p.in[place]); });
    } else {
      tile = part_tile(p, a.tile, t, sh);                     // (its barrier covers hist[]; a.tile <= TILE)
#pragma unroll
      for (uint32_t k = 0; k < TILE / THREADS; ++k) {
        const uint32_t j = k * THREADS + threadIdx.x;
        if (j < tile.count) { count_one(p.in[tile.first + j]); }
      }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < bins; b += THREADS) { p.cnt[part_flat(a, p, tile.c, t, b)] = hist[b]; }
    __syncthreads();
  }
}

// exclusive scan of a flat u32 array in place, two launches: chunk sums, then every workgroup adds up the sums before
// its chunk (a few hundred values) and scans its chunk.  *total = sum of everything.
constexpr uint32_t kFlatPer = kFlatChunk / 256u;
__device__ __forceinline__ uint64_t flat_length(const FlatScanArgs & a, uint32_t i) {
  return a.units[i] != nullptr ? ((uint64_t)*a.units[i] << a.unit_bits) + 1u : a.fixed[i];
}

__global__ __launch_bounds__(256) void k_flat_sums(const FlatScanArgs a) {
  __shared__ uint64_t smem[4];
  const uint32_t * v = a.v[blockIdx.y];
  const uint64_t m = flat_length(a, blockIdx.y);
  for (uint64_t blk = blockIdx.x; blk * kFlatChunk < m; blk += gridDim.x) {
    const uint64_t base = blk * kFlatChunk + (uint64_t)threadIdx.x * kFlatPer;
    uint64_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kFlatPer; ++k) { if (base + k < m) { s += v[base + k]; } }
    uint64_t total;
    (void)block_exclusive_scan(s, smem, total);
    if (threadIdx.x == 0) { a.partial[blockIdx.y][blk] = (uint32_t)total; }
  }
}

__global__ __launch_bounds__(256) void k_flat_apply(const FlatScanArgs a) {
  __shared__ uint64_t smem[4];
  uint32_t * v = a.v[blockIdx.y];
  const uint64_t m = flat_length(a, blockIdx.y);
  const uint32_t * partial = a.partial[blockIdx.y];
  const uint64_t nblk = (m + kFlatChunk - 1) / kFlatChunk;
  for (uint64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    uint64_t before = 0;
    for (uint64_t q = threadIdx.x; q < blk; q += 256u) { before += partial[q]; }
    uint64_t prefix;
    (void)block_exclusive_scan(before, smem, prefix);        // (prefix = the sum over all threads)
    const uint64_t base = blk * kFlatChunk + (uint64_t)threadIdx.x * kFlatPer;
    uint32_t c[kFlatPer];
    uint64_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kFlatPer; ++k) { c[k] = base + k < m ? v[base + k] : 0u; s += c[k]; }
    uint64_t total;
    uint64_t run = prefix + block_exclusive_scan(s, smem, total);
#pragma unroll
    for (uint32_t k = 0; k < kFlatPer; ++k) { if (base + k < m) { v[base + k] = (uint32_t)run; } run += c[k]; }
    if (blk + 1 == nblk && threadIdx.x == 0) { *a.total[blockIdx.y] = (uint32_t)(prefix + total); }
  }
}

// first record of every bucket this level makes: the chunk table of the next level (or of the consumer).  The tail of
// k_part_scatter (a launch of its own until round 17): the scanned counts it reads are final before that launch starts,
// and next_start is the half of the ping-pong starts buffer that no workgroup of the launch reads.  Grid-stride: a small
// input has 8 workgroups and up to 2^17 + 1 entries.  (Behind the tiles, not in front of them, and with 32-bit indices — a
// level has at most 2^27 buckets: in front, the scatter kernels came out 4-8 registers larger and two of them lost a
// workgroup a CU.)
__device__ __forceinline__ void part_write_starts(const PartArgs & a, const PartIdx & p) {
  const uint32_t buckets = (a.single_seg != 0u ? 1u : p.chunks) << a.bits;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= buckets; i += gridDim.x * blockDim.x) {
    uint64_t at;
    if (i == buckets) { at = *p.total; }
    else if (a.single_seg != 0u) { at = p.cnt[(uint64_t)i * p.ctile[p.chunks]]; }
    else {
      // (a chunk without tiles reads the entry of whatever follows it: the position where the next records begin)
      const uint32_t c = i >> a.bits, b = i & ((1u << a.bits) - 1u), t0 = p.ctile[c];
      at = p.cnt[((uint64_t)t0 << a.bits) + (uint64_t)b * (p.ctile[c + 1] - t0)];
    }
    // Never past what the output buffer holds.  The counts include the records the scatter dropped at out_cap (a link
    // partition whose caller guessed too few links: network_run sees the total and repeats with bigger buffers); with the
    // starts as counted, the next level and k_csr_bucket* READ the buffer up to that total — as far past its end as the
    // guess was short, into whatever lies behind the allocation: an illegal access when nothing is mapped there.
    p.next_start[i] = at < p.out_cap ? at : p.out_cap;
  }
}

// THREADS: 512 a workgroup, 1024 for the tile of 8192 — the staging area (22–76 KB) allows one to three workgroups a CU,
// so the waves that hide the loads' and stores' way are a matter of the workgroup's size
// (SPAN: told to stay within the 64 registers that four 512-thread workgroups a CU need — it came out at 70)
template <uint32_t TILE, uint32_t BINS, uint32_t THREADS, bool SPAN = false>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(SPAN && THREADS == 512 ? 8 : 1))) void k_part_scatter(const PartArgs a) {
  constexpr uint32_t kPartPer = TILE / THREADS;
  // (dynamic LDS — part_scatter_lds bytes: a tile of 8192 records with 1024 bins is 76 KB, beyond what a kernel gets unasked)
  extern __shared__ __attribute__((aligned(16))) unsigned long long part_lds[];
  unsigned long long * stage = part_lds;                                     // [TILE]
  uint32_t * hist = reinterpret_cast<uint32_t *>(stage + TILE);               // [BINS]
  uint32_t * lstart = hist + BINS;                                            // [BINS]
  uint32_t * goff = lstart + BINS;                                            // [BINS]
  __shared__ uint64_t smem[THREADS / 64u];
  __shared__ uint32_t sh[1];
  __shared__ typename std::conditional<SPAN, SpanLds, uint32_t>::type span;
  const PartIdx & p = a.p[blockIdx.y];
  const uint32_t bins = 1u << a.bits;
  const uint32_t ntiles = p.ctile[p.chunks];
  for (uint32_t v = blockIdx.x; v < ((ntiles + (8u << a.run_bits) - 1u) & ~((8u << a.run_bits) - 1u)); v += gridDim.x) {
    const uint32_t t = xcd_tile(v, a.run_bits);
    if (t >= ntiles) { continue; }
    for (uint32_t b = threadIdx.x; b < bins; b += THREADS) { hist[b] = 0u; }
    PartTile tile{0u, 0u, 0ull};
    unsigned long long rec[kPartPer];
    uint32_t pos[kPartPer];
    const auto digit_of = [&](unsigned long long r) { return (((uint32_t)(r >> 32) - a.bias) >> a.shift) & (bins - 1u); };
    if constexpr (SPAN) {
#pragma unroll
      for (uint32_t k = 0; k < kPartPer; ++k) { rec[k] = kRecAbsent; pos[k] = 0u; }
      (void)part_span<kPartPer, THREADS>(p, TILE, t, span, [&](uint32_t k, uint64_t place) {
        rec[k] = p.in[place];
        if (rec[k] != kRecAbsent) { pos[k] = atomicAdd(&hist[digit_of(rec[k])], 1u); }
      });
    } else {
      tile = part_tile(p, TILE, t, sh);
#pragma unroll
      for (uint32_t k = 0; k < kPartPer; ++k) {
        const uint32_t j = k * THREADS + threadIdx.x;
        rec[k] = kRecAbsent; pos[k] = 0u;
        if (j < tile.count) { rec[k] = p.in[tile.first + j]; }
        if (rec[k] != kRecAbsent) { pos[k] = atomicAdd(&hist[digit_of(rec[k])], 1u); }
      }
    }
    __syncthreads();
    {
      // exclusive scan of the tile's histogram (consecutive bins per thread) and the tile's output positions
      constexpr uint32_t kB = (BINS + THREADS - 1u) / THREADS;
      uint32_t h[kB];
      uint64_t sum = 0;
#pragma unroll
      for (uint32_t q = 0; q < kB; ++q) { const uint32_t b = kB * threadIdx.x + q; h[q] = b < bins ? hist[b] : 0u; sum += h[q]; }
      uint64_t total;
      uint32_t run = (uint32_t)block_exclusive_scan_of<THREADS>(sum, smem, total);
#pragma unroll
      for (uint32_t q = 0; q < kB; ++q) {
        const uint32_t b = kB * threadIdx.x + q;
        if (b < bins) { lstart[b] = run; goff[b] = p.cnt[part_flat(a, p, tile.c, t, b)]; }
        run += h[q];
      }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kPartPer; ++k) {
      if (rec[k] != kRecAbsent) {
        const uint32_t at = lstart[(((uint32_t)(rec[k] >> 32) - a.bias) >> a.shift) & (bins - 1u)] + pos[k];
        stage[at] = rec[k];
      }
    }
    __syncthreads();
    const uint32_t present = lstart[bins - 1u] + hist[bins - 1u];
    // (unrolled over the thread's places: the staged records, then their bins' offsets, are read side by side — a loop
    // with a run-time bound walks four dependent LDS round trips per record one record after the other)
#pragma unroll
    for (uint32_t k = 0; k < kPartPer; ++k) {
      const uint32_t j = k * THREADS + threadIdx.x;
      if (j < present) {
        const unsigned long long r = stage[j];
        const uint32_t d = (((uint32_t)(r >> 32) - a.bias) >> a.shift) & (bins - 1u);
        const uint64_t g = (uint64_t)goff[d] + (j - lstart[d]);
        if (g < p.out_cap) {
          p.out[g] = r;
        }
      }
    }
    __syncthreads();
  }
  part_write_starts(a, p);
}

constexpr size_t part_scatter_lds(uint32_t tile, uint32_t bins) { return (size_t)tile * 8u + 3u * (size_t)bins * 4u; }

// ---- CSR from the partitioned links --------------------------------------------------------------------------------
// After the partition a bucket holds the links of 2^r consecutive sources.  One WAVE per bucket (k_csr_bucket): count
// per source in LDS, scan, place the targets row by row, sort every row, write — the rows of the bucket are contiguous
// in the neighbour array, and their offsets come from the same scan.  The database is in abundance order, so the
// link-rich sources sit together at its start: buckets with more links than a wave stages are listed and taken by a
// whole workgroup each (k_csr_bucket_big); what even that cannot stage is placed directly in the neighbour array and
// sorted there, one row at a time through LDS.
constexpr uint32_t kCsrMaxR = SWA_CSR_MAX_R;                 // sources per bucket: 2^r, r <= this
constexpr uint32_t kCsrStage = 1024;              // links a wave stages in LDS
constexpr uint32_t kCsrBigStage = 8192;           // links a workgroup stages in LDS
struct CsrArgs {
  const unsigned long long * links;  // partitioned: source << 32 | target
  const uint64_t * bstart;           // [buckets + 1]
  uint32_t buckets, r, first, count;
  uint64_t * offsets;                // [count + 1]
  uint32_t * neighbours;
  uint64_t cap;
  uint32_t * heavy;                  // [buckets] buckets left to k_csr_bucket_big
  uint32_t * heavy_count;
  uint64_t * end_copy;               // the last offset once more, in the context's status block (the guard reads it from there)
};

// ascending sort of v[0, len) in LDS by one wave (odd-even transposition; rows are short)
__device__ __forceinline__ void wave_sort_lds(uint32_t * v, uint32_t len, uint32_t lane) {
  for (uint32_t phase = 0; phase < len; ++phase) {
    for (uint32_t i = (phase & 1u) + 2u * lane; i + 1u < len; i += 128u) {
      const uint32_t x = v[i], y = v[i + 1u];
      if (x > y) { v[i] = y; v[i + 1u] = x; }
    }
    wave_lds_sync();
  }
}

// insertion sort of the short rows a thread owns: rows [first_row, rows) step `step`, bounds in off[]
__device__ __forceinline__ void sort_short_rows(uint32_t * stage, const uint32_t * off, uint32_t rows, uint32_t first_row, uint32_t step) {
  for (uint32_t i = first_row; i < rows; i += step) {
    const uint32_t lo = off[i], hi = off[i + 1u];
    if (hi - lo > 32u) { continue; }
    for (uint32_t x = lo + 1u; x < hi; ++x) {
      const uint32_t v = stage[x];
      uint32_t y = x;
      while (y > lo && stage[y - 1u] > v) { stage[y] = stage[y - 1u]; --y; }
      stage[y] = v;
    }
  }
}

// ... the rows of a wave's bucket, lane i the rows i, i + 64, ..: a row of up to 16 targets is sorted in REGISTERS by a
// bitonic network of the next power of two (its targets read side by side, padded with the largest value, written back):
// two LDS round trips and 6 / 24 / 80 comparators instead of the insertion sort's len^2 / 4 DEPENDENT round trips by
// one lane while 63 wait — a seed's row of twenty links was ~100 of them (the kernel cut short after each of its stages:
// sorting 0.067 of its 0.16 ms at 10 M, profiles/r04/NOTES.md).  Longer rows are left to the whole wave (rank sort up to 64,
// wave_sort_lds beyond).  Round 6: the network of 32 is gone — 240 comparators run by the whole wave for ONE lane's row,
// and the 113 registers it cost kept the kernel at four workgroups a CU where its LDS allows six.
__device__ __forceinline__ void order2(uint32_t & x, uint32_t & y) { const uint32_t lo = min(x, y), hi = max(x, y); x = lo; y = hi; }
template <int N>
__device__ __forceinline__ void sort_row_in_registers(uint32_t * row, uint32_t len) {
  uint32_t v[N];
#pragma unroll
  for (int k = 0; k < N; ++k) { v[k] = (uint32_t)k < len ? row[k] : 0xFFFFFFFFu; }
#pragma unroll
  for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const int l = i ^ j;
        if (l > i) { if ((i & k) == 0) { order2(v[i], v[l]); } else { order2(v[l], v[i]); } }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) { if ((uint32_t)k < len) { row[k] = v[k]; } }
}
// a row of 33..64 targets by the whole wave: lane x counts the targets that come before its own (every lane reads the same
// target at a time — a broadcast), then puts it there.  (The odd-even transposition sort takes `len` synchronised phases.)
__device__ __forceinline__ void wave_rank_sort64(uint32_t * row, uint32_t len, uint32_t lane) {
  const bool have = lane < len;
  const uint32_t mine = have ? row[lane] : 0xFFFFFFFFu;
  uint32_t rank = 0;
  for (uint32_t y = 0; y < len; ++y) { const uint32_t u = row[y]; rank += (u < mine || (u == mine && y < lane)) ? 1u : 0u; }
  wave_lds_sync();
  if (have) { row[rank] = mine; }
  wave_lds_sync();
}
template <uint32_t ROWS_MAX>
__device__ __forceinline__ void sort_rows_of_wave(uint32_t * stage, const uint32_t * off, uint32_t rows, uint32_t lane) {
  uint32_t lo[ROWS_MAX / 64u], len[ROWS_MAX / 64u];
#pragma unroll
  for (uint32_t q = 0; q < ROWS_MAX / 64u; ++q) {
    const uint32_t i = lane + 64u * q;
    lo[q] = i < rows ? off[i] : 0u; len[q] = i < rows ? off[i + 1u] - lo[q] : 0u;
    if (len[q] >= 2u && len[q] <= 4u) { sort_row_in_registers<4>(stage + lo[q], len[q]); }
    if (len[q] > 4u && len[q] <= 8u) { sort_row_in_registers<8>(stage + lo[q], len[q]); }
    if (len[q] > 8u && len[q] <= 16u) { sort_row_in_registers<16>(stage + lo[q], len[q]); }
  }
  // the long rows, one after the other, by the whole wave (found by a ballot: not by walking every row's bounds)
#pragma unroll
  for (uint32_t q = 0; q < ROWS_MAX / 64u; ++q) {
    unsigned long long todo = __ballot(len[q] > 16u);
    while (todo != 0ull) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const uint32_t l = lane_value(len[q], src), at = lane_value(lo[q], src);
      if (l <= 64u) { wave_rank_sort64(stage + at, l, lane); } else { wave_sort_lds(stage + at, l, lane); }
    }
  }
}

// (89 registers: five workgroups a CU.  Held to the 85 of six — amdgpu_waves_per_eu — it spills 32 bytes and takes 0.145 ms for 0.129)
template <int RB>
__global__ __launch_bounds__(256) void k_csr_bucket(const CsrArgs a) {
  __shared__ uint32_t cnt_all[4][1u << RB];
  __shared__ uint32_t off_all[4][(1u << RB) + 1u];
  __shared__ uint32_t stage_all[4][kCsrStage];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  uint32_t * cnt = cnt_all[wave];
  uint32_t * off = off_all[wave];
  uint32_t * stage = stage_all[wave];
  const uint32_t rows = 1u << a.r;
  const uint32_t nwaves = gridDim.x * 4u;
  for (uint32_t b = blockIdx.x * 4u + wave; b < a.buckets; b += nwaves) {
    const uint64_t start = a.bstart[b];
    const uint32_t c = (uint32_t)(a.bstart[b + 1] - start);
    const uint32_t row0 = b << a.r;                           // first source of the bucket, relative to a.first
    if (c > kCsrStage) {
      if (lane == 0u) { a.heavy[atomicAdd(a.heavy_count, 1u)] = b; }
      continue;
    }
    for (uint32_t i = lane; i < rows; i += 64u) { cnt[i] = 0u; }
    wave_lds_sync();
    // ONE pass over the bucket's links, all loads in flight together: target and row stay in registers, the counting
    // atomic returns the link's place inside its row
    constexpr uint32_t kPer = kCsrStage / 64u;
    const uint32_t turns = (c + 63u) >> 6;                    // (wave-uniform: the unrolled loops below stop there)
    uint32_t dst[kPer], rowpos[kPer];
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      if (k >= turns) { break; }
      const uint32_t j = k * 64u + lane;
      const unsigned long long e = j < c ? a.links[start + j] : 0ull;
      dst[k] = (uint32_t)e;
      rowpos[k] = ((uint32_t)(e >> 32) - a.first) & (rows - 1u);
    }
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      if (k >= turns) { break; }
      if (k * 64u + lane < c) { rowpos[k] |= atomicAdd(&cnt[rowpos[k]], 1u) << 16; }
    }
    wave_lds_sync();
    // exclusive scan of the row sizes: every lane takes rows / 64 consecutive rows
    {
      const uint32_t per = (rows + 63u) >> 6;
      uint32_t s = 0;
      for (uint32_t k = 0; k < per; ++k) { const uint32_t i = lane * per + k; s += i < rows ? cnt[i] : 0u; }
      uint32_t incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, (unsigned)d, 64); if ((int)lane >= d) { incl += up; } }
      uint32_t run = incl - s;
      for (uint32_t k = 0; k < per; ++k) { const uint32_t i = lane * per + k; if (i < rows) { off[i] = run; run += cnt[i]; } }
      if (lane == 63u) { off[rows] = run; }
    }
    wave_lds_sync();
    for (uint32_t i = lane; i < rows; i += 64u) { if (row0 + i < a.count) { a.offsets[row0 + i] = start + off[i]; } }
    if (b + 1u == a.buckets && lane == 0u) { a.offsets[a.count] = start + c; *a.end_copy = start + c; }
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      if (k >= turns) { break; }
      if (k * 64u + lane < c) { stage[off[rowpos[k] & 0xFFFFu] + (rowpos[k] >> 16)] = dst[k]; }
    }
    wave_lds_sync();
    // every lane sorts the rows it owns (about two targets per row) in registers; the few long rows are sorted by the whole wave
    sort_rows_of_wave<(1u << RB)>(stage, off, rows, lane);
    wave_lds_sync();
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      if (k >= turns) { break; }
      const uint32_t j = k * 64u + lane;
      if (j < c && start + j < a.cap) { a.neighbours[start + j] = stage[j]; }
    }
    wave_lds_sync();
  }
}

// the buckets k_csr_bucket listed: one workgroup each
__global__ __launch_bounds__(256) void k_csr_bucket_big(const CsrArgs a) {
  __shared__ uint32_t cnt[1u << kCsrMaxR];
  __shared__ uint32_t off[(1u << kCsrMaxR) + 1u];
  __shared__ uint32_t stage[kCsrBigStage];
  __shared__ uint64_t smem[4];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t rows = 1u << a.r;
  const uint32_t nheavy = *a.heavy_count;
  for (uint32_t h = blockIdx.x; h < nheavy; h += gridDim.x) {
    const uint32_t b = a.heavy[h];
    const uint64_t start = a.bstart[b];
    const uint32_t c = (uint32_t)(a.bstart[b + 1] - start);
    const uint32_t row0 = b << a.r;
    for (uint32_t i = threadIdx.x; i < rows; i += 256u) { cnt[i] = 0u; }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < c; j += 256u) { atomicAdd(&cnt[((uint32_t)(a.links[start + j] >> 32) - a.first) & (rows - 1u)], 1u); }
    __syncthreads();
    {
      const uint32_t i0 = 2u * threadIdx.x, i1 = i0 + 1u;      // (rows <= 512)
      const uint32_t c0 = i0 < rows ? cnt[i0] : 0u, c1 = i1 < rows ? cnt[i1] : 0u;
      uint64_t total;
      const uint32_t ex = (uint32_t)block_exclusive_scan((uint64_t)c0 + c1, smem, total);
      if (i0 < rows) { off[i0] = ex; }
      if (i1 < rows) { off[i1] = ex + c0; }
      if (threadIdx.x == 0) { off[rows] = (uint32_t)total; }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < rows; i += 256u) {
      if (row0 + i < a.count) { a.offsets[row0 + i] = start + off[i]; }
      cnt[i] = off[i];
    }
    if (b + 1u == a.buckets && threadIdx.x == 0) { a.offsets[a.count] = start + c; *a.end_copy = start + c; }
    __syncthreads();
    if (c <= kCsrBigStage) {
      for (uint32_t j = threadIdx.x; j < c; j += 256u) {
        const unsigned long long e = a.links[start + j];
        stage[atomicAdd(&cnt[((uint32_t)(e >> 32) - a.first) & (rows - 1u)], 1u)] = (uint32_t)e;
      }
      __syncthreads();
      sort_short_rows(stage, off, rows, threadIdx.x, 256u);
      // (long rows: a wave each; rows are disjoint, so the waves need no barrier between them)
      for (uint32_t i = wave; i < rows; i += 4u) {
        const uint32_t lo = off[i], len = off[i + 1u] - lo;
        if (len > 32u) { wave_sort_lds(stage + lo, len, lane); }
      }
      __syncthreads();
      for (uint32_t j = threadIdx.x; j < c; j += 256u) { if (start + j < a.cap) { a.neighbours[start + j] = stage[j]; } }
    } else if (start + c <= a.cap) {
      for (uint32_t j = threadIdx.x; j < c; j += 256u) {
        const unsigned long long e = a.links[start + j];
        a.neighbours[start + atomicAdd(&cnt[((uint32_t)(e >> 32) - a.first) & (rows - 1u)], 1u)] = (uint32_t)e;
      }
      __threadfence();
      __syncthreads();
      // one row at a time through a wave's quarter of the staging area (rows of such a bucket are long)
      uint32_t * mine = stage + wave * (kCsrBigStage / 4u);
      for (uint32_t i = wave; i < rows; i += 4u) {
        const uint32_t lo = off[i], len = off[i + 1u] - lo;
        if (len < 2u) { continue; }
        uint32_t * row = a.neighbours + start + lo;
        if (len <= kCsrBigStage / 4u) {
          for (uint32_t x = lane; x < len; x += 64u) { mine[x] = row[x]; }
          wave_lds_sync();
          wave_sort_lds(mine, len, lane);
          for (uint32_t x = lane; x < len; x += 64u) { row[x] = mine[x]; }
          wave_lds_sync();
        } else {                                               // (longer than any row of sequences up to 256 nt: in place)
          for (uint32_t phase = 0; phase < len; ++phase) {
            for (uint32_t x = (phase & 1u) + 2u * lane; x + 1u < len; x += 128u) {
              const uint32_t u = row[x], v = row[x + 1u];
              if (u > v) { row[x] = v; row[x + 1u] = u; }
            }
            __threadfence_block();
            __builtin_amdgcn_wave_barrier();
          }
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

__global__ __launch_bounds__(256) void k_clear_many(const ClearList c) {
  for (uint32_t k = 0; k < c.n; ++k) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.words[k]; i += (uint64_t)gridDim.x * blockDim.x) { c.p[k][i] = 0u; }
  }
}

// loads this translation unit's code object (see swa_ctx_warmup): an empty launch
void swa_warm_d1_part(swa_ctx * ctx) { hipLaunchKernelGGL(k_clear_many, dim3(1), dim3(64), 0, ctx->stream, ClearList{}); }

// (the member offsets of the --fastidious groups: its only caller is the pair route of fastidious.hip)
int swa_scan_offsets(swa_ctx * ctx, const uint32_t * counts, uint32_t n, uint64_t * offsets) {
  static_assert(kScanTile == (int)kScanOffsetsTile, "swa_scan_offsets: the tile the caller sized d_scan_tmp for");
  const uint32_t tiles = (uint32_t)(((uint64_t)n + kScanTile - 1) / kScanTile);
  auto * sums = static_cast<uint64_t *>(ctx->d_scan_tmp.ptr);
  hipLaunchKernelGGL(k_scan_tiles, dim3(tiles), dim3(kScanBlock), 0, ctx->stream, counts, n, sums);
  hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(kScanBlock), 0, ctx->stream, sums, tiles);
  hipLaunchKernelGGL(k_scan_apply, dim3(tiles), dim3(kScanBlock), 0, ctx->stream, counts, n, sums, offsets);
  return SWA_OK;
}

// scratch sizes of a job (entries): flat counts, tile table, chunk starts (per half), scan partials
void swa_part_scratch(const PartJob & j, uint64_t * cnt, uint64_t * ctile, uint64_t * starts_half, uint64_t * partial) {
  uint64_t chunks = j.chunks0, c_max = 0, t_max = 0, s_max = 0;
  bool single = j.single0;
  for (uint32_t l = 0; l < j.plan.levels; ++l) {
    const uint64_t tiles = (l == 0 ? j.max_tiles0 : j.max_records / j.tile + chunks + 1);
    c_max = std::max(c_max, (tiles << j.plan.bits[l]) + 2);
    t_max = std::max(t_max, chunks + 2 + tiles + 2);              // (the tile table of the chunks, and behind it the chunk of every tile)
    chunks = (single ? 1 : chunks) << j.plan.bits[l];
    single = false;
    s_max = std::max(s_max, chunks + 2);
  }
  *cnt = c_max; *ctile = t_max; *starts_half = s_max; *partial = c_max / kFlatChunk + 2;
}

int swa_clear_launch(swa_ctx * ctx, const ClearList & c) {
  uint64_t most = 0;
  for (uint32_t k = 0; k < c.n; ++k) { most = std::max(most, c.words[k]); }
  if (c.n == 0 || most == 0) { return SWA_OK; }
  hipLaunchKernelGGL(k_clear_many, dim3(swa_grid_for(ctx, most, 256, 8)), dim3(256), 0, ctx->stream, c);
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}

void swa_flat_scan(swa_ctx * ctx, dim3 grid, const FlatScanArgs & f) {
  hipLaunchKernelGGL(k_flat_sums, grid, dim3(256), 0, ctx->stream, f);
  hipLaunchKernelGGL(k_flat_apply, grid, dim3(256), 0, ctx->stream, f);
}

// The forms of a level, chosen by the job: 512 bins in tiles of 2048 (key records) or 4096 (links: the first level of
// several chunks cuts its tiles from the chunks laid end to end — part_span); 1024 bins for the one-level key partition,
// in tiles of 8192 when k_keys has taken the histogram, else of 4096 (routed builds).
int swa_part_run(swa_ctx * ctx, PartJob & j) {
  uint64_t chunks = j.chunks0;
  bool single = j.single0;
  uint32_t used_bits = 0;
  const int cu_grid = ctx->num_cus * 8;
  for (uint32_t l = 0; l < j.plan.levels; ++l) {
    const uint32_t bits = j.plan.bits[l];
    used_bits += bits;
    const bool wide = bits > kPartMaxBits;                      // (1024 bins: the one-level key partition)
    const bool hist_done = l == 0 && j.hist0_done;
    // (k_part_hist holds tiles of up to 4096)
    const bool have_form = wide ? j.tile == 4096 || (j.tile == 8192 && hist_done) : j.tile == 2048 || j.tile == 4096;
    if (!have_form) { return swa_fail_msg(ctx, SWA_E_ARG, "partition: no kernel for this tile and bin count"); }
    PartArgs a{};
    a.single_seg = single ? 1u : 0u; a.bits = bits; a.shift = j.top_bit - used_bits; a.bias = j.bias; a.tile = j.tile;
    a.span = (single && l == 0 && chunks > 1 && j.tile == 4096 && !wide && !hist_done) ? 1u : 0u;
    // runs of 16 consecutive tiles per XCD (xcd_tile; measured at 10 M amplicons: key partition 0.44 -> 0.33 ms, link partition
    // 0.39 -> 0.36, the same for runs of 8 .. 64) — unless there are fewer tiles than workgroups in flight, where the runs
    // would leave XCDs without work
    const uint64_t tiles = (l == 0 ? j.max_tiles0 : j.max_records / j.tile + chunks + 1);
    a.run_bits = tiles >= (uint64_t)cu_grid ? 4u : 0u;
    for (uint32_t i = 0; i < j.nidx; ++i) {
      PartIdx & p = a.p[i];
      p.in = l == 0 ? j.in[i] : j.buf[i][(l - 1) & 1u];
      p.out = j.buf[i][l & 1u];
      p.out_cap = j.out_cap;
      p.cstart = l == 0 ? j.cstart0[i] : j.starts[i] + ((l - 1) & 1u) * j.starts_stride;
      p.cstride = l == 0 ? j.cstride0[i] : 0;
      p.csize = l == 0 ? j.csize0[i] : nullptr;
      p.csize_cap = j.csize_cap;
      p.chunks = (uint32_t)chunks;
      p.ctile = j.ctile[i]; p.cnt = j.cnt[i];
      p.tchunk = j.ctile[i] + chunks + 1; p.tchunk_cap = (uint32_t)std::min<uint64_t>(tiles + 1, 0xFFFFFFFFu);
      p.next_start = j.starts[i] + (l & 1u) * j.starts_stride;
      p.total = j.total[i];
    }
    // (a multiple of 8 workgroups: turn v of the tile loops then stays on XCD v mod 8 — xcd_tile)
    const dim3 grid_t((unsigned)((std::min<uint64_t>(std::max<uint64_t>(tiles, 1), (uint64_t)cu_grid) + 7) & ~7ull), j.nidx);
    if (hist_done && j.tiles0_done) { /* (k_keys has left the three entries of the single chunk's table) */ }
    else if (l == 0 && j.seg != nullptr) {
      if (chunks > 2048) { hipLaunchKernelGGL((k_part_tiles<1024, true>), dim3(1, 1), dim3(1024), 0, ctx->stream, a, *j.seg); }
      else { hipLaunchKernelGGL((k_part_tiles<256, true>), dim3(1, 1), dim3(256), 0, ctx->stream, a, *j.seg); }
    }
    else if (chunks > 2048) { hipLaunchKernelGGL(k_part_tiles<1024>, dim3(1, j.nidx), dim3(1024), 0, ctx->stream, a, SegArgs{}); }
    else { hipLaunchKernelGGL(k_part_tiles<256>, dim3(1, j.nidx), dim3(256), 0, ctx->stream, a, SegArgs{}); }
    if (hist_done) { /* (k_keys has left the counts) */ }
    else if (wide) { hipLaunchKernelGGL((k_part_hist<1024, kPartTileMax, 256>), grid_t, dim3(256), 0, ctx->stream, a); }
    else if (a.span != 0u) { hipLaunchKernelGGL((k_part_hist<512, kPartTileMax, 256, true>), grid_t, dim3(256), 0, ctx->stream, a); }
    else { hipLaunchKernelGGL((k_part_hist<512, kPartTileMax, 256>), grid_t, dim3(256), 0, ctx->stream, a); }
    FlatScanArgs f{};
    f.unit_bits = bits;
    for (uint32_t i = 0; i < j.nidx; ++i) { f.v[i] = j.cnt[i]; f.units[i] = j.ctile[i] + chunks; f.partial[i] = j.partial[i]; f.total[i] = j.total[i]; }
    const dim3 grid_f((unsigned)std::min<uint64_t>(((tiles << bits) + 1 + kFlatChunk - 1) / kFlatChunk, (uint64_t)cu_grid), j.nidx);
    swa_flat_scan(ctx, grid_f, f);
    // (512 threads a workgroup — key partition 0.269 -> 0.239, link partition 0.317 -> 0.303 ms at 10 M against 256 —, 1024
    // for the tile of 8192, whose 76 KB of LDS are asked for: the attribute belongs to the function on a device, once per context)
    if (wide && j.tile == 8192) {
      constexpr size_t lds = part_scatter_lds(8192, 1024);
      if (!ctx->part_lds_opt_in) {
        SWA_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&k_part_scatter<8192, 1024, 1024>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        ctx->part_lds_opt_in = true;
      }
      hipLaunchKernelGGL((k_part_scatter<8192, 1024, 1024>), grid_t, dim3(1024), lds, ctx->stream, a);
    }
    else if (wide) { hipLaunchKernelGGL((k_part_scatter<4096, 1024, 512>), grid_t, dim3(512), part_scatter_lds(4096, 1024), ctx->stream, a); }
    else if (j.tile == 2048) { hipLaunchKernelGGL((k_part_scatter<2048, 512, 512>), grid_t, dim3(512), part_scatter_lds(2048, 512), ctx->stream, a); }
    else if (a.span != 0u) { hipLaunchKernelGGL((k_part_scatter<4096, 512, 512, true>), grid_t, dim3(512), part_scatter_lds(4096, 512), ctx->stream, a); }
    else { hipLaunchKernelGGL((k_part_scatter<4096, 512, 512>), grid_t, dim3(512), part_scatter_lds(4096, 512), ctx->stream, a); }
    // (the scatter has written the bucket starts on its way: part_write_starts)
    chunks = (single ? 1 : chunks) << bits;
    single = false;
    SWA_HIP(ctx, hipGetLastError());
  }
  j.buckets = (uint32_t)chunks;
  j.last = (int)((j.plan.levels - 1) & 1u);
  for (uint32_t i = 0; i < j.nidx; ++i) {
    j.out[i] = j.buf[i][j.last];
    j.bstart[i] = j.starts[i] + (uint64_t)j.last * j.starts_stride;
  }
  return SWA_OK;
}

// CSR of the links in the per-wave segments by the streaming route: the links partitioned by the top bits of their
// source (relative to `first`) until a bucket holds 2^r consecutive sources, then one wave per bucket (k_csr_bucket).
// link_cap: entries of the two internal link buffers; a run with more links than that leaves garbage and is repeated
// by the caller with bigger buffers (the total is known after the host has synchronised).
// (the chunks of the first level: `chunks` runs of links, run c = links[cstart[c] .. + min(csize[c], csize_cap)) — the per-wave
// segments of the pair kernels, or the ranks' lists of a multi-GPU job gathered on one device)
static int csr_from_chunks(swa_ctx * ctx, uint32_t first, uint32_t count, const unsigned long long * links, const uint64_t * d_cstart, uint64_t cstride,
                           const uint32_t * d_csize, uint32_t chunks, uint32_t csize_cap, uint64_t max_tiles0, uint64_t link_cap,
                           uint64_t * d_offsets, uint32_t * d_neighbours, uint64_t cap, const SegArgs * seg = nullptr, bool heavy_cleared = false) {
  const swa_csr_plan plan = swa_csr_plan_for(count);          // (host_tables.cpp)
  const uint32_t nbits = plan.nbits, r = plan.r;
  PartJob j;
  j.nidx = 1;
  j.plan = plan.lv;
  j.max_records = link_cap;
  j.out_cap = link_cap;
  j.tile = 4096;
  j.max_tiles0 = max_tiles0;
  j.chunks0 = chunks; j.single0 = true; j.top_bit = nbits; j.bias = first;
  j.csize_cap = csize_cap;
  uint64_t e_cnt, e_tile, e_start, e_partial;
  swa_part_scratch(j, &e_cnt, &e_tile, &e_start, &e_partial);
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbLinkA], (link_cap + 1) * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbLinkB], (link_cap + 1) * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbCnt], e_cnt * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbTile], e_tile * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbStart], (2 * e_start + 4) * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbPartial], e_partial * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbScal], 64 * sizeof(uint64_t)));
  j.in[0] = links;
  j.buf[0][0] = static_cast<unsigned long long *>(ctx->d_stream[kSbLinkA].ptr);
  j.buf[0][1] = static_cast<unsigned long long *>(ctx->d_stream[kSbLinkB].ptr);
  j.cstart0[0] = d_cstart; j.cstride0[0] = cstride;
  j.csize0[0] = d_csize;
  j.seg = d_csize != nullptr && j.nidx == 1 ? seg : nullptr;
  j.cnt[0] = static_cast<uint32_t *>(ctx->d_stream[kSbCnt].ptr);
  j.ctile[0] = static_cast<uint32_t *>(ctx->d_stream[kSbTile].ptr);
  j.starts[0] = static_cast<uint64_t *>(ctx->d_stream[kSbStart].ptr);
  ctx->ix.part_starts_valid = false;                             // (the prefix index's bucket starts lay there: selectors 17 / 18)
  j.partial[0] = static_cast<uint32_t *>(ctx->d_stream[kSbPartial].ptr);
  j.total[0] = &swa_status(ctx)->links_sorted;
  j.starts_stride = e_start + 2;
  swa_t0(ctx, kTimeLinkPartition);
  SWA_TRY(swa_part_run(ctx, j));
  swa_t1(ctx, kTimeLinkPartition);
  CsrArgs c{};
  c.links = j.out[0]; c.bstart = j.bstart[0]; c.buckets = j.buckets; c.r = r; c.first = first; c.count = count;
  c.offsets = d_offsets; c.neighbours = d_neighbours; c.cap = d_neighbours != nullptr ? cap : 0;
  const void * heavy_before = ctx->d_stream[kSbHeavy].ptr;
  SWA_TRY(swa_reserve(ctx, ctx->d_stream[kSbHeavy], csr_heavy_bytes(count)));
  c.heavy = static_cast<uint32_t *>(ctx->d_stream[kSbHeavy].ptr) + 1;
  c.heavy_count = static_cast<uint32_t *>(ctx->d_stream[kSbHeavy].ptr);
  c.end_copy = &swa_status(ctx)->csr_end;
  // (the anchored network call has cleared the count with its other counters — launch_network_anchored — unless the
  // buffer is a new one since)
  if (!heavy_cleared || ctx->d_stream[kSbHeavy].ptr != heavy_before) { SWA_HIP(ctx, hipMemsetAsync(c.heavy_count, 0, sizeof(uint32_t), ctx->stream)); }
  swa_t0(ctx, kTimeCsrRows);
  // (as many workgroups as are resident together — every wave walks its share of the buckets; a grid of 8 a CU ran a second,
  // partly empty round behind the first)
  static const int csr_per_cu[2] = {
    [] { int nb = 0; return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_csr_bucket<8>, 256, 0) == hipSuccess && nb > 0 ? nb : 4; }(),
    [] { int nb = 0; return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_csr_bucket<9>, 256, 0) == hipSuccess && nb > 0 ? nb : 4; }() };
  const dim3 cgrid((unsigned)std::min<uint64_t>(((uint64_t)j.buckets + 3) / 4, (uint64_t)ctx->num_cus * (uint64_t)csr_per_cu[r <= 8 ? 0 : 1]));
  if (r <= 8) { hipLaunchKernelGGL(k_csr_bucket<8>, cgrid, dim3(256), 0, ctx->stream, c); }
  else { hipLaunchKernelGGL(k_csr_bucket<9>, cgrid, dim3(256), 0, ctx->stream, c); }
  hipLaunchKernelGGL(k_csr_bucket_big, dim3((unsigned)ctx->num_cus * 4), dim3(256), 0, ctx->stream, c);
  swa_t1(ctx, kTimeCsrRows);
  SWA_HIP(ctx, hipGetLastError());
  return SWA_OK;
}

int swa_d1_csr_stream(swa_ctx * ctx, uint32_t first, uint32_t count, uint32_t nseg, uint64_t link_cap, uint64_t * d_offsets,
                             uint32_t * d_neighbours, uint64_t cap, bool heavy_cleared) {
  // (the first level's k_part_tiles also makes of the segment fills what k_seg_reduce does: SegArgs)
  swa_status_block * st = swa_status(ctx);
  SegArgs seg{};
  seg.staged = static_cast<const uint32_t *>(ctx->d_seg_fill.ptr) + nseg;
  seg.out = reinterpret_cast<unsigned long long *>(st->stats) + kStatSeg;
  seg.fallback = st->counters + kCounterFallback; seg.fallback_copy = &st->fallback_copy;
  const uint64_t tiles_per_seg = (ctx->seg_cap + 4096 - 1) / 4096;
  return csr_from_chunks(ctx, first, count, static_cast<const unsigned long long *>(ctx->d_edges.ptr), nullptr, ctx->seg_cap,
                         static_cast<const uint32_t *>(ctx->d_seg_fill.ptr), nseg, (uint32_t)std::min<uint64_t>(ctx->seg_cap, 0xFFFFFFFFu),
                         (uint64_t)nseg * tiles_per_seg + 2, link_cap, d_offsets, d_neighbours, cap, &seg, heavy_cleared);
}

int swa_d1_seg_compact(swa_ctx * ctx, uint32_t nseg, uint64_t * d_edge_list, uint64_t cap) {
  swa_status_block * st = swa_status(ctx);
  SWA_TRY(swa_reserve(ctx, ctx->d_seg_base, uint64_t(nseg) * sizeof(uint64_t)));
  hipLaunchKernelGGL(k_seg_reduce, dim3(1), dim3(1024), 0, ctx->stream, static_cast<const uint32_t *>(ctx->d_seg_fill.ptr),
                     nseg, reinterpret_cast<unsigned long long *>(st->stats) + kStatSeg, st->counters + kCounterFallback, &st->fallback_copy);
  hipLaunchKernelGGL(k_seg_bases, dim3(1), dim3(256), 0, ctx->stream, static_cast<const uint32_t *>(ctx->d_seg_fill.ptr), nseg,
                     static_cast<unsigned long long *>(ctx->d_seg_base.ptr));
  hipLaunchKernelGGL(k_seg_compact, dim3(std::min<uint32_t>(nseg, (uint32_t)ctx->num_cus * 8u)), dim3(256), 0, ctx->stream,
                     static_cast<const uint64_t *>(ctx->d_edges.ptr), static_cast<const uint32_t *>(ctx->d_seg_fill.ptr),
                     nseg, ctx->seg_cap, static_cast<const unsigned long long *>(ctx->d_seg_base.ptr), d_edge_list, cap);
  return SWA_OK;
}

// The link exchange of a multi-GPU job, second half (include/swarm_amd.h): the CSR of the sources [first, first + count)
// from `lists` runs of (source << 32 | target) links as they lie on this context's device — the pieces a rank received, or
// the ranks' lists gathered on one device (multi.hip) — by the partition + row kernels of the single-GPU step (levels by
// source bits, then a wave per 256 sources) instead of a 64-bit radix sort of everything.  Every link lands in a row, so the
// need is the sum of the counts: known before anything is launched, and nothing is read back.
extern "C" int swa_d1_csr_from_lists(swa_ctx * ctx, const uint64_t * d_links, const uint64_t * starts, const uint64_t * counts, uint32_t lists,
                                     uint32_t first, uint32_t count, uint64_t * d_offsets, uint32_t * d_neighbours, uint64_t cap, uint64_t * total) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (count == 0 || (uint64_t)first + count > 0x100000000ull || d_offsets == nullptr || total == nullptr || (d_neighbours == nullptr && cap != 0) ||
      (lists != 0 && (starts == nullptr || counts == nullptr))) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_csr_from_lists: bad range or null buffer");
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  const uint32_t chunks = std::max<uint32_t>(lists, 1u);      // (no list: one without links)
  uint64_t all = 0, tiles = 2;
  std::vector<uint64_t> h_start(chunks, 0);
  std::vector<uint32_t> h_size(chunks, 0);
  for (uint32_t r = 0; r < lists; ++r) {
    if (counts[r] > 0xFFFFFFFFull) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_csr_from_lists: a list of more than 2^32 links"); }
    h_start[r] = starts[r]; h_size[r] = (uint32_t)counts[r];
    all += counts[r]; tiles += (counts[r] + 4095) / 4096;
  }
  if (all != 0 && d_links == nullptr) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_csr_from_lists: null link buffer"); }
  *total = all;
  SWA_TRY(swa_reserve(ctx, ctx->d_seg_base, ((uint64_t)chunks * 3 / 2 + 2) * sizeof(uint64_t)));
  auto * d_start = static_cast<uint64_t *>(ctx->d_seg_base.ptr);
  auto * d_size = reinterpret_cast<uint32_t *>(d_start + chunks);
  SWA_HIP(ctx, hipMemcpyAsync(d_start, h_start.data(), chunks * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  SWA_HIP(ctx, hipMemcpyAsync(d_size, h_size.data(), chunks * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));           // (the host vectors are temporaries)
  SWA_TRY(csr_from_chunks(ctx, first, count, reinterpret_cast<const unsigned long long *>(d_links), d_start, 0, d_size, chunks, 0xFFFFFFFFu, tiles,
                          all + 1, d_offsets, d_neighbours, cap));
  if (all > cap) { return swa_fail_msg(ctx, SWA_E_CAPACITY, "swa_d1_csr_from_lists: neighbour buffer too small"); }
  return SWA_OK;
}

// The link exchange, first half: a flat link list split by the rank that owns each link's source (k_links_split).
extern "C" int swa_d1_links_split(swa_ctx * ctx, const uint64_t * d_links, uint64_t m, const uint32_t * bounds, uint32_t world,
                                  uint64_t * d_out, uint64_t * d_counts) {
  if (ctx == nullptr) { return SWA_E_ARG; }
  if (world == 0 || world > kRouteMaxWorld || bounds == nullptr || d_counts == nullptr || (m != 0 && (d_links == nullptr || d_out == nullptr)) ||
      ((reinterpret_cast<uintptr_t>(d_links) | reinterpret_cast<uintptr_t>(d_out) | reinterpret_cast<uintptr_t>(d_counts)) & 7u) != 0) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_links_split: bad argument (1..64 ranks, 8-byte aligned buffers)");
  }
  SplitArgs a{};
  for (uint32_t r = 0; r <= world; ++r) {
    if (r == 0 ? bounds[0] != 0 : bounds[r] < bounds[r - 1]) { return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_links_split: bounds must begin at 0 and ascend"); }
    a.bounds[r] = bounds[r];
  }
  SWA_HIP(ctx, hipSetDevice(ctx->device));
  SWA_HIP(ctx, hipMemsetAsync(d_counts, 0, ((uint64_t)world + 1) * sizeof(uint64_t), ctx->stream));
  if (m == 0) {                                              // (nothing but the clear — and the counts are final on return here too)
    SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SWA_OK;
  }
  static_assert(kRouteMaxWorld * sizeof(uint64_t) <= sizeof(swa_status_block::cursors), "a run cursor for every rank");
  auto * cursor = reinterpret_cast<unsigned long long *>(swa_status(ctx)->cursors);
  SWA_HIP(ctx, hipMemsetAsync(cursor, 0, (uint64_t)world * sizeof(uint64_t), ctx->stream));
  a.head = (uint32_t)((reinterpret_cast<uintptr_t>(d_links) >> 3) & 1u);
  a.links = reinterpret_cast<const unsigned long long *>(d_links) - a.head;
  a.end = a.head + m;
  a.world = world;
  a.counts = reinterpret_cast<unsigned long long *>(d_counts);
  a.cursor = cursor;
  a.out = reinterpret_cast<unsigned long long *>(d_out);
  const uint64_t tiles = (a.end + kSplitTile - 1) / kSplitTile;
  const dim3 grid((unsigned)std::min<uint64_t>(tiles, (uint64_t)ctx->num_cus * 8));
  hipLaunchKernelGGL(k_links_split<false>, grid, dim3(kSplitThreads), 0, ctx->stream, a);
  hipLaunchKernelGGL(k_links_split<true>, grid, dim3(kSplitThreads), 0, ctx->stream, a);
  SWA_HIP(ctx, hipGetLastError());
  // ONE read, of the links no rank owns, into the pinned mirror of the status block: the counts are final when this returns
  uint64_t * beyond = ctx->h_status->cursors;
  SWA_HIP(ctx, hipMemcpyAsync(beyond, d_counts + world, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (*beyond != 0) {
    return swa_fail_msg(ctx, SWA_E_ARG, "swa_d1_links_split: " + std::to_string(*beyond) + " links with a source beyond the last rank's range (not written)");
  }
  return SWA_OK;
}
