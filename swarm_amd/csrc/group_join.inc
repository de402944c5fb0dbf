// group_join.inc — the grouped join of the --fastidious pair route (fastidious.hip, d1_fast.inc) and of the bulk d >= 2 graph
// route (dn_graph.hip), included inside each file's anonymous namespace after wave_ops.inc and key_ops.inc (kEmpty, kKeyEmpty,
// mix64).
//
// Two kinds of amplicons meet under 63-bit keys.  CREATORS (light amplicons; targets at all their shifts) claim slots of
// an open-addressing key table and count themselves, up to per_a keys each; JOINERS (heavy amplicons; queries) look one
// key up and count themselves where it exists.  Both are kernels of the route — which amplicons take part and under
// which keys is its business — written with join_claim / join_find.  The rest is here, once (join_run): a totals pass
// gives room only to the groups that can yield a pair, an exclusive scan (the route's: the one step the two do not share)
// turns the totals into member offsets, a scatter writes the member lists (creators first, then joiners), and an items
// pass deals every group's tiles round-robin to at most Shape::stride work items.  The route's pair kernel walks the
// items (tile = item.tile, + stride, ...) and keeps what it finds in a PairStage.

// ---- the key table --------------------------------------------------------------------------------------------------
// the slot of `key`, claimed if nobody had it (linear probing from the mixed key); kEmpty: the table is full
__device__ __forceinline__ uint32_t join_claim(unsigned long long * keys, uint64_t amask, uint64_t key) {
  uint64_t idx = mix64(key) & amask;
  for (uint64_t probes = 0; probes <= amask; ++probes) {
    const unsigned long long old = atomicCAS(&keys[idx], kKeyEmpty, (unsigned long long)key);
    if (old == kKeyEmpty || old == key) { return (uint32_t)idx; }
    idx = (idx + 1) & amask;
  }
  return kEmpty;
}

// the slot of `key` if a creator claimed one (the table is complete: the creators' kernel ran before), else kEmpty
__device__ __forceinline__ uint32_t join_find(const unsigned long long * keys, uint64_t amask, uint64_t key) {
  uint64_t idx = mix64(key) & amask;
  for (uint64_t probes = 0; probes <= amask; ++probes) {
    const unsigned long long have = keys[idx];
    if (have == key) { return (uint32_t)idx; }
    if (have == kKeyEmpty) { break; }
    idx = (idx + 1) & amask;
  }
  return kEmpty;
}

struct join_item { uint32_t begin, na, nb, tile; };   // members[begin, begin + na) creators, then nb joiners; first tile

// How a pair kernel cuts a group of na creators and nb joiners into tiles, and to how many items they are dealt
template <uint32_t A, uint32_t B, uint32_t STRIDE>
struct JoinBlocks {                        // A creators x B joiners a tile
  static constexpr uint32_t stride = STRIDE;
  static __device__ __forceinline__ uint64_t tiles(uint32_t na, uint32_t nb) { return (uint64_t)((na + A - 1u) / A) * ((nb + B - 1u) / B); }
};
template <uint32_t PAIRS, uint32_t STRIDE>
struct JoinPairTiles {                     // PAIRS of the na x nb pairs a tile
  static constexpr uint32_t stride = STRIDE;
  static __device__ __forceinline__ uint64_t tiles(uint32_t na, uint32_t nb) { return ((uint64_t)na * nb + PAIRS - 1u) / PAIRS; }
};

// The table and its lists, carved out of the context's d_f* buffers (join_table)
struct JoinTable {
  unsigned long long * keys;     // [asize]
  uint32_t * cnt_a, * cnt_b;     // [asize] creators / joiners of a slot
  uint32_t * cur_a, * cur_b;     // [asize] the scatter's cursors
  uint32_t * tot;                // [asize + 1] members of a group that has room in the member list, 0 for the others
  uint64_t * offsets;            // [asize + 1] first member of a slot's group
  uint32_t * aslot;              // [n * per_a] the slots an amplicon claimed (kEmpty: none)
  uint32_t * bslot;              // [n] the slot it found
  uint32_t * members;
  join_item * items;
  uint32_t * flags;              // the status block's flags + kFlagJoin: kJoinKeyOverflow, kJoinItemOverflow, and from kJoinItemCount
                                 // on item counters, one a join whose items are read while another join's are made
  uint64_t asize;                // a power of two
  uint32_t n, per_a;
};

__global__ __launch_bounds__(256) void k_join_clear(const JoinTable t) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.asize; i += (uint64_t)gridDim.x * blockDim.x) {
    t.keys[i] = kKeyEmpty; t.cnt_a[i] = 0u; t.cnt_b[i] = 0u; t.cur_a[i] = 0u; t.cur_b[i] = 0u;
  }
}

// room in the member list only for the groups with at least min_product (creator, joiner) combinations: 1 — one of each
// kind (--fastidious) — or 2 — a pair of DIFFERENT amplicons, an amplicon alone being its own target (d >= 2)
__global__ __launch_bounds__(256) void k_join_totals(const JoinTable t, uint32_t min_product) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.asize; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t a = t.cnt_a[i], b = t.cnt_b[i];
    t.tot[i] = a * b >= min_product ? (uint32_t)(a + b) : 0u;
  }
}

// One condition for both kinds: the group has room.  (Where min_product = 1 a creator's slot has cnt_a >= 1, so it has
// room exactly when a joiner found it, and a joiner has a slot only where a creator made the group, which then counts
// both: for those groups "has a slot" and "has room" are the same thing.)
__global__ __launch_bounds__(256) void k_join_scatter(const JoinTable t) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < t.n; i += gridDim.x * blockDim.x) {
    for (uint32_t j = 0; j < t.per_a; ++j) {
      const uint32_t s = t.aslot[(uint64_t)i * t.per_a + j];
      if (s != kEmpty && t.tot[s] != 0u) { t.members[t.offsets[s] + atomicAdd(&t.cur_a[s], 1u)] = i; }
    }
    const uint32_t s = t.bslot[i];
    if (s != kEmpty && t.tot[s] != 0u) { t.members[t.offsets[s] + t.cnt_a[s] + atomicAdd(&t.cur_b[s], 1u)] = i; }
  }
}

// one thread per key slot: the group's work items, min(Shape::tiles, Shape::stride) of them, item.tile = its first tile.
// Items past the cap are not dropped quietly: flags[kJoinItemOverflow] is raised and the route fails.
template <class Shape>
__global__ __launch_bounds__(256) void k_join_items(const JoinTable t, uint32_t * counter, uint32_t cap) {
  __shared__ uint32_t n_items, base;
  if (threadIdx.x == 0) { n_items = 0u; }
  __syncthreads();
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t start = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  auto items_of = [&](uint64_t s) -> uint32_t {
    if (t.tot[s] == 0u) { return 0u; }
    const uint64_t tiles = Shape::tiles(t.cnt_a[s], t.cnt_b[s]);
    return (uint32_t)(tiles < Shape::stride ? tiles : Shape::stride);
  };
  for (uint64_t s = start; s < t.asize; s += stride) {
    const uint32_t k = items_of(s);
    if (k != 0u) { atomicAdd(&n_items, k); }
  }
  __syncthreads();
  if (threadIdx.x == 0) { base = n_items != 0u ? atomicAdd(counter, n_items) : 0u; n_items = 0u; }
  __syncthreads();
  for (uint64_t s = start; s < t.asize; s += stride) {
    const uint32_t k = items_of(s);
    if (k == 0u) { continue; }
    const uint32_t at = base + atomicAdd(&n_items, k);
    join_item it;
    it.begin = (uint32_t)t.offsets[s]; it.na = t.cnt_a[s]; it.nb = t.cnt_b[s];
    if ((uint64_t)at + k > cap) { t.flags[kJoinItemOverflow] = 1u; }
    for (uint32_t j = 0; j < k; ++j) { it.tile = j; if ((uint64_t)at + j < cap) { t.items[at + j] = it; } }
  }
}

// ---- a wave's found pairs, staged in LDS ------------------------------------------------------------------------------
// One global atomic per flush instead of one per ballot (a single address takes ~90 atomics a microsecond).  The kernel
// declares  __shared__ unsigned long long stage[waves][kPairStage];  and every wave builds a PairStage on its row.
constexpr uint32_t kPairStage = 256;

struct PairStage {
  unsigned long long * slice;          // this wave's row
  unsigned long long * pairs;          // the global list, room for `cap`: what lies past it is counted, not written
  unsigned long long * counter;
  uint64_t cap;
  uint32_t fill;
  int lane;
  uint64_t lane_lt;

  __device__ __forceinline__ PairStage(unsigned long long (*rows)[kPairStage], unsigned long long * pairs_, unsigned long long * counter_, uint64_t cap_)
      : slice(rows[threadIdx.x >> 6]), pairs(pairs_), counter(counter_), cap(cap_), fill(0u), lane((int)(threadIdx.x & 63u)),
        lane_lt((1ull << (threadIdx.x & 63u)) - 1ull) {}

  __device__ __forceinline__ void flush() {
    wave_lds_sync();
    unsigned long long base = 0;
    if (lane == 0) { base = atomicAdd(counter, (unsigned long long)fill); }
    base = swa_shfl_u64(base, 0);
    for (uint32_t i = (uint32_t)lane; i < fill; i += 64u) { if (base + i < cap) { pairs[base + i] = slice[i]; } }
    fill = 0u;
    wave_lds_sync();
  }
  // all lanes of the wave call it; the lanes with `take` add their value
  __device__ __forceinline__ void push(bool take, unsigned long long value) {
    const uint64_t m = __ballot(take);
    if (m != 0ull) {
      if (take) { slice[fill + (uint32_t)__popcll(m & lane_lt)] = value; }
      fill += (uint32_t)__popcll(m);
      if (fill > kPairStage - 64u) { flush(); }
    }
  }
  __device__ __forceinline__ void finish() { if (fill != 0u) { flush(); } }
};

// ---- host -------------------------------------------------------------------------------------------------------------
// room for a table of up to `asize` slots over n amplicons with up to per_a keys a creator; the caps are the route's
inline int join_reserve(swa_ctx * ctx, uint64_t asize, uint32_t n, uint32_t per_a, uint64_t member_cap, uint32_t item_cap) {
  SWA_TRY(swa_reserve(ctx, ctx->d_fkeys, asize * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_fcnt, (asize * 5 + 4) * sizeof(uint32_t)));                // (the scan reads one entry past `tot`)
  SWA_TRY(swa_reserve(ctx, ctx->d_foff, (asize + 2) * sizeof(uint64_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_fslot, (uint64_t)n * (per_a + 1u) * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_fmembers, member_cap * sizeof(uint32_t)));
  SWA_TRY(swa_reserve(ctx, ctx->d_fitems, (uint64_t)item_cap * sizeof(join_item)));
  return SWA_OK;
}

inline JoinTable join_table(swa_ctx * ctx, uint64_t asize, uint32_t n, uint32_t per_a) {
  JoinTable t{};
  t.keys = static_cast<unsigned long long *>(ctx->d_fkeys.ptr);
  t.cnt_a = static_cast<uint32_t *>(ctx->d_fcnt.ptr);
  t.cnt_b = t.cnt_a + asize; t.cur_a = t.cnt_b + asize; t.cur_b = t.cur_a + asize; t.tot = t.cur_b + asize;
  t.offsets = static_cast<uint64_t *>(ctx->d_foff.ptr);
  t.aslot = static_cast<uint32_t *>(ctx->d_fslot.ptr);
  t.bslot = t.aslot + (uint64_t)n * per_a;
  t.members = static_cast<uint32_t *>(ctx->d_fmembers.ptr);
  t.items = static_cast<join_item *>(ctx->d_fitems.ptr);
  t.flags = swa_status(ctx)->flags + kFlagJoin;
  t.asize = asize; t.n = n; t.per_a = per_a;
  return t;
}

// clear -> key_kernels(grid, block) (the route's creators, then its joiners) -> totals -> scan(t) -> scatter -> items on
// ctx->stream.  scan(t) enqueues the exclusive scan of t.tot[0, asize) into t.offsets (64-bit sums) and returns SWA_OK or
// an error.  *counter (zeroed by the route) += the items made, at t.items from entry 0 on.
template <class Shape, class KeyKernels, class Scan>
int join_run(swa_ctx * ctx, const JoinTable & t, uint32_t min_product, uint32_t * counter, uint32_t item_cap, KeyKernels && key_kernels,
             Scan && scan) {
  const dim3 gn(swa_grid256(ctx, t.n)), ga(swa_grid256(ctx, t.asize)), b(256);
  hipLaunchKernelGGL(k_join_clear, ga, b, 0, ctx->stream, t);
  key_kernels(gn, b);
  hipLaunchKernelGGL(k_join_totals, ga, b, 0, ctx->stream, t, min_product);
  SWA_TRY(scan(t));
  hipLaunchKernelGGL(k_join_scatter, gn, b, 0, ctx->stream, t);
  hipLaunchKernelGGL(k_join_items<Shape>, ga, b, 0, ctx->stream, t, counter, item_cap);
  return SWA_OK;
}

// After the route's pair kernels: the first `ngot` words of its counters and the table's flags, on the host.  Neither
// overflow can happen (load <= 0.5; the routes' item caps hold whatever the groups: tests/test_fastidious_identity.py,
// tests/test_pair_identity.py), so either is an error with the route's message.
inline int join_status(swa_ctx * ctx, const JoinTable & t, const unsigned long long * counters, uint32_t ngot, uint64_t * got,
                       const char * key_overflow, const char * item_overflow) {
  uint32_t fl[kJoinItemCount] = {};
  SWA_HIP(ctx, hipMemcpyAsync(got, counters, ngot * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipMemcpyAsync(fl, t.flags, sizeof(fl), hipMemcpyDeviceToHost, ctx->stream));
  SWA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (fl[kJoinKeyOverflow] != 0) { return swa_fail_msg(ctx, SWA_E_DEVICE, key_overflow); }
  if (fl[kJoinItemOverflow] != 0) { return swa_fail_msg(ctx, SWA_E_INTERNAL, item_overflow); }
  return SWA_OK;
}
