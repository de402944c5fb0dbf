// key_ops.inc — the empty marks and the two helpers every grouping by 63-bit window keys shares: the anchor indexes of the
// d = 1 step (d1.hip), the grouped join (group_join.inc) of the --fastidious pair route (fastidious.hip) and of the d >= 2
// graph route (dn_graph.hip).  Included inside each file's anonymous namespace; defines no kernel.

constexpr uint32_t kEmpty = SWA_NO_AMPLICON;
constexpr uint64_t kKeyEmpty = ~0ull;

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull; x ^= x >> 33;
  return x;
}

// 32 nucleotides from position pos on (may read the following word: the database ends in two zero words)
__device__ __forceinline__ uint64_t window32(const uint64_t * seq, uint32_t pos) {
  const uint32_t w = pos >> 5, sh = (pos & 31u) << 1;
  uint64_t v = seq[w] >> sh;
  if (sh != 0u) { v |= seq[w + 1] << (64u - sh); }
  return v;
}
