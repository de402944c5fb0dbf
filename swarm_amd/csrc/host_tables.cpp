// host_tables.cpp — the small constant tables of the d=1 path, generated on the host
// and uploaded once.  They are made bit-identical to the reference's so that every
// intermediate of the GPU path (sequence hashes, variant hashes, Bloom bitmap) can be
// compared word for word with the oracle; no output of the program depends on them.
#include "swa_internal.h"

#include <cmath>
#include <random>

// The reference draws from `static std::mt19937_64 rand_64(1)`, one private instance
// per translation unit (src/utils/pseudo_rng.h:30-31), so each table below starts from
// a fresh generator seeded with 1.

// src/zobrist.cc:49-80 — 4 values per position; each value folds four draws with
// 16-bit left shifts in between.
void swa_zobrist_table(uint32_t zobrist_len, std::vector<uint64_t> & tab) {
  std::mt19937_64 gen(1);
  tab.resize(4ull * zobrist_len);
  for (auto & v : tab) {
    uint64_t x = gen();
    for (int k = 0; k < 3; ++k) { x = (x << 16) ^ gen(); }
    v = x;
  }
}

// src/bloompat.cc:74-90 (count 1024, k 8) and src/bloomflex.cc:72-88 (count 65536,
// k = number of hash functions): k distinct bit positions per pattern, redrawn on
// collision.
void swa_bloom_patterns(uint32_t count, uint32_t k, std::vector<uint64_t> & pat) {
  std::mt19937_64 gen(1);
  pat.assign(count, 0);
  for (auto & p : pat) {
    for (uint32_t j = 0; j < k; ++j) {
      uint64_t bit;
      do { bit = 1ull << (gen() & 63u); } while ((p & bit) != 0);
      p |= bit;
    }
  }
}

// src/utils/hashtable_size.cc:29-42 — smallest power of two >= the INTEGER quotient
// 10*(n+1)/7, evaluated through log/ceil/pow in doubles like the reference.
uint64_t swa_hashtable_size(uint64_t n) {
  const uint64_t quotient = 10ull * (n + 1ull) / 7ull;
  return static_cast<uint64_t>(std::pow(2.0, std::ceil(std::log(static_cast<double>(quotient)) / std::log(2.0))));
}

// ---- the dispatch of the --fastidious pass (d1.hip: fast_plan; d1_fast.inc) -------------------------------------------
// Pure host arithmetic, no HIP call: what d1.hip launches and what swa_d1_fastidious_plan reports have this one source.

// LDS of k_fast_count for `waves` waves per block: the Zobrist table of longest + 2 positions, and per wave two sequence
// copies (words + 3) and the set; 0 = does not fit 160 KB
size_t swa_fast_count_lds(uint32_t longest, uint32_t slots, int waves) {
  const uint32_t maxwords = (longest + 31u) >> 5;
  const size_t zlen = (size_t)longest + 2u;                  // = ctx->zobrist_len (prepare_hashing) when longest is the database's
  const size_t bytes = sizeof(uint64_t) * (4ull * zlen + (size_t)waves * (2ull * (maxwords + 3u) + slots));
  return bytes <= 160u * 1024u ? bytes : 0;
}

// slots of a wave's set: a power of two >= 1.5 * (7 longest + 4), the microvariants of the longest sequence at load 2/3
uint32_t swa_fast_count_slots(uint32_t longest) {
  uint32_t slots = 1024;
  const uint64_t v = 7ull * longest + 4ull;
  while (slots < v + v / 2) { slots <<= 1; }
  return slots;
}

// the longest sequence k_fast_count still serves (one wave per block): 1004.  (The LDS grows with the length, so the
// first length that does not fit ends the search.)
uint32_t swa_fast_cap() {
  static const uint32_t cap = [] {
    uint32_t L = 0;
    while (swa_fast_count_lds(L + 1u, swa_fast_count_slots(L + 1u), 1) != 0) { ++L; }
    return L;
  }();
  return cap;
}

swa_fast_plan swa_fast_plan_for(uint32_t longest, uint32_t pair_longest, bool split, bool bloom, bool words) {
  swa_fast_plan p{};
  const uint32_t cap = swa_fast_cap();
  // the division at the long end (SWA_FAST_LONG=split): only where the longest sequence alone would send every pair to the
  // Bloom route, and where some pair is left for the pair route
  p.split = split && !bloom && longest > cap && pair_longest >= SWA_FAST_MIN_LEN && pair_longest <= cap;
  const uint32_t served = p.split ? pair_longest : longest;   // the longest sequence the pair route has to hold
  p.served = served;
  p.max_len = p.split ? cap : 0xFFFFFFFFu;
  // which pairs the pair route can take: k_fast_count's LDS set must hold the microvariants of the longest sequence
  p.slots = swa_fast_count_slots(served);
  for (int w : {4, 2, 1}) { if (p.count_waves == 0 && swa_fast_count_lds(served, p.slots, w) != 0) { p.count_waves = w; } }
  p.count_lds = p.count_waves != 0 ? swa_fast_count_lds(served, p.slots, p.count_waves) : 0;
  p.pair_route = p.count_waves != 0 && served >= SWA_FAST_MIN_LEN && !bloom;
  // pairs on the amplicon lines, sequences in registers (the register kernels exist for 5, 8 and 13 words: sequences up
  // to 416 nt, which 128-byte lines hold); 0: k_fast_pairs, which walks the packed sequences.  Under the split always
  // the latter: the lines' width, and whether they exist, follow the whole database.
  p.pair_w = (words || p.split) ? 0 : (served <= 160u ? 5 : (served <= 256u ? 8 : (served <= 416u ? 13 : 0)));
  p.count_w = served <= 159u ? 5 : (served <= 255u ? 8 : 0);
  // the Bloom route stages the whole Zobrist table: by the longest sequence of the database, split or not
  p.zobrist_lds = 4ull * ((size_t)longest + 2u) * sizeof(uint64_t) <= SWA_MAX_ZOBRIST_LDS;
  return p;
}

void swa_fast_plan_report(const swa_fast_plan & p, uint32_t out[8]) {
  const bool set = p.pair_route && p.count_w == 0;           // k_fast_count runs
  out[0] = p.pair_route ? 1u : 0u;
  out[1] = p.pair_route ? (uint32_t)p.pair_w : 0u;
  out[2] = p.pair_route ? (uint32_t)p.count_w : 0u;
  out[3] = set ? (uint32_t)p.count_waves : 0u;
  out[4] = set ? p.slots : 0u;
  out[5] = set ? (uint32_t)p.count_lds : 0u;
  out[6] = p.zobrist_lds ? 1u : 0u;
  out[7] = SWA_FAST_MIN_LEN;
}

extern "C" int swa_d1_fastidious_plan_for(uint32_t longest, uint32_t pair_longest, int split, int bloom, int words, uint32_t out[8]) {
  if (out == nullptr || longest == 0) { return SWA_E_ARG; }
  swa_fast_plan_report(swa_fast_plan_for(longest, pair_longest, split != 0, bloom != 0, words != 0), out);
  return SWA_OK;
}
