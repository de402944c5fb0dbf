// host_tables.cpp — the small constant tables of the d=1 path, generated on the host
// and uploaded once.  They are made bit-identical to the reference's so that every
// intermediate of the GPU path (sequence hashes, variant hashes, Bloom bitmap) can be
// compared word for word with the oracle; no output of the program depends on them.
#include "swa_internal.h"

#include <algorithm>
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

// ---- the dispatch of the --fastidious pass (fastidious.hip: fast_plan; d1_fast.inc) -----------------------------------
// Pure host arithmetic, no HIP call: what fastidious.hip launches and what swa_d1_fastidious_plan reports have this one source.

// LDS of k_fast_count for `waves` waves per block: the Zobrist table of longest + 2 positions, and per wave two sequence
// copies (words + 3) and the set; 0 = does not fit 160 KB
size_t swa_fast_count_lds(uint32_t longest, uint32_t slots, int waves) {
  const uint32_t maxwords = (longest + 31u) >> 5;
  const size_t zlen = (size_t)longest + 2u;                  // = ctx->zobrist_len (swa_prepare_hashing) when longest is the database's
  const size_t bytes = sizeof(uint64_t) * (4ull * zlen + (size_t)waves * (2ull * (maxwords + 3u) + slots));
  return bytes <= 160u * 1024u ? bytes : 0;
}

// slots of a wave's set: a power of two >= 1.5 * (7 longest + 4), the microvariants of the longest sequence at load 2/3
uint32_t swa_fast_count_slots(uint32_t longest) {
  uint32_t slots = 1024;
  const uint64_t v = 7ull * longest + 4ull;
  while (slots < v + v / 2 && slots < (1u << 31)) { slots <<= 1; }   // (2^31 slots fit no LDS: the search ends there for any length)
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

// LDS of k_fast_count_sites_words for `waves` waves per block: per wave two sequence copies (words + 3), nothing else;
// 0 = does not fit 160 KB
size_t swa_fast_sites_lds(uint32_t longest, int waves) {
  const size_t maxwords = ((size_t)longest + 31u) >> 5;
  const size_t bytes = sizeof(uint64_t) * (size_t)waves * 2ull * (maxwords + 3u);
  return bytes <= 160u * 1024u ? bytes : 0;
}

// the longest sequence k_fast_count_sites_words serves (one wave per block): 10 237 words = 327 584 nt
uint32_t swa_fast_sites_cap() {
  static const uint32_t cap = [] {
    uint32_t words = 1;
    while (swa_fast_sites_lds(32u * (words + 1u), 1) != 0) { ++words; }
    return 32u * words;
  }();
  return cap;
}

// the cap of SWA_FAST_LONG=pairs: the derived one, or a lower one from the test hook (counted only within [swa_fast_cap(),
// the derived cap])
uint32_t swa_fast_sites_cap_in_effect(uint32_t sites_cap) {
  return sites_cap >= swa_fast_cap() && sites_cap <= swa_fast_sites_cap() ? sites_cap : swa_fast_sites_cap();
}

static void plan_count_sites_words(swa_fast_plan & p) {
  p.count_words = true;
  p.count_w = 0;
  p.count_waves = 0;
  p.slots = 0;
  for (int w : {4, 2, 1}) { if (p.count_waves == 0 && swa_fast_sites_lds(p.served, w) != 0) { p.count_waves = w; } }
  p.count_lds = p.count_waves != 0 ? swa_fast_sites_lds(p.served, p.count_waves) : 0;
}

swa_fast_plan swa_fast_plan_modes(uint32_t longest, uint32_t pair_longest, int long_mode, bool bloom, bool words, bool count_sites,
                                  uint32_t sites_cap) {
  swa_fast_plan p{};
  const uint32_t cap = swa_fast_cap();
  p.max_len = 0xFFFFFFFFu;
  // SWA_FAST_LONG=pairs: only where the longest sequence alone would send every pair to the Bloom route.  Every sequence
  // up to C stays on the pair route; where longer ones exist, the division of the split at C instead of cap.
  if (long_mode == 2 && !bloom && longest > cap) {
    const uint32_t C = swa_fast_sites_cap_in_effect(sites_cap);
    const uint32_t served = longest <= C ? longest : pair_longest;
    if (served >= SWA_FAST_MIN_LEN && served <= C) {
      p.long_mode = 2;
      p.served = served;
      p.max_len = longest <= C ? 0xFFFFFFFFu : C;
      p.pair_route = true;
      p.pair_w = 0;                                           // k_fast_pairs, which walks the packed sequences
      plan_count_sites_words(p);
      p.zobrist_lds = 4ull * ((size_t)longest + 2u) * sizeof(uint64_t) <= SWA_MAX_ZOBRIST_LDS;
      return p;
    }
  }
  // the division at the long end (SWA_FAST_LONG=split): only where the longest sequence alone would send every pair to the
  // Bloom route, and where some pair is left for the pair route
  p.split = long_mode == 1 && !bloom && longest > cap && pair_longest >= SWA_FAST_MIN_LEN && pair_longest <= cap;
  p.long_mode = p.split ? 1 : 0;
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
  // SWA_FAST_COUNT=sites: k_fast_count_sites_words where k_fast_count would run
  if (count_sites && p.pair_route && p.count_w == 0) { plan_count_sites_words(p); }
  // the Bloom route stages the whole Zobrist table: by the longest sequence of the database, split or not
  p.zobrist_lds = 4ull * ((size_t)longest + 2u) * sizeof(uint64_t) <= SWA_MAX_ZOBRIST_LDS;
  return p;
}

swa_fast_plan swa_fast_plan_for(uint32_t longest, uint32_t pair_longest, bool split, bool bloom, bool words) {
  return swa_fast_plan_modes(longest, pair_longest, split ? 1 : 0, bloom, words, false, 0u);
}

void swa_fast_plan_report(const swa_fast_plan & p, uint32_t out[8]) {
  const bool set = p.pair_route && p.count_w == 0 && !p.count_words;   // k_fast_count runs
  const bool staged = p.pair_route && p.count_words;                    // k_fast_count_sites_words runs
  out[0] = p.pair_route ? 1u : 0u;
  out[1] = p.pair_route ? (uint32_t)p.pair_w : 0u;
  out[2] = staged ? 1u : (p.pair_route ? (uint32_t)p.count_w : 0u);
  out[3] = set || staged ? (uint32_t)p.count_waves : 0u;
  out[4] = set ? p.slots : 0u;
  out[5] = set || staged ? (uint32_t)p.count_lds : 0u;
  out[6] = p.zobrist_lds ? 1u : 0u;
  out[7] = SWA_FAST_MIN_LEN;
}

extern "C" int swa_d1_fastidious_plan_for(uint32_t longest, uint32_t pair_longest, int split, int bloom, int words, uint32_t out[8]) {
  if (out == nullptr || longest == 0) { return SWA_E_ARG; }
  swa_fast_plan_report(swa_fast_plan_for(longest, pair_longest, split != 0, bloom != 0, words != 0), out);
  return SWA_OK;
}

extern "C" int swa_d1_fastidious_plan_modes(uint32_t longest, uint32_t pair_longest, int long_mode, int bloom, int words,
                                            int count_sites, uint32_t sites_cap, uint32_t out[8]) {
  if (out == nullptr || longest == 0 || long_mode < 0 || long_mode > 2) { return SWA_E_ARG; }
  swa_fast_plan_report(swa_fast_plan_modes(longest, pair_longest, long_mode, bloom != 0, words != 0, count_sites != 0, sites_cap), out);
  return SWA_OK;
}

extern "C" uint32_t swa_d1_fastidious_sites_cap(uint32_t sites_cap) { return swa_fast_sites_cap_in_effect(sites_cap); }

// ---- the forms of the key partition and of the link partition (d1.hip: build_stream_index; d1_part.hip: csr_from_chunks) ----------
// Pure host arithmetic, no HIP call: what swa_part_run (d1_part.hip) launches and what swa_d1_part_plan reports have this one source.

// total_bits spread over as few levels of at most max_bits as hold them, the earlier levels one bit wider where it does not divide
swa_part_levels swa_plan_levels(uint32_t total_bits, uint32_t max_bits) {
  swa_part_levels p{};
  p.total = std::max(1u, total_bits);
  p.levels = (p.total + max_bits - 1) / max_bits;
  for (uint32_t l = 0; l < p.levels; ++l) { p.bits[l] = p.total / p.levels + (l < p.total % p.levels ? 1u : 0u); }
  return p;
}

// buckets of ~10 000 records for k_group1: ONE partition level of up to 10 bits at 10 M amplicons
swa_part_plan swa_part_plan_for(uint64_t records, uint32_t extra_bits, bool routed, uint32_t forced_bits) {
  const uint32_t most = 3 * SWA_PART_MAX_BITS;
  uint32_t total_bits = 1;
  if (forced_bits != 0) { total_bits = std::min(forced_bits, most); }
  else { while ((records >> total_bits) > SWA_G1_TARGET && total_bits < most) { ++total_bits; } }
  total_bits = std::min<uint32_t>(total_bits + extra_bits, most);
  swa_part_plan p{};
  // (one level of up to 1024 bins, or levels of up to 512: the partition has 1024-bin forms for one level only)
  p.lv = total_bits <= SWA_PART_WIDE_BITS ? swa_plan_levels(total_bits, SWA_PART_WIDE_BITS) : swa_plan_levels(total_bits);
  // the first partition level's histogram is taken on the way (one read pass over the records less: 0.07 ms at 10 M);
  // not for routed id lists (their length is the device's to know)
  p.keys_hist = !routed;
  p.wide = total_bits > SWA_PART_MAX_BITS && p.lv.levels == 1;
  // tiles of 2048 records for 512 bins; one level of 1024 bins: 4096 (or the flat count array — bins x tiles — and the 16-byte
  // runs a tile leaves per bin cost more than the saved level: 0.56 -> 0.43 ms at 10 M amplicons) — or 8192 when k_keys takes
  // the histogram (k_part_hist holds 4096 a workgroup): a tile then leaves runs of 64 bytes per bin, whole lines (key
  // partition 0.239 -> 0.225 ms at 10 M)
  p.tile = p.wide ? (p.keys_hist ? 8192u : 4096u) : 2048u;
  p.lists_inline = swa_lists_inline(1ull << p.lv.total);
  return p;
}

bool swa_lists_inline(uint64_t buckets) { return buckets <= SWA_LISTS_INLINE_BUCKETS; }

extern "C" int swa_d1_lists_form_for(uint64_t buckets) { return buckets == 0 ? -1 : (swa_lists_inline(buckets) ? 1 : 0); }

void swa_part_plan_report(const swa_part_plan & p, uint32_t out[8]) {
  out[0] = p.lv.total; out[1] = p.lv.levels;
  for (uint32_t l = 0; l < 3; ++l) { out[2 + l] = l < p.lv.levels ? p.lv.bits[l] : 0u; }
  out[5] = p.tile; out[6] = p.keys_hist ? 1u : 0u; out[7] = p.wide ? 1u : 0u;
}

extern "C" int swa_d1_part_plan_for(uint64_t records, uint32_t extra_bits, int routed, uint32_t forced_bits, uint32_t out[8]) {
  if (out == nullptr || forced_bits > 3 * SWA_PART_MAX_BITS) { return SWA_E_ARG; }
  swa_part_plan_report(swa_part_plan_for(records, extra_bits, routed != 0, forced_bits), out);
  return SWA_OK;
}

// The links are partitioned by the top bits of their source until a bucket holds 2^r consecutive sources: r = 8 (fewer
// for a handful of sources), 9 where that saves a third level
swa_csr_plan swa_csr_plan_for(uint32_t count) {
  swa_csr_plan p{};
  p.nbits = 1;
  while (p.nbits < 32 && ((uint64_t)1 << p.nbits) < count) { ++p.nbits; }
  p.r = std::min<uint32_t>(8, p.nbits - 1);
  if (p.nbits - p.r > 2 * SWA_PART_MAX_BITS) { p.r = std::min<uint32_t>(SWA_CSR_MAX_R, p.nbits - 2 * SWA_PART_MAX_BITS); }
  p.lv = swa_plan_levels(p.nbits - p.r);
  return p;
}

extern "C" int swa_d1_csr_plan_for(uint32_t count, uint32_t out[6]) {
  if (out == nullptr || count == 0) { return SWA_E_ARG; }
  const swa_csr_plan p = swa_csr_plan_for(count);
  out[0] = p.nbits; out[1] = p.r; out[2] = p.lv.levels;
  for (uint32_t l = 0; l < 3; ++l) { out[3 + l] = l < p.lv.levels ? p.lv.bits[l] : 0u; }
  return SWA_OK;
}
