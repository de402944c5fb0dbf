// uclust_gpu.h — the -u writers on the GPU (seam B5): the H lines' pairs collected in printing order, aligned by
// swa_nw_batch in chunks of bounded size, and formatted by the multi-threaded formatter while the GPU aligns the next
// chunk.  The d = 1 and d >= 2 writers differ only in how they walk their swarms; who aligns a chunk — one context, or
// the ranks of a swa_multi among which swa_multi_nw_batch divides it (uclust_multi.cpp) — is the aligner they are given.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <thread>
#include <vector>

#include "hostdb.h"
#include "out.h"

struct swa_uclust_chunk {
  size_t begin = 0, end = 0;          // swarms [begin, end)
  std::vector<uint64_t> first;        // per swarm of the chunk: its first pair; one more entry at the end
  std::vector<uint32_t> d, q;         // (member, seed) of every H line, in printing order
  std::vector<uint32_t> diffs, columns;
  std::vector<uint64_t> cigar_end;
  std::unique_ptr<char[]> cigar;
  uint64_t cigar_cap = 0;             // sum of dl + ql: no CIGAR is longer than its alignment
  int rc = SWA_OK;
};

// Who aligns a chunk: swa_nw_batch and its three counter calls, or calls with their arguments and results, on `handle`.
struct swa_uclust_aligner {
  void * handle = nullptr;            // NULL only for a result without H lines
  int (*batch)(void * handle, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t npairs, const uint32_t * d_ids,
               const uint32_t * q_ids, uint32_t * diffs, uint32_t * columns, uint64_t * cigar_end, char * cigar, uint64_t cigar_cap,
               uint64_t * cigar_total) = nullptr;
  int (*totals)(void * handle, uint64_t * out4) = nullptr;
  int (*tiers)(void * handle, uint64_t * out8) = nullptr;
  int (*text_full)(void * handle, uint64_t * out1) = nullptr;
};

// one context: the _gpu writers
inline swa_uclust_aligner swa_uclust_on_ctx(swa_ctx * ctx) {
  swa_uclust_aligner a;
  a.handle = ctx;
  a.batch = [](void * h, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t npairs, const uint32_t * d_ids, const uint32_t * q_ids,
               uint32_t * diffs, uint32_t * columns, uint64_t * cigar_end, char * cigar, uint64_t cigar_cap, uint64_t * cigar_total) {
    return swa_nw_batch(static_cast<swa_ctx *>(h), mismatch, gapopen, gapextend, npairs, d_ids, q_ids, diffs, columns, cigar_end, cigar, cigar_cap,
                        cigar_total);
  };
  a.totals = [](void * h, uint64_t * out4) { return swa_nw_batch_totals(static_cast<swa_ctx *>(h), out4); };
  a.tiers = [](void * h, uint64_t * out8) { return swa_nw_batch_tiers(static_cast<swa_ctx *>(h), out8); };
  a.text_full = [](void * h, uint64_t * out1) { return swa_nw_batch_text_full(static_cast<swa_ctx *>(h), out1); };
  return a;
}

// The writers proper (cluster_d1.cpp, cluster_dn.cpp), behind swa_d1_write_uclust_gpu / _multi and swa_dn_write_uclust_gpu /
// _multi: the arguments of the _gpu writers, the aligner in the context's place.
int swa_d1_write_uclust_with(const swa_uclust_aligner & aligner, const swa_d1_result * res, const swa_hostdb * db, const char * path, int usearch,
                             int64_t append_abundance, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend);
int swa_dn_write_uclust_with(const swa_uclust_aligner & aligner, const swa_dn_result * res, const swa_hostdb * db, const char * path, int usearch,
                             int64_t append_abundance);

// pairs per chunk: SWA_NW_CHUNK (a test hook: many chunks on small inputs), else 2^20
inline uint64_t swa_uclust_chunk_pairs() {
  const char * e = std::getenv("SWA_NW_CHUNK");
  const long long v = e != nullptr ? std::atoll(e) : 0;
  return v > 0 ? (uint64_t)v : (uint64_t)1 << 20;
}

// collect(k, push): push(member, seed) for every H line of swarm k, in printing order.  weight(k): what swarm k costs to
// format.  format(sink, k, chunk, p): prints swarm k, whose first H line is pair p of the chunk.
template <class Collect, class Weight, class Format>
int swa_uclust_gpu(const swa_uclust_aligner & aligner, const swa_hostdb * db, BufOut & o, size_t nswarms, bool parallel, uint64_t mismatch,
                   uint64_t gapopen, uint64_t gapextend, Collect && collect, Weight && weight, Format && format) {
  const uint64_t cap = swa_uclust_chunk_pairs();
  auto fill = [&](swa_uclust_chunk & c, size_t from) {
    c.begin = from;
    c.first.clear(); c.d.clear(); c.q.clear();
    c.cigar_cap = 0;
    c.rc = SWA_OK;
    size_t k = from;
    for (; k < nswarms && c.d.size() < cap; ++k) {
      c.first.push_back(c.d.size());
      collect(k, [&](uint32_t member, uint32_t seed) {
        c.d.push_back(member);
        c.q.push_back(seed);
        c.cigar_cap += (uint64_t)db->seqlen[member] + db->seqlen[seed];
      });
    }
    c.first.push_back(c.d.size());
    c.end = k;
  };
  uint64_t tiers[4] = {}, all[8] = {}, text_full = 0;
  auto align = [&](swa_uclust_chunk & c) {
    const size_t n = c.d.size();
    c.diffs.resize(n); c.columns.resize(n); c.cigar_end.resize(n);
    c.cigar.reset(new char[std::max<uint64_t>(c.cigar_cap, 1)]);
    uint64_t total = 0;
    // (a result without H lines needs no context, and the command line has none for an empty input)
    if (n == 0) { c.rc = SWA_OK; return; }
    if (aligner.handle == nullptr) { c.rc = SWA_E_ARG; return; }
    c.rc = aligner.batch(aligner.handle, mismatch, gapopen, gapextend, n, c.d.data(), c.q.data(), c.diffs.data(), c.columns.data(),
                         c.cigar_end.data(), c.cigar.get(), c.cigar_cap, &total);
    uint64_t t[4] = {};
    if (c.rc == SWA_OK && aligner.totals(aligner.handle, t) == SWA_OK) { for (int i = 0; i < 4; ++i) { tiers[i] += t[i]; } }
    uint64_t t8[8] = {}, full = 0;
    if (c.rc == SWA_OK && aligner.tiers(aligner.handle, t8) == SWA_OK) { for (int i = 0; i < 8; ++i) { all[i] += t8[i]; } }
    if (c.rc == SWA_OK && aligner.text_full(aligner.handle, &full) == SWA_OK) { text_full += full; }
  };
  swa_uclust_chunk cur, next;
  fill(cur, 0);
  align(cur);
  while (cur.rc == SWA_OK && cur.begin < cur.end) {
    fill(next, cur.end);
    std::thread gpu;
    if (next.begin < next.end) { gpu = std::thread([&] { align(next); }); }
    const swa_uclust_chunk & c = cur;
    swa_format_in_weighted_pieces(o, c.end - c.begin, parallel, [&](size_t i) { return weight(c.begin + i); },
                                  [&](BufOut & sink, size_t b, size_t e) {
                                    for (size_t i = b; i < e; ++i) { format(sink, c.begin + i, c, c.first[i]); }
                                  });
    if (gpu.joinable()) { gpu.join(); }
    std::swap(cur, next);
  }
  if (std::getenv("SWARM_AMD_TIMING") != nullptr) {      // (the CLI's milestones: where the pairs were aligned)
    std::fprintf(stderr, "[nw] pairs by band half-width 6 / 14 / 30 / host: %llu %llu %llu %llu\n", (unsigned long long)tiers[0],
                 (unsigned long long)tiers[1], (unsigned long long)tiers[2], (unsigned long long)tiers[3]);
    std::fprintf(stderr, "[nw] pairs by tier, LDS 6 / 14 / 30, wide 30 / 62 / 126 / 254, host:");
    for (int i = 0; i < 8; ++i) { std::fprintf(stderr, " %llu", (unsigned long long)all[i]); }
    std::fprintf(stderr, "; of the host's, text buffer full: %llu\n", (unsigned long long)text_full);
  }
  return cur.rc;
}

// the CIGAR of pair p of a chunk
inline const char * swa_uclust_cigar(const swa_uclust_chunk & c, uint64_t p, size_t * len) {
  const uint64_t from = p == 0 ? 0 : c.cigar_end[p - 1];
  *len = (size_t)(c.cigar_end[p] - from);
  return c.cigar.get() + from;
}
