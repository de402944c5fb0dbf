// uclust_multi.cpp — the -u writers on several GPUs (seam B5): the writers of cluster_d1.cpp and cluster_dn.cpp with every
// chunk's alignments divided among the ranks of a swa_multi (swa_multi_nw_batch).  The calls that name swa_multi_* live
// here, apart from the writers: cluster_d1.cpp also links into a program of its own without the device library.
#include "hostdb.h"
#include "uclust_gpu.h"

namespace {

swa_uclust_aligner on_ranks(swa_multi * multi) {
  swa_uclust_aligner a;
  a.handle = multi;
  a.batch = [](void * h, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t npairs, const uint32_t * d_ids, const uint32_t * q_ids,
               uint32_t * diffs, uint32_t * columns, uint64_t * cigar_end, char * cigar, uint64_t cigar_cap, uint64_t * cigar_total) {
    return swa_multi_nw_batch(static_cast<swa_multi *>(h), mismatch, gapopen, gapextend, npairs, d_ids, q_ids, diffs, columns, cigar_end, cigar,
                              cigar_cap, cigar_total);
  };
  a.totals = [](void * h, uint64_t * out4) { return swa_multi_nw_batch_totals(static_cast<swa_multi *>(h), out4); };   // (the sums over the ranks)
  a.tiers = [](void * h, uint64_t * out8) { return swa_multi_nw_batch_tiers(static_cast<swa_multi *>(h), out8); };
  a.text_full = [](void * h, uint64_t * out1) { return swa_multi_nw_batch_text_full(static_cast<swa_multi *>(h), out1); };
  return a;
}

}  // namespace

extern "C" int swa_d1_write_uclust_multi(swa_multi * multi, const swa_d1_result * res, const swa_hostdb * db, const char * path, int usearch,
                                         int64_t append_abundance, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend) {
  return swa_d1_write_uclust_with(on_ranks(multi), res, db, path, usearch, append_abundance, mismatch, gapopen, gapextend);
}

extern "C" int swa_dn_write_uclust_multi(swa_multi * multi, const swa_dn_result * res, const swa_hostdb * db, const char * path, int usearch,
                                         int64_t append_abundance) {
  return swa_dn_write_uclust_with(on_ranks(multi), res, db, path, usearch, append_abundance);
}
