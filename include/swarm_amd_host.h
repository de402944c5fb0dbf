/*
 * swarm_amd_host.h — host-side C ABI of libswarm_amd.so: the pieces either side of the
 * GPU path that the reference keeps in plain host C++ (SURVEY.md §8f "next" rows):
 * FASTA ingest into the packed database, and the greedy single-linkage clustering +
 * writers that consume the GPU-returned neighbour lists.  No GPU is needed for any
 * function in this header.
 */
#ifndef SWARM_AMD_HOST_H
#define SWARM_AMD_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "swarm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct swa_hostdb swa_hostdb;

/* Replaces db_read (src/db.h:29-33, src/db.cc:432-803).  path "-" = stdin.
   usearch_abundance = -z; append_abundance = -a (0 = off); check_duplicate_sequences
   != 0 reproduces the d > 1 duplicate check of src/db.cc:763-790.
   On failure *out still receives a handle whose swa_hostdb_error() is the reference's
   fatal() text (the caller prints it and exits 1). */
int swa_hostdb_read_fasta(const char * path, int usearch_abundance, int64_t append_abundance,
                          int check_duplicate_sequences, swa_hostdb ** out);
/* The same with a notice as soon as the packed words are final (right after the parse, before the sort): on_words(user,
   pools, words per pool, pools) runs on the calling thread; the pools stay where they are for the life of the handle
   (they are the database's storage), so a GPU context coming up on another thread can start swa_db_stage_words on
   them while this call sorts.  on_words may be NULL. */
typedef void (*swa_words_ready_fn)(void * user, const uint64_t * const * piece_words, const uint64_t * piece_word_count, uint32_t pieces);
int swa_hostdb_read_fasta_staged(const char * path, int usearch_abundance, int64_t append_abundance, int check_duplicate_sequences,
                                 swa_words_ready_fn on_words, void * user, swa_hostdb ** out);
void swa_hostdb_free(swa_hostdb * db);
const char * swa_hostdb_error(const swa_hostdb * db);
/* host pointers into the handle (valid until swa_hostdb_free).  swa_hostdb_view: the packed sequences contiguous in db
   order — gathered on the host the first time it is asked for; swa_hostdb_unordered_view: the database as the reader
   keeps it (words in file order + where each amplicon's begin), what swa_db_upload_unordered takes — no host copy. */
void swa_hostdb_view(const swa_hostdb * db, swa_db_view * view);
void swa_hostdb_unordered_view(const swa_hostdb * db, swa_db_unordered_view * view);
uint64_t swa_hostdb_nucleotides(const swa_hostdb * db);
/* header of amplicon i (db order), NUL terminated; replaces db_getheader (src/db.h:47) */
const char * swa_hostdb_header(const swa_hostdb * db, uint32_t i, uint32_t * len);

/* ---- d = 1 host side: clustering over the neighbour CSR, grafting, writers --------- */
typedef struct swa_d1_result swa_d1_result;

/* Greedy breadth-first agglomeration over the CSR returned by swa_d1_network
   (replaces the clustering loop of algo_d1_run, src/algod1.cc:1185-1280). */
int  swa_d1_cluster(const swa_hostdb * db, const uint64_t * offsets, const uint32_t * neighbours,
                    swa_d1_result ** out);
/* The same result from the network that swa_d1_network_resident left in HBM: evaluated on the GPU
   (swa_d1_cluster_device), per-swarm sums on the host.  Needs the context that holds the network. */
int  swa_d1_cluster_resident(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result ** out);
/* The command line's form of the above: swarm / generation / parent and the per-swarm sums stay in HBM until an accessor,
   swa_d1_light_flags, swa_d1_graft or one of the -i -s -u -w writers asks for them (a plain `-o` run never does).  The
   caller keeps `ctx` alive, and its clustering untouched, until swa_d1_result_detach returned or the result is freed.
   swa_d1_result_detach fetches what is still on the device (SWA_E_DEVICE and swa_d1_result_error when that fails);
   after it the result does not refer to the context any more. */
int  swa_d1_cluster_resident_lazy(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result ** out);
/* The lazy form in two steps, for a caller that has a thread to spare while the network is being built: _prepare sizes the
   result's arrays for `db` and pins them (swa_host_pin) — any thread, any time after the context exists —, _prepared then
   clusters into them: the member order comes home as one DMA. */
int  swa_d1_result_prepare(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result ** out);
int  swa_d1_cluster_resident_prepared(swa_ctx * ctx, const swa_hostdb * db, swa_d1_result * prepared);
int  swa_d1_result_detach(swa_d1_result * res);
const char * swa_d1_result_error(const swa_d1_result * res);
void swa_d1_result_free(swa_d1_result * res);
/* out4 = {swarms after grafting, largest swarm, max generations, swarms before grafting}
   (the numbers of the log's summary lines, src/algod1.cc:1484-1487) */
void swa_d1_result_summary(const swa_d1_result * res, uint64_t * out4);
const uint32_t * swa_d1_result_swarmid(const swa_d1_result * res);     /* [n] */
const uint32_t * swa_d1_result_parent(const swa_d1_result * res);      /* [n], SWA_NO_AMPLICON for seeds */
const uint32_t * swa_d1_result_generation(const swa_d1_result * res);  /* [n] */
/* is_light[n] <- swarm mass < boundary; stats5 = {light swarms, amplicons in light swarms,
   nt in light swarms, heavy swarms, amplicons in heavy swarms} (src/algod1.cc:1291-1328) */
int  swa_d1_light_flags(const swa_d1_result * res, int64_t boundary, uint8_t * is_light, uint64_t * stats5);
/* attach_candidates (src/algod1.cc:274-336): graft_cand[n] as returned by swa_d1_fastidious; returns the number of
   grafts made.  A grafted result holds one form: a printed swarm's members — its own, then those of the light swarms it
   won, in the order it won them — are one range of the member order, an attached swarm's range lies inside its heavy
   swarm's, and every writer reads ranges.  The winners are decided as the reference's walk over the sorted (parent, child)
   pairs decides them, for well-formed candidates: no parent lies in a swarm that is some child's swarm.  Ill-formed
   candidates (and candidates that are no amplicon, or a result that holds grafts already) make no graft: swa_d1_graft
   returns 0, leaves the result untouched, and sets swa_d1_result_error. */
uint32_t swa_d1_graft(swa_d1_result * res, const uint32_t * graft_cand);
/* The same from the four arrays of swa_d1_graft_device (grafts in chain order — by heavy swarm, ascending, a heavy swarm's
   in the order it won them: heavy swarm, light swarm, parent amplicon, child amplicon): the same layout made on the host,
   by all threads, with the grown sizes, the largest swarm, the swarm count and graft_cand of the winning children.  On a
   result whose details are still in HBM (swa_d1_cluster_resident_lazy) nothing is fetched: the sums and graft_cand are
   settled when a writer or accessor asks for the details, and -s, -w, -i, -u come out as after swa_d1_graft.  SWA_E_ARG,
   a text in swa_d1_result_error and a result left as it was for arrays that are no graft of this result: a swarm or
   amplicon it does not have, heavy swarms that do not ascend, a light swarm listed twice, a heavy swarm that is somebody's
   light swarm, a result that holds grafts already. */
int  swa_d1_result_install_graft(swa_d1_result * res, const uint32_t * heavy_swarm, const uint32_t * light_swarm,
                                 const uint32_t * parent, const uint32_t * child, uint32_t grafts);
/* The same from the layout swa_d1_graft_layout_device left in the context's HBM, with no per-graft array on the host and
   nothing to check or move: the printed member order is downloaded into the result's own member order (one DMA after
   swa_d1_result_prepare), the three per-swarm arrays beside it, and the loop over the swarms that ends every route sets
   each swarm's bounds [begin, begin + grown), the end of its own members, its size and whether it is attached; the largest
   swarm and the swarm count come from the layout's summary.  The writers print the same bytes.  On a result whose details
   are still in HBM nothing else is fetched; when the details are asked for, mass, length and singletons are summed over a
   swarm's whole range, the deepest generation over its own members (the reference leaves a heavy swarm's alone), and
   graft_cand comes from swa_d1_graft_candidates_fetch (the winners').  SWA_E_ARG, a text in swa_d1_result_error and a result
   left as it was when the context holds no layout, the layout is of another n or number of swarms, or the result holds grafts
   already.  What ends the layout (swarm_amd.h: what ends what) must not happen before the details are fetched.
   swa_d1_result_graft_route: how the result's grafts came — 0 none, 1 swa_d1_graft, 2 swa_d1_result_install_graft,
   3 swa_d1_result_adopt_layout. */
int  swa_d1_result_adopt_layout(swa_d1_result * res, swa_ctx * ctx);
uint32_t swa_d1_result_graft_route(const swa_d1_result * res);
/* how often swarm id, generation and parent were downloaded for this result (0 for a plain -o run, with or without -f) */
uint32_t swa_d1_result_detail_fetches(const swa_d1_result * res);
/* writers (path "-" = stdout): -o/-r, -s, -i, -w, -j  (src/algod1.cc:755-1062) */
int swa_d1_write_swarms(const swa_d1_result * res, const swa_hostdb * db, const char * path, int mothur,
                        int usearch_abundance, int64_t append_abundance, int64_t differences);
int swa_d1_write_stats(const swa_d1_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_d1_write_structure(const swa_d1_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_d1_write_seeds(const swa_d1_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_d1_write_network(const swa_hostdb * db, const uint64_t * offsets, const uint32_t * neighbours,
                         const char * path, int usearch_abundance, int64_t append_abundance);

/* -u for d = 1 (src/algod1.cc:849-932); penalties after gcd reduction (18/24/13 by default) */
int swa_d1_write_uclust(const swa_d1_result * res, const swa_hostdb * db, const char * path, int usearch_abundance,
                        int64_t append_abundance, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend);
/* the same file with the alignments on the GPU (seam B5, swa_nw_batch on `ctx`, which holds the same database; NULL
   only for a result without H lines).  SWA_NW_CHUNK=n (a test hook): n pairs per chunk instead of 2^20. */
int swa_d1_write_uclust_gpu(swa_ctx * ctx, const swa_d1_result * res, const swa_hostdb * db, const char * path,
                            int usearch_abundance, int64_t append_abundance, uint64_t mismatch, uint64_t gapopen,
                            uint64_t gapextend);
/* ... and with every chunk's alignments divided among the ranks of `multi` (swa_multi_nw_batch; every rank holds the same
   database: swa_multi_db_upload).  The same file for any device list; the [nw] lines under SWARM_AMD_TIMING show the
   sums over the ranks. */
int swa_d1_write_uclust_multi(swa_multi * multi, const swa_d1_result * res, const swa_hostdb * db, const char * path,
                              int usearch_abundance, int64_t append_abundance, uint64_t mismatch, uint64_t gapopen,
                              uint64_t gapextend);

/* ---- d >= 2 host side: the greedy loop of algo_run over the GPU's fused scan step ------- */
typedef struct swa_dn_result swa_dn_result;

/* Replaces algo_run's clustering loop (src/algo.cc:384-602).  Needs a context with the
   database resident (swa_db_upload of the same hostdb); runs swa_qgram_build,
   swa_search_begin, swa_scan_begin itself, then one swa_scan_step per seed / sub-seed.
   Penalties after the reference's gcd reduction (src/swarm.cc:466-483). */
int  swa_dn_cluster(swa_ctx * ctx, const swa_hostdb * db, int64_t differences, int no_cluster_breaking,
                    uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, swa_dn_result ** out);
/* the same on the GPUs of a swa_multi (d >= 2 graph divided by ownership of window groups: swa_multi_dn_graph and the walk on
   the host, or — where swa_multi_cluster_on_device() — swa_multi_dn_graph_resident and the walk and tables on rank 0's GPU;
   where the fused scan serves, the same greedy loop over swa_multi_scan_*, the pool divided among the ranks, unless
   SWARM_AMD_MULTI_SCAN=root leaves it to rank 0 alone: the comparison switch) */
int  swa_dn_cluster_multi(swa_multi * multi, const swa_hostdb * db, int64_t differences, int no_cluster_breaking,
                          uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, swa_dn_result ** out);
/* SWARM_AMD_MULTI_CLUSTER=device|host: where a run on several GPUs clusters what the exchange assembled on rank 0 — there
   (1: the network or graph stays resident, as on one GPU; the default, by the measurement of profiles/r23/NOTES.md) or on the host behind a download (0: =host). */
int  swa_multi_cluster_on_device(void);
void swa_dn_result_free(swa_dn_result * res);
const char * swa_dn_result_error(const swa_dn_result * res);
/* 1 when the bulk graph (swa_dn_graph*) served the clustering, 0 when the fused scan did.  SWARM_AMD_DN=scan|graph
   choose; without it the graph serves d <= 8 (where swa_dn_graph_supported) and the scan everything else. */
int  swa_dn_result_over_graph(const swa_dn_result * res);
/* the ranks the fused scan ran on: 0 when the bulk graph served, 1 for one context (swa_dn_cluster, SWARM_AMD_MULTI_SCAN=root),
   else the ranks of the swa_multi */
uint32_t swa_dn_result_scan_ranks(const swa_dn_result * res);
/* The graph route's swarm tables are made on the host from five downloaded arrays (SWARM_AMD_DN_TABLES=host, the default) or
   in HBM (=device: swa_dn_tables_device).  On the device route the links stay in HBM until the first writer that reads them
   (-i, -u) asks; this is how often they were downloaded for this result (0 for a run that writes -o, -s, -w alone; else 1).
   Until then the result needs its context alive and with this clustering still in place: after another upload, network or
   clustering call on it, -i and -u of this result fail with a message (swa_dn_result_error); -o, -s, -w never need it. */
uint32_t swa_dn_result_link_fetches(const swa_dn_result * res);
/* out3 = {number of swarms, largest swarm, max generations} (src/algo.cc:699-705) */
void swa_dn_result_summary(const swa_dn_result * res, uint64_t * out3);
/* writers: -o/-r, -s, -i, -w, -u  (src/algo.cc:122-325, 473-488, 573-589, 608-674) */
int swa_dn_write_swarms(const swa_dn_result * res, const swa_hostdb * db, const char * path, int mothur,
                        int usearch_abundance, int64_t append_abundance);
int swa_dn_write_stats(const swa_dn_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_dn_write_structure(const swa_dn_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_dn_write_seeds(const swa_dn_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_dn_write_uclust(const swa_dn_result * res, const swa_hostdb * db, const char * path, int usearch_abundance,
                        int64_t append_abundance);
/* the same file with the alignments on the GPU (as swa_d1_write_uclust_gpu) */
int swa_dn_write_uclust_gpu(swa_ctx * ctx, const swa_dn_result * res, const swa_hostdb * db, const char * path,
                            int usearch_abundance, int64_t append_abundance);
/* ... divided among the ranks of `multi` (as swa_d1_write_uclust_multi) */
int swa_dn_write_uclust_multi(swa_multi * multi, const swa_dn_result * res, const swa_hostdb * db, const char * path,
                              int usearch_abundance, int64_t append_abundance);

/* ---- the uclust aligner on the host (src/nw.cc:237-255): what both -u writers print, and what swa_nw_batch must equal ----
   dseq / qseq 2-bit packed.  Returns the differences (columns - matches); *columns = alignment length; the CIGAR into
   cigar[cigar_cap] (NUL terminated, cut short if it does not fit), *cigar_len = its full length. */
uint64_t swa_nw_align_host(const uint64_t * dseq, uint32_t dlen, const uint64_t * qseq, uint32_t qlen, uint64_t mismatch,
                           uint64_t gapopen, uint64_t gapextend, uint64_t * columns, char * cigar, uint64_t cigar_cap,
                           uint64_t * cigar_len);

/* ---- d = 0: dereplication (src/derep.cc) ------------------------------------------------
   Clusters of identical sequences from swa_derep's array: members in db order, the first one
   is the seed; clusters by decreasing mass, then by seed index (src/derep.cc:67-90). */
typedef struct swa_d0_result swa_d0_result;
int  swa_d0_cluster(const swa_hostdb * db, const uint32_t * first_identical, swa_d0_result ** out);
/* The same result with the clustering made on the device (src/derep.cc:276-354, 67-90): swa_derep_resident has left
   first_identical in HBM on `ctx`, swa_d0_cluster_device makes the tables there and swa_d0_cluster_fetch brings them
   home.  No first_identical array on the host; every writer below works on the result unchanged. */
int  swa_d0_cluster_resident(swa_ctx * ctx, const swa_hostdb * db, swa_d0_result ** out);
void swa_d0_result_free(swa_d0_result * res);
/* A result of either origin as plain arrays, in output order: seed, mass, size, singletons and begin of every cluster
   (cluster_cap entries each) and members[n] — cluster c's are members[begin[c], begin[c] + size[c]), db order, seed first.
   Any array may be NULL.  *clusters (may be NULL) = the number of clusters; SWA_E_CAPACITY when a cluster array is wanted
   and cluster_cap is smaller (nothing is copied then). */
int  swa_d0_result_tables(const swa_d0_result * res, uint32_t * seed, uint64_t * mass, uint32_t * size, uint32_t * singletons,
                          uint32_t * begin, uint32_t cluster_cap, uint32_t * members, uint32_t * clusters);
/* out3 ={clusters, largest cluster (members), heaviest cluster (mass)}  (src/derep.cc:405-410) */
void swa_d0_result_summary(const swa_d0_result * res, uint64_t * out3);
/* writers: src/derep.cc:207-273 (-o / -r), 188-204 (-w), 107-124 (-s), 127-148 (-i), 151-185 (-u) */
int swa_d0_write_swarms(const swa_d0_result * res, const swa_hostdb * db, const char * path, int mothur,
                        int usearch_abundance, int64_t append_abundance, int64_t differences);
int swa_d0_write_seeds(const swa_d0_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_d0_write_stats(const swa_d0_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_d0_write_structure(const swa_d0_result * res, const swa_hostdb * db, const char * path, int usearch_abundance);
int swa_d0_write_uclust(const swa_d0_result * res, const swa_hostdb * db, const char * path, int usearch_abundance,
                        int64_t append_abundance);

/* ---- the command line (src/swarm.cc:96-124, 269-463, 486-630) ---------------------------
   `swarm` itself: options, log lines, FASTA in, output files out, exit status; everything above driven the way the
   reference's main() drives its own functions.  The executable swarm_amd/bin/swarm is a launcher that sets the OpenMP
   wait policy and calls this (host/launcher.cpp). */
int swa_cli_main(int argc, char ** argv);

#ifdef __cplusplus
}
#endif
#endif
