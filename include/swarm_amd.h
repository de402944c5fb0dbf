/*
 * swarm_amd.h — C ABI of the MI355X-native amplicon neighbour-finding library
 * (libswarm_amd.so, built from swarm_amd/csrc/ with hipcc --offload-arch=gfx950).
 *
 * The reference (torognes/swarm 3.1.6) has no plugin/FFI interface; its hot path is
 * reached through four internal C++ call seams.  This header is the
 * thin C ABI a maintainer would bind at exactly those seams: plain pointers and
 * sizes, caller-allocated result buffers (as in the reference, where algo_d1_run /
 * algo_run own every vector: src/algod1.cc:1104-1125, src/algo.cc:352-361), int
 * status instead of fatal()+exit(1) (src/utils/fatal.cc:27-31).
 *
 *   seam  reference interface replaced                               entry point
 *   ----  ---------------------------------------------------------  --------------------------
 *   L2    global seqindex[] read through db_get*() (src/db.h:35-53)  swa_db_upload / swa_db_attach
 *   B1    hash_insert loop + network_thread/check_variants           swa_d1_index_build
 *         (src/algod1.cc:188-208, 606-670, 1122-1171)                swa_d1_network[_device]
 *   B2    mark_light_thread / check_heavy_thread                     swa_d1_fastidious
 *         (src/algod1.cc:453-552, 1411-1467)
 *   B3    db_qgrams_init + qgram_diff_fast (src/db.cc:819-842,       swa_qgram_build
 *         src/qgram.h:31-35)                                         swa_qgram_diff
 *   B4    search_begin + search_do (src/scan.h:30-37, 259)           swa_search_begin / swa_search_do
 *   B5    nw() per H line of the uclust writers (src/algod1.cc:896-  swa_nw_batch
 *         925, src/algo.cc:620-655, src/nw.cc:237-255)               (several GPUs: swa_multi_nw_batch)
 *
 * Amplicon numbering everywhere = the reference's db order after db_read():
 * abundance descending, then header ascending (src/db.cc:388-413).  Sequences are
 * 2-bit packed exactly as the reference packs them (A0 C1 G2 T/U3, 32 nt per
 * little-endian u64, LSB first, zero padded: src/db.cc:541-628,
 * src/utils/nt_codec.cc:35-75) but 8-byte aligned, one amplicon after the other.
 *
 * All functions are synchronous with respect to the caller unless the name ends in
 * _device (those only enqueue on the context's HIP stream and leave results in HBM).
 * One swa_ctx is bound to one GPU and one HIP stream; use one context per GPU (one
 * process per GPU, or one host thread per GPU).  The library never falls back to the
 * CPU: without a usable gfx950 device every call fails with SWA_E_DEVICE.
 */
#ifndef SWARM_AMD_H
#define SWARM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SWA_ABI_VERSION 1

enum {
  SWA_OK = 0,
  SWA_E_DEVICE = 1,      /* no GPU / HIP runtime error (see swa_last_error) */
  SWA_E_ARG = 2,         /* invalid argument or call order */
  SWA_E_NOMEM = 3,       /* hipMalloc / host allocation failed */
  SWA_E_CAPACITY = 4,    /* caller's result buffer too small; *total tells the need */
  SWA_E_DUPLICATES = 5,  /* identical sequences present (reference: fatal, src/algod1.cc:1141-1150) */
  SWA_E_INTERNAL = 6     /* the d = 1 guard: index / network counts that must balance do not (never a short network instead) */
};

#define SWA_NO_AMPLICON 0xFFFFFFFFu   /* the reference's no_swarm (src/algod1.cc:80) */

typedef struct swa_ctx swa_ctx;

/* The packed amplicon database, n amplicons in db order.  Host or device pointers
   depending on the call that takes it. */
typedef struct swa_db_view {
  uint32_t n;                  /* amplicons */
  uint32_t longest;            /* longest sequence (nt) */
  const uint64_t * seqs;       /* packed words, amplicon i at words [seq_off[i], seq_off[i+1]) */
  const uint64_t * seq_off;    /* n+1 word offsets; seq_off[i+1]-seq_off[i] >= ceil(seqlen[i]/32) */
  const uint32_t * seqlen;     /* n lengths, nt (>= 1) */
  const uint64_t * abundance;  /* n abundances (>= 1) */
} swa_db_view;

/* ---- context ------------------------------------------------------------------ */
int  swa_abi_version(void);
/* device: HIP ordinal.  stream: a hipStream_t to run on (NULL -> the context creates
   its own non-blocking stream). */
int  swa_ctx_create(int device, void * stream, swa_ctx ** out);
void swa_ctx_destroy(swa_ctx * ctx);
/* message of the last failing call on this context ("" if none) */
const char * swa_last_error(const swa_ctx * ctx);
/* blocks until everything enqueued on the context's stream has finished */
int  swa_ctx_synchronize(swa_ctx * ctx);
/* Optional: pays the device's first-use costs (memory pools, copy queues, code-object loads) now — e.g. on a helper
   thread while the caller reads its input. */
int  swa_ctx_warmup(swa_ctx * ctx);
/* The same for a caller that knows its d: 1 loads the d = 1 step's and the clustering's code objects, >= 2 those of the q-gram,
   pair-graph and alignment kernels (and the clustering's), anything else all of them. */
int  swa_ctx_warmup_for(swa_ctx * ctx, int differences);
/* the copy engine's first download (~7.5 ms of runtime set-up whatever the size), paid ahead: any thread, beside the
   other warm-up calls */
int  swa_ctx_warmup_downloads(swa_ctx * ctx);

/* Per-kernel timing with HIP events on the context's stream (off by default).
   swa_timing_read: ms[0] seqhash, [1] table+Bloom build, [2] duplicate check,
   [3] d1 network kernels (anchored passes + fallback, or the plain kernel), [4] CSR assembly,
   [5] fastidious light pass, [6] fastidious heavy pass, [7] anchored-index build — durations
   of the most recent launches. */
int  swa_timing_enable(swa_ctx * ctx, int on);
int  swa_timing_read(swa_ctx * ctx, float * ms8);
/* the kernel groups of the streaming d = 1 step (swarm_amd/csrc/d1_stream.inc), same mechanism: ms[0] amplicon keys,
   [1] partition of the key records, [2] groups + work lists (+ identical sequences), [3] pair kernels of the prefix
   groups, [4] of the suffix groups, [5] partition of the links by source, [6] CSR rows, [7] amplicon lines (once per
   uploaded database) — durations of the most recent launches, 0 for a group that did not run. */
int  swa_timing_read_stream(swa_ctx * ctx, float * ms8);

/* ---- L2: database residency ---------------------------------------------------- */
/* copy a host-resident database into HBM (replicated on this context's GPU) */
int swa_db_upload(swa_ctx * ctx, const swa_db_view * host_db);
/* adopt a database whose arrays are ALREADY device memory on this GPU (not copied,
   not freed; must outlive the context's use of it) */
int swa_db_attach(swa_ctx * ctx, const swa_db_view * device_db);
/* The same database handed over as the FASTA reader leaves it (src/db.cc:432-628 packs while it reads; :388-413 sorts
   afterwards): the packed words in FILE order, in `pieces` pools, and per amplicon k of the db order where its words
   begin in the concatenation of the pools.  The GPU puts the words in db order (one gather kernel) — the host never
   copies them.  swa_db_stage_words starts the copy of the pools as soon as they exist (asynchronous, on the context's
   stream; the pools must stay as they are until swa_db_upload_unordered has returned); swa_db_upload_unordered stages
   them itself if that was not done (same pool pointers), copies the three per-amplicon arrays and leaves the context
   exactly as swa_db_upload does. */
typedef struct swa_db_unordered_view {
  uint32_t n;                          /* amplicons */
  uint32_t longest;                    /* longest sequence (nt) */
  uint32_t pieces;                     /* word pools */
  const uint64_t * const * piece_words; /* pools[pieces]: packed words, every sequence from a word boundary */
  const uint64_t * piece_word_count;   /* words per pool */
  const uint64_t * src_off;            /* [n] db order: first word of amplicon k, counted through the pools in order */
  const uint32_t * seqlen;             /* [n] db order */
  const uint64_t * abundance;          /* [n] db order */
} swa_db_unordered_view;
int swa_db_stage_words(swa_ctx * ctx, const uint64_t * const * piece_words, const uint64_t * piece_word_count, uint32_t pieces);
int swa_db_upload_unordered(swa_ctx * ctx, const swa_db_unordered_view * host_db);
/* Result buffers are the caller's (as in the reference: src/algod1.cc:1104-1125).  A caller that wants its downloads — the
   member order of swa_d1_cluster_device, the lists of swa_d1_network — at the link's speed pins them first: the copy is then
   one DMA instead of a staged copy through the runtime's bounce buffers.  Any thread; the memory stays the caller's
   (unpin before freeing it). */
int  swa_host_pin(swa_ctx * ctx, void * ptr, size_t bytes);
void swa_host_unpin(void * ptr);

/* ---- B1: d = 1 network --------------------------------------------------------- */
/* The index the network calls work on — what the reference's hash_insert loop builds (src/algod1.cc:188-208,
   1122-1150).  IDENTICAL SEQUENCES (the reference: fatal inside that loop, src/algod1.cc:1131-1150) are reported with
   SWA_E_DUPLICATES by whichever call meets them (round 6): the index build when it builds a table (*has_duplicates != 0:
   the database-wide table, or the table of the members left to the plain kernel) — and otherwise the NETWORK call, whose
   prefix pass compares the members of every group with one another anyway and sees two whose every word agrees for two
   instructions a pair (rounds 3-5 ran a second hash table over sequence fingerprints inside the index build for that: a
   quarter of its largest kernel).  A binding checks both return codes; the message is the reference's either way.
   What is built depends on the database: sequences of 65..256 nt in abundance order get the two
   anchor indexes of the streaming build (amplicons grouped by their first / last w nt, w = 32, 64 or 128: swa_d1_anchor_width; members and work lists
   in one pass over the amplicon lines: swarm_amd/csrc/d1_stream.inc) and nothing else; the
   database-wide structures of the reference — Zobrist table (bit-identical, src/zobrist.cc:49-80), seqhash[]
   (src/db.cc:761), amplicon hash table + Bloom filter (src/hashtable.cc, src/bloompat.cc) — are built only for what
   needs them: sequences under 65 nt, groups too large for the pair kernels, a database not in abundance order, the
   debug readers. */
int swa_d1_index_build(swa_ctx * ctx, int * has_duplicates);
/* Range form: the index covers the whole database as above; a table-based duplicate check looks only at the amplicons of
   [first, first + count) (their twin may be anywhere in the database).  On the pair route the network call reports a
   pair of identical sequences when one of the two is a seed of that call — [first, first + count) of swa_d1_network*,
   or, under swa_d1_set_ownership, any member of a group the rank owns: over the ranks every such pair is met by exactly
   one of them; OR the codes. */
int swa_d1_index_build_range(swa_ctx * ctx, uint32_t first, uint32_t count, int * has_duplicates);
/* Where the last index build put the two anchor windows that group the amplicons: out2 = {nt from the start, nt from
   the end}; (0, 0) = the first / last w nt, moved inwards (32-nt windows then) when those are (nearly) the same for everybody. */
int swa_d1_anchor_windows(const swa_ctx * ctx, uint32_t * out2);
/* ... and how wide it made them, in nucleotides: 32, 64 or 128 — the widest that leaves the shortest sequence of the
   database two windows and a nucleotide.  Two sequences of at least 2 w + 1 nt one edit apart share their first w or
   their last w nucleotides for any w; the reference has no such notion (it enumerates: src/variants.cc:184-249). */
uint32_t swa_d1_anchor_width(const swa_ctx * ctx);
/* Multi-GPU by ownership (no reference counterpart: src/algod1.cc:641-669 splits the seeds over
   threads that share one table).  With world > 1 this context serves only its share of the
   probes: the anchor groups (amplicons sharing their first / last w nucleotides) whose key maps
   to `rank` — with ALL their members, so the groups' LDS tables are built once per job instead
   of once per rank —, its share of the seeds only the plain kernel can serve, and, when the
   anchored route is not in use, the seeds with id mod world == rank.  swa_d1_network[_device]
   over a range then returns the PARTIAL rows of that range; over all ranks every link of the
   network appears exactly once (they are redistributed by source range: swa_d1_network_edges_device below for the
   form that travels, swa_d1_links_split / swa_d1_csr_from_lists for the two ends of the exchange,
   swarm_amd/sharding.py for the collectives between them).
   world = 1 restores the complete network.  Takes effect at the next network call.
   An index build made under ownership contains only what the rank's groups need: hashes of their
   members, duplicates found inside the owned prefix groups (identical sequences share one, so
   over all ranks every duplicate pair is reported by exactly one of them — OR the flags), and
   the database-wide table + Bloom only if some seed needs the plain kernel; after changing the
   owner call swa_d1_index_build[_range] again. */
int swa_d1_set_ownership(swa_ctx * ctx, uint32_t rank, uint32_t world);

/* Routed index build of a multi-GPU job: no rank walks the whole (replicated) database any more.
   (The reference has no counterpart: its threads share one table, src/algod1.cc:188-208; this is the distributed
   form of that hash_insert loop.)
   1. every rank keys ITS slice [first, first + count) of the amplicons: swa_d1_route_slice leaves, per anchor index
      (0 = prefix side, 1 = suffix side) and per owning rank, the ids of the slice whose key that rank owns —
      d_ids[(index * world + owner) * cap + ..], d_counts[index * world + owner]; d_counts[2 * world] != 0 reports a
      region that was too small (cap >= 1.5 * count / world + 1024 never is, ownership being hashed).  Device
      pointers; the lists and counts are complete when the call returns.
   2. the ranks exchange the lists all-to-all (RCCL / torch.distributed: 8 bytes per amplicon in total);
   3. every rank builds its indexes from what it received: swa_d1_index_build_routed(ids of index 0, of index 1) —
      as swa_d1_index_build under swa_d1_set_ownership(rank, world), which must have been called, but from the lists.
      Databases the anchored passes cannot serve alone (sequences under 65 nt, oversized groups, not in abundance
      order) take the database-wide route inside the call, as always. */
int swa_d1_route_slice(swa_ctx * ctx, uint32_t first, uint32_t count, uint32_t world, uint32_t * d_ids, uint64_t cap,
                       uint32_t * d_counts);
int swa_d1_index_build_routed(swa_ctx * ctx, const uint32_t * d_ids_prefix, uint32_t n_prefix, const uint32_t * d_ids_suffix,
                              uint32_t n_suffix, int * has_duplicates);
/* The same three steps with the KEY RECORDS travelling instead of the ids (round 6; what the multi-GPU drivers use): the rank
   that holds an amplicon's slice computes its key record (record key << 32 | id: 8 bytes) per index — a streaming pass over
   its own share of the packed database —, and the owner of the key starts at the partition: it no longer fetches one random
   64-byte line per received id out of a line array N times its share.  d_records[(index * world + owner) * cap + ..],
   d_counts as above.  8 + 8 bytes per amplicon through the exchange instead of 4 + 4. */
int swa_d1_route_slice_records(swa_ctx * ctx, uint32_t first, uint32_t count, uint32_t world, uint64_t * d_records,
                               uint64_t cap, uint32_t * d_counts);
int swa_d1_index_build_records(swa_ctx * ctx, const uint64_t * d_records_prefix, uint32_t n_prefix,
                               const uint64_t * d_records_suffix, uint32_t n_suffix, int * has_duplicates);

/* Neighbour lists of amplicons [first, first+count) as CSR: offsets[count+1],
   neighbours[offsets[count]]; row k = { j != first+k : seq_j is a microvariant of
   seq_(first+k) and (no_cluster_breaking or abundance[first+k] >= abundance[j]) },
   each neighbour once, ascending.  cap = capacity of `neighbours` in entries;
   *total = entries needed.  SWA_E_CAPACITY if total > cap (offsets still valid).
   SWA_E_DUPLICATES: two identical sequences among the seeds' groups (see swa_d1_index_build): like the reference, no
   network then. */
int swa_d1_network(swa_ctx * ctx, int no_cluster_breaking, uint32_t first, uint32_t count,
                   uint64_t * offsets, uint32_t * neighbours, uint64_t cap, uint64_t * total);
/* same, results left in HBM: d_offsets / d_neighbours are device pointers; only
   enqueues + one 8-byte readback of *total */
int swa_d1_network_device(swa_ctx * ctx, int no_cluster_breaking, uint32_t first, uint32_t count,
                          uint64_t * d_offsets, uint32_t * d_neighbours, uint64_t cap, uint64_t * total);
/* same links as one flat list in HBM: d_edge_list[i] = source << 32 | target, each link once, in
   no particular order (what the kernels emit before the CSR is assembled).  This is the form a
   multi-GPU job exchanges (swa_d1_set_ownership): nothing in it is proportional to the database
   size.  cap = capacity in entries; SWA_E_CAPACITY / *total as above. */
int swa_d1_network_edges_device(swa_ctx * ctx, int no_cluster_breaking, uint32_t first, uint32_t count,
                                uint64_t * d_edge_list, uint64_t cap, uint64_t * total);
/* The link exchange of a multi-GPU job on the device (no reference counterpart: its threads share one network array,
   src/algod1.cc:630-670).  Under swa_d1_set_ownership every rank holds the links of the anchor groups it owns, whichever
   amplicons they start from (swa_d1_network_edges_device); the final partition gives every rank a contiguous range of
   sources.  Three steps: split the rank's list by destination (swa_d1_links_split), exchange the runs all-to-all (RCCL /
   torch.distributed: 8 bytes per link, no link travels twice), assemble what arrived into the rank's slice of the CSR
   (swa_d1_csr_from_lists).  Neither call needs a database on the context.

   swa_d1_links_split: d_links = m links (source << 32 | target) on the device; d_links, d_out and d_counts must be
   8-byte aligned (SWA_E_ARG otherwise); bounds = world + 1 ascending
   ids on the HOST, bounds[0] = 0: rank r owns the sources [bounds[r], bounds[r + 1]) — ranks that own nothing are fine;
   world = 1 .. 64.  d_out (m entries) receives the links grouped by destination, run r beginning at the sum of
   d_counts[0 .. r), in no particular order inside a run; d_counts (world + 1 entries, device) the size of every run and, in
   [world], the links whose source is >= bounds[world]: those are written nowhere, and the call returns SWA_E_ARG.  d_out
   must not overlap d_links.  Stream-ordered on the context's stream, two kernel launches (none when m = 0: only the
   clear of d_counts), and then ONE 8-byte read of d_counts[world] on which the call waits (m = 0: it waits for the
   clear): d_out and d_counts are complete when it returns, whatever m (a caller needs the counts on the host next
   anyway, to size the exchange). */
int swa_d1_links_split(swa_ctx * ctx, const uint64_t * d_links, uint64_t m, const uint32_t * bounds, uint32_t world,
                       uint64_t * d_out, uint64_t * d_counts);
/* swa_d1_csr_from_lists: the CSR of the sources [first, first + count) from `lists` runs of links in one device buffer,
   run r = d_links[starts[r] .. starts[r] + counts[r]) (starts / counts on the HOST; runs may lie anywhere, be empty, and
   hold their links in any order).  Row i of the result is source first + i: d_offsets[count + 1] beginning at 0,
   d_neighbours ascending within a row.  Capacity protocol of swa_d1_network_device: the offsets are always complete,
   *total = entries needed (the sum of the counts: every link lands in a row), SWA_E_CAPACITY when it exceeds cap — call
   again with room; d_neighbours may be NULL with cap = 0.  Only enqueues (after the upload of starts / counts).
   The call works in the context's own scratch of the d = 1 step (the partition buffers, the segment table, the words
   "last CSR offset / links sorted" of the status block, timing slots 13 and 14): use it between the d = 1 calls of a
   context, as any other call on it, never from a second thread while one of them runs, and do not expect
   swa_timing_read's CSR slots to describe the last network call afterwards.
   Every source must lie in [first, first + count).  One that does not yields a wrong network but no write outside the
   buffers: with B = ceil(log2(count)), every partition level forms its bin as ((source - first) >> shift) & (bins - 1)
   and the row kernels their row as (source - first) & (rows - 1), so such a link is filed under the source congruent
   to it modulo 2^B; bins and rows are always inside their tables, the places of the links inside the count of links
   (each level is a counting sort of exactly the links it was given), d_offsets is written for rows below count only
   and d_neighbours below cap only.  (swa_d1_links_split + the exchange deliver in-range sources by construction.) */
int swa_d1_csr_from_lists(swa_ctx * ctx, const uint64_t * d_links, const uint64_t * starts, const uint64_t * counts,
                          uint32_t lists, uint32_t first, uint32_t count, uint64_t * d_offsets, uint32_t * d_neighbours,
                          uint64_t cap, uint64_t * total);
/* The guard (SWA_E_INTERNAL).  The reference's network thread cannot return a partial network
   (src/algod1.cc:630-670); the three calls above compare the counts their kernels hand to one another and,
   should they not balance, make everything derived from the uploaded database again and repeat the step ONCE
   (one line on stderr names the count) before they give up with SWA_E_INTERNAL.  This returns how many steps
   of this context were repeated that way (0 on every run seen so far). */
int swa_d1_guard_retries(const swa_ctx * ctx);

/* Introspection used by the parity tests (bit-exact against the oracle): copies to host.
   what: 0 seqhash u64[n] · 1 Bloom bitmap u64[table_size/8] · 2 Zobrist table
   u64[4*(longest+2)] · 3 the per-amplicon records of the hash kernel, n records of 64 bytes: u64 h, dall, iall, a32,
   d32, i32 (the Zobrist hash, the deletion and insertion XOR streams, and the three restricted to positions below
   pb), u32 pb (first position of the run of equal nucleotides that holds position anchor width - 1; the width itself
   for a shorter sequence, whose restricted streams are the full ones), u32[3] zero (0..3 build the database-wide
   structures on demand)
   · 4 facts of the uploaded database as the host holds them, u32[8]: the shortest sequence, the sequences of every
   width class (up to 160, 256, 480, 672 nt, longer), SWA_MAX_ZOBRIST_LDS of this build, 0; SWA_E_ARG when no build
   has read them · 5 the window sample of this upload as the host saw it, u32[16]: per candidate offset 0 / 32 / 64 /
   96 the sampled amplicons too short for it [4] and the sampled amplicons in stranded groups [4], the stride, the
   number of samples, the offset and the window width chosen FROM THE SAMPLE (swa_d1_anchor_windows tells what the
   first build's safety net made of it), 1 when a sample was drawn (0 under SWA_D1_WINDOWS=0, all of the above 0
   then), 0, 0, 0; SWA_E_ARG when no build has chosen windows (4 and 5 copy host memory: no kernel runs, nothing changes)
   · 10 / 11 member ids in group order of the streaming prefix / suffix index u32[n] · 12 / 13 their work-item
   buffers · 14 the counters u32[64] · 15 the amplicon lines (tools/check_index.py, tools/check_stream.py)
   · 17 / 18 the bucket starts of the key partition of the prefix / suffix index, u64[buckets + 1] with buckets =
   2^(total bits of swa_d1_part_plan); SWA_E_ARG once a network call has run (it sorts its links in the same scratch) */
int swa_d1_debug_read(swa_ctx * ctx, int what, void * out, size_t out_bytes);
/* Which forms the two partitions of the d = 1 step take.  The number of records decides it, never the data:
   swa_d1_part_plan_for: the key partition in front of the group kernel, as a pure function (no context, no device) of
   the records per index, the bits a key-overflow retry has added (0, 2, .. 8), whether the build is routed (0 / 1) and
   the bits forced by SWA_D1_PART_BITS (0: none; test hook).  out = {total bits, levels, bits of level 0, 1, 2 (0: no
   such level), records per tile, 1 when k_keys takes the first level's histogram, 1 for the one level of 1024 bins}.
   swa_d1_part_plan: the same for the streaming index in place, with the retry's bits in out[7] instead; SWA_E_ARG
   without such an index.
   swa_d1_csr_plan_for: the link partition and the row kernels of a CSR over `count` sources (swa_d1_network*,
   swa_d1_csr_from_lists).  out = {bits of a source index, r (a bucket of the row kernels holds 2^r sources), levels,
   bits of level 0, 1, 2}. */
int swa_d1_part_plan_for(uint64_t records, uint32_t extra_bits, int routed, uint32_t forced_bits, uint32_t out[8]);
int swa_d1_part_plan(const swa_ctx * ctx, uint32_t out[8]);
int swa_d1_csr_plan_for(uint32_t count, uint32_t out[6]);
/* ... and the work lists behind the key partition: 1 when every workgroup of k_group_lists finds the positions of its
   buckets' items itself (up to 1024 buckets), 0 when the counts are scanned by two launches first.
   swa_d1_lists_form_for: as a pure function of the number of buckets (2^total bits of the plan); -1 for 0 buckets.
   swa_d1_lists_form: what the streaming index in place was built with; -1 without such an index. */
int swa_d1_lists_form_for(uint64_t buckets);
int swa_d1_lists_form(const swa_ctx * ctx);
uint64_t swa_d1_table_size(const swa_ctx * ctx);

/* The same network computed into the context's own HBM buffers and kept there (no host copy):
   *total = number of links.  swa_d1_network_fetch copies it out later if somebody wants the lists (-j);
   swa_d1_cluster_device evaluates the agglomeration of src/algod1.cc:1175-1257 on it where it lies:
   swarmid / generation / parent per amplicon (parent = SWA_NO_AMPLICON for seeds), `order` = the members
   swarm after swarm (swarms by seed id, members seed first, then by generation and id), swarm s =
   order[swarm_begin[s], swarm_begin[s + 1]).  swarm_begin holds swarm_cap + 1 entries; SWA_E_CAPACITY
   with *nswarms = the number of swarms when that is too small (n always suffices). */
int swa_d1_network_resident(swa_ctx * ctx, int no_cluster_breaking, uint64_t * total);
int swa_d1_network_fetch(swa_ctx * ctx, uint64_t * offsets, uint32_t * neighbours, uint64_t cap);
/* the differences of every link of a resident d >= 2 graph (swa_dn_graph_resident, swa_multi_dn_graph_resident, an adopted
   graph with diffs), one byte per link in the order of swa_d1_network_fetch's neighbours; SWA_E_ARG for a network without */
int swa_d1_network_fetch_diffs(swa_ctx * ctx, uint8_t * diffs, uint64_t cap);
int swa_d1_cluster_device(swa_ctx * ctx, uint32_t * swarmid, uint32_t * generation, uint32_t * parent, uint32_t * order,
                          uint32_t * swarm_begin, uint32_t swarm_cap, uint32_t * nswarms);
/* swarmid / generation / parent may be null in swa_d1_cluster_device: they stay in HBM, and a caller that wants them
   after all (the reference's -i, -s, -u, -w outputs and --fastidious read ampinfo[].generation / parent,
   src/algod1.cc:994-1037) fetches them here (any of the three may be null again); valid until the next upload, index
   build, network or clustering call of the context.  swa_d1_cluster_maxgen: the deepest generation ("Max generations"). */
int swa_d1_cluster_fetch(swa_ctx * ctx, uint32_t * swarmid, uint32_t * generation, uint32_t * parent);
uint32_t swa_d1_cluster_maxgen(const swa_ctx * ctx);
/* A caller's own CSR over the n amplicons of the resident database installed as the resident network, for
   swa_d1_cluster_device (and, with one byte of differences per link in `diffs`, swa_dn_parent_diffs; diffs may be null).
   Checked on the host before anything is copied or launched: offsets[0] = 0, offsets never falling, offsets[n] = total,
   every neighbour < n, every row strictly ascending, no link from an amplicon to itself.  SWA_E_ARG otherwise, and no
   resident network is left.  The arrays are the caller's again on return.
   swa_d1_cluster_effort: what the last swa_d1_cluster_device call cost, out3 = {label sweeps launched, restarts of their
   numbering (a graph that needs more than 1023 sweeps), level batches (32 generations each)}. */
int swa_d1_network_adopt(swa_ctx * ctx, const uint64_t * offsets, const uint32_t * neighbours, const uint8_t * diffs, uint64_t total);
int swa_d1_cluster_effort(const swa_ctx * ctx, uint32_t out3[3]);

/* ---- B2: fastidious second pass ------------------------------------------------- */
/* is_light[n]: != 0 when the amplicon's swarm has mass < boundary.  light_nt: total
   nt of amplicons in light swarms; bloom_bits: --bloom-bits (src/algod1.cc:1337-1357).
   graft_cand[n] <- min heavy amplicon id two microvariant steps away, or
   SWA_NO_AMPLICON.  counters[0..4] = {light variants, heavy variants, graft
   candidates, Bloom m (bits), Bloom k} = the reference's logged numbers
   (src/algod1.cc:1394-1396, 1436-1438, 1469-1470). */
int swa_d1_fastidious(swa_ctx * ctx, const uint8_t * is_light, uint64_t light_nt, uint32_t bloom_bits,
                      uint32_t * graft_cand, uint64_t * counters);
/* Multi-GPU form: the light side (Bloom + light table, src/algod1.cc:453-489) is built whole
   on this GPU, the heavy side (check_heavy_thread, src/algod1.cc:492-552) covers only slice
   `shard` of `nshards` of the heavy amplicons.  Combining the shards: graft_cand = element-wise
   minimum (the reference keeps the smallest heavy id, src/algod1.cc:244-258), counters[1] and
   counters[2] add up, counters[0], [3], [4] are identical on every shard. */
int swa_d1_fastidious_shard(swa_ctx * ctx, const uint8_t * is_light, uint64_t light_nt, uint32_t bloom_bits,
                            uint32_t shard, uint32_t nshards, uint32_t * graft_cand, uint64_t * counters);
/* Which kernels the pass takes for the resident database: chosen from its longest sequence alone (and the switches
   SWA_FAST_BLOOM / SWA_FAST_PAIRS; SWA_FAST_LONG: below), so valid once a database is resident; the launches read the same plan.
   out[0] pair route on (1) or the Bloom route for every pair (0); [1] pair kernel: 5, 8, 13 = k_fast_pairs_lines on
   that many register words, 0 = k_fast_pairs on the packed words; [2] count kernel: 5, 8 = k_fast_count_sites, 0 =
   k_fast_count (the LDS set), 1 = k_fast_count_sites_words (the sites rule on words staged in LDS: SWA_FAST_LONG=pairs
   and SWA_FAST_COUNT=sites, below); [3] waves per block of k_fast_count or k_fast_count_sites_words, [4] slots of a
   wave's set (0 without a set), [5] the count kernel's dynamic LDS in bytes ([3] .. [5] all 0 under the register
   forms); [6] Bloom route: the Zobrist table in LDS (1) or read from memory (0);
   [7] the shortest sequence the pair route takes (a pair with a shorter member goes the Bloom route). */
int swa_d1_fastidious_plan(swa_ctx * ctx, uint32_t out[8]);
/* SWA_FAST_LONG=split (opt-in; without it nothing below applies and the plan is the one above).  k_fast_count's LDS set
   holds the microvariants of a sequence of up to cap nt (the largest length whose set fits 160 KB: 1004), so a single
   longer sequence sends every pair of the database to the Bloom route.  Under the switch, and only when the longest
   sequence exceeds cap, the pass is divided at the long end as it is at the short end.  Two sequences within two edits
   differ in length by at most 2, so:
     pair route:  the pairs whose two lengths both lie in [112, cap];
     Bloom route: every other pair, min(len) < 112 or max(len) > cap; the amplicons that can be half of such a pair
                  are those of len <= 113 or len >= cap - 1.
   The two sets of pairs are disjoint and complete, so graft_cand (a minimum) and the candidate count (a sum) stay
   exact.  The pair route's kernels are then chosen from pair_longest, the longest sequence <= cap, and the pair kernel
   is always k_fast_pairs on the packed words (out[1] = 0): the amplicon lines of the d = 1 index follow the whole
   database.  out[6] still follows the longest sequence.  SWA_FAST_BLOOM=1 wins over the switch; with no sequence of
   112 .. cap nt the pass stays all Bloom.  Which of the two is faster has been measured on one mixed set only
   (README, "Measured"): hence opt-in.
   swa_d1_fastidious_plan reports the plan actually launched.
   swa_d1_fastidious_split: out[0] 1 when the division is taken for the resident database, [1] cap, [2] pair_longest
   (0: no sequence <= cap), [3] amplicons longer than cap.  SWA_E_ARG when no database is resident.  [2] and [3] are
   facts of the database, reported with or without the switch: where the longest sequence exceeds cap, the first call
   after an upload runs the length pass on the device (one kernel over the lengths, one synchronisation) and caches its
   result; swa_d1_fastidious and swa_d1_fastidious_plan run that pass only under the split.
   swa_d1_fastidious_plan_for: the same dispatch as a pure function of (longest sequence, pair_longest, the three
   switches as 0 / 1), out laid out as in swa_d1_fastidious_plan; no context, no device.  pair_longest is read only
   when split != 0 and longest > cap.

   SWA_FAST_LONG=pairs (opt-in, and like the split only where the longest sequence exceeds 1004 nt and SWA_FAST_BLOOM=1
   is not set): the pair route itself serves the long sequences.  The count kernel of the whole pass is then
   k_fast_count_sites_words, which keeps no set and no Zobrist table: one wave a pair, both sequences staged in LDS as
   words + 3 64-bit words each, so 8 * waves * 2 * (words + 3) bytes, and the cap C is the longest sequence that fits
   160 KB with one wave (10 237 words = 327 584 nt; four waves up to 2 557 words = 81 824 nt).  The pair kernel is
   k_fast_pairs.  Every pair whose two lengths lie in [112, C] takes the pair route; the Bloom route keeps what the
   split's rule leaves it with C in the place of cap.  SWA_FAST_SITES_CAP=n (a test hook) lowers C to n where
   1004 <= n <= the derived cap, and is ignored otherwise.  The plan is [1, 0, 1, waves, 0, LDS bytes, [6], 112].
   swa_d1_fastidious_split then reports out[0] = 2, [1] = C, [2] the longest sequence <= C, [3] the amplicons longer
   than C (the length pass is cached per upload and cap).
   SWA_FAST_COUNT=sites (a comparison switch, same results): wherever the plan would run k_fast_count (a served length
   of 256 .. 1004, with or without the split), k_fast_count_sites_words runs in its place; out[2] = 1, [1] as without
   it.  No effect on the register forms or on the Bloom route.  Unknown values of either variable change nothing.
   swa_d1_fastidious_plan_modes: the dispatch with every switch as a pure function; long_mode 0 / 1 = split / 2 = pairs,
   sites_cap 0 = derived.  With long_mode <= 1 and count_sites = 0 it equals swa_d1_fastidious_plan_for.
   swa_d1_fastidious_sites_cap: C for a value of SWA_FAST_SITES_CAP (0: unset). */
int swa_d1_fastidious_split(swa_ctx * ctx, uint32_t out[4]);
int swa_d1_fastidious_plan_for(uint32_t longest, uint32_t pair_longest, int split, int bloom, int words, uint32_t out[8]);
int swa_d1_fastidious_plan_modes(uint32_t longest, uint32_t pair_longest, int long_mode, int bloom, int words, int count_sites,
                                 uint32_t sites_cap, uint32_t out[8]);
uint32_t swa_d1_fastidious_sites_cap(uint32_t sites_cap);
/* Of the last swa_d1_fastidious[_shard] call: out[0] pairs within two edits found by the pair route, [1] light and
   [2] heavy amplicons handed to the Bloom route (those of the short band and, under the split or pairs, of the long band),
   [3] attempts the pair list took (2 or more: it was regrown; 0: the pair route did not run). */
int swa_d1_fastidious_totals(swa_ctx * ctx, uint64_t out[4]);
/* Of the last swa_d1_fastidious[_shard] call, the batch loop of the Bloom route: out[0] launches of the heavy side's
   enumeration (k_d1_flex<., 1>), [1] how many of them produced more tasks than the list holds and were redone smaller,
   [2] the task cap in effect (1 GiB of tasks, or SWA_FAST_TASK_CAP; never below 7 longest + 4), [3] the most tasks a batch
   that ran produced (<= [2]).  All zero when the Bloom route did not run. */
int swa_d1_fastidious_bloom_batches(swa_ctx * ctx, uint64_t out[4]);
/* Of the last swa_d1_fastidious[_shard | _resident] call, the filter of the Bloom route (bloomflex.cc:91-115) as its light pass
   left it: facts[0] fsize, its 64-bit words (n_bytes >> 3 with n_bytes = (m - 1) / 8 + 1), [1] m, its bits (7 bloom_bits a
   nucleotide of the light amplicons handed to the route, at least 64), [2] k, the bits of a pattern (int(0.4 bloom_bits), at
   least 1), [3] bloom_bits as passed, [4] the tasks (heavy microvariants that passed the filter) summed over the batches that
   ran to the end — a batch that was redone smaller counts as it ran, not twice — [5..7] 0.  words may be NULL: the facts
   alone.  Otherwise it receives the fsize words (inverted polarity: a cleared bit is a set one of the reference's filter),
   cap_words = the room in words; SWA_E_CAPACITY when it is less than fsize (the facts are valid).  All zero, and words
   untouched, when that call did not run the Bloom route, and after a database upload.  A copy: no kernel runs and nothing of
   the pass changes.  Each shard of a sharded pass builds the whole filter; [4] is the shard's own. */
int swa_d1_fastidious_bloom_read(swa_ctx * ctx, uint64_t facts[8], uint64_t * words, uint64_t cap_words);

/* ---- B2 on the clustering in place: swarm sums, light flags, candidates and grafting without the host ----------------
   The reference does its fastidious bookkeeping on the host, around the two passes above; a caller that binds seam B2 and
   clusters with swa_d1_cluster_device has everything that bookkeeping reads in HBM already, and these calls do it there.
   All of them work on the clustering swa_d1_cluster_device left in place and fail with SWA_E_ARG and a message without one.
   Integer sums, minima and maxima only: every result is independent of scheduling.
   What ends what: an upload, index build, network or clustering call ends all of it (as for swa_d1_cluster_fetch).
   swa_d1_fastidious, _shard and _resident leave the clustering and the sums in place (they work in buffers of their own)
   and replace the candidates; swa_derep ends the candidates.  Whatever ends or replaces the candidates — a caller's
   candidates handed to swa_d1_graft_device included — ends the grafts made from them and their layout
   (swa_d1_graft_layout_device), and so does the start of every swa_d1_graft_device call.

   swa_d1_swarm_sums_device (src/algod1.cc:1232-1257, where the reference adds them up while it clusters): per swarm, in
   swarm order, the sum of the members' abundances, of their lengths, the members of abundance 1 and the deepest
   generation — one pass over the member order on the device.  `nswarms` = entries of the caller's arrays (SWA_E_CAPACITY
   when that is fewer than there are swarms); any output may be NULL: the sums stay in HBM for the calls below, which make
   them themselves when nobody has.  Sizes are not among them: they follow from swarm_begin.  After swa_d1_graft_device
   the call returns the sums as the grafts grew them.
   swa_d1_light_flags_device (src/algod1.cc:1291-1328, = swa_d1_light_flags of the host header): a swarm is light when its
   mass is below `boundary`.  is_light[n] (may be NULL) != 0 for the amplicons of light swarms; stats5 = {light swarms,
   amplicons in them, their nucleotides, heavy swarms, amplicons in them}.  The flags stay in HBM in the form the second
   pass reads; only the five numbers (and is_light, when asked for) are read back.  The masses are the sums in HBM as
   they are: call it before swa_d1_graft_device, as the reference does.
   swa_d1_fastidious_resident (src/algod1.cc:1337-1467, = swa_d1_fastidious): the second pass with its roles taken from
   the flags of the last swa_d1_light_flags_device call instead of a host array.  graft_cand may be NULL: the
   candidates are then not downloaded.  counters as swa_d1_fastidious.  Needs the d = 1 index (swa_d1_index_build).
   swa_d1_graft_device (attach_candidates and attach, src/algod1.cc:214-336): the reference sorts the (parent, child)
   pairs and walks them; what the walk decides is: a light swarm hangs on the parent of the smallest pair
   parent << 32 | child among its members' candidates, and a heavy swarm's chain holds the light swarms it won in
   ascending order of those pairs.  graft_cand = n candidates on the host (SWA_NO_AMPLICON: none; every other value must
   be an amplicon, SWA_E_ARG otherwise), or NULL for the candidates the last whole swa_d1_fastidious* pass of the context
   left in HBM.  No swarm with a candidate child may hold a candidate parent (light swarms have the children, heavy ones
   the parents).  *grafts = G; the four arrays (any may be NULL) receive the grafts in chain order — sorted by (heavy
   swarm, pair): heavy swarm, light swarm, parent amplicon, child amplicon.  SWA_E_CAPACITY with *grafts = the need when
   cap < G: nothing but the withdrawal below has happened then; call again with room (and the same graft_cand, or
   NULL).  The candidates of the children that did not win are withdrawn (SWA_NO_AMPLICON) in HBM, and the heavy swarms'
   sums grow by their light swarms' mass, length and singletons (the deepest generation stays, like the reference).  A
   further call starts from the swarms' own sums again.
   swa_d1_graft_candidates_fetch: the n candidates as they lie in HBM (after swa_d1_graft_device: the winners').
   swa_d1_graft_layout_device: the grafted clustering as ONE layout, made from the grafts a completed swa_d1_graft_device
   left in HBM (SWA_E_ARG without one; G = 0 is one, and the layout is then the clustering's own).  With own[s] the members
   of swarm s before grafting: attached[s] = 1 iff s is some graft's light swarm; grown[s] = own[s] for an attached swarm,
   else own[s] plus own of the light swarms it won; the printed swarms are the unattached ones, in swarm order;
   printed_order[n] holds, for every printed swarm, its own members in the order of swarm_members, then the members of
   each light swarm of its chain, in chain order; new_begin[s], for EVERY swarm, is where the own members of s begin in
   printed_order — a printed swarm with everything grafted is printed_order[new_begin[s], new_begin[s] + grown[s]), its
   own members the first own[s] of them.  summary3 = {w - G, the largest grown among the printed swarms, G}.  Integer
   scans and one scatter; any output may be NULL and the arrays stay in HBM either way; SWA_E_CAPACITY when nswarms (the
   entries of the per-swarm arrays) is below the number of swarms.  A second call returns the same arrays.
   swa_d1_graft_layout_info: out4 = {1 when a layout is in place else 0, and then: amplicons, swarms, grafts}; no device. */
int swa_d1_swarm_sums_device(swa_ctx * ctx, uint64_t * mass, uint64_t * sumlen, uint32_t * singletons, uint32_t * maxgen,
                             uint32_t nswarms);
int swa_d1_light_flags_device(swa_ctx * ctx, uint64_t boundary, uint8_t * is_light, uint64_t stats5[5]);
int swa_d1_fastidious_resident(swa_ctx * ctx, uint64_t light_nt, uint32_t bloom_bits, uint32_t * graft_cand, uint64_t * counters);
int swa_d1_graft_device(swa_ctx * ctx, const uint32_t * graft_cand, uint32_t * heavy_swarm, uint32_t * light_swarm,
                        uint32_t * parent, uint32_t * child, uint32_t cap, uint32_t * grafts);
int swa_d1_graft_candidates_fetch(swa_ctx * ctx, uint32_t * graft_cand);
int swa_d1_graft_layout_device(swa_ctx * ctx, uint32_t * printed_order, uint32_t * new_begin, uint32_t * grown,
                               uint8_t * attached, uint32_t nswarms, uint64_t summary3[3]);
int swa_d1_graft_layout_info(const swa_ctx * ctx, uint64_t out4[4]);
/* Shard owners: who expands which heavy amplicon when the second pass is divided among S shards (swa_d1_fastidious_shard:
   shard s takes the heavy amplicons whose ordinal h among the H heavy ones, in amplicon order, lies in
   [floor(H s / S), floor(H (s + 1) / S))).  swa_d1_shard_owners_device makes, from the flags of the last
   swa_d1_light_flags_device call and where they lie, one owner byte per amplicon: 255 for an amplicon of a light swarm, else
   the shard that owns it, floor(((h + 1) S - 1) / H); nshards = 1 .. 64; *heavy = H; owners (n bytes on the host) may be NULL:
   the bytes stay in HBM either way.  SWA_E_ARG without flags in place.  swa_d1_shard_owner_for: that closed form as a pure
   function (no device; SWA_E_ARG unless h < heavy <= 2^32 - 1 and 1 <= nshards <= 64).  swa_d1_shard_owner_plan: out =
   {amplicons per tile of the kernels, tiles per turn of the scan of the tiles' counts}. */
int swa_d1_shard_owners_device(swa_ctx * ctx, uint32_t nshards, uint8_t * owners, uint64_t * heavy);
int swa_d1_shard_owner_for(uint64_t heavy, uint32_t nshards, uint64_t h, uint32_t * owner);
int swa_d1_shard_owner_plan(uint32_t out[2]);

/* ---- d = 0: dereplication -------------------------------
   Replaces the bucket search of dereplicating() (src/derep.cc:276-354: Zobrist hash, open
   addressing, exact sequence comparison on a hash match).  first_identical[i] = the smallest
   amplicon index whose sequence is identical to amplicon i's (== i for the first occurrence);
   caller allocates u32[n].  Independent of swa_d1_index_build, and invalidates a d = 1 index
   built on the same context. */
int swa_derep(swa_ctx * ctx, uint32_t * first_identical);
/* The same search without the download: first_identical stays in HBM for swa_d0_cluster_device (swa_derep is this plus
   the copy).  What ends it, and the tables made from it: an upload or attach, the next swa_derep / swa_derep_resident,
   and the calls that reuse its buffer for graft candidates (swa_d1_fastidious*, swa_d1_graft_device). */
int swa_derep_resident(swa_ctx * ctx);
/* The clustering of dereplicating() and its order (src/derep.cc:276-354 and 67-90) made on the device from the resident
   array: what swa_d0_cluster of the host header makes, array for array.  Clusters in output order — mass descending, ties
   by the seed's db index ascending —, each with its seed (first member in db order), mass (sum of the members'
   abundances), size, singletons (members of abundance 1) and begin: its members are members[begin, begin + size),
   ascending db index, the seed first (members[] is grouped by cluster in SEED order, as the host's is).
   summary3 (may be NULL) = {clusters, largest size, heaviest mass}  (src/derep.cc:405-410).
   SWA_E_ARG with a message without a resident array.  Integer sums, maxima and stable sorts only: nothing depends on
   scheduling.
   swa_d0_cluster_fetch copies out any of the six arrays (NULL: not wanted): the five cluster arrays hold cluster_cap
   entries, members n.  *clusters (may be NULL) = the number of clusters; SWA_E_CAPACITY when a cluster array is wanted
   and cluster_cap is smaller than that (nothing is copied then).  SWA_E_ARG with a message without tables in place. */
int swa_d0_cluster_device(swa_ctx * ctx, uint64_t * summary3);
int swa_d0_cluster_fetch(swa_ctx * ctx, uint32_t * seed, uint64_t * mass, uint32_t * size, uint32_t * singletons,
                         uint32_t * begin, uint32_t cluster_cap, uint32_t * members, uint32_t * clusters);

/* ---- B3: q-gram prefilter -------------------------------------------------------- */
/* 1024-bit 5-mer parity signature per amplicon (src/qgram.cc:68-96), kept in HBM */
int swa_qgram_build(swa_ctx * ctx);
/* difflist[i] = ceil(popcount(sig[seed] xor sig[amplist[i]]) / 10)  (src/qgram.cc:247-252) */
int swa_qgram_diff(swa_ctx * ctx, uint64_t seed, uint64_t listlen, const uint64_t * amplist,
                   uint64_t * difflist);
/* copy the signature matrix to host: out = u8[n][128] */
int swa_qgram_debug_read(swa_ctx * ctx, uint8_t * out, size_t out_bytes);

/* ---- B4: alignment scan ----------------------------------------------------------- */
/* penalties after the reference's gcd reduction (src/swarm.cc:466-483): defaults
   mismatch 18, gapopen 24, gapextend 13.  resolution d = -d value. */
int swa_search_begin(swa_ctx * ctx, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t d);
/* 1 when the penalties / d given to swa_search_begin admit the wavefront kernel (every cost <= T
   decomposes uniquely, so the optimal cost alone fixes diff and alignment length), 0 when the
   banded tie-tracking kernel is used.  Same results either way; informational. */
int swa_search_uses_wavefront(const swa_ctx * ctx);
/* The kernel form every alignment launch (swa_search_do, the fused scan, the d >= 2 graph) takes for the penalties / d
   of swa_search_begin and the resident database's longest sequence: with_lengths != 0 for a launch that asks for
   alignment lengths (swa_search_do with alignlengths != NULL), 0 for one that does not (the scan and graph routes).
   *saturation = 255 or 65535 (the reference's 8- or 16-bit mode); *lds_bytes = the dynamic LDS a workgroup of the form
   stages (0 for SWA_FORM_GENERIC, which keeps its state in global scratch: 24 B a thread per nucleotide of the longest
   sequence, within 2 GiB).  A form whose staging does not fit the device's LDS is never chosen.  Any output may be
   NULL.
   The WIDE forms serve the bands that exceed the 64 lanes of k_align<64> (2 W + 3 > 64, W = d * max(mismatch, gapopen +
   gapextend) / gapextend + 1): k_align_wide<K> gives a pair one wave and a lane K = 2, 4, 8 adjacent band offsets, so
   W <= 62, 126, 254, with the results of SWA_FORM_GENERIC bit for bit.  They are opt-in: chosen only while the
   environment has SWA_ALIGN_WIDE=1 (read at every call) and their staging (64 B a word of the longest sequence) fits
   the LDS; otherwise such bands take SWA_FORM_GENERIC as before.
   swa_align_wide_for: that choice as a pure function of the scoring and d, out = {W, saturation, K}; K = 0 when the band
   fits 64 lanes or exceeds 254.  SWA_E_ARG for what swa_search_begin refuses.  SWA_E_ARG before swa_search_begin, without a database, or when the longest sequence is too long even for
   the generic kernel (one thread's scratch above 2 GiB, ~89 M nt); every alignment launch then fails the same way. */
typedef enum {
  SWA_FORM_WFA16 = 1,          /* k_align_wfa<16>: wavefront, four pairs a wave */
  SWA_FORM_WFA32 = 2,          /* k_align_wfa<32> */
  SWA_FORM_BANDED32 = 3,       /* k_align<32, false> */
  SWA_FORM_BANDED32_LEN = 4,   /* k_align<32, true> */
  SWA_FORM_BANDED64 = 5,       /* k_align<64, false> */
  SWA_FORM_BANDED64_LEN = 6,   /* k_align<64, true> */
  SWA_FORM_GENERIC = 7,        /* k_align_generic: one thread a pair, any band, any length */
  SWA_FORM_WIDE2 = 8,          /* k_align_wide<2, false>: one wave a pair, two band offsets a lane */
  SWA_FORM_WIDE2_LEN = 9,      /* k_align_wide<2, true> */
  SWA_FORM_WIDE4 = 10,         /* k_align_wide<4, false> */
  SWA_FORM_WIDE4_LEN = 11,     /* k_align_wide<4, true> */
  SWA_FORM_WIDE8 = 12,         /* k_align_wide<8, false> */
  SWA_FORM_WIDE8_LEN = 13      /* k_align_wide<8, true> */
} swa_align_form;
int swa_align_wide_for(uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t d, uint64_t out[3]);
int swa_search_form(swa_ctx * ctx, int with_lengths, int * form, uint32_t * saturation, uint64_t * lds_bytes);
/* diffs[i] == the reference's nw() value (src/nw.cc, which its search8/search16 + backtrack
   follow) whenever that value is <= d; otherwise some value > d.  Known exceptions, where the
   reference's 16-bit search departs from its own nw() and this library does not follow it: some
   pairs at the default scoring in 16-bit mode (the -d 11 case of tests/test_align_forms_gpu.py, a strict xfail) and gapopen + gapextend
   above 32767 (-g 30000: the search's 16-bit start value wraps).  The caller only tests diff <= d
   (src/algo.cc:460, 554).  scores / alignlengths may be NULL (never read by the reference's caller). */
int swa_search_do(swa_ctx * ctx, uint64_t query_no, uint64_t listlength, const uint64_t * targets,
                  uint64_t * scores, uint64_t * diffs, uint64_t * alignlengths);

/* ---- B3 + B4 fused: one (sub)seed of the d >= 2 greedy loop, pool state in HBM ------
   Replaces, per step of src/algo.cc:384-602, the host-side candidate list construction
   (abundance rule + `diffestimate <= radius + d` prune), qgram_diff_fast, the `qdiff <= d`
   filter, search_do and the `diff <= d` filter.  Requires swa_qgram_build and
   swa_search_begin.  swa_scan_begin: every amplicon unswarmed.
   swa_scan_step(seed, lowest_unswarmed, first_generation, radius, ncb, ...):
     candidates = unswarmed amplicons i >= lowest_unswarmed, i != seed, with
       (first_generation or est[i] <= radius + d) and (ncb or abundance[i] <= abundance[seed]);
     first_generation != 0 also marks `seed` as swarmed and stores est[i] = q-gram bound
       against this seed (src/algo.cc:442);
     hits = candidates with q-gram bound <= d and alignment diff <= d, returned in ascending
       id order (= the reference's pool order) with their diffs, and marked swarmed. */
int swa_scan_begin(swa_ctx * ctx);
int swa_scan_step(swa_ctx * ctx, uint32_t seed, uint32_t lowest_unswarmed, int first_generation, uint32_t radius,
                  int no_cluster_breaking, uint32_t * hit_ids, uint32_t * hit_diffs, uint32_t cap, uint32_t * nhits);
/* Batched form: all sub-seeds of one generation in one launch sequence.  seeds[k] with radius
   radii[k]; hits come back as triples (index k into seeds[], target id, diff) sorted by
   (k, id) and are computed against the pool as it was when the call started: a target may
   appear under several seeds, the caller keeps it for the first (queue order) and drops the
   others — which is exactly what processing the sub-seeds one by one gives.  Every returned
   target leaves the pool.  first_generation != 0 requires nseeds == 1. */
int swa_scan_batch(swa_ctx * ctx, uint32_t nseeds, const uint32_t * seeds, const uint32_t * radii,
                   uint32_t lowest_unswarmed, int first_generation, int no_cluster_breaking,
                   uint32_t * hit_seedidx, uint32_t * hit_ids, uint32_t * hit_diffs, uint32_t cap, uint32_t * nhits);
/* the (sorted) hits of the most recent swa_scan_batch again — for a caller whose buffers were
   too small (SWA_E_CAPACITY, *nhits = need): grow to *nhits and fetch; hit_seedidx may be NULL */
int swa_scan_fetch(swa_ctx * ctx, uint32_t * hit_seedidx, uint32_t * hit_ids, uint32_t * hit_diffs, uint32_t cap);
/* out3 = {q-gram comparisons, aligned pairs, launch sequences} since swa_scan_begin */
int swa_scan_totals(swa_ctx * ctx, uint64_t * out3);
/* test / triage read: out4 = {current capacity (pairs) of the scan's pair arrays, batches redone after the pair arrays
   overflowed, re-lists of the candidate list, batches whose hits were fetched by copy (more than the pinned mirror
   holds)}; the three counts run from the creation of the context */
int swa_scan_debug_state(swa_ctx * ctx, uint64_t * out4);
/* Ownership of the pool, for the scan divided among several contexts (swa_multi_scan_*).  Whether (seed, target) is a hit
   depends on the pair alone, so every context can scan a part of the pool against all seeds.  Amplicon id belongs to rank
   (id >> 5) % world: block-cyclic in blocks of 32 amplicons (one turn of a workgroup of the pool kernel, 4 KB of contiguous
   signatures; the shares stay even while lowest_unswarmed rises).
   swa_scan_set_ownership(rank, world): the context scans its own amplicons only — its estimates, pool flags and candidate
     list mean something for those alone, its hits are its share of the hits.  (0, 1), the state of a new context, is the
     whole pool.  1 <= world <= 64, rank < world (SWA_E_ARG otherwise); a change ends the scan in progress: swa_scan_begin next.
   swa_scan_owner_for(id, world): the owner; a pure function, no device.
   swa_scan_share_for(n, lowest_unswarmed, rank, world, out2): out2 = {how many amplicons of [lowest_unswarmed, n) the rank
     owns, the first of them (n when there is none)}; a pure function, no device; SWA_E_ARG for world = 0 or rank >= world. */
int swa_scan_set_ownership(swa_ctx * ctx, uint32_t rank, uint32_t world);
uint32_t swa_scan_owner_for(uint32_t id, uint32_t world);
int swa_scan_share_for(uint32_t n, uint32_t lowest_unswarmed, uint32_t rank, uint32_t world, uint32_t * out2);

/* ---- B5: the uclust alignments ------------------------------------------------------------
   Seam B5 (src/algod1.cc:880-925, src/algo.cc:608-659, src/nw.cc:237-255): npairs global alignments of amplicon
   d_ids[k] (the reference's dseq, the member) against q_ids[k] (qseq, the seed) of the resident database, with affine
   gaps under the reduced penalties and the reference's tie-breaking.  diffs[k] / columns[k] = nw()'s nwdiff / alignment
   length; cigar receives the pairs' CIGAR strings back to back (src/utils/cigar.cc:28-60: counts of 1 omitted, no NUL),
   cigar_end[k] = end of pair k's.  No CIGAR is longer than dl + ql.  SWA_E_CAPACITY when cigar_cap is too small:
   *cigar_total = the need (the other results are complete).  Banded tiers on the GPU, each result accepted only with its
   certificate: three tiers with the direction bits in LDS (16, 32, 64 lanes a pair: band half-width
   W = 6, 14, 30; min(dl, ql) <= 1024 and |dl - ql| <= 30), then four wide tiers with the bits in a bounded global
   scratch area (one wave a pair, 1, 2, 4, 8 band offsets a lane: W = 30, 62, 126, 254).  A pair enters at the narrowest
   tier that covers |dl - ql| and moves to the next wider one when its end cost is not below gapopen + (W + 1) gapextend.
   The host aligns, within the call and with the same result bit for bit, only:
     - pairs with |dl - ql| > 254, or whose end cost is at least gapopen + 255 gapextend (the widest certificate);
     - pairs with dl + ql > 32 768 (the length limit: two amplicons of 16 384 nt; sequences and CIGAR text of a pair are
       kept in LDS);
     - pairs whose costs could reach 2^30 (mismatch + 3 gapopen + (dl + ql + 4) gapextend), which need more than 32 bits;
     - pairs that found the device's CIGAR buffer full (swa_nw_batch_text_full counts them). */
int swa_nw_batch(swa_ctx * ctx, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t npairs,
                 const uint32_t * d_ids, const uint32_t * q_ids, uint32_t * diffs, uint32_t * columns,
                 uint64_t * cigar_end, char * cigar, uint64_t cigar_cap, uint64_t * cigar_total);
/* out4 = pairs of the last swa_nw_batch: certified by the 16-, 32-, 64-lane LDS tiers (half-width 6, 14, 30), and
   out4[3] = left by the LDS tiers (the wide tiers and the host together) */
int swa_nw_batch_totals(const swa_ctx * ctx, uint64_t * out4);
/* out8 = pairs of the last swa_nw_batch per tier: the three LDS tiers, the four wide tiers (half-width 30, 62, 126,
   254), the host.  A pair is counted in the tier that certified it. */
int swa_nw_batch_tiers(const swa_ctx * ctx, uint64_t * out8);
/* *out1 = pairs of the last swa_nw_batch that the widest tier certified but that found the CIGAR buffer full (host pairs) */
int swa_nw_batch_text_full(const swa_ctx * ctx, uint64_t * out1);

/* ---- B3 + B4 in bulk: the whole d >= 2 search as ONE graph --------------------------------
   Everything qgram_diff_fast + search_do can ever answer during algo_run (src/algo.cc:423-602: per seed
   and sub-seed, the pool amplicons with q-gram bound <= d and alignment diff <= d) depends only on the
   pair, not on the pool, so it is computed for the whole database at once:
     row q of the CSR = every target t != q with diff(query q, target t) <= d that the abundance rule
     allows q to take (abundance[t] <= abundance[q], or all with no_cluster_breaking), ascending t,
     diffs[e] = that diff (the reference's value, src/algo.cc:460, 554).
   The caller's greedy loop then needs no further device call.  Candidate pairs come from d + 1 disjoint
   windows per sequence (an alignment with <= d differences leaves one of them intact, shifted by at most
   d).  A sequence without room for them (fewer than 16 (d + 1) nucleotides: "short") joins no window group;
   its pairs are found by comparing it with every sequence whose length differs by at most d (no pair within
   d differences has a larger length difference).  That part is quadratic in the short sequences, so the
   number B of its candidate pairs — known from the count of sequences per length — is capped at 16 n + 2^20
   (test hook: SWA_DN_BRUTE_CAP): swa_dn_graph_supported != 0 when d <= 16 and B is within the cap (else use
   swa_scan_*; swa_dn_graph then fails with SWA_E_ARG).  For 9 <= d <= 16 the pairs of a window group come from a
   pair kernel of their own (k_dg_pairs_deep: runtime d, up to 33 shifts of up to 17 windows); everything behind the
   pair list is the same for every d.
   Requires swa_qgram_build and swa_search_begin.  Buffers as swa_d1_network: offsets[n + 1] always
   filled, *total = entries needed, SWA_E_CAPACITY when total > cap (call again with room: nothing is
   recomputed). */
int swa_dn_graph_supported(swa_ctx * ctx);
int swa_dn_graph(swa_ctx * ctx, int no_cluster_breaking, uint64_t * offsets, uint32_t * neighbours, uint8_t * diffs,
                 uint64_t cap, uint64_t * total);
/* The same graph left in HBM as the resident network: swa_d1_cluster_device then runs the greedy agglomeration of
   src/algo.cc:384-602 on it where it lies (seeds by lowest id, members by generation then id: src/algo.cc:205-219 — the
   same function of the directed graph as for d = 1), and swa_dn_parent_diffs returns, per amplicon, the differences to
   its parent in that clustering (0 for seeds; n bytes): radius(v) = radius(parent) + that (src/algo.cc:560-574). */
int swa_dn_graph_resident(swa_ctx * ctx, int no_cluster_breaking, uint64_t * total);
int swa_dn_parent_diffs(swa_ctx * ctx, uint8_t * pdiff);
/* What the writers need beyond the member order, made in HBM from that clustering instead of on the host (dn_tables.inc):
   radius of every amplicon (pointer jumping along the parents, bit_width(deepest generation) rounds), mass / singletons /
   deepest generation / deepest radius of every swarm, and the -i / -u links in acceptance order — the non-seed positions
   of the member order, stably sorted by their parent's position; swarm s owns the links [begin[s] - s, begin[s + 1] - s - 1).
   swa_dn_tables_device makes them and returns the sizes: *nswarms, *nlinks = n - *nswarms.  swa_dn_tables_fetch downloads
   what the caller asks for: radius[n]; mass, singletons, maxgen (0 for a swarm of one), maxradius [nswarms each];
   link_parent, link_child, link_generation, link_diff [nlinks each]; every output may be null.  Both return SWA_E_ARG
   with a message when no clustering is in place or the resident network carries no differences (as
   swa_dn_parent_diffs), the fetch also when no tables are in place; swa_dn_tables_device returns SWA_E_DEVICE ("a parent
   without a link to its child") when a member's parent has no link to it (or one of 255 differences: the byte that
   says so).  An empty database succeeds with nothing made.  The tables end with the clustering: upload, index build,
   network, adopt, swa_d1_cluster_device.  swa_dn_tables_serial: which swa_dn_tables_device call of this context made the
   tables in place (counted from 1; 0: none in place) — a caller that fetches later can tell whether they are still its own. */
uint64_t swa_dn_tables_serial(const swa_ctx * ctx);
int swa_dn_tables_device(swa_ctx * ctx, uint32_t * nswarms, uint64_t * nlinks);
int swa_dn_tables_fetch(swa_ctx * ctx, uint32_t * radius, uint64_t * mass, uint32_t * singletons, uint32_t * maxgen, uint32_t * maxradius,
                        uint32_t * link_parent, uint32_t * link_child, uint32_t * link_generation, uint8_t * link_diff);
/* out3 = {q-gram comparisons, aligned pairs, kernel launches} of the last swa_dn_graph */
int swa_dn_graph_totals(swa_ctx * ctx, uint64_t * out3);

/* ---- d = 1 (and, below, d = 0) on several GPUs of one node --------------------------------
   Replaces the thread fan-out of src/algod1.cc:1166-1167 / src/utils/threads.h:145-162: one context, stream and
   host thread per listed device inside the calling process; the database replicated, the probing divided by
   ownership of anchor groups (swa_d1_set_ownership): routed index build (every rank keys its own slice and the key
   records travel to their owners, grouped ncclSend / ncclRecv over xGMI), every rank's flat link list gathered on
   rank 0 only (grouped ncclSend / ncclRecv: the network has one consumer, rank 0), CSR assembled
   there on the device (swa_d1_csr_from_lists over the whole range, the ranks' lists as its runs) and either downloaded for the
   host (swa_multi_d1_network) or left as rank 0's resident network, where the agglomeration, the swarm sums, the light flags
   and the grafting run as on a single GPU (swa_multi_d1_network_resident); fastidious: heavy amplicons split — by the host from
   host flags (swa_multi_d1_fastidious) or by owner bytes made on rank 0's GPU and broadcast (swa_multi_d1_fastidious_resident)
   —, graft_cand combined with ncclAllReduce(min).  librccl.so is
   loaded when the first handle with ranks on distinct devices is created, not with the library.  A device may be listed more than once (several ranks on one GPU: the exchange then uses
   device-to-device copies — RCCL admits one rank per GPU); results never depend on the device list.
   Every route of the command line is divided among the ranks: d = 0 and the d >= 2 graph and scan routes further below,
   and the alignments of the uclust writers (seam B5: swa_multi_nw_batch, at the end of this section — no exchange at all,
   every rank aligns a contiguous run of a batch's pairs). */
typedef struct swa_multi swa_multi;
int  swa_multi_create(const int * devices, int ndevices, swa_multi ** out);
void swa_multi_destroy(swa_multi * m);
int  swa_multi_size(const swa_multi * m);
int  swa_multi_uses_rccl(const swa_multi * m);
swa_ctx * swa_multi_ctx(swa_multi * m, int rank);
const char * swa_multi_last_error(const swa_multi * m);
int  swa_multi_db_upload(swa_multi * m, const swa_db_view * host);
/* = swa_d1_index_build + swa_d1_network over the whole database (same buffers, same capacity protocol);
   *has_duplicates as swa_d1_index_build (SWA_E_DUPLICATES returned) */
int  swa_multi_d1_network(swa_multi * m, int no_cluster_breaking, uint64_t * offsets, uint32_t * neighbours, uint64_t cap,
                          uint64_t * total, int * has_duplicates);
/* = swa_d1_fastidious */
int  swa_multi_d1_fastidious(swa_multi * m, const uint8_t * is_light, uint64_t light_nt, uint32_t bloom_bits,
                             uint32_t * graft_cand, uint64_t * counters);
/* = swa_d1_index_build + swa_d1_network_resident on swa_multi_ctx(m, 0): the network stays on rank 0's device, nothing is
   downloaded; swa_d1_network_fetch, swa_d1_cluster_device and the calls behind it then work on that context.  After a
   failure rank 0 holds no resident network. */
int  swa_multi_d1_network_resident(swa_multi * m, int no_cluster_breaking, uint64_t * total, int * has_duplicates);
/* How the ranks got the members of their anchor groups in the last swa_multi_d1_network / swa_multi_d1_network_resident call:
   SWA_MULTI_BUILD_NONE (no call yet, or the call failed before the build), _ROUTED (every rank keyed its slice and the
   key records travelled to their owners), _STREAMED (every rank walked the whole database because it was asked to:
   SWARM_AMD_MULTI_BUILD=streamed, or one rank), _OVERFLOWED (the routed build was tried, a destination region of a rank's
   outgoing lists was too small — many amplicons sharing one window key — and the ranks then streamed). */
enum { SWA_MULTI_BUILD_NONE = 0, SWA_MULTI_BUILD_ROUTED = 1, SWA_MULTI_BUILD_STREAMED = 2, SWA_MULTI_BUILD_OVERFLOWED = 3 };
int  swa_multi_d1_last_build(const swa_multi * m);
/* = swa_d1_fastidious_resident on swa_multi_ctx(m, 0), the heavy amplicons divided among the ranks: needs rank 0's clustering
   and the flags of swa_d1_light_flags_device on it (SWA_E_ARG otherwise).  The owner bytes (swa_d1_shard_owners_device, S =
   the ranks) go from rank 0 to every rank (ncclBroadcast; device-to-device copies between ranks on one GPU), every rank runs
   its share, the candidates are combined in rank 0's HBM, where swa_d1_graft_device(ctx0, NULL, ...) reads them; graft_cand
   may be NULL: they are then not downloaded.  counters as swa_multi_d1_fastidious. */
int  swa_multi_d1_fastidious_resident(swa_multi * m, uint64_t light_nt, uint32_t bloom_bits, uint32_t * graft_cand, uint64_t * counters);

/* ---- d = 0 on several GPUs ------------------------------------------------------------------------------------------
   The bucket search of dereplicating() (src/derep.cc:276-354) divided among the ranks by ownership of the sequence
   hashes.  The database is replicated (swa_multi_db_upload); rank r hashes the slice [n r / world, n (r + 1) / world) only,
   groups its (hash, id) records by owner on the GPU — runs sized exactly from a count pass: a read with 10^6 copies sends
   10^6 records to one owner, nothing overflows —, the records travel all-to-all (grouped ncclSend / ncclRecv, device-to-
   device copies between ranks on one GPU; one rank takes the same path), every owner runs the search of swa_derep over
   what it received (all copies of a sequence are there, so the re-key rounds stay local), and rank 0 gathers
   first_identical << 32 | id of every read and writes the array into its HBM.
   swa_multi_derep_resident (src/derep.cc:276-354) = swa_derep_resident on swa_multi_ctx(m, 0): swa_d0_cluster_device,
   swa_d0_cluster_fetch and swa_d0_cluster_resident then work on that context.  On every rank the call ends the previous
   dereplication and a d = 1 index; no rank but rank 0 holds a resident array afterwards (swa_d0_cluster_device on another
   rank's context: SWA_E_ARG), none after a failure.  SWA_E_INTERNAL if the owners do not hold exactly n records.
   swa_multi_derep (src/derep.cc:276-354) = swa_derep: the resident form plus one download, first_identical = u32[n].
   swa_multi_derep_owner_for (src/derep.cc:276-354 keeps one table; here a hash has one owner): *owner = the rank of
   `world` (1 .. 64, SWA_E_ARG otherwise) that dereplicates every read whose Zobrist hash is `hash` — a pure function of the
   full 64-bit hash of the first round (the 64-bit finaliser of MurmurHash3, then the high word of its product with world),
   not of the narrowed or re-mixed key of a later round; needs no device.
   swa_multi_derep_totals (src/derep.cc:276-354), of the last call: received[world] = the records every owner got (their sum
   is n; 0: an empty inbox), out2 = {rounds of the owner that needed most, records routed}. */
int  swa_multi_derep_resident(swa_multi * m);
int  swa_multi_derep(swa_multi * m, uint32_t * first_identical);
int  swa_multi_derep_owner_for(uint64_t hash, uint32_t world, uint32_t * owner);
int  swa_multi_derep_totals(swa_multi * m, uint64_t * received, uint64_t * out2);


/* ---- d >= 2 on several GPUs (second paragraph) --------------------------------------------------
   Replaces the scan fan-out of src/scan.cc:221-256 under the loop of src/algo.cc:505-602.  swa_dn_set_ownership(rank,
   world): this context makes only the window groups of swa_dn_graph whose key maps to `rank`; a pair is reported
   through the first window it shares, and that window's group lives on one rank; a pair with a short member is
   reported by the rank that owns the short sequence emitting it (id modulo world; of two short ones the lower id
   emits); so over all ranks every pair of the graph is found exactly once.  swa_multi_dn_begin = swa_qgram_build + swa_search_begin on every rank;
   swa_multi_dn_graph = swa_dn_graph: every rank finds and aligns its share, the accepted (query, target, diff)
   triples travel to rank 0 (RCCL send / receive over xGMI, device-to-device copies for ranks sharing a GPU), which
   merges them into the CSR; same buffers and capacity protocol as swa_dn_graph.  swa_multi_dn_graph_resident =
   swa_dn_graph_resident on swa_multi_ctx(m, 0): the merged graph is left there as the resident network (with differences),
   for swa_d1_cluster_device, swa_dn_parent_diffs and swa_dn_tables_device on that context. */
int  swa_dn_set_ownership(swa_ctx * ctx, uint32_t rank, uint32_t world);
int  swa_multi_dn_begin(swa_multi * m, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t d);
int  swa_multi_dn_graph_supported(swa_multi * m);
int  swa_multi_dn_graph(swa_multi * m, int no_cluster_breaking, uint64_t * offsets, uint32_t * neighbours, uint8_t * diffs,
                        uint64_t cap, uint64_t * total);
int  swa_multi_dn_graph_resident(swa_multi * m, int no_cluster_breaking, uint64_t * total);
int  swa_multi_dn_graph_totals(swa_multi * m, uint64_t * out3);
/* The fused scan (swa_scan_*) divided among the ranks by ownership of the pool (swa_scan_set_ownership: rank r scans the
   amplicons i with (i >> 5) % world == r against every seed) — what src/scan.cc:221-256 does with threads.
   swa_multi_scan_begin comes after swa_multi_dn_begin: ownership and swa_scan_begin on every rank.
   swa_multi_scan_batch / _step / _fetch take the arguments of the single-context calls and keep their contract: triples
   sorted by (seed index, id), SWA_E_CAPACITY with the whole count in *nhits, every returned target leaves the pool; the
   same refusals with SWA_E_ARG.  One host thread enqueues the batch on every rank's stream, then finishes rank by rank; a
   rank whose pair arrays overflowed repeats its sequence alone; a rank that owns no amplicon at or above lowest_unswarmed
   launches nothing; the ranks' hit lists are merged on the host.  No collective: ranks on one device and ranks on
   distinct devices run the same code.  (A rank that launches nothing for a first generation does not mark the initial
   seed either: as the name says, everything below lowest_unswarmed counts as swarmed, so lowest_unswarmed must not fall
   back below an earlier initial seed — the greedy loop's never does.)
   swa_multi_scan_totals: out3 = {q-gram comparisons, aligned pairs — summed over the ranks, and those of a single context,
   because the shares partition the candidates —, launch sequences = batches since swa_multi_scan_begin (not a sum)}.
   The per-rank state (swa_scan_debug_state, swa_scan_totals) stays readable through swa_multi_ctx(m, r). */
int  swa_multi_scan_begin(swa_multi * m);
int  swa_multi_scan_batch(swa_multi * m, uint32_t nseeds, const uint32_t * seeds, const uint32_t * radii, uint32_t lowest_unswarmed,
                          int first_generation, int no_cluster_breaking, uint32_t * hit_seedidx, uint32_t * hit_ids,
                          uint32_t * hit_diffs, uint32_t cap, uint32_t * nhits);
int  swa_multi_scan_step(swa_multi * m, uint32_t seed, uint32_t lowest_unswarmed, int first_generation, uint32_t radius,
                         int no_cluster_breaking, uint32_t * hit_ids, uint32_t * hit_diffs, uint32_t cap, uint32_t * nhits);
int  swa_multi_scan_fetch(swa_multi * m, uint32_t * hit_seedidx, uint32_t * hit_ids, uint32_t * hit_diffs, uint32_t cap);
int  swa_multi_scan_totals(swa_multi * m, uint64_t * out3);

/* ---- B5 on several GPUs: the uclust alignments divided among the ranks (src/algod1.cc:880-925, src/algo.cc:608-659) ----
   Whether (member, seed) aligns with some CIGAR depends on the pair alone and the database is replicated
   (swa_multi_db_upload), so rank r aligns the contiguous pairs [bounds[r], bounds[r + 1]) of the batch with swa_nw_batch on
   its own context and stream, one host thread a rank: the one-thread host parts of a batch overlap as well as the kernels,
   also between ranks that share a device.  No collective and no kernel of its own; ranks on one device and ranks on
   distinct devices run the same code.
   swa_multi_nw_batch takes the arguments of swa_nw_batch and gives its outputs, bit for bit the same for any device list:
   diffs, columns, cigar_end (cumulative over the whole batch), the CIGAR text back to back, *cigar_total = the need;
   SWA_E_CAPACITY when the text does not fit or `cigar` is NULL with text to write — all other results are complete then, and
   a second call with room gives the same bytes.  Every rank writes diffs, columns and cigar_end at its slice's offset and
   its text where no other rank writes — the caller's buffer at the weight of the lower slices where the slice's bound fits
   there, else a buffer of its own —; the texts are then moved together in rank order and every rank's ends raised by the
   totals of the ranks below it.  A rank with an empty slice launches nothing, its counters are zero.  A failing rank ends
   the call with its code and "rank r: ..." in swa_multi_last_error, after every thread has been joined (an id >= n: SWA_E_ARG
   from the rank whose slice holds it; such a pair weighs nothing where the batch is divided).  SWA_E_ARG for a handle without a database when there are pairs.
   swa_multi_nw_batch_totals / _tiers / _text_full: the counters of swa_nw_batch_totals / _tiers / _text_full summed over the
   ranks.  The tier sums are those of a single context as long as no pair found a CIGAR buffer full (text_full = 0 on both
   sides: the device's text buffer is sized per slice).  A rank's own counters stay readable through swa_multi_ctx(m, r).
   swa_multi_nw_bounds_for: the division; a pure function, no device.  With w_k = seqlen[d_ids[k]] + seqlen[q_ids[k]] (also
   the bound of the pair's CIGAR), P(k) the sum of w_j over j < k and W = P(npairs): bounds[0] = 0, bounds[world] = npairs,
   and for 0 < r < world bounds[r] = the smallest k with P(k) >= floor(r W / world) (the product split, so that it stays
   inside 64 bits).  bounds holds world + 1 entries.  SWA_E_ARG for world = 0, world > 64, a null array with npairs > 0 or
   an id >= n.  The weight is a first rule: how a pair's cost follows its lengths across the tiers — cells grow with the
   product of the lengths and with the band, the host parts with the pair count and the text — has not been measured. */
int  swa_multi_nw_batch(swa_multi * m, uint64_t mismatch, uint64_t gapopen, uint64_t gapextend, uint64_t npairs,
                        const uint32_t * d_ids, const uint32_t * q_ids, uint32_t * diffs, uint32_t * columns,
                        uint64_t * cigar_end, char * cigar, uint64_t cigar_cap, uint64_t * cigar_total);
int  swa_multi_nw_batch_totals(swa_multi * m, uint64_t * out4);
int  swa_multi_nw_batch_tiers(swa_multi * m, uint64_t * out8);
int  swa_multi_nw_batch_text_full(swa_multi * m, uint64_t * out1);
int  swa_multi_nw_bounds_for(uint64_t npairs, const uint32_t * d_ids, const uint32_t * q_ids, const uint32_t * seqlen, uint32_t n,
                             uint32_t world, uint64_t * bounds);
/* Debug entry: the merge rank 0 runs on the gathered shares (k_merge_sorted_lists, launched as swa_multi_dn_graph launches
   it), from host arrays to host arrays on the context's stream.  List r = [at[r], at[r + 1]) of keys / vals, every list
   sorted by key, at[0] = 0, at[] not descending, 1 <= world <= 64 (SWA_E_ARG otherwise); out_keys / out_vals take
   at[world] entries: the lists merged by key, equal keys in list order.  at[world] = 0: nothing is launched or written. */
int  swa_merge_sorted_lists(swa_ctx * ctx, const uint64_t * keys, const uint32_t * vals, const uint64_t * at, uint32_t world,
                            uint64_t * out_keys, uint32_t * out_vals);

#ifdef __cplusplus
}
#endif
#endif /* SWARM_AMD_H */
