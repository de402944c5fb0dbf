// swa_internal.h — shared by the HIP translation units of libswarm_amd.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/swarm_amd.h"

// ---- device-side layout of one amplicon hash-table slot ----------------------------
// The reference keeps an occupied bitmap + u64 hash_values[] + u32 hash_data[]
// (src/hashtable.cc:41-44): three cache lines per probe step.  Here one 16-byte slot
// carries all three, so a probe step is ONE 16-B HBM/L2 transaction.
struct alignas(16) swa_slot {
  uint64_t hash;
  uint32_t amp;   // SWA_NO_AMPLICON = empty
  uint32_t pad;
};

// a growable device buffer (never shrinks; the db and tables stay resident in HBM)
struct swa_dbuf {
  void * ptr = nullptr;
  size_t bytes = 0;
};

// ---- the status block ----------------------------------------------------------------
// Every context owns one 4 KB block in HBM (d_status) and a pinned mirror of it (h_status): every small status array of
// the context, so that the host reads them with ONE copy per phase (a device-to-host copy of a few bytes is a kernel of
// its own, ~5 us with its gap: the d = 1 step made nine).  What a kernel writes here decides whether a step is repeated,
// fails with SWA_E_INTERNAL or returns SWA_E_DUPLICATES.  The members and the k* indices below are the whole contract:
// kernels get plain pointers to the arrays (or into them) and index them with the same names.
struct swa_status_block {
  uint32_t flags[16];            // kFlag*
  uint64_t stats[16];            // kStat* (cleared per network call)
  uint64_t guard[24];            // kGuard* (d1.hip: guard_check)
  uint64_t csr_end;              // the last CSR offset once more (k_csr_*: CsrArgs::end_copy)
  uint32_t links_sorted;         // links the partition of the CSR stage sorted (its total, 32 bits)
  uint32_t fallback_copy;        // counters[kCounterFallback] once more, in the head the host copies anyway (k_part_tiles<., true> / k_seg_reduce)
  uint32_t pad0[28];
  uint32_t host_unserved;        // (the end of the head that network_run copies; no longer written)
  uint32_t pad1[127];
  uint32_t counters[256];        // kCounter*: work counters of the d = 1 step (kCounterWords)
  uint64_t cursors[64];          // swa_d1_links_split: the run cursor of every rank; in the mirror [0] receives the links no rank owns
                                 // (swa_derep_route_slice: as 32-bit words, 64 counts and 64 run cursors; the mirror receives the counts)
  uint8_t pad2[1536];
};
static_assert(std::is_standard_layout<swa_status_block>::value, "status block: plain data");
static_assert(sizeof(swa_status_block) == 4096, "status block: 4 KB");
static_assert(offsetof(swa_status_block, flags) == 0 && offsetof(swa_status_block, stats) == 64 &&
              offsetof(swa_status_block, guard) == 192 && offsetof(swa_status_block, csr_end) == 384 &&
              offsetof(swa_status_block, links_sorted) == 392 && offsetof(swa_status_block, fallback_copy) == 396 &&
              offsetof(swa_status_block, host_unserved) == 512 &&
              offsetof(swa_status_block, counters) == 1024 && offsetof(swa_status_block, cursors) == 2048,
              "status block: the regions lie where the kernels and the debug reads expect them");

// flags[]: the d = 1 index build and step ...
constexpr uint32_t kFlagDuplicates = 0;    // identical sequences (k_dup_check; the prefix pass of the pair kernels: pair_twin)
constexpr uint32_t kFlagUnordered = 1;     // the database is not in abundance order (k_abundance_rank)
constexpr uint32_t kFlagKeyOverflow = 2;   // a bucket with more distinct keys than k_group1's table holds: partition finer
constexpr uint32_t kFlagUnserved = 3;      // a sequence too short for two windows: a seed the anchored passes cannot serve
constexpr uint32_t kFlagOversized = 4;     // groups left to the plain kernel (oversized / a member too long) ...
constexpr uint32_t kFlagOverMass = 5;      // ... and how many members they have
constexpr uint32_t kFlagShortest = 6;      // 0xFFFFFFFF - the shortest sequence
constexpr uint32_t kFlagsD1 = 7;           // (so many of them)
// ... the dereplication's count of amplicons left for the next round, ON THE WORD OF kFlagOversized: swa_derep drops the
// d = 1 index before its first round (swa_d1_index::table_repurposed), so no build or step reads the flag it overwrites
constexpr uint32_t kFlagDerepLeft = kFlagOversized;
// ... and the grouped join (group_join.inc: JoinTable::flags = flags + kFlagJoin), indexed from there:
constexpr uint32_t kFlagJoin = 8;
constexpr uint32_t kJoinKeyOverflow = 0;   // the key table is full
constexpr uint32_t kJoinItemOverflow = 1;  // more work items than the route's cap
constexpr uint32_t kJoinItemCount = 2;     // item counters: one for d >= 2, one a group type (+ 0..2) for --fastidious
constexpr uint32_t kJoinFlagWords = 5;
static_assert(kFlagsD1 <= kFlagJoin && kFlagJoin + kJoinFlagWords <= 16, "status block: flags");

// stats[]: [0, kStatSeg) unused; from kStatSeg on what k_seg_reduce makes of the per-wave segments, indexed from there:
constexpr uint32_t kStatSeg = 8;
constexpr uint32_t kSegLinks = 0;          // links found
constexpr uint32_t kSegFullest = 1;        // the fullest segment
constexpr uint32_t kSegStaged = 2;         // + pass: members the pair kernels staged

// guard[]: [0, kGuardCall) describe the index in place (cleared by the streaming build), two words each, + index:
constexpr uint32_t kGuardMade = 0;         // key records made (k_keys, k_set_guard_made)
constexpr uint32_t kGuardListed = 2;       // members of listed groups        (k_group1 relies on these three lying
constexpr uint32_t kGuardSingleton = 4;    // ... of singleton groups          two words apart in this order)
constexpr uint32_t kGuardOversized = 6;    // ... of groups left to the plain kernel
// [kGuardCall, kGuardKeys) belong to one network call (launch_network_anchored clears them at its start):
constexpr uint32_t kGuardCall = 8;
constexpr uint32_t kGuardMisfiled = 10;    // members found under an anchor key that is not theirs (the pair kernels)
// k_group1 counts a bucket whose member total disagrees with its record count into THE SAME WORD while the index is
// BUILT: the clear of the next network call wipes that count before guard_check reads the word, so it never reaches the
// host.  Kept as it is (what the guard reports is unchanged); a word of its own, in [0, kGuardCall), would make it count.
constexpr uint32_t kGuardBucketTotal = kGuardMisfiled;
// [kGuardKeys, 24): the second opinion on the key records, once per uploaded database (cleared before it is taken): two
// triples, the third word of each — once the fingerprints' sum — unused
constexpr uint32_t kGuardKeys = 16;
constexpr uint32_t kGuardKeysDb = 16;      // + index: sums from the packed database (k_guard_db)
constexpr uint32_t kGuardKeysRec = 19;     // + index: sums of the partitioned records (k_guard_records)

// counters[]: the streaming build clears all of them, every network call [0, kCounterBase)
constexpr uint32_t kCounterFallback = 2;   // seeds (or halves of seeds) listed for the plain kernel (k_stream_fallback)
constexpr uint32_t kCounterSchedBig = 8;   // + 2 (kWidthClasses pass + class): work counter of the 65..pair_big groups of k_d1_group_pairs
constexpr uint32_t kCounterSchedTiled = 9; // + 2 (kWidthClasses pass + class): work counter of k_d1_pairs_tiled
constexpr uint32_t kCounterBase = 64;      // + (index * kWidthClasses + class) * 8 + kind: items in that work list (k_group_lists)
constexpr uint32_t kCounterWords = 256;
static_assert(kCounterWords * sizeof(uint32_t) == sizeof(swa_status_block::counters), "status block: counters");

// ---- the device counters of the --fastidious pass ---------------------------------------------------------------------
// d_fcounters as fastidious.hip lays it out (dn_graph.hip keeps a layout of its own in the same buffer for its own pass).
// As with the status block the members are the whole contract: kernels get plain pointers to them, the host copies
// neighbouring members with one copy.  unsigned long long: what the kernels' atomics take.
struct swa_fast_counters {
  unsigned long long light_variants;   // sum of |V1(x)| over the light amplicons (k_fast_variant_totals: counters[0]) ...
  unsigned long long heavy_variants;   // ... and over this shard's heavy ones (counters[1])
  unsigned long long candidates;       // graft candidates (k_d1_probe<., 1>, k_fast_count*)
  unsigned long long batch_tasks;      // Bloom route, the current batch of heavy amplicons: tasks k_d1_flex<., 1> made ...
  unsigned long long batch_variants;   // ... and microvariants it tested (cleared and read together with the tasks)
  unsigned long long pairs;            // pair route: (heavy, light) pairs within two edits
  unsigned long long bands[3];         // k_fast_band_lists: light / heavy amplicons of the Bloom route's bands, nucleotides of those light ones
  unsigned long long scratch;          // the variant count of the Bloom route's light side: written, never read
  unsigned long long pad0[2];
  uint32_t length_classes[4];          // k_fast_length_classes: longest sequence <= cap, amplicons > cap, amplicons >= cap - 1, unused
  unsigned long long pad1[2];
};
static_assert(std::is_standard_layout<swa_fast_counters>::value, "fastidious counters: plain data");
static_assert(sizeof(swa_fast_counters) == 128, "fastidious counters: sixteen 64-bit words");
static_assert(offsetof(swa_fast_counters, light_variants) == 0 && offsetof(swa_fast_counters, heavy_variants) == 8 &&
              offsetof(swa_fast_counters, candidates) == 16 && offsetof(swa_fast_counters, batch_tasks) == 24 &&
              offsetof(swa_fast_counters, batch_variants) == 32 && offsetof(swa_fast_counters, pairs) == 40 &&
              offsetof(swa_fast_counters, bands) == 48 && offsetof(swa_fast_counters, scratch) == 72 &&
              offsetof(swa_fast_counters, pad0) == 80 && offsetof(swa_fast_counters, length_classes) == 96 &&
              offsetof(swa_fast_counters, pad1) == 112,
              "fastidious counters: every member lies on the word the pass has always used for it");

// dn_graph.hip keeps a count per sequence length below this: 16 (d + 1) + d for d <= 16, the lengths a short sequence can pair with
#define SWA_DN_HIST_LEN 288u

// ---- the context's state, by lifetime ----------------------------------------------------------
// A member that is a fact OF something lies in that something's group, default-initialised to "nothing there": ending a
// lifetime is `group = {}`.  What lives as long as the context (buffers, capacities, the owner ...): in swa_ctx.

// facts of the uploaded database (ended by swa_db_upload* / swa_db_attach)
struct swa_db_facts {
  // ... those the d = 1 step derives from the packed database: a guard retry (d1.hip: network_run_guarded) makes them again
  struct d1_facts {
    bool rank_ready = false;       // d_arank holds the abundance ranks of this database
    bool db_unordered = false;     // ... which is not in abundance order (the anchored passes are then not used)
    bool props_ready = false;      // db_shortest / class_pop below
    uint32_t db_shortest = 0;      // shortest sequence
    uint32_t class_pop[8] = {};    // sequences per width class (d1_anchor.inc: width_class; [kTooLong]: beyond the pair kernels)
    bool windows_ready = false;    // the anchor windows of this database are known (choose_anchor_windows + the safety net):
    uint32_t windows_chosen = 0;   // anchor_a = anchor_b = this
    uint32_t windows_w = 32;       // ... and anchor_w = this
    // the window sample as choose_anchor_windows saw it (its scratch is reused by the build: this host copy is all that is
    // left of it) and what it chose from it, before the safety net of the first build may replace windows_chosen
    bool sample_taken = false;     // a sample was drawn for this upload (not under SWA_D1_WINDOWS=0)
    uint32_t sample_stats[8] = {}; // [0..4) sampled amplicons too short for candidate offset 32 c, [4..8) their stranded mass
    uint32_t sample_stride = 0, sample_count = 0;   // every sample_stride-th amplicon, sample_count of them
    uint32_t sample_offset = 0, sample_w = 32;      // the choice made from the sample: anchor_a = anchor_b, anchor_w
    bool lines_ready = false;      // d_lines holds this database's amplicon lines (made once per upload), lines_w words each
    uint32_t lines_quads = 0;      // ... of this many 16-byte quads each (4, 8 or 16)
    // length classes of the database against the pair route's cap (k_fast_length_classes; read once per upload, and only
    // where the longest sequence exceeds the cap: by the pass under SWA_FAST_LONG=split or =pairs, by swa_d1_fastidious_split always): the longest sequence <= cap (0: none), amplicons > cap, amplicons >= cap - 1
    bool fast_classes_ready = false;
    uint32_t fast_classes_cap = 0;  // ... the cap they were read against (SWA_FAST_LONG=pairs has its own)
    uint32_t fast_pair_longest = 0, fast_n_long = 0, fast_n_band = 0;
    bool guard_keys_done = false;  // the key records of this upload have had their second opinion (k_guard_db / k_guard_records)
    bool guard_keys_pending = false;   // ... its sums, guard[kGuardKeys ..), wait for the next guard_check
    uint32_t stream_extra_bits = 0;   // finer partition after a bucket held more distinct keys than the group kernel's table
  } d1;
  // the uclust alignments (nw_trace.hip): the database's lengths on the host (filled by the first swa_nw_batch after an upload)
  std::vector<uint32_t> nw_seqlen;
  bool qgram_ready = false, scan_ready = false;
  // d >= 2 in bulk (dn_graph.hip): the graph of all pairs within d differences, kept sorted on the device
  bool dn_graph_ready = false, dn_graph_ncb = false;
  uint32_t dn_shortest = 0;      // shortest sequence of the database (0 = not measured yet)
  // ... with it: how many sequences have each length below SWA_DN_HIST_LEN, and the shortest of the others (none: ~0).
  // What window_length() decides everything from: the shortest LONG sequence, the short ones and their candidates B.
  uint32_t dn_len_hist[SWA_DN_HIST_LEN] = {};
  uint32_t dn_shortest_rest = 0xFFFFFFFFu;
};

// the d = 1 index in place (ended when an index build starts: d1.hip, index_build)
struct swa_d1_index {
  bool d1_ready = false;
  uint64_t table_size = 0;       // slots, power of two
  uint64_t bloom_words = 0;      // u64 words in the amplicon Bloom
  // anchored d=1 index (d1_anchor.inc, d1_stream.inc): [0] prefix groups, [1] suffix groups
  bool anchor_usable = false;    // decided by swa_d1_index_build: lengths fit, db order holds, not switched off
  bool anchor_ready = false;     // the streaming index below exists (for the owner in owner_rank / owner_world)
  bool full_index = false;       // d_seqhash / d_aux cover ALL amplicons and d_table / d_bloom are built (swa_ensure_full_index)
  uint32_t anchor_a = 0, anchor_b = 0;   // anchor windows moved inwards by this many nt ("window mode", chosen at index build)
  uint32_t anchor_w = 32;        // width of the anchor windows in nt: 32, 64 or 128 (wider: fewer pairs per group; needs 2 w + 1 nt)
  bool head_clear_pending = false;   // index_build has left the clear of the status block's head to the streaming build's own clear
  bool guard_index = false;      // guard[0, kGuardCall) of the status block describe the index in place (made by the streaming build since the last clear)
  // streaming index build (d1_stream.inc) / CSR assembly (d1_part.hip)
  uint32_t list_counts[2 * 4 * 8] = {};   // items per work list of the index in place ([index][width class][8]: the status block's counters + kCounterBase)
  bool list_counts_ready = false;
  uint64_t list_regions_items = 0;   // entries of an index's item buffer (d1.hip: list_regions)
  bool stream_index = false;     // the anchor indexes in place were made by the streaming build: members = ids in d_members
  // the key partition of the index in place, as swa_d1_part_plan reports it, and where its bucket starts lie (u64 entries
  // into d_stream[kSbStart + i]; the link partition of a network call reuses those buffers: part_starts_valid falls then)
  uint32_t part_plan[8] = {};
  int lists_form = -1;           // the work lists of the index in place: 1 positions inside k_group_lists, 0 the two-launch scan (swa_d1_lists_form)
  uint64_t part_starts_at = 0;
  uint32_t part_buckets = 0;
  bool part_starts_valid = false;
  // member index: hash table + Bloom of the members of oversized groups only (what the plain kernel probes for them)
  bool member_index = false, only_oversized = false;
  uint32_t over_mass = 0;
  uint64_t mtable_size = 0, mbloom_words = 0;
  uint32_t index_first = 0, index_count = 0;   // the range of the last index build (network_run_guarded repeats it)
  bool index_routed = false;

  // A partial end: the owner changed (swa_d1_set_ownership).  The database-wide table, if built, serves any owner (d1_ready,
  // full_index stay); the streaming index and the member table were the previous owner's: the next network call makes this one's
  void owner_changed() { anchor_ready = false; member_index = false; }
  // ... and d_table / d_bloom were given another content (swa_derep; the Bloom route of --fastidious, which goes on to
  // fill the table it has the size of): nothing is served until the next build, which ends the rest
  void table_repurposed() { d1_ready = false; full_index = false; anchor_ready = false; }
};

// the network resident in d_offsets_tmp / d_nb_tmp and its clustering (cluster_gpu.hip); ended with the index it was made from
struct swa_resident {
  bool csr_ready = false;
  bool csr_has_diffs = false;                 // the resident network is a d >= 2 graph: one byte of differences per link behind the neighbours
  uint64_t csr_total = 0;
  bool cluster_ready = false;                  // swa_d1_cluster_device's arrays lie in d_cluster (swa_d1_cluster_fetch)
  uint32_t cluster_maxgen = 0;
  uint32_t cluster_effort[3] = {};             // of the last swa_d1_cluster_device call: label sweeps launched, restarts of their numbering, level batches
  uint32_t cluster_nswarms = 0;                // swarms of the clustering in place
  // what --fastidious derives from the clustering in place and keeps in HBM (fast_graft.inc); ended with it
  struct fastidious_facts {
    bool sums_ready = false;                   // d_swarm_sums: mass | sumlen | singletons | maxgen of every swarm
    bool sums_grafted = false;                 // ... grown by swa_d1_graft_device (its next call makes the swarms' own sums again first)
    bool roles_ready = false;                  // d_swarm_role: 0 light / 1 heavy per amplicon, against the boundary of the last flags call
    uint64_t light_amps = 0;                   // ... and how many amplicons it found in light swarms
    bool cand_ready = false;                   // d_graft: the candidates of a whole swa_d1_fastidious* pass (or a caller's) over this clustering
    bool owners_ready = false;                 // d_shard_owner: the owner byte of every amplicon, made from d_swarm_role (swa_d1_shard_owners_device)
    uint32_t owners_shards = 0;                // ... for so many shards,
    uint64_t owners_heavy = 0;                 // and how many heavy amplicons it counted
    bool grafts_ready = false;                 // d_graft_work: the grafts of a completed swa_d1_graft_device, in chain order,
    uint32_t grafts = 0;                       // ... so many of them (0: the call made none)
    bool layout_ready = false;                 // d_graft_layout: the grafted clustering laid out (swa_d1_graft_layout_device),
    uint32_t layout_largest = 0;               // ... and the members of its largest printed swarm
    // what ends the candidates ends the grafts made from them and their layout (as does the next swa_d1_graft_device call)
    void candidates_end() { cand_ready = false; grafts_ready = false; layout_ready = false; }
  } fast;
  // what the d >= 2 graph route derives from the clustering in place and keeps in HBM (dn_tables.inc): every member's radius,
  // the deepest radius of every swarm, the -i links in acceptance order; ended with the clustering
  struct dn_tables_facts {
    bool ready = false;                        // d_dn_tables holds them (swa_dn_tables_fetch)
    uint64_t nlinks = 0;                       // n - swarms
    uint32_t radius_at = 0;                    // which of the two jumping buffers the last round wrote
    uint64_t serial = 0;                       // which swa_dn_tables_device call of this context made them (swa_dn_tables_serial)
  } tables;
};

// the dereplication in place (derep.hip): ended by swa_db_upload* / swa_db_attach, by the start of every swa_derep* (on every
// rank of a swa_multi by the start of every swa_multi_derep*, which leaves a new one on rank 0 alone) and by
// every call that writes d_graft, where its array lies (the --fastidious pass, swa_d1_graft_device with a caller's candidates)
struct swa_derep_facts {
  bool first_ready = false;      // d_graft holds first_identical[] of the database in place (swa_derep_resident)
  bool tables_ready = false;     // d_d0 / d_d0_tab hold the clusters made from it (swa_d0_cluster_device; swa_d0_cluster_fetch)
  uint32_t clusters = 0;         // ... so many of them,
  uint32_t largest = 0;          // the members of the largest
  uint64_t heaviest = 0;         // and the mass of the heaviest
};

struct swa_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int num_cus = 256;
  size_t max_lds = 65536;        // the most dynamic LDS a workgroup of this device can be given (opted in per kernel)
  std::string err;

  // optional per-kernel timing (HIP events on `stream`)
  bool timing = false;
  hipEvent_t ev[32] = {};
  bool ev_ready = false;
  bool ev_used[16] = {};

  swa_db_facts up;               // what is known of the uploaded database
  swa_d1_index ix;               // the d = 1 index in place
  swa_resident res;              // the resident network and its clustering
  swa_derep_facts dr;            // the dereplication in place and its cluster tables

  // database (device pointers)
  swa_db_view db{};
  bool db_owned = false;
  swa_dbuf d_seqs, d_seq_off, d_seqlen, d_abund;

  // d=1 index
  uint32_t zobrist_len = 0;      // positions in the Zobrist table (longest + 2; set by whoever hashes: swa_prepare_hashing)
  uint32_t zobrist_resident = 0; // length of the table currently in d_zobrist (0 = none)
  bool patterns_resident = false;
  swa_dbuf d_zobrist, d_seqhash, d_table, d_bloom, d_patterns;
  swa_dbuf d_status;             // one swa_status_block in HBM (swa_status(ctx): its device address) ...
  swa_status_block * h_status = nullptr;   // ... and its mirror in pinned host memory: where the host looks at what it copied
  swa_dbuf d_edges;              // u64 edge list (src << 32 | dst)
  swa_dbuf d_counts, d_cursor, d_scan_tmp, d_offsets_tmp, d_nb_tmp;
  uint32_t owner_rank = 0, owner_world = 1;   // swa_d1_set_ownership: this context serves the anchor groups of one rank
  // d_akeys[0] / d_acounts[0]: scratch of the window sample; d_aitems: the work lists of the two indexes
  swa_dbuf d_aux, d_akeys[1], d_acounts[1], d_aitems[2];
  swa_dbuf d_afallback, d_arank, d_rank_tmp;
  swa_dbuf d_seg_fill;           // u32 fill of every per-wave edge segment
  swa_dbuf d_seg_base;           // u64 start of every segment in the compacted edge list (swa_d1_network_edges_device)
  uint64_t seg_cap = 0;          // entries per segment

  // q-gram / alignment state
  swa_dbuf d_qgrams, d_list_a, d_list_b, d_list_c, d_list_d;
  uint64_t pen_mismatch = 18, pen_gapopen = 24, pen_gapextend = 13, resolution = 1;
  bool search_ready = false;
  uint32_t wfa_steps = 0;        // > 0: the wavefront alignment kernel is exact for the penalties / d in use
  uint32_t wfa_ring = 0;         // steps of history k_align_wfa keeps (the furthest a step looks back + 1)
  uint32_t align_lds_opt_in = 0; // the align kernels (bit = swa_align_form) whose dynamic-LDS attribute is set to max_lds
  swa_dbuf d_wfa;

  // fused d >= 2 scan state (scan.hip)
  swa_dbuf d_scan_est, d_scan_swarmed, d_scan_targets, d_scan_diffs, d_scan_hits, d_scan_counters;
  swa_dbuf d_scan_cand;          // candidate list of the current swarm (scan.hip)
  swa_dbuf d_scan_seeds;         // seeds + limits of the current batch
  swa_dbuf d_scan_compares;      // q-gram comparison counts, one slot per workgroup
  uint32_t scan_cand_bound = 0;
  void * h_scan_pinned = nullptr;   // pinned, GPU-visible: seeds + limits in, hit mirror out
  std::vector<uint32_t> scan_host, scan_perm, scan_idx_tmp;
  std::vector<uint64_t> scan_sorted;
  uint64_t scan_pair_cap = 0;
  uint64_t scan_launches = 0;
  uint64_t scan_compare_discount = 0;   // comparisons of passes that overflowed the pair arrays and were redone
  uint64_t scan_redone = 0, scan_relists = 0, scan_by_copy = 0;   // swa_scan_debug_state
  uint32_t scan_rank = 0, scan_world = 1;   // swa_scan_set_ownership: the part of the pool this context scans

  // fastidious state
  swa_dbuf d_light, d_graft, d_bloomflex, d_fpatterns, d_queue, d_fcounters;
  // pair route (d1_fast.inc): roles, group key table + counters, offsets, slot of every amplicon, member lists,
  // work items, the (heavy, light) pairs within two edits
  swa_dbuf d_frole, d_fkeys, d_fcnt, d_foff, d_fslot, d_fmembers, d_fitems, d_fpairs;
  uint64_t fast_pair_cap = 0;
  uint64_t fast_totals[4] = {};  // of the last pass: pairs found, light / heavy amplicons of the Bloom route's bands, attempts of the pair list
  uint64_t fast_batches[4] = {}; // of the last pass's Bloom route: k_d1_flex<., 1> launches, those that overflowed and were redone, the task cap, the most tasks of a batch that ran
  uint64_t fast_bloom[5] = {};   // ... and its filter: words (fsize), m, k, the bits asked for, tasks of the batches that ran to the end; all 0 when the route
                                 // did not run, and after an upload (d_bloomflex then holds another database's filter): swa_d1_fastidious_bloom_read

  // d >= 2 in bulk (dn_graph.hip)
  uint64_t dn_pair_cap = 0, dn_comparisons = 0, dn_aligned = 0, dn_launches = 0, dn_edges = 0, dn_work = 0;
  swa_dbuf d_dn_keys, d_dn_vals;
  uint32_t dn_owner_rank = 0, dn_owner_world = 1;   // swa_dn_set_ownership: this context finds the pairs of the window groups (and short sequences) it owns

  swa_dbuf d_stream[30];         // streaming index build (d1_stream.inc) / CSR assembly (d1_part.hip): indexed by kSb* (below)

  uint32_t guard_retries = 0;                  // steps repeated after the guard found counts that did not balance
  swa_dbuf d_words_stage;                      // swa_db_stage_words: the reader's word pools, file order
  const void * staged_first = nullptr; uint64_t staged_words = 0;
  int pair_blocks[4] = {};                      // workgroups of k_d1_group_pairs a CU holds, per width class (0: not asked yet)
  bool g1_lds_opt_in = false;                  // k_group1's dynamic-LDS attribute has been set on this context's device
  bool part_lds_opt_in = false;                // ... and the wide-tile form of k_part_scatter
  uint32_t pair_lds_opt_in = 0;    // ... and the W = 15 / 21 forms of k_d1_group_pairs (pass + 2 (W = 21) + 4 (NW = 2) + 8 (NW = 4))
  swa_dbuf d_cluster, d_cluster_ctl;
  // --fastidious on the clustering in place (fast_graft.inc): the per-swarm sums, the role byte of every amplicon, and the
  // grafting's slots, winner lists and result arrays
  swa_dbuf d_swarm_sums, d_swarm_role, d_graft_work;
  // the grafted clustering as one layout (fast_graft.inc: GraftLayout): the member order as the writers print it, and per swarm
  // where its members lie in it, how many it has with everything grafted, whether it hangs on another
  swa_dbuf d_graft_layout;
  // the shard owner of every amplicon (fast_graft.inc): owner u8[n + 4, rounded up to 8] | tile bases u64[tiles + 1] | tile counts u32[tiles];
  // on the other ranks of a swa_multi the owner bytes alone, as rank 0 sent them
  swa_dbuf d_shard_owner;
  // d >= 2 on the clustering in place (dn_tables.inc): jumping buffers, positions, sort keys, the four link arrays
  swa_dbuf d_dn_tables;
  uint64_t dn_tables_made = 0;                 // swa_dn_tables_device calls of this context that left tables
  // d = 0 (derep.hip): the grouping's work arrays with the member order (n words each), and the cluster tables
  swa_dbuf d_d0, d_d0_tab;

  // the uclust alignments (nw_trace.hip): the pairs per tier of the last batch (three LDS tiers, four wide tiers, host), how
  // many of them the widest tier certified but found the text buffer full, and the device buffers of one slice (d_nw_bits: the wide tiers'
  // direction bits, one slot per wave; reserved on every run, 256 slots at least for what the LDS tiers may pass down)
  uint64_t nw_totals[8] = {};
  uint64_t nw_text_full = 0;
  swa_dbuf d_nw_ids, d_nw_lists, d_nw_res, d_nw_text, d_nw_gather, d_nw_bits;
};

// the buffers of d_stream[]; where two are named, one per index (+ i), the records ping / pong per index (+ 2 i + h)
enum { kSbLines = 0,             // the amplicon lines
       kSbRec = 1,               // [1..4] key records
       kSbCnt = 8, kSbTile = 10, kSbStart = 12, kSbPartial = 14,   // the partition's flat counts, tile tables, chunk starts, scan partials
       kSbScal = 16,             // scalars
       kSbMembers = 17,          // [17, 18] ids in group order
       kSbOver = 19,             // oversized-group bits, a byte an amplicon
       kSbKind = 20,             // [20, 21] items per list kind
       kSbLinkA = 22, kSbLinkB = 23,   // link sort: records ping, pong
       kSbHeavy = 24,            // buckets of the CSR stage left to whole workgroups
       kSbMTable = 26, kSbMBloom = 27,   // member table and its Bloom filter
       kSbSched = 28 };          // work counters of k_d1_group_pairs

// the device address of the context's status block: for taking the addresses of members (kernel arguments, copies, fills),
// never to be dereferenced on the host — the host reads ctx->h_status after a copy
inline swa_status_block * swa_status(const swa_ctx * ctx) { return static_cast<swa_status_block *>(ctx->d_status.ptr); }

int swa_fail(swa_ctx * ctx, int code, const char * what, hipError_t e);
int swa_fail_msg(swa_ctx * ctx, int code, const std::string & msg);
// SWARM_AMD_STEP_TIMING=1: wall-clock laps between the host-visible points of the d = 1 index build and network call, on
// stderr (what a first step in a fresh process is made of; the device is synchronised at each lap, so the numbers are
// not the pipelined step's)
inline void swa_lap(swa_ctx * ctx, const char * what);
int swa_reserve(swa_ctx * ctx, swa_dbuf & buf, size_t bytes);   // grow-only hipMalloc
void swa_release(swa_dbuf & buf);
int swa_hash_sequences(swa_ctx * ctx);                           // d1.hip: Zobrist table + d_seqhash + d_aux

// ---- what multi.hip takes from scan.hip: one batch of the fused d >= 2 scan in two halves ---------------------------------
// the arguments of swa_scan_batch; seeds and radii stay the caller's and valid until swa_scan_finish has returned
struct swa_scan_call {
  uint32_t nseeds;
  const uint32_t * seeds, * radii;
  uint32_t lowest_unswarmed;
  int first_generation, no_cluster_breaking;
};
// nullptr, or why swa_scan_batch refuses these arguments
const char * swa_scan_check_call(const swa_ctx * ctx, const swa_scan_call & call, const uint32_t * hit_seedidx, const uint32_t * hit_ids,
                                 const uint32_t * hit_diffs, uint32_t cap, const uint32_t * nhits);
// nw_trace.hip: the lengths of the resident database on the host (ctx->up.nw_seqlen), downloaded once a database — what
// swa_nw_batch sorts its pairs into tiers by, and swa_multi_nw_batch divides them among the ranks by
int swa_nw_host_seqlen(swa_ctx * ctx);
int swa_scan_enqueue(swa_ctx * ctx, const swa_scan_call & call);                  // the launch sequence on ctx->stream; does not wait
int swa_scan_finish(swa_ctx * ctx, const swa_scan_call & call, uint32_t * nhits); // waits; redoes an overflowed pass; leaves the sorted hits for swa_scan_fetch

// ---- what fastidious.hip takes from d1.hip ----------------------------------------------------------------------------
// Host functions, defined in d1.hip (swa_scan_offsets: in d1_part.hip), whose kernels stay in that unit's code object.  All enqueue on ctx->stream and return SWA_OK
// or the error they recorded.
int swa_prepare_hashing(swa_ctx * ctx);        // the Zobrist table for this database's longest sequence in HBM (uploaded when its length changes), room for d_seqhash / d_aux
int swa_ensure_full_index(swa_ctx * ctx);      // hashes of ALL amplicons, the database-wide table and its Bloom filter: built unless swa_d1_index::full_index says they stand
int swa_launch_abundance_rank(swa_ctx * ctx);  // d_arank, once per upload; raises (or restores) kFlagUnordered
int swa_ensure_lines(swa_ctx * ctx);           // the amplicon lines (d_stream[kSbLines]), once per upload and line width; needs the abundance ranks
int swa_grid_for(const swa_ctx * ctx, uint64_t items, int per_block, int max_per_cu);   // workgroups for `items` at per_block each: 1 .. num_cus * max_per_cu
// exclusive scan of counts[0, n) into the 64-bit offsets[0, n] (three launches); the caller has reserved d_scan_tmp: a uint64_t
// per kScanOffsetsTile counts
constexpr uint32_t kScanOffsetsTile = 2048;
int swa_scan_offsets(swa_ctx * ctx, const uint32_t * counts, uint32_t n, uint64_t * offsets);
// d_table / d_bloom cleared and refilled with the amplicons whose byte in d_is_member is not 0 (nullptr: all of them);
// hashes and room as swa_ensure_full_index left them
int swa_d1_rebuild_table(swa_ctx * ctx, const uint8_t * d_is_member);
// dn_graph.hip, for multi.hip: the (partial, under ownership) graph computed and left sorted in HBM — d_dn_keys / d_dn_vals
// from entry dn_work on, dn_edges entries —, and a sorted (query << 32 | target, diff) list written out as the CSR of swa_dn_graph
int swa_dn_graph_compute(swa_ctx * ctx, int no_cluster_breaking);
int swa_dn_graph_emit(swa_ctx * ctx, const unsigned long long * sorted, const uint32_t * svals, uint64_t nedges, uint64_t * offsets,
                      uint32_t * neighbours, uint8_t * diffs, uint64_t cap, uint64_t * total);
// ... or left in HBM as the resident network (the tail of swa_dn_graph_resident: offsets, neighbours | diffs, csr_has_diffs)
int swa_dn_graph_install(swa_ctx * ctx, const unsigned long long * sorted, const uint32_t * svals, uint64_t nedges);
// cluster_gpu.hip (fast_graft.inc), for fastidious.hip: role[a] = 0 where owner[a] is 255 (light), 1 where it is `shard`, else 2;
// both arrays in HBM, n bytes (the owners reserved with four more)
int swa_d1_roles_from_owners(swa_ctx * ctx, const uint8_t * d_owner, uint32_t shard, uint8_t * d_role);
// fastidious.hip, for multi.hip: the pass of swa_d1_fastidious_shard with its roles made on the device from owner bytes in this
// context's HBM (n_light / n_heavy: the light amplicons and this shard's heavy ones); the candidates are left in d_graft and come
// home only when graft_cand is not null
int swa_d1_fastidious_owned(swa_ctx * ctx, const uint8_t * d_owner, uint32_t shard, uint64_t n_light, uint64_t n_heavy, uint64_t light_nt,
                            uint32_t bloom_bits, uint32_t * graft_cand, uint64_t * counters);

// derep.hip, for multi.hip (swa_multi_derep_resident): the steps of one rank.  Every one returns with the context's stream
// synchronised: the exchange between them runs on other contexts' streams, which do not order against this one.
// A rank's outgoing records: the hashes of its slice, then the (hash, id) records in owner order — two arrays, one position
struct swa_derep_routed {
  uint64_t * slice_hash, * hash; uint32_t * id;
  static uint64_t bytes(uint64_t count) { return (2 * (count + (count & 1u)) + 2) * sizeof(uint64_t) + (count + 2) * sizeof(uint32_t); }
  explicit swa_derep_routed(void * base, uint64_t count) {
    slice_hash = static_cast<uint64_t *>(base);                  // (16-byte aligned: k_derep_route reads two at a time)
    hash = slice_hash + count + (count & 1u);
    id = reinterpret_cast<uint32_t *>(hash + count + (count & 1u));
  }
};
// ... and what a rank received: the same two arrays
struct swa_derep_inbox {
  uint64_t * hash; uint32_t * id;
  static uint64_t bytes(uint64_t count) { return (count + 2) * sizeof(uint64_t) + (count + 2) * sizeof(uint32_t); }
  explicit swa_derep_inbox(void * base, uint64_t count) { hash = static_cast<uint64_t *>(base); id = reinterpret_cast<uint32_t *>(hash + count); }
};
uint32_t swa_derep_owner_of(uint64_t hash, uint32_t world);     // the rank that dereplicates every read with this round-0 hash
// the previous dereplication of this context ends; hashes [first, first + count) and routes them by owner into `work`
// (reserved here, laid out as swa_derep_routed(work.ptr, count)); counts[world] on the host
int swa_derep_route_slice(swa_ctx * ctx, uint32_t first, uint32_t count, uint32_t world, swa_dbuf & work, uint32_t * counts);
// the owner's rounds over the `received` records of its inbox (device arrays); packed[t] = first_identical << 32 | id of
// record t (device, `received` words); *rounds = how many rounds ran
int swa_derep_owner_rounds(swa_ctx * ctx, const uint64_t * in_hash, const uint32_t * in_id, uint32_t received, uint64_t * packed, uint32_t * rounds);
// rank 0: the n packed words of all owners (device) into d_graft; leaves the state of swa_derep_resident
int swa_derep_home(swa_ctx * ctx, const uint64_t * packed);

// RAII-less timing brackets: swa_t0(ctx, slot) ... swa_t1(ctx, slot).  The slots: swa_timing_read reports [0, 8),
// swa_timing_read_stream [8, 16), both by position (include/swarm_amd.h)
enum { kTimeSeqhash = 0, kTimeTable = 1, kTimeDupCheck = 2, kTimeNetwork = 3, kTimeCsr = 4,
       kTimePairs = 5,           // --fastidious: light pass; d >= 2: groups + pairs
       kTimeAlign = 6,           // --fastidious: heavy pass; d >= 2: alignments + CSR
       kTimeIndex = 7,           // the whole anchored-index build
       kTimeKeys = 8, kTimeKeyPartition = 9, kTimeGroups = 10,
       kTimePass = 11,           // + pass: the pair kernels of the prefix / suffix groups
       kTimeLinkPartition = 13, kTimeCsrRows = 14, kTimeLines = 15 };
inline void swa_t0(swa_ctx * ctx, int slot) {
  if (ctx->timing && ctx->ev_ready) { (void)hipEventRecord(ctx->ev[2 * slot], ctx->stream); }
}
inline void swa_t1(swa_ctx * ctx, int slot) {
  if (ctx->timing && ctx->ev_ready) { (void)hipEventRecord(ctx->ev[2 * slot + 1], ctx->stream); ctx->ev_used[slot] = true; }
}

#define SWA_HIP(ctx, expr)                                                     \
  do {                                                                         \
    hipError_t e_ = (expr);                                                    \
    if (e_ != hipSuccess) return swa_fail((ctx), SWA_E_DEVICE, #expr, e_);     \
  } while (0)

#define SWA_TRY(expr)                  \
  do {                                 \
    int rc_ = (expr);                  \
    if (rc_ != SWA_OK) return rc_;     \
  } while (0)

// host-side table generators (host_tables.cpp): bit-identical to the reference's
// first zobrist_init()/bloom_init()/bloomflex_init() of a process
void swa_zobrist_table(uint32_t zobrist_len, std::vector<uint64_t> & tab);    // src/zobrist.cc:49-80
void swa_bloom_patterns(uint32_t count, uint32_t k, std::vector<uint64_t> & pat); // src/bloompat.cc:74-90, src/bloomflex.cc:72-88
uint64_t swa_hashtable_size(uint64_t n);                                       // src/utils/hashtable_size.cc:29-42

// Every choice of the --fastidious pass (host_tables.cpp: pure arithmetic; fastidious.hip launches from it, swa_d1_fastidious_plan
// and swa_d1_fastidious_plan_for report it)
#define SWA_FAST_MIN_LEN 112u                       // both sequences at least this long => the pair route is complete (d1_fast.inc)
#define SWA_MAX_ZOBRIST_LDS (96u * 1024u)           // the Zobrist table sits in LDS up to this many bytes
struct swa_fast_plan {
  bool pair_route;               // false: the Bloom route for every pair
  int pair_w;                    // k_fast_pairs_lines<., W>: 5, 8, 13; 0 = k_fast_pairs on the packed words
  int count_w;                   // k_fast_count_sites<W>: 5, 8; 0 = k_fast_count, or
  bool count_words;              // k_fast_count_sites_words (SWA_FAST_LONG=pairs, SWA_FAST_COUNT=sites)
  int count_waves;               // k_fast_count / k_fast_count_sites_words: waves per block, slots of a wave's set (0: no set), dynamic LDS
  uint32_t slots;
  size_t count_lds;
  bool zobrist_lds;              // Bloom route: the Zobrist table sits in LDS
  bool split;                    // SWA_FAST_LONG=split in effect: pairs with a member longer than max_len take the Bloom route
  uint32_t served;               // the longest sequence the pair route holds: the database's, under the split pair_longest
  uint32_t max_len;              // the longest sequence the pair route takes (0xFFFFFFFF: no bound)
  int long_mode;                 // the division at the long end in effect: 0 none, 1 SWA_FAST_LONG=split, 2 =pairs
};
size_t swa_fast_count_lds(uint32_t longest, uint32_t slots, int waves);
uint32_t swa_fast_count_slots(uint32_t longest);
uint32_t swa_fast_cap();
swa_fast_plan swa_fast_plan_for(uint32_t longest, uint32_t pair_longest, bool split, bool bloom, bool words);
size_t swa_fast_sites_lds(uint32_t longest, int waves);         // k_fast_count_sites_words
uint32_t swa_fast_sites_cap();
uint32_t swa_fast_sites_cap_in_effect(uint32_t sites_cap);
// ... with every switch: long_mode 0 / 1 = split / 2 = pairs, SWA_FAST_COUNT=sites, SWA_FAST_SITES_CAP (0: derived)
swa_fast_plan swa_fast_plan_modes(uint32_t longest, uint32_t pair_longest, int long_mode, bool bloom, bool words, bool count_sites,
                                  uint32_t sites_cap);
void swa_fast_plan_report(const swa_fast_plan & p, uint32_t out[8]);

// The forms of the two partitions of the d = 1 step (host_tables.cpp: pure arithmetic; d1.hip and d1_part.hip launch from it,
// swa_d1_part_plan_for / swa_d1_csr_plan_for / swa_d1_part_plan report it)
#define SWA_PART_MAX_BITS 9u                        // bits per partition level (512 bins); the one-level key partition takes 10
#define SWA_PART_WIDE_BITS 10u
#define SWA_G1_TARGET 10240u                        // records per bucket the key partition aims at (k_group1)
#define SWA_CSR_MAX_R 9u                            // sources per bucket of the row kernels: 2^r, r <= this
struct swa_part_levels { uint32_t levels; uint32_t bits[4]; uint32_t total; };
swa_part_levels swa_plan_levels(uint32_t total_bits, uint32_t max_bits = SWA_PART_MAX_BITS);
struct swa_part_plan {
  swa_part_levels lv;
  uint32_t tile;                 // records per tile: 2048 (512 bins), 8192 / 4096 (the one level of 1024 bins, whole database / routed)
  bool keys_hist;                // k_keys takes the first level's histogram on the way (not for routed builds)
  bool wide;                     // one level of 1024 bins
  bool lists_inline;             // swa_lists_inline(2^lv.total)
};
// forced_bits != 0 (SWA_D1_PART_BITS, a test hook) stands in for the bit count derived from `records`
swa_part_plan swa_part_plan_for(uint64_t records, uint32_t extra_bits, bool routed, uint32_t forced_bits);
// the work lists behind the partition: up to this many buckets every workgroup of k_group_lists adds up the positions it needs
// itself, beyond it the counts are scanned by two launches first (a pure function of the bucket count; swa_d1_lists_form_for)
#define SWA_LISTS_INLINE_BUCKETS 1024u
bool swa_lists_inline(uint64_t buckets);
void swa_part_plan_report(const swa_part_plan & p, uint32_t out[8]);
struct swa_csr_plan { uint32_t nbits, r; swa_part_levels lv; };
swa_csr_plan swa_csr_plan_for(uint32_t count);

// ---- device helpers -------------------------------------------------------------
#ifdef __HIPCC__

__device__ __forceinline__ unsigned swa_nt(const uint64_t * seq, uint32_t pos) {
  return (unsigned)((seq[pos >> 5] >> ((pos & 31u) << 1)) & 3u);
}

__device__ __forceinline__ uint64_t swa_shfl_u64(uint64_t v, int src) {
  const int lo = __shfl((int)(uint32_t)v, src, 64);
  const int hi = __shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t swa_shfl_xor_u64(uint64_t v, int mask) {
  const int lo = __shfl_xor((int)(uint32_t)v, mask, 64);
  const int hi = __shfl_xor((int)(uint32_t)(v >> 32), mask, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t swa_shfl_up_u64(uint64_t v, unsigned d) {
  const int lo = __shfl_up((int)(uint32_t)v, d, 64);
  const int hi = __shfl_up((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t swa_shfl_down_u64(uint64_t v, unsigned d) {
  const int lo = __shfl_down((int)(uint32_t)v, d, 64);
  const int hi = __shfl_down((int)(uint32_t)(v >> 32), d, 64);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}

// ---- runs of equal keys along a wave -------------------------------------------------------------------------------------
// One position of a sorted order per lane: the keys never fall from lane to lane.  A segmented inclusive scan over the 64
// lanes, six steps, reduces every run of equal keys into its LAST lane; the payload P moves itself up d lanes (P::shfl_up:
// the fields it has, no others) and takes in what arrived (P::absorb).  Returns whether the lane is the last of its run,
// and the run's length.  Every lane takes part: the loop around it runs to swa_wave_span(count), lanes beyond the count
// carry a key no position has and write nothing.  The callers (k_swarm_sums, k_graft_apply, k_dt_maxradius, k_d0_sums)
// store plainly where the run is the whole cluster and add with one atomic per (wave, cluster) otherwise.
struct swa_run { bool last; uint32_t length; };
template <class P> __device__ __forceinline__ swa_run swa_wave_run_reduce(uint32_t key, P & p) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t length = 1;
#pragma unroll
  for (uint32_t d = 1; d < 64u; d <<= 1) {
    const uint32_t key2 = __shfl_up(key, d, 64), length2 = __shfl_up(length, d, 64);
    const P p2 = p.shfl_up(d);
    if (lane >= d && key2 == key) { p.absorb(p2); length += length2; }
  }
  const uint32_t next = __shfl_down(key, 1, 64);
  return swa_run{lane == 63u || next != key, length};
}
// positions of a grid-stride loop in which whole waves take part: the count rounded up to the wave
__device__ __forceinline__ uint64_t swa_wave_span(uint64_t count) { return (count + 63u) & ~uint64_t(63); }

// whether v stands in the strictly ascending row of p (nb[offsets[p] .. offsets[p + 1])), by bisection; at = where, if it does
__device__ __forceinline__ bool swa_row_find(const uint64_t * __restrict__ offsets, const uint32_t * __restrict__ nb, uint32_t p, uint32_t v, uint64_t & at) {
  uint64_t lo = offsets[p], hi = offsets[p + 1];
  const uint64_t end = hi;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (nb[mid] < v) { lo = mid + 1; } else { hi = mid; }
  }
  return (at = lo) < end && nb[lo] == v;
}

// Word `w` of the microvariant of `seed` (len nt, nw = ceil(len/32) valid words,
// zero padded) described by (type, pos, base): what generate_variant_sequence
// (src/variants.cc:78-115) materialises nucleotide by nucleotide, computed here
// with 64-bit shifts.  type: 0 substitution, 1 deletion, 2 insertion.
__device__ __forceinline__ uint64_t swa_variant_word(const uint64_t * seed, uint32_t nw, uint32_t type,
                                                     uint32_t pos, uint32_t base, uint32_t w) {
  const uint32_t wp = pos >> 5;
  const uint32_t sh = (pos & 31u) << 1;
  const uint64_t cur = (w < nw) ? seed[w] : 0ull;
  if (type == 0u) {
    if (w != wp) return cur;
    return (cur & ~(3ull << sh)) | ((uint64_t)base << sh);
  }
  const uint64_t lowmask = (1ull << sh) - 1ull;   // nts below `pos` inside word wp (sh < 64)
  if (type == 1u) {
    const uint64_t nxt = (w + 1 < nw) ? seed[w + 1] : 0ull;
    const uint64_t shifted = (cur >> 2) | (nxt << 62);      // every nt one position down
    if (w < wp) return cur;
    if (w > wp) return shifted;
    return (cur & lowmask) | (shifted & ~lowmask);
  }
  {
    const uint64_t prv = (w >= 1 && w - 1 < nw) ? seed[w - 1] : 0ull;
    const uint64_t shifted = (cur << 2) | (prv >> 62);      // every nt one position up
    if (w < wp) return cur;
    if (w > wp) return shifted;
    return (cur & lowmask) | ((uint64_t)base << sh) | (shifted & ~(lowmask | (3ull << sh)));
  }
}

#endif  // __HIPCC__

// A caller's result buffer about to receive a large download: its pages are faulted in by the library's worker threads first
// (one zero byte a page; the copy overwrites the whole range right after).  The runtime's copy into pageable pages that do not
// exist yet — a freshly allocated / calloc'ed array — faults them in one by one on its own thread: 8-13 GB/s instead of the
// 40-55 of touched pages (tools/experiments/d2h_cost.hip, profiles/r06).  Costs ~10 us per MB when the pages exist already.
#include "host/pool.h"
inline void swa_touch_pages(void * ptr, size_t bytes) {
  if (ptr == nullptr || bytes < (size_t(4) << 20)) { return; }
  char * p = static_cast<char *>(ptr);
  const size_t pages = (bytes + 4095) / 4096;
  const unsigned parts = std::min<unsigned>(swa_pool::get().size(), 16u);
  swa_pool::get().run(parts, [&](unsigned t) {
    for (size_t k = pages * t / parts; k < pages * (t + 1) / parts; ++k) {
      // (a plain write: the whole range is overwritten by the copy that follows.  Reading the byte first — "keep what is
      // there" — makes an untouched page a read fault onto the shared zero page and then a copy-on-write, i.e. an
      // invalidation every MMU notifier of the process hears: measured, 30 ms more for 160 MB under the runtime's notifiers)
      p[k * 4096] = 0;
    }
  });
}

// The download tail of a call: every destination's pages are faulted in BEFORE any copy is queued (swa_touch_pages writes a
// zero byte a page: behind a queued copy it would race with it), then the copies, then one wait; null and empty ones are skipped
struct swa_copy { void * to; const void * from; uint64_t bytes; };
inline int swa_download(swa_ctx * ctx, std::initializer_list<swa_copy> copies, bool wait = true) {
  for (const swa_copy & c : copies) { swa_touch_pages(c.to, c.bytes); }
  for (const swa_copy & c : copies) {
    if (c.to != nullptr && c.bytes != 0) { SWA_HIP(ctx, hipMemcpyAsync(c.to, c.from, c.bytes, hipMemcpyDeviceToHost, ctx->stream)); }
  }
  if (wait) { SWA_HIP(ctx, hipStreamSynchronize(ctx->stream)); }
  return SWA_OK;
}

inline int swa_grid256(const swa_ctx * ctx, uint64_t items) { return swa_grid_for(ctx, items, 256, 8); }   // 256 items a workgroup, 8 a CU at most
inline uint32_t swa_bit_width(uint64_t v) { uint32_t b = 0; while (v != 0u) { ++b; v >>= 1; } return b; }

// ---- buffers that hold several arrays --------------------------------------------------------------------------------------
// A struct of named pointers says in lay(carver, count) how its buffer is cut up: take(count, a, b ...) gives each of its
// arguments `count` elements at its type's alignment (hipMalloc's buffers are 256-byte aligned), one behind the other.
// swa_carve runs lay() from a null base for the size to reserve and from the buffer for the pointers — no second formula —
// and fails with SWA_E_INTERNAL if the walk ends beyond the buffer.  extent(first): the bytes from an array taken earlier
// up to here, what ONE fill may cover when it clears several arrays.
struct swa_extent { void * ptr; uint64_t bytes; };
struct swa_carver {
  uintptr_t base;
  uint64_t used = 0;
  template <class T, class... R> void take(uint64_t count, T *& first, R *&... rest) {
    used = (used + alignof(T) - 1) & ~uint64_t(alignof(T) - 1);
    first = reinterpret_cast<T *>(base + used);
    used += count * sizeof(T);
    if constexpr (sizeof...(rest) != 0) { take(count, rest...); }
  }
  void spare(uint64_t bytes) { used += bytes; }             // room nobody names (kept: no buffer is smaller than it used to be)
  swa_extent extent(void * first) const { return swa_extent{first, base + used - reinterpret_cast<uintptr_t>(first)}; }
};
template <class L> int swa_carve(swa_ctx * ctx, swa_dbuf & buf, uint64_t count, bool grow, L & out) {
  swa_carver size{0}, c{0};
  out.lay(size, count);
  if (grow) { SWA_TRY(swa_reserve(ctx, buf, size.used)); }
  c.base = reinterpret_cast<uintptr_t>(buf.ptr);
  out.lay(c, count);
  if (buf.ptr == nullptr || c.used > buf.bytes) { return swa_fail_msg(ctx, SWA_E_INTERNAL, "a buffer's layout ends beyond the buffer"); }
  return SWA_OK;
}

// d_cluster (swa_d1_cluster_device), n amplicons: among its work arrays what the clustering leaves for swa_d1_cluster_fetch,
// fast_graft.inc, dn_tables.inc and swa_dn_parent_diffs: swarmid, gen, parent, order (swarm s = order[begins[s], begins[s + 1]))
struct swa_cluster_arrays {
  uint32_t * label, * gen, * parent, * swarmid, * ids_in, * order, * seed_rank, * begins, * stamp;
  unsigned long long * keys_in, * keys_out;                 // sort keys, read as 32-bit ones where they are narrow
  uint8_t * is_seed;
  void lay(swa_carver & c, uint64_t n) {
    c.take(n, label, gen, parent, swarmid, ids_in, order, seed_rank);
    c.take(n + 4, begins);                                  // (n + 1 are used: begins[swarms] = n)
    c.take(n, stamp, keys_in, keys_out, is_seed);
    c.spare(4 * n + 128);                                   // (a tenth array of n words that nobody uses has always been part of it)
  }
};

#include <chrono>
inline void swa_lap(swa_ctx * ctx, const char * what) {
  static const bool on = std::getenv("SWARM_AMD_STEP_TIMING") != nullptr;
  if (!on) { return; }
  static auto last = std::chrono::steady_clock::now();
  (void)hipStreamSynchronize(ctx->stream);
  const auto now = std::chrono::steady_clock::now();
  std::fprintf(stderr, "[step] %-34s %8.3f ms\n", what, 1e3 * std::chrono::duration<double>(now - last).count());
  last = std::chrono::steady_clock::now();
}
