"""ctypes binding of libswarm_amd.so (include/swarm_amd.h) — the thin Python face of the
C ABI used by the tests, bench.py and __graft_entry__.py.

There is deliberately NO fallback here: if the HIP library is missing or no gfx950
device is usable, everything raises.  Nothing in this package imports oracle/.
"""
from __future__ import annotations

import ctypes as C
import os

# libgomp's default (workers spin between parallel regions) costs the host phases up to 30x on a many-core GPU host
# (see host/main.cpp); it reads the variable when it is first loaded, which importing this module usually precedes.
os.environ.setdefault("OMP_WAIT_POLICY", "passive")


def usable_cpus() -> int:
    """CPUs this process may really use: affinity, cut down to the cgroup's CPU quota (what swa_host_cpus, host/pool.h,
    computes for the library's own worker threads) — a container that sees 256 CPUs and may use 16 is throttled as soon
    as more than 16 threads are busy."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, round(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and p > 0:
                n = min(n, max(1, round(q / p)))
        except (OSError, ValueError):
            pass
    return max(1, n)


# (The library sizes its own OpenMP teams — num_threads(swa_host_team()) on every parallel region, host/out.h — so this
# module does not touch OMP_NUM_THREADS: other OpenMP users of the importing process keep their own setting.)
import subprocess
from pathlib import Path

import numpy as np

PKG = Path(__file__).resolve().parent
# SWARM_AMD_LIB=<path>: another build of the library (triage: tools/gpu_selfcheck.py; `make asan`)
LIB_PATH = Path(os.environ.get("SWARM_AMD_LIB") or PKG / "lib" / "libswarm_amd.so")

SWA_OK, SWA_E_DEVICE, SWA_E_ARG, SWA_E_NOMEM, SWA_E_CAPACITY, SWA_E_DUPLICATES, SWA_E_INTERNAL = range(7)
NO_AMPLICON = 0xFFFFFFFF

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)


class SwaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libswarm_amd error {code}: {msg}")
        self.code = code


class DbView(C.Structure):
    _fields_ = [("n", C.c_uint32), ("longest", C.c_uint32), ("seqs", C.c_void_p), ("seq_off", C.c_void_p),
                ("seqlen", C.c_void_p), ("abundance", C.c_void_p)]


# struct swa_aux (csrc/d1_common.inc): what k_seqhash writes per amplicon, selector 3 of swa_d1_debug_read
AUX_DTYPE = np.dtype([("h", "<u8"), ("dall", "<u8"), ("iall", "<u8"), ("a32", "<u8"), ("d32", "<u8"), ("i32", "<u8"),
                      ("pb", "<u4"), ("pad", "<u4", (3,))])
assert AUX_DTYPE.itemsize == 64


class DbUnorderedView(C.Structure):
    """swa_db_unordered_view: the reader's word pools in file order + where every amplicon's words begin"""
    _fields_ = [("n", C.c_uint32), ("longest", C.c_uint32), ("pieces", C.c_uint32), ("piece_words", C.c_void_p),
                ("piece_word_count", C.c_void_p), ("src_off", C.c_void_p), ("seqlen", C.c_void_p), ("abundance", C.c_void_p)]


EXPORTS = [
    "swa_abi_version", "swa_ctx_create", "swa_ctx_destroy", "swa_last_error", "swa_ctx_synchronize", "swa_ctx_warmup", "swa_ctx_warmup_for", "swa_d1_anchor_windows", "swa_d1_anchor_width",
    "swa_d1_network_resident", "swa_d1_network_fetch", "swa_d1_cluster_device", "swa_d1_cluster_fetch", "swa_d1_cluster_maxgen", "swa_d1_network_adopt", "swa_d1_cluster_effort", "swa_d1_cluster_resident", "swa_d1_cluster_resident_lazy", "swa_d1_result_detach", "swa_d1_result_error", "swa_d1_result_prepare",
    "swa_d1_cluster_resident_prepared", "swa_host_pin", "swa_host_unpin", "swa_ctx_warmup_downloads",
    "swa_db_upload", "swa_db_attach", "swa_db_stage_words", "swa_db_upload_unordered", "swa_hostdb_unordered_view", "swa_hostdb_read_fasta_staged", "swa_cli_main", "swa_d1_index_build", "swa_d1_index_build_range", "swa_d1_set_ownership", "swa_d1_route_slice", "swa_d1_index_build_routed", "swa_d1_route_slice_records", "swa_d1_index_build_records", "swa_d1_network", "swa_d1_network_edges_device", "swa_d1_network_device", "swa_d1_guard_retries",
    "swa_d1_links_split", "swa_d1_csr_from_lists",
    "swa_d1_debug_read", "swa_d1_table_size", "swa_search_uses_wavefront", "swa_d1_fastidious", "swa_d1_fastidious_shard", "swa_d1_fastidious_plan", "swa_d1_fastidious_totals", "swa_d1_fastidious_bloom_batches", "swa_d1_fastidious_bloom_read", "swa_d1_fastidious_split", "swa_d1_fastidious_plan_for", "swa_d1_fastidious_plan_modes", "swa_d1_fastidious_sites_cap", "swa_d1_part_plan_for", "swa_d1_part_plan", "swa_d1_csr_plan_for", "swa_d1_lists_form_for", "swa_d1_lists_form", "swa_qgram_build", "swa_qgram_diff",
    "swa_qgram_debug_read", "swa_search_begin", "swa_search_do", "swa_search_form", "swa_align_wide_for", "swa_timing_enable", "swa_timing_read",
    "swa_hostdb_read_fasta", "swa_hostdb_free", "swa_hostdb_error", "swa_hostdb_view", "swa_hostdb_nucleotides",
    "swa_hostdb_header", "swa_d1_cluster", "swa_d1_result_free", "swa_d1_result_summary", "swa_d1_result_swarmid",
    "swa_d1_result_parent", "swa_d1_result_generation", "swa_d1_light_flags", "swa_d1_graft", "swa_d1_write_swarms",
    "swa_d1_write_stats", "swa_d1_write_structure", "swa_d1_write_seeds", "swa_d1_write_network",
    "swa_d1_swarm_sums_device", "swa_d1_light_flags_device", "swa_d1_fastidious_resident", "swa_d1_graft_device",
    "swa_d1_graft_candidates_fetch", "swa_d1_result_install_graft", "swa_d1_result_detail_fetches",
    "swa_d1_graft_layout_device", "swa_d1_graft_layout_info", "swa_d1_result_adopt_layout", "swa_d1_result_graft_route",
    "swa_d1_network_fetch_diffs", "swa_d1_shard_owners_device", "swa_d1_shard_owner_for", "swa_d1_shard_owner_plan",
    "swa_multi_d1_network_resident", "swa_multi_d1_fastidious_resident", "swa_multi_dn_graph_resident",
    "swa_multi_d1_last_build", "swa_merge_sorted_lists",
]


def build_library(force: bool = False) -> Path:
    """Compile every HIP translation unit for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", str(PKG / "csrc"), "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", str(PKG / "csrc"), "-j4"], check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def load_library() -> C.CDLL:
    """dlopen libswarm_amd.so and declare the prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise FileNotFoundError(f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
    lib = C.CDLL(str(LIB_PATH))
    lib.swa_abi_version.restype = C.c_int
    lib.swa_ctx_create.argtypes = [C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.swa_ctx_destroy.argtypes = [C.c_void_p]
    lib.swa_ctx_destroy.restype = None
    lib.swa_last_error.argtypes = [C.c_void_p]
    lib.swa_last_error.restype = C.c_char_p
    lib.swa_ctx_synchronize.argtypes = [C.c_void_p]
    lib.swa_db_upload.argtypes = [C.c_void_p, C.POINTER(DbView)]
    lib.swa_db_attach.argtypes = [C.c_void_p, C.POINTER(DbView)]
    lib.swa_d1_index_build.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    lib.swa_d1_network.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.c_uint64, u64p]
    lib.swa_d1_network_device.argtypes = lib.swa_d1_network.argtypes
    lib.swa_d1_network_edges_device.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                                C.POINTER(C.c_uint64)]
    lib.swa_d1_links_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, u32p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.swa_d1_csr_from_lists.argtypes = [C.c_void_p, C.c_void_p, u64p, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_uint64, u64p]
    lib.swa_d1_set_ownership.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.swa_d1_route_slice.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.swa_d1_index_build_routed.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]
    lib.swa_d1_route_slice_records.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]
    lib.swa_d1_index_build_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_int)]
    lib.swa_d1_debug_read.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    lib.swa_d1_table_size.argtypes = [C.c_void_p]
    lib.swa_d1_table_size.restype = C.c_uint64
    lib.swa_d1_fastidious.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.swa_d1_fastidious_shard.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p]
    lib.swa_d1_swarm_sums_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.swa_d1_light_flags_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, u64p]
    lib.swa_d1_fastidious_resident.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.swa_d1_graft_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, u32p]
    lib.swa_d1_graft_candidates_fetch.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_result_install_graft.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.swa_d1_graft_layout_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.swa_d1_graft_layout_info.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_result_adopt_layout.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_result_graft_route.argtypes = [C.c_void_p]
    lib.swa_d1_result_graft_route.restype = C.c_uint32
    lib.swa_d1_shard_owners_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, u64p]
    lib.swa_d1_shard_owner_for.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, u32p]
    lib.swa_merge_sorted_lists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.swa_d1_shard_owner_plan.argtypes = [C.c_void_p]
    lib.swa_d1_result_detail_fetches.argtypes = [C.c_void_p]
    lib.swa_d1_result_detail_fetches.restype = C.c_uint32
    lib.swa_d1_fastidious_plan.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_fastidious_totals.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_fastidious_bloom_batches.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_fastidious_bloom_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    lib.swa_d1_fastidious_split.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_fastidious_plan_for.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.swa_d1_fastidious_plan_modes.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    lib.swa_d1_fastidious_sites_cap.argtypes = [C.c_uint32]
    lib.swa_d1_fastidious_sites_cap.restype = C.c_uint32
    lib.swa_d1_part_plan_for.argtypes = [C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p]
    lib.swa_d1_part_plan.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_csr_plan_for.argtypes = [C.c_uint32, C.c_void_p]
    lib.swa_d1_lists_form_for.argtypes = [C.c_uint64]
    lib.swa_d1_lists_form.argtypes = [C.c_void_p]
    lib.swa_qgram_build.argtypes = [C.c_void_p]
    lib.swa_qgram_diff.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    lib.swa_qgram_debug_read.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.swa_search_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
    lib.swa_align_wide_for.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.swa_search_do.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]
    lib.swa_timing_enable.argtypes = [C.c_void_p, C.c_int]
    lib.swa_timing_read.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.swa_hostdb_read_fasta.argtypes = [C.c_char_p, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]
    lib.swa_hostdb_free.argtypes = [C.c_void_p]
    lib.swa_hostdb_free.restype = None
    lib.swa_hostdb_error.argtypes = [C.c_void_p]
    lib.swa_hostdb_error.restype = C.c_char_p
    lib.swa_hostdb_view.argtypes = [C.c_void_p, C.POINTER(DbView)]
    lib.swa_hostdb_view.restype = None
    lib.swa_hostdb_nucleotides.argtypes = [C.c_void_p]
    lib.swa_hostdb_nucleotides.restype = C.c_uint64
    lib.swa_hostdb_header.argtypes = [C.c_void_p, C.c_uint32, u32p]
    lib.swa_hostdb_header.restype = C.c_char_p
    lib.swa_d1_cluster.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.swa_d1_result_free.argtypes = [C.c_void_p]
    lib.swa_d1_result_free.restype = None
    lib.swa_d1_result_summary.argtypes = [C.c_void_p, u64p]
    lib.swa_d1_result_summary.restype = None
    for fn in (lib.swa_d1_result_swarmid, lib.swa_d1_result_parent, lib.swa_d1_result_generation):
        fn.argtypes = [C.c_void_p]
        fn.restype = C.c_void_p
    lib.swa_d1_light_flags.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, u64p]
    lib.swa_d1_light_flags.restype = C.c_int
    lib.swa_d1_result_detach.argtypes = [C.c_void_p]
    lib.swa_d1_result_detach.restype = C.c_int
    lib.swa_d1_result_error.argtypes = [C.c_void_p]
    lib.swa_d1_result_error.restype = C.c_char_p
    lib.swa_d1_graft.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d1_graft.restype = C.c_uint32
    lib.swa_d1_write_swarms.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int64, C.c_int64]
    lib.swa_d1_write_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.swa_d1_write_structure.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.swa_d1_write_seeds.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.swa_d1_write_network.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int64]
    _lib = lib
    return lib


def fastidious_plan_for(longest: int, pair_longest: int = 0, split: bool = False, bloom: bool = False,
                        words: bool = False) -> list:
    """swa_d1_fastidious_plan_for: the dispatch of the --fastidious pass as a pure function (no context, no device), laid
    out as Context.d1_fastidious_plan.  split: SWA_FAST_LONG=split, with pair_longest the longest sequence <= the cap;
    bloom: SWA_FAST_BLOOM=1; words: SWA_FAST_PAIRS=words."""
    out = np.zeros(8, dtype=np.uint32)
    rc = load_library().swa_d1_fastidious_plan_for(int(longest), int(pair_longest), int(split), int(bloom), int(words), _ptr(out))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_d1_fastidious_plan_for: bad argument")
    return [int(v) for v in out]


def shard_owner_for(heavy: int, nshards: int, h: int) -> int:
    """swa_d1_shard_owner_for: the shard (of nshards) that expands the h-th of `heavy` heavy amplicons — the one whose
    slice [heavy * s // nshards, heavy * (s + 1) // nshards) holds h — in closed form; no context, no device."""
    owner = C.c_uint32(0)
    rc = load_library().swa_d1_shard_owner_for(int(heavy), int(nshards), int(h), C.byref(owner))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_d1_shard_owner_for: bad argument")
    return int(owner.value)


def shard_owner_plan() -> list:
    """swa_d1_shard_owner_plan: [amplicons per tile of the owner kernels, tiles per turn of the scan of the tiles' counts
    (0: the scan has no turns)]."""
    out = np.zeros(2, dtype=np.uint32)
    rc = load_library().swa_d1_shard_owner_plan(_ptr(out))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_d1_shard_owner_plan failed")
    return [int(v) for v in out]


def fastidious_plan_modes(longest: int, pair_longest: int = 0, long_mode: int = 0, bloom: bool = False, words: bool = False,
                          count_sites: bool = False, sites_cap: int = 0) -> list:
    """swa_d1_fastidious_plan_modes: fastidious_plan_for with every switch.  long_mode: 0, 1 = SWA_FAST_LONG=split, 2 =
    SWA_FAST_LONG=pairs (pair_longest: the longest sequence <= the cap in effect, read where longer ones exist);
    count_sites: SWA_FAST_COUNT=sites; sites_cap: SWA_FAST_SITES_CAP (0: the derived cap)."""
    out = np.zeros(8, dtype=np.uint32)
    rc = load_library().swa_d1_fastidious_plan_modes(int(longest), int(pair_longest), int(long_mode), int(bloom), int(words),
                                                     int(count_sites), int(sites_cap), _ptr(out))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_d1_fastidious_plan_modes: bad argument")
    return [int(v) for v in out]


def fastidious_sites_cap(sites_cap: int = 0) -> int:
    """swa_d1_fastidious_sites_cap: the longest sequence SWA_FAST_LONG=pairs keeps on the pair route — derived from the
    LDS of k_fast_count_sites_words, or `sites_cap` (SWA_FAST_SITES_CAP) where that lies in [1004, the derived cap]."""
    return int(load_library().swa_d1_fastidious_sites_cap(int(sites_cap)))


def part_plan_for(records: int, extra_bits: int = 0, routed: bool = False, forced_bits: int = 0) -> list:
    """swa_d1_part_plan_for: the form of the key partition of the d = 1 index build as a pure function (no context, no
    device): [total bits, levels, bits of level 0, 1, 2, records per tile, histogram taken by k_keys, one level of 1024
    bins].  forced_bits: what SWA_D1_PART_BITS would set (0: unset)."""
    out = np.zeros(8, dtype=np.uint32)
    rc = load_library().swa_d1_part_plan_for(int(records), int(extra_bits), int(routed), int(forced_bits), _ptr(out))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_d1_part_plan_for: bad argument")
    return [int(v) for v in out]


def lists_form_for(buckets: int) -> int:
    """swa_d1_lists_form_for: how the work lists behind a key partition of `buckets` buckets get their positions: 1 inside
    k_group_lists, 0 by the two-launch scan of the counts."""
    form = load_library().swa_d1_lists_form_for(int(buckets))
    if form < 0:
        raise SwaError(2, "swa_d1_lists_form_for: bad argument")
    return form


def align_wide_for(mismatch: int, gapopen: int, gapextend: int, d: int) -> tuple:
    """swa_align_wide_for: (W, saturation, K) of a reduced scoring and d — the band half-width, 255 or 65535, and the
    offsets a lane of the wide alignment form (2, 4, 8; 0 when the band fits 64 lanes or exceeds W = 254)."""
    out = np.zeros(3, dtype=np.uint64)
    rc = load_library().swa_align_wide_for(int(mismatch), int(gapopen), int(gapextend), int(d), _ptr(out))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_align_wide_for: bad argument")
    return int(out[0]), int(out[1]), int(out[2])


def csr_plan_for(count: int) -> list:
    """swa_d1_csr_plan_for: link partition and row kernels of a CSR over `count` sources: [bits of a source index, r (2^r
    sources per bucket of the row kernels), levels, bits of level 0, 1, 2]."""
    out = np.zeros(6, dtype=np.uint32)
    rc = load_library().swa_d1_csr_plan_for(int(count), _ptr(out))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_d1_csr_plan_for: bad argument")
    return [int(v) for v in out]


def _p64(a: np.ndarray):
    return a.ctypes.data_as(u64p)


def _ptr(a) -> int:
    """Address of a numpy array (host) or of anything with data_ptr() (a torch tensor: device)."""
    if a is None:
        return 0
    if hasattr(a, "data_ptr"):
        return int(a.data_ptr())
    return int(a.ctypes.data)


def _dev(a) -> int:
    """A device address: a raw pointer (int) as it is, else _ptr()."""
    return int(a) if isinstance(a, int) else _ptr(a)


class HostDb:
    """Packed amplicon database on the host, read from FASTA by the library's own reader
    (mirror of the reference's db_read, src/db.cc:432-803).  Arrays are numpy views into the
    handle's memory (db order)."""

    def __init__(self, path, usearch_abundance: bool = False, append_abundance: int = 0,
                 check_duplicate_sequences: bool = False):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.swa_hostdb_read_fasta(str(path).encode(), int(usearch_abundance), int(append_abundance),
                                            int(check_duplicate_sequences), C.byref(h))
        self.h = h
        if rc != SWA_OK:
            msg = self.lib.swa_hostdb_error(h).decode() if h else "allocation failed"
            self.close()
            raise SwaError(rc, msg)
        u = DbUnorderedView()
        self.lib.swa_hostdb_unordered_view(h, C.byref(u))
        self.n = int(u.n)
        self.longest = int(u.longest)
        self.nucleotides = int(self.lib.swa_hostdb_nucleotides(h))
        self._ordered = None

    @staticmethod
    def _array(ptr, count, dtype):
        if count == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=count)

    def _view(self):
        """The packed sequences contiguous in db order (swa_hostdb_view): gathered by the library on first use."""
        if self._ordered is None:
            v = DbView()
            self.lib.swa_hostdb_view(self.h, C.byref(v))
            seq_off = self._array(v.seq_off, self.n + 1, np.uint64)
            self._ordered = {"seq_off": seq_off, "seqlen": self._array(v.seqlen, self.n, np.uint32),
                             "abundance": self._array(v.abundance, self.n, np.uint64),
                             "seqs": self._array(v.seqs, int(seq_off[self.n]) if self.n else 0, np.uint64)}
        return self._ordered

    seq_off = property(lambda self: self._view()["seq_off"])
    seqlen = property(lambda self: self._view()["seqlen"])
    abundance = property(lambda self: self._view()["abundance"])
    seqs = property(lambda self: self._view()["seqs"])

    def header(self, i: int) -> bytes:
        return self.lib.swa_hostdb_header(self.h, i, None)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.swa_hostdb_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class D1Clusters:
    """Host-side greedy clustering of the d=1 network (mirror of algo_d1_run's host loop,
    src/algod1.cc:1185-1280) with the fastidious bookkeeping and the writers."""

    def __init__(self, hdb: HostDb, offsets: np.ndarray, neighbours: np.ndarray):
        self.lib = load_library()
        self.hdb = hdb
        self._keep = (np.ascontiguousarray(offsets, dtype=np.uint64), np.ascontiguousarray(neighbours, dtype=np.uint32))
        h = C.c_void_p()
        rc = self.lib.swa_d1_cluster(hdb.h, _ptr(self._keep[0]), _ptr(self._keep[1]) if len(self._keep[1]) else 0,
                                     C.byref(h))
        if rc != SWA_OK:
            raise SwaError(rc, "swa_d1_cluster failed")
        self.h = h

    @classmethod
    def from_resident(cls, ctx: "Context", hdb: HostDb, lazy: bool = False, pinned: bool = False) -> "D1Clusters":
        """The same result from the network ctx.d1_network_resident() left in HBM: agglomeration on the GPU
        (swa_d1_cluster_device), per-swarm sums on the host.  lazy = the command line's form (swa_d1_cluster_resident_lazy):
        swarm / generation / parent stay in HBM until asked for; the result then keeps the context alive."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.hdb = hdb
        self._keep = None
        self._ctx = ctx if (lazy or pinned) else None
        if pinned:
            # the command line's two steps: result arrays sized and pinned ahead (swa_d1_result_prepare), then clustered into
            self.lib.swa_d1_result_prepare.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
            self.lib.swa_d1_cluster_resident_prepared.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            h = C.c_void_p()
            rc = self.lib.swa_d1_result_prepare(ctx.h, hdb.h, C.byref(h))
            self.h = h
            if rc == SWA_OK:
                rc = self.lib.swa_d1_cluster_resident_prepared(ctx.h, hdb.h, h)
            if rc != SWA_OK:
                raise SwaError(rc, "swa_d1_cluster_resident_prepared failed: " + ctx.lib.swa_last_error(ctx.h).decode())
            return self
        fn = self.lib.swa_d1_cluster_resident_lazy if lazy else self.lib.swa_d1_cluster_resident
        fn.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        rc = fn(ctx.h, hdb.h, C.byref(h))
        self.h = h
        if rc != SWA_OK:
            raise SwaError(rc, "swa_d1_cluster_resident failed: " + (self.lib.swa_d1_result_error(h) or ctx.lib.swa_last_error(ctx.h)).decode())
        return self

    def detach(self) -> None:
        """Fetch whatever a lazy result still has on the device; afterwards it does not need its context."""
        rc = self.lib.swa_d1_result_detach(self.h)
        if rc != SWA_OK:
            raise SwaError(rc, "swa_d1_result_detach failed: " + self.lib.swa_d1_result_error(self.h).decode())
        self._ctx = None

    def summary(self) -> dict:
        out = np.zeros(4, dtype=np.uint64)
        self.lib.swa_d1_result_summary(self.h, _p64(out))
        return {"swarms": int(out[0]), "largest": int(out[1]), "maxgen": int(out[2]), "swarms_before_grafting": int(out[3])}

    def _arr(self, fn) -> np.ndarray:
        ptr = fn(self.h)
        n = self.hdb.n
        if not ptr:
            if n == 0:
                return np.zeros(0, dtype=np.uint32)
            raise SwaError(SWA_E_DEVICE, "the clustering's details could not be fetched: " + self.lib.swa_d1_result_error(self.h).decode())
        buf = (C.c_char * (4 * n)).from_address(ptr)
        return np.frombuffer(buf, dtype=np.uint32, count=n).copy()

    def swarmid(self) -> np.ndarray:
        return self._arr(self.lib.swa_d1_result_swarmid)

    def parent(self) -> np.ndarray:
        return self._arr(self.lib.swa_d1_result_parent)

    def generation(self) -> np.ndarray:
        return self._arr(self.lib.swa_d1_result_generation)

    def light_flags(self, boundary: int = 3):
        flags = np.zeros(self.hdb.n, dtype=np.uint8)
        stats = np.zeros(5, dtype=np.uint64)
        rc = self.lib.swa_d1_light_flags(self.h, boundary, _ptr(flags), _p64(stats))
        if rc != SWA_OK:
            raise SwaError(rc, "swa_d1_light_flags failed: " + self.lib.swa_d1_result_error(self.h).decode())
        return flags, [int(x) for x in stats]

    def graft(self, graft_cand: np.ndarray) -> int:
        """swa_d1_graft: the grafts decided from the candidates and laid out in the member order; 0 (result untouched, a text
        in swa_d1_result_error) for ill-formed candidates."""
        g = np.ascontiguousarray(graft_cand, dtype=np.uint32)
        return int(self.lib.swa_d1_graft(self.h, _ptr(g)))

    def install_graft(self, heavy_swarm, light_swarm, parent, child) -> None:
        """swa_d1_result_install_graft: the grafts of Context.d1_graft_device (chain order) laid out as graft() would
        leave them; a lazy result downloads nothing for it."""
        four = [np.ascontiguousarray(a, dtype=np.uint32) for a in (heavy_swarm, light_swarm, parent, child)]
        assert len({len(a) for a in four}) == 1
        rc = self.lib.swa_d1_result_install_graft(self.h, *(_ptr(a) if len(a) else None for a in four), len(four[0]))
        if rc != SWA_OK:
            raise SwaError(rc, "swa_d1_result_install_graft failed: " + self.lib.swa_d1_result_error(self.h).decode())

    def adopt_layout(self, ctx: "Context") -> None:
        """swa_d1_result_adopt_layout: the layout Context.d1_graft_layout_device left in HBM becomes the result's member order
        and bounds — no per-graft array, nothing moved on the host; the writers print what they print after graft() / install_graft().  A
        lazy result keeps needing its context."""
        rc = self.lib.swa_d1_result_adopt_layout(self.h, ctx.h)
        if rc != SWA_OK:
            raise SwaError(rc, "swa_d1_result_adopt_layout failed: " + self.lib.swa_d1_result_error(self.h).decode())

    def graft_route(self) -> int:
        """swa_d1_result_graft_route: 0 no grafts, 1 graft(), 2 install_graft(), 3 adopt_layout()"""
        return int(self.lib.swa_d1_result_graft_route(self.h))

    def detail_fetches(self) -> int:
        """swa_d1_result_detail_fetches: downloads of swarm id / generation / parent made for this result"""
        return int(self.lib.swa_d1_result_detail_fetches(self.h))

    def write_swarms(self, path, mothur=False, usearch=False, append_abundance=0, differences=1) -> None:
        assert self.lib.swa_d1_write_swarms(self.h, self.hdb.h, str(path).encode(), int(mothur), int(usearch),
                                            append_abundance, differences) == SWA_OK

    def write_stats(self, path, usearch=False) -> None:
        assert self.lib.swa_d1_write_stats(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_structure(self, path, usearch=False) -> None:
        assert self.lib.swa_d1_write_structure(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_seeds(self, path, usearch=False) -> None:
        assert self.lib.swa_d1_write_seeds(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_network(self, path, usearch=False, append_abundance=0) -> None:
        assert self.lib.swa_d1_write_network(self.hdb.h, _ptr(self._keep[0]), _ptr(self._keep[1]),
                                             str(path).encode(), int(usearch), append_abundance) == SWA_OK

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.swa_d1_result_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One GPU + one HIP stream.  Mirrors the reference's implicit global state for the path
    (seqindex, hash table, Bloom filters) as an explicit handle."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.swa_ctx_create(device, C.c_void_p(stream or 0), C.byref(h))
        if rc != SWA_OK:
            raise SwaError(rc, "swa_ctx_create failed: no usable gfx950 device (there is no CPU fallback)")
        self.h = h
        self.n = 0
        self._keep = None
        self._owned = True

    @classmethod
    def _view(cls, handle, n: int, keep) -> "Context":
        """A Context over a handle somebody else owns (MultiContext.ctx): close() lets go of it without destroying it."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.h = C.c_void_p(handle)
        self.n = n
        self._keep = keep
        self._owned = False
        return self

    def close(self) -> None:
        if self.h:
            if getattr(self, "_owned", True):
                self.lib.swa_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, allow=()) -> int:
        if rc != SWA_OK and rc not in allow:
            raise SwaError(rc, self.lib.swa_last_error(self.h).decode())
        return rc

    def warmup(self, differences: int | None = None) -> None:
        """First-use costs of the device (code objects of the kernel files, copy queues) now, not inside the first call that
        needs them: what the command line does on a helper thread beside the FASTA read (swa_ctx_warmup; with `differences`
        only the kernel files a run at that d launches: swa_ctx_warmup_for)."""
        self.lib.swa_ctx_warmup_for.argtypes = [C.c_void_p, C.c_int]
        self._check(self.lib.swa_ctx_warmup_for(self.h, -1 if differences is None else int(differences)))

    def synchronize(self) -> None:
        self._check(self.lib.swa_ctx_synchronize(self.h))

    def timing_enable(self, on: bool = True) -> None:
        self._check(self.lib.swa_timing_enable(self.h, int(on)))

    def timing_read_stream(self) -> list:
        """ms of the kernel groups of the streaming d=1 step: keys, partition, groups + lists, pair pass 0, pair pass 1,
        link partition, CSR rows, amplicon lines"""
        ms = (C.c_float * 8)()
        self.lib.swa_timing_read_stream.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        self._check(self.lib.swa_timing_read_stream(self.h, ms))
        return [float(x) for x in ms]

    def timing_read(self) -> list:
        ms = (C.c_float * 8)()
        self._check(self.lib.swa_timing_read(self.h, ms))
        return [float(x) for x in ms]

    def upload_hostdb(self, hdb: "HostDb") -> None:
        """The database as the reader keeps it — words in file order — put in db order on the GPU (swa_db_upload_unordered:
        what the command line does)."""
        u = DbUnorderedView()
        self.lib.swa_hostdb_unordered_view(hdb.h, C.byref(u))
        self._check(self.lib.swa_db_upload_unordered(self.h, C.byref(u)))
        self.n = hdb.n

    # ---- L2
    def upload_db(self, seqs, seq_off, seqlen, abundance, longest: int) -> None:
        """Host numpy arrays (db order) -> HBM."""
        n = int(seqlen.shape[0])
        v = DbView(n, int(longest), _ptr(seqs), _ptr(seq_off), _ptr(seqlen), _ptr(abundance))
        self._check(self.lib.swa_db_upload(self.h, C.byref(v)))
        self.n = n

    def attach_db(self, seqs, seq_off, seqlen, abundance, longest: int) -> None:
        """Arrays already in HBM (torch tensors on this GPU); not copied."""
        n = int(seqlen.shape[0])
        v = DbView(n, int(longest), _ptr(seqs), _ptr(seq_off), _ptr(seqlen), _ptr(abundance))
        self._check(self.lib.swa_db_attach(self.h, C.byref(v)))
        self._keep = (seqs, seq_off, seqlen, abundance)
        self.n = n

    # ---- d = 0 on the device
    def derep_resident(self) -> None:
        """swa_derep_resident: the identical-sequence search with its array left in HBM (for d0_cluster_device)."""
        _declare_d0(self.lib)
        self._check(self.lib.swa_derep_resident(self.h))

    def d0_cluster_device(self) -> dict:
        """swa_d0_cluster_device + swa_d0_cluster_fetch: the clusters of the resident dereplication, made on the GPU.  The six
        arrays in output order (mass descending, then seed ascending) — seed, mass (u64), size, singletons, begin, and
        members[n] — plus the summary's three numbers."""
        _declare_d0(self.lib)
        s = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.swa_d0_cluster_device(self.h, _p64(s)))
        out = self.d0_cluster_fetch(int(s[0]))
        out.update(swarms=int(s[0]), largest=int(s[1]), heaviest=int(s[2]))
        return out

    def d0_cluster_fetch(self, cluster_cap: int | None = None) -> dict:
        """swa_d0_cluster_fetch alone: the arrays of the tables in place (cluster_cap None: asked for first)."""
        _declare_d0(self.lib)
        nc = C.c_uint32(0)
        if cluster_cap is None:
            self._check(self.lib.swa_d0_cluster_fetch(self.h, None, None, None, None, None, 0, None, C.byref(nc)))
            cluster_cap = int(nc.value)
        u32 = {k: np.zeros(cluster_cap, dtype=np.uint32) for k in ("seed", "size", "singletons", "begin")}
        mass = np.zeros(cluster_cap, dtype=np.uint64)
        members = np.zeros(self.n, dtype=np.uint32)
        self._check(self.lib.swa_d0_cluster_fetch(self.h, _ptr(u32["seed"]), _ptr(mass), _ptr(u32["size"]), _ptr(u32["singletons"]),
                                                  _ptr(u32["begin"]), cluster_cap, _ptr(members), C.byref(nc)))
        c = int(nc.value)
        return {"seed": u32["seed"][:c], "mass": mass[:c], "size": u32["size"][:c], "singletons": u32["singletons"][:c],
                "begin": u32["begin"][:c], "members": members}

    # ---- B1
    def d1_index_build(self, first: int = 0, count: int | None = None) -> bool:
        """Returns True when duplicate sequences were found (the reference aborts in that case).
        With a range only the amplicons of [first, first+count) are checked for a twin (multi-GPU:
        every rank its slice, flags combined with a MAX all-reduce)."""
        dup = C.c_int(0)
        if count is None:
            count = self.n - first
        self.lib.swa_d1_index_build_range.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int)]
        self._check(self.lib.swa_d1_index_build_range(self.h, first, count, C.byref(dup)), allow=(SWA_E_DUPLICATES,))
        return bool(dup.value)

    def d1_set_ownership(self, rank: int = 0, world: int = 1) -> None:
        """Multi-GPU by ownership: from the next network call on this context finds only its share of
        the links (the anchor groups whose key maps to `rank`, its share of the plain-kernel seeds),
        so a network call returns PARTIAL rows; sharding.exchange_owned_links merges the ranks' links.
        world = 1 restores the complete network."""
        self._check(self.lib.swa_d1_set_ownership(self.h, rank, world))

    def d1_route_slice(self, first: int, count: int, world: int, d_ids, cap: int, d_counts) -> None:
        """Routed multi-GPU index build, step 1 (swa_d1_route_slice): the ids of [first, first+count) grouped by the
        rank that owns their prefix-side / suffix-side key.  d_ids: device int32/uint32 tensor [2 * world * cap],
        d_counts: device tensor [2 * world + 1] (anything with data_ptr()); complete on return."""
        self._check(self.lib.swa_d1_route_slice(self.h, first, count, world, C.c_void_p(d_ids.data_ptr()), cap,
                                                C.c_void_p(d_counts.data_ptr())))

    def d1_index_build_routed(self, d_ids_prefix, n_prefix: int, d_ids_suffix, n_suffix: int) -> bool:
        """Step 3 (swa_d1_index_build_routed): this rank's indexes from the member ids it received; ownership must be
        set.  Returns True when duplicate sequences were found."""
        dup = C.c_int(0)
        self._check(self.lib.swa_d1_index_build_routed(self.h, C.c_void_p(d_ids_prefix.data_ptr() if n_prefix else 0), n_prefix,
                                                       C.c_void_p(d_ids_suffix.data_ptr() if n_suffix else 0), n_suffix, C.byref(dup)),
                    allow=(SWA_E_DUPLICATES,))
        return bool(dup.value)

    def d1_route_slice_records(self, first: int, count: int, world: int, d_records, cap: int, d_counts) -> None:
        """Routed multi-GPU index build with the key records travelling, step 1 (swa_d1_route_slice_records): torch tensors
        d_records int64 [2 * world * cap], d_counts int32 [2 * world + 1]."""
        self._check(self.lib.swa_d1_route_slice_records(self.h, first, count, world, C.c_void_p(d_records.data_ptr()), cap,
                                                        C.c_void_p(d_counts.data_ptr())))

    def d1_index_build_records(self, rec_prefix, rec_suffix) -> bool:
        """Step 3 (swa_d1_index_build_records): this rank's indexes from the key records it received; ownership must be set.
        Returns the duplicate flag of the build (identical sequences inside the rank's prefix groups are met by the
        network call: SwaError SWA_E_DUPLICATES there)."""
        dup = C.c_int(0)
        n_p, n_s = int(rec_prefix.numel()), int(rec_suffix.numel())
        self._check(self.lib.swa_d1_index_build_records(self.h, C.c_void_p(rec_prefix.data_ptr() if n_p else 0), n_p,
                                                        C.c_void_p(rec_suffix.data_ptr() if n_s else 0), n_s, C.byref(dup)),
                    allow=(SWA_E_DUPLICATES,))
        return bool(dup.value)

    def d1_has_duplicates(self, first: int = 0, count: int | None = None) -> bool:
        """The reference's duplicate check over both calls that can meet identical sequences (include/swarm_amd.h): the
        index build when it builds a table, else the network call's prefix pass.  (A test helper: index build + network.)"""
        if self.d1_index_build(first, count):
            return True
        try:
            self.d1_network(False, first, self.n - first if count is None else count)
        except SwaError as e:
            if e.code == SWA_E_DUPLICATES:
                return True
            raise
        return False

    def d1_network(self, no_cluster_breaking: bool = False, first: int = 0, count: int | None = None):
        """CSR over [first, first+count): (offsets u64[count+1], neighbours u32[total]), rows ascending.
        SwaError(SWA_E_DUPLICATES): identical sequences among the seeds' groups."""
        if count is None:
            count = self.n - first
        offsets = np.zeros(count + 1, dtype=np.uint64)
        cap = max(1024, 4 * count)
        total = C.c_uint64(0)
        while True:
            nb = np.zeros(cap, dtype=np.uint32)
            rc = self._check(self.lib.swa_d1_network(self.h, int(no_cluster_breaking), first, count,
                                                     _ptr(offsets), _ptr(nb), cap, C.byref(total)),
                             allow=(SWA_E_CAPACITY,))
            if rc == SWA_OK:
                return offsets, nb[:total.value]
            cap = int(total.value)

    def d1_anchor_windows(self):
        out = np.zeros(2, dtype=np.uint32)
        self.lib.swa_d1_anchor_windows.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.lib.swa_d1_anchor_windows(self.h, _ptr(out)))
        return int(out[0]), int(out[1])

    def d1_anchor_width(self) -> int:
        """Width of the anchor windows the last index build chose, in nucleotides (32, 64 or 128)."""
        self.lib.swa_d1_anchor_width.argtypes = [C.c_void_p]
        self.lib.swa_d1_anchor_width.restype = C.c_uint32
        return int(self.lib.swa_d1_anchor_width(self.h))

    def d1_network_resident(self, no_cluster_breaking: bool = False) -> int:
        """The network of the whole database computed into the context's own HBM buffers and kept there."""
        self.lib.swa_d1_network_resident.argtypes = [C.c_void_p, C.c_int, u64p]
        total = C.c_uint64(0)
        self._check(self.lib.swa_d1_network_resident(self.h, int(no_cluster_breaking), C.byref(total)))
        return int(total.value)

    def d1_network_fetch(self, total: int):
        self.lib.swa_d1_network_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        offsets = np.zeros(self.n + 1, dtype=np.uint64)
        nb = np.zeros(max(total, 1), dtype=np.uint32)
        self._check(self.lib.swa_d1_network_fetch(self.h, _ptr(offsets), _ptr(nb), len(nb)))
        return offsets, nb[:total]

    def d1_network_fetch_diffs(self, total: int) -> np.ndarray:
        """swa_d1_network_fetch_diffs: the byte of differences of every link of the resident d >= 2 graph, in the order
        of d1_network_fetch's neighbours"""
        self.lib.swa_d1_network_fetch_diffs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        diffs = np.zeros(max(total, 1), dtype=np.uint8)
        self._check(self.lib.swa_d1_network_fetch_diffs(self.h, _ptr(diffs), len(diffs)))
        return diffs[:total]

    def d1_network_adopt(self, offsets, neighbours, diffs=None) -> int:
        """swa_d1_network_adopt: a host CSR over the resident database's amplicons installed as the resident network (with
        `diffs`, a byte per link, as swa_dn_graph_resident leaves it).  Validated on the host before anything reaches the
        device; SwaError(SWA_E_ARG) for a malformed graph.  Returns the number of links."""
        self.lib.swa_d1_network_adopt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        neighbours = np.ascontiguousarray(neighbours, dtype=np.uint32)
        total = len(neighbours)
        if diffs is not None:
            diffs = np.ascontiguousarray(diffs, dtype=np.uint8)
            if len(diffs) != total:
                raise ValueError("d1_network_adopt: one byte of differences per link")
        if len(offsets) != self.n + 1:
            raise ValueError("d1_network_adopt: offsets needs one entry per amplicon of the resident database and one more")
        if diffs is not None and total == 0:
            diffs = np.zeros(1, dtype=np.uint8)                     # (a graph without links still says "with differences")
        self._check(self.lib.swa_d1_network_adopt(self.h, _ptr(offsets), _ptr(neighbours) if total else None,
                                                  _ptr(diffs) if diffs is not None else None, total))
        return total

    def d1_cluster_effort(self):
        """swa_d1_cluster_effort: (label sweeps launched, restarts of their numbering, level batches) of the last
        d1_cluster_device call."""
        self.lib.swa_d1_cluster_effort.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(3, dtype=np.uint32)
        self._check(self.lib.swa_d1_cluster_effort(self.h, _ptr(out)))
        return tuple(int(x) for x in out)

    def d1_cluster_maxgen(self) -> int:
        """swa_d1_cluster_maxgen: the deepest generation of the clustering in place"""
        self.lib.swa_d1_cluster_maxgen.argtypes = [C.c_void_p]
        self.lib.swa_d1_cluster_maxgen.restype = C.c_uint32
        return int(self.lib.swa_d1_cluster_maxgen(self.h))

    def d1_cluster_fetch(self):
        """swa_d1_cluster_fetch: (swarmid, generation, parent) of the clustering d1_cluster_device left in HBM"""
        self.lib.swa_d1_cluster_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        swarmid, generation, parent = (np.zeros(self.n, dtype=np.uint32) for _ in range(3))
        self._check(self.lib.swa_d1_cluster_fetch(self.h, _ptr(swarmid), _ptr(generation), _ptr(parent)))
        return swarmid, generation, parent

    def d1_cluster_device(self, swarm_cap: int | None = None, details: bool = True):
        """swa_d1_cluster_device on the resident network with all five result arrays on the host (none null):
        (swarmid, generation, parent, order, begins); the members of swarm s are order[begins[s]:begins[s + 1]].
        swarm_cap: the entries of the swarm table handed over at once (default: asked for first, by a call without a
        table); when it is too small, SwaError(SWA_E_CAPACITY) whose `nswarms` is the number needed.  details = False:
        swarmid / generation / parent are passed as null and stay in HBM (d1_cluster_fetch); three None come back."""
        lib = self.lib
        lib.swa_d1_cluster_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint32, u32p]
        swarmid, generation, parent, order = (np.zeros(self.n, dtype=np.uint32) for _ in range(4))
        three = (_ptr(swarmid), _ptr(generation), _ptr(parent)) if details else (None, None, None)
        nswarms = C.c_uint32(0)
        if swarm_cap is None:
            rc = self._check(lib.swa_d1_cluster_device(self.h, *three, _ptr(order), None, 0, C.byref(nswarms)), allow=(SWA_E_CAPACITY,))
            begins = np.zeros(1, dtype=np.uint32)
            if rc == SWA_E_CAPACITY:
                begins = np.zeros(nswarms.value + 1, dtype=np.uint32)
                self._check(lib.swa_d1_cluster_device(self.h, *three, _ptr(order), _ptr(begins), nswarms.value, C.byref(nswarms)))
        else:
            begins = np.zeros(int(swarm_cap) + 1, dtype=np.uint32)
            try:
                self._check(lib.swa_d1_cluster_device(self.h, *three, _ptr(order), _ptr(begins), int(swarm_cap), C.byref(nswarms)))
            except SwaError as e:
                e.nswarms = int(nswarms.value)
                raise
            begins = begins[:nswarms.value + 1]
        if not details:
            swarmid = generation = parent = None
        return swarmid, generation, parent, order, begins

    def d1_network_device(self, d_offsets, d_neighbours, cap: int, no_cluster_breaking: bool = False,
                          first: int = 0, count: int | None = None) -> int:
        """Device-resident CSR (torch tensors); returns the number of neighbours written."""
        if count is None:
            count = self.n - first
        total = C.c_uint64(0)
        self._check(self.lib.swa_d1_network_device(self.h, int(no_cluster_breaking), first, count,
                                                   _ptr(d_offsets), _ptr(d_neighbours), cap, C.byref(total)))
        return int(total.value)

    def d1_guard_retries(self) -> int:
        """Steps this context repeated because the guard's counts did not balance (swa_d1_guard_retries)."""
        self.lib.swa_d1_guard_retries.argtypes = [C.c_void_p]
        return int(self.lib.swa_d1_guard_retries(self.h))

    def d1_network_edges_device(self, d_edge_list, cap: int, no_cluster_breaking: bool = False,
                                first: int = 0, count: int | None = None) -> int:
        """The same links as one flat device list (int64 tensor): source << 32 | target, each once,
        unordered.  Returns the number of links; raises SwaError(SWA_E_CAPACITY) if cap is too small."""
        if count is None:
            count = self.n - first
        total = C.c_uint64(0)
        self._check(self.lib.swa_d1_network_edges_device(self.h, int(no_cluster_breaking), first, count,
                                                         _ptr(d_edge_list), cap, C.byref(total)))
        return int(total.value)

    def d1_links_split(self, d_links, m: int, bounds, d_out, d_counts) -> None:
        """The link exchange of a multi-GPU job, first half (swa_d1_links_split): the first m links of d_links
        (source << 32 | target) grouped by the rank that owns their source — rank r owns [bounds[r], bounds[r + 1]);
        bounds: world + 1 ascending ids on the host, bounds[0] = 0.  d_out [m] receives the runs, run r beginning at
        sum(d_counts[:r]); d_counts [world + 1] their sizes and, in [world], the links no rank owns (SwaError SWA_E_ARG
        then; they are written nowhere).  d_links / d_out / d_counts: 64-bit torch tensors on the context's device or raw
        device pointers; complete on return."""
        b = np.ascontiguousarray(bounds, dtype=np.uint32)
        self._check(self.lib.swa_d1_links_split(self.h, C.c_void_p(_dev(d_links)), int(m), b.ctypes.data_as(u32p), len(b) - 1,
                                                C.c_void_p(_dev(d_out)), C.c_void_p(_dev(d_counts))))

    def d1_csr_from_lists(self, d_links, starts, counts, first: int, count: int, d_offsets, d_neighbours, cap: int) -> int:
        """... second half (swa_d1_csr_from_lists): the CSR of the sources [first, first + count) from runs of links in one
        device buffer, run r = d_links[starts[r]: starts[r] + counts[r]] (host sequences).  d_offsets [count + 1] (64-bit,
        beginning at 0) is always complete; d_neighbours (32-bit, ascending within a row; None with cap = 0) is written up
        to cap entries.  Returns the entries needed; when they exceed cap raises SwaError(SWA_E_CAPACITY) whose `total`
        attribute holds the need.  Tensors on the context's device or raw device pointers."""
        st = np.ascontiguousarray(starts, dtype=np.uint64)
        ct = np.ascontiguousarray(counts, dtype=np.uint64)
        assert st.shape == ct.shape and st.ndim == 1
        total = C.c_uint64(0)
        rc = self.lib.swa_d1_csr_from_lists(self.h, C.c_void_p(_dev(d_links)), _p64(st), _p64(ct), len(st), int(first), int(count),
                                            C.c_void_p(_dev(d_offsets)), C.c_void_p(_dev(d_neighbours)), int(cap), C.byref(total))
        if rc != SWA_OK:
            err = SwaError(rc, self.lib.swa_last_error(self.h).decode())
            err.total = int(total.value)
            raise err
        return int(total.value)

    def d1_table_size(self) -> int:
        return int(self.lib.swa_d1_table_size(self.h))

    def d1_debug(self, what: int, count: int) -> np.ndarray:
        out = np.zeros(count, dtype=np.uint64)
        self._check(self.lib.swa_d1_debug_read(self.h, what, _ptr(out), out.nbytes))
        return out

    def d1_aux(self) -> np.ndarray:
        """Selector 3 of swa_d1_debug_read: the record k_seqhash writes per amplicon (AUX_DTYPE), n of them."""
        out = np.zeros(self.n, dtype=AUX_DTYPE)
        self._check(self.lib.swa_d1_debug_read(self.h, 3, _ptr(out), out.nbytes))
        return out

    def d1_db_facts(self) -> dict:
        """Selector 4: what the host keeps of k_db_lengths — the shortest sequence and the sequences per width class (up
        to 160, 256, 480, 672 nt, longer) — and SWA_MAX_ZOBRIST_LDS of the build."""
        w = self.d1_debug(4, 4).view(np.uint32)
        return {"shortest": int(w[0]), "class_pop": [int(v) for v in w[1:6]], "max_zobrist_lds": int(w[6])}

    def d1_window_sample(self) -> dict:
        """Selector 5: the window sample of this upload as choose_anchor_windows saw it, and the choice made from it (before
        the safety net of the first build)."""
        w = self.d1_debug(5, 8).view(np.uint32)
        return {"too_short": [int(v) for v in w[0:4]], "mass": [int(v) for v in w[4:8]], "stride": int(w[8]), "samples": int(w[9]),
                "offset": int(w[10]), "width": int(w[11]), "taken": bool(w[12])}

    def d1_lists_form(self) -> int:
        """swa_d1_lists_form: the form the work lists of the streaming index in place were built with (lists_form_for)"""
        form = self.lib.swa_d1_lists_form(self.h)
        if form < 0:
            raise SwaError(2, "swa_d1_lists_form: no streaming index in place")
        return form

    def d1_part_plan(self) -> list:
        """swa_d1_part_plan: the key partition of the streaming index in place, laid out as part_plan_for() with the bits
        a key-overflow retry added in [7]."""
        out = np.zeros(8, dtype=np.uint32)
        self._check(self.lib.swa_d1_part_plan(self.h, _ptr(out)))
        return [int(v) for v in out]

    def d1_bucket_starts(self, which: int) -> np.ndarray:
        """Selectors 17 / 18 of swa_d1_debug_read: first record of every bucket of the key partition of the prefix (0) /
        suffix (1) index and, last, the number of records; to be read before the first network call."""
        return self.d1_debug(17 + int(which), (1 << self.d1_part_plan()[0]) + 1)

    # ---- B2
    def d1_fastidious(self, is_light: np.ndarray, light_nt: int, bloom_bits: int = 16, shard: int = 0,
                      nshards: int = 1):
        """B2.  With nshards > 1 only slice `shard` of the heavy amplicons is expanded on this GPU;
        combine the shards with sharding.combine_grafts (minimum of graft_cand, sum of counters 1, 2)."""
        is_light = np.ascontiguousarray(is_light, dtype=np.uint8)
        graft = np.zeros(self.n, dtype=np.uint32)
        counters = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.swa_d1_fastidious_shard(self.h, _ptr(is_light), int(light_nt), int(bloom_bits),
                                                     int(shard), int(nshards), _ptr(graft), _ptr(counters)))
        return graft, counters

    def d1_swarm_sums_device(self, nswarms: int | None = None):
        """swa_d1_swarm_sums_device: (mass u64, sumlen u64, singletons u32, maxgen u32) of every swarm of the clustering
        in place, summed on the device.  nswarms: the entries of the arrays to hand over (the number of swarms, which
        d1_cluster_device told; fewer: SwaError SWA_E_CAPACITY); None: no array, the sums only stay in HBM."""
        if nswarms is None:
            self._check(self.lib.swa_d1_swarm_sums_device(self.h, None, None, None, None, 0))
            return None
        w = int(nswarms)
        mass, sumlen = np.zeros(w, dtype=np.uint64), np.zeros(w, dtype=np.uint64)
        singletons, maxgen = np.zeros(w, dtype=np.uint32), np.zeros(w, dtype=np.uint32)
        self._check(self.lib.swa_d1_swarm_sums_device(self.h, _ptr(mass), _ptr(sumlen), _ptr(singletons), _ptr(maxgen), w))
        return mass, sumlen, singletons, maxgen

    def d1_light_flags_device(self, boundary: int = 3, flags: bool = True):
        """swa_d1_light_flags_device: (is_light u8[n] or None, [light swarms, light amplicons, their nt, heavy swarms,
        heavy amplicons]); the flags stay in HBM for d1_fastidious_resident either way."""
        is_light = np.zeros(self.n, dtype=np.uint8) if flags else None
        stats = np.zeros(5, dtype=np.uint64)
        self._check(self.lib.swa_d1_light_flags_device(self.h, int(boundary), _ptr(is_light), _p64(stats)))
        return is_light, [int(x) for x in stats]

    def d1_fastidious_resident(self, light_nt: int, bloom_bits: int = 16, fetch: bool = True):
        """swa_d1_fastidious_resident: the second pass with its roles from the flags d1_light_flags_device left in HBM.
        (graft_cand or None when fetch is False: the candidates then stay in HBM for d1_graft_device, counters)."""
        graft = np.zeros(self.n, dtype=np.uint32) if fetch else None
        counters = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.swa_d1_fastidious_resident(self.h, int(light_nt), int(bloom_bits), _ptr(graft), _ptr(counters)))
        return graft, counters

    def d1_shard_owners_device(self, nshards: int, fetch: bool = True):
        """swa_d1_shard_owners_device: (owner u8[n] or None, H).  owner[a] = 255 for an amplicon of a light swarm, else the
        shard of `nshards` that expands heavy amplicon a; made from the flags d1_light_flags_device left in HBM, where the
        bytes stay."""
        owners = np.zeros(self.n, dtype=np.uint8) if fetch else None
        heavy = C.c_uint64(0)
        self._check(self.lib.swa_d1_shard_owners_device(self.h, int(nshards), _ptr(owners), C.byref(heavy)))
        return owners, int(heavy.value)

    def merge_sorted_lists(self, keys, vals, at, world: int | None = None, out_keys=None, out_vals=None):
        """swa_merge_sorted_lists: the merge rank 0 of a MultiContext runs on the gathered shares of a d >= 2 graph, on host
        arrays: list r = keys / vals [at[r], at[r + 1]), sorted by key; (merged keys, merged values), equal keys in list
        order.  world: len(at) - 1 unless given; out_keys / out_vals: arrays to write into (at[world] entries at least)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        at = np.ascontiguousarray(at, dtype=np.uint64)
        if world is None:
            world = len(at) - 1
        count = int(at[world]) if 0 <= world < len(at) else 0
        if len(keys) < count or len(vals) < count:
            raise ValueError("merge_sorted_lists: fewer keys or values than at[world]")
        out_keys = np.zeros(count, dtype=np.uint64) if out_keys is None else out_keys
        out_vals = np.zeros(count, dtype=np.uint32) if out_vals is None else out_vals
        if out_keys.dtype != np.uint64 or out_vals.dtype != np.uint32 or len(out_keys) < count or len(out_vals) < count:
            raise ValueError("merge_sorted_lists: out_keys u64 / out_vals u32 of at[world] entries")
        self._check(self.lib.swa_merge_sorted_lists(self.h, _ptr(keys), _ptr(vals), _ptr(at), int(world), _ptr(out_keys), _ptr(out_vals)))
        return out_keys, out_vals

    def d1_graft_device(self, graft_cand=None, cap: int | None = None):
        """swa_d1_graft_device: (heavy swarm, light swarm, parent, child) of the G grafts in chain order.  graft_cand: n
        candidates on the host, or None for those the last fastidious pass left in HBM.  cap: entries of the result arrays
        (default: asked for first); SwaError(SWA_E_CAPACITY) whose `grafts` is the need when it is too small.  cap = 0: no
        arrays are wanted — the grafts stay in HBM for d1_graft_layout_device, four empty arrays come back."""
        cand = None if graft_cand is None else np.ascontiguousarray(graft_cand, dtype=np.uint32)
        if cand is not None and len(cand) != self.n:
            raise ValueError("d1_graft_device: one candidate per amplicon of the resident database")
        made = C.c_uint32(0)
        if cap is not None and int(cap) == 0:
            self._check(self.lib.swa_d1_graft_device(self.h, _ptr(cand), None, None, None, None, 0, C.byref(made)))
            return tuple(np.zeros(0, dtype=np.uint32) for _ in range(4))
        if cap is None:
            rc = self._check(self.lib.swa_d1_graft_device(self.h, _ptr(cand), None, None, None, _ptr(np.zeros(1, dtype=np.uint32)), 0,
                                                          C.byref(made)), allow=(SWA_E_CAPACITY,))
            cap = int(made.value)
            if rc == SWA_OK:
                return tuple(np.zeros(0, dtype=np.uint32) for _ in range(4))
        four = [np.zeros(max(int(cap), 1), dtype=np.uint32) for _ in range(4)]
        rc = self.lib.swa_d1_graft_device(self.h, _ptr(cand), *(_ptr(a) for a in four), int(cap), C.byref(made))
        if rc != SWA_OK:
            err = SwaError(rc, self.lib.swa_last_error(self.h).decode())
            err.grafts = int(made.value)
            raise err
        return tuple(a[:made.value] for a in four)

    def d1_graft_layout_info(self) -> dict:
        """swa_d1_graft_layout_info: whether a layout is in place, and of how many amplicons, swarms and grafts"""
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.swa_d1_graft_layout_info(self.h, _ptr(out)))
        return {"in_place": bool(out[0]), "n": int(out[1]), "swarms": int(out[2]), "grafts": int(out[3])}

    def d1_graft_layout_device(self, fetch: bool = True, nswarms: int | None = None) -> dict:
        """swa_d1_graft_layout_device: the grafted clustering laid out in HBM from the grafts of the last d1_graft_device call.
        {"printed_order": u32[n], "new_begin": u32[w], "grown": u32[w], "attached": u8[w] (all None when fetch is False),
        "summary": [printed swarms, largest printed swarm, grafts]}.  nswarms: entries of the per-swarm arrays (default:
        the swarms of the clustering; fewer: SwaError(SWA_E_CAPACITY))."""
        summary = np.zeros(3, dtype=np.uint64)
        if nswarms is None or not fetch:
            self._check(self.lib.swa_d1_graft_layout_device(self.h, None, None, None, None, 0xFFFFFFFF if nswarms is None else int(nswarms), _ptr(summary)))
            if nswarms is None:
                nswarms = self.d1_graft_layout_info()["swarms"]
        out = {"printed_order": None, "new_begin": None, "grown": None, "attached": None}
        if fetch:
            room = max(int(nswarms), 1)
            out = {"printed_order": np.zeros(self.n, dtype=np.uint32), "new_begin": np.zeros(room, dtype=np.uint32),
                   "grown": np.zeros(room, dtype=np.uint32), "attached": np.zeros(room, dtype=np.uint8)}
            self._check(self.lib.swa_d1_graft_layout_device(self.h, _ptr(out["printed_order"]), _ptr(out["new_begin"]), _ptr(out["grown"]),
                                                            _ptr(out["attached"]), int(nswarms), _ptr(summary)))
            for k in ("new_begin", "grown", "attached"):
                out[k] = out[k][:int(nswarms)]
        out["summary"] = [int(v) for v in summary]
        return out

    def d1_graft_candidates(self) -> np.ndarray:
        """swa_d1_graft_candidates_fetch: the candidates as they lie in HBM (after d1_graft_device: the winners' only)"""
        out = np.zeros(self.n, dtype=np.uint32)
        self._check(self.lib.swa_d1_graft_candidates_fetch(self.h, _ptr(out)))
        return out

    def d1_fastidious_plan(self) -> list:
        """swa_d1_fastidious_plan: [pair route, pair kernel words (0: packed words), count kernel words (0: the LDS set,
        1: k_fast_count_sites_words), the count kernel's waves, slots, LDS bytes, Zobrist table in LDS on the Bloom route, kFastMinLen]"""
        out = np.zeros(8, dtype=np.uint32)
        self._check(self.lib.swa_d1_fastidious_plan(self.h, _ptr(out)))
        return [int(v) for v in out]

    def d1_fastidious_split(self) -> list:
        """swa_d1_fastidious_split: [1 when SWA_FAST_LONG=split divides the pass for the resident database (2: SWA_FAST_LONG=pairs
        serves it), the cap of the pair route in effect, the longest sequence <= cap, amplicons longer than cap]"""
        out = np.zeros(4, dtype=np.uint32)
        self._check(self.lib.swa_d1_fastidious_split(self.h, _ptr(out)))
        return [int(v) for v in out]

    def d1_fastidious_totals(self) -> list:
        """swa_d1_fastidious_totals of the last d1_fastidious call: [pairs the pair route found, light amplicons and
        heavy amplicons handed to the Bloom route (short band and, under the split, long band), attempts of the pair list]"""
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.swa_d1_fastidious_totals(self.h, _ptr(out)))
        return [int(v) for v in out]

    def d1_fastidious_bloom_batches(self) -> list:
        """swa_d1_fastidious_bloom_batches of the last d1_fastidious call: [launches of the heavy side's enumeration, those
        that overflowed the task list and were redone, the task cap in effect, the most tasks of a batch that ran]; all
        zero when the Bloom route did not run"""
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.swa_d1_fastidious_bloom_batches(self.h, _ptr(out)))
        return [int(v) for v in out]

    def d1_fastidious_bloom_read(self, words: bool = True, cap_words: int | None = None):
        """swa_d1_fastidious_bloom_read of the last d1_fastidious call: ([fsize, m, k, bloom_bits, tasks of the batches that
        ran, 0, 0, 0], the fsize words of the filter as the light pass left them); the array is None with words=False and
        when the Bloom route did not run.  cap_words: the room offered instead of fsize (less: SwaError(SWA_E_CAPACITY))."""
        facts = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.swa_d1_fastidious_bloom_read(self.h, _ptr(facts), None, 0))
        fsize = int(facts[0])
        if not words or fsize == 0:
            return [int(v) for v in facts], None
        room = fsize if cap_words is None else int(cap_words)
        out = np.zeros(max(room, 1), dtype=np.uint64)
        self._check(self.lib.swa_d1_fastidious_bloom_read(self.h, _ptr(facts), _ptr(out), room))
        return [int(v) for v in facts], out[:fsize]

    # ---- B3
    def qgram_build(self) -> None:
        self._check(self.lib.swa_qgram_build(self.h))

    def qgram_diff(self, seed: int, amplist: np.ndarray) -> np.ndarray:
        amplist = np.ascontiguousarray(amplist, dtype=np.uint64)
        out = np.zeros(amplist.shape[0], dtype=np.uint64)
        self._check(self.lib.swa_qgram_diff(self.h, int(seed), amplist.shape[0], _ptr(amplist), _ptr(out)))
        return out

    def qgram_signatures(self) -> np.ndarray:
        out = np.zeros((self.n, 128), dtype=np.uint8)
        self._check(self.lib.swa_qgram_debug_read(self.h, _ptr(out), out.nbytes))
        return out

    # ---- B3 + B4 in bulk (dn_graph.hip); after qgram_build + search_begin
    def dn_graph_supported(self) -> bool:
        """swa_dn_graph_supported: d <= 16 and few enough candidate pairs with a sequence too short for d + 1 windows"""
        self.lib.swa_dn_graph_supported.argtypes = [C.c_void_p]
        return bool(self.lib.swa_dn_graph_supported(self.h))

    def dn_graph_raw(self, cap: int, no_cluster_breaking: bool = False):
        """One swa_dn_graph call with room for `cap` entries: (return code, offsets, neighbours, diffs, total)."""
        self.lib.swa_dn_graph.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
        offsets = np.zeros(self.n + 1, dtype=np.uint64)
        nb = np.zeros(max(1, cap), dtype=np.uint32)
        df = np.zeros(max(1, cap), dtype=np.uint8)
        total = C.c_uint64(0)
        rc = self.lib.swa_dn_graph(self.h, int(no_cluster_breaking), _ptr(offsets), _ptr(nb) if cap else None,
                                   _ptr(df) if cap else None, cap, C.byref(total))
        return rc, offsets, nb[:min(cap, total.value)], df[:min(cap, total.value)], int(total.value)

    def dn_graph(self, no_cluster_breaking: bool = False):
        """swa_dn_graph by its capacity protocol (cap = 0, then the total): (offsets, neighbours, diffs)."""
        rc, offsets, nb, df, total = self.dn_graph_raw(0, no_cluster_breaking)
        if rc == SWA_E_CAPACITY:
            rc, offsets, nb, df, total = self.dn_graph_raw(total, no_cluster_breaking)
        self._check(rc)
        return offsets, nb, df

    def dn_graph_totals(self) -> dict:
        out = np.zeros(3, dtype=np.uint64)
        self.lib.swa_dn_graph_totals.argtypes = [C.c_void_p, u64p]
        self._check(self.lib.swa_dn_graph_totals(self.h, _p64(out)))
        return {"qgram_comparisons": int(out[0]), "aligned_pairs": int(out[1]), "launch_sequences": int(out[2])}

    def dn_graph_resident(self, no_cluster_breaking: bool = False) -> int:
        """swa_dn_graph_resident: the graph left in HBM for d1_cluster_device; returns its number of links."""
        self.lib.swa_dn_graph_resident.argtypes = [C.c_void_p, C.c_int, u64p]
        total = C.c_uint64(0)
        self._check(self.lib.swa_dn_graph_resident(self.h, int(no_cluster_breaking), C.byref(total)))
        return int(total.value)

    def dn_parent_diffs(self) -> np.ndarray:
        """swa_dn_parent_diffs: per amplicon the differences to its parent in the clustering d1_cluster_device just made"""
        self.lib.swa_dn_parent_diffs.argtypes = [C.c_void_p, C.c_void_p]
        out = np.zeros(self.n, dtype=np.uint8)
        self._check(self.lib.swa_dn_parent_diffs(self.h, _ptr(out)))
        return out

    def dn_tables_device(self) -> tuple:
        """swa_dn_tables_device: radii, per-swarm sums and the links in acceptance order of the clustering d1_cluster_device
        just made of a graph with differences, made and left in HBM; returns (nswarms, nlinks)"""
        _declare_dn(self.lib)
        nswarms, nlinks = C.c_uint32(0), C.c_uint64(0)
        self._check(self.lib.swa_dn_tables_device(self.h, C.byref(nswarms), C.byref(nlinks)))
        self._dn_tables_sizes = (int(nswarms.value), int(nlinks.value))
        return self._dn_tables_sizes

    def dn_tables_serial(self) -> int:
        """swa_dn_tables_serial: which dn_tables_device call of this context made the tables in place (from 1), 0: none"""
        _declare_dn(self.lib)
        return int(self.lib.swa_dn_tables_serial(self.h))

    def dn_tables_fetch(self) -> dict:
        """swa_dn_tables_fetch: the nine arrays of the tables dn_tables_device made — radius [n]; mass, singletons, maxgen,
        maxradius [nswarms]; link_parent, link_child, link_generation, link_diff [nlinks]"""
        _declare_dn(self.lib)
        nswarms, nlinks = getattr(self, "_dn_tables_sizes", (0, 0))
        out = {"radius": np.zeros(self.n, dtype=np.uint32), "mass": np.zeros(nswarms, dtype=np.uint64)}
        for name in ("singletons", "maxgen", "maxradius"):
            out[name] = np.zeros(nswarms, dtype=np.uint32)
        for name in ("link_parent", "link_child", "link_generation"):
            out[name] = np.zeros(nlinks, dtype=np.uint32)
        out["link_diff"] = np.zeros(nlinks, dtype=np.uint8)
        self._check(self.lib.swa_dn_tables_fetch(self.h, *(_ptr(a) for a in out.values())))
        return out

    # ---- B4
    def search_begin(self, mismatch: int = 18, gapopen: int = 24, gapextend: int = 13, d: int = 3) -> None:
        self._check(self.lib.swa_search_begin(self.h, mismatch, gapopen, gapextend, d))

    def search_uses_wavefront(self) -> bool:
        self.lib.swa_search_uses_wavefront.argtypes = [C.c_void_p]
        return bool(self.lib.swa_search_uses_wavefront(self.h))

    SEARCH_FORMS = {1: "wfa16", 2: "wfa32", 3: "banded32", 4: "banded32_len", 5: "banded64", 6: "banded64_len", 7: "generic",
                    8: "wide2", 9: "wide2_len", 10: "wide4", 11: "wide4_len", 12: "wide8", 13: "wide8_len"}

    def search_form(self, with_lengths: bool = True) -> tuple:
        """(form, saturation, LDS bytes a workgroup) of the alignment kernel a launch takes for the penalties / d of
        search_begin and the resident database (swa_search_form): form one of SEARCH_FORMS' names; with_lengths as
        search_do(lengths=...)."""
        self.lib.swa_search_form.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint64)]
        form, sat, lds = C.c_int(0), C.c_uint32(0), C.c_uint64(0)
        self._check(self.lib.swa_search_form(self.h, int(with_lengths), C.byref(form), C.byref(sat), C.byref(lds)))
        return self.SEARCH_FORMS[form.value], int(sat.value), int(lds.value)

    def search_do(self, query: int, targets: np.ndarray, lengths: bool = True):
        """(scores, diffs, alignment lengths) of `query` against `targets`; lengths=False asks for the differences alone
        (NULL scores and lengths: the kernel forms the scan and graph routes launch) and returns (None, diffs, None)."""
        targets = np.ascontiguousarray(targets, dtype=np.uint64)
        m = targets.shape[0]
        diffs = np.zeros(m, dtype=np.uint64)
        scores = np.zeros(m, dtype=np.uint64) if lengths else None
        alens = np.zeros(m, dtype=np.uint64) if lengths else None
        self._check(self.lib.swa_search_do(self.h, int(query), m, _ptr(targets), _ptr(scores), _ptr(diffs),
                                           _ptr(alens)))
        return scores, diffs, alens

    # ---- B3 + B4 fused, one batch of (sub)seeds at a time (scan.hip); after qgram_build + search_begin
    def scan_begin(self) -> None:
        _declare_dn(self.lib)
        self._check(self.lib.swa_scan_begin(self.h))

    def scan_batch(self, seeds, radii, lowest_unswarmed: int, first_generation: bool, ncb: bool, cap: int | None = None):
        """One swa_scan_batch call with room for `cap` hits (default: the database): (return code, nhits, seed indices,
        ids, diffs) — the three arrays hold min(nhits, cap) sorted triples after SWA_OK and nothing after another code."""
        _declare_dn(self.lib)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        radii = np.ascontiguousarray(radii, dtype=np.uint32)
        assert seeds.shape == radii.shape
        cap = self.n if cap is None else int(cap)
        sidx, ids, diffs = (np.zeros(max(1, cap), dtype=np.uint32) for _ in range(3))
        nh = C.c_uint32(0)
        rc = self.lib.swa_scan_batch(self.h, seeds.shape[0], _ptr(seeds), _ptr(radii), int(lowest_unswarmed), int(first_generation),
                                     int(ncb), _ptr(sidx), _ptr(ids), _ptr(diffs), cap, C.byref(nh))
        k = min(int(nh.value), cap) if rc == SWA_OK else 0
        return rc, int(nh.value), sidx[:k], ids[:k], diffs[:k]

    def scan_fetch(self, nhits: int):
        """swa_scan_fetch: the sorted (seed indices, ids, diffs) of the most recent scan_batch"""
        _declare_dn(self.lib)
        sidx, ids, diffs = (np.zeros(max(1, int(nhits)), dtype=np.uint32) for _ in range(3))
        self._check(self.lib.swa_scan_fetch(self.h, _ptr(sidx), _ptr(ids), _ptr(diffs), int(nhits)))
        return sidx[:nhits], ids[:nhits], diffs[:nhits]

    def scan_totals(self) -> dict:
        _declare_dn(self.lib)
        out = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.swa_scan_totals(self.h, _p64(out)))
        return {"qgram_comparisons": int(out[0]), "aligned_pairs": int(out[1]), "launch_sequences": int(out[2])}

    def scan_debug_state(self) -> dict:
        """swa_scan_debug_state: which of the scan step's rare branches this context has taken"""
        _declare_dn(self.lib)
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.swa_scan_debug_state(self.h, _p64(out)))
        return {"pair_cap": int(out[0]), "redone": int(out[1]), "relists": int(out[2]), "by_copy": int(out[3])}

    def nw_batch(self, d_ids, q_ids, mismatch: int = 18, gapopen: int = 24, gapextend: int = 13):
        """Seam B5 (swa_nw_batch): global alignments of amplicons d_ids[k] (member) against q_ids[k] (seed) of the
        resident database -> (diffs, columns, list of CIGAR strings)."""
        _declare_dn(self.lib)
        return _nw_batch_call(self.lib.swa_nw_batch, self, d_ids, q_ids, mismatch, gapopen, gapextend)

    def nw_batch_totals(self) -> list:
        """pairs of the last nw_batch: [16-lane, 32-lane, 64-lane LDS tier, left by the LDS tiers (wide tiers + host)]"""
        _declare_dn(self.lib)
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.swa_nw_batch_totals(self.h, _p64(out)))
        return [int(v) for v in out]

    def nw_batch_tiers(self) -> list:
        """pairs of the last nw_batch per tier: the three LDS tiers (band half-width 6, 14, 30), the four wide tiers
        (30, 62, 126, 254), the host"""
        _declare_dn(self.lib)
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.swa_nw_batch_tiers(self.h, _p64(out)))
        return [int(v) for v in out]

    def nw_batch_text_full(self) -> int:
        """pairs of the last nw_batch that went to the host only because the device's CIGAR buffer was full"""
        _declare_dn(self.lib)
        out = np.zeros(1, dtype=np.uint64)
        self._check(self.lib.swa_nw_batch_text_full(self.h, _p64(out)))
        return int(out[0])


def _nw_batch_call(fn, owner, d_ids, q_ids, mismatch, gapopen, gapextend):
    """swa_nw_batch or swa_multi_nw_batch on owner.h, with their capacity protocol -> (diffs, columns, CIGAR strings)"""
    d_ids = np.ascontiguousarray(d_ids, dtype=np.uint32)
    q_ids = np.ascontiguousarray(q_ids, dtype=np.uint32)
    m = len(d_ids)
    assert len(q_ids) == m
    diffs = np.zeros(m, dtype=np.uint32)
    cols = np.zeros(m, dtype=np.uint32)
    ends = np.zeros(m, dtype=np.uint64)
    total = C.c_uint64(0)
    cap = 16 * m + 64
    while True:
        buf = C.create_string_buffer(max(cap, 1))
        rc = fn(owner.h, mismatch, gapopen, gapextend, m, _ptr(d_ids), _ptr(q_ids), _ptr(diffs), _ptr(cols), _ptr(ends), buf, cap,
                C.byref(total))
        if rc == SWA_E_CAPACITY and total.value > cap:
            cap = int(total.value)
            continue
        owner._check(rc)
        break
    raw = buf.raw[:int(total.value)]
    starts = np.concatenate(([0], ends[:-1])).astype(np.int64) if m else []
    cigars = [raw[int(a):int(b)].decode() for a, b in zip(starts, ends)]
    return diffs, cols, cigars


# ---- d >= 2: host greedy loop over the GPU's fused scan step ---------------------------------

_DN_EXPORTS = ["swa_dn_cluster", "swa_dn_result_free", "swa_dn_result_error", "swa_dn_result_summary", "swa_dn_result_over_graph",
               "swa_dn_write_swarms", "swa_dn_write_stats", "swa_dn_write_structure", "swa_dn_write_seeds",
               "swa_dn_write_uclust", "swa_d1_write_uclust", "swa_scan_begin", "swa_scan_step", "swa_scan_batch", "swa_scan_fetch", "swa_scan_totals", "swa_scan_debug_state",
               "swa_dn_graph_supported", "swa_dn_graph", "swa_dn_graph_totals", "swa_dn_graph_resident", "swa_dn_parent_diffs",
               "swa_dn_tables_device", "swa_dn_tables_fetch", "swa_dn_tables_serial", "swa_dn_result_link_fetches",
               "swa_multi_create", "swa_multi_destroy", "swa_multi_size", "swa_multi_uses_rccl", "swa_multi_ctx", "swa_multi_last_error",
               "swa_multi_db_upload", "swa_multi_d1_network", "swa_multi_d1_fastidious", "swa_dn_set_ownership", "swa_multi_dn_begin",
               "swa_multi_dn_graph_supported", "swa_multi_dn_graph", "swa_multi_dn_graph_totals", "swa_dn_cluster_multi",
               "swa_timing_read_stream", "swa_nw_batch", "swa_nw_batch_totals", "swa_nw_batch_tiers", "swa_nw_batch_text_full", "swa_d1_write_uclust_gpu", "swa_dn_write_uclust_gpu",
               "swa_nw_align_host"]
EXPORTS.extend(_DN_EXPORTS)


def reduced_penalties(match_reward: int = 5, mismatch_penalty: int = 4, gap_open: int = 12, gap_extend: int = 4):
    """The reference's scoring reduction (src/swarm.cc:466-483): (2m+2p, 2g, m+2e) / gcd -> 18, 24, 13."""
    from math import gcd
    mm = 2 * match_reward + 2 * mismatch_penalty
    go = 2 * gap_open
    ge = match_reward + 2 * gap_extend
    f = gcd(gcd(mm, go), ge)
    return mm // f, go // f, ge // f


def _declare_dn(lib) -> None:
    if getattr(lib, "_dn_declared", False):
        return
    lib.swa_dn_cluster.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.POINTER(C.c_void_p)]
    lib.swa_dn_result_free.argtypes = [C.c_void_p]
    lib.swa_dn_result_free.restype = None
    lib.swa_dn_result_error.argtypes = [C.c_void_p]
    lib.swa_dn_result_error.restype = C.c_char_p
    lib.swa_dn_result_summary.argtypes = [C.c_void_p, u64p]
    lib.swa_dn_result_summary.restype = None
    lib.swa_dn_result_link_fetches.argtypes = [C.c_void_p]
    lib.swa_dn_result_link_fetches.restype = C.c_uint32
    lib.swa_dn_tables_device.argtypes = [C.c_void_p, u32p, u64p]
    lib.swa_dn_tables_fetch.argtypes = [C.c_void_p] + [C.c_void_p] * 9
    lib.swa_dn_tables_serial.argtypes = [C.c_void_p]
    lib.swa_dn_tables_serial.restype = C.c_uint64
    lib.swa_dn_write_swarms.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int64]
    for fn in (lib.swa_dn_write_stats, lib.swa_dn_write_structure, lib.swa_dn_write_seeds):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.swa_dn_write_uclust.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int64]
    lib.swa_d1_write_uclust.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint64,
                                        C.c_uint64]
    lib.swa_scan_begin.argtypes = [C.c_void_p]
    lib.swa_scan_step.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_uint32, u32p]
    lib.swa_scan_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_uint32, u32p]
    lib.swa_scan_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.swa_scan_totals.argtypes = [C.c_void_p, u64p]
    lib.swa_scan_debug_state.argtypes = [C.c_void_p, u64p]
    lib.swa_dn_write_uclust_gpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int64]
    lib.swa_d1_write_uclust_gpu.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_uint64,
                                            C.c_uint64, C.c_uint64]
    lib.swa_nw_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    lib.swa_nw_batch_totals.argtypes = [C.c_void_p, u64p]
    lib.swa_nw_batch_tiers.argtypes = [C.c_void_p, u64p]
    lib.swa_nw_batch_text_full.argtypes = [C.c_void_p, u64p]
    lib.swa_nw_align_host.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                      u64p, C.c_char_p, C.c_uint64, u64p]
    lib.swa_nw_align_host.restype = C.c_uint64
    lib._dn_declared = True


class DnClusters:
    """d >= 2 clustering: the reference's algo_run loop (src/algo.cc:384-676) with every
    q-gram / alignment step executed on the GPU (swa_scan_step)."""

    def __init__(self, ctx: "Context", hdb: HostDb, differences: int, no_cluster_breaking: bool = False,
                 penalties=None, multi: "MultiContext | None" = None):
        self.lib = load_library()
        _declare_dn(self.lib)
        _declare_multi_scan(self.lib)
        self.hdb = hdb
        self.ctx = ctx                    # (multi: rank 0's, which the writers use)
        self.multi = multi
        mm, go, ge = penalties or reduced_penalties()
        h = C.c_void_p()
        if multi is not None:
            rc = self.lib.swa_dn_cluster_multi(multi.h, hdb.h, differences, int(no_cluster_breaking), mm, go, ge, C.byref(h))
        else:
            rc = self.lib.swa_dn_cluster(ctx.h, hdb.h, differences, int(no_cluster_breaking), mm, go, ge, C.byref(h))
        self.h = h
        if rc != SWA_OK:
            raise SwaError(rc, self.lib.swa_dn_result_error(h).decode() if h else "swa_dn_cluster failed")

    def route(self):
        """(route, ranks): ("graph", 0) when the bulk graph served, else ("scan", the ranks the fused scan ran on: 1 for one
        context — also rank 0 alone under SWARM_AMD_MULTI_SCAN=root —, else the ranks of the MultiContext)"""
        self.lib.swa_dn_result_over_graph.argtypes = [C.c_void_p]
        ranks = int(self.lib.swa_dn_result_scan_ranks(self.h))
        return ("graph", 0) if self.lib.swa_dn_result_over_graph(self.h) else ("scan", ranks)

    def summary(self) -> dict:
        out = np.zeros(3, dtype=np.uint64)
        self.lib.swa_dn_result_summary(self.h, _p64(out))
        return {"swarms": int(out[0]), "largest": int(out[1]), "maxgen": int(out[2])}

    def link_fetches(self) -> int:
        """swa_dn_result_link_fetches: downloads of the -i / -u links made for this result (SWARM_AMD_DN_TABLES=device keeps
        them in HBM until a writer reads them: 0 after -o, -s, -w alone, else 1)"""
        return int(self.lib.swa_dn_result_link_fetches(self.h))

    def scan_totals(self) -> dict:
        """Work counters of the route that ran: the bulk graph (swa_dn_graph) or the fused scan (swa_scan_*)."""
        out = np.zeros(3, dtype=np.uint64)
        self.lib.swa_dn_graph_totals.argtypes = [C.c_void_p, u64p]
        self.lib.swa_dn_result_over_graph.argtypes = [C.c_void_p]
        if self.lib.swa_dn_result_over_graph(self.h):
            self.ctx._check(self.lib.swa_dn_graph_totals(self.ctx.h, _p64(out)))
            return {"route": "graph", "qgram_comparisons": int(out[0]), "aligned_pairs": int(out[1]), "launch_sequences": int(out[2])}
        if self.multi is not None and self.route()[1] > 1:
            return {"route": "scan", **self.multi.scan_totals()}
        self.ctx._check(self.lib.swa_scan_totals(self.ctx.h, _p64(out)))
        return {"route": "scan", "qgram_comparisons": int(out[0]), "aligned_pairs": int(out[1]), "launch_sequences": int(out[2])}

    def write_swarms(self, path, mothur=False, usearch=False, append_abundance=0) -> None:
        assert self.lib.swa_dn_write_swarms(self.h, self.hdb.h, str(path).encode(), int(mothur), int(usearch),
                                            append_abundance) == SWA_OK

    def write_stats(self, path, usearch=False) -> None:
        assert self.lib.swa_dn_write_stats(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_structure(self, path, usearch=False) -> None:
        assert self.lib.swa_dn_write_structure(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_seeds(self, path, usearch=False) -> None:
        assert self.lib.swa_dn_write_seeds(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_uclust(self, path, usearch=False, append_abundance=0, ctx: "Context | MultiContext | None" = None) -> None:
        """-u; with ctx= the alignments run on that context's GPU (seam B5, swa_dn_write_uclust_gpu), or divided among the
        ranks of a MultiContext (swa_dn_write_uclust_multi)."""
        if isinstance(ctx, MultiContext):
            ctx._check(self.lib.swa_dn_write_uclust_multi(ctx.h, self.h, self.hdb.h, str(path).encode(), int(usearch),
                                                          append_abundance))
            return
        if ctx is not None:
            ctx._check(self.lib.swa_dn_write_uclust_gpu(ctx.h, self.h, self.hdb.h, str(path).encode(), int(usearch),
                                                        append_abundance))
            return
        assert self.lib.swa_dn_write_uclust(self.h, self.hdb.h, str(path).encode(), int(usearch),
                                            append_abundance) == SWA_OK

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.swa_dn_result_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- d = 0: dereplication ----------------------------------------------------------------------

_D0_EXPORTS = ["swa_derep", "swa_derep_resident", "swa_d0_cluster_device", "swa_d0_cluster_fetch", "swa_d0_cluster_resident",
               "swa_d0_result_tables", "swa_d0_cluster", "swa_d0_result_free", "swa_d0_result_summary", "swa_d0_write_swarms",
               "swa_d0_write_seeds", "swa_d0_write_stats", "swa_d0_write_structure", "swa_d0_write_uclust"]
EXPORTS.extend(_D0_EXPORTS)


def _declare_d0(lib) -> None:
    if getattr(lib, "_d0_declared", False):
        return
    lib.swa_derep.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_d0_cluster.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.swa_derep_resident.argtypes = [C.c_void_p]
    lib.swa_d0_cluster_device.argtypes = [C.c_void_p, u64p]
    lib.swa_d0_cluster_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                         C.c_void_p, C.POINTER(C.c_uint32)]
    lib.swa_d0_cluster_resident.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.swa_d0_result_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                         C.c_void_p, C.POINTER(C.c_uint32)]
    lib.swa_d0_result_free.argtypes = [C.c_void_p]
    lib.swa_d0_result_free.restype = None
    lib.swa_d0_result_summary.argtypes = [C.c_void_p, u64p]
    lib.swa_d0_result_summary.restype = None
    lib.swa_d0_write_swarms.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int64, C.c_int64]
    for fn in (lib.swa_d0_write_seeds, lib.swa_d0_write_stats, lib.swa_d0_write_structure):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    lib.swa_d0_write_uclust.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int64]
    lib._d0_declared = True


def derep(ctx: "Context") -> np.ndarray:
    """swa_derep: per amplicon the smallest index with the identical sequence (GPU)."""
    _declare_d0(ctx.lib)
    out = np.zeros(ctx.n, dtype=np.uint32)
    ctx._check(ctx.lib.swa_derep(ctx.h, _ptr(out)))
    return out


class D0Clusters:
    """d = 0 clustering (src/derep.cc): from swa_derep's array on the host, or — from_device — from the tables the GPU makes
    of the resident array.  The writers work on either."""

    def __init__(self, hdb: HostDb, first_identical: np.ndarray):
        self.lib = load_library()
        _declare_d0(self.lib)
        self.hdb = hdb
        first_identical = np.ascontiguousarray(first_identical, dtype=np.uint32)
        h = C.c_void_p()
        rc = self.lib.swa_d0_cluster(hdb.h, _ptr(first_identical), C.byref(h))
        if rc != SWA_OK:
            raise SwaError(rc, "swa_d0_cluster failed")
        self.h = h

    @classmethod
    def from_device(cls, ctx: "Context", hdb: HostDb) -> "D0Clusters":
        """swa_d0_cluster_resident: ctx.derep_resident() has run on hdb's database; the clusters are made on the GPU."""
        self = cls.__new__(cls)
        self.lib = ctx.lib
        _declare_d0(self.lib)
        self.hdb = hdb
        h = C.c_void_p()
        ctx._check(self.lib.swa_d0_cluster_resident(ctx.h, hdb.h, C.byref(h)))
        self.h = h
        return self

    def tables(self) -> dict:
        """swa_d0_result_tables: seed, mass, size, singletons, begin of every cluster in output order, members[n], and the
        summary — the same keys as Context.d0_cluster_device."""
        nc = C.c_uint32(0)
        assert self.lib.swa_d0_result_tables(self.h, None, None, None, None, None, 0, None, C.byref(nc)) == SWA_OK
        c = int(nc.value)
        u32 = {k: np.zeros(c, dtype=np.uint32) for k in ("seed", "size", "singletons", "begin")}
        mass = np.zeros(c, dtype=np.uint64)
        members = np.zeros(self.hdb.n, dtype=np.uint32)
        assert self.lib.swa_d0_result_tables(self.h, _ptr(u32["seed"]), _ptr(mass), _ptr(u32["size"]), _ptr(u32["singletons"]),
                                             _ptr(u32["begin"]), c, _ptr(members), C.byref(nc)) == SWA_OK
        out = dict(u32, mass=mass, members=members)
        out.update(self.summary())
        return out

    def summary(self) -> dict:
        out = np.zeros(3, dtype=np.uint64)
        self.lib.swa_d0_result_summary(self.h, _p64(out))
        return {"swarms": int(out[0]), "largest": int(out[1]), "heaviest": int(out[2])}

    def write_swarms(self, path, mothur=False, usearch=False, append_abundance=0) -> None:
        assert self.lib.swa_d0_write_swarms(self.h, self.hdb.h, str(path).encode(), int(mothur), int(usearch),
                                            append_abundance, 0) == SWA_OK

    def write_seeds(self, path, usearch=False) -> None:
        assert self.lib.swa_d0_write_seeds(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_stats(self, path, usearch=False) -> None:
        assert self.lib.swa_d0_write_stats(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_structure(self, path, usearch=False) -> None:
        assert self.lib.swa_d0_write_structure(self.h, self.hdb.h, str(path).encode(), int(usearch)) == SWA_OK

    def write_uclust(self, path, usearch=False, append_abundance=0) -> None:
        assert self.lib.swa_d0_write_uclust(self.h, self.hdb.h, str(path).encode(), int(usearch),
                                            append_abundance) == SWA_OK

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.swa_d0_result_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def d1_write_uclust(clusters: "D1Clusters", path, usearch=False, append_abundance=0, penalties=None,
                    ctx: "Context | MultiContext | None" = None) -> None:
    """-u for d = 1; with ctx= the alignments run on that context's GPU (seam B5, swa_d1_write_uclust_gpu), or divided
    among the ranks of a MultiContext (swa_d1_write_uclust_multi)."""
    lib = load_library()
    _declare_dn(lib)
    mm, go, ge = penalties or reduced_penalties()
    if isinstance(ctx, MultiContext):
        ctx._check(lib.swa_d1_write_uclust_multi(ctx.h, clusters.h, clusters.hdb.h, str(path).encode(), int(usearch),
                                                 append_abundance, mm, go, ge))
        return
    if ctx is not None:
        ctx._check(lib.swa_d1_write_uclust_gpu(ctx.h, clusters.h, clusters.hdb.h, str(path).encode(), int(usearch),
                                               append_abundance, mm, go, ge))
        return
    assert lib.swa_d1_write_uclust(clusters.h, clusters.hdb.h, str(path).encode(), int(usearch), append_abundance,
                                   mm, go, ge) == SWA_OK


def nw_align_host(dseq: np.ndarray, dlen: int, qseq: np.ndarray, qlen: int, mismatch: int = 18, gapopen: int = 24,
                  gapextend: int = 13):
    """The host's uclust aligner (swa_nw_align_host): (diffs, columns, CIGAR) of member dseq against seed qseq,
    both 2-bit packed u64 words."""
    lib = load_library()
    _declare_dn(lib)
    dseq = np.ascontiguousarray(dseq, dtype=np.uint64)
    qseq = np.ascontiguousarray(qseq, dtype=np.uint64)
    cols = C.c_uint64(0)
    clen = C.c_uint64(0)
    cap = int(dlen) + int(qlen) + 1
    buf = C.create_string_buffer(cap)
    diffs = lib.swa_nw_align_host(_ptr(dseq), int(dlen), _ptr(qseq), int(qlen), mismatch, gapopen, gapextend,
                                  C.byref(cols), buf, cap, C.byref(clen))
    return int(diffs), int(cols.value), buf.value[:clen.value].decode()


# ---- d = 1 on several GPUs from one process (multi.hip) -----------------------------------------

MULTI_BUILD_NONE, MULTI_BUILD_ROUTED, MULTI_BUILD_STREAMED, MULTI_BUILD_OVERFLOWED = range(4)
MULTI_BUILD_NAMES = ("none", "routed records", "streamed on request", "streamed after overflow")


_MULTI_SCAN_EXPORTS = ["swa_scan_set_ownership", "swa_scan_owner_for", "swa_scan_share_for", "swa_multi_scan_begin", "swa_multi_scan_batch",
                       "swa_multi_scan_step", "swa_multi_scan_fetch", "swa_multi_scan_totals", "swa_dn_result_scan_ranks"]
EXPORTS.extend(_MULTI_SCAN_EXPORTS)


def _declare_multi_scan(lib) -> None:
    lib.swa_scan_set_ownership.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
    lib.swa_scan_owner_for.argtypes = [C.c_uint32, C.c_uint32]
    lib.swa_scan_owner_for.restype = C.c_uint32
    lib.swa_scan_share_for.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, u32p]
    lib.swa_multi_dn_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
    lib.swa_multi_scan_begin.argtypes = [C.c_void_p]
    lib.swa_multi_scan_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_uint32, u32p]
    lib.swa_multi_scan_step.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_uint32, u32p]
    lib.swa_multi_scan_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.swa_multi_scan_totals.argtypes = [C.c_void_p, u64p]
    lib.swa_dn_result_scan_ranks.argtypes = [C.c_void_p]
    lib.swa_dn_result_scan_ranks.restype = C.c_uint32
    lib.swa_dn_cluster_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.POINTER(C.c_void_p)]


def scan_owner_for(id: int, world: int) -> int:
    """swa_scan_owner_for: the rank of `world` that scans amplicon `id` in MultiContext.scan_batch — (id >> 5) % world,
    block-cyclic in blocks of 32; a pure function, needs no device."""
    lib = load_library()
    _declare_multi_scan(lib)
    return int(lib.swa_scan_owner_for(int(id), int(world)))


def scan_share_for(n: int, lowest_unswarmed: int, rank: int, world: int):
    """swa_scan_share_for: (how many amplicons of [lowest_unswarmed, n) `rank` of `world` owns, the first of them — n when
    there is none); a pure function, needs no device."""
    lib = load_library()
    _declare_multi_scan(lib)
    out = np.zeros(2, dtype=np.uint32)
    rc = lib.swa_scan_share_for(int(n), int(lowest_unswarmed), int(rank), int(world), out.ctypes.data_as(u32p))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_scan_share_for: bad argument")
    return int(out[0]), int(out[1])


_MULTI_NW_EXPORTS = ["swa_multi_nw_batch", "swa_multi_nw_batch_totals", "swa_multi_nw_batch_tiers", "swa_multi_nw_batch_text_full",
                     "swa_multi_nw_bounds_for", "swa_d1_write_uclust_multi", "swa_dn_write_uclust_multi"]
EXPORTS.extend(_MULTI_NW_EXPORTS)


def _declare_multi_nw(lib) -> None:
    lib.swa_multi_nw_batch.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
    lib.swa_multi_nw_batch_totals.argtypes = [C.c_void_p, u64p]
    lib.swa_multi_nw_batch_tiers.argtypes = [C.c_void_p, u64p]
    lib.swa_multi_nw_batch_text_full.argtypes = [C.c_void_p, u64p]
    lib.swa_multi_nw_bounds_for.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.swa_dn_write_uclust_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int64]
    lib.swa_d1_write_uclust_multi.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_uint64,
                                              C.c_uint64, C.c_uint64]


def nw_bounds_for(d_ids, q_ids, seqlen, world: int) -> np.ndarray:
    """swa_multi_nw_bounds_for: how MultiContext.nw_batch divides a batch — rank r of `world` aligns the pairs
    [bounds[r], bounds[r + 1]), cut where the running sum of seqlen[d] + seqlen[q] passes r / world of the whole; a pure
    function, needs no device.  world + 1 entries (uint64)."""
    lib = load_library()
    _declare_multi_nw(lib)
    d_ids = np.ascontiguousarray(d_ids, dtype=np.uint32)
    q_ids = np.ascontiguousarray(q_ids, dtype=np.uint32)
    seqlen = np.ascontiguousarray(seqlen, dtype=np.uint32)
    assert len(d_ids) == len(q_ids)
    world = int(world)
    bounds = np.zeros(max(world, 0) + 1, dtype=np.uint64)
    rc = lib.swa_multi_nw_bounds_for(len(d_ids), _ptr(d_ids), _ptr(q_ids), _ptr(seqlen), len(seqlen), world & 0xFFFFFFFF, _ptr(bounds))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_multi_nw_bounds_for: bad argument")
    return bounds


_MULTI_DEREP_EXPORTS = ["swa_multi_derep_resident", "swa_multi_derep", "swa_multi_derep_owner_for", "swa_multi_derep_totals"]
EXPORTS.extend(_MULTI_DEREP_EXPORTS)


def _declare_multi_derep(lib) -> None:
    lib.swa_multi_derep_resident.argtypes = [C.c_void_p]
    lib.swa_multi_derep.argtypes = [C.c_void_p, C.c_void_p]
    lib.swa_multi_derep_owner_for.argtypes = [C.c_uint64, C.c_uint32, u32p]
    lib.swa_multi_derep_totals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]


def derep_owner_for(hash: int, world: int) -> int:
    """swa_multi_derep_owner_for: the rank (of world, 1 .. 64) that dereplicates every read whose Zobrist hash is `hash` in
    MultiContext.derep — a pure function of the full 64-bit hash; needs no device."""
    lib = load_library()
    _declare_multi_derep(lib)
    owner = C.c_uint32(0)
    rc = lib.swa_multi_derep_owner_for(int(hash) & 0xFFFFFFFFFFFFFFFF, int(world), C.byref(owner))
    if rc != SWA_OK:
        raise SwaError(rc, "swa_multi_derep_owner_for: bad argument")
    return int(owner.value)


class MultiContext:
    """swa_multi_*: one context + stream + host thread per listed device inside the library; RCCL for the exchange
    when the devices are distinct, device-to-device copies when a device is listed twice."""

    def __init__(self, devices):
        self.lib = load_library()
        lib = self.lib
        lib.swa_multi_create.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]
        lib.swa_multi_destroy.argtypes = [C.c_void_p]
        lib.swa_multi_destroy.restype = None
        lib.swa_multi_last_error.argtypes = [C.c_void_p]
        lib.swa_multi_last_error.restype = C.c_char_p
        lib.swa_multi_uses_rccl.argtypes = [C.c_void_p]
        lib.swa_multi_db_upload.argtypes = [C.c_void_p, C.POINTER(DbView)]
        lib.swa_multi_d1_network.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.POINTER(C.c_int)]
        lib.swa_multi_d1_fastidious.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.swa_multi_size.argtypes = [C.c_void_p]
        lib.swa_multi_ctx.argtypes = [C.c_void_p, C.c_int]
        lib.swa_multi_ctx.restype = C.c_void_p
        lib.swa_multi_d1_network_resident.argtypes = [C.c_void_p, C.c_int, u64p, C.POINTER(C.c_int)]
        lib.swa_multi_d1_fastidious_resident.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]
        lib.swa_multi_dn_graph_resident.argtypes = [C.c_void_p, C.c_int, u64p]
        lib.swa_multi_d1_last_build.argtypes = [C.c_void_p]
        _declare_multi_derep(lib)
        _declare_multi_scan(lib)
        _declare_multi_nw(lib)
        arr = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        rc = lib.swa_multi_create(arr, len(devices), C.byref(h))
        self.h = h
        if rc != SWA_OK:
            msg = lib.swa_multi_last_error(h).decode() if h else "allocation failed"
            self.close()
            raise SwaError(rc, msg)
        self.n = 0

    def _check(self, rc: int, allow=()) -> int:
        if rc != SWA_OK and rc not in allow:
            raise SwaError(rc, self.lib.swa_multi_last_error(self.h).decode())
        return rc

    def uses_rccl(self) -> bool:
        return bool(self.lib.swa_multi_uses_rccl(self.h))

    def upload_hostdb(self, hdb: "HostDb") -> None:
        v = DbView(hdb.n, hdb.longest, _ptr(hdb.seqs), _ptr(hdb.seq_off), _ptr(hdb.seqlen), _ptr(hdb.abundance))
        self._check(self.lib.swa_multi_db_upload(self.h, C.byref(v)))
        self.n = hdb.n

    def upload_db(self, seqs, seq_off, seqlen, abundance, longest: int) -> None:
        """Host numpy arrays (db order) -> every rank's HBM, as Context.upload_db."""
        n = int(seqlen.shape[0])
        v = DbView(n, int(longest), _ptr(seqs), _ptr(seq_off), _ptr(seqlen), _ptr(abundance))
        self._check(self.lib.swa_multi_db_upload(self.h, C.byref(v)))
        self.n = n

    def d1_network(self, no_cluster_breaking: bool = False):
        offsets = np.zeros(self.n + 1, dtype=np.uint64)
        cap = max(1024, 4 * self.n)
        total = C.c_uint64(0)
        dup = C.c_int(0)
        while True:
            nb = np.zeros(cap, dtype=np.uint32)
            rc = self._check(self.lib.swa_multi_d1_network(self.h, int(no_cluster_breaking), _ptr(offsets), _ptr(nb), cap,
                                                           C.byref(total), C.byref(dup)), allow=(SWA_E_CAPACITY,))
            if rc == SWA_OK:
                return offsets, nb[:total.value]
            cap = int(total.value)

    def dn_graph(self, d: int, no_cluster_breaking: bool = False, mismatch: int = 18, gapopen: int = 24, gapextend: int = 13):
        """swa_multi_dn_begin + swa_multi_dn_graph: (offsets, neighbours, diffs) of the whole d >= 2 graph, or None when the
        graph route does not serve the database: d > 16, or more candidate pairs with a sequence too short for d + 1
        windows than the brute-force part takes (16 n + 2^20; SWA_DN_BRUTE_CAP)."""
        lib = self.lib
        lib.swa_multi_dn_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
        lib.swa_multi_dn_graph_supported.argtypes = [C.c_void_p]
        lib.swa_multi_dn_graph.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
        self._check(lib.swa_multi_dn_begin(self.h, mismatch, gapopen, gapextend, d))
        if not lib.swa_multi_dn_graph_supported(self.h):
            return None
        offsets = np.zeros(self.n + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        rc = self._check(lib.swa_multi_dn_graph(self.h, int(no_cluster_breaking), _ptr(offsets), None, None, 0, C.byref(total)), allow=(SWA_E_CAPACITY,))
        nb = np.zeros(max(1, total.value), dtype=np.uint32)
        df = np.zeros(max(1, total.value), dtype=np.uint8)
        if rc == SWA_E_CAPACITY:
            self._check(lib.swa_multi_dn_graph(self.h, int(no_cluster_breaking), _ptr(offsets), _ptr(nb), _ptr(df), total.value, C.byref(total)))
        return offsets, nb[:total.value], df[:total.value]

    # ---- d = 0
    def derep_resident(self) -> None:
        """swa_multi_derep_resident: the identical-sequence search divided among the ranks, first_identical left in rank 0's
        HBM (ctx(0): d0_cluster_device, D0Clusters.from_device)."""
        self._check(self.lib.swa_multi_derep_resident(self.h))

    def derep(self) -> np.ndarray:
        """swa_multi_derep: derep_resident plus the download — per amplicon the smallest index with the identical sequence."""
        out = np.zeros(self.n, dtype=np.uint32)
        self._check(self.lib.swa_multi_derep(self.h, _ptr(out)))
        return out

    def derep_totals(self) -> dict:
        """swa_multi_derep_totals, of the last derep / derep_resident call: received (the records every owner got), rounds (of
        the owner that needed most), routed (records that travelled: n)."""
        received = np.zeros(self.lib.swa_multi_size(self.h), dtype=np.uint64)
        out2 = np.zeros(2, dtype=np.uint64)
        self._check(self.lib.swa_multi_derep_totals(self.h, _ptr(received), _ptr(out2)))
        return {"received": received, "rounds": int(out2[0]), "routed": int(out2[1])}

    # ---- d >= 2: the fused scan divided among the ranks by ownership of the pool (scan_owner_for)
    def size(self) -> int:
        return int(self.lib.swa_multi_size(self.h))

    def dn_begin(self, d: int, mismatch: int = 18, gapopen: int = 24, gapextend: int = 13) -> None:
        """swa_multi_dn_begin: q-gram signatures and the scoring for d on every rank"""
        self._check(self.lib.swa_multi_dn_begin(self.h, mismatch, gapopen, gapextend, d))

    def scan_begin(self) -> None:
        """swa_multi_scan_begin (after dn_begin): ownership and swa_scan_begin on every rank"""
        self._check(self.lib.swa_multi_scan_begin(self.h))

    def scan_batch(self, seeds, radii, lowest_unswarmed: int, first_generation: bool, ncb: bool, cap: int | None = None):
        """swa_multi_scan_batch, as Context.scan_batch: (return code, nhits, seed indices, ids, diffs)"""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        radii = np.ascontiguousarray(radii, dtype=np.uint32)
        assert seeds.shape == radii.shape
        cap = self.n if cap is None else int(cap)
        sidx, ids, diffs = (np.zeros(max(1, cap), dtype=np.uint32) for _ in range(3))
        nh = C.c_uint32(0)
        rc = self.lib.swa_multi_scan_batch(self.h, seeds.shape[0], _ptr(seeds), _ptr(radii), int(lowest_unswarmed), int(first_generation),
                                           int(ncb), _ptr(sidx), _ptr(ids), _ptr(diffs), cap, C.byref(nh))
        k = min(int(nh.value), cap) if rc == SWA_OK else 0
        return rc, int(nh.value), sidx[:k], ids[:k], diffs[:k]

    def scan_fetch(self, nhits: int):
        """swa_multi_scan_fetch: the merged (seed indices, ids, diffs) of the most recent scan_batch"""
        sidx, ids, diffs = (np.zeros(max(1, int(nhits)), dtype=np.uint32) for _ in range(3))
        self._check(self.lib.swa_multi_scan_fetch(self.h, _ptr(sidx), _ptr(ids), _ptr(diffs), int(nhits)))
        return sidx[:nhits], ids[:nhits], diffs[:nhits]

    def scan_totals(self) -> dict:
        """swa_multi_scan_totals: comparisons and pairs summed over the ranks, launch sequences = batches"""
        out = np.zeros(3, dtype=np.uint64)
        self._check(self.lib.swa_multi_scan_totals(self.h, _p64(out)))
        return {"qgram_comparisons": int(out[0]), "aligned_pairs": int(out[1]), "launch_sequences": int(out[2])}

    # ---- seam B5: the -u alignments divided among the ranks (nw_bounds_for)
    def nw_batch(self, d_ids, q_ids, mismatch: int = 18, gapopen: int = 24, gapextend: int = 13):
        """swa_multi_nw_batch, as Context.nw_batch and with its results for any device list: (diffs, columns, list of CIGAR
        strings)."""
        return _nw_batch_call(self.lib.swa_multi_nw_batch, self, d_ids, q_ids, mismatch, gapopen, gapextend)

    def nw_batch_totals(self) -> list:
        """Context.nw_batch_totals of the last nw_batch, summed over the ranks"""
        out = np.zeros(4, dtype=np.uint64)
        self._check(self.lib.swa_multi_nw_batch_totals(self.h, _p64(out)))
        return [int(v) for v in out]

    def nw_batch_tiers(self) -> list:
        """Context.nw_batch_tiers of the last nw_batch, summed over the ranks (a rank's own: ctx(r).nw_batch_tiers())"""
        out = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.swa_multi_nw_batch_tiers(self.h, _p64(out)))
        return [int(v) for v in out]

    def nw_batch_text_full(self) -> int:
        """Context.nw_batch_text_full of the last nw_batch, summed over the ranks"""
        out = np.zeros(1, dtype=np.uint64)
        self._check(self.lib.swa_multi_nw_batch_text_full(self.h, _p64(out)))
        return int(out[0])

    def dn_cluster(self, hdb: "HostDb", differences: int, no_cluster_breaking: bool = False, penalties=None) -> "DnClusters":
        """swa_dn_cluster_multi on a database uploaded with upload_hostdb: a DnClusters whose route() names what served —
        ("graph", 0), ("scan", ranks) for the scan divided among the ranks, ("scan", 1) for rank 0 alone
        (SWARM_AMD_MULTI_SCAN=root)."""
        return DnClusters(self.ctx(0), hdb, differences, no_cluster_breaking, penalties, multi=self)

    def ctx(self, rank: int = 0) -> "Context":
        """swa_multi_ctx: rank's context as a Context that neither owns nor closes the handle (it lives as long as this
        MultiContext, which the view keeps alive)."""
        handle = self.lib.swa_multi_ctx(self.h, int(rank))
        if not handle:
            raise SwaError(SWA_E_ARG, f"swa_multi_ctx: no rank {rank}")
        return Context._view(handle, self.n, self)

    def d1_network_resident(self, no_cluster_breaking: bool = False) -> int:
        """swa_multi_d1_network_resident: the network of the whole database left resident on rank 0's GPU (ctx(0):
        d1_network_fetch, d1_cluster_device, ...); returns the number of links.  SwaError(SWA_E_DUPLICATES) as d1_network."""
        total = C.c_uint64(0)
        dup = C.c_int(0)
        self._check(self.lib.swa_multi_d1_network_resident(self.h, int(no_cluster_breaking), C.byref(total), C.byref(dup)))
        return int(total.value)

    def last_build(self) -> str:
        """swa_multi_d1_last_build: how the ranks got the members of their anchor groups in the last d1_network /
        d1_network_resident call: one of MULTI_BUILD_NAMES."""
        return MULTI_BUILD_NAMES[self.lib.swa_multi_d1_last_build(self.h)]

    def dn_graph_resident(self, d: int, no_cluster_breaking: bool = False, mismatch: int = 18, gapopen: int = 24, gapextend: int = 13):
        """swa_multi_dn_begin + swa_multi_dn_graph_resident: the whole d >= 2 graph left resident on rank 0's GPU (ctx(0):
        d1_cluster_device, dn_parent_diffs, dn_tables_device); the number of links, or None when the graph route does
        not serve the database (as dn_graph)."""
        lib = self.lib
        lib.swa_multi_dn_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]
        lib.swa_multi_dn_graph_supported.argtypes = [C.c_void_p]
        self._check(lib.swa_multi_dn_begin(self.h, mismatch, gapopen, gapextend, d))
        if not lib.swa_multi_dn_graph_supported(self.h):
            return None
        total = C.c_uint64(0)
        self._check(lib.swa_multi_dn_graph_resident(self.h, int(no_cluster_breaking), C.byref(total)))
        return int(total.value)

    def d1_fastidious_resident(self, light_nt: int, bloom_bits: int = 16, fetch: bool = True):
        """swa_multi_d1_fastidious_resident: the second pass on all ranks from the flags ctx(0).d1_light_flags_device left
        in rank 0's HBM.  (graft_cand or None when fetch is False: the combined candidates then stay on rank 0 for
        ctx(0).d1_graft_device(None), counters)."""
        graft = np.zeros(self.n, dtype=np.uint32) if fetch else None
        counters = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.swa_multi_d1_fastidious_resident(self.h, int(light_nt), int(bloom_bits), _ptr(graft), _ptr(counters)))
        return graft, counters

    def d1_fastidious(self, is_light: np.ndarray, light_nt: int, bloom_bits: int = 16):
        is_light = np.ascontiguousarray(is_light, dtype=np.uint8)
        graft = np.zeros(self.n, dtype=np.uint32)
        counters = np.zeros(8, dtype=np.uint64)
        self._check(self.lib.swa_multi_d1_fastidious(self.h, _ptr(is_light), int(light_nt), int(bloom_bits), _ptr(graft), _ptr(counters)))
        return graft, counters

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.swa_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
