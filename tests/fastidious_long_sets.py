"""Inputs and restated arithmetic for the tests of SWA_FAST_LONG=pairs and SWA_FAST_COUNT=sites (swarm_amd/csrc/d1_fast.inc:
k_fast_count_sites_words; fastidious.hip: fast_plan), on top of tests/fastidious_sets.py and tests/fastidious_split_sets.py.  Not
product code.

The sets are fastidious_split_sets' by name: "1005", "1025", "2049" = edit_atlas(L, L, small) alone —
  1005   the first length past k_fast_count's cap (records of 1001 .. 1005 nt),
  1025   33 words, records of 1021 .. 1025 nt: sequences on both sides of the 32-word boundary,
  2049   65 words: more words than lanes, so the kernel's strided loops take a second turn —
"long" and "three" as there, and edit_atlas(L) for the rows of k_fast_count.

k_fast_count_sites_words keeps two copies of words + 3 64-bit words a wave in LDS and nothing else."""
from __future__ import annotations

LONG_ATLASES = [1005, 1025, 2049]
LDS_BYTES = 160 * 1024


def sites_lds(longest: int, waves: int) -> int:
    return 8 * waves * 2 * ((longest + 31) // 32 + 3)


def sites_waves(longest: int) -> int:
    return next((w for w in (4, 2, 1) if sites_lds(longest, w) <= LDS_BYTES), 0)


SITES_CAP = 32 * (LDS_BYTES // 16 - 3)          # one wave: 16 (words + 3) <= 160 KB; 327 584 nt


def sites_plan(served: int, longest: int, pair_w: int = 0) -> list:
    """the plan vector under k_fast_count_sites_words: [1, pair kernel words, 1, waves, 0, LDS bytes, Zobrist table in LDS
    on the Bloom route (by the longest sequence of the database), 112]"""
    waves = sites_waves(served)
    return [1, pair_w, 1, waves, 0, sites_lds(served, waves), int(32 * (longest + 2) <= 96 * 1024), 112]
