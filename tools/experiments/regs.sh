#!/bin/bash
# tools/experiments/regs.sh KERNEL_SUBSTRING [flags...] : VGPRs / scratch bytes / LDS of the kernels of a unit whose name contains the substring
# UNIT=d1 (default) | d1_part | fastidious: the unit —
#   d1.hip          index build and network step: k_seqhash, k_table_*, k_dup_check, k_db_lengths, k_anchor_*, k_sample_mass, k_abundance_rank*, k_lines_build,
#                   k_keys, k_guard_*, k_group1, k_group_lists, k_set_*, k_d1_group_pairs, k_d1_pairs_tiled, k_d1_probe<., 0 | 2>, k_stream_fallback
#   d1_part.hip     partition and rows: k_part_*, k_flat_*, k_csr_bucket*, k_seg_*, k_links_split, k_clear_many, k_scan_*
#   fastidious.hip  --fastidious: k_fast_*, k_fg_*, k_d1_flex, k_d1_probe<., 1>, k_join_*
cd "$(dirname "$0")/../../swarm_amd/csrc"
k=$1; shift
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 "$@" -x hip --cuda-device-only -S -o /tmp/regs_$$.s ${UNIT:-d1}.hip 2>/dev/null
awk -v k="$k" '/^[ \t]*\.amdhsa_kernel/ {name=$2; on = index(name, k) > 0} on && /amdhsa_private_segment_fixed_size|amdhsa_next_free_vgpr|amdhsa_group_segment_fixed_size/ {print name, $1, $2}' /tmp/regs_$$.s
rm -f /tmp/regs_$$.s
