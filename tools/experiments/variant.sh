#!/bin/bash
# tools/experiments/variant.sh NAME "-DX=1 ..." : libswarm_amd_NAME.so = this tree with one unit compiled under extra flags
# UNIT=d1 (default: index build and network step) | d1_part (partition and rows: k_part_*, k_flat_*, k_csr_bucket*, k_seg_*, k_links_split) |
# fastidious (the --fastidious pass); tools/experiments/regs.sh lists every kernel's unit
# (A/B of kernel variants on one lease: SWARM_AMD_LIB=swarm_amd/lib/libswarm_amd_NAME.so python bench.py ...)
set -e
cd "$(dirname "$0")/../../swarm_amd/csrc"
name=$1; shift
unit=${UNIT:-d1}
make -s -j 16 all
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wextra -Wno-unused-parameter "$@" -x hip -c -o build/variant_${unit}_$name.o $unit.hip
objs=$(ls build/*.o | grep -v "^build/$unit.o$" | grep -v "^build/variant_" | grep -v "^build/asan_")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../lib/libswarm_amd_$name.so $objs build/variant_${unit}_$name.o \
  -L$(dirname $(g++ -print-file-name=libgomp.so)) -lgomp -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
echo built ../lib/libswarm_amd_$name.so
