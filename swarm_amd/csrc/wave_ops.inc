// wave_ops.inc — lane-to-lane helpers of the kernels, included inside each file's anonymous namespace (a file uses those
// it needs; the rest cost nothing).
// value of `v` in the neighbouring lane (full-wave DPP shifts, GFX9 family): a few cycles
// instead of an LDS-crossbar ds_bpermute on the critical path of every anti-diagonal step
__device__ __forceinline__ uint32_t from_lane_below(uint32_t v) {   // lane i <- lane i-1
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t from_lane_above(uint32_t v) {   // lane i <- lane i+1
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
}

// LDS written by some lanes of a wave, read by others of the same wave
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The same for a one-wave workgroup whose lanes also read global memory that other lanes of the wave wrote (nw_trace.hip:
// the wide tiers' direction bits).  Writer and reader run on one CU and share its write-through L1, so workgroup scope
// orders them; the wider scope makes the compiler wait for the global stores too, which the function above does not.
__device__ __forceinline__ void wave_mem_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
