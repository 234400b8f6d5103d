// Wave-level helpers of the CSR clock kernels (csr_merge.hip, clock_ops.hip):
// cross-lane reads, the ballot prefix count, and the rank of an actor in a
// sorted run held in registers (<= 64 entries, one per lane) or in HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crdts_hip {
namespace csr_rank {

__device__ __forceinline__ uint32_t rd32(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
}
__device__ __forceinline__ uint64_t rd64(uint64_t v, uint32_t src) {
  return ((uint64_t)rd32((uint32_t)(v >> 32), src) << 32) | rd32((uint32_t)v, src);
}
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, uint32_t l) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l);
}
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, uint32_t l) {
  return ((uint64_t)lane_u32((uint32_t)(v >> 32), l) << 32) | lane_u32((uint32_t)v, l);
}
__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// lane k's value moved to lane k + 1 (lane 0 gets 0): DPP wave_shr:1
__device__ __forceinline__ uint32_t from_below(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xf, 0xf, false);
}

// # of the first n actors held by lanes [0, n) of `a` that are < x
// (n <= 64; lanes past n are never probed): 6-step binary lifting.
__device__ __forceinline__ uint32_t rank_regs(uint32_t a, uint32_t n, uint32_t x) {
  uint32_t b = 0;
#pragma unroll
  for (uint32_t step = 32u; step; step >>= 1) {
    const uint32_t c = b + step;  // candidate count: probe element c - 1
    const uint32_t p = rd32(a, (c - 1u) & 63u);
    b = (c <= n && p < x) ? c : b;
  }
  const uint32_t c = b + 1u;  // the last step (element b) as one more probe
  const uint32_t p = rd32(a, b & 63u);
  return (c <= n && p < x) ? c : b;
}

// # of entries of the sorted run a[0, n) (in HBM) below x.
__device__ __forceinline__ uint64_t rank_mem(const uint32_t* a, uint64_t n, uint32_t x) {
  uint64_t lo = 0, len = n;
  while (len) {
    const uint64_t half = len >> 1;
    if (a[lo + half] < x) {
      lo += half + 1u;
      len -= half + 1u;
    } else {
      len = half;
    }
  }
  return lo;
}

}  // namespace csr_rank
}  // namespace crdts_hip
