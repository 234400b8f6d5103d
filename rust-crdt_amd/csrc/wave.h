// The wave toolkit (internal): the one definition of every wave-level
// primitive the kernels share — the wave fence, uniform and cross-lane reads,
// the ballot prefix count, the u32 inclusive scan, the wave-strided set probe
// and the first-error latch. A helper that only one kernel family uses, or a
// second algorithm for the same job (the DPP / bpermute / xor-shuffle sums and
// scans), stays in that family's file. The Orswot join (orswot_merge.hip,
// diag/) keeps its own copies.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace crdts_hip {
namespace wave {

constexpr uint32_t kW = 64;  // the wave width

// Hand-off between the lanes of one wave through memory: fence + barrier.
// Global: the memory is HBM scratch, whose stores must have landed first.
template <bool Global = false>
__device__ __forceinline__ void sync() {
  if constexpr (Global) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  } else {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

// a wave-uniform value, moved to scalar registers
__device__ __forceinline__ uint32_t uni32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | (uint64_t)uni32((uint32_t)v);
}
// lane l's value (l wave-uniform)
__device__ __forceinline__ uint32_t lane32(uint32_t v, uint32_t l) {
  return (uint32_t)__builtin_amdgcn_readlane(v, l);
}
__device__ __forceinline__ uint64_t lane64(uint64_t v, uint32_t l) {
  return ((uint64_t)lane32((uint32_t)(v >> 32), l) << 32) | (uint64_t)lane32((uint32_t)v, l);
}
// lane l's value (l may differ per lane)
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t l) {
  return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), (int)l, kW) << 32) |
         (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, (int)l, kW);
}
// set bits of m below this lane
__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// inclusive prefix sum over the wave
__device__ __forceinline__ uint32_t scan_incl(uint32_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < kW; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, kW);
    v += lane >= d ? t : 0u;
  }
  return v;
}
// is `key` among set[0, n)? The wave probes 64 elements per step.
__device__ __forceinline__ bool set_has(const uint64_t* set, uint32_t n, uint64_t key, uint32_t lane) {
  bool f = false;
  for (uint32_t j = lane; j < n; j += kW) f = f || set[j] == key;
  return __ballot(f) != 0ull;
}

// the first error of a launch wins
__device__ __forceinline__ void fail(int* status, int code) { atomicCAS(status, 0, code); }

}  // namespace wave
}  // namespace crdts_hip
