// Wave-level helpers of the CSR clock kernels (csr_merge.hip, clock_ops.hip,
// read.hip, lwwreg.hip, clock_bincode.hip, ops_bincode.hip): the ds_bpermute
// cross-lane reads, the rank of an actor in a sorted run held in registers
// (<= 64 entries, one per lane) or in HBM, the flat walk over the op ranges of
// 64 objects, and over 64 counts with the owner mask of its bad entries. The
// readlane reads (lane32 / lane64), the ballot prefix count (mbcnt) and fail
// are wave.h's, seen through namespace csr_rank.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave.h"

namespace crdts_hip {
namespace csr_rank {

using namespace wave;

__device__ __forceinline__ uint32_t rd32(uint32_t v, uint32_t src) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v);
}
__device__ __forceinline__ uint64_t rd64(uint64_t v, uint32_t src) {
  return ((uint64_t)rd32((uint32_t)(v >> 32), src) << 32) | rd32((uint32_t)v, src);
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

// The ops (or queries) of 64 objects, flat. Lane k holds object k's range
// [b, e) of a per-object grouped batch (b = the previous object's end), `valid`
// where the object exists and `good` where its range ascends inside the batch.
// Calls f(j, has, t) for every op j of the chunk: `has` says the lane holds op
// j, t is the lane that stands for j's object. Every lane makes every call (f
// may read across lanes). The ops of objects that are not good are skipped.
template <class F>
__device__ __forceinline__ void for_each_in_ranges(bool valid, bool good, uint64_t b, uint64_t e, uint32_t lane,
                                                   F f) {
  const uint64_t badm = __ballot(valid && !good);
  const uint32_t nv = (uint32_t)__popcll(__ballot(valid));  // the valid lanes are [0, nv), nv >= 1
  const uint64_t start = lane64(b, 0u), span = lane64(e, nv - 1u) - start;
  if (!badm && span < 0xffffffffull) {
    // the ends ascend: op j belongs to the object after the last end <= j
    const uint32_t T = (uint32_t)span;
    const uint32_t rel = valid ? (uint32_t)(e - start) : T;
    for (uint32_t base = 0; base < T; base += 64u) {
      const uint32_t jr = base + lane;
      const bool has = jr < T;
      const uint32_t t = rank_regs(rel, 64u, (has ? jr : 0u) + 1u);
      f(start + jr, has, t & 63u);
    }
  } else {
    uint64_t run = __ballot(valid && good && e > b);
    while (run) {
      const uint32_t t = (uint32_t)__builtin_ctzll(run);
      run &= run - 1u;
      const uint64_t bb = lane64(b, t), ee = lane64(e, t);
      for (uint64_t j0 = bb; j0 < ee; j0 += 64u) f(j0 + lane, j0 + lane < ee, t);
    }
  }
}

__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v, uint32_t lane) {
#pragma unroll
  for (uint32_t d = 1; d < kW; d <<= 1) {
    const uint64_t u = rd64(v, (lane - d) & 63u);
    if (lane >= d) v += u;
  }
  return v;
}

// Lane k stands for an object of n entries. Calls f(t, k, has) for every entry
// of the 64 objects, 64 entries a step: `has` says the lane holds an entry,
// which is entry k of lane t's object; the lane below holds entry k - 1 of the
// same object except in lane 0. Every lane makes every call. The sum of the 64
// counts must fit a u64.
template <class F>
__device__ __forceinline__ void flat_walk(uint64_t n, uint32_t lane, F f) {
  const uint64_t e = wave_incl_scan(n, lane), b = e - n;
  for_each_in_ranges(true, true, b, e, lane,
                     [&](uint64_t j, bool has, uint32_t t) { f(t, j - rd64(b, t), has); });
}

// bit t: some lane says `bad` of lane t's object
__device__ __forceinline__ uint64_t owners(bool bad, uint32_t t) {
  uint64_t m = __ballot(bad), r = 0;
  while (m) {
    const uint32_t l = (uint32_t)__builtin_ctzll(m);
    m &= m - 1u;
    r |= 1ull << lane32(t, l);
  }
  return r;
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
