// The bincode byte fields shared by the Orswot codec (bincode.hip) and the
// MVReg / Map codecs (map_bincode.hip) (internal): the blob reader over an LDS
// window or over HBM, the CLOCK ORDER comparison of two encoded clocks, and
// the byte-loop field writer. How a blob gets into the window stays with each
// codec (bc_prefetch, stage_blob), and the clock and LWWReg codecs keep their
// own readers: fixed-width, bounds-aware ones (clock_bincode.hip) and a
// runtime-width single aligned access (lwwreg.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace crdts_hip {
namespace blob {

// Blob bytes, read as little-endian unsigned integers of w bytes at a blob
// position (the caller has checked pos + w <= len). LDS window (S = true): b
// is the window's 16-B aligned base and the blob starts at b + d; a field is
// two aligned u64 reads and a funnel shift (the window has >= 16 spare bytes
// past the blob). Global (S = false, blobs too large for the window): byte
// loads.
template <bool S>
struct Src;
template <>
struct Src<true> {
  static constexpr bool kWindow = true;
  const uint8_t* b;
  uint32_t d;
  __device__ __forceinline__ uint64_t get(uint64_t pos, uint32_t w) const {
    const uint32_t a = d + (uint32_t)pos;
    const uint64_t* q = (const uint64_t*)(b + (a & ~7u));
    const uint32_t sh = 8u * (a & 7u);
    const uint64_t lo = q[0], hi = q[1];
    const uint64_t v = sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
    return w >= 8u ? v : v & ((1ull << (8u * w)) - 1u);
  }
  // the low 32 bits of the field at pos: two aligned u32 reads + v_alignbit
  __device__ __forceinline__ uint32_t lo32(uint32_t pos) const {
    const uint32_t a = d + pos;
    const uint32_t* q = (const uint32_t*)(b + (a & ~3u));
    return __builtin_amdgcn_alignbit(q[1], q[0], (a & 3u) * 8u);
  }
};
template <>
struct Src<false> {
  static constexpr bool kWindow = false;
  const uint8_t* b;
  __device__ __forceinline__ uint64_t get(uint64_t pos, uint32_t w) const {
    uint64_t v = 0;
    for (uint32_t i = 0; i < w; ++i) v |= (uint64_t)b[pos + i] << (8u * i);
    return v;
  }
};

// v as w little-endian bytes at p + pos (blobs are placed at any alignment)
__device__ __forceinline__ void wr(uint8_t* p, uint64_t pos, uint64_t v, uint32_t w) {
  for (uint32_t i = 0; i < w; ++i) p[pos + i] = (uint8_t)(v >> (8u * i));
}

// lexicographic (actor, counter) order of two bincode clocks, a proper prefix
// first (CLOCK ORDER): -1, 0, 1
template <class SRC>
__device__ __forceinline__ int clock_cmp(const SRC& B, uint64_t pa, uint32_t na, uint64_t pb, uint32_t nb,
                                         uint32_t wa) {
  const uint32_t n = na < nb ? na : nb;
  const uint64_t sa = wa + 8u;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t xa = B.get(pa + sa * i, wa), xb = B.get(pb + sa * i, wa);
    if (xa != xb) return xa < xb ? -1 : 1;
    const uint64_t ca = B.get(pa + sa * i + wa, 8), cb = B.get(pb + sa * i + wa, 8);
    if (ca != cb) return ca < cb ? -1 : 1;
  }
  return na == nb ? 0 : (na < nb ? -1 : 1);
}

}  // namespace blob
}  // namespace crdts_hip
