// The bincode byte fields shared by the Orswot codec (bincode.hip) and the
// MVReg / Map codecs (map_bincode.hip) (internal): the blob reader over an LDS
// window or over HBM, the CLOCK ORDER comparison of two encoded clocks, and
// the byte-loop field writer; and the bounds-aware field reader and piecewise
// writer of the codecs that leave their blobs in HBM (clock_bincode.hip,
// ops_bincode.hip). How a blob gets into the window stays with each codec
// (bc_prefetch, stage_blob), and the LWWReg codec keeps its own reader: a
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

// ------------------------------------------------------------------------
// Fields of blobs that stay in HBM, at any alignment (the clock codec and the
// op-stream codec: a lane per field, no window).
// [lo, hi): the bytes that may be read (d_blobs)
struct Bounds {
  uintptr_t lo, hi;
};

// A field of W bytes, read as the one or two aligned 8-byte words that hold
// it where those lie inside the bounds, else byte by byte.
template <uint32_t W>
__device__ __forceinline__ uint64_t rd_le(const uint8_t* p, const Bounds& s) {
  const uint32_t r = (uint32_t)((uintptr_t)p & 7u);
  const uintptr_t w0 = (uintptr_t)p - r;
  const bool two = r + W > 8u;
  if (w0 >= s.lo && w0 + (two ? 16u : 8u) <= s.hi) {
    uint64_t v = *(const uint64_t*)w0 >> (8u * r);
    if (two) v |= *(const uint64_t*)(w0 + 8u) << (64u - 8u * r);  // two: r > 0
    return W == 8u ? v : v & ((1ull << (8u * (W & 7u))) - 1ull);
  }
  uint64_t v = 0;
  for (uint32_t k = 0; k < W; ++k) v |= (uint64_t)p[k] << (8u * k);
  return v;
}

// A field stored in aligned pieces, without a loop: up to the next 8-byte
// boundary in rising sizes (1, 2, 4), past it in falling sizes (4, 2, 1).
template <uint32_t W>
__device__ __forceinline__ void wr_le(uint8_t* p, uint64_t v) {
  const uint32_t r = (uint32_t)((uintptr_t)p & 7u);
  if (W == 1u) {
    *p = (uint8_t)v;
  } else if (W == 2u) {
    if (r & 1u) {
      p[0] = (uint8_t)v;
      p[1] = (uint8_t)(v >> 8);
    } else {
      *(uint16_t*)p = (uint16_t)v;
    }
  } else if (W == 4u) {
    if ((r & 3u) == 0u) {
      *(uint32_t*)p = (uint32_t)v;
    } else if ((r & 1u) == 0u) {
      *(uint16_t*)p = (uint16_t)v;
      *(uint16_t*)(p + 2) = (uint16_t)(v >> 16);
    } else {
      p[0] = (uint8_t)v;
      *(uint16_t*)(p + 1) = (uint16_t)(v >> 8);
      p[3] = (uint8_t)(v >> 24);
    }
  } else {
    if (r == 0u) {
      *(uint64_t*)p = v;
      return;
    }
    const uint32_t h = 8u - r;  // bytes up to the boundary
    if (h & 1u) { *p = (uint8_t)v; p += 1; v >>= 8; }
    if (h & 2u) { *(uint16_t*)p = (uint16_t)v; p += 2; v >>= 16; }
    if (h & 4u) { *(uint32_t*)p = (uint32_t)v; p += 4; v >>= 32; }
    if (r & 4u) { *(uint32_t*)p = (uint32_t)v; p += 4; v >>= 32; }
    if (r & 2u) { *(uint16_t*)p = (uint16_t)v; p += 2; v >>= 16; }
    if (r & 1u) *p = (uint8_t)v;
  }
}

template <uint32_t AB>
__device__ __forceinline__ bool fits(uint64_t v) {
  return AB >= 8u || (v >> (8u * (AB & 7u))) == 0ull;
}

// The same three for a width w in {1, 2, 4, 8} that is only known at run time
// (wave-uniform: the switch is a scalar branch).
__device__ __forceinline__ uint64_t rd_le(const uint8_t* p, uint32_t w, const Bounds& s) {
  switch (w) {
    case 1u: return rd_le<1>(p, s);
    case 2u: return rd_le<2>(p, s);
    case 4u: return rd_le<4>(p, s);
    default: return rd_le<8>(p, s);
  }
}
__device__ __forceinline__ void wr_le(uint8_t* p, uint32_t w, uint64_t v) {
  switch (w) {
    case 1u: wr_le<1>(p, v); break;
    case 2u: wr_le<2>(p, v); break;
    case 4u: wr_le<4>(p, v); break;
    default: wr_le<8>(p, v); break;
  }
}
__device__ __forceinline__ bool fits(uint64_t v, uint32_t w) { return w >= 8u || (v >> (8u * w)) == 0ull; }

}  // namespace blob
}  // namespace crdts_hip
