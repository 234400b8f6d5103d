// LWWReg<u64, M>, batched (include/crdts_hip.h "LWWReg<u64, M>, batched"):
// merge, the op-list apply, the rank-order fold and the bincode codec, with
// their ABI functions.
//
// Reference: src/lwwreg.rs:27-32 (state: val, marker), :56-66 (merge: a larger
// marker replaces self; an equal marker with a different value is
// Err(ConflictingMarker) and leaves self; anything else is an Ok no-op),
// :69-77 (apply == merge), :104-118 (update == merge of LWWReg{val, marker}).
// One device function, lww_merge, serves all of them.
//
// State: val[n] u64, marker[n][MW] u64 (MW = 1 or 2 words, compared word 0
// first: Rust tuple Ord).
//   merge  a pure stream, 48 B per register at MW = 1. On 16-byte aligned
//          arrays a lane owns two consecutive registers (MW = 1: 16-B loads of
//          the val and marker pairs) or one register's marker row (MW = 2);
//          a wave covers an aligned run of 128 / 64 registers (two runs
//          per step at MW = 1: 8 loads in flight per lane, as the dense merge
//          has) and lane 0 stores the run's ballot words of the bitmap;
//          a wave adds its conflicts to the count once, after its last run.
//   fold   the same shape: replica r's registers for r = 0..R-1 through the
//          same function, four replicas' loads in flight; the replica
//          pointers travel in the kernel arguments.
//   apply  one kernel, a wave per 64 registers. Lists shorter than
//          CRDT_LWWREG_WAVE_MIN_OPS run in their lane, one op per step. The
//          longer ones are then taken one by one by the whole wave: 64 ops per
//          step, an inclusive scan of a (+) b = b.marker > a.marker ? b : a
//          (the leftmost arg-max, associative) over the lanes, shifted by one
//          and joined with the state carried from the chunks before: lane k
//          holds the state op k meets, so its Result is the closed form
//          marker == state.marker && val != state.val.
//   codec  a lane per blob, field by field: one access for a field whose
//          address is a multiple of its width, byte by byte otherwise (any
//          alignment, every byte touched once).
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "csr_rank.h"
#include "ctx.h"
#include "kernels.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace csr_rank;

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWaveMin = CRDT_LWWREG_WAVE_MIN_OPS;
constexpr uint32_t kMaxReps = CRDT_LWWREG_MAX_REPS;


bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// ------------------------------------------------------------------ the rule
template <int MW>
struct Reg {
  uint64_t v;
  uint64_t m[MW];
};

template <int MW>
__device__ __forceinline__ bool marker_gt(const Reg<MW>& a, const Reg<MW>& b) {  // a.marker > b.marker
  if (MW == 1) return a.m[0] > b.m[0];
  return a.m[0] > b.m[0] || (a.m[0] == b.m[0] && a.m[MW - 1] > b.m[MW - 1]);
}
template <int MW>
__device__ __forceinline__ bool marker_eq(const Reg<MW>& a, const Reg<MW>& b) {
  return a.m[0] == b.m[0] && a.m[MW - 1] == b.m[MW - 1];
}

// a (+) b: the leftmost of the two with the largest marker
template <int MW>
__device__ __forceinline__ Reg<MW> leftmost_max(const Reg<MW>& a, const Reg<MW>& b) {
  return marker_gt(b, a) ? b : a;
}

// s.merge(&o) (src/lwwreg.rs:56-66); true = Err(ConflictingMarker)
template <int MW>
__device__ __forceinline__ bool lww_merge(Reg<MW>& s, const Reg<MW>& o) {
  const bool conflict = marker_eq(o, s) && o.v != s.v;
  s = leftmost_max(s, o);
  return conflict;
}

// V16: the marker row of a 2-word register in one 16-byte access; NT: a
// streamed access (merge, fold)
template <int MW, bool V16, bool NT>
__device__ __forceinline__ Reg<MW> load_reg(const uint64_t* val, const uint64_t* marker, uint64_t i) {
  Reg<MW> r;
  r.v = NT ? __builtin_nontemporal_load(val + i) : val[i];
  if (MW == 1) {
    r.m[0] = NT ? __builtin_nontemporal_load(marker + i) : marker[i];
  } else if (V16) {
    const u64x2* p = (const u64x2*)marker + i;
    const u64x2 m = NT ? __builtin_nontemporal_load(p) : *p;
    r.m[0] = m.x;
    r.m[MW - 1] = m.y;
  } else {
    r.m[0] = marker[2u * i];
    r.m[MW - 1] = marker[2u * i + 1u];
  }
  return r;
}

template <int MW, bool V16, bool NT>
__device__ __forceinline__ void store_reg(uint64_t* val, uint64_t* marker, uint64_t i, const Reg<MW>& r) {
  if (NT) __builtin_nontemporal_store(r.v, val + i); else val[i] = r.v;
  if (MW == 1) {
    if (NT) __builtin_nontemporal_store(r.m[0], marker + i); else marker[i] = r.m[0];
  } else if (V16) {
    u64x2 m;
    m.x = r.m[0];
    m.y = r.m[MW - 1];
    if (NT) __builtin_nontemporal_store(m, (u64x2*)marker + i); else *((u64x2*)marker + i) = m;
  } else {
    marker[2u * i] = r.m[0];
    marker[2u * i + 1u] = r.m[MW - 1];
  }
}

// bit k of the low word of x -> bit 2k
__device__ __forceinline__ uint64_t spread32(uint64_t x) {
  x &= 0xffffffffull;
  x = (x | (x << 16)) & 0x0000ffff0000ffffull;
  x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
  x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x << 2)) & 0x3333333333333333ull;
  x = (x | (x << 1)) & 0x5555555555555555ull;
  return x;
}

// The two bitmap words of a run of 128 registers whose lane k owns registers
// 2k (ballot B0) and 2k + 1 (ballot B1), stored by lane 0.
__device__ __forceinline__ void store_pair_ballots(uint64_t* bitmap, uint64_t ch, uint64_t n_words, uint64_t B0,
                                                   uint64_t B1, uint32_t lane) {
  if (lane != 0u) return;
  bitmap[2u * ch] = spread32(B0) | (spread32(B1) << 1);
  if (2u * ch + 1u < n_words) bitmap[2u * ch + 1u] = spread32(B0 >> 32) | (spread32(B1 >> 32) << 1);
}

// ---------------------------------------------------------------------- merge
// MW = 1 on 16-byte aligned arrays: lane k of a run owns registers 2k, 2k + 1
__global__ __launch_bounds__(kBlock) void merge_pair_kernel(uint64_t* sval, uint64_t* smark, const uint64_t* oval,
                                                            const uint64_t* omark, uint64_t n, uint64_t* bitmap,
                                                            unsigned long long* count) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const uint64_t chunks = (n + 2u * kW - 1u) / (2u * kW), n_words = (n + 63u) / 64u;
  uint32_t mine = 0;  // this wave's conflicts
  for (uint64_t ch0 = wave; ch0 < chunks; ch0 += 2u * n_waves) {  // two runs per step: 8 loads in flight per lane
    u64x2 sv[2], sm[2], ov[2], om[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint64_t k = (ch0 + u * n_waves) * kW + lane;
      if (ch0 + u * n_waves < chunks && 2u * k + 1u < n) {
        sv[u] = __builtin_nontemporal_load((const u64x2*)sval + k);
        sm[u] = __builtin_nontemporal_load((const u64x2*)smark + k);
        ov[u] = __builtin_nontemporal_load((const u64x2*)oval + k);
        om[u] = __builtin_nontemporal_load((const u64x2*)omark + k);
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const uint64_t ch = ch0 + u * n_waves;
      if (ch >= chunks) break;  // wave-uniform
      const uint64_t k = ch * kW + lane, r0 = 2u * k;
      bool c0 = false, c1 = false;
      if (r0 + 1u < n) {
        Reg<1> a{sv[u].x, {sm[u].x}}, b{sv[u].y, {sm[u].y}};
        c0 = lww_merge(a, Reg<1>{ov[u].x, {om[u].x}});
        c1 = lww_merge(b, Reg<1>{ov[u].y, {om[u].y}});
        u64x2 wv, wm;
        wv.x = a.v; wv.y = b.v;
        wm.x = a.m[0]; wm.y = b.m[0];
        __builtin_nontemporal_store(wv, (u64x2*)sval + k);
        __builtin_nontemporal_store(wm, (u64x2*)smark + k);
      } else if (r0 < n) {  // the odd last register
        Reg<1> a = load_reg<1, false, true>(sval, smark, r0);
        c0 = lww_merge(a, load_reg<1, false, true>(oval, omark, r0));
        store_reg<1, false, true>(sval, smark, r0, a);
      }
      const uint64_t B0 = __ballot(c0), B1 = __ballot(c1);
      mine += (uint32_t)__popcll(B0) + (uint32_t)__popcll(B1);
      if (bitmap) store_pair_ballots(bitmap, ch, n_words, B0, B1, lane);
    }
  }
  if (count && mine && lane == 0u) atomicAdd(count, (unsigned long long)mine);
}

// a lane per register, a ballot word per run of 64
template <int MW, bool V16>
__global__ __launch_bounds__(kBlock) void merge_kernel(uint64_t* sval, uint64_t* smark, const uint64_t* oval,
                                                       const uint64_t* omark, uint64_t n, uint64_t* bitmap,
                                                       unsigned long long* count) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const uint64_t chunks = (n + kW - 1u) / kW;
  uint32_t mine = 0;
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    bool c = false;
    if (i < n) {
      Reg<MW> s = load_reg<MW, V16, true>(sval, smark, i);
      c = lww_merge(s, load_reg<MW, V16, true>(oval, omark, i));
      store_reg<MW, V16, true>(sval, smark, i, s);
    }
    const uint64_t B = __ballot(c);
    mine += (uint32_t)__popcll(B);
    if (bitmap && lane == 0u) bitmap[ch] = B;
  }
  if (count && mine && lane == 0u) atomicAdd(count, (unsigned long long)mine);
}

// ----------------------------------------------------------------------- fold
struct FoldReps {  // in the kernel arguments: 32 x 16 B
  const uint64_t* val[kMaxReps];
  const uint64_t* marker[kMaxReps];
};

// MW = 1 on 16-byte aligned arrays: lane k owns registers 2k, 2k + 1
__global__ __launch_bounds__(kBlock) void fold_pair_kernel(FoldReps P, uint32_t R, uint64_t n, uint64_t* oval,
                                                           uint64_t* omark, uint32_t* n_err) {
  const uint64_t pairs = (n + 1u) / 2u;
  for (uint64_t k = (uint64_t)blockIdx.x * kBlock + threadIdx.x; k < pairs; k += (uint64_t)gridDim.x * kBlock) {
    const uint64_t r0 = 2u * k;
    if (r0 + 1u < n) {
      const u64x2 v0 = __builtin_nontemporal_load((const u64x2*)P.val[0] + k);
      const u64x2 m0 = __builtin_nontemporal_load((const u64x2*)P.marker[0] + k);
      Reg<1> a{v0.x, {m0.x}}, b{v0.y, {m0.y}};
      uint32_t ea = 0, eb = 0;
#pragma unroll
      for (uint32_t g = 1; g < kMaxReps; g += 4u) {  // four replicas' loads in flight
        if (g >= R) break;
        u64x2 v[4], m[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u)
          if (g + u < R && g + u < kMaxReps) {
            v[u] = __builtin_nontemporal_load((const u64x2*)P.val[g + u] + k);
            m[u] = __builtin_nontemporal_load((const u64x2*)P.marker[g + u] + k);
          }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u)
          if (g + u < R && g + u < kMaxReps) {
            ea += lww_merge(a, Reg<1>{v[u].x, {m[u].x}}) ? 1u : 0u;
            eb += lww_merge(b, Reg<1>{v[u].y, {m[u].y}}) ? 1u : 0u;
          }
      }
      u64x2 wv, wm;
      wv.x = a.v; wv.y = b.v;
      wm.x = a.m[0]; wm.y = b.m[0];
      __builtin_nontemporal_store(wv, (u64x2*)oval + k);
      __builtin_nontemporal_store(wm, (u64x2*)omark + k);
      if (n_err) {
        n_err[r0] = ea;
        n_err[r0 + 1u] = eb;
      }
    } else {  // the odd last register
      Reg<1> a = load_reg<1, false, true>(P.val[0], P.marker[0], r0);
      uint32_t ea = 0;
#pragma unroll
      for (uint32_t r = 1; r < kMaxReps; ++r) {
        if (r >= R) break;
        ea += lww_merge(a, load_reg<1, false, true>(P.val[r], P.marker[r], r0)) ? 1u : 0u;
      }
      store_reg<1, false, true>(oval, omark, r0, a);
      if (n_err) n_err[r0] = ea;
    }
  }
}

template <int MW, bool V16>
__global__ __launch_bounds__(kBlock) void fold_kernel(FoldReps P, uint32_t R, uint64_t n, uint64_t* oval,
                                                      uint64_t* omark, uint32_t* n_err) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    Reg<MW> a = load_reg<MW, V16, true>(P.val[0], P.marker[0], i);
    uint32_t ea = 0;
#pragma unroll
    for (uint32_t g = 1; g < kMaxReps; g += 4u) {
      if (g >= R) break;
      Reg<MW> x[4];
#pragma unroll
      for (uint32_t u = 0; u < 4u; ++u)
        if (g + u < R && g + u < kMaxReps) x[u] = load_reg<MW, V16, true>(P.val[g + u], P.marker[g + u], i);
#pragma unroll
      for (uint32_t u = 0; u < 4u; ++u)
        if (g + u < R && g + u < kMaxReps) ea += lww_merge(a, x[u]) ? 1u : 0u;
    }
    store_reg<MW, V16, true>(oval, omark, i, a);
    if (n_err) n_err[i] = ea;
  }
}

// ---------------------------------------------------------------------- apply
template <int MW>
__device__ __forceinline__ Reg<MW> from_lane(const Reg<MW>& x, uint32_t src) {  // bpermute: every lane active
  Reg<MW> y;
  y.v = rd64(x.v, src);
  y.m[0] = rd64(x.m[0], src);
  if (MW > 1) y.m[MW - 1] = rd64(x.m[MW - 1], src);
  return y;
}
template <int MW>
__device__ __forceinline__ Reg<MW> of_lane(const Reg<MW>& x, uint32_t t) {  // readlane: t wave-uniform
  Reg<MW> y;
  y.v = lane64(x.v, t);
  y.m[0] = lane64(x.m[0], t);
  if (MW > 1) y.m[MW - 1] = lane64(x.m[MW - 1], t);
  return y;
}

template <int MW>
__global__ __launch_bounds__(kBlock) void apply_kernel(uint64_t* sval, uint64_t* smark, crdt_lwwreg_ops P,
                                                       uint64_t n_obj, uint32_t* n_err, uint8_t* op_err,
                                                       uint64_t chunks, int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    const bool valid = i < n_obj;
    uint64_t b = 0, e = 0;
    if (valid) {
      e = P.obj_end[i];
      b = i ? P.obj_end[i - 1u] : 0ull;
    }
    const bool good = valid && b <= e && e <= P.n_ops;
    if (__ballot(valid && !good) && lane == 0u) fail(status, CRDT_ENONCANON);
    const uint64_t len = good ? e - b : 0ull;
    Reg<MW> s{};
    if (len) s = load_reg<MW, false, false>(sval, smark, i);
    uint32_t errs = 0;
    // ---- short lists: one op per step in the register's own lane
    if (len < kWaveMin) {
      for (uint64_t j = b; j < b + len; ++j) {
        const bool c = lww_merge(s, load_reg<MW, false, false>(P.val, P.marker, j));
        errs += c ? 1u : 0u;
        if (op_err) op_err[j] = c ? 1 : 0;
      }
    }
    // ---- long lists: one register at a time, 64 ops per step over the wave
    uint64_t pend = __ballot(len >= kWaveMin);
    while (pend) {
      const uint32_t t = (uint32_t)__builtin_ctzll(pend);
      pend &= pend - 1u;
      const uint64_t bb = lane64(b, t), ee = lane64(e, t);
      Reg<MW> carry = of_lane(s, t);  // the state before the chunk's first op
      uint32_t ne = 0;
      for (uint64_t j0 = bb; j0 < ee; j0 += kW) {
        const uint64_t j = j0 + lane;
        const bool has = j < ee;
        // a lane past the list holds marker 0: on the right of (+) it never wins
        Reg<MW> x{};
        if (has) x = load_reg<MW, false, false>(P.val, P.marker, j);
        Reg<MW> inc = x;  // inclusive scan: inc[k] = x[0] (+) .. (+) x[k]
#pragma unroll
        for (uint32_t d = 1; d < kW; d <<= 1) {
          const Reg<MW> y = from_lane(inc, (lane - d) & 63u);
          if (lane >= d) inc = leftmost_max(y, inc);
        }
        const Reg<MW> prev = from_lane(inc, (lane - 1u) & 63u);
        const Reg<MW> st = lane ? leftmost_max(carry, prev) : carry;  // the state op j meets
        const bool c = has && marker_eq(x, st) && x.v != st.v;
        if (has && op_err) op_err[j] = c ? 1 : 0;
        ne += (uint32_t)__popcll(__ballot(c));
        carry = leftmost_max(carry, of_lane(inc, kW - 1u));
      }
      if (lane == t) {
        s = carry;
        errs = ne;
      }
    }
    if (len) store_reg<MW, false, false>(sval, smark, i, s);
    if (valid) n_err[i] = errs;
  }
}

// ---------------------------------------------------------------------- codec
// a field at an address that is a multiple of its width moves in one access,
// any other byte by byte
__device__ __forceinline__ uint64_t rd_le(const uint8_t* p, uint32_t w) {
  if (((uintptr_t)p & (w - 1u)) == 0u) {
    if (w == 8u) return *(const uint64_t*)p;
    if (w == 4u) return *(const uint32_t*)p;
    if (w == 2u) return *(const uint16_t*)p;
    return *p;
  }
  uint64_t v = 0;
  for (uint32_t k = 0; k < w; ++k) v |= (uint64_t)p[k] << (8u * k);
  return v;
}
__device__ __forceinline__ void wr_le(uint8_t* p, uint32_t w, uint64_t v) {
  if (((uintptr_t)p & (w - 1u)) == 0u) {
    if (w == 8u) *(uint64_t*)p = v;
    else if (w == 4u) *(uint32_t*)p = (uint32_t)v;
    else if (w == 2u) *(uint16_t*)p = (uint16_t)v;
    else *p = (uint8_t)v;
    return;
  }
  for (uint32_t k = 0; k < w; ++k) p[k] = (uint8_t)(v >> (8u * k));
}
__device__ __forceinline__ bool fits(uint64_t v, uint32_t w) { return w >= 8u || (v >> (8u * w)) == 0ull; }

template <int MW>
__global__ __launch_bounds__(kBlock) void from_bincode_kernel(const uint8_t* blobs, uint64_t stride, uint64_t n,
                                                              uint32_t vb, uint32_t mb0, uint32_t mb1, uint64_t* val,
                                                              uint64_t* marker) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint8_t* p = blobs + i * stride;
    Reg<MW> r;
    r.v = rd_le(p, vb);
    r.m[0] = rd_le(p + vb, mb0);
    if (MW > 1) r.m[MW - 1] = rd_le(p + vb + mb0, mb1);
    store_reg<MW, false, false>(val, marker, i, r);
  }
}

template <int MW>
__global__ __launch_bounds__(kBlock) void to_bincode_kernel(const uint64_t* val, const uint64_t* marker, uint64_t n,
                                                            uint32_t vb, uint32_t mb0, uint32_t mb1, uint8_t* blobs,
                                                            uint64_t stride, int* status) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const Reg<MW> r = load_reg<MW, false, false>(val, marker, i);
    if (!(fits(r.v, vb) && fits(r.m[0], mb0) && (MW == 1 || fits(r.m[MW - 1], mb1)))) {
      fail(status, CRDT_ENONCANON);  // the blob is not written
      continue;
    }
    uint8_t* p = blobs + i * stride;
    wr_le(p, vb, r.v);
    wr_le(p + vb, mb0, r.m[0]);
    if (MW > 1) wr_le(p + vb + mb0, mb1, r.m[MW - 1]);
  }
}

uint32_t wave_blocks(uint64_t chunks) { return resident_blocks((chunks + kBlock / kW - 1) / (kBlock / kW)); }
uint32_t lane_blocks(uint64_t items) { return resident_blocks((items + kBlock - 1) / kBlock); }

int launched() { return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP; }

}  // namespace

int launch_lwwreg_merge(uint64_t* sval, uint64_t* smark, const uint64_t* oval, const uint64_t* omark, uint64_t n,
                        uint32_t marker_words, uint64_t* bitmap, uint64_t* count, hipStream_t stream) {
  if (n == 0) return CRDT_OK;
  if (count && hipMemsetAsync(count, 0, sizeof(uint64_t), stream) != hipSuccess) return CRDT_EHIP;
  auto* cnt = (unsigned long long*)count;
  const bool a16 = aligned16(sval) && aligned16(smark) && aligned16(oval) && aligned16(omark);
  const dim3 block(kBlock);
  if (marker_words == 1 && a16) {
    const dim3 grid(wave_blocks((n + 2u * kW - 1u) / (2u * kW)));
    hipLaunchKernelGGL(merge_pair_kernel, grid, block, 0, stream, sval, smark, oval, omark, n, bitmap, cnt);
    return launched();
  }
  const dim3 grid(wave_blocks((n + kW - 1u) / kW));
  if (marker_words == 1)
    hipLaunchKernelGGL((merge_kernel<1, false>), grid, block, 0, stream, sval, smark, oval, omark, n, bitmap, cnt);
  else if (aligned16(smark) && aligned16(omark))
    hipLaunchKernelGGL((merge_kernel<2, true>), grid, block, 0, stream, sval, smark, oval, omark, n, bitmap, cnt);
  else
    hipLaunchKernelGGL((merge_kernel<2, false>), grid, block, 0, stream, sval, smark, oval, omark, n, bitmap, cnt);
  return launched();
}

int launch_lwwreg_apply(uint64_t* sval, uint64_t* smark, const crdt_lwwreg_ops& P, uint64_t n_obj,
                        uint32_t marker_words, uint32_t* n_err, uint8_t* op_err, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const uint64_t chunks = (n_obj + kW - 1u) / kW;
  const dim3 grid(wave_blocks(chunks)), block(kBlock);
  if (marker_words == 1)
    hipLaunchKernelGGL(apply_kernel<1>, grid, block, 0, stream, sval, smark, P, n_obj, n_err, op_err, chunks, status);
  else
    hipLaunchKernelGGL(apply_kernel<2>, grid, block, 0, stream, sval, smark, P, n_obj, n_err, op_err, chunks, status);
  return launched();
}

int launch_lwwreg_fold(const crdt_lwwreg_view* reps, uint32_t n_reps, uint64_t n, uint32_t marker_words,
                       uint64_t* oval, uint64_t* omark, uint32_t* n_err, hipStream_t stream) {
  if (n == 0) return CRDT_OK;
  FoldReps P{};
  bool a16 = aligned16(oval) && aligned16(omark), m16 = aligned16(omark);
  for (uint32_t r = 0; r < n_reps; ++r) {
    P.val[r] = reps[r].val;
    P.marker[r] = reps[r].marker;
    a16 = a16 && aligned16(reps[r].val) && aligned16(reps[r].marker);
    m16 = m16 && aligned16(reps[r].marker);
  }
  const dim3 block(kBlock);
  if (marker_words == 1 && a16) {
    hipLaunchKernelGGL(fold_pair_kernel, dim3(lane_blocks((n + 1u) / 2u)), block, 0, stream, P, n_reps, n, oval, omark,
                       n_err);
    return launched();
  }
  const dim3 grid(lane_blocks(n));
  if (marker_words == 1)
    hipLaunchKernelGGL((fold_kernel<1, false>), grid, block, 0, stream, P, n_reps, n, oval, omark, n_err);
  else if (m16)
    hipLaunchKernelGGL((fold_kernel<2, true>), grid, block, 0, stream, P, n_reps, n, oval, omark, n_err);
  else
    hipLaunchKernelGGL((fold_kernel<2, false>), grid, block, 0, stream, P, n_reps, n, oval, omark, n_err);
  return launched();
}

int launch_lwwreg_from_bincode(const uint8_t* blobs, uint64_t stride, uint64_t n, uint32_t vb, uint32_t marker_words,
                               uint32_t mb0, uint32_t mb1, uint64_t* val, uint64_t* marker, hipStream_t stream) {
  if (n == 0) return CRDT_OK;
  const dim3 grid(lane_blocks(n)), block(kBlock);
  if (marker_words == 1)
    hipLaunchKernelGGL(from_bincode_kernel<1>, grid, block, 0, stream, blobs, stride, n, vb, mb0, mb1, val, marker);
  else
    hipLaunchKernelGGL(from_bincode_kernel<2>, grid, block, 0, stream, blobs, stride, n, vb, mb0, mb1, val, marker);
  return launched();
}

int launch_lwwreg_to_bincode(const uint64_t* val, const uint64_t* marker, uint64_t n, uint32_t vb,
                             uint32_t marker_words, uint32_t mb0, uint32_t mb1, uint8_t* blobs, uint64_t stride,
                             int* status, hipStream_t stream) {
  if (n == 0) return CRDT_OK;
  const dim3 grid(lane_blocks(n)), block(kBlock);
  if (marker_words == 1)
    hipLaunchKernelGGL(to_bincode_kernel<1>, grid, block, 0, stream, val, marker, n, vb, mb0, mb1, blobs, stride,
                       status);
  else
    hipLaunchKernelGGL(to_bincode_kernel<2>, grid, block, 0, stream, val, marker, n, vb, mb0, mb1, blobs, stride,
                       status);
  return launched();
}

}  // namespace crdts_hip

// ------------------------------------------------------------------- the ABI
using namespace crdts_hip;

namespace {
inline hipStream_t S(void* s) { return (hipStream_t)s; }
int set_device(crdt_ctx* ctx) { return hipSetDevice(ctx->device) == hipSuccess ? CRDT_OK : CRDT_EHIP; }
bool words_ok(uint32_t marker_words) { return marker_words == 1u || marker_words == 2u; }
bool width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }
bool same(const void* a, const void* b) { return a && a == b; }
}  // namespace

extern "C" {

int crdt_lwwreg_merge(crdt_ctx* ctx, uint64_t* d_self_val, uint64_t* d_self_marker, const uint64_t* d_other_val,
                      const uint64_t* d_other_marker, size_t n, uint32_t marker_words, uint64_t* d_conflict,
                      uint64_t* d_n_conflict, void* stream) {
  if (!ctx || !words_ok(marker_words)) return CRDT_EINVAL;
  if (n && (!d_self_val || !d_self_marker || !d_other_val || !d_other_marker)) return CRDT_EINVAL;
  if (n && (d_self_val == d_other_val || d_self_marker == d_other_marker)) return CRDT_EINVAL;
  if (n == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_lwwreg_merge(d_self_val, d_self_marker, d_other_val, d_other_marker, n, marker_words, d_conflict,
                             d_n_conflict, S(stream));
}

int crdt_lwwreg_apply(crdt_ctx* ctx, uint64_t* d_self_val, uint64_t* d_self_marker, const crdt_lwwreg_ops* ops,
                      size_t n_obj, uint32_t marker_words, uint32_t* d_n_err, uint8_t* d_op_err, void* stream) {
  if (!ctx || !ops || !words_ok(marker_words)) return CRDT_EINVAL;
  if (n_obj && (!d_self_val || !d_self_marker || !d_n_err || !ops->obj_end)) return CRDT_EINVAL;
  if (ops->n_ops && (!ops->val || !ops->marker)) return CRDT_EINVAL;
  if (n_obj)
    for (const void* w : {(const void*)d_self_val, (const void*)d_self_marker})
      if (same(w, ops->obj_end) || same(w, ops->val) || same(w, ops->marker)) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_lwwreg_apply(d_self_val, d_self_marker, *ops, n_obj, marker_words, d_n_err, d_op_err, ctx->d_status,
                             S(stream));
}

int crdt_lwwreg_fold(crdt_ctx* ctx, const crdt_lwwreg_view* h_reps, uint32_t n_reps, size_t n, uint32_t marker_words,
                     uint64_t* d_out_val, uint64_t* d_out_marker, uint32_t* d_n_err, void* stream) {
  if (!ctx || !h_reps || n_reps == 0 || n_reps > CRDT_LWWREG_MAX_REPS || !words_ok(marker_words)) return CRDT_EINVAL;
  if (n && (!d_out_val || !d_out_marker)) return CRDT_EINVAL;
  for (uint32_t r = 0; n && r < n_reps; ++r) {
    if (!h_reps[r].val || !h_reps[r].marker) return CRDT_EINVAL;
    // in place on replica 0 only: a later replica is still to be read when
    // other lanes have written their output
    if (r && (h_reps[r].val == d_out_val || h_reps[r].marker == d_out_marker)) return CRDT_EINVAL;
  }
  if (n == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_lwwreg_fold(h_reps, n_reps, n, marker_words, d_out_val, d_out_marker, d_n_err, S(stream));
}

int crdt_lwwreg_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t stride, size_t n, uint32_t val_bytes,
                             uint32_t marker_words, uint32_t marker_bytes0, uint32_t marker_bytes1,
                             uint64_t* d_out_val, uint64_t* d_out_marker, void* stream) {
  if (!ctx || !words_ok(marker_words) || !width_ok(val_bytes) || !width_ok(marker_bytes0)) return CRDT_EINVAL;
  if (marker_words == 2u && !width_ok(marker_bytes1)) return CRDT_EINVAL;
  if (stride < (size_t)val_bytes + marker_bytes0 + (marker_words == 2u ? marker_bytes1 : 0u)) return CRDT_EINVAL;
  if (n && (!d_blobs || !d_out_val || !d_out_marker)) return CRDT_EINVAL;
  if (n && ((const void*)d_blobs == d_out_val || (const void*)d_blobs == d_out_marker || d_out_val == d_out_marker))
    return CRDT_EINVAL;
  if (n == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_lwwreg_from_bincode(d_blobs, stride, n, val_bytes, marker_words, marker_bytes0, marker_bytes1,
                                    d_out_val, d_out_marker, S(stream));
}

int crdt_lwwreg_to_bincode(crdt_ctx* ctx, const uint64_t* d_val, const uint64_t* d_marker, size_t n,
                           uint32_t val_bytes, uint32_t marker_words, uint32_t marker_bytes0, uint32_t marker_bytes1,
                           uint8_t* d_blobs, size_t stride, void* stream) {
  if (!ctx || !words_ok(marker_words) || !width_ok(val_bytes) || !width_ok(marker_bytes0)) return CRDT_EINVAL;
  if (marker_words == 2u && !width_ok(marker_bytes1)) return CRDT_EINVAL;
  if (stride < (size_t)val_bytes + marker_bytes0 + (marker_words == 2u ? marker_bytes1 : 0u)) return CRDT_EINVAL;
  if (n && (!d_blobs || !d_val || !d_marker)) return CRDT_EINVAL;
  if (n && ((const void*)d_blobs == d_val || (const void*)d_blobs == d_marker)) return CRDT_EINVAL;
  if (n == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_lwwreg_to_bincode(d_val, d_marker, n, val_bytes, marker_words, marker_bytes0, marker_bytes1, d_blobs,
                                  stride, ctx->d_status, S(stream));
}

}  // extern "C"
