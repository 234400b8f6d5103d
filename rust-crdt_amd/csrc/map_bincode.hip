// Ingest / egest codec between the reference's binary form of an MVReg<V, A>
// and of a Map<K, MVReg<V, A>, A> and the dense slabs of crdt_mvreg_merge /
// crdt_map_mvreg_merge (include/crdts_hip.h). SURVEY.md §8(f) rank 1, after
// bincode.hip (the Orswot codec).
// Further down: the same for the two Map types whose values are containers,
// Map<K, Orswot<M, A>, A> and Map<K, Map<K2, MVReg<V, A>, A>, A>, over
// crdt_map_orswot_slab / crdt_map_map_slab with the helpers of this file.
//
// The reference form is `to_binary(&x)` = bincode 0.9 of the serde derives
// (src/lib.rs:62-83; MVReg src/mvreg.rs:42-46, Map src/map.rs:81-99, Entry
// src/map.rs:69-77, VClock src/vclock.rs:54-57): fields in order, Vec / map /
// set as a u64 length + elements, fixed-width little-endian integers:
//
//   VClock   u64 n | n x (A actor | u64 counter)          actors ascending
//   MVReg    u64 n_vals | n_vals x (VClock | V val)       Vec order
//   Map      VClock clock
//            u64 n_entries | n_entries x (K key | VClock clock | MVReg val)
//            u64 n_def | n_def x (VClock | u64 n | n x K) clocks in any order
//
// One wave per object, grid-stride. A blob that fits the wave's LDS window is
// staged there by aligned 16-B loads of the covering span and indexed with
// its misalignment; a longer one is walked from HBM byte by byte. The walk
// over the length words is wave-uniform (an inherently serial chain: every
// word is checked against the bytes left before anything it sizes is read);
// what a length word sizes is lane-parallel: a clock's pairs are scattered
// into a dense row, a deferred set's keys copied, the deferred clocks ranked
// by comparison count (<= 64 of them) into CLOCK ORDER. Egest sizes the keys
// of a map (the values of a register) one per lane, places them by a wave
// prefix sum and writes every clock's pairs lane-parallel, byte stores only
// (blobs are placed at any alignment).
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "blob.h"
#include "kernels.h"
#include "map_limits.h"
#include "sched.h"
#include "wave.h"

namespace crdts_hip {
namespace {

typedef uint32_t v4u __attribute__((ext_vector_type(4)));

using namespace blob;  // Src, clock_cmp, wr (blob.h)
using namespace wave;  // kW, sync, uni32 / uni64, scan_incl (wave.h)

constexpr uint32_t kWaves = 4;       // waves per block
constexpr uint32_t kStage = 4096;    // LDS window per wave: blobs of <= kStage - 32 bytes
constexpr uint32_t kRowMax = kMapActorsMax;  // dense rows up to this many actors are built in LDS
constexpr uint32_t kDefMax = kMapMvregDcap;  // deferred clocks per map (Map<u64, MVReg>, the nested map's two levels)
constexpr uint32_t kNestMax = kMapOrswotMcap;  // members / deferred clocks per nested set or map (Map<u64, Orswot>)
static_assert(kMapMapDcap <= kDefMax, "one table holds an outer map's deferred clocks");
static_assert(kMapOrswotVdcap <= kNestMax && kMapOrswotDcap <= kNestMax, "one table holds either deferred list");

// One wave's LDS: the blob window, the dense row under construction (all zero
// between two clocks) and the deferred clocks' positions, sizes and ranks.
// N: the deferred clocks (Map<u64, Orswot>: or the members of a nested set,
// Pd / Ld its member clock, Ps the member, Rd its rank) one table holds.
template <uint32_t N>
struct alignas(16) WaveLdsT {
  static constexpr uint32_t kDef = N;
  v4u stage[kStage / 16];
  uint64_t row[kRowMax];
  uint64_t Pd[N];  // first pair of deferred clock d
  uint64_t Ps[N];  // first key of its set
  uint32_t Ld[N];  // its pairs
  uint32_t Ls[N];  // its keys
  uint32_t Rd[N];  // its rank in CLOCK ORDER
};
typedef WaveLdsT<kDefMax> WaveLds;
typedef WaveLdsT<kNestMax> NestLds;

struct Widths {
  uint32_t wa, wk, wv;  // actor, key, value bytes
};

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
  for (uint32_t d = 32; d >= 1; d >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, d, kW), hi = __shfl_xor((uint32_t)(v >> 32), d, kW);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ bool fits(uint64_t x, uint32_t w) { return w >= 8u || x < (1ull << (8u * w)); }

// The aligned 16-B lines covering blob [off, off + len) of the buffer, into
// the window; returns the blob's misalignment. A line that reaches outside
// the buffer (before its first byte: an unaligned buffer; past its last) is
// gathered byte by byte from the bytes inside. len + 32 <= kStage.
__device__ __forceinline__ uint32_t stage_blob(v4u* st, const uint8_t* blobs, uint64_t blob_bytes, uint64_t off,
                                               uint64_t len, uint32_t lane) {
  const uintptr_t base = (uintptr_t)blobs, end = base + blob_bytes;
  const uintptr_t s = base + off, a0 = s & ~(uintptr_t)15;
  const uint32_t n16 = (uint32_t)((((s + len + 15u) & ~(uintptr_t)15) - a0) / 16u);
  for (uint32_t idx = lane; idx < n16; idx += kW) {
    const uintptr_t g = a0 + 16u * (uintptr_t)idx;
    if (g >= base && g + 16u <= end) {
      st[idx] = __builtin_nontemporal_load((const v4u*)g);
    } else {
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      for (uint32_t i = 0; i < 16u; ++i)
        if (g + i >= base && g + i < end) w[i / 4u] |= (uint32_t)*(const uint8_t*)(g + i) << (8u * (i & 3u));
      st[idx] = v4u{w[0], w[1], w[2], w[3]};
    }
  }
  return (uint32_t)(s & 15u);
}

// ------------------------------------------------------------------ the walk
// A length word at p whose elements take at least `unit` bytes each: checked
// against the bytes left before anything it sizes is read. p moves past it.
template <class SRC>
__device__ __forceinline__ bool take_len(const SRC& B, uint64_t& p, uint64_t len, uint32_t unit, uint64_t& n) {
  if (len - p < 8u) return false;
  n = uni64(B.get(p, 8));
  p += 8u;
  return n <= (len - p) / unit;
}
// A clock's length word at p: n <= A pairs (actors are strictly ascending and
// below A) that the bytes left can hold. p moves to the first pair.
template <class SRC>
__device__ __forceinline__ bool take_clock(const SRC& B, uint64_t& p, uint64_t len, uint32_t wa, uint32_t A,
                                           uint32_t& n) {
  uint64_t n64;
  if (!take_len(B, p, len, wa + 8u, n64) || n64 > A) return false;
  n = (uint32_t)n64;
  return true;
}

// The n pairs at p, scattered into the dense row dst[A] (0 = absent). Returns
// this lane's verdict: an actor >= A, a zero counter, actors not strictly
// ascending. Rows of <= kRowMax actors are built in the wave's LDS row (all
// zero on entry and on return) and written once, coalesced.
template <class SRC>
__device__ __forceinline__ bool put_clock(const SRC& B, uint64_t p, uint32_t n, uint32_t wa, uint32_t A,
                                          uint64_t* dst, uint64_t* row, uint32_t lane) {
  const uint64_t sa = wa + 8u;
  const bool lds = A <= kRowMax;
  bool bad = false;
  if (!lds) {
    for (uint32_t a = lane; a < A; a += kW) dst[a] = 0ull;
    __threadfence_block();
  }
  for (uint32_t k = lane; k < n; k += kW) {
    const uint64_t x = B.get(p + k * sa, wa), c = B.get(p + k * sa + wa, 8);
    const uint64_t px = k ? B.get(p + (k - 1u) * sa, wa) : 0ull;
    bad = bad || x >= A || c == 0ull || (k && px >= x);
    if (x < A) {
      if (lds) row[x] = c;
      else dst[x] = c;
    }
  }
  if (lds) {
    sync();
    for (uint32_t a = lane; a < A; a += kW) {
      dst[a] = row[a];
      row[a] = 0ull;
    }
    sync();
  }
  return bad;
}

// One MVReg at p (the stand-alone register, or an entry's value): its values
// in Vec order into clk[cap][A] / val[cap]; n out = the count. 0 or CRDT_E*.
template <class SRC>
__device__ __forceinline__ int walk_mvreg(const SRC& B, uint64_t& p, uint64_t len, uint32_t wa, uint32_t wv,
                                          uint32_t A, uint64_t* clk, uint64_t* val, uint32_t cap, uint32_t& n,
                                          bool& bad, uint64_t* row, uint32_t lane) {
  uint64_t nv;
  if (!take_len(B, p, len, 8u + wv, nv)) return CRDT_ENONCANON;
  if (nv > cap) return CRDT_ECAPACITY;
  for (uint32_t v = 0; v < (uint32_t)nv; ++v) {
    uint32_t nc;
    if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
    bad = put_clock(B, p, nc, wa, A, clk + (uint64_t)v * A, row, lane) || bad;
    p += (uint64_t)nc * (wa + 8u);
    if (len - p < wv) return CRDT_ENONCANON;
    const uint64_t x = B.get(p, wv);
    if (lane == 0u) val[v] = x;
    p += wv;
  }
  n = (uint32_t)nv;
  return 0;
}

// One Map<K, MVReg> at p into row i of R; p moves past it. whole: the map is
// the blob (bytes after it are trailing bytes); else it is an inner map of
// the nested map and the blob goes on. Only the used slots are written. 0 or
// CRDT_E* (the row is then unspecified).
template <class SRC, class LDS>
__device__ __forceinline__ int ingest_map(const SRC& B, uint64_t& p, uint64_t len, bool whole, Widths W, uint32_t A,
                                          const crdt_map_mvreg_slab& R, uint64_t i, LDS* X, uint32_t lane) {
  const uint32_t wa = W.wa, wk = W.wk, wv = W.wv;
  const uint64_t sa = wa + 8u;
  bool bad = false;
  uint32_t nc;
  if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
  bad = put_clock(B, p, nc, wa, A, R.clock + i * A, X->row, lane);
  p += nc * sa;
  // entries: BTreeMap order, keys strictly ascending
  uint64_t ne;
  if (!take_len(B, p, len, wk + 16u, ne)) return CRDT_ENONCANON;
  if (ne > R.kcap) return CRDT_ECAPACITY;
  uint64_t prev = 0;
  for (uint32_t e = 0; e < (uint32_t)ne; ++e) {
    const uint64_t slot = i * R.kcap + e;
    if (len - p < wk) return CRDT_ENONCANON;
    const uint64_t key = uni64(B.get(p, wk));
    p += wk;
    if (e && key <= prev) return CRDT_ENONCANON;
    prev = key;
    if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
    bad = put_clock(B, p, nc, wa, A, R.eclock + slot * A, X->row, lane) || bad;
    p += nc * sa;
    uint32_t nv = 0;
    const int rc = walk_mvreg(B, p, len, wa, wv, A, R.mv_clock + slot * R.mcap * A, R.mv_val + slot * R.mcap, R.mcap,
                              nv, bad, X->row, lane);
    if (rc) return rc;
    if (lane == 0u) {
      R.keys[slot] = key;
      R.mv_n[slot] = nv;
    }
  }
  // deferred: a HashMap, clocks in any order; the key sets ascending
  uint64_t nd;
  if (!take_len(B, p, len, 16u, nd)) return CRDT_ENONCANON;
  if (nd > R.dcap || nd > kDefMax) return CRDT_ECAPACITY;
  for (uint32_t d = 0; d < (uint32_t)nd; ++d) {
    if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
    const uint64_t pc = p;
    p += nc * sa;
    uint64_t ns;
    if (!take_len(B, p, len, wk, ns)) return CRDT_ENONCANON;
    if (ns > R.scap) return CRDT_ECAPACITY;
    if (lane == 0u) {
      X->Pd[d] = pc;
      X->Ld[d] = nc;
      X->Ps[d] = p;
      X->Ls[d] = (uint32_t)ns;
    }
    p += ns * wk;
  }
  if (whole && p != len) return CRDT_ENONCANON;  // trailing bytes
  if (nd) {
    sync();
    // rank by comparison count: lane d counts the clocks below clock d
    uint32_t r = 0;
    bool dup = false;
    if (lane < (uint32_t)nd) {
      const uint64_t pm = X->Pd[lane];
      const uint32_t lm = X->Ld[lane];
      for (uint32_t f = 0; f < (uint32_t)nd; ++f) {
        if (f == lane) continue;
        const int c = clock_cmp(B, X->Pd[f], X->Ld[f], pm, lm, wa);
        r += c < 0 ? 1u : 0u;
        dup = dup || c == 0;  // structurally equal HashMap keys
      }
      X->Rd[lane] = r;
    }
    if (__ballot(dup)) return CRDT_ENONCANON;
    sync();
    for (uint32_t d = 0; d < (uint32_t)nd; ++d) {
      const uint64_t slot = i * R.dcap + uni32(X->Rd[d]);  // ranks are distinct and < nd
      const uint64_t pc = uni64(X->Pd[d]), ps = uni64(X->Ps[d]);
      const uint32_t lc = uni32(X->Ld[d]), ls = uni32(X->Ls[d]);
      bad = put_clock(B, pc, lc, wa, A, R.dclock + slot * A, X->row, lane) || bad;
      for (uint32_t j = lane; j < ls; j += kW) {
        const uint64_t k = B.get(ps + (uint64_t)j * wk, wk);
        bad = bad || (j && B.get(ps + (uint64_t)(j - 1u) * wk, wk) >= k);
        R.dset[slot * R.scap + j] = k;
      }
      if (lane == 0u) R.dset_n[slot] = ls;
    }
  }
  if (lane == 0u) {
    R.n_keys[i] = (uint32_t)ne;
    R.n_def[i] = (uint32_t)nd;
  }
  return __ballot(bad) ? CRDT_ENONCANON : 0;
}

// object i of the MVReg slab from slot `from` on: all zero
__device__ __forceinline__ void mvreg_zero_tail(uint64_t* outclk, uint64_t* outval, uint32_t cap, uint32_t A,
                                                uint64_t i, uint32_t from, uint32_t lane) {
  uint64_t* c = outclk + (i * cap + from) * A;
  const uint64_t nc = (uint64_t)(cap - from) * A;
  for (uint64_t k = lane; k < nc; k += kW) c[k] = 0ull;
  for (uint32_t k = from + lane; k < cap; k += kW) outval[i * cap + k] = 0ull;
}

// One MVReg blob into object i of the zero-filled slab (n, clk[cap][A],
// val[cap]). An object in error is written as the empty register.
template <class SRC>
__device__ __forceinline__ int ingest_mvreg(const SRC& B, uint64_t len, uint32_t wa, uint32_t wv, uint32_t A,
                                            uint32_t* outn, uint64_t* outclk, uint64_t* outval, uint32_t cap,
                                            uint64_t i, WaveLds* X, uint32_t lane) {
  uint64_t p = 0;
  uint32_t n = 0;
  bool bad = false;
  int rc = walk_mvreg(B, p, len, wa, wv, A, outclk + i * cap * A, outval + i * cap, cap, n, bad, X->row, lane);
  if (!rc && p != len) rc = CRDT_ENONCANON;  // trailing bytes
  if (!rc && __ballot(bad)) rc = CRDT_ENONCANON;
  if (rc) return rc;
  mvreg_zero_tail(outclk, outval, cap, A, i, n, lane);
  if (lane == 0u) outn[i] = n;
  return 0;
}

// MAP: blobs -> rows of R; else blobs -> the MVReg slab (outn, outclk, outval, cap).
template <bool MAP>
__global__ __launch_bounds__(kW* kWaves) void map_bincode_ingest_kernel(
    const uint8_t* __restrict__ blobs, uint64_t blob_bytes, const uint64_t* __restrict__ boff,
    const uint64_t* __restrict__ blen, uint64_t n_obj, Widths W, uint32_t A, crdt_map_mvreg_slab R,
    uint32_t* __restrict__ outn, uint64_t* __restrict__ outclk, uint64_t* __restrict__ outval, uint32_t cap,
    int* __restrict__ status) {
  __shared__ WaveLds lds[kWaves];
  const uint32_t lane = threadIdx.x & (kW - 1u), wave = threadIdx.x / kW;
  WaveLds* X = &lds[wave];
  for (uint32_t a = lane; a < kRowMax; a += kW) X->row[a] = 0ull;
  sync();
  const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < n_obj; i += n_waves) {
    const uint64_t off = uni64(boff[i]), len = uni64(blen[i]);
    int rc;
    if (off > blob_bytes || len > blob_bytes - off) {
      rc = CRDT_ENONCANON;  // the blob is not inside the buffer: nothing of it is read
    } else if (len + 32u <= kStage) {
      sync();  // the previous object's window readers are done
      const uint32_t d = stage_blob(X->stage, blobs, blob_bytes, off, len, lane);
      sync();
      const Src<true> B{(const uint8_t*)X->stage, d};
      uint64_t p = 0;
      rc = MAP ? ingest_map(B, p, len, true, W, A, R, i, X, lane)
               : ingest_mvreg(B, len, W.wa, W.wv, A, outn, outclk, outval, cap, i, X, lane);
    } else {
      const Src<false> B{blobs + off};
      uint64_t p = 0;
      rc = MAP ? ingest_map(B, p, len, true, W, A, R, i, X, lane)
               : ingest_mvreg(B, len, W.wa, W.wv, A, outn, outclk, outval, cap, i, X, lane);
    }
    rc = (int)uni32((uint32_t)rc);
    if (rc) {
      if (!MAP) {  // the empty register (after the rows the walk wrote)
        __threadfence_block();
        mvreg_zero_tail(outclk, outval, cap, A, i, 0u, lane);
        if (lane == 0u) outn[i] = 0u;
      }
      if (lane == 0u) atomicCAS(status, 0, rc);
    }
  }
}

// ------------------------------------------------------------------- egest
// One lane: the pairs of the dense row (its non-zero slots); bad if one of
// them is an actor id that does not fit the actor width (amax = 2^(8 wa)).
__device__ __forceinline__ uint32_t lane_row_nnz(const uint64_t* row, uint32_t A, uint32_t amax, bool& bad) {
  uint32_t n = 0;
  for (uint32_t a = 0; a < A; ++a) {
    const bool nz = row[a] != 0ull;
    n += nz ? 1u : 0u;
    bad = bad || (nz && a >= amax);
  }
  return n;
}
// The same by the whole wave.
__device__ __forceinline__ uint32_t wave_row_nnz(const uint64_t* row, uint32_t A, uint32_t amax, bool& bad,
                                                 uint32_t lane) {
  uint32_t n = 0;
  for (uint32_t a0 = 0; a0 < A; a0 += kW) {
    const bool nz = a0 + lane < A && row[a0 + lane] != 0ull;
    bad = bad || (nz && a0 + lane >= amax);
    n += (uint32_t)__popcll(__ballot(nz));
  }
  return n;
}

// The dense row as a bincode clock at o + q, every lane writing the pair of
// its own slot at the place the ballot gives it; returns the position after it.
__device__ __forceinline__ uint64_t write_clock(uint8_t* o, uint64_t q, const uint64_t* row, uint32_t A, uint32_t wa,
                                                uint32_t lane) {
  const uint64_t sa = wa + 8u;
  const uint64_t v0 = lane < A ? row[lane] : 0ull;
  const uint64_t m0 = __ballot(v0 != 0ull);
  uint32_t n = (uint32_t)__popcll(m0);
  for (uint32_t a0 = kW; a0 < A; a0 += kW) n += (uint32_t)__popcll(__ballot(a0 + lane < A && row[a0 + lane] != 0ull));
  if (lane == 0u) wr(o, q, n, 8);
  q += 8u;
  if (v0 != 0ull) {
    const uint64_t at = q + sa * (uint32_t)__popcll(m0 & ((1ull << lane) - 1ull));
    wr(o, at, lane, wa);
    wr(o, at + wa, v0, 8);
  }
  uint32_t done = (uint32_t)__popcll(m0);
  for (uint32_t a0 = kW; a0 < A; a0 += kW) {
    const uint64_t v = a0 + lane < A ? row[a0 + lane] : 0ull;
    const uint64_t m = __ballot(v != 0ull);
    if (v != 0ull) {
      const uint64_t at = q + sa * (done + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)));
      wr(o, at, a0 + lane, wa);
      wr(o, at + wa, v, 8);
    }
    done += (uint32_t)__popcll(m);
  }
  return q + sa * n;
}

// One lane: the encoded bytes of value slot v of a register (clock + value).
__device__ __forceinline__ uint32_t lane_val_size(const uint64_t* clk, const uint64_t* val, uint32_t v, uint32_t A,
                                                  uint32_t wa, uint32_t wv, uint32_t amax, bool& bad) {
  bad = bad || !fits(val[v], wv);
  return 8u + (wa + 8u) * lane_row_nnz(clk + (uint64_t)v * A, A, amax, bad) + wv;
}

// One lane: the encoded bytes of key slot k of map row i (key, entry clock, register).
__device__ __forceinline__ uint32_t lane_entry_size(const crdt_map_mvreg_slab& S, uint64_t i, uint32_t k, Widths W,
                                                    uint32_t A, uint32_t amax, bool& bad) {
  const uint64_t slot = i * S.kcap + k;
  bad = bad || !fits(S.keys[slot], W.wk);
  uint32_t sz = W.wk + 8u + (W.wa + 8u) * lane_row_nnz(S.eclock + slot * A, A, amax, bad) + 8u;
  uint32_t nv = S.mv_n[slot];
  if (nv > S.mcap) {
    bad = true;
    nv = 0u;
  }
  for (uint32_t v = 0; v < nv; ++v)
    sz += lane_val_size(S.mv_clock + slot * S.mcap * A, S.mv_val + slot * S.mcap, v, A, W.wa, W.wv, amax, bad);
  return sz;
}

// The blob bytes of map row i (wave-uniform); bad: a count above its capacity
// or a key, value or actor that does not fit its width. first: the bytes of
// key slot `lane` (0 past the keys), which the write pass places first.
__device__ __forceinline__ uint64_t map_size(const crdt_map_mvreg_slab& S, uint64_t i, Widths W, uint32_t A,
                                             uint32_t amax, bool& bad_out, uint32_t& first, uint32_t lane) {
  first = 0u;
  const uint32_t nk = uni32(S.n_keys[i]), nd = uni32(S.n_def[i]);
  if (nk > S.kcap || nd > S.dcap) {
    bad_out = true;
    return 0u;
  }
  const uint64_t sa = W.wa + 8u;
  bool bad = false;
  uint64_t mine = 0;
  for (uint32_t k = lane; k < nk; k += kW) {
    const uint32_t sz = lane_entry_size(S, i, k, W, A, amax, bad);
    if (k < kW) first = sz;
    mine += sz;
  }
  for (uint32_t d = lane; d < nd; d += kW) {
    const uint64_t slot = i * S.dcap + d;
    uint32_t ns = S.dset_n[slot];
    if (ns > S.scap) {
      bad = true;
      ns = 0u;
    }
    for (uint32_t j = 0; j < ns; ++j) bad = bad || !fits(S.dset[slot * S.scap + j], W.wk);
    mine += 8u + sa * lane_row_nnz(S.dclock + slot * A, A, amax, bad) + 8u + (uint64_t)ns * W.wk;
  }
  const uint64_t total = 24u + sa * wave_row_nnz(S.clock + i * A, A, amax, bad, lane) + wave_sum64(mine);
  bad_out = __ballot(bad) != 0ull;
  return uni64(total);
}

// Map row i as a blob at o (its size and fit are checked; first: map_size's).
__device__ __forceinline__ void map_write(const crdt_map_mvreg_slab& S, uint64_t i, Widths W, uint32_t A,
                                          uint32_t amax, uint8_t* o, uint32_t first, uint32_t lane) {
  const uint32_t wa = W.wa, wk = W.wk, wv = W.wv;
  const uint32_t nk = uni32(S.n_keys[i]), nd = uni32(S.n_def[i]);
  uint64_t p = write_clock(o, 0u, S.clock + i * A, A, wa, lane);
  if (lane == 0u) wr(o, p, nk, 8);
  p += 8u;
  for (uint32_t k0 = 0; k0 < nk; k0 += kW) {
    // 64 keys: sized one per lane, placed by the prefix sum, written by the wave
    const uint32_t cnt = nk - k0 < kW ? nk - k0 : kW;
    bool ign = false;
    const uint32_t sz = k0 == 0u ? first : lane < cnt ? lane_entry_size(S, i, k0 + lane, W, A, amax, ign) : 0u;
    const uint32_t incl = scan_incl(sz, lane), excl = incl - sz;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint64_t slot = i * S.kcap + k0 + j;
      uint64_t q = p + (uint32_t)__builtin_amdgcn_readlane(excl, j);
      if (lane == 0u) wr(o, q, S.keys[slot], wk);
      q = write_clock(o, q + wk, S.eclock + slot * A, A, wa, lane);
      const uint32_t nv = uni32(S.mv_n[slot]);
      if (lane == 0u) wr(o, q, nv, 8);
      q += 8u;
      for (uint32_t v = 0; v < nv; ++v) {
        q = write_clock(o, q, S.mv_clock + (slot * S.mcap + v) * A, A, wa, lane);
        if (lane == 0u) wr(o, q, S.mv_val[slot * S.mcap + v], wv);
        q += wv;
      }
    }
    p += (uint32_t)__builtin_amdgcn_readlane(incl, kW - 1u);
  }
  if (lane == 0u) wr(o, p, nd, 8);
  p += 8u;
  for (uint32_t d = 0; d < nd; ++d) {  // the slab's CLOCK ORDER
    const uint64_t slot = i * S.dcap + d;
    p = write_clock(o, p, S.dclock + slot * A, A, wa, lane);
    const uint32_t ns = uni32(S.dset_n[slot]);
    if (lane == 0u) wr(o, p, ns, 8);
    p += 8u;
    for (uint32_t j = lane; j < ns; j += kW) wr(o, p + (uint64_t)j * wk, S.dset[slot * S.scap + j], wk);
    p += (uint64_t)ns * wk;
  }
}

__device__ __forceinline__ uint64_t mvreg_size(const uint32_t* sn, const uint64_t* clk, const uint64_t* val,
                                               uint32_t cap, uint64_t i, uint32_t A, uint32_t wa, uint32_t wv,
                                               uint32_t amax, bool& bad_out, uint32_t& first,
                                               uint32_t lane) {
  first = 0u;
  const uint32_t n = uni32(sn[i]);
  if (n > cap) {
    bad_out = true;
    return 0u;
  }
  bool bad = false;
  uint64_t mine = 0;
  for (uint32_t v = lane; v < n; v += kW) {
    const uint32_t sz = lane_val_size(clk + i * cap * A, val + i * cap, v, A, wa, wv, amax, bad);
    if (v < kW) first = sz;
    mine += sz;
  }
  const uint64_t total = 8u + wave_sum64(mine);
  bad_out = __ballot(bad) != 0ull;
  return uni64(total);
}

__device__ __forceinline__ void mvreg_write(const uint32_t* sn, const uint64_t* clk, const uint64_t* val, uint32_t cap,
                                            uint64_t i, uint32_t A, uint32_t wa, uint32_t wv, uint32_t amax,
                                            uint8_t* o, uint32_t first, uint32_t lane) {
  const uint32_t n = uni32(sn[i]);
  const uint64_t* c = clk + i * cap * A;
  const uint64_t* x = val + i * cap;
  if (lane == 0u) wr(o, 0u, n, 8);
  uint64_t p = 8u;
  for (uint32_t v0 = 0; v0 < n; v0 += kW) {
    const uint32_t cnt = n - v0 < kW ? n - v0 : kW;
    bool ign = false;
    const uint32_t sz = v0 == 0u ? first : lane < cnt ? lane_val_size(c, x, v0 + lane, A, wa, wv, amax, ign) : 0u;
    const uint32_t incl = scan_incl(sz, lane), excl = incl - sz;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint64_t q = write_clock(o, p + (uint32_t)__builtin_amdgcn_readlane(excl, j), c + (uint64_t)(v0 + j) * A,
                                     A, wa, lane);
      if (lane == 0u) wr(o, q, x[v0 + j], wv);
    }
    p += (uint32_t)__builtin_amdgcn_readlane(incl, kW - 1u);
  }
}

// WRITE: blob i at out + ooff[i]; else sizes[i] = its bytes (0: an object in error).
template <bool MAP, bool WRITE>
__global__ __launch_bounds__(kW* kWaves) void map_bincode_egest_kernel(
    crdt_map_mvreg_slab S, const uint32_t* __restrict__ sn, const uint64_t* __restrict__ sclk,
    const uint64_t* __restrict__ sval, uint32_t cap, uint64_t n_obj, Widths W, uint32_t A,
    uint64_t* __restrict__ sizes, uint8_t* __restrict__ out, const uint64_t* __restrict__ ooff, uint64_t out_bytes,
    int* __restrict__ status) {
  const uint32_t lane = threadIdx.x & (kW - 1u), wave = threadIdx.x / kW;
  const uint32_t amax = W.wa >= 4u ? 0xFFFFFFFFu : 1u << (8u * W.wa);
  const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < n_obj; i += n_waves) {
    bool bad = false;
    uint32_t first = 0;
    const uint64_t size = MAP ? map_size(S, i, W, A, amax, bad, first, lane)
                              : mvreg_size(sn, sclk, sval, cap, i, A, W.wa, W.wv, amax, bad, first, lane);
    int rc = bad ? CRDT_ENONCANON : 0;
    if (WRITE && !rc) {
      const uint64_t oo = uni64(ooff[i]);
      if (oo > out_bytes || size > out_bytes - oo) rc = CRDT_ECAPACITY;  // the placed blob leaves the buffer
      else if (MAP) map_write(S, i, W, A, amax, out + oo, first, lane);
      else mvreg_write(sn, sclk, sval, cap, i, A, W.wa, W.wv, amax, out + oo, first, lane);
    }
    if (lane == 0u) {
      if (!WRITE) sizes[i] = rc ? 0ull : size;
      if (rc) atomicCAS(status, 0, rc);
    }
  }
}

// ---------------------------------------- Map<u64, Orswot> and the nested map
// The two Map types whose values are containers (crdt_map_orswot_slab,
// crdt_map_map_slab). Format, after the Map form above:
//
//   Orswot   VClock clock
//            u64 n_mem | n_mem x (M member | VClock)        HashMap: any order
//            u64 n_def | n_def x (VClock | u64 n | n x M)   HashMap of HashSet:
//                                             clocks and members in any order
//   Map<K, Orswot>          entries: K key | VClock | Orswot
//   Map<K, Map<K2, MVReg>>  entries: K key | VClock | Map<K2, MVReg> (the Map form)
//
// Ingest sorts what the reference leaves unordered, all by comparison count
// out of one table of kNestMax positions: lane l ranks elements l, l + 64, ...
// A tie is a duplicate.
struct NWidths {
  uint32_t wa, wk, wx, wv;  // actor, key, member / inner key, value bytes
};

// A deferred section at p (u64 n | n x (VClock | u64 n | n x E), E of we
// bytes): the clocks ranked into CLOCK ORDER into dclock[dcap][A], their sets
// into dset_n[dcap] / dset[dcap][scap] — HASHSET: sorted ascending by rank (a
// HashSet, <= kNestMax elements), else copied and checked strictly ascending
// (a BTreeSet). p moves past the section; n = the clocks. 0 or CRDT_E*.
template <bool HASHSET, class SRC, class LDS>
__device__ __forceinline__ int walk_deferred(const SRC& B, uint64_t& p, uint64_t len, uint32_t wa, uint32_t we,
                                             uint32_t A, uint64_t* dclock, uint32_t* dset_n, uint64_t* dset,
                                             uint32_t dcap, uint32_t scap, uint32_t& n, bool& bad, LDS* X,
                                             uint32_t lane) {
  const uint64_t sa = wa + 8u;
  uint64_t nd;
  if (!take_len(B, p, len, 16u, nd)) return CRDT_ENONCANON;
  if (nd > dcap || nd > LDS::kDef) return CRDT_ECAPACITY;
  sync();  // the table's earlier readers are done
  for (uint32_t d = 0; d < (uint32_t)nd; ++d) {
    uint32_t nc;
    if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
    const uint64_t pc = p;
    p += nc * sa;
    uint64_t ns;
    if (!take_len(B, p, len, we, ns)) return CRDT_ENONCANON;
    if (ns > scap) return CRDT_ECAPACITY;
    if (lane == 0u) {
      X->Pd[d] = pc;
      X->Ld[d] = nc;
      X->Ps[d] = p;
      X->Ls[d] = (uint32_t)ns;
    }
    p += ns * we;
  }
  n = (uint32_t)nd;
  if (!nd) return 0;
  sync();
  bool dup = false;
  for (uint32_t d = lane; d < (uint32_t)nd; d += kW) {
    const uint64_t pm = X->Pd[d];
    const uint32_t lm = X->Ld[d];
    uint32_t r = 0;
    for (uint32_t f = 0; f < (uint32_t)nd; ++f) {
      if (f == d) continue;
      const int c = clock_cmp(B, X->Pd[f], X->Ld[f], pm, lm, wa);
      r += c < 0 ? 1u : 0u;
      dup = dup || c == 0;  // structurally equal HashMap keys
    }
    X->Rd[d] = r;
  }
  if (__ballot(dup)) return CRDT_ENONCANON;
  sync();
  for (uint32_t d = 0; d < (uint32_t)nd; ++d) {
    const uint64_t slot = uni32(X->Rd[d]);  // ranks are distinct and < nd
    const uint64_t pc = uni64(X->Pd[d]), ps = uni64(X->Ps[d]);
    const uint32_t lc = uni32(X->Ld[d]), ls = uni32(X->Ls[d]);
    bad = put_clock(B, pc, lc, wa, A, dclock + slot * A, X->row, lane) || bad;
    for (uint32_t j = lane; j < ls; j += kW) {
      const uint64_t k = B.get(ps + (uint64_t)j * we, we);
      if (HASHSET) {
        uint32_t r = 0;
        for (uint32_t f = 0; f < ls; ++f) {
          const uint64_t x = B.get(ps + (uint64_t)f * we, we);
          r += x < k ? 1u : 0u;
          bad = bad || (x == k && f != j);  // two equal members: their ranks tie (and stay < ls)
        }
        dset[slot * scap + r] = k;
      } else {
        bad = bad || (j && B.get(ps + (uint64_t)(j - 1u) * we, we) >= k);
        dset[slot * scap + j] = k;
      }
    }
    if (lane == 0u) dset_n[slot] = ls;
  }
  return 0;
}

// One Map<K, Orswot> blob into row i of R: only the used slots. 0 or CRDT_E*.
template <class SRC>
__device__ __forceinline__ int ingest_obj(const SRC& B, uint64_t len, NWidths W, uint32_t A,
                                          const crdt_map_orswot_slab& R, uint64_t i, NestLds* X, uint32_t lane) {
  const uint32_t wa = W.wa, wk = W.wk, wm = W.wx;
  const uint64_t sa = wa + 8u;
  uint64_t p = 0;
  bool bad = false;
  uint32_t nc;
  if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
  bad = put_clock(B, p, nc, wa, A, R.clock + i * A, X->row, lane);
  p += nc * sa;
  // entries: BTreeMap order; an entry is at least its key, two clocks and two length words
  uint64_t ne;
  if (!take_len(B, p, len, wk + 32u, ne)) return CRDT_ENONCANON;
  if (ne > R.kcap) return CRDT_ECAPACITY;
  uint64_t prev = 0;
  for (uint32_t e = 0; e < (uint32_t)ne; ++e) {
    const uint64_t slot = i * R.kcap + e;
    if (len - p < wk) return CRDT_ENONCANON;
    const uint64_t key = uni64(B.get(p, wk));
    p += wk;
    if (e && key <= prev) return CRDT_ENONCANON;
    prev = key;
    if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
    bad = put_clock(B, p, nc, wa, A, R.eclock + slot * A, X->row, lane) || bad;
    p += nc * sa;
    if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
    bad = put_clock(B, p, nc, wa, A, R.vclock + slot * A, X->row, lane) || bad;
    p += nc * sa;
    // members: a HashMap, any order; sorted by rank, each clock row with its member
    uint64_t nm;
    if (!take_len(B, p, len, wm + 8u, nm)) return CRDT_ENONCANON;
    if (nm > R.mcap || nm > kNestMax) return CRDT_ECAPACITY;
    sync();  // the table's earlier readers are done
    for (uint32_t j = 0; j < (uint32_t)nm; ++j) {
      if (len - p < wm) return CRDT_ENONCANON;
      const uint64_t x = B.get(p, wm);
      p += wm;
      if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
      if (lane == 0u) {
        X->Ps[j] = x;
        X->Pd[j] = p;
        X->Ld[j] = nc;
      }
      p += nc * sa;
    }
    if (nm) {
      sync();
      bool dup = false;
      for (uint32_t j = lane; j < (uint32_t)nm; j += kW) {
        const uint64_t x = X->Ps[j];
        uint32_t r = 0;
        for (uint32_t f = 0; f < (uint32_t)nm; ++f) {
          const uint64_t y = X->Ps[f];
          r += y < x ? 1u : 0u;
          dup = dup || (y == x && f != j);
        }
        X->Rd[j] = r;
      }
      if (__ballot(dup)) return CRDT_ENONCANON;  // two equal members
      sync();
      for (uint32_t j = 0; j < (uint32_t)nm; ++j) {
        const uint64_t ms = slot * R.mcap + uni32(X->Rd[j]);  // ranks are distinct and < nm
        bad = put_clock(B, uni64(X->Pd[j]), uni32(X->Ld[j]), wa, A, R.vmclock + ms * A, X->row, lane) || bad;
        if (lane == 0u) R.vmem[ms] = X->Ps[j];
      }
    }
    uint32_t nv = 0;
    const int rc = walk_deferred<true>(B, p, len, wa, wm, A, R.vdclock + slot * R.vdcap * A, R.vdset_n + slot * R.vdcap,
                                       R.vdset + slot * R.vdcap * R.vscap, R.vdcap, R.vscap, nv, bad, X, lane);
    if (rc) return rc;
    if (lane == 0u) {
      R.keys[slot] = key;
      R.vn_mem[slot] = (uint32_t)nm;
      R.vn_def[slot] = nv;
    }
  }
  uint32_t nd = 0;
  const int rc = walk_deferred<false>(B, p, len, wa, wk, A, R.dclock + i * R.dcap * A, R.dset_n + i * R.dcap,
                                      R.dset + i * R.dcap * R.scap, R.dcap, R.scap, nd, bad, X, lane);
  if (rc) return rc;
  if (p != len) return CRDT_ENONCANON;  // trailing bytes
  if (lane == 0u) {
    R.n_keys[i] = (uint32_t)ne;
    R.n_def[i] = nd;
  }
  return __ballot(bad) ? CRDT_ENONCANON : 0;
}

// One Map<K, Map<K2, MVReg>> blob into row i of R, inner map k as row
// i * kcap + k of R.inner: only the used slots. 0 or CRDT_E*.
template <class SRC>
__device__ __forceinline__ int ingest_obj(const SRC& B, uint64_t len, NWidths W, uint32_t A,
                                          const crdt_map_map_slab& R, uint64_t i, NestLds* X, uint32_t lane) {
  const uint32_t wa = W.wa, wk = W.wk;
  const uint64_t sa = wa + 8u;
  uint64_t p = 0;
  bool bad = false;
  uint32_t nc;
  if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
  bad = put_clock(B, p, nc, wa, A, R.clock + i * A, X->row, lane);
  p += nc * sa;
  // entries: an entry is at least its key, its clock and the empty inner map (24 bytes)
  uint64_t ne;
  if (!take_len(B, p, len, wk + 32u, ne)) return CRDT_ENONCANON;
  if (ne > R.kcap) return CRDT_ECAPACITY;
  uint64_t prev = 0;
  for (uint32_t e = 0; e < (uint32_t)ne; ++e) {
    const uint64_t slot = i * R.kcap + e;
    if (len - p < wk) return CRDT_ENONCANON;
    const uint64_t key = uni64(B.get(p, wk));
    p += wk;
    if (e && key <= prev) return CRDT_ENONCANON;
    prev = key;
    if (!take_clock(B, p, len, wa, A, nc)) return CRDT_ENONCANON;
    bad = put_clock(B, p, nc, wa, A, R.eclock + slot * A, X->row, lane) || bad;
    p += nc * sa;
    sync();  // the table's earlier readers are done
    const int rc = ingest_map(B, p, len, false, Widths{wa, W.wx, W.wv}, A, R.inner, slot, X, lane);
    if (rc) return rc;
    if (lane == 0u) R.keys[slot] = key;
  }
  uint32_t nd = 0;
  const int rc = walk_deferred<false>(B, p, len, wa, wk, A, R.dclock + i * R.dcap * A, R.dset_n + i * R.dcap,
                                      R.dset + i * R.dcap * R.scap, R.dcap, R.scap, nd, bad, X, lane);
  if (rc) return rc;
  if (p != len) return CRDT_ENONCANON;  // trailing bytes
  if (lane == 0u) {
    R.n_keys[i] = (uint32_t)ne;
    R.n_def[i] = nd;
  }
  return __ballot(bad) ? CRDT_ENONCANON : 0;
}

// SLAB: crdt_map_orswot_slab or crdt_map_map_slab; blobs -> rows of R.
template <class SLAB>
__global__ __launch_bounds__(kW* kWaves) void nested_bincode_ingest_kernel(
    const uint8_t* __restrict__ blobs, uint64_t blob_bytes, const uint64_t* __restrict__ boff,
    const uint64_t* __restrict__ blen, uint64_t n_obj, NWidths W, uint32_t A, SLAB R, int* __restrict__ status) {
  __shared__ NestLds lds[kWaves];
  const uint32_t lane = threadIdx.x & (kW - 1u), wave = threadIdx.x / kW;
  NestLds* X = &lds[wave];
  for (uint32_t a = lane; a < kRowMax; a += kW) X->row[a] = 0ull;
  sync();
  const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < n_obj; i += n_waves) {
    const uint64_t off = uni64(boff[i]), len = uni64(blen[i]);
    int rc;
    if (off > blob_bytes || len > blob_bytes - off) {
      rc = CRDT_ENONCANON;  // the blob is not inside the buffer: nothing of it is read
    } else if (len + 32u <= kStage) {
      sync();  // the previous object's window readers are done
      const uint32_t d = stage_blob(X->stage, blobs, blob_bytes, off, len, lane);
      sync();
      rc = ingest_obj(Src<true>{(const uint8_t*)X->stage, d}, len, W, A, R, i, X, lane);
    } else {
      rc = ingest_obj(Src<false>{blobs + off}, len, W, A, R, i, X, lane);
    }
    rc = (int)uni32((uint32_t)rc);
    if (rc && lane == 0u) atomicCAS(status, 0, rc);
  }
}

// ------------------------------------------------ egest, one level down
// One lane: the bytes of deferred entry `slot` (clock, length word, set of we-
// byte elements); bad: a set above scap, an element or actor that does not fit.
__device__ __forceinline__ uint64_t lane_def_size(const uint64_t* dclock, const uint32_t* dset_n, const uint64_t* dset,
                                                  uint64_t slot, uint32_t scap, uint32_t A, uint32_t wa, uint32_t we,
                                                  uint32_t amax, bool& bad) {
  uint32_t ns = dset_n[slot];
  if (ns > scap) {
    bad = true;
    ns = 0u;
  }
  if (we < 8u)
    for (uint32_t j = 0; j < ns; ++j) bad = bad || !fits(dset[slot * scap + j], we);
  return 8u + (uint64_t)(wa + 8u) * lane_row_nnz(dclock + slot * A, A, amax, bad) + 8u + (uint64_t)ns * we;
}

// One lane's share of the pairs of n dense rows laid end to end (coalesced).
__device__ __forceinline__ uint32_t flat_nnz(const uint64_t* rows, uint32_t n, uint32_t A, uint32_t amax, bool& bad,
                                             uint32_t lane) {
  uint32_t c = 0;
  for (uint32_t x = lane; x < n * A; x += kW) {  // n <= 512 rows of A <= 128
    const bool nz = rows[x] != 0ull;
    c += nz ? 1u : 0u;
    bad = bad || (nz && x % A >= amax);
  }
  return c;
}

// n deferred entries from slot d0 on, at o + p, in slab order; returns the position after them.
__device__ __forceinline__ uint64_t write_deferred(uint8_t* o, uint64_t p, const uint64_t* dclock,
                                                   const uint32_t* dset_n, const uint64_t* dset, uint64_t d0,
                                                   uint32_t n, uint32_t scap, uint32_t A, uint32_t wa, uint32_t we,
                                                   uint32_t lane) {
  if (lane == 0u) wr(o, p, n, 8);
  p += 8u;
  for (uint32_t d = 0; d < n; ++d) {
    const uint64_t slot = d0 + d;
    p = write_clock(o, p, dclock + slot * A, A, wa, lane);
    const uint32_t ns = uni32(dset_n[slot]);
    if (lane == 0u) wr(o, p, ns, 8);
    p += 8u;
    for (uint32_t j = lane; j < ns; j += kW) wr(o, p + (uint64_t)j * we, dset[slot * scap + j], we);
    p += (uint64_t)ns * we;
  }
  return p;
}

// The blob bytes of row i of a Map<u64, Orswot> slab (wave-uniform): the wave
// goes key by key and counts each nested set's pairs over its member rows laid
// end to end. bad: a count above its capacity or a key, member or actor that
// does not fit its width.
__device__ __forceinline__ uint64_t obj_size(const crdt_map_orswot_slab& S, uint64_t i, NWidths W, uint32_t A,
                                             uint32_t amax, bool& bad_out, uint32_t lane) {
  const uint32_t wk = W.wk, wm = W.wx;
  const uint32_t nk = uni32(S.n_keys[i]), nd = uni32(S.n_def[i]);
  if (nk > S.kcap || nd > S.dcap) {
    bad_out = true;
    return 0u;
  }
  const uint64_t sa = W.wa + 8u;
  bool bad = false;
  uint64_t fixed = 24u, pairs = 0, mine = 0;  // wave-uniform bytes; this lane's pairs and bytes
  for (uint32_t k = 0; k < nk; ++k) {
    const uint64_t slot = i * S.kcap + k;
    const uint32_t nm = uni32(S.vn_mem[slot]), nv = uni32(S.vn_def[slot]);
    if (nm > S.mcap || nv > S.vdcap) {
      bad = true;
      continue;
    }
    fixed += wk + 32u + (uint64_t)nm * (wm + 8u);
    pairs += flat_nnz(S.vmclock + slot * S.mcap * A, nm, A, amax, bad, lane);
    if (wm < 8u)
      for (uint32_t j = lane; j < nm; j += kW) bad = bad || !fits(S.vmem[slot * S.mcap + j], wm);
    for (uint32_t d = lane; d < nv; d += kW)
      mine += lane_def_size(S.vdclock, S.vdset_n, S.vdset, slot * S.vdcap + d, S.vscap, A, W.wa, wm, amax, bad);
  }
  for (uint32_t d = lane; d < nd; d += kW)
    mine += lane_def_size(S.dclock, S.dset_n, S.dset, i * S.dcap + d, S.scap, A, W.wa, wk, amax, bad);
  // the map clock, and the keys' entry clocks and top clocks, each laid end to end
  pairs += flat_nnz(S.clock + i * A, 1u, A, amax, bad, lane);
  pairs += flat_nnz(S.eclock + i * S.kcap * A, nk, A, amax, bad, lane);
  pairs += flat_nnz(S.vclock + i * S.kcap * A, nk, A, amax, bad, lane);
  if (wk < 8u)
    for (uint32_t k = lane; k < nk; k += kW) bad = bad || !fits(S.keys[i * S.kcap + k], wk);
  const uint64_t total = fixed + wave_sum64(mine + sa * pairs);
  bad_out = __ballot(bad) != 0ull;
  return uni64(total);
}

// Row i as a blob at o (its size and fit are checked), every container in slab order.
__device__ __forceinline__ void obj_write(const crdt_map_orswot_slab& S, uint64_t i, NWidths W, uint32_t A,
                                          uint32_t amax, uint8_t* o, uint32_t lane) {
  const uint32_t wa = W.wa, wk = W.wk, wm = W.wx;
  const uint32_t nk = uni32(S.n_keys[i]), nd = uni32(S.n_def[i]);
  uint64_t p = write_clock(o, 0u, S.clock + i * A, A, wa, lane);
  if (lane == 0u) wr(o, p, nk, 8);
  p += 8u;
  for (uint32_t k = 0; k < nk; ++k) {
    const uint64_t slot = i * S.kcap + k;
    if (lane == 0u) wr(o, p, S.keys[slot], wk);
    p = write_clock(o, p + wk, S.eclock + slot * A, A, wa, lane);
    p = write_clock(o, p, S.vclock + slot * A, A, wa, lane);
    const uint32_t nm = uni32(S.vn_mem[slot]);
    if (lane == 0u) wr(o, p, nm, 8);
    p += 8u;
    for (uint32_t j = 0; j < nm; ++j) {
      if (lane == 0u) wr(o, p, S.vmem[slot * S.mcap + j], wm);
      p = write_clock(o, p + wm, S.vmclock + (slot * S.mcap + j) * A, A, wa, lane);
    }
    p = write_deferred(o, p, S.vdclock, S.vdset_n, S.vdset, slot * S.vdcap, uni32(S.vn_def[slot]), S.vscap, A, wa, wm,
                       lane);
  }
  write_deferred(o, p, S.dclock, S.dset_n, S.dset, i * S.dcap, nd, S.scap, A, wa, wk, lane);
}

// The bytes of row r of a Map<u64, MVReg> slab as an inner map of the nested
// map, counted like a nested set: the wave-uniform bytes into fixed, this
// lane's pairs and bytes into pairs / mine. (map_size gives a lane a whole
// entry; here the wave reads the entry clocks and each register's rows laid
// end to end.)
__device__ __forceinline__ void inner_size(const crdt_map_mvreg_slab& S, uint64_t r, Widths W, uint32_t A,
                                           uint32_t amax, uint64_t& fixed, uint64_t& pairs, uint64_t& mine, bool& bad,
                                           uint32_t lane) {
  const uint32_t wk = W.wk, wv = W.wv;
  const uint32_t nk = uni32(S.n_keys[r]), nd = uni32(S.n_def[r]);
  if (nk > S.kcap || nd > S.dcap) {
    bad = true;
    return;
  }
  fixed += 24u + (uint64_t)nk * (wk + 16u);
  pairs += flat_nnz(S.clock + r * A, 1u, A, amax, bad, lane);
  pairs += flat_nnz(S.eclock + r * S.kcap * A, nk, A, amax, bad, lane);
  if (wk < 8u)
    for (uint32_t k = lane; k < nk; k += kW) bad = bad || !fits(S.keys[r * S.kcap + k], wk);
  for (uint32_t k = 0; k < nk; ++k) {
    const uint64_t slot = r * S.kcap + k;
    const uint32_t nv = uni32(S.mv_n[slot]);
    if (nv > S.mcap) {
      bad = true;
      continue;
    }
    fixed += (uint64_t)nv * (8u + wv);
    pairs += flat_nnz(S.mv_clock + slot * S.mcap * A, nv, A, amax, bad, lane);
    if (wv < 8u)
      for (uint32_t v = lane; v < nv; v += kW) bad = bad || !fits(S.mv_val[slot * S.mcap + v], wv);
  }
  for (uint32_t d = lane; d < nd; d += kW)
    mine += lane_def_size(S.dclock, S.dset_n, S.dset, r * S.dcap + d, S.scap, A, W.wa, wk, amax, bad);
}

// Row r of a Map<u64, MVReg> slab at o + p, field after field; returns the position after it.
__device__ __forceinline__ uint64_t inner_write(const crdt_map_mvreg_slab& S, uint64_t r, Widths W, uint32_t A,
                                                uint8_t* o, uint64_t p, uint32_t lane) {
  const uint32_t wa = W.wa, wk = W.wk, wv = W.wv;
  const uint32_t nk = uni32(S.n_keys[r]), nd = uni32(S.n_def[r]);
  p = write_clock(o, p, S.clock + r * A, A, wa, lane);
  if (lane == 0u) wr(o, p, nk, 8);
  p += 8u;
  for (uint32_t k = 0; k < nk; ++k) {
    const uint64_t slot = r * S.kcap + k;
    if (lane == 0u) wr(o, p, S.keys[slot], wk);
    p = write_clock(o, p + wk, S.eclock + slot * A, A, wa, lane);
    const uint32_t nv = uni32(S.mv_n[slot]);
    if (lane == 0u) wr(o, p, nv, 8);
    p += 8u;
    for (uint32_t v = 0; v < nv; ++v) {
      p = write_clock(o, p, S.mv_clock + (slot * S.mcap + v) * A, A, wa, lane);
      if (lane == 0u) wr(o, p, S.mv_val[slot * S.mcap + v], wv);
      p += wv;
    }
  }
  return write_deferred(o, p, S.dclock, S.dset_n, S.dset, r * S.dcap, nd, S.scap, A, wa, wk, lane);
}

// The same for the nested map: a key's bytes are its inner map's.
__device__ __forceinline__ uint64_t obj_size(const crdt_map_map_slab& S, uint64_t i, NWidths W, uint32_t A,
                                             uint32_t amax, bool& bad_out, uint32_t lane) {
  const uint32_t wk = W.wk;
  const uint32_t nk = uni32(S.n_keys[i]), nd = uni32(S.n_def[i]);
  if (nk > S.kcap || nd > S.dcap) {
    bad_out = true;
    return 0u;
  }
  const uint64_t sa = W.wa + 8u;
  const Widths WI{W.wa, W.wx, W.wv};
  bool bad = false;
  uint64_t fixed = 24u + (uint64_t)nk * (wk + 8u), pairs = 0, mine = 0;
  pairs += flat_nnz(S.clock + i * A, 1u, A, amax, bad, lane);
  pairs += flat_nnz(S.eclock + i * S.kcap * A, nk, A, amax, bad, lane);
  if (wk < 8u)
    for (uint32_t k = lane; k < nk; k += kW) bad = bad || !fits(S.keys[i * S.kcap + k], wk);
  for (uint32_t k = 0; k < nk; ++k) inner_size(S.inner, i * S.kcap + k, WI, A, amax, fixed, pairs, mine, bad, lane);
  for (uint32_t d = lane; d < nd; d += kW)
    mine += lane_def_size(S.dclock, S.dset_n, S.dset, i * S.dcap + d, S.scap, A, W.wa, wk, amax, bad);
  const uint64_t total = fixed + wave_sum64(mine + sa * pairs);
  bad_out = __ballot(bad) != 0ull;
  return uni64(total);
}

__device__ __forceinline__ void obj_write(const crdt_map_map_slab& S, uint64_t i, NWidths W, uint32_t A,
                                          uint32_t amax, uint8_t* o, uint32_t lane) {
  const uint32_t wa = W.wa, wk = W.wk;
  const uint32_t nk = uni32(S.n_keys[i]), nd = uni32(S.n_def[i]);
  const Widths WI{wa, W.wx, W.wv};
  uint64_t p = write_clock(o, 0u, S.clock + i * A, A, wa, lane);
  if (lane == 0u) wr(o, p, nk, 8);
  p += 8u;
  for (uint32_t k = 0; k < nk; ++k) {
    const uint64_t slot = i * S.kcap + k;
    if (lane == 0u) wr(o, p, S.keys[slot], wk);
    p = write_clock(o, p + wk, S.eclock + slot * A, A, wa, lane);
    p = inner_write(S.inner, slot, WI, A, o, p, lane);
  }
  write_deferred(o, p, S.dclock, S.dset_n, S.dset, i * S.dcap, nd, S.scap, A, wa, wk, lane);
}

// WRITE: blob i at out + ooff[i]; else sizes[i] = its bytes (0: an object in error).
template <class SLAB, bool WRITE>
__global__ __launch_bounds__(kW* kWaves) void nested_bincode_egest_kernel(
    SLAB S, uint64_t n_obj, NWidths W, uint32_t A, uint64_t* __restrict__ sizes, uint8_t* __restrict__ out,
    const uint64_t* __restrict__ ooff, uint64_t out_bytes, int* __restrict__ status) {
  const uint32_t lane = threadIdx.x & (kW - 1u), wave = threadIdx.x / kW;
  const uint32_t amax = W.wa >= 4u ? 0xFFFFFFFFu : 1u << (8u * W.wa);
  const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
  for (uint64_t i = (uint64_t)blockIdx.x * kWaves + wave; i < n_obj; i += n_waves) {
    bool bad = false;
    const uint64_t size = obj_size(S, i, W, A, amax, bad, lane);
    int rc = bad ? CRDT_ENONCANON : 0;
    if (WRITE && !rc) {
      const uint64_t oo = uni64(ooff[i]);
      if (oo > out_bytes || size > out_bytes - oo) rc = CRDT_ECAPACITY;  // the placed blob leaves the buffer
      else obj_write(S, i, W, A, amax, out + oo, lane);
    }
    if (lane == 0u) {
      if (!WRITE) sizes[i] = rc ? 0ull : size;
      if (rc) atomicCAS(status, 0, rc);
    }
  }
}

uint32_t grid_for(uint64_t n_obj, uint32_t blocks_per_cu) {
  const uint64_t want = (n_obj + kWaves - 1u) / kWaves, cap = (uint64_t)cu_count() * blocks_per_cu;
  return (uint32_t)(want < cap ? want : cap);
}

const crdt_map_mvreg_slab kNoSlab{};

}  // namespace

int launch_map_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                              uint64_t n_obj, uint32_t wa, uint32_t wk, uint32_t wv, uint32_t A,
                              const crdt_map_mvreg_slab& R, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  hipLaunchKernelGGL((map_bincode_ingest_kernel<true>), dim3(grid_for(n_obj, 5u)), dim3(kW * kWaves), 0, stream, blobs,
                     blob_bytes, boff, blen, n_obj, Widths{wa, wk, wv}, A, R, nullptr, nullptr, nullptr, 0u, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_mvreg_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                                uint64_t n_obj, uint32_t wa, uint32_t wv, uint32_t A, uint32_t* outn, uint64_t* outclk,
                                uint64_t* outval, uint32_t cap, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  hipLaunchKernelGGL((map_bincode_ingest_kernel<false>), dim3(grid_for(n_obj, 5u)), dim3(kW * kWaves), 0, stream,
                     blobs, blob_bytes, boff, blen, n_obj, Widths{wa, 1u, wv}, A, kNoSlab, outn, outclk, outval, cap,
                     status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_map_bincode_egest(const crdt_map_mvreg_slab& S, uint64_t n_obj, uint32_t A, uint32_t wa, uint32_t wk,
                             uint32_t wv, uint64_t* sizes, uint8_t* out, const uint64_t* ooff, uint64_t out_bytes,
                             int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const dim3 grid(grid_for(n_obj, 8u)), block(kW * kWaves);
  const Widths W{wa, wk, wv};
  if (out)
    hipLaunchKernelGGL((map_bincode_egest_kernel<true, true>), grid, block, 0, stream, S, nullptr, nullptr, nullptr, 0u,
                       n_obj, W, A, nullptr, out, ooff, out_bytes, status);
  else
    hipLaunchKernelGGL((map_bincode_egest_kernel<true, false>), grid, block, 0, stream, S, nullptr, nullptr, nullptr,
                       0u, n_obj, W, A, sizes, nullptr, nullptr, 0u, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_mvreg_bincode_egest(const uint32_t* sn, const uint64_t* sclk, const uint64_t* sval, uint32_t cap,
                               uint64_t n_obj, uint32_t A, uint32_t wa, uint32_t wv, uint64_t* sizes, uint8_t* out,
                               const uint64_t* ooff, uint64_t out_bytes, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const dim3 grid(grid_for(n_obj, 8u)), block(kW * kWaves);
  const Widths W{wa, 1u, wv};
  if (out)
    hipLaunchKernelGGL((map_bincode_egest_kernel<false, true>), grid, block, 0, stream, kNoSlab, sn, sclk, sval, cap,
                       n_obj, W, A, nullptr, out, ooff, out_bytes, status);
  else
    hipLaunchKernelGGL((map_bincode_egest_kernel<false, false>), grid, block, 0, stream, kNoSlab, sn, sclk, sval, cap,
                       n_obj, W, A, sizes, nullptr, nullptr, 0u, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

namespace {
template <class SLAB>
int nested_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                  uint64_t n_obj, NWidths W, uint32_t A, const SLAB& R, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  // 48 KB of LDS per block: three blocks per CU
  hipLaunchKernelGGL((nested_bincode_ingest_kernel<SLAB>), dim3(grid_for(n_obj, 3u)), dim3(kW * kWaves), 0, stream,
                     blobs, blob_bytes, boff, blen, n_obj, W, A, R, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}
template <class SLAB>
int nested_egest(const SLAB& S, uint64_t n_obj, NWidths W, uint32_t A, uint64_t* sizes, uint8_t* out,
                 const uint64_t* ooff, uint64_t out_bytes, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const dim3 grid(grid_for(n_obj, 8u)), block(kW * kWaves);
  if (out)
    hipLaunchKernelGGL((nested_bincode_egest_kernel<SLAB, true>), grid, block, 0, stream, S, n_obj, W, A, nullptr, out,
                       ooff, out_bytes, status);
  else
    hipLaunchKernelGGL((nested_bincode_egest_kernel<SLAB, false>), grid, block, 0, stream, S, n_obj, W, A, sizes,
                       nullptr, nullptr, 0u, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}
}  // namespace

int launch_map_orswot_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                     const uint64_t* blen, uint64_t n_obj, uint32_t wa, uint32_t wk, uint32_t wm,
                                     uint32_t A, const crdt_map_orswot_slab& R, int* status, hipStream_t stream) {
  return nested_ingest(blobs, blob_bytes, boff, blen, n_obj, NWidths{wa, wk, wm, 1u}, A, R, status, stream);
}

int launch_map_orswot_bincode_egest(const crdt_map_orswot_slab& S, uint64_t n_obj, uint32_t A, uint32_t wa,
                                    uint32_t wk, uint32_t wm, uint64_t* sizes, uint8_t* out, const uint64_t* ooff,
                                    uint64_t out_bytes, int* status, hipStream_t stream) {
  return nested_egest(S, n_obj, NWidths{wa, wk, wm, 1u}, A, sizes, out, ooff, out_bytes, status, stream);
}

int launch_map_map_bincode_ingest(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                  const uint64_t* blen, uint64_t n_obj, uint32_t wa, uint32_t wk, uint32_t wk2,
                                  uint32_t wv, uint32_t A, const crdt_map_map_slab& R, int* status,
                                  hipStream_t stream) {
  return nested_ingest(blobs, blob_bytes, boff, blen, n_obj, NWidths{wa, wk, wk2, wv}, A, R, status, stream);
}

int launch_map_map_bincode_egest(const crdt_map_map_slab& S, uint64_t n_obj, uint32_t A, uint32_t wa, uint32_t wk,
                                 uint32_t wk2, uint32_t wv, uint64_t* sizes, uint8_t* out, const uint64_t* ooff,
                                 uint64_t out_bytes, int* status, hipStream_t stream) {
  return nested_egest(S, n_obj, NWidths{wa, wk, wk2, wv}, A, sizes, out, ooff, out_bytes, status, stream);
}

}  // namespace crdts_hip
