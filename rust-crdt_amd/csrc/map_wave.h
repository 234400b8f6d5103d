// The slab-edit toolkit of the Map kernels (internal): what one wave needs to
// edit the sorted arrays of a Map slab row in place — lane-0 reads, block
// copies, one-slot shifts, the key search, and a map's deferred removes
// (clocks in CLOCK ORDER with their key sets). Lane = actor slot (map_rows.h);
// the wave fence, the uniform and cross-lane reads and kW are wave.h's, seen
// through namespace maprow. Used by map_mvreg_ws.h, map_orswot_ws.h, map_ops.h
// and the apply / truncate kernels built on them.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "map_rows.h"

namespace crdts_hip {
namespace maprow {

// a value only lane 0 ever touches
__device__ __forceinline__ uint32_t cnt0(const uint32_t* p, uint32_t lane) {
  uint32_t x = 0u;
  if (lane == 0u) x = *p;
  return uni32(x);
}
__device__ __forceinline__ uint64_t val0(const uint64_t* p, uint32_t lane) {
  uint64_t x = 0ull;
  if (lane == 0u) x = *p;
  return uni64(x);
}
// n elements, lane l moving offsets l, l + 64, ...
template <class T>
__device__ __forceinline__ void copy_n(T* dst, const T* src, uint32_t n, uint32_t lane) {
  for (uint32_t e = lane; e < n; e += kW) dst[e] = src[e];
}
// a[k + 1] = a[k] for k in [p, n), the last 64 first; a[k - 1] = a[k] for k in
// (p, n), the first 64 first: a chunk's loads are all done before its stores
__device__ inline void shift_up(uint64_t* a, uint32_t p, uint32_t n, uint32_t lane) {
  for (uint32_t hi = n; hi > p;) {
    const uint32_t lo = hi - p > kW ? hi - kW : p;
    const uint32_t k = lo + lane;
    uint64_t x = 0ull;
    if (k < hi) x = a[k];
    sync();
    if (k < hi) a[k + 1u] = x;
    sync();
    hi = lo;
  }
}
__device__ inline void shift_down(uint64_t* a, uint32_t p, uint32_t n, uint32_t lane) {
  for (uint32_t lo = p + 1u; lo < n; lo += kW) {
    const uint32_t k = lo + lane;
    uint64_t x = 0ull;
    if (k < n) x = a[k];
    sync();
    if (k < n) a[k - 1u] = x;
    sync();
  }
}
// `key` in the ascending a[0, n): pos = how many are below it; is it there?
__device__ inline bool find_key(const uint64_t* a, uint32_t n, uint64_t key, uint32_t lane, uint32_t& pos) {
  uint32_t below = 0u;
  bool hit = false;
  for (uint32_t b = 0u; b < n; b += kW) {
    const uint32_t k = b + lane;
    const uint64_t x = k < n ? a[k] : ~0ull;
    below += (uint32_t)__popcll(__ballot(k < n && x < key));
    hit = hit || __ballot(k < n && x == key) != 0ull;
  }
  pos = below;
  return hit;
}

// ---- the deferred removes of one map: clocks [Rd][A] in CLOCK ORDER, their
// key sets [Rd][Rs] ascending (an outer map's or an inner map's alike)
struct DefRef {
  uint64_t* dcl;
  uint32_t* dsn;
  uint64_t* dse;
  uint32_t Rd, Rs;
};
// row i's list in a slab (any of the three Map slab types: the fields have one name)
template <class Slab>
__device__ __forceinline__ DefRef def_ref(const Slab& R, uint64_t i, uint32_t A) {
  return DefRef{R.dclock + i * R.dcap * A, R.dset_n + i * R.dcap, R.dset + i * R.dcap * R.scap, R.dcap, R.scap};
}
// entry src -> slot dst (dst != src)
template <int NS>
__device__ inline void def_move(const DefRef& d, uint32_t dst, uint32_t src, uint32_t A, uint32_t lane) {
  const uint32_t sn = cnt0(d.dsn + src, lane);
  strow<NS>(d.dcl + (uint64_t)dst * A, ldrow<NS>(d.dcl + (uint64_t)src * A, A, lane), A, lane);
  copy_n(d.dse + (uint64_t)dst * d.Rs, d.dse + (uint64_t)src * d.Rs, sn, lane);
  if (lane == 0u) d.dsn[dst] = sn;
}
template <int NS>
__device__ inline void def_swap(const DefRef& d, uint32_t p, uint32_t q, uint32_t A, uint32_t lane) {
  const uint32_t np = cnt0(d.dsn + p, lane), nq = cnt0(d.dsn + q, lane);
  const Row<NS> rp = ldrow<NS>(d.dcl + (uint64_t)p * A, A, lane), rq = ldrow<NS>(d.dcl + (uint64_t)q * A, A, lane);
  strow<NS>(d.dcl + (uint64_t)p * A, rq, A, lane);
  strow<NS>(d.dcl + (uint64_t)q * A, rp, A, lane);
  uint64_t* const sp = d.dse + (uint64_t)p * d.Rs;
  uint64_t* const sq = d.dse + (uint64_t)q * d.Rs;
  for (uint32_t e = lane; e < (np > nq ? np : nq); e += kW) {  // both counts <= Rs
    const uint64_t x = sp[e], y = sq[e];
    sp[e] = y;
    sq[e] = x;
  }
  if (lane == 0u) {
    d.dsn[p] = nq;
    d.dsn[q] = np;
  }
}
// apply_rm's deferral (src/map.rs:337-341) of a clock the map clock does not
// cover: the key joins an equal clock's set, or a new entry is inserted at its
// CLOCK ORDER place. 0, or CRDT_ECAPACITY.
template <int NS>
__device__ inline int def_insert(const DefRef& d, uint32_t& nd, uint64_t key, const Row<NS>& C, uint32_t A,
                                 uint32_t lane) {
  uint32_t at = nd;
  bool eq = false;
  for (uint32_t e = 0; e < nd; ++e) {
    const int o = vorder(C, ldrow<NS>(d.dcl + (uint64_t)e * A, A, lane), lane);
    if (o > 0) continue;
    at = e;
    eq = o == 0;
    break;
  }
  if (eq) {
    uint64_t* const set = d.dse + (uint64_t)at * d.Rs;
    const uint32_t sn = cnt0(d.dsn + at, lane);
    uint32_t p;
    if (!find_key(set, sn, key, lane, p)) {
      if (sn >= d.Rs) return CRDT_ECAPACITY;
      shift_up(set, p, sn, lane);
      if (lane == 0u) {
        set[p] = key;
        d.dsn[at] = sn + 1u;
      }
    }
  } else {
    if (nd >= d.Rd) return CRDT_ECAPACITY;
    for (uint32_t e = nd; e-- > at;) def_move<NS>(d, e + 1u, e, A, lane);  // entries from `at` one slot up, last first
    // lane 0 writes the new set's only element: offset 0 is lane 0's in copy_n
    strow<NS>(d.dcl + (uint64_t)at * A, C, A, lane);
    if (lane == 0u) {
      d.dse[(uint64_t)at * d.Rs] = key;
      d.dsn[at] = 1u;
    }
    ++nd;
  }
  sync();
  return 0;
}

}  // namespace maprow
}  // namespace crdts_hip
