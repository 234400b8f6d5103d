// One Map<u64, MVReg<u64, A>, A> row edited in place by one wave (internal):
// the per-op edits of Map::apply (src/map.rs:160-190) and Map::truncate
// (:131-158) as device functions over (slab, row), for the kernels that hold
// such a map as a value — the nested map's op path (map_map_apply.hip), whose
// inner maps are rows of a scratch slab.
//
// Lane = actor slot (map_rows.h). A row's arrays are touched under fixed lane
// mappings: a clock row by the lane of its actor slot (ldrow / strow); a
// block of elements by lane e % 64 (copy_n); the per-key / per-entry counts
// (mv_n, dset_n) and single values by lane 0. An address is used under one
// mapping between two sync() and every edit ends in one, so a lane's own
// program order covers the rest. keys[] and dset[] are searched by all lanes.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "map_rows.h"
#include "map_wave.h"

namespace crdts_hip {
namespace mapws {

using namespace maprow;  // Row<NS>, and the wave-edit toolkit with DefRef (map_wave.h)

// ---- one Map<u64, MVReg> row of a slab, and its state held in registers
struct MapRef {
  uint64_t* clock;
  uint32_t* n_keys;
  uint32_t* n_def;
  uint64_t* keys;
  uint64_t* ecl;
  uint32_t* mvn;
  uint64_t* mvc;
  uint64_t* mvv;
  DefRef def;
  uint32_t Rk, Rm;
};
template <int NS>
struct MapSt {
  Row<NS> cM;
  uint32_t nk, nd;
};
__device__ __forceinline__ MapRef map_ref(const crdt_map_mvreg_slab& R, uint64_t row, uint32_t A) {
  MapRef m;
  m.clock = R.clock + row * A;
  m.n_keys = R.n_keys + row;
  m.n_def = R.n_def + row;
  m.keys = R.keys + row * R.kcap;
  m.ecl = R.eclock + row * R.kcap * A;
  m.mvn = R.mv_n + row * R.kcap;
  m.mvc = R.mv_clock + row * R.kcap * R.mcap * A;
  m.mvv = R.mv_val + row * R.kcap * R.mcap;
  m.def = def_ref(R, row, A);
  m.Rk = R.kcap;
  m.Rm = R.mcap;
  return m;
}
template <int NS>
__device__ inline MapSt<NS> map_open(const MapRef& m, uint32_t A, uint32_t lane) {
  MapSt<NS> st;
  st.cM = ldrow<NS>(m.clock, A, lane);
  st.nk = cnt0(m.n_keys, lane);
  st.nd = cnt0(m.n_def, lane);
  return st;
}
template <int NS>
__device__ inline void map_close(const MapRef& m, const MapSt<NS>& st, uint32_t A, uint32_t lane) {
  strow<NS>(m.clock, st.cM, A, lane);
  if (lane == 0u) {
    *m.n_keys = st.nk;
    *m.n_def = st.nd;
  }
  sync();
}
// an empty map in row `m`
template <int NS>
__device__ inline void map_clear(const MapRef& m, uint32_t A, uint32_t lane) {
  MapSt<NS> st;
  st.cM = zrow<NS>();
  st.nk = st.nd = 0u;
  map_close<NS>(m, st, A, lane);
}

// Row srow of S -> row rrow of R, used slots only (R's capacities >= S's).
// false, and nothing written, for a row the merge rejects (a count above its
// capacity). Ends in sync().
__device__ inline bool map_copy_row(const crdt_map_mvreg_slab& S, uint64_t srow, const crdt_map_mvreg_slab& R,
                                    uint64_t rrow, uint32_t A, uint32_t lane) {
  const uint32_t nS = uni32(S.n_keys[srow]), dS = uni32(S.n_def[srow]);
  if (nS > S.kcap || dS > S.dcap) return false;
  const uint32_t vnS = lane < nS ? S.mv_n[srow * S.kcap + lane] : 0u;
  const uint32_t dnS = lane < dS ? S.dset_n[srow * S.dcap + lane] : 0u;
  bool bad = vnS > S.mcap || dnS > S.scap;
  for (uint32_t k = lane + kW; k < nS; k += kW) bad = bad || S.mv_n[srow * S.kcap + k] > S.mcap;
  for (uint32_t d = lane + kW; d < dS; d += kW) bad = bad || S.dset_n[srow * S.dcap + d] > S.scap;
  if (__ballot(bad) != 0ull) return false;
  const MapRef m = map_ref(R, rrow, A);
  copy_n(m.clock, S.clock + srow * A, A, lane);
  copy_n(m.keys, S.keys + srow * S.kcap, nS, lane);
  copy_n(m.ecl, S.eclock + srow * S.kcap * A, nS * A, lane);
  for (uint32_t k = 0; k < nS; ++k) {
    const uint64_t sk = srow * S.kcap + k;
    const uint32_t n = k < kW ? (uint32_t)__builtin_amdgcn_readlane(vnS, k) : uni32(S.mv_n[sk]);
    if (lane == 0u) m.mvn[k] = n;
    copy_n(m.mvc + (uint64_t)k * m.Rm * A, S.mv_clock + sk * S.mcap * A, n * A, lane);
    copy_n(m.mvv + (uint64_t)k * m.Rm, S.mv_val + sk * S.mcap, n, lane);
  }
  copy_n(m.def.dcl, S.dclock + srow * S.dcap * A, dS * A, lane);
  for (uint32_t d = 0; d < dS; ++d) {
    const uint64_t sd = srow * S.dcap + d;
    const uint32_t sn = d < kW ? (uint32_t)__builtin_amdgcn_readlane(dnS, d) : uni32(S.dset_n[sd]);
    if (lane == 0u) m.def.dsn[d] = sn;
    copy_n(m.def.dse + (uint64_t)d * m.def.Rs, S.dset + sd * S.scap, sn, lane);
  }
  if (lane == 0u) {
    *m.n_keys = nS;
    *m.n_def = dS;
  }
  sync();
  return true;
}

// apply_rm's entry edit (src/map.rs:343-349): the key's entry clock loses D;
// an emptied entry is removed, else its register takes MVReg::truncate(D)
// (src/mvreg.rs:100-113, order kept)
template <int NS>
__device__ inline void map_rm_entry(const MapRef& m, MapSt<NS>& st, uint64_t key, const Row<NS>& D, uint32_t A,
                                    uint32_t lane) {
  const uint64_t Rm = m.Rm;
  uint32_t pos;
  if (!find_key(m.keys, st.nk, key, lane, pos)) return;
  const Row<NS> ec = vsub(ldrow<NS>(m.ecl + (uint64_t)pos * A, A, lane), D);
  if (!vany(ec)) {
    for (uint32_t k = pos + 1u; k < st.nk; ++k) {  // rows above it one slot down, first row first
      const uint32_t n = cnt0(m.mvn + k, lane);
      strow<NS>(m.ecl + (uint64_t)(k - 1u) * A, ldrow<NS>(m.ecl + (uint64_t)k * A, A, lane), A, lane);
      copy_n(m.mvc + (k - 1u) * Rm * A, m.mvc + k * Rm * A, n * A, lane);
      copy_n(m.mvv + (k - 1u) * Rm, m.mvv + k * Rm, n, lane);
      if (lane == 0u) m.mvn[k - 1u] = n;
    }
    shift_down(m.keys, pos, st.nk, lane);
    --st.nk;
  } else {
    strow<NS>(m.ecl + (uint64_t)pos * A, ec, A, lane);
    const uint32_t n = cnt0(m.mvn + pos, lane);
    uint64_t* const vc = m.mvc + pos * Rm * A;
    uint64_t* const vv = m.mvv + pos * Rm;
    uint32_t w = 0;
    for (uint32_t v = 0; v < n; ++v) {
      const Row<NS> r = vsub(ldrow<NS>(vc + (uint64_t)v * A, A, lane), D);
      if (!vany(r)) continue;
      strow<NS>(vc + (uint64_t)w * A, r, A, lane);
      if (lane == 0u && w != v) vv[w] = vv[v];
      ++w;
    }
    if (lane == 0u) m.mvn[pos] = w;
  }
  sync();
}

// Op::Rm -> apply_rm (src/map.rs:336-350). 0, or CRDT_ECAPACITY.
template <int NS>
__device__ inline int map_rm(const MapRef& m, MapSt<NS>& st, uint64_t key, const Row<NS>& C, uint32_t A,
                             uint32_t lane) {
  if (!vany(C)) return 0;  // empty <= every clock, and subtracts nothing
  if (!vle(C, st.cM)) {
    const int e = def_insert<NS>(m.def, st.nd, key, C, A, lane);
    if (e) return e;
  }
  map_rm_entry<NS>(m, st, key, C, A, lane);
  return 0;
}

// Op::Up { dot (da, dc), key, Put { C, val } } (src/map.rs:169-187, the Put:
// src/mvreg.rs:158-186), da < A. 0, or CRDT_ECAPACITY.
template <int NS>
__device__ inline int map_up(const MapRef& m, MapSt<NS>& st, uint32_t da, uint64_t dc, uint64_t key,
                             const Row<NS>& C, uint64_t val, uint32_t A, uint32_t lane) {
  const uint64_t Rm = m.Rm;
  const uint32_t ds = da >> 6, dl = da & 63u;
  uint64_t seen = 0ull;
  for (int s = 0; s < NS; ++s)
    if ((uint32_t)s == ds) seen = lane64(st.cM.v[s], dl);
  if (seen >= dc) return 0;  // the map has this dot: the whole op is skipped
  uint32_t pos;
  const bool found = find_key(m.keys, st.nk, key, lane, pos);
  if (!found) {
    if (st.nk >= m.Rk) return CRDT_ECAPACITY;
    for (uint32_t k = st.nk; k-- > pos;) {  // rows from pos one slot up, last row first
      const uint32_t n = cnt0(m.mvn + k, lane);
      strow<NS>(m.ecl + (uint64_t)(k + 1u) * A, ldrow<NS>(m.ecl + (uint64_t)k * A, A, lane), A, lane);
      copy_n(m.mvc + (k + 1u) * Rm * A, m.mvc + k * Rm * A, n * A, lane);
      copy_n(m.mvv + (k + 1u) * Rm, m.mvv + k * Rm, n, lane);
      if (lane == 0u) m.mvn[k + 1u] = n;
    }
    shift_up(m.keys, pos, st.nk, lane);
    if (lane == 0u) m.keys[pos] = key;
    ++st.nk;
  }
  Row<NS> ec = found ? ldrow<NS>(m.ecl + (uint64_t)pos * A, A, lane) : zrow<NS>();
  for (int s = 0; s < NS; ++s) {  // witness(dot) on the entry clock and on the map clock
    if ((uint32_t)s != ds || lane != dl) continue;
    ec.v[s] = ec.v[s] > dc ? ec.v[s] : dc;
    st.cM.v[s] = dc;
  }
  strow<NS>(m.ecl + (uint64_t)pos * A, ec, A, lane);
  uint32_t n = found ? cnt0(m.mvn + pos, lane) : 0u;
  if (vany(C)) {  // MVReg Put: drop the values the clock covers, append unless one is ahead
    uint64_t* const vc = m.mvc + pos * Rm * A;
    uint64_t* const vv = m.mvv + pos * Rm;
    uint32_t w = 0;
    bool ahead = false;
    for (uint32_t v = 0; v < n; ++v) {
      const Row<NS> r = ldrow<NS>(vc + (uint64_t)v * A, A, lane);
      if (vle(r, C)) continue;
      ahead = ahead || vstrict_less(C, r);
      if (w != v) {
        strow<NS>(vc + (uint64_t)w * A, r, A, lane);
        if (lane == 0u) vv[w] = vv[v];
      }
      ++w;
    }
    if (!ahead) {
      if (w >= m.Rm) return CRDT_ECAPACITY;
      strow<NS>(vc + (uint64_t)w * A, C, A, lane);
      if (lane == 0u) vv[w] = val;
      ++w;
    }
    n = w;
  }
  if (lane == 0u) m.mvn[pos] = n;
  sync();
  // apply_deferred (:325-333): every (clock, key) removed again; the clocks
  // the map clock still does not cover stay, with their sets (a subsequence
  // of a CLOCK ORDER list is in CLOCK ORDER)
  const DefRef& d = m.def;
  uint32_t w = 0;
  for (uint32_t e = 0; e < st.nd; ++e) {
    const Row<NS> D = ldrow<NS>(d.dcl + (uint64_t)e * A, A, lane);
    const uint32_t sn = cnt0(d.dsn + e, lane);
    for (uint32_t s = 0; s < sn; ++s) map_rm_entry<NS>(m, st, uni64(d.dse[(uint64_t)e * d.Rs + s]), D, A, lane);
    if (vle(D, st.cM)) continue;
    if (w != e) def_move<NS>(d, w, e, A, lane);
    ++w;
  }
  if (w != st.nd) sync();
  st.nd = w;
  return 0;
}

// Map::truncate(T) (src/map.rs:131-158): every entry clock loses T, an emptied
// entry is dropped, any other takes MVReg::truncate(T); every deferred clock
// loses T, an emptied one is dropped, the rest go back in CLOCK ORDER — where
// two become equal, the key set of the later one (CLOCK ORDER before the
// subtract) is kept, as crdt_map_map_merge does; the map clock loses T.
template <int NS>
__device__ inline void map_truncate(const MapRef& m, MapSt<NS>& st, const Row<NS>& T, uint32_t A, uint32_t lane) {
  const uint64_t Rm = m.Rm;
  uint32_t w = 0;
  for (uint32_t k = 0; k < st.nk; ++k) {  // entries compacted forwards: slot w <= k
    const Row<NS> ec = vsub(ldrow<NS>(m.ecl + (uint64_t)k * A, A, lane), T);
    if (!vany(ec)) continue;
    strow<NS>(m.ecl + (uint64_t)w * A, ec, A, lane);
    const uint32_t n = cnt0(m.mvn + k, lane);
    uint32_t wv = 0;
    for (uint32_t v = 0; v < n; ++v) {
      const Row<NS> r = vsub(ldrow<NS>(m.mvc + (k * Rm + v) * A, A, lane), T);
      if (!vany(r)) continue;
      strow<NS>(m.mvc + (w * Rm + wv) * A, r, A, lane);
      if (lane == 0u) m.mvv[w * Rm + wv] = m.mvv[k * Rm + v];
      ++wv;
    }
    if (lane == 0u) {
      m.mvn[w] = wv;
      if (w != k) m.keys[w] = m.keys[k];
    }
    ++w;
  }
  st.nk = w;
  const DefRef& d = m.def;
  uint32_t wd = 0;
  for (uint32_t e = 0; e < st.nd; ++e) {
    const Row<NS> D = vsub(ldrow<NS>(d.dcl + (uint64_t)e * A, A, lane), T);
    if (!vany(D)) continue;
    if (wd != e) def_move<NS>(d, wd, e, A, lane);
    strow<NS>(d.dcl + (uint64_t)wd * A, D, A, lane);
    // from slot wd down to its CLOCK ORDER place among the kept ones
    uint32_t p = wd;
    bool dup = false;
    while (p > 0u) {
      const int o = vorder(D, ldrow<NS>(d.dcl + (uint64_t)(p - 1u) * A, A, lane), lane);
      if (o > 0) break;
      if (o == 0) {
        dup = true;
        break;
      }
      def_swap<NS>(d, p, p - 1u, A, lane);
      --p;
    }
    if (dup) {  // its set replaces the equal clock's; the entries it passed go one slot down
      for (uint32_t q = p; q <= wd; ++q) def_move<NS>(d, q - 1u, q, A, lane);
    } else {
      ++wd;
    }
  }
  st.nd = wd;
  st.cM = vsub(st.cM, T);
  sync();
}

// ---- Map::truncate from one slab row into another (source != destination):
// the source's used slots are read once and only the survivors are written.

// The deferred part of Map::truncate(T) (src/map.rs:147-154): the n source
// entries (clocks sdcl[.][A] in CLOCK ORDER, set sizes sdsn, sets sdse[.][sRs])
// less T into the empty list `d` (d.Rd >= n, d.Rs >= sRs), by map_truncate's
// rule: an emptied clock is dropped, the rest go to their CLOCK ORDER place,
// and of two that become equal the later one (CLOCK ORDER before the
// subtract) stays. The order is worked out on source indices in `ord` (LDS, n
// slots; the wave's own) and every kept entry is then written once, its used
// slots only. Returns the count written. Every set size must be <= sRs. Ends
// in sync().
template <int NS>
__device__ inline uint32_t def_truncate_to(const uint64_t* sdcl, const uint32_t* sdsn, const uint64_t* sdse,
                                           uint32_t sRs, uint32_t n, const DefRef& d, const Row<NS>& T, uint32_t* ord,
                                           uint32_t A, uint32_t lane) {
  uint32_t wd = 0;
  sync();  // the previous list's readers of ord are done
  for (uint32_t e = 0; e < n; ++e) {
    const Row<NS> D = vsub(ldrow<NS>(sdcl + (uint64_t)e * A, A, lane), T);
    if (!vany(D)) continue;
    uint32_t p = wd;  // its place: above every kept clock it follows
    bool dup = false;
    while (p > 0u) {
      const uint32_t f = uni32(ord[p - 1u]);
      const int o = vorder(D, vsub(ldrow<NS>(sdcl + (uint64_t)f * A, A, lane), T), lane);
      if (o > 0) break;
      if (o == 0) {
        dup = true;
        break;
      }
      --p;
    }
    if (dup) {
      sync();
      if (lane == 0u) ord[p - 1u] = e;  // it takes the equal clock's place
    } else {
      for (uint32_t hi = wd; hi > p;) {  // the ones above it one slot up, the last 64 first
        const uint32_t lo = hi - p > kW ? hi - kW : p;
        const uint32_t k = lo + lane;
        uint32_t x = 0u;
        if (k < hi) x = ord[k];
        sync();
        if (k < hi) ord[k + 1u] = x;
        sync();
        hi = lo;
      }
      if (lane == 0u) ord[p] = e;
      ++wd;
    }
    sync();
  }
  for (uint32_t j = 0; j < wd; ++j) {
    const uint32_t e = uni32(ord[j]);
    const uint32_t sn = uni32(sdsn[e]);
    strow<NS>(d.dcl + (uint64_t)j * A, vsub(ldrow<NS>(sdcl + (uint64_t)e * A, A, lane), T), A, lane);
    copy_n(d.dse + (uint64_t)j * d.Rs, sdse + (uint64_t)e * sRs, sn, lane);
    if (lane == 0u) d.dsn[j] = sn;
  }
  sync();
  return wd;
}

// Row rrow of R = row srow of S after Map::truncate(T) (src/map.rs:131-158),
// R's capacities >= S's and R != S: map_truncate's forward compaction with the
// reads on S and the writes on R (slot w <= k), so nothing is written twice.
// `ord`: S.dcap LDS slots (def_truncate_to). false, and nothing written, for a
// row the merge rejects (a count above its capacity). Ends in sync().
template <int NS>
__device__ inline bool map_truncate_to(const crdt_map_mvreg_slab& S, uint64_t srow, const crdt_map_mvreg_slab& R,
                                       uint64_t rrow, const Row<NS>& T, uint32_t* ord, uint32_t A, uint32_t lane) {
  const uint32_t nS = uni32(S.n_keys[srow]), dS = uni32(S.n_def[srow]);
  if (nS > S.kcap || dS > S.dcap) return false;
  const uint32_t vnS = lane < nS ? S.mv_n[srow * S.kcap + lane] : 0u;
  const uint32_t dnS = lane < dS ? S.dset_n[srow * S.dcap + lane] : 0u;
  bool bad = vnS > S.mcap || dnS > S.scap;
  for (uint32_t k = lane + kW; k < nS; k += kW) bad = bad || S.mv_n[srow * S.kcap + k] > S.mcap;
  for (uint32_t d = lane + kW; d < dS; d += kW) bad = bad || S.dset_n[srow * S.dcap + d] > S.scap;
  if (__ballot(bad) != 0ull) return false;
  const MapRef m = map_ref(R, rrow, A);
  const uint64_t Rm = m.Rm, Sm = S.mcap;
  const uint64_t* const skeys = S.keys + srow * S.kcap;
  const uint64_t* const secl = S.eclock + srow * S.kcap * A;
  const uint64_t* const smvc = S.mv_clock + srow * S.kcap * Sm * A;
  const uint64_t* const smvv = S.mv_val + srow * S.kcap * Sm;
  const uint64_t kreg = lane < nS ? skeys[lane] : 0ull;  // lane k: key k (the first 64)
  uint32_t w = 0;
  for (uint32_t k = 0; k < nS; ++k) {
    const Row<NS> ec = vsub(ldrow<NS>(secl + (uint64_t)k * A, A, lane), T);
    if (!vany(ec)) continue;
    strow<NS>(m.ecl + (uint64_t)w * A, ec, A, lane);
    const uint32_t n = k < kW ? (uint32_t)__builtin_amdgcn_readlane(vnS, k) : uni32(S.mv_n[srow * S.kcap + k]);
    uint32_t wv = 0;
    for (uint32_t v = 0; v < n; ++v) {
      const Row<NS> r = vsub(ldrow<NS>(smvc + (k * Sm + v) * A, A, lane), T);
      if (!vany(r)) continue;
      strow<NS>(m.mvc + (w * Rm + wv) * A, r, A, lane);
      if (lane == 0u) m.mvv[w * Rm + wv] = smvv[k * Sm + v];
      ++wv;
    }
    const uint64_t key = k < kW ? lane64(kreg, k) : uni64(skeys[k]);
    if (lane == 0u) {
      m.mvn[w] = wv;
      m.keys[w] = key;
    }
    ++w;
  }
  const uint32_t wd = def_truncate_to<NS>(S.dclock + srow * S.dcap * A, S.dset_n + srow * S.dcap,
                                          S.dset + srow * S.dcap * S.scap, S.scap, dS, m.def, T, ord, A, lane);
  MapSt<NS> st;
  st.cM = vsub(ldrow<NS>(S.clock + srow * A, A, lane), T);
  st.nk = w;
  st.nd = wd;
  map_close<NS>(m, st, A, lane);
  return true;
}

}  // namespace mapws
}  // namespace crdts_hip
