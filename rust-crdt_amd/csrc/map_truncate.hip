// Causal::truncate of the three Map types (src/map.rs:131-158), batched:
// out[i] = self[i] after Map::truncate(clock[i]) (include/crdts_hip.h,
// crdt_map_mvreg_truncate / crdt_map_orswot_truncate / crdt_map_map_truncate).
//
// Reference: every entry clock loses T (VClock::subtract, src/vclock.rs:
// 236-242); an emptied entry is dropped, any other value takes its own
// truncate(T) — MVReg (src/mvreg.rs:100-113), Orswot (src/orswot.rs:159-172)
// or the nested Map; every deferred clock loses T, an emptied one is dropped
// and the rest are re-inserted (a HashMap in the reference: here back in CLOCK
// ORDER, and where two become equal the later one's key set, CLOCK ORDER
// before the subtract, is kept); the map clock loses T. No apply_deferred.
//
// One wave per object; lane = actor slot (map_rows.h). Every kernel is one
// fused pass: self's used slots are read once and only the survivors are
// written, at out slot w <= source slot k.
//  - Map<u64, MVReg>: map_truncate_to (map_mvreg_ws.h, on map_wave.h's toolkit).
//  - Map<u64, Orswot>: each surviving key's set is staged in the LDS workspace
//    (map_orswot_ws.h), truncated there by ws_truncate and written to slot w.
//  - the nested map, two launches (after map_map_apply.hip): (1) the outer
//    arrays, one wave per object, which leaves per out key slot the self inner
//    row it holds; (2) one wave per out key slot: map_truncate_to of that
//    inner row by the object's clock row.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/crdts_hip.h"
#include "kernels.h"
#include "map_limits.h"
#include "map_mvreg_ws.h"
#include "map_orswot_ws.h"
#include "map_rows.h"
#include "map_wave.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace maprow;  // rows (map_rows.h) and the wave toolkit with DefRef (map_wave.h)

constexpr uint64_t kSrcNone = ~0ull;  // an unused out key slot: no task
// (self's deferred capacity is within its side limit, map_limits.h: the `ord` arrays)
static_assert(kMapMapDcap <= kMapMvregDcap, "the nested map's outer and inner lists share the kernels' ord[]");

// TASKS (the nested map's second launch): n tasks, task t truncates S row
// src[t] (kSrcNone: none) into R row t by clock row t / slots.
template <int NS, bool TASKS>
__global__ __launch_bounds__(kW) void map_mvreg_truncate_kernel(crdt_map_mvreg_slab S,
                                                                const uint64_t* __restrict__ clk,
                                                                crdt_map_mvreg_slab R, uint64_t n, uint32_t A,
                                                                int* __restrict__ status, uint32_t* __restrict__ ctl,
                                                                const uint64_t* __restrict__ src, uint32_t slots) {
  __shared__ uint32_t ord[kMapMvregDcap];  // the deferred survivors' order
  const uint32_t lane = threadIdx.x;
  // (sched.h; TASKS: most tasks are empty slots, a plain stride balances them)
  typename std::conditional<TASKS, GridStride, BlockTickets<4>>::type sched(n, ctl + 3, lane);
  for (uint64_t t = sched.first(); t < n; t = sched.next(t)) {
    const uint64_t s = TASKS ? uni64(src[t]) : t;
    if (TASKS && s == kSrcNone) continue;
    const Row<NS> T = rowv<NS>(clk, TASKS ? t / slots : t, A, lane);
    if (!mapws::map_truncate_to<NS>(S, s, R, t, T, ord, A, lane) && lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
  }
}

// The nested map's outer arrays: out[i]'s keys, entry clocks, deferred removes
// and clock, and src[i * R.kcap + w] = the self inner row out key slot w holds.
template <int NS>
__global__ __launch_bounds__(kW) void map_map_truncate_outer_kernel(crdt_map_map_slab S,
                                                                    const uint64_t* __restrict__ clk,
                                                                    crdt_map_map_slab R, uint64_t* __restrict__ src,
                                                                    uint64_t n_obj, uint32_t A,
                                                                    int* __restrict__ status,
                                                                    uint32_t* __restrict__ ctl) {
  __shared__ uint32_t ord[kMapMvregDcap];  // the deferred survivors' order
  const uint32_t lane = threadIdx.x;
  const uint64_t Rk = R.kcap;
  BlockTickets<4> sched(n_obj, ctl + 3, lane);
  for (uint64_t i = sched.first(); i < n_obj; i = sched.next(i)) {
    uint64_t* const tsrc = src + i * Rk;
    const uint32_t nS = uni32(S.n_keys[i]), dS = uni32(S.n_def[i]);
    bool bad = nS > S.kcap || dS > S.dcap;
    if (!bad) {
      bool b = false;
      for (uint32_t d = lane; d < dS; d += kW) b = b || S.dset_n[i * S.dcap + d] > S.scap;
      bad = __ballot(b) != 0ull;
    }
    uint32_t w = 0;
    if (bad) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
    } else {
      const Row<NS> T = rowv<NS>(clk, i, A, lane);
      const uint64_t* const skeys = S.keys + i * S.kcap;
      const uint64_t* const secl = S.eclock + i * S.kcap * A;
      uint64_t* const keys = R.keys + i * Rk;
      uint64_t* const ecl = R.eclock + i * Rk * A;
      const uint64_t kreg = lane < nS ? skeys[lane] : 0ull;  // lane k: key k (the first 64)
      for (uint32_t k = 0; k < nS; ++k) {
        const Row<NS> ec = vsub(ldrow<NS>(secl + (uint64_t)k * A, A, lane), T);
        if (!vany(ec)) continue;
        strow<NS>(ecl + (uint64_t)w * A, ec, A, lane);
        const uint64_t key = k < kW ? lane64(kreg, k) : uni64(skeys[k]);
        if (lane == 0u) {
          keys[w] = key;
          tsrc[w] = i * S.kcap + k;
        }
        ++w;
      }
      const DefRef def = def_ref(R, i, A);
      const uint32_t wd = mapws::def_truncate_to<NS>(S.dclock + i * S.dcap * A, S.dset_n + i * S.dcap,
                                                     S.dset + i * S.dcap * S.scap, S.scap, dS, def, T, ord, A, lane);
      strow<NS>(R.clock + i * A, vsub(rowv<NS>(S.clock, i, A, lane), T), A, lane);
      if (lane == 0u) {
        R.n_keys[i] = w;
        R.n_def[i] = wd;
      }
    }
    // the slots past the kept keys hold no task (a rejected object: none at all);
    // slots below w are lane 0's
    for (uint32_t k = w + lane; k < Rk; k += kW) tsrc[k] = kSrcNone;
  }
}

// Map<u64, Orswot>: the workspace is one nested set of self's capacities.
template <int NS>
__global__ __launch_bounds__(kW) void map_orswot_truncate_kernel(crdt_map_orswot_slab S,
                                                                         const uint64_t* __restrict__ clk,
                                                                         crdt_map_orswot_slab R, uint64_t n_obj,
                                                                         uint32_t A, int* __restrict__ status,
                                                                         uint32_t* __restrict__ ctl) {
  extern __shared__ uint64_t mt_lds[];
  __shared__ uint32_t ord[kMapOrswotDcap];  // the map deferred survivors' order
  const uint32_t lane = threadIdx.x;
  const uint64_t Sk = S.kcap, Sm = S.mcap, Sv = S.vdcap, Svs = S.vscap;
  const uint64_t Rk = R.kcap, Rm = R.mcap, Rv = R.vdcap, Rvs = R.vscap;
  const mows::Caps c{S.mcap, S.vdcap, S.vscap, A};
  mows::Ws W;
  W.key = mt_lds;
  W.row = W.key + Sm;
  W.dclk = W.row + Sm * A;
  W.dset = W.dclk + Sv * A;
  W.sw = S.vscap;
  W.dn = (uint32_t*)(W.dset + Sv * Svs);
  W.nm = W.nd = 0u;
  uint32_t* const ddead = W.dn + Sv;
  uint32_t* const mdead = ddead + Sv;
  for (uint32_t j = lane; j < S.vdcap + S.mcap; j += kW) ddead[j] = 0u;
  sync();
  BlockTickets<4> sched(n_obj, ctl + 3, lane);
  for (uint64_t i = sched.first(); i < n_obj; i = sched.next(i)) {
    // ---- the input row, checked as the merge checks it (map_orswot.hip)
    const uint32_t nS = uni32(S.n_keys[i]), dS = uni32(S.n_def[i]);
    if (nS > S.kcap || dS > S.dcap) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    const bool ls = lane < nS;
    const uint32_t vmS = ls ? S.vn_mem[i * Sk + lane] : 0u, vdS = ls ? S.vn_def[i * Sk + lane] : 0u;
    bool bad = vmS > S.mcap || vdS > S.vdcap;
    for (uint32_t d = 0; !bad && d < vdS; ++d) bad = S.vdset_n[(i * Sk + lane) * Sv + d] > S.vscap;
    for (uint32_t k = kW + lane; k < nS; k += kW) {
      const uint64_t ki = i * Sk + k;
      bad = bad || S.vn_mem[ki] > S.mcap || S.vn_def[ki] > S.vdcap;
      for (uint32_t d = 0; !bad && d < S.vn_def[ki]; ++d) bad = S.vdset_n[ki * Sv + d] > S.vscap;
    }
    for (uint32_t d = lane; d < dS; d += kW) bad = bad || S.dset_n[i * S.dcap + d] > S.scap;
    if (__ballot(bad) != 0ull) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    const Row<NS> T = rowv<NS>(clk, i, A, lane);
    const uint64_t kreg = ls ? S.keys[i * Sk + lane] : 0ull;  // lane k: key k (the first 64)
    uint32_t w = 0;
    for (uint32_t k = 0; k < nS; ++k) {
      const uint64_t sk = i * Sk + k, rw = i * Rk + w;
      const Row<NS> ec = vsub(rowv<NS>(S.eclock, sk, A, lane), T);
      if (!vany(ec)) continue;
      // ---- the key's set into the workspace (its used slots)
      Row<NS> vc = rowv<NS>(S.vclock, sk, A, lane);
      W.nm = k < kW ? (uint32_t)__builtin_amdgcn_readlane(vmS, k) : uni32(S.vn_mem[sk]);
      W.nd = k < kW ? (uint32_t)__builtin_amdgcn_readlane(vdS, k) : uni32(S.vn_def[sk]);
      for (uint32_t e = lane; e < W.nm; e += kW) W.key[e] = S.vmem[sk * Sm + e];
      for (uint32_t e = lane; e < W.nm * A; e += kW) W.row[e] = S.vmclock[sk * Sm * A + e];
      for (uint32_t e = lane; e < W.nd * A; e += kW) W.dclk[e] = S.vdclock[sk * Sv * A + e];
      for (uint32_t e = lane; e < W.nd; e += kW) W.dn[e] = S.vdset_n[sk * Sv + e];
      for (uint32_t e = lane; e < W.nd * W.sw; e += kW) {
        const uint32_t d = e / W.sw;
        if (e - d * W.sw < S.vdset_n[sk * Sv + d]) W.dset[e] = S.vdset[sk * Sv * Svs + e];
      }
      sync();
      mows::ws_truncate<NS>(W, vc, T, mdead, ddead, c, lane);
      // ---- out key slot w
      strow<NS>(R.eclock + rw * A, ec, A, lane);
      strow<NS>(R.vclock + rw * A, vc, A, lane);
      const uint64_t key = k < kW ? lane64(kreg, k) : uni64(S.keys[sk]);
      if (lane == 0u) {
        R.keys[rw] = key;
        R.vn_mem[rw] = W.nm;
        R.vn_def[rw] = W.nd;
      }
      for (uint32_t e = lane; e < W.nm; e += kW) R.vmem[rw * Rm + e] = W.key[e];
      for (uint32_t e = lane; e < W.nm * A; e += kW) R.vmclock[rw * Rm * A + e] = W.row[e];
      for (uint32_t e = lane; e < W.nd * A; e += kW) R.vdclock[rw * Rv * A + e] = W.dclk[e];
      for (uint32_t e = lane; e < W.nd; e += kW) R.vdset_n[rw * Rv + e] = W.dn[e];
      for (uint32_t e = lane; e < W.nd * W.sw; e += kW) {
        const uint32_t d = e / W.sw, o = e - d * W.sw;
        if (o < W.dn[d]) R.vdset[(rw * Rv + d) * Rvs + o] = W.dset[e];
      }
      sync();  // the next key's stage overwrites what other lanes read here
      ++w;
    }
    const DefRef def = def_ref(R, i, A);
    const uint32_t wd = mapws::def_truncate_to<NS>(S.dclock + i * S.dcap * A, S.dset_n + i * S.dcap,
                                                   S.dset + i * S.dcap * S.scap, S.scap, dS, def, T, ord, A, lane);
    strow<NS>(R.clock + i * A, vsub(rowv<NS>(S.clock, i, A, lane), T), A, lane);
    if (lane == 0u) {
      R.n_keys[i] = w;
      R.n_def[i] = wd;
    }
  }
}

uint32_t grid_cap() {
  return (uint32_t)cu_count() * 28u;  // 7 single-wave blocks per SIMD, as the merges launch
}

}  // namespace

int launch_map_mvreg_truncate(const crdt_map_mvreg_slab& S, const uint64_t* clk, const crdt_map_mvreg_slab& R,
                              uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  if (hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), stream) != hipSuccess) return CRDT_EHIP;  // ctl[3]: tickets
  const uint64_t cap = grid_cap();
  const uint32_t blocks = (uint32_t)(n_obj < cap ? n_obj : cap);
  if (A > 64u)  // 65-128 actors: two slots per lane
    hipLaunchKernelGGL((map_mvreg_truncate_kernel<2, false>), dim3(blocks), dim3(kW), 0, stream, S, clk, R, n_obj, A,
                       status, ctl, nullptr, 1u);
  else
    hipLaunchKernelGGL((map_mvreg_truncate_kernel<1, false>), dim3(blocks), dim3(kW), 0, stream, S, clk, R, n_obj, A,
                       status, ctl, nullptr, 1u);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

// the scratch: per out key slot, the self inner row it holds
size_t map_map_truncate_scratch_bytes(const crdt_map_map_slab& R, uint64_t n_obj, uint32_t) {
  return (size_t)(n_obj * R.kcap * sizeof(uint64_t)) + 16u;
}

int launch_map_map_truncate(const crdt_map_map_slab& S, const uint64_t* clk, const crdt_map_map_slab& R,
                            uint64_t n_obj, uint32_t A, uint8_t* scratch, int* status, uint32_t* ctl,
                            hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  uint64_t* const src = (uint64_t*)scratch;
  if (hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), stream) != hipSuccess) return CRDT_EHIP;  // ctl[3]: tickets
  const uint64_t cap = grid_cap();
  uint32_t blocks = (uint32_t)(n_obj < cap ? n_obj : cap);
  if (A > 64u)
    hipLaunchKernelGGL((map_map_truncate_outer_kernel<2>), dim3(blocks), dim3(kW), 0, stream, S, clk, R, src, n_obj, A,
                       status, ctl);
  else
    hipLaunchKernelGGL((map_map_truncate_outer_kernel<1>), dim3(blocks), dim3(kW), 0, stream, S, clk, R, src, n_obj, A,
                       status, ctl);
  if (hipGetLastError() != hipSuccess) return CRDT_EHIP;
  const uint64_t nt = n_obj * R.kcap;
  blocks = coprime_grid((uint32_t)(nt < cap ? nt : cap), R.kcap);  // (sched.h)
  if (A > 64u)
    hipLaunchKernelGGL((map_mvreg_truncate_kernel<2, true>), dim3(blocks), dim3(kW), 0, stream, S.inner, clk, R.inner,
                       nt, A, status, ctl, src, R.kcap);
  else
    hipLaunchKernelGGL((map_mvreg_truncate_kernel<1, true>), dim3(blocks), dim3(kW), 0, stream, S.inner, clk, R.inner,
                       nt, A, status, ctl, src, R.kcap);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_map_orswot_truncate(const crdt_map_orswot_slab& S, const uint64_t* clk, const crdt_map_orswot_slab& R,
                               uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const size_t lds = map_orswot_apply_lds_bytes(S, A);  // one nested set of self's capacities
  if (lds > kMapOrswotApplyLdsMax) return CRDT_EINVAL;
  const void* fn = A > 64u ? (const void*)map_orswot_truncate_kernel<2> : (const void*)map_orswot_truncate_kernel<1>;
  int occ = 0;
  // one single-wave block per resident slot (the workspace sizes it)
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, kW, lds) != hipSuccess || occ < 1) occ = 16;
  const uint64_t cap = (uint64_t)cu_count() * (uint32_t)occ;
  const uint32_t blocks = (uint32_t)(n_obj < cap ? n_obj : cap);
  if (hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), stream) != hipSuccess) return CRDT_EHIP;  // ctl[3]: tickets
  void* args[] = {(void*)&S, (void*)&clk, (void*)&R, &n_obj, &A, &status, &ctl};
  if (hipLaunchKernel(fn, dim3(blocks), dim3(kW), args, lds, stream) != hipSuccess) return CRDT_EHIP;
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
