// Map<u64, MVReg<u64, A>, A>::apply (CmRDT), batched: out[i] = self[i] after
// each of object i's ops in order (include/crdts_hip.h, crdt_map_mvreg_apply).
//
// Reference: Map::apply (src/map.rs:160-190) — Op::Nop; Op::Rm -> apply_rm
// (:336-350: defer a clock the map clock does not cover, subtract it from the
// key's entry clock, drop an emptied entry, else MVReg::truncate,
// src/mvreg.rs:100-113); Op::Up -> skipped when the map clock has the dot
// (:170-173), else the entry is taken out (or starts empty), witnesses the
// dot, takes the nested Put (MVReg::apply, src/mvreg.rs:158-186), goes back
// in, the map clock witnesses the dot and apply_deferred (:325-333) re-applies
// every deferred remove. With MVReg values every step of apply_deferred is a
// subtract and subtracts commute (map.hip), so the pass walks the deferred
// entries in slab order and keeps the clocks the map clock still does not
// cover — a subsequence of a CLOCK ORDER list is in CLOCK ORDER.
//
// One wave per object; lane = actor slot (map_rows.h). self[i]'s used slots
// are copied into out[i], which is then edited in place one op at a time, the
// map clock and the two counts held in registers. A key insert moves the used
// tail of keys / eclock / mv_n / mv_clock / mv_val one slot up, last row
// first; a removal moves it down, first row first; deferred entries likewise.
// Row data (clock rows, a key's value block, a deferred set) is always moved
// with the same lane <-> offset mapping, so a row's reads and writes in
// consecutive iterations are ordered by each lane's own program order; the
// per-key / per-entry counts (mv_n, dset_n) are read and written by lane 0
// only. keys[] and dset[] are searched by all lanes: every edit ends in
// ma_sync(). The per-op edits are map_mvreg_ws.h's (shared with the nested
// map's op path, map_map_apply.hip, whose inner maps take them). The op headers, and the clock pairs of the first ops, are staged
// in LDS 64 ops at a time, so that no op waits for its own header loads.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "kernels.h"
#include "map_mvreg_ws.h"
#include "map_rows.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace maprow;
using namespace mapws;

constexpr uint32_t kMaW = kW;
__device__ __forceinline__ void ma_sync() { mw_sync(); }

// (7 waves/SIMD: bounded to 72 VGPRs, the kernel keeps a few values in
// scratch and is faster than unbounded at 5 waves/SIMD — DESIGN.md §5h)
template <int NS>
__global__ __launch_bounds__(kMaW, 7) void map_mvreg_apply_kernel(crdt_map_mvreg_slab S, crdt_map_mvreg_ops P,
                                                              crdt_map_mvreg_slab R, uint64_t n_obj, uint32_t A,
                                                              int* __restrict__ status, uint32_t* __restrict__ ctl) {
  __shared__ uint64_t oc[128];  // the op's clock, scattered to a dense row
  // a chunk of 64 op headers and the first 64 clock pairs of its ops
  __shared__ uint32_t hkind[kMaW], hact[kMaW], pact[kMaW];
  __shared__ uint64_t hkey[kMaW], hctr[kMaW], hval[kMaW], hend[kMaW], pctr[kMaW];
  const uint32_t lane = threadIdx.x;
  const uint64_t Rm = R.mcap, Rs = R.scap;
  BlockTickets<4> sched(n_obj, ctl + 3, lane);
  for (uint64_t i = sched.first(); i < n_obj; i = sched.next(i)) {
    // ---- the input row, checked as the merge checks it (map.hip)
    const uint32_t nS = uni32(S.n_keys[i]), dS = uni32(S.n_def[i]);
    const uint64_t lo = i ? uni64(P.obj_end[i - 1u]) : 0ull, hi = uni64(P.obj_end[i]);
    if (nS > S.kcap || dS > S.dcap || lo > hi || hi > (uint64_t)P.n_ops) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    const uint32_t vnS = lane < nS ? S.mv_n[i * S.kcap + lane] : 0u;
    const uint32_t dnS = lane < dS ? S.dset_n[i * S.dcap + lane] : 0u;
    bool bad = vnS > S.mcap || dnS > S.scap;
    for (uint32_t k = lane + kMaW; k < nS; k += kMaW) bad = bad || S.mv_n[i * S.kcap + k] > S.mcap;
    for (uint32_t d = lane + kMaW; d < dS; d += kMaW) bad = bad || S.dset_n[i * S.dcap + d] > S.scap;
    if (__ballot(bad) != 0ull) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    // ---- out[i]'s arrays; self[i]'s used slots copied in (out caps >= self's: api.hip)
    const MapRef m = map_ref(R, i, A);
    uint64_t* const keys = m.keys;
    uint64_t* const ecl = m.ecl;
    uint32_t* const mvn = m.mvn;
    uint64_t* const mvc = m.mvc;
    uint64_t* const mvv = m.mvv;
    uint64_t* const dcl = m.def.dcl;
    uint32_t* const dsn = m.def.dsn;
    uint64_t* const dse = m.def.dse;
    copy_n(keys, S.keys + i * S.kcap, nS, lane);
    copy_n(ecl, S.eclock + i * S.kcap * A, nS * A, lane);
    for (uint32_t k = 0; k < nS; ++k) {
      const uint64_t sk = i * S.kcap + k;
      const uint32_t vn = k < kMaW ? (uint32_t)__builtin_amdgcn_readlane(vnS, k) : uni32(S.mv_n[sk]);
      if (lane == 0u) mvn[k] = vn;
      copy_n(mvc + k * Rm * A, S.mv_clock + sk * S.mcap * A, vn * A, lane);
      copy_n(mvv + k * Rm, S.mv_val + sk * S.mcap, vn, lane);
    }
    copy_n(dcl, S.dclock + i * S.dcap * A, dS * A, lane);
    for (uint32_t d = 0; d < dS; ++d) {
      const uint64_t sd = i * S.dcap + d;
      const uint32_t sn = d < kMaW ? (uint32_t)__builtin_amdgcn_readlane(dnS, d) : uni32(S.dset_n[sd]);
      if (lane == 0u) dsn[d] = sn;
      copy_n(dse + d * Rs, S.dset + sd * S.scap, sn, lane);
    }
    MapSt<NS> st;  // the map clock and the two counts, in registers across the op list
    st.cM = rowv<NS>(S.clock, i, A, lane);
    st.nk = nS;
    st.nd = dS;
    int err = 0;
    ma_sync();

    // The op headers are staged in LDS 64 ops at a time (slot t: the chunk's op
    // t), with the first 64 clock pairs of those ops, before the chunk's edits
    // start: these loads are independent of each other and of the state, so
    // none sits on an op's chain of dependent round trips.
    uint64_t pb = 0ull;  // the staged pairs' first index
    for (uint64_t j = lo; j < hi && !err; ++j) {
      const uint32_t t = (uint32_t)(j - lo) & (kMaW - 1u);
      if (t == 0u) {
        const bool inb = lane < hi - j;
        const uint32_t k_ = inb ? P.kind[j + lane] : 0u, a_ = inb ? P.actor[j + lane] : 0u;
        const uint64_t y_ = inb ? P.key[j + lane] : 0ull, c_ = inb ? P.counter[j + lane] : 0ull;
        const uint64_t v_ = inb ? P.val[j + lane] : 0ull, e_ = inb ? P.clk_end[j + lane] : 0ull;
        pb = j ? uni64(P.clk_end[j - 1u]) : 0ull;
        const bool pin = pb < (uint64_t)P.n_clk && lane < (uint64_t)P.n_clk - pb;
        const uint32_t pa_ = pin ? P.clk_act[pb + lane] : 0u;
        const uint64_t pc_ = pin ? P.clk_ctr[pb + lane] : 0ull;
        ma_sync();  // the previous chunk's reads of the stage are done
        hkind[lane] = k_;
        hact[lane] = a_;
        hkey[lane] = y_;
        hctr[lane] = c_;
        hval[lane] = v_;
        hend[lane] = e_;
        pact[lane] = pa_;
        pctr[lane] = pc_;
        ma_sync();
      }
      const uint32_t kind = uni32(hkind[t]);
      const uint64_t clo = t ? uni64(hend[t - 1u]) : pb, chi = uni64(hend[t]);
      const uint64_t key = uni64(hkey[t]);
      // an op clock is strictly increasing actors below A: at most A pairs
      if (kind > CRDT_MAP_OP_UP || clo > chi || chi > (uint64_t)P.n_clk || chi - clo > A) {
        err = CRDT_ENONCANON;
        break;
      }
      if (kind == CRDT_MAP_OP_NOP) continue;
      // ---- the op's clock as a dense row (and its canonicity)
      const uint32_t np = (uint32_t)(chi - clo);
      ma_sync();  // the previous op's reads of oc are done
      oc[lane] = 0ull;
      oc[lane + kMaW] = 0ull;
      ma_sync();
      bool cbad = false;
      if (chi - pb <= kMaW) {  // its pairs are staged, from slot clo - pb (clo >= pb: checked op by op)
        const uint32_t f = (uint32_t)(clo - pb);
        if (lane < np) {
          const uint32_t a = pact[f + lane];
          const uint64_t c = pctr[f + lane];
          cbad = c == 0ull || a >= A || (lane && pact[f + lane - 1u] >= a);
          if (a < A) oc[a] = c;
        }
      } else {
        for (uint32_t p = lane; p < np; p += kMaW) {
          const uint32_t a = P.clk_act[clo + p];
          const uint64_t c = P.clk_ctr[clo + p];
          cbad = cbad || c == 0ull || a >= A || (p && P.clk_act[clo + p - 1u] >= a);
          if (a < A) oc[a] = c;
        }
      }
      if (__ballot(cbad) != 0ull) {
        err = CRDT_ENONCANON;
        break;
      }
      ma_sync();
      const Row<NS> C = ldrow<NS>(oc, A, lane);

      if (kind == CRDT_MAP_OP_RM) {
        err = map_rm<NS>(m, st, key, C, A, lane);
        continue;
      }
      // ---- Op::Up
      const uint32_t da = uni32(hact[t]);
      if (da >= A) {
        err = CRDT_ENONCANON;
        break;
      }
      err = map_up<NS>(m, st, da, uni64(hctr[t]), key, C, uni64(hval[t]), A, lane);
    }
    if (err) {
      if (lane == 0u) atomicCAS(status, 0, err);
      continue;
    }
    if (lane == 0u) {
      R.n_keys[i] = st.nk;
      R.n_def[i] = st.nd;
    }
    strow<NS>(R.clock + i * A, st.cM, A, lane);
  }
}

}  // namespace

int launch_map_mvreg_apply(const crdt_map_mvreg_slab& S, const crdt_map_mvreg_ops& P, const crdt_map_mvreg_slab& R,
                           uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  if (hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), stream) != hipSuccess) return CRDT_EHIP;  // ctl[3]: tickets
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const uint64_t cap = (uint64_t)cus * 28u;  // 7 single-wave blocks per SIMD (the kernel's register bound)
  const uint32_t blocks = (uint32_t)(n_obj < cap ? n_obj : cap);
  if (A > 64u)  // 65-128 actors: two slots per lane
    hipLaunchKernelGGL((map_mvreg_apply_kernel<2>), dim3(blocks), dim3(kMaW), 0, stream, S, P, R, n_obj, A, status,
                       ctl);
  else
    hipLaunchKernelGGL((map_mvreg_apply_kernel<1>), dim3(blocks), dim3(kMaW), 0, stream, S, P, R, n_obj, A, status,
                       ctl);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
