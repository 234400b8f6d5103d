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
// sync() (map_wave.h). The per-op edits are map_mvreg_ws.h's (shared with
// the nested map's op path, map_map_apply.hip, whose inner maps take them).
// The ops are read through map_ops.h: headers, and the clock pairs of the
// first ops, staged in LDS 64 ops at a time, each op's clock as a dense row.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "kernels.h"
#include "map_mvreg_ws.h"
#include "map_ops.h"
#include "map_rows.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace maprow;
using namespace mapws;

// (7 waves/SIMD: bounded to 72 VGPRs, the kernel keeps a few values in
// scratch and is faster than unbounded at 5 waves/SIMD — DESIGN.md §5h)
template <int NS>
__global__ __launch_bounds__(kW, 7) void map_mvreg_apply_kernel(crdt_map_mvreg_slab S, crdt_map_mvreg_ops P,
                                                              crdt_map_mvreg_slab R, uint64_t n_obj, uint32_t A,
                                                              int* __restrict__ status, uint32_t* __restrict__ ctl) {
  const mapops::OpStage ops = mapops::op_stage();  // the op reader's LDS stage (map_ops.h)
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
    for (uint32_t k = lane + kW; k < nS; k += kW) bad = bad || S.mv_n[i * S.kcap + k] > S.mcap;
    for (uint32_t d = lane + kW; d < dS; d += kW) bad = bad || S.dset_n[i * S.dcap + d] > S.scap;
    if (__ballot(bad) != 0ull) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    // ---- out[i]'s arrays; self[i]'s used slots copied in (out caps >= self's: api.hip's out_caps_ok)
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
      const uint32_t vn = k < kW ? (uint32_t)__builtin_amdgcn_readlane(vnS, k) : uni32(S.mv_n[sk]);
      if (lane == 0u) mvn[k] = vn;
      copy_n(mvc + k * Rm * A, S.mv_clock + sk * S.mcap * A, vn * A, lane);
      copy_n(mvv + k * Rm, S.mv_val + sk * S.mcap, vn, lane);
    }
    copy_n(dcl, S.dclock + i * S.dcap * A, dS * A, lane);
    for (uint32_t d = 0; d < dS; ++d) {
      const uint64_t sd = i * S.dcap + d;
      const uint32_t sn = d < kW ? (uint32_t)__builtin_amdgcn_readlane(dnS, d) : uni32(S.dset_n[sd]);
      if (lane == 0u) dsn[d] = sn;
      copy_n(dse + d * Rs, S.dset + sd * S.scap, sn, lane);
    }
    MapSt<NS> st;  // the map clock and the two counts, in registers across the op list
    st.cM = rowv<NS>(S.clock, i, A, lane);
    st.nk = nS;
    st.nd = dS;
    int err = 0;
    sync();

    uint64_t pb = 0ull;  // the staged pairs' first index
    for (uint64_t j = lo; j < hi && !err; ++j) {
      const uint32_t t = (uint32_t)(j - lo) & (kW - 1u);
      if (t == 0u) pb = mapops::refill(ops, P, P.val, j, hi, lane);
      mapops::OpHdr h;
      if (!mapops::read_hdr(ops, P, t, pb, CRDT_MAP_OP_UP, A, h)) {
        err = CRDT_ENONCANON;
        break;
      }
      if (h.kind == CRDT_MAP_OP_NOP) continue;
      const mapops::OpClock<NS> oc = mapops::read_clock<NS>(ops, P, h, pb, A, lane);
      if (!oc.ok) {
        err = CRDT_ENONCANON;
        break;
      }
      const Row<NS>& C = oc.C;

      if (h.kind == CRDT_MAP_OP_RM) {
        err = map_rm<NS>(m, st, h.key, C, A, lane);
        continue;
      }
      // ---- Op::Up
      const uint32_t da = uni32(ops.hact[t]);
      if (da >= A) {
        err = CRDT_ENONCANON;
        break;
      }
      err = map_up<NS>(m, st, da, uni64(ops.hctr[t]), h.key, C, uni64(ops.hpay[t]), A, lane);
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
  const uint64_t cap = (uint64_t)cu_count() * 28u;  // 7 single-wave blocks per SIMD (the kernel's register bound)
  const uint32_t blocks = (uint32_t)(n_obj < cap ? n_obj : cap);
  if (A > 64u)  // 65-128 actors: two slots per lane
    hipLaunchKernelGGL((map_mvreg_apply_kernel<2>), dim3(blocks), dim3(kW), 0, stream, S, P, R, n_obj, A, status,
                       ctl);
  else
    hipLaunchKernelGGL((map_mvreg_apply_kernel<1>), dim3(blocks), dim3(kW), 0, stream, S, P, R, n_obj, A, status,
                       ctl);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
