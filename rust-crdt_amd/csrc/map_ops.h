// The op reader of the Map apply kernels (internal; map_apply.hip and
// map_orswot_apply.hip — map_map_apply.hip keeps a copy with the inner op's
// fields): one wave walks one object's slice of an op batch
// (crdt_map_mvreg_ops / crdt_map_orswot_ops, include/crdts_hip.h) and gets
// each op's header and its clock as a dense row.
//
// The op headers are staged in LDS 64 ops at a time (slot t: the chunk's op
// t), with the first 64 clock pairs of those ops, before the chunk's edits
// start: these loads are independent of each other and of the map's state, so
// none sits on an op's chain of dependent round trips. Every global load of a
// refill is issued before the refill's first barrier.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "map_rows.h"
#include "map_wave.h"

namespace crdts_hip {
namespace mapops {

using namespace maprow;

static_assert(CRDT_MAP_OP_NOP == 0, "kind 0 is the op without a clock");

// The block's stage: static LDS arrays, 4.25 KB. Separate arrays, as the
// kernels' register bounds were tuned with (one LDS struct changes the
// kernels' scratch use).
struct OpStage {
  uint64_t* oc;  // [128] the op's clock, scattered to a dense row
  // a chunk of 64 op headers and the first 64 clock pairs of its ops
  uint32_t *hkind, *hact, *pact;
  uint64_t *hkey, *hctr, *hpay, *hend, *pctr;  // hpay: the op's one payload (val / member)
};
__device__ __forceinline__ OpStage op_stage() {
  __shared__ uint64_t oc[128];
  __shared__ uint32_t hkind[kW], hact[kW], pact[kW];
  __shared__ uint64_t hkey[kW], hctr[kW], hpay[kW], hend[kW], pctr[kW];
  return OpStage{oc, hkind, hact, pact, hkey, hctr, hpay, hend, pctr};
}

// The chunk of ops [j, min(j + 64, hi)) into the stage; `pay` is the batch's
// payload array. Returns the staged pairs' first index (the caller's `pb`).
template <class Ops>
__device__ __forceinline__ uint64_t refill(const OpStage& s, const Ops& P, const uint64_t* pay, uint64_t j,
                                           uint64_t hi, uint32_t lane) {
  const bool inb = lane < hi - j;
  const uint32_t k_ = inb ? P.kind[j + lane] : 0u, a_ = inb ? P.actor[j + lane] : 0u;
  const uint64_t y_ = inb ? P.key[j + lane] : 0ull, c_ = inb ? P.counter[j + lane] : 0ull;
  const uint64_t v_ = inb ? pay[j + lane] : 0ull, e_ = inb ? P.clk_end[j + lane] : 0ull;
  const uint64_t pb = j ? uni64(P.clk_end[j - 1u]) : 0ull;
  const bool pin = pb < (uint64_t)P.n_clk && lane < (uint64_t)P.n_clk - pb;
  const uint32_t pa_ = pin ? P.clk_act[pb + lane] : 0u;
  const uint64_t pc_ = pin ? P.clk_ctr[pb + lane] : 0ull;
  sync();  // the previous chunk's reads of the stage are done
  s.hkind[lane] = k_;
  s.hact[lane] = a_;
  s.hkey[lane] = y_;
  s.hctr[lane] = c_;
  s.hpay[lane] = v_;
  s.hend[lane] = e_;
  s.pact[lane] = pa_;
  s.pctr[lane] = pc_;
  sync();
  return pb;
}

// Op t of the staged chunk: its kind (<= max_kind, the Map type's largest), its
// key and its clock's pair range. false: a header out of bounds
// (CRDT_ENONCANON). The rest of the header is read from the stage by the
// caller (the dot's actor < A is the kernel's check).
struct OpHdr {
  uint32_t kind;
  uint64_t key, clo, chi;
};
template <class Ops>
__device__ __forceinline__ bool read_hdr(const OpStage& s, const Ops& P, uint32_t t, uint64_t pb,
                                         uint32_t max_kind, uint32_t A, OpHdr& h) {
  h.kind = uni32(s.hkind[t]);
  h.clo = t ? uni64(s.hend[t - 1u]) : pb;
  h.chi = uni64(s.hend[t]);
  h.key = uni64(s.hkey[t]);
  // an op clock is strictly increasing actors below A: at most A pairs
  if (h.kind > max_kind || h.clo > h.chi || h.chi > (uint64_t)P.n_clk || h.chi - h.clo > A) return false;
  return true;
}
// The clock of an op that has one (every kind but NOP, kind 0) as a dense
// row. !ok: not strictly increasing actors below A with non-zero counters
// (CRDT_ENONCANON).
template <int NS>
struct OpClock {
  Row<NS> C;
  bool ok;
};
template <int NS, class Ops>
__device__ __forceinline__ OpClock<NS> read_clock(const OpStage& s, const Ops& P, const OpHdr& h, uint64_t pb,
                                                  uint32_t A, uint32_t lane) {
  const uint64_t clo = h.clo, chi = h.chi;
  const uint32_t np = (uint32_t)(chi - clo);
  sync();  // the previous op's reads of oc are done
  s.oc[lane] = 0ull;
  s.oc[lane + kW] = 0ull;
  sync();
  bool cbad = false;
  if (chi - pb <= kW) {  // its pairs are staged, from slot clo - pb (clo >= pb: checked op by op)
    const uint32_t f = (uint32_t)(clo - pb);
    if (lane < np) {
      const uint32_t a = s.pact[f + lane];
      const uint64_t c = s.pctr[f + lane];
      cbad = c == 0ull || a >= A || (lane && s.pact[f + lane - 1u] >= a);
      if (a < A) s.oc[a] = c;
    }
  } else {  // read in place, 64 pairs at a time
    for (uint32_t p = lane; p < np; p += kW) {
      const uint32_t a = P.clk_act[clo + p];
      const uint64_t c = P.clk_ctr[clo + p];
      cbad = cbad || c == 0ull || a >= A || (p && P.clk_act[clo + p - 1u] >= a);
      if (a < A) s.oc[a] = c;
    }
  }
  if (__ballot(cbad) != 0ull) return {zrow<NS>(), false};
  sync();
  return {ldrow<NS>(s.oc, A, lane), true};
}

}  // namespace mapops
}  // namespace crdts_hip
