// Map<u64, Map<u64, MVReg<u64, A>, A>, A>::apply (CmRDT), batched — the op path
// of the reference's own test type (TestMap, test/map.rs:4-8): out[i] = self[i]
// after each of object i's ops in order (include/crdts_hip.h, crdt_map_map_apply).
//
// Reference: Map::apply (src/map.rs:160-190) with V = the inner map. Op::Rm ->
// apply_rm (:336-350): defer a clock the map clock does not cover, subtract it
// from the key's entry clock, drop an emptied entry, else the inner map takes
// Map::truncate (:131-158). Op::Up: skipped whole when the map clock has the
// dot (:170-173); else the entry is taken out (or starts with an empty clock
// and an empty inner map), witnesses the dot, its inner map takes the inner op
// by the same Map::apply against its own clock, the entry goes back, the map
// clock witnesses the dot and apply_deferred (:325-333) re-applies every
// deferred remove. Every step of the outer apply_deferred is a subtract (of an
// entry clock, and slot-wise inside the inner map), so the pass walks the
// deferred entries in CLOCK ORDER, keys ascending, and keeps the clocks the
// map clock still does not cover.
//
// Key slot k's inner map is inner row i * kcap + k, so an outer key insert or
// removal in place would move whole inner maps. Two launches instead:
//  (1) the edits, one wave per object (lane = actor slot, map_rows.h). The
//      outer part is edited in out[i] in place as map_apply.hip edits a
//      Map<u64, MVReg> row, each key with a source beside it: its inner row of
//      self, or a physical slot of a scratch inner slab laid out like out's
//      (row i * kcap + p). An inner map is copied (used slots) into a free
//      physical slot on its first edit or truncation and edited there in place
//      (map_mvreg_ws.h, map_wave.h); a dropped entry frees its slot. The sources of the
//      final keys are the tasks of (2).
//  (2) the placement, one wave per out key slot: the source's used slots to
//      inner row i * kcap + k of out. Inner maps no op touched go self -> out
//      here and never pass through (1).
// The op headers, and the clock pairs of the first ops, are staged in LDS 64
// ops at a time. This kernel keeps its own copy of map_ops.h's reader, with the
// inner op's dot and key beside the header: through the shared reader its
// registers and scratch were the same and it measured 0.4 % slower (DESIGN.md
// §5p). A change to the staging window in map_ops.h is made here as well.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "kernels.h"
#include "map_limits.h"
#include "map_mvreg_ws.h"
#include "map_rows.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace maprow;
using namespace mapws;

static_assert(kMapMapDcap <= kW, "lane d holds outer deferred entry d's set size");
constexpr uint64_t kSrcNone = ~0ull;      // an unused out key slot: no task
constexpr uint64_t kSrcWork = 1ull << 63;  // | p: physical slot p of the object's scratch rows (else: a self inner row)

// (NS = 1 at 6 waves/SIMD: bounded to 80 VGPRs the kernel keeps a few values in
// scratch and is 7.7 % faster than unbounded at 4 waves/SIMD — DESIGN.md §5j)
template <int NS>
__global__ __launch_bounds__(kW, NS == 1 ? 6 : 1) void map_map_apply_kernel(crdt_map_map_slab S, crdt_map_map_ops P, crdt_map_map_slab R,
                                                           crdt_map_mvreg_slab W, uint64_t* __restrict__ src,
                                                           uint32_t* __restrict__ fre, uint64_t n_obj, uint32_t A,
                                                           int* __restrict__ status, uint32_t* __restrict__ ctl) {
  __shared__ uint64_t oc[128];  // the op's clock, scattered to a dense row
  // a chunk of 64 op headers and the first 64 clock pairs of its ops
  __shared__ uint32_t hkind[kW], hact[kW], hact2[kW], pact[kW];
  __shared__ uint64_t hkey[kW], hctr[kW], hkey2[kW], hctr2[kW], hval[kW], hend[kW], pctr[kW];
  const uint32_t lane = threadIdx.x;
  const uint64_t Rk = R.kcap;
  BlockTickets<4> sched(n_obj, ctl + 3, lane);
  for (uint64_t i = sched.first(); i < n_obj; i = sched.next(i)) {
    uint64_t* const tsrc = src + i * Rk;  // per key slot, moved with the keys
    uint32_t* const tfre = fre + i * Rk;  // the freed physical slots (a stack; lane 0's)
    uint32_t nk = 0u;
    int err = 0;
    // ---- the outer row, checked as the merge checks it (map_map.hip)
    const uint32_t nS = uni32(S.n_keys[i]), dS = uni32(S.n_def[i]);
    const uint64_t lo = i ? uni64(P.obj_end[i - 1u]) : 0ull, hi = uni64(P.obj_end[i]);
    if (nS > S.kcap || dS > S.dcap || lo > hi || hi > (uint64_t)P.n_ops) err = CRDT_ENONCANON;
    if (!err) {
      const uint32_t dnS = lane < dS ? S.dset_n[i * S.dcap + lane] : 0u;  // (dcap <= kMapMapDcap)
      if (__ballot(dnS > S.scap) != 0ull) err = CRDT_ENONCANON;
      if (!err) {
        // ---- out[i]'s outer arrays; self[i]'s used slots copied in (out caps >= self's)
        uint64_t* const keys = R.keys + i * Rk;
        uint64_t* const ecl = R.eclock + i * Rk * A;
        const DefRef def = def_ref(R, i, A);
        copy_n(keys, S.keys + i * S.kcap, nS, lane);
        copy_n(ecl, S.eclock + i * S.kcap * A, nS * A, lane);
        for (uint32_t k = lane; k < nS; k += kW) tsrc[k] = i * S.kcap + k;
        copy_n(def.dcl, S.dclock + i * S.dcap * A, dS * A, lane);
        for (uint32_t d = 0; d < dS; ++d) {
          const uint32_t sn = (uint32_t)__builtin_amdgcn_readlane(dnS, d);
          if (lane == 0u) def.dsn[d] = sn;
          copy_n(def.dse + (uint64_t)d * def.Rs, S.dset + (i * S.dcap + d) * S.scap, sn, lane);
        }
        Row<NS> cM = rowv<NS>(S.clock, i, A, lane);  // the map clock, in registers across the op list
        uint32_t nd = dS;
        uint32_t nfree = 0u, nphys = 0u;  // freed slots on the stack; slots ever handed out
        nk = nS;
        sync();

        // the key slot's inner map as a scratch row (copied from self on its
        // first edit); ~0 with err set for a malformed self row
        auto inner_row = [&](uint32_t pos) -> uint64_t {
          const uint64_t s = val0(tsrc + pos, lane);
          if (s & kSrcWork) return i * Rk + (s & ~kSrcWork);
          uint32_t p;
          if (nfree) {
            p = cnt0(tfre + --nfree, lane);
          } else {
            p = nphys++;
          }
          // (every live key holds at most one slot and nk <= kcap: p < kcap)
          if (p >= Rk || !map_copy_row(S.inner, s, W, i * Rk + p, A, lane)) {
            err = CRDT_ENONCANON;
            return ~0ull;
          }
          if (lane == 0u) tsrc[pos] = kSrcWork | p;
          sync();
          return i * Rk + p;
        };
        // apply_rm's entry edit (:343-349): the key's entry clock loses D; an
        // emptied entry is removed (its physical slot freed), else its inner
        // map takes Map::truncate(D)
        auto rm_entry = [&](uint64_t key, const Row<NS>& D) {
          uint32_t pos;
          if (!find_key(keys, nk, key, lane, pos)) return;
          const Row<NS> ec = vsub(ldrow<NS>(ecl + (uint64_t)pos * A, A, lane), D);
          if (!vany(ec)) {
            const uint64_t s = val0(tsrc + pos, lane);
            if ((s & kSrcWork) && nfree < Rk) {
              if (lane == 0u) tfre[nfree] = (uint32_t)(s & ~kSrcWork);
              ++nfree;
            }
            for (uint32_t k = pos + 1u; k < nk; ++k)  // rows above it one slot down, first row first
              strow<NS>(ecl + (uint64_t)(k - 1u) * A, ldrow<NS>(ecl + (uint64_t)k * A, A, lane), A, lane);
            shift_down(keys, pos, nk, lane);
            shift_down(tsrc, pos, nk, lane);
            --nk;
            sync();
            return;
          }
          strow<NS>(ecl + (uint64_t)pos * A, ec, A, lane);
          const uint64_t q = inner_row(pos);
          if (err) return;
          const MapRef m = map_ref(W, q, A);
          MapSt<NS> st = map_open<NS>(m, A, lane);
          map_truncate<NS>(m, st, D, A, lane);
          map_close<NS>(m, st, A, lane);
        };

        uint64_t pb = 0ull;  // the staged pairs' first index
        for (uint64_t j = lo; j < hi && !err; ++j) {
          const uint32_t t = (uint32_t)(j - lo) & (kW - 1u);
          if (t == 0u) {
            const bool inb = lane < hi - j;
            const uint32_t k_ = inb ? P.kind[j + lane] : 0u, a_ = inb ? P.actor[j + lane] : 0u;
            const uint32_t a2_ = inb ? P.actor2[j + lane] : 0u;
            const uint64_t y_ = inb ? P.key[j + lane] : 0ull, c_ = inb ? P.counter[j + lane] : 0ull;
            const uint64_t y2_ = inb ? P.key2[j + lane] : 0ull, c2_ = inb ? P.counter2[j + lane] : 0ull;
            const uint64_t v_ = inb ? P.val[j + lane] : 0ull, e_ = inb ? P.clk_end[j + lane] : 0ull;
            pb = j ? uni64(P.clk_end[j - 1u]) : 0ull;
            const bool pin = pb < (uint64_t)P.n_clk && lane < (uint64_t)P.n_clk - pb;
            const uint32_t pa_ = pin ? P.clk_act[pb + lane] : 0u;
            const uint64_t pc_ = pin ? P.clk_ctr[pb + lane] : 0ull;
            sync();  // the previous chunk's reads of the stage are done
            hkind[lane] = k_;
            hact[lane] = a_;
            hact2[lane] = a2_;
            hkey[lane] = y_;
            hctr[lane] = c_;
            hkey2[lane] = y2_;
            hctr2[lane] = c2_;
            hval[lane] = v_;
            hend[lane] = e_;
            pact[lane] = pa_;
            pctr[lane] = pc_;
            sync();
          }
          const uint32_t kind = uni32(hkind[t]);
          const uint64_t clo = t ? uni64(hend[t - 1u]) : pb, chi = uni64(hend[t]);
          const uint64_t key = uni64(hkey[t]);
          // an op clock is strictly increasing actors below A: at most A pairs
          if (kind > CRDT_MAPMAP_OP_UP_NOP || clo > chi || chi > (uint64_t)P.n_clk || chi - clo > A) {
            err = CRDT_ENONCANON;
            break;
          }
          if (kind == CRDT_MAPMAP_OP_NOP) continue;
          // ---- the op's clock as a dense row (and its canonicity)
          const uint32_t np = (uint32_t)(chi - clo);
          sync();  // the previous op's reads of oc are done
          oc[lane] = 0ull;
          oc[lane + kW] = 0ull;
          sync();
          bool cbad = false;
          if (chi - pb <= kW) {  // its pairs are staged, from slot clo - pb (clo >= pb: checked op by op)
            const uint32_t f = (uint32_t)(clo - pb);
            if (lane < np) {
              const uint32_t a = pact[f + lane];
              const uint64_t c = pctr[f + lane];
              cbad = c == 0ull || a >= A || (lane && pact[f + lane - 1u] >= a);
              if (a < A) oc[a] = c;
            }
          } else {
            for (uint32_t p = lane; p < np; p += kW) {
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
          sync();
          const Row<NS> C = ldrow<NS>(oc, A, lane);

          if (kind == CRDT_MAPMAP_OP_RM) {
            if (!vany(C)) continue;  // empty <= every clock, and subtracts nothing
            if (!vle(C, cM)) {
              err = def_insert<NS>(def, nd, key, C, A, lane);
              if (err) break;
            }
            rm_entry(key, C);
            continue;
          }

          // ---- Op::Up
          const uint32_t da = uni32(hact[t]), da2 = uni32(hact2[t]);
          const uint64_t dc = uni64(hctr[t]);
          if (da >= A || (kind == CRDT_MAPMAP_OP_UP_UP && da2 >= A)) {
            err = CRDT_ENONCANON;
            break;
          }
          const uint32_t ds = da >> 6, dl = da & 63u;
          uint64_t seen = 0ull;
          for (int s = 0; s < NS; ++s)
            if ((uint32_t)s == ds) seen = lane64(cM.v[s], dl);
          if (seen >= dc) continue;  // the map has this dot: the whole op is skipped
          uint32_t pos;
          const bool found = find_key(keys, nk, key, lane, pos);
          uint64_t q = 0ull;
          if (!found) {  // a fresh entry: an empty clock, an empty inner map in a free physical slot
            if (nk >= Rk) {
              err = CRDT_ECAPACITY;
              break;
            }
            uint32_t p;
            if (nfree) {
              p = cnt0(tfre + --nfree, lane);
            } else {
              p = nphys++;
            }
            if (p >= Rk) {  // (cannot be: at most one slot per live key)
              err = CRDT_ECAPACITY;
              break;
            }
            for (uint32_t k = nk; k-- > pos;)  // rows from pos one slot up, last row first
              strow<NS>(ecl + (uint64_t)(k + 1u) * A, ldrow<NS>(ecl + (uint64_t)k * A, A, lane), A, lane);
            shift_up(keys, pos, nk, lane);
            shift_up(tsrc, pos, nk, lane);
            if (lane == 0u) {
              keys[pos] = key;
              tsrc[pos] = kSrcWork | p;
            }
            ++nk;
            q = i * Rk + p;
            map_clear<NS>(map_ref(W, q, A), A, lane);
          } else if (kind != CRDT_MAPMAP_OP_UP_NOP) {
            q = inner_row(pos);
            if (err) break;
          }
          Row<NS> ec = found ? ldrow<NS>(ecl + (uint64_t)pos * A, A, lane) : zrow<NS>();
          for (int s = 0; s < NS; ++s) {  // witness(dot) on the entry clock and on the map clock
            if ((uint32_t)s != ds || lane != dl) continue;
            ec.v[s] = ec.v[s] > dc ? ec.v[s] : dc;
            cM.v[s] = dc;
          }
          strow<NS>(ecl + (uint64_t)pos * A, ec, A, lane);
          if (kind != CRDT_MAPMAP_OP_UP_NOP) {  // the inner op, by the same Map::apply on the inner map
            const MapRef m = map_ref(W, q, A);
            MapSt<NS> st = map_open<NS>(m, A, lane);
            if (kind == CRDT_MAPMAP_OP_UP_RM)
              err = map_rm<NS>(m, st, uni64(hkey2[t]), C, A, lane);
            else
              err = map_up<NS>(m, st, da2, uni64(hctr2[t]), uni64(hkey2[t]), C, uni64(hval[t]), A, lane);
            if (err) break;
            map_close<NS>(m, st, A, lane);
          }
          sync();
          // ---- apply_deferred: every (clock, key) removed again; the clocks
          // the map clock still does not cover stay, with their sets
          uint32_t w = 0;
          for (uint32_t d = 0; d < nd && !err; ++d) {
            const Row<NS> D = ldrow<NS>(def.dcl + (uint64_t)d * A, A, lane);
            const uint32_t sn = cnt0(def.dsn + d, lane);
            for (uint32_t s = 0; s < sn && !err; ++s) rm_entry(uni64(def.dse[(uint64_t)d * def.Rs + s]), D);
            if (vle(D, cM)) continue;
            if (w != d) def_move<NS>(def, w, d, A, lane);
            ++w;
          }
          if (w != nd) sync();
          nd = w;
        }
        if (!err) {
          if (lane == 0u) {
            R.n_keys[i] = nk;
            R.n_def[i] = nd;
          }
          strow<NS>(R.clock + i * A, cM, A, lane);
        }
      }
    }
    // the slots past the kept keys hold no task (a rejected object: none at all)
    if (err) {
      nk = 0u;
      if (lane == 0u) atomicCAS(status, 0, err);
    }
    sync();
    for (uint32_t k = nk + lane; k < Rk; k += kW) tsrc[k] = kSrcNone;
    sync();
  }
}

// The placement: out key slot t's inner map, the used slots of its source row
// (a self inner row, or a scratch row of the same object), to inner row t of out.
__global__ __launch_bounds__(kW) void map_map_place_kernel(crdt_map_mvreg_slab Si, crdt_map_mvreg_slab W,
                                                           crdt_map_mvreg_slab Ri, const uint64_t* __restrict__ src,
                                                           uint64_t n_tasks, uint32_t slots, uint32_t A,
                                                           int* __restrict__ status) {
  const uint32_t lane = threadIdx.x;
  for (uint64_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {
    const uint64_t s = uni64(src[t]);
    if (s == kSrcNone) continue;
    bool ok;
    if (s & kSrcWork)
      ok = map_copy_row(W, t / slots * slots + (s & ~kSrcWork), Ri, t, A, lane);
    else
      ok = map_copy_row(Si, s, Ri, t, A, lane);
    if (!ok && lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
  }
}

struct Carve {
  uint8_t* p;
  template <typename T>
  T* take(uint64_t n) {
    T* q = (T*)p;
    p += (n * sizeof(T) + 15u) & ~15ull;
    return q;
  }
};
// the scratch: the key slots' sources, the free-slot stacks, an inner slab like R's
crdt_map_mvreg_slab carve(uint8_t* base, const crdt_map_map_slab& R, uint64_t n_obj, uint32_t A, uint64_t** src,
                          uint32_t** fre, size_t* bytes) {
  const crdt_map_mvreg_slab& I = R.inner;
  const uint64_t nt = n_obj * R.kcap;
  Carve c{base};
  uint64_t* s = c.take<uint64_t>(nt);
  uint32_t* f = c.take<uint32_t>(nt);
  crdt_map_mvreg_slab W = I;
  W.clock = c.take<uint64_t>(nt * A);
  W.n_keys = c.take<uint32_t>(nt);
  W.keys = c.take<uint64_t>(nt * I.kcap);
  W.eclock = c.take<uint64_t>(nt * I.kcap * A);
  W.mv_n = c.take<uint32_t>(nt * I.kcap);
  W.mv_clock = c.take<uint64_t>(nt * I.kcap * I.mcap * A);
  W.mv_val = c.take<uint64_t>(nt * I.kcap * I.mcap);
  W.n_def = c.take<uint32_t>(nt);
  W.dclock = c.take<uint64_t>(nt * I.dcap * A);
  W.dset_n = c.take<uint32_t>(nt * I.dcap);
  W.dset = c.take<uint64_t>(nt * I.dcap * I.scap);
  if (src) *src = s;
  if (fre) *fre = f;
  if (bytes) *bytes = (size_t)(c.p - base);
  return W;
}

}  // namespace

size_t map_map_apply_scratch_bytes(const crdt_map_map_slab& R, uint64_t n_obj, uint32_t A) {
  size_t bytes = 0;
  (void)carve(nullptr, R, n_obj, A, nullptr, nullptr, &bytes);
  return bytes + 16u;
}

int launch_map_map_apply(const crdt_map_map_slab& S, const crdt_map_map_ops& P, const crdt_map_map_slab& R,
                         uint64_t n_obj, uint32_t A, uint8_t* scratch, int* status, uint32_t* ctl,
                         hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  uint64_t* src = nullptr;
  uint32_t* fre = nullptr;
  const crdt_map_mvreg_slab W = carve(scratch, R, n_obj, A, &src, &fre, nullptr);
  if (hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), stream) != hipSuccess) return CRDT_EHIP;  // ctl[3]: tickets
  const uint64_t cap = (uint64_t)cu_count() * 28u;
  uint32_t blocks = (uint32_t)(n_obj < cap ? n_obj : cap);
  if (A > 64u)  // 65-128 actors: two slots per lane
    hipLaunchKernelGGL((map_map_apply_kernel<2>), dim3(blocks), dim3(kW), 0, stream, S, P, R, W, src, fre, n_obj, A,
                       status, ctl);
  else
    hipLaunchKernelGGL((map_map_apply_kernel<1>), dim3(blocks), dim3(kW), 0, stream, S, P, R, W, src, fre, n_obj, A,
                       status, ctl);
  if (hipGetLastError() != hipSuccess) return CRDT_EHIP;
  const uint64_t nt = n_obj * R.kcap;
  blocks = coprime_grid((uint32_t)(nt < cap ? nt : cap), R.kcap);  // (sched.h)
  hipLaunchKernelGGL(map_map_place_kernel, dim3(blocks), dim3(kW), 0, stream, S.inner, W, R.inner, src, nt, R.kcap, A,
                     status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
