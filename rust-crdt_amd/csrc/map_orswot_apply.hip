// Map<u64, Orswot<u64, A>, A>::apply (CmRDT), batched: out[i] = self[i] after
// each of object i's ops in order (include/crdts_hip.h, crdt_map_orswot_apply).
//
// Reference: Map::apply (src/map.rs:160-190) — Op::Nop; Op::Rm -> apply_rm
// (:336-350: defer a clock the map clock does not cover, subtract it from the
// key's entry clock, drop an emptied entry, else Orswot::truncate,
// src/orswot.rs:159-172); Op::Up -> skipped when the map clock has the dot
// (:170-173), else the entry is taken out (or starts empty), witnesses the
// dot, takes the nested op (Orswot::apply, src/orswot.rs:66-82: Add, or Rm ->
// apply_remove :195-211), goes back in, the map clock witnesses the dot and
// apply_deferred (:325-333) re-applies every deferred remove, in CLOCK ORDER
// and keys ascending: a truncate is not a plain subtract, so with Orswot
// values the order can matter.
//
// One wave per object; lane = actor slot (map_rows.h). self[i]'s used slots
// are copied into out[i]. The key-level arrays and the map's deferred removes
// are then edited in out[i] in place, as map_apply.hip does (the edits'
// helpers: map_wave.h); the nested set an
// op works on is staged in an LDS workspace (map_orswot_ws.h: members, member
// clocks, deferred clocks and their sets, with the entry clock and the set's
// top clock in registers), edited there, and written back only when another
// key's set is needed, a key slot moves, or the op list ends — consecutive
// ops on one key cost no HBM round trip for its value. A fresh key's set
// starts in the workspace and is never read from HBM. Up to 64 keys are
// mirrored in LDS, so the search every op starts with reads no HBM. Every
// cross-lane edit of out[i] or of the workspace ends in a wave-local fence +
// barrier. The ops are read through map_ops.h: headers, and the clock pairs
// of the first ops, staged in LDS 64 ops at a time.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "kernels.h"
#include "map_ops.h"
#include "map_orswot_ws.h"
#include "map_rows.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace mows;

constexpr uint32_t kOaLdsMax = kMapOrswotApplyLdsMax;  // dynamic workspace limit per wave (kernels.h)
constexpr uint32_t kNone = 0xFFFFFFFFu;

// (5 waves/SIMD at one slot per lane: bounded to 96 VGPRs the kernel keeps
// 40 B/lane in scratch and is faster than at 4 or 6 waves/SIMD — DESIGN.md §5i)
template <int NS>
__global__ __launch_bounds__(kW, NS == 1 ? 5 : 4) void map_orswot_apply_kernel(
    crdt_map_orswot_slab S, crdt_map_orswot_ops P, crdt_map_orswot_slab R, uint64_t n_obj, uint32_t A,
    int* __restrict__ status, uint32_t* __restrict__ ctl) {
  extern __shared__ uint64_t oa_lds[];
  const mapops::OpStage ops = mapops::op_stage();  // the op reader's LDS stage (map_ops.h)
  __shared__ uint64_t lk[kW];  // a copy of out[i]'s keys while there are at most 64 (kvalid)
  const uint32_t lane = threadIdx.x;
  const uint64_t Rk = R.kcap, Rm = R.mcap, Rv = R.vdcap, Rvs = R.vscap, Rd = R.dcap, Rs = R.scap;
  const Caps c{R.mcap, R.vdcap, R.vscap, A};
  // the workspace: one nested set of out's capacities, then its deferred set
  // sizes and the drop flags of ws_apply_deferred
  Ws W;
  W.key = oa_lds;
  W.row = W.key + Rm;
  W.dclk = W.row + Rm * A;
  W.dset = W.dclk + Rv * A;
  W.sw = R.vscap;
  W.dn = (uint32_t*)(W.dset + Rv * Rvs);
  W.nm = W.nd = 0u;
  uint32_t* const ddead = W.dn + Rv;
  uint32_t* const mdead = ddead + Rv;
  for (uint32_t j = lane; j < R.vdcap + R.mcap; j += kW) ddead[j] = 0u;
  sync();
  BlockTickets<4> sched(n_obj, ctl + 3, lane);
  for (uint64_t i = sched.first(); i < n_obj; i = sched.next(i)) {
    // ---- the input row, checked as the merge checks it (map_orswot.hip)
    const uint32_t nS = uni32(S.n_keys[i]), dS = uni32(S.n_def[i]);
    const uint64_t lo = i ? uni64(P.obj_end[i - 1u]) : 0ull, hi = uni64(P.obj_end[i]);
    if (nS > S.kcap || dS > S.dcap || lo > hi || hi > (uint64_t)P.n_ops) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    const bool ls = lane < nS;
    const uint32_t vmS = ls ? S.vn_mem[i * S.kcap + lane] : 0u, vdS = ls ? S.vn_def[i * S.kcap + lane] : 0u;
    bool bad = vmS > S.mcap || vdS > S.vdcap;
    for (uint32_t d = 0; !bad && d < vdS; ++d) bad = S.vdset_n[(i * S.kcap + lane) * S.vdcap + d] > S.vscap;
    for (uint32_t k = kW + lane; k < nS; k += kW) {
      const uint64_t ki = i * S.kcap + k;
      bad = bad || S.vn_mem[ki] > S.mcap || S.vn_def[ki] > S.vdcap;
      for (uint32_t d = 0; !bad && d < S.vn_def[ki]; ++d) bad = S.vdset_n[ki * S.vdcap + d] > S.vscap;
    }
    for (uint32_t d = lane; d < dS; d += kW) bad = bad || S.dset_n[i * S.dcap + d] > S.scap;
    if (__ballot(bad) != 0ull) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    // ---- out[i]'s arrays; self[i]'s used slots copied in (out caps >= self's: api.hip's out_caps_ok)
    uint64_t* const keys = R.keys + i * Rk;
    uint64_t* const ecl = R.eclock + i * Rk * A;
    uint64_t* const vcl = R.vclock + i * Rk * A;
    uint32_t* const vnm = R.vn_mem + i * Rk;
    uint64_t* const vme = R.vmem + i * Rk * Rm;
    uint64_t* const vmc = R.vmclock + i * Rk * Rm * A;
    uint32_t* const vnd = R.vn_def + i * Rk;
    uint64_t* const vdc = R.vdclock + i * Rk * Rv * A;
    uint32_t* const vdn = R.vdset_n + i * Rk * Rv;
    uint64_t* const vds = R.vdset + i * Rk * Rv * Rvs;
    uint64_t* const dcl = R.dclock + i * Rd * A;
    uint32_t* const dsn = R.dset_n + i * Rd;
    uint64_t* const dse = R.dset + i * Rd * Rs;
    const DefRef def{dcl, dsn, dse, R.dcap, R.scap};  // the map's deferred removes (map_wave.h)
    copy_n(keys, S.keys + i * S.kcap, nS, lane);
    copy_n(ecl, S.eclock + i * S.kcap * A, nS * A, lane);
    copy_n(vcl, S.vclock + i * S.kcap * A, nS * A, lane);
    for (uint32_t k = 0; k < nS; ++k) {
      const uint64_t sk = i * S.kcap + k;
      const uint32_t m = k < kW ? (uint32_t)__builtin_amdgcn_readlane(vmS, k) : uni32(S.vn_mem[sk]);
      const uint32_t dn = k < kW ? (uint32_t)__builtin_amdgcn_readlane(vdS, k) : uni32(S.vn_def[sk]);
      if (lane == 0u) {
        vnm[k] = m;
        vnd[k] = dn;
      }
      copy_n(vme + k * Rm, S.vmem + sk * S.mcap, m, lane);
      copy_n(vmc + k * Rm * A, S.vmclock + sk * S.mcap * A, m * A, lane);
      copy_n(vdc + k * Rv * A, S.vdclock + sk * S.vdcap * A, dn * A, lane);
      copy_n(vdn + k * Rv, S.vdset_n + sk * S.vdcap, dn, lane);
      const uint32_t vs = S.vscap;
      for (uint32_t e = lane; e < dn * vs; e += kW) {  // the used part of each set
        const uint32_t d = e / vs, o = e - d * vs;
        if (o < S.vdset_n[sk * S.vdcap + d]) vds[(k * Rv + d) * Rvs + o] = S.vdset[sk * S.vdcap * vs + e];
      }
    }
    copy_n(dcl, S.dclock + i * S.dcap * A, dS * A, lane);
    copy_n(dsn, S.dset_n + i * S.dcap, dS, lane);
    {
      const uint32_t ss = S.scap;
      for (uint32_t e = lane; e < dS * ss; e += kW) {
        const uint32_t d = e / ss, o = e - d * ss;
        if (o < S.dset_n[i * S.dcap + d]) dse[d * Rs + o] = S.dset[i * S.dcap * ss + e];
      }
    }
    Row<NS> cM = rowv<NS>(S.clock, i, A, lane);  // the map clock, in registers across the op list
    uint32_t nk = nS, nd = dS;
    int err = 0;
    // the staged entry: key slot `cur` of out[i] (kNone: none), its entry
    // clock and its set's top clock; `dirty`: out[i]'s slot is behind it
    uint32_t cur = kNone;
    bool dirty = false;
    Row<NS> ec = zrow<NS>(), vc = zrow<NS>();
    // keys[] is searched by every op: up to 64 keys are mirrored in LDS, so the
    // search costs no global round trip (an object that passes 64 keys goes on
    // searching out[i] itself)
    bool kvalid = nS <= kW;
    if (kvalid && lane < nS) lk[lane] = S.keys[i * S.kcap + lane];
    sync();
    auto find_map_key = [&](uint64_t key, uint32_t& pos) -> bool {
      if (!kvalid) return find_key(keys, nk, key, lane, pos);
      const uint64_t x = lane < nk ? lk[lane] : ~0ull;
      pos = (uint32_t)__popcll(__ballot(lane < nk && x < key));
      return __ballot(lane < nk && x == key) != 0ull;
    };

    auto store_entry = [&]() {
      const uint64_t p = cur;
      strow<NS>(ecl + p * A, ec, A, lane);
      strow<NS>(vcl + p * A, vc, A, lane);
      if (lane == 0u) {
        vnm[p] = W.nm;
        vnd[p] = W.nd;
      }
      copy_n(vme + p * Rm, (const uint64_t*)W.key, W.nm, lane);
      copy_n(vmc + p * Rm * A, (const uint64_t*)W.row, W.nm * A, lane);
      copy_n(vdc + p * Rv * A, (const uint64_t*)W.dclk, W.nd * A, lane);
      copy_n(vdn + p * Rv, (const uint32_t*)W.dn, W.nd, lane);
      for (uint32_t e = lane; e < W.nd * W.sw; e += kW) {  // only the used slots
        const uint32_t d = e / W.sw;
        if (e - d * W.sw < W.dn[d]) vds[p * Rv * Rvs + e] = W.dset[e];
      }
      sync();
    };
    auto flush = [&]() {
      if (cur != kNone && dirty) store_entry();
      dirty = false;
    };
    auto acquire = [&](uint32_t pos) {
      if (cur == pos) return;
      flush();
      cur = pos;
      const uint64_t p = pos;
      ec = ldrow<NS>(ecl + p * A, A, lane);
      vc = ldrow<NS>(vcl + p * A, A, lane);
      W.nm = cnt0(vnm + p, lane);
      W.nd = cnt0(vnd + p, lane);
      copy_n(W.key, (const uint64_t*)(vme + p * Rm), W.nm, lane);
      copy_n(W.row, (const uint64_t*)(vmc + p * Rm * A), W.nm * A, lane);
      copy_n(W.dclk, (const uint64_t*)(vdc + p * Rv * A), W.nd * A, lane);
      copy_n(W.dn, (const uint32_t*)(vdn + p * Rv), W.nd, lane);
      // capacity-strided (the workspace's stride is out's): no wait for the sizes
      copy_n(W.dset, (const uint64_t*)(vds + p * Rv * Rvs), W.nd * W.sw, lane);
      sync();
    };
    // key slot src of out[i] to slot dst (its used part); the slot is not the staged one
    auto move_slot = [&](uint32_t dst_, uint32_t src_) {
      const uint64_t dst = dst_, src = src_;
      const uint32_t m = cnt0(vnm + src, lane), dn = cnt0(vnd + src, lane);
      strow<NS>(ecl + dst * A, ldrow<NS>(ecl + src * A, A, lane), A, lane);
      strow<NS>(vcl + dst * A, ldrow<NS>(vcl + src * A, A, lane), A, lane);
      copy_n(vme + dst * Rm, (const uint64_t*)(vme + src * Rm), m, lane);
      copy_n(vmc + dst * Rm * A, (const uint64_t*)(vmc + src * Rm * A), m * A, lane);
      copy_n(vdc + dst * Rv * A, (const uint64_t*)(vdc + src * Rv * A), dn * A, lane);
      copy_n(vdn + dst * Rv, (const uint32_t*)(vdn + src * Rv), dn, lane);
      for (uint32_t e = lane; e < dn * W.sw; e += kW) {
        const uint32_t d = e / W.sw;
        if (e - d * W.sw < vdn[src * Rv + d]) vds[dst * Rv * Rvs + e] = vds[src * Rv * Rvs + e];
      }
      if (lane == 0u) {
        vnm[dst] = m;
        vnd[dst] = dn;
      }
      sync();  // the next slot's copy overwrites what other lanes read here
    };

    // apply_rm's entry edit (src/map.rs:341-349): the key's entry clock loses
    // D; an emptied entry is removed, else its set is truncated by D
    auto rm_entry = [&](uint64_t key, const Row<NS>& D) {
      uint32_t pos;
      if (!find_map_key(key, pos)) return;
      const Row<NS> e = vsub(cur == pos ? ec : ldrow<NS>(ecl + (uint64_t)pos * A, A, lane), D);
      if (!vany(e)) {
        if (cur != pos) flush();  // (the staged entry itself is simply dropped)
        cur = kNone;
        dirty = false;
        for (uint32_t k = pos + 1u; k < nk; ++k) move_slot(k - 1u, k);
        shift_down(keys, pos, nk, lane);
        if (kvalid) shift_down(lk, pos, nk, lane);
        --nk;
        sync();
        return;
      }
      acquire(pos);
      ec = e;
      ws_truncate<NS>(W, vc, D, mdead, ddead, c, lane);
      dirty = true;
    };

    // Orswot::apply_remove (src/orswot.rs:195-211) on the staged set
    auto nested_rm = [&](uint64_t member, const Row<NS>& C) -> bool {
      if (!vle(C, vc)) {  // deferred: into an equal clock's set, or a new entry in CLOCK ORDER
        uint32_t at = W.nd;
        bool eq = false;
        for (uint32_t d = 0; d < W.nd; ++d) {
          const int o = vorder(C, ldrow<NS>(W.dclk + d * A, A, lane), lane);
          if (o > 0) continue;
          at = d;
          eq = o == 0;
          break;
        }
        if (eq) {
          uint64_t* const set = W.dset + at * W.sw;
          const uint32_t sn = uni32(W.dn[at]);
          uint32_t p;
          if (!find_key(set, sn, member, lane, p)) {
            if (sn >= W.sw) return false;
            shift_up(set, p, sn, lane);
            if (lane == 0u) {
              set[p] = member;
              W.dn[at] = sn + 1u;
            }
          }
        } else {
          if (W.nd >= c.DW) return false;
          for (uint32_t d = W.nd; d-- > at;) {  // entries from `at` one slot up, last first
            const uint32_t sn = uni32(W.dn[d]);
            const Row<NS> r = ldrow<NS>(W.dclk + d * A, A, lane);
            copy_n(W.dset + (d + 1u) * W.sw, (const uint64_t*)(W.dset + d * W.sw), sn, lane);
            strow<NS>(W.dclk + (d + 1u) * A, r, A, lane);
            if (lane == 0u) W.dn[d + 1u] = sn;
            sync();
          }
          strow<NS>(W.dclk + at * A, C, A, lane);
          if (lane == 0u) {
            W.dset[at * W.sw] = member;
            W.dn[at] = 1u;
          }
          ++W.nd;
        }
        sync();
      }
      uint32_t mp;
      if (find_key(W.key, W.nm, member, lane, mp)) {
        const Row<NS> r = vsub(ldrow<NS>(W.row + mp * A, A, lane), C);
        if (vany(r)) {
          strow<NS>(W.row + mp * A, r, A, lane);
        } else {  // an emptied member is dropped
          for (uint32_t j = mp + 1u; j < W.nm; ++j) {
            const Row<NS> q = ldrow<NS>(W.row + j * A, A, lane);
            strow<NS>(W.row + (j - 1u) * A, q, A, lane);
          }
          shift_down(W.key, mp, W.nm, lane);
          --W.nm;
        }
        sync();
      }
      return true;
    };
    // Orswot::apply, Op::Add (src/orswot.rs:66-79) on the staged set
    auto nested_add = [&](uint64_t member, uint32_t ds, uint32_t dl, uint64_t dc) -> bool {
      uint64_t seen = 0ull;
      for (int s = 0; s < NS; ++s)
        if ((uint32_t)s == ds) seen = lane64(vc.v[s], dl);
      if (seen >= dc) return true;  // the set has this dot
      uint32_t mp;
      Row<NS> r = zrow<NS>();
      if (find_key(W.key, W.nm, member, lane, mp)) {
        r = ldrow<NS>(W.row + mp * A, A, lane);
      } else {
        if (W.nm >= c.MW) return false;
        for (uint32_t j = W.nm; j-- > mp;) {  // rows from mp one slot up, last first
          const Row<NS> q = ldrow<NS>(W.row + j * A, A, lane);
          strow<NS>(W.row + (j + 1u) * A, q, A, lane);
        }
        shift_up(W.key, mp, W.nm, lane);
        if (lane == 0u) W.key[mp] = member;
        ++W.nm;
      }
      for (int s = 0; s < NS; ++s) {
        if ((uint32_t)s != ds || lane != dl) continue;
        r.v[s] = r.v[s] > dc ? r.v[s] : dc;
        vc.v[s] = dc;
      }
      strow<NS>(W.row + mp * A, r, A, lane);
      sync();
      if (W.nd) ws_apply_deferred<NS>(W, vc, mdead, ddead, c, lane);
      return true;
    };

    uint64_t pb = 0ull;  // the staged pairs' first index
    for (uint64_t j = lo; j < hi && !err; ++j) {
      const uint32_t t = (uint32_t)(j - lo) & (kW - 1u);
      if (t == 0u) pb = mapops::refill(ops, P, P.member, j, hi, lane);
      mapops::OpHdr h;
      if (!mapops::read_hdr(ops, P, t, pb, CRDT_MAP_OP_UP_RM, A, h)) {
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
      const uint32_t kind = h.kind;
      const uint64_t key = h.key;

      if (kind == CRDT_MAP_OP_RM) {
        if (!vle(C, cM)) {  // deferred: into an equal clock's key set, or a new entry in CLOCK ORDER
          err = def_insert<NS>(def, nd, key, C, A, lane);
          if (err) break;
        }
        rm_entry(key, C);
        continue;
      }

      // ---- Op::Up
      const uint32_t da = uni32(ops.hact[t]);
      const uint64_t dc = uni64(ops.hctr[t]);
      if (da >= A) {
        err = CRDT_ENONCANON;
        break;
      }
      const uint32_t ds = da >> 6, dl = da & 63u;
      uint64_t seen = 0ull;
      for (int s = 0; s < NS; ++s)
        if ((uint32_t)s == ds) seen = lane64(cM.v[s], dl);
      if (seen >= dc) continue;  // the map has this dot: the whole op is skipped
      uint32_t pos;
      if (find_map_key(key, pos)) {
        acquire(pos);
      } else {
        if (nk >= R.kcap) {
          err = CRDT_ECAPACITY;
          break;
        }
        flush();
        cur = kNone;
        for (uint32_t k = nk; k-- > pos;) move_slot(k + 1u, k);  // slots from pos one up, last first
        shift_up(keys, pos, nk, lane);
        if (lane == 0u) keys[pos] = key;
        kvalid = kvalid && nk < kW;
        if (kvalid) {
          shift_up(lk, pos, nk, lane);
          if (lane == 0u) lk[pos] = key;
        }
        ++nk;
        sync();
        cur = pos;  // an empty clock and an empty set, in the workspace only
        ec = zrow<NS>();
        vc = zrow<NS>();
        W.nm = W.nd = 0u;
      }
      dirty = true;
      for (int s = 0; s < NS; ++s) {  // witness(dot) on the entry clock and on the map clock
        if ((uint32_t)s != ds || lane != dl) continue;
        ec.v[s] = ec.v[s] > dc ? ec.v[s] : dc;
        cM.v[s] = dc;
      }
      const uint64_t member = uni64(ops.hpay[t]);
      if (!(kind == CRDT_MAP_OP_UP ? nested_add(member, ds, dl, dc) : nested_rm(member, C))) {
        err = CRDT_ECAPACITY;
        break;
      }
      // ---- apply_deferred: every (clock, key) removed again, CLOCK ORDER and
      // keys ascending; the clocks the map clock still does not cover stay
      uint32_t w = 0;
      for (uint32_t d = 0; d < nd; ++d) {
        const Row<NS> D = ldrow<NS>(dcl + (uint64_t)d * A, A, lane);
        const uint32_t sn = cnt0(dsn + d, lane);
        for (uint32_t s = 0; s < sn; ++s) rm_entry(uni64(dse[d * Rs + s]), D);
        if (vle(D, cM)) continue;
        if (w != d) def_move<NS>(def, w, d, A, lane);
        ++w;
      }
      if (w != nd) sync();
      nd = w;
    }
    if (err) {
      if (lane == 0u) atomicCAS(status, 0, err);
      continue;
    }
    flush();
    if (lane == 0u) {
      R.n_keys[i] = nk;
      R.n_def[i] = nd;
    }
    strow<NS>(R.clock + i * A, cM, A, lane);
  }
}

}  // namespace

// The kernel's dynamic workspace: one nested set of out's capacities (members,
// member clocks, deferred clocks and their sets), its deferred set sizes and
// the two drop-flag arrays. crdt_map_orswot_apply checks it against 64 KB less
// the 4.75 KB of the op stage and the key mirror (kMapOrswotApplyLdsMax).
size_t map_orswot_apply_lds_bytes(const crdt_map_orswot_slab& R, uint32_t A) {
  const size_t m = R.mcap, d = R.vdcap, s = R.vscap;
  return 8 * (m + m * A + d * A + d * s) + 8 * ((2 * d + m + 1) / 2);
}

int launch_map_orswot_apply(const crdt_map_orswot_slab& S, const crdt_map_orswot_ops& P,
                            const crdt_map_orswot_slab& R, uint64_t n_obj, uint32_t A, int* status, uint32_t* ctl,
                            hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const size_t lds = map_orswot_apply_lds_bytes(R, A);
  if (lds > kOaLdsMax) return CRDT_EINVAL;
  const void* fn = A > 64u ? (const void*)map_orswot_apply_kernel<2> : (const void*)map_orswot_apply_kernel<1>;
  int occ = 0;
  // one single-wave block per resident slot (the workspace and the register bound size it)
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, kW, lds) != hipSuccess || occ < 1) occ = 16;
  const uint64_t cap = (uint64_t)cu_count() * (uint32_t)occ;
  const uint32_t blocks = (uint32_t)(n_obj < cap ? n_obj : cap);
  if (hipMemsetAsync(ctl, 0, 4 * sizeof(uint32_t), stream) != hipSuccess) return CRDT_EHIP;  // ctl[3]: tickets
  void* args[] = {(void*)&S, (void*)&P, (void*)&R, &n_obj, &A, &status, &ctl};
  if (hipLaunchKernel(fn, dim3(blocks), dim3(kW), args, lds, stream) != hipSuccess) return CRDT_EHIP;
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
