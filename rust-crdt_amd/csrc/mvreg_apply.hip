// MVReg<u64, A> op path, batched (include/crdts_hip.h: crdt_mvreg_apply,
// crdt_mvreg_truncate, crdt_mvreg_read_clock) over the slabs of
// crdt_mvreg_merge: n[i] slots in use, clk[i][cap][A] dense rows (0 = absent),
// val[i][cap], Vec order.
//
// CmRDT::apply of Op::Put { clock, val } (src/mvreg.rs:158-186): an empty
// clock changes nothing (:161-163); else every value whose clock is <= the
// Put clock is dropped (:165), and (clock, val) is appended unless a remaining
// clock is strictly greater (:173-183). Causal::truncate (:100-113): every
// clock is VClock::subtract-ed (src/vclock.rs:236-242: an actor whose counter
// is <= the truncating clock's goes) and a value whose clock empties is
// dropped. read().add_clock (:201-222): the pointwise max of the clocks.
//
// Fast tier (out_cap <= 64 slots, the [out_cap][A] block within the LDS
// budget): one wave per register, W waves per block, each with its own LDS
// region holding the block, the op's clock scattered to a dense row, the
// values and the output slot table. An op is one pass of one compare per
// stored element (lane = element, 64 per step); "some stored > op" / "some
// stored < op" of slot k are taken by lane k from the two ballots of each
// step, masked to the slot's lane segment. A drop only clears the slot's bit
// in the wave-uniform `used` mask: no row moves. The append goes to the first
// slot past the highest used one; rows are compacted in place only when that
// runs into out_cap. Physical order is therefore always Vec order, and the
// output block is written once, slot-major and coalesced, zero fill included.
// The object's op bounds are loaded two objects ahead, its slot count, first
// 64 clock elements, values and op headers one object ahead.
//
// General tier (the rest, up to the ABI limits): one wave per register, the
// state edited in the output block in HBM. No dense op row: with nnz[k] the
// number of non-zero counters of stored row k (kept in LDS), "some stored >
// op" is "some pair (a, c) has row[a] > c, or the row has a non-zero counter
// at an actor the op does not name (nnz[k] > the named non-zero ones)", and
// "some stored < op" is "some pair has row[a] < c": a Put costs one gather
// per (slot, pair), lane = slot.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "kernels.h"
#include "sched.h"
#include "wave.h"

namespace crdts_hip {
namespace {

using namespace wave;  // kW, sync, uni32 / uni64, lane64, shfl64, mbcnt (wave.h)

constexpr uint32_t kBigCap = 2048;   // out_cap's ABI limit (api.hip)
constexpr uint32_t kTruncCap = 1024;  // self_cap's ABI limit

// Does `ballot` (of elements base .. base + 63) have a bit inside the element
// range [sA, eA)?
__device__ __forceinline__ bool seg_any(uint64_t ballot, uint32_t base, uint32_t sA, uint32_t eA) {
  const uint32_t lo = sA > base ? sA : base, hi = eA < base + kW ? eA : base + kW;
  if (lo >= hi) return false;
  const uint32_t w = hi - lo;
  const uint64_t m = (w >= 64u ? ~0ull : ((1ull << w) - 1ull)) << (lo - base);
  return (ballot & m) != 0ull;
}

// ------------------------------------------------------------------ fast tier
__global__ __launch_bounds__(256) void mvreg_apply_kernel(
    const uint32_t* __restrict__ sn, const uint64_t* __restrict__ sclk, const uint64_t* __restrict__ sval, uint32_t scap,
    crdt_mvreg_ops P, uint32_t* __restrict__ outn, uint64_t* __restrict__ outclk, uint64_t* __restrict__ outval,
    uint32_t outcap, uint64_t n_obj, uint32_t A, uint32_t per_wave, int* __restrict__ status) {
  extern __shared__ uint64_t ra_s[];
  const uint32_t lane = threadIdx.x & (kW - 1u), wave = threadIdx.x / kW, W = blockDim.x / kW;
  uint64_t* Wk = ra_s + (size_t)wave * (per_wave / 8u);  // [outcap][A]
  uint64_t* oc = Wk + (size_t)outcap * A;                 // [A]: the op's clock, dense
  uint64_t* V = oc + A;                                   // [outcap]
  uint8_t* tab = (uint8_t*)(V + outcap);                  // [outcap]: output slot -> physical slot
  const uint32_t AO = outcap * A;
  const uint32_t k0 = lane / A, x0 = lane % A, dk = kW / A, dx = kW % A;  // lane's first element; per step of 64
  const uint32_t sA = lane * A, eA = sA + A;                              // slot `lane`'s element range
  const uint32_t pf = scap * A < kW ? scap * A : kW;
  const uint64_t stride = (uint64_t)gridDim.x * W, nops = (uint64_t)P.n_ops, nclk = (uint64_t)P.n_clk;

  // stage A (two objects ahead): the op bounds; stage B (one ahead): the slot
  // count, the first 64 clock elements, the values, the first 64 op headers
  uint64_t alo = 0, ahi = 0;
  uint32_t bn = 0;
  uint64_t bS = 0, bV = 0, bhv = 0, bhe = 0, bpb = 0, blo = 0, bhi = 0;
  auto stage_a = [&](uint64_t u) {
    alo = u ? P.obj_end[u - 1u] : 0ull;
    ahi = P.obj_end[u];
  };
  auto stage_b = [&](uint64_t u) {
    blo = uni64(alo);
    bhi = uni64(ahi);
    bn = sn[u];
    if (lane < scap) bV = sval[u * scap + lane];
    if (lane < pf) bS = sclk[u * scap * A + lane];
    bhv = bhe = bpb = 0ull;
    if (blo <= bhi && bhi <= nops) {  // else the object latches CRDT_ENONCANON: nothing of its ops is read
      if (lane < bhi - blo) {
        bhv = P.val[blo + lane];
        bhe = P.clk_end[blo + lane];
      }
      if (blo) bpb = P.clk_end[blo - 1u];
    }
  };
  uint64_t o = (uint64_t)blockIdx.x * W + wave;
  if (o < n_obj) {
    stage_a(o);
    stage_b(o);
    if (o + stride < n_obj) stage_a(o + stride);
  }
  for (; o < n_obj; o += stride) {
    const uint32_t ns = uni32(bn);
    const uint64_t cS = bS, cV = bV, lo = blo, hi = bhi;
    uint64_t hv = bhv, he = bhe, pb = uni64(bpb);
    if (o + stride < n_obj) {
      stage_b(o + stride);
      if (o + 2u * stride < n_obj) stage_a(o + 2u * stride);
    }
    if (ns > scap || lo > hi || hi > nops) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    // the first 64 clock pairs of the object's ops
    uint32_t pa = 0u;
    uint64_t pc = 0ull;
    if (lo < hi && pb < nclk && lane < nclk - pb) {
      pa = P.clk_act[pb + lane];
      pc = P.clk_ctr[pb + lane];
    }
    sync();  // the previous object's readers of the region are done
    if (lane < ns * A) Wk[lane] = cS;
    for (uint32_t e = kW + lane; e < ns * A; e += kW) Wk[e] = sclk[o * scap * A + e];
    if (lane < ns) V[lane] = cV;
    uint64_t used = ns >= 64u ? ~0ull : ((1ull << ns) - 1ull);  // physical slots in use (bit k: slot k)
    uint32_t hw = ns;                                            // one past the highest used slot
    int err = 0;
    for (uint64_t j = lo; j < hi; ++j) {
      const uint32_t t = (uint32_t)(j - lo) & (kW - 1u);
      if (t == 0u && j > lo) {  // the next 64 headers and their first 64 pairs
        const bool inb = lane < hi - j;
        hv = inb ? P.val[j + lane] : 0ull;
        he = inb ? P.clk_end[j + lane] : 0ull;
        pb = uni64(P.clk_end[j - 1u]);
        const bool pin = pb < nclk && lane < nclk - pb;
        pa = pin ? P.clk_act[pb + lane] : 0u;
        pc = pin ? P.clk_ctr[pb + lane] : 0ull;
      }
      const uint64_t clo = t ? lane64(he, t - 1u) : pb, chi = lane64(he, t);
      if (clo > chi || chi > nclk || chi - clo > A) {  // strictly increasing actors below A: at most A pairs
        err = CRDT_ENONCANON;
        break;
      }
      const uint32_t np = (uint32_t)(chi - clo);
      if (np == 0u) continue;  // an empty Put clock: unchanged
      const uint64_t val = lane64(hv, t);
      sync();  // the previous op's reads of oc are done
      for (uint32_t x = lane; x < A; x += kW) oc[x] = 0ull;
      sync();
      bool cbad = false;
      if (chi - pb <= kW) {  // its pairs are staged, from lane clo - pb
        const uint32_t f = (uint32_t)(clo - pb);
        const uint32_t a = (uint32_t)__shfl((int)pa, (int)(f + lane), kW);
        const uint32_t ap = (uint32_t)__shfl((int)pa, (int)(f + lane - 1u), kW);
        const uint64_t c = shfl64(pc, f + lane);
        if (lane < np) {
          cbad = c == 0ull || a >= A || (lane && ap >= a);
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
      // one compare per stored element; slot `lane` collects its segment's flags
      bool gt = false, lt = false;
      {
        uint32_t x = x0;
        const uint32_t E = hw * A;
        for (uint32_t base = 0; base < E; base += kW) {
          const uint32_t e = base + lane;
          bool g = false, l = false;
          if (e < E) {
            const uint64_t s = Wk[e], c = oc[x];
            g = s > c;
            l = s < c;
          }
          const uint64_t G = __ballot(g), L = __ballot(l);
          gt = gt || seg_any(G, base, sA, eA);
          lt = lt || seg_any(L, base, sA, eA);
          x += dx;
          if (x >= A) x -= A;
        }
      }
      const bool mine = lane < hw && ((used >> lane) & 1ull);
      const uint64_t keep = __ballot(mine && gt);          // not <= the Put clock
      const uint64_t dom = __ballot(mine && gt && !lt);    // strictly greater than it
      const uint32_t nk = (uint32_t)__popcll(keep);
      const bool add = dom == 0ull;
      if (nk + (add ? 1u : 0u) > outcap) {
        err = CRDT_ECAPACITY;
        break;
      }
      used = keep;
      hw = used ? 64u - (uint32_t)__builtin_clzll(used) : 0u;
      if (!add) continue;
      if (hw == outcap) {  // holes below: move the kept rows down, in order
        uint32_t dst = 0u;
        for (uint32_t s = 0; s < hw; ++s) {
          if (!((used >> s) & 1ull)) continue;
          if (dst != s) {
            for (uint32_t x = lane; x < A; x += kW) Wk[dst * A + x] = Wk[s * A + x];
            if (lane == 0u) V[dst] = V[s];
          }
          ++dst;
        }
        hw = dst;
        used = (1ull << hw) - 1ull;  // hw < outcap <= 64
      }
      for (uint32_t x = lane; x < A; x += kW) Wk[hw * A + x] = oc[x];
      if (lane == 0u) V[hw] = val;
      used |= 1ull << hw;
      ++hw;
    }
    if (err) {
      if (lane == 0u) atomicCAS(status, 0, err);
      continue;
    }
    const uint32_t nk = (uint32_t)__popcll(used);
    if (lane < hw && ((used >> lane) & 1ull)) tab[mbcnt(used)] = (uint8_t)lane;
    sync();
    if (lane == 0u) outn[o] = nk;
    if (lane < outcap) outval[o * outcap + lane] = lane < nk ? V[tab[lane]] : 0ull;
    uint64_t* od = outclk + o * (uint64_t)AO;
    uint32_t k = k0, x = x0;
    for (uint32_t e = lane; e < AO; e += kW) {
      od[e] = k < nk ? Wk[(uint32_t)tab[k] * A + x] : 0ull;
      k += dk;
      x += dx;
      if (x >= A) { x -= A; ++k; }
    }
  }
}

// --------------------------------------------------------------- general tier
// The kept rows of W[0, hw) moved down in order (used_s: which are kept);
// returns their count. Every row moves with the same lane <-> actor mapping.
__device__ uint32_t big_compact(uint64_t* W, uint64_t* V, uint32_t* nnz_s, uint8_t* used_s, uint32_t hw, uint32_t A,
                                uint32_t lane) {
  sync();
  uint32_t dst = 0u;
  for (uint32_t s = 0; s < hw; ++s) {
    if (!uni32(used_s[s])) continue;
    if (dst != s) {
      for (uint32_t x = lane; x < A; x += kW) W[(uint64_t)dst * A + x] = W[(uint64_t)s * A + x];
      if (lane == 0u) {
        V[dst] = V[s];
        nnz_s[dst] = nnz_s[s];
      }
    }
    ++dst;
  }
  sync();
  for (uint32_t k = lane; k < hw; k += kW) used_s[k] = k < dst ? 1u : 0u;
  sync();
  return dst;
}

__global__ __launch_bounds__(kW) void mvreg_apply_big_kernel(
    const uint32_t* __restrict__ sn, const uint64_t* __restrict__ sclk, const uint64_t* __restrict__ sval, uint32_t scap,
    crdt_mvreg_ops P, uint32_t* __restrict__ outn, uint64_t* __restrict__ outclk, uint64_t* __restrict__ outval,
    uint32_t outcap, uint64_t n_obj, uint32_t A, int* __restrict__ status) {
  __shared__ uint32_t nnz_s[kBigCap];  // non-zero counters of stored row k
  __shared__ uint8_t used_s[kBigCap];
  const uint32_t lane = threadIdx.x;
  const uint64_t nops = (uint64_t)P.n_ops, nclk = (uint64_t)P.n_clk;
  for (uint64_t o = blockIdx.x; o < n_obj; o += gridDim.x) {
    const uint32_t ns = uni32(sn[o]);
    const uint64_t lo = o ? uni64(P.obj_end[o - 1u]) : 0ull, hi = uni64(P.obj_end[o]);
    if (ns > scap || lo > hi || hi > nops) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    uint64_t* W = outclk + o * (uint64_t)outcap * A;
    uint64_t* V = outval + o * (uint64_t)outcap;
    const uint64_t* S = sclk + o * (uint64_t)scap * A;
    sync();  // the previous object's readers of nnz_s / used_s are done
    for (uint32_t k = 0; k < ns; ++k) {
      uint32_t cnt = 0u;
      for (uint32_t x0 = 0; x0 < A; x0 += kW) {
        const uint32_t x = x0 + lane;
        uint64_t v = 0ull;
        if (x < A) {
          v = S[(uint64_t)k * A + x];
          W[(uint64_t)k * A + x] = v;
        }
        cnt += (uint32_t)__popcll(__ballot(v != 0ull));
      }
      if (lane == 0u) {
        nnz_s[k] = cnt;
        used_s[k] = 1u;
      }
    }
    for (uint32_t k = lane; k < ns; k += kW) V[k] = sval[o * scap + k];
    uint32_t hw = ns, cnt = ns;
    int err = 0;
    uint64_t clo = lo ? uni64(P.clk_end[lo - 1u]) : 0ull;
    sync();
    for (uint64_t j = lo; j < hi; ++j) {
      const uint64_t chi = uni64(P.clk_end[j]);
      if (clo > chi || chi > nclk || chi - clo > A) {
        err = CRDT_ENONCANON;
        break;
      }
      const uint32_t np = (uint32_t)(chi - clo);
      const uint64_t c0 = clo;
      clo = chi;
      if (np == 0u) continue;
      bool cbad = false;
      for (uint32_t p = lane; p < np; p += kW) {
        const uint32_t a = P.clk_act[c0 + p];
        cbad = cbad || P.clk_ctr[c0 + p] == 0ull || a >= A || (p && P.clk_act[c0 + p - 1u] >= a);
      }
      if (__ballot(cbad) != 0ull) {
        err = CRDT_ENONCANON;
        break;
      }
      uint32_t nk = 0u;
      bool anydom = false;
      for (uint32_t b = 0; b < hw; b += kW) {
        const uint32_t k = b + lane;
        bool keep = false, dom = false;
        if (k < hw && used_s[k]) {
          const uint64_t* row = W + (uint64_t)k * A;
          bool gt = false, lt = false;
          uint32_t named = 0u;
          for (uint32_t p = 0; p < np; ++p) {
            const uint64_t r = row[P.clk_act[c0 + p]], c = P.clk_ctr[c0 + p];
            gt = gt || r > c;
            lt = lt || r < c;
            named += r != 0ull ? 1u : 0u;
          }
          gt = gt || nnz_s[k] > named;
          keep = gt;
          dom = gt && !lt;
          if (!keep) used_s[k] = 0u;
        }
        const uint64_t K = __ballot(keep), D = __ballot(dom);
        nk += (uint32_t)__popcll(K);
        anydom = anydom || D != 0ull;
      }
      if (nk + (anydom ? 0u : 1u) > outcap) {
        err = CRDT_ECAPACITY;
        break;
      }
      cnt = nk;
      if (anydom) continue;
      if (hw == outcap) hw = big_compact(W, V, nnz_s, used_s, hw, A, lane);
      sync();
      for (uint32_t x = lane; x < A; x += kW) W[(uint64_t)hw * A + x] = 0ull;
      sync();
      for (uint32_t p = lane; p < np; p += kW) W[(uint64_t)hw * A + P.clk_act[c0 + p]] = P.clk_ctr[c0 + p];
      if (lane == 0u) {
        V[hw] = P.val[j];
        nnz_s[hw] = np;
        used_s[hw] = 1u;
      }
      ++hw;
      ++cnt;
      sync();
    }
    if (err) {
      if (lane == 0u) atomicCAS(status, 0, err);
      continue;
    }
    if (cnt != hw) hw = big_compact(W, V, nnz_s, used_s, hw, A, lane);
    for (uint64_t e = (uint64_t)hw * A + lane; e < (uint64_t)outcap * A; e += kW) W[e] = 0ull;
    for (uint32_t k = hw + lane; k < outcap; k += kW) V[k] = 0ull;
    if (lane == 0u) outn[o] = hw;
  }
}

// ------------------------------------------------------------------- truncate
// One wave per register. The kept slots (some counter above the truncating
// clock's) go to the wave's slot table; the output block is then written
// slot-major in one coalesced pass, subtracting on the way.
__global__ __launch_bounds__(256) void mvreg_truncate_kernel(
    const uint32_t* __restrict__ sn, const uint64_t* __restrict__ sclk, const uint64_t* __restrict__ sval, uint32_t scap,
    const uint64_t* __restrict__ clock, uint32_t* __restrict__ outn, uint64_t* __restrict__ outclk,
    uint64_t* __restrict__ outval, uint32_t outcap, uint64_t n_obj, uint32_t A, int* __restrict__ status) {
  __shared__ uint16_t tab_s[4][kTruncCap];
  const uint32_t lane = threadIdx.x & (kW - 1u), wave = threadIdx.x / kW, W = blockDim.x / kW;
  uint16_t* tab = tab_s[wave];
  const uint32_t x0 = lane % A, k0 = lane / A, dk = kW / A, dx = kW % A;
  const uint32_t sA = lane * A, eA = sA + A;
  const uint64_t stride = (uint64_t)gridDim.x * W, AO = (uint64_t)outcap * A;
  for (uint64_t o = (uint64_t)blockIdx.x * W + wave; o < n_obj; o += stride) {
    const uint32_t ns = uni32(sn[o]);
    if (ns > scap) {
      if (lane == 0u) atomicCAS(status, 0, CRDT_ENONCANON);
      continue;
    }
    const uint64_t* S = sclk + o * (uint64_t)scap * A;
    const uint64_t* T = clock + o * (uint64_t)A;
    sync();  // the previous object's readers of tab are done
    uint32_t nk = 0u;
    if (ns <= kW && A <= 65536u) {  // lane = element; slot `lane` collects its segment's ballot bits
      bool keep = false;
      uint32_t x = x0;
      const uint32_t E = ns * A;
      for (uint32_t base = 0; base < E; base += kW) {
        const uint32_t e = base + lane;
        const bool g = e < E && S[e] > T[x];
        const uint64_t G = __ballot(g);  // by every lane: not under the || below
        keep = keep || seg_any(G, base, sA, eA);
        x += dx;
        if (x >= A) x -= A;
      }
      keep = keep && lane < ns;
      const uint64_t m = __ballot(keep);
      if (keep) tab[mbcnt(m)] = (uint16_t)lane;
      nk = (uint32_t)__popcll(m);
    } else {  // lane = slot
      for (uint32_t b = 0; b < ns; b += kW) {
        const uint32_t k = b + lane;
        bool keep = false;
        if (k < ns)
          for (uint32_t x = 0; x < A && !keep; ++x) keep = S[(uint64_t)k * A + x] > T[x];
        const uint64_t m = __ballot(keep);
        if (keep) tab[nk + mbcnt(m)] = (uint16_t)k;
        nk += (uint32_t)__popcll(m);
      }
    }
    sync();
    if (lane == 0u) outn[o] = nk;
    for (uint32_t k = lane; k < outcap; k += kW) outval[o * outcap + k] = k < nk ? sval[o * scap + tab[k]] : 0ull;
    uint64_t* od = outclk + o * AO;
    uint32_t k = k0, x = x0;
    for (uint64_t e = lane; e < AO; e += kW) {
      uint64_t v = 0ull;
      if (k < nk) {
        v = S[(uint64_t)tab[k] * A + x];
        if (v <= T[x]) v = 0ull;
      }
      od[e] = v;
      k += dk;
      x += dx;
      if (x >= A) { x -= A; ++k; }
    }
  }
}

// ----------------------------------------------------------------- read clock
// One thread per (register, actor): the max over the used slots' counters.
__global__ __launch_bounds__(256) void mvreg_read_clock_kernel(const uint32_t* __restrict__ sn,
                                                                const uint64_t* __restrict__ sclk, uint32_t scap,
                                                                uint64_t* __restrict__ out, uint64_t n_obj, uint32_t A,
                                                                int* __restrict__ status) {
  const uint64_t total = n_obj * A, step = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const uint64_t o = i / A;
    const uint32_t x = (uint32_t)(i - o * A);
    uint32_t ns = sn[o];
    if (ns > scap) {
      atomicCAS(status, 0, CRDT_ENONCANON);
      ns = 0u;
    }
    const uint64_t* S = sclk + o * (uint64_t)scap * A + x;
    uint64_t m = 0ull;
    for (uint32_t k = 0; k < ns; ++k) {
      const uint64_t v = S[(uint64_t)k * A];
      m = v > m ? v : m;
    }
    out[i] = m;
  }
}

}  // namespace

int launch_mvreg_apply(const uint32_t* sn, const uint64_t* sclk, const uint64_t* sval, uint32_t scap,
                       const crdt_mvreg_ops& P, uint32_t* outn, uint64_t* outclk, uint64_t* outval, uint32_t outcap,
                       uint64_t n_obj, uint32_t A, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  if (outcap > kBigCap || scap > outcap) return CRDT_EINVAL;
  const uint64_t cus = (uint64_t)cu_count();
  // per-wave LDS: the block, the op row, the values, the slot table; 16-B multiple
  const size_t per_wave = (8ull * ((size_t)outcap * A + A + outcap) + outcap + 15u) & ~15ull;
  if (outcap > 64u || per_wave > 60u * 1024u) {
    const uint64_t cap = cus * 16u;
    hipLaunchKernelGGL(mvreg_apply_big_kernel, dim3((uint32_t)(n_obj < cap ? n_obj : cap)), dim3(kW), 0, stream, sn,
                       sclk, sval, scap, P, outn, outclk, outval, outcap, n_obj, A, status);
    return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
  }
  uint32_t W = 4;  // waves per block, as many as 60 KB of LDS allow
  while (W > 1u && W * per_wave > 60u * 1024u) --W;
  // 64 waves per SIMD's worth of blocks, ~13 times the resident 5: blocks are
  // handed out as others finish (13 % faster than a resident grid), and a wave
  // still has objects to prefetch ahead of
  const uint64_t want = (n_obj + W - 1) / W, cap = cus * (256u / W);
  hipLaunchKernelGGL(mvreg_apply_kernel, dim3((uint32_t)(want < cap ? want : cap)), dim3(kW * W), W * per_wave, stream,
                     sn, sclk, sval, scap, P, outn, outclk, outval, outcap, n_obj, A, (uint32_t)per_wave, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_mvreg_truncate(const uint32_t* sn, const uint64_t* sclk, const uint64_t* sval, uint32_t scap,
                          const uint64_t* clock, uint32_t* outn, uint64_t* outclk, uint64_t* outval, uint32_t outcap,
                          uint64_t n_obj, uint32_t A, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  if (scap > kTruncCap || scap > outcap) return CRDT_EINVAL;
  const uint64_t want = (n_obj + 3u) / 4u, cap = (uint64_t)cu_count() * 8u;  // 8 waves per SIMD
  hipLaunchKernelGGL(mvreg_truncate_kernel, dim3((uint32_t)(want < cap ? want : cap)), dim3(256), 0, stream, sn, sclk,
                     sval, scap, clock, outn, outclk, outval, outcap, n_obj, A, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_mvreg_read_clock(const uint32_t* sn, const uint64_t* sclk, uint32_t scap, uint64_t* out, uint64_t n_obj,
                            uint32_t A, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const uint64_t want = (n_obj * A + 255u) / 256u, cap = (uint64_t)cu_count() * 8u;
  hipLaunchKernelGGL(mvreg_read_clock_kernel, dim3((uint32_t)(want < cap ? want : cap)), dim3(256), 0, stream, sn,
                     sclk, scap, out, n_obj, A, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
