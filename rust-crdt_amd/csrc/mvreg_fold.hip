// MVReg fold: out[i] = reps[0][i].merge(reps[1][i]).merge(reps[2][i])... in
// rank order (MVReg<V, A>::merge, src/mvreg.rs:121-153, V = u64), R replicas'
// slabs in one pass: every replica's used rows are read once, the output is
// written once, no intermediate register leaves the chip.
//
// The chain has an exact one-pass form. Write (r, k) for used slot k of
// replica r and `>` for strictly greater (VClock::partial_cmp):
//   1. (r, k) is dropped when a used slot of another replica is > it. (A slot
//      that only its own replica dominates is kept, as merge keeps it.)
//   2. Otherwise a slot of replica 0 is kept, duplicates inside it included.
//   3. Otherwise (r >= 1) it is dropped as already kept when an equal clock
//      sits at an earlier slot of replica r, or when an equal clock sits in an
//      earlier replica and no slot of replica r is > this clock (when one is,
//      it dropped the earlier equal entry in the same step of the chain and
//      this one is new).
//   4. Survivors come out in (r, k) order.
// Why 1 is exact: whatever drops a slot in the chain is itself kept or dropped
// by something no smaller from another step, so a clock >= the dominator, of
// another replica than r, survives to meet (r, k). Why 3 is exact: the
// earliest equal clock e of the earlier replicas either lives to step r (then
// (r, k) is its duplicate, unless replica r drops e in that very step) or was
// dropped by a replica other than r, which rule 1 applies to (r, k) as well.
// tests/mvreg_foldgen.py restates the rule in numpy and checks it against the
// chained merge on every batch the GPU tests use.
//
// Tiers. T = the capacities' sum. The fast kernel takes T <= 64 when a wave's
// LDS region, 8 T n_actors + 18 T bytes rounded up to 16 (the rows by capacity
// slot; the T x T relation as two 64-bit sets per slot, its dominators and its
// equals; the used-slot list; the output slot table), is at most 60 KB; a
// block holds as many waves, 4 at the most, as 60 KB allow. Everything else
// takes the one-wave-per-register kernel, which compares the rows in HBM.
#include <hip/hip_runtime.h>

#include <cassert>

#include "../../include/crdts_hip.h"
#include "kernels.h"
#include "sched.h"
#include "wave.h"

namespace crdts_hip {
namespace {

using namespace wave;  // sync, lane32, mbcnt, fail (wave.h)

constexpr uint32_t kMaxReps = CRDT_MVREG_MAX_REPS;
constexpr uint32_t kFoldBigCap = 2048;  // slots of all replicas, one-wave kernel
constexpr uint32_t kPf = 8;             // replicas whose first 64 clock words are prefetched, at the most
constexpr size_t kFoldLds = 60u * 1024u;

// the replicas' views and the capacity slots' layout: replica r's slot k is
// capacity slot base[r] + k; base[r] = T from r = n_reps on
struct FoldViews {
  const uint32_t* n[kMaxReps];
  const uint64_t* clk[kMaxReps];
  const uint64_t* val[kMaxReps];
  uint16_t cap[kMaxReps];
  uint16_t base[kMaxReps + 1u];
};

// 1: some a > b, 2: some a < b (mvreg.hip's mv_cmp_rows, which is private to that file)
__device__ __forceinline__ uint32_t fold_cmp_rows(const uint64_t* a, const uint64_t* b, uint32_t A) {
  uint32_t f = 0u;
  for (uint32_t x = 0; x < A; ++x) f |= (a[x] > b[x] ? 1u : 0u) | (a[x] < b[x] ? 2u : 0u);
  return f;
}

__device__ __forceinline__ uint64_t low_bits(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }
// a bit set in LDS that several lanes of the wave add to
__device__ __forceinline__ void lds_or(uint64_t* p, uint64_t v) {
  __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One wave per register, W waves per block, each with its own LDS region
// (`per_wave` bytes). Lane c < T stands for capacity slot c; lane r < R holds
// replica r's slot count. Output rows are written slot-major in one coalesced
// pass, as mvreg_merge_kernel writes them.
// NPF: the replicas whose first 64 clock words are prefetched, 1, 2, 4 or kPf
// (the launcher takes the smallest that covers n_reps). Each costs a register
// pair, and registers are occupancy here: 8 waves per SIMD at NPF = 2, 7 at 4,
// 5 at 8, and this kernel's time follows its occupancy.
template <uint32_t NPF>
__global__ __launch_bounds__(256) void mvreg_fold_kernel(FoldViews P, uint32_t R, uint32_t T,
                                                         uint32_t* __restrict__ outn, uint64_t* __restrict__ outclk,
                                                         uint64_t* __restrict__ outval, uint32_t outcap, uint64_t n_obj,
                                                         uint32_t A, uint32_t per_wave, int* __restrict__ status) {
  extern __shared__ uint64_t mf_s[];
  const uint32_t lane = threadIdx.x & (kW - 1u), wave = threadIdx.x / kW, W = blockDim.x / kW;
  uint64_t* S = mf_s + (size_t)wave * (per_wave / 8u);  // [T][A] by capacity slot, used rows only
  uint64_t* bits = S + (size_t)T * A;                   // [c][2]: the slots > slot c, the slots == slot c, as bit sets
  uint8_t* ul = (uint8_t*)(bits + 2u * T);              // [t]: the t-th used slot
  uint8_t* tab = ul + T;                                // [k]: output slot -> capacity slot
  const uint32_t AO = outcap * A;
  // this lane's capacity slot (lane < T) and replica count (lane < R)
  uint32_t rc = 0u;
  for (uint32_t r = 1; r < R; ++r) rc = lane >= P.base[r] ? r : rc;
  const bool incap = lane < T;
  const uint32_t cb = P.base[rc], ce = P.base[rc + 1u], kc = lane - cb, vstr = P.cap[rc];
  const uint64_t* vptr = P.val[rc] + kc;
  const uint32_t* nptr = P.n[lane < R ? lane : 0u];
  const uint32_t capr = lane < R ? P.cap[lane] : 0u;
  const uint32_t npf = R < NPF ? R : NPF;
  // the slots of this lane's replica, those of them before this lane's, and the slots of earlier replicas
  const uint64_t own = low_bits(ce) & ~low_bits(cb), own_before = low_bits(lane < ce ? lane : ce) & ~low_bits(cb);
  const uint64_t earlier = low_bits(cb);
  // Software pipeline: the next register's slot counts, values (every
  // capacity slot: the counts are not known yet) and the first 64 clock words
  // of the first NPF replicas are loaded while this register is folded; they
  // go from their registers to LDS before the loads after them are issued.
  const uint64_t stride = (uint64_t)gridDim.x * W;
  uint32_t nn = 0u;
  uint64_t nV = 0ull, pf[NPF];
#pragma unroll
  for (uint32_t j = 0; j < NPF; ++j) pf[j] = 0ull;
  auto fetch = [&](uint64_t u) {
    if (lane < R) nn = nptr[u];
    if (incap) nV = vptr[u * vstr];
#pragma unroll
    for (uint32_t j = 0; j < NPF; ++j)
      if (j < npf) {
        const uint32_t w = (uint32_t)P.cap[j] * A;
        if (lane < w) pf[j] = P.clk[j][u * w + lane];
      }
  };
  uint64_t o = (uint64_t)blockIdx.x * W + wave;
  if (o < n_obj) fetch(o);
  for (; o < n_obj; o += stride) {
    const uint32_t cn = nn;
    const uint64_t cV = nV;
    const bool canon = __ballot(cn > capr) == 0ull;
    sync();  // the previous register's readers of the region are done
    if (canon) {
#pragma unroll
      for (uint32_t j = 0; j < NPF; ++j)
        if (j < npf && lane < lane32(cn, j) * A) S[(uint32_t)P.base[j] * A + lane] = pf[j];
    }
    if (o + stride < n_obj) fetch(o + stride);
    if (!canon) {
      if (lane == 0u) fail(status, CRDT_ENONCANON);
      continue;
    }
    for (uint32_t r = 0; r < R; ++r) {
      const uint32_t w = lane32(cn, r) * A, b = (uint32_t)P.base[r] * A;
      const uint64_t* src = P.clk[r] + o * P.cap[r] * A;
      for (uint32_t k = (r < npf ? kW : 0u) + lane; k < w; k += kW) S[b + k] = src[k];
    }
    const bool used = incap && kc < (uint32_t)__shfl((int)cn, (int)rc, kW);
    const uint64_t UM = __ballot(used);
    if (used) ul[mbcnt(UM)] = (uint8_t)lane;
    if (incap) bits[2u * lane] = bits[2u * lane + 1u] = 0ull;
    sync();
    {  // the relation matrix: replica 0's slots against the others', then every pair of the others' (V of
       // them; with V' = V | 1, the pairs {a, a + d mod V'}, d = 1..V'/2, are each unordered pair once).
       // G lanes per pair (the largest power of two with G pairs <= 64 and G <= A), strided over the
       // actors, OR-reduced.
      const uint32_t n0 = lane32(cn, 0u), U = (uint32_t)__popcll(UM), V = U - n0, D = V >> 1, Vp = V | 1u;
      const uint32_t P1 = n0 * V, PP = P1 + Vp * D;
      const uint32_t lgp = PP <= 1u ? 0u : 32u - (uint32_t)__builtin_clz(PP - 1u);  // ceil(log2(pairs))
      const uint32_t lga = 31u - (uint32_t)__builtin_clz(A);
      const uint32_t lg = lgp >= 6u ? 0u : (6u - lgp < lga ? 6u - lgp : lga), G = 1u << lg;
      for (uint32_t base = 0; base < PP << lg; base += kW) {
        const uint32_t id = base + lane, p = id >> lg, gl = id & (G - 1u);
        bool valid = false;
        uint32_t t = 0u, u = 0u, f = 0u;
        if (p < P1) {
          t = p / V;
          u = n0 + p % V;
          valid = true;
        } else if (p < PP) {
          const uint32_t q = p - P1, a = q / D;
          uint32_t b = a + q % D + 1u;
          b = b >= Vp ? b - Vp : b;
          valid = a < V && b < V;
          t = n0 + a;
          u = n0 + b;
        }
        uint32_t ct = 0u, cu = 0u;
        if (valid) {
          ct = ul[t];
          cu = ul[u];
          const uint64_t* pa = S + ct * A;
          const uint64_t* pb = S + cu * A;
          for (uint32_t x = gl; x < A; x += G) {
            const uint64_t va = pa[x], vb = pb[x];
            f |= (va > vb ? 1u : 0u) | (va < vb ? 2u : 0u);
          }
        }
        for (uint32_t off = 1; off < G; off <<= 1) f |= (uint32_t)__shfl_xor((int)f, (int)off, kW);
        if (valid && gl == 0u && f != 3u) {  // (3: concurrent, no bit)
          // 0: equal, both rows; 2: t < u, t's row; 1: u < t, u's row
          const uint32_t lo = f == 1u ? cu : ct, hi = f == 1u ? ct : cu, w = f == 0u ? 1u : 0u;
          lds_or(bits + 2u * lo + w, 1ull << hi);
          if (f == 0u) lds_or(bits + 2u * hi + 1u, 1ull << lo);
        }
      }
    }
    sync();
    // the rule, per used slot (pairs inside replica 0 are not compared: its slots have no `own` bits)
    uint64_t lt = 0ull, eq = 0ull;
    if (used) {
      lt = bits[2u * lane];
      eq = bits[2u * lane + 1u];
    }
    const bool domo = (lt & ~own) != 0ull;                      // another replica's clock is > this one
    // already kept: an earlier equal slot of its replica, or an equal clock in
    // an earlier replica that no clock of its own replica drops
    const bool dup = (eq & own_before) != 0ull || ((eq & earlier) != 0ull && (lt & own) == 0ull);
    const bool keep = used && !domo && !dup;
    const uint64_t K = __ballot(keep);
    const uint32_t nk = (uint32_t)__popcll(K);
    if (nk > outcap) {
      if (lane == 0u) fail(status, CRDT_ECAPACITY);
      continue;
    }
    const uint32_t rk = mbcnt(K);
    if (keep) tab[rk] = (uint8_t)lane;
    if (lane == 0u) outn[o] = nk;
    if (keep) outval[o * outcap + rk] = cV;
    for (uint32_t k = nk + lane; k < outcap; k += kW) outval[o * outcap + k] = 0u;
    sync();
    uint64_t* oc = outclk + o * (uint64_t)AO;
    uint32_t k = lane / A, x = lane % A;        // slot and actor of this lane's first element
    const uint32_t dk = kW / A, dx = kW % A;  // per step of 64 elements
    for (uint32_t e = lane; e < AO; e += kW) {
      uint64_t v = 0ull;
      if (k < nk) v = S[(uint32_t)tab[k] * A + x];
      oc[e] = v;
      k += dk;
      x += dx;
      if (x >= A) { x -= A; ++k; }
    }
  }
}

// Registers past the fast kernel's limits: one wave per register, one lane
// per capacity slot in rounds of 64, the clock rows compared in HBM, the same
// rule and output form; the kept flags of the current register in LDS.
__global__ __launch_bounds__(kW) void mvreg_fold_big_kernel(FoldViews P, uint32_t R, uint32_t T,
                                                            uint32_t* __restrict__ outn, uint64_t* __restrict__ outclk,
                                                            uint64_t* __restrict__ outval, uint32_t outcap,
                                                            uint64_t n_obj, uint32_t A, int* __restrict__ status) {
  __shared__ uint8_t ks_s[kFoldBigCap];   // kept flags by capacity slot
  __shared__ uint8_t rep_s[kFoldBigCap];  // the replica of a capacity slot
  __shared__ uint32_t cnt_s[kMaxReps];
  const uint32_t lane = threadIdx.x;
  for (uint32_t c = lane; c < T; c += kW) {
    uint32_t r = 0u;
    for (uint32_t q = 1; q < R; ++q) r = c >= P.base[q] ? q : r;
    rep_s[c] = (uint8_t)r;
  }
  for (uint64_t o = blockIdx.x; o < n_obj; o += gridDim.x) {
    sync();  // rep_s is written; the previous register's readers of ks_s and cnt_s are done
    const uint32_t cn = lane < R ? P.n[lane][o] : 0u;
    if (__ballot(lane < R && cn > P.cap[lane]) != 0ull) {
      if (lane == 0u) fail(status, CRDT_ENONCANON);
      continue;
    }
    if (lane < R) cnt_s[lane] = cn;
    sync();
    uint32_t nk = 0u;
    for (uint32_t c0 = 0; c0 < T; c0 += kW) {
      const uint32_t c = c0 + lane;
      bool keep = false;
      if (c < T) {
        const uint32_t r = rep_s[c], k = c - P.base[r];
        if (k < cnt_s[r]) {
          const uint64_t* row = P.clk[r] + (o * P.cap[r] + k) * A;
          bool domo = false, domw = false, eqw = false, eqe = false;
          for (uint32_t q = r == 0u ? 1u : 0u; q < R && !domo; ++q) {
            const uint32_t nq = cnt_s[q];
            const uint64_t* oq = P.clk[q] + o * P.cap[q] * A;
            for (uint32_t j = 0; j < nq && !domo; ++j) {
              if (q == r && j == k) continue;
              const uint32_t f = fold_cmp_rows(row, oq + (uint64_t)j * A, A);
              if (q != r) {
                domo = f == 2u;
                eqe = eqe || (q < r && f == 0u);
              } else {
                domw = domw || f == 2u;
                eqw = eqw || (j < k && f == 0u);
              }
            }
          }
          keep = !domo && (r == 0u || !(eqw || (eqe && !domw)));
        }
        ks_s[c] = keep ? 1u : 0u;
      }
      nk += (uint32_t)__popcll(__ballot(keep));
    }
    if (nk > outcap) {
      if (lane == 0u) fail(status, CRDT_ECAPACITY);
      continue;
    }
    sync();
    // survivors in order, one row per lane-round; then the unused slots zeroed
    uint64_t* oc = outclk + o * (uint64_t)outcap * A;
    uint32_t pos = 0u;
    for (uint32_t c0 = 0; c0 < T; c0 += kW) {
      const uint32_t c = c0 + lane;
      const bool keep = c < T && ks_s[c];
      const uint64_t m = __ballot(keep);
      const uint32_t rk = pos + mbcnt(m);
      if (keep) {
        const uint32_t r = rep_s[c], k = c - P.base[r];
        const uint64_t* src = P.clk[r] + (o * P.cap[r] + k) * A;
        for (uint32_t x = 0; x < A; ++x) oc[(uint64_t)rk * A + x] = src[x];
        outval[o * outcap + rk] = P.val[r][o * P.cap[r] + k];
      }
      pos += (uint32_t)__popcll(m);
    }
    for (uint64_t e = (uint64_t)nk * A + lane; e < (uint64_t)outcap * A; e += kW) oc[e] = 0ull;
    for (uint32_t k = nk + lane; k < outcap; k += kW) outval[o * outcap + k] = 0u;
    if (lane == 0u) outn[o] = nk;
  }
}

}  // namespace

int launch_mvreg_fold(const crdt_mvreg_view* reps, uint32_t n_reps, uint32_t* outn, uint64_t* outclk, uint64_t* outval,
                      uint32_t outcap, uint64_t n_obj, uint32_t A, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  assert(n_reps >= 1u && n_reps <= kMaxReps);  // the limits are api.hip's to reject
  FoldViews P{};
  uint32_t T = 0;
  for (uint32_t r = 0; r < n_reps; ++r) {
    assert(reps[r].cap >= 1u && reps[r].cap <= 1024u);
    P.n[r] = reps[r].n;
    P.clk[r] = reps[r].clk;
    P.val[r] = reps[r].val;
    P.cap[r] = (uint16_t)reps[r].cap;
    P.base[r] = (uint16_t)T;
    T += reps[r].cap;
  }
  assert(T <= kFoldBigCap);
  for (uint32_t r = n_reps; r <= kMaxReps; ++r) P.base[r] = (uint16_t)T;
  for (uint32_t r = n_reps; r < kMaxReps; ++r) {  // (never dereferenced)
    P.n[r] = P.n[0];
    P.clk[r] = P.clk[0];
    P.val[r] = P.val[0];
  }
  // per-wave LDS: rows by capacity slot, relation bit sets, used-slot list, slot table; 16-B multiple
  const size_t per_wave = (8ull * T * A + 18ull * T + 15u) & ~15ull;
  if (T > kW || per_wave > kFoldLds) {  // past the fast kernel's limits
    hipLaunchKernelGGL(mvreg_fold_big_kernel, dim3(resident_blocks(n_obj, 16u)), dim3(kW), 0, stream, P, n_reps, T,
                       outn, outclk, outval, outcap, n_obj, A, status);
    return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
  }
  uint32_t W = 4;  // waves per block, as many as 60 KB of LDS allow
  while (W > 1u && W * per_wave > kFoldLds) --W;
  const uint32_t blocks = resident_blocks((n_obj + W - 1) / W, 32u / W);  // ~8 waves per SIMD
  auto* kernel = n_reps <= 1u ? mvreg_fold_kernel<1> : n_reps <= 2u ? mvreg_fold_kernel<2>
                 : n_reps <= 4u ? mvreg_fold_kernel<4> : mvreg_fold_kernel<kPf>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kW * W), W * per_wave, stream, P, n_reps, T, outn, outclk, outval,
                     outcap, n_obj, A, (uint32_t)per_wave, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
