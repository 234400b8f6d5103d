// Rank-order fold of R replicas of a VClock / GCounter / PNCounter batch in
// one launch (include/crdts_hip.h "Clock and counter fold"): the chain
// reps[0].merge(reps[1]).merge(reps[2])... of VClock::merge
// (src/vclock.rs:131-137; GCounter src/gcounter.rs:58-62 and PNCounter
// src/pncounter.rs:90-95 delegate to it), which is a max per actor and so has
// no order: every replica entry is read once, the output is written once, no
// intermediate union goes through HBM.
//
// Dense rows: flat over n_obj * n_slots words, R + 1 words of traffic per slot
// against the chain's 3 (R - 1). The R pointers travel by value in the launch
// struct; a lane reads its words from every replica before it writes them, so
// the output may be one of the replicas.
//
// CSR runs: csr_merge.hip's outer shape — a resident grid, a wave per object,
// chunks of 64 objects (lane k <-> object c + k) whose R offsets and lengths
// are loaded coalesced and checked per replica. Inside a chunk lane r stands
// for replica r: it holds the run of the current object in replica r, and the
// next object's runs are in flight while the current one is folded.
//
// The union of one object, exact and loop-free over the output: entry (a, c)
// of replica r takes p = the sum over the replicas q of a's rank in run q (its
// own index in run r). p is strictly increasing over distinct actors and at
// most T - 1, T = the lengths' sum. The first replica that holds a owns it and
// carries the largest counter of a's holders. The owners' p form a bit set;
// the union position of an actor is the number of set bits below its p.
//
// Tiers, chosen per object on the device:
//   1. T <= 64: lane j holds entry j of the runs laid end to end; the ranks are
//      binary searches over registers (ds_bpermute); the bit set is one word.
//   2. T <= CRDT_CLOCK_FOLD_STAGE_ENTRIES: the runs are staged in LDS end to
//      end, the ranks are binary searches in LDS, an owner leaves its index at
//      src[p] and its maxed counter in place, and the union is written front
//      to back from the bit set, coalesced.
//   3. anything longer: binary searches in HBM (rank_mem); an owner writes its
//      entry at region cell p (the counters of the region are zeroed first: a
//      zero counter is never an entry), then the wave compacts the region front
//      to back. Only the object's own output region is used.
#include <hip/hip_runtime.h>

#include <cassert>

#include "../../include/crdts_hip.h"
#include "csr_rank.h"
#include "kernels.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace csr_rank;  // rd32 / rd64 / from_below / rank_regs / rank_mem / wave_incl_scan, and wave.h

constexpr uint32_t kMaxReps = CRDT_CLOCK_FOLD_MAX_REPS;

// ---------------------------------------------------------------- dense rows
typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;
constexpr int kUnroll = 4;

struct DenseRows {
  const uint64_t* p[kMaxReps];
};

__device__ __forceinline__ uint64_t vmax(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ u64x2 vmax(u64x2 a, u64x2 b) {
  u64x2 r;
  r.x = a.x > b.x ? a.x : b.x;
  r.y = a.y > b.y ? a.y : b.y;
  return r;
}

// V: u64x2 (16-B loads, every pointer 16-B aligned) or uint64_t (the tail, and unaligned rows)
template <class V>
__global__ __launch_bounds__(kThreads) void clock_dense_fold_kernel(DenseRows P, uint32_t R, V* out, uint64_t nv) {
  const uint64_t tile = (uint64_t)kThreads * kUnroll;
  for (uint64_t base = (uint64_t)blockIdx.x * tile; base < nv; base += (uint64_t)gridDim.x * tile) {
    V acc[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t k = base + (uint64_t)u * kThreads + threadIdx.x;
      if (k < nv) acc[u] = __builtin_nontemporal_load((const V*)P.p[0] + k);
    }
    for (uint32_t r = 1; r < R; ++r) {
      const V* src = (const V*)P.p[r];
      V b[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint64_t k = base + (uint64_t)u * kThreads + threadIdx.x;
        if (k < nv) b[u] = __builtin_nontemporal_load(src + k);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint64_t k = base + (uint64_t)u * kThreads + threadIdx.x;
        if (k < nv) acc[u] = vmax(acc[u], b[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {  // (every replica's word is read: out may be one of them)
      const uint64_t k = base + (uint64_t)u * kThreads + threadIdx.x;
      if (k < nv) __builtin_nontemporal_store(acc[u], out + k);
    }
  }
}

// ------------------------------------------------------------------ CSR runs
constexpr uint32_t kBlock = 256;
constexpr uint32_t kWaves = kBlock / kW;
constexpr uint32_t kStage = CRDT_CLOCK_FOLD_STAGE_ENTRIES;
constexpr uint32_t kWords = kStage / kW;  // words of the owners' bit set
static_assert(kStage % kW == 0 && kStage <= 0x8000u, "src[] holds u16 indices");

struct FoldReps {
  const uint64_t* off[kMaxReps];
  const uint32_t* len[kMaxReps];
  const uint32_t* act[kMaxReps];
  const uint64_t* ctr[kMaxReps];
  uint64_t entries[kMaxReps];
};
struct FoldOut {
  uint64_t* off;
  uint32_t* len;
  uint32_t* act;
  uint64_t* ctr;
  uint64_t entries;
};

// a wave's LDS: 14 B per staged entry, the bit set and its prefix counts
struct WaveLds {
  uint64_t ctr[kStage];
  uint32_t act[kStage];
  uint16_t src[kStage];
  uint64_t mask[kWords];
  uint32_t pref[kWords];
};

// One object's runs, lane r <-> replica r (lanes past R hold an empty run):
// n entries at ap / cp; e = the lengths' inclusive prefix sum; T = their sum.
struct Obj {
  uint64_t e, T;
  uint32_t n;
  const uint32_t* ap;
  const uint64_t* cp;
};
// entry j = lane of the runs laid end to end (tier 1): entry k of replica r
struct Ent {
  uint32_t a, r, k;
  uint64_t c;
  bool has;
};

__device__ __forceinline__ uint64_t low_bits(uint32_t n) { return n >= 64u ? ~0ull : (1ull << n) - 1ull; }
__device__ __forceinline__ void lds_or(uint64_t* p, uint64_t v) {
  __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <class T>
__device__ __forceinline__ const T* lane_ptr(const T* p, uint32_t l) {
  return (const T*)lane64((uint64_t)p, l);
}

__device__ __forceinline__ Obj make_obj(uint64_t o, uint32_t n, const uint32_t* actp, const uint64_t* ctrp,
                                        uint32_t lane) {
  Obj D;
  D.n = n;
  D.e = wave_incl_scan((uint64_t)n, lane);
  D.T = lane64(D.e, kW - 1u);
  D.ap = actp + o;
  D.cp = ctrp + o;
  return D;
}

// tier 1's loads: lane j < T takes entry j of the runs laid end to end
__device__ __forceinline__ Ent fetch_ent(const Obj& D, uint32_t lane) {
  Ent E{0u, 0u, 0u, 1ull, false};
  if (D.T <= kW) {
    const uint32_t e32 = (uint32_t)D.e;
    E.has = lane < (uint32_t)D.T;
    // the replica of entry j: the first whose end is past j (# of ends <= j)
    E.r = rank_regs(e32, kW, (E.has ? lane : 0u) + 1u) & 63u;
    E.k = lane - rd32(e32 - D.n, E.r);
    const uint32_t* ap = (const uint32_t*)rd64((uint64_t)D.ap, E.r);
    const uint64_t* cp = (const uint64_t*)rd64((uint64_t)D.cp, E.r);
    if (E.has) {
      E.a = ap[E.k];
      E.c = cp[E.k];
    }
  }
  return E;
}

// Tier 1. Returns the union's length, ~0u for a non-canonical run (nothing written).
__device__ __forceinline__ uint32_t fold_regs(const Obj& D, const Ent& E, uint32_t R, WaveLds& L, const FoldOut& W,
                                              uint64_t ob, uint32_t lane) {
  const uint32_t e32 = (uint32_t)D.e, a = E.a;
  const uint32_t below = from_below(a);
  const bool bad = E.has && (E.c == 0ull || (E.k && below >= a));
  if (__ballot(bad)) return ~0u;
  uint32_t p = 0u;
  uint64_t cm = E.c;
  bool first = true;
  for (uint32_t q = 0; q < R; ++q) {  // (every lane runs the searches: ds_bpermute sources must be active lanes)
    const uint32_t nq = lane32(D.n, q);
    if (nq == 0u) continue;
    const uint32_t bq = lane32(e32, q) - nq;  // run q sits in lanes [bq, bq + nq)
    uint32_t b = 0u;
#pragma unroll
    for (uint32_t step = 32u; step; step >>= 1) {
      const uint32_t cnd = b + step;
      const uint32_t pr = rd32(a, (bq + cnd - 1u) & 63u);
      b = (cnd <= nq && pr < a) ? cnd : b;
    }
    {
      const uint32_t pr = rd32(a, (bq + b) & 63u);
      b = (b + 1u <= nq && pr < a) ? b + 1u : b;
    }
    const uint32_t at = (bq + b) & 63u;
    const uint32_t aq = rd32(a, at);
    const uint64_t cq = rd64(E.c, at);
    const bool eq = b < nq && aq == a;
    p += b;
    cm = eq && cq > cm ? cq : cm;
    first = first && !(eq && q < E.r);
  }
  if (lane == 0u) L.mask[0] = 0ull;
  sync();
  const bool own = E.has && first;
  if (own) lds_or(&L.mask[0], 1ull << (p & 63u));
  sync();
  const uint64_t M = L.mask[0];
  if (own) {  // VClock::witness: the largest counter (src/vclock.rs:159-163)
    const uint32_t d = (uint32_t)__popcll(M & low_bits(p & 63u));
    W.act[ob + d] = a;
    W.ctr[ob + d] = cm;
  }
  return (uint32_t)__popcll(M);
}

// Tier 2: 64 < T <= kStage.
__device__ __forceinline__ uint32_t fold_lds(const Obj& D, uint32_t R, WaveLds& L, const FoldOut& W, uint64_t ob,
                                             uint32_t lane) {
  const uint32_t T = (uint32_t)D.T, e32 = (uint32_t)D.e;
  bool bad = false;
  for (uint32_t r = 0; r < R; ++r) {  // stage the runs end to end, checking them
    const uint32_t nr = lane32(D.n, r), br = lane32(e32, r) - nr;
    const uint32_t* ap = lane_ptr(D.ap, r);
    const uint64_t* cp = lane_ptr(D.cp, r);
    for (uint32_t k = lane; k < nr; k += kW) {
      const uint32_t a = ap[k];
      const uint64_t c = cp[k];
      bad = bad || c == 0ull || (k && ap[k - 1u] >= a);
      L.act[br + k] = a;
      L.ctr[br + k] = c;
    }
  }
  if (lane < kWords) L.mask[lane] = 0ull;
  sync();
  if (__ballot(bad)) return ~0u;
  for (uint32_t j0 = 0; j0 < T; j0 += kW) {
    const uint32_t j = j0 + lane;
    const bool has = j < T;
    const uint32_t myr = rank_regs(e32, kW, (has ? j : 0u) + 1u) & 63u;
    const uint32_t k = j - rd32(e32 - D.n, myr);
    uint32_t a = 0u, p = 0u;
    uint64_t cm = 1ull;
    bool first = true;
    if (has) {
      a = L.act[j];
      cm = L.ctr[j];
    }
    for (uint32_t q = 0; q < R; ++q) {
      const uint32_t nq = lane32(D.n, q);
      if (nq == 0u) continue;
      const uint32_t bq = lane32(e32, q) - nq;
      if (has) {
        uint32_t b = k;  // its own index in its own run
        bool eq = true;
        if (q != myr) {
          b = (uint32_t)rank_mem(L.act + bq, nq, a);
          eq = b < nq && L.act[bq + b] == a;
        }
        p += b;
        if (eq) {  // (a holder's counter may already be the maxed one: the same maximum)
          const uint64_t cq = L.ctr[bq + b];
          cm = cq > cm ? cq : cm;
          first = first && q >= myr;
        }
      }
    }
    if (has && first) {
      L.ctr[j] = cm;
      L.src[p] = (uint16_t)j;
      lds_or(&L.mask[p >> 6], 1ull << (p & 63u));
    }
  }
  sync();
  const uint32_t words = (T + kW - 1u) / kW;
  const uint32_t cnt = lane < words ? (uint32_t)__popcll(L.mask[lane]) : 0u;
  const uint32_t inc = scan_incl(cnt, lane);
  if (lane < words) L.pref[lane] = inc - cnt;
  sync();
  for (uint32_t p0 = 0; p0 < T; p0 += kW) {  // the union front to back
    const uint64_t M = L.mask[p0 >> 6];
    if ((M >> lane) & 1ull) {
      const uint32_t d = L.pref[p0 >> 6] + (uint32_t)__popcll(M & low_bits(lane));
      const uint32_t j = L.src[p0 + lane];
      W.act[ob + d] = L.act[j];
      W.ctr[ob + d] = L.ctr[j];
    }
  }
  return lane32(inc, kW - 1u);
}

// Tier 3: T > kStage. The object's output region [ob, ob + T) is the scratch.
__device__ __forceinline__ uint32_t fold_mem(const Obj& D, uint32_t R, const FoldOut& W, uint64_t ob, uint32_t lane) {
  const uint64_t T = D.T;
  bool bad = false;
  for (uint32_t r = 0; r < R; ++r) {  // canonical form first: a rank of an unsorted run may leave the region
    const uint32_t nr = lane32(D.n, r);
    const uint32_t* ap = lane_ptr(D.ap, r);
    const uint64_t* cp = lane_ptr(D.cp, r);
    for (uint32_t k0 = 0; k0 < nr; k0 += kW) {
      const uint32_t k = k0 + lane;
      if (k < nr) bad = bad || cp[k] == 0ull || (k && ap[k - 1u] >= ap[k]);
    }
  }
  if (__ballot(bad)) return ~0u;
  for (uint64_t x = lane; x < T; x += kW) W.ctr[ob + x] = 0ull;
  sync<true>();
  for (uint32_t r = 0; r < R; ++r) {
    const uint32_t nr = lane32(D.n, r);
    const uint32_t* ap = lane_ptr(D.ap, r);
    const uint64_t* cp = lane_ptr(D.cp, r);
    for (uint32_t k0 = 0; k0 < nr; k0 += kW) {
      const uint32_t k = k0 + lane;
      const bool has = k < nr;
      const uint32_t a = has ? ap[k] : 0u;
      uint64_t cm = has ? cp[k] : 1ull, p = k;
      bool first = true;
      for (uint32_t q = 0; q < R; ++q) {
        const uint32_t nq = lane32(D.n, q);
        if (nq == 0u || q == r) continue;
        const uint32_t* aq = lane_ptr(D.ap, q);
        const uint64_t* cq = lane_ptr(D.cp, q);
        if (has) {
          const uint64_t b = rank_mem(aq, nq, a);
          p += b;
          if (b < nq && aq[b] == a) {
            const uint64_t v = cq[b];
            cm = v > cm ? v : cm;
            first = first && q > r;
          }
        }
      }
      if (has && first) {  // p < T: the runs are canonical
        W.act[ob + p] = a;
        W.ctr[ob + p] = cm;
      }
    }
  }
  sync<true>();
  uint64_t count = 0;
  for (uint64_t x0 = 0; x0 < T; x0 += kW) {  // compact: cell x goes to a cell at or before x
    const uint64_t x = x0 + lane;
    const bool has = x < T;
    const uint32_t a = has ? W.act[ob + x] : 0u;
    const uint64_t c = has ? W.ctr[ob + x] : 0ull;
    const uint64_t m = __ballot(has && c != 0ull);
    sync<true>();  // the chunk is read before any of its cells is written
    if (has && c != 0ull) {
      const uint64_t d = count + mbcnt(m);
      W.act[ob + d] = a;
      W.ctr[ob + d] = c;
    }
    count += (uint64_t)__popcll(m);
  }
  return (uint32_t)count;  // (a union holds each u32 actor once at the most; 2^32 of them is past any batch)
}

// One chunk of 64 objects (lane k <-> object c0 + k).
__device__ __forceinline__ void fold_chunk(const FoldReps& P, uint32_t R, const FoldOut& W, uint64_t n_obj,
                                           const uint64_t* offp, const uint32_t* lenp, const uint32_t* actp,
                                           const uint64_t* ctrp, uint64_t c0, uint32_t lane, WaveLds& L,
                                           int* status) {
  const uint64_t i = c0 + lane;
  const bool valid = i < n_obj, has_next = i + 1u < n_obj;
  // placement per replica, as crdt_vclock_csr_merge checks its two sides; the
  // region [sum of offsets, + sum of lengths) must fit the output
  bool inb = true, placed = true;
  uint64_t so = 0, sl = 0;
  for (uint32_t r = 0; r < R; ++r) {
    const uint64_t* op = P.off[r];
    const uint32_t* lp = P.len[r];
    const uint64_t ent = P.entries[r];
    uint64_t o = 0;
    uint32_t l = 0;
    if (valid) {
      o = op[i];
      l = lp[i];
    }
    uint64_t no = rd64(o, (lane + 1u) & 63u);
    if (lane == kW - 1u && has_next) no = op[i + 1u];
    inb = inb && o <= ent && o + l <= ent;
    placed = placed && (!has_next || no >= o + l);
    so += o;
    sl += l;
  }
  inb = inb && so + sl <= W.entries && so <= W.entries;
  if (__ballot(valid && !placed) && lane == 0u) fail(status, CRDT_EINVAL);
  if (__ballot(valid && !inb) && lane == 0u) fail(status, CRDT_EINVAL);
  const bool ok = valid && placed && inb;
  uint32_t myU = 0u;

  // ---- the chunk's objects one by one: the next one's runs (tier 1) and the
  // offsets and lengths of the one after it are in flight
  uint64_t pend = __ballot(ok);
  const bool rep = lane < R;
  Obj D{};
  Ent E{};
  uint64_t ro = 0;
  uint32_t rn = 0;
  if (pend) {
    const uint64_t i0 = c0 + (uint32_t)__builtin_ctzll(pend);
    if (rep) {
      ro = offp[i0];
      rn = lenp[i0];
    }
    D = make_obj(ro, rn, actp, ctrp, lane);
    E = fetch_ent(D, lane);
    ro = 0;
    rn = 0;
    const uint64_t rest = pend & (pend - 1u);
    if (rest && rep) {
      const uint64_t i1 = c0 + (uint32_t)__builtin_ctzll(rest);
      ro = offp[i1];
      rn = lenp[i1];
    }
  }
  while (pend) {
    const uint32_t t = (uint32_t)__builtin_ctzll(pend);
    pend &= pend - 1u;
    const Obj Dc = D;
    const Ent Ec = E;
    if (pend) {
      D = make_obj(ro, rn, actp, ctrp, lane);
      E = fetch_ent(D, lane);
      ro = 0;
      rn = 0;
      const uint64_t rest = pend & (pend - 1u);
      if (rest && rep) {
        const uint64_t i2 = c0 + (uint32_t)__builtin_ctzll(rest);
        ro = offp[i2];
        rn = lenp[i2];
      }
    }
    const uint64_t ob = lane64(so, t);
    uint32_t U;
    sync();  // the previous object's readers of the LDS region are done
    if (Dc.T <= kW)
      U = fold_regs(Dc, Ec, R, L, W, ob, lane);
    else if (Dc.T <= kStage)
      U = fold_lds(Dc, R, L, W, ob, lane);
    else
      U = fold_mem(Dc, R, W, ob, lane);
    if (U == ~0u) {
      U = 0u;
      if (lane == 0u) fail(status, CRDT_ENONCANON);
    }
    myU = lane == t ? U : myU;
  }
  if (valid) {
    W.off[i] = so;
    W.len[i] = ok ? myU : 0u;
  }
}

__global__ __launch_bounds__(kBlock) void clock_csr_fold_kernel(FoldReps P, uint32_t R, FoldOut W, uint64_t n_obj,
                                                                uint64_t chunks, int* status) {
  __shared__ WaveLds lds[kWaves];
  const uint32_t lane = threadIdx.x & (kW - 1u), w = threadIdx.x / kW;
  const uint64_t wave = (uint64_t)blockIdx.x * kWaves + w;
  const uint64_t n_waves = (uint64_t)gridDim.x * kWaves;
  // lane r <-> replica r
  const uint32_t rr = lane < R ? lane : 0u;
  const uint64_t* offp = P.off[rr];
  const uint32_t* lenp = P.len[rr];
  const uint32_t* actp = P.act[rr];
  const uint64_t* ctrp = P.ctr[rr];
  for (uint64_t ch = wave; ch < chunks; ch += n_waves)
    fold_chunk(P, R, W, n_obj, offp, lenp, actp, ctrp, ch * kW, lane, lds[w], status);
}

}  // namespace

int launch_clock_dense_fold(const uint64_t* const* rows, uint32_t n_reps, uint64_t* out, uint64_t n_words,
                            hipStream_t stream) {
  if (n_words == 0) return CRDT_OK;
  assert(n_reps >= 1u && n_reps <= kMaxReps);  // the limits are api.hip's to reject
  DenseRows P{};
  bool aligned = (uintptr_t)out % 16 == 0;
  for (uint32_t r = 0; r < kMaxReps; ++r) {
    P.p[r] = rows[r < n_reps ? r : 0u];
    aligned = aligned && (uintptr_t)P.p[r] % 16 == 0;
  }
  const uint64_t tile = (uint64_t)kThreads * kUnroll;
  const uint64_t n2 = aligned ? n_words / 2 : 0;
  if (n2) {
    hipLaunchKernelGGL(clock_dense_fold_kernel<u64x2>, dim3(resident_blocks((n2 + tile - 1) / tile)), dim3(kThreads), 0,
                       stream, P, n_reps, (u64x2*)out, n2);
  }
  const uint64_t done = 2 * n2, rest = n_words - done;
  if (rest) {
    for (uint32_t r = 0; r < kMaxReps; ++r) P.p[r] += done;
    hipLaunchKernelGGL(clock_dense_fold_kernel<uint64_t>, dim3(resident_blocks((rest + tile - 1) / tile)),
                       dim3(kThreads), 0, stream, P, n_reps, out + done, rest);
  }
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_clock_csr_fold(const crdt_clock_csr* reps, uint32_t n_reps, const crdt_clock_csr_out& out, int* status,
                          hipStream_t stream) {
  const uint64_t n_obj = reps[0].n_obj;
  if (n_obj == 0) return CRDT_OK;
  assert(n_reps >= 1u && n_reps <= kMaxReps);
  FoldReps P{};
  for (uint32_t r = 0; r < kMaxReps; ++r) {  // (past n_reps: never dereferenced)
    const crdt_clock_csr& s = reps[r < n_reps ? r : 0u];
    P.off[r] = s.off;
    P.len[r] = s.len;
    P.act[r] = s.act;
    P.ctr[r] = s.ctr;
    P.entries[r] = s.n_entries;
  }
  const FoldOut W{out.off, out.len, out.act, out.ctr, out.n_entries};
  const uint64_t chunks = (n_obj + kW - 1) / kW;
  // 4 blocks of 4 waves per CU: what the kernel's registers allow (its LDS would allow 5)
  const uint32_t blocks = resident_blocks((chunks + kWaves - 1) / kWaves, 4u);
  hipLaunchKernelGGL(clock_csr_fold_kernel, dim3(blocks), dim3(kBlock), 0, stream, P, n_reps, W, n_obj, chunks,
                     status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
