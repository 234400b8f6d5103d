// The op path of VClock / GCounter / PNCounter, batched (include/crdts_hip.h
// "Batched op path of the clocks and counters"): CmRDT::apply, Causal::truncate,
// subtract, intersection and the reads, on dense rows and on CSR runs.
//
// Reference: VClock::apply == witness (src/vclock.rs:126-128, 159-163: keep
// the larger counter, never store 0), get (:206-210), Causal::truncate
// (:103-120: the smaller counter, an actor absent on either side goes),
// intersection (:219-228: equal counters stay), subtract (:236-242: an actor
// whose counter `other` reaches goes); GCounter::apply / value
// (src/gcounter.rs:53-55, 76-78); PNCounter::apply / value
// (src/pncounter.rs:82-87, 117-119).
//
// Dense rows (u64[n_obj][slots], 0 = absent):
//   binops  flat over n_obj * slots words in the shape of dense_max_kernel:
//           16-B loads, 4 pairs in flight per lane, grid-stride, 24 B per slot.
//   apply   a wave takes 64 objects (lane k <-> object c + k: the op ranges in
//           one coalesced step), then its lanes take the chunk's ops flat —
//           an op finds its object by a 6-step search over the 64 range ends
//           held in registers — and witness with a 64-bit atomic max to HBM,
//           so a repeated actor keeps its largest counter in any order.
//           12 B (16 B: PNCounter) read per op + one 8-B atomic.
//   get     the same walk; a read instead of the atomic.
//   value   a row reduction: 64 / G rows per wave, G = the power of two >=
//           the row's words (<= 64) lanes per row, a DPP / bpermute butterfly over
//           the G lanes; rows wider than 64 words are strided by a wave. A
//           word is 16 bytes for an even n_actors on an aligned base, else 8.
//           8 B per slot read, 8 B per object written.
// CSR runs (crdt_clock_csr; one wave per object, chunks of 64 objects like
// csr_merge.hip, the same placement and canonical-form checks):
//   filters each self entry finds other's counter by rank (registers for runs
//           <= 64, binary search in HBM past that) and the kept entries are
//           compacted with ballot + mbcnt; out.off = self.off.
//   apply   the object's dots become a canonical run (sorted by actor, the
//           largest counter per actor, no zero) — in registers for <= 64
//           dots, through the context's HBM scratch past that — which is
//           then joined with self's run exactly as the CSR merge does.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "csr_rank.h"
#include "kernels.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace csr_rank;

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kBlock = 256;
constexpr int kUnroll = 4;


// ---------------------------------------------------------------- dense binops
template <int OP>
__device__ __forceinline__ uint64_t binop(uint64_t s, uint64_t o) {
  if (OP == kClockTruncate) return s < o ? s : o;  // src/vclock.rs:103-120
  if (OP == kClockSubtract) return o >= s ? 0ull : s;  // :236-242
  return s == o ? s : 0ull;  // :219-228
}

template <int OP>
__global__ __launch_bounds__(kBlock) void dense_binop_kernel(u64x2* __restrict__ s, const u64x2* __restrict__ o,
                                                             uint64_t n2) {
  const uint64_t tile = (uint64_t)kBlock * kUnroll;
  for (uint64_t base = (uint64_t)blockIdx.x * tile; base < n2; base += (uint64_t)gridDim.x * tile) {
    u64x2 a[kUnroll], b[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t k = base + (uint64_t)u * kBlock + threadIdx.x;
      if (k < n2) {
        a[u] = __builtin_nontemporal_load(s + k);
        b[u] = __builtin_nontemporal_load(o + k);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint64_t k = base + (uint64_t)u * kBlock + threadIdx.x;
      if (k < n2) {
        u64x2 r;
        r.x = binop<OP>(a[u].x, b[u].x);
        r.y = binop<OP>(a[u].y, b[u].y);
        __builtin_nontemporal_store(r, s + k);
      }
    }
  }
}

template <int OP>
__global__ void dense_binop_tail(uint64_t* s, const uint64_t* o, uint64_t n) {
  const uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (k < n) s[k] = binop<OP>(s[k], o[k]);
}

template <int OP>
int dense_binop(uint64_t* self, const uint64_t* other, uint64_t n_words, hipStream_t stream) {
  const bool aligned = ((uintptr_t)self % 16 == 0) && ((uintptr_t)other % 16 == 0);
  const uint64_t n2 = aligned ? n_words / 2 : 0;
  if (n2) {
    const uint64_t tile = (uint64_t)kBlock * kUnroll;
    hipLaunchKernelGGL(dense_binop_kernel<OP>, dim3(resident_blocks((n2 + tile - 1) / tile)), dim3(kBlock), 0, stream,
                       (u64x2*)self, (const u64x2*)other, n2);
  }
  const uint64_t done = 2 * n2, rest = n_words - done;  // unaligned rows, or the odd last word
  if (rest)
    hipLaunchKernelGGL(dense_binop_tail<OP>, dim3((uint32_t)((rest + 255) / 256)), dim3(256), 0, stream, self + done,
                       other + done, rest);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

// ------------------------------------------------- the ops of 64 objects, flat
// Calls f(j, has, t) for every op j of objects [c0, c0 + 64): `has` says the
// lane holds op j, t is the lane that stands for j's object (object c0 + t).
// Every lane makes every call (f may read across lanes). Ranges that decrease
// or run past n_ops latch CRDT_ENONCANON and their objects' ops are skipped.
template <class F>
__device__ __forceinline__ void for_each_op(const uint64_t* obj_end, uint64_t n_obj, uint64_t n_ops, uint64_t c0,
                                            uint32_t lane, int* status, F f) {
  const uint64_t i = c0 + lane;
  const bool valid = i < n_obj;
  uint64_t b = 0, e = 0;
  if (valid) {
    e = obj_end[i];
    b = i ? obj_end[i - 1u] : 0ull;
  }
  const bool good = b <= e && e <= n_ops;
  if (__ballot(valid && !good) && lane == 0u) fail(status, CRDT_ENONCANON);
  for_each_in_ranges(valid, good, b, e, lane, f);  // csr_rank.h
}

// MODE 0: VClock / GCounter apply; 1: PNCounter apply ([P|N] rows); 2: get
template <int MODE>
__global__ __launch_bounds__(kBlock) void dense_ops_kernel(uint64_t* rows, crdt_clock_ops P, uint64_t* out,
                                                           uint64_t n_obj, uint32_t A, uint64_t chunks, int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const uint64_t slots = MODE == 1 ? 2ull * A : A;
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t c0 = ch * kW;
    bool bad = false;
    for_each_op(P.obj_end, n_obj, P.n_ops, c0, lane, status, [&](uint64_t j, bool has, uint32_t t) {
      if (!has) return;
      const uint32_t a = P.actor[j];
      uint64_t* row = rows + (c0 + t) * slots;
      if (MODE == 2) {  // VClock::get: an absent actor is 0
        out[j] = a < A ? row[a] : 0ull;
        return;
      }
      const uint64_t c = P.counter[j];
      const uint32_t d = MODE == 1 ? P.dir[j] : 0u;
      if (a >= A || d > 1u) {
        bad = true;  // skipped; the object's other ops still apply
      } else if (c) {  // witness: the larger counter; a 0 is never stored
        atomicMax((unsigned long long*)(row + (uint64_t)d * A + a), (unsigned long long)c);
      }
    });
    if (__ballot(bad) && lane == 0u) fail(status, CRDT_ENONCANON);
  }
}

// ---------------------------------------------------------------- dense values
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, false);
  return ((uint64_t)hi << 32) | lo;
}

// every lane of an aligned group of G lanes gets the group's wrapping sum
// (all 64 lanes active)
template <int G>
__device__ __forceinline__ uint64_t group_sum(uint64_t v, uint32_t lane) {
  if (G >= 2) v += dpp64<0xB1>(v);    // quad_perm [1,0,3,2]
  if (G >= 4) v += dpp64<0x4E>(v);    // quad_perm [2,3,0,1]
  if (G >= 8) v += dpp64<0x141>(v);   // row_half_mirror
  if (G >= 16) v += dpp64<0x140>(v);  // row_mirror
  if (G >= 32) v += rd64(v, lane ^ 16u);
  if (G >= 64) v += rd64(v, lane ^ 32u);
  return v;
}

// T = uint64_t: 8-byte loads, any row; T = u64x2: 16-byte loads for rows of an
// even number of slots on a 16-byte aligned base (W = words of T per clock)
__device__ __forceinline__ uint64_t word_sum(uint64_t v) { return v; }
__device__ __forceinline__ uint64_t word_sum(u64x2 v) { return v.x + v.y; }

template <int G, bool PN, class T>
__global__ __launch_bounds__(kBlock) void value_kernel(const T* __restrict__ rows, uint64_t* __restrict__ out,
                                                       uint64_t n_obj, uint32_t W) {
  constexpr uint32_t kRows = kW / G;  // rows per wave
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const uint32_t g = lane / G, t = lane % G;
  const uint64_t slots = PN ? 2ull * W : W;
  for (uint64_t w = wave; w * kRows < n_obj; w += n_waves) {
    const uint64_t i = w * kRows + g;
    const bool valid = i < n_obj;
    uint64_t p = 0, q = 0;
    if (valid) {
      const T* row = rows + i * slots;
#pragma unroll 4
      for (uint32_t k = t; k < W; k += G) {
        p += word_sum(row[k]);
        if (PN) q += word_sum(row[(uint64_t)W + k]);
      }
    }
    p = group_sum<G>(p, lane);
    if (PN) q = group_sum<G>(q, lane);
    // PNCounter::value: p as i64 - n as i64 (src/pncounter.rs:117-119), wrapping
    if (valid && t == 0u) out[i] = PN ? p - q : p;
  }
}

template <bool PN, class T>
int launch_value_as(const T* rows, uint64_t* out, uint64_t n_obj, uint32_t W, hipStream_t stream) {
  uint32_t G = 1;
  while (G < W && G < kW) G <<= 1;
  const uint64_t waves = (n_obj + kW / G - 1) / (kW / G);
  const dim3 grid(resident_blocks((waves + kBlock / kW - 1) / (kBlock / kW))), block(kBlock);
  switch (G) {
    case 1: hipLaunchKernelGGL((value_kernel<1, PN, T>), grid, block, 0, stream, rows, out, n_obj, W); break;
    case 2: hipLaunchKernelGGL((value_kernel<2, PN, T>), grid, block, 0, stream, rows, out, n_obj, W); break;
    case 4: hipLaunchKernelGGL((value_kernel<4, PN, T>), grid, block, 0, stream, rows, out, n_obj, W); break;
    case 8: hipLaunchKernelGGL((value_kernel<8, PN, T>), grid, block, 0, stream, rows, out, n_obj, W); break;
    case 16: hipLaunchKernelGGL((value_kernel<16, PN, T>), grid, block, 0, stream, rows, out, n_obj, W); break;
    case 32: hipLaunchKernelGGL((value_kernel<32, PN, T>), grid, block, 0, stream, rows, out, n_obj, W); break;
    default: hipLaunchKernelGGL((value_kernel<64, PN, T>), grid, block, 0, stream, rows, out, n_obj, W); break;
  }
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

template <bool PN>
int launch_value(const uint64_t* rows, uint64_t* out, uint64_t n_obj, uint32_t A, hipStream_t stream) {
  // every clock (a PNCounter's P and N halves too) starts 16-byte aligned
  if (A % 2u == 0u && (uintptr_t)rows % 16 == 0)
    return launch_value_as<PN>((const u64x2*)rows, out, n_obj, A / 2u, stream);
  return launch_value_as<PN>(rows, out, n_obj, A, stream);
}

// ------------------------------------------------------------------ CSR shared
struct CsrIn {
  const uint64_t* off;
  const uint32_t* len;
  const uint32_t* act;
  const uint64_t* ctr;
  uint64_t n_entries;
};
struct CsrOut {
  uint64_t* off;
  uint32_t* len;
  uint32_t* act;
  uint64_t* ctr;
  uint64_t n_entries;
};
CsrIn in_of(const crdt_clock_csr& c) { return CsrIn{c.off, c.len, c.act, c.ctr, c.n_entries}; }
CsrOut out_of(const crdt_clock_csr_out& c) { return CsrOut{c.off, c.len, c.act, c.ctr, c.n_entries}; }

// lane k <-> object c0 + k of one side: offset, length, and whether the run
// lies inside [0, n_entries) before the next object's run (the merge's
// placement precondition)
__device__ __forceinline__ bool load_run(const CsrIn& S, uint64_t n, uint64_t i, uint64_t& so, uint32_t& sl,
                                         bool& placed) {
  so = 0;
  sl = 0;
  placed = true;
  if (i >= n) return false;
  so = S.off[i];
  sl = S.len[i];
  if (i + 1u < n) placed = S.off[i + 1u] >= so + sl;
  return so <= S.n_entries && sl <= S.n_entries - so;
}

// a run of HBM is canonical: actors strictly increasing, counters > 0
__device__ __forceinline__ bool run_bad(const uint32_t* a, const uint64_t* c, uint32_t n, uint32_t lane) {
  bool bad = false;
  for (uint32_t base = 0; base < n; base += kW) {
    const uint32_t k = base + lane;
    if (k < n) bad = bad || c[k] == 0ull || (k && a[k - 1u] >= a[k]);
  }
  return __ballot(bad) != 0ull;
}

// ----------------------------------------------------------------- CSR filters
template <int OP>
__device__ __forceinline__ bool keep_entry(bool present, uint64_t c, uint64_t d, uint64_t& v) {
  v = c;
  if (OP == kClockTruncate) {  // both sides hold the actor: the smaller counter
    v = d < c ? d : c;
    return present;
  }
  if (OP == kClockSubtract) return !(present && d >= c);  // absent in other: 0 >= c never holds (c > 0)
  return present && d == c;
}

// self's run filtered by other's, written at ob; the kept length or ~0u for a
// non-canonical run
template <int OP>
__device__ __forceinline__ uint32_t filter_one(const CsrIn& S, const CsrIn& O, const CsrOut& R, uint64_t s0,
                                               uint32_t ns, uint64_t o0, uint32_t no, uint64_t ob, uint32_t lane) {
  if (ns <= kW && no <= kW) {
    const bool hs = lane < ns, ho = lane < no;
    uint32_t a = 0u, b = 0u;
    uint64_t c = 1ull, d = 1ull;
    if (hs) { a = S.act[s0 + lane]; c = S.ctr[s0 + lane]; }
    if (ho) { b = O.act[o0 + lane]; d = O.ctr[o0 + lane]; }
    const uint32_t ap = from_below(a), bp = from_below(b);
    const bool bad = (hs && (c == 0ull || (lane && ap >= a))) || (ho && (d == 0ull || (lane && bp >= b)));
    // (every lane runs the search: ds_bpermute sources must be active lanes)
    const uint32_t r0 = rank_regs(b, no, a);
    const uint32_t rs = hs ? r0 : 0u;  // # other actors below my actor
    const uint32_t bs = rd32(b, rs & 63u);
    const uint64_t dv = rd64(d, rs & 63u);
    if (__ballot(bad)) return ~0u;
    uint64_t v;
    const bool keep = keep_entry<OP>(hs && rs < no && bs == a, c, dv, v) && hs;
    const uint64_t K = __ballot(keep);
    if (keep) {
      const uint32_t pos = mbcnt(K);
      R.act[ob + pos] = a;
      R.ctr[ob + pos] = v;
    }
    return (uint32_t)__popcll(K);
  }
  const uint32_t* sa = S.act + s0;
  const uint64_t* sc = S.ctr + s0;
  const uint32_t* oa = O.act + o0;
  const uint64_t* oc = O.ctr + o0;
  if (run_bad(sa, sc, ns, lane) || run_bad(oa, oc, no, lane)) return ~0u;
  uint32_t kept = 0;
  for (uint32_t base = 0; base < ns; base += kW) {  // 64 self entries at a time, ranks by binary search in HBM
    const uint32_t k = base + lane;
    const bool h = k < ns;
    const uint32_t a = h ? sa[k] : 0u;
    const uint64_t c = h ? sc[k] : 1ull;
    const uint64_t r = h ? rank_mem(oa, no, a) : 0ull;
    const bool present = h && r < no && oa[r] == a;
    const uint64_t d = present ? oc[r] : 0ull;
    uint64_t v;
    const bool keep = keep_entry<OP>(present, c, d, v) && h;
    const uint64_t K = __ballot(keep);
    if (keep) {
      const uint32_t pos = kept + mbcnt(K);
      R.act[ob + pos] = a;
      R.ctr[ob + pos] = v;
    }
    kept += (uint32_t)__popcll(K);
  }
  return kept;
}

template <int OP>
__global__ __launch_bounds__(kBlock) void csr_filter_kernel(CsrIn S, CsrIn O, CsrOut R, uint64_t n, uint64_t chunks,
                                                            int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    const bool valid = i < n;
    uint64_t so, oo;
    uint32_t sl, ol;
    bool sp, op;
    const bool sin = load_run(S, n, i, so, sl, sp), oin = load_run(O, n, i, oo, ol, op);
    const bool inb = sin && oin && so + sl <= R.n_entries;
    const bool placed = sp && op;
    if (__ballot(valid && !(placed && inb)) && lane == 0u) fail(status, CRDT_EINVAL);
    const bool ok = valid && placed && inb;
    uint32_t myU = 0u;
    uint64_t pend = __ballot(ok);
    bool noncanon = false;
    while (pend) {  // the chunk's objects one by one, the whole wave on each
      const uint32_t t = (uint32_t)__builtin_ctzll(pend);
      pend &= pend - 1u;
      const uint64_t s0 = lane64(so, t);
      uint32_t U = filter_one<OP>(S, O, R, s0, lane32(sl, t), lane64(oo, t), lane32(ol, t), s0, lane);
      if (U == ~0u) {
        U = 0u;
        noncanon = true;
      }
      myU = lane == t ? U : myU;
    }
    if (noncanon && lane == 0u) fail(status, CRDT_ENONCANON);
    if (valid) {
      R.off[i] = so;
      R.len[i] = ok ? myU : 0u;
    }
  }
}

// ------------------------------------------------------------------- CSR apply
// The sorted union of two canonical runs in HBM, counters max'ed, written at
// (ua, uc): each entry's rank in the other run by binary search (the long form
// of the CSR merge). Returns the union's length.
__device__ uint32_t union_long(const uint32_t* sa, const uint64_t* sc, uint32_t ns, const uint32_t* oa,
                               const uint64_t* oc, uint32_t no, uint32_t* ua, uint64_t* uc, uint32_t lane) {
  uint32_t eq_before = 0;
  for (uint32_t base = 0; base < ns; base += kW) {  // self entries: every one is written
    const uint32_t k = base + lane;
    const bool h = k < ns;
    const uint32_t a = h ? sa[k] : 0u;
    const uint64_t c = h ? sc[k] : 1ull;
    const uint64_t r = h ? rank_mem(oa, no, a) : 0ull;
    const bool eq = h && r < no && oa[r] == a;
    const uint64_t E = __ballot(eq);
    const uint64_t v = eq ? (oc[r] > c ? oc[r] : c) : c;
    const uint64_t pos = k + r - (eq_before + mbcnt(E));
    eq_before += (uint32_t)__popcll(E);
    if (h) {
      ua[pos] = a;
      uc[pos] = v;
    }
  }
  uint32_t eqo_before = 0;
  for (uint32_t base = 0; base < no; base += kW) {  // other entries not met by a self entry
    const uint32_t k = base + lane;
    const bool h = k < no;
    const uint32_t a = h ? oa[k] : 0u;
    const uint64_t c = h ? oc[k] : 1ull;
    const uint64_t r = h ? rank_mem(sa, ns, a) : 0ull;
    const bool eq = h && r < ns && sa[r] == a;
    const uint64_t E = __ballot(eq);
    const uint64_t pos = k + r - (eqo_before + mbcnt(E));
    eqo_before += (uint32_t)__popcll(E);
    if (h && !eq) {
      ua[pos] = a;
      uc[pos] = c;
    }
  }
  return ns + no - eq_before;
}

struct ApplyJob {
  CsrIn S;
  CsrOut R;
  const uint64_t* obj_end;
  const uint32_t* actor;
  const uint64_t* counter;
  uint64_t n_ops, n;
  // HBM scratch of the long paths, n_ops entries each (null with n_ops == 0:
  // never touched then)
  uint32_t* w_flag;
  uint32_t* w_act;
  uint64_t* w_ctr;
};

// More than 64 dots: the canonical run of ops [bb, bb + m) into the scratch at
// bb. A dot stands for its actor when it is alive (counter > 0) and no other
// alive dot of the actor has a larger counter, or the same one at a lower
// index; its place is the number of standing dots with a smaller actor.
__device__ uint32_t canon_long(const ApplyJob& J, uint64_t bb, uint32_t m, uint32_t lane) {
  const uint32_t* xa = J.actor + bb;
  const uint64_t* ya = J.counter + bb;
  uint32_t mo = 0;
  for (uint32_t base = 0; base < m; base += kW) {
    const uint32_t j = base + lane;
    const bool h = j < m;
    const uint32_t x = h ? xa[j] : 0u;
    const uint64_t y = h ? ya[j] : 0ull;
    bool rep = h && y > 0ull;
    for (uint32_t kb = 0; kb < m; kb += kW) {
      const uint32_t kl = kb + lane;
      const uint32_t xl = kl < m ? xa[kl] : 0u;
      const uint64_t yl = kl < m ? ya[kl] : 0ull;
      const uint32_t cnt = m - kb < kW ? m - kb : kW;
      for (uint32_t kk = 0; kk < cnt; ++kk) {
        const uint32_t xk = lane32(xl, kk);
        const uint64_t yk = lane64(yl, kk);
        if (yk && xk == x && (yk > y || (yk == y && kb + kk < j))) rep = false;
      }
    }
    if (h) J.w_flag[bb + j] = rep ? 1u : 0u;
    mo += (uint32_t)__popcll(__ballot(rep));
  }
  sync();
  for (uint32_t base = 0; base < m; base += kW) {
    const uint32_t j = base + lane;
    const bool h = j < m;
    const uint32_t x = h ? xa[j] : 0u;
    const uint64_t y = h ? ya[j] : 0ull;
    const bool rep = h && J.w_flag[bb + j] != 0u;
    uint32_t rnk = 0;
    for (uint32_t kb = 0; kb < m; kb += kW) {
      const uint32_t kl = kb + lane;
      const uint32_t xl = kl < m ? xa[kl] : 0u;
      uint64_t F = __ballot(kl < m && J.w_flag[bb + kl] != 0u);
      while (F) {
        const uint32_t kk = (uint32_t)__builtin_ctzll(F);
        F &= F - 1u;
        rnk += lane32(xl, kk) < x ? 1u : 0u;
      }
    }
    if (rep) {
      J.w_act[bb + rnk] = x;
      J.w_ctr[bb + rnk] = y;
    }
  }
  sync();
  return mo;
}

// self's run [s0, s0 + ns) after witnessing ops [bb, bb + m), written at ob;
// the length, or ~0u for a non-canonical self run
__device__ __forceinline__ uint32_t apply_one(const ApplyJob& J, uint64_t s0, uint32_t ns, uint64_t bb, uint64_t m64,
                                              uint64_t ob, uint32_t lane) {
  const uint32_t* sa = J.S.act + s0;
  const uint64_t* sc = J.S.ctr + s0;
  uint32_t* ua = J.R.act + ob;
  uint64_t* uc = J.R.ctr + ob;
  uint32_t mo;
  if (m64 <= kW) {
    // ---- the dots in registers: lane j <-> dot j
    const uint32_t m = (uint32_t)m64;
    const bool hq = lane < m;
    const uint32_t x = hq ? J.actor[bb + lane] : 0u;
    const uint64_t y = hq ? J.counter[bb + lane] : 0ull;
    bool rep = hq && y > 0ull;
    for (uint32_t k = 0; k < m; ++k) {
      const uint32_t xk = lane32(x, k);
      const uint64_t yk = lane64(y, k);
      if (yk && xk == x && (yk > y || (yk == y && k < lane))) rep = false;
    }
    const uint64_t Rm = __ballot(rep);
    mo = (uint32_t)__popcll(Rm);
    uint32_t rnk = 0;
    for (uint64_t F = Rm; F; F &= F - 1u) rnk += lane32(x, (uint32_t)__builtin_ctzll(F)) < x ? 1u : 0u;
    // lane p <- the standing dot of rank p (the others push to lane 63, which
    // is past the run whenever one of them exists)
    const int dst = (int)((rep ? rnk : 63u) << 2);
    const uint32_t b = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)x);
    const uint64_t d = ((uint64_t)(uint32_t)__builtin_amdgcn_ds_permute(dst, (int)(uint32_t)(y >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)(uint32_t)y);
    if (ns <= kW) {
      // ---- both runs in registers: the CSR merge's loop-free join
      const bool hs = lane < ns, ho = lane < mo;
      uint32_t a = 0u;
      uint64_t c = 1ull;
      if (hs) { a = sa[lane]; c = sc[lane]; }
      const uint32_t ap = from_below(a);
      const bool bad = hs && (c == 0ull || (lane && ap >= a));
      const uint32_t rs0 = rank_regs(b, mo, a), ro0 = rank_regs(a, ns, b);
      const uint32_t rs = hs ? rs0 : 0u, ro = ho ? ro0 : 0u;
      const uint32_t bs = rd32(b, rs & 63u), as = rd32(a, ro & 63u);
      const uint64_t dv = rd64(d, rs & 63u);
      if (__ballot(bad)) return ~0u;
      const bool eqs = hs && rs < mo && bs == a;
      const bool eqo = ho && ro < ns && as == b;
      const uint64_t ES = __ballot(eqs), EO = __ballot(eqo);
      const uint32_t ps = lane + rs - mbcnt(ES), po = lane + ro - mbcnt(EO);
      if (hs) {  // VClock::witness: the larger counter (src/vclock.rs:159-163)
        ua[ps] = a;
        uc[ps] = eqs && dv > c ? dv : c;
      }
      if (ho && !eqo) {
        ua[po] = b;
        uc[po] = d;
      }
      return ns + mo - (uint32_t)__popcll(ES);
    }
    if (lane < mo) {  // a long self run: the canonical dots go through the scratch
      J.w_act[bb + lane] = b;
      J.w_ctr[bb + lane] = d;
    }
    sync();
  } else {
    if (m64 > 0xfffffffeull - ns) return ~0u;  // (a u32 length cannot hold it)
    mo = canon_long(J, bb, (uint32_t)m64, lane);
  }
  if (run_bad(sa, sc, ns, lane)) return ~0u;
  return union_long(sa, sc, ns, J.w_act + bb, J.w_ctr + bb, mo, ua, uc, lane);
}

__global__ __launch_bounds__(kBlock) void csr_apply_kernel(ApplyJob J, uint64_t chunks, int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    const bool valid = i < J.n;
    uint64_t so, b = 0, e = 0;
    uint32_t sl;
    bool placed;
    const bool sin = load_run(J.S, J.n, i, so, sl, placed);
    if (valid) {
      e = J.obj_end[i];
      b = i ? J.obj_end[i - 1u] : 0ull;
    }
    const bool good = b <= e && e <= J.n_ops;
    const bool inb = sin && good && so + sl + e <= J.R.n_entries;
    if (__ballot(valid && !good) && lane == 0u) fail(status, CRDT_ENONCANON);
    if (__ballot(valid && good && !(placed && inb)) && lane == 0u) fail(status, CRDT_EINVAL);
    const bool ok = valid && placed && inb;
    uint32_t myU = 0u;
    uint64_t pend = __ballot(ok);
    bool noncanon = false;
    while (pend) {
      const uint32_t t = (uint32_t)__builtin_ctzll(pend);
      pend &= pend - 1u;
      const uint64_t s0 = lane64(so, t), bb = lane64(b, t), ee = lane64(e, t);
      uint32_t U = apply_one(J, s0, lane32(sl, t), bb, ee - bb, s0 + bb, lane);
      if (U == ~0u) {
        U = 0u;
        noncanon = true;
      }
      myU = lane == t ? U : myU;
    }
    if (noncanon && lane == 0u) fail(status, CRDT_ENONCANON);
    if (valid) {
      J.R.off[i] = so + (good ? b : 0ull);
      J.R.len[i] = ok ? myU : 0u;
    }
  }
}

// --------------------------------------------------------------- CSR value, get
__global__ __launch_bounds__(kBlock) void csr_value_kernel(CsrIn S, uint64_t* out, uint64_t n, uint64_t chunks,
                                                           int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    const bool valid = i < n;
    uint64_t so = 0;
    uint32_t sl = 0;
    if (valid) {
      so = S.off[i];
      sl = S.len[i];
    }
    const bool inb = so <= S.n_entries && sl <= S.n_entries - so;
    if (__ballot(valid && !inb) && lane == 0u) fail(status, CRDT_EINVAL);
    uint64_t mine = 0;
    uint64_t pend = __ballot(valid && inb && sl);
    while (pend) {
      const uint32_t t = (uint32_t)__builtin_ctzll(pend);
      pend &= pend - 1u;
      const uint64_t s0 = lane64(so, t);
      const uint32_t ns = lane32(sl, t);
      uint64_t v = 0;
      for (uint32_t k = lane; k < ns; k += kW) v += S.ctr[s0 + k];
      v = group_sum<64>(v, lane);
      mine = lane == t ? v : mine;
    }
    if (valid) out[i] = mine;
  }
}

__global__ __launch_bounds__(kBlock) void csr_get_kernel(CsrIn S, crdt_clock_ops P, uint64_t* out, uint64_t n,
                                                         uint64_t chunks, int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t c0 = ch * kW, i = c0 + lane;
    const bool valid = i < n;
    uint64_t so = 0;
    uint32_t sl = 0;
    if (valid) {
      so = S.off[i];
      sl = S.len[i];
    }
    const bool inb = so <= S.n_entries && sl <= S.n_entries - so;
    if (__ballot(valid && !inb) && lane == 0u) fail(status, CRDT_EINVAL);
    if (!inb) sl = 0u;  // reads as empty
    for_each_op(P.obj_end, n, P.n_ops, c0, lane, status, [&](uint64_t j, bool has, uint32_t t) {
      const uint64_t s0 = rd64(so, t);
      const uint32_t ns = rd32(sl, t);
      if (!has) return;
      const uint32_t x = P.actor[j];
      const uint64_t r = rank_mem(S.act + s0, ns, x);  // VClock::get: an absent actor is 0
      out[j] = (r < ns && S.act[s0 + r] == x) ? S.ctr[s0 + r] : 0ull;
    });
  }
}

uint32_t chunk_blocks(uint64_t chunks) { return resident_blocks((chunks + kBlock / kW - 1) / (kBlock / kW)); }

}  // namespace

int launch_dense_clock_binop(int op, uint64_t* self, const uint64_t* other, uint64_t n_words, hipStream_t stream) {
  if (n_words == 0) return CRDT_OK;
  switch (op) {
    case kClockTruncate: return dense_binop<kClockTruncate>(self, other, n_words, stream);
    case kClockSubtract: return dense_binop<kClockSubtract>(self, other, n_words, stream);
    default: return dense_binop<kClockIntersection>(self, other, n_words, stream);
  }
}

int launch_dense_clock_apply(uint64_t* rows, const crdt_clock_ops& ops, bool pn, uint64_t n_obj, uint32_t A,
                             int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const uint64_t chunks = (n_obj + kW - 1) / kW;
  if (pn)
    hipLaunchKernelGGL(dense_ops_kernel<1>, dim3(chunk_blocks(chunks)), dim3(kBlock), 0, stream, rows, ops,
                       (uint64_t*)nullptr, n_obj, A, chunks, status);
  else
    hipLaunchKernelGGL(dense_ops_kernel<0>, dim3(chunk_blocks(chunks)), dim3(kBlock), 0, stream, rows, ops,
                       (uint64_t*)nullptr, n_obj, A, chunks, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_dense_clock_get(const uint64_t* rows, const crdt_clock_ops& queries, uint64_t* out, uint64_t n_obj,
                           uint32_t A, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const uint64_t chunks = (n_obj + kW - 1) / kW;
  hipLaunchKernelGGL(dense_ops_kernel<2>, dim3(chunk_blocks(chunks)), dim3(kBlock), 0, stream, (uint64_t*)rows,
                     queries, out, n_obj, A, chunks, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_dense_clock_value(const uint64_t* rows, uint64_t* out, bool pn, uint64_t n_obj, uint32_t A,
                             hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  return pn ? launch_value<true>(rows, out, n_obj, A, stream) : launch_value<false>(rows, out, n_obj, A, stream);
}

int launch_clock_csr_filter(int op, const crdt_clock_csr& self, const crdt_clock_csr& other,
                            const crdt_clock_csr_out& out, int* status, hipStream_t stream) {
  const uint64_t n = self.n_obj, chunks = (n + kW - 1) / kW;
  if (chunks == 0) return CRDT_OK;
  const dim3 grid(chunk_blocks(chunks)), block(kBlock);
  const CsrIn S = in_of(self), O = in_of(other);
  const CsrOut R = out_of(out);
  switch (op) {
    case kClockTruncate:
      hipLaunchKernelGGL(csr_filter_kernel<kClockTruncate>, grid, block, 0, stream, S, O, R, n, chunks, status);
      break;
    case kClockSubtract:
      hipLaunchKernelGGL(csr_filter_kernel<kClockSubtract>, grid, block, 0, stream, S, O, R, n, chunks, status);
      break;
    default:
      hipLaunchKernelGGL(csr_filter_kernel<kClockIntersection>, grid, block, 0, stream, S, O, R, n, chunks, status);
      break;
  }
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

size_t clock_csr_apply_scratch_bytes(const crdt_clock_ops& ops) { return 16 * ops.n_ops; }

int launch_clock_csr_apply(const crdt_clock_csr& self, const crdt_clock_ops& ops, const crdt_clock_csr_out& out,
                           uint8_t* scratch, int* status, hipStream_t stream) {
  const uint64_t n = self.n_obj, chunks = (n + kW - 1) / kW;
  if (chunks == 0) return CRDT_OK;
  ApplyJob J{in_of(self), out_of(out), ops.obj_end, ops.actor, ops.counter, ops.n_ops, n, nullptr, nullptr, nullptr};
  if (scratch) {  // [n_ops] u64 counters, u32 actors, u32 flags
    J.w_ctr = (uint64_t*)scratch;
    J.w_act = (uint32_t*)(scratch + 8 * ops.n_ops);
    J.w_flag = (uint32_t*)(scratch + 12 * ops.n_ops);
  }
  hipLaunchKernelGGL(csr_apply_kernel, dim3(chunk_blocks(chunks)), dim3(kBlock), 0, stream, J, chunks, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_clock_csr_value(const crdt_clock_csr& self, uint64_t* out, int* status, hipStream_t stream) {
  const uint64_t n = self.n_obj, chunks = (n + kW - 1) / kW;
  if (chunks == 0) return CRDT_OK;
  hipLaunchKernelGGL(csr_value_kernel, dim3(chunk_blocks(chunks)), dim3(kBlock), 0, stream, in_of(self), out, n,
                     chunks, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_clock_csr_get(const crdt_clock_csr& self, const crdt_clock_ops& queries, uint64_t* out, int* status,
                         hipStream_t stream) {
  const uint64_t n = self.n_obj, chunks = (n + kW - 1) / kW;
  if (chunks == 0) return CRDT_OK;
  hipLaunchKernelGGL(csr_get_kernel, dim3(chunk_blocks(chunks)), dim3(kBlock), 0, stream, in_of(self), queries, out,
                     n, chunks, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
