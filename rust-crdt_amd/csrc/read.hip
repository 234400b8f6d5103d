// The batched read path (include/crdts_hip.h "Batched read path"):
// Orswot::contains / value (src/orswot.rs:214-233), Map::get / len
// (src/map.rs:282-302) and the contexts derived from them, ReadCtx::
// derive_add_ctx / derive_rm_ctx (src/ctx.rs:45-60), over Orswot record
// batches and over the outer arrays the three Map slabs share; and the value of
// Map::get: for Map<u64, MVReg> as rows of an MVReg slab, for Map<u64, Orswot>
// as Orswot records (a slab-to-record conversion, two calls), for the nested
// map as rows of a Map<u64, MVReg> slab (a gather by the used counts).
//
// Layout of a read. A wave takes 64 objects (lane k <-> object c + k: the query
// ranges and, for objects that have queries, the record header or the row's
// key count in one step) and then the chunk's queries flat, 64 at a time: a
// query finds its object by a 6-step search over the 64 range ends held in
// registers (for_each_in_ranges, csr_rank.h: the walk of the clocks' op path), so an object with 70
// queries and 70 objects with one query cost the same steps.
//
//   lane tier  one lane per query. The lane finds its key by binary search over
//              the object's ascending keys in HBM (a loop: any number of
//              members; 6 probes for 40 members, the probes of an object's
//              queries share its key lines), reads the two mem_dend words of
//              the member (Orswot) or nothing more (Map: the entry clock is row
//              `slot`), counts the non-zero slots of a dense row of at most
//              kLaneRun slots and, in the write call, copies a run of at most
//              kLaneRun pairs itself (a member's 1-3 dots: neighbouring lanes
//              write neighbouring pairs).
//   group tier (write call) a dense row of at most kLaneRun (16) slots is
//              emitted by 16 lanes, four queries a step (emit_rows16): the
//              16-actor add clocks of config 3 and of the Map benchmarks.
//              Left to the lanes these rows cost 16 stores a lane, each to a
//              line of its own.
//   wave tier  a run of more than kLaneRun (16) words or slots — a dense clock
//              row to count or to emit, a member's dot run, a CSR top clock,
//              the key list of value() — is handed to the whole wave: the lanes
//              that hold such a query are taken one by one (ballot) and the 64
//              lanes count non-zero slots or copy the run, coalesced, the kept
//              slots compacted with ballot + mbcnt. Config 3's 16-actor clocks
//              and 1-3 dot member clocks stay in the lane tier; a 64- or
//              128-actor row, a 1000-member value() do not.
//
// Both calls of the protocol (sizes, write) are the one kernel below with WRITE
// false / true: `locate` and `resolve_counts` derive the slot and the lengths
// for both, the write call checks every span against them before it stores.
// What a caller does not want is not read: without an add group and dot_ctr no
// load touches the top clock; with an actor and dot_ctr alone a dense clock
// costs the actor's one word.
//
// All offsets are 64-bit; stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "csr_rank.h"
#include "kernels.h"
#include "record_layout.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace csr_rank;

constexpr uint32_t kBlock = 256;
// lane tier / wave tier boundary: runs of more words (or dense slots) than
// this are counted and copied by the wave
constexpr uint32_t kLaneRun = 16;


// a resident grid: 8 blocks of 4 waves per CU of the current device (sched.h)
uint32_t chunk_blocks(uint64_t chunks) {
  return resident_blocks((chunks + kBlock / kW - 1) / (kBlock / kW));
}

// A clock as the kernels meet it: act == null is a dense row of n slots (slot k
// = actor k, 0 = absent), else n (actor, counter) pairs, actors ascending.
struct Run {
  const uint64_t* ctr;
  const uint32_t* act;
  uint32_t n;
};

// What the caller wants of a query (wave-uniform): the add group's pairs or
// length, the dot counter, the rm group, the key list.
struct Want {
  bool add, dot, rm, list;
};

// One object as its lane holds it: where it is (record byte offset / map row),
// its counts, and whether it can be read at all.
struct Obj {
  uint64_t at;
  uint32_t n_clk, n_mem, n_dot, ok;
};

struct OrswotSrc {
  const uint8_t* base;
  const uint64_t* off;
  uint64_t bytes;
  uint32_t A;
  bool sparse;
};

struct MapSrc {
  const uint64_t* clock;
  const uint32_t* n_keys;
  const uint64_t* keys;
  const uint64_t* eclock;
  uint32_t kcap, A;
};

// ---------------------------------------------------------------- the sources
__device__ __forceinline__ Obj open_obj(const OrswotSrc& S, uint64_t i, bool& bad) {
  Obj o{0, 0, 0, 0, 0};
  const uint64_t off = S.off[i];
  if (off > S.bytes || S.bytes - off < kHdrBytes || (((uintptr_t)S.base + off) & 15u)) {
    bad = true;
    return o;
  }
  const uint4* h = (const uint4*)(S.base + off);
  const uint4 h0 = h[0], h1 = h[1];  // size n_clk n_mem n_dot | n_def n_def_dot n_def_mem flags
  const bool sparse = (h1.w & CRDT_ORSWOT_SPARSE_CLOCK) != 0;
  const uint64_t need = record_size64(h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, sparse);
  const bool form = (h1.w & ~(CRDT_ORSWOT_SPARSE_CLOCK | CRDT_ORSWOT_EMPTY_MEMBER_CLOCK)) == 0u &&
                    sparse == S.sparse && (sparse ? h0.y <= S.A : h0.y == S.A);
  if (!form || need > h0.x || h0.x > S.bytes - off) {  // counts past the extent, extent past the batch
    bad = true;
    return o;
  }
  o.at = off;
  o.n_clk = h0.y;
  o.n_mem = h0.z;
  o.n_dot = h0.w;
  o.ok = 1u;
  return o;
}
__device__ __forceinline__ const uint64_t* keys_of(const OrswotSrc& S, const Obj& o) {
  const uint64_t cb = S.sparse ? ((12ull * o.n_clk + 7u) & ~7ull) : 8ull * o.n_clk;
  return (const uint64_t*)(S.base + o.at + kHdrBytes + cb);
}
__device__ __forceinline__ Run top_run(const OrswotSrc& S, const Obj& o) {
  const uint64_t* ctr = (const uint64_t*)(S.base + o.at + kHdrBytes);
  return Run{ctr, S.sparse ? (const uint32_t*)(ctr + o.n_clk) : nullptr, o.n_clk};
}
// member `pos`'s clock: its dot run, clamped to the record's n_dot
__device__ __forceinline__ Run entry_run(const OrswotSrc& S, const Obj& o, uint32_t pos) {
  const uint64_t* dctr = keys_of(S, o) + o.n_mem;
  const uint32_t* dact = (const uint32_t*)(dctr + o.n_dot);
  const uint32_t* dend = dact + o.n_dot;
  uint32_t d1 = dend[pos];
  d1 = d1 < o.n_dot ? d1 : o.n_dot;
  uint32_t d0 = pos ? dend[pos - 1u] : 0u;
  d0 = d0 < d1 ? d0 : d1;
  return Run{dctr + d0, dact + d0, d1 - d0};
}

__device__ __forceinline__ Obj open_obj(const MapSrc& S, uint64_t i, bool& bad) {
  const uint32_t nk = S.n_keys[i];
  if (nk > S.kcap) {
    bad = true;
    return Obj{0, 0, 0, 0, 0};
  }
  return Obj{i, S.A, nk, 0u, 1u};
}
__device__ __forceinline__ const uint64_t* keys_of(const MapSrc& S, const Obj& o) { return S.keys + o.at * S.kcap; }
__device__ __forceinline__ Run top_run(const MapSrc& S, const Obj& o) {
  return Run{S.clock + o.at * S.A, nullptr, S.A};
}
__device__ __forceinline__ Run entry_run(const MapSrc& S, const Obj& o, uint32_t pos) {
  return Run{S.eclock + (o.at * S.kcap + pos) * S.A, nullptr, S.A};
}

// ---------------------------------------------------------------- one query
// # of the ascending keys a[0, n) below x
__device__ __forceinline__ uint32_t lower_bound64(const uint64_t* a, uint32_t n, uint64_t x) {
  uint32_t lo = 0, len = n;
  while (len) {
    const uint32_t half = len >> 1;
    if (a[lo + half] < x) {
      lo += half + 1u;
      len -= half + 1u;
    } else {
      len = half;
    }
  }
  return lo;
}

// VClock::get
__device__ __forceinline__ uint64_t run_get(const Run& r, uint32_t actor) {
  if (!r.act) return actor < r.n ? r.ctr[actor] : 0ull;
  const uint64_t k = rank_mem(r.act, r.n, actor);
  return (k < r.n && r.act[k] == actor) ? r.ctr[k] : 0ull;
}

__device__ __forceinline__ bool wide(const Run& r) { return r.n > kLaneRun; }

// pairs of a run, by its lane (lane tier)
__device__ __forceinline__ uint32_t count_lane(const Run& r) {
  if (r.act) return r.n;
  uint32_t c = 0;
  for (uint32_t k = 0; k < r.n; ++k) c += r.ctr[k] != 0ull;
  return c;
}
// non-zero slots of a dense row, by the wave (wave tier; arguments uniform)
__device__ __forceinline__ uint32_t count_wave(const uint64_t* ctr, uint32_t n, uint32_t lane) {
  uint32_t c = 0;
  for (uint32_t k0 = 0; k0 < n; k0 += kW) {
    const uint32_t k = k0 + lane;
    c += (uint32_t)__popcll(__ballot(k < n && ctr[k] != 0ull));
  }
  return c;
}

// A query as located: the slot and value, the runs its groups come from, the
// witnessed dot (wa == NO_ACTOR: none; grow: the actor is new to the add clock).
struct Loc {
  uint64_t val, dot;
  uint32_t slot, wa, grow, list_n;
  Run add, rm;
  const uint64_t* list;
};

// The one routine both calls share: finds the key and picks the runs. Reads
// the header's counts (o), the probed keys, a member's two mem_dend words, and
// the top clock only for an add group or a dot.
template <class Src>
__device__ __forceinline__ Loc locate(const Src& S, const Obj& o, uint32_t kind, uint64_t key, uint32_t actor,
                                      const Want& w, bool& bad) {
  Loc L;
  L.val = L.dot = 0;
  L.slot = CRDT_READ_NO_SLOT;
  L.wa = CRDT_READ_NO_ACTOR;
  L.grow = L.list_n = 0;
  L.add = L.rm = Run{nullptr, nullptr, 0u};
  L.list = nullptr;
  if (!o.ok) return L;  // a bad record or row, or an unknown kind among the object's queries
  const uint64_t* K = keys_of(S, o);
  if (kind == CRDT_READ_KEY) {
    const uint32_t pos = lower_bound64(K, o.n_mem, key);
    if (pos < o.n_mem && K[pos] == key) {
      L.val = 1;
      L.slot = pos;
      if (w.rm) L.rm = entry_run(S, o, pos);
    }
  } else {
    L.val = o.n_mem;
    if (w.list) {
      L.list = K;
      L.list_n = o.n_mem;
    }
    if (w.rm) L.rm = top_run(S, o);
  }
  if (w.add) L.add = top_run(S, o);
  if (actor != CRDT_READ_NO_ACTOR) {
    if (actor >= S.A) {
      bad = true;  // answered as without an actor
    } else if (w.add || w.dot) {
      const uint64_t g = run_get(top_run(S, o), actor);
      if (g == ~0ull) {
        bad = true;  // VClock::inc overflows (src/vclock.rs:182-185): no dot
      } else {
        L.dot = g + 1u;
        L.wa = actor;
        L.grow = g == 0ull;
      }
    }
  }
  return L;
}

// The lengths of the add and rm groups: lane tier runs by their lane, dense rows
// past kLaneRun by the wave. Every lane of the wave calls this.
__device__ __forceinline__ void resolve_counts(const Loc& L, bool has, const Want& w, uint32_t lane, uint32_t& add_len,
                                               uint32_t& rm_len) {
  add_len = rm_len = 0;
  const bool add_w = has && w.add && !L.add.act && wide(L.add);
  const bool rm_w = has && w.rm && !L.rm.act && wide(L.rm);
  if (has && w.add && !add_w) add_len = count_lane(L.add);
  if (has && w.rm && !rm_w) rm_len = count_lane(L.rm);
  uint64_t pa = __ballot(add_w);
  while (pa) {
    const uint32_t t = (uint32_t)__builtin_ctzll(pa);
    pa &= pa - 1u;
    const uint32_t c = count_wave((const uint64_t*)lane64((uint64_t)L.add.ctr, t), lane32(L.add.n, t), lane);
    add_len = lane == t ? c : add_len;
  }
  uint64_t pr = __ballot(rm_w);
  while (pr) {
    const uint32_t t = (uint32_t)__builtin_ctzll(pr);
    pr &= pr - 1u;
    const uint32_t c = count_wave((const uint64_t*)lane64((uint64_t)L.rm.ctr, t), lane32(L.rm.n, t), lane);
    rm_len = lane == t ? c : rm_len;
  }
  if (has && w.add) add_len += L.grow;
}

// ---------------------------------------------------------------- the write call's stores
// The pairs of run r, with actor wa's counter set to wc (wa == NO_ACTOR: as it
// is), to oa / oc at [at, lim): a run of pairs by one lane ...
__device__ __forceinline__ void emit_lane(const Run& r, uint32_t wa, uint64_t wc, uint32_t* oa, uint64_t* oc,
                                          uint64_t at, uint64_t lim) {
  uint64_t p = at;
  bool done = wa == CRDT_READ_NO_ACTOR;
  for (uint32_t k = 0; k < r.n; ++k) {
    const uint32_t a = r.act[k];
    uint64_t c = r.ctr[k];
    if (!done && wa <= a) {
      done = true;
      if (wa < a) {
        if (p < lim) {
          oa[p] = wa;
          oc[p] = wc;
          ++p;
        }
      } else {
        c = wc;
      }
    }
    if (p < lim) {
      oa[p] = a;
      oc[p] = c;
      ++p;
    }
  }
  if (!done && p < lim) {
    oa[p] = wa;
    oc[p] = wc;
  }
}
// ... and by the wave (arguments uniform)
__device__ __forceinline__ void emit_wave(const Run& r, uint32_t wa, uint64_t wc, uint32_t* oa, uint64_t* oc,
                                          uint64_t at, uint64_t lim, uint32_t lane) {
  if (!r.act) {
    uint64_t p = at;
    for (uint32_t k0 = 0; k0 < r.n; k0 += kW) {
      const uint32_t k = k0 + lane;
      uint64_t c = k < r.n ? r.ctr[k] : 0ull;
      if (k < r.n && k == wa) c = wc;
      const uint64_t m = __ballot(c != 0ull);
      const uint64_t q = p + mbcnt(m);
      if (c && q < lim) {
        oa[q] = k;
        oc[q] = c;
      }
      p += (uint64_t)__popcll(m);
    }
    return;
  }
  uint32_t rk = r.n;
  bool present = false;
  if (wa != CRDT_READ_NO_ACTOR) {
    rk = (uint32_t)rank_mem(r.act, r.n, wa);
    present = rk < r.n && r.act[rk] == wa;
  }
  const bool ins = wa != CRDT_READ_NO_ACTOR && !present;
  for (uint32_t k0 = 0; k0 < r.n; k0 += kW) {
    const uint32_t k = k0 + lane;
    if (k < r.n) {
      const uint64_t c = (present && k == rk) ? wc : r.ctr[k];
      const uint64_t q = at + k + ((ins && k >= rk) ? 1u : 0u);
      if (q < lim) {
        oa[q] = r.act[k];
        oc[q] = c;
      }
    }
  }
  if (ins && lane == 0u && at + rk < lim) {
    oa[at + rk] = wa;
    oc[at + rk] = wc;
  }
}

// Query j's span [end[j-1], end[j]) of a group of n words: it must be `len` long.
__device__ __forceinline__ bool span_ok(const uint64_t* end, uint64_t j, uint64_t len, uint64_t n, uint64_t& at) {
  const uint64_t e = end[j];
  at = j ? end[j - 1u] : 0ull;
  return at <= e && e - at == len && e <= n;
}

// Dense rows of at most kLaneRun slots (group tier): 16 lanes per row, the rows
// of four queries per step — lane 16 g + k takes slot k of the query held by
// lane 4 step + g — so that a row's pairs leave as one 64-B and one 128-B
// piece instead of 16 stores a lane, each to a line of its own.
__device__ __forceinline__ void emit_rows16(const Run& r, bool go, uint32_t wa, uint64_t wc, uint32_t* oa,
                                            uint64_t* oc, uint64_t at, uint32_t len, uint32_t lane) {
  static_assert(kLaneRun == 16, "16 lanes per row");
  const uint64_t todo = __ballot(go);
  const uint32_t g = lane >> 4, k = lane & 15u;
  for (uint32_t step = 0; step < 16u; ++step) {
    if (!((todo >> (4u * step)) & 0xFull)) continue;  // none of the step's four queries (uniform)
    const uint32_t src = 4u * step + g;
    const bool on = rd32(go ? 1u : 0u, src) != 0u;
    const uint64_t* ctr = (const uint64_t*)rd64((uint64_t)r.ctr, src);
    const uint32_t n = rd32(r.n, src), a = rd32(wa, src), room = rd32(len, src);
    const uint64_t c_w = rd64(wc, src), a0 = rd64(at, src);
    uint64_t c = (on && k < n) ? ctr[k] : 0ull;
    if (on && k < n && k == a) c = c_w;
    const uint64_t m = __ballot(c != 0ull);
    const uint32_t below = (uint32_t)__popcll((m >> (16u * g)) & ((1ull << k) - 1ull));
    if (c && below < room) {
      oa[a0 + below] = k;
      oc[a0 + below] = c;
    }
  }
}

// One pair group of the 64 queries in flight: runs of pairs of the lane tier by
// their lanes, dense rows of the group tier four at a time, wide ones by the
// wave, one after the other.
__device__ __forceinline__ void emit_group(const Run& r, bool go, uint32_t wa, uint64_t wc, uint32_t* oa, uint64_t* oc,
                                           uint64_t at, uint32_t len, uint32_t lane) {
  const bool w = go && wide(r);
  const bool rows = go && !w && !r.act;
  if (go && !w && !rows) emit_lane(r, wa, wc, oa, oc, at, at + len);
  emit_rows16(r, rows, wa, wc, oa, oc, at, len, lane);
  uint64_t pend = __ballot(w);
  while (pend) {
    const uint32_t t = (uint32_t)__builtin_ctzll(pend);
    pend &= pend - 1u;
    const Run rt{(const uint64_t*)lane64((uint64_t)r.ctr, t), (const uint32_t*)lane64((uint64_t)r.act, t),
                 lane32(r.n, t)};
    const uint64_t a0 = lane64(at, t);
    emit_wave(rt, lane32(wa, t), lane64(wc, t), oa, oc, a0, a0 + lane32(len, t), lane);
  }
}

// An unknown kind closes its object: every query of it reads as nothing, in
// both calls and whatever step of the walk below holds it. A flat walk of the
// chunk's kinds (64 a step, coalesced) ahead of the answers; `ok` and `bad`
// are the object's lane's.
__device__ __forceinline__ void close_unknown_kinds(const crdt_read_queries& Q, bool valid, bool good, uint64_t b,
                                                    uint64_t e, uint32_t lane, uint32_t& ok, bool& bad) {
  for_each_in_ranges(valid, good, b, e, lane, [&](uint64_t j, bool has, uint32_t t) {
    uint64_t m = __ballot(has && Q.kind[j] > CRDT_READ_ALL);
    while (m) {
      const uint32_t u = (uint32_t)__builtin_ctzll(m);
      m &= m - 1u;
      if (lane == lane32(t, u)) {
        ok = 0u;
        bad = true;
      }
    }
  });
}

// ---------------------------------------------------------------- the kernels
// The queries of 64 objects are walked flat by for_each_in_ranges (csr_rank.h),
// the walk of the clocks' op path.
template <class Src, bool WRITE>
__global__ __launch_bounds__(kBlock) void read_kernel(Src S, crdt_read_queries Q, crdt_read_sizes Z, crdt_read_out O,
                                                      uint64_t n_obj, uint64_t chunks, int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  Want w;
  if (WRITE) {
    w.add = O.add_end != nullptr;
    w.rm = O.rm_end != nullptr;
    w.list = O.list_end != nullptr;
    w.dot = false;
  } else {
    w.add = Z.add_len != nullptr;
    w.rm = Z.rm_len != nullptr;
    w.list = Z.list_len != nullptr;
    w.dot = Z.dot_ctr != nullptr;
  }
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t c0 = ch * kW, i = c0 + lane;
    const bool valid = i < n_obj;
    uint64_t b = 0, e = 0;
    if (valid) {
      e = Q.obj_end[i];
      b = i ? Q.obj_end[i - 1u] : 0ull;
    }
    const bool good = b <= e && e <= Q.n_q;
    bool bad = valid && !good, over = false;
    Obj mine{0, 0, 0, 0, 0};
    if (valid && good && e > b) mine = open_obj(S, i, bad);  // objects without queries are not read
    close_unknown_kinds(Q, valid, good, b, e, lane, mine.ok, bad);
    for_each_in_ranges(valid, good, b, e, lane, [&](uint64_t j, bool has, uint32_t t) {
      const Obj o{rd64(mine.at, t), rd32(mine.n_clk, t), rd32(mine.n_mem, t), rd32(mine.n_dot, t), rd32(mine.ok, t)};
      Loc L;
      L.val = L.dot = 0;
      L.slot = CRDT_READ_NO_SLOT;
      L.wa = CRDT_READ_NO_ACTOR;
      L.grow = L.list_n = 0;
      L.add = L.rm = Run{nullptr, nullptr, 0u};
      L.list = nullptr;
      if (has) L = locate(S, o, Q.kind[j], Q.key[j], Q.actor ? Q.actor[j] : CRDT_READ_NO_ACTOR, w, bad);
      uint32_t add_len, rm_len;
      resolve_counts(L, has, w, lane, add_len, rm_len);
      if (!WRITE) {
        if (has) {
          if (Z.val) Z.val[j] = L.val;
          if (Z.slot) Z.slot[j] = L.slot;
          if (Z.dot_ctr) Z.dot_ctr[j] = L.dot;
          if (Z.add_len) Z.add_len[j] = add_len;
          if (Z.rm_len) Z.rm_len[j] = rm_len;
          if (Z.list_len) Z.list_len[j] = L.list_n;
        }
        return;
      }
      uint64_t at = 0;
      bool go = has && w.add && span_ok(O.add_end, j, add_len, O.n_add, at);
      over |= has && w.add && !go;
      emit_group(L.add, go, L.wa, L.dot, O.add_act, O.add_ctr, at, add_len, lane);
      go = has && w.rm && span_ok(O.rm_end, j, rm_len, O.n_rm, at);
      over |= has && w.rm && !go;
      emit_group(L.rm, go, CRDT_READ_NO_ACTOR, 0ull, O.rm_act, O.rm_ctr, at, rm_len, lane);
      // the key list: a copy, by the lane up to kLaneRun keys, else by the wave
      go = has && w.list && span_ok(O.list_end, j, L.list_n, O.n_list, at);
      over |= has && w.list && !go;
      const bool lw = go && L.list_n > kLaneRun;
      if (go && !lw)
        for (uint32_t k = 0; k < L.list_n; ++k) O.list_key[at + k] = L.list[k];
      uint64_t pend = __ballot(lw);
      while (pend) {
        const uint32_t u = (uint32_t)__builtin_ctzll(pend);
        pend &= pend - 1u;
        const uint64_t* src = (const uint64_t*)lane64((uint64_t)L.list, u);
        const uint32_t n = lane32(L.list_n, u);
        const uint64_t a0 = lane64(at, u);
        for (uint32_t k = lane; k < n; k += kW) O.list_key[a0 + k] = src[k];
      }
    });
    if (__ballot(bad) && lane == 0u) fail(status, CRDT_ENONCANON);
    if (__ballot(over) && lane == 0u) fail(status, CRDT_ECAPACITY);
  }
}

// ---------------------------------------------------------------- Map<u64, MVReg>::get's value
// Query j's register -> row j of the output slab: the lanes find their keys as
// above, then the wave copies the 64 registers one after the other, coalesced,
// zero-filling the slots past the count (crdt_mvreg_merge's convention).
__global__ __launch_bounds__(kBlock) void mvreg_get_kernel(MapSrc S, const uint32_t* mv_n, const uint64_t* mv_clock,
                                                           const uint64_t* mv_val, uint32_t mcap, crdt_read_queries Q,
                                                           uint32_t* out_n, uint64_t* out_clk, uint64_t* out_val,
                                                           uint32_t out_cap, uint64_t n_obj, uint64_t chunks,
                                                           int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const Want w{false, false, false, false};
  const uint32_t A = S.A;
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t c0 = ch * kW, i = c0 + lane;
    const bool valid = i < n_obj;
    uint64_t b = 0, e = 0;
    if (valid) {
      e = Q.obj_end[i];
      b = i ? Q.obj_end[i - 1u] : 0ull;
    }
    const bool good = b <= e && e <= Q.n_q;
    bool bad = valid && !good;
    Obj mine{0, 0, 0, 0, 0};
    if (valid && good && e > b) mine = open_obj(S, i, bad);
    close_unknown_kinds(Q, valid, good, b, e, lane, mine.ok, bad);
    for_each_in_ranges(valid, good, b, e, lane, [&](uint64_t j, bool has, uint32_t t) {
      const Obj o{rd64(mine.at, t), rd32(mine.n_clk, t), rd32(mine.n_mem, t), rd32(mine.n_dot, t), rd32(mine.ok, t)};
      uint64_t row = 0;  // the entry's row of the nested arrays
      uint32_t n = 0;
      if (has) {
        const Loc L = locate(S, o, Q.kind[j], Q.key[j], CRDT_READ_NO_ACTOR, w, bad);
        if (L.slot != CRDT_READ_NO_SLOT) {
          row = o.at * S.kcap + L.slot;
          n = mv_n[row];
          if (n > mcap) {
            n = 0u;
            bad = true;
          }
        }
        out_n[j] = n;
      }
      uint64_t pend = __ballot(has);
      while (pend) {
        const uint32_t u = (uint32_t)__builtin_ctzll(pend);
        pend &= pend - 1u;
        const uint64_t jr = lane64(j, u), rr = lane64(row, u);
        const uint32_t nn = lane32(n, u);
        const uint64_t* sc = mv_clock + rr * mcap * A;
        uint64_t* dc = out_clk + jr * out_cap * A;
        const uint64_t used = (uint64_t)nn * A, all = (uint64_t)out_cap * A;
        for (uint64_t k = lane; k < all; k += kW) dc[k] = k < used ? sc[k] : 0ull;
        const uint64_t* sv = mv_val + rr * mcap;
        uint64_t* dv = out_val + jr * out_cap;
        for (uint32_t k = lane; k < out_cap; k += kW) dv[k] = k < nn ? sv[k] : 0ull;
      }
    });
    if (__ballot(bad) && lane == 0u) fail(status, CRDT_ENONCANON);
  }
}

// ---------------------------------------------------------------- Map<u64, Orswot>::get's and the nested map's value
// The first step the three kernels below share with mvreg_get_kernel: a wave
// takes 64 objects' query ranges and each lane finds its key; f(j, has, row,
// found, lane, bad) is then called by every lane for every 64 queries: `row`
// is the nested value's row (object * kcap + slot) where `found`.
template <class F>
__device__ __forceinline__ void for_each_located(const MapSrc& S, const crdt_read_queries& Q, uint64_t n_obj,
                                                 uint64_t chunks, int* status, F f) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const Want w{false, false, false, false};
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t c0 = ch * kW, i = c0 + lane;
    const bool valid = i < n_obj;
    uint64_t b = 0, e = 0;
    if (valid) {
      e = Q.obj_end[i];
      b = i ? Q.obj_end[i - 1u] : 0ull;
    }
    const bool good = b <= e && e <= Q.n_q;
    bool bad = valid && !good;
    Obj mine{0, 0, 0, 0, 0};
    if (valid && good && e > b) mine = open_obj(S, i, bad);
    close_unknown_kinds(Q, valid, good, b, e, lane, mine.ok, bad);
    for_each_in_ranges(valid, good, b, e, lane, [&](uint64_t j, bool has, uint32_t t) {
      const Obj o{rd64(mine.at, t), rd32(mine.n_clk, t), rd32(mine.n_mem, t), rd32(mine.n_dot, t), rd32(mine.ok, t)};
      uint64_t row = 0;
      bool found = false;
      if (has) {
        const Loc L = locate(S, o, Q.kind[j], Q.key[j], CRDT_READ_NO_ACTOR, w, bad);
        found = L.slot != CRDT_READ_NO_SLOT;
        row = found ? o.at * S.kcap + L.slot : 0ull;
      }
      f(j, has, row, found, lane, bad);
    });
    if (__ballot(bad) && lane == 0u) fail(status, CRDT_ENONCANON);
  }
}

// The non-zero cells of `rows` dense clock rows of A cells each, contiguous at
// p, walked row-major 64 cells a step (a row's end falls anywhere in a step):
// cell(r, a, c, at) for slot a of row r holding c != 0, the at-th non-zero
// cell (the wave prefix: mbcnt of the step's ballot plus the running base);
// row_end(r, end) by the lane of row r's last slot, `end` the cells up to and
// including the row's. A lane that ends a row without cells sets `hollow`.
// Returns the number of cells. Arguments uniform; rows * A fits 32 bits.
template <class F, class G>
__device__ __forceinline__ uint32_t walk_rows(const uint64_t* p, uint32_t rows, uint32_t A, uint32_t lane, bool& hollow,
                                              F cell, G row_end) {
  const uint32_t cells = rows * A, dr = kW / A, da = kW % A;
  uint32_t base = 0, last_end = 0, r = lane / A, a = lane % A;
  for (uint32_t c0 = 0; c0 < cells; c0 += kW) {
    const bool in = lane < cells - c0;
    const uint64_t c = in ? p[c0 + lane] : 0ull;
    const uint64_t m = __ballot(c != 0ull);
    const uint32_t incl = base + mbcnt(m) + (c != 0ull ? 1u : 0u);
    if (c) cell(r, a, c, incl - 1u);
    const bool end = in && a == A - 1u;
    // the end of the row before: A lanes below, or the last one of an earlier step
    const uint32_t below = rd32(incl, (lane - A) & 63u);
    const uint32_t prev = lane >= A ? below : last_end;
    if (end) row_end(r, incl);
    hollow |= end && incl == prev;
    const uint64_t em = __ballot(end);
    if (em) last_end = lane32(incl, 63u - (uint32_t)__builtin_clzll(em));
    base += (uint32_t)__popcll(m);
    r += dr;
    a += da;
    if (a >= A) {
      a -= A;
      ++r;
    }
  }
  return base;
}

// The nested Orswots of a Map<u64, Orswot> slab.
struct OrswotVals {
  const uint64_t* vclock;
  const uint32_t* vn_mem;
  const uint64_t* vmem;
  const uint64_t* vmclock;
  const uint32_t* vn_def;
  const uint64_t* vdclock;
  const uint32_t* vdset_n;
  const uint64_t* vdset;
  uint32_t mcap, vdcap, vscap, A;
};
// The counts of a value's record and its size (record_size64: the formula of
// crdt_orswot_record_bytes).
struct ValCounts {
  uint32_t n_mem, n_dot, n_def, n_def_dot, n_def_mem;
  uint64_t size;
};
__device__ __forceinline__ ValCounts default_counts(uint32_t A) {
  return ValCounts{0u, 0u, 0u, 0u, 0u, record_size64(A, 0u, 0u, 0u, 0u, 0u)};
}

// Counts the value at `row` by its used slots, for both calls. False: the
// counts exceed the capacities, a deferred clock row is all zero, a deferred
// set is empty, or the record would outgrow its 32-bit size — c is then the
// default's. Arguments uniform.
__device__ __forceinline__ bool count_value(const OrswotVals& V, uint64_t row, uint32_t lane, ValCounts& c) {
  const uint32_t A = V.A;
  c = default_counts(A);
  const uint32_t nm = V.vn_mem[row], nd = V.vn_def[row];
  if (nm > V.mcap || nd > V.vdcap || (uint64_t)nm * A > 0xffffffffull || (uint64_t)nd * A > 0xffffffffull)
    return false;
  uint64_t in_sets = 0;
  bool bad_set = false;
  for (uint32_t d0 = 0; d0 < nd; d0 += kW) {
    const uint32_t d = d0 + lane;
    const uint32_t n = d < nd ? V.vdset_n[row * V.vdcap + d] : 1u;
    bad_set |= n == 0u || n > V.vscap;
    in_sets += d < nd ? n : 0u;
  }
  if (__ballot(bad_set)) return false;
  in_sets = lane64(wave_incl_scan(in_sets, lane), kW - 1u);
  bool hollow = false;
  const auto no_cell = [](uint32_t, uint32_t, uint64_t, uint32_t) {};
  const auto no_end = [](uint32_t, uint32_t) {};
  const uint32_t def_dot = walk_rows(V.vdclock + row * V.vdcap * A, nd, A, lane, hollow, no_cell, no_end);
  if (__ballot(hollow)) return false;
  const uint32_t dot = walk_rows(V.vmclock + row * V.mcap * A, nm, A, lane, hollow, no_cell, no_end);
  if (in_sets > 0xffffffffull) return false;
  const uint64_t size = record_size64(A, nm, dot, nd, def_dot, (uint32_t)in_sets);
  if (size > 0xffffffffull) return false;
  c = ValCounts{nm, dot, nd, def_dot, (uint32_t)in_sets, size};
  return true;
}

// Writes the record of the value at `row` (`ok`: else the default record) with
// counts c to R (16-B aligned, c.size bytes). Arguments uniform.
__device__ __forceinline__ void write_value(const OrswotVals& V, uint64_t row, bool ok, const ValCounts& c, uint8_t* R,
                                            uint32_t lane) {
  const uint32_t A = V.A;
  RecLayout L;
  rec_layout(L, A, c.n_mem, c.n_dot, c.n_def, c.n_def_dot, c.n_def_mem);
  uint64_t* clk = (uint64_t*)(R + L.o_clk);
  for (uint32_t k = lane; k < A; k += kW) clk[k] = ok ? V.vclock[row * A + k] : 0ull;
  uint32_t flags = 0u;
  if (ok) {
    uint64_t* key = (uint64_t*)(R + L.o_key);
    for (uint32_t k = lane; k < c.n_mem; k += kW) key[k] = V.vmem[row * V.mcap + k];
    uint64_t* dctr = (uint64_t*)(R + L.o_dctr);
    uint32_t* dact = (uint32_t*)(R + L.o_dact);
    uint32_t* mdend = (uint32_t*)(R + L.o_mdend);
    bool hollow = false;
    walk_rows(
        V.vmclock + row * V.mcap * A, c.n_mem, A, lane, hollow,
        [&](uint32_t, uint32_t a, uint64_t v, uint32_t at) {
          if (at < c.n_dot) {
            dctr[at] = v;
            dact[at] = a;
          }
        },
        [&](uint32_t r, uint32_t end) { mdend[r] = end; });
    if (__ballot(hollow)) flags = CRDT_ORSWOT_EMPTY_MEMBER_CLOCK;
    if (L.o_def != L.o_mpad && lane == 0u) *(uint32_t*)(R + L.o_mpad) = 0u;
    uint64_t* fctr = (uint64_t*)(R + L.o_fctr);
    uint64_t* fkey = (uint64_t*)(R + L.o_fkey);
    uint32_t* fact = (uint32_t*)(R + L.o_fact);
    uint32_t* fdend = (uint32_t*)(R + L.o_fdend);
    uint32_t* fmend = (uint32_t*)(R + L.o_fmend);
    walk_rows(
        V.vdclock + row * V.vdcap * A, c.n_def, A, lane, hollow,
        [&](uint32_t, uint32_t a, uint64_t v, uint32_t at) {
          if (at < c.n_def_dot) {
            fctr[at] = v;
            fact[at] = a;
          }
        },
        [&](uint32_t r, uint32_t end) { fdend[r] = end; });
    uint32_t mbase = 0;
    for (uint32_t d0 = 0; d0 < c.n_def; d0 += kW) {
      const uint32_t d = d0 + lane;
      const uint32_t n = d < c.n_def ? V.vdset_n[row * V.vdcap + d] : 0u;
      const uint32_t incl = scan_incl(n, lane);
      if (d < c.n_def) fmend[d] = mbase + incl;
      const uint32_t cnt = c.n_def - d0 < kW ? c.n_def - d0 : kW;
      for (uint32_t t = 0; t < cnt; ++t) {
        const uint32_t nt = lane32(n, t), at = mbase + lane32(incl, t) - nt;
        const uint64_t* src = V.vdset + (row * V.vdcap + d0 + t) * V.vscap;
        for (uint32_t k = lane; k < nt; k += kW)
          if (at + k < c.n_def_mem) fkey[at + k] = src[k];
      }
      mbase += lane32(incl, kW - 1u);
    }
  }
  if (L.o_end + 4u * lane < L.size) *(uint32_t*)(R + L.o_end + 4u * lane) = 0u;
  if (lane == 0u) {
    uint4* h = (uint4*)R;
    h[0] = make_uint4((uint32_t)c.size, A, c.n_mem, c.n_dot);
    h[1] = make_uint4(c.n_def, c.n_def_dot, c.n_def_mem, flags);
  }
}

// Query j's record size and whether it is a located value's.
__global__ __launch_bounds__(kBlock) void map_orswot_get_sizes_kernel(MapSrc S, OrswotVals V, crdt_read_queries Q,
                                                                      uint64_t* sizes, uint32_t* present,
                                                                      uint64_t n_obj, uint64_t chunks, int* status) {
  for_each_located(S, Q, n_obj, chunks, status,
                   [&](uint64_t j, bool has, uint64_t row, bool found, uint32_t lane, bool& bad) {
                     uint64_t size = default_counts(V.A).size;
                     uint32_t pres = 0u;
                     uint64_t pend = __ballot(has && found);
                     while (pend) {
                       const uint32_t u = (uint32_t)__builtin_ctzll(pend);
                       pend &= pend - 1u;
                       ValCounts c;
                       const bool ok = count_value(V, lane64(row, u), lane, c);
                       if (lane == u) {
                         size = c.size;
                         pres = ok ? 1u : 0u;
                         bad |= !ok;
                       }
                     }
                     if (has) {
                       sizes[j] = size;
                       if (present) present[j] = pres;
                     }
                   });
}

// Query j's record at out + ooff[j]: the counts are taken again, never from
// the sizes call; a record that is misplaced is not written.
__global__ __launch_bounds__(kBlock) void map_orswot_get_kernel(MapSrc S, OrswotVals V, crdt_read_queries Q,
                                                                uint8_t* out, const uint64_t* ooff, uint64_t out_bytes,
                                                                uint64_t n_obj, uint64_t chunks, int* status) {
  for_each_located(S, Q, n_obj, chunks, status,
                   [&](uint64_t j, bool has, uint64_t row, bool found, uint32_t lane, bool& bad) {
                     const uint64_t off = has ? ooff[j] : 0ull;
                     bool over = false;
                     uint64_t pend = __ballot(has);
                     while (pend) {
                       const uint32_t u = (uint32_t)__builtin_ctzll(pend);
                       pend &= pend - 1u;
                       const bool fnd = lane32(found ? 1u : 0u, u) != 0u;
                       const uint64_t ru = lane64(row, u), at = lane64(off, u);
                       ValCounts c = default_counts(V.A);
                       const bool ok = fnd && count_value(V, ru, lane, c);
                       if (lane == u) bad |= fnd && !ok;
                       if ((((uintptr_t)out + at) & 15u) || at > out_bytes || out_bytes - at < c.size) {
                         if (lane == u) over = true;
                         continue;
                       }
                       write_value(V, ru, ok, c, out + at, lane);
                     }
                     if (__ballot(over) && lane == 0u) fail(status, CRDT_ECAPACITY);
                   });
}

// Query j's inner map -> row j of `O`, a gather by the used counts: source
// strides are I's capacities, destination strides O's. A value whose counts
// exceed I's capacities, an absent key and an ALL query give the empty map.
__global__ __launch_bounds__(kBlock) void map_map_get_kernel(MapSrc S, crdt_map_mvreg_slab I, crdt_read_queries Q,
                                                             crdt_map_mvreg_slab O, uint32_t* present, uint64_t n_obj,
                                                             uint64_t chunks, int* status) {
  const uint32_t A = S.A;
  for_each_located(S, Q, n_obj, chunks, status,
                   [&](uint64_t j, bool has, uint64_t row, bool found, uint32_t lane, bool& bad) {
    uint32_t pres = 0u;
    uint64_t pend = __ballot(has);
    while (pend) {
      const uint32_t u = (uint32_t)__builtin_ctzll(pend);
      pend &= pend - 1u;
      const uint64_t jr = lane64(j, u), rr = lane64(row, u);
      bool ok = lane32(found ? 1u : 0u, u) != 0u;
      uint32_t nk = 0u, nd = 0u;
      if (ok) {
        nk = I.n_keys[rr];
        nd = I.n_def[rr];
        bool big = nk > I.kcap || nd > I.dcap;
        if (!big) {
          for (uint32_t k = lane; k < nk; k += kW) big |= I.mv_n[rr * I.kcap + k] > I.mcap;
          for (uint32_t d = lane; d < nd; d += kW) big |= I.dset_n[rr * I.dcap + d] > I.scap;
        }
        ok = !__ballot(big);
        if (lane == u) {
          pres = ok ? 1u : 0u;
          bad |= !ok;
        }
        if (!ok) nk = nd = 0u;
      }
      for (uint32_t k = lane; k < A; k += kW) O.clock[jr * A + k] = ok ? I.clock[rr * A + k] : 0ull;
      if (lane == 0u) {
        O.n_keys[jr] = nk;
        O.n_def[jr] = nd;
      }
      // the entries: keys, entry clocks (nk rows of A, contiguous on both sides), registers
      for (uint32_t k = lane; k < nk; k += kW) O.keys[jr * O.kcap + k] = I.keys[rr * I.kcap + k];
      {
        const uint64_t* s = I.eclock + rr * I.kcap * A;
        uint64_t* d = O.eclock + jr * O.kcap * A;
        for (uint32_t k = lane; k < nk * A; k += kW) d[k] = s[k];
      }
      for (uint32_t k0 = 0; k0 < nk; k0 += kW) {
        const uint32_t k = k0 + lane;
        const uint32_t n = k < nk ? I.mv_n[rr * I.kcap + k] : 0u;
        if (k < nk) O.mv_n[jr * O.kcap + k] = n;
        const uint32_t cnt = nk - k0 < kW ? nk - k0 : kW;
        for (uint32_t t = 0; t < cnt; ++t) {
          const uint32_t nt = lane32(n, t);
          const uint64_t sr = rr * I.kcap + k0 + t, dr = jr * O.kcap + k0 + t;
          const uint64_t* sc = I.mv_clock + sr * I.mcap * A;
          uint64_t* dc = O.mv_clock + dr * O.mcap * A;
          for (uint32_t x = lane; x < nt * A; x += kW) dc[x] = sc[x];
          for (uint32_t x = lane; x < nt; x += kW) O.mv_val[dr * O.mcap + x] = I.mv_val[sr * I.mcap + x];
        }
      }
      // the deferred removes
      {
        const uint64_t* s = I.dclock + rr * I.dcap * A;
        uint64_t* d = O.dclock + jr * O.dcap * A;
        for (uint32_t k = lane; k < nd * A; k += kW) d[k] = s[k];
      }
      for (uint32_t d0 = 0; d0 < nd; d0 += kW) {
        const uint32_t d = d0 + lane;
        const uint32_t n = d < nd ? I.dset_n[rr * I.dcap + d] : 0u;
        if (d < nd) O.dset_n[jr * O.dcap + d] = n;
        const uint32_t cnt = nd - d0 < kW ? nd - d0 : kW;
        for (uint32_t t = 0; t < cnt; ++t) {
          const uint32_t nt = lane32(n, t);
          const uint64_t* ss = I.dset + (rr * I.dcap + d0 + t) * I.scap;
          uint64_t* ds = O.dset + (jr * O.dcap + d0 + t) * O.scap;
          for (uint32_t x = lane; x < nt; x += kW) ds[x] = ss[x];
        }
      }
    }
    if (has && present) present[j] = pres;
  });
}

template <class Src>
int launch_read(const Src& S, const crdt_read_queries& Q, const crdt_read_sizes* Z, const crdt_read_out* O,
                uint64_t n_obj, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const uint64_t chunks = (n_obj + kW - 1) / kW;
  const dim3 grid(chunk_blocks(chunks)), block(kBlock);
  if (Z)
    hipLaunchKernelGGL((read_kernel<Src, false>), grid, block, 0, stream, S, Q, *Z, crdt_read_out{}, n_obj, chunks,
                       status);
  else
    hipLaunchKernelGGL((read_kernel<Src, true>), grid, block, 0, stream, S, Q, crdt_read_sizes{}, *O, n_obj, chunks,
                       status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace

int launch_orswot_read(const crdt_orswot_batch& B, const crdt_read_queries& Q, uint32_t A, uint32_t flags,
                       const crdt_read_sizes* sizes, const crdt_read_out* out, int* status, hipStream_t stream) {
  const OrswotSrc S{B.base, B.off, B.bytes, A, (flags & CRDT_ORSWOT_SPARSE_CLOCK) != 0u};
  return launch_read(S, Q, sizes, out, B.n_obj, status, stream);
}

int launch_map_read(const crdt_map_read_view& V, const crdt_read_queries& Q, uint64_t n_obj, uint32_t A,
                    const crdt_read_sizes* sizes, const crdt_read_out* out, int* status, hipStream_t stream) {
  const MapSrc S{V.clock, V.n_keys, V.keys, V.eclock, V.kcap, A};
  return launch_read(S, Q, sizes, out, n_obj, status, stream);
}

int launch_map_mvreg_get(const crdt_map_mvreg_slab& M, const crdt_read_queries& Q, uint64_t n_obj, uint32_t A,
                         uint32_t* out_n, uint64_t* out_clk, uint64_t* out_val, uint32_t out_cap, int* status,
                         hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const MapSrc S{M.clock, M.n_keys, M.keys, M.eclock, M.kcap, A};
  const uint64_t chunks = (n_obj + kW - 1) / kW;
  hipLaunchKernelGGL(mvreg_get_kernel, dim3(chunk_blocks(chunks)), dim3(kBlock), 0, stream, S, M.mv_n, M.mv_clock,
                     M.mv_val, M.mcap, Q, out_n, out_clk, out_val, out_cap, n_obj, chunks, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_map_orswot_get(const crdt_map_orswot_slab& M, const crdt_read_queries& Q, uint64_t n_obj, uint32_t A,
                          uint64_t* sizes, uint32_t* present, uint8_t* out, const uint64_t* ooff, uint64_t out_bytes,
                          int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const MapSrc S{M.clock, M.n_keys, M.keys, M.eclock, M.kcap, A};
  const OrswotVals V{M.vclock, M.vn_mem, M.vmem, M.vmclock, M.vn_def, M.vdclock, M.vdset_n, M.vdset,
                     M.mcap,   M.vdcap,  M.vscap, A};
  const uint64_t chunks = (n_obj + kW - 1) / kW;
  const dim3 grid(chunk_blocks(chunks)), block(kBlock);
  if (sizes)
    hipLaunchKernelGGL(map_orswot_get_sizes_kernel, grid, block, 0, stream, S, V, Q, sizes, present, n_obj, chunks,
                       status);
  else
    hipLaunchKernelGGL(map_orswot_get_kernel, grid, block, 0, stream, S, V, Q, out, ooff, out_bytes, n_obj, chunks,
                       status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

int launch_map_map_get(const crdt_map_map_slab& M, const crdt_read_queries& Q, uint64_t n_obj, uint32_t A,
                       const crdt_map_mvreg_slab& out, uint32_t* present, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const MapSrc S{M.clock, M.n_keys, M.keys, M.eclock, M.kcap, A};
  const uint64_t chunks = (n_obj + kW - 1) / kW;
  hipLaunchKernelGGL(map_map_get_kernel, dim3(chunk_blocks(chunks)), dim3(kBlock), 0, stream, S, M.inner, Q, out,
                     present, n_obj, chunks, status);
  return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP;
}

}  // namespace crdts_hip
