// bincode codec of the Orswot, MVReg and Map op streams (include/crdts_hip.h
// "bincode of the Orswot, MVReg and Map ops"): the reference's `Op` enums as
// they travel between replicas, into and out of the arrays of crdt_orswot_ops,
// crdt_mvreg_ops and crdt_map_*_ops.
//
// Wire format (bincode 0.9 of the serde derives; an enum is a u32 variant
// index and its fields in declaration order; A / K / K2 / V = actor / key /
// key2 / val of wa / wk / w2 / wv bytes, little-endian):
//   VClock     u64 n | n x (A actor | u64 counter), actors strictly ascending
//   Orswot Op  Add: 0 | A | u64 | K2 member        Rm: 1 | VClock | K2 member
//   MVReg  Op  Put: 0 | VClock | V val
//   Map    Op  Nop: 0    Rm: 1 | VClock | K key    Up: 2 | A | u64 | K key | <V::Op>
// An op is a head of fixed fields, at most one clock, and at most one field
// after it (the tail): which fields, and so the position of the clock and of
// the tail, is a pure function of the variant indices and the widths (shape()).
//   ingest  a lane frames one op (frame(): the variant words, the clock's
//           length word against the bytes left, the exact blob length); the
//           pairs of 64 ops are then walked flat across the wave over the ops'
//           clk_end spans (for_each_in_ranges, csr_rank.h): lane j takes flat
//           pair j, its neighbour below holds the pair before it (lane 0
//           re-reads), a bad pair marks its op's lane through a ballot, and
//           only then does that lane write the fixed fields.
//   egest   the mirror image: a lane per op validates and sizes, the same walk
//           checks the pairs, the lane stores the head, the length word and
//           the tail in aligned pieces (blob.h wr_le), a second walk stores the
//           pairs. The sizes call is the same kernel without the stores.
// Fields are read as in the clock codec: the one or two aligned 8-byte words
// that hold them, where those lie inside d_blobs. Nothing outside a blob is
// written.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "blob.h"
#include "csr_rank.h"
#include "kernels.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace blob;
using namespace csr_rank;

constexpr uint32_t kBlock = 256;

// ------------------------------------------------------------------- shapes
// What an op carries, in wire order: variant word, S_DOT, S_KEY, S_V1 (the
// nested op's variant word), S_DOT2, S_KEY2, S_PUT (the innermost Put's variant
// word), S_CLOCK, then one tail field. S_DUP: the second dot is the first one
// again (Map<Orswot>: the nested Add's dot is the Up's).
enum : uint32_t {
  S_DOT = 1u, S_KEY = 2u, S_V1 = 4u, S_DOT2 = 8u, S_DUP = 16u, S_KEY2 = 32u, S_PUT = 64u, S_CLOCK = 128u,
  S_TKEY = 256u, S_TKEY2 = 512u, S_TVAL = 1024u,
};

template <uint32_t T>
constexpr bool is_map() {
  return T == CRDT_OPS_MAP_MVREG || T == CRDT_OPS_MAP_ORSWOT || T == CRDT_OPS_MAP_MAP;
}
// the last variant index of the op and of the op nested in a Map's Up
template <uint32_t T>
constexpr uint32_t last0() {
  return T == CRDT_OPS_ORSWOT ? 1u : T == CRDT_OPS_MVREG ? 0u : 2u;
}
template <uint32_t T>
constexpr uint32_t last1() {
  return T == CRDT_OPS_MAP_MVREG ? 0u : T == CRDT_OPS_MAP_ORSWOT ? 1u : 2u;
}

template <uint32_t T>
__device__ __forceinline__ uint32_t shape(uint32_t v0, uint32_t v1) {
  if (T == CRDT_OPS_ORSWOT) return v0 == 0u ? S_DOT | S_KEY2 : S_CLOCK | S_TKEY2;
  if (T == CRDT_OPS_MVREG) return S_CLOCK | S_TVAL;
  if (v0 == 0u) return 0u;
  if (v0 == 1u) return S_CLOCK | S_TKEY;
  constexpr uint32_t up = S_DOT | S_KEY | S_V1;
  if (T == CRDT_OPS_MAP_MVREG) return up | S_CLOCK | S_TVAL;
  if (T == CRDT_OPS_MAP_ORSWOT) return v1 == 0u ? up | S_DOT2 | S_DUP | S_KEY2 : up | S_CLOCK | S_TKEY2;
  return v1 == 0u ? up : v1 == 1u ? up | S_CLOCK | S_TKEY2 : up | S_DOT2 | S_KEY2 | S_PUT | S_CLOCK | S_TVAL;
}

// variant indices <-> the kind of the crdt_*_ops structs
template <uint32_t T>
__device__ __forceinline__ uint32_t kind_of(uint32_t v0, uint32_t v1) {
  if (!is_map<T>() || v0 < 2u) return v0;
  if (T == CRDT_OPS_MAP_MVREG) return CRDT_MAP_OP_UP;
  if (T == CRDT_OPS_MAP_ORSWOT) return CRDT_MAP_OP_UP + v1;  // Add: UP 2, Rm: UP_RM 3
  return CRDT_MAPMAP_OP_UP_NOP - v1;                         // Nop: 4, Rm: 3, Up: 2
}
template <uint32_t T>
__device__ __forceinline__ bool variants_of(uint32_t kind, uint32_t& v0, uint32_t& v1) {
  v0 = v1 = 0u;
  if (T == CRDT_OPS_MVREG) return true;  // no kind array: every op is a Put
  if (kind < 2u) {
    v0 = kind;
    return true;
  }
  if (!is_map<T>()) return false;
  v0 = 2u;
  if (T == CRDT_OPS_MAP_MVREG) return kind == CRDT_MAP_OP_UP;
  if (T == CRDT_OPS_MAP_ORSWOT) {
    v1 = kind - CRDT_MAP_OP_UP;
    return kind <= CRDT_MAP_OP_UP_RM;
  }
  v1 = CRDT_MAPMAP_OP_UP_NOP - kind;
  return kind <= CRDT_MAPMAP_OP_UP_NOP;
}

__device__ __forceinline__ uint64_t head_bytes(uint32_t sh, const crdt_op_widths& W) {
  const uint64_t E = W.actor_bytes + 8u;
  return 4u + (sh & S_DOT ? E : 0u) + (sh & S_KEY ? W.key_bytes : 0u) + (sh & S_V1 ? 4u : 0u) +
         (sh & S_DOT2 ? E : 0u) + (sh & S_KEY2 ? W.key2_bytes : 0u) + (sh & S_PUT ? 4u : 0u);
}
__device__ __forceinline__ uint64_t tail_bytes(uint32_t sh, const crdt_op_widths& W) {
  return sh & S_TKEY ? W.key_bytes : sh & S_TKEY2 ? W.key2_bytes : sh & S_TVAL ? W.val_bytes : 0u;
}

// ------------------------------------------------------------------ framing
// One op blob against the bytes it has: the variant words, the clock's length
// word (checked against the bytes left before any multiply; no canonical clock
// has 2^32 pairs) and the exact length. n pairs start at byte cpos of d_blobs,
// the tail field at byte tpos. The one function of _clk_lens and
// _from_bincode, so the two calls cannot disagree.
struct Frame {
  bool ok;
  uint32_t sh, kind;
  uint64_t n, at, cpos, tpos;
};

template <uint32_t T>
__device__ __forceinline__ Frame frame(const uint8_t* blobs, uint64_t blob_bytes, uint64_t off, uint64_t len,
                                       const crdt_op_widths& W, const Bounds& src) {
  Frame F{};
  F.kind = CRDT_OP_KIND_BAD;
  if (!(off <= blob_bytes && len <= blob_bytes - off) || len < 4u) return F;
  const uint8_t* p = blobs + off;
  const uint64_t E = W.actor_bytes + 8u;
  const uint32_t v0 = (uint32_t)rd_le<4>(p, src);  // all four bytes of a variant index
  if (v0 > last0<T>()) return F;
  uint32_t v1 = 0;
  if (is_map<T>() && v0 == 2u) {
    const uint64_t q = 4u + E + W.key_bytes;
    if (len < q + 4u) return F;
    v1 = (uint32_t)rd_le<4>(p + q, src);
    if (v1 > last1<T>()) return F;
  }
  const uint32_t sh = shape<T>(v0, v1);
  const uint64_t H = head_bytes(sh, W), Tl = tail_bytes(sh, W);
  if (len < H + (sh & S_CLOCK ? 8u + Tl : 0u)) return F;
  if ((sh & S_PUT) && rd_le<4>(p + H - 4u, src) != 0ull) return F;
  uint64_t n = 0;
  if (sh & S_CLOCK) {
    n = rd_le<8>(p + H, src);
    const uint64_t rem = len - H - 8u - Tl;
    if (n > rem / E || n > 0xffffffffull || n * E != rem) return F;
  } else if (len != H) {
    return F;
  }
  F.ok = true;
  F.sh = sh;
  F.kind = kind_of<T>(v0, v1);
  F.n = n;
  F.at = off;
  F.cpos = off + H + 8u;
  F.tpos = off + len - Tl;
  return F;
}

// the pairs an op owns in clk_act / clk_ctr: a badly framed Put keeps one, for
// the sentinel crdt_mvreg_apply rejects (it has no kind to carry it)
template <uint32_t T>
__device__ __forceinline__ uint64_t span_pairs(const Frame& F) {
  return F.ok ? F.n : (T == CRDT_OPS_MVREG ? 1ull : 0ull);
}

// ------------------------------------------------------------------- ingest
template <uint32_t T>
__global__ __launch_bounds__(kBlock) void lens_kernel(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                                      const uint64_t* blen, uint64_t n_ops, crdt_op_widths W,
                                                      uint32_t* clk_len, int* status) {
  const Bounds src{(uintptr_t)blobs, (uintptr_t)blobs + blob_bytes};
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_ops; i += (uint64_t)gridDim.x * kBlock) {
    const Frame F = frame<T>(blobs, blob_bytes, boff[i], blen[i], W, src);
    if (!F.ok) fail(status, CRDT_ENONCANON);
    clk_len[i] = (uint32_t)span_pairs<T>(F);
  }
}

template <uint32_t T>
__global__ __launch_bounds__(kBlock) void from_kernel(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                                      const uint64_t* blen, crdt_op_widths W, crdt_op_arrays A,
                                                      uint32_t* op_err, uint64_t chunks, int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const Bounds src{(uintptr_t)blobs, (uintptr_t)blobs + blob_bytes};
  const uint32_t wa = W.actor_bytes;
  const uint64_t E = wa + 8u;
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    const bool valid = i < A.n_ops;
    Frame F{};
    F.kind = CRDT_OP_KIND_BAD;
    uint64_t b = 0, e = 0;
    if (valid) {
      F = frame<T>(blobs, blob_bytes, boff[i], blen[i], W, src);
      e = A.clk_end[i];
      b = i ? A.clk_end[i - 1u] : 0ull;
    }
    const bool inside = b <= e && e <= A.n_clk;  // the caller's span lies in the pair arrays
    const bool span_ok = inside && e - b == span_pairs<T>(F);
    int err = !valid ? CRDT_OK : !F.ok ? CRDT_ENONCANON : !span_ok ? CRDT_ECAPACITY : CRDT_OK;
    // the pairs, flat: lane j <-> pair j of the chunk's spans
    const uint64_t livem = __ballot(valid && F.ok && span_ok);
    uint64_t badobj = 0;
    for_each_in_ranges(valid, inside, b, e, lane, [&](uint64_t j, bool has, uint32_t t) {
      const bool live = has && ((livem >> t) & 1u);
      const uint64_t k = j - rd64(b, t);
      const uint8_t* p = blobs + rd64(F.cpos, t) + k * E;
      uint64_t a = 0, c = 1;
      if (live) {
        a = rd_le(p, wa, src);
        c = rd_le<8>(p + wa, src);
      }
      uint64_t prev = rd64(a, (lane - 1u) & 63u);  // pair k - 1 of the same op, except in lane 0
      if (live && k && lane == 0u) prev = rd_le(p - E, wa, src);
      const bool bad = live && (c == 0ull || (a >> 32) != 0ull || (k && prev >= a));
      badobj |= owners(bad, t);
      if (live && !bad) {
        A.clk_act[j] = (uint32_t)a;
        A.clk_ctr[j] = c;
      }
    });
    // the fixed fields: fields the kind does not carry are 0
    uint64_t act = 0, ctr = 0, key = 0, act2 = 0, ctr2 = 0, key2 = 0, val = 0;
    bool mybad = (badobj >> lane) & 1u;
    if (valid && F.ok) {
      const uint8_t* q = blobs + F.at + 4u;
      const uint8_t* tp = blobs + F.tpos;
      const uint32_t sh = F.sh;
      if (sh & S_DOT) {
        act = rd_le(q, wa, src);
        ctr = rd_le<8>(q + wa, src);
        q += E;
      }
      if (sh & S_KEY) {
        key = rd_le(q, W.key_bytes, src);
        q += W.key_bytes;
      }
      if (sh & S_V1) q += 4u;
      if (sh & S_DOT2) {
        act2 = rd_le(q, wa, src);
        ctr2 = rd_le<8>(q + wa, src);
        q += E;
      }
      if (sh & S_KEY2) key2 = rd_le(q, W.key2_bytes, src);
      if (sh & S_TKEY) key = rd_le(tp, W.key_bytes, src);
      if (sh & S_TKEY2) key2 = rd_le(tp, W.key2_bytes, src);
      if (sh & S_TVAL) val = rd_le(tp, W.val_bytes, src);
      if ((act >> 32) != 0ull || (act2 >> 32) != 0ull) mybad = true;
      if (sh & S_DUP) {  // the arrays hold one dot per op
        if (act2 != act || ctr2 != ctr) mybad = true;
        act2 = ctr2 = 0ull;
      }
    }
    if (valid && err == CRDT_OK && mybad) err = CRDT_ENONCANON;
    uint32_t kind = F.kind;
    if (err != CRDT_OK) {
      kind = CRDT_OP_KIND_BAD;
      act = ctr = key = act2 = ctr2 = key2 = val = 0ull;
    }
    if (valid) {
      if (T != CRDT_OPS_MVREG) {
        A.kind[i] = kind;
        A.actor[i] = (uint32_t)act;
        A.counter[i] = ctr;
      }
      if (is_map<T>()) A.key[i] = key;
      if (T == CRDT_OPS_ORSWOT || T == CRDT_OPS_MAP_ORSWOT || T == CRDT_OPS_MAP_MAP) A.key2[i] = key2;
      if (T == CRDT_OPS_MAP_MAP) {
        A.actor2[i] = (uint32_t)act2;
        A.counter2[i] = ctr2;
      }
      if (T == CRDT_OPS_MVREG || T == CRDT_OPS_MAP_MVREG || T == CRDT_OPS_MAP_MAP) A.val[i] = val;
      if (op_err) op_err[i] = (uint32_t)err;
      if (err != CRDT_OK) fail(status, err);
    }
    if (T == CRDT_OPS_MVREG) {  // the sentinel pair, after the walk's stores to the same span
      const bool mark = valid && err != CRDT_OK && inside && b < e;
      if (__ballot(mark)) {
        sync<true>();
        if (mark) {
          A.clk_act[b] = 0xffffffffu;
          A.clk_ctr[b] = 0ull;
        }
      }
    }
  }
}

// -------------------------------------------------------------------- egest
// WRITE false: the sizes call; true: the blobs (the same kernel, so the two
// cannot disagree).
template <uint32_t T, bool WRITE>
__global__ __launch_bounds__(kBlock) void to_kernel(crdt_op_widths W, crdt_op_arrays A, uint64_t* sizes, uint8_t* out,
                                                    const uint64_t* ooff, uint64_t out_bytes, uint64_t chunks,
                                                    int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const uint32_t wa = W.actor_bytes;
  const uint64_t E = wa + 8u;
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    const bool valid = i < A.n_ops;
    uint32_t kind = 0, v0 = 0, v1 = 0;
    uint64_t b = 0, e = 0;
    if (valid) {
      e = A.clk_end[i];
      b = i ? A.clk_end[i - 1u] : 0ull;
      if (T != CRDT_OPS_MVREG) kind = A.kind[i];
    }
    const bool inside = b <= e && e <= A.n_clk;
    bool bad = valid && (!inside || !variants_of<T>(kind, v0, v1));
    const uint32_t sh = bad ? 0u : shape<T>(v0, v1);
    const uint64_t n = inside ? e - b : 0ull;
    if (!(sh & S_CLOCK) && n) bad = true;  // pairs under a kind without a clock: the wire cannot say it
    uint64_t act = 0, ctr = 0, key = 0, act2 = 0, ctr2 = 0, key2 = 0, val = 0;
    if (valid && !bad) {
      if (sh & S_DOT) {
        act = A.actor[i];
        ctr = A.counter[i];
      }
      if (sh & (S_KEY | S_TKEY)) key = A.key[i];
      if (sh & (S_KEY2 | S_TKEY2)) key2 = A.key2[i];
      if (sh & S_DUP) {
        act2 = act;
        ctr2 = ctr;
      } else if (T == CRDT_OPS_MAP_MAP && (sh & S_DOT2)) {
        act2 = A.actor2[i];
        ctr2 = A.counter2[i];
      }
      if (sh & S_TVAL) val = A.val[i];
      bad = !fits(act, wa) || !fits(act2, wa) || !fits(key, W.key_bytes) || !fits(key2, W.key2_bytes) ||
            !fits(val, W.val_bytes);
    }
    // the pairs: canonical, actors that fit
    const uint64_t checkm = __ballot(valid && !bad && (sh & S_CLOCK));
    uint64_t badobj = 0;
    for_each_in_ranges(valid, inside, b, e, lane, [&](uint64_t j, bool has, uint32_t t) {
      const bool live = has && ((checkm >> t) & 1u);
      const uint64_t k = j - rd64(b, t);
      uint32_t a = 0;
      uint64_t c = 1;
      if (live) {
        a = A.clk_act[j];
        c = A.clk_ctr[j];
      }
      uint32_t prev = rd32(a, (lane - 1u) & 63u);
      if (live && k && lane == 0u) prev = A.clk_act[j - 1u];
      const bool pb = live && (c == 0ull || !fits(a, wa) || (k && prev >= a));
      badobj |= owners(pb, t);
    });
    bad = bad || ((badobj >> lane) & 1u);
    const uint64_t H = head_bytes(sh, W), Tl = tail_bytes(sh, W);
    const uint64_t size = bad ? 0ull : H + (sh & S_CLOCK ? 8u + n * E : 0ull) + Tl;
    if (valid && bad) fail(status, CRDT_ENONCANON);
    if (!WRITE) {
      if (valid) sizes[i] = size;
      continue;
    }
    const uint64_t at = valid ? ooff[i] : 0ull;
    const bool room = at <= out_bytes && size <= out_bytes - at;
    if (valid && !bad && !room) fail(status, CRDT_ECAPACITY);
    const bool go = valid && !bad && room;
    if (go) {  // head, length word, tail: fixed order, aligned pieces
      uint8_t* q = out + at;
      wr_le<4>(q, v0);
      q += 4u;
      if (sh & S_DOT) {
        wr_le(q, wa, act);
        wr_le<8>(q + wa, ctr);
        q += E;
      }
      if (sh & S_KEY) {
        wr_le(q, W.key_bytes, key);
        q += W.key_bytes;
      }
      if (sh & S_V1) {
        wr_le<4>(q, v1);
        q += 4u;
      }
      if (sh & S_DOT2) {
        wr_le(q, wa, act2);
        wr_le<8>(q + wa, ctr2);
        q += E;
      }
      if (sh & S_KEY2) {
        wr_le(q, W.key2_bytes, key2);
        q += W.key2_bytes;
      }
      if (sh & S_PUT) {
        wr_le<4>(q, 0ull);
        q += 4u;
      }
      if (sh & S_CLOCK) {
        wr_le<8>(q, n);
        q += 8u + n * E;
      }
      if (sh & S_TKEY) wr_le(q, W.key_bytes, key);
      if (sh & S_TKEY2) wr_le(q, W.key2_bytes, key2);
      if (sh & S_TVAL) wr_le(q, W.val_bytes, val);
    }
    const uint64_t gom = __ballot(go && (sh & S_CLOCK));
    const uint64_t ent = at + H + 8u;  // byte of out of the op's first pair
    for_each_in_ranges(valid, inside, b, e, lane, [&](uint64_t j, bool has, uint32_t t) {
      const uint64_t k = j - rd64(b, t);
      uint8_t* q = out + rd64(ent, t) + k * E;
      if (has && ((gom >> t) & 1u)) {
        wr_le(q, wa, A.clk_act[j]);
        wr_le<8>(q + wa, A.clk_ctr[j]);
      }
    });
  }
}

uint32_t wave_blocks(uint64_t chunks) { return resident_blocks((chunks + kBlock / kW - 1) / (kBlock / kW)); }
uint32_t lane_blocks(uint64_t items) { return resident_blocks((items + kBlock - 1) / kBlock); }
int launched() { return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP; }

// CALL with T = op_type as a constant
#define OPS_BINCODE_TYPE(op_type, CALL)                                       \
  switch (op_type) {                                                          \
    case CRDT_OPS_ORSWOT: { constexpr uint32_t T = CRDT_OPS_ORSWOT; CALL; } break;         \
    case CRDT_OPS_MVREG: { constexpr uint32_t T = CRDT_OPS_MVREG; CALL; } break;           \
    case CRDT_OPS_MAP_MVREG: { constexpr uint32_t T = CRDT_OPS_MAP_MVREG; CALL; } break;   \
    case CRDT_OPS_MAP_ORSWOT: { constexpr uint32_t T = CRDT_OPS_MAP_ORSWOT; CALL; } break; \
    default: { constexpr uint32_t T = CRDT_OPS_MAP_MAP; CALL; } break;                     \
  }

}  // namespace

int launch_ops_bincode_clk_lens(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                                uint64_t n_ops, uint32_t op_type, const crdt_op_widths& W, uint32_t* clk_len,
                                int* status, hipStream_t stream) {
  if (n_ops == 0) return CRDT_OK;
  const dim3 grid(lane_blocks(n_ops)), block(kBlock);
  OPS_BINCODE_TYPE(op_type, hipLaunchKernelGGL(lens_kernel<T>, grid, block, 0, stream, blobs, blob_bytes, boff, blen,
                                               n_ops, W, clk_len, status));
  return launched();
}

int launch_ops_from_bincode(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff, const uint64_t* blen,
                            uint32_t op_type, const crdt_op_widths& W, const crdt_op_arrays& A, uint32_t* op_err,
                            int* status, hipStream_t stream) {
  if (A.n_ops == 0) return CRDT_OK;
  const uint64_t chunks = (A.n_ops + kW - 1u) / kW;
  const dim3 grid(wave_blocks(chunks)), block(kBlock);
  OPS_BINCODE_TYPE(op_type, hipLaunchKernelGGL(from_kernel<T>, grid, block, 0, stream, blobs, blob_bytes, boff, blen, W,
                                               A, op_err, chunks, status));
  return launched();
}

int launch_ops_to_bincode(uint32_t op_type, const crdt_op_widths& W, const crdt_op_arrays& A, uint64_t* sizes,
                          uint8_t* out, const uint64_t* ooff, uint64_t out_bytes, int* status, hipStream_t stream) {
  if (A.n_ops == 0) return CRDT_OK;
  const uint64_t chunks = (A.n_ops + kW - 1u) / kW;
  const dim3 grid(wave_blocks(chunks)), block(kBlock);
  if (out) {
    OPS_BINCODE_TYPE(op_type, hipLaunchKernelGGL((to_kernel<T, true>), grid, block, 0, stream, W, A, sizes, out, ooff,
                                                 out_bytes, chunks, status));
  } else {
    OPS_BINCODE_TYPE(op_type, hipLaunchKernelGGL((to_kernel<T, false>), grid, block, 0, stream, W, A, sizes, out, ooff,
                                                 out_bytes, chunks, status));
  }
  return launched();
}

}  // namespace crdts_hip
