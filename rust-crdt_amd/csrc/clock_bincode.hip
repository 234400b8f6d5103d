// bincode codec of VClock / GCounter / PNCounter and of their ops
// (include/crdts_hip.h "bincode of the clocks, the counters and their ops").
//
// Wire format (bincode 0.9 of the serde derives; A = actor_bytes LE):
//   VClock     u64 n | n x (A actor | u64 counter), actors strictly ascending
//              (src/vclock.rs:53-57: a BTreeMap); GCounter is its inner VClock
//              (src/gcounter.rs:26-28), PNCounter is VClock p | VClock n
//              (src/pncounter.rs:33-36).
//   Dot        A actor | u64 counter (src/vclock.rs:33-39); PNCounter's Op is
//              Dot | u32 Dir, Pos = 0, Neg = 1 (src/pncounter.rs:39-56).
// Entry k of a clock sits at 8 + k * (A + 8): no position chain, so the ingest
// kernels walk the entries of 64 objects flat — a wave frames 64 blobs (lane k
// <-> blob k: the length words), scans the entry counts, and then lane j takes
// flat entry j and finds its blob by the 6-step search of for_each_in_ranges
// (csr_rank.h). Clocks of any length take the same loop, 64 entries a step.
//   dense ingest  entries scatter into an LDS tile of R rows (R * slots <=
//                 kTile words per wave); the tile leaves with one flat,
//                 coalesced 8-B-per-lane copy. Rows past the tile go through
//                 it in windows of kTile slots.
//   dense egest   a group of G lanes (G = the power of two >= n_actors, <= 64)
//                 per row: nonzero slots are ranked with ballot + mbcnt and
//                 each lane stores its entry at its rank, so neighbouring
//                 lanes store neighbouring bytes.
//   CSR           the same flat walk from the blobs to act / ctr and back.
//   ops           fixed-size blobs, a lane per op.
// An unaligned field is read as the one or two aligned 8-byte words that hold
// it, where those lie inside d_blobs, else byte by byte; it is stored in the
// largest aligned pieces its address allows. Nothing outside a blob is written.
#include <hip/hip_runtime.h>

#include "../../include/crdts_hip.h"
#include "blob.h"
#include "csr_rank.h"
#include "ctx.h"
#include "kernels.h"
#include "sched.h"

namespace crdts_hip {
namespace {

using namespace blob;
using namespace csr_rank;

constexpr uint32_t kBlock = 256;
constexpr uint32_t kTile = 1024;  // u64 words of LDS per wave (dense ingest)

// (the byte fields — Bounds, rd_le, wr_le, fits — are blob.h's)

// ------------------------------------------------------------------ framing
// The length words of one blob against the bytes it has. n[c] entries of
// clock c start at byte pos[c] of d_blobs. Checked before any multiply: a
// length word above what the bytes left can hold (or above n_max, which no
// strictly ascending clock exceeds) fails.
struct Frame {
  bool ok;
  uint64_t n[2], pos[2];
};

template <uint32_t AB>
__device__ __forceinline__ Frame frame(const uint8_t* blobs, uint64_t blob_bytes, uint64_t off, uint64_t len,
                                       uint32_t nc, uint64_t n_max, const Bounds& src) {
  constexpr uint64_t E = AB + 8u;
  Frame F{};
  F.ok = off <= blob_bytes && len <= blob_bytes - off;
  uint64_t rem = len, pos = off;
#pragma unroll
  for (uint32_t c = 0; c < 2u; ++c) {
    if (c >= nc) break;
    if (!F.ok || rem < 8u) {  // (PNCounter: p ran up to, or past, the blob's end)
      F.ok = false;
      break;
    }
    const uint64_t n = rd_le<8>(blobs + pos, src);
    rem -= 8u;
    pos += 8u;
    if (n > rem / E || n > n_max) {
      F.ok = false;
      break;
    }
    F.n[c] = n;
    F.pos[c] = pos;
    pos += n * E;
    rem -= n * E;
  }
  if (rem) F.ok = false;  // trailing bytes
  if (!F.ok) F.n[0] = F.n[1] = 0;
  return F;
}

// ---------------------------------------------------------------- flat walk
// (flat_walk and owners are csr_rank.h's)
// The entries of one clock of 64 blobs (lane k: n entries from byte pos of
// blobs). Canonical form per entry: counter > 0, actor < limit, actor above
// the entry before it (lane below, or re-read in lane 0: a clock's first
// entry has none). Returns the mask of objects with a bad entry. Every lane
// calls f(t, k, actor, counter, live) (f may read across lanes); `live` says
// the lane holds a good entry.
template <uint32_t AB, class F>
__device__ __forceinline__ uint64_t walk_blobs(const uint8_t* blobs, const Bounds& src, uint64_t n, uint64_t pos,
                                               uint64_t limit, uint32_t lane, F f) {
  constexpr uint64_t E = AB + 8u;
  uint64_t badobj = 0;
  flat_walk(n, lane, [&](uint32_t t, uint64_t k, bool has) {
    const uint8_t* p = blobs + rd64(pos, t) + k * E;
    uint64_t a = 0, c = 1;
    if (has) {
      a = rd_le<AB>(p, src);
      c = rd_le<8>(p + AB, src);
    }
    uint64_t prev = rd64(a, (lane - 1u) & 63u);
    if (has && k && lane == 0u) prev = rd_le<AB>(p - E, src);
    const bool bad = has && (c == 0ull || a >= limit || (k && prev >= a));
    badobj |= owners(bad, t);
    f(t, k, a, c, has && !bad);
  });
  return badobj;
}

// ------------------------------------------------------------- dense ingest
// R (a power of two) objects per wave step, lane k < R <-> object c0 + k.
template <uint32_t AB>
__global__ __launch_bounds__(kBlock) void dense_from_kernel(const uint8_t* blobs, uint64_t blob_bytes,
                                                            const uint64_t* boff, const uint64_t* blen,
                                                            uint64_t n_obj, uint32_t A, uint32_t nc, uint32_t R,
                                                            uint64_t* rows, uint64_t chunks, int* status) {
  __shared__ uint64_t lds[kBlock / kW][kTile];
  uint64_t* tile = lds[threadIdx.x / kW];
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const Bounds src{(uintptr_t)blobs, (uintptr_t)blobs + blob_bytes};
  const uint64_t S = (uint64_t)A * nc;
  const bool windows = S > kTile;              // then R == 1
  const uint64_t rowW = windows ? kTile : S;   // a row's words in the tile
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t c0 = ch * R, i = c0 + lane;
    const bool valid = lane < R && i < n_obj;
    Frame F{};
    if (valid) F = frame<AB>(blobs, blob_bytes, boff[i], blen[i], nc, A, src);
    bool mybad = valid && !F.ok;
    if (windows) {  // all of a row's windows or none: the verdict first
      uint64_t bo = 0;
#pragma unroll
      for (uint32_t c = 0; c < 2u; ++c) {
        if (c >= nc) break;
        bo |= walk_blobs<AB>(blobs, src, F.n[c], F.pos[c], A, lane,
                             [](uint32_t, uint64_t, uint64_t, uint64_t, bool) {});
      }
      if ((bo >> lane) & 1u) {
        mybad = true;
        F.n[0] = F.n[1] = 0;
      }
    }
    const uint64_t live = (n_obj - c0 < R ? n_obj - c0 : R);
    for (uint64_t w0 = 0; w0 < S; w0 += kTile) {
      const uint64_t words = windows ? (S - w0 < kTile ? S - w0 : kTile) : live * S;
      for (uint64_t k = lane; k < words; k += kW) tile[k] = 0ull;
      sync();
      uint64_t bo = 0;
#pragma unroll
      for (uint32_t c = 0; c < 2u; ++c) {
        if (c >= nc) break;
        bo |= walk_blobs<AB>(blobs, src, F.n[c], F.pos[c], A, lane,
                             [&](uint32_t t, uint64_t, uint64_t a, uint64_t v, bool live_entry) {
                               const uint64_t slot = (uint64_t)c * A + a;  // a live entry: a < A
                               if (live_entry && slot - w0 < kTile) tile[t * rowW + (slot - w0)] = v;
                             });
      }
      mybad = mybad || ((bo >> lane) & 1u);
      uint64_t zero = __ballot(mybad);  // a bad object's row is all zero
      if (zero) {
        sync();
        if (lane == 0u) fail(status, CRDT_ENONCANON);
        while (zero) {
          const uint32_t t = (uint32_t)__builtin_ctzll(zero);
          zero &= zero - 1u;
          for (uint64_t k = lane; k < (windows ? words : S); k += kW) tile[t * rowW + k] = 0ull;
        }
      }
      sync();
      uint64_t* dst = rows + c0 * S + w0;
      for (uint64_t k = lane; k < words; k += kW) dst[k] = tile[k];
      sync();  // the tile is free again
    }
  }
}

// -------------------------------------------------------------- dense egest
// G = 1 << lg lanes per row, 64 >> lg rows per wave step. WRITE false: the
// sizes call; true: the blobs (the same walk, so the two cannot disagree).
template <uint32_t AB, bool WRITE>
__global__ __launch_bounds__(kBlock) void dense_to_kernel(const uint64_t* rows, uint64_t n_obj, uint32_t A,
                                                          uint32_t nc, uint32_t lg, uint64_t* sizes, uint8_t* out,
                                                          const uint64_t* ooff, uint64_t out_bytes, uint64_t chunks,
                                                          int* status) {
  constexpr uint64_t E = AB + 8u;
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const uint32_t G = 1u << lg, R = kW >> lg, g = lane >> lg, gl = lane & (G - 1u);
  const uint64_t gmask = (G == kW ? ~0ull : (1ull << G) - 1ull) << (g * G);
  const uint64_t below = (1ull << lane) - 1ull;
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * R + g;
    const bool valid = i < n_obj;
    const uint64_t* row = rows + i * ((uint64_t)A * nc);
    uint64_t cnt[2] = {0, 0}, v0[2] = {0, 0};
    bool bad = false;
#pragma unroll
    for (uint32_t c = 0; c < 2u; ++c) {
      if (c >= nc) break;
      for (uint64_t base = 0; base < A; base += G) {
        const uint64_t s = base + gl;
        const uint64_t v = valid && s < A ? row[(uint64_t)c * A + s] : 0ull;
        if (base == 0) v0[c] = v;
        cnt[c] += (uint32_t)__popcll(__ballot(v != 0ull) & gmask);
        bad = bad || (v != 0ull && !fits<AB>(s));
      }
    }
    const bool gbad = (__ballot(bad) & gmask) != 0ull;
    const uint64_t size = gbad ? 0ull : 8ull * nc + (cnt[0] + cnt[1]) * E;
    if (gbad && gl == 0u) fail(status, CRDT_ENONCANON);
    if (!WRITE) {
      if (valid && gl == 0u) sizes[i] = size;
      continue;
    }
    const uint64_t o = valid ? ooff[i] : 0ull;
    const bool room = o <= out_bytes && size <= out_bytes - o;
    if (valid && !gbad && !room && gl == 0u) fail(status, CRDT_ECAPACITY);
    const bool go = valid && !gbad && room;
    uint8_t* p = out + o;
#pragma unroll
    for (uint32_t c = 0; c < 2u; ++c) {
      if (c >= nc) break;
      if (go && gl == 0u) wr_le<8>(p, cnt[c]);
      p += 8u;
      uint64_t run = 0;
      for (uint64_t base = 0; base < A; base += G) {
        const uint64_t s = base + gl;
        const uint64_t v = base == 0 ? v0[c] : (go && s < A ? row[(uint64_t)c * A + s] : 0ull);
        const bool nz = go && v != 0ull;
        const uint64_t m = __ballot(nz) & gmask;
        if (nz) {
          uint8_t* q = p + (run + (uint32_t)__popcll(m & below)) * E;
          wr_le<AB>(q, s);
          wr_le<8>(q + AB, v);
        }
        run += (uint32_t)__popcll(m);
      }
      p += cnt[c] * E;
    }
  }
}

// ---------------------------------------------------------------------- CSR
struct CsrOut {
  const uint64_t* off;
  uint32_t* len;
  uint32_t* act;
  uint64_t* ctr;
  uint64_t n_entries;
};
struct CsrIn {
  const uint64_t* off;
  const uint32_t* len;
  const uint32_t* act;
  const uint64_t* ctr;
  uint64_t n_entries;
};

// framing only: a lane per blob
template <uint32_t AB>
__global__ __launch_bounds__(kBlock) void csr_lens_kernel(const uint8_t* blobs, uint64_t blob_bytes,
                                                          const uint64_t* boff, const uint64_t* blen, uint64_t n_obj,
                                                          uint32_t nc, uint32_t* len_p, uint32_t* len_n, int* status) {
  const Bounds src{(uintptr_t)blobs, (uintptr_t)blobs + blob_bytes};
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n_obj; i += (uint64_t)gridDim.x * kBlock) {
    const Frame F = frame<AB>(blobs, blob_bytes, boff[i], blen[i], nc, 0xffffffffull, src);
    if (!F.ok) fail(status, CRDT_ENONCANON);
    len_p[i] = (uint32_t)F.n[0];
    if (nc == 2u) len_n[i] = (uint32_t)F.n[1];
  }
}

template <uint32_t AB>
__global__ __launch_bounds__(kBlock) void csr_from_kernel(const uint8_t* blobs, uint64_t blob_bytes,
                                                          const uint64_t* boff, const uint64_t* blen, uint64_t n_obj,
                                                          uint32_t nc, CsrOut P, CsrOut N, uint64_t chunks,
                                                          int* status) {
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  const Bounds src{(uintptr_t)blobs, (uintptr_t)blobs + blob_bytes};
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    const bool valid = i < n_obj;
    Frame F{};
    if (valid) F = frame<AB>(blobs, blob_bytes, boff[i], blen[i], nc, 0xffffffffull, src);
    bool mybad = valid && !F.ok;
    uint64_t o[2] = {0, 0};
    bool room = true;  // the caller's placement holds the runs
#pragma unroll
    for (uint32_t c = 0; c < 2u; ++c) {
      if (c >= nc) break;
      const CsrOut& O = c ? N : P;
      o[c] = valid ? O.off[i] : 0ull;
      room = room && o[c] <= O.n_entries && F.n[c] <= O.n_entries - o[c];
    }
    if (__ballot(valid && !room) && lane == 0u) fail(status, CRDT_ECAPACITY);
    if (!room) F.n[0] = F.n[1] = 0;
    uint64_t bo = 0;
#pragma unroll
    for (uint32_t c = 0; c < 2u; ++c) {
      if (c >= nc) break;
      const CsrOut& O = c ? N : P;
      bo |= walk_blobs<AB>(blobs, src, F.n[c], F.pos[c], 1ull << 32, lane,
                           [&](uint32_t t, uint64_t k, uint64_t a, uint64_t v, bool live) {
                             const uint64_t at = rd64(o[c], t) + k;
                             if (live) {
                               O.act[at] = (uint32_t)a;
                               O.ctr[at] = v;
                             }
                           });
    }
    mybad = mybad || ((bo >> lane) & 1u);
    if (__ballot(mybad) && lane == 0u) fail(status, CRDT_ENONCANON);
    if (valid) {
      P.len[i] = mybad ? 0u : (uint32_t)F.n[0];
      if (nc == 2u) N.len[i] = mybad ? 0u : (uint32_t)F.n[1];
    }
  }
}

// The entries of one run of 64 objects (lane k: n entries from entry o of
// act / ctr, inside the arrays). Every lane calls f(t, k, actor, counter,
// has); returns the mask of objects with a run that is not canonical or holds
// an actor too wide for AB bytes.
template <uint32_t AB, class F>
__device__ __forceinline__ uint64_t walk_runs(const CsrIn& B, uint64_t n, uint64_t o, uint32_t lane, F f) {
  uint64_t badobj = 0;
  flat_walk(n, lane, [&](uint32_t t, uint64_t k, bool has) {
    const uint64_t at = rd64(o, t) + k;
    uint32_t a = 0;
    uint64_t c = 1;
    if (has) {
      a = B.act[at];
      c = B.ctr[at];
    }
    uint32_t prev = rd32(a, (lane - 1u) & 63u);
    if (has && k && lane == 0u) prev = B.act[at - 1u];
    const bool bad = has && (c == 0ull || !fits<AB>(a) || (k && prev >= a));
    badobj |= owners(bad, t);
    f(t, k, a, c, has);
  });
  return badobj;
}

template <uint32_t AB, bool WRITE>
__global__ __launch_bounds__(kBlock) void csr_to_kernel(CsrIn P, CsrIn N, uint64_t n_obj, uint32_t nc,
                                                        uint64_t* sizes, uint8_t* out, const uint64_t* ooff,
                                                        uint64_t out_bytes, uint64_t chunks, int* status) {
  constexpr uint64_t E = AB + 8u;
  const uint32_t lane = threadIdx.x & (kW - 1u);
  const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / kW) + threadIdx.x / kW;
  const uint64_t n_waves = (uint64_t)gridDim.x * (kBlock / kW);
  for (uint64_t ch = wave; ch < chunks; ch += n_waves) {
    const uint64_t i = ch * kW + lane;
    const bool valid = i < n_obj;
    uint64_t o[2] = {0, 0}, n[2] = {0, 0};
    bool placed = true;
#pragma unroll
    for (uint32_t c = 0; c < 2u; ++c) {
      if (c >= nc) break;
      const CsrIn& B = c ? N : P;
      if (valid) {
        o[c] = B.off[i];
        n[c] = B.len[i];
      }
      placed = placed && o[c] <= B.n_entries && n[c] <= B.n_entries - o[c];
    }
    if (!placed) n[0] = n[1] = 0;
    uint64_t bo = 0;
#pragma unroll
    for (uint32_t c = 0; c < 2u; ++c) {
      if (c >= nc) break;
      bo |= walk_runs<AB>(c ? N : P, n[c], o[c], lane, [](uint32_t, uint64_t, uint32_t, uint64_t, bool) {});
    }
    const bool mybad = !placed || ((bo >> lane) & 1u);
    if (__ballot(valid && mybad) && lane == 0u) fail(status, CRDT_ENONCANON);
    const uint64_t size = mybad ? 0ull : 8ull * nc + (n[0] + n[1]) * E;
    if (!WRITE) {
      if (valid) sizes[i] = size;
      continue;
    }
    const uint64_t at = valid ? ooff[i] : 0ull;
    const bool room = at <= out_bytes && size <= out_bytes - at;
    if (__ballot(valid && !mybad && !room) && lane == 0u) fail(status, CRDT_ECAPACITY);
    const bool go = valid && !mybad && room;
    if (!go) n[0] = n[1] = 0;
    uint64_t first = at;  // byte of out where clock c's length word goes
#pragma unroll
    for (uint32_t c = 0; c < 2u; ++c) {
      if (c >= nc) break;
      if (go) wr_le<8>(out + first, n[c]);
      const uint64_t ent = first + 8u;
      (void)walk_runs<AB>(c ? N : P, n[c], o[c], lane, [&](uint32_t t, uint64_t k, uint32_t a, uint64_t v, bool has) {
        uint8_t* q = out + rd64(ent, t) + k * E;
        if (has) {
          wr_le<AB>(q, a);
          wr_le<8>(q + AB, v);
        }
      });
      first = ent + n[c] * E;
    }
  }
}

// ---------------------------------------------------------------------- ops
template <uint32_t AB, bool DIR>
__global__ __launch_bounds__(kBlock) void ops_from_kernel(const uint8_t* blobs, uint64_t stride, uint64_t n,
                                                          uint32_t* actor, uint64_t* counter, uint32_t* dir,
                                                          int* status) {
  constexpr uint64_t size = AB + 8u + (DIR ? 4u : 0u);
  const Bounds src{(uintptr_t)blobs, (uintptr_t)blobs + (n - 1u) * stride + size};
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    const uint8_t* p = blobs + j * stride;
    uint64_t a = rd_le<AB>(p, src), c = rd_le<8>(p + AB, src);
    uint32_t d = DIR ? (uint32_t)rd_le<4>(p + AB + 8u, src) : 0u;  // all four bytes of the variant index
    if (a >> 32 || d > 1u) {  // the sentinel every apply skips and latches
      fail(status, CRDT_ENONCANON);
      a = 0xffffffffull;
      c = 0ull;
      d = 0u;
    }
    actor[j] = (uint32_t)a;
    counter[j] = c;
    if (DIR) dir[j] = d;
  }
}

template <uint32_t AB, bool DIR>
__global__ __launch_bounds__(kBlock) void ops_to_kernel(const uint32_t* actor, const uint64_t* counter,
                                                        const uint32_t* dir, uint64_t n, uint8_t* blobs,
                                                        uint64_t stride, int* status) {
  for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < n; j += (uint64_t)gridDim.x * kBlock) {
    const uint32_t a = actor[j], d = DIR ? dir[j] : 0u;
    if (!fits<AB>(a) || d > 1u) {
      fail(status, CRDT_ENONCANON);  // the blob is not written
      continue;
    }
    uint8_t* p = blobs + j * stride;
    wr_le<AB>(p, a);
    wr_le<8>(p + AB, counter[j]);
    if (DIR) wr_le<4>(p + AB + 8u, d);
  }
}

uint32_t wave_blocks(uint64_t chunks) { return resident_blocks((chunks + kBlock / kW - 1) / (kBlock / kW)); }
uint32_t lane_blocks(uint64_t items) { return resident_blocks((items + kBlock - 1) / kBlock); }
int launched() { return hipGetLastError() == hipSuccess ? CRDT_OK : CRDT_EHIP; }

// CALL with AB = actor_bytes as a constant
#define CLOCK_BINCODE_WIDTH(ab, CALL) \
  switch (ab) {                       \
    case 1u: { constexpr uint32_t AB = 1u; CALL; } break; \
    case 2u: { constexpr uint32_t AB = 2u; CALL; } break; \
    case 4u: { constexpr uint32_t AB = 4u; CALL; } break; \
    default: { constexpr uint32_t AB = 8u; CALL; } break; \
  }

CsrOut csr_out(const crdt_clock_csr_out* o) {
  return o ? CsrOut{o->off, o->len, o->act, o->ctr, o->n_entries} : CsrOut{nullptr, nullptr, nullptr, nullptr, 0};
}
CsrIn csr_in(const crdt_clock_csr* s) {
  return s ? CsrIn{s->off, s->len, s->act, s->ctr, s->n_entries} : CsrIn{nullptr, nullptr, nullptr, nullptr, 0};
}

}  // namespace

int launch_clock_dense_from_bincode(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                    const uint64_t* blen, uint64_t n_obj, uint32_t ab, uint32_t A, uint32_t nc,
                                    uint64_t* rows, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const uint64_t S = (uint64_t)A * nc;
  uint32_t R = kW;  // rows per wave step: the tile holds them
  while (R > 1u && R * S > kTile) R >>= 1;
  const uint64_t chunks = (n_obj + R - 1u) / R;
  const dim3 grid(wave_blocks(chunks)), block(kBlock);
  CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL(dense_from_kernel<AB>, grid, block, 0, stream, blobs, blob_bytes, boff,
                                             blen, n_obj, A, nc, R, rows, chunks, status));
  return launched();
}

int launch_clock_dense_to_bincode(const uint64_t* rows, uint64_t n_obj, uint32_t A, uint32_t nc, uint32_t ab,
                                  uint64_t* sizes, uint8_t* out, const uint64_t* ooff, uint64_t out_bytes,
                                  int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  uint32_t lg = 0;  // lanes per row: the power of two >= A, at most a wave
  while (lg < 6u && (1u << lg) < A) ++lg;
  const uint64_t R = kW >> lg, chunks = (n_obj + R - 1u) / R;
  const dim3 grid(wave_blocks(chunks)), block(kBlock);
  if (out) {
    CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL((dense_to_kernel<AB, true>), grid, block, 0, stream, rows, n_obj, A, nc,
                                               lg, sizes, out, ooff, out_bytes, chunks, status));
  } else {
    CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL((dense_to_kernel<AB, false>), grid, block, 0, stream, rows, n_obj, A,
                                               nc, lg, sizes, out, ooff, out_bytes, chunks, status));
  }
  return launched();
}

int launch_clock_csr_bincode_lens(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                  const uint64_t* blen, uint64_t n_obj, uint32_t ab, uint32_t nc, uint32_t* len_p,
                                  uint32_t* len_n, int* status, hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const dim3 grid(lane_blocks(n_obj)), block(kBlock);
  CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL(csr_lens_kernel<AB>, grid, block, 0, stream, blobs, blob_bytes, boff,
                                             blen, n_obj, nc, len_p, len_n, status));
  return launched();
}

int launch_clock_csr_from_bincode(const uint8_t* blobs, uint64_t blob_bytes, const uint64_t* boff,
                                  const uint64_t* blen, uint64_t n_obj, uint32_t ab, uint32_t nc,
                                  const crdt_clock_csr_out* out_p, const crdt_clock_csr_out* out_n, int* status,
                                  hipStream_t stream) {
  if (n_obj == 0) return CRDT_OK;
  const uint64_t chunks = (n_obj + kW - 1u) / kW;
  const dim3 grid(wave_blocks(chunks)), block(kBlock);
  const CsrOut P = csr_out(out_p), N = csr_out(out_n);
  CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL(csr_from_kernel<AB>, grid, block, 0, stream, blobs, blob_bytes, boff,
                                             blen, n_obj, nc, P, N, chunks, status));
  return launched();
}

int launch_clock_csr_to_bincode(const crdt_clock_csr* self_p, const crdt_clock_csr* self_n, uint32_t ab,
                                uint64_t* sizes, uint8_t* out, const uint64_t* ooff, uint64_t out_bytes, int* status,
                                hipStream_t stream) {
  const uint64_t n_obj = self_p->n_obj;
  if (n_obj == 0) return CRDT_OK;
  const uint32_t nc = self_n ? 2u : 1u;
  const uint64_t chunks = (n_obj + kW - 1u) / kW;
  const dim3 grid(wave_blocks(chunks)), block(kBlock);
  const CsrIn P = csr_in(self_p), N = csr_in(self_n);
  if (out) {
    CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL((csr_to_kernel<AB, true>), grid, block, 0, stream, P, N, n_obj, nc,
                                               sizes, out, ooff, out_bytes, chunks, status));
  } else {
    CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL((csr_to_kernel<AB, false>), grid, block, 0, stream, P, N, n_obj, nc,
                                               sizes, out, ooff, out_bytes, chunks, status));
  }
  return launched();
}

int launch_clock_ops_from_bincode(const uint8_t* blobs, uint64_t stride, uint64_t n_ops, uint32_t ab, bool with_dir,
                                  uint32_t* actor, uint64_t* counter, uint32_t* dir, int* status,
                                  hipStream_t stream) {
  if (n_ops == 0) return CRDT_OK;
  const dim3 grid(lane_blocks(n_ops)), block(kBlock);
  if (with_dir) {
    CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL((ops_from_kernel<AB, true>), grid, block, 0, stream, blobs, stride,
                                               n_ops, actor, counter, dir, status));
  } else {
    CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL((ops_from_kernel<AB, false>), grid, block, 0, stream, blobs, stride,
                                               n_ops, actor, counter, dir, status));
  }
  return launched();
}

int launch_clock_ops_to_bincode(const uint32_t* actor, const uint64_t* counter, const uint32_t* dir, uint64_t n_ops,
                                uint32_t ab, bool with_dir, uint8_t* blobs, uint64_t stride, int* status,
                                hipStream_t stream) {
  if (n_ops == 0) return CRDT_OK;
  const dim3 grid(lane_blocks(n_ops)), block(kBlock);
  if (with_dir) {
    CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL((ops_to_kernel<AB, true>), grid, block, 0, stream, actor, counter, dir,
                                               n_ops, blobs, stride, status));
  } else {
    CLOCK_BINCODE_WIDTH(ab, hipLaunchKernelGGL((ops_to_kernel<AB, false>), grid, block, 0, stream, actor, counter, dir,
                                               n_ops, blobs, stride, status));
  }
  return launched();
}

}  // namespace crdts_hip

// ------------------------------------------------------------------- the ABI
using namespace crdts_hip;

namespace {
inline hipStream_t S(void* s) { return (hipStream_t)s; }
int set_device(crdt_ctx* ctx) { return hipSetDevice(ctx->device) == hipSuccess ? CRDT_OK : CRDT_EHIP; }
bool width_ok(uint32_t w) { return w == 1u || w == 2u || w == 4u || w == 8u; }
bool clocks_ok(uint32_t n_clocks) { return n_clocks == 1u || n_clocks == 2u; }
bool same(const void* a, const void* b) { return a && a == b; }
bool out_ok(const crdt_clock_csr_out* o) { return o && o->off && o->len && (o->n_entries == 0 || (o->act && o->ctr)); }
bool in_ok(const crdt_clock_csr* s) { return s->off && s->len && (s->n_entries == 0 || (s->act && s->ctr)); }
bool in_aliases(const crdt_clock_csr* s, const void* p) {
  return same(s->off, p) || same(s->len, p) || same(s->act, p) || same(s->ctr, p);
}
}  // namespace

extern "C" {

int crdt_clock_dense_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                                  const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t n_actors,
                                  uint32_t n_clocks, uint64_t* d_rows, void* stream) {
  if (!ctx || !width_ok(actor_bytes) || n_actors == 0 || !clocks_ok(n_clocks)) return CRDT_EINVAL;
  if (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !d_rows)) return CRDT_EINVAL;
  if (n_obj && (same(d_rows, d_blobs) || same(d_rows, d_blob_off) || same(d_rows, d_blob_len))) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_dense_from_bincode(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, n_actors,
                                         n_clocks, d_rows, ctx->d_status, S(stream));
}

int crdt_clock_dense_bincode_sizes(crdt_ctx* ctx, const uint64_t* d_rows, size_t n_obj, uint32_t n_actors,
                                   uint32_t n_clocks, uint32_t actor_bytes, uint64_t* d_sizes, void* stream) {
  if (!ctx || !width_ok(actor_bytes) || n_actors == 0 || !clocks_ok(n_clocks)) return CRDT_EINVAL;
  if (n_obj && (!d_rows || !d_sizes || d_rows == d_sizes)) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_dense_to_bincode(d_rows, n_obj, n_actors, n_clocks, actor_bytes, d_sizes, nullptr, nullptr, 0,
                                       ctx->d_status, S(stream));
}

int crdt_clock_dense_to_bincode(crdt_ctx* ctx, const uint64_t* d_rows, size_t n_obj, uint32_t n_actors,
                                uint32_t n_clocks, uint32_t actor_bytes, uint8_t* d_out, const uint64_t* d_out_off,
                                size_t out_bytes, void* stream) {
  if (!ctx || !width_ok(actor_bytes) || n_actors == 0 || !clocks_ok(n_clocks)) return CRDT_EINVAL;
  if (n_obj && (!d_rows || !d_out || !d_out_off)) return CRDT_EINVAL;
  if (n_obj && (same(d_out, d_rows) || same(d_out, d_out_off))) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_dense_to_bincode(d_rows, n_obj, n_actors, n_clocks, actor_bytes, nullptr, d_out, d_out_off,
                                       out_bytes, ctx->d_status, S(stream));
}

int crdt_clock_csr_bincode_lens(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                                const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t n_clocks,
                                uint32_t* d_len_p, uint32_t* d_len_n, void* stream) {
  if (!ctx || !width_ok(actor_bytes) || !clocks_ok(n_clocks)) return CRDT_EINVAL;
  if (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !d_len_p || (n_clocks == 2u && !d_len_n))) return CRDT_EINVAL;
  if (n_obj)
    for (const void* w : {(const void*)d_len_p, (const void*)(n_clocks == 2u ? d_len_n : nullptr)})
      if (same(w, d_blobs) || same(w, d_blob_off) || same(w, d_blob_len)) return CRDT_EINVAL;
  if (n_obj && n_clocks == 2u && d_len_p == d_len_n) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_csr_bincode_lens(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, n_clocks,
                                       d_len_p, d_len_n, ctx->d_status, S(stream));
}

int crdt_clock_csr_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t blob_bytes, const uint64_t* d_blob_off,
                                const uint64_t* d_blob_len, size_t n_obj, uint32_t actor_bytes, uint32_t n_clocks,
                                const crdt_clock_csr_out* out_p, const crdt_clock_csr_out* out_n, void* stream) {
  if (!ctx || !width_ok(actor_bytes) || !clocks_ok(n_clocks)) return CRDT_EINVAL;
  if (n_obj && (!d_blobs || !d_blob_off || !d_blob_len || !out_ok(out_p) || (n_clocks == 2u && !out_ok(out_n))))
    return CRDT_EINVAL;
  if (n_obj) {  // out.off is an input here
    const bool two = n_clocks == 2u;
    const void* ins[] = {d_blobs, d_blob_off, d_blob_len, out_p->off, two ? out_n->off : nullptr};
    const void* outs[] = {out_p->len, out_p->act, out_p->ctr, two ? out_n->len : nullptr,
                          two ? out_n->act : nullptr, two ? out_n->ctr : nullptr};
    for (const void* w : outs)
      for (const void* r : ins)
        if (same(w, r)) return CRDT_EINVAL;
    for (int k = 0; two && k < 3; ++k)
      if (same(outs[k], outs[k + 3])) return CRDT_EINVAL;
  }
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_csr_from_bincode(d_blobs, blob_bytes, d_blob_off, d_blob_len, n_obj, actor_bytes, n_clocks,
                                       out_p, n_clocks == 2u ? out_n : nullptr, ctx->d_status, S(stream));
}

int crdt_clock_csr_bincode_sizes(crdt_ctx* ctx, const crdt_clock_csr* self_p, const crdt_clock_csr* self_n,
                                 uint32_t actor_bytes, uint64_t* d_sizes, void* stream) {
  if (!ctx || !self_p || !width_ok(actor_bytes)) return CRDT_EINVAL;
  if (self_n && self_n->n_obj != self_p->n_obj) return CRDT_EINVAL;
  const size_t n_obj = self_p->n_obj;
  if (n_obj && (!d_sizes || !in_ok(self_p) || (self_n && !in_ok(self_n)))) return CRDT_EINVAL;
  if (n_obj && (in_aliases(self_p, d_sizes) || (self_n && in_aliases(self_n, d_sizes)))) return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_csr_to_bincode(self_p, self_n, actor_bytes, d_sizes, nullptr, nullptr, 0, ctx->d_status,
                                     S(stream));
}

int crdt_clock_csr_to_bincode(crdt_ctx* ctx, const crdt_clock_csr* self_p, const crdt_clock_csr* self_n,
                              uint32_t actor_bytes, uint8_t* d_out, const uint64_t* d_out_off, size_t out_bytes,
                              void* stream) {
  if (!ctx || !self_p || !width_ok(actor_bytes)) return CRDT_EINVAL;
  if (self_n && self_n->n_obj != self_p->n_obj) return CRDT_EINVAL;
  const size_t n_obj = self_p->n_obj;
  if (n_obj && (!d_out || !d_out_off || !in_ok(self_p) || (self_n && !in_ok(self_n)))) return CRDT_EINVAL;
  if (n_obj && (in_aliases(self_p, d_out) || (self_n && in_aliases(self_n, d_out)) || same(d_out, d_out_off)))
    return CRDT_EINVAL;
  if (n_obj == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_csr_to_bincode(self_p, self_n, actor_bytes, nullptr, d_out, d_out_off, out_bytes,
                                     ctx->d_status, S(stream));
}

int crdt_clock_ops_from_bincode(crdt_ctx* ctx, const uint8_t* d_blobs, size_t stride, size_t n_ops,
                                uint32_t actor_bytes, uint32_t with_dir, uint32_t* d_actor, uint64_t* d_counter,
                                uint32_t* d_dir, void* stream) {
  if (!ctx || !width_ok(actor_bytes)) return CRDT_EINVAL;
  if (stride < (size_t)actor_bytes + 8u + (with_dir ? 4u : 0u)) return CRDT_EINVAL;
  if (n_ops && (!d_blobs || !d_actor || !d_counter || (with_dir && !d_dir))) return CRDT_EINVAL;
  if (n_ops && (same(d_actor, d_blobs) || same(d_counter, d_blobs) || (with_dir && same(d_dir, d_blobs)) ||
                same(d_actor, d_counter) || (with_dir && (d_dir == d_actor || same(d_dir, d_counter)))))
    return CRDT_EINVAL;
  if (n_ops == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_ops_from_bincode(d_blobs, stride, n_ops, actor_bytes, with_dir != 0, d_actor, d_counter, d_dir,
                                       ctx->d_status, S(stream));
}

int crdt_clock_ops_to_bincode(crdt_ctx* ctx, const uint32_t* d_actor, const uint64_t* d_counter,
                              const uint32_t* d_dir, size_t n_ops, uint32_t actor_bytes, uint32_t with_dir,
                              uint8_t* d_blobs, size_t stride, void* stream) {
  if (!ctx || !width_ok(actor_bytes)) return CRDT_EINVAL;
  if (stride < (size_t)actor_bytes + 8u + (with_dir ? 4u : 0u)) return CRDT_EINVAL;
  if (n_ops && (!d_blobs || !d_actor || !d_counter || (with_dir && !d_dir))) return CRDT_EINVAL;
  if (n_ops && (same(d_blobs, d_actor) || same(d_blobs, d_counter) || (with_dir && same(d_blobs, d_dir))))
    return CRDT_EINVAL;
  if (n_ops == 0) return CRDT_OK;
  int rc = set_device(ctx);
  if (rc) return rc;
  return launch_clock_ops_to_bincode(d_actor, d_counter, d_dir, n_ops, actor_bytes, with_dir != 0, d_blobs, stride,
                                     ctx->d_status, S(stream));
}

}  // extern "C"
