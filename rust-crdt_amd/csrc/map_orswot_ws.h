// A nested Orswot<u64, A> staged in LDS, one wave, lane = actor slot
// (internal; shared by the Map<u64, Orswot> merge and apply kernels,
// map_orswot.hip and map_orswot_apply.hip): the workspace, the nested
// apply_deferred (src/orswot.rs:235-243) and Orswot::truncate
// (src/orswot.rs:159-172), both keeping the deferred clocks in CLOCK ORDER.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "map_rows.h"
#include "map_wave.h"

namespace crdts_hip {
namespace mows {

using namespace maprow;  // Row<NS> and the VClock ops on it (map_rows.h); the wave toolkit (map_wave.h)

// A nested Orswot under construction (LDS). The top clock is a register
// (lane = actor) held by the caller.
struct Ws {
  uint64_t* key;   // [MW] members, ascending
  uint64_t* row;   // [MW][A] member clocks
  uint64_t* dclk;  // [DW][A] deferred clocks, CLOCK ORDER
  uint32_t* dn;    // [DW] set sizes
  uint64_t* dset;  // [DW][sw] member sets, ascending
  uint32_t nm, nd, sw;
};
struct Caps {
  uint32_t MW, DW, SW, A;
};

// Orswot::apply_deferred (src/orswot.rs:235-243) on W under top clock `clk`,
// after the members flagged in mdead are dropped: every deferred clock is
// subtracted from the members of its set (a member left empty is dropped),
// and kept only if `clk` does not cover it. Then both lists are compacted.
template <int NS>
__device__ void ws_apply_deferred(Ws& W, Row<NS> clk, uint32_t* mdead, uint32_t* ddead, const Caps& c,
                                  uint32_t lane) {
  for (uint32_t d = 0; d < W.nd; ++d) {
    const Row<NS> D = ldrow<NS>(W.dclk + d * c.A, c.A, lane);
    const uint32_t n = uni32(W.dn[d]);
    for (uint32_t j = 0; j < n; ++j) {
      const uint64_t m = uni64(W.dset[d * W.sw + j]);
      uint32_t lo = 0, hi = W.nm;  // binary search over the (sorted) members
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (uni64(W.key[mid]) < m) lo = mid + 1u;
        else hi = mid;
      }
      if (lo >= W.nm || uni64(W.key[lo]) != m || uni32(mdead[lo])) continue;
      const Row<NS> r = vsub(ldrow<NS>(W.row + lo * c.A, c.A, lane), D);
      strow(W.row + lo * c.A, r, c.A, lane);
      const bool gone = !vany(r);
      sync();
      if (gone && lane == 0u) mdead[lo] = 1u;
      sync();
    }
    const bool drop = vle(D, clk);
    if (lane == 0u) ddead[d] = drop ? 1u : 0u;
  }
  sync();
  // compaction, in place (destination <= source)
  uint32_t k = 0;
  for (uint32_t j = 0; j < W.nm; ++j) {
    if (uni32(mdead[j])) continue;
    if (k != j) {
      const uint64_t key = W.key[j];
      const Row<NS> r = ldrow<NS>(W.row + j * c.A, c.A, lane);
      sync();
      if (lane == 0u) W.key[k] = key;
      strow(W.row + k * c.A, r, c.A, lane);
      sync();
    }
    ++k;
  }
  W.nm = k;
  k = 0;
  for (uint32_t d = 0; d < W.nd; ++d) {
    if (uni32(ddead[d])) continue;
    if (k != d) {
      const Row<NS> D = ldrow<NS>(W.dclk + d * c.A, c.A, lane);
      const uint32_t n = uni32(W.dn[d]);
      sync();
      strow(W.dclk + k * c.A, D, c.A, lane);
      if (lane == 0u) W.dn[k] = n;
      for (uint32_t j = lane; j < n; j += kW) W.dset[k * W.sw + j] = W.dset[d * W.sw + j];  // (rows k < d)
      sync();
    }
    ++k;
  }
  W.nd = k;
  for (uint32_t j = lane; j < c.MW; j += kW) mdead[j] = 0u;
  for (uint32_t j = lane; j < c.DW; j += kW) ddead[j] = 0u;
  sync();
}

// Orswot::truncate (src/orswot.rs:159-172) of W (top clock `clk`) by `t`.
template <int NS>
__device__ void ws_truncate(Ws& W, Row<NS>& clk, Row<NS> t, uint32_t* mdead, uint32_t* ddead, const Caps& c,
                            uint32_t lane) {
  // merge with an empty set whose clock is t: members t covers are dropped
  // (:94-104); it has no entries or deferred removes; the clocks merge
  for (uint32_t j = 0; j < W.nm; ++j) {
    const bool covered = vle(ldrow<NS>(W.row + j * c.A, c.A, lane), t);
    if (covered && lane == 0u) mdead[j] = 1u;
  }
  clk = vmax(clk, t);
  sync();
  ws_apply_deferred(W, clk, mdead, ddead, c, lane);
  // forget t from the top clock and every member clock (an emptied member stays)
  clk = vsub(clk, t);
  for (uint32_t j = 0; j < W.nm; ++j) strow(W.row + j * c.A, vsub(ldrow<NS>(W.row + j * c.A, c.A, lane), t), c.A, lane);
  sync();
}

}  // namespace mows
}  // namespace crdts_hip
