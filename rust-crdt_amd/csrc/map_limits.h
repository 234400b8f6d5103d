// The capacity limits of the three Map slab types (internal), named once: the
// C ABI checks them (api.hip) and the kernels size their static LDS arrays by
// them (map.hip, map_map.hip, map_truncate.hip, map_bincode.hip).
//
// A "side" limit holds for an input of a merge, for self of apply and
// truncate and for the slab a bincode ingest fills. An output (out of apply
// and truncate, a slab a bincode egest reads) may be kMapOutFactor times as
// large: the sums a merge of two sides can need.
#pragma once
#include <cstdint>

namespace crdts_hip {

constexpr uint32_t kMapActorsMax = 128;  // n_actors: two slots per lane (map_rows.h)
constexpr uint32_t kMapOutFactor = 2;

// crdt_map_mvreg_slab (also the nested map's inner slab)
constexpr uint32_t kMapMvregKcap = 4096, kMapMvregMcap = 128, kMapMvregDcap = 64, kMapMvregScap = 4096;
// crdt_map_orswot_slab
constexpr uint32_t kMapOrswotKcap = 4096, kMapOrswotMcap = 256, kMapOrswotVdcap = 256, kMapOrswotVscap = 256,
                   kMapOrswotDcap = 256, kMapOrswotScap = 4096;
// crdt_map_map_slab, the outer arrays
constexpr uint32_t kMapMapKcap = 4096, kMapMapDcap = 64, kMapMapScap = 4096;

}  // namespace crdts_hip
