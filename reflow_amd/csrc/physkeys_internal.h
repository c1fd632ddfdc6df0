// physkeys_internal.h -- internal: what the physical keys' device side
// (physkeys_dev.cpp) shares with its kernels (k13_physkeys.hip).  Not part of
// the public ABI.
#pragma once
#include "ctx.h"
#include "phys_emit.h"

namespace rf {

constexpr uint32_t kPhysBlock = 256;
constexpr uint32_t kPhysPer = RF_PHYS_LIST_TILE / kPhysBlock;  // consecutive items per lane of a scan tile
static_assert(RF_PHYS_LIST_TILE == kPhysBlock * kPhysPer, "a tile is whole lanes");
static_assert(RF_PHYS_COPY_TILE == kPhysBlock * 16, "a lane of the gather stores 16 bytes");

inline uint64_t phys_tiles(uint64_t n) { return (n + RF_PHYS_LIST_TILE - 1) / RF_PHYS_LIST_TILE; }

// Exclusive scan of vals[0 .. n) in place, the total to *total (device memory;
// may be vals + n): tile-local scan / scan of the tile sums / apply.
// tile_tmp: [phys_tiles(n)].
hipError_t launch_phys_scan(uint64_t* vals, uint64_t n, uint64_t* tile_tmp, uint64_t* total, hipStream_t s);

// ---- set values: a forest's documents into the store's arena ----------------
struct PhysSetDev {
    PhysVals v;                    // device pointers
    uint64_t* node_pre = nullptr;  // [n_nodes + 1] material bytes before the node; [n_nodes] the total
    uint64_t* doc_len = nullptr;   // [n_docs] unpadded material bytes (0 for a skipped document)
    uint64_t* doc_off = nullptr;   // [n_docs + 1] padded bytes before the document; [n_docs] the total
    uint64_t* tile_tmp = nullptr;  // [phys_tiles(max(n_nodes, n_docs))]
};
// node lengths and their scan, the documents' lengths, their 16-byte padded scan
hipError_t launch_phys_lengths(const PhysSetDev& d, hipStream_t s);
// entries to arena + base + doc_off; then node g of document d: val_off, val_len, has
hipError_t launch_phys_emit(const PhysSetDev& d, uint8_t* arena, uint64_t base, uint64_t* val_off, uint64_t* val_len,
                            uint8_t* has, hipStream_t s);
hipError_t launch_phys_clear(const uint32_t* nodes, uint64_t n, uint8_t* has, hipStream_t s);

// ---- update -----------------------------------------------------------------
struct PhysUpdDev {
    uint64_t n = 0;  // graph nodes
    const uint64_t *dep_ptr = nullptr, *cons_ptr = nullptr, *phys_row = nullptr, *suffix_ptr = nullptr;
    const uint32_t *deps = nullptr, *cons = nullptr;
    const uint64_t *val_off = nullptr, *val_len = nullptr;
    const uint8_t* has = nullptr;
    const uint32_t* listed = nullptr;  // [n_listed] (n_listed >= 1)
    uint64_t* list_off = nullptr;      // [n_listed + 1] consumer entries of listed[i], then before it; the last: the total
    uint64_t* list_tmp = nullptr;      // [phys_tiles(n_listed)]
    uint64_t n_listed = 0, n_rows = 0;
    uint32_t flags = 0;
    uint8_t* mark = nullptr;       // [n]
    uint64_t* tile_cnt = nullptr;  // [phys_tiles(n) + 1] affected per tile, then before the tile; the last: the total
    uint32_t* aff = nullptr;       // [affected] ascending
    // per affected node k (sized for n_aff + 1: the scans' totals)
    uint64_t n_aff = 0;
    uint8_t* comp = nullptr;       // computable
    uint64_t* mlen = nullptr;      // material bytes (0 when not computable)
    uint64_t* moff = nullptr;      // padded bytes, then the material's offset in the gather arena
    uint64_t* seg_ptr = nullptr;   // segments (deps + 1, 0 when not computable), then the first segment
    uint64_t* crank = nullptr;     // computable, then computable nodes before k
    uint64_t* tile_tmp = nullptr;  // [phys_tiles(n_aff)]
    uint32_t* ctl = nullptr;       // [0]: a phys_row >= n_rows
    uint64_t *seg_dst = nullptr, *seg_src = nullptr, *seg_len = nullptr;
};
// mark, per-tile counts, their scan
hipError_t launch_phys_affected(const PhysUpdDev& u, hipStream_t s);
// the affected list; comp, mlen and the three scans; ctl
hipError_t launch_phys_measure(const PhysUpdDev& u, hipStream_t s);
hipError_t launch_phys_segments(const PhysUpdDev& u, hipStream_t s);
hipError_t launch_phys_gather(const PhysUpdDev& u, uint64_t n_segs, const uint8_t* arena, const uint8_t* suffix,
                              uint8_t* out, uint64_t out_bytes, hipStream_t s);
// digests (row crank[k] of dig) and zero rows to d_keys32[phys_row]
hipError_t launch_phys_scatter(const PhysUpdDev& u, const uint8_t* dig, uint8_t* keys32, hipStream_t s);

}  // namespace rf
