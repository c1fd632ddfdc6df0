// unmarshal_internal.h -- internal: what the device unmarshal of Fileset JSON
// (unmarshal_dev.cpp) shares with its kernels (k12_unmarshal.hip).  Not part of
// the public ABI.
#pragma once
#include "ctx.h"
#include "engine.h"

namespace rf {

constexpr uint32_t kUnBlock = 256;
constexpr uint32_t kUnPer = 16;  // consecutive arena bytes per lane: one 16-byte load
static_assert(RF_UNMARSHAL_TILE == kUnBlock * kUnPer, "a tile is whole lanes");
constexpr uint32_t kUnDisagree = 0x80000000u;  // reason word: the per-byte form refused what the sequential form accepts

// A batch of documents in an arena and the passes' scratch.  "chunk" = the 16
// bytes of one lane; per-chunk words hold a value before the chunk within its
// tile, per-tile words the tile's sum and, after launch_tile_scan, the sum
// before the tile.  Sums are taken mod 2^32 over the whole arena and only ever
// used as differences against the same sum at a document's first byte, so
// every pass is segmented by document without a segmented scan.
struct UnDev {
    const uint8_t* arena = nullptr;
    uint32_t arena_bytes = 0, n = 0, tiles = 0;
    const uint64_t* offs = nullptr;  // [n] the caller's
    const int64_t* lens = nullptr;   // [n]
    uint32_t *ds = nullptr, *de = nullptr;  // [n] document d = arena[ds, de)
    uint32_t* ctl = nullptr;  // [0]: the layout is bad (every later kernel returns at once); [1]: the scatter met a
                              // node or entry its counts did not announce (nothing is written there; RF_EDEVICE)
    uint16_t *qm = nullptr, *pm = nullptr;  // [chunks] quote bits; parity of the quote bits before each byte
    uint16_t *lq = nullptr, *ld = nullptr, *ln = nullptr, *le = nullptr;  // [chunks] quotes, depth, nodes, entries: at most a tile's bytes
    uint32_t* lp = nullptr;  // [chunks] decoded path bytes: not bounded by the tile, a path may have begun tiles earlier
    uint32_t *tq = nullptr, *td = nullptr, *tn = nullptr, *te = nullptr, *tp = nullptr;  // [tiles]
    uint32_t* bad = nullptr;                                             // [n] refused (every writer stores 1)
    uint32_t *sd = nullptr, *sn = nullptr, *se = nullptr, *sp = nullptr;  // [n] in-chunk sums before the first byte
    uint32_t *en = nullptr, *ee = nullptr, *ep = nullptr;                 // [n] in-chunk sums after the last byte
    uint32_t *bn = nullptr, *be = nullptr, *bp = nullptr;  // [n] counts masked by bad; after the scans, the dense bases
    uint32_t *counts = nullptr, *node_cnt = nullptr;       // [n] the masked entry and node counts, kept
    uint32_t* reason = nullptr;                            // [n]
    uint64_t* totals = nullptr;                            // {nodes, entries, path bytes}
    // the scatter's outputs and their sizes
    uint64_t n_nodes = 0, n_entries = 0, path_bytes = 0;
    uint32_t* node_depth = nullptr;
    uint64_t *entry_ptr = nullptr, *path_off = nullptr;
    uint8_t *paths = nullptr, *ids32 = nullptr;
    int64_t* sizes = nullptr;
};

// layout check (ctl, ds, de, bad for empty documents), quote bits, their scan,
// token checks and counts, their scans, depth checks, masked per-document
// counts and their scans, the refused documents' reasons
hipError_t launch_unmarshal_check(const UnDev& u, hipStream_t s);
// nodes, entries, paths, IDs and sizes of the accepted documents, dense
hipError_t launch_unmarshal_scatter(const UnDev& u, hipStream_t s);

// unmarshal_dev.cpp: the structure a device-form forest keeps in HBM (valid
// until rf_fileset_forest_free), for the physical keys (physkeys_dev.cpp).
// False for a host-form forest.
struct ForestArraysDev {
    rf_ctx* ctx = nullptr;
    const uint32_t* node_depth = nullptr;
    const uint64_t *entry_ptr = nullptr, *path_off = nullptr;
    const uint8_t *paths = nullptr, *ids32 = nullptr;
};
bool forest_dev_arrays(const rf_fileset_forest* f, ForestArraysDev* out);

}  // namespace rf
