// cwrite_internal.h -- internal: what the device marshal (marshal_dev.cpp) and
// the cache write (cache_write.cpp) share with their kernels (k11_cwrite.hip),
// and the locked entry points of the objects a cache write goes through.  Not
// part of the public ABI.
#pragma once
#include "ctx.h"
#include "engine.h"

namespace rf {

constexpr uint32_t kMarshalBlock = 256;
constexpr uint32_t kMarshalPer = RF_MARSHAL_TILE / kMarshalBlock;  // consecutive pieces (rows) per lane
static_assert(RF_MARSHAL_TILE == kMarshalBlock * kMarshalPer, "a tile is whole lanes");

// A piece stream (marshal_flat.h) and the entries it names, in device memory.
struct MarshalDev {
    uint32_t n_pieces = 0, n_values = 0;
    const uint32_t* pa = nullptr;         // [n_pieces] entry index, or a literal's blob offset
    const uint32_t* pb = nullptr;         // [n_pieces] kPieceEntry | comma, or a literal's length
    const uint32_t* pv = nullptr;         // [n_pieces] the piece's value
    const uint32_t* value_ptr = nullptr;  // [n_values + 1]
    const uint8_t* blob = nullptr;        // the literals
    const uint8_t* paths = nullptr;       // every entry's path bytes, concatenated
    const uint64_t* path_off = nullptr;   // [entries + 1] entry e's path is [path_off[e], path_off[e + 1])
    const int64_t* sizes = nullptr;       // [entries]
    const uint8_t* ids32 = nullptr;       // [entries][32]
    uint32_t* local = nullptr;            // [n_pieces] bytes before the piece within its tile
    uint32_t* tile_count = nullptr;       // [tiles] bytes per tile; after the scan, bytes before the tile
    uint64_t* ustart = nullptr;           // [n_values + 1] bytes before the value, unpadded; [n_values] = the total
    uint32_t* zero_seen = nullptr;        // one word: an entry piece names a zero ID
};
// length pass: local, tile_count, zero_seen; then the tile scan and ustart
hipError_t launch_marshal_len(const MarshalDev& m, hipStream_t s);
// emit pass: value v's bytes at arena + offs[v]
hipError_t launch_marshal_emit(const MarshalDev& m, const uint64_t* offs, uint8_t* arena, hipStream_t s);

// The key gather of a cache write, over the listed nodes.
enum : uint32_t { kCwWritten = 0, kCwNotCacheable = 1, kCwExtern = 2, kCwNoKey = 3 };
enum : uint32_t { kCwBad = 0, kCwSkip = 1 /* [3] by reason - 1 */, kCwWords = 8 };
struct CwDev {
    uint32_t n = 0;
    const uint32_t* nodes = nullptr;      // [n] the listed nodes
    const uint8_t* flags = nullptr;       // the wave object's node flags, states and key rows
    const uint8_t* state = nullptr;
    const uint64_t* key_ptr = nullptr;
    const uint32_t* key_slots = nullptr;
    const uint8_t* keys = nullptr;        // rows in key_ptr order, or (by_slot) the graph's slot table
    bool by_slot = false;
    int no_cache_extern = 0;
    const uint8_t* fsids = nullptr;       // [n][32]
    const int64_t* sizes = nullptr;       // [n]
    uint8_t* nput = nullptr;              // [n] keys put for row i
    uint8_t* reason = nullptr;            // [n] kCw*
    uint32_t* tile_keys = nullptr;        // [tiles] keys put per tile; after the scan, before the tile
    uint32_t* tile_nodes = nullptr;       // [tiles] participating rows, likewise
    uint64_t* totals = nullptr;           // {keys put, rows written}
    uint32_t* ctl = nullptr;              // [kCwWords]
};
// mark: nput, reason, the tile counts, ctl[kCwBad] (a listed node not DONE); both scans; the skip counts
hipError_t launch_cw_mark(const CwDev& c, hipStream_t s);
// scatter: the Puts in row order then key order, and the participating rows' (fsid, size)
hipError_t launch_cw_scatter(const CwDev& c, uint8_t* put_keys, uint8_t* put_vals, uint8_t* repo_ids,
                             int64_t* repo_sizes, hipStream_t s);

// capi.cpp (context mutex held): Put(zero expect) over device rows on the
// context's stream, growth decided on the host first; SHA-256 of n messages
// resident in d_arena (offs 16-byte aligned, host arrays) into d_out32 through
// the context's one-shot plan, GPU legs only, queued on s.
int assoc_put_rows_locked(rf_assoc* a, int kind, const uint8_t* d_keys, const uint8_t* d_vals, uint64_t n,
                          int32_t* d_status);
int sha_resident_locked(rf_ctx* ctx, const void* d_arena, const uint64_t* offs, const uint64_t* lens, uint64_t n,
                        void* d_out32, hipStream_t s);
// repo.cpp (context mutex held): rf_repo_put_device's body
rf_ctx* repo_ctx(rf_repo* r);
int repo_put_rows_locked(rf_repo* r, const uint8_t* d_ids, const int64_t* d_sizes, uint64_t n, int32_t* d_status,
                         hipStream_t s);

}  // namespace rf
