// live_internal.h -- internal: what the GC liveset's host driver (liveset.cpp)
// shares with its kernels (k8_live.hip) and with the filter object of
// capi.cpp.  Not part of the public ABI.
#pragma once
#include "ctx.h"
#include "engine.h"

namespace rf {

constexpr uint32_t kLiveBlock = 256;
constexpr uint32_t kLiveMaxGrid = 1024;   // the round kernel's fixed grid: at most this many workgroups
constexpr uint32_t kLiveListTile = 1024;  // nodes (or contributions) per tile: 256 lanes of four
// control words (u32) of a liveset, device memory
enum : uint32_t {
    kLiveLo = 0,      // the next round's frontier is queue[lo, hi)
    kLiveHi,
    kLiveTail,        // queue entries appended so far
    kLiveArrived,     // workgroups of the running round that are through (zero between launches)
    kLiveCounts = 8,  // [3] nodes per state
    kLiveWords = 16,
};
// result words (u64) of a run, device memory
enum : uint32_t {
    kLiveEst = 0,   // rows over all contributions
    kLiveN,         // distinct (ID, Size) per contribution, summed
    kLiveBytes,     // the sum of their sizes (two's complement)
    kLiveFlags,     // bit 0: the dedup's probe bound was hit; bit 1: a filter word differs
    kLiveResWords = 8,
};
constexpr uint64_t kLiveFlagProbe = 1, kLiveFlagDiff = 2;

struct LiveDev {
    uint32_t n = 0;
    const uint64_t* edge_ptr = nullptr;  // [n+1]
    const uint32_t* edges = nullptr;
    uint8_t* has = nullptr;              // [n] 1: the node has a value
    uint64_t* val_off = nullptr;         // [n] its first arena row
    uint32_t* val_cnt = nullptr;         // [n] its rows
    const uint8_t* ids = nullptr;        // the arena: [rows][32]
    const int64_t* sizes = nullptr;      //            [rows]
    uint32_t* claim = nullptr;           // [ceil(n/32)] bit i: node i was reached
    uint8_t* state = nullptr;            // [n rounded up to whole list tiles]
    uint32_t* queue = nullptr;           // [n] every expanded node once, in arrival order
    uint32_t* ctl = nullptr;             // [kLiveWords]
    unsigned long long* res = nullptr;   // [kLiveResWords]
};
// one run's rows: contributions, their row offsets, and the dedup's arrays
struct LiveRows {
    uint64_t n_contrib = 0;             // C
    const uint32_t* contrib = nullptr;  // [C] node per contribution
    uint64_t* row_off = nullptr;        // [C+1] exclusive scan of the row counts
    uint64_t* tile_rows = nullptr;      // [ceil(C / kLiveListTile)]
    uint32_t n_rows = 0;                // R = row_off[C] <= RF_LIVE_MAX_ROWS
    uint32_t* row_ord = nullptr;        // [R] the row's contribution
    uint64_t* row_src = nullptr;        // [R] its arena row
    uint32_t* slot_of = nullptr;        // [R] the table slot of its class
    uint32_t* table = nullptr;          // [mask + 1] row indices, ~0: empty
    uint32_t mask = 0;
};

uint32_t live_grid(uint32_t n);
uint32_t live_table_slots(uint32_t rows);
// entry i: node nodes[i] has (has[i], off[i], cnt[i]); a node listed twice carries the same triple twice
hipError_t launch_live_set(const LiveDev& d, const uint32_t* nodes, const uint8_t* has, const uint64_t* off,
                           const uint32_t* cnt, uint32_t n, hipStream_t s);
hipError_t launch_live_seed(const LiveDev& d, const uint32_t* roots, uint32_t n_roots, hipStream_t s);
hipError_t launch_live_rounds(const LiveDev& d, uint32_t rounds, hipStream_t s);
hipError_t launch_live_count(const LiveDev& d, hipStream_t s);  // ctl counts zeroed here
// list: tile_count [ceil(n / kLiveListTile)], *d_found (u64) = nodes in `state`
hipError_t launch_live_list(const LiveDev& d, uint32_t state, uint64_t cap, uint32_t* tile_count, uint32_t* nodes,
                            uint64_t* d_found, hipStream_t s);
// row_off = exclusive scan of the contributions' row counts; res[kLiveEst] = row_off[C] = their sum
hipError_t launch_live_offsets(const LiveDev& d, const LiveRows& r, hipStream_t s);
// locate every row, dedup per contribution, sum the firsts and add them to the filter (zeroed, length m)
hipError_t launch_live_rows(const LiveDev& d, const LiveRows& r, const BloomDev& b, hipStream_t s);
// res[kLiveFlags] |= kLiveFlagDiff iff a[0..nwords) != b[0..nwords)
hipError_t launch_live_compare(const LiveDev& d, const uint64_t* a, const uint64_t* b, uint64_t nwords,
                               hipStream_t s);

// liveset.cpp: the object behind rf_liveset*, as far as the repository index's
// need_transfer (repo.cpp) needs it: its context, and the graph and value
// records on the device (the view: context mutex held, and for as long as it is).
rf_ctx* live_ctx(rf_liveset* l);
const LiveDev& live_dev(rf_liveset* l);

// capi.cpp: a filter the liveset owns and lends out (rf_bloom_destroy leaves
// it alone).  *slot: null or a filter made here; it becomes an empty filter of
// (m, k) with length m on s.  Context mutex held, device set.
int bloom_lent_shape(rf_ctx* ctx, rf_bloom** slot, uint64_t m, uint64_t k, hipStream_t s);
void bloom_lent_free(rf_bloom* b);
uint64_t bloom_device_bytes(rf_bloom* b);

}  // namespace rf
