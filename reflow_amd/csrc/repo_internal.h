// repo_internal.h -- internal: what the repository index's host driver
// (repo.cpp) shares with its kernels (k9_repo.hip).  Not part of the public ABI.
#pragma once
#include "ctx.h"
#include "engine.h"
#include "live_internal.h"

namespace rf {

constexpr uint32_t kRepoBlock = 256;
constexpr uint32_t kRepoListTile = 1024;  // rows (or counts) per tile: 256 lanes of four
// counter words (u64) of an index, device memory
enum : uint32_t {
    kRepoObjects = 0,  // live objects
    kRepoBytes,        // the sum of their sizes (two's complement)
    kRepoTombs,        // tombstones
    kRepoFlags,        // bit 0: a probe bound was hit
    kRepoLastFiles,    // the last missing / need_transfer call: distinct files over its groups
    kRepoLastMissing,  //   those not in the index
    kRepoGone,         // the last collect: objects removed
    kRepoGoneBytes,    //   their sizes summed
    kRepoCtrWords = 8,
};
constexpr uint64_t kRepoFlagProbe = 1;

// The table: a tag word, the 32-B ID and the size per slot.
struct RepoView {
    uint32_t* tag = nullptr;
    uint4* keys = nullptr;  // [slots][2]
    long long* size = nullptr;
    uint32_t mask = 0;
    unsigned long long* ctr = nullptr;  // [kRepoCtrWords]
};

// One call's rows and the dedup's arrays.  A row's class: (group, ID, size)
// with by_size (Files() per group), else the ID alone, rows of negative size
// left out (put / remove: one object per ID).
struct RepoRows {
    uint32_t n_rows = 0;
    const uint8_t* ids = nullptr;       // the rows' source arrays
    const int64_t* sizes = nullptr;     //   (null: remove -- no size)
    const uint32_t* row_ord = nullptr;  // [R] the row's group (null: one group)
    const uint64_t* row_src = nullptr;  // [R] its source row (null: the row itself)
    uint32_t* slot_of = nullptr;        // [R] the table slot of its class
    uint32_t* table = nullptr;          // [mask + 1] row indices, ~0: empty
    uint32_t mask = 0;
    uint32_t by_size = 0;
};

// table cleared, every row inserted: table[slot_of[i]] = the lowest row of i's class
hipError_t launch_repo_dedup(const RepoRows& r, hipStream_t s);
// canon[i] = that row; ~0 for a row left out (negative size) or one that hit the probe bound (flagged in ctr)
hipError_t launch_repo_canon(const RepoRows& r, uint32_t* canon, unsigned long long* ctr, hipStream_t s);
// Put of the deduplicated batch: status per row (int32)
hipError_t launch_repo_put(const RepoView& t, const RepoRows& r, const uint32_t* canon, int32_t* status, hipStream_t s);
hipError_t launch_repo_remove(const RepoView& t, const RepoRows& r, const uint32_t* canon, uint8_t* removed,
                              hipStream_t s);
hipError_t launch_repo_stat(const RepoView& t, const uint8_t* ids, uint64_t n, int64_t* sizes_out, hipStream_t s);
// every live object of `from` into the empty table `to` (tombstones stay behind)
hipError_t launch_repo_rebuild(const RepoView& from, uint64_t from_slots, const RepoView& to, uint64_t to_slots,
                               hipStream_t s);
// Repository.Collect over the slots: live null removes everything; ctr[kRepoGone, kRepoGoneBytes] = the result
hipError_t launch_repo_collect(const RepoView& t, uint64_t slots, const BloomDev* live, hipStream_t s);

// off[0 .. n] = exclusive scan of cnt[0 .. n), off[n] = *total = the sum; tile_sums: [ceil(n / kRepoListTile)] scratch
hipError_t launch_repo_scan(const uint32_t* cnt, uint64_t n, uint64_t* tile_sums, uint64_t* off, uint64_t* total,
                            hipStream_t s);
// need_transfer 1/2: deg[g] = the edges of nodes[g]; bad[g] = 0, or RF_EINVAL for a node >= n (deg 0)
hipError_t launch_repo_nt_degrees(const LiveDev& d, const uint32_t* nodes, uint64_t n_groups, uint32_t* deg,
                                  uint32_t* bad, hipStream_t s);
// need_transfer 2/2: one segment per edge, seg_base = the scan of deg: its group, first arena row and rows;
// an edge without a value sets bad[g] = RF_EPRECONDITION, and a bad group's segments get zero rows
hipError_t launch_repo_nt_segments(const LiveDev& d, const uint32_t* nodes, const uint64_t* seg_base,
                                   uint64_t n_groups, uint64_t n_segs, uint32_t* seg_group, uint64_t* seg_src,
                                   uint32_t* seg_cnt, uint32_t* bad, hipStream_t s);
// row i lies in the segment g with seg_off[g] <= i < seg_off[g + 1]: row_ord[i] = seg_group[g] (null: g),
// row_src[i] (null: not written) = seg_src[g] + i - seg_off[g]
hipError_t launch_repo_locate(const uint64_t* seg_off, uint64_t n_segs, const uint32_t* seg_group,
                              const uint64_t* seg_src, uint32_t n_rows, uint32_t* row_ord, uint64_t* row_src,
                              hipStream_t s);
// the firsts of every class: counted per group, looked up in the index; miss[i] = 1 for a first whose ID is absent.
// n_files / n_missing / missing_bytes: [groups], zeroed by the caller; miss: [rows padded to whole tiles], zeroed
hipError_t launch_repo_resolve(const RepoView& t, const RepoRows& r, uint32_t* n_files, uint32_t* n_missing,
                               unsigned long long* missing_bytes, uint8_t* miss, hipStream_t s);
// the rows with miss[i] = 1, ascending: *d_total = their number; ranks below cap get the row (out_rows), its ID
// and its size -- any of the three may be null
hipError_t launch_repo_list(const RepoRows& r, const uint8_t* miss, uint32_t* tile_count, uint64_t cap,
                            uint64_t* out_rows, uint8_t* out_ids, int64_t* out_sizes, uint64_t* d_total,
                            hipStream_t s);
// The live objects in ascending slot order.  count: *d_total = their number and tile_off = the first rank of every
// tile of kRepoListTile slots (tile_count: [slots / kRepoListTile]; tile_off: one more, u64; tile_sums:
// launch_repo_scan's).  scatter: ranks below cap get the ID and the size (either may be null).
hipError_t launch_repo_index_count(const RepoView& t, uint64_t slots, uint32_t* tile_count, uint64_t* tile_sums,
                                   uint64_t* tile_off, uint64_t* d_total, hipStream_t s);
hipError_t launch_repo_index_scatter(const RepoView& t, uint64_t slots, const uint64_t* tile_off, uint64_t cap,
                                     uint8_t* out_ids, int64_t* out_sizes, hipStream_t s);
// Repository.Collect that lists what it removes, ascending slot order.  mark: dead[slot] = 1 for the objects `live`
// does not contain (null: all), *d_total = their number, tile_off as above; nothing is removed, and
// ctr[kRepoGone, kRepoGoneBytes] are zeroed.  apply: if *d_total (device memory) exceeds cap nothing happens --
// decided on the device; otherwise the dead become tombstones, the counters move as launch_repo_collect moves
// them, and rank i gets the i-th removed object's ID and size (either may be null).
hipError_t launch_repo_collect_mark(const RepoView& t, uint64_t slots, const BloomDev* live, uint8_t* dead,
                                    uint32_t* tile_count, uint64_t* tile_sums, uint64_t* tile_off, uint64_t* d_total,
                                    hipStream_t s);
hipError_t launch_repo_collect_apply(const RepoView& t, uint64_t slots, const uint8_t* dead, const uint64_t* tile_off,
                                     const uint64_t* d_total, uint64_t cap, uint8_t* out_ids, int64_t* out_sizes,
                                     hipStream_t s);
// n dense objects with distinct IDs into the empty table `to` (the counters are the caller's)
hipError_t launch_repo_load(const uint8_t* ids, const int64_t* sizes, uint64_t n, const RepoView& to,
                            uint64_t to_slots, hipStream_t s);
// status[g] = bad[g] (int32)
hipError_t launch_repo_copy_status(const uint32_t* bad, int32_t* status, uint64_t n_groups, hipStream_t s);

}  // namespace rf
