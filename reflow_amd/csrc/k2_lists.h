// k2_lists.h -- the level kernels' arguments and the per-level work lists'
// layout (moved verbatim out of k2_graph.hip), shared with the change feed's
// kernels (k6_feed.hip), which read the lists a plain incremental step left.
// Device code only; not part of the public ABI.
#pragma once
#include "engine.h"

namespace rf {

// Diagnostic builds (-DRF_DIAG, diag.h) only: the phase stamps, the
// per-workgroup records, the timing probes (LevelArgs::dbg_twice) and the
// measured-dead kernel forms.  In the release build every such branch folds
// away at compile time and the dead forms are not instantiated.
#ifdef RF_DIAG
constexpr bool kDiag = true;
#else
constexpr bool kDiag = false;
#endif

struct LevelArgs;
__device__ __forceinline__ uint32_t dbg_mode(const LevelArgs& a);
struct LevelArgs {
    uint32_t s, e, lvl;  // internal job range of the level
    int full;
    uint32_t dbg_twice;  // diagnostic: hash every block twice (RF_DBG_HASH2), result unchanged
    const uint4* __restrict__ meta;
    const uint2* __restrict__ holes;
    const uint2* __restrict__ cons;          // {consumer job, its level}
    const uint32_t* __restrict__ lvl_start;  // [L+1] on device
    uint32_t n_levels;
    const uint8_t* __restrict__ tmpl;
    uint8_t* slots;
    uint32_t* dirty;
    uint32_t* list;
    uint32_t* counts;
    unsigned long long* stamps;  // diagnostic (RF_K2_STAMPS): phase times of workgroup 0, else null
    const uint4* __restrict__ mid;  // [2J] initial chaining values, or null (= IV for every job)
    const uint32_t* __restrict__ cons_ptr;  // [S+1] slot -> reverse-edge range (mark / apply kernels)
    uint4* lmeta;                           // [2J] the listed jobs' records, beside list
    uint32_t cb0;  // k2_level_pl<2,false>: chain-built block 0 of fused jobs (1: via the ring, 2: in registers)
    // k2_level_pl: workgroups take the level's list from its END -- the jobs
    // appended last (the chains that reached this level) before the sinks the
    // mark kernel queued early (ALAP-moved physical keys): at 100M nodes the
    // sinks alone fill the first ~2k workgroups of the OpK level
    uint32_t rev;
    uint32_t* zero_counts;  // [L+1] the previous plain step's cursor half, zeroed by workgroup 0 (or null)
    unsigned long long* wgst;  // diagnostic (RF_K2_WGSTAMPS=1): per-workgroup records [L][kWgStamps][4], else null
    // an attached sink list (k2_level_pl / k2_level_lf): the sink level lvl2's
    // list (at s2) is taken after this level's own, in the same launch
    // (graph_enqueue, GraphDev kLvlSink); lvl2 = ~0u: none
    uint32_t s2 = 0, lvl2 = ~0u;
    // split block 0 (k2_level_pl<2> cb0 = 2, GraphDev::split_b0): the
    // producer expands the upper half of a fusion target's block 0 and builds
    // its template-only block 1 during the job before it
    uint32_t split = 0;
    uint32_t oct_wg = 0;  // k2_level_oct: workgroups of the level's own list (the rest run the sink list)
    // k2_level_pl: nonzero = workgroups from sink_wg on run the attached sink
    // list one job per lane at the lowest priority (lf_job), the rest the
    // level's own list; ovf = 1: the own list only up to sink_wg x 64 jobs
    // (one batch per latency-form workgroup, one per CU), its overflow one
    // chain per lane in those lane workgroups too, before the sinks
    uint32_t sink_wg = 0, ovf = 0;
    uint32_t handoff = 1;  // k2_level_pl cb0 = 2: the producer hands the chain its next target's operands
    uint32_t n_cu = 256;   // the device's CUs (k2_level_lf's issue priorities)
    // GraphDev::fuse_pos2: every fusion target's one hole at byte 2 of its
    // first block, reading its producer's slot -- its hole record need not be
    // loaded (fused_hole)
    uint32_t fuse_pos2 = 0;
    uint32_t sf_pos = ~0u;  // GraphDev::sf_pos (slot-fused jobs, the mark kernels)
    // GraphDev::lvl_lead0 of lvl / lvl2: the listed jobs start from the IV
    uint32_t lead0 = 0, lead0_2 = 0;
    const uint4* __restrict__ plan = nullptr;  // [3S] the mark kernels' per-slot plan (GraphDev::plan), or null
};
// The diagnostic mode of a launch (LevelArgs::dbg_twice): always 0 in a release build.
__device__ __forceinline__ uint32_t dbg_mode(const LevelArgs& a) { return kDiag ? a.dbg_twice : 0u; }

// A level's append cursors (engine.h kListShards): run k of level l holds
// the listed jobs whose ids fall in [lvl_start[l] + k * 2^sh, ... + 2^sh),
// its cursor at list_shard_off(L) + k * Lp + l.
__device__ __forceinline__ const uint32_t* shard_cursors(const LevelArgs& a, uint32_t l) {
    return a.counts + list_shard_off(a.n_levels) + l;
}
// Jobs listed at level l this step.
__device__ __forceinline__ uint32_t level_count(const LevelArgs& a, uint32_t l) {
    if constexpr (kLegacyLists) return a.counts[l];
    const uint32_t* c = shard_cursors(a, l);
    const uint32_t lp = cursor_lp(a.n_levels);
    uint32_t n = 0;
#pragma unroll
    for (uint32_t k = 0; k < kListShards; ++k) n += c[k * lp];
    return n;
}
// The list position of level l's i-th listed job: runs in order, each run's
// entries from its start (branch-free over the runs).
__device__ __forceinline__ uint32_t level_pos(const LevelArgs& a, uint32_t l, uint32_t i) {
    if constexpr (kLegacyLists) return a.lvl_start[l] + i;
    const uint32_t* c = shard_cursors(a, l);
    const uint32_t lp = cursor_lp(a.n_levels), b = a.lvl_start[l];
    const uint32_t sh = list_shard_shift(a.lvl_start[l + 1] - b);
    uint32_t k = 0;
#pragma unroll
    for (uint32_t q = 0; q < kListShards; ++q) {
        const uint32_t cq = c[q * lp];
        const bool past = k == q && i >= cq;
        i -= past ? cq : 0u;
        k += past ? 1u : 0u;
    }
    return b + (k << sh) + i;
}

}  // namespace rf
