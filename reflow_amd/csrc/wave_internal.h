// wave_internal.h -- internal: what the evaluation wave's host side
// (eval_wave.cpp) shares with its kernels (k10_wave.hip).  Node flags
// (RF_PLAN_F_*), states (RF_PLAN_*) and key rows as the plan's; the block,
// grid and list-tile constants are the plan's too (engine.h).  Not part of the
// public ABI.
#pragma once
#include "ctx.h"
#include "engine.h"

#include <vector>

namespace rf {

// control words (u32) of a wave object, device memory
enum : uint32_t {
    kWaveLo = 0,      // the next descent round's frontier is queue[lo, hi)
    kWaveHi,
    kWaveTail,        // descent queue entries appended so far
    kWaveArrived,     // workgroups of the running descent round that are through (zero between launches)
    kWaveHits,        // hit rows handed out since the last begin
    kWaveLooked,      // nodes looked up by the last call
    kWaveProbed,      // their keys that went to the assoc
    kWaveFiltered,    // their keys the liveset ruled out
    kWaveBad,         // a check found a listed node (or a state byte) it refuses
    kWaveWTail,       // nodes in the wave queue: the last wave's size
    kWaveCounts = 16,  // [5] nodes per state
    kWaveWords = 32,
};

struct WaveDev {
    uint32_t n = 0;
    const uint64_t* dep_ptr = nullptr;   // [n+1]
    const uint32_t* deps = nullptr;
    const uint64_t* cons_ptr = nullptr;  // [n+1] the consumer CSR (wave_check.h)
    const uint32_t* cons = nullptr;
    const uint8_t* flags = nullptr;      // [n]
    const uint64_t* key_ptr = nullptr;   // [n+1]
    const uint32_t* key_slots = nullptr; // [K] or null
    uint32_t* claim = nullptr;    // [ceil(n/32)] bit i: the descent reached node i
    uint32_t* rootbit = nullptr;  // [ceil(n/32)] bit i: node i is a listed root
    uint32_t* fin = nullptr;      // [ceil(n/32)] bit i: a step finished node i
    uint32_t* last = nullptr;     // [n_pad/32] bit i: node i entered by the last begin or step
    uint8_t* state = nullptr;     // [n rounded up to whole list tiles]
    uint32_t* pending = nullptr;  // [n] a TODO node's dep entries whose dep has not finished
    uint8_t* which = nullptr;     // [n] a hit's first key with a value
    uint8_t* found = nullptr;     // [n] a looked-up node's found mask
    uint32_t* hitrow = nullptr;   // [n] a hit's row in rows
    uint4* rows = nullptr;        // [2 * row_cap] the hits' values, in arrival order
    uint32_t row_cap = 0;         // nodes with at least one key: no begin has more hits
    uint32_t* queue = nullptr;    // [n] the descent's queue: every reached node once, in arrival order
    uint32_t* wq = nullptr;       // [n] the wave queue: the nodes that just became ready, in arrival order
    uint32_t* ctl = nullptr;      // [kWaveWords]
};

// what a wave's lookups read; lookup false (top-down continuation): none happen
struct WaveLook {
    bool lookup = false;
    const uint8_t* keys = nullptr;  // rows in key_ptr order, or (with slots) the graph's slot table
    bool by_slot = false;
    int no_cache_extern = 0;
    const uint64_t* words = nullptr;    // the liveset, as PlanLook
    const uint64_t* len_dev = nullptr;
    uint64_t m = 1, mu = 0;
    uint32_t k = 0;
    AssocView t{};
    uint32_t kind = 0;
};

// the object behind rf_eval_wave* (eval_wave.cpp; cache_write.cpp reads its structure and states)
enum { kModeNone = 0, kModeBottomUp = 1, kModeTopDown = 2 };

}  // namespace rf

struct rf_eval_wave {
    rf_ctx* ctx = nullptr;
    int device = 0;  // (kept: close must not touch a context that was destroyed first)
    uint64_t n = 0, n_deps = 0, n_keys = 0;
    uint32_t depth = 0, rounds = 0, round_batch = 1;
    bool has_slots = false;
    uint32_t max_slot = 0;
    int mode = rf::kModeNone;
    int nce = 0;
    uint32_t waves = 0, last_wave = 0;
    rf::WaveDev d;
    DevBuf b_dep_ptr, b_deps, b_cons_ptr, b_cons, b_flags, b_key_ptr, b_key_slots, b_claim, b_root, b_fin, b_last,
        b_state, b_pending, b_which, b_found, b_hitrow, b_rows, b_queue, b_wq, b_ctl;
    DevBuf b_keys, b_ids, b_vals8, b_in;      // host-form keys; roots / listed nodes; set_flags' bytes; begin_states' input
    DevBuf b_ln, b_lw, b_lv, b_lf, b_lcount;  // the host-form list's device outputs
    StreamScratch sc_tiles;                   // the list's tile counts, handed between streams
    uint32_t ctl[rf::kWaveWords] = {};        // as last read
    std::vector<DevBuf*> all() {
        return {&b_dep_ptr, &b_deps,  &b_cons_ptr, &b_cons,  &b_flags,  &b_key_ptr, &b_key_slots, &b_claim, &b_root,
                &b_fin,     &b_last,  &b_state,    &b_pending, &b_which, &b_found,   &b_hitrow,    &b_rows,  &b_queue,
                &b_wq,      &b_ctl,   &b_keys,     &b_ids,   &b_vals8,  &b_in,      &b_ln,        &b_lw,    &b_lv,
                &b_lf,      &b_lcount};
    }
};

namespace rf {

// begin, bottom-up: roots claimed (advance moves the bounds), then descent rounds
hipError_t launch_wave_seed(const WaveDev& w, const uint32_t* roots, uint32_t n_roots, hipStream_t s);
hipError_t launch_wave_descend(const WaveDev& w, uint32_t rounds, hipStream_t s);
// begin from states: bad word = a byte above 4 or a tracked node over an UNSEEN dep; then states, pending, wave 0
hipError_t launch_wave_states_check(const WaveDev& w, const uint8_t* in, hipStream_t s);
hipError_t launch_wave_states_apply(const WaveDev& w, const uint8_t* in, hipStream_t s);
// step: bad word = a listed node neither READY nor HIT; then DONE, the decrements, the wave queue
hipError_t launch_wave_step_check(const WaveDev& w, const uint32_t* nodes, uint32_t n, hipStream_t s);
hipError_t launch_wave_complete(const WaveDev& w, const uint32_t* nodes, uint32_t n, hipStream_t s);
// the wave queue resolved: HIT or READY, membership bits
hipError_t launch_wave_resolve(const WaveDev& w, const WaveLook& l, hipStream_t s);
// reject: bad word = a listed node that is no hit; then READY
hipError_t launch_wave_reject_check(const WaveDev& w, const uint32_t* nodes, uint32_t n, hipStream_t s);
hipError_t launch_wave_reject(const WaveDev& w, const uint32_t* nodes, uint32_t n, hipStream_t s);
hipError_t launch_wave_count(const WaveDev& w, hipStream_t s);
// list: as launch_plan_list; only_last: members of the last wave only
hipError_t launch_wave_list(const WaveDev& w, uint32_t state, bool only_last, uint64_t cap, uint32_t* tile_count,
                            uint32_t* nodes, uint8_t* which, uint8_t* vals, uint8_t* key_found, uint64_t* d_found,
                            hipStream_t s);

}  // namespace rf
