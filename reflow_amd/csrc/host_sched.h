// host_sched.h -- the K1 planner's model of the host leg's schedule, and the
// prefix hand-over it derives from it (DESIGN.md §5 "Prefix hand-over").
//
// host_leg_run is list scheduling: threads x ways lanes pull messages from one
// shared queue in the plan's order (largest first).  A message that is not
// among the first threads x ways waits in that queue, and while it waits an
// idle duo wave on the GPU can hash its first blocks and hand the host the
// chaining value.  The model replays the pool to learn when each message
// starts, and sizes each prefix to what a duo wave finishes by then.
//
// A pure function of its arguments: no HIP, no clocks, no environment.
#pragma once
#include <stdint.h>

#include <vector>

namespace rf {

struct HostSchedParams {
    unsigned threads = 0;
    int ways = 1;  // lanes per thread, 1..4
    // lane_rate[k-1]: bytes/s of ONE lane while k of its thread's lanes are
    // active (rf_host_rate(1), ..., rf_host_rate(ways) / ways)
    double lane_rate[4] = {0, 0, 0, 0};
    double link = 0.0;       // D2H bytes/s every host-leg byte crosses; 0: host-resident
    double msg_cost = 20e-6;  // per message: first D2H chunk / queue hop (s)
    double wake = 100e-6;     // waking the pool (s)
    // prefixes (alpha <= 0 or t_duo <= 0: none)
    double t_duo = 0.0;        // duo chain, s per 64-byte block
    double alpha = 0.0;        // share of a message's wait a duo wave is trusted to use
    uint64_t min_blocks = 0;   // a shorter prefix is not worth a wave: 0 blocks instead
    double end_frac = 0.9;     // longest prefix's modelled end <= end_frac x modelled makespan
    // checkpointed hand-over: the host resumes from the wave's latest record,
    // on average half a checkpoint interval behind the wave -- blocks taken
    // off every prefix (0: the wave's own stopping point, as planned lengths are)
    uint64_t loss_blocks = 0;
    // lone lanes: the first `lone` messages of the queue run alone on their
    // thread.  The thread that claims one claims nothing into its other lanes
    // until that message ends (lanes already running finish their message and
    // then stay empty), so the message runs at lane_rate[0]; afterwards the
    // thread claims normally again.  0, or ways == 1: none.
    uint64_t lone = 0;
};

struct HostSched {
    std::vector<double> t_start;          // s after the pool woke, per message
    std::vector<uint64_t> prefix_blocks;  // whole 64-byte blocks the GPU hashes first
    double makespan = 0.0;                // s, link bound and wake included
    double skipped_bytes = 0.0;           // 64 x sum of prefix_blocks
    // the replay's own record (of the last replay, like the rest)
    std::vector<double> t_end;       // s after the pool woke, per message (-1: never ran)
    std::vector<uint32_t> thread;    // the thread that claimed it (~0u: none did)
    std::vector<uint8_t> lane;       // ... and into which of its lanes
    uint64_t claims = 0;             // messages handed out, all told
    double thread_end = 0.0;         // s: the last thread's end, without link bound and wake
};

// Messages lens[0..n) in queue order.
HostSched host_schedule(const uint64_t* lens, uint64_t n, const HostSchedParams& p);

}  // namespace rf
