// host_sched.cpp -- the host leg's schedule model (host_sched.h).
#include "host_sched.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <queue>
#include <utility>

namespace rf {

namespace {

struct Thread {
    double t = 0.0;
    double rem[4] = {0, 0, 0, 0};  // bytes left per lane (the per-message cost folded in)
    bool act[4] = {false, false, false, false};
    uint64_t msg[4] = {0, 0, 0, 0};
    int na = 0;
    int lone = -1;  // the lane that holds a lone message
};

// One replay of the pool; prefixes longer than cap_blocks are cut to it.
// Returns the largest prefix before the cut.
uint64_t replay(const uint64_t* lens, uint64_t n, const HostSchedParams& p, uint64_t cap_blocks, HostSched* out) {
    const int W = std::min(4, std::max(1, p.ways));
    const bool prefixes = p.alpha > 0 && p.t_duo > 0;
    out->t_start.assign(n, 0.0);
    out->prefix_blocks.assign(n, 0);
    out->skipped_bytes = 0.0;
    out->makespan = 0.0;
    out->t_end.assign(n, -1.0);
    out->thread.assign(n, ~0u);
    out->lane.assign(n, 0);
    out->claims = 0;
    out->thread_end = 0.0;
    if (!n || !p.threads) return 0;
    const double msg_bytes = p.msg_cost * p.lane_rate[W - 1];
    uint64_t next = 0, longest = 0;
    double cross = 0.0;
    std::vector<Thread> ths(p.threads);
    auto claim = [&](Thread& th, int k) {
        th.act[k] = false;
        if (th.lone >= 0 && th.lone != k) return;  // beside a lone message: stay empty
        if (next >= n) return;
        const uint64_t i = next++;
        if (i < p.lone && W > 1) th.lone = k;
        out->thread[i] = (uint32_t)(&th - ths.data());
        out->lane[i] = (uint8_t)k;
        ++out->claims;
        uint64_t pb = 0;
        if (prefixes) {
            pb = std::min<uint64_t>((uint64_t)std::floor(p.alpha * th.t / p.t_duo), lens[i] / 64);
            longest = std::max(longest, pb);
            pb = std::min(pb, cap_blocks);
            pb -= std::min(pb, p.loss_blocks);
            if (pb < std::max<uint64_t>(p.min_blocks, 1)) pb = 0;
        }
        out->t_start[i] = th.t;
        out->prefix_blocks[i] = pb;
        out->skipped_bytes += 64.0 * (double)pb;
        const double left = (double)(lens[i] - 64 * pb);
        cross += left;
        th.rem[k] = left + msg_bytes;
        th.msg[k] = i;
        th.act[k] = true;
        ++th.na;
    };
    // (finish time of the thread's next lane, thread)
    typedef std::pair<double, unsigned> Ev;
    std::priority_queue<Ev, std::vector<Ev>, std::greater<Ev>> q;
    auto push = [&](unsigned w) {
        const Thread& th = ths[w];
        if (!th.na) return;
        double m = 1e300;
        for (int k = 0; k < W; ++k)
            if (th.act[k]) m = std::min(m, th.rem[k]);
        q.push(Ev(th.t + m / p.lane_rate[th.na - 1], w));
    };
    for (unsigned w = 0; w < p.threads; ++w) {
        for (int k = 0; k < W; ++k) claim(ths[w], k);
        push(w);
    }
    double end = 0.0;
    while (!q.empty()) {
        const unsigned w = q.top().second;
        const double t = q.top().first;
        q.pop();
        Thread& th = ths[w];
        double m = 1e300;
        for (int k = 0; k < W; ++k)
            if (th.act[k]) m = std::min(m, th.rem[k]);
        th.t = t;
        end = std::max(end, t);
        bool lone_ended = false;
        for (int k = 0; k < W; ++k) {
            if (!th.act[k]) continue;
            th.rem[k] -= m;
            if (th.rem[k] <= 1e-6) {  // done (and any lane that ties with it)
                --th.na;
                out->t_end[th.msg[k]] = t;
                if (th.lone == k) {
                    th.lone = -1;
                    lone_ended = true;
                }
                claim(th, k);
            }
        }
        // the lanes that stayed empty beside a lone message claim again
        for (int k = 0; k < W && lone_ended; ++k)
            if (!th.act[k]) claim(th, k);
        push(w);
    }
    out->thread_end = end;
    out->makespan = std::max(end, p.link > 0 ? cross / p.link : 0.0) + p.wake;
    return longest;
}

}  // namespace

HostSched host_schedule(const uint64_t* lens, uint64_t n, const HostSchedParams& p) {
    HostSched s;
    const uint64_t longest = replay(lens, n, p, ~0ull, &s);
    if (p.alpha > 0 && p.t_duo > 0 && p.end_frac > 0) {
        // The uncut makespan is the shorter one, so a cut sized to it also
        // holds against the makespan of the replay with the cut applied.
        const uint64_t cap = (uint64_t)std::floor(p.end_frac * s.makespan / p.t_duo);
        if (longest > cap) replay(lens, n, p, cap, &s);
    }
    return s;
}

}  // namespace rf
