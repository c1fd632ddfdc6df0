// lone_lane_test.cpp -- lone lanes on the host, no GPU and no HIP runtime: the
// schedule model's lone rule (host_sched.cpp) and host_leg_run with lone
// flags, in host memory and through the copy ring.  Driven by
// tests/test_lone_lane.py; built plain, under ASan + UBSan and under
// ThreadSanitizer (make lone_test), each a plain executable.
//
//   lone_lane_test model LENS.txt
//       LENS.txt: message lengths, one per line, in queue order.  Prints the
//       lone = 0 outputs of three parameter sets in full ("S ..." and "M ..."
//       lines, hex floats: the driver compares them with the record of the
//       model before it knew lone lanes), checks the lone rule for every
//       shape, and prints "T lone thread_end makespan@52 makespan@53.5".
//   lone_lane_test leg THREADS host|eager|lazy ORDER LONE
//       The leg over messages made here, at the lengths that straddle the
//       chunk and the ring (in chunks of host_chunk_bytes()).  ORDER: up |
//       down (largest first, as the planner queues them).  LONE: a count (the
//       first LONE messages are lone) or "alt" (every second one).  Every
//       digest must equal host_sha run serially.  "host": in place; "eager" /
//       "lazy": through the chunked copy path over the stand-ins below.
//
// The stand-ins for the HIP calls keep a stream's one queued copy.  "eager"
// performs it when it is queued, so a copy queued into a buffer whose chunk is
// not yet hashed spoils that chunk's digest; "lazy" performs it only in
// hipStreamSynchronize, so a chunk hashed before its stream was waited for is
// stale.  A second copy queued on a stream that still holds one is counted and
// fails the run: that is the ring's rule.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "host_leg.h"
#include "host_sched.h"
#include "host_sha.h"

namespace {
struct FakeStream {
    void* dst = nullptr;
    const void* src = nullptr;
    size_t n = 0;
    bool queued = false;
};
bool g_lazy = false;
std::atomic<uint64_t> g_double_queued{0}, g_copies{0}, g_max_inflight{0};
thread_local uint64_t t_inflight = 0;
}  // namespace

extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
    *s = reinterpret_cast<hipStream_t>(new FakeStream());
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s) {
    FakeStream* f = reinterpret_cast<FakeStream*>(s);
    if (f->queued) {
        if (g_lazy) memcpy(f->dst, f->src, f->n);
        f->queued = false;
        --t_inflight;
    }
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    delete reinterpret_cast<FakeStream*>(s);
    return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
    *p = malloc(n);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) {
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t s) {
    FakeStream* f = reinterpret_cast<FakeStream*>(s);
    if (f->queued) g_double_queued.fetch_add(1);
    f->dst = dst;
    f->src = src;
    f->n = n;
    if (!f->queued) ++t_inflight;
    f->queued = true;
    if (!g_lazy) memcpy(dst, src, n);
    g_copies.fetch_add(1);
    uint64_t m = g_max_inflight.load();
    while (t_inflight > m && !g_max_inflight.compare_exchange_weak(m, t_inflight)) {
    }
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "stub"; }
}

#define CHECK(c, ...)                                 \
    do {                                              \
        if (!(c)) {                                   \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);             \
            fprintf(stderr, "\n");                    \
            return 1;                                 \
        }                                             \
    } while (0)

// configs[1]'s host leg as DESIGN.md §5 quotes it: 16 threads x 2 lanes,
// 2.44 GB/s a lane alone and 1.79 GB/s beside its partner, the duo chain's
// 1.13 us a block, a checkpoint interval of 2,048 blocks.
static rf::HostSchedParams design_params(double link, double alpha, uint64_t loss) {
    rf::HostSchedParams p;
    p.threads = 16;
    p.ways = 2;
    p.lane_rate[0] = 2.44e9;
    p.lane_rate[1] = 1.79e9;
    p.link = link;
    p.t_duo = 1.13e-6;
    p.alpha = alpha;
    p.min_blocks = alpha > 0 ? 2048 : 0;
    p.end_frac = 1.0;
    p.loss_blocks = loss;
    return p;
}

static void dump(const char* name, const rf::HostSched& s) {
    printf("S %s %a %a %zu\n", name, s.makespan, s.skipped_bytes, s.t_start.size());
    for (size_t i = 0; i < s.t_start.size(); ++i)
        printf("M %s %zu %a %llu\n", name, i, s.t_start[i], (unsigned long long)s.prefix_blocks[i]);
}

static bool same(const rf::HostSched& a, const rf::HostSched& b) {
    return a.makespan == b.makespan && a.skipped_bytes == b.skipped_bytes && a.t_start == b.t_start &&
           a.prefix_blocks == b.prefix_blocks;
}

// every message claimed exactly once, and nothing claimed beside a lone message
static int check_rule(const std::vector<uint64_t>& lens, const rf::HostSchedParams& p, const rf::HostSched& s) {
    const uint64_t n = lens.size();
    CHECK(s.t_start.size() == n && s.t_end.size() == n && s.thread.size() == n && s.lane.size() == n, "sizes");
    CHECK(s.claims == n, "%llu claims for %llu messages", (unsigned long long)s.claims, (unsigned long long)n);
    double end = 0;
    for (uint64_t i = 0; i < n; ++i) {
        CHECK(s.thread[i] < p.threads && s.lane[i] < std::min(4, std::max(1, p.ways)), "message %llu: no lane",
              (unsigned long long)i);
        CHECK(s.t_end[i] > s.t_start[i], "message %llu never ran", (unsigned long long)i);
        CHECK(s.prefix_blocks[i] <= lens[i] / 64, "prefix %llu exceeds len/64", (unsigned long long)i);
        end = std::max(end, s.t_end[i]);
    }
    CHECK(end == s.thread_end, "thread_end");
    // one message at a time in a lane
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = i + 1; j < n; ++j)
            if (s.thread[i] == s.thread[j] && s.lane[i] == s.lane[j])
                CHECK(s.t_start[j] >= s.t_end[i], "messages %llu, %llu overlap in one lane", (unsigned long long)i,
                      (unsigned long long)j);
    if (p.ways < 2) return 0;
    // queue order is claim order, so a message j > i was claimed after i
    for (uint64_t i = 0; i < std::min<uint64_t>(n, p.lone); ++i)
        for (uint64_t j = i + 1; j < n; ++j)
            if (s.thread[j] == s.thread[i])
                CHECK(s.t_start[j] >= s.t_end[i], "message %llu claimed beside lone message %llu (%g < %g)",
                      (unsigned long long)j, (unsigned long long)i, s.t_start[j], s.t_end[i]);
    return 0;
}

static int run_model(const char* path) {
    std::vector<uint64_t> lens;
    FILE* f = fopen(path, "r");
    CHECK(f, "cannot open %s", path);
    unsigned long long x;
    while (fscanf(f, "%llu", &x) == 1) lens.push_back(x);
    fclose(f);
    CHECK(!lens.empty(), "no lengths");
    const uint64_t n = lens.size();
    // lone = 0: the outputs in full
    const rf::HostSchedParams sets[3] = {design_params(0.0, 0.0, 0), design_params(52e9, 1.0, 1024),
                                         design_params(53.5e9, 1.25, 0)};
    const char* names[3] = {"bare", "price", "caps"};
    for (int k = 0; k < 3; ++k) {
        const rf::HostSched s = rf::host_schedule(lens.data(), n, sets[k]);
        if (check_rule(lens, sets[k], s)) return 1;
        dump(names[k], s);
    }
    // the lone rule on every shape; the table
    double te0 = 0;
    for (uint64_t lone : {0ull, 1ull, 2ull, 3ull, 4ull, 5ull, 6ull, 7ull, 8ull, 16ull, 17ull, 40ull, (unsigned long long)n,
                          (unsigned long long)n + 5}) {
        rf::HostSchedParams off = design_params(0.0, 1.0, 1024), l52 = design_params(52e9, 1.0, 1024),
                            l535 = design_params(53.5e9, 1.0, 1024);
        off.lone = l52.lone = l535.lone = lone;
        const rf::HostSched a = rf::host_schedule(lens.data(), n, off), b = rf::host_schedule(lens.data(), n, l52),
                            c = rf::host_schedule(lens.data(), n, l535);
        if (check_rule(lens, off, a) || check_rule(lens, l52, b) || check_rule(lens, l535, c)) return 1;
        if (lone == 0) te0 = a.thread_end;
        if (lone == 1) CHECK(a.thread_end < te0, "the thread-bound end does not fall: %.6f -> %.6f", te0, a.thread_end);
        printf("T %llu %.6f %.6f %.6f %.0f\n", (unsigned long long)lone, a.thread_end, b.makespan, c.makespan,
               b.skipped_bytes);
    }
    for (unsigned threads : {1u, 2u, 3u, 16u, 64u})
        for (int ways : {1, 2, 3, 4})
            for (uint64_t lone : {0ull, 1ull, 2ull, 5ull, 1000ull}) {
                rf::HostSchedParams p = design_params(10e9, 1.0, 1024);
                p.threads = threads;
                p.ways = ways;
                for (int k = 0; k < 4; ++k) p.lane_rate[k] = 2.44e9 / (1 + 0.36 * k);
                std::vector<uint64_t> l2(lens.begin(), lens.begin() + std::min<size_t>(n, 40));
                l2.insert(l2.end(), {0, 63, 64, 0});
                p.lone = lone;
                const rf::HostSched s = rf::host_schedule(l2.data(), l2.size(), p);
                if (check_rule(l2, p, s)) return 1;
                rf::HostSchedParams p0 = p;
                p0.lone = 0;
                const rf::HostSched s0 = rf::host_schedule(l2.data(), l2.size(), p0);
                if (ways == 1) CHECK(same(s, s0), "ways = 1: lone %llu changes the schedule", (unsigned long long)lone);
                if (lone) {
                    // fewer messages than lone
                    const rf::HostSched s1 = rf::host_schedule(l2.data(), 3, p);
                    if (check_rule(std::vector<uint64_t>(l2.begin(), l2.begin() + 3), p, s1)) return 1;
                }
            }
    rf::HostSchedParams pe = design_params(52e9, 1.0, 1024);
    pe.lone = 3;
    const rf::HostSched e = rf::host_schedule(nullptr, 0, pe);
    CHECK(e.makespan == 0.0 && e.claims == 0 && e.t_end.empty(), "empty schedule");
    printf("PASS\n");
    return 0;
}

static void fill(std::vector<uint8_t>& a) {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    size_t i = 0;
    for (; i + 8 <= a.size(); i += 8) {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        memcpy(&a[i], &x, 8);
    }
    for (; i < a.size(); ++i) a[i] = (uint8_t)(i * 131);
}

static int run_leg(unsigned threads, const char* where, const char* order, const char* lone) {
    if (!rf::host_sha_available()) {
        printf("SKIP\n");
        return 0;
    }
    const bool host = !strcmp(where, "host");
    g_lazy = !strcmp(where, "lazy");
    const uint64_t C = rf::host_chunk_bytes();
    std::vector<uint64_t> lens = {0, 1, 55, 56, 64, 2 * C - 1, 2 * C, 2 * C + 65};
    if (!host) lens.insert(lens.end(), {C - 1, C, C + 1, 3 * C + 63, 4 * C, 5 * C + 64, 7 * C + 1});
    if (!strcmp(order, "down")) std::stable_sort(lens.begin(), lens.end(), std::greater<uint64_t>());
    const size_t n = lens.size();
    std::vector<rf::HostTask> tasks;
    uint64_t pos = 0;
    for (size_t i = 0; i < n; ++i) {
        tasks.push_back(rf::HostTask{(uint32_t)i, pos, lens[i]});
        tasks.back().lone = !strcmp(lone, "alt") ? i % 2 == 0 : i < (size_t)atoll(lone);
        pos += (lens[i] + 15) / 16 * 16;
    }
    std::vector<uint8_t> arena(std::max<uint64_t>(pos, 16));
    fill(arena);
    std::vector<uint8_t> want(32 * n), out(32 * n, 0xEE);
    for (size_t i = 0; i < n; ++i) {  // host_sha, serially
        uint32_t st[8];
        rf::host_sha_init(st);
        const uint8_t* p = arena.data() + tasks[i].off;
        rf::host_sha_blocks(st, p, lens[i] / 64);
        rf::host_sha_final(st, p + lens[i] / 64 * 64, lens[i] % 64, lens[i], &want[32 * i]);
    }
    std::string err;
    for (int rep = 0; rep < 2; ++rep) {
        std::fill(out.begin(), out.end(), 0xEE);
        rf::HostPool pool(0, threads);
        const bool ok = rf::host_leg_run(pool, tasks.data(), n, host ? nullptr : arena.data(),
                                         host ? arena.data() : nullptr, out.data(), &err, nullptr);
        CHECK(ok, "host_leg_run: %s", err.c_str());
        for (size_t i = 0; i < n; ++i)
            CHECK(!memcmp(&out[32 * i], &want[32 * i], 32), "digest of message %zu (%llu bytes, lone %d) differs", i,
                  (unsigned long long)lens[i], (int)tasks[i].lone);
    }
    CHECK(g_double_queued.load() == 0, "%llu copies queued on a stream that held one",
          (unsigned long long)g_double_queued.load());
    CHECK(host == (g_copies.load() == 0), "copies on the host-resident path, or none on the other");
    printf("copies %llu max_inflight %llu\nPASS\n", (unsigned long long)g_copies.load(),
           (unsigned long long)g_max_inflight.load());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "model")) return run_model(argv[2]);
    if (argc == 6 && !strcmp(argv[1], "leg")) return run_leg((unsigned)atoi(argv[2]), argv[3], argv[4], argv[5]);
    fprintf(stderr, "usage: %s model LENS.txt | leg THREADS host|eager|lazy up|down LONE\n", argv[0]);
    return 2;
}
