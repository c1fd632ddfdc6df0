// prefix_plan_test.cpp -- the prefix hand-over on the host, no GPU and no HIP
// runtime: the schedule model (host_sched.cpp) and host_leg_run resuming from
// chaining values made here with host_sha_blocks.  Driven by
// tests/test_prefix_plan.py; built twice (plain, and under ASan + UBSan).
//
//   prefix_plan_test model LENS.txt
//       LENS.txt: message lengths, one per line, in queue order.  Checks the
//       model's invariants on them and prints the figures the driver asserts.
//   prefix_plan_test leg ARENA.bin TASKS.txt THREADS device|host
//       TASKS.txt: "off len prefix_blocks ready" per line.  Prints one hex
//       digest per task.  "device" reads the arena through the (stubbed) D2H
//       chunk path, "host" in place.
//
// The few HIP entry points host_leg.cpp uses are defined below over plain
// host memory, so the leg's chunked copy path runs here too.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "host_leg.h"
#include "host_sched.h"
#include "host_sha.h"

extern "C" {
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int) {
    *s = reinterpret_cast<hipStream_t>(new int(0));
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t s) {
    delete reinterpret_cast<int*>(s);
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
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind, hipStream_t) {
    memcpy(dst, src, n);
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

static rf::HostSchedParams issue_params(double alpha) {
    rf::HostSchedParams p;
    p.threads = 16;
    p.ways = 2;
    p.lane_rate[0] = 2.4e9;
    p.lane_rate[1] = 1.63e9;
    p.link = 0.0;
    p.t_duo = 1.13e-6;
    p.alpha = alpha;
    p.min_blocks = 0;
    return p;
}

static int check_invariants(const std::vector<uint64_t>& lens, const rf::HostSchedParams& p, const rf::HostSched& s) {
    const uint64_t n = lens.size();
    CHECK(s.t_start.size() == n && s.prefix_blocks.size() == n, "sizes");
    const uint64_t first = std::min<uint64_t>(n, (uint64_t)p.threads * p.ways);
    double skipped = 0, longest = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (i < first) CHECK(s.prefix_blocks[i] == 0 && s.t_start[i] == 0.0, "message %llu of the first wave has a prefix", (unsigned long long)i);
        CHECK(s.prefix_blocks[i] <= lens[i] / 64, "prefix %llu exceeds len/64", (unsigned long long)i);
        CHECK(s.prefix_blocks[i] == 0 || s.prefix_blocks[i] >= p.min_blocks, "prefix %llu below the floor", (unsigned long long)i);
        // a prefix never outruns its message's wait
        CHECK((double)s.prefix_blocks[i] * p.t_duo <= p.alpha * s.t_start[i] + 1e-12, "prefix %llu not ready at its start", (unsigned long long)i);
        skipped += 64.0 * (double)s.prefix_blocks[i];
        longest = std::max(longest, (double)s.prefix_blocks[i] * p.t_duo);
    }
    CHECK(skipped == s.skipped_bytes, "skipped bytes");
    CHECK(longest <= p.end_frac * s.makespan + 1e-12, "longest prefix ends after %.2f x makespan", p.end_frac);
    // monotone in start time: a later start never has a shorter prefix unless
    // its message is too short for more (or the floor took it)
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = 0; j < n; ++j)
            if (s.t_start[i] <= s.t_start[j] && s.prefix_blocks[j] < s.prefix_blocks[i])
                CHECK(s.prefix_blocks[j] == lens[j] / 64 || s.prefix_blocks[j] == 0,
                      "prefixes %llu, %llu not monotone in start time", (unsigned long long)i, (unsigned long long)j);
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
    const rf::HostSched s0 = rf::host_schedule(lens.data(), lens.size(), issue_params(0.0));
    if (check_invariants(lens, issue_params(0.0), s0)) return 1;
    CHECK(s0.skipped_bytes == 0.0, "prefixes without alpha");
    printf("alpha 0 makespan %.6f moved 0\n", s0.makespan);
    for (double alpha : {0.8, 0.85, 0.9}) {
        for (uint64_t floor_blocks : {0ull, 4096ull}) {
            rf::HostSchedParams p = issue_params(alpha);
            p.min_blocks = floor_blocks;
            const rf::HostSched s = rf::host_schedule(lens.data(), lens.size(), p);
            if (check_invariants(lens, p, s)) return 1;
            if (!floor_blocks) printf("alpha %.2f makespan %.6f moved %.0f\n", alpha, s.makespan, s.skipped_bytes);
        }
    }
    // degenerate shapes: fewer messages than lanes, one thread, four ways, zero lengths
    for (unsigned threads : {1u, 3u, 64u})
        for (int ways : {1, 2, 4}) {
            rf::HostSchedParams p = issue_params(0.85);
            p.threads = threads;
            p.ways = ways;
            for (int k = 0; k < 4; ++k) p.lane_rate[k] = 2.4e9 / (1 + 0.4 * k);
            p.link = 10e9;
            std::vector<uint64_t> l2(lens.begin(), lens.begin() + std::min<size_t>(lens.size(), 40));
            l2.push_back(0);
            l2.push_back(63);
            l2.push_back(64);
            const rf::HostSched s = rf::host_schedule(l2.data(), l2.size(), p);
            if (check_invariants(l2, p, s)) return 1;
        }
    const rf::HostSched e = rf::host_schedule(nullptr, 0, issue_params(0.85));
    CHECK(e.makespan == 0.0 && e.prefix_blocks.empty(), "empty schedule");
    printf("PASS\n");
    return 0;
}

static int run_leg(const char* arena_path, const char* tasks_path, unsigned threads, bool device) {
    if (!rf::host_sha_available()) {
        printf("SKIP\n");
        return 0;
    }
    std::vector<uint8_t> arena;
    FILE* f = fopen(arena_path, "rb");
    CHECK(f, "cannot open %s", arena_path);
    uint8_t buf[1 << 16];
    for (size_t r; (r = fread(buf, 1, sizeof buf, f)) > 0;) arena.insert(arena.end(), buf, buf + r);
    fclose(f);
    f = fopen(tasks_path, "r");
    CHECK(f, "cannot open %s", tasks_path);
    std::vector<rf::HostTask> tasks;
    std::vector<int> set;
    unsigned long long off, len, pb;
    int ready;
    while (fscanf(f, "%llu %llu %llu %d", &off, &len, &pb, &ready) == 4) {
        CHECK(off + len <= arena.size() && pb <= len / 64, "bad task");
        rf::HostTask t{(uint32_t)tasks.size(), off, len};
        t.prefix_blocks = pb;
        tasks.push_back(t);
        set.push_back(ready);
    }
    fclose(f);
    const size_t n = tasks.size();
    // chaining values as a GPU wave would leave them; a prefix whose flag
    // stays unset keeps a junk value that must not be read
    std::vector<uint32_t> mid(8 * n, 0xABABABABu), flag(n, 0u);
    uint64_t want_taken = 0, want_missed = 0, want_skipped = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!tasks[i].prefix_blocks) continue;
        tasks[i].mid = &mid[8 * i];
        tasks[i].ready = &flag[i];
        if (set[i]) {
            rf::host_sha_init(&mid[8 * i]);
            rf::host_sha_blocks(&mid[8 * i], arena.data() + tasks[i].off, tasks[i].prefix_blocks);
            flag[i] = 1;
            ++want_taken;
            want_skipped += 64 * tasks[i].prefix_blocks;
        } else {
            ++want_missed;
        }
    }
    std::vector<uint8_t> out(32 * std::max<size_t>(n, 1));
    std::string err;
    rf::HostLegStats st;
    {
        rf::HostPool pool(0, threads);
        const bool ok = rf::host_leg_run(pool, tasks.data(), n, device ? arena.data() : nullptr,
                                         device ? nullptr : arena.data(), out.data(), &err, &st);
        CHECK(ok, "host_leg_run: %s", err.c_str());
    }
    CHECK(st.taken == want_taken && st.missed == want_missed && st.skipped_bytes == want_skipped,
          "counters: taken %llu (want %llu), missed %llu (%llu), skipped %llu (%llu)", (unsigned long long)st.taken,
          (unsigned long long)want_taken, (unsigned long long)st.missed, (unsigned long long)want_missed,
          (unsigned long long)st.skipped_bytes, (unsigned long long)want_skipped);
    for (size_t i = 0; i < n; ++i) {
        for (int b = 0; b < 32; ++b) printf("%02x", out[32 * i + b]);
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "model")) return run_model(argv[2]);
    if (argc == 6 && !strcmp(argv[1], "leg"))
        return run_leg(argv[2], argv[3], (unsigned)atoi(argv[4]), !strcmp(argv[5], "device"));
    fprintf(stderr, "usage: %s model LENS.txt | leg ARENA.bin TASKS.txt THREADS device|host\n", argv[0]);
    return 2;
}
