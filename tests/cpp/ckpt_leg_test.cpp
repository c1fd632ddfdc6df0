// ckpt_leg_test.cpp -- the checkpointed prefix hand-over on the host, no GPU
// and no HIP runtime: host_leg_run over tasks whose records (prefix_record.h)
// are prepared here with host_sha_blocks, as a duo wave would leave them.
// Driven by tests/test_ckpt_leg.py; built twice (plain, and under ASan + UBSan).
//
//   ckpt_leg_test THREADS device|host
//       "device" reads the arena through the (stubbed) D2H chunk path, "host"
//       in place.  Prints PASS, or SKIP without SHA extensions.
//
// The few HIP entry points host_leg.cpp uses are defined below over plain
// host memory, so the leg's chunked copy path runs here too.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "host_leg.h"
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

#define CHECK(c, ...)                                            \
    do {                                                         \
        if (!(c)) {                                              \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
            return 1;                                            \
        }                                                        \
    } while (0)

namespace {

struct Case {
    uint64_t len;
    bool record;      // false: a task without a hand-over
    uint32_t latest;  // 0: nothing published
    uint64_t blocks;  // of record `latest`
};

// a resumed start in front of a chunk boundary of the leg: 8 MiB chunks for the
// first, the default 16 MiB for the second
const uint64_t kBig = 9ull * 1024 * 1024 + 197, kBig2 = 17ull * 1024 * 1024 + 197;

std::vector<Case> cases() {
    std::vector<Case> c;
    // every padding edge with every record number; blocks at the chunk edges,
    // at the cap (129 = every whole block: no multiple of 64) and at 65
    for (uint64_t r : {0ull, 1ull, 55ull, 56ull, 63ull}) {
        const uint64_t n = 129 * 64 + r;
        const uint64_t blocks[4] = {64, 128, 129, 65};
        const uint32_t latest[4] = {1, 2, 7, 0};
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) c.push_back({n, true, latest[j], blocks[(i + j) % 4]});
    }
    c.push_back({kBig, true, 1, 64});
    c.push_back({kBig, true, 2, 128});
    c.push_back({kBig, true, 0, 64});
    c.push_back({kBig, true, 7, kBig / 64});
    c.push_back({kBig2, true, 1, 64});
    c.push_back({kBig2, true, 2, 65});
    // the prefix is the whole message: padding only
    c.push_back({64, true, 1, 1});
    c.push_back({128 * 64, true, 2, 128});
    c.push_back({128 * 64, true, 7, 128});
    // beside tasks without a record
    c.push_back({0, false, 0, 0});
    c.push_back({5000, false, 0, 0});
    c.push_back({64 * 200, false, 0, 0});
    return c;
}

int retry_rule() {
    using rf::prefix_copy_intact;
    CHECK(prefix_copy_intact(1, 1) && prefix_copy_intact(1, 2), "a copy is intact while latest moves by <= 1");
    CHECK(!prefix_copy_intact(1, 3) && !prefix_copy_intact(2, 9), "a copy is stale once latest moved by 2");
    CHECK(prefix_copy_intact(0xffffffffu, 0u) && !prefix_copy_intact(0xffffffffu, 1u), "the counter may wrap");
    // nothing published: no take, whatever the slots hold
    rf::PrefixRecord rec;
    memset(&rec, 0xAB, sizeof rec);
    rec.latest = 0;
    uint32_t st[8];
    uint64_t blocks = 0;
    CHECK(!rf::prefix_record_take(&rec, st, &blocks), "take with latest == 0");
    // record 5 sits in slot 1
    rec.latest = 5;
    for (int i = 0; i < 8; ++i) rec.slot[1].state[i] = 100 + i;
    rec.slot[1].blocks = 4096;
    CHECK(rf::prefix_record_take(&rec, st, &blocks) && blocks == 4096 && st[0] == 100 && st[7] == 107, "take slot 1");
    return 0;
}

int run(unsigned threads, bool device) {
    const std::vector<Case> cs = cases();
    const size_t n = cs.size();
    std::vector<uint64_t> offs(n);
    uint64_t pos = 0;
    for (size_t i = 0; i < n; ++i) {
        offs[i] = pos;
        pos += (cs[i].len + 15) / 16 * 16;
    }
    std::vector<uint8_t> arena(pos + 16);
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (uint8_t& b : arena) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        b = (uint8_t)(x >> 56);
    }
    std::vector<rf::HostTask> tasks;
    std::vector<rf::PrefixRecord> rec(n);
    std::vector<uint32_t> claimed(n, 0u);
    uint64_t want_taken = 0, want_missed = 0, want_skipped = 0;
    for (size_t i = 0; i < n; ++i) {
        rf::HostTask t{(uint32_t)i, offs[i], cs[i].len};
        // both slots junk, the junk block count past the message's end
        memset(&rec[i], 0xAB, sizeof rec[i]);
        rec[i].latest = 0;
        if (cs[i].record) {
            CHECK(cs[i].blocks <= cs[i].len / 64, "bad case %zu", i);
            t.prefix_blocks = cs[i].len / 64;  // the cap
            t.rec = &rec[i];
            t.claimed = &claimed[i];
            if (cs[i].latest) {
                rf::PrefixSlot& s = rec[i].slot[cs[i].latest & 1];
                rf::host_sha_init(s.state);
                rf::host_sha_blocks(s.state, arena.data() + offs[i], cs[i].blocks);
                s.blocks = cs[i].blocks;
                rec[i].latest = cs[i].latest;
                ++want_taken;
                want_skipped += 64 * cs[i].blocks;
            } else {
                ++want_missed;
            }
        }
        tasks.push_back(t);
    }
    std::vector<uint8_t> out(32 * n);
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
        uint8_t want[32];
        rf::host_sha256(arena.data() + offs[i], cs[i].len, want);
        CHECK(!memcmp(want, &out[32 * i], 32), "digest of task %zu (len %llu, latest %u, blocks %llu)", i,
              (unsigned long long)cs[i].len, cs[i].latest, (unsigned long long)cs[i].blocks);
        CHECK(claimed[i] == (cs[i].record ? 1u : 0u), "claimed word of task %zu is %u", i, claimed[i]);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: %s THREADS device|host\n", argv[0]);
        return 2;
    }
    if (retry_rule()) return 1;
    if (!rf::host_sha_available()) {
        printf("SKIP\n");
        return 0;
    }
    if (run((unsigned)atoi(argv[1]), !strcmp(argv[2], "device"))) return 1;
    printf("PASS\n");
    return 0;
}
