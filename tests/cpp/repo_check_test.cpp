// repo_check_test.cpp -- the repository index's host-only parts
// (reflow_amd/csrc/repo_check.cpp) on their own: no library, no device.
//
// The table's size rule and the growth decision against a plain restatement
// of the header's rule; counts that overflow and row totals against the limit;
// negative sizes in the host form of put; every NULL combination of an
// rf_repo_missing_out.  Prints PASS; tests/test_repo_check.py runs it plain and
// under AddressSanitizer + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "reflow_hip.h"
#include "repo_check.h"

using namespace rf;

static int failures = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                       \
        }                                                     \
    } while (0)

static void slots() {
    uint64_t s = 0;
    char msg[160] = "";
    CHECK(repo_slots_for(0, &s, msg, sizeof msg) && s == RF_REPO_MIN_SLOTS);
    CHECK(repo_slots_for(512, &s, msg, sizeof msg) && s == 1024);
    CHECK(repo_slots_for(513, &s, msg, sizeof msg) && s == 2048);
    CHECK(repo_slots_for(1000000, &s, msg, sizeof msg) && s == 2097152);
    CHECK(repo_slots_for(1ull << 30, &s, msg, sizeof msg) && s == 1ull << 31);
    CHECK(!repo_slots_for((1ull << 30) + 1, &s, msg, sizeof msg) && msg[0]);
    CHECK(!repo_slots_for(~0ull, &s, msg, sizeof msg));
    CHECK(!repo_slots_for(1, nullptr, msg, sizeof msg));
    CHECK(!repo_slots_for(~0ull, &s, nullptr, 0));  // the message is optional
    for (uint64_t c = 0; c < 5000; ++c) {
        CHECK(repo_slots_for(c, &s, msg, sizeof msg));
        CHECK((s & (s - 1)) == 0 && s >= RF_REPO_MIN_SLOTS && s >= 2 * c && (s == RF_REPO_MIN_SLOTS || s / 2 < 2 * c));
    }
}

static void growth() {
    uint64_t s = 0;
    char msg[160] = "";
    CHECK(repo_growth(1024, 0, 0, 512, &s, msg, sizeof msg) && s == 1024);   // exactly half: stays
    CHECK(repo_growth(1024, 0, 0, 513, &s, msg, sizeof msg) && s == 2048);   // one past: twice the slots
    CHECK(repo_growth(1024, 500, 12, 0, &s, msg, sizeof msg) && s == 1024);
    CHECK(repo_growth(1024, 500, 12, 1, &s, msg, sizeof msg) && s == 2048);  // tombstones count before the rebuild
    CHECK(repo_growth(1024, 10, 510, 1, &s, msg, sizeof msg) && s == 2048);  // ... and not after it
    CHECK(repo_growth(1024, 0, 0, 5000, &s, msg, sizeof msg) && s == 16384);  // doubled until the batch fits
    CHECK(repo_growth(1024, 100, 400, 5000, &s, msg, sizeof msg) && s == 16384);
    CHECK(repo_growth(1ull << 31, 1ull << 29, 0, 1ull << 29, &s, msg, sizeof msg) && s == 1ull << 31);
    CHECK(!repo_growth(1ull << 31, 1ull << 30, 0, 1, &s, msg, sizeof msg) && msg[0]);  // beyond 2^31 slots
    CHECK(!repo_growth(1000, 0, 0, 1, &s, msg, sizeof msg));                             // not a power of two
    CHECK(!repo_growth(512, 0, 0, 1, &s, msg, sizeof msg));                              // below the minimum
    CHECK(!repo_growth(1ull << 32, 0, 0, 1, &s, msg, sizeof msg));
    CHECK(!repo_growth(1024, 2000, 0, 1, &s, msg, sizeof msg));  // more objects than slots
    CHECK(!repo_growth(1024, 600, 600, 1, &s, msg, sizeof msg));
    CHECK(!repo_growth(1024, ~0ull, 1, 1, &s, msg, sizeof msg));  // a sum that would wrap
    CHECK(!repo_growth(1024, 0, 0, (uint64_t)RF_REPO_MAX_ROWS + 1, &s, msg, sizeof msg));
    CHECK(!repo_growth(1024, 0, 0, ~0ull, &s, msg, sizeof msg));
    CHECK(!repo_growth(1024, 0, 0, 1, nullptr, msg, sizeof msg));
    std::mt19937_64 rng(5);
    for (int it = 0; it < 20000; ++it) {
        const uint64_t slots = 1024ull << (rng() % 10);
        const uint64_t live = rng() % (slots / 2 + 1), tomb = rng() % (slots / 2 - live + 1);
        const uint64_t batch = rng() % (4 * slots);
        CHECK(repo_growth(slots, live, tomb, batch, &s, msg, sizeof msg));
        if (2 * (live + tomb + batch) <= slots) {
            CHECK(s == slots);
        } else {
            uint64_t want = 2 * slots;
            while (2 * (live + batch) > want) want *= 2;
            CHECK(s == want);
        }
    }
}

static void rows() {
    uint64_t total = 7;
    char msg[160] = "";
    CHECK(repo_counts_check(nullptr, 0, &total, msg, sizeof msg) && total == 0);
    CHECK(!repo_counts_check(nullptr, 3, &total, msg, sizeof msg) && msg[0] && total == 0);
    const uint32_t some[] = {0, 3, 0, 1025, 0};
    CHECK(repo_counts_check(some, 5, &total, msg, sizeof msg) && total == 1028);
    CHECK(repo_counts_check(some, 5, nullptr, msg, sizeof msg));
    const uint32_t quarter = 1u << 28;
    const uint32_t at[] = {quarter, quarter, quarter, quarter};
    CHECK(repo_counts_check(at, 4, &total, msg, sizeof msg) && total == (uint64_t)RF_REPO_MAX_ROWS);
    const uint32_t past[] = {quarter, quarter, quarter, quarter, 1};
    CHECK(!repo_counts_check(past, 5, &total, msg, sizeof msg) && total == 0);
    // counts whose 64-bit sum is far beyond the limit, and whose 32-bit sum would wrap to a small number
    std::vector<uint32_t> big(5, 0xffffffffu);
    CHECK(!repo_counts_check(big.data(), big.size(), &total, msg, sizeof msg));
    const uint32_t wrap[] = {0x80000000u, 0x80000000u, 5};
    CHECK(!repo_counts_check(wrap, 3, &total, msg, sizeof msg));
    CHECK(repo_rows_check(0, msg, sizeof msg) && repo_rows_check(RF_REPO_MAX_ROWS, msg, sizeof msg));
    CHECK(!repo_rows_check((uint64_t)RF_REPO_MAX_ROWS + 1, msg, sizeof msg) && !repo_rows_check(~0ull, nullptr, 0));
}

static void sizes() {
    char msg[160] = "";
    CHECK(repo_sizes_check(nullptr, 0, msg, sizeof msg));
    CHECK(!repo_sizes_check(nullptr, 2, msg, sizeof msg) && msg[0]);
    const int64_t ok[] = {0, 1, INT64_MAX};
    CHECK(repo_sizes_check(ok, 3, msg, sizeof msg));
    const int64_t bad[] = {0, 1, -1, 5};
    CHECK(!repo_sizes_check(bad, 4, msg, sizeof msg) && std::strstr(msg, "row 2"));
    CHECK(repo_sizes_check(bad, 2, msg, sizeof msg));  // only the rows of the batch are read
    const int64_t low[] = {INT64_MIN};
    CHECK(!repo_sizes_check(low, 1, nullptr, 0));
}

static void outs() {
    char msg[160] = "";
    RepoOutPlan p;
    CHECK(!repo_out_plan(nullptr, true, &p, msg, sizeof msg) && msg[0]);
    rf_repo_missing_out zero{};
    CHECK(!repo_out_plan(&zero, true, nullptr, msg, sizeof msg));
    uint64_t rows_buf[1], n[1];
    uint8_t ids_buf[32];
    int64_t sizes_buf[1];
    // every subset of the three list arrays, both forms, cap 0 and 9
    for (int form = 0; form < 2; ++form)
        for (int mask = 0; mask < 8; ++mask)
            for (uint64_t cap : {0ull, 9ull}) {
                rf_repo_missing_out o{};
                o.cap = cap;
                o.n_listed = n;
                if (mask & 1) o.miss_rows = rows_buf;
                if (mask & 2) o.miss_ids32 = ids_buf;
                if (mask & 4) o.miss_sizes = sizes_buf;
                const bool row_form = form == 0;
                CHECK(repo_out_plan(&o, row_form, &p, msg, sizeof msg));
                const bool rows = row_form && (mask & 1);  // need_transfer never writes miss_rows
                const bool list = rows || (mask & 6);
                CHECK(p.rows == rows && p.list == list && p.cap == (list ? cap : 0));
            }
    // the per-group pointers and n_listed do not make a list
    uint32_t g[1];
    rf_repo_missing_out o{};
    o.n_files = g;
    o.n_missing = g;
    o.cap = 100;
    CHECK(repo_out_plan(&o, true, &p, msg, sizeof msg) && !p.list && !p.rows && p.cap == 0);
    CHECK(repo_out_plan(&zero, false, &p, msg, sizeof msg) && !p.list && p.cap == 0);
}

int main() {
    slots();
    growth();
    rows();
    sizes();
    outs();
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
