// live_check_test.cpp -- the GC liveset's host-only parts
// (reflow_amd/csrc/live_check.cpp) on their own: no library, no device.
//
// bloom.EstimateParameters against the reference's pins and its refusals; the
// argument checks of set_values / clear_values (node range, a row total that
// overflows); the value arena's offset bookkeeping against a plain model under
// random set / replace / clear batches, duplicates in one batch included.
// Prints PASS; tests/test_live_check.py runs it plain and under
// AddressSanitizer + UBSan.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "live_check.h"
#include "reflow_hip.h"

using namespace rf;

static int failures = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                       \
        }                                                     \
    } while (0)

static void estimate() {
    uint64_t m = 0, k = 0;
    char msg[96] = "";
    CHECK(bloom_estimate(1000, 0.001, &m, &k, msg, sizeof msg) && m == 14378 && k == 10);
    CHECK(bloom_estimate(100000000, 0.001, &m, &k, msg, sizeof msg) && m == 1437758757 && k == 10);
    CHECK(bloom_estimate(8, 0.001, &m, &k, msg, sizeof msg) && m == 116 && k == 11);  // TestGC, the intern done
    CHECK(bloom_estimate(7, 0.001, &m, &k, msg, sizeof msg) && m == 101 && k == 11);  // TestGC, the root done
    CHECK(bloom_estimate(1, 0.001, &m, &k, msg, sizeof msg) && m == 15 && k == 11);
    for (uint64_t n = 1; n < 3000; ++n) {  // the expression itself, term by term
        CHECK(bloom_estimate(n, 0.001, &m, &k, msg, sizeof msg));
        const double fm = std::ceil(-1 * double(n) * std::log(0.001) / std::pow(std::log(2.0), 2));
        CHECK(m == (uint64_t)fm && k == (uint64_t)std::ceil(std::log(2.0) * double(m) / double(n)));
    }
    const double bad_p[] = {0.0, 1.0, -0.5, 2.0, NAN};
    for (double p : bad_p) {
        msg[0] = 0;
        CHECK(!bloom_estimate(10, p, &m, &k, msg, sizeof msg) && msg[0]);
    }
    CHECK(!bloom_estimate(0, 0.001, &m, &k, msg, sizeof msg));
    CHECK(!bloom_estimate(10, 0.001, nullptr, &k, msg, sizeof msg));
    CHECK(!bloom_estimate(10, 0.001, &m, nullptr, nullptr, 0));  // the message is optional
    // through the C entry point: the status and rf_last_error
    CHECK(rf_bloom_estimate(1000, 0.001, &m, &k) == RF_OK && m == 14378 && k == 10);
    CHECK(rf_bloom_estimate(0, 0.001, &m, &k) == RF_EINVAL && std::strlen(rf_last_error()) > 0);
    CHECK(rf_bloom_estimate(5, 1.5, &m, &k) == RF_EINVAL);
    CHECK(rf_bloom_estimate(5, 0.5, nullptr, nullptr) == RF_EINVAL);
}

static void checks() {
    char msg[160] = "";
    uint64_t total = 99;
    const uint32_t nodes[] = {0, 4, 4, 2}, counts[] = {3, 0, 7, 1};
    CHECK(live_values_check(5, nodes, counts, 4, 0, &total, msg, sizeof msg) && total == 11);
    CHECK(live_values_check(5, nodes, nullptr, 4, 0, &total, msg, sizeof msg) && total == 0);  // clear_values
    CHECK(live_values_check(5, nullptr, nullptr, 0, 0, &total, msg, sizeof msg) && total == 0);
    CHECK(!live_values_check(4, nodes, counts, 4, 0, &total, msg, sizeof msg) && std::strstr(msg, "out of range"));
    CHECK(!live_values_check(5, nullptr, counts, 4, 0, &total, msg, sizeof msg));
    CHECK(live_values_check(5, nodes, counts, 4, 0, nullptr, nullptr, 0));
    // a row total that overflows the arena's bound, however it is reached
    CHECK(live_values_check(5, nodes, counts, 4, kLiveArenaMaxRows - 11, &total, msg, sizeof msg));
    CHECK(!live_values_check(5, nodes, counts, 4, kLiveArenaMaxRows - 10, &total, msg, sizeof msg) &&
          std::strstr(msg, "overflow"));
    CHECK(!live_values_check(5, nodes, counts, 4, ~0ull, &total, msg, sizeof msg));
    std::vector<uint32_t> many(70000, 0), big(70000, 0xffffffffu);
    CHECK(!live_values_check(1, many.data(), big.data(), many.size(), 0, &total, msg, sizeof msg));  // > 2^48
    CHECK(live_values_check(1, many.data(), big.data(), 60000, 0, &total, msg, sizeof msg) &&
          total == 60000ull * 0xffffffffull);
}

static void arena() {
    std::mt19937 rng(5);
    const uint32_t n = 40;
    LiveArena a;
    a.open(n);
    std::map<uint32_t, std::pair<uint64_t, uint32_t>> model;  // node -> (off, cnt)
    uint64_t rows = 0, stale = 0;
    for (int step = 0; step < 400; ++step) {
        const uint32_t len = rng() % 6;
        std::vector<uint32_t> nodes(len), counts(len);
        for (uint32_t i = 0; i < len; ++i) {
            nodes[i] = rng() % n;  // (duplicates inside a batch happen)
            counts[i] = rng() % 5;
        }
        if (rng() % 4) {
            uint64_t total = 0;
            CHECK(live_values_check(n, nodes.data(), counts.data(), len, a.rows, &total, nullptr, 0));
            const uint64_t base = a.set(nodes.data(), counts.data(), len);
            CHECK(base == rows);
            for (uint32_t i = 0; i < len; ++i) {
                auto it = model.find(nodes[i]);
                if (it != model.end()) stale += it->second.second;
                model[nodes[i]] = {rows, counts[i]};
                rows += counts[i];
            }
            CHECK(a.rows == base + total);
        } else {
            a.clear(nodes.data(), len);
            for (uint32_t v : nodes) {
                auto it = model.find(v);
                if (it != model.end()) {
                    stale += it->second.second;
                    model.erase(it);
                }
            }
        }
        CHECK(a.rows == rows && a.stale == stale);
        uint64_t live_rows = 0;
        for (uint32_t v = 0; v < n; ++v) {
            auto it = model.find(v);
            CHECK((a.has[v] != 0) == (it != model.end()));
            if (it == model.end()) continue;
            CHECK(a.off[v] == it->second.first && a.cnt[v] == it->second.second);
            CHECK(a.off[v] + a.cnt[v] <= a.rows);
            live_rows += a.cnt[v];
        }
        CHECK(live_rows + a.stale == a.rows);  // every stored row is either current or stale
    }
    // growth: doubling from 1024, never below the need
    LiveArena g;
    g.open(1);
    CHECK(g.grown(0) == 1024 && g.grown(1024) == 1024 && g.grown(1025) == 2048);
    g.cap = 4096;
    CHECK(g.grown(10) == 4096 && g.grown(4097) == 8192 && g.grown(100000) == 131072);
    CHECK(g.grown(kLiveArenaMaxRows) == kLiveArenaMaxRows);
}

int main() {
    estimate();
    checks();
    arena();
    if (failures) {
        printf("%d failure(s)\n", failures);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
