// plan_check_test.cpp -- the evaluation plan's structural checks
// (reflow_amd/csrc/plan_check.cpp) on their own: no library, no device.
//
// Depth of a chain, a diamond and an empty graph; a self-loop, a 2-cycle and
// a long cycle refused; pointers that are not monotone and deps out of range
// refused; random DAGs against a plain recursive depth; random edge soups
// either refused or given a depth >= 1.  Prints PASS; tests/test_plan_check.py
// runs it plain and under AddressSanitizer + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "plan_check.h"

using rf::plan_check;

struct G {
    std::vector<uint64_t> ptr{0};
    std::vector<uint32_t> deps;
    void node(std::initializer_list<uint32_t> d) {
        deps.insert(deps.end(), d);
        ptr.push_back(deps.size());
    }
    void node(const std::vector<uint32_t>& d) {
        deps.insert(deps.end(), d.begin(), d.end());
        ptr.push_back(deps.size());
    }
    uint64_t n() const { return ptr.size() - 1; }
};

static int failures = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                       \
        }                                                     \
    } while (0)

static bool ok(const G& g, uint32_t* depth) {
    char msg[128] = "";
    const bool r = plan_check(g.n(), g.ptr.data(), g.deps.empty() ? nullptr : g.deps.data(), depth, msg, sizeof msg);
    if (!r) CHECK(msg[0] != 0 && std::strlen(msg) < sizeof msg);
    return r;
}

static uint32_t rec_depth(const G& g, uint32_t v, std::vector<uint32_t>& memo) {
    if (memo[v]) return memo[v];
    uint32_t d = 0;
    for (uint64_t e = g.ptr[v]; e < g.ptr[v + 1]; ++e) d = std::max(d, rec_depth(g, g.deps[e], memo));
    return memo[v] = d + 1;
}

int main() {
    uint32_t depth = 99;
    {  // empty
        CHECK(plan_check(0, nullptr, nullptr, &depth, nullptr, 0) && depth == 0);
        uint64_t p0 = 0;
        CHECK(plan_check(0, &p0, nullptr, &depth, nullptr, 0) && depth == 0);
    }
    {  // one node, no deps; the depth output may be null
        G g;
        g.node({});
        CHECK(ok(g, &depth) && depth == 1);
        CHECK(plan_check(1, g.ptr.data(), nullptr, nullptr, nullptr, 0));
    }
    {  // chain of 1000, listed leaf last
        G g;
        for (uint32_t i = 0; i < 999; ++i) g.node({i + 1});
        g.node({});
        CHECK(ok(g, &depth) && depth == 1000);
    }
    {  // diamond with a dep listed twice, and an unrelated node
        G g;
        g.node({1, 2, 2});
        g.node({3});
        g.node({3});
        g.node({});
        g.node({});
        CHECK(ok(g, &depth) && depth == 3);
    }
    {  // self-loop
        G g;
        g.node({0});
        CHECK(!ok(g, &depth) && depth == 0);
    }
    {  // 2-cycle beneath a clean node
        G g;
        g.node({1});
        g.node({2});
        g.node({1});
        CHECK(!ok(g, &depth));
    }
    {  // long cycle
        G g;
        const uint32_t n = 5000;
        for (uint32_t i = 0; i < n; ++i) g.node({(i + 1) % n});
        CHECK(!ok(g, &depth));
    }
    {  // pointers: first not zero, not monotone
        G g;
        g.node({1});
        g.node({});
        std::vector<uint64_t> bad = g.ptr;
        bad[0] = 1;
        CHECK(!plan_check(2, bad.data(), g.deps.data(), &depth, nullptr, 0));
        uint64_t down[3] = {0, 1, 0};
        char msg[8];
        CHECK(!plan_check(2, down, g.deps.data(), &depth, msg, sizeof msg) && std::strlen(msg) < sizeof msg);
    }
    {  // dep out of range; null deps with edges
        G g;
        g.node({2});
        g.node({});
        CHECK(!ok(g, &depth));
        uint64_t p[2] = {0, 1};
        CHECK(!plan_check(1, p, nullptr, &depth, nullptr, 0));
    }
    std::mt19937 rng(7);
    for (int t = 0; t < 200; ++t) {  // random DAGs: deps point at higher ids, or at lower ones
        G g;
        const uint32_t n = 1 + rng() % 300;
        const bool up = t & 1;
        for (uint32_t i = 0; i < n; ++i) {
            std::vector<uint32_t> d;
            const uint32_t room = up ? n - 1 - i : i;
            if (room)
                for (uint32_t k = rng() % 5; k; --k) d.push_back(up ? i + 1 + rng() % room : rng() % room);
            g.node(d);
        }
        std::vector<uint32_t> memo(n, 0);
        uint32_t want = 0;
        for (uint32_t i = 0; i < n; ++i) want = std::max(want, rec_depth(g, i, memo));
        CHECK(ok(g, &depth) && depth == want);
    }
    int refused = 0, passed = 0;
    for (int t = 0; t < 300; ++t) {  // edge soups
        G g;
        const uint32_t n = 1 + rng() % 40;
        for (uint32_t i = 0; i < n; ++i) {
            std::vector<uint32_t> d;
            for (uint32_t k = rng() % 3; k; --k) d.push_back(rng() % n);
            g.node(d);
        }
        if (ok(g, &depth)) {
            CHECK(depth >= 1 && depth <= n);
            ++passed;
        } else {
            CHECK(depth == 0);
            ++refused;
        }
    }
    CHECK(refused > 0 && passed > 0);
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
