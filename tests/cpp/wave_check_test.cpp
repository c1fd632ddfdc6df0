// wave_check_test.cpp -- the evaluation waves' consumer CSR
// (reflow_amd/csrc/wave_check.cpp) on its own: no library, no device.
//
// Empty graphs and a single node; a chain; a diamond with a dep listed twice
// (two consumer entries); a node with 0 / 63 / 64 / 65 / 130 consumers; random
// DAGs against a naive inversion, consumers ascending within a node; null
// pointers, pointers that are not monotone and deps out of range refused with
// the outputs untouched.  Prints PASS; tests/test_wave_check.py runs it plain
// and under AddressSanitizer + UBSan.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "wave_check.h"

using rf::wave_consumers;

struct G {
    std::vector<uint64_t> ptr{0};
    std::vector<uint32_t> deps;
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

struct C {
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> cons;
    std::vector<uint32_t> of(uint32_t d) const { return {cons.begin() + ptr[d], cons.begin() + ptr[d + 1]}; }
};

// exactly sized outputs: a write past either end is the sanitizers' to find
static bool invert(const G& g, C* out) {
    out->ptr.assign(g.n() + 1, 0xdeadbeef);
    out->cons.assign(g.deps.size(), 0xdeadbeef);
    char msg[128] = "";
    const bool r = wave_consumers(g.n(), g.ptr.data(), g.deps.empty() ? nullptr : g.deps.data(), out->ptr.data(),
                                  out->cons.empty() ? nullptr : out->cons.data(), msg, sizeof msg);
    if (!r) {
        CHECK(msg[0] != 0 && std::strlen(msg) < sizeof msg);
        for (uint64_t p : out->ptr) CHECK(p == 0xdeadbeef);  // nothing written on a refusal
        for (uint32_t c : out->cons) CHECK(c == 0xdeadbeef);
    }
    return r;
}

static void check_against_naive(const G& g) {
    C c;
    CHECK(invert(g, &c));
    std::vector<std::vector<uint32_t>> want(g.n());
    for (uint32_t i = 0; i < g.n(); ++i)
        for (uint64_t e = g.ptr[i]; e < g.ptr[i + 1]; ++e) want[g.deps[e]].push_back(i);
    CHECK(c.ptr[0] == 0 && c.ptr[g.n()] == g.deps.size());
    for (uint32_t d = 0; d < g.n(); ++d) {
        CHECK(c.ptr[d] <= c.ptr[d + 1]);
        const std::vector<uint32_t> got = c.of(d);
        CHECK(got == want[d]);
        CHECK(std::is_sorted(got.begin(), got.end()));
    }
}

int main() {
    {  // empty: n = 0 writes cons_ptr[0] and nothing else; dep_ptr may be null
        uint64_t cp[2] = {7, 7};
        CHECK(wave_consumers(0, nullptr, nullptr, cp, nullptr, nullptr, 0) && cp[0] == 0 && cp[1] == 7);
        uint64_t p0 = 0;
        cp[0] = 7;
        CHECK(wave_consumers(0, &p0, nullptr, cp, nullptr, nullptr, 0) && cp[0] == 0);
    }
    {  // n = 1, no deps
        G g;
        g.node({});
        C c;
        CHECK(invert(g, &c) && c.ptr == std::vector<uint64_t>({0, 0}));
    }
    {  // chain of 1000, leaf last: node i + 1 has the one consumer i
        G g;
        for (uint32_t i = 0; i < 999; ++i) g.node({i + 1});
        g.node({});
        C c;
        CHECK(invert(g, &c));
        CHECK(c.of(0).empty());
        for (uint32_t i = 1; i < 1000; ++i) CHECK(c.of(i) == std::vector<uint32_t>({i - 1}));
        check_against_naive(g);
    }
    {  // diamond with a dep listed twice, and an unrelated node
        G g;
        g.node({1, 2, 2});
        g.node({3});
        g.node({3});
        g.node({});
        g.node({});
        C c;
        CHECK(invert(g, &c));
        CHECK(c.of(0).empty() && c.of(4).empty());
        CHECK(c.of(1) == std::vector<uint32_t>({0}));
        CHECK(c.of(2) == std::vector<uint32_t>({0, 0}));  // two entries
        CHECK(c.of(3) == std::vector<uint32_t>({1, 2}));
        CHECK(c.ptr == std::vector<uint64_t>({0, 0, 1, 3, 5, 5}));
    }
    for (uint32_t k : {0u, 63u, 64u, 65u, 130u}) {  // one node with k consumers, listed before and after it
        G g;
        const uint32_t d = k / 2;  // the shared dep sits in the middle
        for (uint32_t i = 0; i < k + 1; ++i) g.node(i == d ? std::vector<uint32_t>{} : std::vector<uint32_t>{d});
        C c;
        CHECK(invert(g, &c));
        CHECK(c.of(d).size() == k);
        for (uint32_t i = 0; i < k + 1; ++i)
            if (i != d) CHECK(c.of(i).empty());
        check_against_naive(g);
    }
    {  // refusals
        G g;
        g.node({1});
        g.node({});
        C c;
        std::vector<uint64_t> cp(3, 5);
        std::vector<uint32_t> co(1, 5);
        CHECK(!wave_consumers(2, g.ptr.data(), g.deps.data(), nullptr, co.data(), nullptr, 0));   // null cons_ptr
        CHECK(!wave_consumers(2, nullptr, g.deps.data(), cp.data(), co.data(), nullptr, 0));       // null dep_ptr
        CHECK(!wave_consumers(2, g.ptr.data(), nullptr, cp.data(), co.data(), nullptr, 0));        // null deps
        CHECK(!wave_consumers(2, g.ptr.data(), g.deps.data(), cp.data(), nullptr, nullptr, 0));    // null cons
        std::vector<uint64_t> bad = g.ptr;
        bad[0] = 1;
        CHECK(!wave_consumers(2, bad.data(), g.deps.data(), cp.data(), co.data(), nullptr, 0));    // first not zero
        uint64_t down[3] = {0, 1, 0};
        char msg[8];
        CHECK(!wave_consumers(2, down, g.deps.data(), cp.data(), co.data(), msg, sizeof msg) &&
              std::strlen(msg) < sizeof msg);                                                      // not monotone
        CHECK(!wave_consumers(1ull << 32, g.ptr.data(), g.deps.data(), cp.data(), co.data(), nullptr, 0));
        CHECK(cp == std::vector<uint64_t>(3, 5) && co[0] == 5);
        G r;
        r.node({2});  // dep out of range
        r.node({});
        CHECK(!invert(r, &c));
        G last;
        last.node({});
        last.node({0, 2});  // out of range after a good entry
        CHECK(!invert(last, &c));
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
                for (uint32_t k = rng() % 6; k; --k) d.push_back(up ? i + 1 + rng() % room : rng() % room);
            g.node(d);
        }
        check_against_naive(g);
    }
    for (int t = 0; t < 100; ++t) {  // edge soups (cycles are not this unit's business) and bad ones
        G g;
        const uint32_t n = 1 + rng() % 40;
        bool in_range = true;
        for (uint32_t i = 0; i < n; ++i) {
            std::vector<uint32_t> d;
            for (uint32_t k = rng() % 3; k; --k) {
                d.push_back(rng() % (n + (t % 4 == 0)));
                in_range = in_range && d.back() < n;
            }
            g.node(d);
        }
        C c;
        if (in_range)
            check_against_naive(g);
        else
            CHECK(!invert(g, &c));
    }
    if (failures) return 1;
    printf("PASS\n");
    return 0;
}
