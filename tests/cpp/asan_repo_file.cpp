// asan_repo_file.cpp -- the repository index's file form
// (reflow_amd/csrc/repo_io.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer, no GPU and no library: `make -C reflow_amd/csrc
// asan_repo` links this program with repo_io.cpp, host_sha.cpp and errors.cpp
// alone.  Every input buffer is a heap block of exactly the length handed in,
// so a read past `len` is a sanitizer report.  Walks format -> parse round
// trips with short buffers, every truncation and every single-bit flip of a
// 7-entry file, header fields, rule violations with recomputed checksums, and
// a few thousand seeded random corruptions; prints PASS.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <vector>

#include "host_sha.h"
#include "reflow_hip.h"
#include "repo_io.h"

static int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            ++failures;                                     \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
        }                                                   \
    } while (0)

struct Objects {
    std::vector<uint8_t> ids;
    std::vector<int64_t> sizes;
    uint64_t n() const { return sizes.size(); }
};

// n objects ascending by ID: byte 0 = i
static Objects make(uint64_t n) {
    Objects o;
    for (uint64_t i = 0; i < n; ++i) {
        for (int b = 0; b < 32; ++b) o.ids.push_back((uint8_t)(b == 0 ? i : 17 * i + b));
        o.sizes.push_back((int64_t)(i * 1000003 % 65537));
    }
    return o;
}

static std::vector<uint8_t> format(const Objects& o, uint64_t chunk, int want = RF_OK) {
    uint64_t need = 0;
    int rc = rf_repo_file_format(o.ids.data(), o.sizes.data(), o.n(), chunk, nullptr, 0, &need);
    EXPECT(rc == RF_EINVAL && need >= 104, "size query: rc %d need %llu", rc, (unsigned long long)need);
    // a short buffer is refused and not written (the block is exactly need - 1 bytes), the length still set
    std::unique_ptr<uint8_t[]> small(new uint8_t[need - 1]);
    uint64_t need2 = 0;
    rc = rf_repo_file_format(o.ids.data(), o.sizes.data(), o.n(), chunk, small.get(), need - 1, &need2);
    EXPECT(rc == RF_EINVAL && need2 == need, "short buffer: rc %d", rc);
    std::vector<uint8_t> out(need);
    rc = rf_repo_file_format(o.ids.data(), o.sizes.data(), o.n(), chunk, out.data(), need, &need);
    EXPECT(rc == want, "format: rc %d, want %d (%s)", rc, want, rf_last_error());
    return out;
}

// parse a copy of buf[0, len) that ends exactly at len
static int parse(const uint8_t* buf, uint64_t len, Objects* out = nullptr, uint64_t cap = 1 << 20) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) memcpy(exact.get(), buf, len);
    uint64_t n = 0;
    int rc = rf_repo_file_parse(exact.get(), len, nullptr, nullptr, 0, &n);
    if (rc == RF_OK) return n == 0 ? RF_OK : -1;
    if (rc != RF_EINVAL || n == 0) return rc;  // n is set only for a file that passed every check
    Objects o;
    const uint64_t rows = n < cap ? n : cap;
    o.ids.resize(32 * rows);
    o.sizes.resize(rows);
    uint64_t n2 = 0;
    rc = rf_repo_file_parse(exact.get(), len, o.ids.data(), o.sizes.data(), rows, &n2);
    if (n2 != n) return -2;  // the count is set whether the rows fit or not
    if (out) *out = o;
    return rc;
}
static int parse(const std::vector<uint8_t>& f) { return parse(f.data(), f.size()); }

// the header's total and the trailer of a file whose entry area was edited
static void reseal(std::vector<uint8_t>& f, bool fix_total = true) {
    uint64_t n, chunk;
    memcpy(&n, f.data() + 16, 8);
    memcpy(&chunk, f.data() + 24, 8);
    const uint64_t area = 40 * n, nc = (area + chunk - 1) / chunk;
    if (fix_total) {
        uint64_t total = 0;  // (wraps as the bytes say; the checker must not)
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t s;
            memcpy(&s, f.data() + 64 + 40 * i + 32, 8);
            total += s;
        }
        memcpy(f.data() + 32, &total, 8);
    }
    uint8_t* d = f.data() + 64 + area;
    for (uint64_t c = 0; c < nc; ++c)
        rf::host_sha256(f.data() + 64 + c * chunk, c * chunk + chunk <= area ? chunk : area - c * chunk, d + 32 * c);
    std::vector<uint8_t> all(64 + 32 * nc);
    memcpy(all.data(), f.data(), 64);
    memcpy(all.data() + 64, d, 32 * nc);
    rf::host_sha256(all.data(), all.size(), d + 32 * nc);
}

int main() {
    // round trips over sizes and checksum granules (chunk edges mid-entry and on an entry edge)
    for (uint64_t n : {0, 1, 2, 3, 7, 40})
        for (uint64_t chunk : {0, 1, 39, 40, 80, 100, 40 * 7, 1 << 20}) {
            const Objects o = make(n);
            const std::vector<uint8_t> f = format(o, chunk);
            Objects g;
            const int rc = parse(f.data(), f.size(), &g);
            EXPECT(rc == RF_OK, "round trip n %llu chunk %llu: rc %d (%s)", (unsigned long long)n,
                   (unsigned long long)chunk, rc, rf_last_error());
            EXPECT(n == 0 || (g.ids == o.ids && g.sizes == o.sizes), "round trip differs");
            if (n > 1)  // short entry buffers: refused, rows past them untouched (exact-size blocks)
                EXPECT(parse(f.data(), f.size(), nullptr, n - 1) == RF_EINVAL, "short cap_entries accepted");
        }
    const Objects o7 = make(7);
    const uint64_t area0 = 64;
    for (uint64_t chunk : {0, 80, 100, 40 * 7}) {
        const std::vector<uint8_t> f = format(o7, chunk);
        const uint64_t nc = chunk ? (40 * 7 + chunk - 1) / chunk : 1;
        EXPECT(f.size() == 64 + 280 + 32 * nc + 40, "file of %llu bytes", (unsigned long long)f.size());
        // every truncation, and the file with a byte appended
        for (uint64_t len = 0; len < f.size(); ++len)
            EXPECT(parse(f.data(), len) == RF_EINVAL, "truncation to %llu accepted", (unsigned long long)len);
        std::vector<uint8_t> longer = f;
        longer.push_back(0);
        EXPECT(parse(longer) == RF_EINVAL, "a trailing byte accepted");
        // every single-bit flip is refused; entries and digests: an integrity error; the end marker,
        // magic, version, flags, entry count and reserved bytes: structure
        for (uint64_t bit = 0; bit < 8 * f.size(); ++bit) {
            std::vector<uint8_t> g = f;
            g[bit / 8] ^= (uint8_t)(1u << (bit % 8));
            const int rc = parse(g);
            const uint64_t at = bit / 8;
            int want = 0;  // either
            if (at >= area0 && at < f.size() - 8) want = RF_EINTEGRITY;
            else if (at >= f.size() - 8 || at < 24 || (at >= 40 && at < 64)) want = RF_EINVAL;
            else if (at >= 32 && at < 40) want = RF_EINTEGRITY;  // total_bytes: only the header checksum sees it
            EXPECT(want ? rc == want : (rc == RF_EINVAL || rc == RF_EINTEGRITY), "bit %llu flipped: rc %d, want %d",
                   (unsigned long long)bit, rc, want);
        }
    }
    {  // header fields (checked before any checksum)
        const std::vector<uint8_t> f = format(o7, 80);
        auto with = [&](size_t off, uint64_t v, size_t bytes) {
            std::vector<uint8_t> g = f;
            memcpy(g.data() + off, &v, bytes);
            return g;
        };
        for (auto g : {with(0, 0x3143, 2), with(8, 2, 4), with(8, 0, 4), with(12, 1, 4), with(24, 0, 8),
                       with(16, 8, 8), with(16, ~0ull, 8), with(16, 1ull << 61, 8), with(16, 1ull << 62, 8),
                       with(24, 1, 8), with(24, ~0ull, 8), with(40, 1, 1), with(63, 0x80, 1)})
            EXPECT(parse(g) == RF_EINVAL, "bad header field accepted: rc %d", parse(g));
        std::vector<uint8_t> small(f.begin(), f.begin() + 200);  // 2^61 entries in a 200-byte file
        const uint64_t huge = 1ull << 61;
        memcpy(small.data() + 16, &huge, 8);
        EXPECT(parse(small) == RF_EINVAL, "2^61 entries in 200 bytes accepted");
    }
    {  // entry rules, checksums recomputed
        const std::vector<uint8_t> f = format(o7, 80);
        std::vector<uint8_t> g = f;
        reseal(g);
        EXPECT(g == f && parse(g) == RF_OK, "resealing an untouched file changes it");
        memcpy(g.data() + area0 + 40, g.data() + area0, 32);
        reseal(g);
        EXPECT(parse(g) == RF_EINVAL, "two equal IDs accepted");
        g = f;
        std::swap_ranges(g.begin() + area0, g.begin() + area0 + 40, g.begin() + area0 + 40);
        reseal(g);
        EXPECT(parse(g) == RF_EINVAL, "descending IDs accepted");
        g = f;
        const int64_t neg = -1;
        memcpy(g.data() + area0 + 2 * 40 + 32, &neg, 8);
        reseal(g);
        EXPECT(parse(g) == RF_EINVAL, "a negative size accepted");
        for (int64_t d : {-1, 1}) {
            g = f;
            int64_t t;
            memcpy(&t, g.data() + 32, 8);
            t += d;
            memcpy(g.data() + 32, &t, 8);
            reseal(g, false);
            EXPECT(parse(g) == RF_EINVAL, "total_bytes off by %lld accepted", (long long)d);
        }
        g = f;
        const int64_t big = INT64_MAX;
        memcpy(g.data() + area0 + 32, &big, 8);
        memcpy(g.data() + area0 + 40 + 32, &big, 8);
        reseal(g);  // (the wrapped sum in the header: the running sum must be checked, not the result)
        EXPECT(parse(g) == RF_EINVAL, "sizes that overflow int64 accepted");
        // format applies the same rules to what it is given
        Objects bad = o7;
        std::swap_ranges(bad.ids.begin(), bad.ids.begin() + 32, bad.ids.begin() + 32);
        format(bad, 80, RF_EINVAL);
        bad = o7;
        bad.sizes[3] = -5;
        format(bad, 80, RF_EINVAL);
        bad = o7;
        bad.sizes[0] = bad.sizes[6] = INT64_MAX;
        format(bad, 80, RF_EINVAL);
    }
    {  // seeded random corruptions: bytes overwritten, runs zeroed, cut and extended; never accepted unless unchanged
        const std::vector<uint8_t> f = format(o7, 100);
        uint64_t x = 0x9E3779B97F4A7C15ull;
        auto rnd = [&]() {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;  // xorshift64
            return x;
        };
        for (int it = 0; it < 4000; ++it) {
            std::vector<uint8_t> g = f;
            switch (rnd() % 4) {
            case 0:
                for (uint64_t k = 1 + rnd() % 4; k; --k) g[rnd() % g.size()] = (uint8_t)rnd();
                break;
            case 1: {
                const uint64_t a = rnd() % g.size(), l = 1 + rnd() % 64;
                for (uint64_t i = a; i < g.size() && i < a + l; ++i) g[i] = 0;
                break;
            }
            case 2:
                g.resize(rnd() % (g.size() + 1));
                for (uint64_t k = rnd() % 3; k && !g.empty(); --k) g[rnd() % g.size()] ^= (uint8_t)(1u << (rnd() % 8));
                break;
            default: {
                const uint64_t off = 8 * (1 + rnd() % 4), v = rnd() >> (rnd() % 64);  // a header word
                memcpy(g.data() + off, &v, 8);
                if (off == 32 && (rnd() & 1)) reseal(g, false);  // a wrong total under valid checksums
                break;
            }
            }
            const int rc = parse(g);
            EXPECT(g == f ? rc == RF_OK : (rc == RF_EINVAL || rc == RF_EINTEGRITY), "corruption %d: rc %d", it, rc);
        }
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
