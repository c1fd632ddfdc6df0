// asan_assoc_file.cpp -- the assoc's file form (reflow_amd/csrc/assoc_io.cpp)
// under AddressSanitizer + UndefinedBehaviorSanitizer, no GPU and no library:
// `make -C reflow_amd/csrc asan_assoc` links this program with assoc_io.cpp,
// host_sha.cpp and errors.cpp alone.  Every input buffer is a heap block of
// exactly the length handed in, so a read past `len` is a sanitizer report.
// Walks format -> parse round trips, every truncation, every single-bit flip
// of a small file, header fields, and entry-rule violations with recomputed
// checksums; then host_par.h's pool_sort and hash_chunks on a thread pool of
// every width against their serial results; prints PASS.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "assoc_io.h"
#include "host_par.h"
#include "host_sha.h"
#include "reflow_hip.h"

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

struct Entries {
    std::vector<int32_t> kinds;
    std::vector<uint8_t> keys, vals;
    uint64_t n() const { return kinds.size(); }
};

// n entries ascending by (kind, key): kind i / 3, key byte 0 = i
static Entries make(uint64_t n) {
    Entries e;
    for (uint64_t i = 0; i < n; ++i) {
        e.kinds.push_back((int32_t)(i / 3));
        for (int b = 0; b < 32; ++b) {
            e.keys.push_back((uint8_t)(b == 0 ? i : 17 * i + b));
            e.vals.push_back((uint8_t)(1 + ((i * 31 + b) & 0x7f)));
        }
    }
    return e;
}

static std::vector<uint8_t> format(const Entries& e, uint64_t chunk, int want = RF_OK) {
    uint64_t need = 0;
    int rc = rf_assoc_file_format(e.kinds.data(), e.keys.data(), e.vals.data(), e.n(), chunk, nullptr, 0, &need);
    EXPECT(rc == RF_EINVAL && need >= 104, "size query: rc %d need %llu", rc, (unsigned long long)need);
    // a short buffer is refused and not written (the block is exactly need - 1 bytes)
    std::unique_ptr<uint8_t[]> small(new uint8_t[need - 1]);
    rc = rf_assoc_file_format(e.kinds.data(), e.keys.data(), e.vals.data(), e.n(), chunk, small.get(), need - 1, &need);
    EXPECT(rc == RF_EINVAL, "short buffer: rc %d", rc);
    std::vector<uint8_t> out(need);
    rc = rf_assoc_file_format(e.kinds.data(), e.keys.data(), e.vals.data(), e.n(), chunk, out.data(), need, &need);
    EXPECT(rc == want, "format: rc %d, want %d (%s)", rc, want, rf_last_error());
    return out;
}

// parse a copy of buf[0, len) that ends exactly at len
static int parse(const uint8_t* buf, uint64_t len, Entries* out = nullptr, uint64_t cap = 1 << 20) {
    std::unique_ptr<uint8_t[]> exact(new uint8_t[len ? len : 1]);
    if (len) memcpy(exact.get(), buf, len);
    uint64_t n = 0;
    int rc = rf_assoc_file_parse(exact.get(), len, nullptr, nullptr, nullptr, 0, &n);
    if (rc == RF_OK) return n == 0 ? RF_OK : -1;
    if (rc != RF_EINVAL || n == 0) return rc;  // n is set only for a file that passed every check
    Entries e;
    const uint64_t rows = n < cap ? n : cap;
    e.kinds.resize(rows);
    e.keys.resize(32 * rows);
    e.vals.resize(32 * rows);
    rc = rf_assoc_file_parse(exact.get(), len, e.kinds.data(), e.keys.data(), e.vals.data(), rows, &n);
    if (out) *out = e;
    return rc;
}

// the trailer of a file whose entry area was edited: chunk digests, root
static void reseal(std::vector<uint8_t>& f) {
    uint64_t n, chunk;
    memcpy(&n, f.data() + 16, 8);
    memcpy(&chunk, f.data() + 24, 8);
    const uint64_t area = 68 * n, nc = (area + chunk - 1) / chunk;
    uint8_t* d = f.data() + 64 + area;
    for (uint64_t c = 0; c < nc; ++c)
        rf::host_sha256(f.data() + 64 + c * chunk, c * chunk + chunk <= area ? chunk : area - c * chunk, d + 32 * c);
    std::vector<uint8_t> all(64 + 32 * nc);
    memcpy(all.data(), f.data(), 64);
    memcpy(all.data() + 64, d, 32 * nc);
    rf::host_sha256(all.data(), all.size(), d + 32 * nc);
}

// the pool interface host_par.h needs: fn(w) once on each of n threads
struct Threads {
    unsigned n;
    unsigned size() const { return n; }
    void run(const std::function<void(unsigned)>& fn) {
        std::vector<std::thread> th;
        for (unsigned w = 0; w < n; ++w) th.emplace_back(fn, w);
        for (std::thread& t : th) t.join();
    }
};

static void TestPool() {
    // entries in scrambled order, sorted through a permutation as rf_assoc_save does
    for (uint64_t n : {0ull, 1ull, 16384ull, 100000ull, 150001ull}) {
        std::vector<int32_t> kinds(n);
        std::vector<uint8_t> keys(32 * n);
        uint64_t x = 88172645463325252ull + n;
        for (uint64_t i = 0; i < n; ++i) {
            for (int b = 0; b < 32; b += 8) {
                x ^= x << 13, x ^= x >> 7, x ^= x << 17;  // xorshift64
                memcpy(keys.data() + 32 * i + b, &x, 8);
            }
            kinds[i] = (int32_t)(x % 3);
            if (i % 5 == 4) memcpy(keys.data() + 32 * i, keys.data() + 32 * (i - 1), 24);  // long common prefixes
        }
        auto less = [&](uint32_t a, uint32_t b) { return rf::assoc_entry_less(kinds.data(), keys.data(), a, b); };
        std::vector<uint32_t> want(n);
        for (uint64_t i = 0; i < n; ++i) want[i] = (uint32_t)i;
        std::sort(want.begin(), want.end(), less);
        for (unsigned width : {0u, 1u, 2u, 3u, 5u, 7u, 8u, 16u}) {
            std::vector<uint32_t> perm(n);
            for (uint64_t i = 0; i < n; ++i) perm[i] = (uint32_t)i;
            Threads pool{width};
            rf::pool_sort(width ? &pool : nullptr, perm.begin(), perm.end(), less);
            EXPECT(perm == want, "pool_sort of %llu entries on %u threads differs from std::sort", (unsigned long long)n,
                   width);
        }
        // checksums of the key bytes in granules that do and do not divide them
        for (uint64_t chunk : {1000ull, 4096ull, 1ull << 20, ~0ull}) {
            const uint64_t nc = keys.empty() ? 0 : (keys.size() - 1) / chunk + 1;
            std::vector<uint8_t> serial(32 * nc), par(32 * nc + 1, 0xA5);
            rf::assoc_hash_serial(keys.data(), keys.size(), chunk, serial.data());
            Threads pool{5};
            rf::hash_chunks(&pool, keys.data(), keys.size(), chunk, par.data());
            EXPECT(par.back() == 0xA5 && std::equal(serial.begin(), serial.end(), par.begin()),
                   "hash_chunks on a pool differs (n %llu chunk %llu)", (unsigned long long)n, (unsigned long long)chunk);
        }
    }
}

int main() {
    TestPool();
    // round trips over sizes and checksum granules (chunk edges mid-entry and on an entry edge)
    for (uint64_t n : {0, 1, 2, 3, 5, 40})
        for (uint64_t chunk : {0, 1, 67, 68, 100, 68 * 3, 1 << 20}) {
            const Entries e = make(n);
            const std::vector<uint8_t> f = format(e, chunk);
            Entries g;
            const int rc = parse(f.data(), f.size(), &g);
            EXPECT(rc == RF_OK, "round trip n %llu chunk %llu: rc %d (%s)", (unsigned long long)n,
                   (unsigned long long)chunk, rc, rf_last_error());
            EXPECT(n == 0 || (g.kinds == e.kinds && g.keys == e.keys && g.vals == e.vals), "round trip differs");
            if (n > 1) {  // short entry buffers: refused, rows past them untouched (exact-size blocks)
                EXPECT(parse(f.data(), f.size(), nullptr, n - 1) == RF_EINVAL, "short cap_entries accepted");
            }
        }
    const Entries e3 = make(3);
    for (uint64_t chunk : {0, 100, 68 * 3}) {
        const std::vector<uint8_t> f = format(e3, chunk);
        // every truncation, and the file with bytes appended
        for (uint64_t len = 0; len < f.size(); ++len)
            EXPECT(parse(f.data(), len) == RF_EINVAL, "truncation to %llu accepted", (unsigned long long)len);
        std::vector<uint8_t> longer = f;
        longer.push_back(0);
        EXPECT(parse(longer.data(), longer.size()) == RF_EINVAL, "a trailing byte accepted");
        // every single-bit flip is refused; one inside the entries is an integrity error
        for (uint64_t bit = 0; bit < 8 * f.size(); ++bit) {
            std::vector<uint8_t> g = f;
            g[bit / 8] ^= (uint8_t)(1u << (bit % 8));
            const int rc = parse(g.data(), g.size());
            const bool in_entries = bit / 8 >= 64 && bit / 8 < 64 + 68 * 3;
            EXPECT(in_entries ? rc == RF_EINTEGRITY : (rc == RF_EINVAL || rc == RF_EINTEGRITY),
                   "bit %llu flipped: rc %d", (unsigned long long)bit, rc);
        }
    }
    {  // header fields (checked before any checksum): magic, version, flags, granule, entry count
        const std::vector<uint8_t> f = format(e3, 100);
        auto with = [&](size_t off, uint64_t v, size_t bytes) {
            std::vector<uint8_t> g = f;
            memcpy(g.data() + off, &v, bytes);
            return g;
        };
        for (auto g : {with(0, 0x3143, 2), with(8, 2, 4), with(8, 0, 4), with(12, 1, 4), with(24, 0, 8),
                       with(16, 4, 8), with(16, ~0ull, 8), with(16, 1ull << 62, 8), with(24, 1, 8),
                       with(24, ~0ull, 8)}) {
            EXPECT(parse(g.data(), g.size()) == RF_EINVAL, "bad header field accepted: rc %d", parse(g.data(), g.size()));
        }
        std::vector<uint8_t> g = f;
        g[g.size() - 1] ^= 1;
        EXPECT(parse(g.data(), g.size()) == RF_EINVAL, "bad end marker accepted");
    }
    {  // entry rules, checksums recomputed: zero value, unsorted, duplicate, kind out of range
        const std::vector<uint8_t> f = format(e3, 100);
        std::vector<uint8_t> g = f;
        memset(g.data() + 64 + 68 + 36, 0, 32);
        reseal(g);
        EXPECT(parse(g.data(), g.size()) == RF_EINVAL, "zero value accepted");
        g = f;
        std::swap_ranges(g.begin() + 64, g.begin() + 64 + 68, g.begin() + 64 + 68);
        reseal(g);
        EXPECT(parse(g.data(), g.size()) == RF_EINVAL, "unsorted pair accepted");
        g = f;
        memcpy(g.data() + 64 + 68, g.data() + 64, 36);
        reseal(g);
        EXPECT(parse(g.data(), g.size()) == RF_EINVAL, "duplicate (kind, key) accepted");
        for (uint32_t kind : {0xffffffffu, 0x80000000u, 1u << 30}) {
            g = f;
            memcpy(g.data() + 64 + 2 * 68, &kind, 4);
            reseal(g);
            EXPECT(parse(g.data(), g.size()) == RF_EINVAL, "kind %#x accepted", kind);
        }
        g = f;
        reseal(g);
        EXPECT(g == f && parse(g.data(), g.size()) == RF_OK, "resealing an untouched file changes it");
        // format applies the same rules to what it is given
        Entries bad = e3;
        std::swap(bad.kinds[0], bad.kinds[2]);
        bad.kinds[1] = 5;
        format(bad, 100, RF_EINVAL);
        bad = e3;
        memset(bad.vals.data() + 32, 0, 32);
        format(bad, 100, RF_EINVAL);
    }
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("PASS\n");
    return 0;
}
