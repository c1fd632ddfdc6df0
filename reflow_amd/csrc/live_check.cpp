// live_check.cpp -- HIP-free: the GC liveset's host-only parts (live_check.h).
// rf_bloom_estimate is bloom.EstimateParameters (bloom.go:120-124), the same
// expression in double as the reference evaluates it: the filter's (m, k) are
// part of the wire form, so they are never derived on the device.
#include "live_check.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include "errors.h"
#include "reflow_hip.h"

namespace rf {

static bool refuse(char* err, size_t cap, const char* fmt, ...) {
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, cap, fmt, ap);
        va_end(ap);
    }
    return false;
}

bool bloom_estimate(uint64_t n, double p, uint64_t* m, uint64_t* k, char* err, size_t err_cap) {
    if (!m || !k) return refuse(err, err_cap, "null argument");
    if (n == 0) return refuse(err, err_cap, "n must be positive");
    if (!(p > 0.0 && p < 1.0)) return refuse(err, err_cap, "p must lie in (0, 1)");
    // m = uint(math.Ceil(-1 * float64(n) * math.Log(p) / math.Pow(math.Log(2), 2)))
    const double fm = ceil(-1.0 * (double)n * log(p) / pow(log(2.0), 2.0));
    if (!(fm < 18446744073709551616.0)) return refuse(err, err_cap, "m does not fit 64 bits");
    const uint64_t mm = (uint64_t)fm;
    // k = uint(math.Ceil(math.Log(2) * float64(m) / float64(n)))
    const double fk = ceil(log(2.0) * (double)mm / (double)n);
    *m = mm;
    *k = (uint64_t)fk;
    return true;
}

bool live_values_check(uint64_t n, const uint32_t* nodes, const uint32_t* counts, uint64_t n_nodes,
                       uint64_t arena_rows, uint64_t* total, char* err, size_t err_cap) {
    if (total) *total = 0;
    if (n_nodes && !nodes) return refuse(err, err_cap, "null nodes");
    if (arena_rows > kLiveArenaMaxRows) return refuse(err, err_cap, "arena beyond its bound");
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n_nodes; ++i) {
        if (nodes[i] >= n) return refuse(err, err_cap, "node %u out of range", nodes[i]);
        if (counts) {
            sum += counts[i];  // (no wrap: checked against the bound every step)
            if (sum > kLiveArenaMaxRows - arena_rows)
                return refuse(err, err_cap, "row counts overflow the arena (%llu rows stored)",
                              (unsigned long long)arena_rows);
        }
    }
    if (total) *total = sum;
    return true;
}

void LiveArena::open(uint64_t n) {
    off.assign(n, 0);
    cnt.assign(n, 0);
    has.assign(n, 0);
    rows = stale = cap = 0;
}

uint64_t LiveArena::set(const uint32_t* nodes, const uint32_t* counts, uint64_t n_nodes) {
    const uint64_t base = rows;
    for (uint64_t i = 0; i < n_nodes; ++i) {
        const uint32_t v = nodes[i];
        if (has[v]) stale += cnt[v];
        off[v] = rows;
        cnt[v] = counts[i];
        has[v] = 1;
        rows += counts[i];
    }
    return base;
}

void LiveArena::clear(const uint32_t* nodes, uint64_t n_nodes) {
    for (uint64_t i = 0; i < n_nodes; ++i) {
        const uint32_t v = nodes[i];
        if (has[v]) stale += cnt[v];
        has[v] = 0;
        cnt[v] = 0;
    }
}

uint64_t LiveArena::grown(uint64_t need) const {
    uint64_t c = cap < 1024 ? 1024 : cap;
    while (c < need) c *= 2;  // (need <= 2^48: no wrap)
    return c;
}

}  // namespace rf

extern "C" int rf_bloom_estimate(uint64_t n, double p, uint64_t* m, uint64_t* k) {
    char msg[96];
    if (!rf::bloom_estimate(n, p, m, k, msg, sizeof msg)) return rf::fail(RF_EINVAL, "bloom_estimate: %s", msg);
    return RF_OK;
}
