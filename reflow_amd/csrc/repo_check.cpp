// repo_check.cpp -- HIP-free: the repository index's host-only parts (repo_check.h).
#include "repo_check.h"

#include <stdarg.h>
#include <stdio.h>

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

bool repo_slots_for(uint64_t capacity, uint64_t* slots, char* err, size_t err_cap) {
    if (!slots) return refuse(err, err_cap, "null argument");
    if (capacity > kRepoMaxCapacity) return refuse(err, err_cap, "capacity beyond 2^30 objects");
    uint64_t s = RF_REPO_MIN_SLOTS;
    while (s < 2 * capacity) s <<= 1;  // (capacity <= 2^30: no wrap)
    *slots = s;
    return true;
}

bool repo_growth(uint64_t slots, uint64_t live, uint64_t tombstones, uint64_t batch, uint64_t* new_slots, char* err,
                 size_t err_cap) {
    if (!new_slots) return refuse(err, err_cap, "null argument");
    if (slots < RF_REPO_MIN_SLOTS || slots > kRepoMaxSlots || (slots & (slots - 1)))
        return refuse(err, err_cap, "slots must be a power of two in [%d, 2^31]", RF_REPO_MIN_SLOTS);
    if (live > slots || tombstones > slots || live + tombstones > slots)
        return refuse(err, err_cap, "more objects than slots");
    if (batch > RF_REPO_MAX_ROWS) return refuse(err, err_cap, "more than 2^30 rows in one batch");
    *new_slots = slots;
    if (2 * (live + tombstones + batch) <= slots) return true;  // (each term <= 2^31: no wrap)
    uint64_t s = slots;
    do {
        if (s >= kRepoMaxSlots) return refuse(err, err_cap, "the table would exceed 2^31 slots");
        s <<= 1;
    } while (2 * (live + batch) > s);
    *new_slots = s;
    return true;
}

bool repo_rows_check(uint64_t n_rows, char* err, size_t err_cap) {
    if (n_rows > RF_REPO_MAX_ROWS)
        return refuse(err, err_cap, "%llu rows in one call (at most 2^30)", (unsigned long long)n_rows);
    return true;
}

bool repo_counts_check(const uint32_t* counts, uint64_t n_groups, uint64_t* total, char* err, size_t err_cap) {
    if (total) *total = 0;
    if (n_groups && !counts) return refuse(err, err_cap, "null counts");
    uint64_t sum = 0;
    for (uint64_t g = 0; g < n_groups; ++g) {
        sum += counts[g];  // (no wrap: checked against the bound every step)
        if (sum > RF_REPO_MAX_ROWS)
            return refuse(err, err_cap, "more than 2^30 rows in one call (group %llu)", (unsigned long long)g);
    }
    if (total) *total = sum;
    return true;
}

bool repo_sizes_check(const int64_t* sizes, uint64_t n, char* err, size_t err_cap) {
    if (n && !sizes) return refuse(err, err_cap, "null sizes");
    for (uint64_t i = 0; i < n; ++i)
        if (sizes[i] < 0)
            return refuse(err, err_cap, "row %llu has the negative size %lld", (unsigned long long)i,
                          (long long)sizes[i]);
    return true;
}

bool repo_out_plan(const rf_repo_missing_out* o, bool row_form, RepoOutPlan* plan, char* err, size_t err_cap) {
    if (!o || !plan) return refuse(err, err_cap, "null argument");
    RepoOutPlan p;
    p.rows = row_form && o->miss_rows != nullptr;
    p.list = p.rows || o->miss_ids32 != nullptr || o->miss_sizes != nullptr;
    p.cap = p.list ? o->cap : 0;
    *plan = p;
    return true;
}

}  // namespace rf
