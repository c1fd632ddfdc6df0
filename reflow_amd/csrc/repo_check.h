// repo_check.h -- HIP-free parts of the repository index (rf_repo_*, repo.cpp):
// the table's size rules, the argument checks of put / missing /
// need_transfer and what an rf_repo_missing_out asks for.  Host only; not part
// of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "reflow_hip.h"

namespace rf {

constexpr uint64_t kRepoMaxCapacity = 1ull << 30;  // objects asked for at rf_repo_new
constexpr uint64_t kRepoMaxSlots = 1ull << 31;     // slot indices are 32 bits, kEmpty excluded

// Slots for `capacity` objects: the smallest power of two >= max(RF_REPO_MIN_SLOTS, 2 * capacity).
bool repo_slots_for(uint64_t capacity, uint64_t* slots, char* err, size_t err_cap);

// Before a Put batch of `batch` rows: *new_slots = slots when live + tombstones
// + batch fit in half of them; else twice the slots, doubled again until live +
// batch fit in half (the rebuild drops the tombstones).  false beyond kRepoMaxSlots.
bool repo_growth(uint64_t slots, uint64_t live, uint64_t tombstones, uint64_t batch, uint64_t* new_slots, char* err,
                 size_t err_cap);

// *total = sum(counts[0 .. n_groups)) without wrapping, at most RF_REPO_MAX_ROWS.
bool repo_counts_check(const uint32_t* counts, uint64_t n_groups, uint64_t* total, char* err, size_t err_cap);
// A row total the caller states (the device forms) or a call reads back.
bool repo_rows_check(uint64_t n_rows, char* err, size_t err_cap);
// The host form of put: no negative size.
bool repo_sizes_check(const int64_t* sizes, uint64_t n, char* err, size_t err_cap);

// What a call has to produce for an rf_repo_missing_out.
struct RepoOutPlan {
    bool list = false;        // one of the three list arrays is given: the cap rule holds
    bool rows = false;        // miss_rows is written (row form only)
    uint64_t cap = 0;         // list entries that may be written (0 without list arrays)
};
// false for a null struct; every combination of null members is valid.  row_form:
// rf_repo_missing (miss_rows is honoured, status ignored); else need_transfer.
bool repo_out_plan(const rf_repo_missing_out* o, bool row_form, RepoOutPlan* plan, char* err, size_t err_cap);

}  // namespace rf
