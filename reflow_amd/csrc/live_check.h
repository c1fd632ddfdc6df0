// live_check.h -- HIP-free parts of the GC liveset (rf_liveset_*, liveset.cpp):
// bloom.EstimateParameters, the argument checks of set_values / clear_values
// and the value arena's offset bookkeeping.  Host only; not part of the public
// ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace rf {

// bloom.go:120-124 in double.  false (with a message) for n = 0 or p outside (0, 1).
bool bloom_estimate(uint64_t n, double p, uint64_t* m, uint64_t* k, char* err, size_t err_cap);

// Rows the arena may ever hold: offsets stay far below 2^63 bytes.
constexpr uint64_t kLiveArenaMaxRows = 1ull << 48;

// nodes[i] < n for every i, and arena_rows + sum(counts) <= kLiveArenaMaxRows
// without wrapping; *total = sum(counts).  counts may be null (clear_values).
bool live_values_check(uint64_t n, const uint32_t* nodes, const uint32_t* counts, uint64_t n_nodes,
                       uint64_t arena_rows, uint64_t* total, char* err, size_t err_cap);

// Where each node's current value lies in the append-only arena.
struct LiveArena {
    std::vector<uint64_t> off;  // [n] first row of node i's value
    std::vector<uint32_t> cnt;  // [n] its rows
    std::vector<uint8_t> has;   // [n] 1: node i has a value
    uint64_t rows = 0;          // rows stored (the next value's first row)
    uint64_t stale = 0;         // rows of replaced / cleared values
    uint64_t cap = 0;           // rows the device arena has room for

    void open(uint64_t n);
    // Appends the values of a checked batch: entry i gets rows [base + sum(counts[0..i)), +counts[i]);
    // returns base.  An older value's rows (an earlier entry of the same node included) become stale.
    uint64_t set(const uint32_t* nodes, const uint32_t* counts, uint64_t n_nodes);
    void clear(const uint32_t* nodes, uint64_t n_nodes);
    // The capacity to grow to for `need` rows in all: doubling, at least 1024.
    uint64_t grown(uint64_t need) const;
};

}  // namespace rf
