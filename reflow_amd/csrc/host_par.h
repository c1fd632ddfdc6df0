// host_par.h -- internal: the two host-side jobs the checkpoint files
// (graph_io.cpp, the assoc file of assoc_io.cpp) spread over the host pool:
// per-chunk SHA-256 checksums and a sort.  Templates over the pool type (any
// class with size() and run(fn(worker))), so the HIP-free units can include
// this without host_leg.h's HIP headers; a null pool runs on the caller.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "host_sha.h"

namespace rf {

// SHA-256 of each `chunk`-byte granule of buf[0, n) into out (32 B each, in
// order), on the pool when there is one.
template <class Pool>
void hash_chunks(Pool* pool, const uint8_t* buf, uint64_t n, uint64_t chunk, uint8_t* out) {
    const uint64_t nc = n ? (n - 1) / chunk + 1 : 0;  // (no n + chunk: a file may name any granule)
    if (!pool || nc < 2) {
        for (uint64_t c = 0; c < nc; ++c) host_sha256(buf + c * chunk, std::min(chunk, n - c * chunk), out + 32 * c);
        return;
    }
    std::atomic<uint64_t> next{0};
    pool->run([&](unsigned) {
        for (uint64_t c; (c = next.fetch_add(1)) < nc;)
            host_sha256(buf + c * chunk, std::min(chunk, n - c * chunk), out + 32 * c);
    });
}

// std::sort of [first, last) by less: one run per worker sorted on the pool,
// then rounds of pairwise merges (also on the pool).
template <class Pool, class It, class Less>
void pool_sort(Pool* pool, It first, It last, Less less) {
    const uint64_t n = (uint64_t)(last - first);
    const uint64_t runs = pool ? std::min<uint64_t>(pool->size(), n >> 14) : 0;  // a run is >= 16k items
    if (runs < 2) {
        std::sort(first, last, less);
        return;
    }
    std::vector<uint64_t> cut(runs + 1);
    for (uint64_t r = 0; r <= runs; ++r) cut[r] = n * r / runs;
    std::atomic<uint64_t> next{0};
    pool->run([&](unsigned) {
        for (uint64_t r; (r = next.fetch_add(1)) < runs;) std::sort(first + cut[r], first + cut[r + 1], less);
    });
    for (uint64_t w = 1; w < runs; w *= 2) {  // merge runs [r, r + w) and [r + w, r + 2w)
        next = 0;
        pool->run([&](unsigned) {
            for (uint64_t p; (p = next.fetch_add(1)) * 2 * w + w < runs;) {
                const uint64_t r = p * 2 * w;
                std::inplace_merge(first + cut[r], first + cut[r + w], first + cut[std::min(r + 2 * w, runs)], less);
            }
        });
    }
}

}  // namespace rf
