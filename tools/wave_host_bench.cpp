// wave_host_bench.cpp -- the completion step's bookkeeping on host threads
// (tools/wave_probe.py's host baseline): per finished node, one atomic
// decrement of `pending` per consumer entry; the consumers that reach zero are
// collected.  The input file is written by the probe: u64 n, E, B, then
// cons_ptr u64[n+1], cons u32[E], pending u32[n], finished u32[B].
//
//     wave_host_bench FILE [THREADS] [REPS] [FIRST]
//
// FIRST: only the first FIRST finished nodes of the file count.
//
// Prints one JSON line: median / min / max milliseconds over REPS (the pending
// counters are restored between repetitions, outside the timed window) and the
// number of nodes that became ready.  No library, no device.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, uint64_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s FILE [THREADS] [REPS] [FIRST]\n", argv[0]);
        return 2;
    }
    const unsigned threads = argc > 2 ? (unsigned)std::max(1, atoi(argv[2])) : 16;
    const int reps = argc > 3 ? std::max(1, atoi(argv[3])) : 7;
    FILE* f = fopen(argv[1], "rb");
    uint64_t hdr[3];
    if (!f || fread(hdr, 8, 3, f) != 3) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const uint64_t n = hdr[0], E = hdr[1];
    uint64_t B = hdr[2];
    std::vector<uint64_t> cons_ptr;
    std::vector<uint32_t> cons, pending0, finished;
    if (!read_vec(f, cons_ptr, n + 1) || !read_vec(f, cons, E) || !read_vec(f, pending0, n) ||
        !read_vec(f, finished, B)) {
        fprintf(stderr, "short file %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    if (argc > 4) B = std::min<uint64_t>(B, strtoull(argv[4], nullptr, 10));
    std::vector<std::atomic<uint32_t>> pending(n);
    std::vector<std::vector<uint32_t>> ready(threads);
    std::vector<double> ms;
    uint64_t n_ready = 0;
    for (int r = 0; r < reps + 1; ++r) {  // the first repetition is warm-up
        for (uint64_t i = 0; i < n; ++i) pending[i].store(pending0[i], std::memory_order_relaxed);
        for (auto& v : ready) v.clear();
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < threads; ++t)
            pool.emplace_back([&, t] {
                const uint64_t lo = B * t / threads, hi = B * (t + 1) / threads;
                for (uint64_t i = lo; i < hi; ++i) {
                    const uint32_t d = finished[i];
                    for (uint64_t e = cons_ptr[d]; e < cons_ptr[d + 1]; ++e)
                        if (pending[cons[e]].fetch_sub(1, std::memory_order_relaxed) == 1) ready[t].push_back(cons[e]);
                }
            });
        for (auto& th : pool) th.join();
        const auto t1 = std::chrono::steady_clock::now();
        if (r) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        n_ready = 0;
        for (auto& v : ready) n_ready += v.size();
    }
    std::sort(ms.begin(), ms.end());
    printf("{\"threads\": %u, \"finished\": %llu, \"ready\": %llu, \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f}\n",
           threads, (unsigned long long)B, (unsigned long long)n_ready, ms[ms.size() / 2], ms.front(), ms.back());
    return 0;
}
