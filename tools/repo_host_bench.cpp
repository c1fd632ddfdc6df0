// repo_host_bench.cpp -- missing() for a batch of values on the host, beside
// rf_repo_missing_device (the record in DESIGN.md §5 "Repository index").
//
//   repo_host_bench [GROUPS] [ROWS] [THREADS] [REPS]
//
// GROUPS values of ROWS / GROUPS rows each (the liveset probe's distribution:
// random IDs, one row in ten repeats the first row of its value); the
// repository holds every second distinct file.  The host path is what a shim
// would write with the C++ mirror's pieces: the repository as one
// detail::FlatMap<Digest, size> (read only while the batch runs), THREADS
// threads over contiguous ranges of values, per value Files() as a small
// FlatMap of (ID, Size) and one lookup per distinct file.  Both paths are
// timed over the same arrays already in place (host memory / HBM), REPS times
// after a warm-up, and their per-group answers must agree.  Prints one JSON line.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "reflow_host.hpp"

using namespace reflow;

struct FileKey {
    Digest id;
    int64_t size = 0;
    bool operator==(const FileKey& o) const { return id == o.id && size == o.size; }
};
struct FileKeyHash {
    size_t operator()(const FileKey& f) const { return DigestHash{}(f.id) ^ ((uint64_t)f.size * 0x9E3779B97F4A7C15ull); }
};

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static double median(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

int main(int argc, char** argv) {
    const uint64_t G = argc > 1 ? strtoull(argv[1], nullptr, 10) : 332093;
    const uint64_t want_rows = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1000000;
    const unsigned T = argc > 3 ? (unsigned)atoi(argv[3]) : 16;
    const int reps = argc > 4 ? atoi(argv[4]) : 5;
    try {
        // the values
        std::vector<uint32_t> counts(G);
        std::vector<uint64_t> first(G + 1, 0);
        for (uint64_t g = 0; g < G; ++g) {
            counts[g] = (uint32_t)((g + 1) * want_rows / G - g * want_rows / G);
            first[g + 1] = first[g] + counts[g];
        }
        const uint64_t R = first[G];
        std::vector<Digest> ids(R);
        std::vector<int64_t> sizes(R);
        uint64_t seed = 7;
        for (uint64_t g = 0; g < G; ++g)
            for (uint64_t i = first[g]; i < first[g + 1]; ++i) {
                if (i % 10 == 9 && i > first[g]) {
                    ids[i] = ids[first[g]];
                    sizes[i] = sizes[first[g]];
                    continue;
                }
                for (int w = 0; w < 4; ++w) {
                    const uint64_t x = splitmix(seed);
                    memcpy(ids[i].b.data() + 8 * w, &x, 8);
                }
                sizes[i] = (int64_t)(splitmix(seed) & 0x3fffffff);
            }
        // the repository: every second distinct file
        detail::FlatMap<Digest, int64_t, DigestHash> repo;
        std::vector<Digest> held;
        std::vector<int64_t> held_sizes;
        {
            detail::FlatMap<Digest, char, DigestHash> seen;
            seen.reserve(R);
            uint64_t k = 0;
            for (uint64_t i = 0; i < R; ++i) {
                if (seen.find(ids[i])) continue;
                seen.insert(ids[i], 1);
                if (k++ % 2 == 0) {
                    held.push_back(ids[i]);
                    held_sizes.push_back(sizes[i]);
                }
            }
        }
        repo.reserve(held.size());
        for (size_t i = 0; i < held.size(); ++i) repo.insert(held[i], held_sizes[i]);

        // the host path
        std::vector<uint32_t> h_files(G), h_missing(G);
        std::vector<int64_t> h_bytes(G);
        auto host = [&]() {
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < T; ++t)
                pool.emplace_back([&, t]() {
                    const uint64_t lo = G * t / T, hi = G * (t + 1) / T;
                    for (uint64_t g = lo; g < hi; ++g) {
                        detail::FlatMap<FileKey, char, FileKeyHash> files;  // Files(): map[File]bool of this value
                        uint32_t nf = 0, nm = 0;
                        int64_t bytes = 0;
                        for (uint64_t i = first[g]; i < first[g + 1]; ++i) {
                            const FileKey f{ids[i], sizes[i]};
                            if (files.find(f)) continue;
                            files.insert(f, 1);
                            ++nf;
                            if (!repo.find(f.id)) {
                                ++nm;
                                bytes += f.size;
                            }
                        }
                        h_files[g] = nf;
                        h_missing[g] = nm;
                        h_bytes[g] = bytes;
                    }
                });
            for (auto& th : pool) th.join();
        };

        // the device path
        Engine e(0);
        rf_ctx* ctx = e.ctx();
        rf_repo* r = nullptr;
        Check(rf_repo_new(ctx, held.size(), &r));
        std::vector<int32_t> st(held.size() + 1);
        Check(rf_repo_put(r, held.empty() ? nullptr : held[0].b.data(), held_sizes.data(), held.size(), st.data()));
        void *d_counts, *d_ids, *d_sizes, *d_files, *d_missing, *d_bytes, *d_listed;
        Check(rf_malloc(ctx, 4 * G + 4, &d_counts));
        Check(rf_malloc(ctx, 32 * R + 32, &d_ids));
        Check(rf_malloc(ctx, 8 * R + 8, &d_sizes));
        Check(rf_malloc(ctx, 4 * G + 4, &d_files));
        Check(rf_malloc(ctx, 4 * G + 4, &d_missing));
        Check(rf_malloc(ctx, 8 * G + 8, &d_bytes));
        Check(rf_malloc(ctx, 8, &d_listed));
        Check(rf_memcpy_h2d(ctx, d_counts, counts.data(), 4 * G));
        Check(rf_memcpy_h2d(ctx, d_ids, ids[0].b.data(), 32 * R));
        Check(rf_memcpy_h2d(ctx, d_sizes, sizes.data(), 8 * R));
        rf_repo_missing_out o{};
        o.n_files = (uint32_t*)d_files;
        o.n_missing = (uint32_t*)d_missing;
        o.missing_bytes = (int64_t*)d_bytes;
        o.n_listed = (uint64_t*)d_listed;
        auto device = [&]() {
            Check(rf_repo_missing_device(r, d_counts, G, d_ids, d_sizes, R, &o, nullptr));
            Check(rf_sync(ctx));
        };

        std::vector<double> ms_host, ms_dev;
        for (int i = 0; i <= reps; ++i) {  // the first round is warm-up
            auto t0 = std::chrono::steady_clock::now();
            host();
            const double a = ms_since(t0);
            t0 = std::chrono::steady_clock::now();
            device();
            const double b = ms_since(t0);
            if (i) {
                ms_host.push_back(a);
                ms_dev.push_back(b);
            }
        }
        // the check
        std::vector<uint32_t> g_files(G), g_missing(G);
        std::vector<int64_t> g_bytes(G);
        uint64_t listed = 0, total_missing = 0, total_files = 0;
        Check(rf_memcpy_d2h(ctx, g_files.data(), d_files, 4 * G));
        Check(rf_memcpy_d2h(ctx, g_missing.data(), d_missing, 4 * G));
        Check(rf_memcpy_d2h(ctx, g_bytes.data(), d_bytes, 8 * G));
        Check(rf_memcpy_d2h(ctx, &listed, d_listed, 8));
        for (uint64_t g = 0; g < G; ++g) {
            total_missing += h_missing[g];
            total_files += h_files[g];
        }
        const bool same = g_files == h_files && g_missing == h_missing && g_bytes == h_bytes && listed == total_missing;
        for (void* p : {d_counts, d_ids, d_sizes, d_files, d_missing, d_bytes, d_listed}) rf_free(ctx, p);
        rf_repo_destroy(r);
        printf("{\"groups\": %llu, \"rows\": %llu, \"files\": %llu, \"missing_files\": %llu, \"objects\": %zu, "
               "\"threads\": %u, \"reps\": %d, \"host_flatmap_ms\": %.3f, \"missing_device_ms\": %.3f, \"equal\": %s}\n",
               (unsigned long long)G, (unsigned long long)R, (unsigned long long)total_files,
               (unsigned long long)total_missing, held.size(), T, reps, median(ms_host), median(ms_dev),
               same ? "true" : "false");
        return same ? 0 : 1;
    } catch (const Error& err) {
        fprintf(stderr, "FAIL: Error %d: %s\n", err.code, err.what());
        return 1;
    }
}
