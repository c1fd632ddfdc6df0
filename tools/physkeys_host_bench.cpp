// physkeys_host_bench.cpp -- the physical keys' materials built on host threads
// (tools/physkeys_probe.py's baseline: what a caller did before rf_physkeys).
// From the host arrays of rf_fileset_forest_copy: each finished node's Fileset
// material (path ‖ 00 05 ‖ ID over the Maps of the nodes without List children),
// then, for every consumer of a finished node that has a key row, the
// concatenation of its deps' materials and its suffix in one arena at 16-byte
// aligned offsets -- the input of rf_sha256_arena.  The input file is written by
// the probe: u64 n, E, B, NN, NE, PB, S, then dep_ptr u64[n+1], deps u32[E],
// cons_ptr u64[n+1], cons u32[E], phys_row u64[n], suffix_ptr u64[n+1],
// suffix u8[S], finished u32[B], doc_node_ptr u64[B+1], node_depth u32[NN],
// entry_ptr u64[NN+1], path_off u64[NE+1], paths u8[PB], ids32 u8[32 NE].
//
//     physkeys_host_bench FILE OUT [THREADS] [REPS]
//
// Prints one JSON line: median / min / max milliseconds over REPS after one
// warm-up, the consumers found and their material bytes.  OUT receives, outside
// the timed window, u64 K, A, then rows u64[K], offs u64[K], lens u64[K] and the
// arena u8[A], for the probe's rf_sha256_arena and upload.  No library, no device.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, uint64_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

template <class F>
static void parallel(unsigned threads, uint64_t n, F fn) {
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < threads; ++t)
        pool.emplace_back([&, t] { fn(n * t / threads, n * (t + 1) / threads); });
    for (auto& th : pool) th.join();
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s FILE OUT [THREADS] [REPS]\n", argv[0]);
        return 2;
    }
    const unsigned threads = argc > 3 ? (unsigned)std::max(1, atoi(argv[3])) : 16;
    const int reps = argc > 4 ? std::max(1, atoi(argv[4])) : 5;
    FILE* f = fopen(argv[1], "rb");
    uint64_t h[7];
    if (!f || fread(h, 8, 7, f) != 7) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    const uint64_t n = h[0], E = h[1], B = h[2], NN = h[3], NE = h[4], PB = h[5], S = h[6];
    std::vector<uint64_t> dep_ptr, cons_ptr, phys_row, suffix_ptr, doc_node_ptr, entry_ptr, path_off;
    std::vector<uint32_t> deps, cons, finished, node_depth;
    std::vector<uint8_t> suffix, paths, ids;
    if (!read_vec(f, dep_ptr, n + 1) || !read_vec(f, deps, E) || !read_vec(f, cons_ptr, n + 1) || !read_vec(f, cons, E) ||
        !read_vec(f, phys_row, n) || !read_vec(f, suffix_ptr, n + 1) || !read_vec(f, suffix, S) ||
        !read_vec(f, finished, B) || !read_vec(f, doc_node_ptr, B + 1) || !read_vec(f, node_depth, NN) ||
        !read_vec(f, entry_ptr, NN + 1) || !read_vec(f, path_off, NE + 1) || !read_vec(f, paths, PB) ||
        !read_vec(f, ids, 32 * NE)) {
        fprintf(stderr, "short file %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    std::vector<int64_t> val_of(n, -1);  // the finished node's document
    std::vector<std::string> mat(B);
    std::vector<uint8_t> mark(n), arena;
    std::vector<uint64_t> aff, offs, lens;
    std::vector<double> ms;
    for (int r = 0; r < reps + 1; ++r) {  // the first repetition is warm-up
        std::fill(mark.begin(), mark.end(), 0);
        for (auto& m : mat) m.clear();
        const auto t0 = std::chrono::steady_clock::now();
        // the finished nodes' materials
        parallel(threads, B, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t d = lo; d < hi; ++d) {
                std::string& m = mat[d];
                for (uint64_t j = doc_node_ptr[d]; j < doc_node_ptr[d + 1]; ++j) {
                    if (j > doc_node_ptr[d] && node_depth[j - 1] == node_depth[j] + 1) continue;  // List wins
                    for (uint64_t e = entry_ptr[j]; e < entry_ptr[j + 1]; ++e) {
                        m.append(reinterpret_cast<const char*>(paths.data()) + path_off[e], path_off[e + 1] - path_off[e]);
                        m.append("\x00\x05", 2);
                        m.append(reinterpret_cast<const char*>(ids.data()) + 32 * e, 32);
                    }
                }
            }
        });
        for (uint64_t d = 0; d < B; ++d) val_of[finished[d]] = (int64_t)d;
        // the consumers that have a row, ascending
        parallel(threads, B, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t d = lo; d < hi; ++d)
                for (uint64_t e = cons_ptr[finished[d]]; e < cons_ptr[finished[d] + 1]; ++e) mark[cons[e]] = 1;
        });
        aff.clear();
        for (uint64_t i = 0; i < n; ++i)
            if (mark[i] && phys_row[i] != ~0ull) {
                bool ok = true;
                for (uint64_t e = dep_ptr[i]; e < dep_ptr[i + 1]; ++e) ok = ok && val_of[deps[e]] >= 0;
                if (ok) aff.push_back(i);
            }
        // lengths, offsets, the arena
        const uint64_t K = aff.size();
        offs.assign(K, 0);
        lens.assign(K, 0);
        parallel(threads, K, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t k = lo; k < hi; ++k) {
                const uint64_t i = aff[k];
                uint64_t len = suffix_ptr[i + 1] - suffix_ptr[i];
                for (uint64_t e = dep_ptr[i]; e < dep_ptr[i + 1]; ++e) len += mat[(size_t)val_of[deps[e]]].size();
                lens[k] = len;
            }
        });
        uint64_t pos = 0;
        for (uint64_t k = 0; k < K; ++k) {
            offs[k] = pos;
            pos += (lens[k] + 15) & ~15ull;
        }
        arena.assign(pos + 64, 0);
        parallel(threads, K, [&](uint64_t lo, uint64_t hi) {
            for (uint64_t k = lo; k < hi; ++k) {
                const uint64_t i = aff[k];
                uint8_t* o = arena.data() + offs[k];
                for (uint64_t e = dep_ptr[i]; e < dep_ptr[i + 1]; ++e) {
                    const std::string& m = mat[(size_t)val_of[deps[e]]];
                    memcpy(o, m.data(), m.size());
                    o += m.size();
                }
                memcpy(o, suffix.data() + suffix_ptr[i], suffix_ptr[i + 1] - suffix_ptr[i]);
            }
        });
        const auto t1 = std::chrono::steady_clock::now();
        if (r) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        for (uint64_t d = 0; d < B; ++d) val_of[finished[d]] = -1;
    }
    uint64_t bytes = 0;
    for (uint64_t l : lens) bytes += l;
    FILE* o = fopen(argv[2], "wb");
    const uint64_t K = aff.size(), A = arena.size();
    std::vector<uint64_t> rows(K);
    for (uint64_t k = 0; k < K; ++k) rows[k] = phys_row[aff[k]];
    if (!o || fwrite(&K, 8, 1, o) != 1 || fwrite(&A, 8, 1, o) != 1 || (K && fwrite(rows.data(), 8, K, o) != K) ||
        (K && fwrite(offs.data(), 8, K, o) != K) || (K && fwrite(lens.data(), 8, K, o) != K) ||
        fwrite(arena.data(), 1, A, o) != A) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    fclose(o);
    std::sort(ms.begin(), ms.end());
    printf("{\"threads\": %u, \"finished\": %llu, \"consumers\": %llu, \"material_bytes\": %llu, \"median_ms\": %.4f, "
           "\"min_ms\": %.4f, \"max_ms\": %.4f}\n",
           threads, (unsigned long long)B, (unsigned long long)K, (unsigned long long)bytes, ms[ms.size() / 2], ms.front(),
           ms.back());
    return 0;
}
