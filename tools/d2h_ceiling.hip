// d2h_ceiling.hip -- diagnostic: the D2H link's ceiling for the host leg's kind
// of traffic, with no kernel running and nothing hashed.  T threads x K streams
// (default 16 x 2, the host leg's threads and lanes: 32 streams), each stream
// with its own pinned buffer and one copy of S bytes in flight; a thread goes
// round its streams, waits for one (hipStreamSynchronize, as host_leg.cpp
// waits) and queues its next copy at once, until every stream has moved its
// share; S = 8 / 16 / 32 / 64 MiB in turn, twice.  Prints the aggregate GB/s
// per size.  (32 x 1 puts 32 waiting threads on the box's 16 CPUs.)
//
//   hipcc --offload-arch=gfx950 -O2 tools/d2h_ceiling.hip -o tools/d2h_ceiling -pthread
//   tools/d2h_ceiling [threads] [streams per thread] [GiB per stream and size]
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#define HIPOK(x)                                                                         \
    do {                                                                                 \
        const hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                          \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
            exit(1);                                                                     \
        }                                                                                \
    } while (0)

static double now() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
    const int NT = argc > 1 ? atoi(argv[1]) : 16, K = argc > 2 ? atoi(argv[2]) : 2;
    const size_t per = (size_t)(argc > 3 ? atoi(argv[3]) : 1) << 30;
    const size_t SMAX = 64u << 20;
    if (NT < 1 || K < 1 || NT * K > 64 || per < SMAX) {
        fprintf(stderr, "1..64 streams in all, at least 1 GiB each\n");
        return 2;
    }
    const int T = NT * K;  // streams
    // stream t reads its own SMAX-byte window of the source over and over
    char* dsrc = nullptr;
    HIPOK(hipMalloc((void**)&dsrc, (size_t)T * SMAX));
    HIPOK(hipMemset(dsrc, 1, (size_t)T * SMAX));
    std::vector<hipStream_t> ws(T);
    std::vector<void*> hb(T);
    for (int t = 0; t < T; ++t) {
        HIPOK(hipStreamCreateWithFlags(&ws[t], hipStreamNonBlocking));
        HIPOK(hipHostMalloc(&hb[t], SMAX, hipHostMallocDefault));
    }
    HIPOK(hipDeviceSynchronize());
    for (int round = 0; round < 2; ++round)
        for (size_t S : {(size_t)8 << 20, (size_t)16 << 20, (size_t)32 << 20, (size_t)64 << 20}) {
            const size_t copies = per / S;
            std::vector<std::thread> th;
            const double t0 = now();
            for (int w = 0; w < NT; ++w)
                th.emplace_back([&, w] {
                    HIPOK(hipSetDevice(0));
                    for (size_t c = 0; c <= copies; ++c)
                        for (int t = w * K; t < (w + 1) * K; ++t) {
                            if (c) HIPOK(hipStreamSynchronize(ws[t]));
                            if (c < copies)
                                HIPOK(hipMemcpyAsync(hb[t], dsrc + (size_t)t * SMAX, S, hipMemcpyDeviceToHost, ws[t]));
                        }
                });
            for (auto& x : th) x.join();
            const double dt = now() - t0;
            printf("round %d: %d threads x %d streams x %zu copies of %zu MiB: %.1f ms, %.2f GB/s\n", round, NT, K, copies, S >> 20,
                   dt * 1e3, (double)T * copies * S / dt / 1e9);
            fflush(stdout);
        }
    for (int t = 0; t < T; ++t) {
        HIPOK(hipStreamDestroy(ws[t]));
        HIPOK(hipHostFree(hb[t]));
    }
    HIPOK(hipFree(dsrc));
    return 0;
}
