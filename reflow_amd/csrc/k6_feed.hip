// k6_feed.hip -- K6: the graph change feed (rf_graph_feed_*).
//
// After an incremental step an evaluator needs the cache keys that moved
// (flow.go:796-802 CacheKeys) to look them up again (eval.go:1172-1220
// Eval.lookup): the reference walks its nodes one by one; here the step
// already visited exactly the jobs that can have changed, and the feed keeps
// that knowledge on the device.
//
// State per tracked graph (FeedDev): a SHADOW of the slot table, [S][32], the
// digests as last reported (at open: the table as it stood); a MASK bitmap,
// bit s = slot s is a job output the caller wants reported; a PENDING bitmap,
// bit s = slot s differs from its shadow and has not been delivered yet.
// Both bitmaps are u32 words padded to whole tiles of kFeedTileSlots slots.
//
// A poll sets pending bits, then compacts them.  The bits are set one of two
// ways, always by comparing a slot with its shadow:
//   scan    one lane per slot under the mask (k6_feed_scan);
//   listed  one lane per candidate job of the one plain step since the last
//           poll -- the jobs in its level lists (k6_feed_listed, reading the
//           step's cursor half through k2_lists.h) and the slot-fused jobs of
//           the input slots marked for it, recorded at mark time
//           (k6_feed_record, k6_feed_listed_sf) -- each followed through its
//           fusion targets while a digest moved (feed_walk), the cut-off the
//           level kernels apply.
// Compaction is the three-launch pattern of k4_collect_* / k5_scan_*: a
// per-tile count (k6_feed_count, which first drops the bits of slots that
// moved back to their shadow), the tile scan (k4_collect_scan, reused) and a
// per-tile scatter in ascending slot order (k6_feed_scatter) -- no atomic on
// a counter, plain vector stores.  The scatter delivers ranks below cap:
// slot and digest out, digest into the shadow, bit cleared; the rest keep
// their bits and lead the next poll.
//
// The fused lookup (k6_feed_lookup) runs each delivered key through the
// liveset (bloom_dev.h) and, unless the liveset rules it out, the HBM assoc
// (assoc_dev.h), reading the delivered count from device memory.
#include <algorithm>

#include "engine.h"
#include "k2_lists.h"
#include "assoc_dev.h"
#include "bloom_dev.h"

namespace rf {

static_assert(kFeedTileSlots == 256 * 32, "a tile is one 256-lane workgroup of 32-slot bitmap words");
constexpr uint32_t kFeedBlock = 256;

__device__ __forceinline__ bool feed_differs(const uint8_t* __restrict__ slots, const uint8_t* __restrict__ shadow,
                                             uint32_t s) {
    const uint4* a = reinterpret_cast<const uint4*>(slots + 32ull * s);
    const uint4* b = reinterpret_cast<const uint4*>(shadow + 32ull * s);
    const uint4 alo = a[0], ahi = a[1], blo = b[0], bhi = b[1];
    return ((alo.x ^ blo.x) | (alo.y ^ blo.y) | (alo.z ^ blo.z) | (alo.w ^ blo.w) | (ahi.x ^ bhi.x) |
            (ahi.y ^ bhi.y) | (ahi.z ^ bhi.z) | (ahi.w ^ bhi.w)) != 0;
}

// mask = caller's mask (null: every slot) AND "is a job output", from the job records.
__global__ __launch_bounds__(kFeedBlock) void k6_feed_mask(const uint4* __restrict__ meta, uint32_t n_jobs,
                                                           const uint32_t* __restrict__ want,
                                                           uint32_t* __restrict__ mask) {
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n_jobs; j += gridDim.x * blockDim.x) {
        const uint32_t o = meta[2ull * j + 1].x, bit = 1u << (o & 31);
        if (!want || (want[o >> 5] & bit)) atomicOr(&mask[o >> 5], bit);
    }
}

// The slot-fused job (GraphDev::plan, ~0u: none) of each input slot of a mark batch.
__global__ __launch_bounds__(kFeedBlock) void k6_feed_record(const uint4* __restrict__ plan,
                                                             const uint32_t* __restrict__ sl, uint32_t n,
                                                             uint32_t* __restrict__ out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = plan[3ull * sl[i]].z;
}

// Scan: one lane per slot; a wave owns the two bitmap words of its 64 slots.
__global__ __launch_bounds__(kFeedBlock) void k6_feed_scan(FeedDev f, const uint8_t* __restrict__ slots) {
    const uint64_t n = 32ull * f.words;
    for (uint64_t base = (uint64_t)blockIdx.x * kFeedBlock; base < n; base += (uint64_t)gridDim.x * kFeedBlock) {
        const uint64_t s = base + threadIdx.x;
        const bool on = (f.mask[s >> 5] >> (s & 31)) & 1u;  // (set only below n_slots)
        const bool d = on && feed_differs(slots, f.shadow, (uint32_t)s);
        const unsigned long long bal = __ballot(d);
        const uint32_t lane = threadIdx.x & 63;
        if (lane == 0 && (uint32_t)bal) f.pending[s >> 5] |= (uint32_t)bal;
        if (lane == 32 && (uint32_t)(bal >> 32)) f.pending[s >> 5] |= (uint32_t)(bal >> 32);
    }
}

// A candidate job (its record's second half m1) and its fusion targets: a
// tracked out slot that differs from its shadow gets its pending bit; the
// walk goes on while the digest moved -- or the bit was already set (moved
// since it was last delivered: its target may have moved with it), or the
// slot is not tracked (no shadow to judge by) -- and the job has a target.
__device__ __forceinline__ void feed_walk(const FeedDev& f, const uint4* __restrict__ meta,
                                          const uint8_t* __restrict__ slots, uint4 m1) {
    for (;;) {
        const uint32_t o = m1.x, w = o >> 5, bit = 1u << (o & 31);
        bool go = true;
        if (f.mask[w] & bit) {
            const bool d = feed_differs(slots, f.shadow, o);
            const bool was = (f.pending[w] & bit) != 0;
            if (d && !was) atomicOr(&f.pending[w], bit);
            go = d || was;
        }
        if (!go || m1.w == ~0u) return;
        m1 = meta[2ull * m1.w + 1];
    }
}

// Listed: the jobs in the level lists of the one plain step since the last
// poll (a.counts = that step's cursor half), level lv.lvl[blockIdx.y].
struct FeedLevels {
    uint32_t n;
    uint32_t lvl[31];
};
__global__ __launch_bounds__(kFeedBlock) void k6_feed_listed(FeedDev f, LevelArgs a, FeedLevels lv) {
    const uint32_t l = lv.lvl[blockIdx.y];
    const uint32_t n = level_count(a, l);
    for (uint32_t i = blockIdx.x * kFeedBlock + threadIdx.x; i < n; i += gridDim.x * kFeedBlock)
        feed_walk(f, a.meta, a.slots, a.lmeta[2ull * level_pos(a, l, i) + 1]);
}

// Listed: the slot-fused jobs recorded at mark time.
__global__ __launch_bounds__(kFeedBlock) void k6_feed_listed_sf(FeedDev f, const uint4* __restrict__ meta,
                                                                const uint8_t* __restrict__ slots,
                                                                const uint32_t* __restrict__ sf, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kFeedBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFeedBlock) {
        const uint32_t p = sf[i];
        if (p != ~0u) feed_walk(f, meta, slots, meta[2ull * p + 1]);
    }
}

// Compaction 1/3: per tile, the pending bits under the mask that still differ
// from their shadow (a slot that moved and moved back is dropped).
__global__ __launch_bounds__(kFeedBlock) void k6_feed_count(FeedDev f, const uint8_t* __restrict__ slots) {
    __shared__ uint32_t s_cnt[kFeedBlock / 64];
    const uint64_t w = (uint64_t)blockIdx.x * kFeedBlock + threadIdx.x;
    const uint32_t p0 = f.pending[w] & f.mask[w];
    uint32_t p = p0;
    for (uint32_t q = p0; q; q &= q - 1) {
        const uint32_t b = (uint32_t)__builtin_ctz(q);
        if (!feed_differs(slots, f.shadow, (uint32_t)(32 * w + b))) p &= ~(1u << b);
    }
    if (p != p0) f.pending[w] = p;
    uint32_t cnt = (uint32_t)__builtin_popcount(p);
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < kFeedBlock / 64; ++k) c += s_cnt[k];
        f.tile_count[blockIdx.x] = c;
    }
}

// Compaction 3/3: per tile, ascending: ranks below cap are delivered.
// n2 = {found (the tile scan's total), written}.
__global__ __launch_bounds__(kFeedBlock) void k6_feed_scatter(FeedDev f, const uint8_t* __restrict__ slots,
                                                              uint64_t cap, uint32_t* __restrict__ out_slots,
                                                              uint8_t* __restrict__ out_dig,
                                                              unsigned long long* __restrict__ n2) {
    __shared__ uint32_t s_w[kFeedBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) n2[1] = n2[0] < cap ? n2[0] : cap;
    const uint64_t w = (uint64_t)blockIdx.x * kFeedBlock + threadIdx.x;
    uint64_t rank = f.tile_count[blockIdx.x];  // (exclusive, after the tile scan)
    if (rank >= cap) return;                   // the whole tile stays pending (uniform over the block)
    const uint32_t p0 = f.pending[w];
    const uint32_t c = (uint32_t)__builtin_popcount(p0);
    uint32_t x = c;  // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    for (uint32_t k = 0; k < wave; ++k) rank += s_w[k];
    rank += x - c;
    uint32_t p = p0;
    for (uint32_t q = p0; q && rank < cap; q &= q - 1, ++rank) {
        const uint32_t b = (uint32_t)__builtin_ctz(q), s = (uint32_t)(32 * w + b);
        const uint4* src = reinterpret_cast<const uint4*>(slots + 32ull * s);
        const uint4 lo = src[0], hi = src[1];
        uint4* sh = reinterpret_cast<uint4*>(f.shadow + 32ull * s);
        uint4* od = reinterpret_cast<uint4*>(out_dig + 32ull * rank);
        out_slots[rank] = s;
        od[0] = lo;
        od[1] = hi;
        sh[0] = lo;
        sh[1] = hi;
        p &= ~(1u << b);
    }
    if (p != p0) f.pending[w] = p;
}

// Fused lookup, one lane per delivered key (n2[1] of them): status 2 = the
// liveset (words non-null) does not contain it, the assoc is not read; 1 =
// found (a nonzero value, as rf_assoc_get); 0 = NotExist.
__global__ __launch_bounds__(kFeedBlock) void k6_feed_lookup(const uint64_t* __restrict__ words,
                                                             const uint64_t* __restrict__ len_dev, uint64_t m,
                                                             uint64_t mu, uint32_t k, AssocView t, uint32_t kind,
                                                             const uint8_t* __restrict__ keys,
                                                             const unsigned long long* __restrict__ n2,
                                                             uint8_t* __restrict__ status, uint8_t* __restrict__ vals) {
    const uint64_t n = n2[1];
    const uint64_t length = words ? *len_dev : 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kFeedBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kFeedBlock) {
        uint4 a = make_uint4(0, 0, 0, 0), b = a;
        uint8_t st = 2;
        if (!words || bloom_contains(words, length, m, mu, k, keys + 32 * i)) {
            const uint4* kp = reinterpret_cast<const uint4*>(keys + 32ull * i);
            const uint4 lo = kp[0], hi = kp[1];
            const uint32_t slot = assoc_find(t, kind, lo, hi);
            if (slot != kEmpty) {
                a = t.vals[2 * slot];
                b = t.vals[2 * slot + 1];
            }
            st = (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) != 0;
        }
        uint4* o = reinterpret_cast<uint4*>(vals + 32ull * i);
        o[0] = a;
        o[1] = b;
        status[i] = st;
    }
}

static uint32_t feed_grid(uint64_t items, uint32_t cap = 4096) {
    const uint64_t g = (items + kFeedBlock - 1) / kFeedBlock;
    return (uint32_t)(g < 1 ? 1 : g > cap ? cap : g);
}

hipError_t launch_feed_mask(const GraphDev& g, const FeedDev& f, const uint32_t* want, hipStream_t s) {
    if (!g.n_jobs) return hipSuccess;
    hipLaunchKernelGGL(k6_feed_mask, dim3(feed_grid(g.n_jobs)), dim3(kFeedBlock), 0, s, g.meta, g.n_jobs, want, f.mask);
    return hipGetLastError();
}

hipError_t launch_feed_record(const GraphDev& g, const uint32_t* slots, uint32_t n, uint32_t* out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k6_feed_record, dim3(feed_grid(n)), dim3(kFeedBlock), 0, s, g.plan, slots, n, out);
    return hipGetLastError();
}

hipError_t launch_feed_scan(const GraphDev& g, const FeedDev& f, hipStream_t s) {
    hipLaunchKernelGGL(k6_feed_scan, dim3(feed_grid(32ull * f.words, 16384)), dim3(kFeedBlock), 0, s, f, g.slots);
    return hipGetLastError();
}

hipError_t launch_feed_listed(const GraphDev& g, const FeedDev& f, const uint32_t* lists, const uint32_t* sf,
                              uint64_t n_sf, hipStream_t s) {
    if (lists) {
        LevelArgs a{};
        a.meta = g.meta;
        a.lvl_start = g.lvl_start_dev;
        a.n_levels = g.n_levels;
        a.slots = g.slots;
        a.list = g.list;
        a.lmeta = g.lmeta;
        a.counts = const_cast<uint32_t*>(lists);
        FeedLevels lv{};
        uint32_t most = 0;
        auto flush = [&]() {
            if (lv.n)
                hipLaunchKernelGGL(k6_feed_listed, dim3(feed_grid(most, 1024), lv.n), dim3(kFeedBlock), 0, s, f, a, lv);
            lv.n = 0;
            most = 0;
        };
        for (uint32_t l = 0; l < g.n_levels; ++l) {
            if (!(g.inc_level[l] & kLvlForm)) continue;  // never listed
            lv.lvl[lv.n++] = l;
            most = std::max(most, g.lvl_start[l + 1] - g.lvl_start[l]);
            if (lv.n == 31) flush();
        }
        flush();
    }
    if (n_sf)
        hipLaunchKernelGGL(k6_feed_listed_sf, dim3(feed_grid(n_sf)), dim3(kFeedBlock), 0, s, f, g.meta, g.slots, sf,
                           n_sf);
    return hipGetLastError();
}

hipError_t launch_feed_compact(const GraphDev& g, const FeedDev& f, uint64_t cap, uint32_t* out_slots,
                               uint8_t* out_dig, uint64_t* n2, hipStream_t s) {
    // (f.tiles >= 1: the bitmaps of an empty graph are one tile of zero words)
    hipLaunchKernelGGL(k6_feed_count, dim3(f.tiles), dim3(kFeedBlock), 0, s, f, g.slots);
    hipError_t e = launch_tile_scan(f.tile_count, f.tiles, n2, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k6_feed_scatter, dim3(f.tiles), dim3(kFeedBlock), 0, s, f, g.slots, cap, out_slots, out_dig,
                       reinterpret_cast<unsigned long long*>(n2));
    return hipGetLastError();
}

hipError_t launch_feed_lookup(const BloomDev* live, const AssocView& t, uint32_t kind, const uint8_t* keys,
                              const uint64_t* n2, uint64_t max_n, uint8_t* status, uint8_t* vals, hipStream_t s) {
    if (!max_n) return hipSuccess;
    hipLaunchKernelGGL(k6_feed_lookup, dim3(feed_grid(max_n)), dim3(kFeedBlock), 0, s,
                       live ? live->words : nullptr, live ? live->len_dev : nullptr, live ? live->m : 1,
                       live && live->m ? (~0ull) / live->m : 0ull, live ? (uint32_t)live->k : 0u, t, kind, keys,
                       reinterpret_cast<const unsigned long long*>(n2), status, vals);
    return hipGetLastError();
}

}  // namespace rf
