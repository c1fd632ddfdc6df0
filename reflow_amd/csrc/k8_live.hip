// k8_live.hip -- K8: the GC liveset (rf_liveset_*): Eval.collect's walk, the
// per-value Files() dedup and the filter build (eval.go:791-868).
//
// Walk (eval.go:809-826): K7's frontier traversal with another cut-off.  One
// append-only QUEUE holds every expanded node once, in arrival order; a round
// works on queue[lo, hi) and appends behind hi.  A node is CLAIMED with a
// returning atomicOr on its bit of the claim bitmap, so two parents (or an
// edge listed twice) reach it once; a claimed node that has a value gets its
// VALUE state from the claiming lane and is not queued; the others of a wave
// are appended with one ballot and one atomicAdd per wave.  The workgroup
// whose arrival add comes last moves lo, hi to the appended stretch, so the
// host can enqueue several rounds without reading anything back.  Everything
// one round writes for the next (queue entries, states, the bounds) is read
// only after the kernel boundary.
//
// Contributions: the VALUE nodes by a tile mark / scan / scatter over the
// state array (ascending, never arrival order), the writers copied behind
// them; an exclusive scan of their row counts gives every contribution's row
// offset and nlive_est.
//
// Rows, lane per row: the row's contribution by a binary search on the
// offsets, then a segmented form of k5_dedup_insert / _resolve -- a
// power-of-two table of row indices, at most half full; the probe start
// hashes the contribution ordinal, the eight ID words and the size; a slot
// matches iff ordinal, ID and size equal those of the row it names; the
// smallest row index wins; probing is bounded and a batch that hits the bound
// is flagged.  A row is FIRST iff it is its class's winner: the firsts are
// counted, their sizes summed (integers: order-independent) and their WD(ID)
// added to the filter (Add is idempotent: the words do not depend on which
// row of a class adds them).
#include "live_internal.h"
#include "assoc_dev.h"  // kEmpty, key_hash
#include "bloom_dev.h"
#include "reflow_hip.h"

namespace rf {

static_assert(kLiveListTile == 4 * kLiveBlock, "a list tile is one workgroup of four-state words");
static_assert(kLiveListTile == RF_LIVE_LIST_TILE, "the header states the tile");

constexpr uint32_t kLiveMaxProbe = 1u << 16;

// Every lane of the wave calls this: lanes with `has` claim node k; the fresh
// ones without a value are appended to the queue.
__device__ __forceinline__ void live_claim(const LiveDev& p, bool has, uint32_t k, uint32_t lane) {
    bool fresh = false;
    if (has) {
        const uint32_t m = 1u << (k & 31);
        fresh = !(atomicOr(&p.claim[k >> 5], m) & m);
        if (fresh && p.has[k]) {  // FlowDone with a Fileset: on the frontier, not expanded (eval.go:812-816)
            p.state[k] = RF_LIVE_VALUE;
            fresh = false;
        }
    }
    const uint64_t b = __ballot(fresh);
    if (b) {
        const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)b) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&p.ctl[kLiveTail], (uint32_t)__popcll(b));
        base = __shfl(base, leader, 64);
        const uint32_t at = base + (uint32_t)__popcll(b & lt);
        if (fresh && at < p.n) p.queue[at] = k;  // (at < n always: a node is claimed fresh once)
    }
}

// Every lane of the wave calls this: lanes with `go` reach their node's edges.
// Nodes of degree < 64 go lane per node in wave lockstep; a node of degree
// >= 64 is taken by the whole wave, 64 edges at a time.
__device__ __forceinline__ void live_expand(const LiveDev& p, bool go, uint32_t node, uint32_t lane) {
    uint64_t c = 0, ce = 0;
    if (go) {
        c = p.edge_ptr[node];
        ce = p.edge_ptr[node + 1];
    }
    const bool wide = ce - c >= 64;
    uint64_t wides = __ballot(wide);
    uint64_t c1 = wide ? ce : c;
    while (__any(c1 < ce)) {
        const bool has = c1 < ce;
        uint32_t k = 0;
        if (has) k = p.edges[c1++];
        live_claim(p, has, k, lane);
    }
    while (wides) {
        const int src = __ffsll((unsigned long long)wides) - 1;
        wides &= wides - 1;
        const uint64_t b0 = (uint64_t)__shfl((unsigned long long)c, src, 64);
        const uint64_t e0 = (uint64_t)__shfl((unsigned long long)ce, src, 64);
        for (uint64_t x = b0; x < e0; x += 64) {
            const bool has = x + lane < e0;
            uint32_t k = 0;
            if (has) k = p.edges[x + lane];
            live_claim(p, has, k, lane);
        }
    }
}

__device__ __forceinline__ uint32_t live_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint64_t live_wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}

// lo = hi, hi = tail: the stretch appended since the last move is the next frontier
__global__ void k8_live_advance(LiveDev p) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.ctl[kLiveLo] = p.ctl[kLiveHi];
        p.ctl[kLiveHi] = p.ctl[kLiveTail];
    }
}

__global__ __launch_bounds__(kLiveBlock) void k8_live_seed(LiveDev p, const uint32_t* __restrict__ roots,
                                                           uint32_t n_roots) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kLiveBlock; base < n_roots; base += (uint64_t)gridDim.x * kLiveBlock) {
        const uint64_t i = base + threadIdx.x;
        const bool has = i < n_roots;
        live_claim(p, has, has ? roots[i] : 0u, lane);
    }
}

// One round: lane per frontier node -- WALKED, and its edges are reached (eval.go:817-824).
__global__ __launch_bounds__(kLiveBlock) void k8_live_round(LiveDev p) {
    const uint32_t lo = p.ctl[kLiveLo], hi = p.ctl[kLiveHi];
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = lo + (uint64_t)blockIdx.x * kLiveBlock; base < hi; base += (uint64_t)gridDim.x * kLiveBlock) {
        const uint64_t i = base + threadIdx.x;
        const bool go = i < hi;
        uint32_t node = 0;
        if (go) {
            node = p.queue[i];
            p.state[node] = RF_LIVE_WALKED;
        }
        live_expand(p, go, node, lane);
    }
    __syncthreads();  // every wave's tail adds have returned
    if (threadIdx.x == 0) {
        const uint32_t before = atomicAdd(&p.ctl[kLiveArrived], 1u);
        if (before == gridDim.x - 1) {  // the last workgroup through: the next launch's bounds
            const uint32_t tail = atomicAdd(&p.ctl[kLiveTail], 0u);
            p.ctl[kLiveLo] = hi;
            p.ctl[kLiveHi] = tail;
            atomicExch(&p.ctl[kLiveArrived], 0u);
        }
    }
}

// Nodes per state (counts zeroed by the host), four state bytes per lane.
__global__ __launch_bounds__(kLiveBlock) void k8_live_count(LiveDev p) {
    const uint32_t* __restrict__ w4 = reinterpret_cast<const uint32_t*>(p.state);
    const uint64_t words = ((uint64_t)p.n + 3) / 4;
    uint32_t c[3] = {0, 0, 0};
    for (uint64_t w = (uint64_t)blockIdx.x * kLiveBlock + threadIdx.x; w < words; w += (uint64_t)gridDim.x * kLiveBlock) {
        const uint32_t v = w4[w];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t s = (v >> (8 * j)) & 0xffu;
            if (4 * w + j < p.n) {
#pragma unroll
                for (uint32_t q = 0; q < 3; ++q) c[q] += s == q;
            }
        }
    }
    // one counter word takes ~88 atomics/us: wave sums, then one add per workgroup and state
    __shared__ uint32_t s_c[3][kLiveBlock / 64];
#pragma unroll
    for (uint32_t q = 0; q < 3; ++q) {
        const uint32_t t = live_wave_sum(c[q]);
        if ((threadIdx.x & 63) == 0) s_c[q][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kLiveBlock / 64; ++w) t += s_c[threadIdx.x][w];
        if (t) atomicAdd(&p.ctl[kLiveCounts + threadIdx.x], t);
    }
}

// A lane's four nodes of tile blockIdx.x that are in `state`: a 4-bit mask.
__device__ __forceinline__ uint32_t live_tile_mask(const LiveDev& p, uint32_t state, uint64_t first) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p.state + first);  // (state is padded to whole tiles)
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (((v >> (8 * j)) & 0xffu) == state && first + j < p.n) m |= 1u << j;
    return m;
}

// List 1/3: per tile, the nodes in `state`.
__global__ __launch_bounds__(kLiveBlock) void k8_live_list_count(LiveDev p, uint32_t state,
                                                                 uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t s_cnt[kLiveBlock / 64];
    const uint64_t first = ((uint64_t)blockIdx.x * kLiveBlock + threadIdx.x) * 4;
    const uint32_t cnt = live_wave_sum((uint32_t)__builtin_popcount(live_tile_mask(p, state, first)));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < kLiveBlock / 64; ++k) c += s_cnt[k];
        tile_count[blockIdx.x] = c;
    }
}

// List 3/3 (after the tile scan): per tile, ascending node id; ranks below cap are written.
__global__ __launch_bounds__(kLiveBlock) void k8_live_list_scatter(LiveDev p, uint32_t state, uint64_t cap,
                                                                   const uint32_t* __restrict__ tile_count,
                                                                   uint32_t* __restrict__ nodes) {
    __shared__ uint32_t s_w[kLiveBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t rank = tile_count[blockIdx.x];  // (exclusive, after the tile scan)
    if (rank >= cap) return;                 // uniform over the block
    const uint64_t first = ((uint64_t)blockIdx.x * kLiveBlock + threadIdx.x) * 4;
    const uint32_t m = live_tile_mask(p, state, first);
    const uint32_t c = (uint32_t)__builtin_popcount(m);
    uint32_t x = c;  // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    for (uint32_t k = 0; k < wave; ++k) rank += s_w[k];
    rank += x - c;
    for (uint32_t q = m; q && rank < cap; q &= q - 1, ++rank) nodes[rank] = (uint32_t)(first + (uint32_t)__builtin_ctz(q));
}

// rf_liveset_set_values / _clear_values: the listed nodes' value records
__global__ __launch_bounds__(kLiveBlock) void k8_live_set(LiveDev p, const uint32_t* __restrict__ nodes,
                                                          const uint8_t* __restrict__ has,
                                                          const uint64_t* __restrict__ off,
                                                          const uint32_t* __restrict__ cnt, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kLiveBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kLiveBlock) {
        const uint32_t v = nodes[i];
        if (v >= p.n) continue;  // (checked on the host)
        p.has[v] = has[i];
        p.val_off[v] = off[i];
        p.val_cnt[v] = cnt[i];
    }
}

// ---- contributions' row offsets ------------------------------------------------
__device__ __forceinline__ uint32_t live_contrib_rows(const LiveDev& p, const LiveRows& r, uint64_t c) {
    if (c >= r.n_contrib) return 0;
    const uint32_t node = r.contrib[c];
    if (node >= p.n) return 0;  // (checked on the host)
    return p.has[node] ? p.val_cnt[node] : 0u;  // a writer without a value: zero rows
}

// Offsets 1/3: per tile of kLiveListTile contributions, their rows.
__global__ __launch_bounds__(kLiveBlock) void k8_live_tile_rows(LiveDev p, LiveRows r) {
    __shared__ uint64_t s_sum[kLiveBlock / 64];
    const uint64_t first = ((uint64_t)blockIdx.x * kLiveBlock + threadIdx.x) * 4;
    uint64_t t = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) t += live_contrib_rows(p, r, first + j);
    t = live_wave_sum64(t);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t c = 0;
        for (uint32_t k = 0; k < kLiveBlock / 64; ++k) c += s_sum[k];
        r.tile_rows[blockIdx.x] = c;
    }
}

// Offsets 2/3: exclusive scan of the tile sums by one block, 1024 per pass;
// the total is nlive_est and the offsets' last entry.
__global__ __launch_bounds__(1024) void k8_live_scan64(LiveDev p, LiveRows r, uint64_t tiles) {
    __shared__ uint64_t s_w[16];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t b = 0; b < tiles; b += 1024) {
        const uint64_t t = b + threadIdx.x;
        const uint64_t c = t < tiles ? r.tile_rows[t] : 0ull;
        uint64_t x = c;  // inclusive wave scan
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o, 64);
            if (lane >= (uint32_t)o) x += y;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        uint64_t before = 0, total = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            before += w < wave ? s_w[w] : 0ull;
            total += s_w[w];
        }
        if (t < tiles) r.tile_rows[t] = carry + before + x - c;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        r.row_off[r.n_contrib] = carry;
        p.res[kLiveEst] = carry;
    }
}

// Offsets 3/3: every contribution's first row.
__global__ __launch_bounds__(kLiveBlock) void k8_live_row_offsets(LiveDev p, LiveRows r) {
    __shared__ uint64_t s_w[kLiveBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t first = ((uint64_t)blockIdx.x * kLiveBlock + threadIdx.x) * 4;
    uint32_t cnt[4];
    uint64_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        cnt[j] = live_contrib_rows(p, r, first + j);
        c += cnt[j];
    }
    uint64_t x = c;  // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint64_t at = r.tile_rows[blockIdx.x] + x - c;
    for (uint32_t k = 0; k < wave; ++k) at += s_w[k];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        if (first + j < r.n_contrib) r.row_off[first + j] = at;
        at += cnt[j];
    }
}

// ---- rows ------------------------------------------------------------------------
// Rows 1/3: row i belongs to the contribution c with row_off[c] <= i <
// row_off[c+1] (zero-row contributions own nothing); its arena row.
__global__ __launch_bounds__(kLiveBlock) void k8_live_locate(LiveDev p, LiveRows r) {
    for (uint64_t i = (uint64_t)blockIdx.x * kLiveBlock + threadIdx.x; i < r.n_rows; i += (uint64_t)gridDim.x * kLiveBlock) {
        uint64_t lo = 0, hi = r.n_contrib - 1;  // (n_rows > 0: at least one contribution)
        while (lo < hi) {                       // the smallest c with row_off[c+1] > i
            const uint64_t mid = (lo + hi) >> 1;
            if (r.row_off[mid + 1] <= i) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t node = r.contrib[lo];
        r.row_ord[i] = (uint32_t)lo;  // (a run has at most 2^32 - 1 contributions: checked on the host)
        r.row_src[i] = p.val_off[node] + (i - r.row_off[lo]);
    }
}

struct LiveRow {
    uint4 lo, hi;
    long long size;
};
__device__ __forceinline__ LiveRow live_load_row(const LiveDev& p, uint64_t src) {
    const uint4* d = reinterpret_cast<const uint4*>(p.ids + 32ull * src);
    LiveRow w;
    w.lo = d[0];
    w.hi = d[1];
    w.size = p.sizes[src];
    return w;
}
__device__ __forceinline__ uint32_t live_hash(uint32_t ord, const LiveRow& w) {
    uint32_t h = key_hash(w.lo, w.hi);
    h ^= ord * 0x9E3779B1u;
    h ^= (uint32_t)w.size * 0x85EBCA77u;
    h ^= (uint32_t)((unsigned long long)w.size >> 32) * 0xC2B2AE3Du;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    return h;
}
__device__ __forceinline__ bool live_row_eq(const LiveRow& a, const LiveRow& b) {
    return ((a.lo.x ^ b.lo.x) | (a.lo.y ^ b.lo.y) | (a.lo.z ^ b.lo.z) | (a.lo.w ^ b.lo.w) | (a.hi.x ^ b.hi.x) |
            (a.hi.y ^ b.hi.y) | (a.hi.z ^ b.hi.z) | (a.hi.w ^ b.hi.w)) == 0 &&
           a.size == b.size;
}

// Rows 2/3: insert row i; slot_of[i] = the slot that holds its class.  A slot's
// value only ever moves from empty to a row index and then down (atomicMin),
// and every index a slot ever holds is of the slot's class, so a stale read of
// a non-empty slot still names the right class.
__global__ __launch_bounds__(kLiveBlock) void k8_live_insert(LiveDev p, LiveRows r) {
    for (uint64_t i0 = (uint64_t)blockIdx.x * kLiveBlock + threadIdx.x; i0 < r.n_rows; i0 += (uint64_t)gridDim.x * kLiveBlock) {
        const uint32_t i = (uint32_t)i0;
        const uint32_t ord = r.row_ord[i];
        const LiveRow w = live_load_row(p, r.row_src[i]);
        uint32_t slot = live_hash(ord, w) & r.mask;
        uint32_t probes = 0;
        for (;; ++probes) {
            if (probes >= kLiveMaxProbe) {  // bounded: every wave exits; the batch is flagged in resolve
                slot = kEmpty;
                break;
            }
            uint32_t cur = __hip_atomic_load(&r.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kEmpty) {
                cur = atomicCAS(&r.table[slot], kEmpty, i);
                if (cur == kEmpty) break;  // claimed: this row opens its class
            }
            if (cur >= r.n_rows) {  // not a row of this run: the table was not cleared
                slot = kEmpty;
                break;
            }
            if (r.row_ord[cur] == ord && live_row_eq(w, live_load_row(p, r.row_src[cur]))) {
                if (i < cur) atomicMin(&r.table[slot], i);
                break;
            }
            slot = (slot + 1) & r.mask;
        }
        r.slot_of[i] = slot;
    }
}

// Rows 3/3: the firsts -- counted, their sizes summed, their WD(ID) added.
__global__ __launch_bounds__(kLiveBlock) void k8_live_resolve(LiveDev p, LiveRows r, unsigned long long* __restrict__ words,
                                                              uint64_t m, uint64_t mu, uint32_t k) {
    __shared__ uint32_t s_n[kLiveBlock / 64];
    __shared__ long long s_b[kLiveBlock / 64];
    uint32_t n_first = 0;
    long long bytes = 0;
    bool bad = false;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kLiveBlock + threadIdx.x; i0 < r.n_rows; i0 += (uint64_t)gridDim.x * kLiveBlock) {
        const uint32_t i = (uint32_t)i0;
        const uint32_t so = r.slot_of[i];
        if (so == kEmpty) {
            bad = true;
            continue;
        }
        if (r.table[so] != i) continue;
        const uint64_t src = r.row_src[i];
        ++n_first;
        bytes += p.sizes[src];
        uint64_t D[4], h[4];
        load_digest64(p.ids + 32ull * src, D);
        base_hashes_wd(D, h);
        for (uint32_t j = 0; j < k; ++j) {
            const uint64_t loc = mod_m(bloom_loc(h, j), m, mu);  // (< m = the bitset's length)
            atomicOr(&words[loc >> 6], 1ull << (loc & 63));
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.res[kLiveFlags], (unsigned long long)kLiveFlagProbe);
    n_first = live_wave_sum(n_first);
    bytes = (long long)live_wave_sum64((uint64_t)bytes);
    if ((threadIdx.x & 63) == 0) {
        s_n[threadIdx.x >> 6] = n_first;
        s_b[threadIdx.x >> 6] = bytes;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long c = 0, b = 0;
        for (uint32_t w = 0; w < kLiveBlock / 64; ++w) {
            c += s_n[w];
            b += (unsigned long long)s_b[w];  // two's complement sum
        }
        if (c) atomicAdd(&p.res[kLiveN], c);
        if (b) atomicAdd(&p.res[kLiveBytes], b);
    }
}

// changed: does any word differ (bitset.go:322-340)?
__global__ __launch_bounds__(kLiveBlock) void k8_live_compare(LiveDev p, const uint64_t* __restrict__ a,
                                                              const uint64_t* __restrict__ b, uint64_t nwords) {
    bool diff = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kLiveBlock + threadIdx.x; i < nwords; i += (uint64_t)gridDim.x * kLiveBlock)
        diff |= a[i] != b[i];
    if (__any(diff) && (threadIdx.x & 63) == 0) atomicOr(&p.res[kLiveFlags], (unsigned long long)kLiveFlagDiff);
}

// ---- launches ----------------------------------------------------------------------
uint32_t live_grid(uint32_t n) {
    const uint32_t g = (n + kLiveBlock - 1) / kLiveBlock;
    return g < 1 ? 1 : g > kLiveMaxGrid ? kLiveMaxGrid : g;
}

static uint32_t items_grid(uint64_t items) {
    const uint64_t g = (items + kLiveBlock - 1) / kLiveBlock;
    return (uint32_t)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

uint32_t live_table_slots(uint32_t rows) {
    uint32_t cap = 64;
    while (cap < 2ull * rows && cap < (1u << 31)) cap <<= 1;
    return cap;
}

hipError_t launch_live_set(const LiveDev& d, const uint32_t* nodes, const uint8_t* has, const uint64_t* off,
                           const uint32_t* cnt, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k8_live_set, dim3(items_grid(n)), dim3(kLiveBlock), 0, s, d, nodes, has, off, cnt, n);
    return hipGetLastError();
}

hipError_t launch_live_seed(const LiveDev& d, const uint32_t* roots, uint32_t n_roots, hipStream_t s) {
    if (n_roots) hipLaunchKernelGGL(k8_live_seed, dim3(items_grid(n_roots)), dim3(kLiveBlock), 0, s, d, roots, n_roots);
    hipLaunchKernelGGL(k8_live_advance, dim3(1), dim3(64), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_live_rounds(const LiveDev& d, uint32_t rounds, hipStream_t s) {
    const uint32_t grid = live_grid(d.n);
    for (uint32_t r = 0; r < rounds; ++r) hipLaunchKernelGGL(k8_live_round, dim3(grid), dim3(kLiveBlock), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_live_count(const LiveDev& d, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d.ctl + kLiveCounts, 0, 3 * sizeof(uint32_t), s);
    if (e != hipSuccess || !d.n) return e;
    hipLaunchKernelGGL(k8_live_count, dim3(live_grid((uint32_t)(((uint64_t)d.n + 3) / 4))), dim3(kLiveBlock), 0, s, d);
    return hipGetLastError();
}

hipError_t launch_live_list(const LiveDev& d, uint32_t state, uint64_t cap, uint32_t* tile_count, uint32_t* nodes,
                            uint64_t* d_found, hipStream_t s) {
    const uint32_t tiles = (uint32_t)(((uint64_t)d.n + kLiveListTile - 1) / kLiveListTile);
    if (tiles) hipLaunchKernelGGL(k8_live_list_count, dim3(tiles), dim3(kLiveBlock), 0, s, d, state, tile_count);
    hipError_t e = launch_tile_scan(tile_count, tiles, d_found, s);
    if (e != hipSuccess) return e;
    if (tiles && cap)
        hipLaunchKernelGGL(k8_live_list_scatter, dim3(tiles), dim3(kLiveBlock), 0, s, d, state, cap, tile_count, nodes);
    return hipGetLastError();
}

hipError_t launch_live_offsets(const LiveDev& d, const LiveRows& r, hipStream_t s) {
    const uint64_t tiles = (r.n_contrib + kLiveListTile - 1) / kLiveListTile;
    if (tiles) hipLaunchKernelGGL(k8_live_tile_rows, dim3((uint32_t)tiles), dim3(kLiveBlock), 0, s, d, r);
    hipLaunchKernelGGL(k8_live_scan64, dim3(1), dim3(1024), 0, s, d, r, tiles);
    if (tiles) hipLaunchKernelGGL(k8_live_row_offsets, dim3((uint32_t)tiles), dim3(kLiveBlock), 0, s, d, r);
    return hipGetLastError();
}

hipError_t launch_live_rows(const LiveDev& d, const LiveRows& r, const BloomDev& b, hipStream_t s) {
    if (!r.n_rows) return hipSuccess;
    hipError_t e = hipMemsetAsync(r.table, 0xff, 4ull * ((uint64_t)r.mask + 1), s);
    if (e != hipSuccess) return e;
    const uint32_t grid = items_grid(r.n_rows);
    hipLaunchKernelGGL(k8_live_locate, dim3(grid), dim3(kLiveBlock), 0, s, d, r);
    hipLaunchKernelGGL(k8_live_insert, dim3(grid), dim3(kLiveBlock), 0, s, d, r);
    hipLaunchKernelGGL(k8_live_resolve, dim3(grid < 2048 ? grid : 2048), dim3(kLiveBlock), 0, s, d, r,
                       reinterpret_cast<unsigned long long*>(b.words), b.m, b.m ? (~0ull) / b.m : 0ull, (uint32_t)b.k);
    return hipGetLastError();
}

hipError_t launch_live_compare(const LiveDev& d, const uint64_t* a, const uint64_t* b, uint64_t nwords,
                               hipStream_t s) {
    if (!nwords) return hipSuccess;
    hipLaunchKernelGGL(k8_live_compare, dim3(items_grid(nwords)), dim3(kLiveBlock), 0, s, d, a, b, nwords);
    return hipGetLastError();
}

}  // namespace rf
