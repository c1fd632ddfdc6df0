// k7_plan.hip -- K7: the top-down evaluation plan (rf_eval_plan_*).
//
// Eval.todo and Eval.lookup in top-down mode (eval.go:902-955, 1163-1269): from
// the roots, a cacheable node that is not dirty is looked up; a hit ends the
// walk there, a miss makes the node TODO and its Deps are visited.  The
// reference runs one goroutine per node and one Assoc.Get per key; here the
// walk is a frontier traversal, one launch per round, whose cut-off is the
// fused liveset probe + assoc Get of k6_feed_lookup applied per node.
//
// One append-only QUEUE holds every reached node once, in arrival order; a
// round works on queue[lo, hi) and appends behind hi.  A node enters the
// queue when a lane CLAIMS it: a returning atomicOr on its bit of the claim
// bitmap, so two parents (or a dep listed twice) queue it once; the fresh
// ones of a wave are appended with one ballot and one atomicAdd per wave, as
// k3_reach_step does.  A node flagged done is claimed but not queued: the
// claiming lane writes its DONE state.  The workgroup whose arrival add comes
// last (all the round's tail adds have returned by then) moves lo, hi to the
// appended stretch for the next launch, so the host can enqueue several
// rounds without reading anything back; an empty stretch makes a round a
// no-op.  Everything one round writes for the next (queue entries, states,
// the bounds) is read only after the kernel boundary.
//
// A node's state depends on the node alone and the reached set is a closure,
// so states, lists and counts do not depend on arrival order.  Only the order
// of the queue and of the hit rows does, and neither is an output: the lists
// come from a tile count / scan / scatter over the state array.
#include "engine.h"
#include "assoc_dev.h"
#include "bloom_dev.h"
#include "reflow_hip.h"

namespace rf {

static_assert(kPlanListTile == 4 * kPlanBlock, "a list tile is one workgroup of four-state words");

__device__ __forceinline__ bool plan_bit(const uint32_t* __restrict__ bits, uint32_t i) {
    return (bits[i >> 5] >> (i & 31)) & 1u;
}

// Every lane of the wave calls this: lanes with `has` claim node k; the fresh
// ones that are not flagged done are appended to the queue.
__device__ __forceinline__ void plan_claim(const PlanDev& p, bool has, uint32_t k, uint32_t lane) {
    bool fresh = false;
    if (has) {
        const uint32_t m = 1u << (k & 31);
        fresh = !(atomicOr(&p.claim[k >> 5], m) & m);
        if (fresh && (p.flags[k] & RF_PLAN_F_DONE)) {  // a satisfied dep: reached, not expanded
            p.state[k] = RF_PLAN_DONE;
            fresh = false;
        }
    }
    const uint64_t b = __ballot(fresh);
    if (b) {
        const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)b) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&p.ctl[kPlanTail], (uint32_t)__popcll(b));
        base = __shfl(base, leader, 64);
        const uint32_t at = base + (uint32_t)__popcll(b & lt);
        if (fresh && at < p.n) p.queue[at] = k;  // (at < n always: a node is claimed fresh once)
    }
}

// Every lane of the wave calls this: lanes with `miss` visit their node's
// Deps.  Nodes of degree < 64 go lane per node in wave lockstep; a node of
// degree >= 64 (the wide OpK / Merge fan-ins) is taken by the whole wave, 64
// deps at a time.
__device__ __forceinline__ void plan_expand(const PlanDev& p, bool miss, uint32_t node, uint32_t lane) {
    uint64_t c = 0, ce = 0;
    if (miss) {
        c = p.dep_ptr[node];
        ce = p.dep_ptr[node + 1];
    }
    const bool wide = ce - c >= 64;
    uint64_t wides = __ballot(wide);
    uint64_t c1 = wide ? ce : c;
    while (__any(c1 < ce)) {
        const bool has = c1 < ce;
        uint32_t k = 0;
        if (has) k = p.deps[c1++];
        plan_claim(p, has, k, lane);
    }
    while (wides) {
        const int src = __ffsll((unsigned long long)wides) - 1;
        wides &= wides - 1;
        const uint64_t b0 = (uint64_t)__shfl((unsigned long long)c, src, 64);
        const uint64_t e0 = (uint64_t)__shfl((unsigned long long)ce, src, 64);
        for (uint64_t x = b0; x < e0; x += 64) {
            const bool has = x + lane < e0;
            uint32_t k = 0;
            if (has) k = p.deps[x + lane];
            plan_claim(p, has, k, lane);
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// lo = hi, hi = tail: the stretch appended since the last move is the next frontier
__global__ void k7_plan_advance(PlanDev p) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.ctl[kPlanLo] = p.ctl[kPlanHi];
        p.ctl[kPlanHi] = p.ctl[kPlanTail];
    }
}

// The listed roots: marked as roots (eval.go:1173 f == e.root) and claimed.
__global__ __launch_bounds__(kPlanBlock) void k7_plan_seed(PlanDev p, const uint32_t* __restrict__ roots,
                                                           uint32_t n_roots) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kPlanBlock; base < n_roots; base += (uint64_t)gridDim.x * kPlanBlock) {
        const uint64_t i = base + threadIdx.x;
        const bool has = i < n_roots;
        uint32_t k = 0;
        if (has) {
            k = roots[i];
            atomicOr(&p.rootbit[k >> 5], 1u << (k & 31));
        }
        plan_claim(p, has, k, lane);
    }
}

// One round: lane per frontier node -- eligibility, every key through the
// liveset and the assoc, the state -- then the misses' Deps.
__global__ __launch_bounds__(kPlanBlock) void k7_plan_round(PlanDev p, PlanLook l) {
    const uint32_t lo = p.ctl[kPlanLo], hi = p.ctl[kPlanHi];
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t length = l.words ? *l.len_dev : 0;
    uint32_t n_look = 0, n_probe = 0, n_filt = 0;
    for (uint64_t base = lo + (uint64_t)blockIdx.x * kPlanBlock; base < hi; base += (uint64_t)gridDim.x * kPlanBlock) {
        const uint64_t i = base + threadIdx.x;
        bool miss = false;
        uint32_t node = 0;
        if (i < hi) {
            node = p.queue[i];
            const uint32_t f = p.flags[node];
            const uint64_t k0 = p.key_ptr[node];
            const uint32_t nk = (uint32_t)(p.key_ptr[node + 1] - k0);
            // eval.go:908-913 (cacheable, not dirty), :1173 (valid; under
            // NoCacheExtern no extern and not the root), :1183-1188 (has keys)
            bool look = (f & RF_PLAN_F_CACHEABLE) && !(f & RF_PLAN_F_INVALID) && nk;
            if (look && l.no_cache_extern)
                look = !((f & RF_PLAN_F_EXTERN) || plan_bit(p.rootbit, node) || (l.dirty && plan_bit(l.dirty, node)));
            uint32_t which = 0xffu, fmask = 0;
            uint4 va = make_uint4(0, 0, 0, 0), vb = va;
            if (look) {
                ++n_look;
                for (uint32_t j = 0; j < nk; ++j) {  // every key, as rf_assoc_lookup: precise read repair
                    const uint64_t row = l.by_slot ? (uint64_t)p.key_slots[k0 + j] : k0 + j;
                    const uint8_t* kp = l.keys + 32ull * row;
                    if (l.words && !bloom_contains(l.words, length, l.m, l.mu, l.k, kp)) {
                        ++n_filt;
                        continue;
                    }
                    ++n_probe;
                    const uint4* k4 = reinterpret_cast<const uint4*>(kp);
                    const uint4 klo = k4[0], khi = k4[1];
                    const uint32_t slot = assoc_find(l.t, l.kind, klo, khi);
                    if (slot == kEmpty) continue;
                    const uint4 a = l.t.vals[2 * slot], b = l.t.vals[2 * slot + 1];
                    if ((a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0) continue;  // deleted: NotExist
                    fmask |= 1u << j;
                    if (which == 0xffu) {
                        which = j;
                        va = a;
                        vb = b;
                    }
                }
            }
            p.found[node] = (uint8_t)fmask;
            p.which[node] = (uint8_t)which;
            if (which != 0xffu) {
                const uint32_t r = atomicAdd(&p.ctl[kPlanHits], 1u);
                p.hitrow[node] = r;
                if (r < p.row_cap) {  // (always: a node is looked up once between two runs)
                    p.rows[2ull * r] = va;
                    p.rows[2ull * r + 1] = vb;
                }
                p.state[node] = RF_PLAN_HIT;
            } else {
                p.state[node] = RF_PLAN_TODO;
                miss = true;
            }
        }
        plan_expand(p, miss, node, lane);
    }
    n_look = wave_sum(n_look);
    n_probe = wave_sum(n_probe);
    n_filt = wave_sum(n_filt);
    if (lane == 0) {
        if (n_look) atomicAdd(&p.ctl[kPlanLooked], n_look);
        if (n_probe) atomicAdd(&p.ctl[kPlanProbed], n_probe);
        if (n_filt) atomicAdd(&p.ctl[kPlanFiltered], n_filt);
    }
    __syncthreads();  // every wave's tail adds have returned
    if (threadIdx.x == 0) {
        const uint32_t before = atomicAdd(&p.ctl[kPlanArrived], 1u);
        if (before == gridDim.x - 1) {  // the last workgroup through: the next launch's bounds
            const uint32_t tail = atomicAdd(&p.ctl[kPlanTail], 0u);
            p.ctl[kPlanLo] = hi;
            p.ctl[kPlanHi] = tail;
            atomicExch(&p.ctl[kPlanArrived], 0u);
        }
    }
}

// reject 1/2: is every listed node a hit?
__global__ __launch_bounds__(kPlanBlock) void k7_plan_reject_check(PlanDev p, const uint32_t* __restrict__ nodes,
                                                                   uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kPlanBlock)
        if (p.state[nodes[i]] != RF_PLAN_HIT) atomicOr(&p.ctl[kPlanBad], 1u);
}

// reject 2/2: the listed hits become TODO (eval.go:1268 lookupFailed) and their Deps are visited.
__global__ __launch_bounds__(kPlanBlock) void k7_plan_reject(PlanDev p, const uint32_t* __restrict__ nodes,
                                                             uint32_t n) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kPlanBlock; base < n; base += (uint64_t)gridDim.x * kPlanBlock) {
        const uint64_t i = base + threadIdx.x;
        const bool has = i < n;
        uint32_t node = 0;
        if (has) {
            node = nodes[i];
            p.state[node] = RF_PLAN_TODO;
        }
        plan_expand(p, has, node, lane);
    }
}

// After the fixed point, lane per TODO node: READY iff every dep is DONE or
// HIT (eval.go:930-953; vacuous with no deps).  Neither of those states is
// written here, so the answer does not depend on what other lanes have done.
__global__ __launch_bounds__(kPlanBlock) void k7_plan_ready(PlanDev p) {
    for (uint64_t i = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; i < p.n; i += (uint64_t)gridDim.x * kPlanBlock) {
        const uint8_t s = p.state[i];
        if (s != RF_PLAN_TODO && s != RF_PLAN_READY) continue;
        bool ready = true;
        for (uint64_t e = p.dep_ptr[i], ee = p.dep_ptr[i + 1]; e < ee && ready; ++e) {
            const uint8_t d = p.state[p.deps[e]];
            ready = d == RF_PLAN_HIT || d == RF_PLAN_DONE;
        }
        const uint8_t want = ready ? RF_PLAN_READY : RF_PLAN_TODO;
        if (want != s) p.state[i] = want;
    }
}

// Nodes per state (counts zeroed by the host), four state bytes per lane.
__global__ __launch_bounds__(kPlanBlock) void k7_plan_count(PlanDev p) {
    const uint32_t* __restrict__ w4 = reinterpret_cast<const uint32_t*>(p.state);
    const uint64_t words = ((uint64_t)p.n + 3) / 4;
    uint32_t c[5] = {0, 0, 0, 0, 0};
    for (uint64_t w = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; w < words; w += (uint64_t)gridDim.x * kPlanBlock) {
        const uint32_t v = w4[w];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t s = (v >> (8 * j)) & 0xffu;
            if (4 * w + j < p.n) {
#pragma unroll
                for (uint32_t q = 0; q < 5; ++q) c[q] += s == q;
            }
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 5; ++q) {
        const uint32_t t = wave_sum(c[q]);
        if ((threadIdx.x & 63) == 0 && t) atomicAdd(&p.ctl[kPlanCounts + q], t);
    }
}

// A lane's four nodes of tile blockIdx.x that are in `state`: a 4-bit mask.
__device__ __forceinline__ uint32_t plan_tile_mask(const PlanDev& p, uint32_t state, uint64_t first) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p.state + first);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (((v >> (8 * j)) & 0xffu) == state && first + j < p.n) m |= 1u << j;
    return m;
}

// List 1/3: per tile, the nodes in `state`.
__global__ __launch_bounds__(kPlanBlock) void k7_plan_list_count(PlanDev p, uint32_t state,
                                                                 uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t s_cnt[kPlanBlock / 64];
    const uint64_t first = ((uint64_t)blockIdx.x * kPlanBlock + threadIdx.x) * 4;
    const uint32_t cnt = wave_sum((uint32_t)__builtin_popcount(plan_tile_mask(p, state, first)));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < kPlanBlock / 64; ++k) c += s_cnt[k];
        tile_count[blockIdx.x] = c;
    }
}

// List 3/3: per tile, ascending node id; ranks below cap are written.  For
// hits: the first key with a value, that value (from the node's hit row) and
// the found mask.
__global__ __launch_bounds__(kPlanBlock) void k7_plan_list_scatter(PlanDev p, uint32_t state, uint64_t cap,
                                                                   const uint32_t* __restrict__ tile_count,
                                                                   uint32_t* __restrict__ nodes,
                                                                   uint8_t* __restrict__ which,
                                                                   uint8_t* __restrict__ vals,
                                                                   uint8_t* __restrict__ key_found) {
    __shared__ uint32_t s_w[kPlanBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t rank = tile_count[blockIdx.x];  // (exclusive, after the tile scan)
    if (rank >= cap) return;                 // uniform over the block
    const uint64_t first = ((uint64_t)blockIdx.x * kPlanBlock + threadIdx.x) * 4;
    const uint32_t m = plan_tile_mask(p, state, first);
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
    for (uint32_t q = m; q && rank < cap; q &= q - 1, ++rank) {
        const uint32_t id = (uint32_t)(first + (uint32_t)__builtin_ctz(q));
        nodes[rank] = id;
        if (state == RF_PLAN_HIT) {
            if (which) which[rank] = p.which[id];
            if (key_found) key_found[rank] = p.found[id];
            if (vals) {
                const uint32_t r = p.hitrow[id];
                uint4 a = make_uint4(0, 0, 0, 0), b = a;
                if (r < p.row_cap) {
                    a = p.rows[2ull * r];
                    b = p.rows[2ull * r + 1];
                }
                uint4* o = reinterpret_cast<uint4*>(vals + 32ull * rank);
                o[0] = a;
                o[1] = b;
            }
        }
    }
}

// rf_eval_plan_set_flags: flags[nodes[i]] = vals[i] (a node listed twice carries the same value twice)
__global__ __launch_bounds__(kPlanBlock) void k7_plan_set_flags(uint8_t* __restrict__ flags,
                                                                const uint32_t* __restrict__ nodes,
                                                                const uint8_t* __restrict__ vals, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kPlanBlock)
        flags[nodes[i]] = vals[i];
}

uint32_t plan_grid(uint32_t n) {
    const uint32_t g = (n + kPlanBlock - 1) / kPlanBlock;
    return g < 1 ? 1 : g > kPlanMaxGrid ? kPlanMaxGrid : g;
}

static uint32_t items_grid(uint64_t items) {
    const uint64_t g = (items + kPlanBlock - 1) / kPlanBlock;
    return (uint32_t)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

hipError_t launch_plan_set_flags(uint8_t* flags, const uint32_t* nodes, const uint8_t* vals, uint32_t n,
                                 hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k7_plan_set_flags, dim3(items_grid(n)), dim3(kPlanBlock), 0, s, flags, nodes, vals, n);
    return hipGetLastError();
}

hipError_t launch_plan_seed(const PlanDev& p, const uint32_t* roots, uint32_t n_roots, hipStream_t s) {
    if (n_roots) hipLaunchKernelGGL(k7_plan_seed, dim3(items_grid(n_roots)), dim3(kPlanBlock), 0, s, p, roots, n_roots);
    hipLaunchKernelGGL(k7_plan_advance, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_plan_rounds(const PlanDev& p, const PlanLook& l, uint32_t rounds, hipStream_t s) {
    const uint32_t grid = plan_grid(p.n);
    for (uint32_t r = 0; r < rounds; ++r) hipLaunchKernelGGL(k7_plan_round, dim3(grid), dim3(kPlanBlock), 0, s, p, l);
    return hipGetLastError();
}

hipError_t launch_plan_reject_check(const PlanDev& p, const uint32_t* nodes, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k7_plan_reject_check, dim3(items_grid(n)), dim3(kPlanBlock), 0, s, p, nodes, n);
    return hipGetLastError();
}

hipError_t launch_plan_reject(const PlanDev& p, const uint32_t* nodes, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(k7_plan_reject, dim3(items_grid(n)), dim3(kPlanBlock), 0, s, p, nodes, n);
    hipLaunchKernelGGL(k7_plan_advance, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_plan_finish(const PlanDev& p, hipStream_t s) {
    hipError_t e = hipMemsetAsync(p.ctl + kPlanCounts, 0, 5 * sizeof(uint32_t), s);
    if (e != hipSuccess || !p.n) return e;
    hipLaunchKernelGGL(k7_plan_ready, dim3(items_grid(p.n)), dim3(kPlanBlock), 0, s, p);
    hipLaunchKernelGGL(k7_plan_count, dim3(items_grid(((uint64_t)p.n + 3) / 4)), dim3(kPlanBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_plan_list(const PlanDev& p, uint32_t state, uint64_t cap, uint32_t* tile_count, uint32_t* nodes,
                            uint8_t* which, uint8_t* vals, uint8_t* key_found, uint64_t* d_found, hipStream_t s) {
    const uint32_t tiles = (uint32_t)(((uint64_t)p.n + kPlanListTile - 1) / kPlanListTile);
    if (tiles) hipLaunchKernelGGL(k7_plan_list_count, dim3(tiles), dim3(kPlanBlock), 0, s, p, state, tile_count);
    hipError_t e = launch_tile_scan(tile_count, tiles, d_found, s);
    if (e != hipSuccess) return e;
    if (tiles && cap)
        hipLaunchKernelGGL(k7_plan_list_scatter, dim3(tiles), dim3(kPlanBlock), 0, s, p, state, cap, tile_count, nodes,
                           which, vals, key_found);
    return hipGetLastError();
}

}  // namespace rf
