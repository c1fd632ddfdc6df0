// k10_wave.hip -- K10: evaluation waves driven by completions (rf_eval_wave_*).
//
// Eval.todo and Eval.lookup in bottom-up mode (eval.go:902-955, 1163-1269), and
// what Eval.todo does after the first round in either mode: a node whose deps
// are all done goes to NeedTransfer (:930-947), in bottom-up mode after a
// lookup (:940-941).  The reference walks the whole graph from the roots on
// every scheduling step; here every node carries PENDING, the number of its
// dep entries whose dep has not finished, and a step walks from the nodes that
// just finished to their consumers.
//
// begin (bottom-up): a descent from the roots, k7's traversal without its
// lookups -- a claim bitmap with a returning atomicOr, one ballot and one
// atomicAdd per wave to append, nodes of degree >= 64 taken by a whole wave,
// the bounds advanced by the last workgroup through.  The lane that expands a
// node counts its pending deps from the flag bytes (which no kernel writes), so
// the count does not depend on what other lanes have done.
// step: lane per finished node, claimed once through the `fin` bitmap (a node
// listed twice counts once); every consumer entry whose consumer is TODO takes
// one returning atomicSub on its pending count, and the lane that sees 1
// appends the consumer to the WAVE QUEUE -- that lane is unique, so a node
// enters exactly one wave.  The listed nodes are READY or HIT and their
// consumers TODO, so no lane reads a state byte another lane writes.
// resolve: lane per wave-queue entry -- in bottom-up mode the plan's lookup
// (liveset probe, assoc Get of every present key), else READY at once.
//
// Everything one kernel writes for the next (queue entries, states, pending,
// the bounds) is read only after the kernel boundary.  A node's wave depends
// only on the set of nodes finished so far and its state on the node alone, so
// states, lists and counts do not depend on arrival order; only the order of
// the queues and of the hit rows does, and neither is an output.
#include <algorithm>

#include "wave_internal.h"
#include "assoc_dev.h"
#include "bloom_dev.h"
#include "reflow_hip.h"

namespace rf {

__device__ __forceinline__ bool wv_bit(const uint32_t* __restrict__ bits, uint32_t i) {
    return (bits[i >> 5] >> (i & 31)) & 1u;
}

__device__ __forceinline__ uint32_t wv_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Every lane of the wave calls this: the lanes with `has` append k to q behind
// *tail with one ballot and one atomicAdd per wave.
__device__ __forceinline__ void wv_append(uint32_t* __restrict__ q, uint32_t* tail, uint32_t cap, bool has, uint32_t k,
                                          uint32_t lane) {
    const uint64_t b = __ballot(has);
    if (b) {
        const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)b) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(tail, (uint32_t)__popcll(b));
        base = __shfl(base, leader, 64);
        const uint32_t at = base + (uint32_t)__popcll(b & lt);
        if (has && at < cap) q[at] = k;  // (at < n always: a node enters a queue once per begin)
    }
}

// Every lane of the wave calls this: lanes with `has` claim node k for the
// descent; a fresh one that is flagged done is DONE and not queued.
__device__ __forceinline__ void wv_claim(const WaveDev& w, bool has, uint32_t k, uint32_t lane) {
    bool fresh = false;
    if (has) {
        const uint32_t m = 1u << (k & 31);
        fresh = !(atomicOr(&w.claim[k >> 5], m) & m);
        if (fresh && (w.flags[k] & RF_PLAN_F_DONE)) {
            w.state[k] = RF_PLAN_DONE;
            fresh = false;
        }
    }
    wv_append(w.queue, &w.ctl[kWaveTail], w.n, fresh, k, lane);
}

// Every lane of the wave calls this: lanes with `has` make their node TODO,
// reach its Deps and count the pending ones; a node with none joins wave 0.
__device__ __forceinline__ void wv_descend(const WaveDev& w, bool has, uint32_t node, uint32_t lane) {
    uint64_t c = 0, ce = 0;
    if (has) {
        c = w.dep_ptr[node];
        ce = w.dep_ptr[node + 1];
        w.state[node] = RF_PLAN_TODO;
    }
    const bool wide = ce - c >= 64;
    uint64_t wides = __ballot(wide);
    uint64_t c1 = wide ? ce : c;
    uint32_t pend = 0;
    while (__any(c1 < ce)) {
        const bool h = c1 < ce;
        uint32_t k = 0;
        if (h) {
            k = w.deps[c1++];
            pend += !(w.flags[k] & RF_PLAN_F_DONE);
        }
        wv_claim(w, h, k, lane);
    }
    while (wides) {
        const int src = __ffsll((unsigned long long)wides) - 1;
        wides &= wides - 1;
        const uint64_t b0 = (uint64_t)__shfl((unsigned long long)c, src, 64);
        const uint64_t e0 = (uint64_t)__shfl((unsigned long long)ce, src, 64);
        uint32_t cnt = 0;
        for (uint64_t x = b0; x < e0; x += 64) {
            const bool h = x + lane < e0;
            uint32_t k = 0;
            bool open = false;
            if (h) {
                k = w.deps[x + lane];
                open = !(w.flags[k] & RF_PLAN_F_DONE);
            }
            cnt += (uint32_t)__popcll(__ballot(open));
            wv_claim(w, h, k, lane);
        }
        if (lane == (uint32_t)src) pend = cnt;
    }
    if (has) w.pending[node] = pend;
    wv_append(w.wq, &w.ctl[kWaveWTail], w.n, has && pend == 0, node, lane);
}

// lo = hi, hi = tail: the stretch appended since the last move is the next frontier
__global__ void k10_wave_advance(WaveDev w) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        w.ctl[kWaveLo] = w.ctl[kWaveHi];
        w.ctl[kWaveHi] = w.ctl[kWaveTail];
    }
}

// The listed roots: marked as roots (eval.go:1173 f == e.root) and claimed.
__global__ __launch_bounds__(kPlanBlock) void k10_wave_seed(WaveDev w, const uint32_t* __restrict__ roots,
                                                            uint32_t n_roots) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kPlanBlock; base < n_roots; base += (uint64_t)gridDim.x * kPlanBlock) {
        const uint64_t i = base + threadIdx.x;
        const bool has = i < n_roots;
        uint32_t k = 0;
        if (has) {
            k = roots[i];
            atomicOr(&w.rootbit[k >> 5], 1u << (k & 31));
        }
        wv_claim(w, has, k, lane);
    }
}

// One descent round over queue[lo, hi): no lookups on the way down (eval.go:910).
__global__ __launch_bounds__(kPlanBlock) void k10_wave_descend(WaveDev w) {
    const uint32_t lo = w.ctl[kWaveLo], hi = w.ctl[kWaveHi];
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = lo + (uint64_t)blockIdx.x * kPlanBlock; base < hi; base += (uint64_t)gridDim.x * kPlanBlock) {
        const uint64_t i = base + threadIdx.x;
        const bool has = i < hi;
        wv_descend(w, has, has ? w.queue[i] : 0u, lane);
    }
    __syncthreads();  // every wave's tail adds have returned
    if (threadIdx.x == 0) {
        const uint32_t before = atomicAdd(&w.ctl[kWaveArrived], 1u);
        if (before == gridDim.x - 1) {  // the last workgroup through: the next launch's bounds
            const uint32_t tail = atomicAdd(&w.ctl[kWaveTail], 0u);
            w.ctl[kWaveLo] = hi;
            w.ctl[kWaveHi] = tail;
            atomicExch(&w.ctl[kWaveArrived], 0u);
        }
    }
}

// begin from states 1/2: a byte above DONE, or a TODO / READY node over an UNSEEN dep?
__global__ __launch_bounds__(kPlanBlock) void k10_wave_states_check(WaveDev w, const uint8_t* __restrict__ in) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; i < w.n; i += (uint64_t)gridDim.x * kPlanBlock) {
        const uint8_t s = in[i];
        if (s > RF_PLAN_DONE) bad = true;
        if (s != RF_PLAN_TODO && s != RF_PLAN_READY) continue;
        for (uint64_t e = w.dep_ptr[i], ee = w.dep_ptr[i + 1]; e < ee; ++e)
            if (in[w.deps[e]] == RF_PLAN_UNSEEN) bad = true;
    }
    if (bad) atomicOr(&w.ctl[kWaveBad], 1u);
}

// begin from states 2/2: TODO and READY are tracked (TODO here; wave 0 is
// resolved next), HIT and DONE are satisfied (DONE), UNSEEN stays.  pending =
// the dep entries whose dep is tracked (eval.go:930-947).
__global__ __launch_bounds__(kPlanBlock) void k10_wave_states_apply(WaveDev w, const uint8_t* __restrict__ in) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kPlanBlock; base < w.n; base += (uint64_t)gridDim.x * kPlanBlock) {
        const uint64_t i = base + threadIdx.x;
        bool ready = false;
        if (i < w.n) {
            const uint8_t s = in[i];
            uint8_t out = RF_PLAN_UNSEEN;
            if (s == RF_PLAN_TODO || s == RF_PLAN_READY) {
                uint32_t pend = 0;
                for (uint64_t e = w.dep_ptr[i], ee = w.dep_ptr[i + 1]; e < ee; ++e) {
                    const uint8_t d = in[w.deps[e]];
                    pend += d == RF_PLAN_TODO || d == RF_PLAN_READY;
                }
                w.pending[i] = pend;
                ready = pend == 0;
                out = RF_PLAN_TODO;
            } else if (s == RF_PLAN_HIT || s == RF_PLAN_DONE) {
                out = RF_PLAN_DONE;
            }
            w.state[i] = out;
        }
        wv_append(w.wq, &w.ctl[kWaveWTail], w.n, ready, (uint32_t)i, lane);
    }
}

// step 1/2: is every listed node READY or HIT?
__global__ __launch_bounds__(kPlanBlock) void k10_wave_step_check(WaveDev w, const uint32_t* __restrict__ nodes,
                                                                  uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kPlanBlock) {
        const uint8_t s = w.state[nodes[i]];
        if (s != RF_PLAN_READY && s != RF_PLAN_HIT) atomicOr(&w.ctl[kWaveBad], 1u);
    }
}

// Every lane of the wave calls this: lanes with `has` take one decrement off
// consumer k if it is tracked; the lane whose decrement is the last queues it.
__device__ __forceinline__ void wv_release(const WaveDev& w, bool has, uint32_t k, uint32_t lane) {
    bool ready = false;
    if (has && w.state[k] == RF_PLAN_TODO) ready = atomicSub(&w.pending[k], 1u) == 1u;
    wv_append(w.wq, &w.ctl[kWaveWTail], w.n, ready, k, lane);
}

// step 2/2: the listed nodes become DONE; their consumer entries are
// expanded as the plan expands Deps -- lane per node under 64 consumers, a
// whole wave above.
__global__ __launch_bounds__(kPlanBlock) void k10_wave_complete(WaveDev w, const uint32_t* __restrict__ nodes,
                                                                uint32_t n) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kPlanBlock; base < n; base += (uint64_t)gridDim.x * kPlanBlock) {
        const uint64_t i = base + threadIdx.x;
        uint64_t c = 0, ce = 0;
        if (i < n) {
            const uint32_t node = nodes[i];
            const uint32_t m = 1u << (node & 31);
            if (!(atomicOr(&w.fin[node >> 5], m) & m)) {  // a node listed twice counts once
                w.state[node] = RF_PLAN_DONE;
                c = w.cons_ptr[node];
                ce = w.cons_ptr[node + 1];
            }
        }
        const bool wide = ce - c >= 64;
        uint64_t wides = __ballot(wide);
        uint64_t c1 = wide ? ce : c;
        while (__any(c1 < ce)) {
            const bool h = c1 < ce;
            uint32_t k = 0;
            if (h) k = w.cons[c1++];
            wv_release(w, h, k, lane);
        }
        while (wides) {
            const int src = __ffsll((unsigned long long)wides) - 1;
            wides &= wides - 1;
            const uint64_t b0 = (uint64_t)__shfl((unsigned long long)c, src, 64);
            const uint64_t e0 = (uint64_t)__shfl((unsigned long long)ce, src, 64);
            for (uint64_t x = b0; x < e0; x += 64) {
                const bool h = x + lane < e0;
                uint32_t k = 0;
                if (h) k = w.cons[x + lane];
                wv_release(w, h, k, lane);
            }
        }
    }
}

// The wave queue resolved, lane per node: a member of the last wave; in
// bottom-up mode looked up if eligible (eval.go:1173, 1183-1188; Eval.dirty is
// todo's business, not lookup's), every present key through the liveset and
// the assoc as k7_plan_round does; HIT, or READY (lookupFailed bottom-up is
// NeedTransfer, eval.go:1163-1166).  A key row of zeros is absent
// (flow.go:762-774, 798-800): not probed, not counted, its found bit clear.
__global__ __launch_bounds__(kPlanBlock) void k10_wave_resolve(WaveDev w, WaveLook l) {
    const uint32_t hi = w.ctl[kWaveWTail] < w.n ? w.ctl[kWaveWTail] : w.n;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t length = l.words ? *l.len_dev : 0;
    uint32_t n_look = 0, n_probe = 0, n_filt = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; i < hi; i += (uint64_t)gridDim.x * kPlanBlock) {
        const uint32_t node = w.wq[i];
        atomicOr(&w.last[node >> 5], 1u << (node & 31));
        uint32_t which = 0xffu, fmask = 0;
        uint4 va = make_uint4(0, 0, 0, 0), vb = va;
        if (l.lookup) {
            const uint32_t f = w.flags[node];
            const uint64_t k0 = w.key_ptr[node];
            const uint32_t nk = (uint32_t)(w.key_ptr[node + 1] - k0);
            bool look = (f & RF_PLAN_F_CACHEABLE) && !(f & RF_PLAN_F_INVALID) && nk;
            if (look && l.no_cache_extern) look = !((f & RF_PLAN_F_EXTERN) || wv_bit(w.rootbit, node));
            if (look) {
                bool present = false;
                for (uint32_t j = 0; j < nk; ++j) {
                    const uint64_t row = l.by_slot ? (uint64_t)w.key_slots[k0 + j] : k0 + j;
                    const uint8_t* kp = l.keys + 32ull * row;
                    const uint4* k4 = reinterpret_cast<const uint4*>(kp);
                    const uint4 klo = k4[0], khi = k4[1];
                    if ((klo.x | klo.y | klo.z | klo.w | khi.x | khi.y | khi.z | khi.w) == 0) continue;  // absent
                    present = true;
                    if (l.words && !bloom_contains(l.words, length, l.m, l.mu, l.k, kp)) {
                        ++n_filt;
                        continue;
                    }
                    ++n_probe;
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
                n_look += present;
            }
        }
        w.found[node] = (uint8_t)fmask;
        w.which[node] = (uint8_t)which;
        if (which != 0xffu) {
            const uint32_t r = atomicAdd(&w.ctl[kWaveHits], 1u);
            w.hitrow[node] = r;
            if (r < w.row_cap) {  // (always: a node is looked up once between two begins)
                w.rows[2ull * r] = va;
                w.rows[2ull * r + 1] = vb;
            }
            w.state[node] = RF_PLAN_HIT;
        } else {
            w.state[node] = RF_PLAN_READY;
        }
    }
    n_look = wv_sum(n_look);
    n_probe = wv_sum(n_probe);
    n_filt = wv_sum(n_filt);
    if (lane == 0) {
        if (n_look) atomicAdd(&w.ctl[kWaveLooked], n_look);
        if (n_probe) atomicAdd(&w.ctl[kWaveProbed], n_probe);
        if (n_filt) atomicAdd(&w.ctl[kWaveFiltered], n_filt);
    }
}

// reject 1/2: is every listed node a hit?
__global__ __launch_bounds__(kPlanBlock) void k10_wave_reject_check(WaveDev w, const uint32_t* __restrict__ nodes,
                                                                    uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kPlanBlock)
        if (w.state[nodes[i]] != RF_PLAN_HIT) atomicOr(&w.ctl[kWaveBad], 1u);
}

// reject 2/2: the listed hits become READY (eval.go:1268 lookupFailed, bottom-up: NeedTransfer)
__global__ __launch_bounds__(kPlanBlock) void k10_wave_reject(WaveDev w, const uint32_t* __restrict__ nodes,
                                                              uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kPlanBlock)
        w.state[nodes[i]] = RF_PLAN_READY;
}

// Nodes per state (counts zeroed by the host), four state bytes per lane; the
// grid is small and strides, and a workgroup adds its five sums once, so the
// five counters take a few thousand atomics however large the graph is.
__global__ __launch_bounds__(kPlanBlock) void k10_wave_count(WaveDev w) {
    __shared__ uint32_t s_c[kPlanBlock / 64][5];
    const uint32_t* __restrict__ w4 = reinterpret_cast<const uint32_t*>(w.state);
    const uint64_t words = ((uint64_t)w.n + 3) / 4;
    uint32_t c[5] = {0, 0, 0, 0, 0};
    for (uint64_t x = (uint64_t)blockIdx.x * kPlanBlock + threadIdx.x; x < words; x += (uint64_t)gridDim.x * kPlanBlock) {
        const uint32_t v = w4[x];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t s = (v >> (8 * j)) & 0xffu;
            if (4 * x + j < w.n) {
#pragma unroll
                for (uint32_t q = 0; q < 5; ++q) c[q] += s == q;
            }
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 5; ++q) {
        const uint32_t t = wv_sum(c[q]);
        if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6][q] = t;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        uint32_t t = 0;
        for (uint32_t k = 0; k < kPlanBlock / 64; ++k) t += s_c[k][threadIdx.x];
        if (t) atomicAdd(&w.ctl[kWaveCounts + threadIdx.x], t);
    }
}

// A lane's four nodes (first is a multiple of 4) that are in `state` and, with
// only_last, members of the last wave: a 4-bit mask.
__device__ __forceinline__ uint32_t wv_tile_mask(const WaveDev& w, uint32_t state, bool only_last, uint64_t first) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(w.state + first);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (((v >> (8 * j)) & 0xffu) == state && first + j < w.n) m |= 1u << j;
    if (only_last && m) m &= (w.last[first >> 5] >> (first & 31)) & 0xfu;
    return m;
}

// List 1/3: per tile, the nodes in `state` (and in the last wave).
__global__ __launch_bounds__(kPlanBlock) void k10_wave_list_count(WaveDev w, uint32_t state, bool only_last,
                                                                  uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t s_cnt[kPlanBlock / 64];
    const uint64_t first = ((uint64_t)blockIdx.x * kPlanBlock + threadIdx.x) * 4;
    const uint32_t cnt = wv_sum((uint32_t)__builtin_popcount(wv_tile_mask(w, state, only_last, first)));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < kPlanBlock / 64; ++k) c += s_cnt[k];
        tile_count[blockIdx.x] = c;
    }
}

// List 3/3: per tile, ascending node id; ranks below cap are written.
__global__ __launch_bounds__(kPlanBlock) void k10_wave_list_scatter(WaveDev w, uint32_t state, bool only_last,
                                                                    uint64_t cap,
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
    const uint32_t m = wv_tile_mask(w, state, only_last, first);
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
            if (which) which[rank] = w.which[id];
            if (key_found) key_found[rank] = w.found[id];
            if (vals) {
                const uint32_t r = w.hitrow[id];
                uint4 a = make_uint4(0, 0, 0, 0), b = a;
                if (r < w.row_cap) {
                    a = w.rows[2ull * r];
                    b = w.rows[2ull * r + 1];
                }
                uint4* o = reinterpret_cast<uint4*>(vals + 32ull * rank);
                o[0] = a;
                o[1] = b;
            }
        }
    }
}

static uint32_t items_grid(uint64_t items) {
    const uint64_t g = (items + kPlanBlock - 1) / kPlanBlock;
    return (uint32_t)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

hipError_t launch_wave_seed(const WaveDev& w, const uint32_t* roots, uint32_t n_roots, hipStream_t s) {
    if (n_roots) hipLaunchKernelGGL(k10_wave_seed, dim3(items_grid(n_roots)), dim3(kPlanBlock), 0, s, w, roots, n_roots);
    hipLaunchKernelGGL(k10_wave_advance, dim3(1), dim3(64), 0, s, w);
    return hipGetLastError();
}

hipError_t launch_wave_descend(const WaveDev& w, uint32_t rounds, hipStream_t s) {
    const uint32_t grid = plan_grid(w.n);
    for (uint32_t r = 0; r < rounds; ++r) hipLaunchKernelGGL(k10_wave_descend, dim3(grid), dim3(kPlanBlock), 0, s, w);
    return hipGetLastError();
}

hipError_t launch_wave_states_check(const WaveDev& w, const uint8_t* in, hipStream_t s) {
    if (!w.n) return hipSuccess;
    hipLaunchKernelGGL(k10_wave_states_check, dim3(items_grid(w.n)), dim3(kPlanBlock), 0, s, w, in);
    return hipGetLastError();
}

hipError_t launch_wave_states_apply(const WaveDev& w, const uint8_t* in, hipStream_t s) {
    if (!w.n) return hipSuccess;
    hipLaunchKernelGGL(k10_wave_states_apply, dim3(items_grid(w.n)), dim3(kPlanBlock), 0, s, w, in);
    return hipGetLastError();
}

hipError_t launch_wave_step_check(const WaveDev& w, const uint32_t* nodes, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k10_wave_step_check, dim3(items_grid(n)), dim3(kPlanBlock), 0, s, w, nodes, n);
    return hipGetLastError();
}

hipError_t launch_wave_complete(const WaveDev& w, const uint32_t* nodes, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k10_wave_complete, dim3(items_grid(n)), dim3(kPlanBlock), 0, s, w, nodes, n);
    return hipGetLastError();
}

hipError_t launch_wave_resolve(const WaveDev& w, const WaveLook& l, hipStream_t s) {
    if (!w.n) return hipSuccess;
    hipLaunchKernelGGL(k10_wave_resolve, dim3(plan_grid(w.n)), dim3(kPlanBlock), 0, s, w, l);
    return hipGetLastError();
}

hipError_t launch_wave_reject_check(const WaveDev& w, const uint32_t* nodes, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k10_wave_reject_check, dim3(items_grid(n)), dim3(kPlanBlock), 0, s, w, nodes, n);
    return hipGetLastError();
}

hipError_t launch_wave_reject(const WaveDev& w, const uint32_t* nodes, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k10_wave_reject, dim3(items_grid(n)), dim3(kPlanBlock), 0, s, w, nodes, n);
    return hipGetLastError();
}

hipError_t launch_wave_count(const WaveDev& w, hipStream_t s) {
    hipError_t e = hipMemsetAsync(w.ctl + kWaveCounts, 0, 5 * sizeof(uint32_t), s);
    if (e != hipSuccess || !w.n) return e;
    const uint32_t grid = std::min(items_grid(((uint64_t)w.n + 3) / 4), 512u);
    hipLaunchKernelGGL(k10_wave_count, dim3(grid), dim3(kPlanBlock), 0, s, w);
    return hipGetLastError();
}

hipError_t launch_wave_list(const WaveDev& w, uint32_t state, bool only_last, uint64_t cap, uint32_t* tile_count,
                            uint32_t* nodes, uint8_t* which, uint8_t* vals, uint8_t* key_found, uint64_t* d_found,
                            hipStream_t s) {
    const uint32_t tiles = (uint32_t)(((uint64_t)w.n + kPlanListTile - 1) / kPlanListTile);
    if (tiles)
        hipLaunchKernelGGL(k10_wave_list_count, dim3(tiles), dim3(kPlanBlock), 0, s, w, state, only_last, tile_count);
    hipError_t e = launch_tile_scan(tile_count, tiles, d_found, s);
    if (e != hipSuccess) return e;
    if (tiles && cap)
        hipLaunchKernelGGL(k10_wave_list_scatter, dim3(tiles), dim3(kPlanBlock), 0, s, w, state, only_last, cap,
                           tile_count, nodes, which, vals, key_found);
    return hipGetLastError();
}

}  // namespace rf
