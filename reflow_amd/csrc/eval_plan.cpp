// eval_plan.cpp -- the top-down evaluation plan (rf_eval_plan_*): host side of
// k7_plan.hip.  Owns a Flow graph's structure on the device, seeds the roots,
// enqueues the rounds in batches with one small read-back per batch, then the
// ready pass and the counts; lists come from a tile count / scan / scatter.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "engine.h"
#include "graph_internal.h"
#include "plan_check.h"
#include "plan_internal.h"

using namespace rf;

// Rounds enqueued between two host reads.  A round on an empty frontier costs
// one launch of a grid that finds nothing to do; a host read costs a stream
// synchronisation.  RF_PLAN_BATCH overrides (0: the whole depth bound).
static uint32_t plan_round_batch(uint32_t depth) {
    uint32_t b = 4;
    if (const char* e = getenv("RF_PLAN_BATCH")) {
        const long v = atol(e);
        b = v <= 0 ? depth : (uint32_t)std::min<long>(v, 1 << 20);
    }
    return std::max<uint32_t>(b, 1);
}

struct rf_eval_plan {
    rf_ctx* ctx = nullptr;
    int device = 0;  // (kept: close must not touch a context that was destroyed first)
    uint64_t n = 0, n_deps = 0, n_keys = 0;
    uint32_t depth = 0, rounds = 0, round_batch = 1;
    bool has_slots = false;
    uint32_t max_slot = 0;
    bool ran = false;
    int last_nce = 0;
    bool dirty_valid = false;
    // host copies: the dirty closure builds its reverse edges from them
    std::vector<uint64_t> dep_ptr;
    std::vector<uint32_t> deps;
    std::vector<uint8_t> flags;
    PlanDev d;
    DevBuf b_dep_ptr, b_deps, b_flags, b_key_ptr, b_key_slots, b_claim, b_root, b_state, b_which, b_found, b_hitrow,
        b_rows, b_queue, b_ctl, b_dirty;
    DevBuf b_keys, b_ids, b_vals8;            // host-form keys; roots / listed nodes; set_flags' bytes
    DevBuf b_ln, b_lw, b_lv, b_lf, b_lcount;  // the host-form list's device outputs
    StreamScratch sc_tiles;                   // the list's tile counts, handed between streams
    uint32_t ctl[kPlanWords] = {};            // as last read
    std::vector<DevBuf*> all() {
        return {&b_dep_ptr, &b_deps,  &b_flags,  &b_key_ptr, &b_key_slots, &b_claim, &b_root, &b_state,
                &b_which,   &b_found, &b_hitrow, &b_rows,    &b_queue,     &b_ctl,   &b_dirty, &b_keys,
                &b_ids,     &b_vals8, &b_ln,     &b_lw,      &b_lv,        &b_lf,    &b_lcount};
    }
};

extern "C" int rf_eval_plan_check(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, uint32_t* depth) {
    ARG(n == 0 || dep_ptr, "null argument");
    char msg[160];
    if (!plan_check(n, dep_ptr, deps, depth, msg, sizeof msg)) return fail(RF_EINVAL, "eval_plan: %s", msg);
    return RF_OK;
}

static void plan_free(rf_eval_plan* p) {
    p->sc_tiles.destroy();
    for (DevBuf* b : p->all()) b->release();
    delete p;
}

extern "C" int rf_eval_plan_open(rf_ctx* ctx, uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps,
                                 const uint8_t* flags, const uint64_t* key_ptr, const uint32_t* key_slots,
                                 rf_eval_plan** out) {
    ARG(ctx && out && (n == 0 || (dep_ptr && flags && key_ptr)), "null argument");
    uint32_t depth = 0;
    if (int rc = rf_eval_plan_check(n, dep_ptr, deps, &depth)) return rc;
    uint64_t K = 0, with_keys = 0;
    if (n) {
        ARG(key_ptr[0] == 0, "key_ptr[0] must be 0");
        for (uint64_t i = 0; i < n; ++i) {
            ARG(key_ptr[i] <= key_ptr[i + 1], "key_ptr not monotone");
            if (key_ptr[i + 1] - key_ptr[i] > RF_PLAN_MAX_KEYS)
                return fail(RF_EINVAL, "node %llu: more than %d cache keys", (unsigned long long)i, RF_PLAN_MAX_KEYS);
            with_keys += key_ptr[i + 1] != key_ptr[i];
        }
        K = key_ptr[n];
        ARG(K < (1ull << 32), "too many keys");
    }
    const uint64_t E = n ? dep_ptr[n] : 0;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    auto* p = new rf_eval_plan();
    p->ctx = ctx;
    p->device = ctx->device;
    p->n = n;
    p->n_deps = E;
    p->n_keys = K;
    p->depth = depth;
    p->round_batch = plan_round_batch(depth);
    p->has_slots = key_slots != nullptr;
    if (n) {
        p->dep_ptr.assign(dep_ptr, dep_ptr + n + 1);
        p->deps.assign(deps, deps + E);
        p->flags.assign(flags, flags + n);
    }
    if (key_slots)
        for (uint64_t r = 0; r < K; ++r) p->max_slot = std::max(p->max_slot, key_slots[r]);
    const uint64_t nw = (n + 31) / 32;
    const uint64_t n_pad = (n + kPlanListTile - 1) / kPlanListTile * kPlanListTile;
    struct Want {
        DevBuf* b;
        uint64_t bytes;
        const void* src;
        uint64_t src_bytes;
    } wants[] = {
        {&p->b_dep_ptr, 8 * (n + 1), dep_ptr, n ? 8 * (n + 1) : 0},
        {&p->b_deps, 4 * std::max<uint64_t>(E, 1), deps, 4 * E},
        {&p->b_flags, std::max<uint64_t>(n, 1), flags, n},
        {&p->b_key_ptr, 8 * (n + 1), key_ptr, n ? 8 * (n + 1) : 0},
        {&p->b_key_slots, 4 * std::max<uint64_t>(K, 1), key_slots, key_slots ? 4 * K : 0},
        {&p->b_claim, 4 * std::max<uint64_t>(nw, 1), nullptr, 0},
        {&p->b_root, 4 * std::max<uint64_t>(nw, 1), nullptr, 0},
        {&p->b_state, std::max<uint64_t>(n_pad, 4), nullptr, 0},
        {&p->b_which, std::max<uint64_t>(n, 1), nullptr, 0},
        {&p->b_found, std::max<uint64_t>(n, 1), nullptr, 0},
        {&p->b_hitrow, 4 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&p->b_rows, 32 * std::max<uint64_t>(with_keys, 1), nullptr, 0},
        {&p->b_queue, 4 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&p->b_ctl, 4 * kPlanWords, nullptr, 0},
    };
    for (const Want& w : wants) {
        hipError_t e = w.b->ensure(w.bytes);
        if (e == hipSuccess) e = hipMemsetAsync(w.b->p, 0, w.b->cap, ctx->stream);
        if (e == hipSuccess && w.src_bytes)
            e = hipMemcpyAsync(w.b->p, w.src, w.src_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->stream);
            plan_free(p);
            return fail(e == hipErrorOutOfMemory ? RF_ENOMEM : RF_EDEVICE, "eval_plan alloc: %s", hipGetErrorString(e));
        }
    }
    if (hipError_t e = hipStreamSynchronize(ctx->stream); e != hipSuccess) {
        plan_free(p);
        return fail(RF_EDEVICE, "eval_plan open: %s", hipGetErrorString(e));
    }
    PlanDev& d = p->d;
    d.n = (uint32_t)n;
    d.dep_ptr = p->b_dep_ptr.as<uint64_t>();
    d.deps = p->b_deps.as<uint32_t>();
    d.flags = p->b_flags.as<uint8_t>();
    d.key_ptr = p->b_key_ptr.as<uint64_t>();
    d.key_slots = key_slots ? p->b_key_slots.as<uint32_t>() : nullptr;
    d.claim = p->b_claim.as<uint32_t>();
    d.rootbit = p->b_root.as<uint32_t>();
    d.state = p->b_state.as<uint8_t>();
    d.which = p->b_which.as<uint8_t>();
    d.found = p->b_found.as<uint8_t>();
    d.hitrow = p->b_hitrow.as<uint32_t>();
    d.rows = p->b_rows.as<uint4>();
    d.row_cap = (uint32_t)with_keys;
    d.queue = p->b_queue.as<uint32_t>();
    d.ctl = p->b_ctl.as<uint32_t>();
    p->ctl[kPlanCounts + RF_PLAN_UNSEEN] = (uint32_t)n;
    *out = p;
    return RF_OK;
}

// No context lock, as the other destroy calls: a binding's finalizers may run
// after the context's (its memory, mutex included, is gone by then).
extern "C" void rf_eval_plan_close(rf_eval_plan* p) {
    if (!p) return;
    DevGuard dg(p->device);
    plan_free(p);
}

extern "C" int rf_eval_plan_set_flags(rf_eval_plan* p, const uint32_t* nodes, const uint8_t* flags, uint64_t n) {
    ARG(p && (n == 0 || (nodes && flags)), "null argument");
    ARG(n < (1ull << 32), "too many nodes listed");
    for (uint64_t i = 0; i < n; ++i)
        if (nodes[i] >= p->n) return fail(RF_EINVAL, "set_flags: node %u out of range", nodes[i]);
    if (!n) return RF_OK;
    rf_ctx* ctx = p->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    for (uint64_t i = 0; i < n; ++i) {
        uint8_t& f = p->flags[nodes[i]];
        if ((f ^ flags[i]) & RF_PLAN_F_EXTERN) p->dirty_valid = false;  // the closure's seeds changed
        f = flags[i];
    }
    std::vector<uint8_t> vals(n);  // a node listed twice: its last value, both times
    for (uint64_t i = 0; i < n; ++i) vals[i] = p->flags[nodes[i]];
    HIPC(p->b_ids.ensure(4 * n));
    HIPC(p->b_vals8.ensure(n));
    HIPC(hipMemcpyAsync(p->b_ids.p, nodes, 4 * n, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(p->b_vals8.p, vals.data(), n, hipMemcpyHostToDevice, ctx->stream));
    HIPC(launch_plan_set_flags(p->b_flags.as<uint8_t>(), p->b_ids.as<uint32_t>(), p->b_vals8.as<uint8_t>(), (uint32_t)n,
                               ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

// ---- run / reject -----------------------------------------------------------
static int plan_read_ctl(rf_eval_plan* p, hipStream_t s) {
    HIPC(hipMemcpyAsync(p->ctl, p->b_ctl.p, sizeof p->ctl, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return RF_OK;
}

// What the rounds read: keys, liveset, assoc, dirty bits (context mutex held).
static int plan_look(rf_eval_plan* p, int nce, rf_graph* g, const void* d_keys32, rf_bloom* live, rf_assoc* a, int kind,
                     PlanLook* l) {
    ARG(kind >= 0 && kind < (1 << 30), "assoc kind out of range");
    if (g) {
        if (!p->has_slots) return fail(RF_EPRECONDITION, "eval_plan: keys from a graph need key_slots at open");
        if (!g->initialized || g->marked)
            return fail(RF_EPRECONDITION, "eval_plan: the graph must be recomputed with no input change pending");
        if (p->n_keys && p->max_slot >= g->g.n_slots)
            return fail(RF_EINVAL, "eval_plan: key slot %u beyond the graph's %u slots", p->max_slot, g->g.n_slots);
        l->keys = g->g.slots;
        l->by_slot = true;
    } else {
        ARG(p->n_keys == 0 || d_keys32, "null keys");
        l->keys = static_cast<const uint8_t*>(d_keys32);
        l->by_slot = false;
    }
    l->no_cache_extern = nce ? 1 : 0;
    if (nce && p->n) {
        if (!p->dirty_valid) {  // eval.go:874-887, once per set of externs, kept on the device
            if (int rc = flow_dirty_bits(p->ctx, p->n, p->dep_ptr.data(), p->deps.data(), p->flags.data(),
                                         RF_PLAN_F_EXTERN, p->b_dirty))
                return rc;
            p->dirty_valid = true;
        }
        l->dirty = p->b_dirty.as<uint32_t>();
    }
    if (live) {
        const BloomDev& b = bloom_dev(live);
        l->words = b.words;
        l->len_dev = b.len_dev;
        l->m = b.m;
        l->mu = b.m ? (~0ull) / b.m : 0ull;
        l->k = (uint32_t)b.k;
    }
    l->t = assoc_view(a);
    l->kind = (uint32_t)kind;
    return RF_OK;
}

// Rounds in batches until the frontier is empty: never more than depth.
static int plan_rounds(rf_eval_plan* p, const PlanLook& l, hipStream_t s) {
    p->rounds = 0;
    if (int rc = plan_read_ctl(p, s)) return rc;
    while (p->ctl[kPlanLo] != p->ctl[kPlanHi]) {
        if (p->rounds >= p->depth)
            return fail(RF_EDEVICE, "eval_plan: frontier not empty after %u rounds", p->depth);
        const uint32_t b = std::min(p->round_batch, p->depth - p->rounds);
        HIPC(launch_plan_rounds(p->d, l, b, s));
        p->rounds += b;
        if (int rc = plan_read_ctl(p, s)) return rc;
    }
    HIPC(launch_plan_finish(p->d, s));
    return plan_read_ctl(p, s);
}

static int plan_same_ctx(rf_eval_plan* p, rf_graph* g, rf_bloom* live, rf_assoc* a) {
    ARG(assoc_ctx(a) == p->ctx && (!live || bloom_ctx(live) == p->ctx) && (!g || g->ctx == p->ctx),
        "plan, graph, liveset and assoc of different contexts");
    return RF_OK;
}

static int plan_ids_ok(rf_eval_plan* p, const uint32_t* ids, uint64_t n, const char* what) {
    ARG(n < (1ull << 32), "too many nodes listed");
    for (uint64_t i = 0; i < n; ++i)
        if (ids[i] >= p->n) return fail(RF_EINVAL, "eval_plan: %s %u out of range", what, ids[i]);
    return RF_OK;
}

// (context mutex held, device set)
static int plan_run_locked(rf_eval_plan* p, const uint32_t* roots, uint64_t n_roots, int nce, rf_graph* g,
                           const void* d_keys32, rf_bloom* live, rf_assoc* a, int kind, hipStream_t s) {
    PlanLook l;
    if (int rc = plan_look(p, nce, g, d_keys32, live, a, kind, &l)) return rc;
    const uint64_t nw = std::max<uint64_t>((p->n + 31) / 32, 1);
    HIPC(hipMemsetAsync(p->b_claim.p, 0, 4 * nw, s));
    HIPC(hipMemsetAsync(p->b_root.p, 0, 4 * nw, s));
    HIPC(hipMemsetAsync(p->b_state.p, 0, p->b_state.cap, s));
    HIPC(hipMemsetAsync(p->b_ctl.p, 0, 4 * kPlanWords, s));
    if (n_roots) {
        HIPC(p->b_ids.ensure(4 * n_roots));
        HIPC(hipMemcpyAsync(p->b_ids.p, roots, 4 * n_roots, hipMemcpyHostToDevice, s));
    }
    HIPC(launch_plan_seed(p->d, p->b_ids.as<uint32_t>(), (uint32_t)n_roots, s));
    p->ran = true;
    p->last_nce = nce ? 1 : 0;
    return plan_rounds(p, l, s);
}

extern "C" int rf_eval_plan_run(rf_eval_plan* p, const uint32_t* roots, uint64_t n_roots, int no_cache_extern,
                                rf_graph* g, const void* d_keys32, rf_bloom* live, rf_assoc* a, int kind, void* stream) {
    ARG(p && a && (n_roots == 0 || roots), "null argument");
    if (int rc = plan_same_ctx(p, g, live, a)) return rc;
    if (int rc = plan_ids_ok(p, roots, n_roots, "root")) return rc;
    rf_ctx* ctx = p->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);  // no Put may swap the table meanwhile
    DevGuard dg(ctx->device);
    return plan_run_locked(p, roots, n_roots, no_cache_extern, g, d_keys32, live, a, kind, pick(ctx, stream));
}

static int plan_upload_keys(rf_eval_plan* p, const uint8_t* keys32) {
    if (!p->n_keys) return RF_OK;
    HIPC(p->b_keys.ensure(32 * p->n_keys));
    HIPC(sync_copy(p->ctx, p->b_keys.p, keys32, 32 * p->n_keys, hipMemcpyHostToDevice));
    return RF_OK;
}

extern "C" int rf_eval_plan_run_host(rf_eval_plan* p, const uint32_t* roots, uint64_t n_roots, int no_cache_extern,
                                     const uint8_t* keys32, rf_bloom* live, rf_assoc* a, int kind) {
    ARG(p && a && (n_roots == 0 || roots) && (p->n_keys == 0 || keys32), "null argument");
    if (int rc = plan_same_ctx(p, nullptr, live, a)) return rc;
    if (int rc = plan_ids_ok(p, roots, n_roots, "root")) return rc;
    rf_ctx* ctx = p->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = plan_upload_keys(p, keys32)) return rc;
    return plan_run_locked(p, roots, n_roots, no_cache_extern, nullptr, p->b_keys.p, live, a, kind, ctx->stream);
}

static int plan_reject_locked(rf_eval_plan* p, const uint32_t* nodes, uint64_t n, rf_graph* g, const void* d_keys32,
                              rf_bloom* live, rf_assoc* a, int kind, hipStream_t s) {
    if (!p->ran) return fail(RF_EPRECONDITION, "eval_plan: reject before any run");
    PlanLook l;
    if (int rc = plan_look(p, p->last_nce, g, d_keys32, live, a, kind, &l)) return rc;
    if (n) {
        HIPC(p->b_ids.ensure(4 * n));
        HIPC(hipMemcpyAsync(p->b_ids.p, nodes, 4 * n, hipMemcpyHostToDevice, s));
    }
    HIPC(hipMemsetAsync(p->d.ctl + kPlanBad, 0, 4, s));
    HIPC(launch_plan_reject_check(p->d, p->b_ids.as<uint32_t>(), (uint32_t)n, s));
    if (int rc = plan_read_ctl(p, s)) return rc;
    if (p->ctl[kPlanBad]) return fail(RF_EINVAL, "eval_plan: reject lists a node that is not a hit");
    HIPC(hipMemsetAsync(p->d.ctl + kPlanLooked, 0, 3 * 4, s));  // looked, probed, filtered: of this reject
    HIPC(launch_plan_reject(p->d, p->b_ids.as<uint32_t>(), (uint32_t)n, s));
    return plan_rounds(p, l, s);
}

extern "C" int rf_eval_plan_reject(rf_eval_plan* p, const uint32_t* nodes, uint64_t n, rf_graph* g,
                                   const void* d_keys32, rf_bloom* live, rf_assoc* a, int kind, void* stream) {
    ARG(p && a && (n == 0 || nodes), "null argument");
    if (int rc = plan_same_ctx(p, g, live, a)) return rc;
    if (int rc = plan_ids_ok(p, nodes, n, "node")) return rc;
    rf_ctx* ctx = p->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    return plan_reject_locked(p, nodes, n, g, d_keys32, live, a, kind, pick(ctx, stream));
}

extern "C" int rf_eval_plan_reject_host(rf_eval_plan* p, const uint32_t* nodes, uint64_t n, const uint8_t* keys32,
                                        rf_bloom* live, rf_assoc* a, int kind) {
    ARG(p && a && (n == 0 || nodes) && (p->n_keys == 0 || keys32), "null argument");
    if (int rc = plan_same_ctx(p, nullptr, live, a)) return rc;
    if (int rc = plan_ids_ok(p, nodes, n, "node")) return rc;
    rf_ctx* ctx = p->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = plan_upload_keys(p, keys32)) return rc;
    return plan_reject_locked(p, nodes, n, nullptr, p->b_keys.p, live, a, kind, ctx->stream);
}

// ---- results ------------------------------------------------------------------
extern "C" int rf_eval_plan_states(rf_eval_plan* p, uint8_t* state) {
    ARG(p && (p->n == 0 || state), "null argument");
    std::lock_guard<std::mutex> lk(p->ctx->mu);
    DevGuard dg(p->ctx->device);
    HIPC(sync_copy(p->ctx, state, p->b_state.p, p->n, hipMemcpyDeviceToHost));
    return RF_OK;
}

extern "C" int rf_eval_plan_states_device(rf_eval_plan* p, const void** d_state) {
    ARG(p && d_state, "null argument");
    *d_state = p->b_state.p;
    return RF_OK;
}

// the three list launches on s (context mutex held)
static int plan_list_locked(rf_eval_plan* p, int state, uint64_t cap, void* d_nodes, void* d_which, void* d_vals,
                            void* d_found_mask, void* d_found, hipStream_t s) {
    const uint64_t tiles = (p->n + kPlanListTile - 1) / kPlanListTile;
    StreamScratch& sc = p->sc_tiles;
    std::lock_guard<std::mutex> lk(sc.mu);
    HIPC(sc.acquire(4 * std::max<uint64_t>(tiles, 1), s));
    hipError_t e = launch_plan_list(p->d, (uint32_t)state, cap, sc.buf.as<uint32_t>(), static_cast<uint32_t*>(d_nodes),
                                    static_cast<uint8_t*>(d_which), static_cast<uint8_t*>(d_vals),
                                    static_cast<uint8_t*>(d_found_mask), static_cast<uint64_t*>(d_found), s);
    HIPC(sc.release(s));
    if (e != hipSuccess) return fail(RF_EDEVICE, "eval_plan list: %s", hipGetErrorString(e));
    return RF_OK;
}

extern "C" int rf_eval_plan_list_device(rf_eval_plan* p, int state, uint64_t cap, void* d_nodes, void* d_which,
                                        void* d_vals32, void* d_key_found, void* d_found, void* stream) {
    ARG(p && d_found && (cap == 0 || d_nodes), "null argument");
    ARG(state >= RF_PLAN_UNSEEN && state <= RF_PLAN_DONE, "unknown state");
    std::lock_guard<std::mutex> lk(p->ctx->mu);
    DevGuard dg(p->ctx->device);
    return plan_list_locked(p, state, cap, d_nodes, d_which, d_vals32, d_key_found, d_found, pick(p->ctx, stream));
}

extern "C" int rf_eval_plan_list(rf_eval_plan* p, int state, uint64_t cap, uint32_t* nodes, uint8_t* which,
                                 uint8_t* vals32, uint8_t* key_found, uint64_t* found) {
    ARG(p && found && (cap == 0 || nodes), "null argument");
    ARG(state >= RF_PLAN_UNSEEN && state <= RF_PLAN_DONE, "unknown state");
    rf_ctx* ctx = p->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    const bool hit = state == RF_PLAN_HIT;
    const uint64_t ecap = std::min(cap, p->n);  // (found <= n: min(found, cap) is unchanged)
    HIPC(p->b_lcount.ensure(8));
    HIPC(p->b_ln.ensure(4 * std::max<uint64_t>(ecap, 1)));
    if (hit && which) HIPC(p->b_lw.ensure(std::max<uint64_t>(ecap, 1)));
    if (hit && key_found) HIPC(p->b_lf.ensure(std::max<uint64_t>(ecap, 1)));
    if (hit && vals32) HIPC(p->b_lv.ensure(32 * std::max<uint64_t>(ecap, 1)));
    if (int rc = plan_list_locked(p, state, ecap, p->b_ln.p, hit && which ? p->b_lw.p : nullptr,
                                  hit && vals32 ? p->b_lv.p : nullptr, hit && key_found ? p->b_lf.p : nullptr,
                                  p->b_lcount.p, s))
        return rc;
    uint64_t cnt = 0;
    HIPC(sync_copy(ctx, &cnt, p->b_lcount.p, 8, hipMemcpyDeviceToHost));
    *found = cnt;
    if (cnt > cap) return fail(RF_EINVAL, "list buffers too small: need %llu nodes", (unsigned long long)cnt);
    if (!cnt) return RF_OK;
    HIPC(hipMemcpyAsync(nodes, p->b_ln.p, 4 * cnt, hipMemcpyDeviceToHost, s));
    if (hit && which) HIPC(hipMemcpyAsync(which, p->b_lw.p, cnt, hipMemcpyDeviceToHost, s));
    if (hit && key_found) HIPC(hipMemcpyAsync(key_found, p->b_lf.p, cnt, hipMemcpyDeviceToHost, s));
    if (hit && vals32) HIPC(hipMemcpyAsync(vals32, p->b_lv.p, 32 * cnt, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return RF_OK;
}

extern "C" int rf_eval_plan_stats_get(rf_eval_plan* p, rf_eval_plan_stats* out, uint64_t size) {
    ARG(p && out, "null argument");
    ARG(size == sizeof(rf_eval_plan_stats), "rf_eval_plan_stats of another size (header mismatch)");
    std::lock_guard<std::mutex> lk(p->ctx->mu);
    *out = rf_eval_plan_stats{};
    out->n_nodes = p->n;
    out->depth = p->depth;
    out->rounds = p->rounds;
    out->round_batch = p->round_batch;
    out->round_lanes = plan_grid((uint32_t)p->n) * kPlanBlock;
    out->list_tile = kPlanListTile;
    for (int q = 0; q < 5; ++q) out->counts[q] = p->ctl[kPlanCounts + q];
    out->looked_up = p->ctl[kPlanLooked];
    out->keys_probed = p->ctl[kPlanProbed];
    out->keys_filtered = p->ctl[kPlanFiltered];
    for (DevBuf* b : p->all()) out->device_bytes += b->cap;
    out->device_bytes += p->sc_tiles.buf.cap;
    return RF_OK;
}
