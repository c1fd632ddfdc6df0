// eval_wave.cpp -- evaluation waves driven by completions (rf_eval_wave_*):
// host side of k10_wave.hip.  Owns its own copy of a Flow graph's structure on
// the device, with the consumer CSR (wave_check.cpp) beside the Deps; begin
// enqueues the descent in batches with one small read-back per batch, a step
// is check / read-back / complete / resolve / count / read-back; lists come
// from a tile count / scan / scatter.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "engine.h"
#include "graph_internal.h"
#include "plan_internal.h"
#include "wave_check.h"
#include "wave_internal.h"

using namespace rf;

// Descent rounds enqueued between two host reads (as the plan's; RF_WAVE_BATCH
// overrides, 0: the whole depth bound).
static uint32_t wave_round_batch(uint32_t depth) {
    uint32_t b = 4;
    if (const char* e = getenv("RF_WAVE_BATCH")) {
        const long v = atol(e);
        b = v <= 0 ? depth : (uint32_t)std::min<long>(v, 1 << 20);
    }
    return std::max<uint32_t>(b, 1);
}

extern "C" int rf_eval_wave_consumers(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, uint64_t* cons_ptr,
                                      uint32_t* cons) {
    ARG(cons_ptr && (n == 0 || dep_ptr), "null argument");
    if (int rc = rf_eval_plan_check(n, dep_ptr, deps, nullptr)) return rc;  // monotone, range, no cycle
    char msg[160];
    if (!wave_consumers(n, dep_ptr, deps, cons_ptr, cons, msg, sizeof msg)) return fail(RF_EINVAL, "eval_wave: %s", msg);
    return RF_OK;
}

static void wave_free(rf_eval_wave* w) {
    w->sc_tiles.destroy();
    for (DevBuf* b : w->all()) b->release();
    delete w;
}

extern "C" int rf_eval_wave_open(rf_ctx* ctx, uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps,
                                 const uint8_t* flags, const uint64_t* key_ptr, const uint32_t* key_slots,
                                 rf_eval_wave** out) {
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
    std::vector<uint64_t> cons_ptr(n + 1, 0);
    std::vector<uint32_t> cons(std::max<uint64_t>(E, 1));
    {
        char msg[160];
        if (!wave_consumers(n, dep_ptr, deps, cons_ptr.data(), cons.data(), msg, sizeof msg))
            return fail(RF_EINVAL, "eval_wave: %s", msg);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    auto* w = new rf_eval_wave();
    w->ctx = ctx;
    w->device = ctx->device;
    w->n = n;
    w->n_deps = E;
    w->n_keys = K;
    w->depth = depth;
    w->round_batch = wave_round_batch(depth);
    w->has_slots = key_slots != nullptr;
    if (key_slots)
        for (uint64_t r = 0; r < K; ++r) w->max_slot = std::max(w->max_slot, key_slots[r]);
    const uint64_t nw = (n + 31) / 32;
    const uint64_t n_pad = (n + kPlanListTile - 1) / kPlanListTile * kPlanListTile;
    struct Want {
        DevBuf* b;
        uint64_t bytes;
        const void* src;
        uint64_t src_bytes;
    } wants[] = {
        {&w->b_dep_ptr, 8 * (n + 1), dep_ptr, n ? 8 * (n + 1) : 0},
        {&w->b_deps, 4 * std::max<uint64_t>(E, 1), deps, 4 * E},
        {&w->b_cons_ptr, 8 * (n + 1), cons_ptr.data(), 8 * (n + 1)},
        {&w->b_cons, 4 * std::max<uint64_t>(E, 1), cons.data(), 4 * E},
        {&w->b_flags, std::max<uint64_t>(n, 1), flags, n},
        {&w->b_key_ptr, 8 * (n + 1), key_ptr, n ? 8 * (n + 1) : 0},
        {&w->b_key_slots, 4 * std::max<uint64_t>(K, 1), key_slots, key_slots ? 4 * K : 0},
        {&w->b_claim, 4 * std::max<uint64_t>(nw, 1), nullptr, 0},
        {&w->b_root, 4 * std::max<uint64_t>(nw, 1), nullptr, 0},
        {&w->b_fin, 4 * std::max<uint64_t>(nw, 1), nullptr, 0},
        {&w->b_last, std::max<uint64_t>(n_pad / 8, 4), nullptr, 0},
        {&w->b_state, std::max<uint64_t>(n_pad, 4), nullptr, 0},
        {&w->b_pending, 4 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&w->b_which, std::max<uint64_t>(n, 1), nullptr, 0},
        {&w->b_found, std::max<uint64_t>(n, 1), nullptr, 0},
        {&w->b_hitrow, 4 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&w->b_rows, 32 * std::max<uint64_t>(with_keys, 1), nullptr, 0},
        {&w->b_queue, 4 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&w->b_wq, 4 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&w->b_ctl, 4 * kWaveWords, nullptr, 0},
    };
    for (const Want& x : wants) {
        hipError_t e = x.b->ensure(x.bytes);
        if (e == hipSuccess) e = hipMemsetAsync(x.b->p, 0, x.b->cap, ctx->stream);
        if (e == hipSuccess && x.src_bytes)
            e = hipMemcpyAsync(x.b->p, x.src, x.src_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->stream);
            wave_free(w);
            return fail(e == hipErrorOutOfMemory ? RF_ENOMEM : RF_EDEVICE, "eval_wave alloc: %s", hipGetErrorString(e));
        }
    }
    if (hipError_t e = hipStreamSynchronize(ctx->stream); e != hipSuccess) {
        wave_free(w);
        return fail(RF_EDEVICE, "eval_wave open: %s", hipGetErrorString(e));
    }
    WaveDev& d = w->d;
    d.n = (uint32_t)n;
    d.dep_ptr = w->b_dep_ptr.as<uint64_t>();
    d.deps = w->b_deps.as<uint32_t>();
    d.cons_ptr = w->b_cons_ptr.as<uint64_t>();
    d.cons = w->b_cons.as<uint32_t>();
    d.flags = w->b_flags.as<uint8_t>();
    d.key_ptr = w->b_key_ptr.as<uint64_t>();
    d.key_slots = key_slots ? w->b_key_slots.as<uint32_t>() : nullptr;
    d.claim = w->b_claim.as<uint32_t>();
    d.rootbit = w->b_root.as<uint32_t>();
    d.fin = w->b_fin.as<uint32_t>();
    d.last = w->b_last.as<uint32_t>();
    d.state = w->b_state.as<uint8_t>();
    d.pending = w->b_pending.as<uint32_t>();
    d.which = w->b_which.as<uint8_t>();
    d.found = w->b_found.as<uint8_t>();
    d.hitrow = w->b_hitrow.as<uint32_t>();
    d.rows = w->b_rows.as<uint4>();
    d.row_cap = (uint32_t)with_keys;
    d.queue = w->b_queue.as<uint32_t>();
    d.wq = w->b_wq.as<uint32_t>();
    d.ctl = w->b_ctl.as<uint32_t>();
    w->ctl[kWaveCounts + RF_PLAN_UNSEEN] = (uint32_t)n;
    *out = w;
    return RF_OK;
}

// No context lock, as the other destroy calls: a binding's finalizers may run
// after the context's (its memory, mutex included, is gone by then).
extern "C" void rf_eval_wave_close(rf_eval_wave* w) {
    if (!w) return;
    DevGuard dg(w->device);
    wave_free(w);
}

static int wave_ids_ok(rf_eval_wave* w, const uint32_t* ids, uint64_t n, const char* what) {
    ARG(n < (1ull << 32), "too many nodes listed");
    for (uint64_t i = 0; i < n; ++i)
        if (ids[i] >= w->n) return fail(RF_EINVAL, "eval_wave: %s %u out of range", what, ids[i]);
    return RF_OK;
}

extern "C" int rf_eval_wave_set_flags(rf_eval_wave* w, const uint32_t* nodes, const uint8_t* flags, uint64_t n) {
    ARG(w && (n == 0 || (nodes && flags)), "null argument");
    if (int rc = wave_ids_ok(w, nodes, n, "node")) return rc;
    if (!n) return RF_OK;
    rf_ctx* ctx = w->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    std::vector<uint8_t> vals(flags, flags + n);
    {  // a node listed twice: its last value, both times
        std::vector<std::pair<uint32_t, uint64_t>> order(n);
        for (uint64_t i = 0; i < n; ++i) order[i] = {nodes[i], i};
        std::sort(order.begin(), order.end());
        for (uint64_t i = 0; i < n;) {
            uint64_t j = i;
            while (j + 1 < n && order[j + 1].first == order[i].first) ++j;
            for (uint64_t k = i; k <= j; ++k) vals[order[k].second] = flags[order[j].second];
            i = j + 1;
        }
    }
    HIPC(w->b_ids.ensure(4 * n));
    HIPC(w->b_vals8.ensure(n));
    HIPC(hipMemcpyAsync(w->b_ids.p, nodes, 4 * n, hipMemcpyHostToDevice, ctx->stream));
    HIPC(hipMemcpyAsync(w->b_vals8.p, vals.data(), n, hipMemcpyHostToDevice, ctx->stream));
    HIPC(launch_plan_set_flags(w->b_flags.as<uint8_t>(), w->b_ids.as<uint32_t>(), w->b_vals8.as<uint8_t>(), (uint32_t)n,
                               ctx->stream));
    HIPC(hipStreamSynchronize(ctx->stream));
    return RF_OK;
}

// ---- begin / step / reject ----------------------------------------------------
static int wave_read_ctl(rf_eval_wave* w, hipStream_t s) {
    HIPC(hipMemcpyAsync(w->ctl, w->b_ctl.p, sizeof w->ctl, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return RF_OK;
}

static int wave_same_ctx(rf_eval_wave* w, rf_graph* g, rf_bloom* live, rf_assoc* a) {
    ARG((!a || assoc_ctx(a) == w->ctx) && (!live || bloom_ctx(live) == w->ctx) && (!g || g->ctx == w->ctx),
        "wave, graph, liveset and assoc of different contexts");
    return RF_OK;
}

// What a wave's lookups read: keys, liveset, assoc (context mutex held).
// Nothing is looked up in top-down mode; the arguments are not read then.
static int wave_look(rf_eval_wave* w, int mode, int nce, rf_graph* g, const void* d_keys32, rf_bloom* live,
                     rf_assoc* a, int kind, WaveLook* l) {
    if (mode != kModeBottomUp) return RF_OK;
    ARG(a, "null assoc");
    ARG(kind >= 0 && kind < (1 << 30), "assoc kind out of range");
    if (g) {
        if (!w->has_slots) return fail(RF_EPRECONDITION, "eval_wave: keys from a graph need key_slots at open");
        if (!g->initialized || g->marked)
            return fail(RF_EPRECONDITION, "eval_wave: the graph must be recomputed with no input change pending");
        if (w->n_keys && w->max_slot >= g->g.n_slots)
            return fail(RF_EINVAL, "eval_wave: key slot %u beyond the graph's %u slots", w->max_slot, g->g.n_slots);
        l->keys = g->g.slots;
        l->by_slot = true;
    } else {
        ARG(w->n_keys == 0 || d_keys32, "null keys");
        l->keys = static_cast<const uint8_t*>(d_keys32);
        l->by_slot = false;
    }
    l->lookup = true;
    l->no_cache_extern = nce ? 1 : 0;
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

// claim, roots, finished, membership, (states,) control words: a fresh begin
static int wave_reset(rf_eval_wave* w, bool states, hipStream_t s) {
    const uint64_t nw = std::max<uint64_t>((w->n + 31) / 32, 1);
    HIPC(hipMemsetAsync(w->b_claim.p, 0, 4 * nw, s));
    HIPC(hipMemsetAsync(w->b_root.p, 0, 4 * nw, s));
    HIPC(hipMemsetAsync(w->b_fin.p, 0, 4 * nw, s));
    HIPC(hipMemsetAsync(w->b_last.p, 0, w->b_last.cap, s));
    if (states) HIPC(hipMemsetAsync(w->b_state.p, 0, w->b_state.cap, s));
    HIPC(hipMemsetAsync(w->b_ctl.p, 0, 4 * kWaveWords, s));
    return RF_OK;
}

// the wave queue resolved, the counts, the control words read back
static int wave_finish(rf_eval_wave* w, const WaveLook& l, hipStream_t s) {
    HIPC(launch_wave_resolve(w->d, l, s));
    HIPC(launch_wave_count(w->d, s));
    if (int rc = wave_read_ctl(w, s)) return rc;
    w->last_wave = w->ctl[kWaveWTail];
    return RF_OK;
}

// (context mutex held, device set)
static int wave_begin_locked(rf_eval_wave* w, const uint32_t* roots, uint64_t n_roots, int nce, rf_graph* g,
                             const void* d_keys32, rf_bloom* live, rf_assoc* a, int kind, hipStream_t s) {
    WaveLook l;
    if (int rc = wave_look(w, kModeBottomUp, nce, g, d_keys32, live, a, kind, &l)) return rc;
    if (int rc = wave_reset(w, true, s)) return rc;
    if (n_roots) {
        HIPC(w->b_ids.ensure(4 * n_roots));
        HIPC(hipMemcpyAsync(w->b_ids.p, roots, 4 * n_roots, hipMemcpyHostToDevice, s));
    }
    HIPC(launch_wave_seed(w->d, w->b_ids.as<uint32_t>(), (uint32_t)n_roots, s));
    w->mode = kModeBottomUp;
    w->nce = nce ? 1 : 0;
    w->waves = 1;
    w->rounds = 0;
    if (int rc = wave_read_ctl(w, s)) return rc;
    while (w->ctl[kWaveLo] != w->ctl[kWaveHi]) {  // descent rounds in batches: never more than depth
        if (w->rounds >= w->depth) return fail(RF_EDEVICE, "eval_wave: frontier not empty after %u rounds", w->depth);
        const uint32_t b = std::min(w->round_batch, w->depth - w->rounds);
        HIPC(launch_wave_descend(w->d, b, s));
        w->rounds += b;
        if (int rc = wave_read_ctl(w, s)) return rc;
    }
    return wave_finish(w, l, s);
}

extern "C" int rf_eval_wave_begin(rf_eval_wave* w, const uint32_t* roots, uint64_t n_roots, int no_cache_extern,
                                  rf_graph* g, const void* d_keys32, rf_bloom* live, rf_assoc* a, int kind,
                                  void* stream) {
    ARG(w && a && (n_roots == 0 || roots), "null argument");
    if (int rc = wave_same_ctx(w, g, live, a)) return rc;
    if (int rc = wave_ids_ok(w, roots, n_roots, "root")) return rc;
    rf_ctx* ctx = w->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);  // no Put may swap the table meanwhile
    DevGuard dg(ctx->device);
    return wave_begin_locked(w, roots, n_roots, no_cache_extern, g, d_keys32, live, a, kind, pick(ctx, stream));
}

static int wave_upload_keys(rf_eval_wave* w, const uint8_t* keys32) {
    if (!w->n_keys || !keys32) return RF_OK;
    HIPC(w->b_keys.ensure(32 * w->n_keys));
    HIPC(sync_copy(w->ctx, w->b_keys.p, keys32, 32 * w->n_keys, hipMemcpyHostToDevice));
    return RF_OK;
}

extern "C" int rf_eval_wave_begin_host(rf_eval_wave* w, const uint32_t* roots, uint64_t n_roots, int no_cache_extern,
                                       const uint8_t* keys32, rf_bloom* live, rf_assoc* a, int kind) {
    ARG(w && a && (n_roots == 0 || roots) && (w->n_keys == 0 || keys32), "null argument");
    if (int rc = wave_same_ctx(w, nullptr, live, a)) return rc;
    if (int rc = wave_ids_ok(w, roots, n_roots, "root")) return rc;
    rf_ctx* ctx = w->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = wave_upload_keys(w, keys32)) return rc;
    return wave_begin_locked(w, roots, n_roots, no_cache_extern, nullptr, w->b_keys.p, live, a, kind, ctx->stream);
}

extern "C" int rf_eval_wave_begin_states(rf_eval_wave* w, const void* state, int on_device, void* stream) {
    ARG(w && (w->n == 0 || state), "null argument");
    rf_ctx* ctx = w->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    // a copy of the caller's bytes: they may be this object's own states
    HIPC(w->b_in.ensure(std::max<uint64_t>(w->n, 1)));
    if (w->n)
        HIPC(hipMemcpyAsync(w->b_in.p, state, w->n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    HIPC(hipMemsetAsync(w->d.ctl + kWaveBad, 0, 4, s));
    HIPC(launch_wave_states_check(w->d, w->b_in.as<uint8_t>(), s));
    if (int rc = wave_read_ctl(w, s)) return rc;
    if (w->ctl[kWaveBad])
        return fail(RF_EINVAL, "eval_wave: a state byte above %d, or a TODO / READY node over an UNSEEN dep", RF_PLAN_DONE);
    if (int rc = wave_reset(w, false, s)) return rc;
    HIPC(launch_wave_states_apply(w->d, w->b_in.as<uint8_t>(), s));
    w->mode = kModeTopDown;
    w->nce = 0;
    w->waves = 1;
    w->rounds = 0;
    return wave_finish(w, WaveLook{}, s);
}

// (context mutex held, device set)
static int wave_step_locked(rf_eval_wave* w, const uint32_t* nodes, uint64_t n, rf_graph* g, const void* d_keys32,
                            rf_bloom* live, rf_assoc* a, int kind, hipStream_t s) {
    if (w->mode == kModeNone) return fail(RF_EPRECONDITION, "eval_wave: step before any begin");
    WaveLook l;
    if (int rc = wave_look(w, w->mode, w->nce, g, d_keys32, live, a, kind, &l)) return rc;
    if (n) {
        HIPC(w->b_ids.ensure(4 * n));
        HIPC(hipMemcpyAsync(w->b_ids.p, nodes, 4 * n, hipMemcpyHostToDevice, s));
        HIPC(hipMemsetAsync(w->d.ctl + kWaveBad, 0, 4, s));
        HIPC(launch_wave_step_check(w->d, w->b_ids.as<uint32_t>(), (uint32_t)n, s));
        if (int rc = wave_read_ctl(w, s)) return rc;
        if (w->ctl[kWaveBad]) return fail(RF_EINVAL, "eval_wave: step lists a node that is neither READY nor a HIT");
    }
    HIPC(hipMemsetAsync(w->b_last.p, 0, w->b_last.cap, s));
    HIPC(hipMemsetAsync(w->d.ctl + kWaveLooked, 0, 4 * (kWaveWTail - kWaveLooked + 1), s));  // the figures of this step
    HIPC(launch_wave_complete(w->d, w->b_ids.as<uint32_t>(), (uint32_t)n, s));
    w->waves++;
    return wave_finish(w, l, s);
}

extern "C" int rf_eval_wave_step(rf_eval_wave* w, const uint32_t* nodes, uint64_t n, rf_graph* g, const void* d_keys32,
                                 rf_bloom* live, rf_assoc* a, int kind, void* stream) {
    ARG(w && (n == 0 || nodes), "null argument");
    if (int rc = wave_same_ctx(w, g, live, a)) return rc;
    if (int rc = wave_ids_ok(w, nodes, n, "node")) return rc;
    rf_ctx* ctx = w->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    return wave_step_locked(w, nodes, n, g, d_keys32, live, a, kind, pick(ctx, stream));
}

extern "C" int rf_eval_wave_step_host(rf_eval_wave* w, const uint32_t* nodes, uint64_t n, const uint8_t* keys32,
                                      rf_bloom* live, rf_assoc* a, int kind) {
    ARG(w && (n == 0 || nodes), "null argument");
    ARG(w->mode != kModeBottomUp || w->n_keys == 0 || keys32, "null keys");
    if (int rc = wave_same_ctx(w, nullptr, live, a)) return rc;
    if (int rc = wave_ids_ok(w, nodes, n, "node")) return rc;
    rf_ctx* ctx = w->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (w->mode == kModeBottomUp)
        if (int rc = wave_upload_keys(w, keys32)) return rc;
    return wave_step_locked(w, nodes, n, nullptr, w->b_keys.p, live, a, kind, ctx->stream);
}

extern "C" int rf_eval_wave_reject(rf_eval_wave* w, const uint32_t* nodes, uint64_t n) {
    ARG(w && (n == 0 || nodes), "null argument");
    if (int rc = wave_ids_ok(w, nodes, n, "node")) return rc;
    rf_ctx* ctx = w->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    if (w->mode == kModeNone) return fail(RF_EPRECONDITION, "eval_wave: reject before any begin");
    if (!n) return RF_OK;
    HIPC(w->b_ids.ensure(4 * n));
    HIPC(hipMemcpyAsync(w->b_ids.p, nodes, 4 * n, hipMemcpyHostToDevice, s));
    HIPC(hipMemsetAsync(w->d.ctl + kWaveBad, 0, 4, s));
    HIPC(launch_wave_reject_check(w->d, w->b_ids.as<uint32_t>(), (uint32_t)n, s));
    if (int rc = wave_read_ctl(w, s)) return rc;
    if (w->ctl[kWaveBad]) return fail(RF_EINVAL, "eval_wave: reject lists a node that is not a hit");
    HIPC(launch_wave_reject(w->d, w->b_ids.as<uint32_t>(), (uint32_t)n, s));
    HIPC(launch_wave_count(w->d, s));
    return wave_read_ctl(w, s);
}

// ---- results ------------------------------------------------------------------
extern "C" int rf_eval_wave_states(rf_eval_wave* w, uint8_t* state) {
    ARG(w && (w->n == 0 || state), "null argument");
    std::lock_guard<std::mutex> lk(w->ctx->mu);
    DevGuard dg(w->ctx->device);
    HIPC(sync_copy(w->ctx, state, w->b_state.p, w->n, hipMemcpyDeviceToHost));
    return RF_OK;
}

extern "C" int rf_eval_wave_states_device(rf_eval_wave* w, const void** d_state) {
    ARG(w && d_state, "null argument");
    *d_state = w->b_state.p;
    return RF_OK;
}

// the three list launches on s (context mutex held)
static int wave_list_locked(rf_eval_wave* w, int state, int scope, uint64_t cap, void* d_nodes, void* d_which,
                            void* d_vals, void* d_found_mask, void* d_found, hipStream_t s) {
    const uint64_t tiles = (w->n + kPlanListTile - 1) / kPlanListTile;
    StreamScratch& sc = w->sc_tiles;
    std::lock_guard<std::mutex> lk(sc.mu);
    HIPC(sc.acquire(4 * std::max<uint64_t>(tiles, 1), s));
    hipError_t e = launch_wave_list(w->d, (uint32_t)state, scope == RF_WAVE_LAST, cap, sc.buf.as<uint32_t>(),
                                    static_cast<uint32_t*>(d_nodes), static_cast<uint8_t*>(d_which),
                                    static_cast<uint8_t*>(d_vals), static_cast<uint8_t*>(d_found_mask),
                                    static_cast<uint64_t*>(d_found), s);
    HIPC(sc.release(s));
    if (e != hipSuccess) return fail(RF_EDEVICE, "eval_wave list: %s", hipGetErrorString(e));
    return RF_OK;
}

extern "C" int rf_eval_wave_list_device(rf_eval_wave* w, int state, int scope, uint64_t cap, void* d_nodes,
                                        void* d_which, void* d_vals32, void* d_key_found, void* d_found, void* stream) {
    ARG(w && d_found && (cap == 0 || d_nodes), "null argument");
    ARG(state >= RF_PLAN_UNSEEN && state <= RF_PLAN_DONE, "unknown state");
    ARG(scope == RF_WAVE_ALL || scope == RF_WAVE_LAST, "unknown scope");
    std::lock_guard<std::mutex> lk(w->ctx->mu);
    DevGuard dg(w->ctx->device);
    return wave_list_locked(w, state, scope, cap, d_nodes, d_which, d_vals32, d_key_found, d_found,
                            pick(w->ctx, stream));
}

extern "C" int rf_eval_wave_list(rf_eval_wave* w, int state, int scope, uint64_t cap, uint32_t* nodes, uint8_t* which,
                                 uint8_t* vals32, uint8_t* key_found, uint64_t* found) {
    ARG(w && found && (cap == 0 || nodes), "null argument");
    ARG(state >= RF_PLAN_UNSEEN && state <= RF_PLAN_DONE, "unknown state");
    ARG(scope == RF_WAVE_ALL || scope == RF_WAVE_LAST, "unknown scope");
    rf_ctx* ctx = w->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    const bool hit = state == RF_PLAN_HIT;
    const uint64_t ecap = std::min(cap, w->n);  // (found <= n: min(found, cap) is unchanged)
    HIPC(w->b_lcount.ensure(8));
    HIPC(w->b_ln.ensure(4 * std::max<uint64_t>(ecap, 1)));
    if (hit && which) HIPC(w->b_lw.ensure(std::max<uint64_t>(ecap, 1)));
    if (hit && key_found) HIPC(w->b_lf.ensure(std::max<uint64_t>(ecap, 1)));
    if (hit && vals32) HIPC(w->b_lv.ensure(32 * std::max<uint64_t>(ecap, 1)));
    if (int rc = wave_list_locked(w, state, scope, ecap, w->b_ln.p, hit && which ? w->b_lw.p : nullptr,
                                  hit && vals32 ? w->b_lv.p : nullptr, hit && key_found ? w->b_lf.p : nullptr,
                                  w->b_lcount.p, s))
        return rc;
    uint64_t cnt = 0;
    HIPC(sync_copy(ctx, &cnt, w->b_lcount.p, 8, hipMemcpyDeviceToHost));
    *found = cnt;
    if (cnt > cap) return fail(RF_EINVAL, "list buffers too small: need %llu nodes", (unsigned long long)cnt);
    if (!cnt) return RF_OK;
    HIPC(hipMemcpyAsync(nodes, w->b_ln.p, 4 * cnt, hipMemcpyDeviceToHost, s));
    if (hit && which) HIPC(hipMemcpyAsync(which, w->b_lw.p, cnt, hipMemcpyDeviceToHost, s));
    if (hit && key_found) HIPC(hipMemcpyAsync(key_found, w->b_lf.p, cnt, hipMemcpyDeviceToHost, s));
    if (hit && vals32) HIPC(hipMemcpyAsync(vals32, w->b_lv.p, 32 * cnt, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return RF_OK;
}

extern "C" int rf_eval_wave_stats_get(rf_eval_wave* w, rf_eval_wave_stats* out, uint64_t size) {
    ARG(w && out, "null argument");
    ARG(size == sizeof(rf_eval_wave_stats), "rf_eval_wave_stats of another size (header mismatch)");
    std::lock_guard<std::mutex> lk(w->ctx->mu);
    *out = rf_eval_wave_stats{};
    out->n_nodes = w->n;
    out->n_deps = w->n_deps;
    out->depth = w->depth;
    out->mode = (uint32_t)w->mode;
    out->waves = w->waves;
    out->last_wave = w->last_wave;
    out->rounds = w->rounds;
    out->round_batch = w->round_batch;
    out->wave_lanes = plan_grid((uint32_t)w->n) * kPlanBlock;
    out->list_tile = kPlanListTile;
    for (int q = 0; q < 5; ++q) out->counts[q] = w->ctl[kWaveCounts + q];
    out->looked_up = w->ctl[kWaveLooked];
    out->keys_probed = w->ctl[kWaveProbed];
    out->keys_filtered = w->ctl[kWaveFiltered];
    for (DevBuf* b : w->all()) out->device_bytes += b->cap;
    out->device_bytes += w->sc_tiles.buf.cap;
    return RF_OK;
}
