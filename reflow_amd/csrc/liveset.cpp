// liveset.cpp -- the GC liveset (rf_liveset_*): host side of k8_live.hip.  Owns
// one Flow graph's edges and its nodes' Fileset values (an append-only arena of
// (ID, Size) rows) on the device.  A run seeds the roots, enqueues the walk's
// rounds in batches with one small read-back per batch, lists the frontier
// values, scans their row counts (one 16-byte read-back: the host sizes the
// filter, bloom.EstimateParameters is double arithmetic), then dedups the rows
// per contribution, sums the firsts and builds the filter, and compares it
// with the previous run's.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

#include "ctx.h"
#include "engine.h"
#include "live_check.h"
#include "live_internal.h"
#include "plan_check.h"
#include "plan_internal.h"

using namespace rf;

struct rf_liveset {
    rf_ctx* ctx = nullptr;
    int device = 0;  // (kept: close must not touch a context that was destroyed first)
    uint64_t n = 0, n_edges = 0;
    uint32_t depth = 0;
    LiveArena arena;  // host mirror of the value records
    LiveDev d;
    DevBuf b_edge_ptr, b_edges, b_has, b_val_off, b_val_cnt, b_ids, b_sizes, b_claim, b_state, b_queue, b_ctl, b_res;
    DevBuf b_nodes, b_sh, b_so, b_sc;                             // set / clear: the listed records
    DevBuf b_roots, b_tiles, b_contrib, b_row_off, b_tile_rows;   // a run's lists
    DevBuf b_row_ord, b_row_src, b_slot_of, b_table;              // a run's rows
    DevBuf b_ln, b_lcount;                                        // the host-form list
    rf_bloom* filt[2] = {nullptr, nullptr};  // the last run's filter and the one before: they alternate
    int cur = -1;                            // filt[cur]: the last run's (-1: no run yet)
    uint32_t ctl[kLiveWords] = {};           // as last read
    rf_liveset_stats st{};                   // of the last run
    int64_t maxlivebytes = 0;
    std::vector<DevBuf*> all() {
        return {&b_edge_ptr, &b_edges,   &b_has,     &b_val_off,  &b_val_cnt, &b_ids,     &b_sizes,   &b_claim,
                &b_state,    &b_queue,   &b_ctl,     &b_res,      &b_nodes,   &b_sh,      &b_so,      &b_sc,
                &b_roots,    &b_tiles,   &b_contrib, &b_row_off,  &b_tile_rows, &b_row_ord, &b_row_src, &b_slot_of,
                &b_table,    &b_ln,      &b_lcount};
    }
};

rf_ctx* rf::live_ctx(rf_liveset* l) { return l->ctx; }
const LiveDev& rf::live_dev(rf_liveset* l) { return l->d; }

static void live_free(rf_liveset* l) {
    for (DevBuf* b : l->all()) b->release();
    bloom_lent_free(l->filt[0]);
    bloom_lent_free(l->filt[1]);
    delete l;
}

extern "C" int rf_liveset_open(rf_ctx* ctx, uint64_t n, const uint64_t* edge_ptr, const uint32_t* edges,
                               rf_liveset** out) {
    ARG(ctx && out && (n == 0 || edge_ptr), "null argument");
    uint32_t depth = 0;
    char msg[160];
    if (!plan_check(n, edge_ptr, edges, &depth, msg, sizeof msg)) return fail(RF_EINVAL, "liveset: %s", msg);
    const uint64_t E = n ? edge_ptr[n] : 0;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    auto* l = new rf_liveset();
    l->ctx = ctx;
    l->device = ctx->device;
    l->n = n;
    l->n_edges = E;
    l->depth = depth;
    l->arena.open(n);
    const uint64_t nw = (n + 31) / 32;
    const uint64_t n_pad = (n + kLiveListTile - 1) / kLiveListTile * kLiveListTile;
    struct Want {
        DevBuf* b;
        uint64_t bytes;
        const void* src;
        uint64_t src_bytes;
    } wants[] = {
        {&l->b_edge_ptr, 8 * (n + 1), edge_ptr, n ? 8 * (n + 1) : 0},
        {&l->b_edges, 4 * std::max<uint64_t>(E, 1), edges, 4 * E},
        {&l->b_has, std::max<uint64_t>(n, 1), nullptr, 0},
        {&l->b_val_off, 8 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&l->b_val_cnt, 4 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&l->b_claim, 4 * std::max<uint64_t>(nw, 1), nullptr, 0},
        {&l->b_state, std::max<uint64_t>(n_pad, 4), nullptr, 0},
        {&l->b_queue, 4 * std::max<uint64_t>(n, 1), nullptr, 0},
        {&l->b_ctl, 4 * kLiveWords, nullptr, 0},
        {&l->b_res, 8 * kLiveResWords, nullptr, 0},
    };
    for (const Want& w : wants) {
        hipError_t e = w.b->ensure(w.bytes);
        if (e == hipSuccess) e = hipMemsetAsync(w.b->p, 0, w.b->cap, ctx->stream);
        if (e == hipSuccess && w.src_bytes)
            e = hipMemcpyAsync(w.b->p, w.src, w.src_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->stream);
            live_free(l);
            return fail(e == hipErrorOutOfMemory ? RF_ENOMEM : RF_EDEVICE, "liveset alloc: %s", hipGetErrorString(e));
        }
    }
    if (hipError_t e = hipStreamSynchronize(ctx->stream); e != hipSuccess) {
        live_free(l);
        return fail(RF_EDEVICE, "liveset open: %s", hipGetErrorString(e));
    }
    LiveDev& d = l->d;
    d.n = (uint32_t)n;
    d.edge_ptr = l->b_edge_ptr.as<uint64_t>();
    d.edges = l->b_edges.as<uint32_t>();
    d.has = l->b_has.as<uint8_t>();
    d.val_off = l->b_val_off.as<uint64_t>();
    d.val_cnt = l->b_val_cnt.as<uint32_t>();
    d.claim = l->b_claim.as<uint32_t>();
    d.state = l->b_state.as<uint8_t>();
    d.queue = l->b_queue.as<uint32_t>();
    d.ctl = l->b_ctl.as<uint32_t>();
    d.res = l->b_res.as<unsigned long long>();
    l->st.n_nodes = n;
    l->st.counts[RF_LIVE_UNSEEN] = n;
    *out = l;
    return RF_OK;
}

// No context lock, as the other destroy calls: a binding's finalizers may run
// after the context's (its memory, mutex included, is gone by then).
extern "C" void rf_liveset_close(rf_liveset* l) {
    if (!l) return;
    DevGuard dg(l->device);
    live_free(l);
}

// ---- values ---------------------------------------------------------------------
// Room for `need` rows in all: a larger arena, the stored rows carried over
// (context mutex held; the stream is synchronised, so nothing reads the old one).
static int live_grow(rf_liveset* l, uint64_t need, hipStream_t s) {
    if (need <= l->arena.cap) return RF_OK;
    const uint64_t cap = l->arena.grown(need);
    DevBuf ids, sizes;
    hipError_t e = ids.ensure(32 * cap);
    if (e == hipSuccess) e = sizes.ensure(8 * cap);
    if (e == hipSuccess && l->arena.rows) {
        e = hipMemcpyAsync(ids.p, l->b_ids.p, 32 * l->arena.rows, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(sizes.p, l->b_sizes.p, 8 * l->arena.rows, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) {
        ids.release();
        sizes.release();
        return fail(e == hipErrorOutOfMemory ? RF_ENOMEM : RF_EDEVICE, "liveset arena: %s", hipGetErrorString(e));
    }
    l->b_ids.release();
    l->b_sizes.release();
    l->b_ids = ids;
    l->b_sizes = sizes;
    l->arena.cap = cap;
    l->d.ids = l->b_ids.as<uint8_t>();
    l->d.sizes = l->b_sizes.as<int64_t>();
    return RF_OK;
}

// The listed nodes' new records to the device (a node listed twice carries its
// last record both times).  The host mirror is updated by the caller after
// this has succeeded, so a failure leaves mirror and device in agreement.
static int live_push_records(rf_liveset* l, const uint32_t* nodes, const std::vector<uint8_t>& has,
                             const std::vector<uint64_t>& off, const std::vector<uint32_t>& cnt, uint64_t n_nodes,
                             hipStream_t s) {
    HIPC(l->b_nodes.ensure(4 * n_nodes));
    HIPC(l->b_sh.ensure(n_nodes));
    HIPC(l->b_so.ensure(8 * n_nodes));
    HIPC(l->b_sc.ensure(4 * n_nodes));
    HIPC(hipMemcpyAsync(l->b_nodes.p, nodes, 4 * n_nodes, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(l->b_sh.p, has.data(), n_nodes, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(l->b_so.p, off.data(), 8 * n_nodes, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(l->b_sc.p, cnt.data(), 4 * n_nodes, hipMemcpyHostToDevice, s));
    HIPC(launch_live_set(l->d, l->b_nodes.as<uint32_t>(), l->b_sh.as<uint8_t>(), l->b_so.as<uint64_t>(),
                         l->b_sc.as<uint32_t>(), (uint32_t)n_nodes, s));
    HIPC(hipStreamSynchronize(s));  // (the staging vectors go out of scope)
    return RF_OK;
}

static int live_set(rf_liveset* l, const uint32_t* nodes, const uint32_t* counts, uint64_t n_nodes, const void* ids,
                    const void* sizes, bool from_device, void* stream) {
    ARG(l && (n_nodes == 0 || (nodes && counts)), "null argument");
    ARG(n_nodes < (1ull << 32), "too many nodes listed");
    rf_ctx* ctx = l->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    uint64_t total = 0;
    char msg[160];
    if (!live_values_check(l->n, nodes, counts, n_nodes, l->arena.rows, &total, msg, sizeof msg))
        return fail(RF_EINVAL, "liveset set_values: %s", msg);
    ARG(total == 0 || (ids && sizes), "null rows");
    if (!n_nodes) return RF_OK;
    hipStream_t s = pick(ctx, stream);
    if (int rc = live_grow(l, l->arena.rows + total, s)) return rc;
    const uint64_t base = l->arena.rows;
    if (total) {
        const hipMemcpyKind kind = from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIPC(hipMemcpyAsync(l->b_ids.as<uint8_t>() + 32 * base, ids, 32 * total, kind, s));
        HIPC(hipMemcpyAsync(l->b_sizes.as<int64_t>() + base, sizes, 8 * total, kind, s));
    }
    // entry i's record: the rows of its node's last entry in this batch
    std::vector<uint64_t> at(n_nodes), off(n_nodes);
    std::vector<uint32_t> cnt(n_nodes);
    std::unordered_map<uint32_t, uint64_t> last;
    uint64_t row = base;
    for (uint64_t i = 0; i < n_nodes; ++i) {
        at[i] = row;
        row += counts[i];
        last[nodes[i]] = i;
    }
    for (uint64_t i = 0; i < n_nodes; ++i) {
        const uint64_t j = last[nodes[i]];
        off[i] = at[j];
        cnt[i] = counts[j];
    }
    if (int rc = live_push_records(l, nodes, std::vector<uint8_t>(n_nodes, 1), off, cnt, n_nodes, s)) return rc;
    l->arena.set(nodes, counts, n_nodes);
    return RF_OK;
}

extern "C" int rf_liveset_set_values(rf_liveset* l, const uint32_t* nodes, const uint32_t* counts, uint64_t n_nodes,
                                     const uint8_t* ids32, const int64_t* sizes) {
    return live_set(l, nodes, counts, n_nodes, ids32, sizes, false, nullptr);
}

extern "C" int rf_liveset_set_values_device(rf_liveset* l, const uint32_t* nodes, const uint32_t* counts,
                                            uint64_t n_nodes, const void* d_ids32, const void* d_sizes, void* stream) {
    return live_set(l, nodes, counts, n_nodes, d_ids32, d_sizes, true, stream);
}

extern "C" int rf_liveset_clear_values(rf_liveset* l, const uint32_t* nodes, uint64_t n_nodes) {
    ARG(l && (n_nodes == 0 || nodes), "null argument");
    ARG(n_nodes < (1ull << 32), "too many nodes listed");
    rf_ctx* ctx = l->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    char msg[160];
    if (!live_values_check(l->n, nodes, nullptr, n_nodes, l->arena.rows, nullptr, msg, sizeof msg))
        return fail(RF_EINVAL, "liveset clear_values: %s", msg);
    if (!n_nodes) return RF_OK;
    std::vector<uint64_t> off(n_nodes);
    for (uint64_t i = 0; i < n_nodes; ++i) off[i] = l->arena.off[nodes[i]];
    if (int rc = live_push_records(l, nodes, std::vector<uint8_t>(n_nodes, 0), off, std::vector<uint32_t>(n_nodes, 0),
                                   n_nodes, ctx->stream))
        return rc;
    l->arena.clear(nodes, n_nodes);
    return RF_OK;
}

// ---- run -------------------------------------------------------------------------
static int live_read_ctl(rf_liveset* l, hipStream_t s) {
    HIPC(hipMemcpyAsync(l->ctl, l->b_ctl.p, sizeof l->ctl, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return RF_OK;
}

static int live_ids_ok(rf_liveset* l, const uint32_t* ids, uint64_t n, const char* what) {
    ARG(n < (1ull << 32), "too many nodes listed");
    for (uint64_t i = 0; i < n; ++i)
        if (ids[i] >= l->n) return fail(RF_EINVAL, "liveset: %s %u out of range", what, ids[i]);
    return RF_OK;
}

// (context mutex held, device set)
static int live_run_locked(rf_liveset* l, const uint32_t* roots, uint64_t n_roots, const uint32_t* writers,
                           uint64_t n_writers, hipStream_t s) {
    // the walk (eval.go:809-826)
    const uint64_t nw = std::max<uint64_t>((l->n + 31) / 32, 1);
    HIPC(hipMemsetAsync(l->b_claim.p, 0, 4 * nw, s));
    HIPC(hipMemsetAsync(l->b_state.p, 0, l->b_state.cap, s));
    HIPC(hipMemsetAsync(l->b_ctl.p, 0, 4 * kLiveWords, s));
    HIPC(hipMemsetAsync(l->b_res.p, 0, 8 * kLiveResWords, s));
    if (n_roots) {
        HIPC(l->b_roots.ensure(4 * n_roots));
        HIPC(hipMemcpyAsync(l->b_roots.p, roots, 4 * n_roots, hipMemcpyHostToDevice, s));
    }
    HIPC(launch_live_seed(l->d, l->b_roots.as<uint32_t>(), (uint32_t)n_roots, s));
    uint32_t rounds = 0;
    if (int rc = live_read_ctl(l, s)) return rc;
    while (l->ctl[kLiveLo] != l->ctl[kLiveHi]) {
        if (rounds >= l->depth) return fail(RF_EDEVICE, "liveset: frontier not empty after %u rounds", l->depth);
        const uint32_t b = std::min<uint32_t>(RF_LIVE_ROUND_BATCH, l->depth - rounds);
        HIPC(launch_live_rounds(l->d, b, s));
        rounds += b;
        if (int rc = live_read_ctl(l, s)) return rc;
    }
    HIPC(launch_live_count(l->d, s));
    if (int rc = live_read_ctl(l, s)) return rc;
    // the contributions: the frontier's values ascending, then the writers (eval.go:827-835)
    const uint64_t nv = l->ctl[kLiveCounts + RF_LIVE_VALUE];
    const uint64_t C = nv + n_writers;
    ARG(C < (1ull << 32), "too many contributions");
    const uint64_t tiles = (l->n + kLiveListTile - 1) / kLiveListTile;
    const uint64_t ctiles = (C + kLiveListTile - 1) / kLiveListTile;
    HIPC(l->b_tiles.ensure(4 * std::max<uint64_t>(tiles, 1)));
    HIPC(l->b_lcount.ensure(8));
    HIPC(l->b_contrib.ensure(4 * std::max<uint64_t>(C, 1)));
    HIPC(l->b_row_off.ensure(8 * (C + 1)));
    HIPC(l->b_tile_rows.ensure(8 * std::max<uint64_t>(ctiles, 1)));
    if (nv)
        HIPC(launch_live_list(l->d, RF_LIVE_VALUE, nv, l->b_tiles.as<uint32_t>(), l->b_contrib.as<uint32_t>(),
                              l->b_lcount.as<uint64_t>(), s));
    if (n_writers)
        HIPC(hipMemcpyAsync(l->b_contrib.as<uint32_t>() + nv, writers, 4 * n_writers, hipMemcpyHostToDevice, s));
    LiveRows r;
    r.n_contrib = C;
    r.contrib = l->b_contrib.as<uint32_t>();
    r.row_off = l->b_row_off.as<uint64_t>();
    r.tile_rows = l->b_tile_rows.as<uint64_t>();
    HIPC(launch_live_offsets(l->d, r, s));
    uint64_t head[2] = {0, 0};  // nlive_est (and the word behind it): the one read-back the sizing needs
    HIPC(hipMemcpyAsync(head, l->b_res.p, 16, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    const uint64_t est = head[kLiveEst];
    if (est > RF_LIVE_MAX_ROWS)
        return fail(RF_EINVAL, "liveset: %llu rows in one run (at most 2^30)", (unsigned long long)est);
    // the filter (eval.go:838-843)
    uint64_t m = 64, k = 1;
    if (est) {
        char msg[96];
        if (!bloom_estimate(est, 0.001, &m, &k, msg, sizeof msg)) return fail(RF_EINVAL, "liveset: %s", msg);
        m = std::max<uint64_t>(m, 1);  // bloom.New (bloom.go:81-83)
        k = std::max<uint64_t>(k, 1);
    }
    const int next = l->cur < 0 ? 0 : l->cur ^ 1;
    if (int rc = bloom_lent_shape(l->ctx, &l->filt[next], m, k, s)) return rc;
    const BloomDev& fb = bloom_dev(l->filt[next]);
    // the rows (eval.go:848-858)
    if (est) {
        r.n_rows = (uint32_t)est;
        const uint32_t slots = live_table_slots(r.n_rows);
        HIPC(l->b_row_ord.ensure(4 * est));
        HIPC(l->b_row_src.ensure(8 * est));
        HIPC(l->b_slot_of.ensure(4 * est));
        HIPC(l->b_table.ensure(4ull * slots));
        r.row_ord = l->b_row_ord.as<uint32_t>();
        r.row_src = l->b_row_src.as<uint64_t>();
        r.slot_of = l->b_slot_of.as<uint32_t>();
        r.table = l->b_table.as<uint32_t>();
        r.mask = slots - 1;
        HIPC(launch_live_rows(l->d, r, fb, s));
    }
    // changed (eval.go:862; bloom.go:347-349, bitset.go:322-340)
    bool changed = l->cur < 0;
    if (!changed) {
        const BloomDev& pb = bloom_dev(l->filt[l->cur]);
        if (pb.m != m || pb.k != k || pb.length != fb.length) changed = true;
        else HIPC(launch_live_compare(l->d, pb.words, fb.words, (m + 63) / 64, s));
    }
    uint64_t res[kLiveResWords] = {};
    HIPC(hipMemcpyAsync(res, l->b_res.p, sizeof res, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (res[kLiveFlags] & kLiveFlagProbe)
        return fail(RF_EDEVICE, "liveset: dedup probe bound exceeded (run not applied)");
    changed = changed || (res[kLiveFlags] & kLiveFlagDiff);
    l->cur = next;
    rf_liveset_stats& st = l->st;
    for (int q = 0; q < 3; ++q) st.counts[q] = l->ctl[kLiveCounts + q];
    st.contributions = C;
    st.nlive_est = est;
    st.nlive = res[kLiveN];
    st.livebytes = (int64_t)res[kLiveBytes];
    l->maxlivebytes = std::max(l->maxlivebytes, st.livebytes);  // eval.go:859-861
    st.m = m;
    st.k = k;
    st.rounds = rounds;
    st.changed = changed ? 1 : 0;
    return RF_OK;
}

extern "C" int rf_liveset_run(rf_liveset* l, const uint32_t* roots, uint64_t n_roots, const uint32_t* writers,
                              uint64_t n_writers, void* stream) {
    ARG(l && (n_roots == 0 || roots) && (n_writers == 0 || writers), "null argument");
    if (int rc = live_ids_ok(l, roots, n_roots, "root")) return rc;
    if (int rc = live_ids_ok(l, writers, n_writers, "writer")) return rc;
    rf_ctx* ctx = l->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    return live_run_locked(l, roots, n_roots, writers, n_writers, pick(ctx, stream));
}

extern "C" int rf_liveset_filter(rf_liveset* l, rf_bloom** b) {
    ARG(l && b, "null argument");
    std::lock_guard<std::mutex> lk(l->ctx->mu);
    if (l->cur < 0) return fail(RF_EPRECONDITION, "liveset: no run yet");
    *b = l->filt[l->cur];
    return RF_OK;
}

// ---- results -----------------------------------------------------------------------
extern "C" int rf_liveset_states(rf_liveset* l, uint8_t* state) {
    ARG(l && (l->n == 0 || state), "null argument");
    std::lock_guard<std::mutex> lk(l->ctx->mu);
    DevGuard dg(l->ctx->device);
    HIPC(sync_copy(l->ctx, state, l->b_state.p, l->n, hipMemcpyDeviceToHost));
    return RF_OK;
}

extern "C" int rf_liveset_list(rf_liveset* l, int state, uint64_t cap, uint32_t* nodes, uint64_t* found) {
    ARG(l && found && (cap == 0 || nodes), "null argument");
    ARG(state >= RF_LIVE_UNSEEN && state <= RF_LIVE_VALUE, "unknown state");
    rf_ctx* ctx = l->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    const uint64_t ecap = std::min(cap, l->n);  // (found <= n: min(found, cap) is unchanged)
    const uint64_t tiles = (l->n + kLiveListTile - 1) / kLiveListTile;
    HIPC(l->b_tiles.ensure(4 * std::max<uint64_t>(tiles, 1)));
    HIPC(l->b_lcount.ensure(8));
    HIPC(l->b_ln.ensure(4 * std::max<uint64_t>(ecap, 1)));
    HIPC(launch_live_list(l->d, (uint32_t)state, ecap, l->b_tiles.as<uint32_t>(), l->b_ln.as<uint32_t>(),
                          l->b_lcount.as<uint64_t>(), s));
    uint64_t cnt = 0;
    HIPC(sync_copy(ctx, &cnt, l->b_lcount.p, 8, hipMemcpyDeviceToHost));
    *found = cnt;
    if (cnt > cap) return fail(RF_EINVAL, "list buffer too small: need %llu nodes", (unsigned long long)cnt);
    if (cnt) HIPC(sync_copy(ctx, nodes, l->b_ln.p, 4 * cnt, hipMemcpyDeviceToHost));
    return RF_OK;
}

extern "C" int rf_liveset_stats_get(rf_liveset* l, rf_liveset_stats* out, uint64_t size) {
    ARG(l && out, "null argument");
    ARG(size == sizeof(rf_liveset_stats), "rf_liveset_stats of another size (header mismatch)");
    std::lock_guard<std::mutex> lk(l->ctx->mu);
    *out = l->st;
    out->n_nodes = l->n;
    out->maxlivebytes = l->maxlivebytes;
    out->arena_rows = l->arena.rows;
    out->stale_rows = l->arena.stale;
    out->device_bytes = 0;
    for (DevBuf* b : l->all()) out->device_bytes += b->cap;
    out->device_bytes += bloom_device_bytes(l->filt[0]) + bloom_device_bytes(l->filt[1]);
    return RF_OK;
}
