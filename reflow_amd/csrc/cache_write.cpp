// cache_write.cpp -- Eval.CacheWrite for a batch of finished nodes
// (rf_eval_wave_cache_write, eval.go:1113-1154): host side of k11_cwrite.hip's
// key gather.  check + mark / scans / one read-back (a listed node not DONE,
// the Put and row totals, the skip counts) / scatter / the repository index's
// Put / the assoc's Put.  Nothing is touched before the read-back says every
// listed node is DONE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "cwrite_internal.h"
#include "graph_internal.h"
#include "plan_internal.h"
#include "wave_internal.h"

using namespace rf;

namespace {

struct Carve {  // sub-buffers of one allocation, 256-byte aligned; base null: sizing only
    uint8_t* base;
    size_t pos = 0;
    template <class T>
    T* take(size_t count) {
        pos = (pos + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + pos) : nullptr;
        pos += std::max<size_t>(count, 1) * sizeof(T);
        return p;
    }
};

struct Scratch {
    uint32_t *nodes, *tile_keys, *tile_nodes, *ctl;
    uint8_t *nput, *reason, *put_keys, *put_vals, *repo_ids;
    uint64_t* totals;
    int64_t* repo_sizes;
    int32_t* status;
};

size_t lay_out(Carve& c, Scratch& s, uint64_t n) {
    const uint64_t tiles = (n + RF_MARSHAL_TILE - 1) / RF_MARSHAL_TILE;
    s.nodes = c.take<uint32_t>(n);
    s.tile_keys = c.take<uint32_t>(tiles);
    s.tile_nodes = c.take<uint32_t>(tiles);
    s.ctl = c.take<uint32_t>(kCwWords);
    s.totals = c.take<uint64_t>(2);
    s.nput = c.take<uint8_t>(n);
    s.reason = c.take<uint8_t>(n);
    s.repo_ids = c.take<uint8_t>(32 * n);
    s.repo_sizes = c.take<int64_t>(n);
    return c.pos;
}

// the Put rows, once the read-back has said how many
size_t lay_out_puts(Carve& c, Scratch& s, uint64_t n, uint64_t puts) {
    s.put_keys = c.take<uint8_t>(32 * puts);
    s.put_vals = c.take<uint8_t>(32 * puts);
    s.status = c.take<int32_t>(std::max(puts, n));
    return c.pos;
}

}  // namespace

extern "C" int rf_eval_wave_cache_write(rf_eval_wave* w, const uint32_t* nodes, uint64_t n, const void* d_fsids32,
                                        const void* d_sizes, int no_cache_extern, rf_graph* g, const void* d_keys32,
                                        rf_assoc* a, int kind, rf_repo* repo, rf_cache_write_out* o, void* stream) {
    ARG(w && a && (n == 0 || (nodes && d_fsids32 && d_sizes)), "null argument");
    ARG(!o || o->size == sizeof(rf_cache_write_out), "rf_cache_write_out of another size (header mismatch)");
    ARG(kind >= 0 && kind < (1 << 30), "assoc kind out of range");
    ARG(reinterpret_cast<uintptr_t>(d_fsids32) % 16 == 0, "d_fsids32 not 16-byte aligned");
    ARG(n < (1ull << 27), "too many nodes listed");  // (8 keys each stay within one Put batch)
    rf_ctx* ctx = w->ctx;
    ARG(assoc_ctx(a) == ctx && (!g || g->ctx == ctx) && (!repo || repo_ctx(repo) == ctx),
        "wave, graph, assoc and repository index of different contexts");
    for (uint64_t i = 0; i < n; ++i)
        if (nodes[i] >= w->n) return fail(RF_EINVAL, "cache write: node %u out of range", nodes[i]);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    if (w->mode == kModeNone) return fail(RF_EPRECONDITION, "cache write: before any begin");
    CwDev c;
    if (g) {  // the keys as rf_eval_wave_step reads them
        if (!w->has_slots) return fail(RF_EPRECONDITION, "cache write: keys from a graph need key_slots at open");
        if (!g->initialized || g->marked)
            return fail(RF_EPRECONDITION, "cache write: the graph must be recomputed with no input change pending");
        if (w->n_keys && w->max_slot >= g->g.n_slots)
            return fail(RF_EINVAL, "cache write: key slot %u beyond the graph's %u slots", w->max_slot, g->g.n_slots);
        c.keys = g->g.slots;
        c.by_slot = true;
    } else {
        ARG(w->n_keys == 0 || d_keys32, "null keys");
        c.keys = static_cast<const uint8_t*>(d_keys32);
    }
    if (o) {
        uint8_t* nk = o->node_keys;
        *o = rf_cache_write_out{};
        o->size = sizeof(rf_cache_write_out);
        o->node_keys = nk;
    }
    if (!n) return RF_OK;

    Scratch sc{};
    Carve sizing{nullptr};
    HIPC(ctx->d_cw.ensure(lay_out(sizing, sc, n)));
    {
        Carve cv{ctx->d_cw.as<uint8_t>()};
        lay_out(cv, sc, n);
    }
    HIPC(hipMemcpyAsync(sc.nodes, nodes, 4 * n, hipMemcpyHostToDevice, s));
    HIPC(hipMemsetAsync(sc.ctl, 0, 4 * kCwWords, s));
    c.n = (uint32_t)n;
    c.nodes = sc.nodes;
    c.flags = w->d.flags;
    c.state = w->d.state;
    c.key_ptr = w->d.key_ptr;
    c.key_slots = w->d.key_slots;
    c.no_cache_extern = no_cache_extern ? 1 : 0;
    c.fsids = static_cast<const uint8_t*>(d_fsids32);
    c.sizes = static_cast<const int64_t*>(d_sizes);
    c.nput = sc.nput;
    c.reason = sc.reason;
    c.tile_keys = sc.tile_keys;
    c.tile_nodes = sc.tile_nodes;
    c.totals = sc.totals;
    c.ctl = sc.ctl;
    HIPC(launch_cw_mark(c, s));
    uint32_t ctl[kCwWords];
    uint64_t totals[2];
    HIPC(hipMemcpyAsync(ctl, sc.ctl, sizeof ctl, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(totals, sc.totals, sizeof totals, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (ctl[kCwBad]) return fail(RF_EINVAL, "cache write: a listed node is not DONE (call after the step)");
    const uint64_t puts = totals[0], rows = totals[1];
    if (puts > RF_PLAN_MAX_KEYS * n || rows > n) return fail(RF_EDEVICE, "cache write: the gather's totals are off");

    if (puts) {
        Carve sizing2{nullptr};
        HIPC(ctx->d_cw2.ensure(lay_out_puts(sizing2, sc, n, puts)));
        Carve cv{ctx->d_cw2.as<uint8_t>()};
        lay_out_puts(cv, sc, n, puts);
        HIPC(launch_cw_scatter(c, sc.put_keys, sc.put_vals, sc.repo_ids, sc.repo_sizes, s));
        if (s != ctx->stream) HIPC(hipStreamSynchronize(s));  // the Puts run on the context's stream
        if (repo)
            if (int rc = repo_put_rows_locked(repo, sc.repo_ids, sc.repo_sizes, rows, sc.status, ctx->stream)) return rc;
        if (int rc = assoc_put_rows_locked(a, kind, sc.put_keys, sc.put_vals, puts, sc.status)) return rc;
        HIPC(hipStreamSynchronize(ctx->stream));
    }
    if (o) {
        o->nodes_written = rows;
        o->keys_put = puts;
        o->skipped_not_cacheable = ctl[kCwSkip + kCwNotCacheable - 1];
        o->skipped_extern = ctl[kCwSkip + kCwExtern - 1];
        o->skipped_no_key = ctl[kCwSkip + kCwNoKey - 1];
        if (o->node_keys) HIPC(sync_copy(ctx, o->node_keys, sc.nput, n, hipMemcpyDeviceToHost));
    }
    return RF_OK;
}
