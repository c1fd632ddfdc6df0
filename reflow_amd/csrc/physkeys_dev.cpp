// physkeys_dev.cpp -- physical cache keys on the device (rf_physkeys_*): host
// side of k13_physkeys.hip.  Setting values: lengths + scans / one read-back of
// the documents' lengths / the arena's capacity decided here / emit.  An update:
// affected set / one read-back of its size / measure + scans / one read-back of
// the lengths for K1's planner / segments, gather, K1 through the context's
// one-shot plan, scatter.  The host keeps each value's (offset, length) beside
// the device's copy, so the value digests need no kernel of their own.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "cwrite_internal.h"
#include "physkeys_flat.h"
#include "physkeys_internal.h"
#include "unmarshal_flat.h"
#include "unmarshal_internal.h"
#include "wave_check.h"

using namespace rf;

struct rf_physkeys {
    rf_ctx* ctx = nullptr;
    int device = 0;
    uint64_t n = 0;
    DevBuf d_dep_ptr, d_deps, d_cons_ptr, d_cons, d_phys_row, d_suffix_ptr, d_suffix;
    DevBuf d_val_off, d_val_len, d_has, d_mark, d_tile_cnt;
    DevBuf d_arena;  // the store: every value's material at a 16-byte aligned offset, pads zero
    DevBuf d_set, d_upd, d_seg, d_out, d_dig, d_listed;  // per-call scratch: context mutex held, synced before return
    uint64_t used = 0, stale = 0, n_values = 0;
    std::vector<uint8_t> h_has;
    std::vector<uint64_t> h_off, h_len;
    std::vector<uint32_t> seen;  // [n] the call that last named the node (set values: which document is the last)
    uint32_t call = 0;
    hipEvent_t ev[7] = {};
    double last_ms[6] = {0, 0, 0, 0, 0, 0};
    std::vector<DevBuf*> all() {
        return {&d_dep_ptr, &d_deps, &d_cons_ptr, &d_cons, &d_phys_row, &d_suffix_ptr, &d_suffix, &d_val_off, &d_val_len,
                &d_has,     &d_mark, &d_tile_cnt, &d_arena, &d_set,     &d_upd,        &d_seg,    &d_out,     &d_dig,
                &d_listed};
    }
};

namespace {

// sub-buffers of one allocation, 256-byte aligned; base null: sizing only
struct Carve {
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

void pk_free(rf_physkeys* pk) {
    for (hipEvent_t& e : pk->ev)
        if (e) (void)hipEventDestroy(e);
    for (DevBuf* b : pk->all()) b->release();
    delete pk;
}

hipError_t up(void* dst, const void* src, size_t nb, hipStream_t s) {
    return nb ? hipMemcpyAsync(dst, src, nb, hipMemcpyHostToDevice, s) : hipSuccess;
}

// What a set-values call brings: the structure in host or device memory.
struct SetInput {
    uint64_t n_docs = 0, n_nodes = 0, n_entries = 0;
    const uint32_t* nodes = nullptr;              // host, the caller's
    std::vector<uint64_t> doc_node_ptr;           // host
    // device-resident (a forest) ...
    ForestArraysDev dev;
    // ... or host vectors to upload (a tree)
    const PhysTreeForest* host = nullptr;
    const uint8_t* h_ids32 = nullptr;   // the tree's IDs, when they are not on the device
    const uint8_t* d_ids32 = nullptr;   // the caller's device rows
    uint64_t n_id_rows = 0;             // rows of h_ids32
};

struct SetScratch {
    uint32_t *doc_node, *node_depth, *id_row;
    uint64_t *doc_node_ptr, *node_pre, *doc_len, *doc_off, *tile_tmp, *entry_ptr, *path_off;
    uint8_t *paths, *ids;
};

size_t lay_out(Carve& c, SetScratch& x, const SetInput& in) {
    x.doc_node = c.take<uint32_t>(in.n_docs);
    x.doc_node_ptr = c.take<uint64_t>(in.n_docs + 1);
    x.node_pre = c.take<uint64_t>(in.n_nodes + 1);
    x.doc_len = c.take<uint64_t>(in.n_docs);
    x.doc_off = c.take<uint64_t>(in.n_docs + 1);
    x.tile_tmp = c.take<uint64_t>(phys_tiles(std::max(in.n_nodes, in.n_docs)));
    const bool h = in.host != nullptr;
    x.node_depth = c.take<uint32_t>(h ? in.n_nodes : 0);
    x.entry_ptr = c.take<uint64_t>(h ? in.n_nodes + 1 : 0);
    x.path_off = c.take<uint64_t>(h ? in.n_entries + 1 : 0);
    x.id_row = c.take<uint32_t>(h ? in.n_entries : 0);
    x.paths = c.take<uint8_t>(h ? in.host->paths.size() : 0);
    x.ids = c.take<uint8_t>(in.h_ids32 ? 32 * in.n_id_rows + 16 : 0);
    return c.pos;
}

// Room for `need` bytes in the store: a larger arena, the stored bytes carried
// over (context mutex held; the stream is synchronised, nothing reads the old one).
int arena_reserve(rf_physkeys* pk, uint64_t need, hipStream_t s) {
    if (need <= pk->d_arena.cap) return RF_OK;
    DevBuf bigger;
    HIPC(bigger.ensure(std::max<uint64_t>(need, 2 * pk->d_arena.cap)));
    if (pk->used) {
        hipError_t e = hipMemcpyAsync(bigger.p, pk->d_arena.p, pk->used, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            bigger.release();
            return fail(RF_EDEVICE, "physkeys: arena growth: %s", hipGetErrorString(e));
        }
    }
    pk->d_arena.release();
    pk->d_arena = bigger;
    return RF_OK;
}

// (context mutex held)
int set_locked(rf_physkeys* pk, const SetInput& in, hipStream_t s) {
    const uint64_t nd = in.n_docs;
    // which documents count: a real node, accepted, the last that names its node
    std::vector<uint32_t> doc_node(in.nodes, in.nodes + nd);
    for (uint64_t d = 0; d < nd; ++d) {
        const uint32_t g = doc_node[d];
        if (g == kPhysSkip) continue;
        if (g >= pk->n) return fail(RF_EINVAL, "physkeys: value %llu: node %u out of range", (unsigned long long)d, g);
        if (in.doc_node_ptr[d] == in.doc_node_ptr[d + 1])
            return fail(RF_EINVAL, "physkeys: value %llu of node %u is a refused document", (unsigned long long)d, g);
    }
    if (++pk->call == 0) {
        std::fill(pk->seen.begin(), pk->seen.end(), 0u);
        pk->call = 1;
    }
    for (uint64_t d = nd; d-- > 0;) {
        const uint32_t g = doc_node[d];
        if (g == kPhysSkip) continue;
        if (pk->seen[g] == pk->call)
            doc_node[d] = kPhysSkip;
        else
            pk->seen[g] = pk->call;
    }
    SetScratch x{};
    Carve sizing{nullptr};
    const size_t bytes = lay_out(sizing, x, in);
    HIPC(pk->d_set.ensure(bytes));
    Carve c{pk->d_set.as<uint8_t>()};
    lay_out(c, x, in);
    HIPC(up(x.doc_node, doc_node.data(), 4 * nd, s));
    HIPC(up(x.doc_node_ptr, in.doc_node_ptr.data(), 8 * (nd + 1), s));
    PhysSetDev sd;
    sd.v.n_docs = nd;
    sd.v.n_nodes = in.n_nodes;
    sd.v.n_entries = in.n_entries;
    sd.v.doc_node = x.doc_node;
    sd.v.doc_node_ptr = x.doc_node_ptr;
    if (in.host) {
        const PhysTreeForest& h = *in.host;
        HIPC(up(x.node_depth, h.node_depth.data(), 4 * in.n_nodes, s));
        HIPC(up(x.entry_ptr, h.entry_ptr.data(), 8 * (in.n_nodes + 1), s));
        HIPC(up(x.path_off, h.path_off.data(), 8 * (in.n_entries + 1), s));
        HIPC(up(x.id_row, h.id_row.data(), 4 * in.n_entries, s));
        HIPC(up(x.paths, h.paths.data(), h.paths.size(), s));
        if (in.h_ids32) HIPC(up(x.ids, in.h_ids32, 32 * in.n_id_rows, s));
        sd.v.node_depth = x.node_depth;
        sd.v.entry_ptr = x.entry_ptr;
        sd.v.path_off = x.path_off;
        sd.v.paths = x.paths;
        sd.v.ids32 = in.h_ids32 ? x.ids : in.d_ids32;
        sd.v.id_row = x.id_row;
    } else {
        sd.v.node_depth = in.dev.node_depth;
        sd.v.entry_ptr = in.dev.entry_ptr;
        sd.v.path_off = in.dev.path_off;
        sd.v.paths = in.dev.paths;
        sd.v.ids32 = in.dev.ids32;
    }
    sd.node_pre = x.node_pre;
    sd.doc_len = x.doc_len;
    sd.doc_off = x.doc_off;
    sd.tile_tmp = x.tile_tmp;
    HIPC(launch_phys_lengths(sd, s));
    // the one read-back: the documents' lengths and the padded total
    std::vector<uint64_t> doc_len(nd);
    uint64_t total = 0;
    HIPC(hipMemcpyAsync(doc_len.data(), x.doc_len, 8 * nd, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(&total, x.doc_off + nd, 8, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    uint64_t pos = 0;
    for (uint64_t d = 0; d < nd; ++d) pos += phys_align16(doc_len[d]);
    if (pos != total) return fail(RF_EDEVICE, "physkeys: the documents' lengths do not add up to the scan's total");
    if (int rc = arena_reserve(pk, pk->used + total + 64, s)) return rc;
    if (total) HIPC(hipMemsetAsync(pk->d_arena.as<uint8_t>() + pk->used, 0, total, s));  // the pad bytes
    HIPC(launch_phys_emit(sd, pk->d_arena.as<uint8_t>(), pk->used, pk->d_val_off.as<uint64_t>(),
                          pk->d_val_len.as<uint64_t>(), pk->d_has.as<uint8_t>(), s));
    HIPC(hipStreamSynchronize(s));
    pos = pk->used;
    for (uint64_t d = 0; d < nd; ++d) {
        const uint32_t g = doc_node[d];
        if (g != kPhysSkip) {
            if (pk->h_has[g])
                pk->stale += phys_align16(pk->h_len[g]);
            else
                ++pk->n_values;
            pk->h_has[g] = 1;
            pk->h_off[g] = pos;
            pk->h_len[g] = doc_len[d];
        }
        pos += phys_align16(doc_len[d]);
    }
    pk->used += total;
    return RF_OK;
}

int nodes_ok(const rf_physkeys* pk, const uint32_t* nodes, uint64_t n) {
    ARG(n == 0 || nodes, "null nodes");
    ARG(n < (1ull << 32), "too many nodes listed");
    for (uint64_t i = 0; i < n; ++i)
        if (nodes[i] >= pk->n) return fail(RF_EINVAL, "physkeys: node %u out of range", nodes[i]);
    return RF_OK;
}

}  // namespace

extern "C" int rf_physkeys_open(rf_ctx* ctx, uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps,
                                const uint64_t* phys_row, const uint64_t* suffix_ptr, const uint8_t* suffix,
                                rf_physkeys** out) {
    ARG(ctx && out, "null argument");
    if (int rc = phys_graph_check(n, dep_ptr, deps, phys_row, suffix_ptr, suffix)) return rc;
    const uint64_t E = n ? dep_ptr[n] : 0, S = n ? suffix_ptr[n] : 0;
    std::vector<uint64_t> cons_ptr(n + 1, 0);
    std::vector<uint32_t> cons(E);
    char msg[160];
    if (!wave_consumers(n, dep_ptr, deps, cons_ptr.data(), cons.data(), msg, sizeof msg))
        return fail(RF_EINVAL, "physkeys: %s", msg);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    auto* pk = new rf_physkeys();
    pk->ctx = ctx;
    pk->device = ctx->device;
    pk->n = n;
    pk->h_has.assign(n, 0);
    pk->h_off.assign(n, 0);
    pk->h_len.assign(n, 0);
    pk->seen.assign(n, 0);
    auto run = [&]() -> int {
        hipStream_t s = ctx->stream;
        for (hipEvent_t& e : pk->ev) HIPC(hipEventCreate(&e));
        HIPC(pk->d_dep_ptr.ensure(8 * (n + 1)));
        HIPC(pk->d_cons_ptr.ensure(8 * (n + 1)));
        HIPC(pk->d_suffix_ptr.ensure(8 * (n + 1)));
        HIPC(pk->d_deps.ensure(4 * E));
        HIPC(pk->d_cons.ensure(4 * E));
        HIPC(pk->d_phys_row.ensure(8 * n));
        HIPC(pk->d_suffix.ensure(S));
        HIPC(pk->d_val_off.ensure(8 * n));
        HIPC(pk->d_val_len.ensure(8 * n));
        HIPC(pk->d_has.ensure(n));
        HIPC(pk->d_mark.ensure(n));
        HIPC(pk->d_tile_cnt.ensure(8 * (phys_tiles(n) + 1)));
        const uint64_t zero = 0;
        HIPC(up(pk->d_dep_ptr.p, n ? dep_ptr : &zero, 8 * (n + 1), s));
        HIPC(up(pk->d_cons_ptr.p, cons_ptr.data(), 8 * (n + 1), s));
        HIPC(up(pk->d_suffix_ptr.p, n ? suffix_ptr : &zero, 8 * (n + 1), s));
        HIPC(up(pk->d_deps.p, deps, 4 * E, s));
        HIPC(up(pk->d_cons.p, cons.data(), 4 * E, s));
        HIPC(up(pk->d_phys_row.p, phys_row, 8 * n, s));
        HIPC(up(pk->d_suffix.p, suffix, S, s));
        if (n) HIPC(hipMemsetAsync(pk->d_has.p, 0, n, s));
        HIPC(hipStreamSynchronize(s));
        return RF_OK;
    };
    if (int rc = run()) {
        (void)hipStreamSynchronize(ctx->stream);
        pk_free(pk);
        return rc;
    }
    *out = pk;
    return RF_OK;
}

// No context lock, as the other close calls.
extern "C" void rf_physkeys_close(rf_physkeys* pk) {
    if (!pk) return;
    DevGuard dg(pk->device);
    pk_free(pk);
}

extern "C" int rf_physkeys_set_values_forest(rf_physkeys* pk, const uint32_t* nodes, const rf_fileset_forest* f,
                                             void* stream) {
    ARG(pk && f, "null argument");
    const HostForest& h = f->h;
    if (h.n_docs == 0) return RF_OK;
    ARG(nodes, "null nodes");
    SetInput in;
    ARG(forest_dev_arrays(f, &in.dev), "physkeys: a host-form forest has no device arrays");
    ARG(in.dev.ctx == pk->ctx, "physkeys: the forest belongs to another context");
    in.n_docs = h.n_docs;
    in.n_nodes = h.n_nodes;
    in.n_entries = h.n_entries;
    in.nodes = nodes;
    in.doc_node_ptr.assign(h.n_docs + 1, 0);
    for (uint64_t d = 0; d < h.n_docs; ++d) in.doc_node_ptr[d + 1] = in.doc_node_ptr[d] + h.node_cnt[d];
    rf_ctx* ctx = pk->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    const int rc = set_locked(pk, in, s);
    if (rc) (void)hipStreamSynchronize(s);  // nothing of the call may still read the host arrays
    return rc;
}

extern "C" int rf_physkeys_set_values_tree(rf_physkeys* pk, const uint32_t* nodes, const rf_fileset_tree* t,
                                           const uint32_t* roots, uint64_t n, const void* d_ids32, void* stream) {
    ARG(pk, "null argument");
    if (n == 0) return RF_OK;
    ARG(nodes && roots, "null argument");
    ARG(reinterpret_cast<uintptr_t>(d_ids32) % 16 == 0, "d_ids32 not 16-byte aligned");
    PhysTreeForest tf;
    if (int rc = phys_tree_forest(t, roots, n, &tf)) return rc;
    SetInput in;
    in.n_docs = n;
    in.n_nodes = tf.node_depth.size();
    in.n_entries = tf.id_row.size();
    in.nodes = nodes;
    in.doc_node_ptr = tf.doc_node_ptr;
    in.host = &tf;
    in.d_ids32 = static_cast<const uint8_t*>(d_ids32);
    if (!d_ids32) {
        ARG(in.n_entries == 0 || t->ids32, "null ids32");
        in.h_ids32 = t->ids32;
        in.n_id_rows = t->entry_ptr[t->n_nodes];
    }
    rf_ctx* ctx = pk->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    const int rc = set_locked(pk, in, s);
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}

extern "C" int rf_physkeys_clear_values(rf_physkeys* pk, const uint32_t* nodes, uint64_t n) {
    ARG(pk, "null argument");
    if (int rc = nodes_ok(pk, nodes, n)) return rc;
    if (!n) return RF_OK;
    rf_ctx* ctx = pk->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = ctx->stream;
    HIPC(pk->d_listed.ensure(4 * n));
    HIPC(up(pk->d_listed.p, nodes, 4 * n, s));
    HIPC(launch_phys_clear(pk->d_listed.as<uint32_t>(), n, pk->d_has.as<uint8_t>(), s));
    HIPC(hipStreamSynchronize(s));
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t g = nodes[i];
        if (!pk->h_has[g]) continue;
        pk->h_has[g] = 0;
        pk->stale += phys_align16(pk->h_len[g]);
        --pk->n_values;
    }
    return RF_OK;
}

extern "C" int rf_physkeys_update(rf_physkeys* pk, const uint32_t* nodes, uint64_t n, uint32_t flags, void* d_keys32,
                                  uint64_t n_rows, rf_physkeys_out* o, void* stream) {
    ARG(pk, "null argument");
    ARG(flags && !(flags & ~(RF_PHYS_SELF | RF_PHYS_CONSUMERS)), "physkeys: flags are RF_PHYS_SELF, RF_PHYS_CONSUMERS or both");
    ARG(!o || o->size == sizeof(rf_physkeys_out), "rf_physkeys_out.size does not match this library");
    ARG(n_rows == 0 || d_keys32, "null d_keys32");
    ARG(reinterpret_cast<uintptr_t>(d_keys32) % 16 == 0, "d_keys32 not 16-byte aligned");
    if (int rc = nodes_ok(pk, nodes, n)) return rc;
    if (o) o->affected = o->keys_written = o->keys_zeroed = o->material_bytes = 0;
    if (!n || !pk->n) return RF_OK;
    rf_ctx* ctx = pk->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    auto run = [&]() -> int {
        const uint64_t tiles = phys_tiles(pk->n);
        PhysUpdDev u;
        auto lay_listed = [&](Carve& c) {
            u.listed = c.take<uint32_t>(n);
            u.list_off = c.take<uint64_t>(n + 1);
            u.list_tmp = c.take<uint64_t>(phys_tiles(n));
            return c.pos;
        };
        Carve sizing_listed{nullptr};
        HIPC(pk->d_listed.ensure(lay_listed(sizing_listed)));
        Carve cl{pk->d_listed.as<uint8_t>()};
        lay_listed(cl);
        HIPC(up(const_cast<uint32_t*>(u.listed), nodes, 4 * n, s));
        u.n = pk->n;
        u.dep_ptr = pk->d_dep_ptr.as<uint64_t>();
        u.cons_ptr = pk->d_cons_ptr.as<uint64_t>();
        u.phys_row = pk->d_phys_row.as<uint64_t>();
        u.suffix_ptr = pk->d_suffix_ptr.as<uint64_t>();
        u.deps = pk->d_deps.as<uint32_t>();
        u.cons = pk->d_cons.as<uint32_t>();
        u.val_off = pk->d_val_off.as<uint64_t>();
        u.val_len = pk->d_val_len.as<uint64_t>();
        u.has = pk->d_has.as<uint8_t>();
        u.n_listed = n;
        u.n_rows = n_rows;
        u.flags = flags;
        u.mark = pk->d_mark.as<uint8_t>();
        u.tile_cnt = pk->d_tile_cnt.as<uint64_t>();
        HIPC(hipEventRecord(pk->ev[0], s));
        HIPC(launch_phys_affected(u, s));
        uint64_t na = 0;
        HIPC(hipMemcpyAsync(&na, u.tile_cnt + tiles, 8, hipMemcpyDeviceToHost, s));
        HIPC(hipEventRecord(pk->ev[1], s));
        HIPC(hipStreamSynchronize(s));
        if (na > pk->n) return fail(RF_EDEVICE, "physkeys: more affected nodes than nodes");
        for (double& m : pk->last_ms) m = 0;
        float ms = 0;
        HIPC(hipEventElapsedTime(&ms, pk->ev[0], pk->ev[1]));
        pk->last_ms[0] = ms;
        if (!na) return RF_OK;
        u.n_aff = na;
        auto lay = [&](Carve& c) {
            u.aff = c.take<uint32_t>(na);
            u.comp = c.take<uint8_t>(na);
            u.mlen = c.take<uint64_t>(na);
            u.moff = c.take<uint64_t>(na + 1);
            u.seg_ptr = c.take<uint64_t>(na + 1);
            u.crank = c.take<uint64_t>(na + 1);
            u.tile_tmp = c.take<uint64_t>(phys_tiles(na));
            u.ctl = c.take<uint32_t>(4);
            return c.pos;
        };
        Carve sizing{nullptr};
        HIPC(pk->d_upd.ensure(lay(sizing)));
        Carve c{pk->d_upd.as<uint8_t>()};
        lay(c);
        HIPC(hipMemsetAsync(u.ctl, 0, 16, s));
        HIPC(launch_phys_measure(u, s));
        // the one read-back of an update: the lengths for K1's planner, the
        // computable bits, the scans' totals, the row-bound word
        std::vector<uint64_t> mlen(na);
        std::vector<uint8_t> comp(na);
        uint64_t out_bytes = 0, n_segs = 0, n_comp = 0;
        uint32_t bad_row = 0;
        HIPC(hipMemcpyAsync(mlen.data(), u.mlen, 8 * na, hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(comp.data(), u.comp, na, hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(&out_bytes, u.moff + na, 8, hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(&n_segs, u.seg_ptr + na, 8, hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(&n_comp, u.crank + na, 8, hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(&bad_row, u.ctl, 4, hipMemcpyDeviceToHost, s));
        const uint64_t listed_out = o && o->nodes ? std::min(na, o->cap) : 0;
        if (listed_out) HIPC(hipMemcpyAsync(o->nodes, u.aff, 4 * listed_out, hipMemcpyDeviceToHost, s));
        HIPC(hipEventRecord(pk->ev[2], s));
        HIPC(hipStreamSynchronize(s));
        if (bad_row) return fail(RF_EINVAL, "physkeys: an affected node's phys_row >= n_rows %llu", (unsigned long long)n_rows);
        if (out_bytes >= (1ull << 32))
            return fail(RF_EINVAL, "physkeys: the materials of one update reach 4 GiB (%llu bytes): split the call",
                        (unsigned long long)out_bytes);
        std::vector<uint64_t> offs, lens;
        offs.reserve(n_comp);
        lens.reserve(n_comp);
        uint64_t pos = 0, hashed = 0;
        for (uint64_t k = 0; k < na; ++k) {
            if (!comp[k]) continue;
            offs.push_back(pos);
            lens.push_back(mlen[k]);
            pos += phys_align16(mlen[k]);
            hashed += mlen[k];
        }
        if (offs.size() != n_comp || pos != out_bytes)
            return fail(RF_EDEVICE, "physkeys: the affected nodes' lengths do not add up to the scans' totals");
        HIPC(pk->d_seg.ensure(3 * 8 * std::max<uint64_t>(n_segs, 1)));
        u.seg_dst = pk->d_seg.as<uint64_t>();
        u.seg_src = u.seg_dst + n_segs;
        u.seg_len = u.seg_src + n_segs;
        HIPC(pk->d_out.ensure(out_bytes + 64));
        HIPC(pk->d_dig.ensure(32 * std::max<uint64_t>(n_comp, 1)));
        HIPC(launch_phys_segments(u, s));
        HIPC(hipEventRecord(pk->ev[3], s));
        HIPC(launch_phys_gather(u, n_segs, pk->d_arena.as<uint8_t>(), pk->d_suffix.as<uint8_t>(),
                                pk->d_out.as<uint8_t>(), out_bytes, s));
        HIPC(hipEventRecord(pk->ev[4], s));
        if (int rc = sha_resident_locked(ctx, pk->d_out.p, offs.data(), lens.data(), n_comp, pk->d_dig.p, s)) return rc;
        HIPC(hipEventRecord(pk->ev[5], s));
        HIPC(launch_phys_scatter(u, pk->d_dig.as<uint8_t>(), static_cast<uint8_t*>(d_keys32), s));
        HIPC(hipEventRecord(pk->ev[6], s));
        HIPC(hipStreamSynchronize(s));  // the rows are written; the one-shot plan is free for the next batch
        for (int i = 1; i < 6; ++i) {
            HIPC(hipEventElapsedTime(&ms, pk->ev[i], pk->ev[i + 1]));
            pk->last_ms[i] = ms;
        }
        if (o) {
            o->affected = na;
            o->keys_written = n_comp;
            o->keys_zeroed = na - n_comp;
            o->material_bytes = hashed;
            if (o->computable) memcpy(o->computable, comp.data(), std::min(na, o->cap));
        }
        return RF_OK;
    };
    const int rc = run();
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}

extern "C" int rf_physkeys_value_digests_device(rf_physkeys* pk, const uint32_t* nodes, uint64_t n, void* d_out32,
                                                void* stream) {
    ARG(pk && (n == 0 || d_out32), "null argument");
    if (int rc = nodes_ok(pk, nodes, n)) return rc;
    if (!n) return RF_OK;
    rf_ctx* ctx = pk->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    std::vector<uint64_t> offs(n), lens(n);
    for (uint64_t i = 0; i < n; ++i) {
        if (!pk->h_has[nodes[i]]) return fail(RF_EINVAL, "physkeys: node %u has no value", nodes[i]);
        offs[i] = pk->h_off[nodes[i]];
        lens[i] = pk->h_len[nodes[i]];
    }
    if (int rc = sha_resident_locked(ctx, pk->d_arena.p, offs.data(), lens.data(), n, d_out32, s)) return rc;
    HIPC(hipStreamSynchronize(s));
    return RF_OK;
}

extern "C" int rf_physkeys_value_material(rf_physkeys* pk, uint32_t node, uint8_t* out, uint64_t cap, uint64_t* len) {
    ARG(pk && len, "null argument");
    *len = 0;
    ARG(node < pk->n, "physkeys: node out of range");
    rf_ctx* ctx = pk->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (!pk->h_has[node]) return fail(RF_EINVAL, "physkeys: node %u has no value", node);
    *len = pk->h_len[node];
    if (*len > cap) return fail(RF_EINVAL, "output buffer too small: need %llu bytes", (unsigned long long)*len);
    if (!*len) return RF_OK;
    ARG(out, "null output buffer");
    HIPC(sync_copy(ctx, out, pk->d_arena.as<uint8_t>() + pk->h_off[node], *len, hipMemcpyDeviceToHost));
    return RF_OK;
}

extern "C" int rf_physkeys_stats_get(rf_physkeys* pk, rf_physkeys_stats* out) {
    ARG(pk && out, "null argument");
    std::lock_guard<std::mutex> lk(pk->ctx->mu);
    out->n_nodes = pk->n;
    out->n_values = pk->n_values;
    out->arena_bytes = pk->used;
    out->stale_bytes = pk->stale;
    out->device_bytes = 0;
    for (DevBuf* b : pk->all()) out->device_bytes += b->cap;
    for (int i = 0; i < 6; ++i) out->last_ms[i] = pk->last_ms[i];
    return RF_OK;
}
