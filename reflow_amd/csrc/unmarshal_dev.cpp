// unmarshal_dev.cpp -- Fileset JSON unmarshalled on the device
// (rf_fileset_unmarshal_device, rf_fileset_unmarshal, rf_fileset_forest_*): host
// side of k12_unmarshal.hip.  Check passes / one read-back of the layout word,
// the totals and the per-document status, reason and counts / outputs sized
// exactly / scatter, and the one word that says the scatter placed everything
// the counts announced.  The rows stay in HBM for rf_repo_missing_device and
// rf_liveset_set_values_device; the structure comes to the host on
// rf_fileset_forest_copy.
#include <hip/hip_runtime.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "ctx.h"
#include "unmarshal_flat.h"
#include "unmarshal_internal.h"

using namespace rf;

namespace {

struct ForestDev {
    rf_ctx* ctx = nullptr;
    int device = 0;
    DevBuf counts, ids, sizes, node_depth, entry_ptr, path_off, paths;
};

void forest_dev_free(void* p) {
    auto* d = static_cast<ForestDev*>(p);
    DevGuard dg(d->device);
    d->counts.release();
    d->ids.release();
    d->sizes.release();
    d->node_depth.release();
    d->entry_ptr.release();
    d->path_off.release();
    d->paths.release();
    delete d;
}

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

size_t lay_out(Carve& c, UnDev& u) {
    const size_t chunks = (size_t)u.tiles * kUnBlock, n = u.n;
    u.ctl = c.take<uint32_t>(4);
    u.totals = c.take<uint64_t>(4);
    u.ds = c.take<uint32_t>(n);
    u.de = c.take<uint32_t>(n);
    u.qm = c.take<uint16_t>(chunks);
    u.pm = c.take<uint16_t>(chunks);
    u.lq = c.take<uint16_t>(chunks);
    u.ld = c.take<uint16_t>(chunks);
    u.ln = c.take<uint16_t>(chunks);
    u.le = c.take<uint16_t>(chunks);
    u.lp = c.take<uint32_t>(chunks);
    u.tq = c.take<uint32_t>(u.tiles);
    u.td = c.take<uint32_t>(u.tiles);
    u.tn = c.take<uint32_t>(u.tiles);
    u.te = c.take<uint32_t>(u.tiles);
    u.tp = c.take<uint32_t>(u.tiles);
    u.bad = c.take<uint32_t>(n);
    u.sd = c.take<uint32_t>(n);
    u.sn = c.take<uint32_t>(n);
    u.se = c.take<uint32_t>(n);
    u.sp = c.take<uint32_t>(n);
    u.en = c.take<uint32_t>(n);
    u.ee = c.take<uint32_t>(n);
    u.ep = c.take<uint32_t>(n);
    u.bn = c.take<uint32_t>(n);
    u.be = c.take<uint32_t>(n);
    u.bp = c.take<uint32_t>(n);
    u.node_cnt = c.take<uint32_t>(n);
    u.reason = c.take<uint32_t>(n);
    return c.pos;
}

using clk = std::chrono::steady_clock;
double since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// (context mutex held) the arena and the document arrays are device memory
int unmarshal_locked(rf_ctx* ctx, const void* d_arena, uint64_t arena_bytes, const void* d_offs, const void* d_lens,
                     uint64_t n, rf_fileset_forest* f, hipStream_t s) {
    clk::time_point t0 = clk::now();
    HostForest& h = f->h;
    auto* fd = new ForestDev();
    fd->ctx = ctx;
    fd->device = ctx->device;
    f->dev = fd;
    f->dev_free = forest_dev_free;
    UnDev u;
    u.arena = static_cast<const uint8_t*>(d_arena);
    u.arena_bytes = (uint32_t)arena_bytes;
    u.n = (uint32_t)n;
    u.tiles = (uint32_t)((arena_bytes + RF_UNMARSHAL_TILE - 1) / RF_UNMARSHAL_TILE);
    u.offs = static_cast<const uint64_t*>(d_offs);
    u.lens = static_cast<const int64_t*>(d_lens);
    Carve sizing{nullptr};
    const size_t bytes = lay_out(sizing, u);
    HIPC(ctx->d_cw.ensure(bytes));
    Carve c{ctx->d_cw.as<uint8_t>()};
    lay_out(c, u);
    HIPC(fd->counts.ensure(4 * n));
    u.counts = fd->counts.as<uint32_t>();
    HIPC(hipMemsetAsync(u.ctl, 0, 16, s));
    HIPC(hipMemsetAsync(u.totals, 0, 32, s));
    HIPC(launch_unmarshal_check(u, s));
    // the one read-back
    uint32_t ctl = 0;
    uint64_t totals[3] = {0, 0, 0};
    h.reason.assign(n, 0);
    h.node_cnt.assign(n, 0);
    h.entry_cnt.assign(n, 0);
    HIPC(hipMemcpyAsync(&ctl, u.ctl, 4, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(totals, u.totals, 24, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h.reason.data(), u.reason, 4 * n, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h.node_cnt.data(), u.node_cnt, 4 * n, hipMemcpyDeviceToHost, s));
    HIPC(hipMemcpyAsync(h.entry_cnt.data(), u.counts, 4 * n, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (ctl) return fail(RF_EINVAL, "fileset unmarshal: documents not ascending, overlapping or outside the arena");
    h.status.assign(n, RF_OK);
    uint64_t nodes = 0, entries = 0;
    for (uint64_t d = 0; d < n; ++d) {
        if (h.reason[d] & kUnDisagree)
            return fail(RF_EDEVICE, "fileset unmarshal: the passes refused document %llu, which is canonical",
                        (unsigned long long)d);
        if (h.reason[d]) h.status[d] = RF_ENOTCANONICAL;
        h.n_accepted += h.reason[d] == 0;
        nodes += h.node_cnt[d];
        entries += h.entry_cnt[d];
    }
    if (nodes != totals[0] || entries != totals[1] || totals[2] > arena_bytes)
        return fail(RF_EDEVICE, "fileset unmarshal: the document counts do not add up to the scans' totals");
    h.n_docs = n;
    h.n_nodes = nodes;
    h.n_entries = entries;
    h.path_bytes = totals[2];
    f->ms[1] = since(t0);
    t0 = clk::now();
    HIPC(fd->ids.ensure(32 * entries));
    HIPC(fd->sizes.ensure(8 * entries));
    HIPC(fd->node_depth.ensure(4 * nodes));
    HIPC(fd->entry_ptr.ensure(8 * (nodes + 1)));
    HIPC(fd->path_off.ensure(8 * (entries + 1)));
    HIPC(fd->paths.ensure(h.path_bytes));
    u.n_nodes = nodes;
    u.n_entries = entries;
    u.path_bytes = h.path_bytes;
    u.node_depth = fd->node_depth.as<uint32_t>();
    u.entry_ptr = fd->entry_ptr.as<uint64_t>();
    u.path_off = fd->path_off.as<uint64_t>();
    u.paths = fd->paths.as<uint8_t>();
    u.ids32 = fd->ids.as<uint8_t>();
    u.sizes = fd->sizes.as<int64_t>();
    HIPC(hipMemsetAsync(u.entry_ptr, 0, 8, s));
    HIPC(hipMemcpyAsync(u.path_off + entries, &h.path_bytes, 8, hipMemcpyHostToDevice, s));
    HIPC(launch_unmarshal_scatter(u, s));
    uint32_t lost = 0;
    HIPC(hipMemcpyAsync(&lost, u.ctl + 1, 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (lost) return fail(RF_EDEVICE, "fileset unmarshal: the scatter and the counts of the check passes disagree");
    f->ms[2] = since(t0);
    return RF_OK;
}

int empty_forest(rf_fileset_forest** out) {
    auto* f = new rf_fileset_forest();
    f->h.structure = true;
    f->h.doc_node_ptr.assign(1, 0);
    f->h.entry_ptr.assign(1, 0);
    f->h.path_off.assign(1, 0);
    *out = f;
    return RF_OK;
}

}  // namespace

bool rf::forest_dev_arrays(const rf_fileset_forest* f, ForestArraysDev* out) {
    const auto* d = static_cast<const ForestDev*>(f->dev);
    if (!d) return false;
    out->ctx = d->ctx;
    out->node_depth = d->node_depth.as<uint32_t>();
    out->entry_ptr = d->entry_ptr.as<uint64_t>();
    out->path_off = d->path_off.as<uint64_t>();
    out->paths = d->paths.as<uint8_t>();
    out->ids32 = d->ids.as<uint8_t>();
    return true;
}

extern "C" void rf_fileset_forest_free(rf_fileset_forest* f) {
    if (!f) return;
    if (f->dev) f->dev_free(f->dev);
    delete f;
}

extern "C" int rf_fileset_unmarshal_device(rf_ctx* ctx, const void* d_arena, uint64_t arena_bytes, const void* d_offs,
                                           const void* d_lens, uint64_t n, rf_fileset_forest** out, void* stream) {
    ARG(ctx && out, "null argument");
    if (n == 0) return empty_forest(out);
    ARG(d_offs && d_lens && (d_arena || arena_bytes == 0), "null argument");
    ARG(arena_bytes < (1ull << 32), "fileset unmarshal: an arena of 4 GiB or more: split the batch");
    ARG(n < 0xffffffffull, "too many documents");
    ARG(reinterpret_cast<uintptr_t>(d_arena) % 16 == 0, "d_arena not 16-byte aligned");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    auto* f = new rf_fileset_forest();
    const int rc = unmarshal_locked(ctx, d_arena, arena_bytes, d_offs, d_lens, n, f, s);
    if (rc) {
        (void)hipStreamSynchronize(s);
        rf_fileset_forest_free(f);
        return rc;
    }
    *out = f;
    return RF_OK;
}

extern "C" int rf_fileset_unmarshal(rf_ctx* ctx, const uint8_t* json, const uint64_t* offs, uint64_t n,
                                    rf_fileset_forest** out, void* stream) {
    ARG(ctx && out, "null argument");
    if (n == 0) return empty_forest(out);
    ARG(offs && (json || offs[n] == 0), "null argument");
    ARG(n < 0xffffffffull, "too many documents");
    for (uint64_t d = 0; d < n; ++d) ARG(offs[d] <= offs[d + 1], "document offsets not ascending");
    ARG(offs[n] < (1ull << 32), "fileset unmarshal: 4 GiB of documents or more: split the batch");
    const clk::time_point t0 = clk::now();
    std::vector<int64_t> lens(n);
    for (uint64_t d = 0; d < n; ++d) lens[d] = (int64_t)(offs[d + 1] - offs[d]);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    const uint64_t total = offs[n];
    const size_t o_off = (total + 255) & ~size_t(255), l_off = o_off + 8 * n;
    HIPC(ctx->d_cw2.ensure(l_off + 8 * n));
    uint8_t* base = ctx->d_cw2.as<uint8_t>();
    if (total) HIPC(hipMemcpyAsync(base, json, total, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(base + o_off, offs, 8 * n, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(base + l_off, lens.data(), 8 * n, hipMemcpyHostToDevice, s));
    HIPC(hipStreamSynchronize(s));
    auto* f = new rf_fileset_forest();
    f->ms[0] = since(t0);
    const int rc = unmarshal_locked(ctx, base, total, base + o_off, base + l_off, n, f, s);
    if (rc) {
        (void)hipStreamSynchronize(s);
        rf_fileset_forest_free(f);
        return rc;
    }
    *out = f;
    return RF_OK;
}

extern "C" int rf_fileset_forest_rows_device(const rf_fileset_forest* f, const void** d_counts, const void** d_ids32,
                                             const void** d_sizes, uint64_t* n_rows) {
    ARG(f, "null forest");
    ARG(f->dev || f->h.n_docs == 0, "a host-form forest has no device rows");
    const auto* d = static_cast<const ForestDev*>(f->dev);
    if (d_counts) *d_counts = d ? d->counts.p : nullptr;
    if (d_ids32) *d_ids32 = d ? d->ids.p : nullptr;
    if (d_sizes) *d_sizes = d ? d->sizes.p : nullptr;
    if (n_rows) *n_rows = f->h.n_entries;
    return RF_OK;
}

extern "C" int rf_fileset_forest_copy(rf_fileset_forest* f, uint64_t* doc_node_ptr, uint32_t* node_depth,
                                      uint64_t* entry_ptr, uint64_t* path_off, uint8_t* paths, uint8_t* ids32,
                                      int64_t* sizes) {
    ARG(f, "null forest");
    HostForest& h = f->h;
    if (doc_node_ptr) {
        doc_node_ptr[0] = 0;
        for (uint64_t d = 0; d < h.n_docs; ++d) doc_node_ptr[d + 1] = doc_node_ptr[d] + h.node_cnt[d];
    }
    if (h.structure) {
        if (node_depth && h.n_nodes) memcpy(node_depth, h.node_depth.data(), 4 * h.n_nodes);
        if (entry_ptr) memcpy(entry_ptr, h.entry_ptr.data(), 8 * (h.n_nodes + 1));
        if (path_off) memcpy(path_off, h.path_off.data(), 8 * (h.n_entries + 1));
        if (paths && h.path_bytes) memcpy(paths, h.paths.data(), h.path_bytes);
        if (ids32 && h.n_entries) memcpy(ids32, h.ids32.data(), 32 * h.n_entries);
        if (sizes && h.n_entries) memcpy(sizes, h.sizes.data(), 8 * h.n_entries);
        return RF_OK;
    }
    auto* d = static_cast<ForestDev*>(f->dev);
    ARG(d, "forest without its device side");
    rf_ctx* ctx = d->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    const hipMemcpyKind k = hipMemcpyDeviceToHost;
    if (node_depth) HIPC(sync_copy(ctx, node_depth, d->node_depth.p, 4 * h.n_nodes, k));
    if (entry_ptr) HIPC(sync_copy(ctx, entry_ptr, d->entry_ptr.p, 8 * (h.n_nodes + 1), k));
    if (path_off) HIPC(sync_copy(ctx, path_off, d->path_off.p, 8 * (h.n_entries + 1), k));
    if (paths) HIPC(sync_copy(ctx, paths, d->paths.p, h.path_bytes, k));
    if (ids32) HIPC(sync_copy(ctx, ids32, d->ids.p, 32 * h.n_entries, k));
    if (sizes) HIPC(sync_copy(ctx, sizes, d->sizes.p, 8 * h.n_entries, k));
    return RF_OK;
}
