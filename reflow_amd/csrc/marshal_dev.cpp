// marshal_dev.cpp -- Fileset values marshalled on the device (rf_fileset_marshal_device,
// rf_json_batch_*, rf_fileset_value_digest_device): host side of k11_cwrite.hip's
// marshal kernels.  Flatten (marshal_flat.cpp) / upload / length + scan / one
// read-back of the value lengths and the zero-ID word / emit; the digests run
// on K1 through the context's one-shot plan.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "ctx.h"
#include "cwrite_internal.h"
#include "marshal_flat.h"

using namespace rf;

struct rf_json_batch {
    rf_ctx* ctx = nullptr;
    int device = 0;
    uint64_t n = 0, total = 0, n_pieces = 0;
    double ms[3] = {0, 0, 0};  // flatten + sort / upload + length + scan + read-back / arena + emit
    std::vector<uint64_t> offs, lens;  // the values in the arena
    DevBuf d_arena, d_offs, d_lens;
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

struct Scratch {
    uint32_t *pa, *pb, *pv, *value_ptr, *local, *tile_count, *zero;
    uint8_t *blob, *paths, *ids;
    uint64_t *path_off, *ustart;
    int64_t* sizes;
};

size_t lay_out(Carve& c, Scratch& s, uint64_t np, uint64_t n, uint64_t ne, uint64_t blob, uint64_t path_bytes,
               bool ids) {
    const uint64_t tiles = (np + RF_MARSHAL_TILE - 1) / RF_MARSHAL_TILE;
    s.pa = c.take<uint32_t>(np);
    s.pb = c.take<uint32_t>(np);
    s.pv = c.take<uint32_t>(np);
    s.value_ptr = c.take<uint32_t>(n + 1);
    s.local = c.take<uint32_t>(np);
    s.tile_count = c.take<uint32_t>(tiles);
    s.zero = c.take<uint32_t>(1);
    s.blob = c.take<uint8_t>(blob);
    s.paths = c.take<uint8_t>(path_bytes);
    s.ids = c.take<uint8_t>(ids ? 32 * ne : 0);
    s.path_off = c.take<uint64_t>(ne + 1);
    s.ustart = c.take<uint64_t>(n + 1);
    s.sizes = c.take<int64_t>(ne);
    return c.pos;
}

void batch_free(rf_json_batch* b) {
    b->d_arena.release();
    b->d_offs.release();
    b->d_lens.release();
    delete b;
}

}  // namespace

extern "C" int rf_fileset_marshal_device(rf_ctx* ctx, const rf_fileset_tree* t, const uint32_t* roots, uint64_t n,
                                         const void* d_ids32, rf_json_batch** out, void* stream) {
    ARG(ctx && out && (n == 0 || roots), "null argument");
    ARG(reinterpret_cast<uintptr_t>(d_ids32) % 16 == 0, "d_ids32 not 16-byte aligned");
    using clock = std::chrono::steady_clock;
    auto since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
    clock::time_point t0 = clock::now();
    FlatPieces f;
    if (int rc = fileset_flatten(t, roots, n, d_ids32 == nullptr, 0, &f)) return rc;
    const uint64_t np = f.a.size();
    const uint64_t ne = t->entry_ptr[t->n_nodes];
    // the paths in one blob with offsets, and a bound on the JSON: every path
    // byte makes at most six, and the kernels count bytes in 32 bits
    std::vector<uint64_t> path_off(ne + 1, 0);
    for (uint64_t e = 0; e < ne; ++e) path_off[e + 1] = path_off[e] + t->path_lens[e];
    std::vector<uint8_t> paths(std::max<uint64_t>(path_off[ne], 1));
    for (uint64_t e = 0; e < ne; ++e)
        if (t->path_lens[e]) {
            ARG(t->paths[e], "null path");
            memcpy(paths.data() + path_off[e], t->paths[e], t->path_lens[e]);
        }
    uint64_t bound = 0;
    for (uint64_t p = 0; p < np; ++p)
        bound += (f.b[p] & kPieceEntry) ? 6ull * t->path_lens[f.a[p]] + 128 : f.b[p];
    if (bound >= (1ull << 32))
        return fail(RF_EINVAL, "fileset batch: the JSON may reach 4 GiB (bound %llu bytes): split the batch",
                    (unsigned long long)bound);

    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    auto* b = new rf_json_batch();
    b->ctx = ctx;
    b->device = ctx->device;
    b->n = n;
    b->n_pieces = np;
    b->ms[0] = since(t0);
    t0 = clock::now();
    b->offs.assign(n, 0);
    b->lens.assign(n, 0);
    if (n == 0) {
        *out = b;
        return RF_OK;
    }
    Scratch sc{};
    Carve sizing{nullptr};
    const size_t bytes = lay_out(sizing, sc, np, n, ne, f.blob.size(), paths.size(), d_ids32 == nullptr);
    int rc = RF_OK;
    auto run = [&]() -> int {
        HIPC(ctx->d_cw.ensure(bytes));
        Carve c{ctx->d_cw.as<uint8_t>()};
        lay_out(c, sc, np, n, ne, f.blob.size(), paths.size(), d_ids32 == nullptr);
        auto up = [&](void* dst, const void* src, size_t nb) {
            return nb ? hipMemcpyAsync(dst, src, nb, hipMemcpyHostToDevice, s) : hipSuccess;
        };
        HIPC(up(sc.pa, f.a.data(), 4 * np));
        HIPC(up(sc.pb, f.b.data(), 4 * np));
        HIPC(up(sc.pv, f.val.data(), 4 * np));
        HIPC(up(sc.value_ptr, f.value_ptr.data(), 4 * (n + 1)));
        HIPC(up(sc.blob, f.blob.data(), f.blob.size()));
        HIPC(up(sc.paths, paths.data(), path_off[ne]));
        HIPC(up(sc.path_off, path_off.data(), 8 * (ne + 1)));
        HIPC(up(sc.sizes, t->sizes, 8 * ne));
        if (!d_ids32) HIPC(up(sc.ids, t->ids32, 32 * ne));
        HIPC(hipMemsetAsync(sc.zero, 0, 4, s));
        MarshalDev m;
        m.n_pieces = (uint32_t)np;
        m.n_values = (uint32_t)n;
        m.pa = sc.pa;
        m.pb = sc.pb;
        m.pv = sc.pv;
        m.value_ptr = sc.value_ptr;
        m.blob = sc.blob;
        m.paths = sc.paths;
        m.path_off = sc.path_off;
        m.sizes = sc.sizes;
        m.ids32 = d_ids32 ? static_cast<const uint8_t*>(d_ids32) : sc.ids;
        m.local = sc.local;
        m.tile_count = sc.tile_count;
        m.ustart = sc.ustart;
        m.zero_seen = sc.zero;
        HIPC(launch_marshal_len(m, s));
        // the one read-back: bytes before each value, the total, the zero-ID word
        std::vector<uint64_t> ustart(n + 1);
        uint32_t zero = 0;
        HIPC(hipMemcpyAsync(ustart.data(), sc.ustart, 8 * (n + 1), hipMemcpyDeviceToHost, s));
        HIPC(hipMemcpyAsync(&zero, sc.zero, 4, hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        if (zero) return fail(RF_EINVAL, "fileset batch: zero file ID has no pinned JSON form");
        b->ms[1] = since(t0);
        t0 = clock::now();
        uint64_t pos = 0;
        for (uint64_t v = 0; v < n; ++v) {
            if (ustart[v + 1] < ustart[v] || ustart[v + 1] > bound)
                return fail(RF_EDEVICE, "fileset batch: value %llu has no length", (unsigned long long)v);
            b->lens[v] = ustart[v + 1] - ustart[v];
            b->offs[v] = pos;
            pos += (b->lens[v] + 15) & ~15ull;  // K1 wants offs % 16 == 0
        }
        b->total = ustart[n];
        HIPC(b->d_arena.ensure(pos + 64));
        HIPC(b->d_offs.ensure(8 * n));
        HIPC(b->d_lens.ensure(8 * n));
        HIPC(hipMemsetAsync(b->d_arena.p, 0, b->d_arena.cap, s));  // the pad bytes
        HIPC(up(b->d_offs.p, b->offs.data(), 8 * n));
        HIPC(up(b->d_lens.p, b->lens.data(), 8 * n));
        HIPC(launch_marshal_emit(m, b->d_offs.as<uint64_t>(), b->d_arena.as<uint8_t>(), s));
        HIPC(hipStreamSynchronize(s));
        b->ms[2] = since(t0);
        return RF_OK;
    };
    rc = run();
    if (rc) {
        (void)hipStreamSynchronize(s);  // nothing of the call may still read the host arrays
        batch_free(b);
        return rc;
    }
    *out = b;
    return RF_OK;
}

extern "C" int rf_json_batch_info(const rf_json_batch* b, uint64_t* n, uint64_t* total_bytes, uint64_t* n_pieces) {
    ARG(b, "null batch");
    if (n) *n = b->n;
    if (total_bytes) *total_bytes = b->total;
    if (n_pieces) *n_pieces = b->n_pieces;
    return RF_OK;
}

extern "C" int rf_json_batch_times(const rf_json_batch* b, double ms[3]) {
    ARG(b && ms, "null argument");
    for (int i = 0; i < 3; ++i) ms[i] = b->ms[i];
    return RF_OK;
}

extern "C" int rf_json_batch_lens(const rf_json_batch* b, int64_t* lens) {
    ARG(b && (b->n == 0 || lens), "null argument");
    for (uint64_t i = 0; i < b->n; ++i) lens[i] = (int64_t)b->lens[i];
    return RF_OK;
}

extern "C" int rf_json_batch_device(const rf_json_batch* b, const void** d_arena, const void** d_offs,
                                    const void** d_lens) {
    ARG(b, "null batch");
    if (d_arena) *d_arena = b->d_arena.p;
    if (d_offs) *d_offs = b->d_offs.p;
    if (d_lens) *d_lens = b->d_lens.p;
    return RF_OK;
}

extern "C" int rf_json_batch_copy(rf_json_batch* b, const uint64_t* which, uint64_t n, uint8_t* out, uint64_t cap,
                                  uint64_t* offs) {
    ARG(b && offs, "null argument");
    ARG(which || n <= b->n, "more values than the batch holds");
    uint64_t need = 0, lo = ~0ull, hi = 0;
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t v = which ? which[j] : j;
        if (v >= b->n) return fail(RF_EINVAL, "json batch: value %llu out of range", (unsigned long long)v);
        offs[j] = need;
        need += b->lens[v];
        if (b->lens[v]) {
            lo = std::min(lo, b->offs[v]);
            hi = std::max(hi, b->offs[v] + b->lens[v]);
        }
    }
    offs[n] = need;
    if (need > cap) return fail(RF_EINVAL, "output buffer too small: need %llu bytes", (unsigned long long)need);
    if (!need) return RF_OK;
    ARG(out, "null output buffer");
    rf_ctx* ctx = b->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    // one copy of the span the chosen values lie in, then the values out of it
    HIPC(ctx->h_stage.ensure(hi - lo));
    HIPC(sync_copy(ctx, ctx->h_stage.p, b->d_arena.as<uint8_t>() + lo, hi - lo, hipMemcpyDeviceToHost));
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t v = which ? which[j] : j;
        if (b->lens[v]) memcpy(out + offs[j], ctx->h_stage.bytes() + (b->offs[v] - lo), b->lens[v]);
    }
    return RF_OK;
}

extern "C" int rf_json_batch_digests_device(rf_json_batch* b, void* d_out32, void* stream) {
    ARG(b && (b->n == 0 || d_out32), "null argument");
    if (!b->n) return RF_OK;
    rf_ctx* ctx = b->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    hipStream_t s = pick(ctx, stream);
    if (int rc = sha_resident_locked(ctx, b->d_arena.p, b->offs.data(), b->lens.data(), b->n, d_out32, s)) return rc;
    HIPC(hipStreamSynchronize(s));  // the one-shot plan is free for the next batch
    return RF_OK;
}

// No context lock, as the other destroy calls.
extern "C" void rf_json_batch_free(rf_json_batch* b) {
    if (!b) return;
    DevGuard dg(b->device);
    batch_free(b);
}

extern "C" int rf_fileset_value_digest_device(rf_ctx* ctx, const rf_fileset_tree* t, const uint32_t* roots, uint64_t n,
                                              const void* d_ids32, void* d_out32, void* d_sizes, void* stream) {
    ARG(ctx && (n == 0 || d_out32), "null argument");
    rf_json_batch* b = nullptr;
    if (int rc = rf_fileset_marshal_device(ctx, t, roots, n, d_ids32, &b, stream)) return rc;
    int rc = rf_json_batch_digests_device(b, d_out32, stream);
    if (rc == RF_OK && d_sizes && n) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        DevGuard dg(ctx->device);
        hipError_t e = sync_copy(ctx, d_sizes, b->d_lens.p, 8 * n, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) rc = fail(RF_EDEVICE, "value digests: %s", hipGetErrorString(e));
    }
    rf_json_batch_free(b);
    return rc;
}
