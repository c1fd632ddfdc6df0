// repo.cpp -- the repository index (rf_repo_*): host side of k9_repo.hip.  Owns
// the table (tag, ID, size per slot) and its counters on the device, decides
// growth before a Put batch from one read of the counters, and drives the
// missing / need_transfer sequence: segment offsets, one read-back of the row
// total (the host sizes the dedup table), rows located, deduplicated per group,
// the firsts counted and looked up, the missing ones listed.
//
// A device-form call may leave work on the caller's stream that reads the
// table and the object's scratch; it records an event there, and every later
// call on the object waits for that event before it touches either.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "ctx.h"
#include "cwrite_internal.h"
#include "engine.h"
#include "host_par.h"
#include "live_internal.h"
#include "plan_internal.h"  // bloom_ctx, bloom_dev: the filter object behind rf_bloom*, as a fused lookup sees it
#include "repo_check.h"
#include "repo_internal.h"
#include "repo_io.h"

using namespace rf;

struct rf_repo {
    rf_ctx* ctx = nullptr;
    int device = 0;  // (kept: destroy must not touch a context that was destroyed first)
    uint64_t slots = 0, rebuilds = 0, last_rows = 0;
    hipEvent_t e_reader = nullptr;
    bool reader_pending = false;
    DevBuf tag, keys, size, ctr;                                             // the table
    DevBuf b_ids, b_sizes, b_status, b_removed, b_canon, b_slot_of, b_table;  // a batch
    DevBuf b_counts, b_nodes, b_deg, b_bad, b_seg_base, b_seg_group, b_seg_src, b_seg_cnt, b_seg_off, b_tile_sums;
    DevBuf b_row_ord, b_row_src, b_nfiles, b_nmissing, b_mbytes, b_gstatus, b_miss, b_tiles, b_total, b_miss_ptr;
    DevBuf b_lrows, b_lids, b_lsizes;  // the host form's list
    DevBuf b_itiles, b_ioff, b_dead;   // scan / collect_list: counts and offsets per tile of slots, the dead marks
    std::vector<DevBuf*> scratch() {
        return {&b_ids,     &b_sizes,    &b_status,  &b_removed,  &b_canon,   &b_slot_of,  &b_table,  &b_counts,
                &b_nodes,   &b_deg,      &b_bad,     &b_seg_base, &b_seg_group, &b_seg_src, &b_seg_cnt, &b_seg_off,
                &b_tile_sums, &b_row_ord, &b_row_src, &b_nfiles,  &b_nmissing, &b_mbytes,  &b_gstatus, &b_miss,
                &b_tiles,   &b_total,    &b_miss_ptr, &b_lrows,   &b_lids,    &b_lsizes,  &b_itiles,  &b_ioff,
                &b_dead};
    }
    RepoView view() {
        return RepoView{tag.as<uint32_t>(), keys.as<uint4>(), size.as<long long>(), (uint32_t)(slots - 1),
                        ctr.as<unsigned long long>()};
    }
};

static void repo_free(rf_repo* r) {
    if (r->e_reader) {
        if (r->reader_pending) (void)hipEventSynchronize(r->e_reader);
        (void)hipEventDestroy(r->e_reader);
    }
    for (DevBuf* b : {&r->tag, &r->keys, &r->size, &r->ctr}) b->release();
    for (DevBuf* b : r->scratch()) b->release();
    delete r;
}

static hipError_t repo_alloc_table(DevBuf& tag, DevBuf& keys, DevBuf& size, uint64_t slots, hipStream_t s) {
    hipError_t e;
    if ((e = tag.ensure(4 * slots)) != hipSuccess || (e = keys.ensure(32 * slots)) != hipSuccess ||
        (e = size.ensure(8 * slots)) != hipSuccess)
        return e;
    return hipMemsetAsync(tag.p, 0, 4 * slots, s);
}

extern "C" int rf_repo_new(rf_ctx* ctx, uint64_t capacity, rf_repo** out) {
    ARG(ctx && out, "null argument");
    uint64_t slots = 0;
    char msg[160];
    if (!repo_slots_for(capacity, &slots, msg, sizeof msg)) return fail(RF_EINVAL, "repo: %s", msg);
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    auto* r = new rf_repo();
    r->ctx = ctx;
    r->device = ctx->device;
    r->slots = slots;
    hipError_t e = repo_alloc_table(r->tag, r->keys, r->size, slots, ctx->stream);
    if (e == hipSuccess) e = r->ctr.ensure(8 * kRepoCtrWords);
    if (e == hipSuccess) e = hipMemsetAsync(r->ctr.p, 0, 8 * kRepoCtrWords, ctx->stream);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->e_reader, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        repo_free(r);
        return fail(e == hipErrorOutOfMemory ? RF_ENOMEM : RF_EDEVICE, "repo alloc: %s", hipGetErrorString(e));
    }
    *out = r;
    return RF_OK;
}

// No context lock, as the other destroy calls.
extern "C" void rf_repo_destroy(rf_repo* r) {
    if (!r) return;
    DevGuard dg(r->device);
    repo_free(r);
}

// (context mutex held) what an earlier device-form call left on its stream is done
static int repo_quiesce(rf_repo* r) {
    if (r->reader_pending) {
        HIPC(hipEventSynchronize(r->e_reader));
        r->reader_pending = false;
    }
    return RF_OK;
}
static int repo_mark_reader(rf_repo* r, hipStream_t s) {
    HIPC(hipEventRecord(r->e_reader, s));
    r->reader_pending = true;
    return RF_OK;
}

// The counters, read on s.  A probe bound hit by any call so far fails this one too (fail-stop).
static int repo_read_ctr(rf_repo* r, uint64_t (&c)[kRepoCtrWords], hipStream_t s) {
    HIPC(hipMemcpyAsync(c, r->ctr.p, sizeof c, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    if (c[kRepoFlags] & kRepoFlagProbe) return fail(RF_EDEVICE, "repo: probe bound exceeded (the index is not usable)");
    return RF_OK;
}

static int repo_rebuild(rf_repo* r, uint64_t slots, hipStream_t s) {
    DevBuf tag, keys, size;
    hipError_t e = repo_alloc_table(tag, keys, size, slots, s);
    if (e != hipSuccess) {  // no room for the new table: the old one stays in place
        tag.release();
        keys.release();
        size.release();
        return fail(e == hipErrorOutOfMemory ? RF_ENOMEM : RF_EDEVICE, "repo alloc: %s", hipGetErrorString(e));
    }
    RepoView to{tag.as<uint32_t>(), keys.as<uint4>(), size.as<long long>(), (uint32_t)(slots - 1),
                r->ctr.as<unsigned long long>()};
    e = launch_repo_rebuild(r->view(), r->slots, to, slots, s);
    if (e == hipSuccess) e = hipMemsetAsync(r->ctr.as<uint64_t>() + kRepoTombs, 0, 8, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        tag.release();
        keys.release();
        size.release();
        return fail(RF_EDEVICE, "repo rebuild: %s", hipGetErrorString(e));
    }
    r->tag.release();
    r->keys.release();
    r->size.release();
    r->tag = tag;
    r->keys = keys;
    r->size = size;
    r->slots = slots;
    ++r->rebuilds;
    return RF_OK;
}

// the dedup's arrays for n rows
static int repo_dedup_bufs(rf_repo* r, RepoRows& rows) {
    const uint32_t slots = live_table_slots(rows.n_rows);
    HIPC(r->b_slot_of.ensure(4ull * rows.n_rows));
    HIPC(r->b_table.ensure(4ull * slots));
    rows.slot_of = r->b_slot_of.as<uint32_t>();
    rows.table = r->b_table.as<uint32_t>();
    rows.mask = slots - 1;
    return RF_OK;
}

// ---- put / remove / stat ---------------------------------------------------------
// (context mutex held, device set, quiesced) rows and status in device memory
static int repo_put_locked(rf_repo* r, const uint8_t* d_ids, const int64_t* d_sizes, uint64_t n, int32_t* d_status,
                           hipStream_t s) {
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, s)) return rc;
    uint64_t want = r->slots;
    char msg[160];
    if (!repo_growth(r->slots, c[kRepoObjects], c[kRepoTombs], n, &want, msg, sizeof msg))
        return fail(RF_EINVAL, "repo put: %s", msg);
    if (want != r->slots)
        if (int rc = repo_rebuild(r, want, s)) return rc;
    if (!n) return RF_OK;
    RepoRows rows;
    rows.n_rows = (uint32_t)n;
    rows.ids = d_ids;
    rows.sizes = d_sizes;
    if (int rc = repo_dedup_bufs(r, rows)) return rc;
    HIPC(r->b_canon.ensure(4 * n));
    HIPC(launch_repo_dedup(rows, s));
    HIPC(launch_repo_canon(rows, r->b_canon.as<uint32_t>(), r->ctr.as<unsigned long long>(), s));
    HIPC(launch_repo_put(r->view(), rows, r->b_canon.as<uint32_t>(), d_status, s));
    return repo_read_ctr(r, c, s);
}

extern "C" int rf_repo_put(rf_repo* r, const uint8_t* ids32, const int64_t* sizes, uint64_t n, int32_t* status) {
    ARG(r && (n == 0 || (ids32 && sizes && status)), "null argument");
    char msg[160];
    if (!repo_rows_check(n, msg, sizeof msg) || !repo_sizes_check(sizes, n, msg, sizeof msg))
        return fail(RF_EINVAL, "repo put: %s", msg);
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = ctx->stream;
    if (n) {
        HIPC(r->b_ids.ensure(32 * n));
        HIPC(r->b_sizes.ensure(8 * n));
        HIPC(r->b_status.ensure(4 * n));
        HIPC(hipMemcpyAsync(r->b_ids.p, ids32, 32 * n, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(r->b_sizes.p, sizes, 8 * n, hipMemcpyHostToDevice, s));
    }
    if (int rc = repo_put_locked(r, r->b_ids.as<uint8_t>(), r->b_sizes.as<int64_t>(), n, r->b_status.as<int32_t>(), s))
        return rc;
    if (n) HIPC(sync_copy(ctx, status, r->b_status.p, 4 * n, hipMemcpyDeviceToHost));
    return RF_OK;
}

extern "C" int rf_repo_put_device(rf_repo* r, const void* d_ids32, const void* d_sizes, uint64_t n, void* d_status,
                                  void* stream) {
    ARG(r && (n == 0 || (d_ids32 && d_sizes && d_status)), "null argument");
    char msg[160];
    if (!repo_rows_check(n, msg, sizeof msg)) return fail(RF_EINVAL, "repo put: %s", msg);
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    return repo_put_locked(r, static_cast<const uint8_t*>(d_ids32), static_cast<const int64_t*>(d_sizes), n,
                           static_cast<int32_t*>(d_status), pick(ctx, stream));
}

rf_ctx* rf::repo_ctx(rf_repo* r) { return r->ctx; }
int rf::repo_put_rows_locked(rf_repo* r, const uint8_t* d_ids, const int64_t* d_sizes, uint64_t n, int32_t* d_status,
                             hipStream_t s) {
    char msg[160];
    if (!repo_rows_check(n, msg, sizeof msg)) return fail(RF_EINVAL, "repo put: %s", msg);
    if (int rc = repo_quiesce(r)) return rc;
    return repo_put_locked(r, d_ids, d_sizes, n, d_status, s);
}

static int repo_remove_locked(rf_repo* r, const uint8_t* d_ids, uint64_t n, uint8_t* d_removed, hipStream_t s) {
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, s)) return rc;
    if (!n) return RF_OK;
    RepoRows rows;
    rows.n_rows = (uint32_t)n;
    rows.ids = d_ids;
    if (int rc = repo_dedup_bufs(r, rows)) return rc;
    HIPC(r->b_canon.ensure(4 * n));
    HIPC(launch_repo_dedup(rows, s));
    HIPC(launch_repo_canon(rows, r->b_canon.as<uint32_t>(), r->ctr.as<unsigned long long>(), s));
    HIPC(launch_repo_remove(r->view(), rows, r->b_canon.as<uint32_t>(), d_removed, s));
    return repo_read_ctr(r, c, s);
}

extern "C" int rf_repo_remove(rf_repo* r, const uint8_t* ids32, uint64_t n, uint8_t* removed) {
    ARG(r && (n == 0 || (ids32 && removed)), "null argument");
    char msg[160];
    if (!repo_rows_check(n, msg, sizeof msg)) return fail(RF_EINVAL, "repo remove: %s", msg);
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = ctx->stream;
    if (n) {
        HIPC(r->b_ids.ensure(32 * n));
        HIPC(r->b_removed.ensure(n));
        HIPC(hipMemcpyAsync(r->b_ids.p, ids32, 32 * n, hipMemcpyHostToDevice, s));
    }
    if (int rc = repo_remove_locked(r, r->b_ids.as<uint8_t>(), n, r->b_removed.as<uint8_t>(), s)) return rc;
    if (n) HIPC(sync_copy(ctx, removed, r->b_removed.p, n, hipMemcpyDeviceToHost));
    return RF_OK;
}

extern "C" int rf_repo_remove_device(rf_repo* r, const void* d_ids32, uint64_t n, void* d_removed, void* stream) {
    ARG(r && (n == 0 || (d_ids32 && d_removed)), "null argument");
    char msg[160];
    if (!repo_rows_check(n, msg, sizeof msg)) return fail(RF_EINVAL, "repo remove: %s", msg);
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    return repo_remove_locked(r, static_cast<const uint8_t*>(d_ids32), n, static_cast<uint8_t*>(d_removed),
                              pick(ctx, stream));
}

extern "C" int rf_repo_stat(rf_repo* r, const uint8_t* ids32, uint64_t n, int64_t* sizes) {
    ARG(r && (n == 0 || (ids32 && sizes)), "null argument");
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    if (!n) return RF_OK;
    hipStream_t s = ctx->stream;
    HIPC(r->b_ids.ensure(32 * n));
    HIPC(r->b_sizes.ensure(8 * n));
    HIPC(hipMemcpyAsync(r->b_ids.p, ids32, 32 * n, hipMemcpyHostToDevice, s));
    HIPC(launch_repo_stat(r->view(), r->b_ids.as<uint8_t>(), n, r->b_sizes.as<int64_t>(), s));
    HIPC(hipMemcpyAsync(sizes, r->b_sizes.p, 8 * n, hipMemcpyDeviceToHost, s));
    uint64_t c[kRepoCtrWords];
    return repo_read_ctr(r, c, s);
}

extern "C" int rf_repo_stat_device(rf_repo* r, const void* d_ids32, uint64_t n, void* d_sizes, void* stream) {
    ARG(r && (n == 0 || (d_ids32 && d_sizes)), "null argument");
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    if (!n) return RF_OK;
    hipStream_t s = pick(ctx, stream);
    HIPC(launch_repo_stat(r->view(), static_cast<const uint8_t*>(d_ids32), n, static_cast<int64_t*>(d_sizes), s));
    return repo_mark_reader(r, s);
}

extern "C" int rf_repo_collect(rf_repo* r, rf_bloom* live, uint64_t* removed, int64_t* removed_bytes, void* stream) {
    ARG(r, "null argument");
    rf_ctx* ctx = r->ctx;
    ARG(!live || bloom_ctx(live) == ctx, "the filter belongs to another context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = pick(ctx, stream);
    HIPC(launch_repo_collect(r->view(), r->slots, live ? &bloom_dev(live) : nullptr, s));
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, s)) return rc;
    if (removed) *removed = c[kRepoGone];
    if (removed_bytes) *removed_bytes = (int64_t)c[kRepoGoneBytes];
    return RF_OK;
}

extern "C" int rf_repo_stats_get(rf_repo* r, rf_repo_stats* out, uint64_t size) {
    ARG(r && out, "null argument");
    ARG(size == sizeof(rf_repo_stats), "rf_repo_stats of another size (header mismatch)");
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, ctx->stream)) return rc;
    out->objects = c[kRepoObjects];
    out->bytes = (int64_t)c[kRepoBytes];
    out->tombstones = c[kRepoTombs];
    out->capacity = r->slots;
    out->rebuilds = r->rebuilds;
    out->device_bytes = r->tag.cap + r->keys.cap + r->size.cap + r->ctr.cap;
    for (DevBuf* b : r->scratch()) out->device_bytes += b->cap;
    out->last_rows = r->last_rows;
    out->last_files = c[kRepoLastFiles];
    out->last_missing = c[kRepoLastMissing];
    return RF_OK;
}

// ---- missing / need_transfer -------------------------------------------------------
struct MissIn {
    // the row form: counts and rows in device memory; known_rows: the total where the host has it, else ~0
    const uint32_t* d_counts = nullptr;
    const uint8_t* d_ids = nullptr;
    const int64_t* d_sizes = nullptr;
    uint64_t known_rows = ~0ull, max_rows = 0;
    // need_transfer: the liveset and the nodes in device memory
    rf_liveset* l = nullptr;
    const uint32_t* d_nodes = nullptr;
    uint64_t n_groups = 0;
};
// the list arrays the scatter writes (device memory; any may be null)
struct MissList {
    uint64_t cap = 0;
    uint64_t* rows = nullptr;
    uint8_t* ids = nullptr;
    int64_t* sizes = nullptr;
};

static int repo_read_total(rf_repo* r, uint64_t* v, hipStream_t s) {
    HIPC(hipMemcpyAsync(v, r->b_total.p, 8, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    return RF_OK;
}

// (context mutex held, device set, quiesced)  Leaves in the object's buffers:
// b_nfiles / b_nmissing / b_mbytes / b_gstatus [G], b_miss_ptr [G + 1] and
// b_total[0] = the missing files in all, and in `rows` what repo_list_locked needs.
static int repo_missing_locked(rf_repo* r, const MissIn& in, RepoRows& rows, hipStream_t s) {
    const uint64_t G = in.n_groups;
    const uint64_t G1 = std::max<uint64_t>(G, 1);
    char msg[160];
    HIPC(hipMemsetAsync(r->ctr.as<uint64_t>() + kRepoLastFiles, 0, 16, s));
    r->last_rows = 0;
    HIPC(r->b_nfiles.ensure(4 * G1));
    HIPC(r->b_nmissing.ensure(4 * G1));
    HIPC(r->b_mbytes.ensure(8 * G1));
    HIPC(r->b_gstatus.ensure(4 * G1));
    HIPC(r->b_miss_ptr.ensure(8 * (G + 1)));
    HIPC(r->b_total.ensure(16));
    HIPC(r->b_tile_sums.ensure(8 * ((G + kRepoListTile - 1) / kRepoListTile + 1)));
    HIPC(hipMemsetAsync(r->b_nfiles.p, 0, 4 * G1, s));
    HIPC(hipMemsetAsync(r->b_nmissing.p, 0, 4 * G1, s));
    HIPC(hipMemsetAsync(r->b_mbytes.p, 0, 8 * G1, s));
    HIPC(hipMemsetAsync(r->b_gstatus.p, 0, 4 * G1, s));

    rows = RepoRows();
    rows.by_size = 1;
    const uint64_t* seg_off = nullptr;
    const uint32_t* seg_group = nullptr;
    const uint64_t* seg_src = nullptr;
    uint64_t n_segs = 0, R = 0;
    if (in.l) {
        const LiveDev& ld = live_dev(in.l);
        HIPC(r->b_deg.ensure(4 * G1));
        HIPC(r->b_bad.ensure(4 * G1));
        HIPC(r->b_seg_base.ensure(8 * (G + 1)));
        HIPC(launch_repo_nt_degrees(ld, in.d_nodes, G, r->b_deg.as<uint32_t>(), r->b_bad.as<uint32_t>(), s));
        HIPC(launch_repo_scan(r->b_deg.as<uint32_t>(), G, r->b_tile_sums.as<uint64_t>(), r->b_seg_base.as<uint64_t>(),
                              r->b_total.as<uint64_t>(), s));
        uint64_t S = 0;
        if (int rc = repo_read_total(r, &S, s)) return rc;
        if (S > (1ull << 31)) return fail(RF_EINVAL, "repo need_transfer: %llu edges in one call", (unsigned long long)S);
        const uint64_t S1 = std::max<uint64_t>(S, 1);
        HIPC(r->b_seg_group.ensure(4 * S1));
        HIPC(r->b_seg_src.ensure(8 * S1));
        HIPC(r->b_seg_cnt.ensure(4 * S1));
        HIPC(r->b_seg_off.ensure(8 * (S + 1)));
        HIPC(r->b_tile_sums.ensure(8 * ((std::max(S, G) + kRepoListTile - 1) / kRepoListTile + 1)));
        HIPC(launch_repo_nt_segments(ld, in.d_nodes, r->b_seg_base.as<uint64_t>(), G, S, r->b_seg_group.as<uint32_t>(),
                                     r->b_seg_src.as<uint64_t>(), r->b_seg_cnt.as<uint32_t>(),
                                     r->b_bad.as<uint32_t>(), s));
        HIPC(launch_repo_scan(r->b_seg_cnt.as<uint32_t>(), S, r->b_tile_sums.as<uint64_t>(),
                              r->b_seg_off.as<uint64_t>(), r->b_total.as<uint64_t>(), s));
        if (int rc = repo_read_total(r, &R, s)) return rc;
        HIPC(launch_repo_copy_status(r->b_bad.as<uint32_t>(), r->b_gstatus.as<int32_t>(), G, s));
        seg_off = r->b_seg_off.as<uint64_t>();
        seg_group = r->b_seg_group.as<uint32_t>();
        seg_src = r->b_seg_src.as<uint64_t>();
        n_segs = S;
        rows.ids = ld.ids;
        rows.sizes = ld.sizes;
    } else {
        HIPC(r->b_seg_off.ensure(8 * (G + 1)));
        HIPC(launch_repo_scan(in.d_counts, G, r->b_tile_sums.as<uint64_t>(), r->b_seg_off.as<uint64_t>(),
                              r->b_total.as<uint64_t>(), s));
        R = in.known_rows;
        if (R == ~0ull)
            if (int rc = repo_read_total(r, &R, s)) return rc;
        if (R > in.max_rows)
            return fail(RF_EINVAL, "repo missing: the counts sum to %llu rows, %llu given", (unsigned long long)R,
                        (unsigned long long)in.max_rows);
        seg_off = r->b_seg_off.as<uint64_t>();
        n_segs = G;
        rows.ids = in.d_ids;
        rows.sizes = in.d_sizes;
    }
    if (!repo_rows_check(R, msg, sizeof msg)) return fail(RF_EINVAL, "repo missing: %s", msg);
    r->last_rows = R;
    if (R) {
        rows.n_rows = (uint32_t)R;
        const uint64_t tiles = (R + kRepoListTile - 1) / kRepoListTile;
        HIPC(r->b_row_ord.ensure(4 * R));
        if (in.l) HIPC(r->b_row_src.ensure(8 * R));
        HIPC(r->b_miss.ensure(tiles * kRepoListTile));
        HIPC(r->b_tiles.ensure(4 * tiles));
        if (int rc = repo_dedup_bufs(r, rows)) return rc;
        HIPC(hipMemsetAsync(r->b_miss.p, 0, tiles * kRepoListTile, s));
        HIPC(launch_repo_locate(seg_off, n_segs, seg_group, seg_src, rows.n_rows, r->b_row_ord.as<uint32_t>(),
                                in.l ? r->b_row_src.as<uint64_t>() : nullptr, s));
        rows.row_ord = r->b_row_ord.as<uint32_t>();
        rows.row_src = in.l ? r->b_row_src.as<uint64_t>() : nullptr;
        HIPC(launch_repo_dedup(rows, s));
        HIPC(launch_repo_resolve(r->view(), rows, r->b_nfiles.as<uint32_t>(), r->b_nmissing.as<uint32_t>(),
                                 r->b_mbytes.as<unsigned long long>(), r->b_miss.as<uint8_t>(), s));
    }
    // the list's offsets per group, and the total
    HIPC(launch_repo_scan(r->b_nmissing.as<uint32_t>(), G, r->b_tile_sums.as<uint64_t>(), r->b_miss_ptr.as<uint64_t>(),
                          r->b_total.as<uint64_t>(), s));
    return RF_OK;
}

// the missing firsts of the rows just resolved, ascending, into `list`
static int repo_list_locked(rf_repo* r, const RepoRows& rows, const MissList& list, hipStream_t s) {
    if (rows.n_rows && list.cap && (list.rows || list.ids || list.sizes))
        HIPC(launch_repo_list(rows, r->b_miss.as<uint8_t>(), r->b_tiles.as<uint32_t>(), list.cap, list.rows, list.ids,
                              list.sizes, r->b_total.as<uint64_t>() + 1, s));
    return RF_OK;
}

// the per-group arrays and the total to the caller's pointers
static int repo_deliver(rf_repo* r, uint64_t G, const rf_repo_missing_out* o, bool with_status, hipMemcpyKind kind,
                        hipStream_t s) {
    if (o->n_files && G) HIPC(hipMemcpyAsync(o->n_files, r->b_nfiles.p, 4 * G, kind, s));
    if (o->n_missing && G) HIPC(hipMemcpyAsync(o->n_missing, r->b_nmissing.p, 4 * G, kind, s));
    if (o->missing_bytes && G) HIPC(hipMemcpyAsync(o->missing_bytes, r->b_mbytes.p, 8 * G, kind, s));
    if (with_status && o->status && G) HIPC(hipMemcpyAsync(o->status, r->b_gstatus.p, 4 * G, kind, s));
    if (o->miss_ptr) HIPC(hipMemcpyAsync(o->miss_ptr, r->b_miss_ptr.p, 8 * (G + 1), kind, s));
    if (o->n_listed) HIPC(hipMemcpyAsync(o->n_listed, r->b_total.p, 8, kind, s));
    return RF_OK;
}

// the host forms: the list through the object's staging
static int repo_missing_host(rf_repo* r, const MissIn& in, rf_repo_missing_out* o, bool row_form, hipStream_t s) {
    RepoOutPlan plan;
    char msg[160];
    if (!repo_out_plan(o, row_form, &plan, msg, sizeof msg)) return fail(RF_EINVAL, "repo missing: %s", msg);
    RepoRows rows;
    if (int rc = repo_missing_locked(r, in, rows, s)) return rc;
    uint64_t total = 0;
    if (int rc = repo_read_total(r, &total, s)) return rc;
    MissList list;
    list.cap = std::min(plan.cap, total);  // (min(total, cap) entries are written either way)
    if (list.cap) {
        if (plan.rows) {
            HIPC(r->b_lrows.ensure(8 * list.cap));
            list.rows = r->b_lrows.as<uint64_t>();
        }
        if (o->miss_ids32) {
            HIPC(r->b_lids.ensure(32 * list.cap));
            list.ids = r->b_lids.as<uint8_t>();
        }
        if (o->miss_sizes) {
            HIPC(r->b_lsizes.ensure(8 * list.cap));
            list.sizes = r->b_lsizes.as<int64_t>();
        }
    }
    if (int rc = repo_list_locked(r, rows, list, s)) return rc;
    if (int rc = repo_deliver(r, in.n_groups, o, !row_form, hipMemcpyDeviceToHost, s)) return rc;
    const uint64_t w = std::min(total, list.cap);
    if (w) {
        if (list.rows) HIPC(hipMemcpyAsync(o->miss_rows, list.rows, 8 * w, hipMemcpyDeviceToHost, s));
        if (list.ids) HIPC(hipMemcpyAsync(o->miss_ids32, list.ids, 32 * w, hipMemcpyDeviceToHost, s));
        if (list.sizes) HIPC(hipMemcpyAsync(o->miss_sizes, list.sizes, 8 * w, hipMemcpyDeviceToHost, s));
    }
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, s)) return rc;
    if (plan.list && total > plan.cap)
        return fail(RF_EINVAL, "list buffers too small: need %llu entries", (unsigned long long)total);
    return RF_OK;
}

static int repo_missing_device(rf_repo* r, const MissIn& in, rf_repo_missing_out* o, bool row_form, hipStream_t s) {
    RepoOutPlan plan;
    char msg[160];
    if (!repo_out_plan(o, row_form, &plan, msg, sizeof msg)) return fail(RF_EINVAL, "repo missing: %s", msg);
    MissList list;
    list.cap = plan.cap;
    list.rows = plan.rows ? o->miss_rows : nullptr;
    list.ids = o->miss_ids32;
    list.sizes = o->miss_sizes;
    RepoRows rows;
    int rc = repo_missing_locked(r, in, rows, s);
    if (!rc) rc = repo_list_locked(r, rows, list, s);
    if (!rc) rc = repo_deliver(r, in.n_groups, o, !row_form, hipMemcpyDeviceToDevice, s);
    if (int rc2 = repo_mark_reader(r, s)) return rc ? rc : rc2;
    return rc;
}

extern "C" int rf_repo_missing(rf_repo* r, const uint32_t* counts, uint64_t n_groups, const uint8_t* ids32,
                               const int64_t* sizes, rf_repo_missing_out* o) {
    ARG(r && o && (n_groups == 0 || counts), "null argument");
    ARG(n_groups < (1ull << 32), "too many groups");
    uint64_t total = 0;
    char msg[160];
    if (!repo_counts_check(counts, n_groups, &total, msg, sizeof msg)) return fail(RF_EINVAL, "repo missing: %s", msg);
    ARG(total == 0 || (ids32 && sizes), "null rows");
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = ctx->stream;
    HIPC(r->b_counts.ensure(4 * std::max<uint64_t>(n_groups, 1)));
    HIPC(r->b_ids.ensure(32 * std::max<uint64_t>(total, 1)));
    HIPC(r->b_sizes.ensure(8 * std::max<uint64_t>(total, 1)));
    if (n_groups) HIPC(hipMemcpyAsync(r->b_counts.p, counts, 4 * n_groups, hipMemcpyHostToDevice, s));
    if (total) {
        HIPC(hipMemcpyAsync(r->b_ids.p, ids32, 32 * total, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(r->b_sizes.p, sizes, 8 * total, hipMemcpyHostToDevice, s));
    }
    MissIn in;
    in.d_counts = r->b_counts.as<uint32_t>();
    in.d_ids = r->b_ids.as<uint8_t>();
    in.d_sizes = r->b_sizes.as<int64_t>();
    in.known_rows = in.max_rows = total;
    in.n_groups = n_groups;
    return repo_missing_host(r, in, o, true, s);
}

extern "C" int rf_repo_missing_device(rf_repo* r, const void* d_counts, uint64_t n_groups, const void* d_ids32,
                                      const void* d_sizes, uint64_t n_rows, rf_repo_missing_out* o, void* stream) {
    ARG(r && o && (n_groups == 0 || d_counts) && (n_rows == 0 || (d_ids32 && d_sizes)), "null argument");
    ARG(n_groups < (1ull << 32), "too many groups");
    char msg[160];
    if (!repo_rows_check(n_rows, msg, sizeof msg)) return fail(RF_EINVAL, "repo missing: %s", msg);
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    MissIn in;
    in.d_counts = static_cast<const uint32_t*>(d_counts);
    in.d_ids = static_cast<const uint8_t*>(d_ids32);
    in.d_sizes = static_cast<const int64_t*>(d_sizes);
    in.max_rows = n_rows;
    in.n_groups = n_groups;
    return repo_missing_device(r, in, o, true, pick(ctx, stream));
}

extern "C" int rf_repo_need_transfer(rf_repo* r, rf_liveset* l, const uint32_t* nodes, uint64_t n_nodes,
                                     rf_repo_missing_out* o) {
    ARG(r && l && o && (n_nodes == 0 || nodes), "null argument");
    ARG(n_nodes < (1ull << 32), "too many nodes listed");
    rf_ctx* ctx = r->ctx;
    ARG(live_ctx(l) == ctx, "the liveset belongs to another context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    const uint32_t n = live_dev(l).n;
    for (uint64_t i = 0; i < n_nodes; ++i)
        if (nodes[i] >= n) return fail(RF_EINVAL, "repo need_transfer: node %u out of range", nodes[i]);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = ctx->stream;
    HIPC(r->b_nodes.ensure(4 * std::max<uint64_t>(n_nodes, 1)));
    if (n_nodes) HIPC(hipMemcpyAsync(r->b_nodes.p, nodes, 4 * n_nodes, hipMemcpyHostToDevice, s));
    MissIn in;
    in.l = l;
    in.d_nodes = r->b_nodes.as<uint32_t>();
    in.n_groups = n_nodes;
    return repo_missing_host(r, in, o, false, s);
}

extern "C" int rf_repo_need_transfer_device(rf_repo* r, rf_liveset* l, const void* d_nodes, uint64_t n_nodes,
                                            rf_repo_missing_out* o, void* stream) {
    ARG(r && l && o && (n_nodes == 0 || d_nodes), "null argument");
    ARG(n_nodes < (1ull << 32), "too many nodes listed");
    rf_ctx* ctx = r->ctx;
    ARG(live_ctx(l) == ctx, "the liveset belongs to another context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    MissIn in;
    in.l = l;
    in.d_nodes = static_cast<const uint32_t*>(d_nodes);
    in.n_groups = n_nodes;
    return repo_missing_device(r, in, o, false, pick(ctx, stream));
}

// ---- scan / collect_list / compact -------------------------------------------------
// the arrays of a pass over the table's tiles
static int repo_tile_bufs(rf_repo* r) {
    const uint64_t tiles = r->slots / kRepoListTile;
    HIPC(r->b_itiles.ensure(4 * tiles));
    HIPC(r->b_ioff.ensure(8 * (tiles + 1)));
    HIPC(r->b_tile_sums.ensure(8 * ((tiles + kRepoListTile - 1) / kRepoListTile + 1)));
    HIPC(r->b_total.ensure(16));
    return RF_OK;
}

// the first w rows of the host form's staging to the caller's arrays
static int repo_rows_to_host(rf_repo* r, uint64_t w, uint8_t* ids32, int64_t* sizes, hipStream_t s) {
    if (w && ids32) HIPC(hipMemcpyAsync(ids32, r->b_lids.p, 32 * w, hipMemcpyDeviceToHost, s));
    if (w && sizes) HIPC(hipMemcpyAsync(sizes, r->b_lsizes.p, 8 * w, hipMemcpyDeviceToHost, s));
    return RF_OK;
}
static int repo_stage_rows(rf_repo* r, uint64_t w, bool ids, bool sizes) {
    if (w && ids) HIPC(r->b_lids.ensure(32 * w));
    if (w && sizes) HIPC(r->b_lsizes.ensure(8 * w));
    return RF_OK;
}

// (context mutex held, device set, quiesced) the live objects counted, then the first min(n, cap) of them staged
static int repo_scan_locked(rf_repo* r, uint64_t cap, bool ids, bool sizes, uint64_t* n, hipStream_t s) {
    if (int rc = repo_tile_bufs(r)) return rc;
    HIPC(launch_repo_index_count(r->view(), r->slots, r->b_itiles.as<uint32_t>(), r->b_tile_sums.as<uint64_t>(),
                                 r->b_ioff.as<uint64_t>(), r->b_total.as<uint64_t>(), s));
    if (int rc = repo_read_total(r, n, s)) return rc;
    const uint64_t w = std::min(*n, cap);
    if (int rc = repo_stage_rows(r, w, ids, sizes)) return rc;
    HIPC(launch_repo_index_scatter(r->view(), r->slots, r->b_ioff.as<uint64_t>(), w,
                                   ids ? r->b_lids.as<uint8_t>() : nullptr, sizes ? r->b_lsizes.as<int64_t>() : nullptr,
                                   s));
    return RF_OK;
}

extern "C" int rf_repo_scan(rf_repo* r, uint64_t cap, uint8_t* ids32, int64_t* sizes, uint64_t* n) {
    ARG(r && n, "null argument");
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = ctx->stream;
    if (int rc = repo_scan_locked(r, cap, ids32 != nullptr, sizes != nullptr, n, s)) return rc;
    if (int rc = repo_rows_to_host(r, std::min(*n, cap), ids32, sizes, s)) return rc;
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, s)) return rc;
    if (*n > cap) return fail(RF_EINVAL, "list buffers too small: need %llu entries", (unsigned long long)*n);
    return RF_OK;
}

extern "C" int rf_repo_scan_device(rf_repo* r, uint64_t cap, void* d_ids32, void* d_sizes, void* d_n, void* stream) {
    ARG(r && d_n, "null argument");
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = pick(ctx, stream);
    if (int rc = repo_tile_bufs(r)) return rc;
    hipError_t e = launch_repo_index_count(r->view(), r->slots, r->b_itiles.as<uint32_t>(),
                                           r->b_tile_sums.as<uint64_t>(), r->b_ioff.as<uint64_t>(),
                                           static_cast<uint64_t*>(d_n), s);
    if (e == hipSuccess)
        e = launch_repo_index_scatter(r->view(), r->slots, r->b_ioff.as<uint64_t>(), cap,
                                      static_cast<uint8_t*>(d_ids32), static_cast<int64_t*>(d_sizes), s);
    const int rc = repo_mark_reader(r, s);  // (whatever was queued reads the table and the scratch)
    if (e != hipSuccess) return fail(RF_EDEVICE, "repo scan: %s", hipGetErrorString(e));
    return rc;
}

extern "C" int rf_repo_collect_list(rf_repo* r, rf_bloom* live, uint64_t cap, uint8_t* ids32, int64_t* sizes,
                                    uint64_t* removed, int64_t* removed_bytes) {
    ARG(r, "null argument");
    if (!ids32 && !sizes) return rf_repo_collect(r, live, removed, removed_bytes, nullptr);
    rf_ctx* ctx = r->ctx;
    ARG(!live || bloom_ctx(live) == ctx, "the filter belongs to another context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = ctx->stream;
    if (int rc = repo_tile_bufs(r)) return rc;
    HIPC(r->b_dead.ensure(r->slots));
    HIPC(launch_repo_collect_mark(r->view(), r->slots, live ? &bloom_dev(live) : nullptr, r->b_dead.as<uint8_t>(),
                                  r->b_itiles.as<uint32_t>(), r->b_tile_sums.as<uint64_t>(), r->b_ioff.as<uint64_t>(),
                                  r->b_total.as<uint64_t>(), s));
    uint64_t dead = 0;
    if (int rc = repo_read_total(r, &dead, s)) return rc;
    if (removed) *removed = dead;
    if (removed_bytes) *removed_bytes = 0;
    if (dead > cap)  // all or nothing: the names of what leaves the index are never lost
        return fail(RF_EINVAL, "list buffers too small: need %llu entries (nothing was removed)",
                    (unsigned long long)dead);
    if (int rc = repo_stage_rows(r, dead, ids32 != nullptr, sizes != nullptr)) return rc;
    HIPC(launch_repo_collect_apply(r->view(), r->slots, r->b_dead.as<uint8_t>(), r->b_ioff.as<uint64_t>(),
                                   r->b_total.as<uint64_t>(), dead, ids32 ? r->b_lids.as<uint8_t>() : nullptr,
                                   sizes ? r->b_lsizes.as<int64_t>() : nullptr, s));
    if (int rc = repo_rows_to_host(r, dead, ids32, sizes, s)) return rc;
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, s)) return rc;
    if (removed_bytes) *removed_bytes = (int64_t)c[kRepoGoneBytes];
    return RF_OK;
}

extern "C" int rf_repo_collect_list_device(rf_repo* r, rf_bloom* live, uint64_t cap, void* d_ids32, void* d_sizes,
                                           void* d_removed, void* d_removed_bytes, void* stream) {
    ARG(r && d_removed, "null argument");
    rf_ctx* ctx = r->ctx;
    ARG(!live || bloom_ctx(live) == ctx, "the filter belongs to another context");
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = pick(ctx, stream);
    const BloomDev* bd = live ? &bloom_dev(live) : nullptr;
    uint64_t* ctr = r->ctr.as<uint64_t>();
    if (!d_ids32 && !d_sizes) {  // a plain collect
        HIPC(launch_repo_collect(r->view(), r->slots, bd, s));
        HIPC(hipMemcpyAsync(d_removed, ctr + kRepoGone, 8, hipMemcpyDeviceToDevice, s));
    } else {
        if (int rc = repo_tile_bufs(r)) return rc;
        HIPC(r->b_dead.ensure(r->slots));
        HIPC(launch_repo_collect_mark(r->view(), r->slots, bd, r->b_dead.as<uint8_t>(), r->b_itiles.as<uint32_t>(),
                                      r->b_tile_sums.as<uint64_t>(), r->b_ioff.as<uint64_t>(),
                                      static_cast<uint64_t*>(d_removed), s));
        HIPC(launch_repo_collect_apply(r->view(), r->slots, r->b_dead.as<uint8_t>(), r->b_ioff.as<uint64_t>(),
                                       static_cast<const uint64_t*>(d_removed), cap, static_cast<uint8_t*>(d_ids32),
                                       static_cast<int64_t*>(d_sizes), s));
    }
    if (d_removed_bytes) HIPC(hipMemcpyAsync(d_removed_bytes, ctr + kRepoGoneBytes, 8, hipMemcpyDeviceToDevice, s));
    uint64_t c[kRepoCtrWords];
    return repo_read_ctr(r, c, s);
}

extern "C" int rf_repo_compact(rf_repo* r, uint64_t min_capacity) {
    ARG(r, "null argument");
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = ctx->stream;
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, s)) return rc;
    uint64_t slots = 0;
    char msg[160];
    if (!repo_slots_for(std::max<uint64_t>(c[kRepoObjects], min_capacity), &slots, msg, sizeof msg))
        return fail(RF_EINVAL, "repo compact: %s", msg);
    if (int rc = repo_rebuild(r, slots, s)) return rc;
    return repo_read_ctr(r, c, s);
}

// ---- save / restore ----------------------------------------------------------------
namespace {
struct CFile {
    FILE* f = nullptr;
    ~CFile() {
        if (f) fclose(f);
    }
};
}  // namespace

extern "C" int rf_repo_save(rf_repo* r, const char* path) {
    ARG(r && path && *path, "null argument");
    rf_ctx* ctx = r->ctx;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    if (int rc = repo_quiesce(r)) return rc;
    hipStream_t s = ctx->stream;
    uint64_t n = 0;
    if (int rc = repo_scan_locked(r, ~0ull, true, true, &n, s)) return rc;
    std::vector<uint8_t> ids(32 * n);
    std::vector<int64_t> sizes(n);
    if (int rc = repo_rows_to_host(r, n, ids.data(), sizes.data(), s)) return rc;
    uint64_t c[kRepoCtrWords];
    if (int rc = repo_read_ctr(r, c, s)) return rc;
    // slot order -> ID order: the file does not depend on the table's history
    HostPool* pool = ctx_pool(ctx);
    std::vector<uint32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    pool_sort(pool, perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) {
        return memcmp(ids.data() + 32ull * x, ids.data() + 32ull * y, 32) < 0;
    });
    std::vector<uint8_t> file(repo_file_bytes(n, kRepoFileChunk));
    if (int rc = repo_file_write(ids.data(), sizes.data(), perm.data(), n, kRepoFileChunk, file.data(),
                                 [&](const uint8_t* b, uint64_t len, uint64_t chunk, uint8_t* out) {
                                     hash_chunks(pool, b, len, chunk, out);
                                 }))
        return rc;
    // a reader never sees a partial file: written beside it, then renamed (rf_assoc_save)
    const std::string tmp = std::string(path) + ".tmp";
    CFile out;
    if (!(out.f = fopen(tmp.c_str(), "wb"))) return fail(RF_EIO, "repo save: cannot create %s", tmp.c_str());
    if (fwrite(file.data(), 1, file.size(), out.f) != file.size()) return fail(RF_EIO, "repo save: write failed");
    if (fflush(out.f) != 0 || fsync(fileno(out.f)) != 0) return fail(RF_EIO, "repo save: flush failed");
    fclose(out.f);
    out.f = nullptr;
    if (rename(tmp.c_str(), path) != 0) return fail(RF_EIO, "repo save: cannot rename to %s", path);
    return RF_OK;
}

extern "C" int rf_repo_restore(rf_ctx* ctx, const char* path, rf_repo** out) {
    ARG(ctx && path && out, "null argument");
    std::vector<uint8_t> file;
    {
        CFile in;
        if (!(in.f = fopen(path, "rb"))) return fail(RF_EIO, "repo restore: cannot open %s", path);
        struct stat st;
        if (fstat(fileno(in.f), &st) != 0 || st.st_size < 0) return fail(RF_EIO, "repo restore: cannot stat %s", path);
        // the largest valid file: 2^30 entries and their checksums
        if ((uint64_t)st.st_size > repo_file_bytes(kRepoFileMaxEntries, 64))
            return fail(RF_EINVAL, "repo restore: %s is too large for a repository index file", path);
        file.resize((size_t)st.st_size);
        if (!file.empty() && fread(file.data(), 1, file.size(), in.f) != file.size())
            return fail(RF_EIO, "repo restore: cannot read %s", path);
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    DevGuard dg(ctx->device);
    // everything is checked on the host before any of it reaches a kernel
    HostPool* pool = ctx_pool(ctx);
    uint64_t n = 0, slots = 0;
    int64_t total = 0;
    if (int rc = repo_file_check(file.data(), file.size(), &n, &total,
                                 [&](const uint8_t* b, uint64_t len, uint64_t chunk, uint8_t* o) {
                                     hash_chunks(pool, b, len, chunk, o);
                                 }))
        return rc;
    char msg[160];
    if (!repo_slots_for(n, &slots, msg, sizeof msg)) return fail(RF_EINVAL, "repo restore: %s", msg);
    std::vector<uint8_t> ids(32 * n);
    std::vector<int64_t> sizes(n);
    repo_file_unpack(file.data(), n, ids.data(), sizes.data());
    auto* r = new rf_repo();
    std::unique_ptr<rf_repo, void (*)(rf_repo*)> guard(r, repo_free);
    r->ctx = ctx;
    r->device = ctx->device;
    r->slots = slots;
    hipStream_t s = ctx->stream;
    hipError_t e = repo_alloc_table(r->tag, r->keys, r->size, slots, s);
    if (e == hipSuccess) e = r->ctr.ensure(8 * kRepoCtrWords);
    if (e == hipSuccess && n) e = r->b_ids.ensure(32 * n);
    if (e == hipSuccess && n) e = r->b_sizes.ensure(8 * n);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? RF_ENOMEM : RF_EDEVICE, "repo alloc: %s", hipGetErrorString(e));
    HIPC(hipEventCreateWithFlags(&r->e_reader, hipEventDisableTiming));
    uint64_t c[kRepoCtrWords] = {};
    c[kRepoObjects] = n;
    c[kRepoBytes] = (uint64_t)total;
    HIPC(hipMemcpyAsync(r->ctr.p, c, sizeof c, hipMemcpyHostToDevice, s));
    if (n) {
        HIPC(hipMemcpyAsync(r->b_ids.p, ids.data(), 32 * n, hipMemcpyHostToDevice, s));
        HIPC(hipMemcpyAsync(r->b_sizes.p, sizes.data(), 8 * n, hipMemcpyHostToDevice, s));
        HIPC(launch_repo_load(r->b_ids.as<uint8_t>(), r->b_sizes.as<int64_t>(), n, r->view(), slots, s));
    }
    if (int rc = repo_read_ctr(r, c, s)) return rc;  // (synchronises: the host arrays are done with)
    guard.release();
    *out = r;
    return RF_OK;
}
