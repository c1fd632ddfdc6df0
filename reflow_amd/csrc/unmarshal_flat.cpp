// unmarshal_flat.cpp -- host-only (no HIP, g++): the batched unmarshal of
// Fileset JSON on host threads, document by document through json_parse.h's
// sequential form -- the subject of the CPU tests and of
// tests/cpp/json_parse_test.cpp under the sanitizers, and the probe's host
// baseline; not a product path.  With RF_UNMARSHAL_CHECK_TILED every document
// also goes through the per-byte form the kernels of k12_unmarshal.hip run, and
// a verdict or a count that differs fails the call.  Also the forest's
// host-side accessors and the List CSR helper.
#include <string.h>

#include <atomic>
#include <thread>

#include "errors.h"
#include "json_parse.h"
#include "unmarshal_flat.h"

namespace rf {
namespace {

struct CountSink {
    uint32_t nodes = 0, entries = 0;
    uint64_t path_bytes = 0;
    void entry(uint32_t, uint32_t, uint32_t dec, const uint8_t*, int64_t) {
        ++entries;
        path_bytes += dec;
    }
    void node(uint32_t) { ++nodes; }
};

struct WriteSink {
    const uint8_t* s;
    HostForest* f;
    uint64_t n_at, e_at, p_at;  // the next node, entry and path byte
    void entry(uint32_t pb, uint32_t pe, uint32_t, const uint8_t* id, int64_t size) {
        uint8_t* end = json::path_decode(s, pb, pe, f->paths.data() + p_at);
        p_at = (uint64_t)(end - f->paths.data());
        memcpy(f->ids32.data() + 32 * e_at, id, 32);
        f->sizes[e_at] = size;
        f->path_off[++e_at] = p_at;
    }
    void node(uint32_t depth) {
        f->node_depth[n_at] = depth;
        f->entry_ptr[++n_at] = e_at;
    }
};

// the per-byte form over one document, as the kernels run it
uint32_t tiled_verdict(const uint8_t* s, uint32_t n, CountSink* c) {
    if (!n) return 1;
    std::vector<uint16_t> qm(n / 16 + 1, 0);
    for (uint32_t i = 0; i < n; ++i)
        if (s[i] == '"' && json::quote_is_delim(s, 0, i)) qm[i >> 4] |= (uint16_t)(1u << (i & 15));
    bool ok = true, pb = false;
    int32_t depth = 0;
    for (uint32_t i = 0; i < n; ++i) {
        json::ByteCounts o;
        ok &= json::tile_check_byte(s, qm.data(), 0, n, i, pb, &o);
        const bool q = json::qbit(qm.data(), i);
        if (!pb && !q) {
            ok &= json::tile_depth_byte(s, 0, n, i, depth);
            const int32_t d = json::depth_delta(s, 0, n, i);
            if (ok && d != o.ddepth) return 2;  // the two passes must see one delta
            depth += d;
        }
        c->nodes += o.nodes;
        c->entries += o.entries;
        c->path_bytes += o.path_bytes;
        pb ^= q;
    }
    return ok ? 0 : 1;
}

// Documents over threads that live for one call.  host_par.h's helpers take a
// pool object, which belongs to a context; this call has none (as
// marshal_flat.cpp, which brings its SpawnPool for the same reason), so this is
// a second small spreader to keep in step with that one.
template <class F>
void par_for(uint64_t n, unsigned threads, F fn) {
    unsigned width = threads ? threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (n < 2 * (uint64_t)width) width = 1;
    std::atomic<uint64_t> next{0};
    auto work = [&] {
        for (uint64_t lo; (lo = next.fetch_add(64)) < n;)
            for (uint64_t i = lo; i < std::min(n, lo + 64); ++i) fn(i);
    };
    std::vector<std::thread> th;
    for (unsigned i = 1; i < width; ++i) th.emplace_back(work);
    work();
    for (std::thread& t : th) t.join();
}

}  // namespace

int unmarshal_flat(const uint8_t* json, const uint64_t* offs, uint64_t n, uint32_t flags, unsigned threads,
                   HostForest* out) {
    ARG(out && (n == 0 || (json && offs)), "null argument");
    for (uint64_t d = 0; d < n; ++d) ARG(offs[d] <= offs[d + 1], "document offsets not ascending");
    HostForest& f = *out;
    f = HostForest{};
    f.n_docs = n;
    f.status.assign(n, RF_OK);
    f.reason.assign(n, 0);
    f.node_cnt.assign(n, 0);
    f.entry_cnt.assign(n, 0);
    std::vector<uint64_t> pbytes(n, 0);
    std::atomic<uint64_t> disagree{~0ull};
    par_for(n, threads, [&](uint64_t d) {
        const uint64_t len = offs[d + 1] - offs[d];
        CountSink c;
        const uint32_t why =
            len >> 32 ? (uint32_t)json::kWhyLength : json::parse_document(json + offs[d], (uint32_t)len, c);
        if ((flags & RF_UNMARSHAL_CHECK_TILED) && !(len >> 32)) {
            CountSink t;
            const uint32_t bad = tiled_verdict(json + offs[d], (uint32_t)len, &t);
            if (bad == 2 || (bad != 0) != (why != 0) ||
                (!why && (t.nodes != c.nodes || t.entries != c.entries || t.path_bytes != c.path_bytes)))
                disagree = d;
        }
        f.reason[d] = why;
        if (why) {
            f.status[d] = RF_ENOTCANONICAL;
            return;
        }
        f.node_cnt[d] = c.nodes;
        f.entry_cnt[d] = c.entries;
        pbytes[d] = c.path_bytes;
    });
    if (disagree != ~0ull)
        return fail(RF_EDEVICE, "fileset unmarshal: the sequential and the per-byte form disagree on document %llu",
                    (unsigned long long)disagree.load());
    f.doc_node_ptr.assign(n + 1, 0);
    std::vector<uint64_t> ebase(n + 1, 0), pbase(n + 1, 0);
    for (uint64_t d = 0; d < n; ++d) {
        f.doc_node_ptr[d + 1] = f.doc_node_ptr[d] + f.node_cnt[d];
        ebase[d + 1] = ebase[d] + f.entry_cnt[d];
        pbase[d + 1] = pbase[d] + pbytes[d];
        f.n_accepted += f.status[d] == RF_OK;
    }
    f.n_nodes = f.doc_node_ptr[n];
    f.n_entries = ebase[n];
    f.path_bytes = pbase[n];
    f.node_depth.assign(f.n_nodes, 0);
    f.entry_ptr.assign(f.n_nodes + 1, 0);
    f.path_off.assign(f.n_entries + 1, 0);
    f.paths.assign(f.path_bytes + 1, 0);
    f.ids32.assign(32 * f.n_entries + 1, 0);
    f.sizes.assign(f.n_entries + 1, 0);
    par_for(n, threads, [&](uint64_t d) {
        if (f.status[d] != RF_OK) return;
        WriteSink w{json + offs[d], &f, f.doc_node_ptr[d], ebase[d], pbase[d]};
        (void)json::parse_document(json + offs[d], (uint32_t)(offs[d + 1] - offs[d]), w);
    });
    f.structure = true;
    return RF_OK;
}

}  // namespace rf

using rf::fail;

extern "C" int rf_fileset_unmarshal_flat(const uint8_t* json, const uint64_t* offs, uint64_t n, uint32_t flags,
                                         unsigned threads, rf_fileset_forest** out) {
    ARG(out, "null argument");
    auto* f = new rf_fileset_forest();
    if (int rc = rf::unmarshal_flat(json, offs, n, flags, threads, &f->h)) {
        delete f;
        return rc;
    }
    *out = f;
    return RF_OK;
}

extern "C" int rf_fileset_forest_info(const rf_fileset_forest* f, uint64_t* n_docs, uint64_t* n_accepted,
                                      uint64_t* n_nodes, uint64_t* n_entries, uint64_t* path_bytes) {
    ARG(f, "null forest");
    if (n_docs) *n_docs = f->h.n_docs;
    if (n_accepted) *n_accepted = f->h.n_accepted;
    if (n_nodes) *n_nodes = f->h.n_nodes;
    if (n_entries) *n_entries = f->h.n_entries;
    if (path_bytes) *path_bytes = f->h.path_bytes;
    return RF_OK;
}

extern "C" int rf_fileset_forest_status(const rf_fileset_forest* f, int32_t* status, uint32_t* reason,
                                        uint32_t* node_counts, uint32_t* entry_counts) {
    ARG(f, "null forest");
    const size_t n = f->h.n_docs;
    if (status && n) memcpy(status, f->h.status.data(), 4 * n);
    if (reason && n) memcpy(reason, f->h.reason.data(), 4 * n);
    if (node_counts && n) memcpy(node_counts, f->h.node_cnt.data(), 4 * n);
    if (entry_counts && n) memcpy(entry_counts, f->h.entry_cnt.data(), 4 * n);
    return RF_OK;
}

extern "C" int rf_fileset_forest_times(const rf_fileset_forest* f, double ms[3]) {
    ARG(f && ms, "null argument");
    for (int i = 0; i < 3; ++i) ms[i] = f->ms[i];
    return RF_OK;
}

// Nodes come in closing order with their depths: when a node of depth d closes,
// the nodes of depth d + 1 on top of the stack are its List, in order.
extern "C" int rf_fileset_forest_tree(const uint64_t* doc_node_ptr, uint64_t n_docs, const uint32_t* node_depth,
                                      uint64_t n_nodes, uint64_t* list_ptr, uint32_t* list_child, uint32_t* roots) {
    ARG((n_docs == 0 || (doc_node_ptr && roots)) && list_ptr && (n_nodes == 0 || (node_depth && list_child)),
        "null argument");
    ARG(n_nodes < 0xffffffffull, "too many nodes");
    ARG(n_docs == 0 || (doc_node_ptr[0] == 0 && doc_node_ptr[n_docs] == n_nodes), "document pointers do not span the nodes");
    std::vector<uint32_t> stack;
    uint64_t nc = 0;
    list_ptr[0] = 0;
    for (uint64_t d = 0; d < n_docs; ++d) {
        const uint64_t b = doc_node_ptr[d], e = doc_node_ptr[d + 1];
        ARG(b <= e && e <= n_nodes, "document pointers not monotone");
        roots[d] = b == e ? 0xffffffffu : (uint32_t)(e - 1);
        stack.clear();
        for (uint64_t p = b; p < e; ++p) {
            const uint32_t dep = node_depth[p];
            size_t k = stack.size();
            while (k > 0 && node_depth[stack[k - 1]] == dep + 1) --k;
            for (size_t j = k; j < stack.size(); ++j) list_child[nc++] = stack[j];
            stack.resize(k);
            list_ptr[p + 1] = nc;
            stack.push_back((uint32_t)p);
        }
        if (b != e && (stack.size() != 1 || node_depth[e - 1] != 0))
            return fail(RF_EINVAL, "document %llu: the depths are not those of one tree in closing order",
                        (unsigned long long)d);
    }
    return RF_OK;
}
