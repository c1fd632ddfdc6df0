// marshal_flat.cpp -- host-only (no HIP, g++): Fileset values flattened into a
// piece stream (marshal_flat.h) for the device marshal of CacheWrite's values
// (eval.go:1141, 1961-1967), and the stream's plain C++ executor over
// json_emit.h -- the same per-piece source the kernels of k11_cwrite.hip run,
// here under the host compiler and its sanitizers (tests/cpp/marshal_flat_test.cpp).
// Host work is O(fileset nodes + entries) plus the sort of the Maps that are
// not in order already.
#include <string.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <unordered_map>

#include "errors.h"
#include "host_par.h"
#include "json_emit.h"
#include "marshal_flat.h"

namespace rf {
namespace {

// host_par.h's pool interface over threads that live for one run()
struct SpawnPool {
    unsigned n;
    unsigned size() const { return n; }
    template <class F>
    void run(F fn) {
        std::vector<std::thread> th;
        for (unsigned i = 1; i < n; ++i) th.emplace_back([&fn, i] { fn(i); });
        fn(0);
        for (std::thread& x : th) x.join();
    }
};

constexpr uint64_t kSortPar = 1 << 15;  // entries below which the sort stays on the caller

struct Group {
    uint64_t first;  // piece index of the Map's first entry
    uint64_t count;
    uint32_t node;
};

struct Flattener {
    const rf_fileset_tree* t;
    bool host_ids;
    FlatPieces* f;
    uint32_t val = 0;
    uint64_t n_entries = 0;
    std::string pend;  // literal bytes not yet made a piece
    std::unordered_map<std::string, uint32_t> lits;
    std::vector<Group> unsorted;

    bool path_less(uint64_t x, uint64_t y) const {
        const size_t lx = t->path_lens[x], ly = t->path_lens[y];
        const size_t m = std::min(lx, ly);
        const int c = m ? memcmp(t->paths[x], t->paths[y], m) : 0;
        return c < 0 || (c == 0 && lx < ly);
    }

    int push(uint32_t a, uint32_t b) {
        if (f->a.size() >= 0x7fffffffull) return fail(RF_EINVAL, "fileset batch: more than 2^31 pieces");
        f->a.push_back(a);
        f->b.push_back(b);
        f->val.push_back(val);
        return RF_OK;
    }

    int flush() {
        if (pend.empty()) return RF_OK;
        auto it = lits.find(pend);
        if (it == lits.end()) {
            if (f->blob.size() + pend.size() >= 0x7fffffffull) return fail(RF_EINVAL, "fileset batch: literal blob too large");
            it = lits.emplace(pend, (uint32_t)f->blob.size()).first;
            f->blob += pend;
        }
        const int rc = push(it->second, (uint32_t)pend.size());
        pend.clear();
        return rc;
    }

    int node(uint32_t node, int depth) {
        if (node >= t->n_nodes)
            return fail(RF_EINVAL, "fileset node %u >= n_nodes %llu", node, (unsigned long long)t->n_nodes);
        if (depth > 4096) return fail(RF_EINVAL, "fileset tree deeper than 4096 (cycle?)");
        const uint64_t lb = t->list_ptr[node], le = t->list_ptr[node + 1];
        const uint64_t eb = t->entry_ptr[node], ee = t->entry_ptr[node + 1];
        if (lb > le || eb > ee) return fail(RF_EINVAL, "fileset node %u: CSR not monotone", node);
        if (ee > n_entries || le > t->list_ptr[t->n_nodes])
            return fail(RF_EINVAL, "fileset node %u: CSR beyond the tree's arrays", node);
        pend.push_back('{');
        if (le > lb) {
            pend += "\"List\":[";
            for (uint64_t c = lb; c < le; ++c) {
                if (c > lb) pend.push_back(',');
                if (int rc = this->node(t->list_child[c], depth + 1)) return rc;
            }
            pend.push_back(']');
        }
        if (ee > eb) {
            if (le > lb) pend.push_back(',');
            pend += "\"Fileset\":{";
            if (int rc = flush()) return rc;
            const uint64_t first = f->a.size();
            bool in_order = true;
            for (uint64_t e = eb; e < ee; ++e) {
                if (!t->paths[e] && t->path_lens[e]) return fail(RF_EINVAL, "fileset node %u: null path", node);
                if (host_ids && json::id_is_zero(t->ids32 + 32 * e))  // digest.Digest's zero text form is unpinned
                    return fail(RF_EINVAL, "fileset node %u: zero file ID has no pinned JSON form", node);
                if (e > eb && !path_less(e - 1, e)) in_order = false;
                if (int rc = push((uint32_t)e, kPieceEntry | (e > eb ? kPieceComma : 0u))) return rc;
            }
            if (in_order) {
                ++f->sorted_groups;
            } else {
                ++f->unsorted_groups;
                unsorted.push_back(Group{first, ee - eb, node});
            }
            pend.push_back('}');
        }
        pend.push_back('}');
        return RF_OK;
    }

    // the Maps that were not in order: sorted (the entry indices move, the comma
    // bits stay with their positions), then checked for equal neighbours
    int sort_groups(unsigned threads) {
        if (unsorted.empty()) return RF_OK;
        uint64_t total = 0;
        for (const Group& g : unsorted) total += g.count;
        unsigned width = threads ? threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
        if (total < kSortPar) width = 1;
        SpawnPool pool{width};
        auto less = [this](uint32_t x, uint32_t y) { return path_less(x, y); };
        uint32_t* a = f->a.data();
        std::vector<const Group*> small;
        for (const Group& g : unsorted) {
            if (width > 1 && g.count >= kSortPar)
                pool_sort(&pool, a + g.first, a + g.first + g.count, less);
            else
                small.push_back(&g);
        }
        std::atomic<uint64_t> next{0};
        auto work = [&](unsigned) {
            for (uint64_t i; (i = next.fetch_add(1)) < small.size();)
                std::sort(a + small[i]->first, a + small[i]->first + small[i]->count, less);
        };
        if (width > 1 && small.size() > 1)
            pool.run(work);
        else
            work(0);
        for (const Group& g : unsorted)
            for (uint64_t q = 1; q < g.count; ++q)
                if (!path_less(a[g.first + q - 1], a[g.first + q]))
                    return fail(RF_EINVAL, "fileset node %u: duplicate map key", g.node);
        return RF_OK;
    }
};

int check_tree(const rf_fileset_tree* t, bool host_ids, uint64_t* n_entries) {
    ARG(t && t->list_ptr && t->entry_ptr, "null fileset tree");
    const uint64_t nl = t->list_ptr[t->n_nodes], ne = t->entry_ptr[t->n_nodes];
    ARG(nl == 0 || t->list_child, "null list_child");
    ARG(ne == 0 || (t->paths && t->path_lens && t->sizes && (t->ids32 || !host_ids)), "null entry arrays");
    ARG(ne < 0xffffffffull, "fileset tree: too many entries");
    *n_entries = ne;
    return RF_OK;
}

}  // namespace

int fileset_flatten(const rf_fileset_tree* t, const uint32_t* roots, uint64_t n, bool host_ids, unsigned threads,
                    FlatPieces* out) {
    ARG(out && (n == 0 || roots), "null argument");
    ARG(n < 0xffffffffull, "too many values");
    Flattener fl{t, host_ids, out};
    if (int rc = check_tree(t, host_ids, &fl.n_entries)) return rc;
    *out = FlatPieces{};
    out->value_ptr.reserve(n + 1);
    out->value_ptr.push_back(0);
    for (uint64_t i = 0; i < n; ++i) {
        fl.val = (uint32_t)i;
        if (int rc = fl.node(roots[i], 0)) return rc;
        if (int rc = fl.flush()) return rc;
        out->value_ptr.push_back((uint32_t)out->a.size());
    }
    // a same-length equal neighbour among entries found "in order" is a
    // duplicate too: path_less is strict, so in_order already excludes it
    return fl.sort_groups(threads);
}

int fileset_flat_execute(const rf_fileset_tree* t, const FlatPieces& f, uint8_t* out, uint64_t cap, uint64_t* offs,
                         uint64_t* out_len) {
    ARG(out_len, "null out_len");
    const uint64_t n = f.value_ptr.empty() ? 0 : f.value_ptr.size() - 1;
    auto path = [&](uint32_t e) { return reinterpret_cast<const uint8_t*>(t->paths[e]); };
    uint64_t total = 0;
    for (uint64_t v = 0; v < n; ++v) {
        if (offs) offs[v] = total;
        for (uint32_t p = f.value_ptr[v]; p < f.value_ptr[v + 1]; ++p) {
            if (f.b[p] & kPieceEntry)
                total += json::entry_len(path(f.a[p]), t->path_lens[f.a[p]], t->sizes[f.a[p]]) + (f.b[p] & kPieceComma);
            else
                total += f.b[p];
        }
    }
    if (offs) offs[n] = total;
    *out_len = total;
    if (total > cap) return fail(RF_EINVAL, "output buffer too small: need %llu bytes", (unsigned long long)total);
    if (!total) return RF_OK;
    ARG(out, "null output buffer");
    uint8_t* o = out;
    for (size_t p = 0; p < f.a.size(); ++p) {
        if (f.b[p] & kPieceEntry) {
            const uint32_t e = f.a[p];
            o = json::emit_entry(o, path(e), t->path_lens[e], t->ids32 + 32 * (uint64_t)e, t->sizes[e],
                                 (f.b[p] & kPieceComma) != 0);
        } else {
            memcpy(o, f.blob.data() + f.a[p], f.b[p]);
            o += f.b[p];
        }
    }
    if ((uint64_t)(o - out) != total) return fail(RF_EDEVICE, "fileset marshal: the emit pass wrote another length");
    return RF_OK;
}

}  // namespace rf

extern "C" int rf_fileset_marshal_flat(const rf_fileset_tree* t, const uint32_t* roots, uint64_t n, uint8_t* out,
                                       uint64_t cap, uint64_t* offs, uint64_t* out_len) {
    rf::FlatPieces f;
    if (int rc = rf::fileset_flatten(t, roots, n, true, 0, &f)) return rc;
    return rf::fileset_flat_execute(t, f, out, cap, offs, out_len);
}
