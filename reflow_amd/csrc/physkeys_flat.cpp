// physkeys_flat.cpp -- host-only (no HIP, g++): the physical keys
// (Flow.PhysicalDigest, flow.go:764-792) computed on the host by the code the
// kernels of k13_physkeys.hip run (phys_emit.h): node lengths / scan / per-entry
// emit for the values' materials, then segment table / tiled gather / SHA-256
// (host_sha.cpp) for the keys.  rf_physkeys_flat is what the CPU tests and the
// GPU tests compare against; phys_graph_check and phys_tree_forest are the host
// steps of the device form too.
#include "physkeys_flat.h"

#include <string.h>

#include <algorithm>

#include "errors.h"
#include "host_sha.h"
#include "marshal_flat.h"
#include "plan_check.h"

namespace rf {

int phys_graph_check(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, const uint64_t* phys_row,
                     const uint64_t* suffix_ptr, const uint8_t* suffix) {
    ARG(n == 0 || (dep_ptr && phys_row && suffix_ptr), "null argument");
    char msg[160];
    if (!plan_check(n, dep_ptr, deps, nullptr, msg, sizeof msg)) return fail(RF_EINVAL, "physkeys: %s", msg);
    if (!n) return RF_OK;
    ARG(suffix_ptr[0] == 0, "physkeys: suffix_ptr[0] must be 0");
    for (uint64_t i = 0; i < n; ++i)
        if (suffix_ptr[i] > suffix_ptr[i + 1])
            return fail(RF_EINVAL, "physkeys: suffix_ptr not monotone at node %llu", (unsigned long long)i);
    ARG(suffix_ptr[n] == 0 || suffix, "physkeys: null suffix bytes");
    ARG(suffix_ptr[n] < kPhysSrcSuffix, "physkeys: suffix blob too large");
    std::vector<uint64_t> rows;
    for (uint64_t i = 0; i < n; ++i)
        if (phys_row[i] != RF_PHYS_NO_ROW) rows.push_back(phys_row[i]);
    std::sort(rows.begin(), rows.end());
    for (size_t i = 1; i < rows.size(); ++i)
        if (rows[i] == rows[i - 1])
            return fail(RF_EINVAL, "physkeys: row %llu is the phys_row of two nodes", (unsigned long long)rows[i]);
    return RF_OK;
}

int phys_tree_forest(const rf_fileset_tree* t, const uint32_t* roots, uint64_t n, PhysTreeForest* out) {
    FlatPieces f;
    if (int rc = fileset_flatten(t, roots, n, false, 0, &f)) return rc;
    *out = PhysTreeForest{};
    out->doc_node_ptr.assign(1, 0);
    out->entry_ptr.assign(1, 0);
    out->path_off.assign(1, 0);
    // The skeleton bytes of the piece stream say where nodes open and close: a
    // brace after a colon is a Map's, every other one a node's.
    std::vector<uint8_t> is_map;
    for (uint64_t v = 0; v < n; ++v) {
        uint32_t depth = 0;
        char prev = 0;
        for (uint32_t p = f.value_ptr[v]; p < f.value_ptr[v + 1]; ++p) {
            if (f.b[p] & kPieceEntry) {
                const uint32_t e = f.a[p];
                const uint32_t len = t->path_lens[e];
                out->id_row.push_back(e);
                if (len) out->paths.insert(out->paths.end(), t->paths[e], t->paths[e] + len);
                out->path_off.push_back(out->paths.size());
                prev = 0;
                continue;
            }
            for (uint32_t k = 0; k < f.b[p]; ++k) {
                const char c = f.blob[f.a[p] + k];
                if (c == '{') {
                    is_map.push_back(prev == ':');
                    depth += prev != ':';
                } else if (c == '}') {
                    if (is_map.empty()) return fail(RF_EDEVICE, "physkeys: piece stream with an unopened brace");
                    if (!is_map.back()) {
                        out->node_depth.push_back(--depth);
                        out->entry_ptr.push_back(out->id_row.size());
                    }
                    is_map.pop_back();
                }
                prev = c;
            }
        }
        if (!is_map.empty()) return fail(RF_EDEVICE, "physkeys: piece stream with an open brace");
        out->doc_node_ptr.push_back(out->node_depth.size());
    }
    return RF_OK;
}

namespace {

void sha256_host(const uint8_t* p, uint64_t len, uint8_t out32[32]) {
    uint32_t st[8];
    host_sha_init(st);
    const uint64_t nb = len / 64, tail = len - 64 * nb;
    host_sha_blocks(st, p, nb);
    uint8_t buf[128] = {0};
    if (tail) memcpy(buf, p + 64 * nb, tail);
    buf[tail] = 0x80;
    const uint64_t fb = tail + 9 <= 64 ? 1 : 2, bits = len * 8;
    for (int i = 0; i < 8; ++i) buf[64 * fb - 1 - i] = (uint8_t)(bits >> (8 * i));
    host_sha_blocks(st, buf, fb);
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 4; ++b) out32[4 * i + b] = (uint8_t)(st[i] >> (24 - 8 * b));
}

}  // namespace
}  // namespace rf

using namespace rf;

extern "C" int rf_physkeys_flat(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, const uint64_t* phys_row,
                                const uint64_t* suffix_ptr, const uint8_t* suffix, const uint32_t* nodes,
                                uint64_t n_values, const rf_forest_arrays* fa, const rf_fileset_tree* tree,
                                const uint32_t* roots, uint8_t* keys32, uint64_t n_rows, uint8_t* materials,
                                uint64_t cap, uint64_t* mat_offs, uint64_t* out_len) {
    ARG(out_len, "null out_len");
    *out_len = 0;
    ARG(n_values == 0 || nodes, "null nodes");
    ARG((fa != nullptr) != (tree != nullptr) || n_values == 0, "physkeys: values as forest arrays or as a tree");
    ARG(n_values < 0xffffffffull, "too many values");
    if (int rc = phys_graph_check(n, dep_ptr, deps, phys_row, suffix_ptr, suffix)) return rc;
    for (uint64_t i = 0; i < n; ++i)
        if (phys_row[i] != RF_PHYS_NO_ROW && phys_row[i] >= n_rows)
            return fail(RF_EINVAL, "physkeys: node %llu: phys_row %llu >= n_rows %llu", (unsigned long long)i,
                        (unsigned long long)phys_row[i], (unsigned long long)n_rows);
    ARG(n_rows == 0 || keys32, "null keys32");

    PhysVals v;
    PhysTreeForest tf;
    v.n_docs = n_values;
    v.doc_node = nodes;
    const uint64_t zero_ptr[1] = {0};
    if (n_values == 0) {
        v.doc_node_ptr = v.entry_ptr = v.path_off = zero_ptr;
    } else if (fa) {
        ARG(fa->n_docs == n_values, "physkeys: one node per document");
        ARG(fa->doc_node_ptr && fa->entry_ptr && fa->path_off, "null forest arrays");
        v.n_nodes = fa->doc_node_ptr[n_values];
        ARG(v.n_nodes == 0 || fa->node_depth, "null node_depth");
        v.n_entries = fa->entry_ptr[v.n_nodes];
        ARG(v.n_entries == 0 || fa->ids32, "null ids32");
        ARG(fa->path_off[v.n_entries] == 0 || fa->paths, "null paths");
        v.doc_node_ptr = fa->doc_node_ptr;
        v.node_depth = fa->node_depth;
        v.entry_ptr = fa->entry_ptr;
        v.path_off = fa->path_off;
        v.paths = fa->paths;
        v.ids32 = fa->ids32;
    } else {
        if (int rc = phys_tree_forest(tree, roots, n_values, &tf)) return rc;
        v.n_nodes = tf.node_depth.size();
        v.n_entries = tf.id_row.size();
        ARG(v.n_entries == 0 || tree->ids32, "null ids32");
        v.doc_node_ptr = tf.doc_node_ptr.data();
        v.node_depth = tf.node_depth.data();
        v.entry_ptr = tf.entry_ptr.data();
        v.path_off = tf.path_off.data();
        v.paths = tf.paths.data();
        v.ids32 = tree->ids32;
        v.id_row = tf.id_row.data();
    }
    // the values: which document is each node's (the last that names it)
    std::vector<int64_t> val_doc(n, -1);
    for (uint64_t d = 0; d < n_values; ++d) {
        if (nodes[d] == kPhysSkip) continue;
        if (nodes[d] >= n) return fail(RF_EINVAL, "physkeys: value %llu: node %u out of range", (unsigned long long)d, nodes[d]);
        if (v.doc_node_ptr[d] == v.doc_node_ptr[d + 1])
            return fail(RF_EINVAL, "physkeys: value %llu of node %u is a refused document", (unsigned long long)d, nodes[d]);
        val_doc[nodes[d]] = (int64_t)d;
    }
    // pass 1: node lengths, their scan, the documents' lengths and offsets
    std::vector<uint64_t> node_pre(v.n_nodes + 1, 0), doc_off(n_values + 1, 0);
    for (uint64_t j = 0; j < v.n_nodes; ++j) node_pre[j + 1] = node_pre[j] + phys_node_len(v, j);
    for (uint64_t d = 0; d < n_values; ++d)
        doc_off[d + 1] = doc_off[d] + (node_pre[v.doc_node_ptr[d + 1]] - node_pre[v.doc_node_ptr[d]]);
    const uint64_t total = doc_off[n_values];
    *out_len = total;
    if (mat_offs) memcpy(mat_offs, doc_off.data(), 8 * (n_values + 1));
    if (total > cap) return fail(RF_EINVAL, "output buffer too small: need %llu bytes", (unsigned long long)total);
    ARG(total == 0 || materials, "null materials");
    // pass 2: the emit, entry by entry
    for (uint64_t e = 0; e < v.n_entries; ++e) {
        uint64_t dst;
        if (!phys_entry_dst(v, node_pre.data(), doc_off.data(), e, &dst)) continue;
        const uint64_t len = phys_entry_len(v, e);
        if (dst + len > total) return fail(RF_EDEVICE, "physkeys: an entry lands outside its value");
        for (uint64_t k = 0; k < len; ++k) materials[dst + k] = phys_entry_byte(v, e, k);
    }
    // passes 3-4: every node that has a row is affected; the segment table
    std::vector<uint64_t> aff, seg_dst, seg_src, seg_len, m_off, m_len;
    for (uint64_t i = 0; i < n; ++i) {
        if (phys_row[i] == RF_PHYS_NO_ROW) continue;
        bool computable = true;
        for (uint64_t e = dep_ptr[i]; e < dep_ptr[i + 1]; ++e) computable = computable && val_doc[deps[e]] >= 0;
        if (!computable) {
            memset(keys32 + 32 * phys_row[i], 0, 32);
            continue;
        }
        uint64_t pos = m_off.empty() ? 0 : phys_align16(m_off.back() + m_len.back());
        m_off.push_back(pos);
        for (uint64_t e = dep_ptr[i]; e <= dep_ptr[i + 1]; ++e) {
            seg_dst.push_back(pos);
            if (e < dep_ptr[i + 1]) {
                const uint64_t d = (uint64_t)val_doc[deps[e]];
                seg_src.push_back(doc_off[d]);
                seg_len.push_back(doc_off[d + 1] - doc_off[d]);
            } else {
                seg_src.push_back(kPhysSrcSuffix | suffix_ptr[i]);
                seg_len.push_back(suffix_ptr[i + 1] - suffix_ptr[i]);
            }
            pos += seg_len.back();
        }
        m_len.push_back(pos - m_off.back());
        aff.push_back(i);
    }
    if (aff.empty()) return RF_OK;
    // pass 5: the gather, tile by tile, sixteen bytes a lane
    const uint64_t out_bytes = phys_align16(m_off.back() + m_len.back());
    std::vector<uint8_t> out(out_bytes);
    PhysSegs g{seg_dst.size(), seg_dst.data(), seg_src.data(), seg_len.data()};
    for (uint64_t t0 = 0; t0 < out_bytes; t0 += RF_PHYS_COPY_TILE) {
        const uint64_t t1 = std::min<uint64_t>(t0 + RF_PHYS_COPY_TILE, out_bytes);
        const uint64_t lo = phys_upper_index(g.dst, 0, g.n, t0), hi = phys_upper_index(g.dst, 0, g.n, t1 - 1) + 1;
        for (uint64_t b = t0; b < t1; b += 16) {
            uint32_t w[4];
            phys_gather_run(g, lo, hi, b, materials, suffix, w);
            for (int i = 0; i < 16; ++i) out[b + i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
        }
    }
    // pass 6: the digests to their rows
    for (size_t k = 0; k < aff.size(); ++k) sha256_host(out.data() + m_off[k], m_len[k], keys32 + 32 * phys_row[aff[k]]);
    return RF_OK;
}
