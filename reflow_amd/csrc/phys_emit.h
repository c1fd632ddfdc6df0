// phys_emit.h -- internal: the per-node, per-entry and per-segment code of the
// physical keys (Flow.PhysicalDigest, flow.go:764-792), shared by the kernels
// (k13_physkeys.hip) and the host-only form (physkeys_flat.cpp) so that CPU
// tests run what the device runs.  No HIP types; __host__ __device__ under hipcc.
//
// A batch of Fileset values is a FOREST (unmarshal_flat.h): per document its
// nodes in closing order with depths, one CSR of entries over the nodes, the
// entries in document order.  A value's material (Fileset.WriteDigest,
// executor.go:214-233) is `path ‖ 00 05 ‖ ID` over the Map entries of the
// nodes that have no List children, in document order: "List wins", and the
// closing order puts a node's List before its Map.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RF_PHYS_HD __host__ __device__
#else
#define RF_PHYS_HD
#endif

namespace rf {

constexpr uint64_t kPhysIdBytes = 34;                  // 00 05 ‖ ID (digest.WriteDigest)
constexpr uint32_t kPhysSkip = 0xffffffffu;            // a document without a graph node
constexpr uint64_t kPhysSrcSuffix = 1ull << 63;        // a segment's source: the suffix blob, not the arena

// The values of one call, host or device memory alike.
struct PhysVals {
    uint64_t n_docs = 0, n_nodes = 0, n_entries = 0;
    const uint32_t* doc_node = nullptr;      // [n_docs] the graph node of document d, kPhysSkip: none
    const uint64_t* doc_node_ptr = nullptr;  // [n_docs + 1]
    const uint32_t* node_depth = nullptr;    // [n_nodes]
    const uint64_t* entry_ptr = nullptr;     // [n_nodes + 1]
    const uint64_t* path_off = nullptr;      // [n_entries + 1]
    const uint8_t* paths = nullptr;          // decoded
    const uint8_t* ids32 = nullptr;          // rows of 32 bytes
    const uint32_t* id_row = nullptr;        // [n_entries] entry e's ID is row id_row[e]; null: row e
};

RF_PHYS_HD inline uint64_t phys_align16(uint64_t x) { return (x + 15) & ~15ull; }

// The last i in [lo, hi) with a[i] <= x.  a ascends over [lo, hi), a[lo] <= x.
RF_PHYS_HD inline uint64_t phys_upper_index(const uint64_t* a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// Node j of the document whose first node is j0 has List children: in closing
// order the node closed just before a parent is its last child.
RF_PHYS_HD inline bool phys_has_children(const uint32_t* node_depth, uint64_t j, uint64_t j0) {
    return j > j0 && node_depth[j - 1] == node_depth[j] + 1;
}

// The document of node j (documents without nodes are stepped over).
RF_PHYS_HD inline uint64_t phys_doc_of(const PhysVals& v, uint64_t j) {
    return phys_upper_index(v.doc_node_ptr, 0, v.n_docs, j);
}

// Material bytes node j contributes: its Map's, or none when the document is
// skipped or the node has children.
RF_PHYS_HD inline uint64_t phys_node_len(const PhysVals& v, uint64_t j) {
    const uint64_t d = phys_doc_of(v, j);
    if (v.doc_node[d] == kPhysSkip || phys_has_children(v.node_depth, j, v.doc_node_ptr[d])) return 0;
    const uint64_t e0 = v.entry_ptr[j], e1 = v.entry_ptr[j + 1];
    return v.path_off[e1] - v.path_off[e0] + kPhysIdBytes * (e1 - e0);
}

// Where entry e's bytes go: false when it contributes nothing.  node_pre [n_nodes]
// = material bytes before node j over the whole call, doc_off [n_docs] = the
// document's offset in the output.
RF_PHYS_HD inline bool phys_entry_dst(const PhysVals& v, const uint64_t* node_pre, const uint64_t* doc_off, uint64_t e,
                                      uint64_t* dst) {
    const uint64_t j = phys_upper_index(v.entry_ptr, 0, v.n_nodes, e);
    const uint64_t d = phys_doc_of(v, j), j0 = v.doc_node_ptr[d];
    if (v.doc_node[d] == kPhysSkip || phys_has_children(v.node_depth, j, j0)) return false;
    const uint64_t e0 = v.entry_ptr[j];
    *dst = doc_off[d] + (node_pre[j] - node_pre[j0]) + (v.path_off[e] - v.path_off[e0]) + kPhysIdBytes * (e - e0);
    return true;
}

RF_PHYS_HD inline uint64_t phys_entry_len(const PhysVals& v, uint64_t e) {
    return v.path_off[e + 1] - v.path_off[e] + kPhysIdBytes;
}

// Byte k of entry e's material.
RF_PHYS_HD inline uint8_t phys_entry_byte(const PhysVals& v, uint64_t e, uint64_t k) {
    const uint64_t p0 = v.path_off[e], plen = v.path_off[e + 1] - p0;
    if (k < plen) return v.paths[p0 + k];
    if (k == plen) return 0;
    if (k == plen + 1) return 5;
    return v.ids32[32 * (uint64_t)(v.id_row ? v.id_row[e] : e) + (k - plen - 2)];
}

// The gather's segment table: segment s copies seg_len[s] bytes to seg_dst[s]
// from the value arena at seg_src[s], or from the suffix blob when
// kPhysSrcSuffix is set.  seg_dst ascends; empty segments share their
// successor's.  Output byte b belongs to the last segment that starts at or
// before it, and is a zero pad byte when that segment ends before it.
struct PhysSegs {
    uint64_t n = 0;
    const uint64_t *dst = nullptr, *src = nullptr, *len = nullptr;
};

RF_PHYS_HD inline uint8_t phys_seg_byte(const PhysSegs& g, uint64_t s, uint64_t b, const uint8_t* arena,
                                        const uint8_t* suffix) {
    const uint64_t k = b - g.dst[s];
    if (k >= g.len[s]) return 0;
    const uint64_t src = g.src[s];
    return (src & kPhysSrcSuffix) ? suffix[(src & ~kPhysSrcSuffix) + k] : arena[src + k];
}

// The sixteen output bytes from b0 on as four little-endian words (one 16-byte
// store), the segment of b0 looked for in [lo, hi).
RF_PHYS_HD inline void phys_gather_run(const PhysSegs& g, uint64_t lo, uint64_t hi, uint64_t b0,
                                       const uint8_t* arena, const uint8_t* suffix, uint32_t w[4]) {
    uint64_t s = phys_upper_index(g.dst, lo, hi, b0);
    w[0] = w[1] = w[2] = w[3] = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t b = b0 + i;
        while (s + 1 < g.n && g.dst[s + 1] <= b) ++s;
        w[i >> 2] |= (uint32_t)phys_seg_byte(g, s, b, arena, suffix) << (8 * (i & 3));
    }
}

}  // namespace rf
