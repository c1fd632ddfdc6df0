// unmarshal_flat.h -- internal, HIP-free: what a batched unmarshal of Fileset
// JSON leaves on the host (the host form fills all of it, the device form the
// per-document part and, on rf_fileset_forest_copy, the rest), and the host
// form itself (unmarshal_flat.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "reflow_hip.h"

namespace rf {

// Nodes in closing order (post-order) per accepted document, so that the
// entries, which stand in document order, form one CSR over the nodes: the
// entries between two closing braces are the later node's Map.
struct HostForest {
    uint64_t n_docs = 0, n_accepted = 0, n_nodes = 0, n_entries = 0, path_bytes = 0;
    std::vector<int32_t> status;      // [n_docs] RF_OK / RF_ENOTCANONICAL
    std::vector<uint32_t> reason;     // [n_docs] RF_UNMARSHAL_WHY_*
    std::vector<uint32_t> node_cnt;   // [n_docs] 0 for a refused document
    std::vector<uint32_t> entry_cnt;  // [n_docs] likewise
    bool structure = false;           // the arrays below are filled
    std::vector<uint64_t> doc_node_ptr;  // [n_docs + 1]
    std::vector<uint32_t> node_depth;    // [n_nodes] a root is 0
    std::vector<uint64_t> entry_ptr;     // [n_nodes + 1]
    std::vector<uint64_t> path_off;      // [n_entries + 1]
    std::vector<uint8_t> paths;          // decoded
    std::vector<uint8_t> ids32;          // [n_entries][32]
    std::vector<int64_t> sizes;          // [n_entries]
};

// Document d = json[offs[d], offs[d + 1]).  threads 0: up to 16.  flags:
// RF_UNMARSHAL_CHECK_TILED.
int unmarshal_flat(const uint8_t* json, const uint64_t* offs, uint64_t n, uint32_t flags, unsigned threads,
                   HostForest* out);

}  // namespace rf

struct rf_fileset_forest {
    rf::HostForest h;
    void* dev = nullptr;  // unmarshal_dev.cpp's device side; null for a host-form forest
    void (*dev_free)(void*) = nullptr;
    double ms[3] = {0, 0, 0};
};
