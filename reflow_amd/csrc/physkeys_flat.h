// physkeys_flat.h -- internal, HIP-free: the host side the physical keys'
// device form (physkeys_dev.cpp) and host-only form (physkeys_flat.cpp) share:
// the checks of rf_physkeys_open and a tree of Fileset values turned into the
// forest form phys_emit.h works on.  Not part of the public ABI.
#pragma once
#include <stdint.h>

#include <vector>

#include "phys_emit.h"
#include "reflow_hip.h"

namespace rf {

// rf_physkeys_open's refusals: rf_eval_plan_open's for the CSR (plan_check.cpp),
// suffix pointers that are not monotone, a phys_row used twice.
int phys_graph_check(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, const uint64_t* phys_row,
                     const uint64_t* suffix_ptr, const uint8_t* suffix);

// Values given as a tree (rf_fileset_tree + roots) in forest form: the nodes in
// closing order with depths, the entries in output order -- each Map bytewise
// ordered by marshal_flat.cpp's detection and sort -- with their paths copied
// and the tree's entry index kept (id_row), since the IDs stay where they are.
struct PhysTreeForest {
    std::vector<uint64_t> doc_node_ptr, entry_ptr, path_off;
    std::vector<uint32_t> node_depth, id_row;
    std::vector<uint8_t> paths;
};
// Refusals are fileset_flatten's, a zero ID excepted (material has no such rule).
int phys_tree_forest(const rf_fileset_tree* t, const uint32_t* roots, uint64_t n, PhysTreeForest* out);

}  // namespace rf
