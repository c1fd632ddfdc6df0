// plan_check.h -- internal, HIP-free: the structural checks of an evaluation
// plan's node graph (rf_eval_plan_check, rf_eval_plan_open).  Not part of the
// public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rf {

// Node i's Deps are deps[dep_ptr[i] .. dep_ptr[i+1]) (a dep may be listed
// twice).  Checks dep_ptr[0] == 0, monotone pointers, deps < n and that the
// graph has no cycle; *depth = the nodes on the longest path (0 for n == 0).
// Returns true, or false with a message in err (at most err_cap bytes,
// NUL-terminated; err may be null).
bool plan_check(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, uint32_t* depth, char* err,
                size_t err_cap);

}  // namespace rf
