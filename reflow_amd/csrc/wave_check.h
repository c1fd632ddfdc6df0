// wave_check.h -- internal, HIP-free: the consumer CSR of an evaluation wave's
// node graph (rf_eval_wave_consumers).  Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rf {

// Inverts node i's Deps deps[dep_ptr[i] .. dep_ptr[i+1]): cons_ptr [n+1] and
// cons [dep_ptr[n]] list, for node d, the nodes that list d as a dep -- one
// entry per dep entry (a dep listed twice gives two), ascending within a node.
// False (and a message in err, truncated to err_cap) for a null pointer,
// dep_ptr[0] != 0, pointers that are not monotone or a dep out of range;
// nothing is written then.  Cycles are not looked for (plan_check does that).
bool wave_consumers(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, uint64_t* cons_ptr, uint32_t* cons,
                    char* err, size_t err_cap);

}  // namespace rf
