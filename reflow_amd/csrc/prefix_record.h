// prefix_record.h -- the checkpointed prefix hand-over's record, shared by the
// duo kernel that writes it (k1_sha.hip) and the host leg that reads it
// (host_leg.cpp); DESIGN.md §5 "Checkpointed hand-over".  It lives in coherent
// pinned host memory.  Internal header, no HIP.
#pragma once
#include <stdint.h>

namespace rf {

// The chaining value after `blocks` whole blocks (eight words, host order).
struct PrefixSlot {
    uint32_t state[8];
    uint64_t blocks;
    uint64_t pad;
};

// Record k (k = 1, 2, ...) of a file goes to slot[k & 1] and then latest = k,
// so while the wave writes record k + 1 the reader's slot stays as it is.
// latest == 0: nothing published.
struct PrefixRecord {
    PrefixSlot slot[2];
    uint32_t latest;
    uint32_t pad[3];
};
static_assert(sizeof(PrefixSlot) == 48 && sizeof(PrefixRecord) == 112, "16-byte stores need this layout");

// A reader takes latest (before), copies slot[before & 1], takes latest again
// (after).  The wave's next write goes to the other slot, so the copy is
// intact if latest moved by at most one; else the reader tries again from
// `after`.
inline bool prefix_copy_intact(uint32_t before, uint32_t after) { return after - before <= 1u; }

}  // namespace rf
