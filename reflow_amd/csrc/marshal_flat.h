// marshal_flat.h -- internal: a batch of Fileset values flattened into a PIECE
// STREAM in output order (marshal_flat.cpp, host-only).  A literal piece is a
// run of skeleton bytes -- {"List":[  ,  ]  "Fileset":{  } -- held once in a
// small blob; an entry piece is one Map entry, with a bit for the comma it
// carries when it is not the first of its Map.  The stream is executed by the
// marshal kernels (k11_cwrite.hip) and by fileset_flat_execute below, both
// through json_emit.h.  No HIP.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "reflow_hip.h"

namespace rf {

constexpr uint32_t kPieceEntry = 0x80000000u;  // b: an entry piece (a = entry index); else a literal (a = blob offset, b = length)
constexpr uint32_t kPieceComma = 1u;           // b of an entry piece: not the first of its Map

struct FlatPieces {
    std::vector<uint32_t> a, b, val;  // per piece: two words and its value's index
    std::vector<uint32_t> value_ptr;  // [n + 1] value i's pieces are [value_ptr[i], value_ptr[i + 1])
    std::string blob;                 // the literals' bytes
    uint64_t sorted_groups = 0, unsorted_groups = 0;  // Maps found in order / sorted here
};

// Flattens roots[0 .. n) of t.  Refuses what rf_fileset_marshal_json refuses,
// with its status: a node out of range, a CSR that is not monotone, a depth
// above 4096, duplicate map keys and -- with host_ids, when t->ids32 holds the
// IDs -- a zero ID.  threads: the width of the sort (0: the machine's, at most 16).
int fileset_flatten(const rf_fileset_tree* t, const uint32_t* roots, uint64_t n, bool host_ids, unsigned threads,
                    FlatPieces* out);

// The stream executed on the host: value i's bytes at out + offs[i], offs[n] =
// the total.  *out_len is set either way; RF_EINVAL when cap is short (nothing
// is written then).
int fileset_flat_execute(const rf_fileset_tree* t, const FlatPieces& f, uint8_t* out, uint64_t cap, uint64_t* offs,
                         uint64_t* out_len);

}  // namespace rf
