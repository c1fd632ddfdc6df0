// plan_internal.h -- internal: what the evaluation plan (eval_plan.cpp) shares
// with dirty.cpp and with the liveset and assoc objects of capi.cpp.  Not part
// of the public ABI.
#pragma once
#include "ctx.h"
#include "engine.h"

namespace rf {

// dirty.cpp: Eval.dirty's closure, left on the device (see there).
int flow_dirty_bits(rf_ctx* ctx, uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, const uint8_t* is_extern,
                    uint8_t extern_mask, DevBuf& b_bits);

// capi.cpp: the objects behind rf_bloom* / rf_assoc*, as far as a fused
// lookup needs them (the view: context mutex held, and for as long as it is).
rf_ctx* bloom_ctx(rf_bloom* b);
const BloomDev& bloom_dev(rf_bloom* b);
rf_ctx* assoc_ctx(rf_assoc* a);
AssocView assoc_view(rf_assoc* a);

}  // namespace rf
