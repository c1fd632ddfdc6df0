// wave_check.cpp -- HIP-free: the consumer CSR of an evaluation wave's node
// graph (wave_check.h).  A completion step walks from the nodes that finished
// to the nodes that wait for them, so the Deps of eval.go:915-920 are inverted
// once, on the host, when the object is opened: a counting sort by dep, which
// keeps the consumers of a node in ascending order.
#include "wave_check.h"

#include <stdarg.h>
#include <stdio.h>

#include <vector>

namespace rf {

static bool refuse(char* err, size_t cap, const char* fmt, ...) {
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, cap, fmt, ap);
        va_end(ap);
    }
    return false;
}

bool wave_consumers(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, uint64_t* cons_ptr, uint32_t* cons,
                    char* err, size_t err_cap) {
    if (n >= (1ull << 32)) return refuse(err, err_cap, "too many nodes");
    if (!cons_ptr) return refuse(err, err_cap, "null cons_ptr");
    if (!n) {
        cons_ptr[0] = 0;
        return true;
    }
    if (!dep_ptr) return refuse(err, err_cap, "null dep_ptr");
    if (dep_ptr[0] != 0) return refuse(err, err_cap, "dep_ptr[0] must be 0");
    for (uint64_t i = 0; i < n; ++i)
        if (dep_ptr[i] > dep_ptr[i + 1])
            return refuse(err, err_cap, "dep_ptr not monotone at node %llu", (unsigned long long)i);
    const uint64_t E = dep_ptr[n];
    if (E && !deps) return refuse(err, err_cap, "null deps");
    if (E && !cons) return refuse(err, err_cap, "null cons");
    std::vector<uint64_t> at(n + 1, 0);  // (the caller's arrays stay untouched on a refusal)
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t e = dep_ptr[i]; e < dep_ptr[i + 1]; ++e) {
            if (deps[e] >= n)
                return refuse(err, err_cap, "node %llu: dep %u out of range", (unsigned long long)i, deps[e]);
            at[(uint64_t)deps[e] + 1]++;
        }
    for (uint64_t i = 0; i < n; ++i) at[i + 1] += at[i];
    for (uint64_t i = 0; i <= n; ++i) cons_ptr[i] = at[i];
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t e = dep_ptr[i]; e < dep_ptr[i + 1]; ++e) cons[at[deps[e]]++] = (uint32_t)i;
    return true;
}

}  // namespace rf
