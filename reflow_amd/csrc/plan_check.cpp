// plan_check.cpp -- HIP-free: CSR validation, cycle detection and the depth
// bound of an evaluation plan's node graph (plan_check.h).  Eval.todo
// (eval.go:902-955) recurses over Deps and so assumes a DAG; the plan's round
// loop runs at most `depth` rounds, so a cycle is refused here, on the host.
#include "plan_check.h"

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

bool plan_check(uint64_t n, const uint64_t* dep_ptr, const uint32_t* deps, uint32_t* depth, char* err,
                size_t err_cap) {
    if (depth) *depth = 0;
    if (n >= (1ull << 32)) return refuse(err, err_cap, "too many nodes");
    if (!n) return true;
    if (!dep_ptr) return refuse(err, err_cap, "null dep_ptr");
    if (dep_ptr[0] != 0) return refuse(err, err_cap, "dep_ptr[0] must be 0");
    for (uint64_t i = 0; i < n; ++i)
        if (dep_ptr[i] > dep_ptr[i + 1]) return refuse(err, err_cap, "dep_ptr not monotone at node %llu", (unsigned long long)i);
    const uint64_t E = dep_ptr[n];
    if (E && !deps) return refuse(err, err_cap, "null deps");
    // reverse edges: dep -> the nodes that list it
    std::vector<uint64_t> cptr(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t e = dep_ptr[i]; e < dep_ptr[i + 1]; ++e) {
            if (deps[e] >= n)
                return refuse(err, err_cap, "node %llu: dep %u out of range", (unsigned long long)i, deps[e]);
            cptr[(uint64_t)deps[e] + 1]++;
        }
    for (uint64_t i = 0; i < n; ++i) cptr[i + 1] += cptr[i];
    std::vector<uint32_t> cons(E ? E : 1);
    {
        std::vector<uint64_t> fill(cptr.begin(), cptr.end() - 1);
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t e = dep_ptr[i]; e < dep_ptr[i + 1]; ++e) cons[fill[deps[e]]++] = (uint32_t)i;
    }
    // Kahn from the leaves: a node is released when all its dep entries are
    std::vector<uint64_t> waiting(n);
    std::vector<uint32_t> d(n, 1), order;
    order.reserve(n);
    for (uint64_t i = 0; i < n; ++i) {
        waiting[i] = dep_ptr[i + 1] - dep_ptr[i];
        if (!waiting[i]) order.push_back((uint32_t)i);
    }
    uint32_t deepest = 0;
    for (size_t h = 0; h < order.size(); ++h) {
        const uint32_t v = order[h];
        if (d[v] > deepest) deepest = d[v];
        for (uint64_t e = cptr[v]; e < cptr[(uint64_t)v + 1]; ++e) {
            const uint32_t c = cons[e];
            if (d[c] < d[v] + 1) d[c] = d[v] + 1;
            if (--waiting[c] == 0) order.push_back(c);
        }
    }
    if (order.size() != n) {
        uint64_t at = 0;
        while (at < n && !waiting[at]) ++at;
        return refuse(err, err_cap, "the graph has a cycle (node %llu is on it or above it)", (unsigned long long)at);
    }
    if (depth) *depth = deepest;
    return true;
}

}  // namespace rf
