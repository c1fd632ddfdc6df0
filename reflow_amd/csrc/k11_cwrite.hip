// k11_cwrite.hip -- K11: the cache write on the device (Eval.CacheWrite,
// eval.go:1113-1154).
//   * Fileset values marshalled to JSON (marshal, eval.go:1961-1967): a piece
//     stream flattened on the host (marshal_flat.cpp) is measured, scanned and
//     emitted here, lane per piece, through json_emit.h -- the source the host
//     executor runs under the sanitizers.  A length pass leaves every piece's
//     bytes-before within its tile of RF_MARSHAL_TILE pieces and the tile's
//     sum; launch_tile_scan turns the sums into offsets; the emit pass writes
//     each piece at its value's 16-byte aligned arena offset plus its place in
//     the value.  No atomic on a shared counter anywhere: a piece's place is a
//     function of the stream alone, so two runs give equal bytes.
//   * The key gather of rf_eval_wave_cache_write: which listed nodes take part,
//     their present keys as Put rows in node order then key order, and their
//     (fsid, size) rows for the repository index -- the same tile mark / scan /
//     scatter.
// Every store is a plain vector store.
#include <hip/hip_runtime.h>

#include "cwrite_internal.h"
#include "json_emit.h"
#include "marshal_flat.h"

namespace rf {

// Bytes (rows) before this lane within its workgroup, and the workgroup's sum:
// wave scans by shuffles, wave totals through LDS (s_w: one word per wave).
__device__ __forceinline__ uint32_t k11_block_excl(uint32_t x, uint32_t* s_w, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = x;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
    for (uint32_t w = 0; w < kMarshalBlock / 64; ++w) {
        before += w < wave ? s_w[w] : 0u;
        tot += s_w[w];
    }
    __syncthreads();
    *total = tot;
    return before + incl - x;
}

// ---- marshal ---------------------------------------------------------------------
// The sequence bound of an entry's path is the path's own end, path_off[e + 1],
// never the blob's: a path that ends inside a multi-byte sequence does not
// borrow the next path's first bytes.
__global__ __launch_bounds__(kMarshalBlock) void k11_marshal_len(MarshalDev m) {
    __shared__ uint32_t s_w[kMarshalBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * RF_MARSHAL_TILE + (uint64_t)threadIdx.x * kMarshalPer;
    uint32_t len[kMarshalPer];
    uint32_t sum = 0;
    bool zero = false;
#pragma unroll
    for (uint32_t j = 0; j < kMarshalPer; ++j) {
        const uint64_t p = base + j;
        len[j] = 0;
        if (p < m.n_pieces) {
            const uint32_t b = m.pb[p];
            if (b & kPieceEntry) {
                const uint32_t e = m.pa[p];
                const uint64_t o0 = m.path_off[e];
                const uint32_t pn = (uint32_t)(m.path_off[e + 1] - o0);
                len[j] = (uint32_t)json::entry_len(m.paths + o0, pn, m.sizes[e]) + (b & kPieceComma);
                const uint4* id = reinterpret_cast<const uint4*>(m.ids32 + 32ull * e);
                const uint4 lo = id[0], hi = id[1];
                zero |= (lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) == 0;
            } else {
                len[j] = b;
            }
        }
        sum += len[j];
    }
    uint32_t total;
    uint32_t before = k11_block_excl(sum, s_w, &total);
#pragma unroll
    for (uint32_t j = 0; j < kMarshalPer; ++j) {
        const uint64_t p = base + j;
        if (p < m.n_pieces) m.local[p] = before;
        before += len[j];
    }
    if (threadIdx.x == 0) m.tile_count[blockIdx.x] = total;
    if (zero) *m.zero_seen = 1u;  // (every writer stores the same word)
}

// bytes before each value, unpadded (after the tile scan; ustart[n_values] is the scan's total)
__global__ __launch_bounds__(kMarshalBlock) void k11_marshal_vstart(MarshalDev m) {
    const uint64_t v = (uint64_t)blockIdx.x * kMarshalBlock + threadIdx.x;
    if (v >= m.n_values) return;
    const uint32_t p = m.value_ptr[v];  // (< n_pieces: a value has at least its braces)
    m.ustart[v] = (uint64_t)m.tile_count[p / RF_MARSHAL_TILE] + m.local[p];
}

__global__ __launch_bounds__(kMarshalBlock) void k11_marshal_emit(MarshalDev m, const uint64_t* __restrict__ offs,
                                                                  uint8_t* __restrict__ arena) {
    const uint64_t p = (uint64_t)blockIdx.x * kMarshalBlock + threadIdx.x;
    if (p >= m.n_pieces) return;
    const uint32_t v = m.pv[p];
    const uint64_t in_value = (uint64_t)m.tile_count[p / RF_MARSHAL_TILE] + m.local[p] - m.ustart[v];
    uint8_t* dst = arena + offs[v] + in_value;
    const uint32_t a = m.pa[p], b = m.pb[p];
    if (b & kPieceEntry) {
        const uint64_t o0 = m.path_off[a];
        const uint32_t pn = (uint32_t)(m.path_off[a + 1] - o0);
        json::emit_entry(dst, m.paths + o0, pn, m.ids32 + 32ull * a, m.sizes[a], (b & kPieceComma) != 0);
    } else {
        const uint8_t* src = m.blob + a;
        for (uint32_t i = 0; i < b; ++i) dst[i] = src[i];
    }
}

hipError_t launch_marshal_len(const MarshalDev& m, hipStream_t s) {
    if (!m.n_pieces) return hipSuccess;
    const uint64_t tiles = ((uint64_t)m.n_pieces + RF_MARSHAL_TILE - 1) / RF_MARSHAL_TILE;
    hipLaunchKernelGGL(k11_marshal_len, dim3((uint32_t)tiles), dim3(kMarshalBlock), 0, s, m);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_tile_scan(m.tile_count, tiles, m.ustart + m.n_values, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k11_marshal_vstart, dim3((m.n_values + kMarshalBlock - 1) / kMarshalBlock), dim3(kMarshalBlock), 0,
                       s, m);
    return hipGetLastError();
}

hipError_t launch_marshal_emit(const MarshalDev& m, const uint64_t* offs, uint8_t* arena, hipStream_t s) {
    if (!m.n_pieces) return hipSuccess;
    hipLaunchKernelGGL(k11_marshal_emit, dim3((m.n_pieces + kMarshalBlock - 1) / kMarshalBlock), dim3(kMarshalBlock), 0, s,
                       m, offs, arena);
    return hipGetLastError();
}

// ---- cache write: the key gather ----------------------------------------------------
// Row i (listed node nodes[i]) takes part iff its node is CACHEABLE, not (EXTERN
// under no_cache_extern) and has a present key (eval.go:1119-1131, 1146-1152); a
// key row of 32 zero bytes is absent (flow.go:798-800).  INVALID does not matter
// for a write.  Returns the present keys' mask.
__device__ __forceinline__ uint32_t k11_cw_row(const CwDev& c, uint32_t node, uint32_t* reason) {
    const uint32_t f = c.flags[node];
    if (!(f & RF_PLAN_F_CACHEABLE)) {
        *reason = kCwNotCacheable;
        return 0;
    }
    if (c.no_cache_extern && (f & RF_PLAN_F_EXTERN)) {
        *reason = kCwExtern;
        return 0;
    }
    const uint64_t k0 = c.key_ptr[node];
    const uint32_t nk = (uint32_t)(c.key_ptr[node + 1] - k0);
    uint32_t mask = 0;
    for (uint32_t j = 0; j < nk; ++j) {
        const uint64_t row = c.by_slot ? (uint64_t)c.key_slots[k0 + j] : k0 + j;
        const uint4* k4 = reinterpret_cast<const uint4*>(c.keys + 32ull * row);
        const uint4 lo = k4[0], hi = k4[1];
        if ((lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) != 0) mask |= 1u << j;
    }
    *reason = mask ? kCwWritten : kCwNoKey;
    return mask;
}

__global__ __launch_bounds__(kMarshalBlock) void k11_cw_mark(CwDev c) {
    __shared__ uint32_t s_w[kMarshalBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * RF_MARSHAL_TILE + (uint64_t)threadIdx.x * kMarshalPer;
    uint32_t keys = 0, rows = 0;
    bool bad = false;
    for (uint32_t j = 0; j < kMarshalPer; ++j) {
        const uint64_t i = base + j;
        if (i >= c.n) break;
        const uint32_t node = c.nodes[i];
        bad |= c.state[node] != RF_PLAN_DONE;
        uint32_t reason;
        const uint32_t np = (uint32_t)__popc(k11_cw_row(c, node, &reason));
        c.nput[i] = (uint8_t)np;
        c.reason[i] = (uint8_t)reason;
        keys += np;
        rows += reason == kCwWritten;
    }
    uint32_t tk, tr;
    (void)k11_block_excl(keys, s_w, &tk);
    (void)k11_block_excl(rows, s_w, &tr);
    if (threadIdx.x == 0) {
        c.tile_keys[blockIdx.x] = tk;
        c.tile_nodes[blockIdx.x] = tr;
    }
    if (bad) c.ctl[kCwBad] = 1u;  // (every writer stores the same word)
}

// the rows skipped, by reason: one workgroup strides over the reason bytes
__global__ __launch_bounds__(1024) void k11_cw_count(CwDev c) {
    __shared__ uint32_t s_c[16][3];
    uint32_t r[3] = {0, 0, 0};
    for (uint64_t i = threadIdx.x; i < c.n; i += 1024) {
        const uint32_t q = c.reason[i];
        r[0] += q == kCwNotCacheable;
        r[1] += q == kCwExtern;
        r[2] += q == kCwNoKey;
    }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t q = 0; q < 3; ++q) {
        uint32_t x = r[q];
        for (int o = 32; o; o >>= 1) x += __shfl_down(x, o, 64);
        if (lane == 0) s_c[wave][q] = x;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        uint32_t x = 0;
        for (uint32_t w = 0; w < 16; ++w) x += s_c[w][threadIdx.x];
        c.ctl[kCwSkip + threadIdx.x] = x;
    }
}

__global__ __launch_bounds__(kMarshalBlock) void k11_cw_scatter(CwDev c, uint4* __restrict__ put_keys,
                                                                uint4* __restrict__ put_vals,
                                                                uint4* __restrict__ repo_ids,
                                                                int64_t* __restrict__ repo_sizes) {
    __shared__ uint32_t s_w[kMarshalBlock / 64];
    const uint64_t base = (uint64_t)blockIdx.x * RF_MARSHAL_TILE + (uint64_t)threadIdx.x * kMarshalPer;
    uint32_t keys = 0, rows = 0;
    for (uint32_t j = 0; j < kMarshalPer; ++j) {
        const uint64_t i = base + j;
        if (i >= c.n) break;
        keys += c.nput[i];
        rows += c.reason[i] == kCwWritten;
    }
    uint32_t unused;
    uint64_t kpos = (uint64_t)c.tile_keys[blockIdx.x] + k11_block_excl(keys, s_w, &unused);
    uint64_t rpos = (uint64_t)c.tile_nodes[blockIdx.x] + k11_block_excl(rows, s_w, &unused);
    for (uint32_t j = 0; j < kMarshalPer; ++j) {
        const uint64_t i = base + j;
        if (i >= c.n) break;
        if (c.reason[i] != kCwWritten) continue;
        const uint32_t node = c.nodes[i];
        const uint4* fs = reinterpret_cast<const uint4*>(c.fsids + 32ull * i);
        const uint4 flo = fs[0], fhi = fs[1];
        repo_ids[2 * rpos] = flo;
        repo_ids[2 * rpos + 1] = fhi;
        repo_sizes[rpos] = c.sizes[i];
        ++rpos;
        const uint64_t k0 = c.key_ptr[node];
        const uint32_t nk = (uint32_t)(c.key_ptr[node + 1] - k0);
        for (uint32_t q = 0; q < nk; ++q) {
            const uint64_t row = c.by_slot ? (uint64_t)c.key_slots[k0 + q] : k0 + q;
            const uint4* k4 = reinterpret_cast<const uint4*>(c.keys + 32ull * row);
            const uint4 lo = k4[0], hi = k4[1];
            if ((lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) == 0) continue;
            put_keys[2 * kpos] = lo;
            put_keys[2 * kpos + 1] = hi;
            put_vals[2 * kpos] = flo;
            put_vals[2 * kpos + 1] = fhi;
            ++kpos;
        }
    }
}

hipError_t launch_cw_mark(const CwDev& c, hipStream_t s) {
    if (!c.n) return hipSuccess;
    const uint64_t tiles = ((uint64_t)c.n + RF_MARSHAL_TILE - 1) / RF_MARSHAL_TILE;
    hipLaunchKernelGGL(k11_cw_mark, dim3((uint32_t)tiles), dim3(kMarshalBlock), 0, s, c);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_tile_scan(c.tile_keys, tiles, c.totals, s)) != hipSuccess) return e;
    if ((e = launch_tile_scan(c.tile_nodes, tiles, c.totals + 1, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k11_cw_count, dim3(1), dim3(1024), 0, s, c);
    return hipGetLastError();
}

hipError_t launch_cw_scatter(const CwDev& c, uint8_t* put_keys, uint8_t* put_vals, uint8_t* repo_ids,
                             int64_t* repo_sizes, hipStream_t s) {
    if (!c.n) return hipSuccess;
    const uint64_t tiles = ((uint64_t)c.n + RF_MARSHAL_TILE - 1) / RF_MARSHAL_TILE;
    hipLaunchKernelGGL(k11_cw_scatter, dim3((uint32_t)tiles), dim3(kMarshalBlock), 0, s, c,
                       reinterpret_cast<uint4*>(put_keys), reinterpret_cast<uint4*>(put_vals),
                       reinterpret_cast<uint4*>(repo_ids), repo_sizes);
    return hipGetLastError();
}

}  // namespace rf
