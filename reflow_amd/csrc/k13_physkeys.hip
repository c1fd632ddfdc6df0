// k13_physkeys.hip -- K13: physical cache keys on the device
// (Flow.PhysicalDigest, flow.go:764-792): the Fileset material of finished
// nodes' values (executor.go:214-233) kept in an HBM arena, and the keys of the
// consumers they affect written to the caller's key rows.  phys_emit.h has the
// per-node, per-entry and per-segment rules; the same source runs on the CPU
// under the sanitizers (physkeys_flat.cpp).
//
// Passes, each a kernel that reads what the one before wrote:
//   lengths  per forest node its contribution (a Map counts iff the node has no
//            List children) / scan in tiles of RF_PHYS_LIST_TILE; per document
//            the difference of two prefix sums, padded to 16 / scan
//   emit     a wave per entry: path ‖ 00 05 ‖ ID at the entry's place, the
//            owner node found through entry_ptr by search
//   affected a byte per graph node (every writer stores 1): the listed nodes, and
//            a lane per consumer entry found through a scan of the listed
//            nodes' fan-outs; per-tile counts / scan / scatter: the affected
//            nodes that have a row, ascending
//   measure  per affected node the computable bit (a has-value byte per dep),
//            the material length and the segment count / three scans
//   segments per dep (offset, length) of its material, then the suffix
//   gather   RF_PHYS_COPY_TILE output bytes per workgroup, 16 per lane; the
//            segments a tile touches are found by search, pad bytes are zero
//   scatter  K1's digests and the zero rows to the key rows
// Integer only, no atomic anywhere; all stores are plain vector stores.
#include <hip/hip_runtime.h>

#include "physkeys_internal.h"

namespace rf {

__device__ __forceinline__ uint64_t k13_block_excl(uint64_t x, uint64_t* s_w, uint64_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t incl = x;
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint64_t before = 0, tot = 0;
    for (uint32_t w = 0; w < kPhysBlock / 64; ++w) {
        before += w < wave ? s_w[w] : 0ull;
        tot += s_w[w];
    }
    __syncthreads();
    *total = tot;
    return before + incl - x;
}

// ---- the scan ---------------------------------------------------------------
__global__ __launch_bounds__(kPhysBlock) void k13_scan_local(uint64_t* __restrict__ vals, uint64_t n,
                                                             uint64_t* __restrict__ tile_sum) {
    __shared__ uint64_t s_w[kPhysBlock / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * RF_PHYS_LIST_TILE + threadIdx.x * kPhysPer;
    uint64_t x[kPhysPer], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPhysPer; ++k) {
        x[k] = i0 + k < n ? vals[i0 + k] : 0ull;
        sum += x[k];
    }
    uint64_t tot, before = k13_block_excl(sum, s_w, &tot);
#pragma unroll
    for (uint32_t k = 0; k < kPhysPer; ++k) {
        if (i0 + k < n) vals[i0 + k] = before;
        before += x[k];
    }
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = tot;
}

// one workgroup: the tile sums become the sums before each tile
__global__ __launch_bounds__(kPhysBlock) void k13_scan_tiles(uint64_t* __restrict__ tile_sum, uint64_t tiles,
                                                             uint64_t* __restrict__ total) {
    __shared__ uint64_t s_w[kPhysBlock / 64];
    uint64_t carry = 0;
    for (uint64_t base = 0; base < tiles; base += RF_PHYS_LIST_TILE) {
        const uint64_t i0 = base + threadIdx.x * kPhysPer;
        uint64_t x[kPhysPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPhysPer; ++k) {
            x[k] = i0 + k < tiles ? tile_sum[i0 + k] : 0ull;
            sum += x[k];
        }
        uint64_t tot, before = carry + k13_block_excl(sum, s_w, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kPhysPer; ++k) {
            if (i0 + k < tiles) tile_sum[i0 + k] = before;
            before += x[k];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kPhysBlock) void k13_scan_add(uint64_t* __restrict__ vals, uint64_t n,
                                                           const uint64_t* __restrict__ tile_sum) {
    const uint64_t add = tile_sum[blockIdx.x];
    const uint64_t i0 = (uint64_t)blockIdx.x * RF_PHYS_LIST_TILE + threadIdx.x * kPhysPer;
#pragma unroll
    for (uint32_t k = 0; k < kPhysPer; ++k)
        if (i0 + k < n) vals[i0 + k] += add;
}

hipError_t launch_phys_scan(uint64_t* vals, uint64_t n, uint64_t* tile_tmp, uint64_t* total, hipStream_t s) {
    if (n == 0) return hipMemsetAsync(total, 0, 8, s);
    const uint64_t tiles = phys_tiles(n);
    k13_scan_local<<<dim3((uint32_t)tiles), dim3(kPhysBlock), 0, s>>>(vals, n, tile_tmp);
    k13_scan_tiles<<<dim3(1), dim3(kPhysBlock), 0, s>>>(tile_tmp, tiles, total);
    if (tiles > 1) k13_scan_add<<<dim3((uint32_t)tiles), dim3(kPhysBlock), 0, s>>>(vals, n, tile_tmp);
    return hipGetLastError();
}

static uint32_t strided_grid(uint64_t items, uint32_t per_block) {
    return (uint32_t)std::min<uint64_t>((items + per_block - 1) / per_block, 16384);
}

// ---- set values -------------------------------------------------------------
__global__ __launch_bounds__(kPhysBlock) void k13_node_len(PhysVals v, uint64_t* __restrict__ node_pre) {
    const uint64_t stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; j < v.n_nodes; j += stride)
        node_pre[j] = phys_node_len(v, j);
}

__global__ __launch_bounds__(kPhysBlock) void k13_doc_len(PhysVals v, const uint64_t* __restrict__ node_pre,
                                                          uint64_t* __restrict__ doc_len,
                                                          uint64_t* __restrict__ doc_off) {
    const uint64_t stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t d = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; d < v.n_docs; d += stride) {
        const uint64_t len =
            v.doc_node[d] == kPhysSkip ? 0ull : node_pre[v.doc_node_ptr[d + 1]] - node_pre[v.doc_node_ptr[d]];
        doc_len[d] = len;
        doc_off[d] = phys_align16(len);
    }
}

hipError_t launch_phys_lengths(const PhysSetDev& d, hipStream_t s) {
    if (d.v.n_nodes)
        k13_node_len<<<dim3(strided_grid(d.v.n_nodes, kPhysBlock)), dim3(kPhysBlock), 0, s>>>(d.v, d.node_pre);
    hipError_t e = launch_phys_scan(d.node_pre, d.v.n_nodes, d.tile_tmp, d.node_pre + d.v.n_nodes, s);
    if (e != hipSuccess) return e;
    if (d.v.n_docs)
        k13_doc_len<<<dim3(strided_grid(d.v.n_docs, kPhysBlock)), dim3(kPhysBlock), 0, s>>>(d.v, d.node_pre, d.doc_len,
                                                                                           d.doc_off);
    return launch_phys_scan(d.doc_off, d.v.n_docs, d.tile_tmp, d.doc_off + d.v.n_docs, s);
}

// a wave per entry, a lane per byte
__global__ __launch_bounds__(kPhysBlock) void k13_emit(PhysVals v, const uint64_t* __restrict__ node_pre,
                                                       const uint64_t* __restrict__ doc_off,
                                                       uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t waves = (uint64_t)gridDim.x * (kPhysBlock / 64);
    for (uint64_t e = (uint64_t)blockIdx.x * (kPhysBlock / 64) + (threadIdx.x >> 6); e < v.n_entries; e += waves) {
        uint64_t dst;
        if (!phys_entry_dst(v, node_pre, doc_off, e, &dst)) continue;
        const uint64_t len = phys_entry_len(v, e);
        for (uint64_t k = lane; k < len; k += 64) out[dst + k] = phys_entry_byte(v, e, k);
    }
}

__global__ __launch_bounds__(kPhysBlock) void k13_set_rows(PhysVals v, const uint64_t* __restrict__ doc_len,
                                                           const uint64_t* __restrict__ doc_off, uint64_t base,
                                                           uint64_t* __restrict__ val_off,
                                                           uint64_t* __restrict__ val_len, uint8_t* __restrict__ has) {
    const uint64_t stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t d = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; d < v.n_docs; d += stride) {
        const uint32_t g = v.doc_node[d];
        if (g == kPhysSkip) continue;
        val_off[g] = base + doc_off[d];
        val_len[g] = doc_len[d];
        has[g] = 1;
    }
}

hipError_t launch_phys_emit(const PhysSetDev& d, uint8_t* arena, uint64_t base, uint64_t* val_off, uint64_t* val_len,
                            uint8_t* has, hipStream_t s) {
    if (d.v.n_entries)
        k13_emit<<<dim3(strided_grid(d.v.n_entries, kPhysBlock / 64)), dim3(kPhysBlock), 0, s>>>(d.v, d.node_pre,
                                                                                                d.doc_off, arena + base);
    if (d.v.n_docs)
        k13_set_rows<<<dim3(strided_grid(d.v.n_docs, kPhysBlock)), dim3(kPhysBlock), 0, s>>>(d.v, d.doc_len, d.doc_off,
                                                                                            base, val_off, val_len, has);
    return hipGetLastError();
}

__global__ __launch_bounds__(kPhysBlock) void k13_clear(const uint32_t* __restrict__ nodes, uint64_t n,
                                                        uint8_t* __restrict__ has) {
    const uint64_t stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; i < n; i += stride) has[nodes[i]] = 0;
}

hipError_t launch_phys_clear(const uint32_t* nodes, uint64_t n, uint8_t* has, hipStream_t s) {
    if (n) k13_clear<<<dim3(strided_grid(n, kPhysBlock)), dim3(kPhysBlock), 0, s>>>(nodes, n, has);
    return hipGetLastError();
}

// ---- update -----------------------------------------------------------------
// the listed nodes themselves, and how many consumer entries each has
__global__ __launch_bounds__(kPhysBlock) void k13_mark_self(PhysUpdDev u) {
    const uint64_t stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; i < u.n_listed; i += stride) {
        const uint32_t v = u.listed[i];
        if (u.flags & RF_PHYS_SELF) u.mark[v] = 1;
        u.list_off[i] = (u.flags & RF_PHYS_CONSUMERS) ? u.cons_ptr[v + 1] - u.cons_ptr[v] : 0ull;
    }
}

// a lane per consumer entry of the listed nodes, whatever their fan-out: entry t
// belongs to the last listed node whose entries begin at or before it
__global__ __launch_bounds__(kPhysBlock) void k13_mark_consumers(PhysUpdDev u) {
    const uint64_t total = u.list_off[u.n_listed], stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; t < total; t += stride) {
        const uint64_t i = phys_upper_index(u.list_off, 0, u.n_listed, t);
        u.mark[u.cons[u.cons_ptr[u.listed[i]] + (t - u.list_off[i])]] = 1;
    }
}

__device__ __forceinline__ bool k13_affected(const PhysUpdDev& u, uint64_t i) {
    return i < u.n && u.mark[i] && u.phys_row[i] != RF_PHYS_NO_ROW;
}

__global__ __launch_bounds__(kPhysBlock) void k13_aff_count(PhysUpdDev u) {
    __shared__ uint64_t s_w[kPhysBlock / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * RF_PHYS_LIST_TILE + threadIdx.x * kPhysPer;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPhysPer; ++k) sum += k13_affected(u, i0 + k);
    uint64_t tot;
    (void)k13_block_excl(sum, s_w, &tot);
    if (threadIdx.x == 0) u.tile_cnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kPhysBlock) void k13_aff_scatter(PhysUpdDev u) {
    __shared__ uint64_t s_w[kPhysBlock / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * RF_PHYS_LIST_TILE + threadIdx.x * kPhysPer;
    bool f[kPhysPer];
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kPhysPer; ++k) {
        f[k] = k13_affected(u, i0 + k);
        sum += f[k];
    }
    uint64_t tot, at = u.tile_cnt[blockIdx.x] + k13_block_excl(sum, s_w, &tot);
#pragma unroll
    for (uint32_t k = 0; k < kPhysPer; ++k)
        if (f[k]) u.aff[at++] = (uint32_t)(i0 + k);
}

hipError_t launch_phys_affected(const PhysUpdDev& u, hipStream_t s) {
    const uint64_t tiles = phys_tiles(u.n);
    hipError_t e = hipMemsetAsync(u.mark, 0, u.n, s);
    if (e != hipSuccess) return e;
    k13_mark_self<<<dim3(strided_grid(u.n_listed, kPhysBlock)), dim3(kPhysBlock), 0, s>>>(u);
    e = launch_phys_scan(u.list_off, u.n_listed, u.list_tmp, u.list_off + u.n_listed, s);
    if (e != hipSuccess) return e;
    if (u.flags & RF_PHYS_CONSUMERS) k13_mark_consumers<<<dim3(4096), dim3(kPhysBlock), 0, s>>>(u);
    k13_aff_count<<<dim3((uint32_t)tiles), dim3(kPhysBlock), 0, s>>>(u);
    k13_scan_tiles<<<dim3(1), dim3(kPhysBlock), 0, s>>>(u.tile_cnt, tiles, u.tile_cnt + tiles);
    return hipGetLastError();
}

__global__ __launch_bounds__(kPhysBlock) void k13_measure(PhysUpdDev u) {
    const uint64_t stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; k < u.n_aff; k += stride) {
        const uint32_t i = u.aff[k];
        if (u.phys_row[i] >= u.n_rows) u.ctl[0] = 1;
        bool comp = true;
        uint64_t len = u.suffix_ptr[i + 1] - u.suffix_ptr[i];
        const uint64_t d0 = u.dep_ptr[i], d1 = u.dep_ptr[i + 1];
        for (uint64_t e = d0; e < d1; ++e) {
            const uint32_t d = u.deps[e];
            if (u.has[d])
                len += u.val_len[d];
            else
                comp = false;
        }
        u.comp[k] = comp;
        u.mlen[k] = comp ? len : 0ull;
        u.moff[k] = comp ? phys_align16(len) : 0ull;
        u.seg_ptr[k] = comp ? d1 - d0 + 1 : 0ull;
        u.crank[k] = comp;
    }
}

hipError_t launch_phys_measure(const PhysUpdDev& u, hipStream_t s) {
    if (!u.n_aff) return hipSuccess;
    const uint64_t tiles = phys_tiles(u.n);
    k13_aff_scatter<<<dim3((uint32_t)tiles), dim3(kPhysBlock), 0, s>>>(u);
    k13_measure<<<dim3(strided_grid(u.n_aff, kPhysBlock)), dim3(kPhysBlock), 0, s>>>(u);
    hipError_t e = launch_phys_scan(u.moff, u.n_aff, u.tile_tmp, u.moff + u.n_aff, s);
    if (e == hipSuccess) e = launch_phys_scan(u.seg_ptr, u.n_aff, u.tile_tmp, u.seg_ptr + u.n_aff, s);
    if (e == hipSuccess) e = launch_phys_scan(u.crank, u.n_aff, u.tile_tmp, u.crank + u.n_aff, s);
    return e;
}

__global__ __launch_bounds__(kPhysBlock) void k13_segments(PhysUpdDev u) {
    const uint64_t stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t k = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; k < u.n_aff; k += stride) {
        if (!u.comp[k]) continue;
        const uint32_t i = u.aff[k];
        uint64_t sg = u.seg_ptr[k], pos = u.moff[k];
        for (uint64_t e = u.dep_ptr[i]; e < u.dep_ptr[i + 1]; ++e, ++sg) {
            const uint32_t d = u.deps[e];
            u.seg_dst[sg] = pos;
            u.seg_src[sg] = u.val_off[d];
            u.seg_len[sg] = u.val_len[d];
            pos += u.val_len[d];
        }
        u.seg_dst[sg] = pos;
        u.seg_src[sg] = kPhysSrcSuffix | u.suffix_ptr[i];
        u.seg_len[sg] = u.suffix_ptr[i + 1] - u.suffix_ptr[i];
    }
}

hipError_t launch_phys_segments(const PhysUpdDev& u, hipStream_t s) {
    if (u.n_aff) k13_segments<<<dim3(strided_grid(u.n_aff, kPhysBlock)), dim3(kPhysBlock), 0, s>>>(u);
    return hipGetLastError();
}

__global__ __launch_bounds__(kPhysBlock) void k13_gather(PhysSegs g, const uint8_t* __restrict__ arena,
                                                         const uint8_t* __restrict__ suffix, uint8_t* __restrict__ out,
                                                         uint64_t out_bytes) {
    __shared__ uint64_t s_rng[2];
    for (uint64_t t0 = (uint64_t)blockIdx.x * RF_PHYS_COPY_TILE; t0 < out_bytes;
         t0 += (uint64_t)gridDim.x * RF_PHYS_COPY_TILE) {
        const uint64_t t1 = t0 + RF_PHYS_COPY_TILE < out_bytes ? t0 + RF_PHYS_COPY_TILE : out_bytes;
        if (threadIdx.x == 0) {
            s_rng[0] = phys_upper_index(g.dst, 0, g.n, t0);
            s_rng[1] = phys_upper_index(g.dst, 0, g.n, t1 - 1) + 1;
        }
        __syncthreads();
        const uint64_t b0 = t0 + 16ull * threadIdx.x;
        if (b0 < t1) {  // out_bytes % 16 == 0: the lane's sixteen bytes lie inside
            uint32_t w[4];
            phys_gather_run(g, s_rng[0], s_rng[1], b0, arena, suffix, w);
            *reinterpret_cast<uint4*>(out + b0) = make_uint4(w[0], w[1], w[2], w[3]);
        }
        __syncthreads();
    }
}

hipError_t launch_phys_gather(const PhysUpdDev& u, uint64_t n_segs, const uint8_t* arena, const uint8_t* suffix,
                              uint8_t* out, uint64_t out_bytes, hipStream_t s) {
    if (!out_bytes || !n_segs) return hipSuccess;
    PhysSegs g;
    g.n = n_segs;
    g.dst = u.seg_dst;
    g.src = u.seg_src;
    g.len = u.seg_len;
    k13_gather<<<dim3(strided_grid(out_bytes, RF_PHYS_COPY_TILE)), dim3(kPhysBlock), 0, s>>>(g, arena, suffix, out,
                                                                                              out_bytes);
    return hipGetLastError();
}

// eight lanes per affected node, a word each
__global__ __launch_bounds__(kPhysBlock) void k13_scatter(PhysUpdDev u, const uint32_t* __restrict__ dig,
                                                          uint32_t* __restrict__ keys) {
    const uint64_t stride = (uint64_t)gridDim.x * kPhysBlock;
    for (uint64_t t = (uint64_t)blockIdx.x * kPhysBlock + threadIdx.x; t < 8 * u.n_aff; t += stride) {
        const uint64_t k = t >> 3, w = t & 7;
        keys[8 * u.phys_row[u.aff[k]] + w] = u.comp[k] ? dig[8 * u.crank[k] + w] : 0u;
    }
}

hipError_t launch_phys_scatter(const PhysUpdDev& u, const uint8_t* dig, uint8_t* keys32, hipStream_t s) {
    if (u.n_aff)
        k13_scatter<<<dim3(strided_grid(8 * u.n_aff, kPhysBlock)), dim3(kPhysBlock), 0, s>>>(
            u, reinterpret_cast<const uint32_t*>(dig), reinterpret_cast<uint32_t*>(keys32));
    return hipGetLastError();
}

}  // namespace rf
