// k12_unmarshal.hip -- K12: Fileset JSON unmarshalled on the device
// (Eval.lookup's unmarshal(fsid), eval.go:1212, 1971-1978): the inverse of
// K11's marshal, for the canonical form only (json_parse.h has the language and
// the per-byte rules; the same source runs on the CPU under the sanitizers).
//
// The arena is cut into tiles of RF_UNMARSHAL_TILE bytes, a lane per 16 bytes
// (one 16-byte load).  Each pass is tile summary / launch_tile_scan / apply:
//   quote   which '"' delimit (an even backslash run before them; a lane walks
//           back over its own run only, to the document's start at most)
//   token   in-string parity = quote bits before the byte since the document's
//           first byte; outside strings every byte is checked against its
//           neighbours (json::tile_check_byte), a string's closing-quote lane
//           reads the string, a path's lane the whole entry and its order
//           against the previous path; counts nodes, entries, decoded path bytes
//           and the depth steps
//   depth   node braces at even depth, List brackets at odd depth, zero exactly
//           at the end, no node deeper than 4096
//   scatter nodes in closing order with depth and entry_ptr, entries in
//           document order with path offset, decoded path, ID and size
// Sums run over the whole arena mod 2^32 and are used as differences against
// the sum at the document's first byte, which makes every scan segmented by
// document (UnDev).  A refused document's counts are masked before the
// per-document scans, so the accepted documents' outputs are dense.  No atomic
// anywhere: bad[d] is a word every writer stores 1 into; all stores are plain
// vector stores.
#include <hip/hip_runtime.h>

#include "json_parse.h"
#include "unmarshal_internal.h"

namespace rf {

__device__ __forceinline__ uint32_t k12_block_excl(uint32_t x, uint32_t* s_w, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = x;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += y;
    }
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    uint32_t before = 0, tot = 0;
    for (uint32_t w = 0; w < kUnBlock / 64; ++w) {
        before += w < wave ? s_w[w] : 0u;
        tot += s_w[w];
    }
    __syncthreads();
    *total = tot;
    return before + incl - x;
}

// the first document whose end lies beyond byte `at` (n: none)
__device__ __forceinline__ uint32_t k12_find_doc(const uint32_t* __restrict__ de, uint32_t n, uint32_t at) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (de[mid] > at)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// The document byte i lies in (or the next one after it): d moves past the
// documents that end at or before i; their bounds are loaded only then.
struct K12Doc {
    uint32_t d, s0 = 0, e0 = 0;  // e0 = 0: nothing loaded yet
    __device__ __forceinline__ bool seek(const UnDev& u, uint32_t i, bool* changed) {
        *changed = false;
        if (i < e0) return true;
        while (d < u.n && (e0 = u.de[d]) <= i) ++d;
        if (d >= u.n) return false;
        s0 = u.ds[d];
        *changed = true;
        return true;
    }
};

__device__ __forceinline__ uint32_t k12_below(uint32_t word, uint32_t j) { return __popc(word & ((1u << j) - 1u)); }
__device__ __forceinline__ uint32_t k12_sx(uint16_t v) { return (uint32_t)(int32_t)(int16_t)v; }

// the lane's 16 bytes in two register pairs
struct K12Bytes {
    uint64_t lo = 0, hi = 0;
    __device__ __forceinline__ uint8_t at(uint32_t j) const { return (uint8_t)((j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8))) & 0xff); }
};
__device__ __forceinline__ K12Bytes k12_load(const uint8_t* __restrict__ arena, uint32_t base, uint32_t lim) {
    K12Bytes b;
    if (lim == kUnPer) {
        const uint4 v = *reinterpret_cast<const uint4*>(arena + base);
        b.lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
        b.hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
    } else {
        for (uint32_t j = 0; j < lim; ++j) {
            const uint64_t c = arena[base + j];
            if (j < 8)
                b.lo |= c << (8 * j);
            else
                b.hi |= c << (8 * (j - 8));
        }
    }
    return b;
}

// ---- layout ----------------------------------------------------------------------
__global__ __launch_bounds__(kUnBlock) void k12_layout(UnDev u) {
    const uint32_t d = blockIdx.x * kUnBlock + threadIdx.x;
    if (d >= u.n) return;
    const uint64_t arena = u.arena_bytes;
    auto span = [&](uint32_t k, uint64_t* b, uint64_t* e) {
        const uint64_t o = u.offs[k];
        const int64_t l = u.lens[k];
        if (l < 0 || o > arena || (uint64_t)l > arena - o) return false;
        *b = o;
        *e = o + (uint64_t)l;
        return true;
    };
    uint64_t b = 0, e = 0, pb = 0, pe = 0;
    bool ok = span(d, &b, &e);
    if (ok && d > 0 && span(d - 1, &pb, &pe)) ok = pe <= b;  // (a bad neighbour flags itself)
    if (!ok) {
        u.ctl[0] = 1u;
        b = e = 0;
    }
    u.ds[d] = (uint32_t)b;
    u.de[d] = (uint32_t)e;
    u.bad[d] = e == b ? 1u : 0u;  // an empty document is refused
}

// ---- quote bits ------------------------------------------------------------------
__global__ __launch_bounds__(kUnBlock) void k12_quote(UnDev u) {
    __shared__ uint32_t s_w[kUnBlock / 64];
    if (u.ctl[0]) return;
    const uint32_t chunk = blockIdx.x * kUnBlock + threadIdx.x;
    const uint64_t base64 = (uint64_t)chunk * kUnPer;
    uint32_t bits = 0;
    if (base64 < u.arena_bytes) {
        const uint32_t base = (uint32_t)base64, lim = min(kUnPer, u.arena_bytes - base);
        const K12Bytes by = k12_load(u.arena, base, lim);
        K12Doc doc{k12_find_doc(u.de, u.n, base)};
        for (uint32_t j = 0; j < lim; ++j) {
            const uint32_t i = base + j;
            bool changed;
            if (!doc.seek(u, i, &changed)) break;
            if (i < doc.s0 || by.at(j) != '"') continue;
            if (json::quote_is_delim(u.arena, doc.s0, i)) bits |= 1u << j;
        }
    }
    u.qm[chunk] = (uint16_t)bits;
    uint32_t total;
    const uint32_t before = k12_block_excl(__popc(bits), s_w, &total);
    u.lq[chunk] = (uint16_t)before;
    if (threadIdx.x == 0) u.tq[blockIdx.x] = total;
}

// ---- parity, token checks, counts ------------------------------------------------------
__global__ __launch_bounds__(kUnBlock) void k12_token(UnDev u) {
    __shared__ uint32_t s_w[kUnBlock / 64];
    if (u.ctl[0]) return;
    const uint32_t chunk = blockIdx.x * kUnBlock + threadIdx.x;
    const uint64_t base64 = (uint64_t)chunk * kUnPer;
    uint32_t pbits = 0, rd = 0, rn = 0, re = 0, rp = 0;
    if (base64 < u.arena_bytes) {
        const uint32_t base = (uint32_t)base64, lim = min(kUnPer, u.arena_bytes - base);
        const uint32_t qw = u.qm[chunk], qbase = u.tq[blockIdx.x] + u.lq[chunk];
        K12Doc doc{k12_find_doc(u.de, u.n, base)};
        uint32_t qs = 0;
        for (uint32_t j = 0; j < lim; ++j) {
            const uint32_t i = base + j;
            bool changed;
            if (!doc.seek(u, i, &changed)) break;
            const uint32_t d = doc.d, s0 = doc.s0, e0 = doc.e0;
            if (changed) qs = u.tq[s0 / RF_UNMARSHAL_TILE] + u.lq[s0 >> 4] + k12_below(u.qm[s0 >> 4], s0 & 15);
            if (i < s0) continue;
            const bool pb = ((qbase + k12_below(qw, j) - qs) & 1u) != 0, q = ((qw >> j) & 1u) != 0;
            pbits |= (uint32_t)pb << j;
            if (i == s0) {
                u.sd[d] = rd;
                u.sn[d] = rn;
                u.se[d] = re;
                u.sp[d] = rp;
            }
            if (pb && !q) {  // inside a string
                if (i + 1 == e0) u.bad[d] = 1u;
            } else {
                json::ByteCounts o;
                if (!json::tile_check_byte(u.arena, u.qm, s0, e0, i, pb, &o)) u.bad[d] = 1u;
                rd += (uint32_t)o.ddepth;
                rn += o.nodes;
                re += o.entries;
                rp += o.path_bytes;
            }
            if (i + 1 == e0) {
                u.en[d] = rn;
                u.ee[d] = re;
                u.ep[d] = rp;
            }
        }
    }
    u.pm[chunk] = (uint16_t)pbits;
    uint32_t total, before;
    before = k12_block_excl(rd, s_w, &total);
    u.ld[chunk] = (uint16_t)before;
    if (threadIdx.x == 0) u.td[blockIdx.x] = total;
    before = k12_block_excl(rn, s_w, &total);
    u.ln[chunk] = (uint16_t)before;
    if (threadIdx.x == 0) u.tn[blockIdx.x] = total;
    before = k12_block_excl(re, s_w, &total);
    u.le[chunk] = (uint16_t)before;
    if (threadIdx.x == 0) u.te[blockIdx.x] = total;
    before = k12_block_excl(rp, s_w, &total);
    u.lp[chunk] = before;  // (32 bits: a path's closing quote carries its whole decoded length, any size)
    if (threadIdx.x == 0) u.tp[blockIdx.x] = total;
}

// ---- depth -----------------------------------------------------------------------
__global__ __launch_bounds__(kUnBlock) void k12_depth(UnDev u) {
    if (u.ctl[0]) return;
    const uint32_t chunk = blockIdx.x * kUnBlock + threadIdx.x;
    const uint64_t base64 = (uint64_t)chunk * kUnPer;
    if (base64 >= u.arena_bytes) return;
    const uint32_t base = (uint32_t)base64, lim = min(kUnPer, u.arena_bytes - base);
    const uint32_t skip = (uint32_t)u.qm[chunk] | (uint32_t)u.pm[chunk];  // quotes and string insides
    const uint32_t dbase = u.td[blockIdx.x] + k12_sx(u.ld[chunk]);
    K12Doc doc{k12_find_doc(u.de, u.n, base)};
    uint32_t dstart = 0, rd = 0;
    for (uint32_t j = 0; j < lim; ++j) {
        const uint32_t i = base + j;
        bool changed;
        if (!doc.seek(u, i, &changed)) break;
        const uint32_t d = doc.d, s0 = doc.s0, e0 = doc.e0;
        if (changed) dstart = u.td[s0 / RF_UNMARSHAL_TILE] + k12_sx(u.ld[s0 >> 4]) + u.sd[d];
        if (i < s0) continue;
        if (i == s0) rd = u.sd[d];  // (the chunk may hold a refused neighbour's bytes before it)
        if ((skip >> j) & 1u) continue;
        if (!json::tile_depth_byte(u.arena, s0, e0, i, (int32_t)(dbase + rd - dstart))) u.bad[d] = 1u;
        rd += (uint32_t)json::depth_delta(u.arena, s0, e0, i);
    }
}

// ---- per-document counts, masked ------------------------------------------------------
__global__ __launch_bounds__(kUnBlock) void k12_doc_counts(UnDev u) {
    if (u.ctl[0]) return;
    const uint32_t d = blockIdx.x * kUnBlock + threadIdx.x;
    if (d >= u.n) return;
    uint32_t cn = 0, ce = 0, cp = 0;
    if (!u.bad[d]) {
        const uint32_t s0 = u.ds[d], l = u.de[d] - 1;
        const uint32_t ts = s0 / RF_UNMARSHAL_TILE, tl = l / RF_UNMARSHAL_TILE;
        cn = (u.tn[tl] + u.ln[l >> 4] + u.en[d]) - (u.tn[ts] + u.ln[s0 >> 4] + u.sn[d]);
        ce = (u.te[tl] + u.le[l >> 4] + u.ee[d]) - (u.te[ts] + u.le[s0 >> 4] + u.se[d]);
        cp = (u.tp[tl] + u.lp[l >> 4] + u.ep[d]) - (u.tp[ts] + u.lp[s0 >> 4] + u.sp[d]);
    }
    u.bn[d] = u.node_cnt[d] = cn;
    u.be[d] = u.counts[d] = ce;
    u.bp[d] = cp;
}

// ---- a refused document's reason: the sequential form, a lane per document -----------
__global__ __launch_bounds__(kUnBlock) void k12_reason(UnDev u) {
    if (u.ctl[0]) return;
    const uint32_t d = blockIdx.x * kUnBlock + threadIdx.x;
    if (d >= u.n) return;
    uint32_t why = 0;
    if (u.bad[d]) {
        json::NullSink sink;
        why = json::parse_document(u.arena + u.ds[d], u.de[d] - u.ds[d], sink);
        if (!why) why = kUnDisagree;
    }
    u.reason[d] = why;
}

// ---- scatter ---------------------------------------------------------------------
__global__ __launch_bounds__(kUnBlock) void k12_scatter(UnDev u) {
    if (u.ctl[0]) return;
    const uint32_t chunk = blockIdx.x * kUnBlock + threadIdx.x;
    const uint64_t base64 = (uint64_t)chunk * kUnPer;
    if (base64 >= u.arena_bytes) return;
    const uint32_t base = (uint32_t)base64, lim = min(kUnPer, u.arena_bytes - base);
    const uint32_t qw = u.qm[chunk], pw = u.pm[chunk];
    const uint32_t t = blockIdx.x;
    const uint32_t dbase = u.td[t] + k12_sx(u.ld[chunk]), nbase = u.tn[t] + u.ln[chunk], ebase = u.te[t] + u.le[chunk],
                   pbase = u.tp[t] + u.lp[chunk];
    K12Doc doc{k12_find_doc(u.de, u.n, base)};
    uint32_t dstart = 0, nstart = 0, estart = 0, pstart = 0, rd = 0, rn = 0, re = 0, rp = 0;
    bool live = false;
    for (uint32_t j = 0; j < lim; ++j) {
        const uint32_t i = base + j;
        bool changed;
        if (!doc.seek(u, i, &changed)) break;
        const uint32_t d = doc.d, s0 = doc.s0, e0 = doc.e0;
        if (changed) {
            live = !u.bad[d];
            const uint32_t ts = s0 / RF_UNMARSHAL_TILE, cs = s0 >> 4;
            dstart = u.td[ts] + k12_sx(u.ld[cs]) + u.sd[d];
            nstart = u.tn[ts] + u.ln[cs] + u.sn[d];
            estart = u.te[ts] + u.le[cs] + u.se[d];
            pstart = u.tp[ts] + u.lp[cs] + u.sp[d];
        }
        if (i < s0 || !live) continue;
        if (i == s0) {
            rd = u.sd[d];
            rn = u.sn[d];
            re = u.se[d];
            rp = u.sp[d];
        }
        const bool q = ((qw >> j) & 1u) != 0, pb = ((pw >> j) & 1u) != 0;
        if (!pb && !q) {
            const int32_t dd = json::depth_delta(u.arena, s0, e0, i);
            if (dd < 0 && u.arena[i] == '}') {  // a node closes
                const uint64_t node = (uint64_t)u.bn[d] + (nbase + rn - nstart);
                if (node < u.n_nodes) {
                    u.node_depth[node] = (dbase + rd - dstart - 1u) / 2u;
                    u.entry_ptr[node + 1] = (uint64_t)u.be[d] + (ebase + re - estart);
                } else {
                    u.ctl[1] = 1u;  // the counts and the scatter disagree: the call fails
                }
                ++rn;
            }
            rd += (uint32_t)dd;
        } else if (pb && q && json::closes_path(u.arena, s0, e0, i)) {
            const uint64_t e = (uint64_t)u.be[d] + (ebase + re - estart);
            const uint64_t po = (uint64_t)u.bp[d] + (pbase + rp - pstart);
            const int64_t q0 = json::prev_delim(u.qm, s0, i);
            uint32_t dec = 0;
            bool wrote = false;
            if (q0 >= 0) {
                bool units = true;
                for (uint32_t k = (uint32_t)q0 + 1; k < i;) {
                    uint8_t tmp[4];
                    uint32_t on, why;
                    const uint32_t take = json::unit_decode(u.arena, i, k, tmp, &on, &why);
                    if (!take) {
                        units = false;
                        break;
                    }
                    k += take;
                    dec += on;
                }
                alignas(16) uint8_t id[32];
                int64_t size = 0;
                uint32_t why;
                const uint32_t end = json::parse_entry_tail(u.arena, e0, i + 1, id, &size, &why);
                if (units && end && e < u.n_entries && po + dec <= u.path_bytes) {
                    wrote = true;
                    (void)json::path_decode(u.arena, (uint32_t)q0 + 1, i, u.paths + po);
                    u.path_off[e] = po;
                    u.sizes[e] = size;
                    uint4* row = reinterpret_cast<uint4*>(u.ids32 + 32 * e);
                    row[0] = reinterpret_cast<const uint4*>(id)[0];
                    row[1] = reinterpret_cast<const uint4*>(id)[1];
                }
            }
            if (!wrote) u.ctl[1] = 1u;  // an accepted document's entry that does not parse or does not fit
            ++re;
            rp += dec;
        }
    }
}

static dim3 k12_grid(uint64_t items) { return dim3((uint32_t)((items + kUnBlock - 1) / kUnBlock)); }

hipError_t launch_unmarshal_check(const UnDev& u, hipStream_t s) {
    if (!u.n) return hipSuccess;
    hipError_t e;
    uint64_t* scrap = u.totals + 3;  // totals of the tile scans nobody reads
    hipLaunchKernelGGL(k12_layout, k12_grid(u.n), dim3(kUnBlock), 0, s, u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (u.tiles) {
        hipLaunchKernelGGL(k12_quote, dim3(u.tiles), dim3(kUnBlock), 0, s, u);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = launch_tile_scan(u.tq, u.tiles, scrap, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(k12_token, dim3(u.tiles), dim3(kUnBlock), 0, s, u);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = launch_tile_scan(u.td, u.tiles, scrap, s)) != hipSuccess) return e;
        if ((e = launch_tile_scan(u.tn, u.tiles, scrap, s)) != hipSuccess) return e;
        if ((e = launch_tile_scan(u.te, u.tiles, scrap, s)) != hipSuccess) return e;
        if ((e = launch_tile_scan(u.tp, u.tiles, scrap, s)) != hipSuccess) return e;
        hipLaunchKernelGGL(k12_depth, dim3(u.tiles), dim3(kUnBlock), 0, s, u);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k12_doc_counts, k12_grid(u.n), dim3(kUnBlock), 0, s, u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_tile_scan(u.bn, u.n, u.totals, s)) != hipSuccess) return e;
    if ((e = launch_tile_scan(u.be, u.n, u.totals + 1, s)) != hipSuccess) return e;
    if ((e = launch_tile_scan(u.bp, u.n, u.totals + 2, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k12_reason, k12_grid(u.n), dim3(kUnBlock), 0, s, u);
    return hipGetLastError();
}

hipError_t launch_unmarshal_scatter(const UnDev& u, hipStream_t s) {
    if (!u.n || !u.tiles) return hipSuccess;
    hipLaunchKernelGGL(k12_scatter, dim3(u.tiles), dim3(kUnBlock), 0, s, u);
    return hipGetLastError();
}

}  // namespace rf
