// k9_repo.hip -- K9: the repository index (rf_repo_*): a set of object IDs
// with their sizes in HBM, and against it Eval.lookup's missing()
// (eval.go:1227-1243, 1983-2014) and Manager.NeedTransfer
// (repository/manager.go:197-234) for batches of Fileset values.
//
// Table: open addressing on key_hash(ID); per slot a tag word (empty, busy,
// live, tombstone), the 32-B ID and the int64 size.  A batch is deduplicated by
// ID first (the row-index table below, the lowest row wins), so the keys one
// launch inserts are distinct: a busy slot is another lane's key and is skipped
// without reading it (k5_assoc_insert's protocol, no per-slot fences), and
// everything a launch writes is read only after the kernel boundary.  A slot's
// key never changes once written; live <-> tombstone moves only the tag, and
// both tags mean "compare the key", so a lane that probes past a slot another
// lane removes or revives sees either tag and decides the same.
//
// missing / need_transfer, lane per row on a fixed grid that strides: the
// row's group by a binary search on the segment offsets; a segmented form of
// k5_dedup_insert / _resolve (k8_live's) -- a power-of-two table of row
// indices, at most half full; a slot matches iff group, ID and size equal those
// of the row it names; the lowest row index wins -- gives Files() per group.  A
// row is FIRST iff it is its class's winner: the firsts are counted per group
// (64-bit integer adds: order-independent; a wave whose rows share one group
// adds once) and looked up by ID in the index.  The missing firsts are marked
// and listed by a tile mark / scan / scatter over the rows, so the list is
// ascending by group and by first occurrence, never arrival order.
#include "repo_internal.h"
#include "assoc_dev.h"  // kEmpty, key_hash, key_eq
#include "bloom_dev.h"
#include "reflow_hip.h"

namespace rf {

static_assert(kRepoListTile == 4 * kRepoBlock, "a list tile is one workgroup of four rows a lane");
static_assert(kRepoListTile == RF_REPO_LIST_TILE, "the header states the tile");

constexpr uint32_t kRepoMaxProbe = 1u << 16;
constexpr uint32_t kRepoTagEmpty = 0, kRepoTagBusy = 1, kRepoTagLive = 2, kRepoTagTomb = 3;
constexpr uint32_t kRepoClaim = 0x80000000u;  // slot_of: this launch claimed the slot

__device__ __forceinline__ uint32_t repo_wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint64_t repo_wave_sum64(uint64_t v) {
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    return v;
}
// Per-thread figures into the counter words: one add per wave and word.  Every lane of the wave calls this.
__device__ __forceinline__ void repo_ctr_add(unsigned long long* ctr, uint32_t word, uint64_t v) {
    v = repo_wave_sum64(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&ctr[word], (unsigned long long)v);
}

static uint32_t repo_grid(uint64_t items) {
    const uint64_t g = (items + kRepoBlock - 1) / kRepoBlock;
    return (uint32_t)(g < 1 ? 1 : g > 4096 ? 4096 : g);
}

// ---- rows and their dedup ----------------------------------------------------------
struct RepoRow {
    uint4 lo, hi;
    long long size;
};
__device__ __forceinline__ RepoRow repo_load_row(const RepoRows& r, uint32_t i) {
    const uint64_t src = r.row_src ? r.row_src[i] : (uint64_t)i;
    const uint4* d = reinterpret_cast<const uint4*>(r.ids + 32ull * src);
    RepoRow w;
    w.lo = d[0];
    w.hi = d[1];
    w.size = r.sizes ? r.sizes[src] : 0;
    return w;
}
__device__ __forceinline__ bool repo_id_eq(const RepoRow& a, const RepoRow& b) {
    return ((a.lo.x ^ b.lo.x) | (a.lo.y ^ b.lo.y) | (a.lo.z ^ b.lo.z) | (a.lo.w ^ b.lo.w) | (a.hi.x ^ b.hi.x) |
            (a.hi.y ^ b.hi.y) | (a.hi.z ^ b.hi.z) | (a.hi.w ^ b.hi.w)) == 0;
}
__device__ __forceinline__ uint32_t repo_row_hash(uint32_t ord, const RepoRow& w, bool by_size) {
    uint32_t h = key_hash(w.lo, w.hi);
    if (!by_size) return h;
    h ^= ord * 0x9E3779B1u;
    h ^= (uint32_t)w.size * 0x85EBCA77u;
    h ^= (uint32_t)((unsigned long long)w.size >> 32) * 0xC2B2AE3Du;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    return h;
}

// Insert row i; slot_of[i] = the slot that holds its class (~0: the probe bound;
// ~0 - 1: the row is left out).  A slot's value only ever moves from empty to a
// row index and then down (atomicMin), and every index a slot ever holds is of
// the slot's class, so a stale read of a non-empty slot still names the right
// class.
constexpr uint32_t kRepoLeftOut = 0xfffffffeu;
__global__ __launch_bounds__(kRepoBlock) void k9_dedup_insert(RepoRows r) {
    const bool by_size = r.by_size != 0;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; i0 < r.n_rows;
         i0 += (uint64_t)gridDim.x * kRepoBlock) {
        const uint32_t i = (uint32_t)i0;
        const uint32_t ord = r.row_ord ? r.row_ord[i] : 0u;
        const RepoRow w = repo_load_row(r, i);
        if (!by_size && w.size < 0) {
            r.slot_of[i] = kRepoLeftOut;
            continue;
        }
        uint32_t slot = repo_row_hash(ord, w, by_size) & r.mask;
        uint32_t probes = 0;
        for (;; ++probes) {
            if (probes >= kRepoMaxProbe) {  // bounded: every wave exits; the batch is flagged by its reader
                slot = kEmpty;
                break;
            }
            uint32_t cur = __hip_atomic_load(&r.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kEmpty) {
                cur = atomicCAS(&r.table[slot], kEmpty, i);
                if (cur == kEmpty) break;  // claimed: this row opens its class
            }
            if (cur >= r.n_rows) {  // not a row of this call: the table was not cleared
                slot = kEmpty;
                break;
            }
            const RepoRow c = repo_load_row(r, cur);
            if (repo_id_eq(w, c) && (!by_size || ((r.row_ord ? r.row_ord[cur] : 0u) == ord && c.size == w.size))) {
                if (i < cur) atomicMin(&r.table[slot], i);
                break;
            }
            slot = (slot + 1) & r.mask;
        }
        r.slot_of[i] = slot;
    }
}

__global__ __launch_bounds__(kRepoBlock) void k9_canon(RepoRows r, uint32_t* __restrict__ canon,
                                                       unsigned long long* __restrict__ ctr) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; i < r.n_rows;
         i += (uint64_t)gridDim.x * kRepoBlock) {
        const uint32_t so = r.slot_of[i];
        uint32_t c = kEmpty;
        if (so == kEmpty) bad = true;
        else if (so != kRepoLeftOut) c = r.table[so];
        canon[i] = c;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&ctr[kRepoFlags], (unsigned long long)kRepoFlagProbe);
}

// ---- the index ---------------------------------------------------------------------
// The slot of a live object with this ID, or kEmpty (absent, or a tombstone).  *probe_hit: the bound.
__device__ __forceinline__ uint32_t repo_find(const RepoView& t, const uint4& lo, const uint4& hi, bool* probe_hit) {
    uint32_t slot = key_hash(lo, hi) & t.mask;
    for (uint32_t probes = 0; probes < kRepoMaxProbe; ++probes) {
        const uint32_t tg = t.tag[slot];
        if (tg == kRepoTagEmpty) return kEmpty;
        if (tg != kRepoTagBusy && key_eq(&t.keys[2 * slot], lo, hi)) return tg == kRepoTagLive ? slot : kEmpty;
        slot = (slot + 1) & t.mask;
    }
    *probe_hit = true;
    return kEmpty;
}

// Put 1/2: the batch's DISTINCT IDs (canon[i] == i) find or claim their slot.
// New and revived objects get their size here; an object that is present keeps
// its own.  status of the distinct rows; slot_of[i] = the slot (kRepoClaim: claimed here).
__global__ __launch_bounds__(kRepoBlock) void k9_put_insert(RepoView t, RepoRows r, const uint32_t* __restrict__ canon,
                                                            int32_t* __restrict__ status) {
    uint64_t objs = 0, bytes = 0, revived = 0;
    bool bad = false;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; i0 < r.n_rows;
         i0 += (uint64_t)gridDim.x * kRepoBlock) {
        const uint32_t i = (uint32_t)i0;
        if (canon[i] != i) continue;
        const RepoRow w = repo_load_row(r, i);
        uint32_t slot = key_hash(w.lo, w.hi) & t.mask, mark = 0;
        int32_t st = RF_OK;
        uint32_t probes = 0;
        for (;; ++probes) {
            if (probes >= kRepoMaxProbe) {
                slot = 0;
                st = RF_EDEVICE;
                bad = true;
                break;
            }
            uint32_t tg = __hip_atomic_load(&t.tag[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (tg == kRepoTagEmpty) {
                tg = atomicCAS(&t.tag[slot], kRepoTagEmpty, kRepoTagBusy);
                if (tg == kRepoTagEmpty) {
                    t.keys[2 * slot] = w.lo;
                    t.keys[2 * slot + 1] = w.hi;
                    t.size[slot] = w.size;
                    ++objs;
                    bytes += (uint64_t)w.size;
                    mark = kRepoClaim;
                    break;
                }
            }
            // live and tombstone tags were set by earlier launches (or, for a key that is not this
            // lane's, move between the two in this one): their keys are visible and never change
            if ((tg == kRepoTagLive || tg == kRepoTagTomb) && key_eq(&t.keys[2 * slot], w.lo, w.hi)) {
                if (tg == kRepoTagTomb) {  // a fresh object of any size (only this lane has this ID)
                    t.size[slot] = w.size;
                    t.tag[slot] = kRepoTagLive;
                    ++objs;
                    ++revived;
                    bytes += (uint64_t)w.size;
                } else if (t.size[slot] != w.size) {
                    st = RF_EINTEGRITY;
                }
                break;
            }
            slot = (slot + 1) & t.mask;
        }
        r.slot_of[i] = slot | mark;
        status[i] = st;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&t.ctr[kRepoFlags], (unsigned long long)kRepoFlagProbe);
    repo_ctr_add(t.ctr, kRepoObjects, objs);
    repo_ctr_add(t.ctr, kRepoBytes, bytes);
    repo_ctr_add(t.ctr, kRepoTombs, (uint64_t)0 - revived);
}

// Put 2/2: the claims become live; a later row of an ID compares its size with the stored one.
__global__ __launch_bounds__(kRepoBlock) void k9_put_finish(RepoView t, RepoRows r, const uint32_t* __restrict__ canon,
                                                            int32_t* __restrict__ status) {
    for (uint64_t i0 = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; i0 < r.n_rows;
         i0 += (uint64_t)gridDim.x * kRepoBlock) {
        const uint32_t i = (uint32_t)i0;
        const uint32_t c = canon[i];
        if (c == kEmpty) {  // left out: a negative size (a row at the dedup's probe bound fails the call)
            status[i] = RF_EINVAL;
            continue;
        }
        if (c >= r.n_rows) continue;
        if (status[c] == RF_EDEVICE) {  // the insert gave up (status of a first row: written by the launch before)
            if (c != i) status[i] = RF_EDEVICE;
            continue;
        }
        const uint32_t so = r.slot_of[c];
        const uint32_t slot = so & ~kRepoClaim;
        if (c == i) {
            if (so & kRepoClaim) t.tag[slot] = kRepoTagLive;
            continue;
        }
        const uint64_t src = r.row_src ? r.row_src[i] : (uint64_t)i;
        status[i] = t.size[slot] == r.sizes[src] ? RF_OK : RF_EINTEGRITY;  // (sizes were written by the launch before)
    }
}

__global__ __launch_bounds__(kRepoBlock) void k9_remove(RepoView t, RepoRows r, const uint32_t* __restrict__ canon,
                                                        uint8_t* __restrict__ removed) {
    uint64_t objs = 0, bytes = 0;
    bool bad = false;
    for (uint64_t i0 = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; i0 < r.n_rows;
         i0 += (uint64_t)gridDim.x * kRepoBlock) {
        const uint32_t i = (uint32_t)i0;
        uint8_t gone = 0;
        if (canon[i] == i) {  // the first row of its ID; the others find it removed
            const RepoRow w = repo_load_row(r, i);
            const uint32_t slot = repo_find(t, w.lo, w.hi, &bad);
            if (slot != kEmpty) {
                t.tag[slot] = kRepoTagTomb;
                ++objs;
                bytes += (uint64_t)t.size[slot];
                gone = 1;
            }
        }
        removed[i] = gone;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&t.ctr[kRepoFlags], (unsigned long long)kRepoFlagProbe);
    repo_ctr_add(t.ctr, kRepoObjects, (uint64_t)0 - objs);
    repo_ctr_add(t.ctr, kRepoBytes, (uint64_t)0 - bytes);
    repo_ctr_add(t.ctr, kRepoTombs, objs);
}

__global__ __launch_bounds__(kRepoBlock) void k9_stat(RepoView t, const uint8_t* __restrict__ ids, uint64_t n,
                                                      long long* __restrict__ out) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kRepoBlock) {
        const uint4* k = reinterpret_cast<const uint4*>(ids + 32ull * i);
        const uint4 lo = k[0], hi = k[1];
        const uint32_t slot = repo_find(t, lo, hi, &bad);
        out[i] = slot == kEmpty ? -1ll : t.size[slot];
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&t.ctr[kRepoFlags], (unsigned long long)kRepoFlagProbe);
}

// Rebuild 1/2: every live object of `from` claims a slot of `to` (distinct keys: busy slots are skipped).
__global__ __launch_bounds__(kRepoBlock) void k9_rebuild(RepoView from, uint64_t from_slots, RepoView to) {
    bool bad = false;
    for (uint64_t q = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; q < from_slots;
         q += (uint64_t)gridDim.x * kRepoBlock) {
        if (from.tag[q] != kRepoTagLive) continue;
        const uint4 lo = from.keys[2 * q], hi = from.keys[2 * q + 1];
        uint32_t slot = key_hash(lo, hi) & to.mask;
        uint32_t probes = 0;
        for (;; ++probes) {
            if (probes >= kRepoMaxProbe) {
                bad = true;
                break;
            }
            if (atomicCAS(&to.tag[slot], kRepoTagEmpty, kRepoTagBusy) == kRepoTagEmpty) {
                to.keys[2 * slot] = lo;
                to.keys[2 * slot + 1] = hi;
                to.size[slot] = from.size[q];
                break;
            }
            slot = (slot + 1) & to.mask;
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&to.ctr[kRepoFlags], (unsigned long long)kRepoFlagProbe);
}
// Rebuild 2/2: the claims become live.
__global__ __launch_bounds__(kRepoBlock) void k9_rebuild_publish(RepoView to, uint64_t to_slots) {
    for (uint64_t q = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; q < to_slots;
         q += (uint64_t)gridDim.x * kRepoBlock)
        if (to.tag[q] == kRepoTagBusy) to.tag[q] = kRepoTagLive;
}

// Repository.Collect (repository/file/repository.go:304-327), lane per slot.
// The filter's length is read from the device (Add grows it there: k4_bloom_add), as every reader of a filter does.
__global__ __launch_bounds__(kRepoBlock) void k9_collect(RepoView t, uint64_t slots, bool all,
                                                         const uint64_t* __restrict__ words,
                                                         const uint64_t* __restrict__ len_dev, uint64_t m, uint64_t mu,
                                                         uint32_t k) {
    const uint64_t length = all ? 0 : *len_dev;
    uint64_t objs = 0, bytes = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; q < slots;
         q += (uint64_t)gridDim.x * kRepoBlock) {
        if (t.tag[q] != kRepoTagLive) continue;
        if (!all && bloom_contains(words, length, m, mu, k, reinterpret_cast<const uint8_t*>(&t.keys[2 * q]))) continue;
        t.tag[q] = kRepoTagTomb;
        ++objs;
        bytes += (uint64_t)t.size[q];
    }
    const uint64_t o = repo_wave_sum64(objs), b = repo_wave_sum64(bytes);
    if ((threadIdx.x & 63) == 0 && o) {
        atomicAdd(&t.ctr[kRepoGone], (unsigned long long)o);
        atomicAdd(&t.ctr[kRepoGoneBytes], (unsigned long long)b);
        atomicAdd(&t.ctr[kRepoObjects], (unsigned long long)((uint64_t)0 - o));
        atomicAdd(&t.ctr[kRepoBytes], (unsigned long long)((uint64_t)0 - b));
        atomicAdd(&t.ctr[kRepoTombs], (unsigned long long)o);
    }
}

// ---- exclusive scan of u32 counts into u64 offsets ---------------------------------
__device__ __forceinline__ uint32_t repo_cnt(const uint32_t* __restrict__ cnt, uint64_t n, uint64_t i) {
    return i < n ? cnt[i] : 0u;
}

// Scan 1/3: per tile of kRepoListTile counts, their sum.
__global__ __launch_bounds__(kRepoBlock) void k9_scan_tiles(const uint32_t* __restrict__ cnt, uint64_t n,
                                                            uint64_t* __restrict__ tile_sums) {
    __shared__ uint64_t s_sum[kRepoBlock / 64];
    const uint64_t first = ((uint64_t)blockIdx.x * kRepoBlock + threadIdx.x) * 4;
    uint64_t t = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) t += repo_cnt(cnt, n, first + j);
    t = repo_wave_sum64(t);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t c = 0;
        for (uint32_t k = 0; k < kRepoBlock / 64; ++k) c += s_sum[k];
        tile_sums[blockIdx.x] = c;
    }
}

// Scan 2/3: exclusive scan of the tile sums by one block, 1024 per pass; the total.
__global__ __launch_bounds__(1024) void k9_scan_top(uint64_t* __restrict__ tile_sums, uint64_t tiles,
                                                    uint64_t* __restrict__ off_end, uint64_t* __restrict__ total) {
    __shared__ uint64_t s_w[16];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t b = 0; b < tiles; b += 1024) {
        const uint64_t t = b + threadIdx.x;
        const uint64_t c = t < tiles ? tile_sums[t] : 0ull;
        uint64_t x = c;  // inclusive wave scan
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o, 64);
            if (lane >= (uint32_t)o) x += y;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        uint64_t before = 0, sum = 0;
        for (uint32_t w = 0; w < 16; ++w) {
            before += w < wave ? s_w[w] : 0ull;
            sum += s_w[w];
        }
        if (t < tiles) tile_sums[t] = carry + before + x - c;
        carry += sum;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *off_end = carry;
        if (total) *total = carry;
    }
}

// Scan 3/3: every entry's offset.
__global__ __launch_bounds__(kRepoBlock) void k9_scan_offsets(const uint32_t* __restrict__ cnt, uint64_t n,
                                                              const uint64_t* __restrict__ tile_sums,
                                                              uint64_t* __restrict__ off) {
    __shared__ uint64_t s_w[kRepoBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t first = ((uint64_t)blockIdx.x * kRepoBlock + threadIdx.x) * 4;
    uint32_t c4[4];
    uint64_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        c4[j] = repo_cnt(cnt, n, first + j);
        c += c4[j];
    }
    uint64_t x = c;  // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = (uint64_t)__shfl_up((unsigned long long)x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint64_t at = tile_sums[blockIdx.x] + x - c;
    for (uint32_t k = 0; k < wave; ++k) at += s_w[k];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        if (first + j < n) off[first + j] = at;
        at += c4[j];
    }
}

// ---- need_transfer's segments ------------------------------------------------------
__global__ __launch_bounds__(kRepoBlock) void k9_nt_degrees(LiveDev p, const uint32_t* __restrict__ nodes,
                                                            uint64_t n_groups, uint32_t* __restrict__ deg,
                                                            uint32_t* __restrict__ bad) {
    for (uint64_t g = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; g < n_groups;
         g += (uint64_t)gridDim.x * kRepoBlock) {
        const uint32_t node = nodes[g];
        uint64_t d = 0;
        uint32_t b = 0;
        if (node >= p.n) b = RF_EINVAL;
        else d = p.edge_ptr[node + 1] - p.edge_ptr[node];
        if (d > 0xffffffffull) {  // (edges are counted with 32 bits per node here)
            d = 0;
            b = RF_EINVAL;
        }
        deg[g] = (uint32_t)d;
        bad[g] = b;
    }
}

// the entry g of off[0 .. n] with off[g] <= i < off[g + 1] (entries of zero length own nothing; n >= 1, i < off[n])
__device__ __forceinline__ uint64_t repo_owner(const uint64_t* __restrict__ off, uint64_t n, uint64_t i) {
    uint64_t lo = 0, hi = n - 1;
    while (lo < hi) {  // the smallest g with off[g + 1] > i
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid + 1] <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kRepoBlock) void k9_nt_segments(LiveDev p, const uint32_t* __restrict__ nodes,
                                                             const uint64_t* __restrict__ seg_base, uint64_t n_groups,
                                                             uint64_t n_segs, uint32_t* __restrict__ seg_group,
                                                             uint64_t* __restrict__ seg_src,
                                                             uint32_t* __restrict__ seg_cnt, uint32_t* __restrict__ bad) {
    for (uint64_t q = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; q < n_segs;
         q += (uint64_t)gridDim.x * kRepoBlock) {
        const uint64_t g = repo_owner(seg_base, n_groups, q);
        const uint32_t node = nodes[g];  // (< n: a node out of range has no segments)
        const uint32_t dep = p.edges[p.edge_ptr[node] + (q - seg_base[g])];
        const bool has = dep < p.n && p.has[dep];
        seg_group[q] = (uint32_t)g;
        seg_src[q] = has ? p.val_off[dep] : 0ull;
        seg_cnt[q] = has ? p.val_cnt[dep] : 0u;
        if (!has) bad[g] = RF_EPRECONDITION;  // (every writer stores the same word)
    }
}
// a group with a dep that has no value contributes nothing
__global__ __launch_bounds__(kRepoBlock) void k9_nt_mask(const uint32_t* __restrict__ seg_group,
                                                         const uint32_t* __restrict__ bad,
                                                         uint32_t* __restrict__ seg_cnt, uint64_t n_segs) {
    for (uint64_t q = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; q < n_segs;
         q += (uint64_t)gridDim.x * kRepoBlock)
        if (bad[seg_group[q]]) seg_cnt[q] = 0;
}

__global__ __launch_bounds__(kRepoBlock) void k9_copy_status(const uint32_t* __restrict__ bad,
                                                             int32_t* __restrict__ status, uint64_t n_groups) {
    for (uint64_t g = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; g < n_groups;
         g += (uint64_t)gridDim.x * kRepoBlock)
        status[g] = (int32_t)bad[g];
}

// ---- missing: rows -----------------------------------------------------------------
__global__ __launch_bounds__(kRepoBlock) void k9_locate(const uint64_t* __restrict__ seg_off, uint64_t n_segs,
                                                        const uint32_t* __restrict__ seg_group,
                                                        const uint64_t* __restrict__ seg_src, uint32_t n_rows,
                                                        uint32_t* __restrict__ row_ord, uint64_t* __restrict__ row_src) {
    for (uint64_t i = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; i < n_rows;
         i += (uint64_t)gridDim.x * kRepoBlock) {
        const uint64_t g = repo_owner(seg_off, n_segs, i);
        row_ord[i] = seg_group ? seg_group[g] : (uint32_t)g;
        if (row_src) row_src[i] = (seg_src ? seg_src[g] : seg_off[g]) + (i - seg_off[g]);
    }
}

// The firsts of every class.  Rows are in group order, so a wave's 64 rows are
// mostly of one group: such a wave adds its sums once per figure; a wave that
// spans groups adds per lane (distinct addresses but for its two ends).
__global__ __launch_bounds__(kRepoBlock) void k9_resolve(RepoView t, RepoRows r, uint32_t* __restrict__ n_files,
                                                         uint32_t* __restrict__ n_missing,
                                                         unsigned long long* __restrict__ missing_bytes,
                                                         uint8_t* __restrict__ miss) {
    bool bad = false;
    uint64_t files = 0, missing = 0;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * kRepoBlock; base < r.n_rows; base += (uint64_t)gridDim.x * kRepoBlock) {
        const uint64_t i0 = base + threadIdx.x;
        const bool on = i0 < r.n_rows;
        const uint32_t i = (uint32_t)i0;
        uint32_t ord = 0, f = 0, m = 0;
        uint64_t b = 0;
        if (on) {
            ord = r.row_ord ? r.row_ord[i] : 0u;
            const uint32_t so = r.slot_of[i];
            if (so == kEmpty) {
                bad = true;
            } else if (r.table[so] == i) {
                const RepoRow w = repo_load_row(r, i);
                f = 1;
                if (repo_find(t, w.lo, w.hi, &bad) == kEmpty) {  // existence is by ID alone, as Stat
                    m = 1;
                    b = (uint64_t)w.size;
                    miss[i] = 1;
                }
            }
        }
        files += f;
        missing += m;
        const uint32_t ord0 = (uint32_t)__shfl((int)ord, 0, 64);  // (lane 0 is on whenever a lane of the wave is)
        if (__all(!on || ord == ord0)) {
            const uint32_t fs = repo_wave_sum(f), ms = repo_wave_sum(m);
            const uint64_t bs = repo_wave_sum64(b);
            if (lane == 0 && on) {
                if (fs) atomicAdd(&n_files[ord0], fs);
                if (ms) atomicAdd(&n_missing[ord0], ms);
                if (bs) atomicAdd(&missing_bytes[ord0], (unsigned long long)bs);
            }
        } else if (f) {
            atomicAdd(&n_files[ord], 1u);
            if (m) {
                atomicAdd(&n_missing[ord], 1u);
                if (b) atomicAdd(&missing_bytes[ord], (unsigned long long)b);
            }
        }
    }
    if (__any(bad) && lane == 0) atomicOr(&t.ctr[kRepoFlags], (unsigned long long)kRepoFlagProbe);
    repo_ctr_add(t.ctr, kRepoLastFiles, files);
    repo_ctr_add(t.ctr, kRepoLastMissing, missing);
}

// ---- missing: the list -------------------------------------------------------------
// A lane's four rows of tile blockIdx.x that are marked: a 4-bit mask (miss is padded to whole tiles).
__device__ __forceinline__ uint32_t repo_tile_mask(const uint8_t* __restrict__ miss, uint64_t first) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(miss + first);
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if ((v >> (8 * j)) & 0xffu) m |= 1u << j;
    return m;
}

__global__ __launch_bounds__(kRepoBlock) void k9_list_count(const uint8_t* __restrict__ miss,
                                                            uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t s_cnt[kRepoBlock / 64];
    const uint64_t first = ((uint64_t)blockIdx.x * kRepoBlock + threadIdx.x) * 4;
    const uint32_t cnt = repo_wave_sum((uint32_t)__builtin_popcount(repo_tile_mask(miss, first)));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < kRepoBlock / 64; ++k) c += s_cnt[k];
        tile_count[blockIdx.x] = c;
    }
}

// (after the tile scan) per tile, ascending row; ranks below cap are written
__global__ __launch_bounds__(kRepoBlock) void k9_list_scatter(RepoRows r, const uint8_t* __restrict__ miss,
                                                              const uint32_t* __restrict__ tile_count, uint64_t cap,
                                                              uint64_t* __restrict__ out_rows,
                                                              uint8_t* __restrict__ out_ids,
                                                              long long* __restrict__ out_sizes) {
    __shared__ uint32_t s_w[kRepoBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t rank = tile_count[blockIdx.x];  // (exclusive, after the tile scan)
    if (rank >= cap) return;                 // uniform over the block
    const uint64_t first = ((uint64_t)blockIdx.x * kRepoBlock + threadIdx.x) * 4;
    const uint32_t m = repo_tile_mask(miss, first);
    const uint32_t c = (uint32_t)__builtin_popcount(m);
    uint32_t x = c;  // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    for (uint32_t k = 0; k < wave; ++k) rank += s_w[k];
    rank += x - c;
    for (uint32_t q = m; q && rank < cap; q &= q - 1, ++rank) {
        const uint64_t i = first + (uint32_t)__builtin_ctz(q);
        if (i >= r.n_rows) break;  // (never: rows beyond the last are not marked)
        const uint64_t src = r.row_src ? r.row_src[i] : i;
        if (out_rows) out_rows[rank] = i;
        if (out_ids) {
            const uint4* d = reinterpret_cast<const uint4*>(r.ids + 32ull * src);
            uint4* o = reinterpret_cast<uint4*>(out_ids + 32ull * rank);
            o[0] = d[0];
            o[1] = d[1];
        }
        if (out_sizes) out_sizes[rank] = r.sizes[src];
    }
}

// ---- the index read back: scan, collect with names, bulk load ----------------------
// A tile is kRepoListTile slots, one workgroup, four slots a lane (slot counts
// are powers of two >= 1024: tiles are whole).  The lane's 4-bit mask of slots
// whose tag is live:
__device__ __forceinline__ uint32_t repo_live_mask(const uint32_t* __restrict__ tag, uint64_t first) {
    const uint4 t = *reinterpret_cast<const uint4*>(tag + first);
    return (t.x == kRepoTagLive ? 1u : 0u) | (t.y == kRepoTagLive ? 2u : 0u) | (t.z == kRepoTagLive ? 4u : 0u) |
           (t.w == kRepoTagLive ? 8u : 0u);
}

// the block's sum of one figure per lane into tile_count[blockIdx.x]
__device__ __forceinline__ void repo_tile_total(uint32_t v, uint32_t* __restrict__ tile_count) {
    __shared__ uint32_t s_cnt[kRepoBlock / 64];
    const uint32_t cnt = repo_wave_sum(v);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < kRepoBlock / 64; ++k) c += s_cnt[k];
        tile_count[blockIdx.x] = c;
    }
}

// the rank of the lane's first marked slot: the tile's offset, the waves before (LDS) and the lanes before
__device__ __forceinline__ uint64_t repo_tile_rank(uint64_t tile_off, uint32_t c) {
    __shared__ uint32_t s_w[kRepoBlock / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = c;  // inclusive wave scan
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= (uint32_t)o) x += y;
    }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint64_t rank = tile_off + (x - c);
    for (uint32_t k = 0; k < wave; ++k) rank += s_w[k];
    return rank;
}

__device__ __forceinline__ void repo_write_row(const RepoView& t, uint64_t q, uint64_t rank,
                                               uint8_t* __restrict__ out_ids, long long* __restrict__ out_sizes) {
    if (out_ids) {
        uint4* o = reinterpret_cast<uint4*>(out_ids + 32ull * rank);
        o[0] = t.keys[2 * q];
        o[1] = t.keys[2 * q + 1];
    }
    if (out_sizes) out_sizes[rank] = t.size[q];
}

// Scan 1/3: live tags per tile.
__global__ __launch_bounds__(kRepoBlock) void k9_index_count(RepoView t, uint32_t* __restrict__ tile_count) {
    const uint64_t first = ((uint64_t)blockIdx.x * kRepoBlock + threadIdx.x) * 4;
    repo_tile_total((uint32_t)__builtin_popcount(repo_live_mask(t.tag, first)), tile_count);
}

// Scan 3/3 (after launch_repo_scan over the tile counts): per tile, ascending slot; ranks below cap are written.
__global__ __launch_bounds__(kRepoBlock) void k9_index_scatter(RepoView t, const uint64_t* __restrict__ tile_off,
                                                               uint64_t cap, uint8_t* __restrict__ out_ids,
                                                               long long* __restrict__ out_sizes) {
    const uint64_t base = tile_off[blockIdx.x];
    if (base >= cap) return;  // uniform over the block
    const uint64_t first = ((uint64_t)blockIdx.x * kRepoBlock + threadIdx.x) * 4;
    const uint32_t m = repo_live_mask(t.tag, first);
    uint64_t rank = repo_tile_rank(base, (uint32_t)__builtin_popcount(m));
    for (uint32_t q = m; q && rank < cap; q &= q - 1, ++rank)
        repo_write_row(t, first + (uint32_t)__builtin_ctz(q), rank, out_ids, out_sizes);
}

// Collect with names 1/3, the mark: a slot is dead when it is live and the
// filter does not hold its ID (or there is no filter).  The filter is probed
// here, once per object; nothing is removed.  dead: a byte per slot.
__global__ __launch_bounds__(kRepoBlock) void k9_collect_mark(RepoView t, bool all,
                                                              const uint64_t* __restrict__ words,
                                                              const uint64_t* __restrict__ len_dev, uint64_t m,
                                                              uint64_t mu, uint32_t k, uint8_t* __restrict__ dead,
                                                              uint32_t* __restrict__ tile_count) {
    const uint64_t length = all ? 0 : *len_dev;
    const uint64_t first = ((uint64_t)blockIdx.x * kRepoBlock + threadIdx.x) * 4;
    const uint32_t live = repo_live_mask(t.tag, first);
    uint32_t bytes4 = 0, c = 0;
    for (uint32_t q = live; q; q &= q - 1) {
        const uint32_t j = (uint32_t)__builtin_ctz(q);
        if (!all && bloom_contains(words, length, m, mu, k, reinterpret_cast<const uint8_t*>(&t.keys[2 * (first + j)])))
            continue;
        bytes4 |= 1u << (8 * j);
        ++c;
    }
    *reinterpret_cast<uint32_t*>(dead + first) = bytes4;
    repo_tile_total(c, tile_count);
}

// Collect with names 3/3, the apply (after launch_repo_scan over the tile
// counts): all or nothing on the scanned total, read from device memory by
// every workgroup alike.  The dead slots become tombstones, their rows go to
// their ranks, and the counters move as k9_collect moves them: a fixed grid
// that strides over the tiles, one add per wave and word at the end (a
// workgroup per tile adding as it goes is 2.6M adds to five addresses at 2^25
// slots: the call measured 8.5 ms that way and 1.3 ms this way).
__global__ __launch_bounds__(kRepoBlock) void k9_collect_apply(RepoView t, uint64_t tiles,
                                                               const uint8_t* __restrict__ dead,
                                                               const uint64_t* __restrict__ tile_off,
                                                               const uint64_t* __restrict__ total, uint64_t cap,
                                                               uint8_t* __restrict__ out_ids,
                                                               long long* __restrict__ out_sizes) {
    if (*total > cap) return;  // uniform over the grid: nothing is removed, no counter moves
    uint64_t objs = 0, bytes = 0;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform over the block)
        const uint64_t first = (tile * kRepoBlock + threadIdx.x) * 4;
        const uint32_t m = repo_tile_mask(dead, first);
        const uint32_t c = (uint32_t)__builtin_popcount(m);
        uint64_t rank = repo_tile_rank(tile_off[tile], c);
        for (uint32_t q = m; q; q &= q - 1, ++rank) {
            const uint64_t slot = first + (uint32_t)__builtin_ctz(q);
            if (rank < cap) repo_write_row(t, slot, rank, out_ids, out_sizes);
            t.tag[slot] = kRepoTagTomb;
            bytes += (uint64_t)t.size[slot];
        }
        objs += c;
        __syncthreads();  // the next tile reuses the waves' sums in LDS
    }
    const uint64_t o = repo_wave_sum64(objs), b = repo_wave_sum64(bytes);
    if ((threadIdx.x & 63) == 0 && o) {
        atomicAdd(&t.ctr[kRepoGone], (unsigned long long)o);
        atomicAdd(&t.ctr[kRepoGoneBytes], (unsigned long long)b);
        atomicAdd(&t.ctr[kRepoObjects], (unsigned long long)((uint64_t)0 - o));
        atomicAdd(&t.ctr[kRepoBytes], (unsigned long long)((uint64_t)0 - b));
        atomicAdd(&t.ctr[kRepoTombs], (unsigned long long)o);
    }
}

// Bulk load 1/2 (rf_repo_restore): n dense objects with DISTINCT IDs (the
// file's order was checked on the host) claim a slot of the empty table `to` --
// k9_rebuild's protocol, no dedup pass; k9_rebuild_publish is 2/2.
__global__ __launch_bounds__(kRepoBlock) void k9_load(const uint8_t* __restrict__ ids,
                                                      const long long* __restrict__ sizes, uint64_t n, RepoView to) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kRepoBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kRepoBlock) {
        const uint4* d = reinterpret_cast<const uint4*>(ids + 32ull * i);
        const uint4 lo = d[0], hi = d[1];
        uint32_t slot = key_hash(lo, hi) & to.mask;
        uint32_t probes = 0;
        for (;; ++probes) {
            if (probes >= kRepoMaxProbe) {
                bad = true;
                break;
            }
            if (atomicCAS(&to.tag[slot], kRepoTagEmpty, kRepoTagBusy) == kRepoTagEmpty) {
                to.keys[2 * slot] = lo;
                to.keys[2 * slot + 1] = hi;
                to.size[slot] = sizes[i];
                break;
            }
            slot = (slot + 1) & to.mask;
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&to.ctr[kRepoFlags], (unsigned long long)kRepoFlagProbe);
}

// ---- launches ----------------------------------------------------------------------
hipError_t launch_repo_index_count(const RepoView& t, uint64_t slots, uint32_t* tile_count, uint64_t* tile_sums,
                                   uint64_t* tile_off, uint64_t* d_total, hipStream_t s) {
    const uint64_t tiles = slots / kRepoListTile;
    hipLaunchKernelGGL(k9_index_count, dim3((uint32_t)tiles), dim3(kRepoBlock), 0, s, t, tile_count);
    return launch_repo_scan(tile_count, tiles, tile_sums, tile_off, d_total, s);
}

hipError_t launch_repo_index_scatter(const RepoView& t, uint64_t slots, const uint64_t* tile_off, uint64_t cap,
                                     uint8_t* out_ids, int64_t* out_sizes, hipStream_t s) {
    if (!cap || !(out_ids || out_sizes)) return hipSuccess;
    hipLaunchKernelGGL(k9_index_scatter, dim3((uint32_t)(slots / kRepoListTile)), dim3(kRepoBlock), 0, s, t, tile_off,
                       cap, out_ids, reinterpret_cast<long long*>(out_sizes));
    return hipGetLastError();
}

hipError_t launch_repo_collect_mark(const RepoView& t, uint64_t slots, const BloomDev* live, uint8_t* dead,
                                    uint32_t* tile_count, uint64_t* tile_sums, uint64_t* tile_off, uint64_t* d_total,
                                    hipStream_t s) {
    hipError_t e = hipMemsetAsync(t.ctr + kRepoGone, 0, 16, s);
    if (e != hipSuccess) return e;
    const uint64_t tiles = slots / kRepoListTile;
    const bool all = live == nullptr;
    hipLaunchKernelGGL(k9_collect_mark, dim3((uint32_t)tiles), dim3(kRepoBlock), 0, s, t, all,
                       all ? nullptr : live->words, all ? nullptr : live->len_dev, all ? 1ull : live->m,
                       all || !live->m ? 0ull : (~0ull) / live->m, all ? 0u : (uint32_t)live->k, dead, tile_count);
    return launch_repo_scan(tile_count, tiles, tile_sums, tile_off, d_total, s);
}

hipError_t launch_repo_collect_apply(const RepoView& t, uint64_t slots, const uint8_t* dead, const uint64_t* tile_off,
                                     const uint64_t* d_total, uint64_t cap, uint8_t* out_ids, int64_t* out_sizes,
                                     hipStream_t s) {
    const uint64_t tiles = slots / kRepoListTile;  // a fixed grid that strides: one add per wave and counter word
    hipLaunchKernelGGL(k9_collect_apply, dim3((uint32_t)std::min<uint64_t>(tiles, 2048)), dim3(kRepoBlock), 0, s, t,
                       tiles, dead, tile_off, d_total, cap, out_ids, reinterpret_cast<long long*>(out_sizes));
    return hipGetLastError();
}

hipError_t launch_repo_load(const uint8_t* ids, const int64_t* sizes, uint64_t n, const RepoView& to,
                            uint64_t to_slots, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k9_load, dim3(repo_grid(n)), dim3(kRepoBlock), 0, s, ids, reinterpret_cast<const long long*>(sizes),
                       n, to);
    hipLaunchKernelGGL(k9_rebuild_publish, dim3(repo_grid(to_slots)), dim3(kRepoBlock), 0, s, to, to_slots);
    return hipGetLastError();
}

hipError_t launch_repo_dedup(const RepoRows& r, hipStream_t s) {
    if (!r.n_rows) return hipSuccess;
    hipError_t e = hipMemsetAsync(r.table, 0xff, 4ull * ((uint64_t)r.mask + 1), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k9_dedup_insert, dim3(repo_grid(r.n_rows)), dim3(kRepoBlock), 0, s, r);
    return hipGetLastError();
}

hipError_t launch_repo_canon(const RepoRows& r, uint32_t* canon, unsigned long long* ctr, hipStream_t s) {
    if (!r.n_rows) return hipSuccess;
    hipLaunchKernelGGL(k9_canon, dim3(repo_grid(r.n_rows)), dim3(kRepoBlock), 0, s, r, canon, ctr);
    return hipGetLastError();
}

hipError_t launch_repo_put(const RepoView& t, const RepoRows& r, const uint32_t* canon, int32_t* status,
                           hipStream_t s) {
    if (!r.n_rows) return hipSuccess;
    const uint32_t grid = repo_grid(r.n_rows);
    hipLaunchKernelGGL(k9_put_insert, dim3(grid), dim3(kRepoBlock), 0, s, t, r, canon, status);
    hipLaunchKernelGGL(k9_put_finish, dim3(grid), dim3(kRepoBlock), 0, s, t, r, canon, status);
    return hipGetLastError();
}

hipError_t launch_repo_remove(const RepoView& t, const RepoRows& r, const uint32_t* canon, uint8_t* removed,
                              hipStream_t s) {
    if (!r.n_rows) return hipSuccess;
    hipLaunchKernelGGL(k9_remove, dim3(repo_grid(r.n_rows)), dim3(kRepoBlock), 0, s, t, r, canon, removed);
    return hipGetLastError();
}

hipError_t launch_repo_stat(const RepoView& t, const uint8_t* ids, uint64_t n, int64_t* sizes_out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k9_stat, dim3(repo_grid(n)), dim3(kRepoBlock), 0, s, t, ids, n,
                       reinterpret_cast<long long*>(sizes_out));
    return hipGetLastError();
}

hipError_t launch_repo_rebuild(const RepoView& from, uint64_t from_slots, const RepoView& to, uint64_t to_slots,
                               hipStream_t s) {
    hipLaunchKernelGGL(k9_rebuild, dim3(repo_grid(from_slots)), dim3(kRepoBlock), 0, s, from, from_slots, to);
    hipLaunchKernelGGL(k9_rebuild_publish, dim3(repo_grid(to_slots)), dim3(kRepoBlock), 0, s, to, to_slots);
    return hipGetLastError();
}

hipError_t launch_repo_collect(const RepoView& t, uint64_t slots, const BloomDev* live, hipStream_t s) {
    hipError_t e = hipMemsetAsync(t.ctr + kRepoGone, 0, 16, s);
    if (e != hipSuccess) return e;
    const bool all = live == nullptr;
    hipLaunchKernelGGL(k9_collect, dim3(repo_grid(slots)), dim3(kRepoBlock), 0, s, t, slots, all,
                       all ? nullptr : live->words, all ? nullptr : live->len_dev, all ? 1ull : live->m,
                       all || !live->m ? 0ull : (~0ull) / live->m, all ? 0u : (uint32_t)live->k);
    return hipGetLastError();
}

hipError_t launch_repo_scan(const uint32_t* cnt, uint64_t n, uint64_t* tile_sums, uint64_t* off, uint64_t* total,
                            hipStream_t s) {
    const uint64_t tiles = (n + kRepoListTile - 1) / kRepoListTile;
    if (tiles) hipLaunchKernelGGL(k9_scan_tiles, dim3((uint32_t)tiles), dim3(kRepoBlock), 0, s, cnt, n, tile_sums);
    hipLaunchKernelGGL(k9_scan_top, dim3(1), dim3(1024), 0, s, tile_sums, tiles, off + n, total);
    if (tiles) hipLaunchKernelGGL(k9_scan_offsets, dim3((uint32_t)tiles), dim3(kRepoBlock), 0, s, cnt, n, tile_sums, off);
    return hipGetLastError();
}

hipError_t launch_repo_nt_degrees(const LiveDev& d, const uint32_t* nodes, uint64_t n_groups, uint32_t* deg,
                                  uint32_t* bad, hipStream_t s) {
    if (!n_groups) return hipSuccess;
    hipLaunchKernelGGL(k9_nt_degrees, dim3(repo_grid(n_groups)), dim3(kRepoBlock), 0, s, d, nodes, n_groups, deg, bad);
    return hipGetLastError();
}

hipError_t launch_repo_nt_segments(const LiveDev& d, const uint32_t* nodes, const uint64_t* seg_base,
                                   uint64_t n_groups, uint64_t n_segs, uint32_t* seg_group, uint64_t* seg_src,
                                   uint32_t* seg_cnt, uint32_t* bad, hipStream_t s) {
    if (!n_segs || !n_groups) return hipSuccess;
    const uint32_t grid = repo_grid(n_segs);
    hipLaunchKernelGGL(k9_nt_segments, dim3(grid), dim3(kRepoBlock), 0, s, d, nodes, seg_base, n_groups, n_segs,
                       seg_group, seg_src, seg_cnt, bad);
    hipLaunchKernelGGL(k9_nt_mask, dim3(grid), dim3(kRepoBlock), 0, s, seg_group, bad, seg_cnt, n_segs);
    return hipGetLastError();
}

hipError_t launch_repo_locate(const uint64_t* seg_off, uint64_t n_segs, const uint32_t* seg_group,
                              const uint64_t* seg_src, uint32_t n_rows, uint32_t* row_ord, uint64_t* row_src,
                              hipStream_t s) {
    if (!n_rows || !n_segs) return hipSuccess;
    hipLaunchKernelGGL(k9_locate, dim3(repo_grid(n_rows)), dim3(kRepoBlock), 0, s, seg_off, n_segs, seg_group, seg_src,
                       n_rows, row_ord, row_src);
    return hipGetLastError();
}

hipError_t launch_repo_resolve(const RepoView& t, const RepoRows& r, uint32_t* n_files, uint32_t* n_missing,
                               unsigned long long* missing_bytes, uint8_t* miss, hipStream_t s) {
    if (!r.n_rows) return hipSuccess;
    const uint32_t grid = repo_grid(r.n_rows);
    hipLaunchKernelGGL(k9_resolve, dim3(grid < 2048 ? grid : 2048), dim3(kRepoBlock), 0, s, t, r, n_files, n_missing,
                       missing_bytes, miss);
    return hipGetLastError();
}

hipError_t launch_repo_list(const RepoRows& r, const uint8_t* miss, uint32_t* tile_count, uint64_t cap,
                            uint64_t* out_rows, uint8_t* out_ids, int64_t* out_sizes, uint64_t* d_total,
                            hipStream_t s) {
    const uint64_t tiles = ((uint64_t)r.n_rows + kRepoListTile - 1) / kRepoListTile;
    if (tiles) hipLaunchKernelGGL(k9_list_count, dim3((uint32_t)tiles), dim3(kRepoBlock), 0, s, miss, tile_count);
    hipError_t e = launch_tile_scan(tile_count, tiles, d_total, s);
    if (e != hipSuccess) return e;
    if (tiles && cap && (out_rows || out_ids || out_sizes))
        hipLaunchKernelGGL(k9_list_scatter, dim3((uint32_t)tiles), dim3(kRepoBlock), 0, s, r, miss, tile_count, cap,
                           out_rows, out_ids, reinterpret_cast<long long*>(out_sizes));
    return hipGetLastError();
}

hipError_t launch_repo_copy_status(const uint32_t* bad, int32_t* status, uint64_t n_groups, hipStream_t s) {
    if (!n_groups) return hipSuccess;
    hipLaunchKernelGGL(k9_copy_status, dim3(repo_grid(n_groups)), dim3(kRepoBlock), 0, s, bad, status, n_groups);
    return hipGetLastError();
}

}  // namespace rf
