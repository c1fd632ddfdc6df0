// assoc_dev.h -- the HBM assoc's device-side key lookup (moved unchanged out
// of k5_table.hip), shared by the K5 kernels and the change feed's fused
// lookup (k6_feed.hip).  Device code only; not part of the public ABI.
#pragma once
#include "engine.h"

namespace rf {

constexpr uint32_t kEmpty = 0xffffffffu;

// 32-bit slot hash over all eight words of a 32-B key.  Each word enters
// through an xor with a rotated partner and an odd multiply (bijections), so
// two keys that differ in any single word never share a pre-finaliser value,
// and the finaliser (also a bijection) spreads them over the low bits.  Keys
// are usually SHA-256 output (any word would do), but callers may hand in
// digests that share all but a few bytes.
__device__ __forceinline__ uint32_t key_hash(const uint4& lo, const uint4& hi) {
    uint32_t h = ((lo.x ^ __builtin_rotateleft32(lo.y, 5)) * 0x9E3779B1u) ^
                 ((lo.z ^ __builtin_rotateleft32(lo.w, 11)) * 0x85EBCA77u) ^
                 ((hi.x ^ __builtin_rotateleft32(hi.y, 17)) * 0xC2B2AE3Du) ^
                 ((hi.z ^ __builtin_rotateleft32(hi.w, 23)) * 0x27D4EB2Fu);
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    return h;
}

// Deleted entries keep their slot with a zero value (Get: NotExist).
constexpr uint32_t kTagEmpty = 0, kTagBusy = 1, kTagReady = 2;

__device__ __forceinline__ bool key_eq(const uint4* k, const uint4& lo, const uint4& hi) {
    const uint4 a = k[0], b = k[1];
    return ((a.x ^ lo.x) | (a.y ^ lo.y) | (a.z ^ lo.z) | (a.w ^ lo.w) | (b.x ^ hi.x) | (b.y ^ hi.y) |
            (b.z ^ hi.z) | (b.w ^ hi.w)) == 0;
}

__device__ __forceinline__ uint32_t assoc_find(const AssocView& t, uint32_t kind, const uint4& lo, const uint4& hi) {
    const uint32_t ready = kTagReady + kind;
    uint32_t slot = key_hash(lo, hi) & t.mask;
    for (;;) {
        const uint32_t tg = t.tag[slot];
        if (tg == kTagEmpty) return kEmpty;
        if (tg == ready && key_eq(&t.keys[2 * slot], lo, hi)) return slot;
        slot = (slot + 1) & t.mask;
    }
}

}  // namespace rf
