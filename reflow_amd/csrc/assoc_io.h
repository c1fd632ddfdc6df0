// assoc_io.h -- internal: the HBM assoc's file form (assoc_io.cpp), host-only.
// No HIP; the sanitizer build (make asan_assoc) links these units alone.
#pragma once
#include <stdint.h>

#include <functional>

#include "reflow_hip.h"

namespace rf {

constexpr uint64_t kAssocHeader = 64, kAssocEntry = 68, kAssocTrailer = 40;
constexpr uint64_t kAssocChunk = 64ull << 20;   // the default checksum granule
constexpr uint64_t kAssocMaxEntries = 1ull << 30;  // a table has at most 2^31 slots, half full

// out[32 c ..] = SHA-256 of the c-th `chunk` bytes of buf[0, n) (host_par.h's
// hash_chunks: the callers with a context pass one that runs on its pool)
using ChunkHasher = std::function<void(const uint8_t* buf, uint64_t n, uint64_t chunk, uint8_t* out)>;
void assoc_hash_serial(const uint8_t* buf, uint64_t n, uint64_t chunk, uint8_t* out);

// Bytes of a file of n entries (chunk > 0).
uint64_t assoc_file_bytes(uint64_t n, uint64_t chunk);
// (kind, key bytes) order of two entries of the dense arrays
bool assoc_entry_less(const int32_t* kinds, const uint8_t* keys32, uint64_t a, uint64_t b);
// The file of the n entries taken in the order perm[0 .. n) (null: as given)
// into out[assoc_file_bytes(n, chunk)].  RF_EINVAL unless, in that order, the
// entries are strictly ascending with kinds in [0, 2^30) and nonzero values.
int assoc_file_write(const int32_t* kinds, const uint8_t* keys32, const uint8_t* vals32, const uint32_t* perm,
                     uint64_t n, uint64_t chunk, uint8_t* out, const ChunkHasher& hash);
// Every check of a file, reading buf[0, len) only: structure (RF_EINVAL),
// checksums (RF_EINTEGRITY), then the entries (RF_EINVAL).  *n = its entries.
int assoc_file_check(const uint8_t* buf, uint64_t len, uint64_t* n, const ChunkHasher& hash);
// The entries of a checked file into the dense arrays.
void assoc_file_unpack(const uint8_t* buf, uint64_t n, int32_t* kinds, uint8_t* keys32, uint8_t* vals32);

}  // namespace rf
