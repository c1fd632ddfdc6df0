// repo_io.h -- internal: the repository index's file form (repo_io.cpp),
// host-only.  No HIP; the sanitizer build (make asan_repo) links these units alone.
#pragma once
#include <stdint.h>

#include "assoc_io.h"  // ChunkHasher
#include "reflow_hip.h"

namespace rf {

constexpr uint64_t kRepoFileHeader = 64, kRepoFileEntry = 40, kRepoFileTrailer = 40;
constexpr uint64_t kRepoFileChunk = 64ull << 20;      // the default checksum granule
constexpr uint64_t kRepoFileMaxEntries = 1ull << 30;  // the capacity rf_repo_new accepts (repo_check.h)

void repo_hash_serial(const uint8_t* buf, uint64_t n, uint64_t chunk, uint8_t* out);

// Bytes of a file of n entries (chunk > 0, n <= kRepoFileMaxEntries).
uint64_t repo_file_bytes(uint64_t n, uint64_t chunk);
// The file of the n objects taken in the order perm[0 .. n) (null: as given)
// into out[repo_file_bytes(n, chunk)].  RF_EINVAL unless, in that order, the
// IDs are strictly ascending, no size is negative and the sizes sum within int64.
int repo_file_write(const uint8_t* ids32, const int64_t* sizes, const uint32_t* perm, uint64_t n, uint64_t chunk,
                    uint8_t* out, const ChunkHasher& hash);
// Every check of a file, reading buf[0, len) only: structure (RF_EINVAL),
// checksums (RF_EINTEGRITY), then the entries (RF_EINVAL).  *n = its entries,
// *total_bytes (may be null) = the sum of their sizes.
int repo_file_check(const uint8_t* buf, uint64_t len, uint64_t* n, int64_t* total_bytes, const ChunkHasher& hash);
// The entries of a checked file into the dense arrays.
void repo_file_unpack(const uint8_t* buf, uint64_t n, uint8_t* ids32, int64_t* sizes);

}  // namespace rf
