// repo_io.cpp -- the repository index's file form (rf_repo_save /
// rf_repo_restore, repo.cpp) on the host alone: format, check and parse.  No HIP.
//
// Reference: a repository outlives the run that filled it
// (repository/file/repository.go:29-47: a directory of objects named by their
// digests); the index is what a process keeps of it in HBM, and the file is what
// it writes so that the next process need not walk the directory and Stat every
// object (repository.go:93-101) before its first missing() is answered.
//
// File, little-endian (the assoc file's layout, assoc_io.cpp):
//   header, 64 B   magic "RFREPO01", u32 version = 1, u32 flags = 0,
//                  u64 n_entries, u64 chunk, i64 total_bytes (the sum of the
//                  sizes), 24 zero bytes
//   entries, 40 B  32-B ID, i64 size >= 0 -- the live objects only, strictly
//                  ascending by ID bytes: equal contents give equal files
//                  whatever the table's history or capacity
//   chunk digests  one SHA-256 per `chunk` bytes of the entry area
//   trailer, 40 B  SHA-256(header || chunk digests), end marker "RFREEND1"
// A mismatch of a checksum is RF_EINTEGRITY (errors.Integrity,
// repository/file/repository.go:160-162); anything else wrong is RF_EINVAL.
#include "repo_io.h"

#include <string.h>

#include <algorithm>
#include <vector>

#include "errors.h"
#include "host_par.h"

namespace rf {

namespace {

constexpr char kMagic[8] = {'R', 'F', 'R', 'E', 'P', 'O', '0', '1'};
constexpr char kEnd[8] = {'R', 'F', 'R', 'E', 'E', 'N', 'D', '1'};
constexpr uint32_t kVersion = 1;

struct Header {
    char magic[8];
    uint32_t version, flags;
    uint64_t n_entries, chunk;
    int64_t total_bytes;
    uint8_t zero[24];
};
static_assert(sizeof(Header) == kRepoFileHeader, "header layout");

struct NoPool {  // hash_chunks on the caller
    unsigned size() const { return 0; }
    template <class F>
    void run(const F&) {}
};

// (no area + chunk: a file may name any granule)
uint64_t n_chunks(uint64_t n, uint64_t chunk) { return n ? (kRepoFileEntry * n - 1) / chunk + 1 : 0; }

// header || chunk digests -> root
void root_digest(const Header& h, const uint8_t* digests, uint64_t nc, uint8_t root[32]) {
    std::vector<uint8_t> all(sizeof h + 32 * nc);
    memcpy(all.data(), &h, sizeof h);
    if (nc) memcpy(all.data() + sizeof h, digests, 32 * nc);
    host_sha256(all.data(), all.size(), root);
}

// entry records: e[0..32) ID, e[32..40) size.  *total = the sum of the sizes.
int check_records(const uint8_t* e, uint64_t n, int64_t* total) {
    int64_t sum = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* r = e + kRepoFileEntry * i;
        int64_t size;
        memcpy(&size, r + 32, 8);
        if (size < 0) return fail(RF_EINVAL, "repo file: entry %llu has a negative size", (unsigned long long)i);
        if (size > INT64_MAX - sum)
            return fail(RF_EINVAL, "repo file: the sizes up to entry %llu overflow int64", (unsigned long long)i);
        sum += size;
        if (i && memcmp(r - kRepoFileEntry, r, 32) >= 0)
            return fail(RF_EINVAL, "repo file: entry %llu is not above its predecessor in ID order",
                        (unsigned long long)i);
    }
    *total = sum;
    return RF_OK;
}

}  // namespace

void repo_hash_serial(const uint8_t* buf, uint64_t n, uint64_t chunk, uint8_t* out) {
    hash_chunks(static_cast<NoPool*>(nullptr), buf, n, chunk, out);
}

uint64_t repo_file_bytes(uint64_t n, uint64_t chunk) {
    return kRepoFileHeader + kRepoFileEntry * n + 32 * n_chunks(n, chunk) + kRepoFileTrailer;
}

int repo_file_write(const uint8_t* ids32, const int64_t* sizes, const uint32_t* perm, uint64_t n, uint64_t chunk,
                    uint8_t* out, const ChunkHasher& hash) {
    uint8_t* e = out + kRepoFileHeader;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t s = perm ? perm[i] : i;
        uint8_t* r = e + kRepoFileEntry * i;
        memcpy(r, ids32 + 32 * s, 32);
        memcpy(r + 32, &sizes[s], 8);
    }
    Header h{};
    memcpy(h.magic, kMagic, 8);
    h.version = kVersion;
    h.n_entries = n;
    h.chunk = chunk;
    if (int rc = check_records(e, n, &h.total_bytes)) return rc;
    memcpy(out, &h, sizeof h);
    const uint64_t nc = n_chunks(n, chunk);
    uint8_t* d = e + kRepoFileEntry * n;
    hash(e, kRepoFileEntry * n, chunk, d);
    root_digest(h, d, nc, d + 32 * nc);
    memcpy(d + 32 * nc + 32, kEnd, 8);
    return RF_OK;
}

int repo_file_check(const uint8_t* buf, uint64_t len, uint64_t* n_out, int64_t* total_out, const ChunkHasher& hash) {
    if (len < kRepoFileHeader + kRepoFileTrailer)
        return fail(RF_EINVAL, "repo file: %llu bytes is too short", (unsigned long long)len);
    Header h;
    memcpy(&h, buf, sizeof h);
    if (memcmp(h.magic, kMagic, 8) != 0) return fail(RF_EINVAL, "repo file: bad magic");
    if (h.version != kVersion) return fail(RF_EINVAL, "repo file: version %u not supported", h.version);
    if (h.flags != 0) return fail(RF_EINVAL, "repo file: unknown flags %#x", h.flags);
    if (h.chunk == 0) return fail(RF_EINVAL, "repo file: zero checksum granule");
    for (uint8_t z : h.zero)
        if (z) return fail(RF_EINVAL, "repo file: nonzero reserved bytes");
    const uint64_t n = h.n_entries;
    if (n > kRepoFileMaxEntries || n > (len - kRepoFileHeader - kRepoFileTrailer) / kRepoFileEntry)
        return fail(RF_EINVAL, "repo file: %llu entries do not fit its %llu bytes", (unsigned long long)n,
                    (unsigned long long)len);
    // n <= 2^30: 40 n and 32 * (its chunks) stay far below 2^64
    if (len != repo_file_bytes(n, h.chunk))
        return fail(RF_EINVAL, "repo file: %llu bytes, its header says %llu", (unsigned long long)len,
                    (unsigned long long)repo_file_bytes(n, h.chunk));
    const uint64_t nc = n_chunks(n, h.chunk);
    const uint8_t* e = buf + kRepoFileHeader;
    const uint8_t* d = e + kRepoFileEntry * n;
    if (memcmp(d + 32 * nc + 32, kEnd, 8) != 0) return fail(RF_EINVAL, "repo file: no end marker");
    uint8_t root[32];
    root_digest(h, d, nc, root);
    if (memcmp(root, d + 32 * nc, 32) != 0) return fail(RF_EINTEGRITY, "repo file: header or checksum list damaged");
    std::vector<uint8_t> got(32 * nc);
    hash(e, kRepoFileEntry * n, h.chunk, got.data());
    if (nc && memcmp(got.data(), d, 32 * nc) != 0)
        return fail(RF_EINTEGRITY, "repo file: entries do not match their checksums");
    // checksums match, but the file may still come from anywhere
    int64_t total = 0;
    if (int rc = check_records(e, n, &total)) return rc;
    if (total != h.total_bytes)
        return fail(RF_EINVAL, "repo file: the sizes sum to %lld, its header says %lld", (long long)total,
                    (long long)h.total_bytes);
    *n_out = n;
    if (total_out) *total_out = total;
    return RF_OK;
}

void repo_file_unpack(const uint8_t* buf, uint64_t n, uint8_t* ids32, int64_t* sizes) {
    const uint8_t* e = buf + kRepoFileHeader;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* r = e + kRepoFileEntry * i;
        if (ids32) memcpy(ids32 + 32 * i, r, 32);
        if (sizes) memcpy(&sizes[i], r + 32, 8);
    }
}

}  // namespace rf

using namespace rf;

extern "C" int rf_repo_file_format(const uint8_t* ids32, const int64_t* sizes, uint64_t n, uint64_t chunk,
                                   uint8_t* out, uint64_t cap, uint64_t* out_len) {
    ARG(out_len && (n == 0 || (ids32 && sizes)), "null argument");
    ARG(n <= kRepoFileMaxEntries, "repo file: too many entries");
    if (!chunk) chunk = kRepoFileChunk;
    *out_len = repo_file_bytes(n, chunk);
    if (*out_len > cap || !out)
        return fail(RF_EINVAL, "output buffer too small: need %llu bytes", (unsigned long long)*out_len);
    return repo_file_write(ids32, sizes, nullptr, n, chunk, out, repo_hash_serial);
}

extern "C" int rf_repo_file_parse(const uint8_t* buf, uint64_t len, uint8_t* ids32, int64_t* sizes,
                                  uint64_t cap_entries, uint64_t* n) {
    ARG(n && (len == 0 || buf), "null argument");
    uint64_t ne = 0;
    if (int rc = repo_file_check(buf, len, &ne, nullptr, repo_hash_serial)) return rc;
    *n = ne;
    if (ne > cap_entries || (ne && !(ids32 && sizes)))
        return fail(RF_EINVAL, "entry buffers too small: need %llu entries", (unsigned long long)ne);
    repo_file_unpack(buf, ne, ids32, sizes);
    return RF_OK;
}
