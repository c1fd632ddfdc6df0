// assoc_io.cpp -- the HBM assoc's file form (rf_assoc_save / rf_assoc_restore,
// capi.cpp) on the host alone: format, check and parse.  No HIP.
//
// Reference: memoization is Reflow's resume mechanism, and the
// assoc is where it lives: (kind, key) -> value (assoc/assoc.go:26-38).  The
// file is what a process writes to keep the tier across runs, what another
// process warms itself from, and what a shim replays into dydbassoc.
//
// File, little-endian (the layout rf_graph_save uses: chunk checksums, a root
// over header and checksums, an end marker):
//   header, 64 B   magic "RFASSOC1", u32 version = 1, u32 flags = 0,
//                  u64 n_entries, u64 chunk, 32 zero bytes
//   entries, 68 B  u32 kind, 32-B key, 32-B value -- the live entries only,
//                  strictly ascending by (kind, key bytes): equal contents
//                  give equal files whatever the table's history or capacity
//   chunk digests  one SHA-256 per `chunk` bytes of the entry area
//   trailer, 40 B  SHA-256(header || chunk digests), end marker "RFASEND1"
// A mismatch of a checksum is RF_EINTEGRITY (errors.Integrity,
// repository/file/repository.go:160-162); anything else wrong is RF_EINVAL.
#include "assoc_io.h"

#include <string.h>

#include <algorithm>
#include <vector>

#include "errors.h"
#include "host_par.h"

namespace rf {

namespace {

constexpr char kMagic[8] = {'R', 'F', 'A', 'S', 'S', 'O', 'C', '1'};
constexpr char kEnd[8] = {'R', 'F', 'A', 'S', 'E', 'N', 'D', '1'};
constexpr uint32_t kVersion = 1;

struct Header {
    char magic[8];
    uint32_t version, flags;
    uint64_t n_entries, chunk;
    uint8_t zero[32];
};
static_assert(sizeof(Header) == kAssocHeader, "header layout");

struct NoPool {  // hash_chunks / pool_sort on the caller
    unsigned size() const { return 0; }
    template <class F>
    void run(const F&) {}
};

// (no area + chunk: a file may name any granule)
uint64_t n_chunks(uint64_t n, uint64_t chunk) { return n ? (kAssocEntry * n - 1) / chunk + 1 : 0; }

// header || chunk digests -> root
void root_digest(const Header& h, const uint8_t* digests, uint64_t nc, uint8_t root[32]) {
    std::vector<uint8_t> all(sizeof h + 32 * nc);
    memcpy(all.data(), &h, sizeof h);
    if (nc) memcpy(all.data() + sizeof h, digests, 32 * nc);
    host_sha256(all.data(), all.size(), root);
}

bool is_zero32(const uint8_t* p) {
    uint8_t x = 0;
    for (int i = 0; i < 32; ++i) x |= p[i];
    return x == 0;
}

// entry records: e[0..4) kind, e[4..36) key
bool record_less(const uint8_t* a, const uint8_t* b) {
    uint32_t ka, kb;
    memcpy(&ka, a, 4);
    memcpy(&kb, b, 4);
    return ka != kb ? ka < kb : memcmp(a + 4, b + 4, 32) < 0;
}

int check_records(const uint8_t* e, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* r = e + kAssocEntry * i;
        uint32_t kind;
        memcpy(&kind, r, 4);
        if (kind >= (1u << 30)) return fail(RF_EINVAL, "assoc file: entry %llu has kind outside [0, 2^30)", (unsigned long long)i);
        if (is_zero32(r + 36)) return fail(RF_EINVAL, "assoc file: entry %llu has a zero value", (unsigned long long)i);
        if (i && !record_less(r - kAssocEntry, r))
            return fail(RF_EINVAL, "assoc file: entry %llu is not above its predecessor in (kind, key) order",
                        (unsigned long long)i);
    }
    return RF_OK;
}

}  // namespace

void assoc_hash_serial(const uint8_t* buf, uint64_t n, uint64_t chunk, uint8_t* out) {
    hash_chunks(static_cast<NoPool*>(nullptr), buf, n, chunk, out);
}

uint64_t assoc_file_bytes(uint64_t n, uint64_t chunk) {
    return kAssocHeader + kAssocEntry * n + 32 * n_chunks(n, chunk) + kAssocTrailer;
}

bool assoc_entry_less(const int32_t* kinds, const uint8_t* keys32, uint64_t a, uint64_t b) {
    const uint32_t ka = (uint32_t)kinds[a], kb = (uint32_t)kinds[b];
    return ka != kb ? ka < kb : memcmp(keys32 + 32 * a, keys32 + 32 * b, 32) < 0;
}

int assoc_file_write(const int32_t* kinds, const uint8_t* keys32, const uint8_t* vals32, const uint32_t* perm,
                     uint64_t n, uint64_t chunk, uint8_t* out, const ChunkHasher& hash) {
    Header h{};
    memcpy(h.magic, kMagic, 8);
    h.version = kVersion;
    h.n_entries = n;
    h.chunk = chunk;
    memcpy(out, &h, sizeof h);
    uint8_t* e = out + kAssocHeader;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t s = perm ? perm[i] : i;
        uint8_t* r = e + kAssocEntry * i;
        memcpy(r, &kinds[s], 4);
        memcpy(r + 4, keys32 + 32 * s, 32);
        memcpy(r + 36, vals32 + 32 * s, 32);
    }
    if (int rc = check_records(e, n)) return rc;
    const uint64_t nc = n_chunks(n, chunk);
    uint8_t* d = e + kAssocEntry * n;
    hash(e, kAssocEntry * n, chunk, d);
    root_digest(h, d, nc, d + 32 * nc);
    memcpy(d + 32 * nc + 32, kEnd, 8);
    return RF_OK;
}

int assoc_file_check(const uint8_t* buf, uint64_t len, uint64_t* n_out, const ChunkHasher& hash) {
    if (len < kAssocHeader + kAssocTrailer) return fail(RF_EINVAL, "assoc file: %llu bytes is too short", (unsigned long long)len);
    Header h;
    memcpy(&h, buf, sizeof h);
    if (memcmp(h.magic, kMagic, 8) != 0) return fail(RF_EINVAL, "assoc file: bad magic");
    if (h.version != kVersion) return fail(RF_EINVAL, "assoc file: version %u not supported", h.version);
    if (h.flags != 0) return fail(RF_EINVAL, "assoc file: unknown flags %#x", h.flags);
    if (h.chunk == 0) return fail(RF_EINVAL, "assoc file: zero checksum granule");
    const uint64_t n = h.n_entries;
    if (n > kAssocMaxEntries || n > (len - kAssocHeader - kAssocTrailer) / kAssocEntry)
        return fail(RF_EINVAL, "assoc file: %llu entries do not fit its %llu bytes", (unsigned long long)n,
                    (unsigned long long)len);
    // n <= 2^30: 68 n and 32 * (its chunks) stay far below 2^64
    if (len != assoc_file_bytes(n, h.chunk))
        return fail(RF_EINVAL, "assoc file: %llu bytes, its header says %llu", (unsigned long long)len,
                    (unsigned long long)assoc_file_bytes(n, h.chunk));
    const uint64_t nc = n_chunks(n, h.chunk);
    const uint8_t* e = buf + kAssocHeader;
    const uint8_t* d = e + kAssocEntry * n;
    if (memcmp(d + 32 * nc + 32, kEnd, 8) != 0) return fail(RF_EINVAL, "assoc file: no end marker");
    uint8_t root[32];
    root_digest(h, d, nc, root);
    if (memcmp(root, d + 32 * nc, 32) != 0) return fail(RF_EINTEGRITY, "assoc file: header or checksum list damaged");
    std::vector<uint8_t> got(32 * nc);
    hash(e, kAssocEntry * n, h.chunk, got.data());
    if (nc && memcmp(got.data(), d, 32 * nc) != 0) return fail(RF_EINTEGRITY, "assoc file: entries do not match their checksums");
    // checksums match, but the file may still come from anywhere
    if (int rc = check_records(e, n)) return rc;
    *n_out = n;
    return RF_OK;
}

void assoc_file_unpack(const uint8_t* buf, uint64_t n, int32_t* kinds, uint8_t* keys32, uint8_t* vals32) {
    const uint8_t* e = buf + kAssocHeader;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* r = e + kAssocEntry * i;
        memcpy(&kinds[i], r, 4);
        memcpy(keys32 + 32 * i, r + 4, 32);
        memcpy(vals32 + 32 * i, r + 36, 32);
    }
}

}  // namespace rf

using namespace rf;

extern "C" int rf_assoc_file_format(const int32_t* kinds, const uint8_t* keys32, const uint8_t* vals32, uint64_t n,
                                    uint64_t chunk, uint8_t* out, uint64_t cap, uint64_t* out_len) {
    ARG(out_len && (n == 0 || (kinds && keys32 && vals32)), "null argument");
    ARG(n <= kAssocMaxEntries, "assoc file: too many entries");
    if (!chunk) chunk = kAssocChunk;
    *out_len = assoc_file_bytes(n, chunk);
    if (*out_len > cap || !out)
        return fail(RF_EINVAL, "output buffer too small: need %llu bytes", (unsigned long long)*out_len);
    return assoc_file_write(kinds, keys32, vals32, nullptr, n, chunk, out, assoc_hash_serial);
}

extern "C" int rf_assoc_file_parse(const uint8_t* buf, uint64_t len, int32_t* kinds, uint8_t* keys32,
                                   uint8_t* vals32, uint64_t cap_entries, uint64_t* n) {
    ARG(n && (len == 0 || buf), "null argument");
    uint64_t ne = 0;
    if (int rc = assoc_file_check(buf, len, &ne, assoc_hash_serial)) return rc;
    *n = ne;
    if (ne > cap_entries || (ne && !(kinds && keys32 && vals32)))
        return fail(RF_EINVAL, "entry buffers too small: need %llu entries", (unsigned long long)ne);
    assoc_file_unpack(buf, ne, kinds, keys32, vals32);
    return RF_OK;
}
