/*
 * reflow_hip.h -- C-ABI of the MI355X memoization engine (libreflow_hip.so).
 *
 * Drop-in boundary for Reflow's data-parallel memoization hot path
 * (reference: LDuderino/reflow @ v0, paths relative to /root/reference).
 * Every entry point is batched: the reference's per-call Go interfaces
 * (one io.Writer per file, one goroutine per cache lookup) are coalesced by
 * the host shim into device batches (INTEGRATION.md shows the cgo binding).
 *
 * Conventions
 *   - Plain pointers and sizes; no C++ or torch types cross this boundary.
 *   - Every function returns an rf_status (0 = RF_OK).  On failure
 *     rf_last_error() returns a thread-local message.  No exception crosses.
 *   - Host buffers are caller-owned and not retained after return (cgo rule).
 *     Device buffers passed to *_device functions are caller-owned HBM.
 *   - "stream" arguments are hipStream_t values passed as void* (NULL = the
 *     context's own stream).  *_device functions are asynchronous on it.
 *   - A digest is 32 raw SHA-256 bytes.  WD(d) = 0x00 0x05 || d (34 bytes) is
 *     the grailbio/base/digest.WriteDigest framing the reference hashes.
 *
 * The product path is the HIP path: if the gfx950 code object cannot be
 * loaded or no device is present, rf_init fails with RF_EDEVICE -- there is
 * no CPU fallback behind this ABI.  The one place host cores hash is the K1
 * planner's host leg (rf_set_host_threads): a scheduled part of a batch, not
 * a fallback -- the longest SHA-256 chains of a skewed batch, which a host
 * core with SHA-NI runs ~40x faster than one GPU wave, go to a pool of host
 * threads (the reference's <=60-goroutine digest pool, local/executor.go:41)
 * while the GPU kernels hash the rest.  It needs a device like every other
 * call, and rf_set_host_threads(ctx, 0) pins every message to the GPU.
 */
#ifndef REFLOW_HIP_H
#define REFLOW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes; the shim maps them onto errors.Kind (errors/errors.go:39-76). */
typedef enum {
    RF_OK = 0,
    RF_EINVAL = 1,     /* errors.Invalid: malformed input, bad graph, cycle */
    RF_EIO = 2,        /* errors.Unavailable: reading an input file failed   */
    RF_EINTEGRITY = 3, /* errors.Integrity: digest mismatch on verify        */
    RF_EDEVICE = 4,    /* errors.Unavailable: HIP runtime / device failure   */
    RF_ENOMEM = 5,     /* errors.ResourcesExhausted: HBM or host allocation  */
    RF_ENOTFOUND = 6,  /* errors.NotExist                                     */
    RF_EPRECONDITION = 7, /* errors.Precondition: assoc compare-and-set failed */
    RF_ENOTCANONICAL = 8  /* per-document status of the Fileset unmarshal, never a call's return: not the
                             encoder's bytes, decode it on the Go path (no errors.Kind: not an error) */
} rf_status;

typedef struct rf_ctx rf_ctx;
typedef struct rf_sha_plan rf_sha_plan;
typedef struct rf_graph rf_graph;
typedef struct rf_bloom rf_bloom;
typedef struct rf_assoc rf_assoc;
typedef struct rf_install rf_install;

/* ---- context ----------------------------------------------------------- */
/* Bind a context to HIP device `device` (one process per GPU).  Replaces the
 * process-global reflow.Digester (flow.go:36) as the owner of device state. */
int rf_init(int device, rf_ctx **out);
void rf_destroy(rf_ctx *ctx);
const char *rf_last_error(void);
int rf_device_count(int *n);
/* The device's compute units as the K1 planner counts them (its octo / pair /
 * lanes thresholds are 16, 64 and 5*256 messages per CU). */
int rf_device_cus(rf_ctx *ctx, int *n_cu);
/* Blocks until all work queued on the context's stream finished. */
int rf_sync(rf_ctx *ctx);
/* Version string, e.g. "reflow-hip 0.1 gfx950". */
const char *rf_version(void);

/* K1 host leg width: n >= 1 threads, 0 = none (every message on the GPU
 * kernels), -1 = default min(60, CPU share): 60 is the reference's
 * DigestLimiter (local/executor.go:41), the share the smaller of the affinity
 * mask and the cgroup cpu.max quota, divided by LOCAL_WORLD_SIZE (ranks per
 * node); RF_HOST_THREADS overrides the default.  Without the x86 SHA
 * extensions the host leg is off whatever n is. */
int rf_set_host_threads(rf_ctx *ctx, int n);
/* Host leg threads in effect, one core's measured SHA-NI rate (bytes/s; 0 if
 * unavailable) and whether the CPU has the SHA extensions. */
int rf_host_info(rf_ctx *ctx, int *threads, double *core_bytes_per_s, int *sha_ext);
/* The host leg's chains per thread (RF_HOST_WAYS, default 2: SHA-NI rounds
 * are latency-bound, two interleaved messages fill the issue slots) and one
 * thread's measured rate at that interleave (bytes/s) -- the per-thread peak
 * bench.py prices the host leg against. */
int rf_host_rate(rf_ctx *ctx, int *ways, double *thread_bytes_per_s);
/* The feed rate (bytes/s) the K1 planner prices the host leg's HBM-resident
 * bytes at: measured by the last RF_SHA_ALL_HOST plan run on this context
 * whose host leg took >= 1 GiB at the current width (*measured = 1; the leg's
 * bytes over its wall time, D2H copies and SHA-NI threads together), else the
 * built-in PCIe Gen5 estimate (52 GB/s, *measured = 0).  Only all-host runs
 * calibrate: a hybrid run's host leg may idle beside the GPU legs or start
 * files from a GPU-made prefix, and a host-resident batch crosses no link, so
 * their bytes over wall time are not the feed rate and leave it as it was.
 * Plans created after a measurement use it: a caller calibrates with one
 * RF_SHA_ALL_HOST run, then plans the split. */
int rf_host_link(rf_ctx *ctx, double *bytes_per_s, int *measured);

/* ---- device memory and timing -------------------------------------------
 * The engine owns its HIP runtime; callers (the cgo shim, bench.py, tests)
 * allocate HBM through these so no second runtime enters the process. */
int rf_malloc(rf_ctx *ctx, uint64_t bytes, void **out);
int rf_free(rf_ctx *ctx, void *p);
int rf_memcpy_h2d(rf_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int rf_memcpy_d2h(rf_ctx *ctx, void *dst, const void *src, uint64_t bytes);
int rf_memset_d(rf_ctx *ctx, void *dst, int value, uint64_t bytes);
int rf_memcpy_d2d(rf_ctx *ctx, void *dst, const void *src, uint64_t bytes);
/* The context's hipStream_t. */
void *rf_stream(rf_ctx *ctx);
/* HIP-event timer on the context stream: start, then stop returns ms. */
int rf_timer_start(rf_ctx *ctx);
int rf_timer_stop(rf_ctx *ctx, float *ms);

/* ---- RCCL over xGMI (multi-GPU: one process per GPU) ----------------------
 * Bootstrap: rank 0 calls rf_comm_unique_id and ships the 128 bytes to the
 * other ranks out of band (bench.py uses torch.distributed/gloo on the CPU). */
typedef struct rf_comm rf_comm;
int rf_comm_unique_id(uint8_t id[128]);
int rf_comm_init(rf_ctx *ctx, int nranks, int rank, const uint8_t id[128], rf_comm **out);
void rf_comm_destroy(rf_comm *comm);
/* d_recv[r*bytes .. +bytes) = rank r's d_send (ncclAllGather). */
int rf_comm_allgather(rf_comm *comm, const void *d_send, void *d_recv, uint64_t bytes, void *stream);
/* In-place bitwise OR of nwords uint64 across ranks.  RCCL has no OR
 * reduction: all-gather of the packed words + a local OR kernel. */
int rf_comm_allreduce_or(rf_comm *comm, void *d_words, uint64_t nwords, void *stream);

/* ---- K1: batched SHA-256 (Digester.NewWriter/FromBytes, Repository.Put) --
 * Replaces the per-file io.Copy into Digester.NewWriter() at
 * repository/file/repository.go:50-63 (Install) and :237-264 (Put), driven by
 * the ≤60-goroutine loop of local/executor.go:514-557.  out32[i] = SHA256(msg i). */
int rf_sha256_batch(rf_ctx *ctx, const uint8_t *const *msgs, const uint64_t *lens, uint64_t n,
                    uint8_t *out32);

/* Same, messages given as one host arena + offsets. */
int rf_sha256_arena(rf_ctx *ctx, const uint8_t *arena, const uint64_t *offs, const uint64_t *lens,
                    uint64_t n, uint8_t *out32);

/* Device-resident form.  A plan is built once from host-side offsets and
 * lengths: it orders messages largest-first and splits them by a makespan
 * model over the legs -- the host leg (the largest messages, SHA-NI threads,
 * bytes streamed D2H in 8 MiB chunks), wave-per-message duo chains, and the
 * lane-per-message kernels; rf_sha_plan_run then digests messages already in
 * HBM.  The GPU legs are queued asynchronously on `stream`; with a host leg
 * the call is SYNCHRONOUS: it returns once the host threads are done (their
 * digests' upload and scatter into out queued on `stream`) -- ~1.3 s on
 * configs[1].  The context's mutex is released while the host threads hash,
 * so other calls on the context proceed meanwhile (calls that need the host
 * leg themselves wait for it); one run of a given plan at a time.
 * Requirements: offs[i] % 16 == 0.  out is n*32 bytes of device memory. */
int rf_sha_plan_create(rf_ctx *ctx, const uint64_t *offs, const uint64_t *lens, uint64_t n,
                       uint32_t flags, rf_sha_plan **out);
int rf_sha_plan_run(rf_sha_plan *plan, const void *d_arena, void *d_out32, void *stream);
typedef struct {
    uint64_t n_msgs, n_solo;     /* messages; messages run wave-per-message */
    uint64_t total_blocks;       /* Σ ceil((len+9)/64): algorithmic unit of K1 */
    uint64_t max_blocks;         /* critical path of the largest message       */
    uint64_t total_bytes;
    float last_ms_lanes, last_ms_solo, last_ms_total; /* HIP-event times of the last run */
    float last_ms_host;          /* wall time of the last run's host leg         */
    uint32_t host_threads;       /* host leg threads (0: no host leg)            */
    uint64_t n_host, host_bytes; /* messages / bytes on the host leg             */
} rf_sha_stats;
int rf_sha_plan_stats(rf_sha_plan *plan, rf_sha_stats *out);
void rf_sha_plan_destroy(rf_sha_plan *plan);
/* flags for rf_sha_plan_create */
#define RF_SHA_NO_SOLO 1u      /* every message lane-per-message */
#define RF_SHA_ALL_SOLO 2u     /* every message wave-per-message */
#define RF_SHA_ONE_LANE_CHAIN 4u /* wave-per-message kernel keeps the round chain on one lane */
#define RF_SHA_NO_PAIR 8u      /* small sets: lanes kernel instead of the producer/chain pair */
#define RF_SHA_NO_OCTO 16u     /* small sets: no eight-per-wave two-lane chains (pair or lanes) */
#define RF_SHA_ALL_HOST 32u    /* every message on the host leg (needs SHA-NI and host threads) */
#define RF_SHA_NO_HOST 64u     /* no host leg: every message on the GPU kernels */
#define RF_SHA_NO_PREFIX 128u  /* no prefix hand-over: the split and the run as without it */

/* Prefix hand-over.  A host-leg message that waits in the pool's queue has
 * its first blocks hashed by an idle duo wave meanwhile, which leaves its
 * chaining value in host memory every few thousand blocks; the host thread
 * that claims the message stops the wave and resumes from the latest value
 * it finds instead of block 0 (it never waits for the wave).
 * Planned for HBM-resident plans with both legs; off with RF_SHA_NO_PREFIX,
 * or with RF_SHA_PREFIX=0 in the environment when the plan is created.  Read
 * there too: RF_SHA_PREFIX_ALPHA, the share of a message's modelled wait the
 * split is priced with (default 1.0); RF_SHA_PREFIX_CKPT, the blocks between
 * two chaining values (a multiple of 64, default 2048); and, for tests,
 * RF_SHA_PREFIX_PRECLAIM=1: every message counts as claimed before the
 * launch, so each wave stops at its first value.
 *
 * Lone lanes.  The first n_lone host-leg messages (the largest) each run alone
 * on their host thread: its other lanes take nothing until that message ends,
 * so the chains that would set the step run at the one-lane rate.  Chosen by
 * the planner's schedule model for the plans that get prefixes; never for
 * all-host, host-resident or one-lane-chain plans.  RF_SHA_LONE=<k> in the
 * environment when the plan is created forces k (0: none). */
typedef struct {
    uint64_t n_prefixed;    /* host-leg messages with a prefix                 */
    uint64_t planned_bytes; /* 64 x the most blocks their waves may hash       */
    uint64_t taken, missed; /* last run: prefixes found ready / not ready      */
    uint64_t skipped_bytes; /* last run: bytes the host leg did not hash       */
    uint64_t n_lone;        /* host-leg messages that run alone on their thread */
} rf_sha_prefix_stats;
int rf_sha_plan_prefix_stats(rf_sha_plan *plan, rf_sha_prefix_stats *out);
/* Test control.  prefix_blocks[i] (NULL: keep the plan's) replaces the prefix
 * of host-leg message i -- the plan's host messages in its own order, largest
 * first, n_host of them -- each at most len / 64.  mode: RF_PREFIX_RACE, the
 * production behaviour; RF_PREFIX_WAIT, the host leg starts only once the
 * prefix launch is done (an event wait), so every prefix is taken;
 * RF_PREFIX_MISS, the prefixes are left out of the launch, so none is. */
#define RF_PREFIX_RACE 0
#define RF_PREFIX_WAIT 1
#define RF_PREFIX_MISS 2
int rf_sha_plan_set_prefixes(rf_sha_plan *plan, const uint64_t *prefix_blocks, int mode);

/* ---- Streaming SHA-256 (Digester.NewWriter: an io.Writer whose state carries
 * across Write calls) for many streams at once -------------------------------
 * Repository.Put hashes an io.Reader as it copies it (repository/file/
 * repository.go:237-264; s3's Put through a TeeReader, repository/s3/s3.go:
 * 120-147): the shim feeds each upload's chunks here as they arrive, so no
 * upload is buffered whole.  Per stream the carried partial block plus its
 * chunks give whole blocks, hashed from the stream's midstate -- the largest
 * on the host leg (in place), the rest by k1_sha256_resume on the GPU, by a
 * makespan model like a K1 plan.  flags: 0, RF_SHA_ALL_HOST or
 * RF_SHA_NO_HOST (every segment on k1_sha256_resume). */
typedef struct rf_sha_streams rf_sha_streams;
int rf_sha_streams_open(rf_ctx *ctx, uint64_t n_streams, uint32_t flags, rf_sha_streams **out);
void rf_sha_streams_close(rf_sha_streams *s);
/* Write chunk i to stream ids[i]; chunks of one stream apply in batch order. */
int rf_sha_streams_write(rf_sha_streams *s, const uint64_t *ids, const uint8_t *const *chunks,
                         const uint64_t *lens, uint64_t n);
/* out32[i] = Digest() of stream ids[i] (distinct ids); the stream restarts empty. */
int rf_sha_streams_digest(rf_sha_streams *s, const uint64_t *ids, uint64_t n, uint8_t *out32);
/* Bytes written to stream id since its last digest (Put's returned size). */
int rf_sha_streams_len(rf_sha_streams *s, uint64_t id, uint64_t *len);
/* Integrity check (ReadFrom / WriteTo re-digest, repository/file/repository.go:
 * 126-166, 212): status[i] = RF_OK or RF_EINTEGRITY (digest of stream ids[i] vs
 * want32[i]); returns RF_EINTEGRITY if any differs (errors.Integrity).  The
 * streams restart empty. */
int rf_sha_streams_verify(rf_sha_streams *s, const uint64_t *ids, const uint8_t *want32, uint64_t n,
                          int32_t *status);
/* The same for whole messages: status[i] for SHA256(msg i) vs want32[i]. */
int rf_sha256_verify(rf_ctx *ctx, const uint8_t *const *msgs, const uint64_t *lens, uint64_t n,
                     const uint8_t *want32, int32_t *status);

/* Synthetic data generator (bench / tests): fills d_arena so that message i
 * is the splitmix64 counter stream with seed (seed ^ i). */
int rf_gen_fill(rf_ctx *ctx, void *d_arena, const uint64_t *d_offs, const uint64_t *d_lens,
                uint64_t n, uint64_t seed, uint64_t arena_bytes, void *stream);

/* ---- Fileset digest (Fileset.Digest/WriteDigest, executor.go:205-233) ----
 * n_sets filesets; set s owns groups [set_group[s], set_group[s+1]); group g
 * owns entries [group_entry[g], group_entry[g+1]).  A Map fileset is one
 * group; a List fileset contributes its (flattened, depth-first) Map leaves as
 * consecutive groups ("List wins if non-nil", executor.go:216-219).  Entries
 * within a group are sorted bytewise here (sort.Strings).  Material per group
 * = Σ path ‖ WD(id).  out32[s] = SHA256(material of set s). */
int rf_fileset_digest_batch(rf_ctx *ctx, uint64_t n_sets, const uint64_t *set_group,
                            const uint64_t *group_entry, const char *const *paths,
                            const uint32_t *path_lens, const uint8_t *ids32, uint8_t *out32);
/* As rf_fileset_digest_batch with the File IDs resident in HBM (d_ids32[e],
 * e.g. the out32 of an rf_sha_plan_run over the installed files): no ID
 * readback; the IDs are placed into the material on the device and only the
 * set digests return (Executor.install -> Fileset.Digest,
 * local/executor.go:514-557 + executor.go:205-233). */
int rf_fileset_digest_device(rf_ctx *ctx, uint64_t n_sets, const uint64_t *set_group,
                             const uint64_t *group_entry, const char *const *paths,
                             const uint32_t *path_lens, const void *d_ids32, uint8_t *out32);

/* ---- Executor.install: walk + read + digest a tree into a Fileset ----------
 * Replaces local/executor.go:514-557 (install: walker loop, <=60 concurrent
 * repo.Install calls, Fileset{Map} assembly) over internal/walker/walker.go:33-99
 * and repository/file/repository.go:50-63 (ID = SHA256(contents)).  Walk
 * semantics are the walker's: os.Stat follows symlinks, a path that does not
 * exist (ENOENT, e.g. a dangling link) is skipped, directory entries are
 * visited in bytewise-sorted, depth-first pre-order; every non-directory
 * entry is read and digested (one K1 batch per <= 8 GiB chunk).  Entry i has
 * relpath = filepath.Rel(root, path) ("." when root is a file), ID and Size =
 * the Stat size (executor.go:525).  A missing root gives n = 0 and the digest
 * of the empty Fileset.  Errors: RF_EIO for stat/readdir/open/read failures
 * (the walker's w.Err(), Install's error) and for a file whose size changed
 * between the walk and the read.  The optional symlink replacement of
 * executor.go:544-552 stays with the caller (it only uses the IDs returned).
 * rf_install_info: entry count, total relpath bytes, and
 * Fileset{Map: relpath -> File}.Digest() (executor.go:205-233).
 * rf_install_entries: caller-allocated paths (path_bytes), path_offs (n+1),
 * ids32 (32n), sizes (n), in walk order; any of them may be NULL. */
int rf_install_dir(rf_ctx *ctx, const char *root, rf_install **out);
int rf_install_info(const rf_install *in, uint64_t *n_entries, uint64_t *path_bytes,
                    uint8_t fileset_digest32[32]);
int rf_install_entries(const rf_install *in, char *paths, uint64_t *path_offs, uint8_t *ids32,
                       int64_t *sizes);
void rf_install_destroy(rf_install *in);
/* The walk alone, host-only (no device): internal/walker's Scan as install
 * uses it -- relpaths ("." for a file root) and Stat sizes of every
 * non-directory entry, bytewise-sorted depth-first pre-order, links
 * followed, vanished entries skipped.  rf_walk_entries: paths concatenated,
 * path_offs[n_entries + 1]. */
typedef struct rf_walk rf_walk;
int rf_walk_dir(const char *root, rf_walk **out);
int rf_walk_info(const rf_walk *w, uint64_t *n_entries, uint64_t *path_bytes);
int rf_walk_entries(const rf_walk *w, char *paths, uint64_t *path_offs, int64_t *sizes);
void rf_walk_free(rf_walk *w);

/* ---- Fileset values as JSON (the assoc value, eval.go:1141 -> marshal
 * eval.go:1961-1967 = json.Marshal + Repository.Put, repository.go:108-114) --
 * A fileset TREE: node i's List = nodes list_child[list_ptr[i] .. list_ptr[i+1])
 * (an empty range = nil or empty List: both omitted, `json:",omitempty"`);
 * node i's Map = entries [entry_ptr[i], entry_ptr[i+1]) with path bytes,
 * 32-B File ID and Size (executor.go:25-38).  JSON bytes follow Go 1.9/1.10
 * encoding/json: {"List":[...],"Fileset":{"<path>":{"ID":"sha256:<hex>","Size":N}}},
 * keys sorted bytewise, HTML-safe escaping, invalid UTF-8 -> �.  The ID's
 * text form is grailbio/base digest's String() (unvendored: parity unpinned). */
typedef struct {
    uint64_t n_nodes;
    const uint64_t *list_ptr;    /* [n_nodes+1] */
    const uint32_t *list_child;  /* [list_ptr[n_nodes]] */
    const uint64_t *entry_ptr;   /* [n_nodes+1] */
    const char *const *paths;    /* [entries] */
    const uint32_t *path_lens;   /* [entries] */
    const uint8_t *ids32;        /* [entries][32] */
    const int64_t *sizes;        /* [entries] */
} rf_fileset_tree;
/* json.Marshal of node `root` into out[cap]; *out_len = bytes needed (RF_EINVAL
 * if cap is short).  Host-only (no device needed). */
int rf_fileset_marshal_json(const rf_fileset_tree *t, uint32_t root, uint8_t *out, uint64_t cap,
                            uint64_t *out_len);
/* out32[i] = SHA256(json.Marshal(roots[i])): the value digests CacheWrite
 * stores (eval.go:1141-1151); the hashes run on K1. */
int rf_fileset_value_digest_batch(rf_ctx *ctx, const rf_fileset_tree *t, const uint32_t *roots,
                                  uint64_t n, uint8_t *out32);

/* ---- Fileset values marshalled on the device (Eval.CacheWrite's marshal(fs),
 * eval.go:1141 -> eval.go:1961-1967 = json.Marshal + Repository.Put) ----------
 * The bytes of rf_fileset_marshal_json, made in HBM for a batch of values whose
 * File IDs may already be there (the out32 of K1 over the installed files,
 * local/executor.go:514-557).  The host flattens each root into a piece stream
 * in output order -- literal pieces (skeleton bytes such as {"List":[ , ]
 * "Fileset":{ }, held once in a small blob) and entry pieces (one Map entry and
 * a bit for its comma), the entries of a Map ordered bytewise (Maps already in
 * order are found in one linear pass and left alone) -- in O(fileset nodes +
 * entries) plus that sort.  The device measures the pieces, scans tiles of
 * RF_MARSHAL_TILE pieces (tile mark / scan / scatter, no atomic on a shared
 * counter) and emits every value at a 16-byte aligned offset of one arena (K1
 * wants offs % 16 == 0), pad bytes zeroed.  The value lengths and a "zero ID
 * seen" word are read back once; the JSON stays in HBM.  Refusals are those of
 * rf_fileset_marshal_json with its status (a node out of range, a CSR that is
 * not monotone, a depth above 4096, duplicate map keys, a zero ID); a batch
 * whose JSON could reach 4 GiB is refused with RF_EINVAL (split it). */
#define RF_MARSHAL_TILE 1024 /* pieces per tile of the marshal's length / scan / emit */
typedef struct rf_json_batch rf_json_batch;
/* Host only, no context, not a product path: the piece stream of roots[0 .. n)
 * run through the per-piece code the kernels run, so that CPU tests cover
 * flatten, sort and emit.  Value i's bytes at out + offs[i], offs[n] = *out_len
 * = the bytes needed (RF_EINVAL, nothing written, if cap is short); offs may be
 * NULL. */
int rf_fileset_marshal_flat(const rf_fileset_tree *t, const uint32_t *roots, uint64_t n, uint8_t *out,
                            uint64_t cap, uint64_t *offs /* n + 1 */, uint64_t *out_len);
/* json.Marshal of roots[0 .. n) into a batch object.  d_ids32 != NULL: entry
 * e's File ID is device row e (16-byte aligned) and t->ids32 may be NULL; a
 * zero ID is then found on the device.  Either way a zero ID fails the call
 * with RF_EINVAL and leaves *out untouched.  Returns when the bytes are
 * written. */
int rf_fileset_marshal_device(rf_ctx *ctx, const rf_fileset_tree *t, const uint32_t *roots, uint64_t n,
                              const void *d_ids32 /* or NULL: t->ids32 */, rf_json_batch **out, void *stream);
/* Values, the sum of their JSON lengths, and pieces; any pointer may be NULL. */
int rf_json_batch_info(const rf_json_batch *b, uint64_t *n, uint64_t *total_bytes, uint64_t *n_pieces);
/* Where the marshal call spent its time, host clock, milliseconds: ms[0]
 * flatten + sort on the host, ms[1] upload + length pass + scan + the
 * read-back, ms[2] arena setup + emit pass (each ends in a synchronise). */
int rf_json_batch_times(const rf_json_batch *b, double ms[3]);
/* lens[i] = bytes of value i: the Size Repository.Put reports (repository.go:108-114). */
int rf_json_batch_lens(const rf_json_batch *b, int64_t *lens);
/* The arena, the values' offsets (u64 [n], each % 16 == 0) and their lengths
 * (i64 [n]) as device pointers, valid until rf_json_batch_free. */
int rf_json_batch_device(const rf_json_batch *b, const void **d_arena, const void **d_offs, const void **d_lens);
/* D2H copy of the values which[0 .. n) (NULL: values 0 .. n-1), packed: value j
 * at out + offs[j], offs[n] = the bytes needed (set either way; RF_EINVAL if
 * cap is short) -- for the caller's real Repository.Put of the bytes. */
int rf_json_batch_copy(rf_json_batch *b, const uint64_t *which, uint64_t n, uint8_t *out, uint64_t cap,
                       uint64_t *offs /* n + 1 */);
/* d_out32[i] = SHA256(value i): the fsid (eval.go:1141-1151).  K1 over the
 * arena through the one-shot plan of rf_sha256_batch, GPU legs only.  Returns
 * when done. */
int rf_json_batch_digests_device(rf_json_batch *b, void *d_out32, void *stream);
void rf_json_batch_free(rf_json_batch *b);
/* Marshal plus digests in one call, the device twin of
 * rf_fileset_value_digest_batch: d_out32[i] = the fsid of roots[i], d_sizes[i]
 * (i64, may be NULL) = its JSON length. */
int rf_fileset_value_digest_device(rf_ctx *ctx, const rf_fileset_tree *t, const uint32_t *roots, uint64_t n,
                                   const void *d_ids32, void *d_out32, void *d_sizes, void *stream);

/* ---- Fileset values unmarshalled on the device (Eval.lookup's unmarshal(fsid),
 * eval.go:1212 -> eval.go:1971-1978 = Repository.Get + JSON decode) -----------
 * The inverse of rf_fileset_marshal_device: a batch of JSON documents, in a
 * device arena (the one rf_json_batch_device hands out, say) or in host bytes,
 * becomes the flat (ID, Size) rows rf_repo_missing_device and
 * rf_liveset_set_values_device take -- one group per document -- plus the full
 * structure (nodes, decoded paths, IDs, sizes) for the caller's Fileset
 * objects.
 *
 * Accepted is the CANONICAL form and nothing else: exactly the bytes
 * json.Marshal(Fileset) / rf_fileset_marshal_json write.
 *   node  := '{' [ '"List":[' node (',' node)* ']' ] [ ',' if both ]
 *                [ '"Fileset":{' entry (',' entry)* '}' ] '}'
 *   entry := string ':{"ID":"sha256:' 64x[0-9a-f] '","Size":' int '}'
 *   int   := '-'? ( '0' | [1-9][0-9]* ), within int64, "-0" refused
 * Deliberately NOT accepted, although Go's tolerant decoder takes them:
 * whitespace, keys in another case or order, unknown or duplicate fields,
 * "Fileset":{} and "List":[] (omitempty never emits them), and escapes the
 * encoder never emits (a u-escape of a plain letter, \/, \b, upper-case hex).
 * A string's units are raw bytes that need no escape (valid UTF-8 other than
 * U+2028/U+2029), \" \\ \n \r \t, the lower-case u-escape 00XX of a control
 * byte or of < > &, and the u-escapes fffd, 2028, 2029; they decode as Go's
 * decoder decodes them.  Within a Map the decoded paths ascend strictly
 * bytewise (the encoder sorts; strict order excludes duplicates).  One
 * consequence: a document made from paths with invalid UTF-8, whose
 * replacement bytes break that order, is reported as not canonical.  An
 * all-zero ID, nodes nested deeper than 4096 and an empty document are refused
 * as the marshal refuses them.  Every other document gets status
 * RF_ENOTCANONICAL and a reason mask, contributes no node, entry or row (its
 * group is empty; the accepted documents' outputs stay dense), and goes to the
 * caller's Go decoder: not a silent fallback, the status says which.  The
 * reason names the first thing wrong reading left to right (LENGTH: the
 * document ends where more must follow); equal bytes give an equal mask.
 *
 * Nodes are numbered per document in CLOSING order (post-order; the root is a
 * document's last node) with their depth (root 0): the entries stand in
 * document order, and the entries between two closing braces are the later
 * node's Map, so entry_ptr is one CSR over nodes and entries.  Closing order
 * with depths determines the tree; rf_fileset_forest_tree rebuilds the List
 * CSR of rf_fileset_tree from it in O(nodes) on the host.
 *
 * The device form works in tiles of RF_UNMARSHAL_TILE arena bytes, every pass
 * tile summary / scan of summaries / apply, no atomic on a shared counter:
 * quote bits, in-string parity, token checks and counts, nesting depth, then
 * the scatter; the results are a function of the bytes alone.  Documents may
 * start at any byte offset; they must be ascending, non-overlapping and inside
 * the arena (RF_EINVAL otherwise, found on the device and reported after the
 * call's one read-back).  An arena of 4 GiB or more is RF_EINVAL.  d_arena
 * must be 16-byte aligned. */
#define RF_UNMARSHAL_TILE 4096 /* arena bytes per tile of the unmarshal's passes */
#define RF_UNMARSHAL_WHY_STRUCTURE 1u
#define RF_UNMARSHAL_WHY_STRING 2u
#define RF_UNMARSHAL_WHY_ID 4u
#define RF_UNMARSHAL_WHY_SIZE 8u
#define RF_UNMARSHAL_WHY_ORDER 16u
#define RF_UNMARSHAL_WHY_DEPTH 32u
#define RF_UNMARSHAL_WHY_LENGTH 64u
#define RF_UNMARSHAL_CHECK_TILED 1u /* rf_fileset_unmarshal_flat: also run the kernels' per-byte form on the host */
typedef struct rf_fileset_forest rf_fileset_forest;
/* Host only, no context, not a product path: document d = json[offs[d],
 * offs[d + 1]), parsed on `threads` host threads (0: up to 16) by the
 * sequential form of the code the kernels run.  With RF_UNMARSHAL_CHECK_TILED
 * every document also goes through the per-byte form of the kernels, and a
 * differing verdict or count fails the call with RF_EDEVICE. */
int rf_fileset_unmarshal_flat(const uint8_t *json, const uint64_t *offs /* n + 1 */, uint64_t n, uint32_t flags,
                              unsigned threads, rf_fileset_forest **out);
/* Document d = d_arena[d_offs[d], d_offs[d] + d_lens[d]) (u64 / i64 device
 * arrays, as rf_json_batch_device gives them).  Returns when the results are
 * complete.  n = 0 gives an empty forest. */
int rf_fileset_unmarshal_device(rf_ctx *ctx, const void *d_arena, uint64_t arena_bytes, const void *d_offs,
                                const void *d_lens, uint64_t n, rf_fileset_forest **out, void *stream);
/* The same over packed host bytes (document d = json[offs[d], offs[d + 1])),
 * which the call uploads. */
int rf_fileset_unmarshal(rf_ctx *ctx, const uint8_t *json, const uint64_t *offs /* n + 1 */, uint64_t n,
                         rf_fileset_forest **out, void *stream);
/* Documents, accepted documents, nodes, entries, decoded path bytes; any pointer may be NULL. */
int rf_fileset_forest_info(const rf_fileset_forest *f, uint64_t *n_docs, uint64_t *n_accepted, uint64_t *n_nodes,
                           uint64_t *n_entries, uint64_t *path_bytes);
/* Per document: RF_OK / RF_ENOTCANONICAL, the reason mask, nodes and entries (0
 * for a refused one).  entry_counts is the `counts` argument of
 * rf_liveset_set_values[_device].  Any pointer may be NULL. */
int rf_fileset_forest_status(const rf_fileset_forest *f, int32_t *status, uint32_t *reason, uint32_t *node_counts,
                             uint32_t *entry_counts);
/* The value rows in HBM, valid until rf_fileset_forest_free: d_counts (u32 per
 * document), d_ids32 (32 B rows, 16-byte aligned), d_sizes (i64) and their
 * number -- the arguments of rf_repo_missing_device.  RF_EINVAL for a
 * host-form forest. */
int rf_fileset_forest_rows_device(const rf_fileset_forest *f, const void **d_counts, const void **d_ids32,
                                  const void **d_sizes, uint64_t *n_rows);
/* The structure on the host; any pointer may be NULL.  doc_node_ptr [docs + 1],
 * node_depth [nodes], entry_ptr [nodes + 1], path_off [entries + 1], paths
 * [path bytes] decoded, ids32 [entries][32], sizes [entries]. */
int rf_fileset_forest_copy(rf_fileset_forest *f, uint64_t *doc_node_ptr, uint32_t *node_depth, uint64_t *entry_ptr,
                           uint64_t *path_off, uint8_t *paths, uint8_t *ids32, int64_t *sizes);
/* Host only: the List CSR of rf_fileset_tree over the forest's node numbering
 * (entry_ptr of the copy is the tree's entry_ptr as it stands) and one root per
 * document, 0xffffffff for a refused one.  list_child has room for n_nodes. */
int rf_fileset_forest_tree(const uint64_t *doc_node_ptr, uint64_t n_docs, const uint32_t *node_depth,
                           uint64_t n_nodes, uint64_t *list_ptr /* n_nodes + 1 */, uint32_t *list_child,
                           uint32_t *roots /* n_docs */);
/* Host clock, milliseconds: ms[0] the upload of the host-input form (0 in the
 * device form), ms[1] the check passes and scans up to and including the
 * read-back, ms[2] the outputs' allocation + the scatter (each ends in a
 * synchronise). */
int rf_fileset_forest_times(const rf_fileset_forest *f, double ms[3]);
void rf_fileset_forest_free(rf_fileset_forest *f);

/* ---- Coalescing concurrent callers (SURVEY §8(b) "Threading") -----------
 * The reference digests files in <=60 goroutines (local/executor.go:41,
 * 522-538) and looks cache keys up in a goroutine per node (eval.go:402-411);
 * called one request at a time, each would be its own tiny device batch.  A
 * coalescer is a queue any number of threads call into: the first caller
 * that finds no flush running becomes the flusher, waits up to max_wait_us
 * (or until max_batch requests are queued), and runs ONE batched call --
 * rf_sha256_batch, rf_bloom_probe or rf_assoc_get -- for everything queued;
 * requests arriving meanwhile form the next batch.  Blocking calls (a cgo
 * call per goroutine) and async tickets (submit, then poll or wait) share
 * it.  A failed batch returns its status to every request in it. */
enum { RF_COALESCE_SHA256 = 1, RF_COALESCE_PROBE = 2, RF_COALESCE_ASSOC_GET = 3 };
typedef struct rf_coalescer rf_coalescer;
typedef struct rf_coalesce_ticket rf_coalesce_ticket;
/* target: the rf_bloom (PROBE) or rf_assoc (ASSOC_GET, with assoc_kind);
 * NULL for SHA256. */
int rf_coalescer_open(rf_ctx *ctx, int kind, void *target, int assoc_kind, uint64_t max_batch,
                      uint64_t max_wait_us, rf_coalescer **out);
void rf_coalescer_close(rf_coalescer *c); /* completes what is queued */
int rf_coalesce_sha256(rf_coalescer *c, const uint8_t *msg, uint64_t len, uint8_t *out32);
int rf_coalesce_probe(rf_coalescer *c, const uint8_t *digest32, uint8_t *contains);
int rf_coalesce_assoc_get(rf_coalescer *c, const uint8_t *key32, uint8_t *val32, uint8_t *found);
/* Async: msg and out32 must stay valid until the ticket is done. */
int rf_coalesce_sha256_async(rf_coalescer *c, const uint8_t *msg, uint64_t len, uint8_t *out32,
                             rf_coalesce_ticket **out);
/* *done = 1 once out32 is written (returns its status); a poll that finds the
 * queue idle flushes it. */
int rf_coalesce_poll(rf_coalescer *c, rf_coalesce_ticket *t, int *done);
int rf_coalesce_wait(rf_coalescer *c, rf_coalesce_ticket *t);
void rf_coalesce_ticket_free(rf_coalescer *c, rf_coalesce_ticket *t); /* completes it first */
/* Batches flushed, requests served, largest batch. */
int rf_coalescer_stats(rf_coalescer *c, uint64_t *batches, uint64_t *requests, uint64_t *largest);

/* ---- K2/K3: incremental digest DAG (Flow.Digest / CacheKeys) ------------
 * The host lowers a Flow graph (flow.go:653-802) into hash JOBS over digest
 * SLOTS.  Job j hashes a byte template (its digest material, flow.go:675-750
 * or the physical material of :764-792) into slot out_slot[j]; the template
 * has "holes": hole h of job j places the 32 digest bytes of slot
 * hole_slot[h] at byte hole_pos[h] of the material (the host already wrote
 * the 0x00 0x05 WD prefix in front of each hole).  Slots written by no job
 * are inputs (e.g. File IDs).  Jobs must form a DAG over slots. */
typedef struct {
    uint32_t n_jobs, n_slots;
    const uint32_t *out_slot;    /* [n_jobs]                                    */
    const uint64_t *tmpl_off;    /* [n_jobs] byte offset of job j's template in blob */
    const uint32_t *tmpl_len;    /* [n_jobs] material length (bytes)            */
    const uint64_t *hole_ptr;    /* [n_jobs+1] CSR into hole_pos/hole_slot      */
    const uint32_t *hole_pos;    /* byte position of the 32 digest bytes         */
    const uint32_t *hole_slot;   /* slot whose digest fills the hole            */
    const uint8_t *blob;         /* templates                                   */
    uint64_t blob_len;
} rf_graph_desc;

/* Device footprint of a loaded graph: ~104 B a job (records, queued flags,
 * lists, midstates), 84 B a slot (digest, reverse-edge pointer, the mark
 * kernels' 48-B per-slot plan), 16 B a hole, and the templates padded to
 * 64-B blocks. */
int rf_graph_load(rf_ctx *ctx, const rf_graph_desc *desc, rf_graph **out);
void rf_graph_destroy(rf_graph *g);
/* Set input-slot digests (e.g. changed File IDs); marks their transitive
 * dependents dirty.  Setting a job's output slot is RF_EINVAL.  On a graph
 * never recomputed (fresh from rf_graph_load) the digests are only written:
 * its first recompute is a full one. */
int rf_graph_set_slots(rf_graph *g, const uint32_t *slots, const uint8_t *digests32, uint32_t n);
/* Device-resident form of set_slots (indices and digests in HBM). */
int rf_graph_set_slots_device(rf_graph *g, const void *d_slots, const void *d_digests32, uint32_t n,
                              void *stream);
/* Recompute dirty jobs level by level (K3 frontier + K2 node digests).
 * full != 0 recomputes every job.  Early cut-off: a job whose digest did not
 * change does not dirty its consumers.  *out_recomputed (may be NULL) receives
 * the number of jobs hashed (synchronises).
 * Each incremental level runs in one of two kernel forms, chosen per level
 * and step from the input slots marked since the last step (set_slots /
 * update): the two-lane latency form, or -- when min(level jobs, marked
 * slots) reaches 24,576 (65,536 for levels of long jobs) -- the lane-per-job
 * throughput form; change sets of >= 98,304 slots also mark in the
 * throughput form.  Results are identical.  The thresholds are fixed per
 * graph: the defaults below, RF_K2_THRU / RF_K2_THRU_WIDE (read once when the
 * graph is loaded or restored; RF_K2_THRU also sets the mark threshold), or
 * rf_graph_set_forms. */
int rf_graph_recompute(rf_graph *g, int full, uint64_t *out_recomputed);
#define RF_K2_THRU_DEFAULT 24576ull      /* levels of short jobs */
#define RF_K2_THRU_WIDE_DEFAULT 65536ull /* levels of long jobs (the per-sample OpK) */
#define RF_K2_THRU_MARK_DEFAULT 98304ull /* the mark kernel's lean form */
/* Kernel-form thresholds for this graph's next incremental steps (tuning and
 * A/B; results never depend on them): 0 = always the throughput form,
 * UINT64_MAX = never.  Not thread-safe against a step in flight on the
 * graph: call it between steps (the caller owns the graph, as for set_slots). */
int rf_graph_set_forms(rf_graph *g, uint64_t thru, uint64_t thru_wide, uint64_t thru_mark);
/* Canonicalize's hand-over when copies collapse (flow.go:814-843, the
 * flowMap's first copy wins, :881-907): g, just loaded from the copies'
 * job table with the duplicates' jobs dropped and every hole re-pointed at
 * its class's first copy (same slot numbering), takes src's whole slot table
 * -- src is the copies' graph, fully recomputed -- device to device, and is
 * ready for incremental steps without a full recompute (the state
 * rf_graph_restore leaves).  Both graphs of one context, equal n_slots, no
 * change set pending on either, src recomputed: RF_EINVAL /
 * RF_EPRECONDITION otherwise.  The caller vouches that src's digests are
 * what g's jobs compute (they are: every kept job is src's, reading slots of
 * equal digests). */
int rf_graph_adopt_slots(rf_graph *g, rf_graph *src);
/* Asynchronous form (no count readback). */
int rf_graph_recompute_async(rf_graph *g, int full, void *stream);
/* rf_graph_set_slots_device + rf_graph_recompute_async(g, 0, stream) in one
 * call.  By default that is the mark kernel and the step's plain level
 * launches (measured faster than a graph replay); with RF_K2_GRAPH=1 it is ONE
 * graph launch (the mark kernel the graph's first node, its parameters updated
 * per call on the host).  The first call on a fresh graph runs a full
 * recompute. */
int rf_graph_update_recompute_async(rf_graph *g, const void *d_slots, const void *d_digests32, uint32_t n,
                                    void *stream);
int rf_graph_get_slots(rf_graph *g, const uint32_t *slots, uint32_t n, uint8_t *out32);
/* Device-resident gather: d_out32[i] = slot d_slots[i] (e.g. boundary digests
 * for rf_comm_allgather).  Asynchronous on `stream`. */
int rf_graph_gather_device(rf_graph *g, const void *d_slots, uint32_t n, void *d_out32, void *stream);
typedef struct {
    uint32_t n_jobs, n_slots, n_levels, max_level_jobs;
    uint64_t total_blocks, hole_count, template_bytes;
    uint64_t last_recomputed;
    float last_ms; /* device time of the last synchronous rf_graph_recompute (asynchronous
                    * incremental steps record no events: RF_K2_EVENTS=1 does) */
    uint32_t last_levels_lf;  /* levels the last plain incremental step ran in the throughput form */
    uint32_t last_mark_lf;    /* the last set_slots batch marked in the throughput form (0/1) */
    uint32_t last_levels_oct; /* levels the last plain incremental step ran in the octo form */
    uint32_t split_block0;    /* fused links split block 0's schedule over chain and producer: 0 off, 1 / 2 (RF_K2_SPLIT) */
    uint32_t last_sink_attach; /* level whose launch ran the sink list in the last plain step (UINT32_MAX: none) */
    uint32_t last_levels_half; /* levels the last plain step ran in 32-job latency-form workgroups */
} rf_graph_stats;
/* Fills the whole struct above (its round-4 layout, unchanged since; a field
 * added later comes with a new, sized entry point rather than a change to
 * this one). */
int rf_graph_stats_get(rf_graph *g, rf_graph_stats *out);

/* ---- Change feed: the cache keys a step changed, found on the device ------
 * After a step an incremental evaluator looks up again only the nodes whose
 * cache keys moved (Flow.CacheKeys, flow.go:796-802, then Eval.lookup's
 * Assoc.Get, eval.go:1172-1220).  An opt-in feed on a loaded graph reports
 * the job-output slots whose digests changed since the last poll, ascending,
 * with their new digests -- on the device, asynchronously on a stream, after
 * one plain incremental step with work proportional to the dirty set -- and a
 * fused lookup runs those keys through the liveset probe and the HBM assoc in
 * the same stream.  One feed per graph, owned by it: rf_graph_destroy frees
 * it.  A graph without a feed launches exactly what it launched before.
 * Footprint: 32 B a slot (the digests as last reported) + 2 bits a slot (mask
 * and pending bitmaps, padded to 8192 slots) + 4 B per input slot marked
 * between two polls.
 *
 * open: the graph must be recomputed with no change set pending and no
 * partition attached (RF_EPRECONDITION otherwise, as for a second open;
 * rf_graph_set_part on a graph with a feed is RF_EPRECONDITION too).  The
 * baseline is the slot table as it stands (steps queued on any stream
 * complete first).  mask_words: [ceil(n_slots / 64)], bit s (bit s % 64 of
 * word s / 64) = report slot s; NULL = every job-output slot.  Input slots
 * are never reported (the caller set them): a mask bit on one, or at or
 * beyond n_slots, is RF_EINVAL.
 *
 * poll: every tracked slot whose digest differs from what the feed last
 * reported for it (or from the baseline), strictly ascending, each with its
 * current digest.  Digests are compared, history is not replayed: a slot that
 * changed and changed back between polls is not reported; one that changed
 * twice is reported once, with the latest digest.  *found = the number of
 * such slots, *written = min(found, cap); the first `written` in ascending
 * order are written, the rest stay pending and lead the next poll (nothing is
 * ever lost; cap = 0 is a count, slots / digests32 may then be NULL).  The
 * host form returns RF_OK whether they all fit or not.  The device form is
 * asynchronous on `stream` (d_n2: u64 {found, written}); the caller orders it
 * after the step, on the same stream or otherwise, as everywhere in this ABI.
 * Modes (rf_graph_feed_stats.last_mode): RF_FEED_LISTED when since the
 * previous poll (or the open) input slots were set any number of times and
 * then exactly one plain incremental step ran -- rf_graph_recompute(_async)
 * with full = 0 or rf_graph_update_recompute_async -- and nothing wrote slots
 * after it: the poll compares that step's listed jobs, the slot-fused jobs of
 * the slots marked for it, and their fused chains; also when nothing happened
 * at all (only what earlier polls left pending).  RF_FEED_SCAN otherwise (two
 * steps, a full recompute, rf_graph_adopt_slots, a captured-graph step, slots
 * set after the step or not stepped yet) and with RF_FEED_FORCE_SCAN: every
 * tracked slot is compared.  The results are identical.
 *
 * lookup: the poll, then for every written key i: status[i] = 2 when `live`
 * (may be NULL: no liveset) does not contain it -- the assoc is not read,
 * vals32[i] zeroed; 1 = found in `a` under `kind`, vals32[i] the value; 0 =
 * NotExist, vals32[i] zeroed: what rf_graph_feed_poll + rf_bloom_probe +
 * rf_assoc_get give composed on the host.  Rows at and beyond `written` are
 * not touched.  g, live and a must share one context (RF_EINVAL).  A later
 * growth or compaction of `a` waits for the queued read, as for
 * rf_assoc_get_device.
 *
 * rf_graph_save ignores the feed; a restored graph has none. */
#define RF_FEED_FORCE_SCAN 1u /* poll flag: test / A-B control, see modes */
enum { RF_FEED_NONE = 0, RF_FEED_LISTED = 1, RF_FEED_SCAN = 2 };
typedef struct {
    uint64_t polls, polls_listed, polls_scan;
    uint32_t last_mode;     /* RF_FEED_* of the last poll */
    uint64_t tracked_slots; /* job-output slots under the mask */
    uint64_t device_bytes;  /* what the feed holds in HBM */
} rf_graph_feed_stats;
int rf_graph_feed_open(rf_graph *g, const uint64_t *mask_words);
int rf_graph_feed_close(rf_graph *g);
int rf_graph_feed_poll_device(rf_graph *g, uint32_t flags, uint64_t cap, void *d_slots /* u32[cap] */,
                              void *d_digests32 /* [cap][32] */, void *d_n2 /* u64[2]: found, written */,
                              void *stream);
int rf_graph_feed_poll(rf_graph *g, uint32_t flags, uint64_t cap, uint32_t *slots, uint8_t *digests32,
                       uint64_t *found, uint64_t *written);
int rf_graph_feed_lookup_device(rf_graph *g, rf_bloom *live /* may be NULL */, rf_assoc *a, int kind, uint32_t flags,
                                uint64_t cap, void *d_slots, void *d_keys32, void *d_status /* u8[cap] */,
                                void *d_vals32, void *d_n2, void *stream);
int rf_graph_feed_stats_get(rf_graph *g, rf_graph_feed_stats *out);

/* ---- Checkpoint / resume of a loaded DAG ------------------------
 * Reference: a run's State is marshalled after every runner step
 * (runner/runner.go:51-85) and the local executor restores its execs from
 * manifests (local/executor.go:122-200); memoization is the resume mechanism.
 * rf_graph_save writes the graph's lowered device form (job records, holes,
 * reverse edges, padded templates, midstates, level layout) AND its current
 * slot digests to `path` (written to path.tmp, fsync'ed, renamed), with a
 * SHA-256 per 64 MiB chunk and one over them.  Steps queued on any stream
 * complete first (device synchronise).  rf_graph_restore loads such a file on
 * ctx's device: the graph is ready for incremental steps (set_slots +
 * recompute) at once -- no lowering, no level analysis, no full recompute.
 * A partition (rf_graph_set_part) is not part of the file: re-attach it.
 * Errors: RF_EIO (cannot create / open / write), RF_EINVAL (not a graph
 * checkpoint, or another version), RF_EINTEGRITY (truncated, the bytes do
 * not match their checksums, or the structure is inconsistent:
 * errors.Integrity), RF_EPRECONDITION from save when input slots were set
 * since the last recompute (the file holds digests, not a pending change
 * set: recompute first). */
int rf_graph_save(rf_graph *g, const char *path);
int rf_graph_restore(rf_ctx *ctx, const char *path, rf_graph **out);

/* ---- One DAG over many GPUs ---------------------------------
 * Each rank loads its PIECE of the global job graph (rf_graph_load on a local
 * desc: its own jobs plus replicated ones, slots renumbered locally) and
 * attaches its place in the partition: EXPORTS (local slots other ranks
 * read; export i of rank r has boundary id r * max_export + i, max_export the
 * same on every rank) and IMPORTS (local input slots fed from another rank's
 * boundary id).  rf_graph_recompute_part runs bulk-synchronous supersteps:
 * local recompute; an OR all-reduce of the bitset of exports changed since
 * they were last sent (RCCL has no bitwise OR: all-gather + local OR); an
 * all-gather of the export digests; changed imports written and their local
 * consumers queued; until no export changed (one exchange when no rank
 * imports, e.g. 1000align split by sample with the shared reference-index
 * chain replicated).  Transport: comm (RCCL over xGMI) or fn, a host
 * all-gather (recv[r*bytes ..] = rank r's send; 0 = ok) for ranks without
 * RCCL (tests on gloo, ranks sharing a GPU). */
typedef struct {
    int nranks, rank;
    uint32_t max_export;
    uint32_t n_export;
    const uint32_t *export_slot;
    uint32_t n_import;
    const uint32_t *import_slot;
    const uint32_t *import_bid;
    int any_import; /* some rank imports something (the same on every rank) */
    /* Exchange rounds per recompute, the same on every rank: the most
     * rank-boundary crossings on any path of the global graph (rf_graph_split;
     * 1 for configs[3]: sample roots -> the global root).  > 0 selects the
     * fixed-round protocol -- recompute, then `rounds` times: all-gather every
     * export digest, write the imports that differ (queueing their consumers)
     * and recompute -- with no OR-reduce and no host round trip, so with an
     * rf_comm and out_recomputed == NULL the whole call is asynchronous on the
     * context's stream.  0: the superstep protocol above (until no change). */
    uint32_t rounds;
} rf_graph_part;
typedef int (*rf_host_allgather_fn)(void *user, const void *send, void *recv, uint64_t bytes);
/* Attach (or replace) g's partition.  Between steps only: RF_EPRECONDITION
 * when input slots were set on a recomputed graph since its last recompute. */
int rf_graph_set_part(rf_graph *g, const rf_graph_part *p);
int rf_graph_recompute_part(rf_graph *g, rf_comm *comm, rf_host_allgather_fn fn, void *user, int full,
                            uint64_t *out_recomputed);
/* The last exchange's gathered export digests (device, [nranks*max_export][32],
 * boundary-id order) and the supersteps the last recompute took. */
int rf_graph_part_gathered(rf_graph *g, const void **d_digests32, uint64_t *n, uint64_t *supersteps);
/* Host-only splitter: rank `rank`'s piece of a global desc, owner[j] = the
 * rank that hashes job j (-1: every rank, e.g. the shared reference index).
 * The piece's desc arrays are owned by the piece (its blob is the global
 * blob, not copied); global_of_local maps its slots back. */
typedef struct rf_graph_piece rf_graph_piece;
int rf_graph_split(const rf_graph_desc *global, int nranks, int rank, const int32_t *owner, rf_graph_piece **out);
void rf_graph_piece_free(rf_graph_piece *p);
int rf_graph_piece_desc(const rf_graph_piece *p, rf_graph_desc *out);
int rf_graph_piece_part(const rf_graph_piece *p, rf_graph_part *out);
int rf_graph_piece_slots(const rf_graph_piece *p, const uint32_t **global_of_local, uint32_t *n);

/* Eval.dirty (eval.go:874-887) for every node of a Flow graph at once:
 * dirty[i] = 1 iff no_cache_extern and node i is an OpExtern (is_extern[i])
 * or one of its Deps is dirty -- Deps only ("dirty considers only visible
 * nodes": not MapFlow, Parent or continuations).  Eval.todo consults it under
 * NoCacheExtern to skip a node's cache lookup (eval.go:910).  Node i's deps
 * are deps[dep_ptr[i] .. dep_ptr[i+1]).  The closure runs on the GPU (K3
 * reachability over reverse edges, one launch per level); the reference's
 * per-node recursion has no memo. */
int rf_flow_dirty(rf_ctx *ctx, uint64_t n, const uint64_t *dep_ptr, const uint32_t *deps,
                  const uint8_t *is_extern, int no_cache_extern, uint8_t *dirty);

/* ---- Evaluation plan: Eval.todo + Eval.lookup, top-down (eval.go:902-955,
 * 1163-1269) ----
 * Which nodes have to run, and which are cached: from the roots, a cacheable
 * node that is not dirty is looked up; a hit ends the walk there, a miss makes
 * the node TODO and its Deps are visited.  The reference runs one goroutine
 * per node and one Assoc.Get per key (the batching its comments ask for,
 * eval.go:403-405, 1190-1201); here the whole walk runs on the device as a
 * frontier traversal whose cut-off per node is the fused liveset probe +
 * assoc Get of rf_graph_feed_lookup_device.  An rf_eval_plan owns one Flow
 * graph's structure on the device: opened once, run many times.
 * A reached node i is looked up iff it is CACHEABLE (eval.go:908-913), not
 * INVALID, has at least one key (eval.go:1183-1188) and, under
 * no_cache_extern, is neither dirty (rf_flow_dirty's closure, eval.go:910)
 * nor an EXTERN nor a listed root (eval.go:1173).  It is a HIT iff one of its
 * keys, not ruled out by the liveset, has a nonzero value in the assoc under
 * `kind`; otherwise it is TODO and every dep not reached yet is reached.  A
 * node flagged DONE that is reached is DONE and is not expanded.  A node's
 * state depends on the node alone and the reached set is a closure, so every
 * result is independent of visit order and identical from run to run.
 * Out of scope: dep.Err short-circuiting (eval.go:924-929), MapFlow, Parent
 * and continuations (Deps only, as Eval.todo), partitioned graphs.  Bottom-up
 * mode and what follows the first round in either mode: rf_eval_wave below.
 * Device footprint of a plan (rf_eval_plan_stats' device_bytes): per node
 * 8 B dep pointer + 8 B key pointer + 4 B queue entry + 4 B hit-row index +
 * 4 B of flag / state / which / found bytes + bitmaps; 4 B per dep; 4 B per
 * key slot; 32 B per node that has keys (the hits' values, copied out of the
 * assoc at lookup time so a later growth or compaction cannot stale them);
 * plus, for the host-form calls, 32 B per key row and the list staging. */
typedef struct rf_eval_plan rf_eval_plan;
/* node flags */
#define RF_PLAN_F_CACHEABLE 1u /* OpIntern, OpExec or OpExtern */
#define RF_PLAN_F_EXTERN 2u    /* OpExtern */
#define RF_PLAN_F_INVALID 4u   /* Eval.Invalidate said so (eval.go:890-899, 1173) */
#define RF_PLAN_F_DONE 8u      /* already FlowDone: left alone, a satisfied dep */
/* node states */
#define RF_PLAN_UNSEEN 0 /* never reached: beneath hits or done nodes, or unreachable */
#define RF_PLAN_TODO 1
#define RF_PLAN_READY 2  /* TODO and every dep DONE or HIT (vacuous with no deps): what
                            todo turns into FlowNeedTransfer / FlowReady (eval.go:930-953) */
#define RF_PLAN_HIT 3
#define RF_PLAN_DONE 4   /* flagged done and reached */
#define RF_PLAN_MAX_KEYS 8
typedef struct {
    uint64_t n_nodes;
    uint32_t depth;       /* nodes on the longest path: the bound on rounds */
    uint32_t rounds;      /* round launches of the last run / reject */
    uint32_t round_batch; /* rounds enqueued between two host reads */
    uint32_t round_lanes; /* lanes of one round launch (a fixed grid that strides) */
    uint32_t list_tile;   /* nodes per tile of the list's mark / scan / scatter */
    uint32_t reserved;
    uint64_t counts[5];   /* nodes per state after the last run / reject */
    uint64_t looked_up;   /* nodes looked up by the last run / reject */
    uint64_t keys_probed; /* their keys that went to the assoc */
    uint64_t keys_filtered; /* their keys the liveset ruled out */
    uint64_t device_bytes;
} rf_eval_plan_stats;
/* Node i's Deps are deps[dep_ptr[i] .. dep_ptr[i+1]) (rf_flow_dirty's CSR; a
 * dep may be listed twice); flags: one RF_PLAN_F_* byte per node; node i's
 * CacheKeys (flow.go:796-802, most concrete first) are key rows
 * [key_ptr[i], key_ptr[i+1]): at most RF_PLAN_MAX_KEYS, zero keys = the lookup
 * fails; key_slots (may be NULL): per key row, the slot of an rf_graph's slot
 * table that holds it.  RF_EINVAL for pointers that are not monotone, deps
 * out of range, a cycle, too many keys.  n < 2^32. */
int rf_eval_plan_open(rf_ctx *ctx, uint64_t n, const uint64_t *dep_ptr, const uint32_t *deps, const uint8_t *flags,
                      const uint64_t *key_ptr, const uint32_t *key_slots, rf_eval_plan **out);
/* The structural checks of rf_eval_plan_open and *depth (may be NULL; nodes on
 * the longest path) on the host alone: no context, no device. */
int rf_eval_plan_check(uint64_t n, const uint64_t *dep_ptr, const uint32_t *deps, uint32_t *depth);
void rf_eval_plan_close(rf_eval_plan *p);
/* Replace the flag bytes of the listed nodes (after a node ran: DONE; after an
 * invalidation).  Results of the last run stay as they are. */
int rf_eval_plan_set_flags(rf_eval_plan *p, const uint32_t *nodes, const uint8_t *flags, uint64_t n);
/* Run from `roots` (host array; duplicates are harmless).  Keys: with g, row r
 * is slot key_slots[r] of g's slot table (needs key_slots at open, and g
 * recomputed with no input change pending: RF_EPRECONDITION otherwise); else
 * d_keys32, device rows in key_ptr order.  live may be NULL; a key it does not
 * contain is not looked up and counts as NotExist, as
 * rf_graph_feed_lookup_device.  Every object of one context (RF_EINVAL).  The
 * call holds the context's lock, so no Put swaps the table under it, and
 * returns when the plan is complete. */
int rf_eval_plan_run(rf_eval_plan *p, const uint32_t *roots, uint64_t n_roots, int no_cache_extern, rf_graph *g,
                     const void *d_keys32, rf_bloom *live, rf_assoc *a, int kind, void *stream);
int rf_eval_plan_run_host(rf_eval_plan *p, const uint32_t *roots, uint64_t n_roots, int no_cache_extern,
                          const uint8_t *keys32, rf_bloom *live, rf_assoc *a, int kind);
/* The caller's post-checks failed for these hits (no fsid that unmarshals,
 * missing files, RecomputeEmpty: eval.go:1210-1246): they become TODO, their
 * deps join the frontier and the traversal goes on to its fixed point, with
 * the no_cache_extern of the last run; the other states are kept.  Every
 * listed node must be a HIT: RF_EINVAL otherwise, the plan untouched.  With
 * an unchanged assoc and liveset the result equals a fresh run with
 * RF_PLAN_F_INVALID on those nodes. */
int rf_eval_plan_reject(rf_eval_plan *p, const uint32_t *nodes, uint64_t n, rf_graph *g, const void *d_keys32,
                        rf_bloom *live, rf_assoc *a, int kind, void *stream);
int rf_eval_plan_reject_host(rf_eval_plan *p, const uint32_t *nodes, uint64_t n, const uint8_t *keys32,
                             rf_bloom *live, rf_assoc *a, int kind);
/* Results of the last run / reject.  state: one RF_PLAN_* byte per node. */
int rf_eval_plan_states(rf_eval_plan *p, uint8_t *state);
int rf_eval_plan_states_device(rf_eval_plan *p, const void **d_state);
/* The nodes in `state`, strictly ascending (a tile mark / scan / scatter over
 * the state array, never arrival order).  For RF_PLAN_HIT each listed node
 * also gets which (index of its first key with a value), vals32 (that value)
 * and key_found (bit j: key j has a value -- every key of a looked-up node is
 * probed, so read repair can be precise); any of the three may be NULL.
 * *found = the nodes in the state; if *found > cap: RF_EINVAL, *found still
 * set, and nothing at or beyond cap is written (cap 0 counts; the outputs
 * may then be NULL).  The device form writes ranks below cap and *d_found
 * (u64) on `stream`; the caller compares. */
int rf_eval_plan_list(rf_eval_plan *p, int state, uint64_t cap, uint32_t *nodes, uint8_t *which, uint8_t *vals32,
                      uint8_t *key_found, uint64_t *found);
int rf_eval_plan_list_device(rf_eval_plan *p, int state, uint64_t cap, void *d_nodes, void *d_which,
                             void *d_vals32, void *d_key_found, void *d_found /* u64 */, void *stream);
/* size = sizeof(rf_eval_plan_stats) of the caller's header. */
int rf_eval_plan_stats_get(rf_eval_plan *p, rf_eval_plan_stats *out, uint64_t size);

/* ---- Evaluation waves: bottom-up evaluation and the completion step
 * (eval.go:902-955, 1163-1269, Deps only) ----
 * Which nodes are ready now that these have finished.  The reference walks
 * the graph from the roots on every scheduling step; an rf_eval_wave keeps,
 * per node, PENDING -- the number of its dep entries whose dep has not
 * finished -- and the consumer edges, so a step costs in proportion to what
 * finished.  Node flags, states and key rows are the plan's (RF_PLAN_F_*,
 * RF_PLAN_UNSEEN / TODO / READY / HIT / DONE, key_ptr / key_slots,
 * RF_PLAN_MAX_KEYS); the object owns its own copy of the structure.
 *   begin, bottom-up (-eval=bottomup, eval.go:301-321): from the listed roots
 * every reached node not flagged DONE becomes TODO and all its deps are
 * reached, with no lookups on the way down (eval.go:910); a reached node
 * flagged DONE is DONE and is not expanded.  pending[i] = the dep entries of i
 * whose dep is not flagged DONE; the reached nodes with none are wave 0.
 *   begin from states, the top-down continuation: the state bytes of an
 * rf_eval_plan (rejects applied).  TODO and READY nodes are tracked, HIT and
 * DONE are satisfied (DONE here), UNSEEN stays; pending[i] = the dep entries
 * whose dep is TODO or READY; wave 0 = the tracked nodes with none, i.e. the
 * plan's READY list.  Nothing is ever looked up in this mode (eval.go:943-947).
 *   A wave is resolved node by node.  Bottom-up, a node is looked up iff it is
 * CACHEABLE, not INVALID, has at least one present key and, under
 * no_cache_extern, is neither an EXTERN nor a listed root (eval.go:1173);
 * rf_flow_dirty's closure is not consulted (Eval.lookup never calls dirty,
 * only top-down todo does).  It is a HIT iff one of its present keys, not
 * ruled out by the liveset, has a nonzero value in the assoc under `kind`
 * (every present key is probed; which, the value -- copied out at lookup
 * time -- and the found mask are kept); a miss is READY (lookupFailed in
 * bottom-up mode is NeedTransfer, eval.go:1163-1166), and so is a node that
 * is not looked up.  A key row of 32 zero bytes is absent (PhysicalDigest not
 * computable yet, flow.go:762-774, 798-800): not probed, not counted, its
 * found bit clear; `which` stays the row index.
 *   step: the listed nodes have finished -- they ran, or they are hits the
 * caller accepted (unmarshal, rf_repo_missing).  Each must be READY or HIT
 * (RF_EINVAL otherwise, the object untouched); a node listed twice counts
 * once.  They become DONE, every consumer entry of each whose consumer is
 * tracked takes one decrement of pending, and the consumers that reach zero
 * are the next wave, resolved as above with the keys as they are now (a
 * consumer's physical key moves when its deps' values are set).  There is no
 * cascade inside a step: a hit is not DONE until the caller says so.
 *   reject: the listed HITs failed the caller's post-checks and become READY.
 * Every result depends only on the set of nodes finished so far, and the
 * decrement that reaches zero is unique, so states, lists and counts are
 * identical from run to run.  Calls hold the context's lock and return when
 * complete; every object of one context (RF_EINVAL).
 * Out of scope: dep.Err short-circuiting (eval.go:924-929); MapFlow, Parent
 * and continuations, graphs that grow at run time; partitioned graphs; any
 * hand-off between workgroups inside a kernel -- everything one kernel writes
 * for the next is read only after the kernel boundary.
 * Device footprint (rf_eval_wave_stats' device_bytes): per node 8 B dep
 * pointer + 8 B consumer pointer + 8 B key pointer + 4 B pending + 4 B + 4 B
 * queue entries + 4 B hit-row index + 4 B of flag / state / which / found
 * bytes + four bitmaps; 8 B per dep entry (dep and consumer); 4 B per key
 * slot; 32 B per node that has keys; plus, for the host-form calls, 32 B per
 * key row, 1 B per node of begin_states input and the list staging. */
typedef struct rf_eval_wave rf_eval_wave;
/* list scopes */
#define RF_WAVE_ALL 0  /* every node in the state */
#define RF_WAVE_LAST 1 /* only nodes that entered by the last begin or step */
typedef struct {
    uint64_t n_nodes;
    uint64_t n_deps;      /* dep entries = consumer entries */
    uint32_t depth;       /* nodes on the longest path: the bound on descent rounds */
    uint32_t mode;        /* 0: no begin yet, 1: bottom-up, 2: top-down continuation */
    uint32_t waves;       /* begin and step calls since (and with) the last begin */
    uint32_t last_wave;   /* nodes that entered by the last begin or step */
    uint32_t rounds;      /* descent launches of the last begin */
    uint32_t round_batch; /* descent rounds enqueued between two host reads */
    uint32_t wave_lanes;  /* lanes of one descent / resolve launch (a fixed grid that strides) */
    uint32_t list_tile;   /* nodes per tile of the list's mark / scan / scatter */
    uint64_t counts[5];   /* nodes per state now */
    uint64_t looked_up;   /* nodes looked up by the last begin or step */
    uint64_t keys_probed; /* their keys that went to the assoc */
    uint64_t keys_filtered; /* their keys the liveset ruled out */
    uint64_t device_bytes;
} rf_eval_wave_stats;
/* Host only, no context: the consumer CSR of rf_eval_plan_open's dep CSR.
 * cons_ptr [n+1], cons [dep_ptr[n]]: for node d the nodes that list d as a
 * dep, one entry per dep entry (a dep listed twice gives two), ascending
 * within a node.  RF_EINVAL as rf_eval_plan_check (a cycle included) and for
 * a NULL output. */
int rf_eval_wave_consumers(uint64_t n, const uint64_t *dep_ptr, const uint32_t *deps, uint64_t *cons_ptr,
                           uint32_t *cons);
/* rf_eval_plan_open's arguments and checks. */
int rf_eval_wave_open(rf_ctx *ctx, uint64_t n, const uint64_t *dep_ptr, const uint32_t *deps, const uint8_t *flags,
                      const uint64_t *key_ptr, const uint32_t *key_slots, rf_eval_wave **out);
void rf_eval_wave_close(rf_eval_wave *w);
/* Replace the flag bytes of the listed nodes, for the next begin. */
int rf_eval_wave_set_flags(rf_eval_wave *w, const uint32_t *nodes, const uint8_t *flags, uint64_t n);
/* Begin bottom-up from `roots` (host array; duplicates are harmless) and
 * resolve wave 0.  Keys, live, a, kind, stream: as rf_eval_plan_run. */
int rf_eval_wave_begin(rf_eval_wave *w, const uint32_t *roots, uint64_t n_roots, int no_cache_extern, rf_graph *g,
                       const void *d_keys32, rf_bloom *live, rf_assoc *a, int kind, void *stream);
int rf_eval_wave_begin_host(rf_eval_wave *w, const uint32_t *roots, uint64_t n_roots, int no_cache_extern,
                            const uint8_t *keys32, rf_bloom *live, rf_assoc *a, int kind);
/* Begin from one RF_PLAN_* byte per node (rf_eval_plan_states, or with
 * on_device rf_eval_plan_states_device; the bytes are copied).  RF_EINVAL,
 * the object unchanged, for a byte above RF_PLAN_DONE or a TODO / READY node
 * with an UNSEEN dep. */
int rf_eval_wave_begin_states(rf_eval_wave *w, const void *state, int on_device, void *stream);
/* The listed nodes (host array) have finished; the next wave is resolved.
 * n == 0 is valid and gives an empty wave.  Keys as rf_eval_wave_begin, read
 * now: with g, RF_EPRECONDITION while an input change is pending.  In the
 * top-down continuation keys, live and a are not read and may be NULL.
 * RF_EPRECONDITION before any begin. */
int rf_eval_wave_step(rf_eval_wave *w, const uint32_t *nodes, uint64_t n, rf_graph *g, const void *d_keys32,
                      rf_bloom *live, rf_assoc *a, int kind, void *stream);
int rf_eval_wave_step_host(rf_eval_wave *w, const uint32_t *nodes, uint64_t n, const uint8_t *keys32, rf_bloom *live,
                           rf_assoc *a, int kind);
/* These hits failed the caller's post-checks: READY.  RF_EINVAL, the object
 * untouched, if one of them is not a HIT. */
int rf_eval_wave_reject(rf_eval_wave *w, const uint32_t *nodes, uint64_t n);
/* One RF_PLAN_* byte per node, as of now. */
int rf_eval_wave_states(rf_eval_wave *w, uint8_t *state);
int rf_eval_wave_states_device(rf_eval_wave *w, const void **d_state);
/* rf_eval_plan_list's rules (strictly ascending, a tile mark / scan / scatter
 * over the state array; which / vals32 / key_found for RF_PLAN_HIT; the cap
 * rule), over every node (RF_WAVE_ALL) or only the members of the last wave
 * (RF_WAVE_LAST: a bitmap cleared per step carries the membership; a member
 * that a reject made READY is still a member). */
int rf_eval_wave_list(rf_eval_wave *w, int state, int scope, uint64_t cap, uint32_t *nodes, uint8_t *which,
                      uint8_t *vals32, uint8_t *key_found, uint64_t *found);
int rf_eval_wave_list_device(rf_eval_wave *w, int state, int scope, uint64_t cap, void *d_nodes, void *d_which,
                             void *d_vals32, void *d_key_found, void *d_found /* u64 */, void *stream);
/* size = sizeof(rf_eval_wave_stats) of the caller's header. */
int rf_eval_wave_stats_get(rf_eval_wave *w, rf_eval_wave_stats *out, uint64_t size);

/* ---- GC liveset: Eval.collect's walk, dedup and filter build (eval.go:791-868) ----
 * What is live, as a bloom filter, without a host walk of the graph.  An
 * rf_liveset owns one Flow graph's edges and its nodes' current Fileset values
 * on the device: opened once, updated as nodes finish, run once per
 * collection.
 * Graph: rf_eval_plan_open's CSR (an edge may be listed twice; monotone
 * pointers, range and no cycle are checked as there; n < 2^32).  Node i's
 * edges are its Deps; for an OpMap node the caller appends its MapFlow
 * (eval.go:822-824).
 * Values: a node has a value iff State == FlowDone and Value is a Fileset: its
 * rows are the (ID, Size) of the Fileset's Map entries with List flattened
 * recursively, exactly Fileset.N() of them (executor.go:95-102; duplicates
 * kept, zero rows valid).  A Done node whose value is not a Fileset has no
 * value here (the reference expands it).
 * Walk (eval.go:809-826) from the listed roots: a reached node with a value is
 * RF_LIVE_VALUE and is not expanded; every other reached node is
 * RF_LIVE_WALKED and all its edges are reached; the rest stays
 * RF_LIVE_UNSEEN.  A node's state depends on the node alone and the reached
 * set is a closure, so every result is identical from run to run.
 * Contributions: the RF_LIVE_VALUE nodes ascending, then each entry of
 * `writers` in the caller's order (eval.go:827-835); a writer without a value
 * contributes zero rows; a writer on the frontier, or listed twice,
 * contributes twice (the reference appends a second *Fileset).
 * nlive_est = rows over all contributions (N(), not unique); the filter is
 * bloom.NewWithEstimates(nlive_est, 0.001) (rf_bloom_estimate, then max(1, .):
 * bloom.go:81-83, 120-131), or bloom.New(64, 1) when nlive_est is 0
 * (eval.go:842); its bitset length is m.  Every row's WD(ID) is added.
 * nlive / livebytes: per contribution separately the distinct (ID, Size)
 * pairs (Files() is a map[File]bool per value): their number and the sum of
 * their sizes over the contributions.
 * changed (eval.go:862): 1 on the first run, then 1 iff m, k, the length or a
 * word differ from the previous run's filter (the object keeps it; the two
 * alternate).  maxlivebytes: the running maximum of livebytes.
 * A run may have at most RF_LIVE_MAX_ROWS rows (nlive_est): RF_EINVAL beyond,
 * the object left usable.  A run that fails after its walk (that refusal, or
 * RF_EDEVICE) keeps the previous run's filter, statistics and maxlivebytes;
 * the states and lists are then undefined until the next run that succeeds.  Replaced and cleared values leave their rows stale
 * in the arena until close (stale_rows); there is no compaction. */
typedef struct rf_liveset rf_liveset;
#define RF_LIVE_UNSEEN 0
#define RF_LIVE_WALKED 1
#define RF_LIVE_VALUE 2
#define RF_LIVE_MAX_ROWS 1073741824 /* 2^30 rows per run: the dedup table indexes rows with 32 bits */
#define RF_LIVE_LIST_TILE 1024      /* nodes per tile of the list's mark / scan / scatter */
#define RF_LIVE_ROUND_BATCH 4       /* walk rounds enqueued between two host reads */
typedef struct {
    uint64_t n_nodes, counts[3];     /* nodes per state after the last run */
    uint64_t contributions;          /* frontier values + writer entries */
    uint64_t nlive_est, nlive;       /* eval.go:813-814 and :856 */
    int64_t livebytes, maxlivebytes;
    uint64_t m, k;
    uint32_t rounds, changed;        /* rounds: round launches enqueued, in batches of RF_LIVE_ROUND_BATCH
                                        (trailing ones may have found an empty frontier); <= the depth bound */
    uint64_t arena_rows, stale_rows; /* rows stored; rows of replaced / cleared values */
    uint64_t device_bytes;
} rf_liveset_stats;
/* bloom.EstimateParameters (bloom.go:120-124) in double, on the host alone:
 * m = ceil(-n ln p / ln^2 2), k = ceil(ln 2 * m / n).  RF_EINVAL for n = 0 or
 * p outside (0, 1). */
int rf_bloom_estimate(uint64_t n, double p, uint64_t *m, uint64_t *k);
int rf_liveset_open(rf_ctx *ctx, uint64_t n, const uint64_t *edge_ptr, const uint32_t *edges, rf_liveset **out);
void rf_liveset_close(rf_liveset *l);
/* nodes[i] now has the value rows [sum(counts[0..i)), +counts[i]) of ids32 /
 * sizes; it replaces an older one (a node listed twice keeps its last).
 * RF_EINVAL for a node >= n or a row total that overflows.  The device form
 * reads the rows from device memory on `stream` and returns when they are
 * stored.  A call that fails changes no value. */
int rf_liveset_set_values(rf_liveset *l, const uint32_t *nodes, const uint32_t *counts, uint64_t n_nodes,
                          const uint8_t *ids32, const int64_t *sizes);
int rf_liveset_set_values_device(rf_liveset *l, const uint32_t *nodes, const uint32_t *counts, uint64_t n_nodes,
                                 const void *d_ids32, const void *d_sizes, void *stream);
/* These nodes are no longer FlowDone: they have no value. */
int rf_liveset_clear_values(rf_liveset *l, const uint32_t *nodes, uint64_t n_nodes);
/* One collection (roots, writers: host arrays; duplicates as above).  Holds
 * the context's lock and returns when the filter is complete. */
int rf_liveset_run(rf_liveset *l, const uint32_t *roots, uint64_t n_roots, const uint32_t *writers,
                   uint64_t n_writers, void *stream);
/* The last run's filter, borrowed: valid until the next run or close, for
 * every rf_bloom_* call that reads a filter (probe, collect, params, words,
 * the marshalers, and as the liveset of a plan or feed lookup);
 * rf_bloom_destroy on it is a no-op.  RF_EPRECONDITION before the first run. */
int rf_liveset_filter(rf_liveset *l, rf_bloom **b);
/* Results of the last run: one RF_LIVE_* byte per node; the nodes in `state`,
 * strictly ascending, with the cap rule of rf_eval_plan_list. */
int rf_liveset_states(rf_liveset *l, uint8_t *state);
int rf_liveset_list(rf_liveset *l, int state, uint64_t cap, uint32_t *nodes, uint64_t *found);
/* size = sizeof(rf_liveset_stats) of the caller's header. */
int rf_liveset_stats_get(rf_liveset *l, rf_liveset_stats *out, uint64_t size);

/* ---- K4: bloomlive / assoc probe (bloom.go:182-190, bloomlive.go:30-36) --
 * Filters cache-key lookups before Assoc.Get (eval.go:1202-1220) and serves
 * Liveset.Contains for Repository.Collect (repository/file/repository.go:304-327). */
/* words: bitset words (uint64, bit i in word i>>6); length = bitset length in bits. */
int rf_bloom_load(rf_ctx *ctx, uint64_t m, uint64_t k, const uint64_t *words, uint64_t nwords,
                  uint64_t length, rf_bloom **out);
/* Go JSON wire form {"m":M,"k":K,"b":"<base64url(BE64 len ‖ BE64 words)>"} (bloom.go:264-286). */
int rf_bloom_load_json(rf_ctx *ctx, const char *json, size_t len, rf_bloom **out);
/* The liveset's wire forms on the host alone (no device; what the loaders
 * above and the marshalers below use): parse into m, k, the bitset length
 * and its wordsNeeded(length) words (*n_words; RF_EINVAL with *n_words set
 * when cap_words is short), and format from host words (*out_len = bytes
 * needed, RF_EINVAL when cap is short).  Malformed or truncated input is
 * RF_EINVAL, never a read past len. */
int rf_bloom_parse_binary(const uint8_t *buf, size_t len, uint64_t *m, uint64_t *k, uint64_t *length,
                          uint64_t *words, uint64_t cap_words, uint64_t *n_words);
int rf_bloom_parse_json(const char *json, size_t len, uint64_t *m, uint64_t *k, uint64_t *length,
                        uint64_t *words, uint64_t cap_words, uint64_t *n_words);
int rf_bloom_format_binary(uint64_t m, uint64_t k, uint64_t length, const uint64_t *words, uint64_t n_words,
                           uint8_t *out, uint64_t cap, uint64_t *out_len);
int rf_bloom_format_json(uint64_t m, uint64_t k, uint64_t length, const uint64_t *words, uint64_t n_words,
                         uint8_t *out, uint64_t cap, uint64_t *out_len);
/* Go binary wire form BE64 m ‖ BE64 k ‖ BE64 len ‖ BE64 words (bloom.go:290-325). */
int rf_bloom_load_binary(rf_ctx *ctx, const uint8_t *buf, size_t len, rf_bloom **out);
/* New empty filter with m bits and k hashes (bloom.New, bloom.go:81-83). */
int rf_bloom_new(rf_ctx *ctx, uint64_t m, uint64_t k, rf_bloom **out);
void rf_bloom_destroy(rf_bloom *b);
/* out[i] = Contains(digest i): key = WD(d), all k bits set. */
int rf_bloom_probe(rf_bloom *b, const uint8_t *digests32, uint64_t n, uint8_t *out);
int rf_bloom_probe_device(rf_bloom *b, const void *d_digests32, uint64_t n, void *d_out,
                          void *stream);
/* Add WD(d) for each digest (eval.go:848-858 build side). */
int rf_bloom_add(rf_bloom *b, const uint8_t *digests32, uint64_t n);
int rf_bloom_add_device(rf_bloom *b, const void *d_digests32, uint64_t n, void *stream);
/* Read back m, k, length and the words (nwords = ceil(length/64) capacity). */
int rf_bloom_params(rf_bloom *b, uint64_t *m, uint64_t *k, uint64_t *length, uint64_t *nwords);
int rf_bloom_words(rf_bloom *b, uint64_t *words, uint64_t nwords);
/* Wire formats out (liveset build side, POST /collect body): Go MarshalJSON
 * {"m":M,"k":K,"b":"<base64.URLEncoding(BE64 len ‖ BE64 words)>"} (bloom.go:270-273,
 * bitset.go:693-702) and WriteTo BE64 m ‖ BE64 k ‖ bitset (bloom.go:290-301).
 * *out_len = bytes needed; RF_EINVAL if cap is short. */
int rf_bloom_marshal_json(rf_bloom *b, uint8_t *out, uint64_t cap, uint64_t *out_len);
int rf_bloom_marshal_binary(rf_bloom *b, uint8_t *out, uint64_t cap, uint64_t *out_len);
/* Repository.Collect (repository/file/repository.go:304-327) over n objects:
 * dead_idx[0 .. *n_dead) = the indices i, ascending, whose digest the liveset
 * does not contain (the objects Collect removes); *dead_bytes (may be NULL) =
 * the sum of their sizes (sizes may be NULL).  n < 2^32. */
int rf_bloom_collect(rf_bloom *b, const uint8_t *digests32, const int64_t *sizes, uint64_t n,
                     uint64_t *dead_idx, uint64_t *n_dead, int64_t *dead_bytes);
/* Device-resident form: d_counts2 receives {n_dead (u64), dead_bytes (i64)}. */
int rf_bloom_collect_device(rf_bloom *b, const void *d_digests32, const void *d_sizes, uint64_t n,
                            void *d_dead_idx, void *d_counts2, void *stream);

/* ---- K5: Canonicalize's flowMap (flow.go:814-843, flowMap.Get/Put :881-907) --
 * canon[i] = min{ j : digests[j] == digests[i] } over n node digests.  With
 * nodes numbered in the post-order of canonicalize's recursion (the order of
 * its m.Put calls) this is the flow the reference's first Put registers: the
 * canonical representative.  *n_unique = |{ i : canon[i] == i }|.  n <= 2^30. */
int rf_dedup_digests(rf_ctx *ctx, const uint8_t *digests32, uint32_t n, uint32_t *canon,
                     uint32_t *n_unique);
/* Device-resident form (digests e.g. gathered from rf_graph slots), on
 * `stream`.  *d_n_unique (uint32) gets the class count; its bit 31 set means
 * the batch hit the kernel's probe bound (65536 slots of linear probing at
 * load <= 1/2: not reachable for SHA-256 digests) and the result
 * must not be used -- rf_dedup_digests returns RF_EDEVICE for it. */
int rf_dedup_digests_device(rf_ctx *ctx, const void *d_digests32, uint32_t n, void *d_canon,
                            void *d_n_unique, void *stream);

/* ---- HBM assoc (assoc.Assoc, assoc/assoc.go:26-38) -----------------------
 * A digest -> digest map per kind in HBM with the semantics of the in-memory
 * assoc (test/testutil/assoc.go:34-56): the cache tier behind the probe, in
 * front of DynamoDB (assoc/dydbassoc).  Batched. */
int rf_assoc_new(rf_ctx *ctx, uint64_t capacity, rf_assoc **out);
void rf_assoc_destroy(rf_assoc *a);
/* Put, op i in batch order (ops on one key apply in index order): if
 * expect32 (may be NULL) row i is nonzero and the current value differs,
 * status[i] = RF_EPRECONDITION and nothing changes; else the value becomes
 * vals32[i] (all-zero deletes) and status[i] = RF_OK. */
int rf_assoc_put(rf_assoc *a, int kind, const uint8_t *expect32, const uint8_t *keys32,
                 const uint8_t *vals32, uint64_t n, int32_t *status);
/* Device-resident form (d_status: int32 per op); returns when applied. */
int rf_assoc_put_device(rf_assoc *a, int kind, const void *d_expect32, const void *d_keys32,
                        const void *d_vals32, uint64_t n, void *d_status);
/* Get: found[i] = 1 and vals32[i] = the value, or found[i] = 0 (NotExist,
 * vals32[i] zeroed). */
int rf_assoc_get(rf_assoc *a, int kind, const uint8_t *keys32, uint64_t n, uint8_t *vals32,
                 uint8_t *found);
int rf_assoc_get_device(rf_assoc *a, int kind, const void *d_keys32, uint64_t n, void *d_vals32,
                        void *d_found, void *stream);
/* Abbreviated keys (dydbassoc.go:111-147, ID4 index + Digest.Expands): key i
 * is given by its first nhex[i] hex digits (8..64) in keys32 row i.  status
 * RF_OK with the expanded key and its value, RF_ENOTFOUND, or RF_EINVAL when
 * more than one key matches. */
int rf_assoc_get_abbrev(rf_assoc *a, int kind, const uint8_t *keys32, const uint8_t *nhex, uint64_t n,
                        uint8_t *keys_out32, uint8_t *vals32, int32_t *status);
/* Eval.lookup's assoc step for a batch of nodes (eval.go:1172-1220), read
 * only: node i's cache keys (CacheKeys order, most to least concrete) are
 * keys32 rows [key_ptr[i], key_ptr[i+1]); all of them go in one Get batch (the
 * batching the TODO at eval.go:1199-1201 asks for).  which[i] = index within
 * the node of its first key with a value (vals32[i] = that value, the Fileset
 * id), or -1 (vals32[i] zeroed).  key_found / key_vals32 (either may be NULL):
 * per key, found and value -- the later candidates the caller tries when the
 * first fsid does not unmarshal (eval.go:1210-1218 moves on to the next key).
 * Nothing is written: read repair waits for the caller's checks
 * (rf_assoc_repair). */
int rf_assoc_lookup(rf_assoc *a, int kind, const uint8_t *keys32, const uint64_t *key_ptr, uint64_t n_nodes,
                    int32_t *which, uint8_t *vals32, uint8_t *key_found, uint8_t *key_vals32);
/* Read repair after the caller's checks (eval.go:1227-1258): node i takes part
 * iff which[i] >= 0 -- the key whose fsid unmarshalled and whose files all
 * exist (missing(), and not an empty value under RecomputeEmpty); the caller
 * sets which[i] = -1 for every other node.  Put(zero expect, key, vals32[i])
 * under every other key of the node (the reference's blind write-back), or,
 * with key_found (rf_assoc_lookup's) given, only under the keys that were
 * missing (precise read repair, the TODO at eval.go:1199-1201).  One Put
 * batch, node order then key order. */
int rf_assoc_repair(rf_assoc *a, int kind, const uint8_t *keys32, const uint64_t *key_ptr, uint64_t n_nodes,
                    const int32_t *which, const uint8_t *vals32, const uint8_t *key_found);
/* Occupied slots (live + deleted keys) and table capacity. */
int rf_assoc_stats(rf_assoc *a, uint64_t *occupied, uint64_t *capacity);
/* Enumeration: what a shim needs to write the tier behind to DynamoDB (one
 * dydbassoc Put per live key, assoc/dydbassoc/dydbassoc.go:40-99) and to
 * inspect it -- the contents of the in-memory assoc's map
 * (test/testutil/assoc.go:21-24), which assoc.Assoc (assoc/assoc.go:26-39)
 * itself cannot list.
 * kind >= 0: that kind; kind < 0: every kind.  live = entries with a nonzero
 * value, deleted = occupied slots whose value is zero (assoc.Delete is Put of
 * a zero value, assoc/assoc.go:41-44).  For kind < 0, live + deleted ==
 * rf_assoc_stats' occupied. */
int rf_assoc_count(rf_assoc *a, int kind, uint64_t *live, uint64_t *deleted);
/* The live entries, each exactly once, in ascending slot order (the same
 * arrays for an unchanged table): keys32 / vals32 rows of 32 B, kinds (int32
 * per entry; required when kind < 0, may be NULL otherwise).  *n = the number
 * of live entries.  If *n > cap_entries: RF_EINVAL, *n still set, and no row
 * at index >= cap_entries is written. */
int rf_assoc_scan(rf_assoc *a, int kind, uint64_t cap_entries, uint8_t *keys32, uint8_t *vals32,
                  int32_t *kinds, uint64_t *n);
/* Device-resident form on `stream`: rows below cap_entries are written, *d_n
 * (u64) gets the number of live entries whether they fit or not (the caller
 * compares).  A later growth or compaction waits for it before it frees the
 * table it reads. */
int rf_assoc_scan_device(rf_assoc *a, int kind, uint64_t cap_entries, void *d_keys32, void *d_vals32,
                         void *d_kinds, void *d_n /* u64 */, void *stream);
/* Rebuild the table without its deleted keys (growth carries them; the
 * in-memory assoc drops the map entry at once, test/testutil/assoc.go:41-42):
 * afterwards occupied == live and capacity = the smallest power of two >=
 * max(1024, 2 * max(live, min_capacity)).  Every Get / Put / abbreviated Get
 * behaves as before the call. */
int rf_assoc_compact(rf_assoc *a, uint64_t min_capacity);
/* The assoc across processes: memoization is the resume mechanism, and the
 * assoc is where a run's cache entries outlive it (Eval.lookup reads them
 * back, eval.go:1172-1220).
 * save writes the live entries to `path` (beside it first, then renamed);
 * restore checks the whole file on the host -- RF_EINVAL for a file that is
 * not one (magic, version, flags, sizes, truncation) or whose entries break
 * the rules below, RF_EINTEGRITY for a checksum mismatch (errors.Integrity,
 * repository/file/repository.go:160-162); *out is then untouched -- and
 * bulk-loads a table of capacity = the smallest power of two >=
 * max(1024, 2 * entries).
 * File, little-endian: header 64 B (magic "RFASSOC1", u32 version = 1, u32
 * flags = 0, u64 n_entries, u64 chunk, 32 zero bytes); n_entries entries of
 * 68 B (u32 kind in [0, 2^30), 32-B key, 32-B nonzero value), strictly
 * ascending by (kind, key bytes), so equal contents give equal files; one
 * SHA-256 per `chunk` bytes of the entry area; SHA-256(header || those
 * digests); the end marker "RFASEND1". */
int rf_assoc_save(rf_assoc *a, const char *path);
int rf_assoc_restore(rf_ctx *ctx, const char *path, rf_assoc **out);
/* The file form on the host alone (no device), as rf_bloom_format_* /
 * rf_bloom_parse_*: chunk = checksum granule in bytes (0 = 64 MiB); the
 * entries are given in file order.  *out_len = bytes needed (RF_EINVAL when
 * cap is short); *n = the file's entries (RF_EINVAL with *n set when
 * cap_entries is short).  parse applies every check of rf_assoc_restore and
 * never reads past len. */
int rf_assoc_file_format(const int32_t *kinds, const uint8_t *keys32, const uint8_t *vals32, uint64_t n,
                         uint64_t chunk, uint8_t *out, uint64_t cap, uint64_t *out_len);
int rf_assoc_file_parse(const uint8_t *buf, uint64_t len, int32_t *kinds, uint8_t *keys32, uint8_t *vals32,
                        uint64_t cap_entries, uint64_t *n);

/* ---- Repository index in HBM: batched Stat, missing() and NeedTransfer ------
 * What a repository holds, as a set of object IDs with their sizes on the
 * device: the object map of the in-memory repository
 * (test/testutil/repository.go:25-115) and file.Repository.Stat
 * (repository/file/repository.go:93-101).  Against it run, for batches of
 * Fileset values, Eval.lookup's missing() (eval.go:1227-1243, 1983-2014) and
 * Manager.NeedTransfer (repository/manager.go:197-234; eval.go:412-444,
 * 1273-1282) -- one Repository.Stat goroutine per file in the reference, whose
 * own comment asks for a batch stat call -- and Repository.Collect
 * (repository/file/repository.go:304-327) on the index itself.
 * Table: open addressing, one slot = tag word, 32-B ID, int64 size; a removed
 * object leaves a tombstone.  Slots: the smallest power of two >=
 * max(RF_REPO_MIN_SLOTS, 2 * capacity), capacity <= 2^30.  Before a Put batch
 * of n rows the host compares live + tombstones + n with half the slots: beyond
 * it the table is rebuilt without its tombstones at twice the slots (doubled
 * again until live + n fit in half).  Probing is bounded (65536 slots at load
 * <= 1/2: not reachable for SHA-256 IDs); a call that hits the bound fails
 * with RF_EDEVICE, and so does every later call on the object (fail-stop; an
 * asynchronous device form reports it through the next call).  Every call
 * holds the context's lock; what a device form leaves on its stream is waited
 * for by the next call on the object.
 *
 * Put (content addressing: an ID determines its size): status[i] = RF_OK when
 * the ID is new, or present with the same size; RF_EINTEGRITY when the index,
 * or a row of the same batch with a lower index, gives the ID another size --
 * the stored size then stays as it was (first wins by row index, the same on
 * every run).  A negative size: the host form refuses the whole batch with
 * RF_EINVAL and changes nothing, the device form sets RF_EINVAL on that row,
 * which then takes no part.  A removed ID that is Put again is a fresh object
 * of any size.  remove: removed[i] = 1 for the first row of an ID the index
 * held, else 0.  stat: the size, or -1 (NotExist).  The device forms of put and
 * remove return when applied; stat_device is asynchronous on `stream`.
 *
 * collect: every object whose WD(ID) `live` does not contain is removed;
 * *removed their number, *removed_bytes the sum of their sizes (either may be
 * NULL).  live = NULL removes everything, as the reference does with a nil
 * liveset.  A filter borrowed from rf_liveset_filter is accepted.  Returns
 * when done.
 *
 * missing / need_transfer: the work comes in GROUPS of (ID, Size) rows, group
 * g's rows following group g-1's, counts[g] of them (the layout
 * rf_liveset_set_values takes; zero rows is valid).  Per group: Files(), the
 * distinct (ID, Size) pairs (executor.go:82-92, 116-125; no dedup across
 * groups), each then looked up by ID (two rows with one ID and two sizes are
 * two files, and both are missing or neither).  need_transfer: group g is
 * Fileset{List: deps' values} of nodes[g] -- the value rows of its edges in
 * the liveset's CSR, in edge order (an edge listed twice contributes twice; an
 * OpMap's appended MapFlow edge is the caller's concern).  An edge whose node
 * has no value: status[g] = RF_EPRECONDITION and zero counts for that group
 * alone; the device form gives a node >= n status RF_EINVAL likewise (the host
 * form refuses the call).  Both objects of one context (RF_EINVAL).
 * The list: the distinct missing files, by group ascending and within a group
 * by the row of their first occurrence ascending (over the concatenated rows
 * one global ascending order, equal bytes from run to run); miss_ptr[g] = the
 * first list entry of group g.  If any of miss_rows / miss_ids32 / miss_sizes
 * is given the cap rule of rf_eval_plan_list holds: nothing at or beyond cap is
 * written, *n_listed is set either way, and the host form returns RF_EINVAL
 * when the total exceeds cap (the device form's caller compares).
 * At most RF_REPO_MAX_ROWS rows per call: RF_EINVAL beyond, the object left
 * usable.  The calls read the row total back once (need_transfer: and the
 * edge total); the rest is asynchronous on `stream` in the device forms. */
typedef struct rf_repo rf_repo;
#define RF_REPO_MAX_ROWS 1073741824 /* 2^30 rows per call: the dedup table indexes rows with 32 bits */
#define RF_REPO_MIN_SLOTS 1024      /* the smallest table */
#define RF_REPO_LIST_TILE 1024      /* rows per tile of the list's mark / scan / scatter */
typedef struct {
    uint64_t objects;    /* live objects */
    int64_t bytes;       /* the sum of their sizes */
    uint64_t tombstones; /* removed objects that still hold a slot */
    uint64_t capacity;   /* slots */
    uint64_t rebuilds;   /* growths so far */
    uint64_t device_bytes;
    uint64_t last_rows, last_files, last_missing; /* the last missing / need_transfer call: rows, distinct
                                                     files over its groups, those not in the index */
} rf_repo_stats;
typedef struct {            /* every pointer may be NULL; host pointers in the host forms, device in the device forms */
    uint32_t *n_files;      /* [n_groups] distinct (ID, Size) */
    uint32_t *n_missing;    /* [n_groups] of those, ID not in the index */
    int64_t  *missing_bytes;/* [n_groups] sum of their sizes: lookup's message (eval.go:1236-1242), TransferSize (eval.go:429-436) */
    int32_t  *status;       /* [n_groups] need_transfer only */
    uint64_t  cap;          /* capacity of the three list arrays */
    uint64_t *miss_ptr;     /* [n_groups + 1] exclusive scan of n_missing */
    uint64_t *miss_rows;    /* row form only: input row of each missing file's first occurrence */
    uint8_t  *miss_ids32;   /* its ID */
    int64_t  *miss_sizes;   /* its size */
    uint64_t *n_listed;     /* total missing, written whether it fits or not */
} rf_repo_missing_out;
int rf_repo_new(rf_ctx *ctx, uint64_t capacity, rf_repo **out);
void rf_repo_destroy(rf_repo *r);
int rf_repo_put(rf_repo *r, const uint8_t *ids32, const int64_t *sizes, uint64_t n, int32_t *status);
int rf_repo_put_device(rf_repo *r, const void *d_ids32, const void *d_sizes, uint64_t n, void *d_status,
                       void *stream);
int rf_repo_remove(rf_repo *r, const uint8_t *ids32, uint64_t n, uint8_t *removed);
int rf_repo_remove_device(rf_repo *r, const void *d_ids32, uint64_t n, void *d_removed, void *stream);
int rf_repo_stat(rf_repo *r, const uint8_t *ids32, uint64_t n, int64_t *sizes);
int rf_repo_stat_device(rf_repo *r, const void *d_ids32, uint64_t n, void *d_sizes, void *stream);
int rf_repo_collect(rf_repo *r, rf_bloom *live, uint64_t *removed, int64_t *removed_bytes, void *stream);
/* size = sizeof(rf_repo_stats) of the caller's header. */
int rf_repo_stats_get(rf_repo *r, rf_repo_stats *out, uint64_t size);
int rf_repo_missing(rf_repo *r, const uint32_t *counts, uint64_t n_groups, const uint8_t *ids32,
                    const int64_t *sizes, rf_repo_missing_out *o);
int rf_repo_missing_device(rf_repo *r, const void *d_counts, uint64_t n_groups, const void *d_ids32,
                           const void *d_sizes, uint64_t n_rows, rf_repo_missing_out *o, void *stream);
int rf_repo_need_transfer(rf_repo *r, rf_liveset *l, const uint32_t *nodes, uint64_t n_nodes,
                          rf_repo_missing_out *o);
int rf_repo_need_transfer_device(rf_repo *r, rf_liveset *l, const void *d_nodes, uint64_t n_nodes,
                                 rf_repo_missing_out *o, void *stream);

/* ---- Repository index: listing, collect with names, compaction, save / restore
 * What reads the set back out of HBM.  The reference's Collect exists to
 * os.Remove every object the liveset does not contain
 * (repository/file/repository.go:304-327), and a repository outlives the run
 * that filled it (a directory of objects, repository.go:29-47): the index has
 * to name what it dropped and to be carried across processes, as the assoc is
 * (rf_assoc_scan / _compact / _save / _restore above).
 *
 * scan: the live objects, each exactly once, in ascending slot order -- IDs as
 * rows of 32 B and sizes; either array may be NULL.  Tombstones and empty
 * slots are not listed.  An unchanged table gives equal arrays in both forms
 * on every call; nothing is promised across histories (which of two colliding
 * keys of one launch gets the earlier slot is decided by arrival).  The cap
 * rule of rf_assoc_scan and rf_eval_plan_list: no row at index >= cap is
 * written, *n is set either way, and the host form returns RF_EINVAL when
 * *n > cap (the device form's caller compares *d_n with cap).  The device form
 * is asynchronous on `stream`; a later growth, compaction or destroy waits for
 * it before it frees the table it reads. */
int rf_repo_scan(rf_repo *r, uint64_t cap, uint8_t *ids32, int64_t *sizes, uint64_t *n);
int rf_repo_scan_device(rf_repo *r, uint64_t cap, void *d_ids32, void *d_sizes, void *d_n /* u64 */, void *stream);
/* Repository.Collect (repository/file/repository.go:304-327) that says what it
 * removed: rf_repo_collect's rule (live = NULL removes everything; a filter
 * borrowed from rf_liveset_filter is accepted; the filter's length is read on
 * the device), and the removed objects' IDs and sizes in ascending slot order,
 * for the caller's os.Remove (repository.go:316-320).  ALL OR NOTHING: if the
 * dead objects outnumber `cap` while either list array is given, nothing is
 * removed and no counter moves; *removed is still set to the number found
 * (*removed_bytes to 0), the host form returns RF_EINVAL, and the device
 * form's caller compares *d_removed with cap -- the names of objects that left
 * the index are never lost.  With both list arrays NULL, cap is ignored and
 * the call is a plain collect.  Both forms return when applied, as
 * rf_repo_put_device does; the device form's outputs stay on the device, and
 * it takes the all-or-nothing decision on the device from the scanned total
 * (the host form reads the total back once).  rf_repo_stats_get afterwards
 * shows objects, bytes and tombstones moved by exactly what was listed. */
int rf_repo_collect_list(rf_repo *r, rf_bloom *live, uint64_t cap, uint8_t *ids32, int64_t *sizes,
                         uint64_t *removed, int64_t *removed_bytes);
int rf_repo_collect_list_device(rf_repo *r, rf_bloom *live, uint64_t cap, void *d_ids32, void *d_sizes,
                                void *d_removed /* u64 */, void *d_removed_bytes /* i64, may be NULL */,
                                void *stream);
/* Rebuild the table without its tombstones (a GC pass leaves one per removed
 * object, and every later probe walks over them until the next growth):
 * slots = the smallest power of two >= max(RF_REPO_MIN_SLOTS, 2 * max(objects,
 * min_capacity)), rf_repo_new's rule.  Afterwards tombstones == 0 and rebuilds
 * is one higher; every Stat, Put, Remove, missing and need_transfer answers as
 * before the call. */
int rf_repo_compact(rf_repo *r, uint64_t min_capacity);
/* The index across processes: a new process restores the file instead of
 * walking the object directory and Stat-ing every object
 * (repository/file/repository.go:93-101) before its first missing().
 * save writes the live objects to `path` (beside it first, then renamed);
 * restore checks the whole file on the host before a kernel sees a byte --
 * RF_EINVAL for a file that is not one (magic, version, flags, reserved
 * bytes, sizes, truncation) or whose entries break the rules below,
 * RF_EINTEGRITY for a checksum mismatch (errors.Integrity,
 * repository.go:160-162), RF_EIO if it cannot be opened or read; *out is then
 * untouched and the context stays usable -- and bulk-loads a table of
 * rf_repo_new(entries)'s slots: objects and bytes from the file, tombstones,
 * rebuilds and the last_* fields zero.
 * File, little-endian: header 64 B (magic "RFREPO01", u32 version = 1, u32
 * flags = 0, u64 n_entries <= 2^30, u64 chunk > 0, i64 total_bytes = the sum of
 * the sizes, 24 zero bytes); n_entries entries of 40 B (32-B ID, i64 size >=
 * 0), strictly ascending by ID bytes, so equal contents give equal files
 * whatever the table's history; one SHA-256 per `chunk` bytes of the entry
 * area (the last chunk may be short); SHA-256(header || those digests); the
 * end marker "RFREEND1". */
int rf_repo_save(rf_repo *r, const char *path);
int rf_repo_restore(rf_ctx *ctx, const char *path, rf_repo **out);
/* The file form on the host alone (no device), as rf_assoc_file_format /
 * _parse: chunk = checksum granule in bytes (0 = 64 MiB); the entries are
 * given in file order.  *out_len = bytes needed (RF_EINVAL when cap is
 * short); *n = the file's entries (RF_EINVAL with *n set when cap_entries is
 * short).  parse applies every check of rf_repo_restore and never reads past
 * len. */
int rf_repo_file_format(const uint8_t *ids32, const int64_t *sizes, uint64_t n, uint64_t chunk,
                        uint8_t *out, uint64_t cap, uint64_t *out_len);
int rf_repo_file_parse(const uint8_t *buf, uint64_t len, uint8_t *ids32, int64_t *sizes,
                       uint64_t cap_entries, uint64_t *n);

/* ---- The cache write (Eval.CacheWrite, eval.go:1113-1154) --------------------
 * What the plan and the waves later look up, written by one call: after
 * rf_eval_wave_step, the nodes that RAN and whose value is a Fileset
 * (eval.go:1119-1130) are listed with their fsids (SHA-256 of the value's JSON,
 * rf_json_batch_digests_device) and JSON lengths, row i of d_fsids32 (16-byte
 * aligned) / d_sizes belonging to nodes[i].  Accepted hits are not listed: the
 * reference repairs those through rf_assoc_repair.  Every listed node must be
 * DONE in the wave object (RF_EINVAL otherwise, nothing touched); a node listed
 * twice takes part twice, in order.
 *   Node i takes part iff it is flagged RF_PLAN_F_CACHEABLE, is not
 * (no_cache_extern and RF_PLAN_F_EXTERN) (eval.go:1131) and has at least one
 * present key -- keys as they are now, from g's slots through key_slots or from
 * d_keys32, by rf_eval_wave_step's rule: a row of 32 zero bytes is absent
 * (flow.go:798-800); with g, RF_EPRECONDITION while an input change is pending.
 * RF_PLAN_F_INVALID does not matter for a write.
 *   Each participating node contributes Put(zero expect, key, fsid) for each of
 * its present keys (eval.go:1146-1152): one batch, node order then key order,
 * through rf_assoc_put_device's insert path, so "ops on one key apply in index
 * order" decides duplicates the same way on every run.  With repo, each
 * participating node's (fsid, JSON length) is Put into the index first (marshal
 * = Repository.Put, eval.go:1961-1967), first-wins as rf_repo_put_device.
 * Growth of either table is decided on the host before the kernels.  The call
 * holds the context's lock, every object of one context (RF_EINVAL), and
 * returns when applied.
 * Out of scope: Transferer.Transfer (eval.go:1138) is I/O -- the caller runs
 * rf_repo_need_transfer / rf_repo_missing against the destination index first;
 * values that are not Filesets; dep.Err. */
typedef struct {
    uint64_t size;                  /* = sizeof(rf_cache_write_out), set by the caller */
    uint64_t nodes_written;         /* listed nodes that took part */
    uint64_t keys_put;              /* their present keys: the Puts */
    uint64_t skipped_not_cacheable; /* listed nodes skipped, by the first reason that holds */
    uint64_t skipped_extern;
    uint64_t skipped_no_key;
    uint8_t *node_keys;             /* host, [n] or NULL (set by the caller): keys put for nodes[i] */
} rf_cache_write_out;
int rf_eval_wave_cache_write(rf_eval_wave *w, const uint32_t *nodes, uint64_t n, const void *d_fsids32,
                             const void *d_sizes /* int64, JSON lengths */, int no_cache_extern, rf_graph *g,
                             const void *d_keys32, rf_assoc *a, int kind, rf_repo *repo /* may be NULL */,
                             rf_cache_write_out *o /* may be NULL */, void *stream);

/* ---- Physical cache keys (Flow.PhysicalDigest, flow.go:764-792) ----------------
 * The key that moves when a consumer's deps get their values: SHA256(FM(dep 0)
 * ‖ ... ‖ FM(dep k) ‖ suffix), computable once every dep has a value, the zero
 * digest (a row of 32 zero bytes, rf_eval_wave_step's "absent" row) before
 * that.  FM is Fileset.WriteDigest (executor.go:214-233): `path ‖ 00 05 ‖ ID`
 * over the Map entries in bytewise path order, a non-empty List flattened in
 * its place ("List wins").  An rf_physkeys object keeps each finished node's
 * material in an HBM arena, built on the device from the arrays an unmarshal
 * left there, and writes the keys of the affected consumers into the caller's
 * d_keys32 rows, where rf_eval_wave_step, rf_eval_plan_run and
 * rf_eval_wave_cache_write read them.  A bottom-up round is then: step ->
 * unmarshal the hits -> rf_repo_missing_device -> rf_physkeys_set_values_forest
 * -> rf_physkeys_update -> next step, with no per-file or per-node host work.
 *
 * Open: n, dep_ptr, deps as rf_eval_plan_open takes and checks them (a dep
 * listed twice contributes twice).  phys_row[i] = the row of d_keys32 that holds
 * node i's physical key, RF_PHYS_NO_ROW for a node that has none (one that is
 * not OpExec / OpExtern); a row used twice is RF_EINVAL.  suffix[suffix_ptr[i] ..
 * suffix_ptr[i+1]) is what follows the deps' materials: URL.String() for
 * OpExtern, Image ‖ Cmd ‖ LE64 argmap for OpExec, rendered by the host
 * (SURVEY Appendix B.5-6); pointers that are not monotone are RF_EINVAL.
 *
 * Passes, all strided fixed grids or tiles, no atomic on a shared counter, each
 * reading what the one before wrote after the kernel boundary, the results a
 * function of the inputs alone: per forest node a contribution flag and length
 * (a node contributes its Map iff it has no List children, which in closing
 * order is: it is the document's first node or the node before it is not one
 * level deeper) and their scan in tiles of RF_PHYS_LIST_TILE; the emit of the
 * entries into the store's arena, each value at a 16-byte aligned offset, pad
 * bytes zero; for an update the affected set (a byte per node, every writer
 * stores the same 1; listed ascending by tile count / scan / scatter), a
 * computable bit and a material length per affected node, the segment table
 * (per dep the offset and length of its material, then the suffix), the gather
 * into a scratch arena in tiles of RF_PHYS_COPY_TILE output bytes (a tile finds
 * the segment of its first byte by search), K1 over that arena through the
 * one-shot plan of rf_json_batch_digests_device (GPU legs only; the lengths are
 * read back once for its planner), and the scatter of digests and zero rows.
 * The arena's growth is decided on the host before a launch.
 *
 * The store does not compact: a replaced or cleared value leaves its bytes
 * behind as stale bytes (rf_physkeys_stats), as the liveset's rows do.
 * Out of scope: physical jobs inside an rf_graph and keys read through
 * key_slots (d_keys32 rows only); reusing a SHA midstate across consumers that
 * share a leading dep; compaction; dep.Err; graphs that grow at run time;
 * values that are not Filesets. */
#define RF_PHYS_NO_ROW 0xffffffffffffffffull
#define RF_PHYS_SELF 1u       /* rf_physkeys_update: the listed nodes */
#define RF_PHYS_CONSUMERS 2u  /* every consumer of a listed node, each once */
#define RF_PHYS_LIST_TILE 1024 /* forest nodes, graph nodes or affected nodes per tile of a scan */
#define RF_PHYS_COPY_TILE 4096 /* output bytes per workgroup of the gather */
typedef struct rf_physkeys rf_physkeys;
int rf_physkeys_open(rf_ctx *ctx, uint64_t n, const uint64_t *dep_ptr, const uint32_t *deps, const uint64_t *phys_row,
                     const uint64_t *suffix_ptr, const uint8_t *suffix, rf_physkeys **out);
void rf_physkeys_close(rf_physkeys *pk);
/* Document d of a device-form forest becomes the value of nodes[d] (host array,
 * one per document); 0xffffffff skips the document.  RF_EINVAL for a refused
 * document with a real node, a node >= n, a host-form forest.  A node listed
 * twice keeps its last value.  A failed call changes no value.  Returns when
 * the values are set. */
int rf_physkeys_set_values_forest(rf_physkeys *pk, const uint32_t *nodes, const rf_fileset_forest *f, void *stream);
/* Values that did not come from JSON (an exec's output): roots[d] of the tree
 * becomes the value of nodes[d], the File IDs optionally in device rows (K1's
 * output, entry e's at row e), as rf_fileset_marshal_device takes them.  The
 * host walks the tree, orders the Maps that are not in order and uploads paths
 * and the entry order; the same device passes then run.  Refusals are those of
 * rf_fileset_marshal_device, a zero ID excepted: material has no such rule. */
int rf_physkeys_set_values_tree(rf_physkeys *pk, const uint32_t *nodes, const rf_fileset_tree *t,
                                const uint32_t *roots, uint64_t n, const void *d_ids32, void *stream);
/* These nodes are no longer FlowDone. */
int rf_physkeys_clear_values(rf_physkeys *pk, const uint32_t *nodes, uint64_t n);
typedef struct {
    uint64_t size;           /* = sizeof(rf_physkeys_out), set by the caller */
    uint64_t affected;       /* affected nodes that have a phys_row */
    uint64_t keys_written;   /* of them, computable: a digest written */
    uint64_t keys_zeroed;    /* of them, not computable: a zero row written */
    uint64_t material_bytes; /* hashed bytes, unpadded */
    uint64_t cap;            /* room in the two arrays below (set by the caller) */
    uint32_t *nodes;         /* host, [cap] or NULL: the affected nodes, ascending, as far as they fit */
    uint8_t *computable;     /* host, [cap] or NULL: 1 where a digest was written */
} rf_physkeys_out;
/* The affected nodes (flags: RF_PHYS_SELF, RF_PHYS_CONSUMERS or both) that have
 * a phys_row, in ascending node order: if every dep has a value,
 * d_keys32[phys_row] becomes SHA256(the deps' materials in Deps order ‖ suffix),
 * otherwise 32 zero bytes (a dep that is done but has no Fileset value panics in
 * the reference, flow.go:775; here it is "no value").  Rows of other nodes are
 * not touched.  A phys_row >= n_rows is RF_EINVAL with nothing written, and so
 * is a call whose padded materials would reach 4 GiB (split it).  d_keys32 is
 * 16-byte aligned.  Holds the context's lock; returns when the rows are written. */
int rf_physkeys_update(rf_physkeys *pk, const uint32_t *nodes, uint64_t n, uint32_t flags, void *d_keys32,
                       uint64_t n_rows, rf_physkeys_out *o /* may be NULL */, void *stream);
/* d_out32[i] = Fileset.Digest() = SHA256(material) of nodes[i]'s value, straight
 * from the stored material (Fileset.Equal, OpVal's logical digest); a node
 * without a value is RF_EINVAL. */
int rf_physkeys_value_digests_device(rf_physkeys *pk, const uint32_t *nodes, uint64_t n, void *d_out32, void *stream);
/* Host read-back of one value's material, for tests: *len is set either way,
 * RF_EINVAL when cap is short or the node has no value. */
int rf_physkeys_value_material(rf_physkeys *pk, uint32_t node, uint8_t *out, uint64_t cap, uint64_t *len);
typedef struct {
    uint64_t n_nodes, n_values; /* graph nodes; of them, with a value */
    uint64_t arena_bytes;       /* used bytes of the store's arena, pads included */
    uint64_t stale_bytes;       /* of them, belonging to replaced or cleared values */
    uint64_t device_bytes;      /* everything the object holds in HBM */
    double last_ms[6];          /* the last update: affected set / lengths + read-back / segments / gather / K1 / scatter */
} rf_physkeys_stats;
int rf_physkeys_stats_get(rf_physkeys *pk, rf_physkeys_stats *out);
/* Host only, no context, not a product path: the same open arguments, the values
 * (value d belongs to nodes[d]) as the host arrays of rf_fileset_forest_copy or
 * as tree + roots (exactly one of fa and tree), run through the per-entry and
 * per-segment code the kernels run (SHA-256 on the host).  Every node with a
 * phys_row gets its row of keys32 [n_rows][32]: the key, or zero bytes.  Value
 * d's material lands at materials + mat_offs[d] (packed; mat_offs may be NULL),
 * mat_offs[n_values] = *out_len = the bytes needed, set either way; RF_EINVAL
 * with nothing written when cap is short. */
typedef struct {
    uint64_t n_docs;
    const uint64_t *doc_node_ptr; /* [n_docs + 1] */
    const uint32_t *node_depth;
    const uint64_t *entry_ptr;
    const uint64_t *path_off;
    const uint8_t *paths;
    const uint8_t *ids32;
} rf_forest_arrays;
int rf_physkeys_flat(uint64_t n, const uint64_t *dep_ptr, const uint32_t *deps, const uint64_t *phys_row,
                     const uint64_t *suffix_ptr, const uint8_t *suffix, const uint32_t *nodes, uint64_t n_values,
                     const rf_forest_arrays *fa, const rf_fileset_tree *tree, const uint32_t *roots, uint8_t *keys32,
                     uint64_t n_rows, uint8_t *materials, uint64_t cap, uint64_t *mat_offs, uint64_t *out_len);

#ifdef __cplusplus
}
#endif
#endif /* REFLOW_HIP_H */
