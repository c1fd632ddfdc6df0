"""ctypes binding of include/reflow_hip.h (libreflow_hip.so).

This is plumbing for the Python test-suite and bench.py: every call goes
through the C-ABI into the gfx950 kernels.  There is no CPU fallback: if the
library or a gfx950 device is missing, the calls raise.
"""
from __future__ import annotations

import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libreflow_hip.so")

RF_OK, RF_EINVAL, RF_EIO, RF_EINTEGRITY, RF_EDEVICE, RF_ENOMEM, RF_ENOTFOUND, RF_EPRECONDITION = range(8)
RF_ENOTCANONICAL = 8  # per-document status of the Fileset unmarshal
RF_SHA_NO_SOLO = 1
RF_SHA_ALL_SOLO = 2
RF_SHA_ONE_LANE_CHAIN = 4
RF_SHA_NO_PAIR = 8
RF_SHA_NO_OCTO = 16
RF_SHA_ALL_HOST = 32
RF_SHA_NO_HOST = 64
RF_SHA_NO_PREFIX = 128
RF_PREFIX_RACE, RF_PREFIX_WAIT, RF_PREFIX_MISS = 0, 1, 2
# change feed (rf_graph_feed_*): poll flag, poll modes, slots per compaction tile
RF_FEED_FORCE_SCAN = 1
RF_FEED_NONE, RF_FEED_LISTED, RF_FEED_SCAN = 0, 1, 2
FEED_TILE_SLOTS = 8192
# evaluation plan (rf_eval_plan_*): node flags, node states, keys per node
RF_PLAN_F_CACHEABLE, RF_PLAN_F_EXTERN, RF_PLAN_F_INVALID, RF_PLAN_F_DONE = 1, 2, 4, 8
RF_PLAN_UNSEEN, RF_PLAN_TODO, RF_PLAN_READY, RF_PLAN_HIT, RF_PLAN_DONE = range(5)
RF_PLAN_MAX_KEYS = 8
# evaluation waves (rf_eval_wave_*): list scopes, modes
RF_WAVE_ALL, RF_WAVE_LAST = 0, 1
RF_WAVE_MODE_NONE, RF_WAVE_MODE_BOTTOMUP, RF_WAVE_MODE_TOPDOWN = 0, 1, 2
# GC liveset (rf_liveset_*): node states, rows per run, nodes per list tile, rounds per host read
RF_LIVE_UNSEEN, RF_LIVE_WALKED, RF_LIVE_VALUE = range(3)
RF_LIVE_MAX_ROWS = 1 << 30
RF_LIVE_LIST_TILE = 1024
RF_LIVE_ROUND_BATCH = 4
# repository index (rf_repo_*): rows per call, the smallest table, rows per list tile
RF_REPO_MAX_ROWS = 1 << 30
RF_REPO_MIN_SLOTS = 1024
RF_REPO_LIST_TILE = 1024
# device marshal of Fileset values (rf_fileset_marshal_device): pieces per tile
RF_MARSHAL_TILE = 1024
# device unmarshal of Fileset values (rf_fileset_unmarshal_device): arena bytes per tile, reason bits, flat-form flag
RF_UNMARSHAL_TILE = 4096
(RF_UNMARSHAL_WHY_STRUCTURE, RF_UNMARSHAL_WHY_STRING, RF_UNMARSHAL_WHY_ID, RF_UNMARSHAL_WHY_SIZE,
 RF_UNMARSHAL_WHY_ORDER, RF_UNMARSHAL_WHY_DEPTH, RF_UNMARSHAL_WHY_LENGTH) = 1, 2, 4, 8, 16, 32, 64
RF_UNMARSHAL_CHECK_TILED = 1
# physical keys (rf_physkeys_*): a node without a key row, update flags, items per scan tile, bytes per gather tile
RF_PHYS_NO_ROW = 2**64 - 1
RF_PHYS_SELF, RF_PHYS_CONSUMERS = 1, 2
RF_PHYS_LIST_TILE = 1024
RF_PHYS_COPY_TILE = 4096
RF_PHYS_SKIP = 0xffffffff  # set values: a document without a node

# Every symbol include/reflow_hip.h declares (checked by tests/test_capi_symbols.py).
EXPORTS = [
    "rf_init", "rf_destroy", "rf_last_error", "rf_device_count", "rf_device_cus", "rf_sync", "rf_version",
    "rf_sha256_batch", "rf_sha256_arena", "rf_sha_plan_create", "rf_sha_plan_run",
    "rf_sha_plan_stats", "rf_sha_plan_destroy", "rf_sha_plan_prefix_stats", "rf_sha_plan_set_prefixes", "rf_gen_fill", "rf_fileset_digest_batch",
    "rf_fileset_digest_device", "rf_install_dir", "rf_install_info", "rf_install_entries",
    "rf_install_destroy",
    "rf_graph_load", "rf_graph_destroy", "rf_graph_set_slots", "rf_graph_set_slots_device",
    "rf_graph_save", "rf_graph_restore", "rf_graph_set_forms",
    "rf_graph_adopt_slots",
    "rf_graph_recompute", "rf_graph_recompute_async", "rf_graph_get_slots", "rf_graph_stats_get",
    "rf_bloom_load", "rf_bloom_load_json", "rf_bloom_load_binary", "rf_bloom_new",
    "rf_bloom_destroy", "rf_bloom_probe", "rf_bloom_probe_device", "rf_bloom_add",
    "rf_bloom_add_device", "rf_bloom_params", "rf_bloom_words",
    "rf_malloc", "rf_free", "rf_memcpy_h2d", "rf_memcpy_d2h", "rf_memset_d", "rf_stream",
    "rf_timer_start", "rf_timer_stop", "rf_comm_unique_id", "rf_comm_init", "rf_comm_destroy",
    "rf_comm_allgather", "rf_comm_allreduce_or", "rf_memcpy_d2d", "rf_graph_gather_device",
    "rf_fileset_marshal_json", "rf_fileset_value_digest_batch",
    "rf_bloom_marshal_json", "rf_bloom_marshal_binary", "rf_bloom_parse_binary", "rf_bloom_parse_json",
    "rf_bloom_format_binary", "rf_bloom_format_json", "rf_bloom_collect", "rf_bloom_collect_device",
    "rf_dedup_digests", "rf_dedup_digests_device", "rf_assoc_lookup",
    "rf_assoc_new", "rf_assoc_destroy", "rf_assoc_put", "rf_assoc_get", "rf_assoc_get_device",
    "rf_assoc_get_abbrev", "rf_assoc_stats", "rf_assoc_put_device",
    "rf_assoc_count", "rf_assoc_scan", "rf_assoc_scan_device", "rf_assoc_compact", "rf_assoc_save",
    "rf_assoc_restore", "rf_assoc_file_format", "rf_assoc_file_parse",
    "rf_set_host_threads", "rf_host_info", "rf_host_rate", "rf_host_link", "rf_assoc_repair",
    "rf_sha_streams_open", "rf_sha_streams_close", "rf_sha_streams_write", "rf_sha_streams_digest",
    "rf_sha_streams_len", "rf_sha_streams_verify", "rf_sha256_verify", "rf_flow_dirty",
    "rf_coalescer_open", "rf_coalescer_close", "rf_coalesce_sha256", "rf_coalesce_probe", "rf_coalesce_assoc_get",
    "rf_coalesce_sha256_async", "rf_coalesce_poll", "rf_coalesce_wait", "rf_coalesce_ticket_free",
    "rf_coalescer_stats", "rf_graph_update_recompute_async", "rf_walk_dir", "rf_walk_info", "rf_walk_entries", "rf_walk_free",
    "rf_graph_set_part", "rf_graph_recompute_part", "rf_graph_part_gathered", "rf_graph_split",
    "rf_graph_piece_free", "rf_graph_piece_desc", "rf_graph_piece_part", "rf_graph_piece_slots",
    "rf_graph_feed_open", "rf_graph_feed_close", "rf_graph_feed_poll", "rf_graph_feed_poll_device",
    "rf_graph_feed_lookup_device", "rf_graph_feed_stats_get",
    "rf_eval_plan_open", "rf_eval_plan_check", "rf_eval_plan_close", "rf_eval_plan_set_flags",
    "rf_eval_plan_run", "rf_eval_plan_run_host", "rf_eval_plan_reject", "rf_eval_plan_reject_host",
    "rf_eval_plan_states", "rf_eval_plan_states_device", "rf_eval_plan_list", "rf_eval_plan_list_device",
    "rf_eval_plan_stats_get",
    "rf_eval_wave_consumers", "rf_eval_wave_open", "rf_eval_wave_close", "rf_eval_wave_set_flags",
    "rf_eval_wave_begin", "rf_eval_wave_begin_host", "rf_eval_wave_begin_states", "rf_eval_wave_step",
    "rf_eval_wave_step_host", "rf_eval_wave_reject", "rf_eval_wave_states", "rf_eval_wave_states_device",
    "rf_eval_wave_list", "rf_eval_wave_list_device", "rf_eval_wave_stats_get",
    "rf_bloom_estimate", "rf_liveset_open", "rf_liveset_close", "rf_liveset_set_values",
    "rf_liveset_set_values_device", "rf_liveset_clear_values", "rf_liveset_run", "rf_liveset_filter",
    "rf_liveset_states", "rf_liveset_list", "rf_liveset_stats_get",
    "rf_repo_new", "rf_repo_destroy", "rf_repo_put", "rf_repo_put_device", "rf_repo_remove",
    "rf_repo_remove_device", "rf_repo_stat", "rf_repo_stat_device", "rf_repo_collect", "rf_repo_stats_get",
    "rf_repo_missing", "rf_repo_missing_device", "rf_repo_need_transfer", "rf_repo_need_transfer_device",
    "rf_repo_scan", "rf_repo_scan_device", "rf_repo_collect_list", "rf_repo_collect_list_device",
    "rf_repo_compact", "rf_repo_save", "rf_repo_restore", "rf_repo_file_format", "rf_repo_file_parse",
    "rf_fileset_marshal_flat", "rf_fileset_marshal_device", "rf_json_batch_info", "rf_json_batch_times", "rf_json_batch_lens",
    "rf_json_batch_device", "rf_json_batch_copy", "rf_json_batch_digests_device", "rf_json_batch_free",
    "rf_fileset_value_digest_device", "rf_eval_wave_cache_write",
    "rf_fileset_unmarshal_flat", "rf_fileset_unmarshal_device", "rf_fileset_unmarshal", "rf_fileset_forest_info",
    "rf_fileset_forest_status", "rf_fileset_forest_rows_device", "rf_fileset_forest_copy", "rf_fileset_forest_tree",
    "rf_fileset_forest_times", "rf_fileset_forest_free",
    "rf_physkeys_open", "rf_physkeys_close", "rf_physkeys_set_values_forest", "rf_physkeys_set_values_tree",
    "rf_physkeys_clear_values", "rf_physkeys_update", "rf_physkeys_value_digests_device",
    "rf_physkeys_value_material", "rf_physkeys_stats_get", "rf_physkeys_flat",
]


class RfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rf error %d: %s" % (code, msg))
        self.code = code


class ShaPrefixStats(ctypes.Structure):
    """rf_sha_prefix_stats: the plan's prefix hand-overs and what the last run's host leg made of them."""
    _fields_ = [("n_prefixed", ctypes.c_uint64), ("planned_bytes", ctypes.c_uint64), ("taken", ctypes.c_uint64),
                ("missed", ctypes.c_uint64), ("skipped_bytes", ctypes.c_uint64), ("n_lone", ctypes.c_uint64)]


class ShaStats(ctypes.Structure):
    _fields_ = [("n_msgs", ctypes.c_uint64), ("n_solo", ctypes.c_uint64),
                ("total_blocks", ctypes.c_uint64), ("max_blocks", ctypes.c_uint64),
                ("total_bytes", ctypes.c_uint64), ("last_ms_lanes", ctypes.c_float),
                ("last_ms_solo", ctypes.c_float), ("last_ms_total", ctypes.c_float),
                ("last_ms_host", ctypes.c_float), ("host_threads", ctypes.c_uint32),
                ("n_host", ctypes.c_uint64), ("host_bytes", ctypes.c_uint64)]


class GraphDesc(ctypes.Structure):
    _fields_ = [("n_jobs", ctypes.c_uint32), ("n_slots", ctypes.c_uint32),
                ("out_slot", ctypes.c_void_p), ("tmpl_off", ctypes.c_void_p),
                ("tmpl_len", ctypes.c_void_p), ("hole_ptr", ctypes.c_void_p),
                ("hole_pos", ctypes.c_void_p), ("hole_slot", ctypes.c_void_p),
                ("blob", ctypes.c_void_p), ("blob_len", ctypes.c_uint64)]


class FilesetTree(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("list_ptr", ctypes.c_void_p),
                ("list_child", ctypes.c_void_p), ("entry_ptr", ctypes.c_void_p),
                ("paths", ctypes.c_void_p), ("path_lens", ctypes.c_void_p),
                ("ids32", ctypes.c_void_p), ("sizes", ctypes.c_void_p)]


class FilesetTreeBuilder:
    """Flattens nested filesets into the rf_fileset_tree CSR form.  A fileset
    is any object with .list (None or a list of filesets) and .map (None or a
    dict path -> (id32, size)); add() returns its root node index."""

    def __init__(self):
        self.list_ptr, self.list_child, self.entry_ptr = [0], [], [0]
        self.paths, self.ids, self.sizes = [], [], []
        self._pending = []

    def add(self, fs) -> int:
        # nodes are numbered in pre-order; children lists refer forward
        node = len(self.list_ptr) - 1
        self.list_ptr.append(None)
        self.entry_ptr.append(None)
        for path, (id32, size) in (fs.map or {}).items():
            self.paths.append(path.encode("utf-8", "surrogateescape") if isinstance(path, str) else path)
            self.ids.append(bytes(id32))
            self.sizes.append(int(size))
        self.entry_ptr[node + 1] = len(self.paths)
        kids = [self.add(c) for c in (fs.list or [])]
        self._pending.append((node, kids))
        return node

    def struct(self):
        n = len(self.list_ptr) - 1
        children = dict(self._pending)
        lp, lc = [0], []
        for i in range(n):
            lc.extend(children[i])
            lp.append(len(lc))
        # a node's entries are recorded before its children's (pre-order), so
        # entry_ptr is already the CSR; list_ptr is rebuilt from the children
        self._keep = dict(
            lp=np.array(lp, dtype=np.uint64), lc=np.array(lc or [0], dtype=np.uint32),
            ep=np.array(self.entry_ptr, dtype=np.uint64),
            pb=[ctypes.create_string_buffer(p, max(len(p), 1)) for p in self.paths],
            pl=np.array([len(p) for p in self.paths] or [0], dtype=np.uint32),
            ids=np.frombuffer(b"".join(self.ids) or b"\0" * 32, dtype=np.uint8).copy(),
            sz=np.array(self.sizes or [0], dtype=np.int64))
        k = self._keep
        k["pp"] = (ctypes.c_void_p * max(len(self.paths), 1))(*[ctypes.addressof(b) for b in k["pb"]])
        return FilesetTree(n, _ptr(k["lp"]), _ptr(k["lc"]), _ptr(k["ep"]),
                           ctypes.cast(k["pp"], ctypes.c_void_p), _ptr(k["pl"]), _ptr(k["ids"]),
                           _ptr(k["sz"]))


def fileset_marshal_json(fs) -> bytes:
    """json.Marshal(Fileset) through the C-ABI (host code, no device)."""
    b = FilesetTreeBuilder()
    root = b.add(fs)
    t = b.struct()
    need = ctypes.c_uint64(0)
    rc = lib().rf_fileset_marshal_json(ctypes.byref(t), root, None, 0, ctypes.byref(need))
    if rc != RF_OK and need.value == 0:
        _check(rc)
    out = ctypes.create_string_buffer(max(need.value, 1))
    _check(lib().rf_fileset_marshal_json(ctypes.byref(t), root, out, need.value, ctypes.byref(need)))
    return out.raw[:need.value]


def fileset_marshal_flat(sets):
    """json.Marshal of each fileset through the piece stream and the per-piece
    code the marshal kernels run (host code, no device): a list of bytes."""
    b = FilesetTreeBuilder()
    roots = np.array([b.add(fs) for fs in sets], dtype=np.uint32)
    t = b.struct()
    n = len(sets)
    offs = np.zeros(n + 1, dtype=np.uint64)
    need = ctypes.c_uint64(0)
    rc = lib().rf_fileset_marshal_flat(ctypes.byref(t), _ptr(roots) if n else None, n, None, 0, _ptr(offs),
                                       ctypes.byref(need))
    if rc != RF_OK and need.value == 0:
        _check(rc)
    out = np.zeros(max(need.value, 1), dtype=np.uint8)
    _check(lib().rf_fileset_marshal_flat(ctypes.byref(t), _ptr(roots) if n else None, n, _ptr(out), need.value,
                                         _ptr(offs), ctypes.byref(need)))
    assert int(offs[n]) == need.value
    return [out[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]


class Fileset:
    """A decoded Fileset value: .list (None or a list of Fileset) and .map (None
    or a dict path bytes -> (id32, size), in key order) -- the shape
    FilesetTreeBuilder and the oracle's OFileset have; omitempty's absent List
    and Map are None."""

    def __init__(self, map=None, list=None):
        self.map, self.list = map, list

    def flat(self):
        """[(depth, ((path, id32, size), ...))] per node in closing order (post-order),
        which determines the value; no recursion, so any depth compares."""
        out, stack = [], [(self, 0, False)]
        while stack:
            v, d, seen = stack.pop()
            if seen:
                out.append((d, tuple((k, e[0], e[1]) for k, e in (v.map or {}).items())))
                continue
            stack.append((v, d, True))
            stack.extend((c, d + 1, False) for c in reversed(v.list or ()))
        return out

    def __eq__(self, other):
        return isinstance(other, Fileset) and self.flat() == other.flat()

    def __repr__(self):
        return "Fileset(map=%r, list=%r)" % (self.map, self.list)


def pack_docs(docs):
    """(uint8 array, uint64 offsets [n + 1]) of documents packed back to back."""
    offs = np.zeros(len(docs) + 1, dtype=np.uint64)
    if docs:
        offs[1:] = np.cumsum([len(d) for d in docs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(docs) or b"\0", dtype=np.uint8).copy()
    return buf, offs


class FilesetForest:
    """rf_fileset_forest: a batch of Fileset JSON documents unmarshalled, by the
    host form (flat) or on the device."""

    def __init__(self, handle, ctx=None):
        self._h, self.ctx = handle, ctx
        v = [ctypes.c_uint64() for _ in range(5)]
        _check(lib().rf_fileset_forest_info(self._h, *[ctypes.byref(x) for x in v]))
        self.n_docs, self.n_accepted, self.n_nodes, self.n_entries, self.path_bytes = [x.value for x in v]

    @classmethod
    def flat(cls, docs, flags=RF_UNMARSHAL_CHECK_TILED, threads=0):
        buf, offs = pack_docs(docs)
        h = ctypes.c_void_p()
        _check(lib().rf_fileset_unmarshal_flat(_ptr(buf), _ptr(offs), len(docs), flags, threads, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def from_host(cls, ctx, docs, stream=None):
        buf, offs = pack_docs(docs)
        h = ctypes.c_void_p()
        _check(lib().rf_fileset_unmarshal(ctx.handle, _ptr(buf), _ptr(offs), len(docs), ctypes.byref(h), stream))
        return cls(h, ctx)

    @classmethod
    def from_device(cls, ctx, d_arena, arena_bytes, d_offs, d_lens, n, stream=None):
        h = ctypes.c_void_p()
        _check(lib().rf_fileset_unmarshal_device(ctx.handle, d_arena, arena_bytes, d_offs, d_lens, n, ctypes.byref(h),
                                                 stream))
        return cls(h, ctx)

    def status(self):
        """(status i32, reason u32, node counts u32, entry counts u32), one per document."""
        n = self.n_docs
        a = [np.zeros(max(n, 1), dtype=t) for t in (np.int32, np.uint32, np.uint32, np.uint32)]
        _check(lib().rf_fileset_forest_status(self._h, *[_ptr(x) for x in a]))
        return tuple(x[:n] for x in a)

    def rows_device(self):
        """(d_counts, d_ids32, d_sizes, n_rows): rf_repo_missing_device's arguments."""
        c, i, s, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        _check(lib().rf_fileset_forest_rows_device(self._h, ctypes.byref(c), ctypes.byref(i), ctypes.byref(s),
                                                   ctypes.byref(n)))
        return c.value, i.value, s.value, n.value

    def copy(self):
        """The structure on the host: a dict of doc_node_ptr, node_depth, entry_ptr,
        path_off, paths, ids32, sizes (numpy arrays)."""
        o = dict(doc_node_ptr=np.zeros(self.n_docs + 1, np.uint64), node_depth=np.zeros(max(self.n_nodes, 1), np.uint32),
                 entry_ptr=np.zeros(self.n_nodes + 1, np.uint64), path_off=np.zeros(self.n_entries + 1, np.uint64),
                 paths=np.zeros(max(self.path_bytes, 1), np.uint8), ids32=np.zeros(max(32 * self.n_entries, 1), np.uint8),
                 sizes=np.zeros(max(self.n_entries, 1), np.int64))
        _check(lib().rf_fileset_forest_copy(self._h, *[_ptr(o[k]) for k in (
            "doc_node_ptr", "node_depth", "entry_ptr", "path_off", "paths", "ids32", "sizes")]))
        o["node_depth"] = o["node_depth"][:self.n_nodes]
        o["paths"] = o["paths"][:self.path_bytes]
        o["ids32"] = o["ids32"][:32 * self.n_entries]
        o["sizes"] = o["sizes"][:self.n_entries]
        return o

    def times(self):
        ms = (ctypes.c_double * 3)()
        _check(lib().rf_fileset_forest_times(self._h, ms))
        return tuple(ms)

    def values(self, structure=None):
        """One Fileset per document, None for a refused one (through
        rf_fileset_forest_tree)."""
        o = structure or self.copy()
        nn, nd = self.n_nodes, self.n_docs
        lp, lc = np.zeros(nn + 1, np.uint64), np.zeros(max(nn, 1), np.uint32)
        roots = np.zeros(max(nd, 1), np.uint32)
        _check(lib().rf_fileset_forest_tree(_ptr(o["doc_node_ptr"]), nd, _ptr(o["node_depth"]) if nn else None, nn,
                                            _ptr(lp), _ptr(lc), _ptr(roots)))
        paths, po, ids, sizes, ep = o["paths"].tobytes(), o["path_off"], o["ids32"].tobytes(), o["sizes"], o["entry_ptr"]
        made = [None] * nn
        for p in range(nn):  # closing order: a node's List is made before it
            kids = [made[c] for c in lc[int(lp[p]):int(lp[p + 1])]]
            m = {paths[int(po[e]):int(po[e + 1])]: (ids[32 * e:32 * e + 32], int(sizes[e]))
                 for e in range(int(ep[p]), int(ep[p + 1]))}
            made[p] = Fileset(map=m or None, list=kids or None)
        return [None if roots[d] == 0xffffffff else made[int(roots[d])] for d in range(nd)]

    def close(self):
        if self._h:
            lib().rf_fileset_forest_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fileset_unmarshal_flat(docs, flags=RF_UNMARSHAL_CHECK_TILED):
    """Each document through the host form (and, by default, the kernels'
    per-byte form beside it): a list of Fileset, None where refused."""
    f = FilesetForest.flat(docs, flags)
    try:
        return f.values()
    finally:
        f.close()


def fileset_unmarshal(ctx, docs=None, device=None):
    """The device form over host documents, or over device=(d_arena, arena_bytes,
    d_offs, d_lens, n): a list of Fileset, None where refused."""
    f = FilesetForest.from_host(ctx, docs) if device is None else FilesetForest.from_device(ctx, *device)
    try:
        return f.values()
    finally:
        f.close()


class JsonBatch:
    """rf_json_batch: Fileset values marshalled to JSON in device memory."""

    def __init__(self, ctx, sets=None, tree=None, roots=None, d_ids32=None, stream=None):
        """sets: fileset objects (FilesetTreeBuilder.add), or tree + roots: an
        rf_fileset_tree struct and its root nodes.  d_ids32: the File IDs as
        device rows, entry e's at row e; the tree's own IDs are then not read."""
        self.ctx = ctx
        if sets is not None:
            b = FilesetTreeBuilder()
            roots = [b.add(fs) for fs in sets]
            tree = b.struct()
            self._keep = b
        r = np.ascontiguousarray(roots, dtype=np.uint32)
        self._h = ctypes.c_void_p()
        _check(lib().rf_fileset_marshal_device(ctx.handle, ctypes.byref(tree), _ptr(r) if len(r) else None, len(r),
                                               d_ids32, ctypes.byref(self._h), stream))
        n, total, pieces = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().rf_json_batch_info(self._h, ctypes.byref(n), ctypes.byref(total), ctypes.byref(pieces)))
        self.n, self.total_bytes, self.n_pieces = n.value, total.value, pieces.value

    def times(self):
        """(flatten + sort, upload + length + scan + read-back, arena + emit) of the marshal call, ms."""
        ms = (ctypes.c_double * 3)()
        _check(lib().rf_json_batch_times(self._h, ms))
        return tuple(ms)

    def lens(self) -> np.ndarray:
        out = np.zeros(max(self.n, 1), dtype=np.int64)
        _check(lib().rf_json_batch_lens(self._h, _ptr(out)))
        return out[:self.n]

    def device(self):
        """(arena, offs, lens) device pointers."""
        a, o, l = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        _check(lib().rf_json_batch_device(self._h, ctypes.byref(a), ctypes.byref(o), ctypes.byref(l)))
        return a.value, o.value, l.value

    def copy(self, which=None):
        """The chosen values' bytes (default: all), a list of bytes."""
        w = None if which is None else np.ascontiguousarray(which, dtype=np.uint64)
        n = self.n if w is None else len(w)
        offs = np.zeros(n + 1, dtype=np.uint64)
        rc = lib().rf_json_batch_copy(self._h, _ptr(w) if w is not None and n else None, n, None, 0, _ptr(offs))
        if rc != RF_OK and int(offs[n]) == 0:
            _check(rc)
        out = np.zeros(max(int(offs[n]), 1), dtype=np.uint8)
        _check(lib().rf_json_batch_copy(self._h, _ptr(w) if w is not None and n else None, n, _ptr(out), int(offs[n]),
                                        _ptr(offs)))
        return [out[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]

    def digests_device(self, d_out32, stream=None):
        _check(lib().rf_json_batch_digests_device(self._h, d_out32, stream))

    def digests(self) -> list:
        """The fsids on the host (a device buffer and a download; for tests)."""
        if not self.n:
            return []
        d = self.ctx.alloc(32 * self.n)
        self.digests_device(d.ptr)
        out = d.to_numpy(np.uint8, 32 * self.n)
        d.free()
        return [out[32 * i:32 * i + 32].tobytes() for i in range(self.n)]

    def close(self):
        if self._h:
            lib().rf_json_batch_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GraphPart(ctypes.Structure):
    _fields_ = [("nranks", ctypes.c_int), ("rank", ctypes.c_int), ("max_export", ctypes.c_uint32),
                ("n_export", ctypes.c_uint32), ("export_slot", ctypes.c_void_p),
                ("n_import", ctypes.c_uint32), ("import_slot", ctypes.c_void_p),
                ("import_bid", ctypes.c_void_p), ("any_import", ctypes.c_int), ("rounds", ctypes.c_uint32)]


# int (*)(void *user, const void *send, void *recv, uint64_t bytes)
HOST_ALLGATHER = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)


def host_allgather_fn(allgather, nranks):
    """Wraps allgather(bytes) -> [bytes per rank] (e.g. torch.distributed
    gloo) as the library's host all-gather callback."""
    def fn(user, send, recv, nbytes):
        try:
            parts = allgather(ctypes.string_at(send, nbytes))
            assert len(parts) == nranks and all(len(p) == nbytes for p in parts)
            ctypes.memmove(recv, b"".join(parts), nranks * nbytes)
            return 0
        except Exception:  # noqa: BLE001 -- reported to the library as a failure
            import traceback
            traceback.print_exc()
            return 1
    return HOST_ALLGATHER(fn)


def _arr(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    c = {np.uint32: ctypes.c_uint32, np.uint64: ctypes.c_uint64}[dtype]
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(c)), shape=(n,)).copy()


class GraphPiece:
    """rf_graph_split (host only): rank `rank`'s piece of a global job graph
    given as rf_graph_desc arrays (a dict like Dag1000.arrays()); owner[j] =
    the rank hashing job j, -1 = every rank.  Attributes: desc (the piece's
    arrays, templates in the global blob), part (exports / imports / boundary
    ids), global_of_local."""

    def __init__(self, arrays, nranks, rank, owner):
        k = {n: np.ascontiguousarray(arrays[n], dtype=dt) for n, dt in
             (("out_slot", np.uint32), ("tmpl_off", np.uint64), ("tmpl_len", np.uint32),
              ("hole_ptr", np.uint64), ("hole_pos", np.uint32), ("hole_slot", np.uint32))}
        blob = arrays["blob"]
        self.blob = np.frombuffer(bytes(blob), np.uint8) if isinstance(blob, (bytes, bytearray)) \
            else np.ascontiguousarray(blob, dtype=np.uint8)
        own = np.ascontiguousarray(owner, dtype=np.int32)
        d = GraphDesc(len(k["out_slot"]), int(arrays["n_slots"]), _ptr(k["out_slot"]), _ptr(k["tmpl_off"]),
                      _ptr(k["tmpl_len"]), _ptr(k["hole_ptr"]), _ptr(k["hole_pos"]) if len(k["hole_pos"]) else None,
                      _ptr(k["hole_slot"]) if len(k["hole_slot"]) else None, _ptr(self.blob), len(self.blob))
        h = ctypes.c_void_p()
        _check(lib().rf_graph_split(ctypes.byref(d), nranks, rank, _ptr(own), ctypes.byref(h)))
        try:
            ld = GraphDesc()
            _check(lib().rf_graph_piece_desc(h, ctypes.byref(ld)))
            J = ld.n_jobs
            hp = _arr(ld.hole_ptr, J + 1, np.uint64)
            H = int(hp[-1]) if J else 0
            self.desc = dict(n_slots=ld.n_slots, out_slot=_arr(ld.out_slot, J, np.uint32),
                             tmpl_off=_arr(ld.tmpl_off, J, np.uint64), tmpl_len=_arr(ld.tmpl_len, J, np.uint32),
                             hole_ptr=hp, hole_pos=_arr(ld.hole_pos, H, np.uint32),
                             hole_slot=_arr(ld.hole_slot, H, np.uint32), blob=self.blob)
            pt = GraphPart()
            _check(lib().rf_graph_piece_part(h, ctypes.byref(pt)))
            self.part = dict(nranks=pt.nranks, rank=pt.rank, max_export=pt.max_export,
                             export_slot=_arr(pt.export_slot, pt.n_export, np.uint32),
                             import_slot=_arr(pt.import_slot, pt.n_import, np.uint32),
                             import_bid=_arr(pt.import_bid, pt.n_import, np.uint32), any_import=bool(pt.any_import),
                             rounds=int(pt.rounds))
            gp, gn = ctypes.c_void_p(), ctypes.c_uint32()
            _check(lib().rf_graph_piece_slots(h, ctypes.byref(gp), ctypes.byref(gn)))
            self.global_of_local = _arr(gp, gn.value, np.uint32)
        finally:
            lib().rf_graph_piece_free(h)


class GraphStats(ctypes.Structure):
    _fields_ = [("n_jobs", ctypes.c_uint32), ("n_slots", ctypes.c_uint32),
                ("n_levels", ctypes.c_uint32), ("max_level_jobs", ctypes.c_uint32),
                ("total_blocks", ctypes.c_uint64), ("hole_count", ctypes.c_uint64),
                ("template_bytes", ctypes.c_uint64), ("last_recomputed", ctypes.c_uint64),
                ("last_ms", ctypes.c_float), ("last_levels_lf", ctypes.c_uint32),
                ("last_mark_lf", ctypes.c_uint32), ("last_levels_oct", ctypes.c_uint32),
                ("split_block0", ctypes.c_uint32),
                ("last_sink_attach", ctypes.c_uint32), ("last_levels_half", ctypes.c_uint32)]


class GraphFeedStats(ctypes.Structure):
    _fields_ = [("polls", ctypes.c_uint64), ("polls_listed", ctypes.c_uint64), ("polls_scan", ctypes.c_uint64),
                ("last_mode", ctypes.c_uint32), ("tracked_slots", ctypes.c_uint64),
                ("device_bytes", ctypes.c_uint64)]


class EvalPlanStats(ctypes.Structure):
    """rf_eval_plan_stats: counts[state] and the lookup figures are those of the last run / reject."""
    _fields_ = [("n_nodes", ctypes.c_uint64), ("depth", ctypes.c_uint32), ("rounds", ctypes.c_uint32),
                ("round_batch", ctypes.c_uint32), ("round_lanes", ctypes.c_uint32),
                ("list_tile", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("counts", ctypes.c_uint64 * 5), ("looked_up", ctypes.c_uint64),
                ("keys_probed", ctypes.c_uint64), ("keys_filtered", ctypes.c_uint64),
                ("device_bytes", ctypes.c_uint64)]


class EvalWaveStats(ctypes.Structure):
    """rf_eval_wave_stats: counts[state] as of now; the lookup figures are those of the last begin / step."""
    _fields_ = [("n_nodes", ctypes.c_uint64), ("n_deps", ctypes.c_uint64), ("depth", ctypes.c_uint32),
                ("mode", ctypes.c_uint32), ("waves", ctypes.c_uint32), ("last_wave", ctypes.c_uint32),
                ("rounds", ctypes.c_uint32), ("round_batch", ctypes.c_uint32),
                ("wave_lanes", ctypes.c_uint32), ("list_tile", ctypes.c_uint32),
                ("counts", ctypes.c_uint64 * 5), ("looked_up", ctypes.c_uint64),
                ("keys_probed", ctypes.c_uint64), ("keys_filtered", ctypes.c_uint64),
                ("device_bytes", ctypes.c_uint64)]


class LivesetStats(ctypes.Structure):
    """rf_liveset_stats: the figures of the last run (arena_rows / stale_rows: as of now)."""
    _fields_ = [("n_nodes", ctypes.c_uint64), ("counts", ctypes.c_uint64 * 3), ("contributions", ctypes.c_uint64),
                ("nlive_est", ctypes.c_uint64), ("nlive", ctypes.c_uint64), ("livebytes", ctypes.c_int64),
                ("maxlivebytes", ctypes.c_int64), ("m", ctypes.c_uint64), ("k", ctypes.c_uint64),
                ("rounds", ctypes.c_uint32), ("changed", ctypes.c_uint32), ("arena_rows", ctypes.c_uint64),
                ("stale_rows", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64)]


class RepoStats(ctypes.Structure):
    """rf_repo_stats: the index as of now, and the last missing / need_transfer call's totals."""
    _fields_ = [("objects", ctypes.c_uint64), ("bytes", ctypes.c_int64), ("tombstones", ctypes.c_uint64),
                ("capacity", ctypes.c_uint64), ("rebuilds", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64),
                ("last_rows", ctypes.c_uint64), ("last_files", ctypes.c_uint64), ("last_missing", ctypes.c_uint64)]


class CacheWriteOut(ctypes.Structure):
    """rf_cache_write_out: what one rf_eval_wave_cache_write call did."""
    _fields_ = [("size", ctypes.c_uint64), ("nodes_written", ctypes.c_uint64), ("keys_put", ctypes.c_uint64),
                ("skipped_not_cacheable", ctypes.c_uint64), ("skipped_extern", ctypes.c_uint64),
                ("skipped_no_key", ctypes.c_uint64), ("node_keys", ctypes.c_void_p)]


class RepoMissingOut(ctypes.Structure):
    """rf_repo_missing_out: host pointers in the host forms, device pointers in the device forms."""
    _fields_ = [("n_files", ctypes.c_void_p), ("n_missing", ctypes.c_void_p), ("missing_bytes", ctypes.c_void_p),
                ("status", ctypes.c_void_p), ("cap", ctypes.c_uint64), ("miss_ptr", ctypes.c_void_p),
                ("miss_rows", ctypes.c_void_p), ("miss_ids32", ctypes.c_void_p), ("miss_sizes", ctypes.c_void_p),
                ("n_listed", ctypes.c_void_p)]


class PhysKeysOut(ctypes.Structure):
    """rf_physkeys_out: what one rf_physkeys_update call did."""
    _fields_ = [("size", ctypes.c_uint64), ("affected", ctypes.c_uint64), ("keys_written", ctypes.c_uint64),
                ("keys_zeroed", ctypes.c_uint64), ("material_bytes", ctypes.c_uint64), ("cap", ctypes.c_uint64),
                ("nodes", ctypes.c_void_p), ("computable", ctypes.c_void_p)]


class PhysKeysStats(ctypes.Structure):
    _fields_ = [("n_nodes", ctypes.c_uint64), ("n_values", ctypes.c_uint64), ("arena_bytes", ctypes.c_uint64),
                ("stale_bytes", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("last_ms", ctypes.c_double * 6)]


class ForestArrays(ctypes.Structure):
    """rf_forest_arrays: the host arrays of rf_fileset_forest_copy, for rf_physkeys_flat."""
    _fields_ = [("n_docs", ctypes.c_uint64), ("doc_node_ptr", ctypes.c_void_p), ("node_depth", ctypes.c_void_p),
                ("entry_ptr", ctypes.c_void_p), ("path_off", ctypes.c_void_p), ("paths", ctypes.c_void_p),
                ("ids32", ctypes.c_void_p)]


_lib = None


class FilesetPaths:
    """Argument arrays of rf_fileset_digest_device, built once: sets is a list
    of filesets, each a list of groups (a Map is one group), each a list of
    paths; File ID of entry e = d_ids32[e] (flattened order)."""

    def __init__(self, ctx, sets):
        self.ctx = ctx
        set_group, group_entry, paths = [0], [0], []
        for groups in sets:
            for g in groups:
                paths.extend(p.encode() if isinstance(p, str) else p for p in g)
                group_entry.append(len(paths))
            set_group.append(len(group_entry) - 1)
        self.n = len(sets)
        self.n_entries = len(paths)
        self.sg = np.array(set_group, dtype=np.uint64)
        self.ge = np.array(group_entry, dtype=np.uint64)
        self._pb = [ctypes.create_string_buffer(p, max(len(p), 1)) for p in paths]
        self.pp = (ctypes.c_void_p * max(len(paths), 1))(*[ctypes.addressof(b) for b in self._pb])
        self.pl = np.array([len(p) for p in paths] or [0], dtype=np.uint32)

    def digest_device(self, d_ids32) -> list:
        out = np.zeros(32 * self.n, dtype=np.uint8)
        _check(lib().rf_fileset_digest_device(self.ctx._h, self.n, _ptr(self.sg), _ptr(self.ge), self.pp,
                                              _ptr(self.pl), d_ids32, _ptr(out)))
        return [out[32 * i:32 * i + 32].tobytes() for i in range(self.n)]


def lib():
    """Load libreflow_hip.so.  Raises if it was not built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libreflow_hip.so not built: run __graft_entry__.build() "
                               "(make -C reflow_amd/csrc)")
        L = ctypes.CDLL(LIB_PATH)
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        sigs = {
            "rf_init": ([i32, vp], i32), "rf_destroy": ([vp], None),
            "rf_last_error": ([], ctypes.c_char_p), "rf_device_count": ([vp], i32),
            "rf_device_cus": ([vp, vp], i32),
            "rf_sync": ([vp], i32), "rf_version": ([], ctypes.c_char_p),
            "rf_sha256_batch": ([vp, vp, vp, u64, vp], i32),
            "rf_sha256_arena": ([vp, vp, vp, vp, u64, vp], i32),
            "rf_sha_plan_create": ([vp, vp, vp, u64, u32, vp], i32),
            "rf_sha_plan_run": ([vp, vp, vp, vp], i32),
            "rf_sha_plan_stats": ([vp, vp], i32), "rf_sha_plan_destroy": ([vp], None),
            "rf_sha_plan_prefix_stats": ([vp, vp], i32), "rf_sha_plan_set_prefixes": ([vp, vp, i32], i32),
            "rf_gen_fill": ([vp, vp, vp, vp, u64, u64, u64, vp], i32),
            "rf_fileset_digest_batch": ([vp, u64, vp, vp, vp, vp, vp, vp], i32),
            "rf_fileset_digest_device": ([vp, u64, vp, vp, vp, vp, vp, vp], i32),
            "rf_install_dir": ([vp, ctypes.c_char_p, vp], i32),
            "rf_install_info": ([vp, vp, vp, vp], i32),
            "rf_install_entries": ([vp, vp, vp, vp, vp], i32),
            "rf_install_destroy": ([vp], None),
            "rf_graph_load": ([vp, vp, vp], i32), "rf_graph_destroy": ([vp], None),
            "rf_graph_save": ([vp, ctypes.c_char_p], i32), "rf_graph_restore": ([vp, ctypes.c_char_p, vp], i32),
            "rf_graph_set_forms": ([vp, u64, u64, u64], i32),
            "rf_graph_set_slots": ([vp, vp, vp, u32], i32),
            "rf_graph_set_slots_device": ([vp, vp, vp, u32, vp], i32),
            "rf_graph_recompute": ([vp, i32, vp], i32),
            "rf_graph_recompute_async": ([vp, i32, vp], i32),
            "rf_graph_get_slots": ([vp, vp, u32, vp], i32),
            "rf_graph_stats_get": ([vp, vp], i32),
            "rf_graph_adopt_slots": ([vp, vp], i32),
            "rf_bloom_load": ([vp, u64, u64, vp, u64, u64, vp], i32),
            "rf_bloom_load_json": ([vp, ctypes.c_char_p, ctypes.c_size_t, vp], i32),
            "rf_bloom_load_binary": ([vp, vp, ctypes.c_size_t, vp], i32),
            "rf_bloom_new": ([vp, u64, u64, vp], i32), "rf_bloom_destroy": ([vp], None),
            "rf_bloom_probe": ([vp, vp, u64, vp], i32),
            "rf_bloom_probe_device": ([vp, vp, u64, vp, vp], i32),
            "rf_bloom_add": ([vp, vp, u64], i32),
            "rf_bloom_add_device": ([vp, vp, u64, vp], i32),
            "rf_bloom_params": ([vp, vp, vp, vp, vp], i32),
            "rf_bloom_words": ([vp, vp, u64], i32),
            "rf_malloc": ([vp, u64, vp], i32), "rf_free": ([vp, vp], i32),
            "rf_memcpy_h2d": ([vp, vp, vp, u64], i32), "rf_memcpy_d2h": ([vp, vp, vp, u64], i32),
            "rf_memset_d": ([vp, vp, i32, u64], i32), "rf_stream": ([vp], vp),
            "rf_timer_start": ([vp], i32), "rf_timer_stop": ([vp, vp], i32),
            "rf_comm_unique_id": ([vp], i32), "rf_comm_init": ([vp, i32, i32, vp, vp], i32),
            "rf_comm_destroy": ([vp], None), "rf_comm_allgather": ([vp, vp, vp, u64, vp], i32),
            "rf_comm_allreduce_or": ([vp, vp, u64, vp], i32),
            "rf_memcpy_d2d": ([vp, vp, vp, u64], i32),
            "rf_graph_gather_device": ([vp, vp, u32, vp, vp], i32),
            "rf_fileset_marshal_json": ([vp, u32, vp, u64, vp], i32),
            "rf_fileset_value_digest_batch": ([vp, vp, vp, u64, vp], i32),
            "rf_bloom_marshal_json": ([vp, vp, u64, vp], i32),
            "rf_bloom_marshal_binary": ([vp, vp, u64, vp], i32),
            "rf_bloom_collect": ([vp, vp, vp, u64, vp, vp, vp], i32),
            "rf_bloom_collect_device": ([vp, vp, vp, u64, vp, vp, vp], i32),
            "rf_dedup_digests": ([vp, vp, u32, vp, vp], i32),
            "rf_dedup_digests_device": ([vp, vp, u32, vp, vp, vp], i32),
            "rf_assoc_new": ([vp, u64, vp], i32), "rf_assoc_destroy": ([vp], None),
            "rf_assoc_put": ([vp, i32, vp, vp, vp, u64, vp], i32),
            "rf_assoc_get": ([vp, i32, vp, u64, vp, vp], i32),
            "rf_assoc_lookup": ([vp, i32, vp, vp, u64, vp, vp, vp, vp], i32),
            "rf_assoc_repair": ([vp, i32, vp, vp, u64, vp, vp, vp], i32),
            "rf_assoc_get_device": ([vp, i32, vp, u64, vp, vp, vp], i32),
            "rf_assoc_get_abbrev": ([vp, i32, vp, vp, u64, vp, vp, vp], i32),
            "rf_assoc_stats": ([vp, vp, vp], i32),
            "rf_assoc_put_device": ([vp, i32, vp, vp, vp, u64, vp], i32),
            "rf_assoc_count": ([vp, i32, vp, vp], i32),
            "rf_assoc_scan": ([vp, i32, u64, vp, vp, vp, vp], i32),
            "rf_assoc_scan_device": ([vp, i32, u64, vp, vp, vp, vp, vp], i32),
            "rf_assoc_compact": ([vp, u64], i32),
            "rf_assoc_save": ([vp, ctypes.c_char_p], i32),
            "rf_assoc_restore": ([vp, ctypes.c_char_p, vp], i32),
            "rf_assoc_file_format": ([vp, vp, vp, u64, u64, vp, u64, vp], i32),
            "rf_assoc_file_parse": ([vp, u64, vp, vp, vp, u64, vp], i32),
            "rf_set_host_threads": ([vp, i32], i32),
            "rf_sha_streams_open": ([vp, u64, u32, vp], i32), "rf_sha_streams_close": ([vp], None),
            "rf_sha_streams_write": ([vp, vp, vp, vp, u64], i32),
            "rf_sha_streams_digest": ([vp, vp, u64, vp], i32),
            "rf_sha_streams_len": ([vp, u64, vp], i32),
            "rf_sha_streams_verify": ([vp, vp, vp, u64, vp], i32),
            "rf_sha256_verify": ([vp, vp, vp, u64, vp, vp], i32),
            "rf_flow_dirty": ([vp, u64, vp, vp, vp, i32, vp], i32),
            "rf_graph_set_part": ([vp, vp], i32),
            "rf_graph_recompute_part": ([vp, vp, vp, vp, i32, vp], i32),
            "rf_graph_part_gathered": ([vp, vp, vp, vp], i32),
            "rf_graph_split": ([vp, i32, i32, vp, vp], i32), "rf_graph_piece_free": ([vp], None),
            "rf_graph_piece_desc": ([vp, vp], i32), "rf_graph_piece_part": ([vp, vp], i32),
            "rf_graph_piece_slots": ([vp, vp, vp], i32),
            "rf_host_info": ([vp, vp, vp, vp], i32), "rf_host_rate": ([vp, vp, vp], i32),
            "rf_host_link": ([vp, vp, vp], i32),
            "rf_bloom_parse_binary": ([vp, u64, vp, vp, vp, vp, u64, vp], i32),
            "rf_bloom_parse_json": ([vp, u64, vp, vp, vp, vp, u64, vp], i32),
            "rf_bloom_format_binary": ([u64, u64, u64, vp, u64, vp, u64, vp], i32),
            "rf_bloom_format_json": ([u64, u64, u64, vp, u64, vp, u64, vp], i32),
            "rf_coalescer_open": ([vp, i32, vp, i32, u64, u64, vp], i32), "rf_coalescer_close": ([vp], None),
            "rf_coalesce_sha256": ([vp, vp, u64, vp], i32), "rf_coalesce_probe": ([vp, vp, vp], i32),
            "rf_coalesce_assoc_get": ([vp, vp, vp, vp], i32),
            "rf_coalesce_sha256_async": ([vp, vp, u64, vp, vp], i32),
            "rf_coalesce_poll": ([vp, vp, vp], i32), "rf_coalesce_wait": ([vp, vp], i32),
            "rf_coalesce_ticket_free": ([vp, vp], None), "rf_coalescer_stats": ([vp, vp, vp, vp], i32),
            "rf_graph_update_recompute_async": ([vp, vp, vp, u32, vp], i32),
            "rf_walk_dir": ([ctypes.c_char_p, vp], i32), "rf_walk_info": ([vp, vp, vp], i32),
            "rf_walk_entries": ([vp, vp, vp, vp], i32), "rf_walk_free": ([vp], None),
            "rf_graph_feed_open": ([vp, vp], i32), "rf_graph_feed_close": ([vp], i32),
            "rf_graph_feed_poll": ([vp, u32, u64, vp, vp, vp, vp], i32),
            "rf_graph_feed_poll_device": ([vp, u32, u64, vp, vp, vp, vp], i32),
            "rf_graph_feed_lookup_device": ([vp, vp, vp, i32, u32, u64, vp, vp, vp, vp, vp, vp], i32),
            "rf_graph_feed_stats_get": ([vp, vp], i32),
            "rf_eval_plan_open": ([vp, u64, vp, vp, vp, vp, vp, vp], i32),
            "rf_eval_plan_check": ([u64, vp, vp, vp], i32), "rf_eval_plan_close": ([vp], None),
            "rf_eval_plan_set_flags": ([vp, vp, vp, u64], i32),
            "rf_eval_plan_run": ([vp, vp, u64, i32, vp, vp, vp, vp, i32, vp], i32),
            "rf_eval_plan_run_host": ([vp, vp, u64, i32, vp, vp, vp, i32], i32),
            "rf_eval_plan_reject": ([vp, vp, u64, vp, vp, vp, vp, i32, vp], i32),
            "rf_eval_plan_reject_host": ([vp, vp, u64, vp, vp, vp, i32], i32),
            "rf_eval_plan_states": ([vp, vp], i32), "rf_eval_plan_states_device": ([vp, vp], i32),
            "rf_eval_plan_list": ([vp, i32, u64, vp, vp, vp, vp, vp], i32),
            "rf_eval_plan_list_device": ([vp, i32, u64, vp, vp, vp, vp, vp, vp], i32),
            "rf_eval_plan_stats_get": ([vp, vp, u64], i32),
            "rf_eval_wave_consumers": ([u64, vp, vp, vp, vp], i32),
            "rf_eval_wave_open": ([vp, u64, vp, vp, vp, vp, vp, vp], i32), "rf_eval_wave_close": ([vp], None),
            "rf_eval_wave_set_flags": ([vp, vp, vp, u64], i32),
            "rf_eval_wave_begin": ([vp, vp, u64, i32, vp, vp, vp, vp, i32, vp], i32),
            "rf_eval_wave_begin_host": ([vp, vp, u64, i32, vp, vp, vp, i32], i32),
            "rf_eval_wave_begin_states": ([vp, vp, i32, vp], i32),
            "rf_eval_wave_step": ([vp, vp, u64, vp, vp, vp, vp, i32, vp], i32),
            "rf_eval_wave_step_host": ([vp, vp, u64, vp, vp, vp, i32], i32),
            "rf_eval_wave_reject": ([vp, vp, u64], i32),
            "rf_eval_wave_states": ([vp, vp], i32), "rf_eval_wave_states_device": ([vp, vp], i32),
            "rf_eval_wave_list": ([vp, i32, i32, u64, vp, vp, vp, vp, vp], i32),
            "rf_eval_wave_list_device": ([vp, i32, i32, u64, vp, vp, vp, vp, vp, vp], i32),
            "rf_eval_wave_stats_get": ([vp, vp, u64], i32),
            "rf_bloom_estimate": ([u64, ctypes.c_double, vp, vp], i32),
            "rf_liveset_open": ([vp, u64, vp, vp, vp], i32), "rf_liveset_close": ([vp], None),
            "rf_liveset_set_values": ([vp, vp, vp, u64, vp, vp], i32),
            "rf_liveset_set_values_device": ([vp, vp, vp, u64, vp, vp, vp], i32),
            "rf_liveset_clear_values": ([vp, vp, u64], i32),
            "rf_liveset_run": ([vp, vp, u64, vp, u64, vp], i32),
            "rf_liveset_filter": ([vp, vp], i32), "rf_liveset_states": ([vp, vp], i32),
            "rf_liveset_list": ([vp, i32, u64, vp, vp], i32),
            "rf_liveset_stats_get": ([vp, vp, u64], i32),
            "rf_repo_new": ([vp, u64, vp], i32), "rf_repo_destroy": ([vp], None),
            "rf_repo_put": ([vp, vp, vp, u64, vp], i32), "rf_repo_put_device": ([vp, vp, vp, u64, vp, vp], i32),
            "rf_repo_remove": ([vp, vp, u64, vp], i32), "rf_repo_remove_device": ([vp, vp, u64, vp, vp], i32),
            "rf_repo_stat": ([vp, vp, u64, vp], i32), "rf_repo_stat_device": ([vp, vp, u64, vp, vp], i32),
            "rf_repo_collect": ([vp, vp, vp, vp, vp], i32), "rf_repo_stats_get": ([vp, vp, u64], i32),
            "rf_repo_missing": ([vp, vp, u64, vp, vp, vp], i32),
            "rf_repo_missing_device": ([vp, vp, u64, vp, vp, u64, vp, vp], i32),
            "rf_repo_need_transfer": ([vp, vp, vp, u64, vp], i32),
            "rf_repo_need_transfer_device": ([vp, vp, vp, u64, vp, vp], i32),
            "rf_repo_scan": ([vp, u64, vp, vp, vp], i32), "rf_repo_scan_device": ([vp, u64, vp, vp, vp, vp], i32),
            "rf_repo_collect_list": ([vp, vp, u64, vp, vp, vp, vp], i32),
            "rf_repo_collect_list_device": ([vp, vp, u64, vp, vp, vp, vp, vp], i32),
            "rf_repo_compact": ([vp, u64], i32),
            "rf_repo_save": ([vp, ctypes.c_char_p], i32),
            "rf_repo_restore": ([vp, ctypes.c_char_p, vp], i32),
            "rf_repo_file_format": ([vp, vp, u64, u64, vp, u64, vp], i32),
            "rf_repo_file_parse": ([vp, u64, vp, vp, u64, vp], i32),
            "rf_fileset_marshal_flat": ([vp, vp, u64, vp, u64, vp, vp], i32),
            "rf_fileset_marshal_device": ([vp, vp, vp, u64, vp, vp, vp], i32),
            "rf_json_batch_info": ([vp, vp, vp, vp], i32), "rf_json_batch_lens": ([vp, vp], i32),
            "rf_json_batch_times": ([vp, vp], i32),
            "rf_json_batch_device": ([vp, vp, vp, vp], i32),
            "rf_json_batch_copy": ([vp, vp, u64, vp, u64, vp], i32),
            "rf_json_batch_digests_device": ([vp, vp, vp], i32), "rf_json_batch_free": ([vp], None),
            "rf_fileset_value_digest_device": ([vp, vp, vp, u64, vp, vp, vp, vp], i32),
            "rf_eval_wave_cache_write": ([vp, vp, u64, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp], i32),
            "rf_fileset_unmarshal_flat": ([vp, vp, u64, u32, u32, vp], i32),
            "rf_fileset_unmarshal_device": ([vp, vp, u64, vp, vp, u64, vp, vp], i32),
            "rf_fileset_unmarshal": ([vp, vp, vp, u64, vp, vp], i32),
            "rf_fileset_forest_info": ([vp, vp, vp, vp, vp, vp], i32),
            "rf_fileset_forest_status": ([vp, vp, vp, vp, vp], i32),
            "rf_fileset_forest_rows_device": ([vp, vp, vp, vp, vp], i32),
            "rf_fileset_forest_copy": ([vp, vp, vp, vp, vp, vp, vp, vp], i32),
            "rf_fileset_forest_tree": ([vp, u64, vp, u64, vp, vp, vp], i32),
            "rf_fileset_forest_times": ([vp, vp], i32), "rf_fileset_forest_free": ([vp], None),
            "rf_physkeys_open": ([vp, u64, vp, vp, vp, vp, vp, vp], i32), "rf_physkeys_close": ([vp], None),
            "rf_physkeys_set_values_forest": ([vp, vp, vp, vp], i32),
            "rf_physkeys_set_values_tree": ([vp, vp, vp, vp, u64, vp, vp], i32),
            "rf_physkeys_clear_values": ([vp, vp, u64], i32),
            "rf_physkeys_update": ([vp, vp, u64, u32, vp, u64, vp, vp], i32),
            "rf_physkeys_value_digests_device": ([vp, vp, u64, vp, vp], i32),
            "rf_physkeys_value_material": ([vp, u32, vp, u64, vp], i32),
            "rf_physkeys_stats_get": ([vp, vp], i32),
            "rf_physkeys_flat": ([u64, vp, vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, u64, vp, vp], i32),
        }
        for name, (args, res) in sigs.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _lib = L
    return _lib


def _check(rc):
    if rc != RF_OK:
        raise RfError(rc, lib().rf_last_error().decode(errors="replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data


def device_count():
    n = ctypes.c_int(0)
    rc = lib().rf_device_count(ctypes.byref(n))
    return n.value if rc == RF_OK else 0


class Context:
    """One rf_ctx bound to one HIP device (one process per GPU).

    host_threads: width of K1's host leg (rf_set_host_threads): None keeps the
    library default (min(60, CPU share)), 0 pins every message to the GPU
    kernels -- what the kernel parity tests use."""

    def __init__(self, device=0, host_threads=None):
        self._h = ctypes.c_void_p()
        _check(lib().rf_init(device, ctypes.byref(self._h)))
        self.device = device
        if host_threads is not None:
            self.set_host_threads(host_threads)

    def set_host_threads(self, n):
        _check(lib().rf_set_host_threads(self._h, -1 if n is None else int(n)))

    def host_info(self):
        """(threads, one core's SHA-NI bytes/s, has SHA extensions)."""
        t, r, e = ctypes.c_int(0), ctypes.c_double(0), ctypes.c_int(0)
        _check(lib().rf_host_info(self._h, ctypes.byref(t), ctypes.byref(r), ctypes.byref(e)))
        return t.value, r.value, bool(e.value)

    def n_cu(self):
        """rf_device_cus: the CU count the K1 planner's form thresholds scale with."""
        n = ctypes.c_int(0)
        _check(lib().rf_device_cus(self._h, ctypes.byref(n)))
        return n.value

    def host_link(self):
        """rf_host_link: (bytes/s the planner prices the host leg's HBM feed at,
        whether a run on this context measured it)."""
        r, m = ctypes.c_double(0), ctypes.c_int(0)
        _check(lib().rf_host_link(self._h, ctypes.byref(r), ctypes.byref(m)))
        return r.value, bool(m.value)

    def host_rate(self):
        """(chains per host-leg thread, one thread's measured bytes/s at that interleave)."""
        w, r = ctypes.c_int(0), ctypes.c_double(0)
        _check(lib().rf_host_rate(self._h, ctypes.byref(w), ctypes.byref(r)))
        return w.value, r.value

    def close(self):
        if self._h:
            lib().rf_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # ---- device memory (HBM owned through the engine's HIP runtime) ------
    def alloc(self, nbytes) -> "DeviceBuffer":
        return DeviceBuffer(self, nbytes)

    def upload(self, arr: np.ndarray) -> "DeviceBuffer":
        arr = np.ascontiguousarray(arr)
        b = DeviceBuffer(self, arr.nbytes)
        b.copy_from(arr)
        return b

    def timer_start(self):
        _check(lib().rf_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = ctypes.c_float(0)
        _check(lib().rf_timer_stop(self._h, ctypes.byref(ms)))
        return ms.value

    @property
    def stream(self):
        return lib().rf_stream(self._h)

    def sync(self):
        _check(lib().rf_sync(self._h))

    # ---- K1 -----------------------------------------------------------
    def sha256_batch(self, msgs):
        """SHA-256 of each bytes object (Digester.FromBytes, batched)."""
        n = len(msgs)
        if n == 0:
            return []
        bufs = [ctypes.create_string_buffer(bytes(m), max(len(m), 1)) for m in msgs]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
        lens = np.array([len(m) for m in msgs], dtype=np.uint64)
        out = np.zeros(32 * n, dtype=np.uint8)
        _check(lib().rf_sha256_batch(self._h, ptrs, _ptr(lens), n, _ptr(out)))
        return [out[32 * i:32 * i + 32].tobytes() for i in range(n)]

    def sha256_arena(self, arena: np.ndarray, offs: np.ndarray, lens: np.ndarray) -> np.ndarray:
        n = len(lens)
        out = np.zeros((n, 32), dtype=np.uint8)
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        _check(lib().rf_sha256_arena(self._h, _ptr(arena), _ptr(offs), _ptr(lens), n, _ptr(out)))
        return out

    def sha256_verify(self, msgs, want):
        """(rc, status per message) of rf_sha256_verify."""
        n = len(msgs)
        bufs = [ctypes.create_string_buffer(bytes(m), max(len(m), 1)) for m in msgs]
        ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(b) for b in bufs])
        lens = np.array([len(m) for m in msgs] or [0], dtype=np.uint64)
        w = np.frombuffer(b"".join(want) or bytes(32), dtype=np.uint8).copy()
        st = np.zeros(max(n, 1), dtype=np.int32)
        rc = lib().rf_sha256_verify(self._h, ptrs, _ptr(lens), n, _ptr(w), _ptr(st))
        if rc not in (RF_OK, RF_EINTEGRITY):
            _check(rc)
        return rc, st[:n]

    def flow_dirty(self, dep_ptr, deps, is_extern, no_cache_extern=True):
        """rf_flow_dirty: Eval.dirty of every node (bool array)."""
        dp = np.ascontiguousarray(dep_ptr, dtype=np.uint64)
        dv = np.ascontiguousarray(deps, dtype=np.uint32)
        ex = np.ascontiguousarray(is_extern, dtype=np.uint8)
        n = len(dp) - 1
        out = np.zeros(max(n, 1), dtype=np.uint8)
        _check(lib().rf_flow_dirty(self._h, n, _ptr(dp), _ptr(dv) if len(dv) else None, _ptr(ex),
                                   1 if no_cache_extern else 0, _ptr(out)))
        return out[:n].astype(bool)

    def sha_streams(self, n, flags=0):
        return ShaStreams(self, n, flags)

    def sha_plan(self, offs, lens, flags=0):
        return ShaPlan(self, offs, lens, flags)

    def gen_fill(self, d_arena, d_offs, d_lens, n, seed, arena_bytes, stream=None):
        _check(lib().rf_gen_fill(self._h, d_arena, d_offs, d_lens, n, seed & (2**64 - 1),
                                 arena_bytes, stream))

    # ---- Executor.install -------------------------------------------------
    def install_dir(self, root):
        """rf_install_dir: walk `root` (walker.go semantics), digest every file
        on the GPU.  Returns (entries, fileset_digest32) with entries a list of
        (relpath bytes, id32, size) in walk order (local/executor.go:514-557)."""
        h = ctypes.c_void_p()
        r = root.encode() if isinstance(root, str) else root
        _check(lib().rf_install_dir(self._h, r, ctypes.byref(h)))
        try:
            n, pb = ctypes.c_uint64(0), ctypes.c_uint64(0)
            fs = np.zeros(32, dtype=np.uint8)
            _check(lib().rf_install_info(h, ctypes.byref(n), ctypes.byref(pb), _ptr(fs)))
            n, pb = n.value, pb.value
            paths = np.zeros(max(pb, 1), dtype=np.uint8)
            offs = np.zeros(n + 1, dtype=np.uint64)
            ids = np.zeros(max(32 * n, 1), dtype=np.uint8)
            sizes = np.zeros(max(n, 1), dtype=np.int64)
            _check(lib().rf_install_entries(h, _ptr(paths), _ptr(offs), _ptr(ids), _ptr(sizes)))
        finally:
            lib().rf_install_destroy(h)
        pbytes = paths.tobytes()
        ents = [(pbytes[int(offs[i]):int(offs[i + 1])], ids[32 * i:32 * i + 32].tobytes(), int(sizes[i]))
                for i in range(n)]
        return ents, fs.tobytes()

    # ---- Fileset --------------------------------------------------------
    def fileset_digest_batch(self, sets):
        """sets: list of filesets, each a list of groups (a Map is one group,
        a List its flattened Map leaves); a group is a list of (path, id32)."""
        set_group = [0]
        group_entry = [0]
        paths, ids = [], []
        for groups in sets:
            for g in groups:
                for path, id32 in g:
                    paths.append(path.encode() if isinstance(path, str) else path)
                    ids.append(id32)
                group_entry.append(len(paths))
            set_group.append(len(group_entry) - 1)
        n = len(sets)
        sg = np.array(set_group, dtype=np.uint64)
        ge = np.array(group_entry, dtype=np.uint64)
        pb = [ctypes.create_string_buffer(p, max(len(p), 1)) for p in paths]
        pp = (ctypes.c_void_p * max(len(paths), 1))(*[ctypes.addressof(b) for b in pb])
        pl = np.array([len(p) for p in paths] or [0], dtype=np.uint32)
        idb = np.frombuffer(b"".join(ids) or b"\0" * 32, dtype=np.uint8).copy()
        out = np.zeros(32 * n, dtype=np.uint8)
        _check(lib().rf_fileset_digest_batch(self._h, n, _ptr(sg), _ptr(ge), pp, _ptr(pl),
                                             _ptr(idb), _ptr(out)))
        return [out[32 * i:32 * i + 32].tobytes() for i in range(n)]

    def fileset_paths(self, sets):
        """Marshals the paths of `sets` once (groups of paths; entry e = the
        e-th path in order) for repeated digests with device-resident IDs."""
        return FilesetPaths(self, sets)

    def dedup_digests(self, digests: np.ndarray):
        """Canonicalize's flowMap: (canon[i] = first index with digest i's value, n_unique)."""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1)
        n = len(d) // 32
        canon = np.zeros(max(n, 1), dtype=np.uint32)
        nu = ctypes.c_uint32(0)
        _check(lib().rf_dedup_digests(self._h, _ptr(d), n, _ptr(canon), ctypes.byref(nu)))
        return canon[:n], nu.value

    def dedup_digests_device(self, d_digests, n, d_canon, d_n_unique, stream=None):
        _check(lib().rf_dedup_digests_device(self._h, d_digests, n, d_canon, d_n_unique, stream))

    def fileset_value_digests(self, sets):
        """SHA256(json.Marshal(fs)) per fileset: CacheWrite's assoc values."""
        if not sets:
            return []
        b = FilesetTreeBuilder()
        roots = np.array([b.add(fs) for fs in sets], dtype=np.uint32)
        t = b.struct()
        out = np.zeros(32 * len(sets), dtype=np.uint8)
        _check(lib().rf_fileset_value_digest_batch(self._h, ctypes.byref(t), _ptr(roots), len(sets),
                                                   _ptr(out)))
        return [out[32 * i:32 * i + 32].tobytes() for i in range(len(sets))]

    def fileset_value_digests_device(self, sets, d_ids32=None):
        """The same through the device marshal (rf_fileset_value_digest_device):
        (fsids, JSON lengths).  d_ids32: the File IDs as device rows."""
        if not sets:
            return [], np.zeros(0, np.int64)
        b = FilesetTreeBuilder()
        roots = np.array([b.add(fs) for fs in sets], dtype=np.uint32)
        t = b.struct()
        n = len(sets)
        d_out, d_sz = self.alloc(32 * n), self.alloc(8 * n)
        try:
            _check(lib().rf_fileset_value_digest_device(self._h, ctypes.byref(t), _ptr(roots), n, d_ids32, d_out.ptr,
                                                        d_sz.ptr, None))
            out = d_out.to_numpy(np.uint8, 32 * n)
            sizes = d_sz.to_numpy(np.int64, n)
        finally:
            d_out.free()
            d_sz.free()
        return [out[32 * i:32 * i + 32].tobytes() for i in range(n)], sizes


class ShaStreams:
    """rf_sha_streams: n streaming SHA-256 writers (Digester.NewWriter)."""

    def __init__(self, ctx, n, flags=0):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(lib().rf_sha_streams_open(ctx.handle, n, flags, ctypes.byref(self._h)))

    def write(self, ids, chunks):
        """chunks[i] (bytes) to stream ids[i], in order."""
        n = len(ids)
        if n == 0:
            return
        bufs = [ctypes.create_string_buffer(bytes(c), max(len(c), 1)) for c in chunks]
        ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(b) for b in bufs])
        lens = np.array([len(c) for c in chunks], dtype=np.uint64)
        idv = np.ascontiguousarray(ids, dtype=np.uint64)
        _check(lib().rf_sha_streams_write(self._h, _ptr(idv), ptrs, _ptr(lens), n))

    def digest(self, ids):
        idv = np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.zeros(32 * max(len(idv), 1), dtype=np.uint8)
        _check(lib().rf_sha_streams_digest(self._h, _ptr(idv), len(idv), _ptr(out)))
        return [out[32 * i:32 * i + 32].tobytes() for i in range(len(idv))]

    def length(self, i):
        n = ctypes.c_uint64(0)
        _check(lib().rf_sha_streams_len(self._h, i, ctypes.byref(n)))
        return n.value

    def verify(self, ids, want):
        """(rc, status per stream): rc RF_OK or RF_EINTEGRITY."""
        idv = np.ascontiguousarray(ids, dtype=np.uint64)
        w = np.frombuffer(b"".join(want), dtype=np.uint8).copy()
        st = np.zeros(max(len(idv), 1), dtype=np.int32)
        rc = lib().rf_sha_streams_verify(self._h, _ptr(idv), _ptr(w), len(idv), _ptr(st))
        if rc not in (RF_OK, RF_EINTEGRITY):
            _check(rc)
        return rc, st[:len(idv)]

    def close(self):
        if self._h:
            lib().rf_sha_streams_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer:
    """HBM allocated through rf_malloc; .ptr is the device address."""

    def __init__(self, ctx: Context, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        _check(lib().rf_malloc(ctx.handle, self.nbytes, ctypes.byref(p)))
        self._p = p

    @property
    def ptr(self):
        return self._p.value

    def copy_from(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        _check(lib().rf_memcpy_h2d(self.ctx.handle, self._p, arr.ctypes.data, arr.nbytes))

    def to_numpy(self, dtype=np.uint8, count=None, offset=0) -> np.ndarray:
        """count elements of dtype from byte `offset` (default: the rest)."""
        dt = np.dtype(dtype)
        n = (self.nbytes - offset) // dt.itemsize if count is None else count
        assert 0 <= offset and offset + n * dt.itemsize <= self.nbytes
        out = np.empty(n, dtype=dt)
        _check(lib().rf_memcpy_d2h(self.ctx.handle, out.ctypes.data, ctypes.c_void_p(self.ptr + offset),
                                   out.nbytes))
        return out

    def zero(self):
        self.fill(0)

    def fill(self, byte):
        _check(lib().rf_memset_d(self.ctx.handle, self._p, int(byte), self.nbytes))

    def free(self):
        if self._p and self._p.value:
            lib().rf_free(self.ctx.handle, self._p)
            self._p = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Comm:
    """RCCL communicator (one rank per GPU) inside the engine."""

    @staticmethod
    def unique_id() -> bytes:
        b = ctypes.create_string_buffer(128)
        _check(lib().rf_comm_unique_id(b))
        return b.raw

    def __init__(self, ctx: Context, nranks, rank, uid: bytes):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(lib().rf_comm_init(ctx.handle, nranks, rank, ctypes.c_char_p(uid), ctypes.byref(self._h)))

    def allgather(self, d_send, d_recv, nbytes, stream=None):
        _check(lib().rf_comm_allgather(self._h, d_send, d_recv, nbytes, stream))

    def allreduce_or(self, d_words, nwords, stream=None):
        _check(lib().rf_comm_allreduce_or(self._h, d_words, nwords, stream))

    def close(self):
        if self._h:
            lib().rf_comm_destroy(self._h)
            self._h = ctypes.c_void_p()


class ShaPlan:
    def __init__(self, ctx: Context, offs, lens, flags=0):
        self.ctx = ctx
        self._offs = np.ascontiguousarray(offs, dtype=np.uint64)
        self._lens = np.ascontiguousarray(lens, dtype=np.uint64)
        self._h = ctypes.c_void_p()
        _check(lib().rf_sha_plan_create(ctx.handle, _ptr(self._offs), _ptr(self._lens),
                                        len(self._lens), flags, ctypes.byref(self._h)))

    def run(self, d_arena: int, d_out: int, stream=None):
        _check(lib().rf_sha_plan_run(self._h, d_arena, d_out, stream))

    def stats(self) -> ShaStats:
        s = ShaStats()
        _check(lib().rf_sha_plan_stats(self._h, ctypes.byref(s)))
        return s

    def prefix_stats(self) -> ShaPrefixStats:
        s = ShaPrefixStats()
        _check(lib().rf_sha_plan_prefix_stats(self._h, ctypes.byref(s)))
        return s

    def set_prefixes(self, prefix_blocks, mode=RF_PREFIX_RACE):
        """Test control: prefix_blocks[i] for host task i (largest first; None keeps
        the planner's) and how the run treats them (RF_PREFIX_RACE / WAIT / MISS)."""
        pb = None if prefix_blocks is None else np.ascontiguousarray(prefix_blocks, dtype=np.uint64)
        _check(lib().rf_sha_plan_set_prefixes(self._h, None if pb is None else pb.ctypes.data, mode))

    def close(self):
        if self._h:
            lib().rf_sha_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Graph:
    """rf_graph: jobs over digest slots (see include/reflow_hip.h)."""

    def __init__(self, ctx: Context, n_slots, out_slot, tmpl_off, tmpl_len, hole_ptr, hole_pos,
                 hole_slot, blob: bytes | np.ndarray):
        self.ctx = ctx
        self._keep = dict(
            out_slot=np.ascontiguousarray(out_slot, dtype=np.uint32),
            tmpl_off=np.ascontiguousarray(tmpl_off, dtype=np.uint64),
            tmpl_len=np.ascontiguousarray(tmpl_len, dtype=np.uint32),
            hole_ptr=np.ascontiguousarray(hole_ptr, dtype=np.uint64),
            hole_pos=np.ascontiguousarray(hole_pos, dtype=np.uint32),
            hole_slot=np.ascontiguousarray(hole_slot, dtype=np.uint32),
            blob=np.frombuffer(bytes(blob), dtype=np.uint8) if isinstance(blob, (bytes, bytearray))
            else np.ascontiguousarray(blob, dtype=np.uint8),
        )
        k = self._keep
        d = GraphDesc(len(k["out_slot"]), n_slots, _ptr(k["out_slot"]), _ptr(k["tmpl_off"]),
                      _ptr(k["tmpl_len"]), _ptr(k["hole_ptr"]),
                      _ptr(k["hole_pos"]) if len(k["hole_pos"]) else None,
                      _ptr(k["hole_slot"]) if len(k["hole_slot"]) else None,
                      _ptr(k["blob"]) if len(k["blob"]) else None, len(k["blob"]))
        self._h = ctypes.c_void_p()
        _check(lib().rf_graph_load(ctx.handle, ctypes.byref(d), ctypes.byref(self._h)))
        self._keep = None  # not retained by the library

    def set_slots(self, slots, digests: np.ndarray):
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        dg = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1)
        _check(lib().rf_graph_set_slots(self._h, _ptr(slots), _ptr(dg), len(slots)))

    def set_slots_device(self, d_slots, d_digests, n, stream=None):
        _check(lib().rf_graph_set_slots_device(self._h, d_slots, d_digests, n, stream))

    def recompute(self, full=False) -> int:
        n = ctypes.c_uint64(0)
        _check(lib().rf_graph_recompute(self._h, 1 if full else 0, ctypes.byref(n)))
        return n.value

    def recompute_async(self, full=False, stream=None):
        _check(lib().rf_graph_recompute_async(self._h, 1 if full else 0, stream))

    def update_recompute_async(self, d_slots, d_digests32, n, stream=None):
        """set_slots_device + recompute_async(full=False) as one graph launch."""
        _check(lib().rf_graph_update_recompute_async(self._h, d_slots, d_digests32, n, stream))

    def gather_device(self, d_slots, n, d_out, stream=None):
        _check(lib().rf_graph_gather_device(self._h, d_slots, n, d_out, stream))

    def get_slots(self, slots) -> np.ndarray:
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros((len(slots), 32), dtype=np.uint8)
        _check(lib().rf_graph_get_slots(self._h, _ptr(slots), len(slots), _ptr(out)))
        return out

    def stats(self) -> GraphStats:
        s = GraphStats()
        _check(lib().rf_graph_stats_get(self._h, ctypes.byref(s)))
        return s

    def adopt_slots(self, src):
        """rf_graph_adopt_slots: take src's whole slot table (same numbering),
        ready for incremental steps without a full recompute."""
        _check(lib().rf_graph_adopt_slots(self._h, src._h))

    # kernel-form thresholds (include/reflow_hip.h RF_K2_THRU*_DEFAULT)
    THRU_DEFAULT, THRU_WIDE_DEFAULT, THRU_MARK_DEFAULT = 24576, 65536, 98304
    NEVER = (1 << 64) - 1

    def set_forms(self, thru, thru_wide=None, thru_mark=None):
        """rf_graph_set_forms: 0 = always the throughput form, Graph.NEVER =
        never; thru_wide / thru_mark default to thru."""
        _check(lib().rf_graph_set_forms(self._h, int(thru), int(thru if thru_wide is None else thru_wide),
                                        int(thru if thru_mark is None else thru_mark)))

    def save(self, path):
        """rf_graph_save: the lowered graph and its slot digests to `path`."""
        _check(lib().rf_graph_save(self._h, os.fsencode(path)))

    @classmethod
    def restore(cls, ctx, path):
        """rf_graph_restore: a graph saved by save(), ready for incremental steps."""
        g = cls.__new__(cls)
        g.ctx, g._keep = ctx, None
        g._h = ctypes.c_void_p()
        _check(lib().rf_graph_restore(ctx.handle, os.fsencode(path), ctypes.byref(g._h)))
        return g

    @classmethod
    def from_arrays(cls, ctx, a):
        return cls(ctx, a["n_slots"], a["out_slot"], a["tmpl_off"], a["tmpl_len"], a["hole_ptr"], a["hole_pos"],
                   a["hole_slot"], a["blob"])

    def set_part(self, part):
        """part: dict(nranks, rank, max_export, export_slot, import_slot,
        import_bid, any_import[, rounds]) (GraphPiece.part); rounds > 0 selects
        the fixed-round exchange (0: supersteps until nothing changes)."""
        ex = np.ascontiguousarray(part["export_slot"], dtype=np.uint32)
        im = np.ascontiguousarray(part["import_slot"], dtype=np.uint32)
        ib = np.ascontiguousarray(part["import_bid"], dtype=np.uint32)
        p = GraphPart(part["nranks"], part["rank"], part["max_export"], len(ex), _ptr(ex) if len(ex) else None,
                      len(im), _ptr(im) if len(im) else None, _ptr(ib) if len(ib) else None,
                      1 if part.get("any_import", True) else 0, int(part.get("rounds", 0)))
        _check(lib().rf_graph_set_part(self._h, ctypes.byref(p)))

    def recompute_part(self, comm=None, allgather=None, nranks=1, full=False, count=True) -> int:
        """Recompute across ranks: comm (Comm, RCCL) or allgather (bytes ->
        [bytes per rank], a host transport).  count=False: no readback of the
        jobs hashed (with comm and fixed rounds the call is then asynchronous)."""
        fn = host_allgather_fn(allgather, nranks) if allgather is not None else None
        self._fn = fn  # alive during the call
        n = ctypes.c_uint64(0)
        _check(lib().rf_graph_recompute_part(self._h, comm._h if comm is not None else None,
                                             ctypes.cast(fn, ctypes.c_void_p) if fn is not None else None, None,
                                             1 if full else 0, ctypes.byref(n) if count else None))
        return n.value

    def part_gathered(self):
        """(device pointer of the gathered export digests, count, supersteps)."""
        p, n, st = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().rf_graph_part_gathered(self._h, ctypes.byref(p), ctypes.byref(n), ctypes.byref(st)))
        return p.value, n.value, st.value

    # ---- change feed (include/reflow_hip.h "Change feed") ----
    def feed_open(self, mask=None):
        """rf_graph_feed_open.  mask: None (every job-output slot), a uint64
        word array [ceil(n_slots / 64)], or a bool array over the slots."""
        if mask is not None:
            mask = np.asarray(mask)
            if mask.dtype == np.bool_:
                bits = np.zeros((len(mask) + 63) // 64 * 64, dtype=np.uint8)
                bits[:len(mask)] = mask
                mask = np.packbits(bits, bitorder="little").view("<u8")
            mask = np.ascontiguousarray(mask, dtype=np.uint64)
        _check(lib().rf_graph_feed_open(self._h, _ptr(mask) if mask is not None and len(mask) else None))

    def feed_close(self):
        _check(lib().rf_graph_feed_close(self._h))

    def feed_poll(self, cap=None, flags=0):
        """rf_graph_feed_poll: (slots uint32[written], digests uint8[written][32],
        found).  cap None: room for every tracked slot."""
        if cap is None:
            cap = self.feed_stats().tracked_slots
        cap = int(cap)
        slots = np.zeros(max(cap, 1), dtype=np.uint32)
        dig = np.zeros((max(cap, 1), 32), dtype=np.uint8)
        found, written = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _check(lib().rf_graph_feed_poll(self._h, flags, cap, _ptr(slots), _ptr(dig), ctypes.byref(found),
                                        ctypes.byref(written)))
        return slots[:written.value].copy(), dig[:written.value].copy(), found.value

    def feed_poll_device(self, cap, d_slots, d_digests32, d_n2, flags=0, stream=None):
        _check(lib().rf_graph_feed_poll_device(self._h, flags, cap, d_slots, d_digests32, d_n2, stream))

    def feed_lookup_device(self, live, assoc, kind, cap, d_slots, d_keys32, d_status, d_vals32, d_n2, flags=0,
                           stream=None):
        """rf_graph_feed_lookup_device: live a Bloom or None, assoc an Assoc."""
        _check(lib().rf_graph_feed_lookup_device(self._h, live._h if live is not None else None, assoc._h, kind,
                                                 flags, cap, d_slots, d_keys32, d_status, d_vals32, d_n2, stream))

    def feed_stats(self) -> GraphFeedStats:
        s = GraphFeedStats()
        _check(lib().rf_graph_feed_stats_get(self._h, ctypes.byref(s)))
        return s

    def close(self):
        if self._h:
            lib().rf_graph_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bloom:
    """rf_bloom: device-resident willf/bloom filter with bloomlive semantics."""

    def __init__(self, ctx: Context, handle, owned=True):
        self.ctx = ctx
        self._h = handle
        self._owned = owned  # False: borrowed (GcLiveset.filter): never destroyed from here

    @classmethod
    def load(cls, ctx, m, k, words: np.ndarray, length):
        h = ctypes.c_void_p()
        w = np.ascontiguousarray(words, dtype=np.uint64)
        _check(lib().rf_bloom_load(ctx.handle, m, k, _ptr(w) if len(w) else None, len(w), length,
                                   ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def new(cls, ctx, m, k):
        h = ctypes.c_void_p()
        _check(lib().rf_bloom_new(ctx.handle, m, k, ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_json(cls, ctx, js: bytes):
        h = ctypes.c_void_p()
        _check(lib().rf_bloom_load_json(ctx.handle, js, len(js), ctypes.byref(h)))
        return cls(ctx, h)

    @classmethod
    def from_binary(cls, ctx, buf: bytes):
        h = ctypes.c_void_p()
        b = np.frombuffer(buf, dtype=np.uint8).copy()
        _check(lib().rf_bloom_load_binary(ctx.handle, _ptr(b), len(b), ctypes.byref(h)))
        return cls(ctx, h)

    def probe(self, digests: np.ndarray) -> np.ndarray:
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1)
        n = len(d) // 32
        out = np.zeros(n, dtype=np.uint8)
        _check(lib().rf_bloom_probe(self._h, _ptr(d), n, _ptr(out)))
        return out

    def probe_device(self, d_digests, n, d_out, stream=None):
        _check(lib().rf_bloom_probe_device(self._h, d_digests, n, d_out, stream))

    def add(self, digests: np.ndarray):
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1)
        _check(lib().rf_bloom_add(self._h, _ptr(d), len(d) // 32))

    def add_device(self, d_digests, n, stream=None):
        _check(lib().rf_bloom_add_device(self._h, d_digests, n, stream))

    def params(self):
        m, k, ln, nw = (ctypes.c_uint64() for _ in range(4))
        _check(lib().rf_bloom_params(self._h, ctypes.byref(m), ctypes.byref(k), ctypes.byref(ln),
                                     ctypes.byref(nw)))
        return m.value, k.value, ln.value, nw.value

    def words(self) -> np.ndarray:
        _, _, _, nw = self.params()
        out = np.zeros(nw, dtype=np.uint64)
        _check(lib().rf_bloom_words(self._h, _ptr(out) if nw else None, nw))
        return out

    def _marshal(self, fn) -> bytes:
        need = ctypes.c_uint64(0)
        rc = fn(self._h, None, 0, ctypes.byref(need))
        if rc != RF_OK and need.value == 0:
            _check(rc)
        out = ctypes.create_string_buffer(max(need.value, 1))
        _check(fn(self._h, out, need.value, ctypes.byref(need)))
        return out.raw[:need.value]

    def marshal_json(self) -> bytes:
        return self._marshal(lib().rf_bloom_marshal_json)

    def marshal_binary(self) -> bytes:
        return self._marshal(lib().rf_bloom_marshal_binary)

    def collect(self, digests: np.ndarray, sizes=None):
        """Repository.Collect over a batch: (ascending dead indices, dead bytes)."""
        d = np.ascontiguousarray(digests, dtype=np.uint8).reshape(-1)
        n = len(d) // 32
        sz = None if sizes is None else np.ascontiguousarray(sizes, dtype=np.int64)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        nd, nb = ctypes.c_uint64(0), ctypes.c_int64(0)
        _check(lib().rf_bloom_collect(self._h, _ptr(d), _ptr(sz), n, _ptr(out), ctypes.byref(nd),
                                      ctypes.byref(nb)))
        return out[:nd.value], nb.value

    def collect_device(self, d_digests, d_sizes, n, d_dead_idx, d_counts2, stream=None):
        _check(lib().rf_bloom_collect_device(self._h, d_digests, d_sizes, n, d_dead_idx, d_counts2, stream))

    def close(self):
        if self._h and self._owned:
            lib().rf_bloom_destroy(self._h)
        self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def walk_dir(root):
    """rf_walk_dir (host-only, no device): internal/walker's Scan as install
    uses it -> [(relpath bytes, Stat size)] in walk order."""
    w = ctypes.c_void_p()
    _check(lib().rf_walk_dir(os.fsencode(root), ctypes.byref(w)))
    try:
        n, pb = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().rf_walk_info(w, ctypes.byref(n), ctypes.byref(pb)))
        paths = ctypes.create_string_buffer(max(pb.value, 1))
        offs = np.zeros(n.value + 1, np.uint64)
        sizes = np.zeros(n.value + 1, np.int64)
        _check(lib().rf_walk_entries(w, paths, _ptr(offs), _ptr(sizes)))
        raw = paths.raw
        return [(raw[int(offs[i]):int(offs[i + 1])], int(sizes[i])) for i in range(n.value)]
    finally:
        lib().rf_walk_free(w)


RF_COALESCE_SHA256, RF_COALESCE_PROBE, RF_COALESCE_ASSOC_GET = 1, 2, 3


class Coalescer:
    """rf_coalescer: concurrent callers (threads) coalesced into device
    batches.  target: a Bloom (PROBE) or an Assoc (ASSOC_GET)."""

    def __init__(self, ctx, kind, target=None, assoc_kind=0, max_batch=4096, max_wait_us=200):
        self.ctx, self.kind, self.target = ctx, kind, target
        self._h = ctypes.c_void_p()
        _check(lib().rf_coalescer_open(ctx.handle, kind, target._h if target is not None else None, assoc_kind,
                                       max_batch, max_wait_us, ctypes.byref(self._h)))

    def sha256(self, msg: bytes) -> bytes:
        out = ctypes.create_string_buffer(32)
        _check(lib().rf_coalesce_sha256(self._h, msg, len(msg), out))
        return out.raw

    def probe(self, digest32: bytes) -> bool:
        out = ctypes.c_uint8(0)
        _check(lib().rf_coalesce_probe(self._h, digest32, ctypes.byref(out)))
        return bool(out.value)

    def assoc_get(self, key32: bytes):
        val, found = ctypes.create_string_buffer(32), ctypes.c_uint8(0)
        _check(lib().rf_coalesce_assoc_get(self._h, key32, val, ctypes.byref(found)))
        return bool(found.value), val.raw

    def sha256_async(self, msg: bytes):
        """-> ticket (msg and the result buffer are kept alive by it)."""
        buf = ctypes.create_string_buffer(msg, len(msg)) if msg else ctypes.create_string_buffer(1)
        out = ctypes.create_string_buffer(32)
        t = ctypes.c_void_p()
        _check(lib().rf_coalesce_sha256_async(self._h, buf, len(msg), out, ctypes.byref(t)))
        return {"t": t, "buf": buf, "out": out}

    def poll(self, ticket) -> bool:
        done = ctypes.c_int(0)
        _check(lib().rf_coalesce_poll(self._h, ticket["t"], ctypes.byref(done)))
        return bool(done.value)

    def wait(self, ticket) -> bytes:
        _check(lib().rf_coalesce_wait(self._h, ticket["t"]))
        return ticket["out"].raw

    def free(self, ticket):
        lib().rf_coalesce_ticket_free(self._h, ticket["t"])
        ticket["t"] = None

    def stats(self):
        b, r, m = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().rf_coalescer_stats(self._h, ctypes.byref(b), ctypes.byref(r), ctypes.byref(m)))
        return b.value, r.value, m.value

    def close(self):
        if self._h:
            lib().rf_coalescer_close(self._h)
            self._h = ctypes.c_void_p()


class Assoc:
    """HBM assoc (assoc.Assoc with the in-memory assoc's semantics)."""

    def __init__(self, ctx: Context, capacity=1024):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(lib().rf_assoc_new(ctx.handle, capacity, ctypes.byref(self._h)))

    def put(self, kind, keys, vals, expect=None) -> np.ndarray:
        k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
        v = np.ascontiguousarray(vals, dtype=np.uint8).reshape(-1)
        e = None if expect is None else np.ascontiguousarray(expect, dtype=np.uint8).reshape(-1)
        n = len(k) // 32
        st = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().rf_assoc_put(self._h, kind, _ptr(e), _ptr(k), _ptr(v), n, _ptr(st)))
        return st[:n]

    def get(self, kind, keys):
        k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
        n = len(k) // 32
        vals = np.zeros((max(n, 1), 32), dtype=np.uint8)
        found = np.zeros(max(n, 1), dtype=np.uint8)
        _check(lib().rf_assoc_get(self._h, kind, _ptr(k), n, _ptr(vals), _ptr(found)))
        return vals[:n], found[:n]

    def lookup(self, kind, keys, key_ptr):
        """rf_assoc_lookup (read only): keys (rows of 32 B) grouped per node by
        key_ptr (n_nodes + 1 offsets).  Returns (which int32 per node, values,
        found per key, value per key)."""
        k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
        kp = np.ascontiguousarray(key_ptr, dtype=np.uint64)
        n, nk = len(kp) - 1, len(k) // 32
        which = np.zeros(max(n, 1), dtype=np.int32)
        vals = np.zeros((max(n, 1), 32), dtype=np.uint8)
        kf = np.zeros(max(nk, 1), dtype=np.uint8)
        kv = np.zeros((max(nk, 1), 32), dtype=np.uint8)
        _check(lib().rf_assoc_lookup(self._h, kind, _ptr(k) if len(k) else None, _ptr(kp), n, _ptr(which),
                                     _ptr(vals), _ptr(kf), _ptr(kv)))
        return which[:n], vals[:n], kf[:nk], kv[:nk]

    def repair(self, kind, keys, key_ptr, which, vals, key_found=None):
        """rf_assoc_repair: read repair of the nodes with which >= 0 (blind, or
        precise with key_found)."""
        k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
        kp = np.ascontiguousarray(key_ptr, dtype=np.uint64)
        w = np.ascontiguousarray(which, dtype=np.int32)
        v = np.ascontiguousarray(vals, dtype=np.uint8).reshape(-1)
        kf = None if key_found is None else np.ascontiguousarray(key_found, dtype=np.uint8)
        _check(lib().rf_assoc_repair(self._h, kind, _ptr(k) if len(k) else None, _ptr(kp), len(kp) - 1, _ptr(w),
                                     _ptr(v), _ptr(kf) if kf is not None and len(kf) else None))

    def put_device(self, kind, d_keys, d_vals, n, d_status, d_expect=None):
        _check(lib().rf_assoc_put_device(self._h, kind, d_expect, d_keys, d_vals, n, d_status))

    def get_device(self, kind, d_keys, n, d_vals, d_found, stream=None):
        _check(lib().rf_assoc_get_device(self._h, kind, d_keys, n, d_vals, d_found, stream))

    def get_abbrev(self, kind, keys, nhex):
        k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
        n = len(k) // 32
        nh = np.ascontiguousarray(nhex, dtype=np.uint8)
        ko = np.zeros((max(n, 1), 32), dtype=np.uint8)
        vo = np.zeros((max(n, 1), 32), dtype=np.uint8)
        st = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().rf_assoc_get_abbrev(self._h, kind, _ptr(k), _ptr(nh), n, _ptr(ko), _ptr(vo), _ptr(st)))
        return ko[:n], vo[:n], st[:n]

    def stats(self):
        o, c = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().rf_assoc_stats(self._h, ctypes.byref(o), ctypes.byref(c)))
        return o.value, c.value

    def count(self, kind=-1):
        """rf_assoc_count: (live, deleted) of one kind, or of every kind (kind < 0)."""
        lv, dl = ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().rf_assoc_count(self._h, kind, ctypes.byref(lv), ctypes.byref(dl)))
        return lv.value, dl.value

    def scan(self, kind=-1, cap_entries=None):
        """rf_assoc_scan: the live entries as (keys [n, 32], vals [n, 32], kinds
        [n] int32), ascending by slot.  cap_entries: the buffers' rows (default:
        the live count); RfError(RF_EINVAL) with .needed = n when short."""
        cap = self.count(kind)[0] if cap_entries is None else int(cap_entries)
        keys = np.zeros((max(cap, 1), 32), dtype=np.uint8)
        vals = np.zeros((max(cap, 1), 32), dtype=np.uint8)
        kinds = np.zeros(max(cap, 1), dtype=np.int32)
        n = ctypes.c_uint64()
        rc = lib().rf_assoc_scan(self._h, kind, cap, _ptr(keys), _ptr(vals), _ptr(kinds), ctypes.byref(n))
        if rc != RF_OK:
            err = RfError(rc, lib().rf_last_error().decode(errors="replace"))
            err.needed = n.value
            raise err
        return keys[:n.value], vals[:n.value], kinds[:n.value]

    def scan_device(self, kind, cap_entries, d_keys, d_vals, d_kinds, d_n, stream=None):
        _check(lib().rf_assoc_scan_device(self._h, kind, cap_entries, d_keys, d_vals, d_kinds, d_n, stream))

    def compact(self, min_capacity=0):
        """rf_assoc_compact: rebuild the table without its deleted keys."""
        _check(lib().rf_assoc_compact(self._h, min_capacity))

    def save(self, path):
        """rf_assoc_save: the live entries as a checksummed file (restore())."""
        _check(lib().rf_assoc_save(self._h, os.fsencode(path)))

    @classmethod
    def restore(cls, ctx, path):
        """rf_assoc_restore: a new assoc holding a saved file's entries."""
        a = cls.__new__(cls)
        a.ctx = ctx
        a._h = ctypes.c_void_p()
        _check(lib().rf_assoc_restore(ctx.handle, os.fsencode(path), ctypes.byref(a._h)))
        return a

    def close(self):
        if self._h:
            lib().rf_assoc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def eval_plan_check(dep_ptr, deps) -> int:
    """rf_eval_plan_check (host only): the depth bound (nodes on the longest
    path) of a node graph in CSR form; RfError RF_EINVAL for pointers that are
    not monotone, a dep out of range or a cycle."""
    dp = np.ascontiguousarray(dep_ptr, dtype=np.uint64)
    de = np.ascontiguousarray(deps, dtype=np.uint32)
    depth = ctypes.c_uint32()
    _check(lib().rf_eval_plan_check(max(len(dp) - 1, 0), _ptr(dp) if len(dp) else None,
                                    _ptr(de) if len(de) else None, ctypes.byref(depth)))
    return depth.value


class EvalPlan:
    """rf_eval_plan: Eval.todo + Eval.lookup in top-down mode for a whole Flow
    graph, on the device.  dep_ptr / deps: the nodes' Deps in CSR form; flags:
    one RF_PLAN_F_* byte per node; key_ptr: node i's cache keys are key rows
    [key_ptr[i], key_ptr[i+1]); key_slots: per key row, a slot of a Graph's
    slot table (for run(graph=...))."""

    def __init__(self, ctx: Context, dep_ptr, deps, flags, key_ptr, key_slots=None):
        self.ctx = ctx
        dp = np.ascontiguousarray(dep_ptr, dtype=np.uint64)
        de = np.ascontiguousarray(deps, dtype=np.uint32)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        kp = np.ascontiguousarray(key_ptr, dtype=np.uint64)
        ks = None if key_slots is None else np.ascontiguousarray(key_slots, dtype=np.uint32)
        self.n = len(fl)
        self.n_keys = int(kp[-1]) if len(kp) else 0
        self._h = ctypes.c_void_p()
        _check(lib().rf_eval_plan_open(ctx.handle, self.n, _ptr(dp) if self.n else None,
                                       _ptr(de) if len(de) else None, _ptr(fl) if self.n else None,
                                       _ptr(kp) if self.n else None,
                                       None if ks is None else (_ptr(ks) if len(ks) else _ptr(np.zeros(1, np.uint32))),
                                       ctypes.byref(self._h)))

    def set_flags(self, nodes, flags):
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        assert len(nd) == len(fl)
        _check(lib().rf_eval_plan_set_flags(self._h, _ptr(nd) if len(nd) else None, _ptr(fl) if len(fl) else None,
                                            len(nd)))

    @staticmethod
    def _h_of(o):
        return None if o is None else o._h

    def run(self, roots, assoc, kind, keys=None, graph=None, d_keys=None, live=None, no_cache_extern=False,
            stream=None):
        """One plan from `roots`.  Keys: keys (host rows in key_ptr order:
        rf_eval_plan_run_host), or d_keys (device rows) / graph (its slot table
        through key_slots): rf_eval_plan_run on `stream`."""
        r = np.ascontiguousarray(roots, dtype=np.uint32)
        rp = _ptr(r) if len(r) else None
        if graph is None and d_keys is None:
            k = np.ascontiguousarray(keys if keys is not None else np.zeros(0, np.uint8), dtype=np.uint8).reshape(-1)
            assert len(k) == 32 * self.n_keys
            _check(lib().rf_eval_plan_run_host(self._h, rp, len(r), int(bool(no_cache_extern)),
                                               _ptr(k) if len(k) else None, self._h_of(live), assoc._h, kind))
        else:
            _check(lib().rf_eval_plan_run(self._h, rp, len(r), int(bool(no_cache_extern)), self._h_of(graph),
                                          d_keys, self._h_of(live), assoc._h, kind, stream))

    def reject(self, nodes, assoc, kind, keys=None, graph=None, d_keys=None, live=None, stream=None):
        """rf_eval_plan_reject(_host): these hits failed the caller's checks."""
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        np_ = _ptr(nd) if len(nd) else None
        if graph is None and d_keys is None:
            k = np.ascontiguousarray(keys if keys is not None else np.zeros(0, np.uint8), dtype=np.uint8).reshape(-1)
            assert len(k) == 32 * self.n_keys
            _check(lib().rf_eval_plan_reject_host(self._h, np_, len(nd), _ptr(k) if len(k) else None,
                                                  self._h_of(live), assoc._h, kind))
        else:
            _check(lib().rf_eval_plan_reject(self._h, np_, len(nd), self._h_of(graph), d_keys, self._h_of(live),
                                             assoc._h, kind, stream))

    def states(self) -> np.ndarray:
        out = np.zeros(max(self.n, 1), dtype=np.uint8)
        _check(lib().rf_eval_plan_states(self._h, _ptr(out)))
        return out[:self.n]

    def states_device(self) -> int:
        p = ctypes.c_void_p()
        _check(lib().rf_eval_plan_states_device(self._h, ctypes.byref(p)))
        return p.value

    def count(self, state) -> int:
        n = ctypes.c_uint64()
        rc = lib().rf_eval_plan_list(self._h, state, 0, None, None, None, None, ctypes.byref(n))
        if rc != RF_OK and not (rc == RF_EINVAL and n.value):
            _check(rc)
        return n.value

    def list(self, state, cap=None, poison=None):
        """rf_eval_plan_list: (nodes uint32 [found], which uint8, vals [found, 32],
        key_found uint8), ascending by node; the last three only carry data for
        RF_PLAN_HIT.  cap: the buffers' rows (default: the count); poison: the
        byte the buffers are filled with first.  RfError(RF_EINVAL) with
        .needed = found and .buffers = the four arrays when short."""
        cap = self.count(state) if cap is None else int(cap)
        fill = 0 if poison is None else poison
        nodes = np.full(max(cap, 1), fill * 0x01010101, dtype=np.uint32)
        which = np.full(max(cap, 1), fill, dtype=np.uint8)
        vals = np.full((max(cap, 1), 32), fill, dtype=np.uint8)
        kf = np.full(max(cap, 1), fill, dtype=np.uint8)
        n = ctypes.c_uint64()
        rc = lib().rf_eval_plan_list(self._h, state, cap, _ptr(nodes), _ptr(which), _ptr(vals), _ptr(kf),
                                     ctypes.byref(n))
        if rc != RF_OK:
            err = RfError(rc, lib().rf_last_error().decode(errors="replace"))
            err.needed = n.value
            err.buffers = (nodes, which, vals, kf)
            raise err
        return nodes[:n.value], which[:n.value], vals[:n.value], kf[:n.value]

    def list_device(self, state, cap, d_nodes, d_which, d_vals, d_key_found, d_found, stream=None):
        _check(lib().rf_eval_plan_list_device(self._h, state, cap, d_nodes, d_which, d_vals, d_key_found, d_found,
                                              stream))

    def stats(self) -> EvalPlanStats:
        s = EvalPlanStats()
        _check(lib().rf_eval_plan_stats_get(self._h, ctypes.byref(s), ctypes.sizeof(s)))
        return s

    def close(self):
        if self._h:
            lib().rf_eval_plan_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def eval_wave_consumers(dep_ptr, deps):
    """rf_eval_wave_consumers (host only): (cons_ptr uint64 [n+1], cons uint32):
    for node d the nodes that list d as a dep, one entry per dep entry,
    ascending within a node; RfError RF_EINVAL as eval_plan_check."""
    dp = np.ascontiguousarray(dep_ptr, dtype=np.uint64)
    de = np.ascontiguousarray(deps, dtype=np.uint32)
    n = max(len(dp) - 1, 0)
    cp = np.zeros(n + 1, dtype=np.uint64)
    co = np.zeros(max(len(de), 1), dtype=np.uint32)
    _check(lib().rf_eval_wave_consumers(n, _ptr(dp) if len(dp) else None, _ptr(de) if len(de) else None,
                                        _ptr(cp), _ptr(co)))
    return cp, co[:len(de)]


class EvalWave:
    """rf_eval_wave: bottom-up evaluation and the completion step on the
    device.  The constructor takes EvalPlan's arguments.  begin() starts
    bottom-up from roots, begin_states() continues a top-down plan; step()
    takes the nodes that finished and resolves the nodes that became ready;
    reject() turns hits the caller's checks refused into READY."""

    def __init__(self, ctx: Context, dep_ptr, deps, flags, key_ptr, key_slots=None):
        self.ctx = ctx
        dp = np.ascontiguousarray(dep_ptr, dtype=np.uint64)
        de = np.ascontiguousarray(deps, dtype=np.uint32)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        kp = np.ascontiguousarray(key_ptr, dtype=np.uint64)
        ks = None if key_slots is None else np.ascontiguousarray(key_slots, dtype=np.uint32)
        self.n = len(fl)
        self.n_keys = int(kp[-1]) if len(kp) else 0
        self._h = ctypes.c_void_p()
        _check(lib().rf_eval_wave_open(ctx.handle, self.n, _ptr(dp) if self.n else None,
                                       _ptr(de) if len(de) else None, _ptr(fl) if self.n else None,
                                       _ptr(kp) if self.n else None,
                                       None if ks is None else (_ptr(ks) if len(ks) else _ptr(np.zeros(1, np.uint32))),
                                       ctypes.byref(self._h)))

    def set_flags(self, nodes, flags):
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        fl = np.ascontiguousarray(flags, dtype=np.uint8)
        assert len(nd) == len(fl)
        _check(lib().rf_eval_wave_set_flags(self._h, _ptr(nd) if len(nd) else None, _ptr(fl) if len(fl) else None,
                                            len(nd)))

    @staticmethod
    def _h_of(o):
        return None if o is None else o._h

    def _host_keys(self, keys):
        k = np.ascontiguousarray(keys if keys is not None else np.zeros(0, np.uint8), dtype=np.uint8).reshape(-1)
        assert len(k) == 32 * self.n_keys
        return k

    def begin(self, roots, assoc, kind, keys=None, graph=None, d_keys=None, live=None, no_cache_extern=False,
              stream=None):
        """Bottom-up from `roots`; wave 0 is resolved.  Keys as EvalPlan.run."""
        r = np.ascontiguousarray(roots, dtype=np.uint32)
        rp = _ptr(r) if len(r) else None
        if graph is None and d_keys is None:
            k = self._host_keys(keys)
            _check(lib().rf_eval_wave_begin_host(self._h, rp, len(r), int(bool(no_cache_extern)),
                                                 _ptr(k) if len(k) else None, self._h_of(live), assoc._h, kind))
        else:
            _check(lib().rf_eval_wave_begin(self._h, rp, len(r), int(bool(no_cache_extern)), self._h_of(graph),
                                            d_keys, self._h_of(live), assoc._h, kind, stream))

    def begin_states(self, states=None, d_states=None, stream=None):
        """The top-down continuation: states (host bytes, one per node) or
        d_states (a device pointer, EvalPlan.states_device())."""
        if d_states is not None:
            _check(lib().rf_eval_wave_begin_states(self._h, d_states, 1, stream))
        else:
            st = np.ascontiguousarray(states, dtype=np.uint8)
            assert len(st) == self.n
            _check(lib().rf_eval_wave_begin_states(self._h, _ptr(st) if self.n else None, 0, stream))

    def step(self, nodes, assoc=None, kind=0, keys=None, graph=None, d_keys=None, live=None, stream=None):
        """The listed nodes have finished; the next wave is resolved."""
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        np_ = _ptr(nd) if len(nd) else None
        if graph is None and d_keys is None:
            k = None if keys is None else self._host_keys(keys)
            _check(lib().rf_eval_wave_step_host(self._h, np_, len(nd), _ptr(k) if k is not None and len(k) else None,
                                                self._h_of(live), self._h_of(assoc), kind))
        else:
            _check(lib().rf_eval_wave_step(self._h, np_, len(nd), self._h_of(graph), d_keys, self._h_of(live),
                                           self._h_of(assoc), kind, stream))

    def reject(self, nodes):
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        _check(lib().rf_eval_wave_reject(self._h, _ptr(nd) if len(nd) else None, len(nd)))

    def cache_write(self, nodes, d_fsids32, d_sizes, assoc, kind, graph=None, d_keys=None, repo=None,
                    no_cache_extern=False, per_node=True, stream=None):
        """rf_eval_wave_cache_write: the listed (DONE) nodes' values, row i of
        d_fsids32 / d_sizes for nodes[i], Put under every present key and into
        the repository index.  Returns (CacheWriteOut, keys put per listed node)."""
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        o = CacheWriteOut()
        o.size = ctypes.sizeof(o)
        per = np.zeros(max(len(nd), 1), dtype=np.uint8) if per_node else None
        o.node_keys = _ptr(per)
        _check(lib().rf_eval_wave_cache_write(self._h, _ptr(nd) if len(nd) else None, len(nd), d_fsids32, d_sizes,
                                              int(bool(no_cache_extern)), self._h_of(graph), d_keys, assoc._h, kind,
                                              self._h_of(repo), ctypes.byref(o), stream))
        return o, (per[:len(nd)] if per_node else None)

    def states(self) -> np.ndarray:
        out = np.zeros(max(self.n, 1), dtype=np.uint8)
        _check(lib().rf_eval_wave_states(self._h, _ptr(out)))
        return out[:self.n]

    def states_device(self) -> int:
        p = ctypes.c_void_p()
        _check(lib().rf_eval_wave_states_device(self._h, ctypes.byref(p)))
        return p.value

    def count(self, state, scope=RF_WAVE_ALL) -> int:
        n = ctypes.c_uint64()
        rc = lib().rf_eval_wave_list(self._h, state, scope, 0, None, None, None, None, ctypes.byref(n))
        if rc != RF_OK and not (rc == RF_EINVAL and n.value):
            _check(rc)
        return n.value

    def list(self, state, scope=RF_WAVE_ALL, cap=None, poison=None):
        """rf_eval_wave_list: as EvalPlan.list, over every node or the last wave."""
        cap = self.count(state, scope) if cap is None else int(cap)
        fill = 0 if poison is None else poison
        nodes = np.full(max(cap, 1), fill * 0x01010101, dtype=np.uint32)
        which = np.full(max(cap, 1), fill, dtype=np.uint8)
        vals = np.full((max(cap, 1), 32), fill, dtype=np.uint8)
        kf = np.full(max(cap, 1), fill, dtype=np.uint8)
        n = ctypes.c_uint64()
        rc = lib().rf_eval_wave_list(self._h, state, scope, cap, _ptr(nodes), _ptr(which), _ptr(vals), _ptr(kf),
                                     ctypes.byref(n))
        if rc != RF_OK:
            err = RfError(rc, lib().rf_last_error().decode(errors="replace"))
            err.needed = n.value
            err.buffers = (nodes, which, vals, kf)
            raise err
        return nodes[:n.value], which[:n.value], vals[:n.value], kf[:n.value]

    def list_device(self, state, scope, cap, d_nodes, d_which, d_vals, d_key_found, d_found, stream=None):
        _check(lib().rf_eval_wave_list_device(self._h, state, scope, cap, d_nodes, d_which, d_vals, d_key_found,
                                              d_found, stream))

    def stats(self) -> EvalWaveStats:
        s = EvalWaveStats()
        _check(lib().rf_eval_wave_stats_get(self._h, ctypes.byref(s), ctypes.sizeof(s)))
        return s

    def close(self):
        if self._h:
            lib().rf_eval_wave_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bloom_estimate(n: int, p: float):
    """rf_bloom_estimate (host only): bloom.EstimateParameters -> (m, k)."""
    m, k = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().rf_bloom_estimate(n, p, ctypes.byref(m), ctypes.byref(k)))
    return m.value, k.value


class GcLiveset:
    """rf_liveset: Eval.collect's walk, dedup and filter build on the device.
    edge_ptr / edges: the nodes' Deps (an OpMap's MapFlow appended) in CSR
    form.  Values are set as nodes finish; run() is one collection."""

    def __init__(self, ctx: Context, edge_ptr, edges):
        self.ctx = ctx
        ep = np.ascontiguousarray(edge_ptr, dtype=np.uint64)
        ed = np.ascontiguousarray(edges, dtype=np.uint32)
        self.n = max(len(ep) - 1, 0)
        self._h = ctypes.c_void_p()
        self._lent = []  # weak references to the Blooms filter() handed out
        _check(lib().rf_liveset_open(ctx.handle, self.n, _ptr(ep) if self.n else None, _ptr(ed) if len(ed) else None,
                                     ctypes.byref(self._h)))

    @staticmethod
    def _lists(nodes, counts):
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        ct = np.ascontiguousarray(counts, dtype=np.uint32)
        assert len(nd) == len(ct)
        return nd, ct

    def set_values(self, nodes, counts, ids32, sizes):
        """nodes[i] gets the next counts[i] rows of ids32 [rows, 32] / sizes [rows]."""
        nd, ct = self._lists(nodes, counts)
        ids = np.ascontiguousarray(ids32, dtype=np.uint8).reshape(-1)
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        assert len(ids) == 32 * len(sz) and len(sz) == int(ct.sum(dtype=np.uint64))
        _check(lib().rf_liveset_set_values(self._h, _ptr(nd) if len(nd) else None, _ptr(ct) if len(ct) else None,
                                           len(nd), _ptr(ids) if len(ids) else None, _ptr(sz) if len(sz) else None))

    def set_values_device(self, nodes, counts, d_ids32, d_sizes, stream=None):
        nd, ct = self._lists(nodes, counts)
        _check(lib().rf_liveset_set_values_device(self._h, _ptr(nd) if len(nd) else None,
                                                  _ptr(ct) if len(ct) else None, len(nd), d_ids32, d_sizes, stream))

    def clear_values(self, nodes):
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        _check(lib().rf_liveset_clear_values(self._h, _ptr(nd) if len(nd) else None, len(nd)))

    def run(self, roots, writers=(), stream=None) -> "LivesetStats":
        r = np.ascontiguousarray(roots, dtype=np.uint32)
        w = np.ascontiguousarray(writers, dtype=np.uint32)
        _check(lib().rf_liveset_run(self._h, _ptr(r) if len(r) else None, len(r), _ptr(w) if len(w) else None,
                                    len(w), stream))
        return self.stats()

    def filter(self) -> "Bloom":
        """The last run's filter, borrowed: valid until the next run or close
        (closing the returned Bloom only drops the handle; close() here
        drops the handles of every Bloom handed out)."""
        h = ctypes.c_void_p()
        _check(lib().rf_liveset_filter(self._h, ctypes.byref(h)))
        b = Bloom(self.ctx, h, owned=False)
        self._lent = [r for r in self._lent if r() is not None] + [weakref.ref(b)]
        return b

    def states(self) -> np.ndarray:
        out = np.zeros(max(self.n, 1), dtype=np.uint8)
        _check(lib().rf_liveset_states(self._h, _ptr(out)))
        return out[:self.n]

    def count(self, state) -> int:
        n = ctypes.c_uint64()
        rc = lib().rf_liveset_list(self._h, state, 0, None, ctypes.byref(n))
        if rc != RF_OK and not (rc == RF_EINVAL and n.value):
            _check(rc)
        return n.value

    def list(self, state, cap=None, poison=None) -> np.ndarray:
        """rf_liveset_list: the nodes in `state`, ascending.  cap: the buffer's
        rows (default: the count); RfError(RF_EINVAL) with .needed and .buffer
        when short."""
        cap = self.count(state) if cap is None else int(cap)
        nodes = np.full(max(cap, 1), (0 if poison is None else poison) * 0x01010101, dtype=np.uint32)
        n = ctypes.c_uint64()
        rc = lib().rf_liveset_list(self._h, state, cap, _ptr(nodes), ctypes.byref(n))
        if rc != RF_OK:
            err = RfError(rc, lib().rf_last_error().decode(errors="replace"))
            err.needed = n.value
            err.buffer = nodes
            raise err
        return nodes[:n.value]

    def stats(self) -> LivesetStats:
        s = LivesetStats()
        _check(lib().rf_liveset_stats_get(self._h, ctypes.byref(s), ctypes.sizeof(s)))
        return s

    def close(self):
        for r in getattr(self, "_lent", []):  # the filters die with the object
            b = r()
            if b is not None:
                b._h = ctypes.c_void_p()
        self._lent = []
        if self._h:
            lib().rf_liveset_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RepoMissing:
    """What Repo.missing / Repo.need_transfer return: per-group arrays, the
    list of distinct missing files (group by group, first occurrence
    ascending) and n_listed, the total whether the list fitted or not."""

    FIELDS = ("n_files", "n_missing", "missing_bytes", "status", "miss_ptr", "miss_rows", "miss_ids32", "miss_sizes",
              "n_listed")

    def __init__(self):
        for f in self.FIELDS:
            setattr(self, f, None)


class Repo:
    """rf_repo: a repository's object index in HBM -- batched Put / Stat /
    Remove / Collect, and missing() / NeedTransfer for batches of values."""

    def __init__(self, ctx: Context, capacity=0):
        self.ctx = ctx
        self._h = ctypes.c_void_p()
        _check(lib().rf_repo_new(ctx.handle, capacity, ctypes.byref(self._h)))

    @staticmethod
    def _ids(ids32):
        ids = np.ascontiguousarray(ids32, dtype=np.uint8).reshape(-1)
        assert len(ids) % 32 == 0
        return ids, len(ids) // 32

    def put(self, ids32, sizes) -> np.ndarray:
        ids, n = self._ids(ids32)
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        assert len(sz) == n
        st = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().rf_repo_put(self._h, _ptr(ids) if n else None, _ptr(sz) if n else None, n, _ptr(st)))
        return st[:n]

    def put_device(self, d_ids32, d_sizes, n, d_status, stream=None):
        _check(lib().rf_repo_put_device(self._h, d_ids32, d_sizes, n, d_status, stream))

    def remove(self, ids32) -> np.ndarray:
        ids, n = self._ids(ids32)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        _check(lib().rf_repo_remove(self._h, _ptr(ids) if n else None, n, _ptr(out)))
        return out[:n]

    def remove_device(self, d_ids32, n, d_removed, stream=None):
        _check(lib().rf_repo_remove_device(self._h, d_ids32, n, d_removed, stream))

    def stat(self, ids32) -> np.ndarray:
        ids, n = self._ids(ids32)
        out = np.zeros(max(n, 1), dtype=np.int64)
        _check(lib().rf_repo_stat(self._h, _ptr(ids) if n else None, n, _ptr(out)))
        return out[:n]

    def stat_device(self, d_ids32, n, d_sizes, stream=None):
        _check(lib().rf_repo_stat_device(self._h, d_ids32, n, d_sizes, stream))

    def collect(self, live=None, stream=None):
        """Repository.Collect on the index: (objects removed, their bytes); live None removes everything."""
        n, b = ctypes.c_uint64(), ctypes.c_int64()
        _check(lib().rf_repo_collect(self._h, live._h if live is not None else None, ctypes.byref(n),
                                     ctypes.byref(b), stream))
        return n.value, b.value

    def stats(self) -> RepoStats:
        s = RepoStats()
        _check(lib().rf_repo_stats_get(self._h, ctypes.byref(s), ctypes.sizeof(s)))
        return s

    def _host_out(self, n_groups, cap, want, poison):
        """Host arrays for the fields in `want` (the others stay NULL), filled with the byte `poison`."""
        res, o = RepoMissing(), RepoMissingOut()
        shapes = {"n_files": (np.uint32, n_groups), "n_missing": (np.uint32, n_groups),
                  "missing_bytes": (np.int64, n_groups), "status": (np.int32, n_groups),
                  "miss_ptr": (np.uint64, n_groups + 1), "miss_rows": (np.uint64, cap),
                  "miss_ids32": (np.uint8, 32 * cap), "miss_sizes": (np.int64, cap), "n_listed": (np.uint64, 1)}
        for f in want:
            dt, n = shapes[f]
            a = np.frombuffer(bytes([poison]) * (max(n, 1) * np.dtype(dt).itemsize), dtype=dt).copy()
            setattr(res, f, a)
            setattr(o, f, a.ctypes.data)
        o.cap = cap
        return res, o

    @staticmethod
    def _trim(res, n_groups, cap, rc):
        """Cut the arrays to their lengths; the list arrays keep all `cap` rows (the caller checks the cap rule)."""
        for f, n in (("n_files", n_groups), ("n_missing", n_groups), ("missing_bytes", n_groups),
                     ("status", n_groups), ("miss_ptr", n_groups + 1), ("miss_rows", cap), ("miss_sizes", cap)):
            if getattr(res, f) is not None:
                setattr(res, f, getattr(res, f)[:n])
        if res.miss_ids32 is not None:
            res.miss_ids32 = res.miss_ids32[:32 * cap].reshape(-1, 32)
        if res.n_listed is not None:
            res.n_listed = int(res.n_listed[0])
        res.rc = rc
        return res

    def missing(self, counts, ids32, sizes, cap=None, want=RepoMissing.FIELDS, poison=0, check=True) -> RepoMissing:
        """rf_repo_missing: counts[g] rows per group.  cap: rows of the list
        arrays (default: every row could be listed).  check=False returns the
        status in .rc instead of raising (the cap rule's RF_EINVAL)."""
        ct = np.ascontiguousarray(counts, dtype=np.uint32)
        ids, n = self._ids(ids32)
        sz = np.ascontiguousarray(sizes, dtype=np.int64)
        assert len(sz) == n
        cap = n if cap is None else int(cap)
        want = [f for f in want if f != "status"]
        res, o = self._host_out(len(ct), cap, want, poison)
        rc = lib().rf_repo_missing(self._h, _ptr(ct) if len(ct) else None, len(ct), _ptr(ids) if n else None,
                                   _ptr(sz) if n else None, ctypes.byref(o))
        if check:
            _check(rc)
        return self._trim(res, len(ct), cap, rc)

    def missing_device(self, d_counts, n_groups, d_ids32, d_sizes, n_rows, out: RepoMissingOut, stream=None):
        _check(lib().rf_repo_missing_device(self._h, d_counts, n_groups, d_ids32, d_sizes, n_rows, ctypes.byref(out),
                                            stream))

    def need_transfer(self, liveset, nodes, cap, want=RepoMissing.FIELDS, poison=0, check=True) -> RepoMissing:
        """rf_repo_need_transfer: group g = the values of nodes[g]'s deps in `liveset` (a GcLiveset)."""
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        want = [f for f in want if f != "miss_rows"]
        res, o = self._host_out(len(nd), int(cap), want, poison)
        rc = lib().rf_repo_need_transfer(self._h, liveset._h, _ptr(nd) if len(nd) else None, len(nd), ctypes.byref(o))
        if check:
            _check(rc)
        return self._trim(res, len(nd), int(cap), rc)

    def need_transfer_device(self, liveset, d_nodes, n_nodes, out: RepoMissingOut, stream=None):
        _check(lib().rf_repo_need_transfer_device(self._h, liveset._h, d_nodes, n_nodes, ctypes.byref(out), stream))

    @staticmethod
    def _list_out(cap, ids, sizes, poison):
        """Host arrays of `cap` rows for a list (None where not wanted), filled with the byte `poison`."""
        a = np.full((max(cap, 1), 32), poison, dtype=np.uint8) if ids else None
        b = np.frombuffer(bytes([poison]) * (8 * max(cap, 1)), dtype=np.int64).copy() if sizes else None
        return a, b

    def scan(self, cap=None, ids=True, sizes=True, poison=0, check=True):
        """rf_repo_scan: (ids [cap, 32] or None, sizes [cap] or None, n, rc) --
        the live objects in ascending slot order in the first min(n, cap) rows.
        cap: rows of the arrays (default: the live count, the arrays then cut to
        n).  check=False returns the cap rule's RF_EINVAL in rc instead of raising."""
        full = cap is None
        cap = self.stats().objects if full else int(cap)
        a, b = self._list_out(cap, ids, sizes, poison)
        n = ctypes.c_uint64()
        rc = lib().rf_repo_scan(self._h, cap, _ptr(a), _ptr(b), ctypes.byref(n))
        if check:
            _check(rc)
        keep = n.value if full else cap
        return (a[:keep] if a is not None else None, b[:keep] if b is not None else None, n.value, rc)

    def scan_device(self, cap, d_ids32, d_sizes, d_n, stream=None):
        _check(lib().rf_repo_scan_device(self._h, cap, d_ids32, d_sizes, d_n, stream))

    def collect_list(self, live=None, cap=None, ids=True, sizes=True, poison=0, check=True):
        """rf_repo_collect_list: (ids, sizes, removed, removed_bytes, rc) -- the
        removed objects in ascending slot order; all or nothing against cap
        (default: the live count, the arrays then cut to `removed`)."""
        full = cap is None
        cap = self.stats().objects if full else int(cap)
        a, b = self._list_out(cap, ids, sizes, poison)
        n, nb = ctypes.c_uint64(), ctypes.c_int64()
        rc = lib().rf_repo_collect_list(self._h, live._h if live is not None else None, cap, _ptr(a), _ptr(b),
                                        ctypes.byref(n), ctypes.byref(nb))
        if check:
            _check(rc)
        keep = n.value if full else cap
        return (a[:keep] if a is not None else None, b[:keep] if b is not None else None, n.value, nb.value, rc)

    def collect_list_device(self, live, cap, d_ids32, d_sizes, d_removed, d_removed_bytes=None, stream=None):
        _check(lib().rf_repo_collect_list_device(self._h, live._h if live is not None else None, cap, d_ids32,
                                                 d_sizes, d_removed, d_removed_bytes, stream))

    def compact(self, min_capacity=0):
        """rf_repo_compact: rebuild the table without its tombstones."""
        _check(lib().rf_repo_compact(self._h, min_capacity))

    def save(self, path):
        """rf_repo_save: the live objects as a checksummed file (restore())."""
        _check(lib().rf_repo_save(self._h, os.fsencode(path)))

    @classmethod
    def restore(cls, ctx, path):
        """rf_repo_restore: a new index holding a saved file's objects."""
        r = cls.__new__(cls)
        r.ctx = ctx
        r._h = ctypes.c_void_p()
        _check(lib().rf_repo_restore(ctx.handle, os.fsencode(path), ctypes.byref(r._h)))
        return r

    def close(self):
        if self._h:
            lib().rf_repo_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def assoc_file_format(kinds, keys, vals, chunk=0) -> bytes:
    """rf_assoc_file_format (host only): the assoc file of entries given in
    (kind, key) order."""
    kd = np.ascontiguousarray(kinds, dtype=np.int32)
    k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1)
    v = np.ascontiguousarray(vals, dtype=np.uint8).reshape(-1)
    n = len(kd)
    need = ctypes.c_uint64()
    lib().rf_assoc_file_format(_ptr(kd), _ptr(k), _ptr(v), n, chunk, None, 0, ctypes.byref(need))  # the size
    out = np.zeros(need.value, dtype=np.uint8)
    _check(lib().rf_assoc_file_format(_ptr(kd), _ptr(k), _ptr(v), n, chunk, _ptr(out), len(out), ctypes.byref(need)))
    return out.tobytes()


def assoc_file_parse(buf: bytes):
    """rf_assoc_file_parse (host only): (kinds int32 [n], keys [n, 32], vals
    [n, 32]) of an assoc file; RfError RF_EINVAL / RF_EINTEGRITY for a bad one."""
    b = np.frombuffer(bytes(buf), dtype=np.uint8)
    n = ctypes.c_uint64()
    rc = lib().rf_assoc_file_parse(_ptr(b) if len(b) else None, len(b), None, None, None, 0, ctypes.byref(n))
    if rc != RF_OK and not (rc == RF_EINVAL and n.value):
        _check(rc)
    kinds = np.zeros(max(n.value, 1), dtype=np.int32)
    keys = np.zeros((max(n.value, 1), 32), dtype=np.uint8)
    vals = np.zeros((max(n.value, 1), 32), dtype=np.uint8)
    _check(lib().rf_assoc_file_parse(_ptr(b), len(b), _ptr(kinds), _ptr(keys), _ptr(vals), n.value, ctypes.byref(n)))
    return kinds[:n.value], keys[:n.value], vals[:n.value]


def repo_file_format(ids32, sizes, chunk=0, cap=None) -> bytes:
    """rf_repo_file_format (host only): the index file of objects given in ID
    order.  cap: the output buffer's bytes (default: what the file needs); a
    short one raises RfError(RF_EINVAL) with .needed = the file's length."""
    ids = np.ascontiguousarray(ids32, dtype=np.uint8).reshape(-1)
    sz = np.ascontiguousarray(sizes, dtype=np.int64)
    n = len(sz)
    assert len(ids) == 32 * n
    need = ctypes.c_uint64()
    if cap is None:
        lib().rf_repo_file_format(_ptr(ids), _ptr(sz), n, chunk, None, 0, ctypes.byref(need))  # the size
        cap = need.value
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    rc = lib().rf_repo_file_format(_ptr(ids), _ptr(sz), n, chunk, _ptr(out), cap, ctypes.byref(need))
    if rc != RF_OK:
        err = RfError(rc, lib().rf_last_error().decode(errors="replace"))
        err.needed = need.value
        raise err
    return out[:need.value].tobytes()


def repo_file_parse(buf: bytes, cap_entries=None):
    """rf_repo_file_parse (host only): (ids [n, 32], sizes int64 [n]) of an
    index file; RfError RF_EINVAL / RF_EINTEGRITY for a bad one.  cap_entries:
    the arrays' rows (default: the file's); a short one raises
    RfError(RF_EINVAL) with .needed = the file's entries."""
    b = np.frombuffer(bytes(buf), dtype=np.uint8)
    n = ctypes.c_uint64()
    if cap_entries is None:
        rc = lib().rf_repo_file_parse(_ptr(b) if len(b) else None, len(b), None, None, 0, ctypes.byref(n))
        if rc != RF_OK and not (rc == RF_EINVAL and n.value):
            _check(rc)
        cap_entries = n.value
    ids = np.zeros((max(cap_entries, 1), 32), dtype=np.uint8)
    sizes = np.zeros(max(cap_entries, 1), dtype=np.int64)
    n = ctypes.c_uint64()
    rc = lib().rf_repo_file_parse(_ptr(b) if len(b) else None, len(b), _ptr(ids), _ptr(sizes), cap_entries,
                                  ctypes.byref(n))
    if rc != RF_OK:
        err = RfError(rc, lib().rf_last_error().decode(errors="replace"))
        err.needed = n.value
        raise err
    return ids[:n.value], sizes[:n.value]


def _phys_graph_args(dep_ptr, deps, phys_row, suffixes):
    """The open arguments as arrays: suffixes is one bytes object per node."""
    dp = np.ascontiguousarray(dep_ptr, dtype=np.uint64)
    de = np.ascontiguousarray(deps, dtype=np.uint32)
    pr = np.ascontiguousarray(phys_row, dtype=np.uint64)
    n = len(pr)
    sp = np.zeros(n + 1, dtype=np.uint64)
    if n:
        sp[1:] = np.cumsum([len(x) for x in suffixes], dtype=np.uint64)
    sb = np.frombuffer(b"".join(suffixes) or b"\0", dtype=np.uint8).copy()
    return n, dp, de, pr, sp, sb


class PhysKeys:
    """rf_physkeys: the finished nodes' Fileset materials in HBM and the
    physical keys (Flow.PhysicalDigest) of the consumers they affect, written
    into the caller's d_keys32 rows.  phys_row[i] = node i's key row or
    RF_PHYS_NO_ROW; suffixes[i] = the bytes after the deps' materials."""

    def __init__(self, ctx: Context, dep_ptr, deps, phys_row, suffixes=None, suffix_ptr=None, suffix=None):
        self.ctx = ctx
        if suffixes is not None:
            self.n, dp, de, pr, sp, sb = _phys_graph_args(dep_ptr, deps, phys_row, suffixes)
        else:  # raw arrays, as the C call takes them
            dp = np.ascontiguousarray(dep_ptr, dtype=np.uint64)
            de = np.ascontiguousarray(deps, dtype=np.uint32)
            pr = np.ascontiguousarray(phys_row, dtype=np.uint64)
            sp = np.ascontiguousarray(suffix_ptr, dtype=np.uint64)
            sb = np.ascontiguousarray(suffix if suffix is not None and len(suffix) else np.zeros(1, np.uint8),
                                      dtype=np.uint8)
            self.n = len(pr)
        self._h = ctypes.c_void_p()
        _check(lib().rf_physkeys_open(ctx.handle, self.n, _ptr(dp) if self.n else None, _ptr(de) if len(de) else None,
                                      _ptr(pr) if self.n else None, _ptr(sp) if self.n else None, _ptr(sb),
                                      ctypes.byref(self._h)))

    def set_values_forest(self, nodes, forest, stream=None):
        """Document d of a device-form FilesetForest becomes the value of nodes[d] (RF_PHYS_SKIP: none)."""
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        assert len(nd) == forest.n_docs
        _check(lib().rf_physkeys_set_values_forest(self._h, _ptr(nd) if len(nd) else None, forest._h, stream))

    def set_values(self, nodes, sets=None, tree=None, roots=None, d_ids32=None, stream=None):
        """Fileset objects (or tree + roots) become the values of nodes; d_ids32: the File IDs as device rows."""
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        if sets is not None:
            b = FilesetTreeBuilder()
            roots = [b.add(fs) for fs in sets]
            tree = b.struct()
        r = np.ascontiguousarray(roots, dtype=np.uint32)
        assert len(r) == len(nd)
        _check(lib().rf_physkeys_set_values_tree(self._h, _ptr(nd) if len(nd) else None, ctypes.byref(tree),
                                                 _ptr(r) if len(r) else None, len(r), d_ids32, stream))

    def clear_values(self, nodes):
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        _check(lib().rf_physkeys_clear_values(self._h, _ptr(nd) if len(nd) else None, len(nd)))

    def update(self, nodes, flags, d_keys32, n_rows, listed=False, stream=None):
        """rf_physkeys_update; returns the PhysKeysOut, with .affected_nodes and
        .computable_bits (numpy) when listed."""
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        o = PhysKeysOut()
        o.size = ctypes.sizeof(PhysKeysOut)
        if listed:
            an, cb = np.zeros(max(self.n, 1), np.uint32), np.zeros(max(self.n, 1), np.uint8)
            o.cap, o.nodes, o.computable = self.n, _ptr(an), _ptr(cb)
        _check(lib().rf_physkeys_update(self._h, _ptr(nd) if len(nd) else None, len(nd), flags, d_keys32, n_rows,
                                        ctypes.byref(o), stream))
        if listed:
            o.affected_nodes, o.computable_bits = an[:o.affected], cb[:o.affected]
        return o

    def value_digests_device(self, nodes, d_out32, stream=None):
        nd = np.ascontiguousarray(nodes, dtype=np.uint32)
        _check(lib().rf_physkeys_value_digests_device(self._h, _ptr(nd) if len(nd) else None, len(nd), d_out32, stream))

    def value_digests(self, nodes) -> list:
        """Fileset.Digest() of the nodes' values on the host (a device buffer and a download; for tests)."""
        n = len(nodes)
        if not n:
            return []
        d = self.ctx.alloc(32 * n)
        try:
            self.value_digests_device(nodes, d.ptr)
            out = d.to_numpy(np.uint8, 32 * n)
        finally:
            d.free()
        return [out[32 * i:32 * i + 32].tobytes() for i in range(n)]

    def value_material(self, node) -> bytes:
        ln = ctypes.c_uint64()
        rc = lib().rf_physkeys_value_material(self._h, node, None, 0, ctypes.byref(ln))
        if rc != RF_OK and ln.value == 0:
            _check(rc)
        out = np.zeros(max(ln.value, 1), dtype=np.uint8)
        _check(lib().rf_physkeys_value_material(self._h, node, _ptr(out), ln.value, ctypes.byref(ln)))
        return out[:ln.value].tobytes()

    def stats(self) -> PhysKeysStats:
        st = PhysKeysStats()
        _check(lib().rf_physkeys_stats_get(self._h, ctypes.byref(st)))
        return st

    def close(self):
        if self._h:
            lib().rf_physkeys_close(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def physkeys_flat(dep_ptr, deps, phys_row, suffixes, nodes, n_rows, structure=None, sets=None, keys=None):
    """rf_physkeys_flat (host only): values as the dict of FilesetForest.copy()
    (structure) or as fileset objects (sets), value d belonging to nodes[d].
    Returns (keys [n_rows, 32] uint8 -- `keys` filled in where given --, the
    values' materials as a list of bytes)."""
    n, dp, de, pr, sp, sb = _phys_graph_args(dep_ptr, deps, phys_row, suffixes)
    nd = np.ascontiguousarray(nodes, dtype=np.uint32)
    nv = len(nd)
    fa, tree, roots, keep = None, None, None, None
    if structure is not None:
        o = structure
        assert len(o["doc_node_ptr"]) == nv + 1
        fa = ForestArrays(nv, _ptr(o["doc_node_ptr"]), _ptr(o["node_depth"]) if len(o["node_depth"]) else None,
                          _ptr(o["entry_ptr"]), _ptr(o["path_off"]), _ptr(o["paths"]) if len(o["paths"]) else None,
                          _ptr(o["ids32"]) if len(o["ids32"]) else None)
    elif nv:
        keep = FilesetTreeBuilder()
        roots = np.array([keep.add(fs) for fs in sets], dtype=np.uint32)
        tree = keep.struct()
    k = np.zeros((max(n_rows, 1), 32), dtype=np.uint8) if keys is None else keys
    offs = np.zeros(nv + 1, dtype=np.uint64)
    need = ctypes.c_uint64(0)

    def call(out, cap):
        return lib().rf_physkeys_flat(n, _ptr(dp) if n else None, _ptr(de) if len(de) else None,
                                      _ptr(pr) if n else None, _ptr(sp) if n else None, _ptr(sb),
                                      _ptr(nd) if nv else None, nv, ctypes.byref(fa) if fa is not None else None,
                                      ctypes.byref(tree) if tree is not None else None,
                                      _ptr(roots) if roots is not None and nv else None, _ptr(k), n_rows, out, cap,
                                      _ptr(offs), ctypes.byref(need))
    rc = call(None, 0)
    if rc != RF_OK and need.value == 0:
        _check(rc)
    out = np.zeros(max(need.value, 1), dtype=np.uint8)
    _check(call(_ptr(out), need.value))
    return k[:n_rows], [out[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(nv)]
