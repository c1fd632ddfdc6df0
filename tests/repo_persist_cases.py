"""Helpers for the repository index's listing and persistence tests
(test_repo_file.py, test_gpu_repo_persist.py).  A helper, not a test.

  write_file: the index file written in Python alone (struct + hashlib) from
  the layout include/reflow_hip.h states, little-endian:
    header 64 B   magic "RFREPO01", u32 version = 1, u32 flags = 0, u64
                  n_entries, u64 chunk, i64 total_bytes (the sum of the
                  sizes), 24 zero bytes
    entries 40 B  32-B ID, i64 size >= 0, strictly ascending by ID bytes
    one SHA-256 per `chunk` bytes of the entry area (the last may be short)
    SHA-256(header || those digests), the end marker "RFREEND1"
  Every field can be overridden, so that files which break one rule and keep
  every checksum valid can be written too.

  Twin / scan helpers: a device index beside tests/repo_model.py's object map,
  with the model's side of compact, collect_list and restore."""
from __future__ import annotations

import hashlib
import struct

import numpy as np

import repo_model as M
from reflow_amd import capi

HEADER, ENTRY, TRAILER = 64, 40, 40
DEFAULT_CHUNK = 64 << 20
MAGIC, END = b"RFREPO01", b"RFREEND1"
POISON = 0xAB
_M64 = (1 << 64) - 1

# the golden fixture tests/golden/repo_v1.bin: 5 entries, chunk 80
GOLDEN_IDS = [bytes([0x00] * 31 + [0x01]),
              bytes([0x00] * 31 + [0x02]),
              bytes([0x10] + list(range(1, 32))),
              bytes([0x7f] * 32),
              bytes([0xff] * 31 + [0xfe])]
GOLDEN_SIZES = [0, 1, 4096, (1 << 40) + 5, (1 << 62) - 1]
GOLDEN_CHUNK = 80


def header(n, chunk, total, magic=MAGIC, version=1, flags=0, reserved=bytes(24)):
    return magic + struct.pack("<IIQQ", version, flags, n & _M64, chunk & _M64) + struct.pack("<Q", total & _M64) + reserved


def write_file(ids, sizes, chunk=0, n_entries=None, total=None, header_chunk=None, end=END, **hdr) -> bytes:
    """The file of the entries as given (no sorting, no checks).  chunk 0: the
    default granule, as rf_repo_file_format reads it.  n_entries / total /
    header_chunk: what the header says instead of the truth (the sum taken
    modulo 2^64)."""
    chunk = chunk or DEFAULT_CHUNK
    area = b"".join(bytes(i) + struct.pack("<Q", int(s) & _M64) for i, s in zip(ids, sizes))
    digests = b"".join(hashlib.sha256(area[o:o + chunk]).digest() for o in range(0, len(area), chunk))
    h = header(len(sizes) if n_entries is None else n_entries, chunk if header_chunk is None else header_chunk,
               sum(int(s) for s in sizes) if total is None else total, **hdr)
    return h + area + digests + hashlib.sha256(h + digests).digest() + end


def objects(rng, n, max_size=1 << 20):
    """n random (ID, size) pairs: bytes [n], ints [n]."""
    ids = [rng.bytes(32) for _ in range(n)]
    return ids, [int(s) for s in rng.integers(0, max_size, size=n)]


def sorted_arrays(objs: dict):
    """(ids uint8 [n, 32], sizes int64 [n]) of an ID -> size map in ID order: the file's order."""
    ids = sorted(objs)
    return (M.ids_array(ids) if ids else np.zeros((0, 32), np.uint8)), np.array([objs[i] for i in ids], np.int64)


# ---- the model's side of the new calls ---------------------------------------------
def model_compact(ref: M.Repo, min_capacity=0):
    ref.slots = M.slots_for(max(len(ref.objs), min_capacity))
    ref.tombs.clear()
    ref.rebuilds += 1


def model_dead(ref: M.Repo, contains=None) -> dict:
    """What a collect with this liveset removes: ID -> size (nothing is removed here)."""
    return {i: s for i, s in ref.objs.items() if contains is None or not contains(i)}


def model_restored(objs: dict) -> M.Repo:
    ref = M.Repo(len(objs))
    ref.objs = dict(objs)
    return ref


def check_stats(repo, model):
    st, want = repo.stats(), model.stats()
    assert {k: getattr(st, k) for k in want} == want


# ---- scans -------------------------------------------------------------------------
def as_dict(ids, sizes):
    """ID -> size of listed rows; every ID once."""
    keys = [bytes(r) for r in np.asarray(ids).reshape(-1, 32)]
    assert len(set(keys)) == len(keys), "an ID is listed twice"
    return dict(zip(keys, (int(s) for s in sizes)))


class DevList:
    """Device arrays of `cap` rows for a list and a u64 (and an i64) beside them, all poisoned."""

    def __init__(self, ctx, cap, ids=True, sizes=True):
        self.cap = cap
        self.ids = ctx.alloc(32 * max(cap, 1)) if ids else None
        self.sizes = ctx.alloc(8 * max(cap, 1)) if sizes else None
        self.n, self.nbytes = ctx.alloc(8), ctx.alloc(8)
        for b in self.bufs():
            b.fill(POISON)

    def bufs(self):
        return [b for b in (self.ids, self.sizes, self.n, self.nbytes) if b is not None]

    def read(self):
        """(ids [cap, 32] or None, sizes [cap] or None, n, bytes); then freed."""
        out = (self.ids.to_numpy(np.uint8)[:32 * self.cap].reshape(-1, 32) if self.ids else None,
               self.sizes.to_numpy(np.int64)[:self.cap] if self.sizes else None,
               int(self.n.to_numpy(np.uint64)[0]), int(self.nbytes.to_numpy(np.int64)[0]))
        for b in self.bufs():
            b.free()
        return out


def scan_device(ctx, repo, cap, ids=True, sizes=True):
    d = DevList(ctx, cap, ids, sizes)
    repo.scan_device(cap, d.ids.ptr if ids else None, d.sizes.ptr if sizes else None, d.n.ptr)
    ctx.sync()
    return d.read()[:3]


def scan_checked(ctx, repo, model: M.Repo):
    """The scan in both forms against the model: the set, every ID once, sizes,
    n == stats.objects, host == device byte for byte, two scans equal.  The
    scanned (ids, sizes)."""
    ids, sizes, n, _ = repo.scan()
    assert n == len(model.objs) == repo.stats().objects == len(sizes) == len(ids)
    assert as_dict(ids, sizes) == model.objs
    d_ids, d_sizes, d_n = scan_device(ctx, repo, n)
    assert d_n == n and d_ids.tobytes() == ids.tobytes() and d_sizes.tobytes() == sizes.tobytes()
    ids2, sizes2, n2, _ = repo.scan()
    assert n2 == n and ids2.tobytes() == ids.tobytes() and sizes2.tobytes() == sizes.tobytes()
    return ids, sizes


def is_subsequence(rows, of_rows):
    it = iter(of_rows)
    return all(any(r == o for o in it) for r in rows)


class Twin:
    """A device index and its model, written together (statuses compared)."""

    def __init__(self, ctx, capacity=0):
        self.ctx, self.dev, self.ref = ctx, capi.Repo(ctx, capacity), M.Repo(capacity)

    def put(self, ids, sizes):
        want = self.ref.put(ids, sizes)
        got = self.dev.put(M.ids_array(ids) if len(ids) else np.zeros((0, 32), np.uint8), sizes)
        assert got.tolist() == want.tolist()

    def remove(self, ids):
        want = self.ref.remove(ids)
        assert self.dev.remove(M.ids_array(ids)).tolist() == want.tolist()

    def stat(self, ids):
        assert self.dev.stat(M.ids_array(ids)).tolist() == self.ref.stat(ids).tolist()

    def scan(self):
        out = scan_checked(self.ctx, self.dev, self.ref)
        check_stats(self.dev, self.ref)
        return out

    def compact(self, min_capacity=0):
        self.dev.compact(min_capacity)
        model_compact(self.ref, min_capacity)

    def close(self):
        self.dev.close()


class Flow:
    """A liveset over OFlow nodes with their values set (host form)."""

    def __init__(self, ctx, nodes):
        import live_model as LM  # (needs the oracle: kept out of the file-form tests' imports)
        self.edge_ptr, self.edges = LM.live_csr(nodes)
        self.L = capi.GcLiveset(ctx, self.edge_ptr, self.edges)
        nd, ct, ids, sz = LM.value_arrays(nodes, list(range(len(nodes))))
        if len(nd):
            self.L.set_values(nd, ct, ids, sz)

    def close(self):
        self.L.close()
