"""tests/hashkeys.py on the CPU: the vectorised mirror against a scalar
restatement of assoc_dev.h key_hash / repo_row_hash / live_hash written out
word by word, and the inverse: crafted keys hash to their target, whichever
word pair is solved for, and are distinct -- 65537 of them included.  (That
the mirror is the device's hash is test_gpu_probe_runs.py's first test.)"""
import struct
import time

import numpy as np
import pytest

import hashkeys as HK

TARGETS = [0, 1, 0xFFFFFFFE, 0xFFFFFFFF, 12345]
M32 = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _fin(h):
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    return h


def scalar_key_hash(key: bytes) -> int:
    lx, ly, lz, lw, hx, hy, hz, hw = struct.unpack("<8I", key)
    h = ((((lx ^ _rotl(ly, 5)) * 0x9E3779B1) & M32) ^ (((lz ^ _rotl(lw, 11)) * 0x85EBCA77) & M32) ^
         (((hx ^ _rotl(hy, 17)) * 0xC2B2AE3D) & M32) ^ (((hz ^ _rotl(hw, 23)) * 0x27D4EB2F) & M32))
    return _fin(h)


def scalar_row_hash(ord_: int, key: bytes, size: int) -> int:
    h = scalar_key_hash(key)
    u = size & 0xFFFFFFFFFFFFFFFF
    h ^= (ord_ * 0x9E3779B1) & M32
    h ^= ((u & M32) * 0x85EBCA77) & M32
    h ^= ((u >> 32) * 0xC2B2AE3D) & M32
    return _fin(h)


def test_mirror_equals_the_scalar_restatement():
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 256, size=(300, 32), dtype=np.uint8)
    keys[0] = 0
    keys[1] = 0xFF
    for w in range(8):  # one word set, the others zero: every word's rotate and constant on its own
        keys[2 + w] = 0
        keys[2 + w, 4 * w:4 * w + 4] = (0x01, 0x23, 0x45, 0x87)
    assert HK.key_hash(keys).tolist() == [scalar_key_hash(k.tobytes()) for k in keys]
    ords = rng.integers(0, 1 << 32, size=300, dtype=np.uint64)
    sizes = rng.integers(-(1 << 62), 1 << 62, size=300, dtype=np.int64)
    sizes[:4] = (0, 1, 1 << 32, -1)
    want = [scalar_row_hash(int(o), k.tobytes(), int(s)) for o, k, s in zip(ords, keys, sizes)]
    assert HK.row_hash(ords, keys, sizes).tolist() == want
    assert HK.row_hash(5, keys, 9).tolist() == [scalar_row_hash(5, k.tobytes(), 9) for k in keys]  # broadcast


def test_the_finaliser_inverts():
    rng = np.random.default_rng(2)
    h = np.concatenate([np.array(TARGETS, np.uint32), rng.integers(0, 1 << 32, size=5000, dtype=np.uint64).astype(np.uint32)])
    assert (HK.fin(HK.unfin(h)) == h).all() and (HK.unfin(HK.fin(h)) == h).all()
    assert HK.fin(h[:50]).tolist() == [_fin(int(x)) for x in h[:50]]


@pytest.mark.parametrize("pair", range(4))
@pytest.mark.parametrize("target", TARGETS)
def test_crafted_keys_hash_to_their_target(target, pair):
    rng = np.random.default_rng(target % 1000 + pair)
    keys = HK.keys_with_hash(rng, target, 1000, pair=pair)
    assert keys.shape == (1000, 32) and keys.dtype == np.uint8
    assert (HK.key_hash(keys) == target).all()
    assert [scalar_key_hash(k.tobytes()) for k in keys[:100]] == [target] * 100
    assert len({k.tobytes() for k in keys}) == 1000


def test_a_target_per_key():
    rng = np.random.default_rng(3)
    t = rng.integers(0, 1 << 32, size=500, dtype=np.uint64).astype(np.uint32)
    keys = HK.keys_with_hash(rng, t, 500)
    assert (HK.key_hash(keys) == t).all()


def test_65537_distinct_keys_quickly():
    rng = np.random.default_rng(4)
    HK.keys_with_hash(rng, 1, 16)  # (first-call costs stay out of the timing)
    t0 = time.perf_counter()
    keys = HK.keys_with_hash(rng, HK.WRAP_HASH, 65537)
    dt = time.perf_counter() - t0
    assert (HK.key_hash(keys) == HK.WRAP_HASH).all()
    assert len(np.unique(keys.view("S32"))) == 65537
    assert dt < 0.5, dt


@pytest.mark.parametrize("pair", range(4))
def test_crafted_rows_hash_to_their_target(pair):
    rng = np.random.default_rng(5 + pair)
    n = 2000
    ords = rng.integers(0, 5, size=n).astype(np.uint32)
    sizes = rng.integers(0, 1 << 40, size=n, dtype=np.int64)
    for target in TARGETS:
        ids = HK.rows_with_hash(rng, target, ords, sizes, pair=pair)
        assert (HK.row_hash(ords, ids, sizes) == target).all()
        assert len(np.unique(ids.view("S32"))) == n
        assert [scalar_row_hash(int(o), k.tobytes(), int(s)) for o, k, s in zip(ords[:50], ids[:50], sizes[:50])] \
            == [target] * 50
    ids = HK.rows_with_hash(rng, HK.WRAP_HASH, 0, np.arange(65537, dtype=np.int64))  # one ord for all
    assert (HK.row_hash(0, ids, np.arange(65537)) == HK.WRAP_HASH).all()
    assert len(np.unique(ids.view("S32"))) == 65537


def test_size_twins_and_the_two_ord_hash():
    for size in (0, 1, 77, 123456789, (5 << 32) | 9):
        t = HK.size_twin(size)
        assert t != size and 0 <= t < 1 << 48
        k = np.zeros((1, 32), np.uint8)
        assert HK.row_hash(3, k, size).tolist() == HK.row_hash(3, k, t).tolist()
        assert scalar_row_hash(3, bytes(32), size) == scalar_row_hash(3, bytes(32), t)
    rng = np.random.default_rng(6)
    for a, b in ((2, 3), (2, 5), (3, 5)):  # (the groups test_gpu_probe_runs.py uses)
        ha, hb = HK.hash_for_two_ords(a, b, 0xFFE)
        assert ha & 0xFFF == hb & 0xFFF == 0xFFE and ha != hb
        ids = HK.rows_with_hash(rng, ha, a, np.full(20, 11, np.int64))
        assert (HK.row_hash(a, ids, 11) == ha).all() and (HK.row_hash(b, ids, 11) == hb).all()
    with pytest.raises(ValueError):
        HK.hash_for_two_ords(0, 1, 0xFFE)
