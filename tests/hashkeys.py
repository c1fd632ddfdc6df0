"""Host mirror of the tables' slot hash (reflow_amd/csrc/assoc_dev.h key_hash;
k9_repo.hip repo_row_hash with by_size; k8_live.hip live_hash) and its
inverse: keys built to hash to a chosen 32-bit value.  A helper, not a test.

key_hash xors four terms, one per pair of the key's eight little-endian words
(as the uint4 loads see them): (a ^ rotl(b, r)) * C with C odd, then a
finaliser h ^= h >> 16; h *= M; h ^= h >> 15.  Every step is a bijection of
32-bit words, so with seven words chosen freely the eighth follows from the
target: undo the finaliser, xor out the three other terms, multiply by C's
inverse, xor out rotl(b, r).

Keys of one full 32-bit hash share their home slot in every table, whatever its
mask; with the hash 0xFFFFFFFE the home is mask - 1 and every run longer than
two wraps round the table's end.

Everything is numpy over whole arrays: no Python loop per key."""
from __future__ import annotations

import numpy as np

PAIR_MUL = (0x9E3779B1, 0x85EBCA77, 0xC2B2AE3D, 0x27D4EB2F)  # pair p = words 2p, 2p + 1
PAIR_ROT = (5, 11, 17, 23)
FIN_MUL = 0x7FEB352D
ORD_MUL, SIZE_LO_MUL, SIZE_HI_MUL = PAIR_MUL[0], PAIR_MUL[1], PAIR_MUL[2]  # the row hash's three terms
WRAP_HASH = 0xFFFFFFFE  # home slot mask - 1

_U32 = np.uint32
_M32 = 0xFFFFFFFF


def _u32(x) -> np.ndarray:
    """An integer or integer array as uint32, modulo 2^32."""
    return (np.asarray(x).astype(np.uint64) & np.uint64(_M32)).astype(_U32)


def _mul(a, c: int) -> np.ndarray:
    return ((a.astype(np.uint64) * np.uint64(c)) & np.uint64(_M32)).astype(_U32)


def _rotl(a, r: int) -> np.ndarray:
    return (a << _U32(r)) | (a >> _U32(32 - r))


def _inv(c: int) -> int:
    return pow(c, -1, 1 << 32)


def fin(h) -> np.ndarray:
    h = _u32(h).copy()
    h ^= h >> _U32(16)
    h = _mul(h, FIN_MUL)
    h ^= h >> _U32(15)
    return h


def unfin(h) -> np.ndarray:
    """fin's inverse."""
    h = _u32(h).copy()
    h = h ^ (h >> _U32(15)) ^ (h >> _U32(30))
    h = _mul(h, _inv(FIN_MUL))
    h ^= h >> _U32(16)
    return h


def words(keys) -> np.ndarray:
    """[n, 8] uint32: the eight little-endian words of each 32-byte key."""
    k = np.ascontiguousarray(keys, dtype=np.uint8).reshape(-1, 32)
    return k.view("<u4").astype(_U32)


def _pair_term(w, p: int) -> np.ndarray:
    return _mul(w[:, 2 * p] ^ _rotl(w[:, 2 * p + 1], PAIR_ROT[p]), PAIR_MUL[p])


def _pre(w) -> np.ndarray:
    return _pair_term(w, 0) ^ _pair_term(w, 1) ^ _pair_term(w, 2) ^ _pair_term(w, 3)


def key_hash(keys) -> np.ndarray:
    """assoc_dev.h key_hash of each 32-byte key: uint32 [n]."""
    return fin(_pre(words(keys)))


def _size_terms(sizes) -> np.ndarray:
    s = np.asarray(sizes, dtype=np.int64).view(np.uint64)
    return _mul((s & np.uint64(_M32)).astype(_U32), SIZE_LO_MUL) ^ _mul((s >> np.uint64(32)).astype(_U32), SIZE_HI_MUL)


def row_hash(ords, keys, sizes) -> np.ndarray:
    """repo_row_hash(by_size) / live_hash of the rows (ord_i, key_i, size_i): uint32 [n]."""
    h = key_hash(keys)
    n = len(h)
    o = np.broadcast_to(_u32(ords), (n,))
    s = np.broadcast_to(np.asarray(sizes, dtype=np.int64), (n,))
    return fin(h ^ _mul(o, ORD_MUL) ^ _size_terms(s))


def keys_with_hash(rng, h, n: int, pair: int = 3) -> np.ndarray:
    """n distinct 32-byte keys [n, 32] with key_hash == h (one value, or one
    per key).  Seven words are random (one of them carries a counter, which
    makes the keys distinct by construction); the first word of `pair` is
    solved for."""
    assert 0 <= pair < 4
    w = rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(_U32)
    free = 2 * ((pair + 1) % 4)  # a word the solve does not touch
    w[:, free] = (np.arange(n, dtype=np.uint64) + np.uint64(int(rng.integers(0, 1 << 32)))).astype(_U32)
    target = unfin(np.broadcast_to(_u32(h), (n,)))
    for p in range(4):
        if p != pair:
            target = target ^ _pair_term(w, p)
    w[:, 2 * pair] = _mul(target, _inv(PAIR_MUL[pair])) ^ _rotl(w[:, 2 * pair + 1], PAIR_ROT[pair])
    return np.ascontiguousarray(w.astype("<u4")).view(np.uint8).reshape(n, 32)


def rows_with_hash(rng, h, ords, sizes, pair: int = 3) -> np.ndarray:
    """IDs [n, 32], distinct, with row_hash(ords_i, id_i, sizes_i) == h: the
    second finaliser undone, the ord and size terms xored out, key_hash inverted."""
    s = np.atleast_1d(np.asarray(sizes, dtype=np.int64))
    n = len(s)
    o = np.broadcast_to(_u32(ords), (n,))
    return keys_with_hash(rng, unfin(np.broadcast_to(_u32(h), (n,))) ^ _mul(o, ORD_MUL) ^ _size_terms(s), n, pair)


def size_twin(size: int, max_hi: int = 1 << 16) -> int:
    """Another non-negative size whose two row-hash terms xor to the same word
    as `size`'s: (ord, ID, size) and (ord, ID, twin) share their row hash.  The
    low word is searched so that the high word stays below max_hi (sums of
    such sizes stay far from 2^63)."""
    want = _size_terms(np.array([size], np.int64))[0]
    lo = np.arange(1, 1 << 22, dtype=np.uint64).astype(_U32)
    hi = _mul(_mul(lo, SIZE_LO_MUL) ^ want, _inv(SIZE_HI_MUL))
    ok = np.flatnonzero(hi < max_hi)
    for j in ok.tolist():
        t = (int(hi[j]) << 32) | int(lo[j])
        if t != int(size):
            return t
    raise AssertionError("no twin below max_hi")


def hash_for_two_ords(ord_a: int, ord_b: int, low: int, bits: int = 12) -> tuple[int, int]:
    """(h_a, h_b): row hashes whose low `bits` bits are both `low`, such that a
    row (ord_a, ID, size) of hash h_a has the hash h_b under ord_b.  The ord
    term is a bijection, so one (ID, size) never has ONE hash under two ords;
    this is the closest there is: one home slot in every table of up to
    2^bits slots.  The search is over all 2^(32 - bits) hashes with these low
    bits; for some pairs of ords it finds none (with low 0xFFE: (0, 1) and
    (1, 2), while (2, 3), (2, 5) and (3, 5) have one): ValueError then."""
    cand = ((np.arange(1 << (32 - bits), dtype=np.uint64) << np.uint64(bits)) | np.uint64(low)).astype(_U32)
    d = (ord_a * ORD_MUL ^ ord_b * ORD_MUL) & _M32
    other = fin(unfin(cand) ^ _U32(d))
    ok = np.flatnonzero((other & _U32((1 << bits) - 1)) == _U32(low))
    if not len(ok):
        raise ValueError("no hash with these low bits under both ords")
    return int(cand[ok[0]]), int(other[ok[0]])
