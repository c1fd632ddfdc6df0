"""The HBM assoc's file form on the host alone (rf_assoc_file_format /
rf_assoc_file_parse, reflow_amd/csrc/assoc_io.cpp; no GPU): the layout is
pinned against a builder written here from its description (struct + hashlib)

    header, 64 B   "RFASSOC1", u32 version = 1, u32 flags = 0, u64 n_entries,
                   u64 chunk, 32 zero bytes
    entries, 68 B  u32 kind, 32-B key, 32-B value; strictly ascending by
                   (kind, key bytes)
    chunk digests  one SHA-256 per `chunk` bytes of the entry area
    trailer        SHA-256(header || chunk digests), "RFASEND1"

the committed version-1 fixture still parses, short buffers are refused with
the size they need, and every malformed input is refused with its code:
RF_EINVAL for a file that is not one or whose entries break the rules,
RF_EINTEGRITY for a checksum mismatch."""
import ctypes
import hashlib
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "assoc_v1.bin")
DEFAULT_CHUNK = 64 << 20


def sha(b):
    return hashlib.sha256(b).digest()


def build_file(entries, chunk, version=1, flags=0, n_entries=None, magic=b"RFASSOC1", end=b"RFASEND1",
               header_chunk=None):
    """The file of entries [(kind, key32, val32)] in the order given."""
    n = len(entries) if n_entries is None else n_entries
    header = struct.pack("<8sIIQQ32x", magic, version, flags, n, chunk if header_chunk is None else header_chunk)
    assert len(header) == 64
    area = b"".join(struct.pack("<I", k & 0xffffffff) + key + val for k, key, val in entries)
    digests = b"".join(sha(area[o:o + chunk]) for o in range(0, len(area), chunk))
    return header + area + digests + sha(header + digests) + end


def fixture_entries():
    """The five entries of tests/golden/assoc_v1.bin: three of kind 0, two of kind 1."""
    es = [(0 if i < 3 else 1, sha(b"assoc-v1-key-%d" % i), sha(b"assoc-v1-val-%d" % i)) for i in range(5)]
    return sorted(es, key=lambda e: (e[0], e[1]))


def some_entries(n, seed=3):
    rng = np.random.default_rng(seed)
    es = [(int(rng.integers(0, 3)), rng.integers(0, 256, 32, dtype=np.uint8).tobytes(),
           rng.integers(1, 256, 32, dtype=np.uint8).tobytes()) for _ in range(n)]
    return sorted(es, key=lambda e: (e[0], e[1]))


def arrays(entries):
    kinds = np.array([e[0] for e in entries], dtype=np.int32)
    keys = np.frombuffer(b"".join(e[1] for e in entries), dtype=np.uint8)
    vals = np.frombuffer(b"".join(e[2] for e in entries), dtype=np.uint8)
    return kinds, keys, vals


def parse_rc(buf):
    """(rc, n) of rf_assoc_file_parse over a buffer of exactly len(buf) bytes."""
    from reflow_amd import capi
    b = np.frombuffer(bytes(buf), dtype=np.uint8).copy()
    n = ctypes.c_uint64(0)
    cap = 64
    kinds = np.zeros(cap, dtype=np.int32)
    keys = np.zeros(32 * cap, dtype=np.uint8)
    vals = np.zeros(32 * cap, dtype=np.uint8)
    rc = capi.lib().rf_assoc_file_parse(b.ctypes.data if len(b) else None, len(b), kinds.ctypes.data,
                                        keys.ctypes.data, vals.ctypes.data, cap, ctypes.byref(n))
    return rc, n.value


def as_entries(parsed):
    kinds, keys, vals = parsed
    return [(int(k), keys[i].tobytes(), vals[i].tobytes()) for i, k in enumerate(kinds)]


@pytest.mark.parametrize("chunk", [0, 100, 68 * 3])
@pytest.mark.parametrize("n", [0, 1, 7])
def test_layout_is_pinned(n, chunk):
    """Chunk edges mid-entry (100) and on an entry boundary (68 * 3); 0 = 64 MiB."""
    from reflow_amd import capi
    es = some_entries(n)
    got = capi.assoc_file_format(*arrays(es), chunk=chunk)
    want = build_file(es, chunk or DEFAULT_CHUNK)
    assert got == want
    assert len(got) == 64 + 68 * n + 32 * -(-68 * n // (chunk or DEFAULT_CHUNK)) + 40


def test_committed_fixture_parses():
    """A version-1 file written when the format was introduced: a later
    format change must keep reading it."""
    from reflow_amd import capi
    data = open(FIXTURE, "rb").read()
    assert len(data) < 1024
    es = fixture_entries()
    assert len(es) == 5 and {e[0] for e in es} == {0, 1}
    assert as_entries(capi.assoc_file_parse(data)) == es
    assert data == build_file(es, DEFAULT_CHUNK)
    assert capi.assoc_file_format(*arrays(es)) == data


@pytest.mark.parametrize("chunk", [0, 1, 67, 100, 68 * 3, 1 << 40])
def test_round_trip(chunk):
    from reflow_amd import capi
    es = some_entries(40, seed=chunk % 97)
    assert as_entries(capi.assoc_file_parse(capi.assoc_file_format(*arrays(es), chunk=chunk))) == es


def test_short_buffers_report_the_size_and_write_nothing():
    from reflow_amd import capi
    L = capi.lib()
    es = some_entries(5)
    kinds, keys, vals = arrays(es)
    want = build_file(es, 100)
    need = ctypes.c_uint64(0)
    for cap in (0, 1, len(want) - 1):
        out = np.full(cap + 64, 0xA5, dtype=np.uint8)
        rc = L.rf_assoc_file_format(kinds.ctypes.data, keys.ctypes.data, vals.ctypes.data, 5, 100, out.ctypes.data,
                                    cap, ctypes.byref(need))
        assert rc == capi.RF_EINVAL and need.value == len(want)
        assert (out == 0xA5).all()
    out = np.full(len(want) + 64, 0xA5, dtype=np.uint8)
    rc = L.rf_assoc_file_format(kinds.ctypes.data, keys.ctypes.data, vals.ctypes.data, 5, 100, out.ctypes.data,
                                len(want), ctypes.byref(need))
    assert rc == capi.RF_OK and out[:len(want)].tobytes() == want and (out[len(want):] == 0xA5).all()
    buf = np.frombuffer(want, dtype=np.uint8)
    n = ctypes.c_uint64(0)
    for cap in (0, 4):
        k = np.full(cap + 64, -1, dtype=np.int32)
        ky = np.full(32 * (cap + 64), 0xA5, dtype=np.uint8)
        vl = np.full(32 * (cap + 64), 0xA5, dtype=np.uint8)
        rc = L.rf_assoc_file_parse(buf.ctypes.data, len(buf), k.ctypes.data, ky.ctypes.data, vl.ctypes.data, cap,
                                   ctypes.byref(n))
        assert rc == capi.RF_EINVAL and n.value == 5
        assert (k == -1).all() and (ky == 0xA5).all() and (vl == 0xA5).all()
    k = np.full(5 + 64, -1, dtype=np.int32)
    ky = np.full(32 * (5 + 64), 0xA5, dtype=np.uint8)
    vl = np.full(32 * (5 + 64), 0xA5, dtype=np.uint8)
    rc = L.rf_assoc_file_parse(buf.ctypes.data, len(buf), k.ctypes.data, ky.ctypes.data, vl.ctypes.data, 5,
                               ctypes.byref(n))
    assert rc == capi.RF_OK and n.value == 5
    assert (k[5:] == -1).all() and (ky[32 * 5:] == 0xA5).all() and (vl[32 * 5:] == 0xA5).all()
    assert k[:5].tolist() == [e[0] for e in es]


@pytest.mark.parametrize("chunk", [100, 68 * 3, DEFAULT_CHUNK])
def test_every_truncation_is_invalid(chunk):
    from reflow_amd import capi
    data = build_file(some_entries(3), chunk)
    assert parse_rc(data) == (capi.RF_OK, 3)
    for length in range(len(data)):
        assert parse_rc(data[:length])[0] == capi.RF_EINVAL, length
    assert parse_rc(data + b"\0")[0] == capi.RF_EINVAL


def test_flipped_entry_bit_is_an_integrity_error():
    from reflow_amd import capi
    data = build_file(some_entries(3), 100)
    for byte in (64, 64 + 3, 64 + 4, 64 + 67, 64 + 68 + 36, 64 + 3 * 68 - 1):
        for bit in (0, 7):
            bad = bytearray(data)
            bad[byte] ^= 1 << bit
            assert parse_rc(bad)[0] == capi.RF_EINTEGRITY, (byte, bit)
    # the checksum list and the root are covered too
    for byte in (64 + 3 * 68, 64 + 3 * 68 + 32 * 3, len(data) - 9):
        bad = bytearray(data)
        bad[byte] ^= 1
        assert parse_rc(bad)[0] == capi.RF_EINTEGRITY, byte


def test_bad_header_fields_are_invalid():
    from reflow_amd import capi
    es = some_entries(3)
    for kw in (dict(magic=b"RFASSOC2"), dict(magic=b"RFGRAPH1"), dict(version=0), dict(version=2), dict(flags=1),
               dict(end=b"RFASEND2"), dict(n_entries=4), dict(n_entries=1 << 40), dict(n_entries=(1 << 64) - 1),
               dict(header_chunk=0), dict(header_chunk=1), dict(header_chunk=(1 << 64) - 1)):
        rc, _ = parse_rc(build_file(es, 100, **kw))
        assert rc == capi.RF_EINVAL, kw
        assert len(capi.lib().rf_last_error()) > 0
    assert parse_rc(b"")[0] == capi.RF_EINVAL


def test_entry_rules_with_valid_checksums():
    """Files whose checksums are right (recomputed here) but whose entries
    break a rule: a zero value, an unsorted pair, a duplicate (kind, key), a
    negative kind."""
    from reflow_amd import capi
    es = some_entries(4)
    assert parse_rc(build_file(es, 100))[0] == capi.RF_OK
    zero = list(es)
    zero[2] = (zero[2][0], zero[2][1], bytes(32))
    unsorted = [es[1], es[0], es[2], es[3]]
    same_kind = [(0, bytes([9]) * 32, b"\1" * 32), (0, bytes([8]) * 32, b"\1" * 32)]
    dup = [es[0], es[1], es[1], es[3]]
    negative = [(-1, es[0][1], es[0][2])]
    high_bit = [(0x80000000, es[0][1], es[0][2])]
    too_big = [(1 << 30, es[0][1], es[0][2])]
    for name, bad in [("zero value", zero), ("unsorted", unsorted), ("unsorted keys of one kind", same_kind),
                      ("duplicate", dup), ("negative kind", negative), ("kind bit 31", high_bit),
                      ("kind 2^30", too_big)]:
        assert parse_rc(build_file(bad, 100))[0] == capi.RF_EINVAL, name
    assert parse_rc(build_file([((1 << 30) - 1, es[0][1], es[0][2])], 100))[0] == capi.RF_OK
    # format refuses to write what parse would refuse
    with pytest.raises(capi.RfError) as ei:
        capi.assoc_file_format(*arrays(unsorted), chunk=100)
    assert ei.value.code == capi.RF_EINVAL


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_assoc_file_code_under_asan_ubsan():
    """tests/cpp/asan_assoc_file: assoc_io.cpp and the HIP-free units it needs
    under AddressSanitizer + UndefinedBehaviorSanitizer, over the same
    truncations and corruptions (every buffer exactly as long as `len`).
    Built and run directly; nothing is preloaded."""
    b = subprocess.run(["make", "-C", CSRC, "asan_assoc"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_assoc_file")], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip() == "PASS"
