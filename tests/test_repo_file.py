"""The repository index's file form on the host alone (rf_repo_file_format /
rf_repo_file_parse, reflow_amd/csrc/repo_io.cpp): no device.  The layout is
pinned by a writer in Python (tests/repo_persist_cases.py write_file: struct
and hashlib, from the header's text); then round trips, short buffers, every
truncation, flipped bits field by field, rule violations under valid
checksums, the committed fixture tests/golden/repo_v1.bin, and the same walk
under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone program."""
import ctypes
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import repo_model as M
import repo_persist_cases as C
from reflow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
FIXTURE = os.path.join(ROOT, "tests", "golden", "repo_v1.bin")


def entries(n):
    """n entries ascending by ID, sizes with zero, small and > 2^32 values."""
    ids = [bytes([i]) + bytes((7 * i + b) & 0xff for b in range(1, 32)) for i in range(n)]
    sizes = [(i * 0x100000001) % 0x7fffffffff if i % 3 else i for i in range(n)]
    return ids, sizes


def arrays(ids, sizes):
    return (M.ids_array(ids) if ids else np.zeros((0, 32), np.uint8)), np.array(sizes, np.int64)


def status(buf, cap_entries=None):
    """rf_repo_file_parse's status for these bytes (RF_OK: the entries came back too)."""
    try:
        capi.repo_file_parse(buf, cap_entries)
        return capi.RF_OK
    except capi.RfError as e:
        return e.code


SEVEN = entries(7)
FILE7 = C.write_file(*SEVEN, chunk=80)  # 64 + 280 + 4 * 32 + 40


# ---- 1. the layout ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7])
@pytest.mark.parametrize("chunk", [80, 100, 40 * 7, 0])
def test_layout_is_pinned(n, chunk):
    """chunk 80: two entries; 100: not a multiple of an entry, a ragged last
    chunk; 280: exactly one chunk at n = 7; 0: the default, 64 MiB."""
    ids, sizes = entries(n)
    want = C.write_file(ids, sizes, chunk)
    nc = -(-40 * n // (chunk or C.DEFAULT_CHUNK))
    assert len(want) == 64 + 40 * n + 32 * nc + 40
    assert capi.repo_file_format(*arrays(ids, sizes), chunk=chunk) == want


def test_header_fields_where_the_text_puts_them():
    f = FILE7
    assert f[:8] == b"RFREPO01" and f[-8:] == b"RFREEND1"
    assert struct.unpack_from("<IIQQq", f, 8) == (1, 0, 7, 80, sum(SEVEN[1])) and f[40:64] == bytes(24)
    assert f[64:96] == SEVEN[0][0] and struct.unpack_from("<q", f, 96)[0] == SEVEN[1][0]


# ---- 2. round trips and short buffers --------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 7])
@pytest.mark.parametrize("chunk", [80, 100, 40 * 7, 0])
def test_round_trip(n, chunk):
    ids, sizes = arrays(*entries(n))
    got_ids, got_sizes = capi.repo_file_parse(capi.repo_file_format(ids, sizes, chunk=chunk))
    assert got_ids.tobytes() == ids.tobytes() and got_sizes.tolist() == sizes.tolist()


def test_short_buffers_report_what_is_needed():
    ids, sizes = arrays(*SEVEN)
    for cap in (0, 1, len(FILE7) - 1):
        with pytest.raises(capi.RfError) as ei:
            capi.repo_file_format(ids, sizes, chunk=80, cap=cap)
        assert ei.value.code == capi.RF_EINVAL and ei.value.needed == len(FILE7)
    assert capi.repo_file_format(ids, sizes, chunk=80, cap=len(FILE7) + 9) == FILE7
    for cap in (0, 1, 6):
        with pytest.raises(capi.RfError) as ei:
            capi.repo_file_parse(FILE7, cap_entries=cap)
        assert ei.value.code == capi.RF_EINVAL and ei.value.needed == 7
    assert len(capi.repo_file_parse(FILE7, cap_entries=8)[1]) == 7
    # a short entry buffer is not written: the rows keep their sentinel (the raw call)
    got_ids, got_sizes, n = np.full((6, 32), 0xAB, np.uint8), np.full(6, -77, np.int64), ctypes.c_uint64()
    buf = np.frombuffer(FILE7, np.uint8)
    rc = capi.lib().rf_repo_file_parse(buf.ctypes.data, len(buf), got_ids.ctypes.data, got_sizes.ctypes.data, 6,
                                       ctypes.byref(n))
    assert rc == capi.RF_EINVAL and n.value == 7 and (got_ids == 0xAB).all() and (got_sizes == -77).all()


# ---- 3. damage ----------------------------------------------------------------------------
def test_every_truncation_and_a_trailing_byte_are_invalid():
    assert status(FILE7) == capi.RF_OK
    for cut in range(len(FILE7)):
        assert status(FILE7[:cut]) == capi.RF_EINVAL, cut
    assert status(FILE7 + b"\0") == capi.RF_EINVAL


def flipped(f, byte, bit):
    g = bytearray(f)
    g[byte] ^= 1 << bit
    return bytes(g)


def test_a_flipped_bit_in_entries_or_digests_is_an_integrity_error():
    area, digests = range(64, 64 + 280), range(64 + 280, 64 + 280 + 4 * 32 + 32)  # (chunk digests and the root)
    for byte in list(area)[::3] + [area[-1]] + list(digests)[::5] + [digests[-1]]:
        assert status(flipped(FILE7, byte, byte % 8)) == capi.RF_EINTEGRITY, byte


# What a flipped bit gives, field by field.  Structure is checked before any
# checksum, so a field the structural checks constrain is RF_EINVAL; a field
# they cannot judge alone is caught by SHA-256(header || digests): RF_EINTEGRITY.
HEADER_FIELDS = [
    ("magic", range(0, 8), capi.RF_EINVAL),
    ("version", range(8, 12), capi.RF_EINVAL),
    ("flags", range(12, 16), capi.RF_EINVAL),
    # 7 entries become another count: the file's length no longer matches (or the count is beyond 2^30)
    ("n_entries", range(16, 24), capi.RF_EINVAL),
    # total_bytes is compared with the entries only after the checksums: the header checksum sees it first
    ("total_bytes", range(32, 40), capi.RF_EINTEGRITY),
    ("reserved", range(40, 64), capi.RF_EINVAL),
]


@pytest.mark.parametrize("name,where,want", HEADER_FIELDS, ids=[f[0] for f in HEADER_FIELDS])
def test_a_flipped_bit_in_a_header_field(name, where, want):
    for byte in where:
        for bit in range(8):
            assert status(flipped(FILE7, byte, bit)) == want, (name, byte, bit)


def test_a_flipped_bit_in_chunk_and_in_the_end_marker():
    """chunk: 280 B in granules of 80 are 4 digests.  A flip that changes the
    number of digests changes the length the header implies: RF_EINVAL.  One
    that keeps 4 (80 -> 81, 88, 72: bits 0, 3 ... ) leaves the structure
    consistent, and the header checksum catches it: RF_EINTEGRITY."""
    for byte in range(24, 32):
        for bit in range(8):
            chunk = 80 ^ (1 << (8 * (byte - 24) + bit))
            want = capi.RF_EINTEGRITY if -(-280 // chunk) == 4 else capi.RF_EINVAL
            assert status(flipped(FILE7, byte, bit)) == want, (byte, bit)
    for byte in range(len(FILE7) - 8, len(FILE7)):
        for bit in range(8):
            assert status(flipped(FILE7, byte, bit)) == capi.RF_EINVAL, (byte, bit)


# ---- 4. rule violations under valid checksums ------------------------------------------------
def test_rule_violations_with_valid_checksums():
    ids, sizes = SEVEN
    assert status(C.write_file(ids, sizes, 80)) == capi.RF_OK
    bad = {
        "two equal IDs": C.write_file(ids[:3] + [ids[2]] + ids[4:], sizes, 80),
        "descending IDs": C.write_file(ids[:2] + [ids[3], ids[2]] + ids[4:], sizes, 80),
        "a negative size": C.write_file(ids, sizes[:5] + [-1] + sizes[6:], 80),
        "total_bytes one too many": C.write_file(ids, sizes, 80, total=sum(sizes) + 1),
        "total_bytes one too few": C.write_file(ids, sizes, 80, total=sum(sizes) - 1),
        "sizes that overflow int64": C.write_file(ids, [2 ** 63 - 1, 2 ** 63 - 1] + sizes[2:], 80),
        "sizes that overflow to the stated total": C.write_file(ids, [2 ** 63 - 1, 1] + sizes[2:], 80),
        "chunk 0 in a file": C.write_file(ids, sizes, 40 * 7, header_chunk=0),
        "chunk 0 in an empty file": C.write_file([], [], 80, header_chunk=0),
        "version 2": C.write_file(ids, sizes, 80, version=2),
        "flags 1": C.write_file(ids, sizes, 80, flags=1),
        "reserved bytes": C.write_file(ids, sizes, 80, reserved=bytes(23) + b"\1"),
        "end marker": C.write_file(ids, sizes, 80, end=b"RFASEND1"),
        "magic": C.write_file(ids, sizes, 80, magic=b"RFASSOC1"),
    }
    for what, f in bad.items():
        assert status(f) == capi.RF_EINVAL, what
    # 2^61 entries in a 200-byte file: 40 * 2^61 wraps to 0 in 64 bits
    h = C.header(2 ** 61, 80, 0)
    f = h + bytes(96) + hashlib.sha256(h).digest() + C.END
    assert len(f) == 200 and status(f) == capi.RF_EINVAL
    for n in (2 ** 30 + 1, 2 ** 64 - 1, (2 ** 64) // 40 + 1):
        h = C.header(n, 80, 0)
        assert status(h + bytes(96) + hashlib.sha256(h).digest() + C.END) == capi.RF_EINVAL, n
    # format applies the rules to what it is given
    for i, s in ((ids[:2] + [ids[3], ids[2]] + ids[4:], sizes), (ids, sizes[:5] + [-1] + sizes[6:]),
                 (ids, [2 ** 63 - 1, 2 ** 63 - 1] + sizes[2:])):
        with pytest.raises(capi.RfError) as ei:
            capi.repo_file_format(*arrays(i, s), chunk=80)
        assert ei.value.code == capi.RF_EINVAL


# ---- 5. the committed fixture -------------------------------------------------------------------
def test_committed_fixture():
    with open(FIXTURE, "rb") as fh:
        f = fh.read()
    assert len(f) == 64 + 5 * 40 + 3 * 32 + 40 < 1024
    assert f == C.write_file(C.GOLDEN_IDS, C.GOLDEN_SIZES, C.GOLDEN_CHUNK)
    ids, sizes = capi.repo_file_parse(f)
    assert [bytes(r) for r in ids] == C.GOLDEN_IDS and sizes.tolist() == C.GOLDEN_SIZES
    assert capi.repo_file_format(ids, sizes, chunk=C.GOLDEN_CHUNK) == f


# ---- 6. the same under the sanitizers -----------------------------------------------------------
def test_repo_file_code_under_asan_ubsan():
    """tests/cpp/asan_repo_file: repo_io.cpp, host_sha.cpp and errors.cpp under
    AddressSanitizer + UndefinedBehaviorSanitizer, a stand-alone program with its
    own main over the round trips, truncations, flips and rule violations above
    (every buffer exactly as long as `len`) and a few thousand seeded random
    corruptions.  Built and run directly; nothing is preloaded."""
    b = subprocess.run(["make", "-C", CSRC, "asan_repo"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "asan_repo_file")], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.strip() == "PASS"
