"""The Fileset values' piece stream without a GPU (rf_fileset_marshal_flat:
flatten, sort and the per-piece emit code the marshal kernels run) against
hand-written bytes of Go 1.9/1.10 encoding/json -- the tables of
tests/test_fileset_json.py, restated here --, against the recursive host
marshaller (rf_fileset_marshal_json) and the oracle (OFileset.json) on seeded
random trees, several roots per call; its refusals; and the stand-alone
program tests/cpp/marshal_flat_test.cpp, plain and under AddressSanitizer +
UBSan."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import reflow_oracle as O
from reflow_amd import capi
from reflow_oracle import OFileset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "marshal_flat_test")

ID1 = bytes(range(1, 33))
HEX1 = ID1.hex().encode()

# Expected bytes written out by hand from encoding/json's rules.
HAND = [
    (OFileset(), b"{}"),
    (OFileset(list=[], map={}), b"{}"),
    (OFileset(map={"a": (ID1, 7)}), b'{"Fileset":{"a":{"ID":"sha256:' + HEX1 + b'","Size":7}}}'),
    (OFileset(list=[OFileset()]), b'{"List":[{}]}'),
    (OFileset(list=[OFileset()], map={"b": (ID1, -2)}),
     b'{"List":[{}],"Fileset":{"b":{"ID":"sha256:' + HEX1 + b'","Size":-2}}}'),
    (OFileset(map={"b": (ID1, 0), "B": (ID1, 0), "a/b": (ID1, 0)}),
     b'{"Fileset":{"B":{"ID":"sha256:' + HEX1 + b'","Size":0},"a/b":{"ID":"sha256:' + HEX1 +
     b'","Size":0},"b":{"ID":"sha256:' + HEX1 + b'","Size":0}}}'),
]

STRINGS = [
    (b"plain/path.fq", b'"plain/path.fq"'),
    (b'a"b\\c', b'"a\\"b\\\\c"'),
    (b"\n\r\t", b'"\\n\\r\\t"'),
    (b"\x00\x08\x0c\x1f", b'"\\u0000\\u0008\\u000c\\u001f"'),   # Go < 1.22: no \b \f short forms
    (b"<>&", b'"\\u003c\\u003e\\u0026"'),                       # escapeHTML
    (b"\x7f", b'"\x7f"'),                                        # DEL is not escaped
    ("\u00e9\u65e5\U0001F600".encode(), b'"' + "\u00e9\u65e5\U0001F600".encode() + b'"'),
    ("\u2028\u2029".encode(), b'"\\u2028\\u2029"'),
    (b"\xff", b'"\\ufffd"'),
    (b"\xe2\x82", b'"\\ufffd\\ufffd"'),                         # truncated: one per byte
    (b"\xed\xa0\x80", b'"\\ufffd\\ufffd\\ufffd"'),              # surrogate half
    (b"\xc0\xaf", b'"\\ufffd\\ufffd"'),                         # overlong
    (b"\xf4\x90\x80\x80", b'"\\ufffd\\ufffd\\ufffd\\ufffd"'),   # > U+10FFFF
    ("\ufffd".encode(), b'"\xef\xbf\xbd"'),                      # a real U+FFFD stays raw
]


def random_tree(rng, depth=0):
    """The generator shape of tests/test_fileset_json.py: depth <= 3, empty Maps
    and Lists, paths biased toward multi-byte sequences and escapes, sizes
    across int64."""
    def path():
        n = rng.randint(0, 12)
        pool = [rng.randrange(256) for _ in range(n)]
        if rng.random() < 0.3:
            pool += list(rng.choice(["\u00e9", "\u65e5", "\u2028", "\U0001F600"]).encode())
        return bytes(pool)
    m = None
    if rng.random() < 0.8:
        m = {}
        for _ in range(rng.randint(0, 6)):
            m[path()] = (bytes(rng.randrange(1, 256) for _ in range(32)), rng.randint(-(1 << 63), (1 << 63) - 1))
    lst = None
    if depth < 3 and rng.random() < 0.4:
        lst = [random_tree(rng, depth + 1) for _ in range(rng.randint(0, 3))]
    return OFileset(map=m, list=lst)


def random_trees(seed=0xB0B, n=300):
    rng = random.Random(seed)
    return [random_tree(rng) for _ in range(n)]


def test_hand_json():
    got = capi.fileset_marshal_flat([v for v, _ in HAND])  # one call, several roots
    assert got == [want for _, want in HAND]
    for v, want in HAND:
        assert capi.fileset_marshal_flat([v]) == [want] == [capi.fileset_marshal_json(v)] == [v.json()]


@pytest.mark.parametrize("s,want", STRINGS)
def test_escaping(s, want):
    v = OFileset(map={s: (ID1, 1)})
    want = b'{"Fileset":{' + want + b':{"ID":"sha256:' + HEX1 + b'","Size":1}}}'
    assert capi.fileset_marshal_flat([v]) == [want]
    assert O.go_json_string(s) + b':{"ID":"sha256:' + HEX1 + b'","Size":1}' in want


@pytest.mark.parametrize("size", [0, -1, (1 << 63) - 1, -(1 << 63), 10, -10])
def test_sizes(size):
    assert capi.fileset_marshal_flat([OFileset(map={"s": (ID1, size)})]) == \
        [b'{"Fileset":{"s":{"ID":"sha256:' + HEX1 + b'","Size":' + str(size).encode() + b'}}}']


def test_random_trees_against_the_host_marshaller_and_the_oracle():
    trees = random_trees()
    want = [v.json() for v in trees]
    assert [capi.fileset_marshal_json(v) for v in trees[:60]] == want[:60]
    for lo in range(0, len(trees), 25):  # 25 roots per call; the offsets are checked by the binding
        assert capi.fileset_marshal_flat(trees[lo:lo + 25]) == want[lo:lo + 25]
    assert capi.fileset_marshal_flat(trees) == want
    assert capi.fileset_marshal_flat([]) == []


def _flat_rc(t, roots):
    r = np.array(roots, np.uint32)
    need = ctypes.c_uint64(0)
    return capi.lib().rf_fileset_marshal_flat(ctypes.byref(t), r.ctypes.data, len(r), None, 0, None, ctypes.byref(need))


def test_refusals():
    with pytest.raises(capi.RfError) as e:  # a zero ID, host-side
        capi.fileset_marshal_flat([OFileset(map={"a": (bytes(32), 1)})])
    assert e.value.code == capi.RF_EINVAL and "zero file ID" in str(e.value)
    b = capi.FilesetTreeBuilder()  # duplicate keys
    b.paths += [b"x", b"y", b"x"]
    b.ids += [ID1, ID1, ID1]
    b.sizes += [1, 2, 3]
    b.list_ptr += [None]
    b.entry_ptr += [3]
    b._pending.append((0, []))
    t = b.struct()
    assert _flat_rc(t, [0]) == capi.RF_EINVAL and b"duplicate" in capi.lib().rf_last_error()
    assert _flat_rc(t, [1]) == capi.RF_EINVAL  # a bad root
    # a cyclic list_child: node 0 lists node 1, node 1 lists node 0
    b = capi.FilesetTreeBuilder()
    b.list_ptr += [None, None]
    b.entry_ptr += [0, 0]
    b._pending += [(0, [1]), (1, [0])]
    t = b.struct()
    assert _flat_rc(t, [0]) == capi.RF_EINVAL and b"4096" in capi.lib().rf_last_error()
    need = ctypes.c_uint64(0)
    assert capi.lib().rf_fileset_marshal_flat(None, None, 0, None, 0, None, ctypes.byref(need)) == capi.RF_EINVAL


@pytest.fixture(scope="module")
def bins():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    b = subprocess.run(["make", "-C", CSRC, "marshal_flat_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_marshal_flat_program(bins, build):
    """The same cases plus random byte strings as paths, a path that ends
    inside a multi-byte sequence followed in one blob by a path that begins
    with continuation bytes, and a 70,000-entry Map through the threaded sort."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([bins[build]], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[-2:] == ["PASS", ""]
