"""The Fileset unmarshal without a GPU (rf_fileset_unmarshal_flat: the
sequential form of reflow_amd/csrc/json_parse.h and, beside it on every
document, the per-byte form the kernels of k12_unmarshal.hip run -- the call
fails where the two differ) against the model of tests/unmarshal_model.py:
the hand tables of tests/test_marshal_flat.py read backwards, round trips,
arbitrary byte paths, the refusal table with its reason bits, every
single-byte mutation of a set of small documents, every proper prefix, and the
stand-alone program tests/cpp/json_parse_test.cpp, plain and under
AddressSanitizer + UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import unmarshal_cases as C
import unmarshal_model as M
from reflow_amd import capi
from test_marshal_flat import HAND, STRINGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "json_parse_test")


def flat_checked(docs, label=""):
    f = capi.FilesetForest.flat(docs)
    try:
        C.check_forest(f, docs, label)
        return f.status(), f.values()
    finally:
        f.close()


def test_hand_tables_backwards():
    _, values = flat_checked([doc for _, doc in HAND])
    assert [v.flat() for v in values] == [M.flat(M.canon(v)) for v, _ in HAND]
    assert capi.fileset_unmarshal_flat([]) == []


def test_strings_backwards():
    docs = [C.one(q) for _, q in STRINGS]
    _, values = flat_checked(docs)
    for (s, q), v in zip(STRINGS, values):
        (path, (fid, size)), = v.map.items()
        assert (fid, size) == (C.ID1, 1)
        assert path == (s if b"\\ufffd" not in q else b"\xef\xbf\xbd" * len(s))
    # the escape decodes to U+FFFD, a raw U+FFFD stays raw: one value, two documents
    a, b = capi.fileset_unmarshal_flat([C.one(b'"\\ufffd"'), C.one(b'"\xef\xbf\xbd"')])
    assert a == b and list(a.map) == [b"\xef\xbf\xbd"]


@pytest.mark.parametrize("size", [0, -1, (1 << 63) - 1, -(1 << 63), 10, -10])
def test_sizes(size):
    v, = capi.fileset_unmarshal_flat([C.one(b'"s"', size)])
    assert v.map == {b"s": (C.ID1, size)}


def test_round_trip_of_valid_utf8_trees():
    """unmarshal(marshal(t)) == t, Maps in key order, empty Lists and Maps absent,
    and every such document is accepted (the reference marshal's condition)."""
    trees = C.random_trees(0xB0B, 300)
    docs = capi.fileset_marshal_flat(trees)
    assert docs == [t.json() for t in trees]
    (status, reason, _, _), values = flat_checked(docs)
    assert not status.any() and not reason.any()
    assert [v.flat() for v in values] == [M.flat(M.canon(t)) for t in trees]
    assert values[0] == capi.fileset_unmarshal_flat(docs[:1])[0]


def test_arbitrary_byte_paths_follow_the_model():
    trees = C.random_trees(0xA11, 300, valid_utf8=False)
    docs = [t.json() for t in trees]
    (status, reason, _, _), _ = flat_checked(docs)
    # replacement bytes may break the order, and nothing else can be wrong with the marshal's bytes
    assert set(reason.tolist()) <= {0, M.ORDER} and int((status == capi.RF_OK).sum()) > len(docs) // 2


def test_refusals_and_their_reasons():
    docs = [d for d, _ in C.REFUSALS]
    (status, reason, ncnt, ecnt), values = flat_checked(docs, "refusals")
    assert reason.tolist() == [bit for _, bit in C.REFUSALS]
    assert (status == capi.RF_ENOTCANONICAL).all() and values == [None] * len(docs)
    assert not ncnt.any() and not ecnt.any()


def test_accepted_edges_and_a_refused_document_between_accepted_ones():
    (status, _, _, _), _ = flat_checked(C.ACCEPTED)
    assert not status.any()
    docs = [C.one(b'"a"', 1), b'{"List":[]}', C.one(b'"b"', 2), b'', b'{}']
    f = capi.FilesetForest.flat(docs)
    C.check_forest(f, docs)
    s = f.copy()
    assert s["doc_node_ptr"].tolist() == [0, 1, 1, 2, 2, 3] and s["sizes"].tolist() == [1, 2]
    assert s["entry_ptr"].tolist() == [0, 1, 2, 2] and s["paths"].tobytes() == b"ab"
    f.close()


def test_every_single_byte_mutation():
    docs = C.mutation_batch()
    (status, _, _, _), _ = flat_checked(docs, "mutations")
    accepted = int((status == capi.RF_OK).sum())
    assert 0 < accepted < len(docs)  # the model accepts some mutants and refuses some


def test_every_proper_prefix_is_refused():
    for doc in C.MUTATION_DOCS + [t.json() for t in C.random_trees(0x9E, 6)]:
        prefixes = [doc[:k] for k in range(len(doc))]
        (status, _, _, _), _ = flat_checked(prefixes)
        assert (status == capi.RF_ENOTCANONICAL).all()


def test_threads_and_the_plain_form_agree():
    docs = [t.json() for t in C.random_trees(0x51, 400, valid_utf8=False)] + C.mutation_batch()[:500]
    a = capi.FilesetForest.flat(docs, flags=0, threads=1)
    b = capi.FilesetForest.flat(docs, flags=capi.RF_UNMARSHAL_CHECK_TILED, threads=4)
    for x, y in zip(a.status(), b.status()):
        assert (x == y).all()
    sa, sb = a.copy(), b.copy()
    assert all((sa[k] == sb[k]).all() for k in sa)
    a.close()
    b.close()


def test_arguments():
    h = ctypes.c_void_p()
    L = capi.lib()
    assert L.rf_fileset_unmarshal_flat(None, None, 1, 0, 0, ctypes.byref(h)) == capi.RF_EINVAL
    assert L.rf_fileset_unmarshal_flat(None, None, 0, 0, 0, None) == capi.RF_EINVAL
    offs = np.array([4, 2], np.uint64)
    buf = np.zeros(8, np.uint8)
    assert L.rf_fileset_unmarshal_flat(buf.ctypes.data, offs.ctypes.data, 1, 0, 0, ctypes.byref(h)) == capi.RF_EINVAL
    # the device forms and the accessors refuse null arguments before they touch a device
    assert L.rf_fileset_unmarshal_device(None, None, 0, None, None, 0, ctypes.byref(h), None) == capi.RF_EINVAL
    assert L.rf_fileset_unmarshal(None, None, None, 0, ctypes.byref(h), None) == capi.RF_EINVAL
    assert L.rf_fileset_forest_info(None, None, None, None, None, None) == capi.RF_EINVAL
    assert L.rf_fileset_forest_status(None, None, None, None, None) == capi.RF_EINVAL
    assert L.rf_fileset_forest_copy(None, None, None, None, None, None, None, None) == capi.RF_EINVAL
    assert L.rf_fileset_forest_rows_device(None, None, None, None, None) == capi.RF_EINVAL
    assert L.rf_fileset_forest_times(None, None) == capi.RF_EINVAL and len(L.rf_last_error()) > 0
    L.rf_fileset_forest_free(None)  # a no-op, like the other destroy calls
    f = capi.FilesetForest.flat([b"{}"])
    with pytest.raises(capi.RfError) as e:  # a host-form forest has no device rows
        f.rows_device()
    assert e.value.code == capi.RF_EINVAL
    f.close()
    # the tree helper refuses depths that are no tree in closing order
    dn = np.array([0, 2], np.uint64)
    lp, lc, roots = np.zeros(3, np.uint64), np.zeros(2, np.uint32), np.zeros(1, np.uint32)
    for depths in ([0, 0], [0, 1], [2, 0]):
        nd = np.array(depths, np.uint32)
        assert L.rf_fileset_forest_tree(dn.ctypes.data, 1, nd.ctypes.data, 2, lp.ctypes.data, lc.ctypes.data,
                                        roots.ctypes.data) == capi.RF_EINVAL, depths


@pytest.fixture(scope="module")
def bins():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    b = subprocess.run(["make", "-C", CSRC, "json_parse_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_json_parse_program(bins, build):
    """The same tables, random trees through json_emit.h and back, single-byte
    and random mutations with both forms on each, documents that end in a
    backslash run and inside a UTF-8 sequence -- every document in a heap block
    of exactly its length."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([bins[build]], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[-2:] == ["PASS", ""]
