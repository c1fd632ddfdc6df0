"""Fileset values marshalled on the device (rf_fileset_marshal_device,
rf_json_batch_*, k11_cwrite.hip): the bytes copied back must equal the host
marshal byte for byte and every digest hashlib's SHA-256 of those bytes -- on
the hand-written tables and the seeded random trees of
tests/test_marshal_flat.py, at the tile, padding and path-length edges, with
the File IDs in device memory, and on one long value."""
import ctypes
import hashlib

import numpy as np
import pytest

import reflow_oracle as O
from reflow_amd import capi
from reflow_oracle import OFileset
from test_marshal_flat import HAND, HEX1, ID1, STRINGS, random_trees

pytestmark = pytest.mark.gpu

T = capi.RF_MARSHAL_TILE


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


def marshal(ctx, sets, want=None):
    """The batch's bytes and digests, checked against the host marshal."""
    want = [v.json() for v in sets] if want is None else want
    b = capi.JsonBatch(ctx, sets)
    got = b.copy()
    assert [len(g) for g in got] == [len(w) for w in want] == b.lens().tolist()
    assert got == want
    assert b.n == len(sets) and b.total_bytes == sum(len(w) for w in want)
    assert b.digests() == [hashlib.sha256(w).digest() for w in want]
    pieces = b.n_pieces
    b.close()
    return got, pieces


def entry_json(path_json, size=1):
    return path_json + b':{"ID":"sha256:' + HEX1 + b'","Size":' + str(size).encode() + b'}'


def test_hand_and_strings(ctx):
    marshal(ctx, [v for v, _ in HAND], [w for _, w in HAND])
    sets = [OFileset(map={s: (ID1, 1)}) for s, _ in STRINGS]
    marshal(ctx, sets, [b'{"Fileset":{' + entry_json(w) + b'}}' for _, w in STRINGS])
    # all the strings as the keys of one Map, against the host marshallers
    one = OFileset(map={s: (ID1, i) for i, (s, _) in enumerate(STRINGS)})
    assert marshal(ctx, [one])[0] == capi.fileset_marshal_flat([one]) == [capi.fileset_marshal_json(one)]


def test_random_trees(ctx):
    trees = random_trees()
    got, _ = marshal(ctx, trees)
    assert got == capi.fileset_marshal_flat(trees)
    marshal(ctx, trees[:1])
    marshal(ctx, [])


def flat_map(k, tag=""):
    """A Map of k entries, keys already in order: k + 2 pieces ({"Fileset":{ , k entries, }})."""
    return OFileset(map={"%s%06d" % (tag, i): (ID1, i) for i in range(k)})


@pytest.mark.parametrize("pieces", [T - 1, T, T + 1, 2 * T + 1])
def test_piece_counts_at_the_tile_edges(ctx, pieces):
    _, got = marshal(ctx, [flat_map(pieces - 2)])
    assert got == pieces


def test_values_straddling_tile_edges_with_empty_values_between(ctx):
    empty = OFileset()
    sets = [empty, flat_map(T - 5, "a"), empty, empty, flat_map(7, "b"), empty, flat_map(2 * T - 3, "c"), empty,
            OFileset(list=[flat_map(3, "d"), empty]), flat_map(T, "e"), empty]
    _, pieces = marshal(ctx, sets)
    assert pieces > 4 * T


def test_lengths_around_the_alignment(ctx):
    """JSON lengths 15, 16, 17 and 0 mod 16 side by side: every value starts at a
    16-byte aligned offset, its neighbours stay intact and the zeroed pad does
    not leak into a digest."""
    sets = [OFileset(map={"p" * n: (ID1, 1)}) for n in (5, 6, 7, 22, 5, 7)]
    got, _ = marshal(ctx, sets)
    assert [len(g) % 16 for g in got] == [15, 0, 1, 0, 15, 1]
    b = capi.JsonBatch(ctx, sets)
    arena, d_offs, _ = b.device()
    offs = np.zeros(len(sets), np.uint64)
    capi._check(capi.lib().rf_memcpy_d2h(ctx.handle, offs.ctypes.data, ctypes.c_void_p(d_offs), offs.nbytes))
    assert (offs % 16 == 0).all() and (np.diff(offs) >= [len(g) for g in got[:-1]]).all()
    end = int(offs[-1]) + len(got[-1])
    raw = np.zeros(end + 15 - (end + 15) % 16, np.uint8)
    capi._check(capi.lib().rf_memcpy_d2h(ctx.handle, raw.ctypes.data, ctypes.c_void_p(arena), raw.nbytes))
    covered = np.zeros(len(raw), bool)
    for o, g in zip(offs, got):
        assert raw[int(o):int(o) + len(g)].tobytes() == g
        covered[int(o):int(o) + len(g)] = True
    assert not raw[~covered].any()  # the pad bytes are zero
    b.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4096])
def test_path_lengths_with_an_escape_last(ctx, n):
    path = b"a" * (n - 1) + b"\n" if n else b""
    want = b'{"Fileset":{' + entry_json(b'"' + b"a" * max(n - 1, 0) + (b"\\n" if n else b"") + b'"') + b'}}'
    marshal(ctx, [OFileset(map={path: (ID1, 1)})], [want])
    for last in (b"\xe2", b"<", "\u2028".encode(), b'"'):  # other final bytes: a cut sequence, an HTML escape, ...
        marshal(ctx, [OFileset(map={b"a" * n + last: (ID1, 1)})])


def test_a_cut_sequence_does_not_borrow_the_next_path(ctx):
    """Entry b"\\xe2\\x82" directly followed in input order by entry b"\\xac":
    together they would be U+20AC; each bad byte is its own replacement."""
    v = OFileset(map={b"\xe2\x82": (ID1, 1), b"\xac": (ID1, 2)})
    want = b'{"Fileset":{' + entry_json(b'"\\ufffd"', 2) + b',' + entry_json(b'"\\ufffd\\ufffd"', 1) + b'}}'
    marshal(ctx, [v], [want])
    # and as two values of one batch, the cut path the last byte of its value's paths
    marshal(ctx, [OFileset(map={b"\xe2\x82": (ID1, 1)}), OFileset(map={b"\xac": (ID1, 2)})])


@pytest.mark.parametrize("size", [0, -1, (1 << 63) - 1, -(1 << 63)])
def test_sizes(ctx, size):
    marshal(ctx, [OFileset(map={"s": (ID1, size)})], [b'{"Fileset":{' + entry_json(b'"s"', size) + b'}}'])


def test_ids_in_device_memory(ctx):
    trees = random_trees(seed=0x1D5, n=40)
    b = capi.FilesetTreeBuilder()
    roots = [b.add(v) for v in trees]
    t = b.struct()
    ids = b._keep["ids"]
    d_ids = ctx.upload(ids)
    host = capi.JsonBatch(ctx, tree=t, roots=roots)
    t_no_ids = capi.FilesetTree(t.n_nodes, t.list_ptr, t.list_child, t.entry_ptr, t.paths, t.path_lens, None, t.sizes)
    dev = capi.JsonBatch(ctx, tree=t_no_ids, roots=roots, d_ids32=d_ids.ptr)
    assert dev.copy() == host.copy() == [v.json() for v in trees]
    assert dev.digests() == host.digests() == [O.sha256(v.json()) for v in trees]
    dev.close()
    host.close()
    # a zero ID in the device form: found on the device, RF_EINVAL, no batch object
    zeroed = ids.copy()
    entry = len(b.paths) // 2
    zeroed[32 * entry:32 * entry + 32] = 0
    d_ids.copy_from(zeroed)
    h = ctypes.c_void_p()
    r = np.array(roots, np.uint32)
    rc = capi.lib().rf_fileset_marshal_device(ctx.handle, ctypes.byref(t_no_ids), r.ctypes.data, len(r), d_ids.ptr,
                                              ctypes.byref(h), None)
    assert rc == capi.RF_EINVAL and not h.value and b"zero file ID" in capi.lib().rf_last_error()
    # host-side IDs: refused before the device sees anything
    with pytest.raises(capi.RfError) as e:
        capi.JsonBatch(ctx, [OFileset(map={"a": (bytes(32), 1)})])
    assert e.value.code == capi.RF_EINVAL
    d_ids.free()


def test_one_long_value_and_the_one_call_form(ctx):
    """A 20,000-file Map is one long message (JSON ~2 MB): its digest is the oracle's."""
    big = OFileset(map={"d%03d/f%05d.bam" % (i % 97, i): (O.from_string(str(i)), i) for i in range(20000)})
    sets = random_trees(seed=0x7A1, n=50) + [big]
    want = [v.json() for v in sets]
    fsids, sizes = ctx.fileset_value_digests_device(sets)
    assert fsids == [O.sha256(w) for w in want] == ctx.fileset_value_digests(sets)
    assert sizes.tolist() == [len(w) for w in want]


def test_two_runs_give_equal_bytes(ctx):
    sets = random_trees(seed=0x2B, n=120) + [flat_map(T + 3)]
    a, b = capi.JsonBatch(ctx, sets), capi.JsonBatch(ctx, sets)
    assert a.copy() == b.copy() and a.digests() == b.digests()
    assert a.copy(which=[5, 5, 0, 119]) == [a.copy()[i] for i in (5, 5, 0, 119)]
    a.close()
    b.close()
