"""Fileset JSON unmarshalled on the device (rf_fileset_unmarshal_device,
rf_fileset_unmarshal, rf_fileset_forest_*, k12_unmarshal.hip).  Every result --
status, reason, counts, depths, pointer arrays, path bytes, IDs, sizes and the
device rows -- is compared with the host form (rf_fileset_unmarshal_flat) and
with the model of tests/unmarshal_model.py, at the tile edges, over long
backslash runs and quote-free tiles, with many documents in one tile, on the
mutation batch of the CPU test, and end to end behind the cache write's
marshal."""
import ctypes

import numpy as np
import pytest

import unmarshal_cases as C
import unmarshal_model as M
from reflow_amd import capi
from reflow_oracle import OFileset

pytestmark = pytest.mark.gpu

T = capi.RF_UNMARSHAL_TILE
KEYS = ("doc_node_ptr", "node_depth", "entry_ptr", "path_off", "paths", "ids32", "sizes")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


class Arena:
    """Documents at chosen offsets of one device arena (default: packed), the
    gaps filled with a byte that would be wrong anywhere."""

    def __init__(self, ctx, docs, offs=None, lens=None, fill=0x7D, tail=0):
        if offs is None:
            offs = np.concatenate([[0], np.cumsum([len(d) for d in docs])])[:len(docs)]
        self.offs = np.asarray(offs, dtype=np.uint64)
        self.lens = np.asarray([len(d) for d in docs] if lens is None else lens, dtype=np.int64)
        end = max([int(o) + len(d) for o, d in zip(self.offs, docs)] + [0]) + tail
        self.bytes = end
        host = np.full(max(end, 1), fill, np.uint8)
        for o, d in zip(self.offs, docs):
            host[int(o):int(o) + len(d)] = np.frombuffer(d, np.uint8)
        self.n = len(docs)
        self.d_arena, self.d_offs, self.d_lens = ctx.upload(host), ctx.upload(self.offs if self.n else np.zeros(1, np.uint64)), \
            ctx.upload(self.lens if self.n else np.zeros(1, np.int64))

    def args(self):
        return self.d_arena.ptr, self.bytes, self.d_offs.ptr, self.d_lens.ptr, self.n

    def free(self):
        for b in (self.d_arena, self.d_offs, self.d_lens):
            b.free()


def snapshot(f):
    """Everything a forest holds, as bytes: the status arrays, the structure, the device rows."""
    out = [a.tobytes() for a in f.status()]
    s = f.copy()
    out += [s[k].tobytes() for k in KEYS]
    if f.ctx is not None:
        d_counts, d_ids, d_sizes, n_rows = f.rows_device()
        L = capi.lib()
        counts, ids, sizes = np.zeros(max(f.n_docs, 1), np.uint32), np.zeros(max(32 * n_rows, 1), np.uint8), \
            np.zeros(max(n_rows, 1), np.int64)
        for dst, src, nb in ((counts, d_counts, 4 * f.n_docs), (ids, d_ids, 32 * n_rows), (sizes, d_sizes, 8 * n_rows)):
            if nb:
                capi._check(L.rf_memcpy_d2h(f.ctx.handle, dst.ctypes.data, ctypes.c_void_p(src), nb))
        assert n_rows == f.n_entries
        assert counts[:f.n_docs].tobytes() == f.status()[3].tobytes()
        assert ids[:32 * n_rows].tobytes() == s["ids32"].tobytes() and sizes[:n_rows].tobytes() == s["sizes"].tobytes()
    return out


def dev_checked(ctx, docs, offs=None, label="", **kw):
    """The device form over docs at offs: equal to the host form in every array, and to the model."""
    a = Arena(ctx, docs, offs, **kw)
    f = capi.FilesetForest.from_device(ctx, *a.args())
    h = capi.FilesetForest.flat(docs)
    try:
        assert snapshot(f) == snapshot(h), label
        C.check_forest(f, docs, label)
        return f.status(), f.copy()
    finally:
        f.close()
        h.close()
        a.free()


def test_tile_edge_sweep(ctx):
    """A leading path of 120 consecutive lengths slides an entry whose path holds
    an escaped quote, a backslash pair, an HTML escape and a 4-byte sequence,
    then its 64 hex digits, its Size digits and the closing }}} over byte T of
    its document; a second set of as many slides the same over 2T.  Every document
    starts on a tile boundary, so T in the document is a tile edge in the arena."""
    last = C.ent(b'"b\\"\\\\\\u003c\xf0\x9f\x98\x80"', b"12345678901")
    window = len(last) + 4
    head, lead = b'{"Fileset":{"', C.ent(b'"', 5)
    docs = []
    for edge in (T, 2 * T):
        for k in range(3, window + 3):
            comma = edge - window + k - 1  # where the entry under test begins; the document ends window - 1 later
            d = head + b"a" * (comma - len(head) - len(lead)) + lead + b"," + last + b"}}"
            assert d[comma:comma + 3] == b',"b' and len(d) > edge and comma <= edge + 1
            docs.append(d)
    assert len(docs) >= 2 * 120
    offs = np.arange(len(docs), dtype=np.uint64) * (3 * T)
    (status, _, _, ecnt), s = dev_checked(ctx, docs, offs, "sweep")
    assert not status.any() and (ecnt == 2).all() and (s["sizes"][1::2] == 12345678901).all()


def test_backslash_runs_and_quote_free_tiles(ctx):
    docs = [C.one(b'"' + b"\\" * 6000 + b'"'),          # 3,000 backslashes, escaped: whole tiles of them
            C.one(b'"' + b"\\" * 6002 + b'"'),          # one more
            C.one(b'"' + b"\\" * 6001 + b'"'),          # an odd run swallows the quote: refused
            C.one(b'"' + b"p" * (3 * T) + b'"', 9),     # parity carried through tiles with no quote
            C.one(b'"' + b"\\" * 6000 + b'\\""')]       # an even run, then an escaped quote
    (status, reason, _, _), s = dev_checked(ctx, docs, [3, 6200, 12400, 18600, 32000], "runs")
    assert status.tolist() == [0, 0, capi.RF_ENOTCANONICAL, 0, 0]
    assert np.diff(s["path_off"]).tolist() == [3000, 3001, 3 * T, 3001]


def test_paths_longer_than_64_kib(ctx):
    """A path's closing quote carries the path's whole decoded length into its
    tile's sums: decoded paths above 65536 bytes whose entries end in the same
    tile as the entries behind them, so the later entries' path offsets depend
    on a per-chunk prefix beyond 16 bits."""
    long_plain = b"p" * 70000
    long_mixed = b"\\\\" * 40000 + b"m" * 30000 + b"\\u003c" * 100  # 110,600 bytes, 70,100 decoded
    docs = [C.one(b'"lead"', 3),
            b'{"Fileset":{' + C.ent(b'"' + long_plain + b'"', 1) + b',' + C.ent(b'"q"', 2) + b',' + C.ent(b'"r"', 3) + b'}}',
            b'{"List":[{"Fileset":{' + C.ent(b'"' + long_mixed + b'"', 4) + b',' + C.ent(b'"n"', 5) + b'}},{}],"Fileset":{' +
            C.ent(b'"' + long_plain + b'p"', 6) + b',' + C.ent(b'"z"', 7) + b'}}',
            C.one(b'"tail"', 8)]
    offs = np.cumsum([9] + [len(d) + 5 for d in docs])[:-1]
    (status, _, _, ecnt), s = dev_checked(ctx, docs, offs, "long paths")
    assert not status.any() and ecnt.tolist() == [1, 3, 4, 1]
    assert np.diff(s["path_off"]).tolist() == [4, 70000, 1, 1, 70100, 1, 70001, 1, 4]
    assert s["sizes"].tolist() == [3, 1, 2, 3, 4, 5, 6, 7, 8] and s["paths"].tobytes().endswith(b"ztail")


def test_many_documents_in_a_tile(ctx):
    empties = [b"{}"] * 3000
    (status, _, ncnt, _), s = dev_checked(ctx, empties, label="pitch 2")
    assert not status.any() and (ncnt == 1).all() and s["doc_node_ptr"].tolist() == list(range(3001))
    dev_checked(ctx, empties, np.arange(3000) * 16, "pitch 16")
    small = [C.one(b'"f%d"' % i, i) for i in range(400)]
    offs = np.cumsum([0] + [len(d) + 1 + 2 * (i % 3) for i, d in enumerate(small)])[:-1] + 1  # odd offsets, ragged gaps
    (status, _, _, _), s = dev_checked(ctx, small, offs, "odd offsets")
    assert not status.any() and s["sizes"].tolist() == list(range(400))
    # a refused document between two accepted ones: its neighbours' rows dense and unchanged
    around = [C.one(b'"x"', 1), b'{"List":[{}],"Fileset":{' + C.ent(b'"y"', 2) + b'}}']
    for bad in (b'{"List":[]}', C.one(b'"q"', b"01"), b"", C.one(b'"<"')):
        docs = [around[0], bad, around[1]]
        (status, _, ncnt, ecnt), s = dev_checked(ctx, docs, [5, 5 + len(around[0]) + 1, 400], "refused between")
        assert status.tolist() == [0, capi.RF_ENOTCANONICAL, 0] and ecnt.tolist() == [1, 0, 1] and ncnt.tolist() == [1, 0, 2]
        assert s["sizes"].tolist() == [1, 2] and s["paths"].tobytes() == b"xy" and s["entry_ptr"].tolist() == [0, 1, 1, 2]


def test_a_cut_document(ctx):
    """len cuts the document short; the arena bytes behind the cut would complete it."""
    full = C.one(b'"a"', 12)
    docs = [full, full, full]
    a = Arena(ctx, docs, [0, 1000, 2 * T - 20], lens=[len(full), len(full) - 1, len(full) - 2], tail=64)
    f = capi.FilesetForest.from_device(ctx, *a.args())
    status, reason, _, ecnt = f.status()
    assert status.tolist() == [0, capi.RF_ENOTCANONICAL, capi.RF_ENOTCANONICAL]
    assert reason.tolist() == [0, M.LENGTH, M.LENGTH] and ecnt.tolist() == [1, 0, 0]
    C.check_forest(f, [full, full[:-1], full[:-2]])
    f.close()
    a.free()


def test_depth(ctx):
    docs = [C.chain(4096), C.chain(4097), C.chain(3)]
    (status, reason, ncnt, _), s = dev_checked(ctx, docs, [7, 50000, 100000], "depth")
    assert status.tolist() == [0, capi.RF_ENOTCANONICAL, 0] and reason.tolist() == [0, M.DEPTH, 0]
    assert ncnt.tolist() == [4097, 0, 4] and s["node_depth"][:4097].tolist() == list(range(4096, -1, -1))


def test_refusal_table(ctx):
    docs = [d for d, _ in C.REFUSALS] + C.ACCEPTED
    (status, reason, _, _), _ = dev_checked(ctx, docs, label="refusals")
    assert reason.tolist() == [bit for _, bit in C.REFUSALS] + [0] * len(C.ACCEPTED)


def test_mutations_in_one_call(ctx):
    docs = C.mutation_batch()
    (status, _, _, _), _ = dev_checked(ctx, docs, label="mutations")
    assert 0 < int((status == capi.RF_OK).sum()) < len(docs)


def test_random_trees_at_ragged_offsets(ctx):
    docs = [t.json() for t in C.random_trees(0xB0B, 300)] + [t.json() for t in C.random_trees(0xA11, 200, False)]
    rng = np.random.default_rng(5)
    offs = np.cumsum([0] + [len(d) + int(rng.integers(0, 40)) for d in docs])[:-1]
    dev_checked(ctx, docs, offs, "random trees")


def test_bad_layouts(ctx):
    d = [C.one(b'"a"'), C.one(b'"b"'), C.one(b'"c"')]
    n = len(d[0])
    assert n < 150
    for offs, lens, size in (([200, 100, 300], None, None),           # descending
                             ([0, n - 1, 300], None, None),            # overlapping
                             ([0, 150, 300], None, 300 + n - 1),       # past the arena
                             ([0, 150, 300], [n, -1, n], None)):       # a negative length
        a = Arena(ctx, d, offs, lens=lens)
        if size is not None:
            a.bytes = size
        with pytest.raises(capi.RfError) as e:
            capi.FilesetForest.from_device(ctx, *a.args())
        assert e.value.code == capi.RF_EINVAL
        a.free()
    a = Arena(ctx, d)
    with pytest.raises(capi.RfError) as e:  # 4 GiB and beyond is refused before anything is read
        capi.FilesetForest.from_device(ctx, a.d_arena.ptr, 1 << 32, a.d_offs.ptr, a.d_lens.ptr, 3)
    assert e.value.code == capi.RF_EINVAL
    a.free()
    dev_checked(ctx, d, [0, 150, 300], "the context stays usable")


def test_empty_batch(ctx):
    for f in (capi.FilesetForest.from_device(ctx, None, 0, None, None, 0), capi.FilesetForest.from_host(ctx, [])):
        assert (f.n_docs, f.n_accepted, f.n_nodes, f.n_entries, f.path_bytes) == (0, 0, 0, 0, 0)
        assert f.values() == [] and f.rows_device()[3] == 0
        assert f.copy()["entry_ptr"].tolist() == [0]
        f.close()
    (status, reason, _, _), _ = dev_checked(ctx, [b"", b""], label="only empty documents")
    assert reason.tolist() == [M.LENGTH, M.LENGTH]


def test_round_trip_with_the_cache_write(ctx):
    """rf_fileset_marshal_device -> rf_json_batch_device -> rf_fileset_unmarshal_device,
    no host copy between; the rows feed missing() and the liveset as they stand."""
    from test_gpu_repo import DevOut
    def sized(t):  # the repository index takes no negative size
        return OFileset(map=None if t.map is None else {k: (i, s & ((1 << 62) - 1)) for k, (i, s) in t.map.items()},
                        list=None if t.list is None else [sized(c) for c in t.list])
    sets = [sized(t) for t in C.random_trees(0x7E, 150)] + [OFileset(map={"d%03d/f%05d" % (i % 7, i): (bytes([1 + i % 250] * 32), i)
                                                     for i in range(1500)})]
    batch = capi.JsonBatch(ctx, sets)
    lens = batch.lens()
    arena_bytes = int(((lens + 15) & ~15).sum())
    d_arena, d_offs, d_lens = batch.device()
    f = capi.FilesetForest.from_device(ctx, d_arena, arena_bytes, d_offs, d_lens, len(sets))
    status, _, _, ecnt = f.status()
    assert not status.any()
    assert [v.flat() for v in f.values()] == [M.flat(M.canon(t)) for t in sets]
    s = f.copy()
    d_counts, d_ids, d_sizes, n_rows = f.rows_device()
    ids, sizes = s["ids32"].reshape(-1, 32), s["sizes"]
    # the rows are the original entries: node by node in closing order, each Map in key order
    rows = [e for t in sets for _, ents in M.flat(M.canon(t)) for e in ents]
    po, paths = s["path_off"], s["paths"].tobytes()
    assert n_rows == len(rows) and ecnt.tolist() == [sum(len(e) for _, e in M.flat(M.canon(t))) for t in sets]
    assert [(paths[int(po[i]):int(po[i + 1])], ids[i].tobytes(), int(sizes[i])) for i in range(n_rows)] == rows
    # missing(): the device rows as they stand against the same rows given from the host
    repo = capi.Repo(ctx)
    have = np.arange(0, n_rows, 3)
    repo.put(ids[have], sizes[have])
    want = repo.missing(ecnt, ids, sizes)
    out = DevOut(ctx, len(sets), n_rows, capi.RepoMissing.FIELDS)
    repo.missing_device(d_counts, len(sets), d_ids, d_sizes, n_rows, out.o)
    ctx.sync()
    got = out.read()
    for k in ("n_files", "n_missing", "missing_bytes", "miss_ptr"):
        assert (getattr(got, k) == getattr(want, k)).all(), k
    assert got.n_listed == want.n_listed
    n = want.n_listed
    assert (got.miss_rows[:n] == want.miss_rows[:n]).all() and (got.miss_ids32[:n] == want.miss_ids32[:n]).all()
    out.free()
    # the liveset: the forest's counts and device rows against the host-form set_values
    nodes = np.arange(len(sets), dtype=np.uint32)
    edge_ptr = np.zeros(len(sets) + 1, np.uint64)
    runs = []
    for device in (True, False):
        live = capi.GcLiveset(ctx, edge_ptr, np.zeros(0, np.uint32))
        if device:
            live.set_values_device(nodes, ecnt, d_ids, d_sizes)
        else:
            live.set_values(nodes, ecnt, ids, sizes)
        st = live.run(nodes)
        runs.append((st.nlive_est, st.nlive, st.livebytes, st.contributions, tuple(st.counts), live.states().tobytes()))
        live.close()
    assert runs[0] == runs[1] and runs[0][0] == n_rows
    repo.close()
    f.close()
    batch.close()


def test_two_calls_give_equal_bytes_and_the_host_input_form_agrees(ctx):
    docs = [t.json() for t in C.random_trees(0x2B, 200, False)] + C.mutation_batch()[:300] + [C.chain(100)]
    a = Arena(ctx, docs)
    f1 = capi.FilesetForest.from_device(ctx, *a.args())
    f2 = capi.FilesetForest.from_device(ctx, *a.args())
    f3 = capi.FilesetForest.from_host(ctx, docs)
    s1 = snapshot(f1)
    assert s1 == snapshot(f2) == snapshot(f3)
    assert len(f1.times()) == 3 and f3.times()[0] > 0
    assert capi.fileset_unmarshal(ctx, docs[:50]) == capi.fileset_unmarshal_flat(docs[:50])
    for f in (f1, f2, f3):
        f.close()
    a.free()
