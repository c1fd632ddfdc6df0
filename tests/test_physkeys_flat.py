"""The physical keys on the host (no GPU): rf_physkeys_flat -- the per-entry
and per-segment code the K13 kernels run (phys_emit.h) -- against the oracle's
OFlow.physical_digest() and OFileset.material() over seeded graphs and values,
values given as forest arrays (through the JSON round trip and the host
unmarshal) and as trees; the has-children rule of the closing order against
rf_fileset_forest_tree; the golden physical digests; and the stand-alone
tests/cpp/phys_flat_test.cpp, plain and under ASan + UBSan."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import physkeys_cases as PC
import reflow_oracle as O
import unmarshal_cases as UC
from reflow_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reflow_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "cpp", "phys_flat_test")

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import golden_io as G  # noqa: E402


def forest_structure(values):
    """The host arrays of rf_fileset_forest_copy for the values' JSON."""
    f = capi.FilesetForest.flat([v.json() for v in values])
    try:
        assert f.n_accepted == len(values)
        return f.copy()
    finally:
        f.close()


@pytest.mark.parametrize("seed,n", [(1, 1), (2, 7), (3, 40), (4, 120), (5, 300)])
def test_flat_matches_the_oracle(seed, n):
    nodes = PC.random_flows(seed, n)
    g = PC.Graph(nodes, seed)
    idx, vals = PC.valued(nodes)
    want = g.want_rows()
    k_forest, m_forest = capi.physkeys_flat(*g.open_args(), idx, g.n_rows, structure=forest_structure(vals),
                                            keys=PC.pattern(g.n_rows))
    k_tree, m_tree = capi.physkeys_flat(*g.open_args(), idx, g.n_rows, sets=vals, keys=PC.pattern(g.n_rows))
    assert m_forest == [v.material() for v in vals]
    assert m_tree == m_forest
    assert (k_forest == want).all() and (k_tree == want).all()
    # something was computable, something was not, something had no row
    keyed = [nodes[i].physical_digest() for i in g.keyed]
    if n >= 40:
        assert any(keyed) and not all(keyed) and len(g.keyed) < n


def test_flat_value_shapes():
    """List of Lists, a node with both List and Map (the Map is ignored), an
    empty value, paths of length 0 and 1, bytes >= 0x80, an escaped byte, a dep
    twice, a node without deps, an empty suffix."""
    A, B, C = (bytes([k]) * 32 for k in (1, 2, 3))
    leaf = O.OFileset(map={"": (A, 1), "b": (B, 2), "é\"\n": (C, 3)})
    vals = [O.OFileset(list=[O.OFileset(list=[leaf, O.OFileset()]), leaf]),
            O.OFileset(map={"ignored": (A, 1)}, list=[O.OFileset(map={"x": (B, 1)})]),
            O.OFileset()]
    assert vals[1].material() == b"x\x00\x05" + B and vals[2].material() == b""
    v = [O.OFlow("OpMerge", done=True, value=x) for x in vals]
    nodes = v + [O.OFlow("OpExec", [v[0], v[1], v[0]], image="i", cmd="c"), O.OFlow("OpExtern", [v[2]], url=""),
                 O.OFlow("OpExtern", [], url="u"), O.OFlow("OpExec", [], image="", cmd="")]
    g = PC.Graph(nodes)
    for form in ("structure", "sets"):
        kw = {form: forest_structure(vals) if form == "structure" else vals}
        keys, mats = capi.physkeys_flat(*g.open_args(), [0, 1, 2], g.n_rows, keys=PC.pattern(g.n_rows), **kw)
        assert mats == [x.material() for x in vals]
        assert (keys == g.want_rows()).all()
        assert keys[g.phys_row[4]].tobytes() == O.sha256(b"") == keys[g.phys_row[6]].tobytes()


def test_flat_last_value_wins_and_skips():
    rng = __import__("random").Random(9)
    a, b = PC.files(rng, 3), PC.files(rng, 2)
    src = O.OFlow("OpMerge", done=True, value=b)
    nodes = [src, O.OFlow("OpExtern", [src], url="u")]
    g = PC.Graph(nodes)
    keys, mats = capi.physkeys_flat(*g.open_args(), [0, capi.RF_PHYS_SKIP, 0], g.n_rows, sets=[a, a, b])
    assert mats == [a.material(), b"", b.material()]
    assert keys[g.phys_row[1]].tobytes() == nodes[1].physical_digest()


def test_flat_refusals():
    rng = __import__("random").Random(3)
    v = PC.files(rng, 1)
    st = forest_structure([v])
    ok = dict(dep_ptr=[0, 0, 1], deps=[0], phys_row=[PC.NO_ROW, 0], suffixes=[b"", b"s"])

    def call(nodes=(0,), n_rows=1, structure=st, **kw):
        a = dict(ok, **kw)
        keys = PC.pattern(max(n_rows, 1))
        with pytest.raises(capi.RfError) as e:
            capi.physkeys_flat(a["dep_ptr"], a["deps"], a["phys_row"], a["suffixes"], list(nodes), n_rows,
                               structure=structure, keys=keys)
        assert e.value.code == capi.RF_EINVAL
        assert (keys == PC.pattern(max(n_rows, 1))).all()

    call(deps=[1])                      # a cycle
    call(deps=[2])                      # a dep out of range
    call(dep_ptr=[0, 1, 0])             # pointers not monotone
    call(phys_row=[0, 0])               # a row used twice
    call(n_rows=0)                      # a row beyond the table
    call(nodes=[2])                     # a value for a node that is not there
    bad = capi.FilesetForest.flat([b'{"List":[]}'])
    try:
        call(structure=bad.copy())      # a refused document with a real node
    finally:
        bad.close()
    keys, _ = capi.physkeys_flat(ok["dep_ptr"], ok["deps"], ok["phys_row"], ok["suffixes"], [0], 1, structure=st)
    assert keys[0].tobytes() == O.sha256(v.material() + b"s")


def test_has_children_rule_matches_forest_tree():
    """Node j has List children iff it is not its document's first node and the
    node before it is one level deeper -- against rf_fileset_forest_tree's CSR."""
    docs = [d for d in UC.ACCEPTED + UC.MUTATION_DOCS] + [v.json() for v in UC.random_trees(11, 200)]
    f = capi.FilesetForest.flat(docs)
    try:
        o = f.copy()
        nn, nd = f.n_nodes, f.n_docs
        lp, lc, roots = np.zeros(nn + 1, np.uint64), np.zeros(max(nn, 1), np.uint32), np.zeros(nd, np.uint32)
        assert capi.lib().rf_fileset_forest_tree(o["doc_node_ptr"].ctypes.data, nd, o["node_depth"].ctypes.data, nn,
                                                 lp.ctypes.data, lc.ctypes.data, roots.ctypes.data) == capi.RF_OK
    finally:
        f.close()
    depth, dptr = o["node_depth"], o["doc_node_ptr"]
    parents = 0
    for d in range(nd):
        for j in range(int(dptr[d]), int(dptr[d + 1])):
            rule = j > int(dptr[d]) and int(depth[j - 1]) == int(depth[j]) + 1
            assert rule == (lp[j + 1] > lp[j]), (d, j)
            parents += rule
    assert parents > 100 and nn > 500


def test_golden_physical_digests():
    checked = 0
    for c in G.load("flows.json")["cases"]:
        _, nodes = G.json_to_flow(c["flow"])
        g = PC.Graph(nodes)
        idx, vals = PC.valued(nodes)

        def round_trips(v):  # an empty non-nil List has no tree (or JSON) form
            return v.list is None or (len(v.list) > 0 and all(round_trips(x) for x in v.list))
        if not g.keyed or not all(round_trips(v) for v in vals):
            continue
        keys, _ = capi.physkeys_flat(*g.open_args(), idx, g.n_rows, sets=vals)
        for i, want in zip(range(len(nodes)), c["nodes"]):
            if g.phys_row[i] != PC.NO_ROW:
                assert keys[g.phys_row[i]].tobytes().hex() == (want["physical"] or PC.ZERO.hex()), (c["name"], i)
                checked += want["physical"] is not None
    assert checked >= 2


@pytest.fixture(scope="module")
def bins():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    b = subprocess.run(["make", "-C", CSRC, "phys_flat_test"], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    return {"plain": BIN, "asan": BIN + "_asan"}


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_phys_flat_program(bins, build):
    """Seeded graphs and values, tree-given and forest-given, through the tiled
    code path against a naive sequential one with its own SHA-256; materials
    that cross gather tiles; the refusals."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([bins[build]], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split("\n")[-2:] == ["PASS", ""]
