"""What the physical-key tests share (CPU and GPU): seeded Fileset values and
node graphs as oracle objects, their arrays for rf_physkeys_open, and the rows
the oracle expects (OFlow.physical_digest / OFileset.material).  A helper, not
a test."""
import random

import numpy as np

import reflow_oracle as O
from reflow_amd import capi

NO_ROW = capi.RF_PHYS_NO_ROW
ZERO = bytes(32)
PATH_CHARS = ["a", "b", "/", '"', "\\", "\n", "<", "é", "日", "\U0001F600", "z", "\t", "0"]


def fid(rng):
    return bytes(rng.randrange(1, 256) for _ in range(32))


def files(rng, n, plen=None, prefix=""):
    """A Map of n distinct paths (plen: each path's length in characters)."""
    assert plen is None or len(PATH_CHARS) ** plen >= 2 * n or n <= 1
    m = {}
    while len(m) < n:
        k = rng.randint(0, 12) if plen is None else plen
        m[prefix + "".join(rng.choice(PATH_CHARS) for _ in range(k))] = (fid(rng), rng.randint(0, 1 << 40))
    return O.OFileset(map=m)


def sized(rng, material_len):
    """A one-file value whose material has exactly this many bytes (>= 34)."""
    assert material_len >= 34
    return O.OFileset(map={"p" * (material_len - 34): (fid(rng), 1)})


def random_value(rng, depth=0):
    """list is None or non-empty: a JSON round trip cannot tell an empty List from nil."""
    m = None
    if rng.random() < 0.8:
        m = files(rng, rng.randint(0, 6)).map or None
    lst = None
    if depth < 3 and rng.random() < 0.4:
        lst = [random_value(rng, depth + 1) for _ in range(rng.randint(1, 3))]
    return O.OFileset(map=m, list=lst)


def random_flows(seed, n, valued=0.7):
    """n oracle flow nodes, deps among the earlier ones (now and then one twice);
    execs and externs have physical keys; a seeded share is done with a value."""
    rng = random.Random(seed)
    nodes = []
    for i in range(n):
        k = min(i, rng.choice([0, 1, 1, 2, 3, 5]))
        deps = [nodes[j] for j in rng.sample(range(i), k)] if k else []
        if deps and rng.random() < 0.2:
            deps.append(deps[0])
        op = rng.choice(["OpExec", "OpExec", "OpExtern", "OpMerge", "OpIntern"])
        kw = {}
        if op == "OpExec":
            kw = dict(image=rng.choice(["", "ubuntu", "img:%d" % i]), cmd="echo %d {{.}}" % i if rng.random() < 0.8 else "",
                      argmap=[(rng.random() < 0.3, rng.randrange(4)) for _ in range(rng.randint(0, 3))])
        elif op in ("OpExtern", "OpIntern"):
            kw = dict(url="s3://bucket/%d" % i if rng.random() < 0.8 else "")
        f = O.OFlow(op, deps, **kw)
        if rng.random() < valued:
            f.done, f.value = True, random_value(rng)
        nodes.append(f)
    return nodes


def has_key(f):
    return f.op in (O.OP["OpExec"], O.OP["OpExtern"])


def suffix_of(f):
    if f.op == O.OP["OpExtern"]:
        return f.url.encode()
    if f.op == O.OP["OpExec"]:
        return f.image.encode() + f.cmd.encode() + f.argbytes()
    return b""


class Graph:
    """The arrays of rf_physkeys_open for a list of oracle flow nodes; the key
    rows are a seeded permutation with gaps, so that a row is not its node."""

    def __init__(self, nodes, seed=0):
        self.nodes = nodes
        ix = {id(f): i for i, f in enumerate(nodes)}
        self.dep_ptr, self.deps = [0], []
        for f in nodes:
            self.deps += [ix[id(d)] for d in f.deps]
            self.dep_ptr.append(len(self.deps))
        self.suffixes = [suffix_of(f) for f in nodes]
        keyed = [i for i, f in enumerate(nodes) if has_key(f)]
        self.n_rows = len(keyed) + 3
        rows = list(range(self.n_rows))
        random.Random(seed).shuffle(rows)
        self.phys_row = [NO_ROW] * len(nodes)
        for i, r in zip(keyed, rows):
            self.phys_row[i] = r
        self.keyed = keyed

    def open_args(self):
        return self.dep_ptr, self.deps, self.phys_row, self.suffixes

    def consumers(self, listed):
        s = set(listed)
        return sorted({i for i, f in enumerate(self.nodes) if any(self.deps[e] in s for e in
                                                                  range(self.dep_ptr[i], self.dep_ptr[i + 1]))})

    def want_rows(self, affected=None, rows=None):
        """The key rows [n_rows, 32] after an update of `affected` (default:
        every node) over `rows` (default: a pattern no digest equals)."""
        out = pattern(self.n_rows) if rows is None else rows.copy()
        for i in (self.keyed if affected is None else affected):
            if self.phys_row[i] == NO_ROW:
                continue
            p = self.nodes[i].physical_digest()
            out[self.phys_row[i]] = np.frombuffer(p or ZERO, dtype=np.uint8)
        return out


def pattern(n_rows):
    return (np.arange(32 * n_rows, dtype=np.uint32) * 7 + 1).astype(np.uint8).reshape(n_rows, 32)


def valued(nodes):
    """(node indices, their OFileset values) of the nodes that are done."""
    idx = [i for i, f in enumerate(nodes) if f.done and f.value is not None]
    return idx, [nodes[i].value for i in idx]
