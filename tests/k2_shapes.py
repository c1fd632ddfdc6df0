"""Ragged byte-2 job graphs for K2's fused-chain fast path, and a short
restatement of the loader's level and fusion rule to check them with.

K2's fast path (k2_level_pl cb0 = 2: split block 0, the producer's operand
hand-off, the block-1 pre-build, sf_pos, hash_fused_chain_lean) is taken when
every fusion target's one hole sits at material byte 2 (GraphDev::fuse_pos2).
The 1000align graphs take it with every lane of a workgroup alike; the random
graphs of test_gpu_dag_fusion vary the lanes but put holes anywhere, which
clears fuse_pos2.  ragged() keeps every single-hole reader of a job output at
byte 2 and varies everything else within a level: template lengths at the
SHA-256 padding edges (1 to 12 blocks), chain depths 0..7, heads with and
without a load-time midstate, producers with a second single-hole consumer
that must be queued -- in levels whose queueable width the caller gives, so
the edges of the kernel forms (32-job half workgroups and chain waves, 64-job
workgroups, 128/192/256 sink lanes, k2_level_lf's 256) are hit exactly.

analyze() derives from the arrays alone what rf_graph_load derives: levels,
fusion targets, slot-fused jobs, the sink level, the internal order.  The CPU
tests (test_k2_shapes.py) assert the mix on it; the GPU tests
(test_gpu_dag_shapes.py) run the graphs.  A helper module, not a conftest."""
import random

import numpy as np

# fusion-target template lengths, by block count (len + 9 + 63) // 64: the
# last 1-block length and the first 2-block one, and so on (bold in the issue)
EDGE_LENGTHS = (34, 35, 54, 55, 56, 57, 63, 64, 65, 118, 119, 120, 127, 128, 183, 184, 247, 248)
LONG_BLOCKS = (9, 10, 11, 12)  # and one length of 9-12 blocks, drawn per job
WIDTHS = (1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 255, 256, 257)
TAILS = (0, 1, 9, 23, 55, 56, 64, 100, 200)
SF_SETTINGS = (2, 8, 40, "mix")


def nblocks(n):
    return (n + 9 + 63) // 64


_BY_BLOCKS = {}
for _n in EDGE_LENGTHS:
    _BY_BLOCKS.setdefault(min(nblocks(_n), 3), []).append(_n)  # 1, 2, 3+ (3, 4 and 5 blocks)


def _target_len(rng):
    """A fusion target's length: 1-block, 2-block and 3+-block targets about
    equally often (a 32-job half must hold all three), the 9-12-block one rare."""
    r = rng.random()
    if r < 0.06:
        b = rng.choice(LONG_BLOCKS)
        return rng.randint(64 * (b - 1) - 8, 64 * b - 9)
    return rng.choice(_BY_BLOCKS[1 if r < 0.37 else 2 if r < 0.68 else 3])


class _Job:
    __slots__ = ("level", "key", "length", "holes", "role", "depth", "tail", "id")

    def __init__(self, level, key, length, holes, role, depth=0, tail=None):
        self.level, self.key, self.length, self.holes = level, key, length, holes
        self.role, self.depth, self.tail = role, depth, tail  # holes: [(pos, ("in", slot) | ("job", _Job))]
        self.id = -1


def ragged(seed, widths, n_in=192, n_sf=72, sf=2, sinks=0, merge=False, break_pos2=False):
    """(a, info): an rf_graph_desc-shaped dict and what was built.

    widths[l]: queueable jobs of level l (multi-hole heads plus the queued
    twin of a producer with two single-hole consumers).  One more level above
    (info["cap_level"]) reads every job still unread, so that no queueable job
    below it is a sink the loader would move; with merge it is a level of few
    long multi-hole jobs above every chain (the octo form's), under one root.
    n_sf slot-fused jobs (one hole on an input slot, at sf or mixed), each
    with a chain.  sinks: multi-hole jobs nobody reads.  break_pos2: one
    fusion target's hole at byte 3."""
    rng = random.Random(seed)
    jobs, by_level = [], {}
    must, opens = [], []  # queueable jobs nobody reads yet; open chain tails
    pending = {}  # level -> twins already queued there

    def add(j):
        jobs.append(j)
        by_level.setdefault(j.level, []).append(j)
        return j

    def chain(head, depth):
        """depth single-hole byte-2 jobs under head; the tail ends open (a sink
        unless a later multi-hole job reads it) or beside a queued twin."""
        head.depth = depth
        prev = head
        for _ in range(depth):
            prev = add(_Job(prev.level + 1, rng.random(), _target_len(rng), [(2, ("job", prev))], "chain"))
        if depth == 0:
            if head.role != "sf":  # (a slot-fused job is never queueable)
                must.append(head)
            return
        lv = prev.level  # the twin reads the tail's producer: same level as the tail
        if lv < len(widths) and pending.get(lv, 0) < widths[lv] // 4 and rng.random() < 0.3:
            producer = prev.holes[0][1][1]
            twin = add(_Job(lv, prev.key + (1 - prev.key) * rng.random(), _target_len(rng),
                            [(2, ("job", producer))], "twin"))
            pending[lv] = pending.get(lv, 0) + 1
            head.tail = "twin"
            chain(twin, rng.randint(0, 3))
        else:
            head.tail = "open"
            opens.append(prev)

    def multi(level, sources, role, first=None, tail=None, gaps=(0, 0, 1, 2, 5, 17, 40)):
        pos = rng.choice([0, 1, 2, 3, 30, 31, 32, 33, 58, 62, 63] if rng.random() < 0.5
                         else [64, 65, 90, 127, 128, 190]) if first is None else first
        holes = []
        for s in sources:
            holes.append((pos, s))
            pos += 32 + rng.choice(gaps)
        return _Job(level, rng.random(), pos + (rng.choice(TAILS) if tail is None else tail), holes, role)

    def source(level):
        """A hole of a multi-hole job at `level`: a job nobody reads yet, an
        open chain tail, a recent job, or an input slot."""
        r = rng.random()
        unread = next((j for j in must if j.level < level), None)
        if unread is not None and r < 0.6:
            must.remove(unread)
            return ("job", unread)
        if r < 0.75:
            for _ in range(4):
                t = rng.choice(opens) if opens else None
                if t is not None and t.level < level:
                    return ("job", t)
        if r < 0.9 and level > 0:
            lv = max(0, level - 1 - min(int(rng.expovariate(0.7)), level - 1))
            return ("job", rng.choice(by_level[lv]))
        return ("in", rng.randrange(n_in))

    # slot-fused jobs: input slot i's only single-hole reader, hole at sf
    for i in range(n_sf):
        p = rng.choice([2, 8, 40]) if sf == "mix" else sf
        lens = [n for n in EDGE_LENGTHS if n >= p + 32]
        chain(add(_Job(0, rng.random(), rng.choice(lens), [(p, ("in", i))], "sf")), rng.randint(0, 7))
    for level, w in enumerate(widths):
        for _ in range(w - pending.get(level, 0)):
            nh = rng.randint(2, 4) if rng.random() < 0.6 else rng.randint(5, 12)
            if level == 0:
                srcs = [("in", rng.randrange(n_in)) for _ in range(nh)]
            else:
                below = [j for j in must if j.level == level - 1]
                if below:
                    must.remove(below[0])
                srcs = [("job", below[0] if below else rng.choice(by_level[level - 1]))]
                srcs += [source(level) for _ in range(nh - 1)]
                rng.shuffle(srcs)
            chain(add(multi(level, srcs, "head")), rng.randint(0, 7))
    top = max(by_level)
    unread, must[:] = list(must), []
    info = dict(widths=list(widths), n_in=n_in, sf=sf)
    for k in range(sinks):  # read inputs and low levels: final by the fill level
        lv = rng.randint(0, min(2, len(widths) - 1))
        srcs = [("in", rng.randrange(n_in)) for _ in range(rng.randint(2, 6))]
        if lv:
            srcs[0] = ("job", rng.choice(by_level[lv - 1]))
        jobs.append(multi(lv, srcs, "sink"))  # (not in by_level: nobody may read it)
    if merge:
        # few long jobs above every chain, none with a fusion target
        cap = top + 1
        deepest = by_level[top]
        n_m = max(4, (len(unread) + 29) // 30)
        ms = []
        for k in range(n_m):
            srcs = [("job", rng.choice(deepest))] + [("job", j) for j in unread[k::n_m]]
            while len(srcs) < 32:
                srcs.append(source(cap))
            ms.append(add(multi(cap, srcs[:40], "merge", first=rng.choice([2, 2, 64, 130]), gaps=(0, 1, 2, 2, 2, 3))))
        add(multi(cap + 1, [("job", m) for m in ms], "root", first=2))
        info["cap_level"], info["cap_width"] = cap, n_m
    else:
        cap = len(widths)
        below = list(by_level[cap - 1])
        n_c = max(1, (len(unread) + 9) // 10)
        for k in range(n_c):
            srcs = [("job", j) for j in unread[k::n_c]] + [("job", rng.choice(below))]
            srcs += [source(cap) for _ in range(rng.randint(0, 2) if len(srcs) > 1 else 2)]
            add(multi(cap, srcs[:12], "cap"))
        info["cap_level"], info["cap_width"] = cap, n_c + pending.get(cap, 0)
    if break_pos2:
        victim = next(j for j in jobs if j.role == "chain" and j.length >= 35 and j.level >= 2)
        victim.holes = [(3, victim.holes[0][1])]
        info["broken"] = victim
    # emit: level ascending, kinds shuffled within a level (a twin after the
    # consumer it shares its producer with: the loader fuses the first)
    jobs.sort(key=lambda j: (j.level, j.key))
    for i, j in enumerate(jobs):
        j.id = i
    blob_rng = np.random.default_rng(seed)
    off, pos, slot, ptr, cur = [], [], [], [0], 0
    for j in jobs:
        off.append(cur)
        cur += j.length
        for p, (kind, s) in j.holes:
            assert p + 32 <= j.length
            pos.append(p)
            slot.append(s if kind == "in" else n_in + s.id)
        ptr.append(len(pos))
    a = dict(n_slots=n_in + len(jobs), out_slot=np.arange(n_in, n_in + len(jobs), dtype=np.uint32),
             tmpl_off=np.array(off, np.uint64), tmpl_len=np.array([j.length for j in jobs], np.uint32),
             hole_ptr=np.array(ptr, np.uint64), hole_pos=np.array(pos, np.uint32),
             hole_slot=np.array(slot, np.uint32), blob=blob_rng.integers(0, 256, size=cur, dtype=np.uint8))
    info["n_jobs"] = len(jobs)
    info["role"] = [j.role for j in jobs]
    info["level"] = np.array([j.level for j in jobs], np.uint32)
    info["holes"] = np.array([len(j.holes) for j in jobs], np.uint32)
    info["blocks"] = np.array([nblocks(j.length) for j in jobs], np.uint32)
    info["depth"] = np.array([j.depth for j in jobs], np.uint32)  # of heads, twins and slot-fused jobs
    info["heads"] = np.array([j.id for j in jobs if j.role in ("head", "twin", "sf")], np.uint32)
    info["tail"] = {j.id: j.tail for j in jobs if j.tail}
    if break_pos2:
        info["broken"] = info["broken"].id
    return a, info


def stride(seed, n_heads=262144 + 257, n_in=4096):
    """The throughput form's grid-stride case, built with numpy: level 0 of
    n_heads two-hole heads over n_in input slots (more than k2_level_lf's 1024
    workgroups of 256 lanes take in one pass), each with a ragged byte-2 chain
    of depth 0..7.  Templates are windows of one 1 MiB random blob."""
    rng = np.random.default_rng(seed)
    # (4,100 slices, each must hold a depth 0; short chains more often: the case is about the grid)
    depth = rng.choice(8, size=n_heads, p=[0.2, 0.25, 0.2, 0.12, 0.08, 0.06, 0.05, 0.04])
    first = rng.choice(np.array([0, 1, 2, 31, 33, 63, 64, 65, 100, 130]), size=n_heads)
    gap = rng.choice(np.array([0, 1, 17, 40]), size=n_heads)
    # 4-6 blocks, whatever the first hole: the loader's blocks-descending order
    # must not sort the heads with a midstate (first hole >= 64) apart
    b = rng.integers(4, 7, size=n_heads)
    h_len = np.maximum(first + 64 + gap, rng.integers(64 * (b - 1) - 8, 64 * b - 8))
    n_chain = int(depth.sum())
    # chain jobs in order of their place in the chain, then head: producers first
    lens = np.array(EDGE_LENGTHS + tuple(64 * b - 9 - 13 * (b - 9) for b in LONG_BLOCKS))
    cls = np.array([min(nblocks(int(n)), 3) if n <= 248 else 4 for n in lens])
    w = np.where(cls == 4, 0.04 / 4, 0.32 / np.array([np.sum(cls == c) for c in cls]))
    c_len = rng.choice(lens, size=n_chain, p=w / w.sum())
    prod = np.empty(n_chain, np.int64)
    prev, base = np.arange(n_heads, dtype=np.int64), n_heads
    for k in range(1, 8):
        idx = np.nonzero(depth >= k)[0]
        prod[base - n_heads:base - n_heads + len(idx)] = prev[idx]
        prev[idx] = base + np.arange(len(idx))
        base += len(idx)
    n_jobs = n_heads + n_chain
    length = np.concatenate([h_len, c_len]).astype(np.uint32)
    hole_ptr = np.concatenate([[0], np.cumsum(np.concatenate([np.full(n_heads, 2), np.ones(n_chain, np.int64)]))])
    hpos = np.empty(2 * n_heads + n_chain, np.uint32)
    hslot = np.empty_like(hpos)
    hpos[0:2 * n_heads:2] = first
    hpos[1:2 * n_heads:2] = first + 32 + gap
    hslot[:2 * n_heads] = rng.integers(0, n_in, size=2 * n_heads)
    hpos[2 * n_heads:] = 2
    hslot[2 * n_heads:] = n_in + prod
    blob = rng.integers(0, 256, size=1 << 20, dtype=np.uint8)
    off = rng.integers(0, (1 << 20) - 1024, size=n_jobs).astype(np.uint64)
    a = dict(n_slots=n_in + n_jobs, out_slot=np.arange(n_in, n_in + n_jobs, dtype=np.uint32), tmpl_off=off,
             tmpl_len=length, hole_ptr=hole_ptr.astype(np.uint64), hole_pos=hpos, hole_slot=hslot, blob=blob)
    info = dict(widths=[n_heads], n_in=n_in, sf=None, n_jobs=n_jobs, depth=depth, heads=np.arange(n_heads))
    return a, info


def analyze(a):
    """What rf_graph_load derives from the arrays (capi.cpp): topological
    levels, each producer's fusion target (its first single-hole consumer),
    slot-fused jobs (an input slot's first single-hole consumer), queueable
    jobs, the sink level (queueable jobs nobody reads, at or below the fill
    level, move to a last level of their own), constant leading blocks, and
    the internal order (level ascending, blocks descending, stable)."""
    S = int(a["n_slots"])
    out = np.asarray(a["out_slot"], np.int64)
    J = len(out)
    ptr = np.asarray(a["hole_ptr"], np.int64)
    hpos = np.asarray(a["hole_pos"], np.int64)
    hslot = np.asarray(a["hole_slot"], np.int64)
    nh = np.diff(ptr)
    blocks = (np.asarray(a["tmpl_len"], np.int64) + 9 + 63) // 64
    producer = np.full(S, -1, np.int64)
    producer[out] = np.arange(J)
    hjob = np.repeat(np.arange(J), nh)
    hprod = producer[hslot]
    assert (hprod < hjob).all(), "jobs are given producers first"
    level = np.zeros(J, np.int64)
    while True:
        nxt = level.copy()
        m = hprod >= 0
        np.maximum.at(nxt, hjob[m], level[hprod[m]] + 1)
        if (nxt == level).all():
            break
        level = nxt
    # first single-hole consumer of each slot, in job order
    single = nh[hjob] == 1
    s1, j1 = hslot[single], hjob[single]
    slots_first, idx = np.unique(s1, return_index=True)
    fuse = np.full(J, -1, np.int64)
    fused_target = np.zeros(J, bool)
    slot_fused = np.zeros(J, bool)
    by_job = producer[slots_first] >= 0
    fuse[producer[slots_first[by_job]]] = j1[idx][by_job]
    fused_target[j1[idx][by_job]] = True
    slot_fused[j1[idx][~by_job]] = True
    queueable = ~fused_target & ~slot_fused & (nh > 0)
    readers = np.bincount(hslot, minlength=S)
    sink = readers[out] == 0
    L = int(level.max()) + 1 if J else 0
    sink_level = fill = None
    qs = queueable & ~sink
    if qs.any():
        nsq = np.bincount(level[qs], minlength=L)
        n_sink = int((queueable & sink).sum())
        lq = int(level[qs].max())
        for l in range(lq, 0, -1):
            if nsq[l] * 64 >= n_sink:
                lq = l
                break
        moved = queueable & sink & (level <= lq)
        if lq > 0 and moved.any():
            level = level.copy()
            level[moved] = L
            sink_level, fill, L = L, lq, L + 1
    first_pos = np.zeros(J, np.int64)
    first_pos[nh > 0] = hpos[ptr[:-1][nh > 0]]
    lead = np.where(nh > 0, np.minimum(first_pos // 64, blocks - 1), 0)
    depth = np.zeros(J, np.int64)
    cur = fuse.copy()
    while (cur >= 0).any():
        depth += cur >= 0
        cur = np.where(cur >= 0, fuse[np.maximum(cur, 0)], -1)
    order = np.lexsort((np.arange(J), -blocks, level))
    return dict(level=level, n_levels=L, holes=nh, blocks=blocks, fuse=fuse, fused_target=fused_target,
                slot_fused=slot_fused, queueable=queueable, sink=sink, sink_level=sink_level, fill_level=fill,
                lead=lead, first_pos=first_pos, depth=depth, order=order, producer=producer,
                width=np.bincount(level[queueable], minlength=L), jobs_at=np.bincount(level, minlength=L))


# The graphs the GPU tests run (test_gpu_dag_shapes.py); the CPU tests assert
# the mix on every one.  Together their levels hit every width of WIDTHS.
GRAPHS = {
    "sf2": dict(seed=101, widths=WIDTHS, sf=2),
    "sf8": dict(seed=102, widths=(33, 65, 97, 129, 257), sf=8),
    "sf40": dict(seed=103, widths=(32, 64, 96, 128, 256), sf=40),
    "mix": dict(seed=104, widths=(31, 63, 127, 255, 1), sf="mix"),
    "merge2": dict(seed=105, widths=(64, 129, 97), sf=2, merge=True),
    "merge40": dict(seed=106, widths=(65, 128), sf=40, merge=True),
    "sink127": dict(seed=107, widths=(65, 129, 96), sf=2, sinks=127),
    "sink128": dict(seed=108, widths=(64, 128, 97), sf=8, sinks=128),
    "sink129": dict(seed=109, widths=(63, 127, 129), sf="mix", sinks=129),
    "msink127": dict(seed=110, widths=(65, 129), sf=2, sinks=127, merge=True),
    "msink128": dict(seed=111, widths=(64, 128), sf=8, sinks=128, merge=True),
    "msink129": dict(seed=112, widths=(33, 97), sf="mix", sinks=129, merge=True),
    "break": dict(seed=113, widths=(33, 65, 97), sf=2, break_pos2=True),
}
_BUILT = {}


def graph(name):
    """GRAPHS[name] (or "stride"), built once per process; treat as read-only."""
    if name not in _BUILT:
        _BUILT[name] = stride(120) if name == "stride" else ragged(**GRAPHS[name])
    return _BUILT[name]
