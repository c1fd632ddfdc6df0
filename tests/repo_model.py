"""CPU restatement of the repository index (rf_repo_*): a dict plus per-group
first-occurrence dedup.  A helper, not a test.

  index: the object map of the in-memory repository
  (test/testutil/repository.go:25-115) and file.Repository.Stat
  (repository/file/repository.go:93-101): ID -> size.  Put is content
  addressed: an ID that is present keeps its size, and a row that gives it
  another one gets RF_EINTEGRITY -- rows apply in index order, so the first
  row of an ID wins.  Remove forgets the ID; a later Put is a fresh object.
  table: slots, tombstones and rebuilds follow the rule of include/reflow_hip.h
  (a rebuild before a Put batch when live + tombstones + rows pass half the
  slots), so that rf_repo_stats can be compared exactly.
  missing (eval.go:1227-1243, 1983-2014) and NeedTransfer
  (repository/manager.go:197-234; eval.go:412-444): per group Files(), the
  distinct (ID, Size) pairs (executor.go:82-92, 116-125), each looked up by ID
  alone as Stat does; the list is by group and, within one, by first
  occurrence.
  Collect (repository/file/repository.go:304-327): every object the liveset
  does not contain goes."""
from __future__ import annotations

import numpy as np

RF_OK, RF_EINVAL, RF_EINTEGRITY, RF_EPRECONDITION = 0, 1, 3, 7
MIN_SLOTS = 1024


def slots_for(capacity: int) -> int:
    s = MIN_SLOTS
    while s < 2 * capacity:
        s *= 2
    return s


def ids_array(ids) -> np.ndarray:
    return np.frombuffer(b"".join(bytes(i) for i in ids), np.uint8).reshape(-1, 32).copy()


class Missing:
    """What one missing / need_transfer call reports."""

    def __init__(self, n_groups):
        self.n_files = np.zeros(n_groups, np.uint32)
        self.n_missing = np.zeros(n_groups, np.uint32)
        self.missing_bytes = np.zeros(n_groups, np.int64)
        self.status = np.zeros(n_groups, np.int32)
        self.miss_ptr = np.zeros(n_groups + 1, np.uint64)
        self.rows, self.ids, self.sizes = [], [], []
        self.n_rows = 0

    @property
    def n_listed(self):
        return len(self.rows)

    @property
    def miss_rows(self):
        return np.array(self.rows, np.uint64)

    @property
    def miss_ids32(self):
        return ids_array(self.ids)

    @property
    def miss_sizes(self):
        return np.array(self.sizes, np.int64)


class Repo:
    def __init__(self, capacity=0):
        self.objs = {}      # ID -> size
        self.tombs = set()  # removed IDs that still hold a slot
        self.slots = slots_for(capacity)
        self.rebuilds = 0
        self.last = (0, 0, 0)  # rows, files, missing of the last missing / need_transfer call

    # ---- the table's bookkeeping ------------------------------------------------
    def _reserve(self, batch):
        if 2 * (len(self.objs) + len(self.tombs) + batch) <= self.slots:
            return
        self.slots *= 2
        while 2 * (len(self.objs) + batch) > self.slots:
            self.slots *= 2
        self.tombs.clear()
        self.rebuilds += 1

    def stats(self):
        return dict(objects=len(self.objs), bytes=sum(self.objs.values()), tombstones=len(self.tombs),
                    capacity=self.slots, rebuilds=self.rebuilds, last_rows=self.last[0], last_files=self.last[1],
                    last_missing=self.last[2])

    # ---- the index --------------------------------------------------------------------
    def put(self, ids, sizes, device_form=False):
        """status per row.  A negative size: None for the whole batch in the
        host form (refused, nothing changes), RF_EINVAL on the row in the device form."""
        ids, sizes = [bytes(i) for i in ids], [int(s) for s in sizes]
        if not device_form and any(s < 0 for s in sizes):
            return None
        self._reserve(len(ids))
        out = []
        for i, s in zip(ids, sizes):
            if s < 0:
                out.append(RF_EINVAL)
            elif i in self.objs:
                out.append(RF_OK if self.objs[i] == s else RF_EINTEGRITY)
            else:
                self.objs[i] = s
                self.tombs.discard(i)
                out.append(RF_OK)
        return np.array(out, np.int32)

    def remove(self, ids):
        out = []
        for i in (bytes(i) for i in ids):
            out.append(1 if i in self.objs else 0)
            if i in self.objs:
                del self.objs[i]
                self.tombs.add(i)
        return np.array(out, np.uint8)

    def stat(self, ids):
        return np.array([self.objs.get(bytes(i), -1) for i in ids], np.int64)

    def collect(self, contains=None):
        """contains: ID -> bool (the liveset), None: a nil liveset.  (objects removed, their bytes)."""
        dead = [i for i in self.objs if contains is None or not contains(i)]
        gone = sum(self.objs[i] for i in dead)
        for i in dead:
            del self.objs[i]
            self.tombs.add(i)
        return len(dead), gone

    # ---- missing / need_transfer ------------------------------------------------------
    def missing(self, groups, status=None) -> Missing:
        """groups: per group its (ID, Size) rows; status: per group a status other
        than RF_OK empties the group (need_transfer)."""
        m = Missing(len(groups))
        row = 0
        for g, rows in enumerate(groups):
            if status is not None and status[g] != RF_OK:
                m.status[g] = status[g]
                rows = []
            seen = set()
            for fid, size in rows:
                f = (bytes(fid), int(size))
                if f not in seen:
                    seen.add(f)
                    m.n_files[g] += 1
                    if f[0] not in self.objs:  # existence is by ID alone, as Stat
                        m.n_missing[g] += 1
                        m.missing_bytes[g] += f[1]
                        m.rows.append(row)
                        m.ids.append(f[0])
                        m.sizes.append(f[1])
                row += 1
            m.miss_ptr[g + 1] = len(m.rows)
        m.n_rows = row
        self.last = (row, int(m.n_files.sum()), len(m.rows))
        return m

    def need_transfer(self, edge_ptr, edges, values, nodes) -> Missing:
        """values: node -> rows, absent = no value.  Group g = the value rows of
        nodes[g]'s edges, in edge order (an edge listed twice contributes twice);
        an edge without a value: RF_EPRECONDITION and an empty group."""
        groups, status = [], []
        for v in nodes:
            deps = [int(d) for d in edges[int(edge_ptr[v]):int(edge_ptr[v + 1])]]
            ok = all(d in values for d in deps)
            status.append(RF_OK if ok else RF_EPRECONDITION)
            groups.append([r for d in deps for r in values[d]] if ok else [])
        return self.missing(groups, status)


def flatten(groups):
    """(counts uint32, ids uint8 [rows, 32], sizes int64) as rf_repo_missing takes them."""
    counts = np.array([len(g) for g in groups], np.uint32)
    rows = [r for g in groups for r in g]
    return counts, ids_array([r[0] for r in rows]), np.array([r[1] for r in rows], np.int64)
