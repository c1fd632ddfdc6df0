"""The repository index's CPU model (tests/repo_model.py) on hand-written
cases: TestCacheLookupMissing's shape (test/evaltest/eval_test.go:279-312),
Put's first-wins rule, tombstones and the growth rule, duplicates inside and
across groups, one ID with two sizes, NeedTransfer's groups and Collect."""
import hashlib

import numpy as np

import repo_model as R


def sha(s: str) -> bytes:
    return hashlib.sha256(s.encode()).digest()


def test_cache_lookup_missing_shape():
    """The cached value holds x, y, z (IDs = SHA-256 of the names, size 1); x is
    deleted from the repository: lookup finds 1 missing file of 1 byte."""
    repo = R.Repo()
    value = [(sha(n), 1) for n in ("x", "y", "z")]
    assert repo.put([f[0] for f in value], [f[1] for f in value]).tolist() == [R.RF_OK] * 3
    m = repo.missing([value])
    assert (m.n_files.tolist(), m.n_missing.tolist(), m.missing_bytes.tolist(), m.n_listed) == ([3], [0], [0], 0)
    assert repo.remove([sha("x")]).tolist() == [1]
    m = repo.missing([value])
    assert (m.n_files.tolist(), m.n_missing.tolist(), m.missing_bytes.tolist()) == ([3], [1], [1])
    assert m.miss_ptr.tolist() == [0, 1] and m.rows == [0] and m.ids == [sha("x")] and m.sizes == [1]
    assert repo.stat([sha("x"), sha("y")]).tolist() == [-1, 1]
    assert repo.stats()["tombstones"] == 1 and repo.last == (3, 3, 1)


def test_put_first_wins_and_reput():
    repo = R.Repo()
    a, b, c = sha("a"), sha("b"), sha("c")
    assert repo.put([a, a, a, b], [5, 5, 6, 1]).tolist() == [R.RF_OK, R.RF_OK, R.RF_EINTEGRITY, R.RF_OK]
    assert repo.stat([a, b, c]).tolist() == [5, 1, -1]
    assert repo.put([a, a], [6, 5]).tolist() == [R.RF_EINTEGRITY, R.RF_OK]  # the index's size stays
    assert repo.stat([a]).tolist() == [5]
    assert repo.remove([a, a, c]).tolist() == [1, 0, 0]
    assert repo.put([a, a], [9, 5]).tolist() == [R.RF_OK, R.RF_EINTEGRITY]  # a fresh object of any size
    assert repo.stat([a]).tolist() == [9] and repo.stats()["tombstones"] == 0
    # a negative size: the host form refuses the batch, the device form the row
    assert repo.put([c, b], [-1, 1]) is None and repo.stat([c]).tolist() == [-1]
    assert repo.put([c, c, c], [-1, 3, 4], device_form=True).tolist() == [R.RF_EINVAL, R.RF_OK, R.RF_EINTEGRITY]
    assert repo.stats()["objects"] == 3 and repo.stats()["bytes"] == 9 + 1 + 3


def test_growth_rule():
    assert [R.slots_for(c) for c in (0, 512, 513, 1024)] == [1024, 1024, 2048, 2048]
    repo = R.Repo()
    ids = [sha("o%d" % i) for i in range(700)]
    repo.put(ids[:512], [1] * 512)
    assert (repo.slots, repo.rebuilds) == (1024, 0)  # exactly half the slots: no growth
    repo.remove(ids[:10])
    assert repo.stats()["tombstones"] == 10
    repo.put(ids[512:513], [1])  # 502 live + 10 tombstones + 1 row pass half
    assert (repo.slots, repo.rebuilds, repo.stats()["tombstones"]) == (2048, 1, 0)
    repo.put(ids[513:] + ids[:10] + [sha("more%d" % i) for i in range(5000)], [1] * (187 + 10 + 5000))
    assert (repo.slots, repo.rebuilds) == (16384, 2) and repo.stats()["objects"] == 5700


def test_duplicates_inside_and_across_groups():
    repo = R.Repo()
    a, b, c = sha("a"), sha("b"), sha("c")
    repo.put([b], [2])
    groups = [[(a, 1), (b, 2), (a, 1), (a, 1)],  # a three times in one group: one file
              [],
              [(a, 1), (c, 3), (c, 4), (c, 3)],  # a again: counted in both groups; c with two sizes: two files
              [(b, 2), (b, 7)]]                  # b is present whatever size a row states
    m = repo.missing(groups)
    assert m.n_files.tolist() == [2, 0, 3, 2]
    assert m.n_missing.tolist() == [1, 0, 3, 0]
    assert m.missing_bytes.tolist() == [1, 0, 8, 0]
    assert m.miss_ptr.tolist() == [0, 1, 1, 4, 4]
    assert m.rows == [0, 4, 5, 6] and m.ids == [a, a, c, c] and m.sizes == [1, 1, 3, 4]
    assert repo.last == (10, 7, 4)
    counts, ids, sizes = R.flatten(groups)
    assert counts.tolist() == [4, 0, 4, 2] and ids.shape == (10, 32) and sizes.tolist() == [1, 2, 1, 1, 1, 3, 4, 3, 2, 7]
    empty = repo.missing([])
    assert empty.miss_ptr.tolist() == [0] and empty.n_listed == 0


def test_need_transfer_groups():
    """Node 0 reads nodes 1 and 2 (2 twice); node 3 reads node 4, which has no value."""
    repo = R.Repo()
    a, b, c = sha("a"), sha("b"), sha("c")
    repo.put([a], [1])
    edge_ptr, edges = np.array([0, 3, 3, 3, 4, 4], np.uint64), np.array([1, 2, 2, 4], np.uint32)
    values = {1: [(a, 1), (b, 2)], 2: [(b, 2), (c, 3)]}
    m = repo.need_transfer(edge_ptr, edges, values, [0, 3, 1, 0])
    assert m.status.tolist() == [R.RF_OK, R.RF_EPRECONDITION, R.RF_OK, R.RF_OK]
    assert m.n_files.tolist() == [3, 0, 0, 3] and m.n_missing.tolist() == [2, 0, 0, 2]
    assert m.missing_bytes.tolist() == [5, 0, 0, 5] and m.ids == [b, c, b, c] and m.n_rows == 12
    values[2] = [(a, 1)]  # the value replaced between two calls
    m = repo.need_transfer(edge_ptr, edges, values, [0])
    assert (m.n_files.tolist(), m.n_missing.tolist(), m.ids) == ([2], [1], [b])


def test_collect():
    repo = R.Repo()
    ids = [sha("o%d" % i) for i in range(10)]
    repo.put(ids, list(range(10)))
    live = set(ids[::2])
    assert repo.collect(lambda i: i in live) == (5, 1 + 3 + 5 + 7 + 9)
    assert repo.stat(ids).tolist() == [0, -1, 2, -1, 4, -1, 6, -1, 8, -1] and repo.stats()["tombstones"] == 5
    assert repo.collect(None) == (5, 20) and repo.stats()["objects"] == 0
