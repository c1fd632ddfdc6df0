"""K1: every SHA-256 kernel form at its own block, chunk and group edges.

k1_sha.hip has five GPU forms behind rf_sha_plan_run (duo, solo, octo, pair,
lanes) plus the host leg; each has its own producer, LDS double buffer and
tail handling.  Every test here forces one form (or one planner threshold)
with the RF_SHA_* flags and compares byte for byte with hashlib.sha256 over
bytes made on the host and uploaded: no rf_gen_fill, no oracle, so the
reference shares no code with the library.  The arena is random everywhere
(gaps included), so a tail guard that reads one chunk too many or too few
changes the digest.

Which kernel a flag set selects (capi.cpp: gpu_model puts every message on the
wave-per-message leg under RF_SHA_ALL_SOLO and none under RF_SHA_NO_SOLO;
plan_setup: p->duo = !ONE_LANE_CHAIN, p->pair = !NO_PAIR && n_lanes <=
64*n_cu, p->octo = !NO_OCTO && n_lanes <= 16*n_cu; plan_run_locked launches
octo before pair before lanes), for the 190-message matrix and any n_cu >= 12
(the MI355X has 256):
  ALL_SOLO                      k1_sha256_duo   (n_solo = n)
  ALL_SOLO|ONE_LANE_CHAIN       k1_sha256_solo  (n_solo = n)
  NO_SOLO                       k1_sha256_octo  (n_lanes = 190 <= 16*n_cu)
  NO_SOLO|NO_OCTO               k1_sha256_pair  (n_lanes = 190 <= 64*n_cu)
  NO_SOLO|NO_OCTO|NO_PAIR       k1_sha256_lanes
  ALL_HOST                      the host leg    (plan_split: h = n)
RF_SHA_NO_HOST zeroes the host model's threads, so no message leaves the GPU.
"""
import hashlib
import random

import numpy as np
import pytest

NO_SOLO, ALL_SOLO, ONE_LANE, NO_PAIR, NO_OCTO, ALL_HOST, NO_HOST = 1, 2, 4, 8, 16, 32, 64
SENTINEL = 0xA5

MATRIX_K = [0, 1, 2, 6, 7, 8, 9, 14, 15, 16, 17, 62, 63, 64, 65, 126, 127, 128, 129]
MATRIX_R = [0, 1, 15, 16, 17, 54, 55, 56, 57, 63]
MATRIX_LENS = [64 * k + r for k in MATRIX_K for r in MATRIX_R]


def nblocks(n):
    return (n + 9 + 63) // 64


class MsgSet:
    """Messages laid out in one random host arena.  align='cycle': message i
    sits at the next 16-aligned offset whose residue mod 64 is 16*(i%4);
    align='pack': at the next 16-aligned offset."""

    def __init__(self, lens, seed, align="cycle", same_content=False):
        self.lens = [int(n) for n in lens]
        offs, pos = [], 0
        for i, n in enumerate(self.lens):
            if align == "cycle":
                pos += (16 * (i % 4) - pos) % 64
            offs.append(pos)
            pos += (n + 15) // 16 * 16
        self.offs = offs
        size = max(pos, 16)
        self.arena = np.random.default_rng(seed).integers(0, 256, size=size, dtype=np.uint8)
        if same_content:
            assert len(set(self.lens)) == 1
            n = self.lens[0]
            for o in offs[1:]:
                self.arena[o:o + n] = self.arena[offs[0]:offs[0] + n]
        mv = memoryview(self.arena)
        self.want = [hashlib.sha256(mv[o:o + n]).digest() for o, n in zip(offs, self.lens)]
        self._dev = {}  # context -> uploaded arena, shared with every view()

    def device_arena(self, ctx):
        if id(ctx) not in self._dev:
            self._dev[id(ctx)] = ctx.upload(self.arena)
        return self._dev[id(ctx)]

    def release(self):
        while self._dev:
            self._dev.popitem()[1].free()

    def view(self, idx):
        """The same arena with the messages listed in another order (or a subset)."""
        v = object.__new__(MsgSet)
        v.arena, v._dev = self.arena, self._dev
        v.lens = [self.lens[i] for i in idx]
        v.offs = [self.offs[i] for i in idx]
        v.want = [self.want[i] for i in idx]
        return v


def run_plan(ctx, ms, flags, n_solo=None, n_host=0):
    """Plan + run ms under `flags` into rows 1..n of an (n+2)-row output filled
    with SENTINEL; asserts the guard rows, the stats and every digest, and
    returns the n x 32 output."""
    n = len(ms.lens)
    offs = np.array(ms.offs, dtype=np.uint64)
    lens = np.array(ms.lens, dtype=np.uint64)
    d_arena = ms.device_arena(ctx)
    d_out = ctx.alloc((n + 2) * 32)
    plan = None
    try:
        d_out.fill(SENTINEL)
        plan = ctx.sha_plan(offs, lens, flags)
        plan.run(d_arena.ptr, d_out.ptr + 32)
        ctx.sync()
        st = plan.stats()
        out = d_out.to_numpy().reshape(n + 2, 32)
    finally:
        if plan is not None:
            plan.close()
        d_out.free()
    nbs = [nblocks(x) for x in ms.lens]
    assert st.n_msgs == n
    assert st.total_blocks == sum(nbs)
    assert st.max_blocks == max(nbs)
    assert st.total_bytes == sum(ms.lens)
    assert st.n_host == n_host
    if n_solo is not None:
        assert st.n_solo == n_solo
    got = out[1:n + 1]
    want = np.frombuffer(b"".join(ms.want), dtype=np.uint8).reshape(n, 32)
    bad = np.flatnonzero((got != want).any(axis=1))
    if len(bad):
        # position in the planner's largest-first (stable) order of the whole set
        pos = {i: q for q, i in enumerate(sorted(range(n), key=lambda i: -nbs[i]))}
        rows = ["flags=%d i=%d len=%d nb=%d off%%64=%d sorted_pos=%d%s" %
                (flags, i, ms.lens[i], nbs[i], ms.offs[i] % 64, pos[i],
                 " (row unwritten)" if (got[i] == SENTINEL).all() else "")
                for i in bad[:12]]
        pytest.fail("%d of %d digests differ from hashlib:\n  %s" % (len(bad), n, "\n  ".join(rows)))
    assert (out[0] == SENTINEL).all(), "stray write into the row before the output (flags=%d)" % flags
    assert (out[n + 1] == SENTINEL).all(), "stray write into the row after the output (flags=%d)" % flags
    return got


@pytest.fixture(scope="module")
def ctx():
    from reflow_amd import capi
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def matrix():
    ms = MsgSet(MATRIX_LENS, seed=0xF0)
    yield ms
    ms.release()


def run_once(ctx, ms, flags, **kw):
    try:
        return run_plan(ctx, ms, flags, **kw)
    finally:
        ms.release()


# --------------------------------------------------------------- CPU ----
def test_oracle_sha256_matches_hashlib_on_matrix(oracle):
    """The oracle every other K1 test trusts, against hashlib, at the matrix lengths."""
    ms = MsgSet(MATRIX_LENS, seed=0xF1)
    for o, n, want in zip(ms.offs, ms.lens, ms.want):
        assert oracle.sha256(ms.arena[o:o + n].tobytes()) == want, n


def test_matrix_layout():
    """The layout the GPU tests rely on: 190 lengths, 16-aligned offsets over
    all four residues mod 64, no overlap, 4087 B = 64 blocks and 4088 B = 65."""
    ms = MsgSet(MATRIX_LENS, seed=0xF0)
    assert len(ms.lens) == 190 and max(ms.lens) == 64 * 129 + 63
    assert {o % 64 for o in ms.offs} == {0, 16, 32, 48}
    assert all(o % 16 == 0 for o in ms.offs)
    assert all(a + n <= b for a, n, b in zip(ms.offs, ms.lens, ms.offs[1:]))
    assert ms.offs[-1] + ms.lens[-1] <= len(ms.arena)
    assert nblocks(4087) == 64 and nblocks(4088) == 65
    for nb in (63, 64, 65, 127, 128, 129):
        assert nb in {nblocks(x) for x in ms.lens}


# ------------------------------------------------ 1. block x tail matrix --
FORMS = [("duo", ALL_SOLO, True), ("solo", ALL_SOLO | ONE_LANE, True), ("octo", NO_SOLO, False),
         ("pair", NO_SOLO | NO_OCTO, False), ("lanes", NO_SOLO | NO_OCTO | NO_PAIR, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,flags,solo", FORMS, ids=[f[0] for f in FORMS])
def test_matrix_per_form(ctx, matrix, form, flags, solo):
    """k in {0..129 at the 8- and 64-block chunk edges} x r in {tail edges},
    on the one kernel the flags select (module docstring)."""
    assert 190 <= 16 * ctx.n_cu()  # the set is octo-sized (and so pair-sized) on this device
    run_plan(ctx, matrix, flags | NO_HOST, n_solo=len(matrix.lens) if solo else 0)


# load_block / load_raw fetch a tail block in four 16-B chunks, chunk c only if
# rem > 16*c.  The matrix tails cover c = 0 and 1 (r = 0/1, 16/17); these cover
# c = 2 and 3 (r = 32/33, 48/49) and the byte before each.
GUARD_LENS = [64 * k + r for k in (0, 1, 8) for r in (31, 32, 33, 47, 48, 49)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,flags,solo", FORMS, ids=[f[0] for f in FORMS])
def test_tail_chunk_guards_per_form(ctx, form, flags, solo):
    run_once(ctx, MsgSet(GUARD_LENS, seed=0xF2), flags | NO_HOST, n_solo=len(GUARD_LENS) if solo else 0)


@pytest.mark.gpu
def test_matrix_host_leg(matrix):
    """RF_SHA_ALL_HOST: every message through the D2H chunks and the SHA-NI threads."""
    from reflow_amd import capi
    c = capi.Context(0, host_threads=2)
    try:
        threads, _, ext = c.host_info()
        if not ext or threads == 0:
            pytest.skip("no x86 SHA extensions or no host threads: the host leg is off")
        run_plan(c, matrix, ALL_HOST, n_solo=0, n_host=len(matrix.lens))
    finally:
        matrix.release()  # the arena copy belongs to this context
        c.close()


# ---------------------------------------------- 2. octo group composition --
def _len_for(nb, r):
    """A length with nb blocks whose last data block holds r bytes (r <= 55),
    or for r > 55 the length 64*(nb-2) + r whose padding spills into block nb."""
    return 64 * (nb - 1) + r if r <= 55 else 64 * (nb - 2) + r


OCTO_SETS = {
    # one wave, members finishing at different blocks; the two nb = 1 members
    # hash unwritten rows for 16 blocks after their digest is taken
    "mixed_nb": [_len_for(17, 1), _len_for(16, 55), _len_for(9, 0), _len_for(8, 17), _len_for(8, 63),
                 _len_for(7, 16), 0, 55],
    # equal nb (several tie for the longest), tails 0/55/56/63
    "equal_nb9": [64 * 8 + 0, 64 * 8 + 55, 64 * 7 + 56, 64 * 7 + 63] * 2,
    "equal_nb8": [64 * 7 + 0, 64 * 7 + 55, 64 * 6 + 56, 64 * 6 + 63] * 2,
    "equal_nb16": [64 * 15 + 0, 64 * 15 + 55, 64 * 14 + 56, 64 * 14 + 63] * 2,
    "two_members": [64 * 16 + 56, 1],
    "two_equal": [64 * 8 + 55, 64 * 8 + 55],
}
for _n in (1, 7, 8, 9, 15, 16, 17):
    # n_order = _n: full and partial last groups, nb from 1 to 18 within a group
    OCTO_SETS["n_order_%d" % _n] = [(64 * (17 - i) + MATRIX_R[i % 10]) if i % 3 else MATRIX_R[i % 10]
                                    for i in range(_n)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(OCTO_SETS))
def test_octo_group_composition(ctx, name):
    lens = OCTO_SETS[name]
    if name.startswith("equal_nb"):
        assert len({nblocks(x) for x in lens}) == 1
    if name == "mixed_nb":
        assert sorted((nblocks(x) for x in lens), reverse=True) == [17, 16, 9, 8, 8, 7, 1, 1]
    assert len(lens) <= 16 * ctx.n_cu()
    run_once(ctx, MsgSet(lens, seed=len(name) * 131 + len(lens)), NO_SOLO | NO_HOST, n_solo=0)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [55, 64 * 8 + 56])
def test_octo_all_ties_identical_content(ctx, length):
    """64 copies of one message: every sort key ties, and every row must come out the same."""
    ms = MsgSet([length] * 64, seed=7, same_content=True)
    assert len(set(ms.want)) == 1
    got = run_once(ctx, ms, NO_SOLO | NO_HOST, n_solo=0)
    assert (got == got[0]).all()


# ------------------------------------------- 3. pair workgroup composition --
PAIR_SETS = {
    # sorted largest-first: one full 64-lane workgroup with nb = 17 .. 1 mixed
    # (tails r = 1, 16, 17 among them), then a one-message workgroup
    "mixed_65": [64 * ((16 * i) // 64) + [1, 16, 17, 0, 15, 54, 55, 63][i % 8] for i in range(64)] + [0],
    "empty_64": [0] * 64,
    "same_63": [64 * 2 + 17] * 63,
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PAIR_SETS))
def test_pair_workgroup_composition(ctx, name):
    lens = PAIR_SETS[name]
    if name == "mixed_65":
        nbs = sorted(nblocks(x) for x in lens)
        assert len(lens) == 65 and nbs[0] == 1 and nbs[-1] == 17
    run_once(ctx, MsgSet(lens, seed=len(name) * 17 + len(lens)), NO_SOLO | NO_OCTO | NO_HOST, n_solo=0)


# ----------------------------------------------------- 4. form thresholds --
@pytest.mark.gpu
def test_form_thresholds(ctx):
    """16*n_cu messages are the last set on octo, 16*n_cu+1 the first on pair,
    64*n_cu the last on pair, 64*n_cu+1 the first on lanes (plan_setup's
    p->octo / p->pair).  One arena; each run takes a prefix of it."""
    n_cu = ctx.n_cu()
    cyc = MATRIX_R + [64 + r for r in MATRIX_R] + [128, 129, 130]
    full = MsgSet([cyc[i % len(cyc)] for i in range(64 * n_cu + 1)], seed=0xC0)
    first = None
    try:
        for n in (16 * n_cu, 16 * n_cu + 1, 64 * n_cu, 64 * n_cu + 1):
            got = run_plan(ctx, full.view(range(n)), NO_SOLO | NO_HOST, n_solo=0)
            if first is None:
                first = got.copy()
            assert (got[:len(first)] == first).all(), "a message's digest changed with the form (n=%d)" % n
    finally:
        full.release()


# -------------------------------------------------------- 5. lanes refetch --
@pytest.mark.gpu
def test_lanes_refetch(ctx):
    """More messages than the persistent lanes grid has lanes (5*n_cu blocks
    of 256), so lanes finish a message and pull another through wave_fetch,
    re-initialising state, block counter, pointer and length."""
    n = 5 * ctx.n_cu() * 256 + 70_000
    cyc = [0, 1, 55, 56, 63, 64, 119, 120, 200]
    ms = MsgSet([cyc[i % 9] for i in range(n)], seed=0x1A, align="pack")
    assert len(ms.arena) < 40_000_000
    run_once(ctx, ms, NO_SOLO | NO_OCTO | NO_PAIR | NO_HOST, n_solo=0)


# ---------------------------------------------------------- 6. permutation --
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_matrix_permuted_default_planner(ctx, matrix, order):
    """The planner's own mix (duo for the largest, a lane form for the rest):
    each message's digest follows the message through order[] / ids[]."""
    idx = list(range(len(matrix.lens)))
    if order == "reversed":
        idx.reverse()
    else:
        random.Random(5).shuffle(idx)
    run_plan(ctx, matrix.view(idx), NO_HOST)
