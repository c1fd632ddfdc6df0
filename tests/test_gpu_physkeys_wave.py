"""A bottom-up evaluation whose physical keys never leave the device: the
scenarios of tests/wave_cases.py replayed on a target that ignores the key rows
the oracle made for each step.  The finished nodes' values go through marshal ->
unmarshal -> rf_physkeys_set_values_forest, rf_physkeys_update(CONSUMERS) writes
the consumers' rows, and the wave object steps with those rows.  The rows must
equal the oracle's, and states and lists the model's, at every step."""
import numpy as np
import pytest

import physkeys_cases as PC
import plan_model as P
import test_gpu_wave as GW
import wave_cases as C
from reflow_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0, host_threads=0)
    yield c
    c.close()


class DeviceKeys(GW.Both):
    """GW.Both with the key rows kept in HBM and the physical ones made there."""

    def __init__(self, ctx, case):
        super().__init__(ctx, case)
        self.ctx, self.case = ctx, case
        dep_ptr, deps = P.flow_csr(case.nodes)
        key_ptr, _ = P.key_arrays(case.keys())
        self.n_rows = int(key_ptr[-1])
        phys_row = [int(key_ptr[i]) if PC.has_key(f) else PC.NO_ROW for i, f in enumerate(case.nodes)]
        self.pk = capi.PhysKeys(ctx, dep_ptr, deps, phys_row, [PC.suffix_of(f) for f in case.nodes])
        self.physical = [r for r in phys_row if r != PC.NO_ROW]
        self.d_keys = ctx.alloc(32 * max(self.n_rows, 1))
        self.updates = self.written = 0

    def set_values(self, nodes):
        """marshal -> unmarshal -> set_values_forest, all in device memory."""
        if not nodes:
            return
        batch = capi.JsonBatch(self.ctx, [self.case.nodes[i].value for i in nodes])
        arena_bytes = int(((batch.lens() + 15) & ~15).sum())
        f = capi.FilesetForest.from_device(self.ctx, *batch.device()[:1], arena_bytes, *batch.device()[1:], len(nodes))
        try:
            assert f.n_accepted == len(nodes)
            self.pk.set_values_forest(nodes, f)
        finally:
            f.close()
            batch.close()

    def rows(self):
        return self.d_keys.to_numpy(np.uint8, 32 * self.n_rows).reshape(-1, 32)

    def begin(self, roots, keys, no_cache_extern=False):
        C.ModelTarget.begin(self, roots, keys, no_cache_extern)
        want = GW.flat_keys(keys)
        mine = want.copy()
        mine[self.physical] = 0xEE  # the oracle's physical rows are not used
        self.d_keys.copy_from(mine)
        self.set_values([i for i, f in enumerate(self.case.nodes) if f.done and f.value is not None])
        o = self.pk.update(list(range(len(self.case.nodes))), capi.RF_PHYS_SELF, self.d_keys.ptr, self.n_rows)
        assert o.affected == len(self.physical)
        assert (self.rows() == want).all()
        self.w.begin(roots, self.dev, C.KIND, d_keys=self.d_keys.ptr, live=self.dlive, no_cache_extern=no_cache_extern)

    def step(self, finished, keys):
        C.ModelTarget.step(self, finished, keys)
        self.set_values(finished)
        o = self.pk.update(finished, capi.RF_PHYS_CONSUMERS, self.d_keys.ptr, self.n_rows)
        self.updates += 1
        self.written += o.keys_written
        assert (self.rows() == GW.flat_keys(keys)).all()
        self.w.step(finished, self.dev, C.KIND, d_keys=self.d_keys.ptr, live=self.dlive)

    def close(self):
        super().close()
        self.pk.close()
        self.d_keys.free()


@pytest.mark.parametrize("seed,n,with_liveset", C.SEEDS)
def test_bottom_up_with_device_made_keys(ctx, seed, n, with_liveset):
    case = C.Case(seed, n, with_liveset)
    t = DeviceKeys(ctx, case)
    try:
        seen = C.play(case, t)
        assert seen["steps"] >= 2 and t.updates == seen["steps"] and t.written > 0
    finally:
        t.close()
