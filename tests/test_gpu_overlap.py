"""Consecutive Q8 batches through dbg_agg_step_async on two handles: eight alternating steps over
three different inputs of 2 M rows (ConfigRunner.pipe_step), batch k + 1 enqueued while batch k is
still in flight.  With `dual` the two handles run on two streams (each handle's own) and the
launches share the chip; with `single` they follow each other on one.  Every batch's published result equals the
oracle over that batch's own rows.  Results only: nothing here depends on whether or how far the
launches overlapped."""
import pytest

from databend_amd import workloads
from databend_amd.filter import cmp
from oracle import oracle
from tests.parity import assert_results_equal
from tests.test_gpu_parity import oracle_aggregate

pytestmark = pytest.mark.gpu
CFG, N, COPIES, STEPS = 2, 2_000_000, 3, 8


@pytest.fixture(scope="module")
def expected():
    """The oracle's result of each of the three inputs, computed once."""
    shape = workloads.SHAPES[CFG]
    name, op, const = shape.predicate
    out = []
    for i in range(COPIES):
        cols = oracle.datagen(CFG, N, start=i * N)
        out.append(oracle_aggregate([cols[c] for c in shape.keys], [(f, cols[c] if c else None) for f, c in shape.aggs],
                                    (cmp(0, op, const), [cols[name]]), threads=8))
    return out


@pytest.mark.parametrize("mode", ["dual", "single"])
def test_alternating_steps_match_oracle(expected, mode):
    r = workloads.ConfigRunner(CFG, N, copies=COPIES)
    try:
        r.enable_pipeline(mode)
        assert r.pipe_mode == mode and len(r.tables) == 2
        got = []
        for k in range(STEPS):
            r.pipe_step(k)  # enqueues batch k, then publishes batch k - 1
            if k:
                got.append(r.results_host())
        r.pipe_drain()
        got.append(r.results_host())
        assert len(got) == STEPS
        for k, (keys, aggs) in enumerate(got):
            ok, oa = expected[k % COPIES]
            assert_results_equal(keys, aggs, ok, oa)
    finally:
        r.close()
