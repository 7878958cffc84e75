"""The hand-offs of the tagged fused chain (agg.hip fused_chain_tagged: COUNT(*) over a key of
<= 16 bits, one fused insert + finalize launch per step): every workgroup parks its table, takes a
ticket and loads its siblings' rows in one round trip, the last arrival of each level merges what
it holds and the last leader finalizes from its own LDS table — or, when something outlives the
launch, from a view of the HBM table.  Checked against numpy.unique, every group of every step:

* every grid shape the two-level tree has (one group, a partial group, a second group of one, a
  partial last group, the full 256 workgroups, a scalar tail), Int16, Int8 and UInt16 keys;
* uneven load: workgroups that select nothing, hold one group, 64 groups (a full parked row) or
  65-300 groups (flushed into the HBM table, so the launch finalizes from the view);
* rows left in the scratch by larger earlier launches of the same handle;
* 80 consecutive launches on a fresh handle, which cross the wrap of both tags;
* tables that outlive the finalize (no recycle, output buffers too short on the first try) next to
  launches that meet the direct finalize's conditions, and the step after them.

Only results are checked: no test observes which finalize a launch took (both give the same
groups), so where a comment names a path it states what the kernel's conditions select for that
input, not something the test verifies.

An Int16 workgroup covers 8 x 1024 x 2 = 16384 rows (16-byte vectors, 1024 threads, two vectors
per thread and grid round) and the grid is capped at 256 workgroups; chunk c of 8192 rows is
streamed by workgroup c % grid."""
import numpy as np
import pytest

from databend_amd import column as col
from databend_amd.column import Column
from databend_amd.ffi import check, lib
from tests.test_gpu_fused_count_small_keys import FusedRunner

pytestmark = pytest.mark.gpu

WG16 = 16384  # Int16 rows per workgroup below the grid cap
GRIDS = [(2, WG16 + 1), (16, 16 * WG16), (17, 16 * WG16 + 1), (33, 32 * WG16 + 1), (255, 254 * WG16 + 1),
         (256, 256 * WG16), (256, 256 * WG16 + 1)]


def reference(vals, pred_ne=None):
    v = vals if pred_ne is None else vals[vals != pred_ne]
    return np.unique(v, return_counts=True)


def check_step(r, t, vals, pred_ne=0, ref=None):
    key = Column.from_numbers(t, vals.astype(t.np_dtype))
    gk, ga = r.step(key, ("<>", pred_ne) if pred_ne is not None else None)
    ek, ec = ref if ref is not None else reference(vals.astype(t.np_dtype), pred_ne)
    k = np.asarray(gk[0].data).view(t.np_dtype)
    c = np.asarray(ga[0].data).view(np.uint64)
    order = np.argsort(k, kind="stable")
    assert len(k) == len(ek), f"group count differs: got {len(k)} expected {len(ek)}"
    np.testing.assert_array_equal(k[order], ek)
    np.testing.assert_array_equal(c[order], ec.astype(np.uint64))


def random_keys(rng, n, lo, hi, distinct, must_have=()):
    pool = rng.integers(lo, hi, distinct)
    pool[0] = 0
    for i, v in enumerate(must_have):
        pool[1 + i] = v
    return np.where(rng.random(n) < 0.6, 0, pool[rng.integers(0, distinct, n)])


@pytest.mark.parametrize("grid,rows", GRIDS, ids=[f"wg{g}_rows{n}" for g, n in GRIDS])
def test_grid_shapes_int16(grid, rows):
    rng = np.random.default_rng(grid * 1000003 + rows)
    r = FusedRunner(col.Int16)
    try:
        for _ in range(2):  # the second launch finds the first one's rows in the scratch
            check_step(r, col.Int16, random_keys(rng, rows, -32768, 32768, 33, must_have=(-32768, 32767, -1)))
    finally:
        r.close()


def test_int8_keys():
    """An Int8 workgroup covers 32768 rows: 17, 2 and 40 workgroups over 30 keys with both ends of
    the range, then every key value in every workgroup (256 groups each: all of them flush)."""
    rng = np.random.default_rng(8)
    r = FusedRunner(col.Int8)
    try:
        for rows in (16 * 32768 + 1, 2 * 32768, 40 * 32768 + 5):
            check_step(r, col.Int8, random_keys(rng, rows, -128, 128, 30, must_have=(-128, 127, -1)))
        check_step(r, col.Int8, rng.integers(-128, 128, 40 * 32768 + 5))
    finally:
        r.close()


def test_uint16_all_ones_key():
    rng = np.random.default_rng(16)
    r = FusedRunner(col.UInt16)
    try:
        for grid, rows in ((33, 32 * WG16 + 1), (256, 256 * WG16 + 1)):
            vals = random_keys(rng, rows, 0, 65536, 40, must_have=(65535, 65534, 1))
            vals[-1] = 65535  # the scalar tail's row carries it too
            check_step(r, col.UInt16, vals)
    finally:
        r.close()


def uneven_column(grid, rows):
    """Keys by workgroup: workgroup w streams the 8192-row chunks c with c % grid == w (and
    workgroup 0 the scalar tail).  By w % 4: nothing selected (all rows equal the `<>` constant
    0), exactly one group, 64 distinct keys, 65-300 distinct keys.  Pools of different workgroups
    overlap, so every level of the merge adds counts of one key from several rows."""
    i = np.arange(rows, dtype=np.int64)
    chunk = i // 8192
    wg = chunk % grid
    wg[(rows // 8) * 8:] = 0
    cls = wg % 4
    n_keys = np.select([cls == 0, cls == 1, cls == 2], [1, 1, 64], default=65 + (wg * 37) % 236)
    base = np.where(cls == 0, 0, 1 + (wg * 29) % 400)
    # consecutive rows of a chunk walk the workgroup's pool, so all of it is present
    vals = np.where(cls == 0, 0, base + (i % n_keys))
    # the same load without a table that has to be flushed, at any level: one pool of 64 keys
    light = np.select([cls == 0, cls == 1], [0, 500 + wg % 64], default=500 + i % 64)
    return (vals - 200).astype(np.int16), (light - 200).astype(np.int16), cls


@pytest.mark.parametrize("grid,rows", [(17, 16 * WG16 + 1), (256, 256 * WG16 + 1)], ids=["wg17", "wg256"])
def test_uneven_load(grid, rows):
    vals, light, cls = uneven_column(grid, rows)
    assert set(np.unique(cls)) == {0, 1, 2, 3}
    r = FusedRunner(col.Int16)
    try:
        # -200 is what the idle workgroups hold: the predicate drops all of their rows
        check_step(r, col.Int16, vals, pred_ne=-200)
        # the same handle without a flushing workgroup (the load the direct finalize is meant for)
        check_step(r, col.Int16, light, pred_ne=-200)
        check_step(r, col.Int16, vals, pred_ne=-200)
    finally:
        r.close()


def test_stale_rows_of_larger_launches():
    """Grid 256, 2, 17, 256 on one handle, each with its own key pool and counts, ten times: the
    scratch rows always hold well-formed words of larger earlier launches."""
    rng = np.random.default_rng(77)
    steps = []
    for rows, distinct, lo in ((256 * WG16 + 1, 60, -3000), (WG16 + 1, 9, 100), (16 * WG16 + 1, 33, -50), (256 * WG16, 64, 2000)):
        vals = random_keys(rng, rows, lo, lo + 500, distinct).astype(np.int16)
        steps.append((vals, reference(vals, 0)))
    r = FusedRunner(col.Int16)
    try:
        for _ in range(10):
            for vals, ref in steps:
                check_step(r, col.Int16, vals, ref=ref)
    finally:
        r.close()


def test_tag_wrap_on_a_fresh_handle():
    """80 consecutive launches of 2 and 17 workgroups, alternating, every one checked: whatever
    sequence number a handle starts from, the run must be exact; a handle starts 32 finalizes
    below the wrap of both tags, so this run crosses them."""
    rng = np.random.default_rng(2024)
    cols = []
    for j in range(8):
        rows = WG16 + 1 if j % 2 == 0 else 16 * WG16 + 1
        vals = random_keys(rng, rows, -400 + 50 * j, 400 + 50 * j, 20 + 5 * j).astype(np.int16)
        cols.append((vals, reference(vals, 0)))
    r = FusedRunner(col.Int16)
    try:
        for step in range(80):
            vals, ref = cols[step % 8]
            check_step(r, col.Int16, vals, ref=ref)
    finally:
        r.close()


@pytest.mark.parametrize("grid,rows", GRIDS, ids=[f"wg{g}_rows{n}" for g, n in GRIDS])
def test_table_kept_without_recycle(grid, rows):
    """Recycle off: the table outlives every finalize (the kernel's condition for the view and its
    write-back); then recycle on again on the same handle."""
    rng = np.random.default_rng(300 + grid)
    r = FusedRunner(col.Int16)
    try:
        check(lib().dbg_agg_set_recycle(r.table.h, 0))
        for _ in range(2):
            check_step(r, col.Int16, random_keys(rng, rows, -1000, 1000, 50))
        check(lib().dbg_agg_set_recycle(r.table.h, 1))
        for _ in range(2):
            check_step(r, col.Int16, random_keys(rng, rows, -1000, 1000, 50))
    finally:
        r.close()


@pytest.mark.parametrize("grid,rows", GRIDS, ids=[f"wg{g}_rows{n}" for g, n in GRIDS])
def test_output_buffers_too_short_first(grid, rows):
    """Result buffers for 4 groups against ~50: the fused launch keeps the table, the runner
    finalizes again with larger ones; the step after it is exact too."""
    rng = np.random.default_rng(400 + grid)
    r = FusedRunner(col.Int16)
    try:
        for _ in range(2):
            r.cap = 4
            check_step(r, col.Int16, random_keys(rng, rows, -1000, 1000, 50))
            assert r.cap > 4
            check_step(r, col.Int16, random_keys(rng, rows, -1000, 1000, 50))
    finally:
        r.close()
