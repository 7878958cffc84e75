"""The device ORDER BY ... LIMIT (csrc/sort.hip) on the case table of tests/sort_cases.py: the row
indices of dbg_sort_limit_indices and dbg_sort_limit_multi against the reference by definition
(tests/sort_ref.py), exactly.  Only this build runs the kernels: the histogram, AND/OR and select
passes per level, the composite key read word by word from the columns, the two bitonic sorts.
tests/test_sort_cases.py pins the same table on the CPU and says which case reaches which path; a
mismatch here names the case, the first differing position and the predicted path.

Every single-column case also goes through dbg_sort_limit_multi with one column: both entry points
must agree.  The block-level test runs databend_amd.sort.sort with payload columns of every kind."""
import ctypes as C

import numpy as np
import pytest

from databend_amd import abi
from databend_amd.column import Column, pack_bits
from databend_amd.ffi import Unsupported, check, lib
from tests import sort_cases as sc
from tests import sort_ref

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in sc.cases()]


def _torch():
    import torch
    return torch


class DevCol:
    """A host Column in HBM as a dbg_column, its validity bitmap starting `voff` bits in and (for
    Boolean) its values `doff` bits in; the bits before them are set, so reading from bit 0 would
    show."""

    def __init__(self, c: Column, voff: int = 0, doff: int = 0):
        torch = _torch()
        self.dtype, self.length = c.dtype, len(c)
        if c.dtype.type_id == abi.BOOLEAN:
            data = pack_bits(np.concatenate([np.ones(doff, bool), np.asarray(c.data, bool)]))
        else:
            data = np.ascontiguousarray(c.data).view(np.uint8)
            doff = 0
        self.data = torch.from_numpy(np.concatenate([data, np.zeros(8, np.uint8)])).cuda()  # never empty
        self.offsets = torch.from_numpy(c.offsets.astype(np.uint64).view(np.int64).copy()).cuda() if c.offsets is not None else None
        self.validity = None
        if c.validity is not None and c.dtype.nullable:
            self.validity = torch.from_numpy(pack_bits(np.concatenate([np.ones(voff, bool), np.asarray(c.validity, bool)]))).cuda()
        else:
            voff = 0
        self.voff, self.doff = voff, doff

    def to_abi(self) -> abi.dbg_column:
        d = abi.dbg_column()
        d.dt = self.dtype.to_abi()
        d.data = self.data.data_ptr()
        if self.offsets is not None:
            d.offsets = self.offsets.data_ptr()
        if self.validity is not None:
            d.validity = self.validity.data_ptr()
        d.validity_offset, d.data_offset, d.len = self.voff, self.doff, self.length
        return d


def run(entry, devs, c):
    """The row indices one entry point returns for the case (raises what check() raises).  The
    entry point gets the case's own limit, also where it is above the row count: it must clamp to
    min(limit, rows) itself, report that count and write no index past it (the buffer holds that
    many and a guard of 8 behind them)."""
    torch = _torch()
    n = devs[0].length
    limit = n if c.limit is None else c.limit
    k = min(limit, n)
    out = torch.full((k + 8,), -1, dtype=torch.int32, device="cuda")
    got = C.c_uint64()
    if entry == "single":
        rc = lib().dbg_sort_limit_indices(C.byref(devs[0].to_abi()), n, int(c.asc[0]), int(c.nulls_first[0]), limit, out.data_ptr(),
                                          C.byref(got), None)
    else:
        arr = (abi.dbg_column * len(devs))(*[d.to_abi() for d in devs])
        asc = (C.c_int * len(devs))(*[int(a) for a in c.asc])
        nf = (C.c_int * len(devs))(*[int(f) for f in c.nulls_first])
        rc = lib().dbg_sort_limit_multi(arr, len(devs), asc, nf, n, limit, out.data_ptr(), C.byref(got), None)
    check(rc)
    assert got.value == k
    host = out.cpu().numpy()
    assert (host[k:] == -1).all(), "indices written past min(limit, rows)"
    return host[:k].view(np.uint32).tolist()


def assert_same(got, want, c, entry):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        pytest.fail("case %s through %s: %d rows for %d; first difference at position %d (device rows %r, reference rows %r); "
                    "predicted %r" % (c.name, entry, len(got), len(want), at, got[at:at + 6], want[at:at + 6], sc.predict(c)))


RUNS = [(c.name, e) for c in sc.cases() for e in (("single", "multi") if sc.runs_multi_too(c) else ("multi",))]


@pytest.mark.parametrize("name,entry", RUNS)
def test_case(name, entry):
    c = sc.case(name)
    devs = [DevCol(x, c.voff, c.doff) for x in c.columns]
    if c.raises:
        with pytest.raises(Unsupported):
            run(entry, devs, c)
    else:
        assert_same(run(entry, devs, c), sc.reference(c), c, entry)


@pytest.mark.parametrize("limit", sc.BLOCK_LIMITS)
@pytest.mark.parametrize("by", ["by-number", "by-string-int"])
def test_block_sort_carries_every_column(by, limit):
    from databend_amd.device import DeviceColumn
    from databend_amd.sort import SortColumnDescription, sort
    cols, sorts = sc.block()
    desc = sorts[by]
    want = sort_ref.sort_limit([cols[o] for o, _, _ in desc], [a for _, a, _ in desc], [f for _, _, f in desc], limit)
    out = sort([DeviceColumn.from_host(x) for x in cols],
               [SortColumnDescription(o, asc=a, nulls_first=f, is_nullable=cols[o].dtype.nullable) for o, a, f in desc], limit)
    assert len(out) == len(cols)
    for j, (host, dev) in enumerate(zip(cols, out)):
        got = dev.to_host()
        assert got.dtype == host.dtype and len(got) == len(want), (by, limit, j)
        values = host.values()
        assert got.values() == [values[i] for i in want], (by, limit, j)
