"""MIN / MAX of a String argument at the boundary (no GPU): dbg_agg_result_type accepts it and
gives the argument's type (MinMaxAnyState<StringType, CMP>), nullable when the argument is or when
the function is wrapped by the or-null adaptor; SUM / AVG of a String stay unsupported."""
import ctypes as C

import pytest

from databend_amd import abi
from databend_amd.ffi import lib


def _result_type(kind, nullable, or_null):
    spec = abi.dbg_agg_spec()
    spec.kind = kind
    spec.arg = abi.dbg_datatype(abi.STRING, 0, 0, 1 if nullable else 0, 0)
    spec.or_null = or_null
    out = abi.dbg_datatype()
    rc = lib().dbg_agg_result_type(C.byref(spec), C.byref(out))
    return rc, out


@pytest.mark.parametrize("kind", [abi.AGG_MIN, abi.AGG_MAX], ids=["min", "max"])
@pytest.mark.parametrize("nullable", [False, True], ids=["String", "Nullable(String)"])
@pytest.mark.parametrize("or_null", [0, 1])
def test_string_min_max_result_type(kind, nullable, or_null):
    rc, out = _result_type(kind, nullable, or_null)
    assert rc == abi.DBG_OK, lib().dbg_last_error()
    assert out.type == abi.STRING
    assert bool(out.nullable) == bool(nullable or or_null)


@pytest.mark.parametrize("kind", [abi.AGG_SUM, abi.AGG_AVG, abi.AGG_AVG_SQL], ids=["sum", "avg", "avg_sql"])
@pytest.mark.parametrize("nullable", [False, True], ids=["String", "Nullable(String)"])
def test_string_sum_avg_still_unsupported(kind, nullable):
    rc, _ = _result_type(kind, nullable, 1)
    assert rc == abi.DBG_ERR_UNSUPPORTED
