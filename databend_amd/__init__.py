"""databend_amd — an MI355X-native filter + hash GROUP BY path for Databend.

The product is libdbgpu_agg.so (HIP kernels for gfx950 behind the C ABI in include/dbgpu_agg.h).
This package is the host-side mirror of the reference's operator interface for that path
(TransformPartialAggregate / TransformFinalAggregate / AggregateFunction / TransformFilter) over
ctypes, plus the multi-GPU exchange over torch.distributed (RCCL).
"""
from .column import Column, DataBlock, DataType  # noqa: F401

__all__ = ["Column", "DataBlock", "DataType", "PartialSingleStateAggregator", "FinalSingleStateAggregator",
           "ExprProgram", "col", "lit"]


def __getattr__(name):
    # the processors without GROUP BY, resolved on first use (the aggregator module binds the library)
    if name in ("PartialSingleStateAggregator", "FinalSingleStateAggregator"):
        from . import aggregator
        return getattr(aggregator, name)
    # the projection in front of the aggregate (expr.py)
    if name in ("ExprProgram", "col", "lit"):
        from . import expr
        return getattr(expr, name)
    raise AttributeError(name)
