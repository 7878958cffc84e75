"""SUM / MIN over Decimal256(50, 2) beside the same integer values as Decimal128(38, 2).

    SELECT key, SUM(x), COUNT(*) ... GROUP BY key      10 M rows, Int32 key, 7 and 500 k groups
    SELECT key, MIN(x), COUNT(*) ... GROUP BY key      500 k groups

The values are random 64-bit integers sign-extended to 16 and to 32 bytes, so both columns hold the
same numbers and the negative ones exercise every carry of the wide add.  A Decimal256 value is
twice the bytes of a Decimal128 one (32 against 16): that ratio is the floor for the slowdown of a
bandwidth-bound insert.

Kernel times come from the library's HIP-event scopes (ffi.prof_enable / prof_read): the insert
(agg_insert and, when the table grows, agg_retry / agg_rehash), the finalize (count_groups or the
one-workgroup finalize_small) and the result writers (write_results).  All variants run in this one
process, alternating, after warm-up repeats of each; every figure is the median over the timed
repeats with its min..max.  `step_ms` is a host clock around reset / add_groups / finalize /
result (device buffers), which ends in the result's stream synchronise.  Every handle runs the HBM
table (DBG_STRATEGY_TABLE): a Decimal256 handle has no other strategy.  With 7 groups the
Decimal128 handle takes the fast integer-key insert and the Decimal256 one the generic insert,
which is what a caller of this build gets.

    python scripts/bench_decimal256.py [--rows N] [--repeats R] [--warmup W]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from databend_amd import abi  # noqa: E402
from databend_amd import column as col  # noqa: E402
from databend_amd import ffi  # noqa: E402
from databend_amd.aggregates import AggregateFunctionFactory  # noqa: E402
from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig  # noqa: E402
from databend_amd.device import DeviceColumn  # noqa: E402

SCOPES = {"insert": ("agg_insert", "agg_retry", "agg_rehash"), "finalize": ("count_groups", "finalize_small"),
          "write": ("write_results",)}


def make_inputs(rows, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    lo = torch.randint(-2 ** 62, 2 ** 62, (rows,), device="cuda", generator=g)
    hi = lo >> 63  # the sign, as every higher word
    d128 = DeviceColumn(col.Decimal128(38, 2), torch.stack([lo, hi], 1).contiguous().view(torch.uint8).reshape(-1), None, None, rows)
    d256 = DeviceColumn(col.Decimal256(50, 2), torch.stack([lo, hi, hi, hi], 1).contiguous().view(torch.uint8).reshape(-1), None, None,
                        rows)
    keys = {n: DeviceColumn(col.Int32, torch.randint(0, n, (rows,), device="cuda", generator=g, dtype=torch.int32).view(torch.uint8),
                            None, None, rows) for n in (7, 500_000)}
    return keys, d128, d256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    keys, d128, d256 = make_inputs(a.rows)
    F = AggregateFunctionFactory.instance()
    tables = {}
    for fn, groups in (("sum", 7), ("sum", 500_000), ("min", 500_000)):
        for tname, arg in (("decimal256", d256), ("decimal128", d128)):
            fns = [F.get(fn, [], [arg.dtype]), F.get("count")]
            ht = AggregateHashTable(AggregatorParams([col.Int32], fns), HashTableConfig(True, groups))
            ht.set_strategy(abi.STRATEGY_TABLE)  # like for like: the only strategy a Decimal256 handle has
            tables[f"{fn}_{groups}_{tname}"] = (ht, keys[groups], arg)

    def step(name):
        ht, key, arg = tables[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ht.reset()
        ht.add_groups([key], [arg, None], rows=a.rows, on_device=True)
        out = ht.merge_result_device()  # ends in dbg_agg_result's stream synchronise
        return (time.perf_counter() - t0) * 1e3, out[0].length

    samples = {n: {k: [] for k in list(SCOPES) + ["step_ms"]} for n in tables}
    groups = {}
    for r in range(a.warmup + a.repeats):
        for name in tables:  # alternating
            timed = r >= a.warmup
            if timed:
                ffi.prof_reset()
                ffi.prof_enable(True)
            ms, groups[name] = step(name)
            if timed:
                ffi.prof_enable(False)
                prof = ffi.prof_read()
                for k, scopes in SCOPES.items():
                    samples[name][k].append(sum(prof.get(s, (0.0, 0))[0] for s in scopes))
        # host clock without the profiler's event records
        for name in tables:
            if r >= a.warmup:
                samples[name]["step_ms"].append(step(name)[0])
    out = {"rows": a.rows, "repeats": a.repeats, "warmup": a.warmup, "bytes_per_value": {"decimal256": 32, "decimal128": 16}}
    for name, s in samples.items():
        out[name] = {"groups": groups[name]}
        for k, v in s.items():
            out[name][k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        print(f"{name:24s} " + "  ".join(f"{k} {out[name][k]['median_ms']:.3f} ms" for k in s))
    print(json.dumps(out))
    for ht, _, _ in tables.values():
        ht.close()


if __name__ == "__main__":
    main()
