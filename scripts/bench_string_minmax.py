"""MIN(String) on the ClickBench shape, beside MIN(Int64) over the same rows as context.

    SELECT key, MIN(arg), COUNT(*) ... GROUP BY key
    10 M rows, 500 k distinct String keys, URL-like String arguments of ~60 bytes

Kernel times come from the library's HIP-event scopes (ffi.prof_enable / prof_read): the insert
(agg_insert), the finalize (count_groups + the String aggregate's size pass str_agg_bytes), the
result writers (write_results) and the String gather (str_gather).  Both variants run in this one
process, alternating, after warm-up repeats of each; every figure is the median over the timed
repeats with its min..max.  `step_ms` is a host clock around reset / add_groups / finalize /
result (device buffers), which ends in the result's stream synchronise.  Both handles run the HBM
table (DBG_STRATEGY_TABLE): a String MIN/MAX handle has no other strategy.

    python scripts/bench_string_minmax.py [--rows N] [--keys K] [--repeats R] [--warmup W]
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

SCOPES = {"insert": ("agg_insert", "agg_retry", "agg_rehash"), "finalize": ("count_groups", "str_agg_bytes"),
          "write": ("write_results",), "gather": ("str_gather",)}


def string_column(mat, lens):
    """Rows of a (n, w) byte matrix cut to lens bytes each -> a device String column."""
    n, w = mat.shape
    keep = torch.arange(w, device=mat.device)[None, :] < lens[:, None]
    offs = torch.zeros(n + 1, dtype=torch.int64, device=mat.device)
    offs[1:] = torch.cumsum(lens, 0)
    return DeviceColumn(col.String, mat[keep].contiguous(), offs, None, n)


def make_inputs(rows, n_keys, seed=7):
    g = torch.Generator(device="cuda").manual_seed(seed)
    # keys: "phrase " + 8 decimal digits, then 0..15 more bytes fixed by the key id
    kid = torch.randint(0, n_keys, (rows,), device="cuda", generator=g)
    kmat = torch.full((rows, 31), ord("q"), dtype=torch.uint8, device="cuda")
    kmat[:, :7] = torch.tensor(list(b"phrase "), dtype=torch.uint8, device="cuda")
    for d in range(8):
        kmat[:, 7 + d] = (48 + (kid // 10 ** (7 - d)) % 10).to(torch.uint8)
    key = string_column(kmat, 15 + kid % 16)
    del kmat
    # arguments: a shared 19-byte prefix, then random lower-case bytes; 40..80 bytes, ~60 on average
    chunk = 1 << 21
    parts, lens = [], torch.randint(40, 81, (rows,), device="cuda", generator=g)
    prefix = torch.tensor(list(b"http://example.com/"), dtype=torch.uint8, device="cuda")
    for lo in range(0, rows, chunk):
        hi = min(rows, lo + chunk)
        m = torch.randint(97, 123, (hi - lo, 80), device="cuda", generator=g, dtype=torch.uint8)
        m[:, :19] = prefix
        parts.append(m[torch.arange(80, device="cuda")[None, :] < lens[lo:hi, None]])
    offs = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(lens, 0)
    url = DeviceColumn(col.String, torch.cat(parts), offs, None, rows)
    num = DeviceColumn(col.Int64, torch.randint(-2 ** 62, 2 ** 62, (rows,), device="cuda", generator=g).view(torch.uint8), None,
                       None, rows)
    return key, url, num


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--keys", type=int, default=500_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    key, url, num = make_inputs(a.rows, a.keys)
    F = AggregateFunctionFactory.instance()
    tables = {}
    for name, arg in (("min_string", url), ("min_int64", num)):
        fns = [F.get("min", [], [arg.dtype]), F.get("count")]
        tables[name] = (AggregateHashTable(AggregatorParams([col.String], fns), HashTableConfig(True, a.keys)), arg)
        # like for like: a String MIN/MAX handle only runs the HBM table, so the Int64 one is kept on it too
        tables[name][0].set_strategy(abi.STRATEGY_TABLE)

    def step(name):
        ht, arg = tables[name]
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
    out = {"rows": a.rows, "distinct_keys": a.keys, "arg_bytes": int(url.data.numel()), "repeats": a.repeats, "warmup": a.warmup}
    for name, s in samples.items():
        out[name] = {"groups": groups[name]}
        for k, v in s.items():
            out[name][k] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        print(f"{name:11s} " + "  ".join(f"{k} {out[name][k]['median_ms']:.3f} ms" for k in s))
    print(json.dumps(out))
    for ht, _ in tables.values():
        ht.close()


if __name__ == "__main__":
    main()
