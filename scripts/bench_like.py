"""LIKE '%needle%' on the ClickBench shape: the two mask kernels beside each other, and the Q22-shaped
step with and without the LIKE.

    10 M rows, URL-like String column of 40..120 bytes sharing a 19-byte prefix, 'google' in ~1 % and
    in ~30 % of the rows (two columns), 500 k distinct String keys

  masks   dbg_filter_select(url LIKE '%google%') with the mask forced to like_scan_kernel and to
          like_rows_kernel (dbg_like_force_kernel), alternating: the `like_mask` scope of each, their
          ratio, and the faster one's bytes/s (blob bytes + offsets, over its time)
  q22     SELECT key, MIN(url), COUNT(*) WHERE url LIKE '%google%' AND key <> '' GROUP BY key beside the
          same step with only key <> '': like_mask, insert (agg_insert + agg_retry + agg_rehash) and a
          host clock around the step

Kernel times are the library's HIP-event scopes (ffi.prof_enable / prof_read); every figure is the
median over the timed repeats, alternating variants after warm-up repeats of each, with min..max.

    python scripts/bench_like.py [--rows N] [--keys K] [--repeats R] [--warmup W]
    python scripts/bench_like.py --tree OTHER_TREE --only-baseline   # the `key <> ''` step alone, with
        the package and library of another checkout (one that has no LIKE: the parent commit)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--keys", type=int, default=500_000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--tree", default=os.path.dirname(HERE))
ap.add_argument("--only-baseline", action="store_true")
A = ap.parse_args()
sys.path.insert(0, os.path.abspath(A.tree))
import torch  # noqa: E402

from databend_amd import abi  # noqa: E402
from databend_amd import column as col  # noqa: E402
from databend_amd import ffi  # noqa: E402
from databend_amd.aggregates import AggregateFunctionFactory  # noqa: E402
from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig  # noqa: E402
from databend_amd.device import DeviceColumn  # noqa: E402
from databend_amd.filter import FilterProgram, and_, cmp  # noqa: E402

NEEDLE = b"google"
INSERT = ("agg_insert", "agg_retry", "agg_rehash")


def key_column(rows, n_keys, g):
    """"phrase " + 8 decimal digits, then 0..15 more bytes fixed by the key id (never empty)."""
    kid = torch.randint(0, n_keys, (rows,), device="cuda", generator=g)
    kmat = torch.full((rows, 31), ord("q"), dtype=torch.uint8, device="cuda")
    kmat[:, :7] = torch.tensor(list(b"phrase "), dtype=torch.uint8, device="cuda")
    for d in range(8):
        kmat[:, 7 + d] = (48 + (kid // 10 ** (7 - d)) % 10).to(torch.uint8)
    lens = 15 + kid % 16
    keep = torch.arange(31, device="cuda")[None, :] < lens[:, None]
    offs = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(lens, 0)
    return DeviceColumn(col.String, kmat[keep].contiguous(), offs, None, rows)


def url_column(rows, share, g):
    """A shared 19-byte prefix, then random lower-case bytes, 40..120 bytes; NEEDLE written into
    `share` of the rows at a random place behind the prefix."""
    w, chunk = 120, 1 << 21
    lens = torch.randint(40, w + 1, (rows,), device="cuda", generator=g)
    prefix = torch.tensor(list(b"http://example.com/"), dtype=torch.uint8, device="cuda")
    needle = torch.tensor(list(NEEDLE), dtype=torch.uint8, device="cuda")
    parts = []
    for lo in range(0, rows, chunk):
        hi = min(rows, lo + chunk)
        n = hi - lo
        m = torch.randint(97, 123, (n, w), device="cuda", generator=g, dtype=torch.uint8)
        m[:, :19] = prefix
        hit = torch.nonzero(torch.rand(n, device="cuda", generator=g) < share)[:, 0]
        room = lens[lo:hi][hit] - 19 - len(NEEDLE) + 1
        at = 19 + (torch.rand(len(hit), device="cuda", generator=g) * room).long()
        m[hit[:, None], at[:, None] + torch.arange(len(NEEDLE), device="cuda")[None, :]] = needle
        parts.append(m[torch.arange(w, device="cuda")[None, :] < lens[lo:hi, None]])
    offs = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(lens, 0)
    return DeviceColumn(col.String, torch.cat(parts), offs, None, rows)


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def profiled(fn):
    ffi.prof_reset()
    ffi.prof_enable(True)
    out = fn()
    torch.cuda.synchronize()
    ffi.prof_enable(False)
    return out, ffi.prof_read()


def bench_masks(url, rows, out):
    from databend_amd.filter import like
    L = ffi.lib()
    sel = torch.empty(rows, dtype=torch.int32, device="cuda")
    prog = FilterProgram(like(0, b"%" + NEEDLE + b"%"), [url])
    n = C.c_uint64()

    def run(kernel):
        ffi.check(L.dbg_like_force_kernel(kernel))
        ffi.check(L.dbg_filter_select(prog.ptr(), rows, sel.data_ptr(), C.byref(n), None))
        ffi.check(L.dbg_like_force_kernel(0))
        return n.value

    t = {"scan": [], "rows": []}
    selected = {}
    for r in range(A.warmup + A.repeats):
        for name, k in (("scan", 2), ("rows", 1)):  # alternating
            selected[name], prof = profiled(lambda: run(k))
            if r >= A.warmup:
                t[name].append(prof["like_mask"][0])
    assert selected["scan"] == selected["rows"]
    nbytes = int(url.data.numel()) + (rows + 1) * 8
    out["selected"] = selected["scan"]
    out["blob_and_offset_bytes"] = nbytes
    for name in t:
        out["like_mask_" + name] = stats(t[name])
    fast = min(t, key=lambda k: statistics.median(t[k]))
    out["scan_over_rows"] = round(statistics.median(t["scan"]) / statistics.median(t["rows"]), 3)
    out["faster"] = fast
    out["faster_TB_per_s"] = round(nbytes / (statistics.median(t[fast]) * 1e-3) / 1e12, 3)


def bench_q22(key, url, rows, variants, out):
    F = AggregateFunctionFactory.instance()
    fns = [F.get("min", [], [url.dtype]), F.get("count")]
    tables = {v: AggregateHashTable(AggregatorParams([col.String], fns), HashTableConfig(True, A.keys)) for v in variants}
    for ht in tables.values():
        ht.set_strategy(abi.STRATEGY_TABLE)  # a String MIN/MAX handle has no other strategy

    def pred(v):
        if v == "key_ne_empty":
            return FilterProgram(cmp(0, "<>", ""), [key])
        from databend_amd.filter import like
        return FilterProgram(and_(like(0, b"%" + NEEDLE + b"%"), cmp(1, "<>", "")), [url, key])

    def step(v):
        ht = tables[v]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ht.reset()
        ht.add_groups([key], [url, None], rows=rows, filter_program=pred(v), on_device=True)
        res = ht.merge_result_device()  # ends in the result's stream synchronise
        return (time.perf_counter() - t0) * 1e3, res[0].length

    s = {v: {"like_mask": [], "insert": [], "step_ms": []} for v in variants}
    groups, paths = {}, {}
    for r in range(A.warmup + A.repeats):
        for v in variants:  # alternating
            (ms, groups[v]), prof = profiled(lambda: step(v))
            if r >= A.warmup:
                s[v]["like_mask"].append(prof.get("like_mask", (0.0, 0))[0])
                s[v]["insert"].append(sum(prof.get(k, (0.0, 0))[0] for k in INSERT))
        for v in variants:  # the host clock without the profiler's event records
            ms, _ = step(v)
            if r >= A.warmup:
                s[v]["step_ms"].append(ms)
    for v in variants:
        paths[v] = {k: n for k, n in tables[v].insert_paths().items() if n}
        out[v] = {"groups": groups[v], "insert_kernels": sorted(paths[v])}
        out[v].update({k: stats(x) for k, x in s[v].items()})
        tables[v].close()


def main():
    g = torch.Generator(device="cuda").manual_seed(7)
    key = key_column(A.rows, A.keys, g)
    out = {"rows": A.rows, "distinct_keys": A.keys, "repeats": A.repeats, "warmup": A.warmup, "library": ffi.LIB_PATH}
    for share in (0.01, 0.30):
        url = url_column(A.rows, share, g)
        o = out[f"needle_in_{int(share * 100)}pct"] = {}
        if A.only_baseline:
            bench_q22(key, url, A.rows, ["key_ne_empty"], o)
        else:
            bench_masks(url, A.rows, o)
            bench_q22(key, url, A.rows, ["like_and_key_ne_empty", "key_ne_empty"], o)
        del url
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
