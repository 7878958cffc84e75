"""Aggregation without GROUP BY: the keyless handle beside the only way the parent commit's library
can run the same query — GROUP BY a constant non-null Int8 key, same arguments, rows and filter.

  count      SELECT COUNT(*)                                                       2^26 rows
  q3         SELECT SUM(x), COUNT(*), AVG(x)            x Int16 (ClickBench Q3)    2^26 rows
  minmax     SELECT MIN(d), MAX(d)                      d Date                     2^26 rows
  q6         SELECT SUM(p) WHERE q >= 5 AND q < 24      p Decimal128(15, 2), q Int32 (TPC-H Q6)  2^26 rows
  like       SELECT COUNT(*) WHERE url LIKE '%google%'  10 M URL-like rows, 'google' in ~1 % (scripts/bench_like.py)

Two child processes, one per side, each holding its own device-resident inputs: `keyless` loads this
tree's library, `baseline` the library named by --baseline-lib through the DBGPU_LIB override (the
parent commit's, built from a clean export of it).  The driver alternates them repeat by repeat
inside this one call: two warm-up repeats of every shape on each side, then --repeats timed ones.
Kernel times are the library's HIP-event scopes (ffi.prof_enable / prof_read) summed over the step
(keyless_reduce + keyless_merge | agg_insert + agg_retry + agg_rehash, plus like_mask);
`step_ms` is a host clock around reset / add_groups / result on device buffers, ending in the
result's stream synchronise, taken in a repeat of its own with the profiler off.  Every figure is the
median with min..max.

Acceptance, per shape: the keyless side's slowest repeat is faster than the baseline's fastest.
Also reported: the bytes the shape must read over the reduce kernel's time, as a share of the
6.29 TB/s copy bandwidth measured on the MI355X; and whether the LIKE pre-pass bounds the shape.

    python scripts/bench_keyless.py --baseline-lib PATH/libdbgpu_agg.so [--rows N] [--like-rows N] [--repeats R] [--warmup W]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SHAPES = ["count", "q3", "minmax", "q6", "like"]
COPY_TBS = 6.29
REDUCE = ("keyless_reduce", "keyless_merge")
INSERT = ("agg_insert", "agg_retry", "agg_rehash")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--like-rows", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--side", choices=["keyless", "baseline"], default=None, help="internal: run as that side's child")
    return ap.parse_args()


# ---- child: one side ------------------------------------------------------------------------------
def child(a):
    sys.path.insert(0, ROOT)
    import torch

    from databend_amd import column as col
    from databend_amd import ffi
    from databend_amd.aggregates import AggregateFunctionFactory
    from databend_amd.aggregator import AggregateHashTable, AggregatorParams, HashTableConfig
    from databend_amd.device import DeviceColumn
    from databend_amd.filter import FilterProgram, and_, cmp, like

    keyless = a.side == "keyless"
    F = AggregateFunctionFactory.instance()
    g = torch.Generator(device="cuda").manual_seed(26)
    n, nl = a.rows, a.like_rows

    def ints(lo, hi, rows, dtype, dt):
        t = torch.randint(lo, hi, (rows,), device="cuda", generator=g, dtype=dtype)
        return DeviceColumn(dt, t.view(torch.uint8), None, None, rows)

    def decimals(rows):  # Decimal128(15, 2): a non-negative i64 value, sign-extended to 16 bytes
        lo = torch.randint(0, 10**13, (rows,), device="cuda", generator=g, dtype=torch.int64)
        t = torch.stack([lo, torch.zeros_like(lo)], dim=1).contiguous()
        return DeviceColumn(col.Decimal128(15, 2), t.view(torch.uint8).reshape(-1), None, None, rows)

    def urls(rows, share):  # scripts/bench_like.py's column
        w, chunk, needle = 120, 1 << 21, torch.tensor(list(b"google"), dtype=torch.uint8, device="cuda")
        lens = torch.randint(40, w + 1, (rows,), device="cuda", generator=g)
        prefix = torch.tensor(list(b"http://example.com/"), dtype=torch.uint8, device="cuda")
        parts = []
        for lo in range(0, rows, chunk):
            hi = min(rows, lo + chunk)
            m = torch.randint(97, 123, (hi - lo, w), device="cuda", generator=g, dtype=torch.uint8)
            m[:, :19] = prefix
            hit = torch.nonzero(torch.rand(hi - lo, device="cuda", generator=g) < share)[:, 0]
            room = lens[lo:hi][hit] - 19 - 6 + 1
            at = 19 + (torch.rand(len(hit), device="cuda", generator=g) * room).long()
            m[hit[:, None], at[:, None] + torch.arange(6, device="cuda")[None, :]] = needle
            parts.append(m[torch.arange(w, device="cuda")[None, :] < lens[lo:hi, None]])
        offs = torch.zeros(rows + 1, dtype=torch.int64, device="cuda")
        offs[1:] = torch.cumsum(lens, 0)
        return DeviceColumn(col.String, torch.cat(parts), offs, None, rows)

    x16 = ints(-2**15, 2**15 - 1, n, torch.int16, col.Int16)
    date = ints(0, 20000, n, torch.int32, col.Date)
    price, qty = decimals(n), ints(0, 50, n, torch.int32, col.Int32)
    url = urls(nl, 0.01)
    zeros = DeviceColumn(col.Int8, torch.zeros(max(n, nl), dtype=torch.uint8, device="cuda"), None, None, max(n, nl))
    # shape -> (aggregates, argument columns, rows, filter, bytes the query must read)
    shapes = {
        "count": ([F.get("count")], [None], n, None, 0),
        "q3": ([F.get("sum", [], [col.Int16]), F.get("count"), F.get("avg", [], [col.Int16])], [x16, None, x16], n, None, 2 * n),
        "minmax": ([F.get("min", [], [col.Date]), F.get("max", [], [col.Date])], [date, date], n, None, 4 * n),
        "q6": ([F.get("sum", [], [price.dtype])], [price], n, FilterProgram(and_(cmp(0, ">=", 5), cmp(0, "<", 24)), [qty]), 20 * n),
        "like": ([F.get("count")], [None], nl, FilterProgram(like(0, b"%google%"), [url]), int(url.data.numel()) + 8 * (nl + 1)),
    }
    tables = {s: AggregateHashTable(AggregatorParams([] if keyless else [col.Int8], v[0]), HashTableConfig(True)) for s, v in shapes.items()}

    def step(shape):
        fns, args, rows, filt, _ = shapes[shape]
        ht = tables[shape]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ht.reset()
        ht.add_groups([] if keyless else [zeros], args, rows=rows, filter_program=filt, on_device=True)
        out = ht.merge_result_device()  # ends in dbg_agg_result's stream synchronise
        ms = (time.perf_counter() - t0) * 1e3
        assert out[0].length == 1, out[0].length
        return ms, out

    def first_values(out):
        return [c.to_host().values()[0] for c in out[:len(out) if keyless else -1]]

    for shape in SHAPES:
        for _ in range(a.warmup):
            step(shape)
    print(json.dumps({"ready": a.side, "like_blob_bytes": int(url.data.numel()), "must_read": {s: v[4] for s, v in shapes.items()},
                      "results": {s: [str(v) for v in first_values(step(s)[1])] for s in SHAPES}}), flush=True)
    for line in sys.stdin:
        shape = line.strip()
        if not shape:
            break
        ffi.prof_reset()
        ffi.prof_enable(True)
        step(shape)
        torch.cuda.synchronize()
        ffi.prof_enable(False)
        prof = {k: v[0] for k, v in ffi.prof_read().items()}
        print(json.dumps({"shape": shape, "prof": prof, "step_ms": step(shape)[0]}), flush=True)
    for ht in tables.values():
        ht.close()


# ---- driver ---------------------------------------------------------------------------------------
def stats(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    a = parse()
    if a.side:
        return child(a)
    if not a.baseline_lib or not os.path.exists(a.baseline_lib):
        sys.exit("--baseline-lib: the parent commit's libdbgpu_agg.so is needed (there is no other baseline)")
    procs = {}
    for side in ("keyless", "baseline"):
        env = dict(os.environ)
        if side == "baseline":
            env["DBGPU_LIB"] = os.path.abspath(a.baseline_lib)
        else:
            env.pop("DBGPU_LIB", None)
        cmd = [sys.executable, os.path.abspath(__file__), "--side", side, "--rows", str(a.rows), "--like-rows", str(a.like_rows),
               "--warmup", str(a.warmup)]
        procs[side] = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
    ready = {side: json.loads(p.stdout.readline()) for side, p in procs.items()}
    assert ready["keyless"]["results"] == ready["baseline"]["results"], ready  # the same answers on both sides
    samples = {side: {s: {"kernel_ms": [], "reduce_ms": [], "like_mask_ms": [], "step_ms": []} for s in SHAPES} for side in procs}
    for _ in range(a.repeats):
        for shape in SHAPES:
            for side, p in procs.items():  # alternating
                p.stdin.write(shape + "\n")
                p.stdin.flush()
                r = json.loads(p.stdout.readline())
                core = sum(r["prof"].get(k, 0.0) for k in (REDUCE if side == "keyless" else INSERT))
                lm = r["prof"].get("like_mask", 0.0)
                S = samples[side][shape]
                S["reduce_ms"].append(core)
                S["like_mask_ms"].append(lm)
                S["kernel_ms"].append(core + lm)
                S["step_ms"].append(r["step_ms"])
    for p in procs.values():
        p.stdin.write("\n")
        p.stdin.close()
        p.wait()
    out = {"rows": a.rows, "like_rows": a.like_rows, "repeats": a.repeats, "warmup": a.warmup, "results": ready["keyless"]["results"],
           "shapes": {}}
    ok = True
    for shape in SHAPES:
        k, b = samples["keyless"][shape], samples["baseline"][shape]
        row = {"keyless": {m: stats(v) for m, v in k.items()}, "baseline": {m: stats(v) for m, v in b.items()}}
        row["accepted_kernel"] = max(k["kernel_ms"]) < min(b["kernel_ms"])
        row["accepted_step"] = max(k["step_ms"]) < min(b["step_ms"])
        must = ready["keyless"]["must_read"][shape]
        row["must_read_bytes"] = must
        med = statistics.median(k["reduce_ms"] if shape != "like" else k["kernel_ms"])
        row["share_of_copy_bandwidth"] = round(must / (med * 1e-3) / (COPY_TBS * 1e12), 4) if must and med > 0 else None
        row["bound_by_like_prepass"] = statistics.median(k["like_mask_ms"]) > statistics.median(k["reduce_ms"])
        ok = ok and row["accepted_kernel"]
        out["shapes"][shape] = row
        print(f"{shape:7s} keyless kernel {row['keyless']['kernel_ms']['median_ms']:9.4f} ms ({row['keyless']['kernel_ms']['min_ms']:.4f}"
              f"..{row['keyless']['kernel_ms']['max_ms']:.4f})  baseline {row['baseline']['kernel_ms']['median_ms']:9.4f} ms "
              f"({row['baseline']['kernel_ms']['min_ms']:.4f}..{row['baseline']['kernel_ms']['max_ms']:.4f})  step "
              f"{row['keyless']['step_ms']['median_ms']:.3f} vs {row['baseline']['step_ms']['median_ms']:.3f} ms  "
              f"accepted {row['accepted_kernel']} / step {row['accepted_step']}  share {row['share_of_copy_bandwidth']}")
    out["accepted"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
