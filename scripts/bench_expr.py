"""The device projection (dbg_expr_eval) beside a device-to-device copy of the same traffic, and what
it costs in front of a TPC-H Q1 step.

  a   Int16 + const -> Int32                              reads 2, writes 4 bytes per row
  b   Float64 * Float64                                   reads 16, writes 8
  c   Q1: extprice * (1 - discount), that * (1 + tax)     three Decimal(15, 2) in, Decimal(31, 4) and
      Decimal(38, 6) out: reads 48, writes 32

Part 1, one process, this tree's library, --rows device-resident rows (default 2^26): two warm-up
repeats of every shape, then --repeats timed ones.  Each repeat runs the projection and, right after
it, the yardstick: one device-to-device copy whose read plus write traffic equals the bytes the
shape must read and write (a copy of (read + write) / 2 bytes), timed with HIP events.  The
projection's kernel time is the library's own HIP-event scope (ffi.prof_enable / prof_read:
expr_eval_narrow / expr_eval_wide); `call_ms` is a host clock around dbg_expr_eval into
preallocated outputs, taken in a repeat of its own with the profiler off.  Per shape: median
(min..max), bytes over kernel time, that rate over the copy's rate, and over the 6.29 TB/s copy
bandwidth measured on the MI355X.  A shape counts as slower than the copy when its median rate is
below the copy's by more than the copy's own spread (max - min) across the repeats.

Part 2, two child processes alternating repeat by repeat: a config-1 step (workloads.ConfigRunner:
reset, fused filter + insert, fused finalize) at its default 6,001,215 rows, fed by the projection
(`projected`, this tree's library: the projection runs in front of every step) and fed by the
generator's precomputed columns (`precomputed`, the library named by --baseline-lib through
DBGPU_LIB: all the parent commit's library can do).  Both sides' results are compared first.  The
difference is the projection's cost, not a regression.

    python scripts/bench_expr.py --baseline-lib PATH/libdbgpu_agg.so [--rows N] [--repeats R] [--warmup W] [--out FILE]
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
COPY_TBS = 6.29
SHAPES = ["a", "b", "c"]
Q1_ROWS = 6_001_215


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--q1-rows", type=int, default=Q1_ROWS)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expr", "bench_expr.json"))
    ap.add_argument("--side", choices=["shapes", "projected", "precomputed"], default=None, help="internal: run as that child")
    return ap.parse_args()


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


# ---- part 1: the three shapes beside a copy ------------------------------------------------------------
def shapes_child(a):
    sys.path.insert(0, ROOT)
    import ctypes as C

    import torch

    from databend_amd import abi, ffi
    from databend_amd import column as col
    from databend_amd import device
    from databend_amd.device import DeviceColumn
    from databend_amd.expr import ExprProgram, col as c_, lit
    from databend_amd.ffi import check, lib

    n = a.rows
    g = torch.Generator(device="cuda").manual_seed(31)

    def decimals(hi):  # Decimal128(15, 2): a non-negative i64 value, zero-extended to 16 bytes
        lo = torch.randint(0, hi, (n,), device="cuda", generator=g, dtype=torch.int64)
        t = torch.stack([lo, torch.zeros_like(lo)], dim=1).contiguous()
        return DeviceColumn(col.Decimal128(15, 2), t.view(torch.uint8).reshape(-1), None, None, n)

    x16 = DeviceColumn(col.Int16, torch.randint(-2**15, 2**15 - 1, (n,), device="cuda", generator=g, dtype=torch.int16).view(torch.uint8),
                       None, None, n)
    f1 = DeviceColumn(col.Float64, torch.rand(n, device="cuda", generator=g, dtype=torch.float64).view(torch.uint8), None, None, n)
    f2 = DeviceColumn(col.Float64, torch.rand(n, device="cuda", generator=g, dtype=torch.float64).view(torch.uint8), None, None, n)
    price, disc, tax = decimals(10**7), decimals(11), decimals(9)
    dp = c_(0) * (1 - c_(1))
    programs = {
        "a": (ExprProgram([c_(0) + lit(7)], [x16]), 2, 4),
        "b": (ExprProgram([c_(0) * c_(1)], [f1, f2]), 16, 8),
        "c": (ExprProgram([dp, dp * (1 + c_(2))], [price, disc, tax]), 48, 32),
    }
    state = {}
    for s, (prog, rd, wr) in programs.items():
        outs = [device.empty(t, n) for t in prog.result_types()]
        arr = (abi.dbg_out_column * len(outs))()
        for i, o in enumerate(outs):
            arr[i].data = o.data.data_ptr()
        half = (rd + wr) * n // 2
        state[s] = dict(prog=prog, outs=outs, arr=arr, src=torch.empty(half, dtype=torch.uint8, device="cuda").zero_(),
                        dst=torch.empty(half, dtype=torch.uint8, device="cuda"), bytes=(rd + wr) * n)
    stream = torch.cuda.current_stream().cuda_stream

    def eval_(s):
        st = state[s]
        t0 = time.perf_counter()
        check(lib().dbg_expr_eval(st["prog"].ptr(), None, n, st["arr"], stream))
        return (time.perf_counter() - t0) * 1e3

    def copy_(s):
        st = state[s]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st["dst"].copy_(st["src"])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for s in SHAPES:
        for _ in range(a.warmup):
            eval_(s)
            copy_(s)
    samples = {s: {"kernel_ms": [], "call_ms": [], "copy_ms": []} for s in SHAPES}
    for _ in range(a.repeats):
        for s in SHAPES:
            ffi.prof_reset()
            ffi.prof_enable(True)
            eval_(s)
            torch.cuda.synchronize()
            ffi.prof_enable(False)
            samples[s]["kernel_ms"].append(sum(v[0] for k, v in ffi.prof_read().items() if k.startswith("expr_eval")))
            samples[s]["copy_ms"].append(copy_(s))
            samples[s]["call_ms"].append(eval_(s))
    out = {}
    for s in SHAPES:
        S, by = samples[s], state[s]["bytes"]
        km, cm = statistics.median(S["kernel_ms"]), statistics.median(S["copy_ms"])
        rate = lambda ms: by / (ms * 1e-3) / 1e12
        copy_rates = [rate(ms) for ms in S["copy_ms"]]
        row = {"bytes": by, "kernel_ms": stats(S["kernel_ms"]), "call_ms": stats(S["call_ms"]), "copy_ms": stats(S["copy_ms"]),
               "kernel_TBps": round(rate(km), 3), "copy_TBps": round(rate(cm), 3), "of_copy": round(cm / km, 3),
               "of_6.29_TBps": round(rate(km) / COPY_TBS, 3), "copy_spread_TBps": round(max(copy_rates) - min(copy_rates), 3)}
        row["slower_than_copy"] = rate(km) < rate(cm) - (max(copy_rates) - min(copy_rates))
        out[s] = row
    print(json.dumps({"shapes": out}), flush=True)


# ---- part 2: one side of the Q1 comparison ---------------------------------------------------------------
def q1_child(a):
    sys.path.insert(0, ROOT)
    import torch

    from databend_amd import ffi, workloads
    projected = a.side == "projected"
    rows = a.q1_rows
    r = workloads.ConfigRunner(1, rows)
    cols = r.inputs[0]
    names = [c for _, c in r.shape.aggs]
    i_dp, i_ch = names.index("disc_price"), names.index("charge")
    prog = None
    if projected:
        from databend_amd.expr import ExprProgram, col as c_
        dp = c_(0) * (1 - c_(1))
        prog = ExprProgram([dp, dp * (1 + c_(2))], [cols["l_extendedprice"], cols["l_discount"], cols["l_tax"]])

    def step():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if projected:
            r.arg_cols[0][i_dp], r.arg_cols[0][i_ch] = prog.eval(rows)
            r._prep = {}
        r.step(0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        step()
    step()
    keys, aggs = r.results_host()
    table = sorted(zip(*[[str(v) for v in c.values()] for c in aggs + keys]))
    print(json.dumps({"ready": a.side, "results": table}), flush=True)
    for line in sys.stdin:
        if not line.strip():
            break
        ffi.prof_reset()
        ffi.prof_enable(True)
        step()
        ffi.prof_enable(False)
        prof = {k: v[0] for k, v in ffi.prof_read().items()}
        print(json.dumps({"step_ms": step(), "kernel_ms": sum(prof.values()),
                          "expr_kernel_ms": sum(v for k, v in prof.items() if k.startswith("expr_eval"))}), flush=True)
    r.close()


# ---- driver --------------------------------------------------------------------------------------------
def main():
    a = parse()
    if a.side == "shapes":
        return shapes_child(a)
    if a.side:
        return q1_child(a)
    if not a.baseline_lib or not os.path.exists(a.baseline_lib):
        sys.exit("--baseline-lib: the parent commit's libdbgpu_agg.so is needed (there is no other baseline)")
    base = [sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--q1-rows", str(a.q1_rows), "--repeats", str(a.repeats),
            "--warmup", str(a.warmup)]
    env = dict(os.environ)
    env.pop("DBGPU_LIB", None)
    p = subprocess.run(base + ["--side", "shapes"], stdout=subprocess.PIPE, text=True, env=env, check=True)
    out = json.loads(p.stdout.strip().splitlines()[-1])
    for s, row in out["shapes"].items():
        print(f"{s}  kernel {row['kernel_ms']['median']:.4f} ms ({row['kernel_ms']['min']:.4f}..{row['kernel_ms']['max']:.4f})  "
              f"{row['kernel_TBps']} TB/s  copy {row['copy_ms']['median']:.4f} ms ({row['copy_ms']['min']:.4f}..{row['copy_ms']['max']:.4f}) "
              f"{row['copy_TBps']} TB/s  of copy {row['of_copy']}  of 6.29 TB/s {row['of_6.29_TBps']}  call {row['call_ms']['median']:.4f} ms")
    procs = {}
    for side in ("projected", "precomputed"):
        e = dict(env)
        if side == "precomputed":
            e["DBGPU_LIB"] = os.path.abspath(a.baseline_lib)
        procs[side] = subprocess.Popen(base + ["--side", side], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=e)
    ready = {side: json.loads(p.stdout.readline()) for side, p in procs.items()}
    assert ready["projected"]["results"] == ready["precomputed"]["results"], "the two sides' Q1 results differ"
    samples = {side: {"step_ms": [], "kernel_ms": [], "expr_kernel_ms": []} for side in procs}
    for _ in range(a.repeats):
        for side, p in procs.items():  # alternating
            p.stdin.write("go\n")
            p.stdin.flush()
            r = json.loads(p.stdout.readline())
            for k in samples[side]:
                samples[side][k].append(r[k])
    for p in procs.values():
        p.stdin.write("\n")
        p.stdin.close()
        p.wait()
    q1 = {side: {k: stats(v) for k, v in S.items()} for side, S in samples.items()}
    q1["rows"] = a.q1_rows
    q1["groups"] = len(ready["projected"]["results"])
    q1["projection_cost_step_ms"] = round(q1["projected"]["step_ms"]["median"] - q1["precomputed"]["step_ms"]["median"], 4)
    q1["projection_cost_kernel_ms"] = round(q1["projected"]["kernel_ms"]["median"] - q1["precomputed"]["kernel_ms"]["median"], 4)
    out.update({"rows": a.rows, "repeats": a.repeats, "warmup": a.warmup, "q1": q1})
    print(f"q1  projected step {q1['projected']['step_ms']['median']:.4f} ms  precomputed {q1['precomputed']['step_ms']['median']:.4f} ms  "
          f"projection cost {q1['projection_cost_step_ms']} ms (kernels {q1['projection_cost_kernel_ms']} ms)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
