"""The projection's date / time functions and length() beside a device-to-device copy of the same
traffic (the method of scripts/bench_expr.py).

  m   to_minute(Timestamp) -> UInt8                 reads 8, writes 1 byte per row
  y   to_year(Date) -> UInt16                       reads 4, writes 2
  s   to_start_of_minute(Timestamp) -> Timestamp    reads 8, writes 8
  l   length(String) -> UInt64 over the generator's string column (workloads config 5): the pre-pass
      reads rows + 1 offsets and every byte of the blob and writes 8 bytes per row; the node loop
      then copies that column to the output (reads 8, writes 8).  Both kernels count.

One process, --rows device-resident rows (default 2^26): two warm-up repeats of every shape, then
--repeats timed ones.  Each repeat runs the projection and, right after it, the yardstick: one
device-to-device copy whose read plus write traffic equals the bytes the shape must read and write,
timed with HIP events.  The projection's kernel time is the library's own HIP-event scopes
(expr_eval_narrow, and expr_length for the pre-pass).  Per shape: median (min..max), bytes over
kernel time, that rate over the copy's rate and over the 6.29 TB/s copy bandwidth of the MI355X.

    python scripts/bench_expr_funcs.py [--rows N] [--repeats R] [--warmup W] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
COPY_TBS = 6.29
SHAPES = ["m", "y", "s", "l"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 26)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expr", "bench_expr_funcs.json"))
    return ap.parse_args()


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    a = parse()
    sys.path.insert(0, ROOT)
    import torch

    from databend_amd import abi, ffi, workloads
    from databend_amd import column as col
    from databend_amd import device
    from databend_amd import expr as X
    from databend_amd.device import DeviceColumn
    from databend_amd.ffi import check, lib

    n = a.rows
    g = torch.Generator(device="cuda").manual_seed(37)
    # 2013-07: ClickBench's month, in microseconds; dates over TPC-H's seven years
    ts = torch.randint(1372636800, 1375315200, (n,), device="cuda", generator=g, dtype=torch.int64) * 1000000
    ts += torch.randint(0, 1000000, (n,), device="cuda", generator=g, dtype=torch.int64)
    dates = torch.randint(8035, 10591, (n,), device="cuda", generator=g, dtype=torch.int32)
    t_col = DeviceColumn(col.Timestamp, ts.view(torch.uint8), None, None, n)
    d_col = DeviceColumn(col.Date, dates.view(torch.uint8), None, None, n)
    s_col = workloads.generate_device(5, n)["SearchPhrase"]
    blob = int(s_col.offsets[-1].item())
    c0 = X.col(0)
    programs = {
        "m": (X.ExprProgram([X.to_minute(c0)], [t_col]), 9 * n),
        "y": (X.ExprProgram([X.to_year(c0)], [d_col]), 6 * n),
        "s": (X.ExprProgram([X.to_start_of_minute(c0)], [t_col]), 16 * n),
        "l": (X.ExprProgram([X.length(c0)], [s_col]), 8 * (n + 1) + blob + 8 * n + 16 * n),
    }
    state = {}
    for s, (prog, by) in programs.items():
        outs = [device.empty(t, n) for t in prog.result_types()]
        arr = (abi.dbg_out_column * len(outs))()
        for i, o in enumerate(outs):
            arr[i].data = o.data.data_ptr()
        state[s] = dict(prog=prog, outs=outs, arr=arr, src=torch.empty(by // 2, dtype=torch.uint8, device="cuda").zero_(),
                        dst=torch.empty(by // 2, dtype=torch.uint8, device="cuda"), bytes=by)
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
    samples = {s: {"kernel_ms": [], "length_kernel_ms": [], "call_ms": [], "copy_ms": []} for s in SHAPES}
    for _ in range(a.repeats):
        for s in SHAPES:
            ffi.prof_reset()
            ffi.prof_enable(True)
            eval_(s)
            torch.cuda.synchronize()
            ffi.prof_enable(False)
            prof = {k: v[0] for k, v in ffi.prof_read().items()}
            samples[s]["kernel_ms"].append(sum(v for k, v in prof.items() if k.startswith("expr_")))
            samples[s]["length_kernel_ms"].append(prof.get("expr_length", 0.0))
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
        if s == "l":
            lm = statistics.median(S["length_kernel_ms"])
            pre = 8 * (n + 1) + blob + 8 * n
            row.update({"blob_bytes": blob, "mean_length_bytes": round(blob / n, 2), "length_kernel_ms": stats(S["length_kernel_ms"]),
                        "length_kernel_bytes": pre, "length_kernel_TBps": round(pre / (lm * 1e-3) / 1e12, 3)})
        out[s] = row
        print(f"{s}  kernel {row['kernel_ms']['median']:.4f} ms ({row['kernel_ms']['min']:.4f}..{row['kernel_ms']['max']:.4f})  "
              f"{row['kernel_TBps']} TB/s  copy {row['copy_ms']['median']:.4f} ms ({row['copy_ms']['min']:.4f}..{row['copy_ms']['max']:.4f}) "
              f"{row['copy_TBps']} TB/s  of copy {row['of_copy']}  of 6.29 TB/s {row['of_6.29_TBps']}  call {row['call_ms']['median']:.4f} ms")
    res = {"rows": n, "repeats": a.repeats, "warmup": a.warmup, "shapes": out}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
