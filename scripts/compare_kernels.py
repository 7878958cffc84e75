#!/usr/bin/env python3
"""Compare the gfx950 kernels of two sets of objects, symbol by symbol.

  compare_kernels.py --parent build_parent/agg.o --result build/agg.o build/agg_finalize.o build/agg_export.o \
      [--parent-remarks agg.remarks] [--result-remarks agg.remarks ...] [--table kernel_resources.txt]

Each object is a `hipcc -c` output: its device code object is taken out of the .hip_fatbin
section, unbundled and disassembled.  Two kernels are the same when their instruction text is the
same, ignoring addresses (the comment llvm-objdump puts after every instruction) and the padding
after a kernel's last instruction.  Every kernel of the parent must exist exactly once on the
result side, under the same mangled name.

The remark files are the stderr of the same compile lines with
-Rpass-analysis=kernel-resource-usage added; with them a table of the six resource figures per
kernel is written (--table), one row per kernel, "a->b" where a figure differs.

Exit status 0: everything identical.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
ARCH = os.environ.get("ARCH", "gfx950")
PAD = ("s_nop", "s_code_end", "...")  # "...": llvm-objdump's mark for a run of zero bytes


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def disassemble(obj, tmp):
    """{mangled kernel name: [instruction lines]} of the object's device code."""
    base = os.path.join(tmp, os.path.basename(obj))
    run(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, base + ".fatbin")
    run(f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{ARCH}",
        f"--input={base}.fatbin", f"--output={base}.co")
    kernels = set()
    for line in run(f"{LLVM}/llvm-readelf", "--symbols", "--wide", base + ".co").splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC" and f[6] != "UND":
            kernels.add(f[7])
    text = collections.OrderedDict()
    cur = None
    for line in run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", base + ".co").splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = text.setdefault(m.group(1), []) if m.group(1) in kernels else None
            continue
        if cur is None or not line.strip():
            continue
        if re.match(r"^<.+>:$", line.strip()):  # a local label: keep its name, it carries no address
            cur.append(line.strip())
            continue
        cur.append(re.sub(r"\s*//.*$", "", line).strip())
    for body in text.values():
        while body and body[-1].split()[0] in PAD:
            body.pop()
    return text


def remarks(path):
    """{mangled name: (VGPRs, AGPRs, TotalSGPRs, scratch, LDS, occupancy)} from a remarks file."""
    keys = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    out, name, cur = {}, None, {}
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name, cur = m.group(1), {}
            out[name] = cur
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+)", line)
        if m and name:
            cur[m.group(1).strip()] = m.group(2)
    return {n: tuple(d.get(k, "?") for k in keys) for n, d in out.items()}


def demangle(names):
    out = run("c++filt", *names).splitlines()
    return {n: re.sub(r"^void ", "", re.sub(r"\(.*$", "", d)) for n, d in zip(names, out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--result", nargs="+", required=True)
    ap.add_argument("--parent-remarks", nargs="*", default=[])
    ap.add_argument("--result-remarks", nargs="*", default=[])
    ap.add_argument("--table")
    a = ap.parse_args()
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        sides = []
        for k, objs in enumerate((a.parent, a.result)):
            os.mkdir(os.path.join(tmp, str(k)))
            side = {}
            for o in objs:
                for name, body in disassemble(o, os.path.join(tmp, str(k))).items():
                    side.setdefault(name, []).append((os.path.basename(o), body))
            sides.append(side)
    parent, result = sides
    verdict = {}
    for name, homes in parent.items():
        got = result.get(name, [])
        if len(homes) != 1 or len(got) != 1:
            verdict[name] = f"parent x{len(homes)}, result x{len(got)}"
        elif homes[0][1] != got[0][1]:
            pa, rb = homes[0][1], got[0][1]
            first = next((i for i, (x, y) in enumerate(zip(pa, rb)) if x != y), min(len(pa), len(rb)))
            verdict[name] = f"differs at instruction {first} ({len(pa)} / {len(rb)} lines)"
        else:
            verdict[name] = "identical"
    extra = sorted(set(result) - set(parent))
    bad += sum(v != "identical" for v in verdict.values()) + len(extra)
    n_insn = sum(len(h[0][1]) for h in parent.values())
    print(f"{len(parent)} kernels on the parent side, {sum(len(v) for v in result.values())} on the result side, "
          f"{sum(v == 'identical' for v in verdict.values())} with identical instruction text ({n_insn} lines compared)")
    for name, v in verdict.items():
        if v != "identical":
            print("  ", name, v)
    for name in extra:
        print("   only on the result side:", name)

    if a.table:
        pr, rr = {}, {}
        for f in a.parent_remarks:
            pr.update(remarks(f))
        for f in a.result_remarks:
            rr.update(remarks(f))
        names = demangle(list(parent))
        rows = []
        for name in parent:
            p, r = pr.get(name), rr.get(name)
            unit = f"{parent[name][0][0]} -> {result[name][0][0] if name in result else '-'}".replace(".o", ".hip")
            if not p or not r:
                rows.append((names[name], unit, ["?"] * 6, "no remark"))
                bad += 1
                continue
            cells = [x if x == y else f"{x}->{y}" for x, y in zip(p, r)]
            same = p == r
            bad += not same
            rows.append((names[name], unit, cells, "identical" if same and verdict[name] == "identical" else
                         ("same resources, " + verdict[name] if same else "DIFFERS")))
        rows.sort()
        with open(a.table, "w") as f:
            f.write(f"{'kernel':<78} {'unit (parent -> result)':<32} {'VGPR':>6} {'AGPR':>6} {'SGPR':>6} {'scratch':>8} {'LDS':>7} "
                    f"{'occ':>4}  verdict\n")
            for n, unit, c, v in rows:
                f.write(f"{n:<78} {unit:<32} {c[0]:>6} {c[1]:>6} {c[2]:>6} {c[3]:>8} {c[4]:>7} {c[5]:>4}  {v}\n")
        print(f"{len(rows)} rows -> {a.table}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
