#!/usr/bin/env python3
"""Extract the reference's recorded plus / minus / multiply results into a data-only fixture.

  make_expr_golden.py <databend tree>/src/query/functions/tests/it/scalars/testdata/arithmetic.txt

Writes tests/golden/expr/reference_arithmetic.json: for every two-argument plus, minus and multiply
block whose operand and result types the projection covers (numbers and Decimal128; no Decimal256,
no Decimal mixed with Float), the operator, each argument (a column with its type and rows, or a
typed constant), the output type and the output rows.  Decimal values are kept as the text the
reference printed; NULL is null.  Nothing but data is written.
"""
import json
import os
import re
import sys

OPS = ("plus", "minus", "multiply")
INT_SUFFIX = {"u8": "UInt8", "u16": "UInt16", "u32": "UInt32", "u64": "UInt64", "i8": "Int8", "i16": "Int16", "i32": "Int32",
              "i64": "Int64"}


def split_args(s):
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "(<":
            depth += 1
        elif ch in ")>":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    out.append(cur.strip())
    return out


def parse_arg(a):
    """{"column": name} or {"const": text, "type": type}; None for anything else (a function call)."""
    m = re.fullmatch(r"CAST\((.*) AS ([^()]*(\([^()]*\))?[^()]*)\)", a)
    if m:
        a = m.group(1).strip()
    if re.fullmatch(r"[a-z][a-z0-9_]*", a):
        return {"column": a}
    m = re.fullmatch(r"(-?\d+)_(u8|u16|u32|u64|i8|i16|i32|i64)", a)
    if m:
        return {"const": m.group(1), "type": INT_SUFFIX[m.group(2)]}
    m = re.fullmatch(r"(-?[\d.]+)_d128\((\d+),(\d+)\)", a)
    if m:
        return {"const": m.group(1), "type": f"Decimal({m.group(2)}, {m.group(3)})"}
    return None


def in_scope(t):
    m = re.match(r"Decimal\((\d+), (\d+)\)", t)
    if m:
        return int(m.group(1)) <= 38
    return t.replace(" NULL", "") in ("Int8", "Int16", "Int32", "Int64", "UInt8", "UInt16", "UInt32", "UInt64", "Float32", "Float64")


def blocks(text):
    return [b for b in re.split(r"\n\s*\n\s*\n", text) if b.strip()]


def parse_block(b):
    lines = b.splitlines()
    expr = None
    for ln in lines:
        if ln.startswith("checked expr") or ln.startswith("optimized expr"):
            expr = ln.split(":", 1)[1].strip()
    if expr is None:
        return None
    m = re.fullmatch(r"(plus|minus|multiply)<(.*?)>\((.*)\)", expr)
    if not m:
        return None
    args = split_args(m.group(3))
    if len(args) != 2:
        return None
    parsed = [parse_arg(a) for a in args]
    if any(p is None for p in parsed):
        return None
    try:
        i0 = next(i for i, ln in enumerate(lines) if ln.strip() == "evaluation:")
    except StopIteration:
        return None
    table = [ln for ln in lines[i0 + 1:] if ln.startswith("|")]
    rows = [[c.strip() for c in ln.strip().strip("|").split("|")] for ln in table]
    head = rows[0]
    types = next(r for r in rows if r[0] == "Type")
    data = [r for r in rows if r[0].startswith("Row")]
    cols = {}
    for j, name in enumerate(head):
        if j == 0:
            continue
        cols[name] = {"type": types[j], "rows": [None if r[j] == "NULL" else r[j] for r in data]}
    if "Output" not in cols:
        return None
    out = cols.pop("Output")
    case_args = []
    for p in parsed:
        if "column" in p:
            if p["column"] not in cols:
                return None
            c = cols[p["column"]]
            case_args.append({"column": p["column"], "type": c["type"], "rows": c["rows"]})
        else:
            case_args.append(p)
    if not all(in_scope(a["type"]) for a in case_args) or not in_scope(out["type"]):
        return None
    kinds = ["Decimal" if a["type"].startswith("Decimal") else ("Float" if a["type"].startswith("Float") else "Int") for a in case_args]
    if "Decimal" in kinds and "Float" in kinds:
        return None
    ast = next(ln.split(":", 1)[1].strip() for ln in lines if ln.startswith("ast"))
    return {"ast": ast, "op": m.group(1), "args": case_args, "output_type": out["type"], "output": out["rows"]}


def main():
    src = sys.argv[1]
    text = open(src, encoding="utf-8").read()
    cases = [c for c in (parse_block(b) for b in blocks(text)) if c]
    here = os.path.dirname(os.path.abspath(__file__))
    dst = os.path.join(here, "expr", "reference_arithmetic.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w", encoding="utf-8") as f:
        json.dump({"source": "src/query/functions/tests/it/scalars/testdata/arithmetic.txt", "cases": cases}, f, indent=1)
        f.write("\n")
    print(len(cases), "cases ->", dst)


if __name__ == "__main__":
    main()
