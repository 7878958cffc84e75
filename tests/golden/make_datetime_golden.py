#!/usr/bin/env python3
"""Extract the reference's recorded date / time function and length() results into a data-only fixture.

  make_datetime_golden.py <databend tree>/src/query/functions/tests/it/scalars/testdata

Reads datetime.txt and string.txt there and writes tests/golden/expr/reference_datetime.json: for
every block whose checked expression is one of the projection's functions applied to a Date or a
Timestamp (a constant made by to_date / to_timestamp, or the column `a`), the date_trunc blocks
included, and for every length() block over a String:
  the function, the ast as the reference printed it (date_trunc(..) where it was one), the operand
  type, the operand values (days, microseconds, or strings), the output type and the output values
  as raw numbers (a Date as days, a Timestamp as microseconds).
to_start_of_week with a mode argument is kept with its "mode".  Nothing but data is written.
"""
import json
import os
import re
import sys

FUNCS = ("to_yyyymm", "to_yyyymmdd", "to_yyyymmddhh", "to_yyyymmddhhmmss", "to_year", "to_quarter", "to_month", "to_day_of_month",
         "to_day_of_week", "to_day_of_year", "to_week_of_year", "to_unix_timestamp", "to_hour", "to_minute", "to_second",
         "to_start_of_second", "to_start_of_minute", "to_start_of_five_minutes", "to_start_of_ten_minutes",
         "to_start_of_fifteen_minutes", "time_slot", "to_start_of_hour", "to_start_of_day", "to_monday", "to_start_of_week",
         "to_start_of_month", "to_start_of_quarter", "to_start_of_year", "to_start_of_iso_year")


def blocks(text):
    return [b for b in re.split(r"\n\s*\n\s*\n", text) if b.strip()]


def field(lines, name):
    for ln in lines:
        if ln.startswith(name):
            return ln.split(":", 1)[1].strip()
    return None


def number(text):
    return int(re.sub(r"_[ui]\d+$", "", text.strip()))


def int_list(text):
    m = re.search(r"\[(.*)\]", text)
    return [int(x) for x in m.group(1).split(",") if x.strip()]


def table_row(lines, name):
    """The cells of the `| name | ... |` row after "evaluation (internal):"."""
    i0 = next(i for i, ln in enumerate(lines) if ln.strip() == "evaluation (internal):")
    for ln in lines[i0:]:
        cells = [c.strip() for c in ln.strip().strip("|").split("|")]
        if cells and cells[0] == name:
            return cells[1]
    return None


def datetime_case(b):
    lines = b.splitlines()
    checked, ast = field(lines, "checked expr"), field(lines, "ast")
    if not checked:
        return None
    m = re.fullmatch(r"(\w+)<(Date|Timestamp)(, Int64)?>\((.*)\)", checked)
    if not m or m.group(1) not in FUNCS:
        return None
    func, kind, arg = m.group(1), m.group(2), m.group(4)
    case = {"func": func, "ast": ast, "type": kind, "output_type": field(lines, "output type")}
    if m.group(3):
        mm = re.search(r", to_int64<UInt8>\((\d+)_u8\)$", arg)
        if not mm:
            return None
        case["mode"] = int(mm.group(1))
        arg = arg[: mm.start()]
    if arg == "a":
        types = next(ln for ln in lines if ln.startswith("| Type"))
        case["output_type"] = [c.strip() for c in types.strip().strip("|").split("|")][-1]
        case["input"] = int_list(table_row(lines, "a"))
        case["output"] = int_list(table_row(lines, "Output"))
        return case
    md = re.fullmatch(r"to_date<Int64>\(to_int64<UInt\d+>\((\d+)_u\d+\)\)", arg)
    mt = re.fullmatch(r"to_timestamp<Int64>\(to_int64<UInt\d+>\((\d+)_u\d+\)\)", arg)
    if kind == "Date" and md:
        case["input"] = [int(md.group(1))]
    elif kind == "Timestamp" and mt:
        case["input"] = [int(mt.group(1)) * 1000000]  # to_timestamp of a number this small reads seconds
    else:
        return None
    case["output"] = [number(field(lines, "optimized expr"))]
    return case


def length_case(b):
    lines = b.splitlines()
    checked = field(lines, "checked expr")
    if not checked:
        return None
    m = re.fullmatch(r"length<String>\((.*)\)", checked)
    if not m:
        return None
    case = {"func": "length", "ast": field(lines, "ast"), "type": "String", "output_type": "UInt64"}
    if m.group(1) == "a":
        rows = [ln for ln in lines if ln.startswith("| Row")]
        case["input"] = [re.fullmatch(r"'(.*)'", [c.strip() for c in ln.strip().strip("|").split("|")][1]).group(1) for ln in rows]
        case["output"] = int_list(table_row(lines, "Output"))
        return case
    ms = re.fullmatch(r'"(.*)"', m.group(1))
    if not ms or "\\" in ms.group(1):
        return None
    case["input"] = [ms.group(1)]
    case["output"] = [number(field(lines, "optimized expr"))]
    return case


def main():
    src = sys.argv[1]
    cases = []
    text = open(os.path.join(src, "datetime.txt"), encoding="utf-8").read()
    cases += [c for c in (datetime_case(b) for b in blocks(text)) if c]
    text = open(os.path.join(src, "string.txt"), encoding="utf-8", errors="replace").read()
    cases += [c for c in (length_case(b) for b in blocks(text)) if c]
    here = os.path.dirname(os.path.abspath(__file__))
    dst = os.path.join(here, "expr", "reference_datetime.json")
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    with open(dst, "w", encoding="utf-8") as f:
        json.dump({"source": "src/query/functions/tests/it/scalars/testdata/{datetime,string}.txt", "cases": cases}, f, indent=1,
                  ensure_ascii=False)
        f.write("\n")
    print(len(cases), "cases ->", dst)


if __name__ == "__main__":
    main()
