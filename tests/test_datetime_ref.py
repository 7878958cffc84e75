"""tests/datetime_ref.py pinned two ways: by the reference's recorded results
(tests/golden/expr/reference_datetime.json, written by tests/golden/make_datetime_golden.py from the
reference's testdata/datetime.txt and string.txt) and by Python's own datetime module for every
civil field and ISO week over seeded days and microseconds of the whole valid range, years
1000-9999, plus every edge value the other tests run."""
import datetime as dt
import json
import os

import pytest

from databend_amd import abi
from databend_amd import column as col
from tests import datetime_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "expr", "reference_datetime.json"), encoding="utf-8"))["cases"]
TYPES = {"Date": col.Date, "Timestamp": col.Timestamp, "String": col.String, "UInt8": col.UInt8, "UInt16": col.UInt16,
         "UInt32": col.UInt32, "UInt64": col.UInt64, "Int64": col.Int64}
EPOCH = dt.datetime(1970, 1, 1)


def test_fixture_covers_what_the_reference_records():
    funcs = {(c["func"], c["type"]) for c in GOLDEN}
    assert len(GOLDEN) >= 70
    # every to-number function the reference's file exercises, on constants and on column a = [-100, 0, 100]
    for f in ("to_yyyymm", "to_yyyymmdd", "to_yyyymmddhhmmss", "to_year", "to_quarter", "to_month", "to_day_of_year", "to_day_of_month",
              "to_day_of_week", "to_week_of_year"):
        assert (f, "Date") in funcs and (f, "Timestamp") in funcs
        assert any(c["func"] == f and c["input"] == [-100, 0, 100] for c in GOLDEN)
    for f in D.TS_FUNCS:
        if f not in ("to_yyyymmddhh", "to_unix_timestamp"):  # the reference's file has no block of these two
            assert (f, "Timestamp") in funcs, f
    assert sum(c["ast"].startswith("date_trunc(") for c in GOLDEN) == 7
    assert ("length", "String") in funcs


@pytest.mark.parametrize("k", range(len(GOLDEN)), ids=[f"{i}-{c['func']}-{c['type']}" for i, c in enumerate(GOLDEN)])
def test_reference_recorded_results(k):
    c = GOLDEN[k]
    t = TYPES[c["type"]]
    name = c["func"]
    if c.get("mode") == 1:
        name = "to_monday"  # to_start_of_week(x, 1) is ToLastMonday
    assert D.takes(name, t)
    assert D.result_type(name, t) == TYPES[c["output_type"]]
    assert [D.evaluate(name, t, v) for v in c["input"]] == c["output"], c["ast"]


def test_date_trunc_maps_to_the_references_rewrite():
    from databend_amd import expr as X
    seen = 0
    for c in GOLDEN:
        if c["ast"].startswith("date_trunc("):
            unit = c["ast"][len("date_trunc("):].split(",")[0]
            e = X.date_trunc(unit, X.col(0))
            assert e.name == c["func"], (unit, e.name)
            assert (TYPES[c["output_type"]] == col.Date) == (unit in ("year", "quarter", "month"))
            seen += 1
    assert seen == 7


def check_against_python(c: D.Civil, d: dt.datetime):
    iso = d.isocalendar()
    assert (c.year, c.month, c.day, c.hour, c.minute, c.second) == (d.year, d.month, d.day, d.hour, d.minute, d.second)
    assert c.ordinal == d.timetuple().tm_yday and c.wd == d.weekday()
    assert c.iso() == (iso[0], iso[1])


def test_civil_fields_against_python_datetime():
    days = D.edge_dates() + D.sweep_dates(4000, 11)
    for n in days:
        d = EPOCH + dt.timedelta(days=n)
        c = D.Civil(n)
        check_against_python(c, d)
        t = col.Date
        assert D.evaluate("to_monday", t, n) == n - d.weekday()
        assert D.evaluate("to_start_of_week", t, n) == n - (d.weekday() + 1) % 7
        assert D.evaluate("to_start_of_month", t, n) == (d.replace(day=1) - EPOCH).days
        assert D.evaluate("to_start_of_quarter", t, n) == (d.replace(month=(d.month - 1) // 3 * 3 + 1, day=1) - EPOCH).days
        assert D.evaluate("to_start_of_year", t, n) == (d.replace(month=1, day=1) - EPOCH).days
        iso_year = d.isocalendar()[0]
        assert D.evaluate("to_start_of_iso_year", t, n) == (dt.datetime.strptime(f"{iso_year}-W01-1", "%G-W%V-%u") - EPOCH).days
        assert D.evaluate("to_yyyymmdd", t, n) == int(d.strftime("%Y%m%d"))
        assert D.evaluate("to_week_of_year", t, n) == d.isocalendar()[1]
        assert D.evaluate("to_day_of_week", t, n) == d.isoweekday()
    assert min(days) == D.DATE_MIN and max(days) == D.DATE_MAX
    assert EPOCH + dt.timedelta(days=D.DATE_MIN) == dt.datetime(1000, 1, 1) and EPOCH + dt.timedelta(days=D.DATE_MAX) == dt.datetime(9999, 12, 31)


def test_timestamp_fields_against_python_datetime():
    t = col.Timestamp
    stamps = D.edge_timestamps() + D.sweep_timestamps(4000, 12)
    for us in stamps:
        d = EPOCH + dt.timedelta(microseconds=us)  # timedelta normalises a negative count by flooring, as to_timestamp does
        check_against_python(D.of_timestamp(us), d)
        assert D.evaluate("to_unix_timestamp", t, us) == us // D.MICROS
        assert D.evaluate("to_hour", t, us) == d.hour and D.evaluate("to_minute", t, us) == d.minute
        assert D.evaluate("to_second", t, us) == d.second
        assert D.evaluate("to_yyyymmddhhmmss", t, us) == int(d.strftime("%Y%m%d%H%M%S"))
        assert D.evaluate("to_yyyymmddhh", t, us) == int(d.strftime("%Y%m%d%H"))
        assert D.evaluate("to_start_of_day", t, us) == (d.replace(hour=0, minute=0, second=0, microsecond=0) - EPOCH).days * D.DAY_US
        if us > 0:  # after the epoch the rounders are what a calendar gives
            assert D.evaluate("to_start_of_minute", t, us) == us - us % (60 * D.MICROS)
            assert D.evaluate("to_start_of_fifteen_minutes", t, us) == us - us % (900 * D.MICROS)
            assert D.evaluate("to_start_of_hour", t, us) == us - us % (3600 * D.MICROS)
            assert D.evaluate("to_start_of_second", t, us) == us - us % D.MICROS
    assert min(stamps) == D.TS_MIN and max(stamps) == D.TS_MAX


def test_rounders_before_the_epoch_follow_the_code_as_written():
    """The reference's recorded results pin the before-epoch cases only for the to-number family; for
    the rounders the code alone does: truncating division, and (us + 10^6 - d) / d * d for us <= 0."""
    t = col.Timestamp
    m = D.MICROS
    assert D.evaluate("to_start_of_second", t, -100) == 0            # -100 / 10^6 truncates to 0
    assert D.evaluate("to_start_of_second", t, -m - 1) == -m
    assert D.evaluate("to_start_of_minute", t, -100) == 0            # (-100 + 10^6 - 6 * 10^7) / (6 * 10^7) truncates to 0
    assert D.evaluate("to_start_of_minute", t, -59999900) == -60 * m  # -118999900 / (6 * 10^7) truncates to -1
    assert D.evaluate("to_start_of_minute", t, -m) == -60 * m
    assert D.evaluate("to_start_of_minute", t, -m + 1) == 0
    assert D.evaluate("to_start_of_minute", t, 0) == 0
    assert D.evaluate("to_start_of_hour", t, -3600 * m) == -3600 * m and D.evaluate("to_start_of_hour", t, -3600 * m - m) == -7200 * m
    assert D.evaluate("time_slot", t, -1800 * m - 1) == -1800 * m
    # the fields come from the floored second
    assert D.evaluate("to_second", t, -100) == 59 and D.evaluate("to_minute", t, -100) == 59 and D.evaluate("to_hour", t, -100) == 23
    assert D.evaluate("to_unix_timestamp", t, -100) == -1 and D.evaluate("to_unix_timestamp", t, -m) == -1
    assert D.evaluate("to_start_of_day", t, -100) == -D.DAY_US


def test_length_is_len_of_python_strings():
    for s in D.LENGTH_STRINGS + [c for g in GOLDEN if g["func"] == "length" for c in g["input"]]:
        assert D.length(s) == len(s) == D.length(s.encode("utf-8"))
    assert D.length(b"\x80\x80a\xbf") == 1 and D.length(b"\xc3") == 1  # stray continuation bytes do not count, nothing raises


def test_types_and_domains():
    for name in abi.EXPR_FUNC_NAMES:
        for t in (col.Date, col.Timestamp, col.String):
            if D.takes(name, t):
                assert D.result_type(name, t.wrap_nullable()) == D.result_type(name, t).wrap_nullable()
    assert not D.takes("to_hour", col.Date) and not D.takes("to_unix_timestamp", col.Date) and D.takes("to_yyyymmddhh", col.Date)
    assert not D.takes("length", col.Date) and not D.takes("to_year", col.String)
