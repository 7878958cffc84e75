"""An independent reference for the projection's date / time functions and length(), in Python
integers: the reference's code restated line by line (FUNCS = src/query/functions/src/scalars,
EXP = src/query/expression/src), session timezone UTC.

  * `to_timestamp` (EXP/utils/date_helper.rs:256-265): secs = us / 10^6 and nanos = us % 10^6 * 1000
    with Rust's truncating `/` and `%`; a negative nanos borrows one second.  Every civil field of a
    Timestamp comes from that floored second, of a Date from its midnight.
  * `ToNumber` (:402-516), `TzLUT::to_hour / to_minute / to_second` (:210-239), `TzLUT::round_us`
    (:147-208, offset_round_hour and offset_round_minute true for UTC) and `DateRounder` (:530-619).
  * `length`: `val.chars().count()` (FUNCS/string.rs:166-170).

The calendar here is the proleptic Gregorian one counted from 0001-01-01 in 400 / 100 / 4 / 1 year
cycles, and the ISO week is that of the week's Thursday: neither is the arithmetic the library uses.
tests/test_datetime_ref.py pins this file by the reference's recorded results and by Python's own
datetime module."""
import numpy as np

from databend_amd import abi
from databend_amd import column as col

MICROS = 10 ** 6
DATE_MIN, DATE_MAX = -354285, 2932896
TS_MIN, TS_MAX = -30610224000000000, 253402300799999999

_DAYS_IN_MONTH = [0, 31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31]
_EPOCH_ORDINAL = 719163  # 1970-01-01 counted from 0001-01-01 = 1


def rust_div(a: int, d: int) -> int:
    """Rust's `/` on integers: towards zero."""
    q = abs(a) // abs(d)
    return q if (a >= 0) == (d > 0) else -q


def rust_rem(a: int, d: int) -> int:
    return a - rust_div(a, d) * d


def is_leap(y: int) -> bool:
    return y % 4 == 0 and (y % 100 != 0 or y % 400 == 0)


def days_before_year(y: int) -> int:
    y -= 1
    return y * 365 + y // 4 - y // 100 + y // 400


def days_before_month(y: int, m: int) -> int:
    return sum(_DAYS_IN_MONTH[1:m]) + (1 if m > 2 and is_leap(y) else 0)


def days_from_civil(y: int, m: int, d: int) -> int:
    return days_before_year(y) + days_before_month(y, m) + d - _EPOCH_ORDINAL


class Civil:
    """chrono's view of one NaiveDateTime: year, month, day, ordinal, weekday (Monday = 0), ISO year
    and week, hour, minute, second, and the day number it came from."""

    def __init__(self, days: int, sod: int = 0):
        self.days = days
        n = days + _EPOCH_ORDINAL - 1
        n400, n = divmod(n, 146097)
        n100, n = divmod(n, 36524)
        n4, n = divmod(n, 1461)
        n1, n = divmod(n, 365)
        y = n400 * 400 + n100 * 100 + n4 * 4 + n1 + 1
        if n1 == 4 or n100 == 4:  # the last day of a leap cycle
            y, n = y - 1, 365
        self.year, self.ordinal = y, n + 1
        m = 1
        while n >= _DAYS_IN_MONTH[m] + (1 if m == 2 and is_leap(y) else 0):
            n -= _DAYS_IN_MONTH[m] + (1 if m == 2 and is_leap(y) else 0)
            m += 1
        self.month, self.day = m, n + 1
        self.wd = (days + 3) % 7  # 1970-01-01 was a Thursday
        self.hour, self.minute, self.second = sod // 3600, sod // 60 % 60, sod % 60

    def iso(self):
        """(ISO year, ISO week): those of the week's Thursday."""
        th = Civil(self.days - self.wd + 3)
        return th.year, (th.ordinal - 1) // 7 + 1


def of_timestamp(us: int) -> Civil:
    secs, nanos = rust_div(us, MICROS), rust_rem(us, MICROS) * 1000
    if nanos < 0:
        secs -= 1
    return Civil(secs // 86400, secs % 86400)


def unix_seconds(us: int) -> int:
    secs = rust_div(us, MICROS)
    return secs - 1 if rust_rem(us, MICROS) < 0 else secs


def start_of_minutes(us: int, minutes: int) -> int:
    d = minutes * 60 * MICROS
    return rust_div(us, d) * d if us > 0 else rust_div(us + MICROS - d, d) * d


def round_down(us: int, seconds: int) -> int:
    d = seconds * MICROS
    return rust_div(us, d) * d if us > 0 else rust_div(us + MICROS - d, d) * d


def start_of_day(us: int) -> int:
    c = of_timestamp(us)
    return days_from_civil(c.year, c.month, c.day) * 86400 * MICROS


def start_of_iso_year(c: Civil) -> int:
    jan4 = Civil(days_from_civil(c.iso()[0], 1, 4))  # always in ISO week 1
    return jan4.days - jan4.wd


# name -> (takes Date, takes Timestamp, result type, value from a Civil)
_CIVIL = {
    "to_yyyymm": (col.UInt32, lambda c: c.year * 100 + c.month),
    "to_yyyymmdd": (col.UInt32, lambda c: c.year * 10000 + c.month * 100 + c.day),
    "to_yyyymmddhh": (col.UInt64, lambda c: c.year * 1000000 + c.month * 10000 + c.day * 100 + c.hour),
    "to_yyyymmddhhmmss": (col.UInt64, lambda c: c.year * 10 ** 10 + c.month * 10 ** 8 + c.day * 10 ** 6 + c.hour * 10 ** 4 + c.minute * 100
                          + c.second),
    "to_year": (col.UInt16, lambda c: c.year),
    "to_quarter": (col.UInt8, lambda c: (c.month - 1) // 3 + 1),
    "to_month": (col.UInt8, lambda c: c.month),
    "to_day_of_month": (col.UInt8, lambda c: c.day),
    "to_day_of_week": (col.UInt8, lambda c: c.wd + 1),
    "to_day_of_year": (col.UInt16, lambda c: c.ordinal),
    "to_week_of_year": (col.UInt32, lambda c: c.iso()[1]),
    "to_monday": (col.Date, lambda c: c.days - c.wd),
    "to_start_of_week": (col.Date, lambda c: c.days - (c.wd + 1) % 7),
    "to_start_of_month": (col.Date, lambda c: days_from_civil(c.year, c.month, 1)),
    "to_start_of_quarter": (col.Date, lambda c: days_from_civil(c.year, (c.month - 1) // 3 * 3 + 1, 1)),
    "to_start_of_year": (col.Date, lambda c: days_from_civil(c.year, 1, 1)),
    "to_start_of_iso_year": (col.Date, start_of_iso_year),
}
_TS_ONLY = {
    "to_unix_timestamp": (col.Int64, unix_seconds),
    "to_hour": (col.UInt8, lambda us: of_timestamp(us).hour),
    # the closed forms of TzLUT::to_minute / to_second hold for us >= 0 only
    "to_minute": (col.UInt8, lambda us: rust_div(rust_div(us, MICROS), 60) % 60 if us >= 0 else of_timestamp(us).minute),
    "to_second": (col.UInt8, lambda us: rust_div(us, MICROS) % 60 if us >= 0 else of_timestamp(us).second),
    "to_start_of_second": (col.Timestamp, lambda us: rust_div(us, MICROS) * MICROS),
    "to_start_of_minute": (col.Timestamp, lambda us: start_of_minutes(us, 1)),
    "to_start_of_five_minutes": (col.Timestamp, lambda us: start_of_minutes(us, 5)),
    "to_start_of_ten_minutes": (col.Timestamp, lambda us: start_of_minutes(us, 10)),
    "to_start_of_fifteen_minutes": (col.Timestamp, lambda us: start_of_minutes(us, 15)),
    "time_slot": (col.Timestamp, lambda us: start_of_minutes(us, 30)),
    "to_start_of_hour": (col.Timestamp, lambda us: round_down(us, 3600)),
    "to_start_of_day": (col.Timestamp, start_of_day),
}
DATE_FUNCS = [n for n in abi.EXPR_FUNC_NAMES if n in _CIVIL]
TS_FUNCS = [n for n in abi.EXPR_FUNC_NAMES if n in _CIVIL or n in _TS_ONLY]
assert len(DATE_FUNCS) == 17 and len(TS_FUNCS) == 29


def takes(name: str, t) -> bool:
    if name == "length":
        return t.type_id == abi.STRING
    return (t.type_id == abi.DATE and name in _CIVIL) or (t.type_id == abi.TIMESTAMP and (name in _CIVIL or name in _TS_ONLY))


def result_type(name: str, t):
    """The result type of name(t): nullable exactly when t is."""
    r = col.UInt64 if name == "length" else (_CIVIL.get(name) or _TS_ONLY[name])[0]
    return r.wrap_nullable() if t.nullable else r


def evaluate(name: str, t, v):
    """name(v) for a Date (days) or Timestamp (microseconds) value, or a str / bytes for length."""
    if name == "length":
        return length(v)
    if name in _TS_ONLY:
        assert t.type_id == abi.TIMESTAMP
        return _TS_ONLY[name][1](v)
    return _CIVIL[name][1](Civil(v) if t.type_id == abi.DATE else of_timestamp(v))


def length(s) -> int:
    """chars().count(): for bytes, those that are not UTF-8 continuation bytes (the same number for
    every valid string)."""
    if isinstance(s, str):
        return len(s)
    return sum(1 for b in s if (b & 0xC0) != 0x80)


# ---- the values every test runs ------------------------------------------------------------------------
DAY_US = 86400 * MICROS


def _d(y, m, d):
    return days_from_civil(y, m, d)


def edge_dates():
    """The epoch +-1 day, the century leap rules, the ISO week 1 / 52 / 53 year ends of 2018-2021 (an
    ISO year that differs from the civil one), a Saturday / Sunday / Monday triple, the valid range's
    ends."""
    out = [0, 1, -1, -100, 100, _d(1900, 2, 28), _d(1900, 3, 1), _d(2000, 2, 29), _d(2000, 3, 1), _d(2100, 2, 28), _d(2100, 3, 1),
           _d(2024, 2, 29), _d(2023, 12, 31)]
    for y in (2018, 2019, 2020, 2021):
        out += [_d(y, 12, 31), _d(y, 1, 1)]
    out += [_d(2021, 9, 4), _d(2021, 9, 5), _d(2021, 9, 6)]  # Saturday, Sunday, Monday
    out += [DATE_MIN, DATE_MIN + 1, DATE_MAX, DATE_MAX - 1]
    return out


def edge_timestamps():
    """Every edge date at its first and last microsecond and at noon, the epoch +-1 us, -100 us and
    -59.9999 s (the rounders' truncation cases), period boundaries either side of zero."""
    out = [0, 1, -1, -100, 100, -59999900, -60000000, -60000001, -MICROS, -MICROS + 1, -MICROS - 1, MICROS, 59 * MICROS, 60 * MICROS,
           -3600 * MICROS, -3600 * MICROS + 1, -1800 * MICROS - 1, 3599999999, 3600000000, 1630812366000000, 1630812366999999]
    for d in edge_dates():
        for us in (d * DAY_US, d * DAY_US + DAY_US - 1, d * DAY_US + 43200 * MICROS + 123456):
            if TS_MIN <= us <= TS_MAX:
                out.append(us)
    out += [TS_MIN, TS_MIN + 1, TS_MAX, TS_MAX - 1]
    return out


def sweep_dates(n: int, seed: int):
    """Seeded days over the whole valid range, years 1000-9999."""
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(DATE_MIN, DATE_MAX + 1, n)]


def sweep_timestamps(n: int, seed: int):
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(TS_MIN, TS_MAX + 1, n)]


LENGTH_STRINGS = ["", "a", "latin", "CAFÉ", "数据库", "кириллица and latin", "\U0001f600\U0001f680", "x" * 15,
                  "x" * 16, "x" * 17, "é" * 8, "é" * 7 + "ab", "€" * 5 + "z"]
