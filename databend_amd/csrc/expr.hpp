// expr.hpp — scalar projection in front of the aggregate: plus / minus / multiply over numbers and
// Decimal128, the date / time functions and length() (BlockOperator::Map -> Evaluator::run,
// SQL/evaluator/block_operator.rs:50-80).
//
// Two halves, both plain C++ so that a host build (tests/csrc/expr_host_main.cpp, under ASan and
// UBSan) runs the very source the kernel compiles, as like.hpp and zstd_dev.hpp do:
//  * expr_compile: the one place a program is checked and typed.  It walks the caller's postfix
//    dbg_expr_program, decides every node's type by the reference's rules and lowers it to ENodes
//    whose operand classes, power-of-ten factors and range limits are resolved.
//  * expr_num / expr_dec_add / expr_dec_mul / expr_func: one operator on one row, called by
//    expr_kernel (expr.hip) and by the host build.  All wrapping arithmetic is done in unsigned types.
//
// The rules, restated from the reference (FUNCS = src/query/functions/src/scalars):
//  Numbers (FUNCS/arithmetic.rs:91-175 with ResultTypeOfBinary): plus / multiply give an integer of
//    min(64, 2 x the wider operand) bits, signed if either operand is; minus the same width, always
//    signed; any Float32 / Float64 operand makes the result Float64.  Operands are converted as
//    Rust's `as` does, then the operation runs in the result type.  A result narrower than 64 bits
//    cannot overflow (it has twice the operands' bits); a 64-bit integer result wraps, which is
//    what the reference's release build does — nothing else in the reference pins that case.
//    Every float operation rounds on its own (no fused multiply-add).
//  Decimal128 (EXP/types/decimal.rs:1000-1067 binary_result_type, FUNCS/decimal/arithmetic.rs:75-172):
//    an integer operand is first the decimal of get_decimal_properties (EXP/types/number.rs:475-484):
//    8-bit (3,0), 16-bit (5,0), 32-bit (10,0), Int64 (19,0), UInt64 (20,0).
//    plus / minus: scale s = max(sa, sb), precision p = min(38, max(la, lb) + s + 1) with l = p - s.
//      Both operands are cast to (p, s): a cast that raises the scale (and every integer operand's)
//      multiplies by 10^(s - sx) and fails when the product leaves +-(10^p - 1)
//      (FUNCS/decimal/cast.rs:489-525, 686-707); a cast at the same scale copies.  The sum is
//      checked against +-(10^p - 1) only when p = 38.
//    multiply: s = min(sa + sb, max(sa, sb, 12)), p = min(38, la + lb + s); the value is do_round_mul
//      (decimal.rs:465-478): the full 256-bit product, plus half of 10^(sa + sb - s) away from zero,
//      divided truncating; it fails only when the quotient leaves the i128 range.
//  NULLs (EXP/function.rs:562-571, 660-710): the result is nullable if an operand is, its validity
//    the AND of theirs; a NULL row raises nothing and its data are unspecified.
//  Date / time functions (FUNCS/datetime.rs:1098-1388 register_to_number_functions, :1611-1862
//    register_rounder_functions; values EXP/utils/date_helper.rs), session timezone UTC only:
//    a Timestamp is first its floored second (to_timestamp, date_helper.rs:256-265: secs = us / 10^6
//    truncating, minus one when the remainder is negative), a Date its midnight; the civil fields
//    come from expr_civil below.  to_minute / to_second take `us / 10^6 / 60 % 60` only for us >= 0
//    (:210-228), where truncating and flooring agree, so the floored second serves every sign.
//    The sub-day rounders (TzLUT::round_us, :147-208) are kept as written, truncation and all:
//    expr_round_us.  Round::Day and the Date rounders (DateRounder, :530-619) rebuild from the
//    floored civil date.  Closed-form integer arithmetic only: a value outside the reference's valid
//    ranges gives an unspecified result, never a fault, and no table is indexed by a data value.
//  length (FUNCS/string.rs:166-170): val.chars().count().  It does not run in the node loop: the
//    host lowers `column, length` to a read of a UInt64 column that a pre-pass fills (expr.hip).
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/dbgpu_agg.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EXPR_HD __host__ __device__ __forceinline__
#else
#define EXPR_HD inline
#endif

typedef unsigned __int128 expr_u128;

// ---- the lowered program --------------------------------------------------------------------
enum { EX_COL = 0, EX_CONST = 1, EX_NUM = 2, EX_DADD = 3, EX_DMUL = 4, EX_STORE = 5, EX_FUNC = 6, EX_NOP = 7 };
enum { EX_PLUS = 0, EX_MINUS = 1, EX_MUL = 2 };
enum { EC_SINT = 0, EC_UINT = 1, EC_F64 = 2, EC_DEC = 3 };  // how a value sits in its 64 / 128 bits

// Values are canonical: integers sign- or zero-extended to 64 bits (to 128 where a program holds a
// Decimal128), floats as the bits of a double, decimals as i128.  Every operator leaves its result
// canonical (a number operator in a 128-bit program through expr_num_hi).
struct ENode {
    uint8_t op;       // EX_*
    uint8_t arith;    // EX_PLUS / EX_MINUS / EX_MUL;  EX_FUNC: the dbg_expr_func
    uint8_t cls_a;    // EX_NUM into Float64: EC_* of each operand;  EX_FUNC: 1 = the operand is a Timestamp, 0 = a Date
    uint8_t cls_b;
    uint8_t to_f64;   // EX_NUM: the operation runs in Float64
    uint8_t flags;    // EX_DADD: EX_F_*;  EX_STORE: EX_F_POP
    uint8_t k;        // EX_DMUL: the divisor is 10^k
    uint8_t cls_r;    // EX_NUM, EX_FUNC: EC_* of the result (its extension to 128 bits in a wide program)
    int32_t idx;      // EX_COL: column;  EX_STORE: output
    int32_t reserved2;
    uint64_t c[2];    // EX_CONST: the value
    // EX_DADD: operand x is multiplied by fx (10^(s - sx)) when EX_F_SCALE_x, after |x| <= lx
    // ((10^p - 1) / fx) was checked.  EX_DMUL: fa = half the divisor, la = {d1, d2} with
    // 10^k = d1 * d2, both <= 10^19.
    uint64_t fa[2], la[2], fb[2], lb[2];
};
enum { EX_F_SCALE_A = 1, EX_F_SCALE_B = 2, EX_F_CHECK38 = 4, EX_F_POP = 8 };

#define DBG_EXPR_STACK 4

// ---- one operator on one row ---------------------------------------------------------------
EXPR_HD double expr_bits_f64(uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}
EXPR_HD uint64_t expr_f64_bits(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}
EXPR_HD double expr_to_f64(int cls, uint64_t v) {
    return cls == EC_F64 ? expr_bits_f64(v) : (cls == EC_SINT ? (double)(int64_t)v : (double)v);
}

// plus / minus / multiply of two numbers in the node's result type
EXPR_HD uint64_t expr_num(const ENode& n, uint64_t a, uint64_t b) {
    if (n.to_f64) {
#pragma clang fp contract(off)
        const double x = expr_to_f64(n.cls_a, a), y = expr_to_f64(n.cls_b, b);
        const double r = n.arith == EX_PLUS ? x + y : (n.arith == EX_MINUS ? x - y : x * y);
        return expr_f64_bits(r);
    }
    return n.arith == EX_PLUS ? a + b : (n.arith == EX_MINUS ? a - b : a * b);
}

// High word of a number operator's result where values are 128 bits wide (a program that holds a
// Decimal128): the sign extension of a signed integer, zero for an unsigned one or a float — the
// canonical form a later decimal operator reads.
EXPR_HD uint64_t expr_num_hi(const ENode& n, uint64_t lo) { return n.cls_r == EC_SINT ? (uint64_t)((int64_t)lo >> 63) : 0; }

struct EU128 {
    uint64_t lo, hi;
};
EXPR_HD EU128 eu128_neg(EU128 a) {
    EU128 r;
    r.lo = ~a.lo + 1;
    r.hi = ~a.hi + (r.lo == 0 ? 1 : 0);
    return r;
}
EXPR_HD EU128 eu128_abs(EU128 a) { return (a.hi >> 63) ? eu128_neg(a) : a; }
EXPR_HD bool eu128_gt(EU128 a, uint64_t blo, uint64_t bhi) { return a.hi != bhi ? a.hi > bhi : a.lo > blo; }
EXPR_HD uint64_t expr_mulhi(uint64_t a, uint64_t b) { return (uint64_t)(((expr_u128)a * b) >> 64); }
// low 128 bits of a * f (the same bits for signed and unsigned operands)
EXPR_HD EU128 eu128_mul_lo(EU128 a, uint64_t flo, uint64_t fhi) {
    EU128 r;
    r.lo = a.lo * flo;
    r.hi = expr_mulhi(a.lo, flo) + a.lo * fhi + a.hi * flo;
    return r;
}
// 10^38 - 1
#define EXPR_DEC38_HI 0x4B3B4CA85A86C47AULL
#define EXPR_DEC38_LO 0x098A223FFFFFFFFFULL

// The cast of one plus / minus operand to the result type: false when it leaves the precision.
EXPR_HD bool expr_dec_cast(EU128& x, const uint64_t f[2], const uint64_t lim[2]) {
    const bool ok = !eu128_gt(eu128_abs(x), lim[0], lim[1]);
    x = eu128_mul_lo(x, f[0], f[1]);
    return ok;
}

// Decimal plus / minus; *err is set when a cast or the precision-38 range check fails.
EXPR_HD EU128 expr_dec_add(const ENode& n, EU128 a, EU128 b, bool* err) {
    bool ok = true;
    if (n.flags & EX_F_SCALE_A) ok = expr_dec_cast(a, n.fa, n.la) && ok;
    if (n.flags & EX_F_SCALE_B) ok = expr_dec_cast(b, n.fb, n.lb) && ok;
    if (n.arith == EX_MINUS) b = eu128_neg(b);  // wraps for i128::MIN exactly as a - b does
    EU128 r;
    r.lo = a.lo + b.lo;
    r.hi = a.hi + b.hi + (r.lo < a.lo ? 1 : 0);
    if ((n.flags & EX_F_CHECK38) && eu128_gt(eu128_abs(r), EXPR_DEC38_LO, EXPR_DEC38_HI)) ok = false;
    *err = !ok;
    return r;
}

// (hi:lo) / d for hi < d: the quotient fits 64 bits; *r = remainder
EXPR_HD uint64_t expr_div128_64(uint64_t hi, uint64_t lo, uint64_t d, uint64_t* r) {
    uint64_t q = 0, rr = hi;
    for (int b = 63; b >= 0; --b) {
        const uint64_t top = rr >> 63;
        rr = (rr << 1) | ((lo >> b) & 1);
        if (top || rr >= d) {
            rr -= d;
            q |= 1ULL << b;
        }
    }
    *r = rr;
    return q;
}
// w /= d, truncating (d > 0), most significant word first; words whose quotient digit is zero cost nothing
EXPR_HD void expr_u256_div(uint64_t& w0, uint64_t& w1, uint64_t& w2, uint64_t& w3, uint64_t d) {
    uint64_t r = 0;
#define EXPR_DIV_STEP(w)                          \
    if (r == 0 && (w) < d) {                      \
        r = (w);                                  \
        (w) = 0;                                  \
    } else {                                      \
        (w) = expr_div128_64(r, (w), d, &r);      \
    }
    EXPR_DIV_STEP(w3)
    EXPR_DIV_STEP(w2)
    EXPR_DIV_STEP(w1)
    EXPR_DIV_STEP(w0)
#undef EXPR_DIV_STEP
}

// do_round_mul: (a * b +- 10^k / 2) / 10^k truncating, in 256 bits; *err when the quotient is no i128.
EXPR_HD EU128 expr_dec_mul(const ENode& n, EU128 a, EU128 b, bool* err) {
    const bool neg = (a.hi >> 63) != (b.hi >> 63);
    const EU128 x = eu128_abs(a), y = eu128_abs(b);
    // |a| * |b| <= 2^254: four 64 x 64 partial products
    const expr_u128 p00 = (expr_u128)x.lo * y.lo, p01 = (expr_u128)x.lo * y.hi, p10 = (expr_u128)x.hi * y.lo,
                    p11 = (expr_u128)x.hi * y.hi;
    uint64_t w0 = (uint64_t)p00;
    expr_u128 t = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;
    uint64_t w1 = (uint64_t)t;
    t = (t >> 64) + (p01 >> 64) + (p10 >> 64) + (uint64_t)p11;
    uint64_t w2 = (uint64_t)t;
    uint64_t w3 = (uint64_t)((t >> 64) + (p11 >> 64));
    if (n.k) {
        // + half the divisor (the magnitude rounds the same way for both signs: truncation is symmetric)
        expr_u128 s = (expr_u128)w0 + n.fa[0];
        w0 = (uint64_t)s;
        s = (s >> 64) + w1 + n.fa[1];
        w1 = (uint64_t)s;
        s = (s >> 64) + w2;
        w2 = (uint64_t)s;
        w3 += (uint64_t)(s >> 64);
        expr_u256_div(w0, w1, w2, w3, n.la[0]);
        if (n.la[1] > 1) expr_u256_div(w0, w1, w2, w3, n.la[1]);  // 10^k > 10^19: two truncating divisions
    }
    // the signed quotient must lie in [-2^127, 2^127 - 1]
    bool bad = (w2 | w3) != 0;
    if (w1 >> 63) bad = bad || !(neg && w1 == 0x8000000000000000ULL && w0 == 0);
    *err = bad;
    EU128 r{w0, w1};
    return neg ? eu128_neg(r) : r;
}

// ---- date / time functions on one row -----------------------------------------------------------
// The Gregorian date of day number `days` (0 = 1970-01-01): chrono's year / month / day / ordinal /
// weekday / iso_week for the NaiveDate that to_date and to_timestamp give.  Shared by the kernel and
// the host build.  Unsigned 32-bit arithmetic throughout (every division is by a constant): the day
// count from 0000-03-01 is positive for every valid Date (>= -354285), anything else wraps to an
// unspecified result.
struct ECivil {
    uint32_t year, month, day;  // month and day from 1
    uint32_t ordinal;           // day of the year from 1
    uint32_t wd;                // weekday, Monday = 0
    uint32_t iso_year, iso_week;
};
EXPR_HD uint32_t expr_dec31_weekday(uint32_t y) { return (y + y / 4u - y / 100u + y / 400u) % 7u; }  // 0 = Sunday
// an ISO year has 53 weeks when it ends on a Thursday or the one before it ended on a Wednesday
EXPR_HD uint32_t expr_iso_long_year(uint32_t y) { return (expr_dec31_weekday(y) == 4u || expr_dec31_weekday(y - 1u) == 3u) ? 1u : 0u; }
EXPR_HD ECivil expr_civil(int64_t days) {
    ECivil c;
    const uint32_t z = (uint32_t)((uint64_t)days + 719468u);  // days since 0000-03-01
    const uint32_t era = z / 146097u, doe = z - era * 146097u;
    const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;
    const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);  // from March 1st
    const uint32_t mp = (5u * doy + 2u) / 153u;                      // March = 0
    c.day = doy - (153u * mp + 2u) / 5u + 1u;
    c.month = mp < 10u ? mp + 3u : mp - 9u;
    c.year = yoe + era * 400u + (c.month <= 2u ? 1u : 0u);
    const uint32_t leap = (c.year % 4u == 0u && (c.year % 100u != 0u || c.year % 400u == 0u)) ? 1u : 0u;
    c.ordinal = mp < 10u ? doy + 60u + leap : doy - 305u;
    c.wd = (z + 2u) % 7u;  // 0000-03-01 was a Wednesday
    // ISO 8601: the week of the year's Thursday
    uint32_t w = (c.ordinal + 9u - c.wd) / 7u;
    c.iso_year = c.year;
    if (w == 0u) {
        c.iso_year = c.year - 1u;
        w = 52u + expr_iso_long_year(c.year - 1u);
    } else if (w == 53u && !expr_iso_long_year(c.year)) {
        c.iso_year = c.year + 1u;
        w = 1u;
    }
    c.iso_week = w;
    return c;
}

// a / d rounded down, d > 0 (Rust's `/` truncates: the reference subtracts one where the remainder is negative)
EXPR_HD int64_t expr_floor_div(int64_t a, int64_t d) {
    const int64_t q = a / d;
    return q - ((a - q * d) < 0 ? 1 : 0);
}
// TzLUT::start_of_minutes / round_down with offset_round_minute / _hour true (date_helper.rs:159-187),
// d = the period in microseconds: truncating division on both branches, as written
EXPR_HD int64_t expr_round_us(int64_t us, int64_t d) {
    if (us > 0) return us / d * d;
    const int64_t t = (int64_t)((uint64_t)us + 1000000u - (uint64_t)d);
    return t / d * d;
}

// One function on one row: v canonical (a Date sign-extended or not: its low 32 bits are read), the
// result canonical.  Every division is by a literal, so the kernel holds no division routine.
EXPR_HD uint64_t expr_func(const ENode& n, uint64_t v) {
    const int f = n.arith;
    const int64_t us = (int64_t)v;
    switch (f) {
        case DBG_FUNC_TO_START_OF_SECOND: return (uint64_t)(us / 1000000 * 1000000);
        case DBG_FUNC_TO_START_OF_MINUTE: return (uint64_t)expr_round_us(us, 60000000LL);
        case DBG_FUNC_TO_START_OF_FIVE_MINUTES: return (uint64_t)expr_round_us(us, 300000000LL);
        case DBG_FUNC_TO_START_OF_TEN_MINUTES: return (uint64_t)expr_round_us(us, 600000000LL);
        case DBG_FUNC_TO_START_OF_FIFTEEN_MINUTES: return (uint64_t)expr_round_us(us, 900000000LL);
        case DBG_FUNC_TIME_SLOT: return (uint64_t)expr_round_us(us, 1800000000LL);
        case DBG_FUNC_TO_START_OF_HOUR: return (uint64_t)expr_round_us(us, 3600000000LL);
        default: break;
    }
    int64_t days, secs = 0;
    uint32_t sod = 0;  // second of the day
    if (n.cls_a) {
        secs = expr_floor_div(us, 1000000);
        days = expr_floor_div(secs, 86400);
        sod = (uint32_t)(secs - days * 86400);
    } else {
        days = (int64_t)(int32_t)(uint32_t)v;
    }
    if (f == DBG_FUNC_TO_UNIX_TIMESTAMP) return (uint64_t)secs;
    if (f == DBG_FUNC_TO_START_OF_DAY) return (uint64_t)days * 86400000000ULL;
    const uint32_t hh = sod / 3600u, mi = sod / 60u % 60u, ss = sod % 60u;
    if (f == DBG_FUNC_TO_HOUR) return hh;
    if (f == DBG_FUNC_TO_MINUTE) return mi;
    if (f == DBG_FUNC_TO_SECOND) return ss;
    const ECivil c = expr_civil(days);
    const uint64_t d = (uint64_t)days;  // Date results wrap like the rest
    switch (f) {
        case DBG_FUNC_TO_YYYYMM: return c.year * 100u + c.month;
        case DBG_FUNC_TO_YYYYMMDD: return c.year * 10000u + c.month * 100u + c.day;
        case DBG_FUNC_TO_YYYYMMDDHH: return (uint64_t)c.year * 1000000u + c.month * 10000u + c.day * 100u + hh;
        case DBG_FUNC_TO_YYYYMMDDHHMMSS:
            return (uint64_t)c.year * 10000000000ULL + (uint64_t)c.month * 100000000u + c.day * 1000000u + hh * 10000u + mi * 100u + ss;
        case DBG_FUNC_TO_YEAR: return c.year & 0xffffu;
        case DBG_FUNC_TO_QUARTER: return (c.month - 1u) / 3u + 1u;
        case DBG_FUNC_TO_MONTH: return c.month;
        case DBG_FUNC_TO_DAY_OF_MONTH: return c.day;
        case DBG_FUNC_TO_DAY_OF_WEEK: return c.wd + 1u;
        case DBG_FUNC_TO_DAY_OF_YEAR: return c.ordinal;
        case DBG_FUNC_TO_WEEK_OF_YEAR: return c.iso_week;
        case DBG_FUNC_TO_MONDAY: return d - c.wd;
        case DBG_FUNC_TO_START_OF_WEEK: return d - (c.wd + 1u) % 7u;
        case DBG_FUNC_TO_START_OF_MONTH: return d - (c.day - 1u);
        case DBG_FUNC_TO_START_OF_QUARTER: {
            // days of the year before the quarter's first month: 0, 90, 181, 273 (+1 from April on in a leap year)
            const uint32_t q = (c.month - 1u) / 3u;
            const uint32_t leap = (c.year % 4u == 0u && (c.year % 100u != 0u || c.year % 400u == 0u)) ? 1u : 0u;
            const uint32_t before = q * 91u - (q > 0u ? 1u : 0u) + (q == 3u ? 1u : 0u) + (q > 0u ? leap : 0u);
            return d - (c.ordinal - 1u - before);
        }
        case DBG_FUNC_TO_START_OF_YEAR: return d - (c.ordinal - 1u);
        case DBG_FUNC_TO_START_OF_ISO_YEAR: return d - c.wd - 7u * (uint64_t)(c.iso_week - 1u);  // the Monday of ISO week 1
        default: return 0;
    }
}

// length(): bit k of the result = byte k of the little-endian word w starts a character, that is,
// it is no UTF-8 continuation byte ((b & 0xC0) != 0x80).  chars().count() of a valid string is the
// number of such bytes; for invalid bytes the same count stands and nothing is raised.
EXPR_HD uint32_t expr_char_starts(uint32_t w) {
    const uint32_t cont = w & 0x80808080u & ~((w & 0x40404040u) << 1);  // bit 7 of every byte 10xxxxxx
    const uint32_t start = (~cont >> 7) & 0x01010101u;
    return (start * 0x01020408u) >> 24 & 0xfu;  // bits 0, 8, 16, 24 gathered into 24..27
}

// ---- host: check, type and lower a program --------------------------------------------------
struct ExprCompiled {
    std::vector<ENode> nodes;
    dbg_datatype out_types[DBG_EXPR_MAX_OUTPUTS];
    int n_outs = 0;
    bool wide = false;  // some value is a Decimal128: the 128-bit instantiation runs it
    int depth = 0;      // most live values on the stack at once
    bool has_func = false;  // some node is an EX_FUNC: the instantiation with the functions runs it
    uint32_t len_cols = 0;  // bit c: String column c is read through length(), so its slot holds the pre-pass's UInt64 column
};

// What a function takes and gives.
struct ExprFuncInfo {
    const char* name;
    bool on_date, on_ts;
    int res;  // dbg_type
};
inline const ExprFuncInfo* expr_func_info(int f) {
    static const ExprFuncInfo T[] = {
        {nullptr, false, false, 0},
        {"to_yyyymm", true, true, DBG_UINT32},
        {"to_yyyymmdd", true, true, DBG_UINT32},
        {"to_yyyymmddhh", true, true, DBG_UINT64},
        {"to_yyyymmddhhmmss", true, true, DBG_UINT64},
        {"to_year", true, true, DBG_UINT16},
        {"to_quarter", true, true, DBG_UINT8},
        {"to_month", true, true, DBG_UINT8},
        {"to_day_of_month", true, true, DBG_UINT8},
        {"to_day_of_week", true, true, DBG_UINT8},
        {"to_day_of_year", true, true, DBG_UINT16},
        {"to_week_of_year", true, true, DBG_UINT32},
        {"to_unix_timestamp", false, true, DBG_INT64},
        {"to_hour", false, true, DBG_UINT8},
        {"to_minute", false, true, DBG_UINT8},
        {"to_second", false, true, DBG_UINT8},
        {"to_start_of_second", false, true, DBG_TIMESTAMP},
        {"to_start_of_minute", false, true, DBG_TIMESTAMP},
        {"to_start_of_five_minutes", false, true, DBG_TIMESTAMP},
        {"to_start_of_ten_minutes", false, true, DBG_TIMESTAMP},
        {"to_start_of_fifteen_minutes", false, true, DBG_TIMESTAMP},
        {"time_slot", false, true, DBG_TIMESTAMP},
        {"to_start_of_hour", false, true, DBG_TIMESTAMP},
        {"to_start_of_day", false, true, DBG_TIMESTAMP},
        {"to_monday", true, true, DBG_DATE},
        {"to_start_of_week", true, true, DBG_DATE},
        {"to_start_of_month", true, true, DBG_DATE},
        {"to_start_of_quarter", true, true, DBG_DATE},
        {"to_start_of_year", true, true, DBG_DATE},
        {"to_start_of_iso_year", true, true, DBG_DATE},
        {"length", false, false, DBG_UINT64},
    };
    return f >= DBG_FUNC_TO_YYYYMM && f <= DBG_FUNC_LENGTH ? &T[f] : nullptr;
}
inline const char* expr_type_name(int t) {
    return t == DBG_DATE ? "Date" : (t == DBG_TIMESTAMP ? "Timestamp" : (t == DBG_STRING ? "String" : "a number"));
}
// Date, Timestamp and String values go into functions only
inline bool expr_is_func_only(int t) { return t == DBG_DATE || t == DBG_TIMESTAMP || t == DBG_STRING; }

inline bool expr_is_int(int t) { return t >= DBG_INT8 && t <= DBG_UINT64; }
inline bool expr_is_float(int t) { return t == DBG_FLOAT32 || t == DBG_FLOAT64; }
inline bool expr_is_signed(int t) { return t >= DBG_INT8 && t <= DBG_INT64; }
inline int expr_int_bits(int t) { return 8 << (t & 3); }
inline int expr_cls(int t) { return t == DBG_DECIMAL128 ? EC_DEC : (expr_is_float(t) ? EC_F64 : (expr_is_signed(t) ? EC_SINT : EC_UINT)); }
inline const char* expr_op_name(int arith) { return arith == EX_PLUS ? "plus" : (arith == EX_MINUS ? "minus" : "multiply"); }
inline expr_u128 expr_pow10(int k) {
    expr_u128 p = 1;
    for (int i = 0; i < k; ++i) p *= 10;
    return p;
}
// get_decimal_properties of a non-decimal operand
inline void expr_dec_props(const dbg_datatype& t, int* p, int* s) {
    if (t.type == DBG_DECIMAL128) {
        *p = t.precision, *s = t.scale;
        return;
    }
    static const int digits[8] = {3, 5, 10, 19, 3, 5, 10, 20};
    *p = digits[t.type], *s = 0;
}

// Why an operand type cannot be projected (nullptr: it can).  Date, Timestamp and String values
// are column leaves only.
inline const char* expr_refuse_type(const dbg_datatype& t, bool constant) {
    switch (t.type) {
        case DBG_DECIMAL256: return "Decimal256 operands are not supported";
        case DBG_BOOLEAN: return "Boolean operands are not supported";
        case DBG_STRING: return constant ? "String constants are not supported" : nullptr;
        case DBG_DATE: return constant ? "Date constants are not supported" : nullptr;
        case DBG_TIMESTAMP: return constant ? "Timestamp constants are not supported" : nullptr;
        default: return nullptr;
    }
}

// The type of `a op b` by the rules at the top; lowers the operator into n.  Returns a dbg status.
inline int expr_type_binary(int arith, const dbg_datatype& a, const dbg_datatype& b, dbg_datatype* out, ENode* n, std::string& msg) {
    memset(out, 0, sizeof(*out));
    out->nullable = (a.nullable || b.nullable) ? 1 : 0;
    n->arith = (uint8_t)arith;
    const bool da = a.type == DBG_DECIMAL128, db = b.type == DBG_DECIMAL128;
    if (!da && !db) {
        n->op = EX_NUM;
        if (expr_is_float(a.type) || expr_is_float(b.type)) {
            out->type = DBG_FLOAT64;
            n->to_f64 = 1;
            n->cls_r = EC_F64;
            n->cls_a = (uint8_t)expr_cls(a.type);
            n->cls_b = (uint8_t)expr_cls(b.type);
            return DBG_OK;
        }
        const int wa = expr_int_bits(a.type), wb = expr_int_bits(b.type);
        int w = 2 * (wa > wb ? wa : wb);
        if (w > 64) w = 64;
        const bool sgn = arith == EX_MINUS || expr_is_signed(a.type) || expr_is_signed(b.type);
        const int lg = w == 16 ? 1 : (w == 32 ? 2 : 3);
        out->type = (sgn ? DBG_INT8 : DBG_UINT8) + lg;
        n->cls_r = sgn ? EC_SINT : EC_UINT;
        return DBG_OK;
    }
    if (expr_is_float(a.type) || expr_is_float(b.type)) {
        msg = std::string(expr_op_name(arith)) + ": Decimal mixed with Float is not supported (the reference goes through to_float64)";
        return DBG_ERR_UNSUPPORTED;
    }
    int pa, sa, pb, sb;
    expr_dec_props(a, &pa, &sa);
    expr_dec_props(b, &pb, &sb);
    const int la = pa - sa, lb = pb - sb;
    out->type = DBG_DECIMAL128;
    if (arith == EX_MUL) {
        int mx = sa > sb ? sa : sb;
        if (mx < 12) mx = 12;
        const int s = sa + sb < mx ? sa + sb : mx;
        int p = la + lb + s;
        if (p > 38) p = 38;
        out->precision = (uint8_t)p, out->scale = (uint8_t)s;
        n->op = EX_DMUL;
        const int k = sa + sb - s;
        n->k = (uint8_t)k;
        const expr_u128 half = expr_pow10(k) / 2;
        n->fa[0] = (uint64_t)half, n->fa[1] = (uint64_t)(half >> 64);
        n->la[0] = (uint64_t)expr_pow10(k > 19 ? 19 : k);
        n->la[1] = (uint64_t)expr_pow10(k > 19 ? k - 19 : 0);
        return DBG_OK;
    }
    const int s = sa > sb ? sa : sb;
    int p = (la > lb ? la : lb) + s + 1;
    if (p > 38) p = 38;
    out->precision = (uint8_t)p, out->scale = (uint8_t)s;
    n->op = EX_DADD;
    const expr_u128 maxp = expr_pow10(p) - 1;
    // a cast that raises the scale is range-checked; one at the same scale cannot fail (an integer
    // of d digits at scale 0 lies within any precision >= d) and copies
    if (s > sa) {
        const expr_u128 f = expr_pow10(s - sa), lim = maxp / f;
        n->flags |= EX_F_SCALE_A;
        n->fa[0] = (uint64_t)f, n->fa[1] = (uint64_t)(f >> 64);
        n->la[0] = (uint64_t)lim, n->la[1] = (uint64_t)(lim >> 64);
    }
    if (s > sb) {
        const expr_u128 f = expr_pow10(s - sb), lim = maxp / f;
        n->flags |= EX_F_SCALE_B;
        n->fb[0] = (uint64_t)f, n->fb[1] = (uint64_t)(f >> 64);
        n->lb[0] = (uint64_t)lim, n->lb[1] = (uint64_t)(lim >> 64);
    }
    if (p == 38) n->flags |= EX_F_CHECK38;
    return DBG_OK;
}

// Check and type a whole program: 0 (DBG_OK) or the status, with `msg` for dbg_last_error.  Column
// data pointers are not read.
inline int expr_compile(const dbg_expr_program* P, ExprCompiled& C, std::string& msg) {
    if (!P || (P->n_nodes > 0 && !P->nodes) || (P->n_cols > 0 && !P->cols)) {
        msg = "expression program: null argument";
        return DBG_ERR_INVALID;
    }
    if (P->n_nodes < 0 || P->n_cols < 0 || P->n_outputs < 0) {
        msg = "expression program: negative count";
        return DBG_ERR_INVALID;
    }
    if (P->n_nodes > DBG_EXPR_MAX_NODES) {
        msg = "expression program: at most " + std::to_string(DBG_EXPR_MAX_NODES) + " nodes";
        return DBG_ERR_UNSUPPORTED;
    }
    if (P->n_outputs > DBG_EXPR_MAX_OUTPUTS) {
        msg = "expression program: at most " + std::to_string(DBG_EXPR_MAX_OUTPUTS) + " outputs";
        return DBG_ERR_UNSUPPORTED;
    }
    if (P->n_cols > DBG_EXPR_MAX_COLUMNS) {
        msg = "expression program: at most " + std::to_string(DBG_EXPR_MAX_COLUMNS) + " columns";
        return DBG_ERR_UNSUPPORTED;
    }
    if (P->n_outputs == 0) {
        msg = "expression program: no outputs";
        return DBG_ERR_INVALID;
    }
    if (P->reserved != 0) {
        msg = "expression program: reserved must be 0 (the session timezone is UTC; another zone keeps the CPU path)";
        return DBG_ERR_INVALID;
    }
    struct Val {
        dbg_datatype dt;
        int last_store;  // node of its last STORE, -1: never stored
        bool consumed;
        int col;  // the column a leaf reads, -1: not a column leaf
    };
    std::vector<Val> vals;   // every value the program makes
    std::vector<int> stack;  // indices into vals
    bool stored[DBG_EXPR_MAX_OUTPUTS] = {};
    C.nodes.assign((size_t)P->n_nodes, ENode{});
    C.n_outs = P->n_outputs;
    C.wide = false;
    C.depth = 0;
    C.has_func = false;
    C.len_cols = 0;
    for (int k = 0; k < P->n_nodes; ++k) {
        const dbg_expr_node& u = P->nodes[k];
        ENode& n = C.nodes[(size_t)k];
        switch (u.op) {
            case DBG_EXPR_COLUMN: {
                if (u.index < 0 || u.index >= P->n_cols) {
                    msg = "expression program: column index out of range";
                    return DBG_ERR_INVALID;
                }
                const dbg_datatype& t = P->cols[u.index].dt;
                if (t.type < DBG_INT8 || t.type > DBG_DECIMAL256) {
                    msg = "expression program: bad column type";
                    return DBG_ERR_INVALID;
                }
                if (const char* why = expr_refuse_type(t, false)) {
                    msg = std::string("expression program: ") + why;
                    return DBG_ERR_UNSUPPORTED;
                }
                if (t.type == DBG_DECIMAL128 && (t.precision < 1 || t.precision > 38 || t.scale > t.precision)) {
                    msg = "expression program: Decimal128 precision 1..38, scale <= precision";
                    return DBG_ERR_INVALID;
                }
                n.op = EX_COL;
                n.idx = u.index;
                dbg_datatype dt = t;
                dt.nullable = t.nullable ? 1 : 0;
                dt.reserved = 0;
                if (t.type != DBG_DECIMAL128) dt.precision = dt.scale = 0;
                vals.push_back({dt, -1, false, u.index});
                stack.push_back((int)vals.size() - 1);
                break;
            }
            case DBG_EXPR_CONST: {
                const dbg_datatype& t = u.dt;
                if (t.type < DBG_INT8 || t.type > DBG_DECIMAL256) {
                    msg = "expression program: bad constant type";
                    return DBG_ERR_INVALID;
                }
                if (const char* why = expr_refuse_type(t, true)) {
                    msg = std::string("expression program: ") + why;
                    return DBG_ERR_UNSUPPORTED;
                }
                if (t.nullable) {
                    msg = "expression program: NULL constants are not supported";
                    return DBG_ERR_UNSUPPORTED;
                }
                if (t.type == DBG_DECIMAL128 && (t.precision < 1 || t.precision > 38 || t.scale > t.precision)) {
                    msg = "expression program: Decimal128 precision 1..38, scale <= precision";
                    return DBG_ERR_INVALID;
                }
                n.op = EX_CONST;
                if (t.type == DBG_DECIMAL128) {
                    n.c[0] = u.i128_lo, n.c[1] = (uint64_t)u.i128_hi;
                } else if (expr_is_float(t.type)) {
                    // a Float32 constant is its value widened, as a Float32 cell is when it is loaded
                    const double d = t.type == DBG_FLOAT32 ? (double)(float)u.f64 : u.f64;
                    n.c[0] = expr_f64_bits(d);
                } else {
                    // the value as the type holds it, then extended
                    const int sh = 64 - expr_int_bits(t.type);
                    const uint64_t raw = (uint64_t)u.i64 << sh;
                    n.c[0] = expr_is_signed(t.type) ? (uint64_t)((int64_t)raw >> sh) : raw >> sh;
                    n.c[1] = expr_is_signed(t.type) && ((int64_t)n.c[0] < 0) ? ~0ULL : 0ULL;
                }
                dbg_datatype dt = t;
                dt.reserved = 0;
                if (t.type != DBG_DECIMAL128) dt.precision = dt.scale = 0;
                vals.push_back({dt, -1, false, -1});
                stack.push_back((int)vals.size() - 1);
                break;
            }
            case DBG_EXPR_PLUS: case DBG_EXPR_MINUS: case DBG_EXPR_MULTIPLY: {
                if (stack.size() < 2) {
                    msg = "expression program: stack underflow at an operator";
                    return DBG_ERR_INVALID;
                }
                const int ib = stack.back();
                stack.pop_back();
                const int ia = stack.back();
                stack.pop_back();
                vals[(size_t)ia].consumed = vals[(size_t)ib].consumed = true;
                const int arith = u.op == DBG_EXPR_PLUS ? EX_PLUS : (u.op == DBG_EXPR_MINUS ? EX_MINUS : EX_MUL);
                for (const int i : {ia, ib}) {
                    const int t = vals[(size_t)i].dt.type;
                    if (expr_is_func_only(t)) {
                        msg = std::string("expression program: ") + expr_op_name(arith) + ": " + expr_type_name(t) +
                              " operands are not supported (a " + expr_type_name(t) + " value goes into a function that takes it)";
                        return DBG_ERR_UNSUPPORTED;
                    }
                }
                dbg_datatype dt;
                const int rc = expr_type_binary(arith, vals[(size_t)ia].dt, vals[(size_t)ib].dt, &dt, &n, msg);
                if (rc != DBG_OK) return rc;
                vals.push_back({dt, -1, false, -1});
                stack.push_back((int)vals.size() - 1);
                break;
            }
            case DBG_EXPR_FUNC: {
                const ExprFuncInfo* fi = expr_func_info(u.index);
                if (!fi) {
                    msg = "expression program: unknown op: function id " + std::to_string(u.index) + " is not defined";
                    return DBG_ERR_INVALID;
                }
                if (stack.empty()) {
                    msg = std::string("expression program: stack underflow at ") + fi->name;
                    return DBG_ERR_INVALID;
                }
                const int ia = stack.back();
                stack.pop_back();
                vals[(size_t)ia].consumed = true;
                const dbg_datatype at = vals[(size_t)ia].dt;
                const bool takes = u.index == DBG_FUNC_LENGTH ? at.type == DBG_STRING
                                                              : ((at.type == DBG_DATE && fi->on_date) || (at.type == DBG_TIMESTAMP && fi->on_ts));
                if (!takes) {
                    msg = std::string("expression program: ") + fi->name + " does not take " + expr_type_name(at.type);
                    return DBG_ERR_INVALID;
                }
                dbg_datatype dt;
                memset(&dt, 0, sizeof(dt));
                dt.type = fi->res;
                dt.nullable = at.nullable;  // register_passthrough_nullable_1_arg
                if (u.index == DBG_FUNC_LENGTH) {
                    // a String value is a column leaf: that leaf reads the pre-pass's column instead
                    n.op = EX_NOP;
                    C.len_cols |= 1u << vals[(size_t)ia].col;
                } else {
                    n.op = EX_FUNC;
                    n.arith = (uint8_t)u.index;
                    n.cls_a = at.type == DBG_TIMESTAMP ? 1 : 0;
                    n.cls_r = (fi->res == DBG_DATE || fi->res == DBG_TIMESTAMP || fi->res == DBG_INT64) ? EC_SINT : EC_UINT;
                    C.has_func = true;
                }
                vals.push_back({dt, -1, false, -1});
                stack.push_back((int)vals.size() - 1);
                break;
            }
            case DBG_EXPR_STORE: {
                if (stack.empty()) {
                    msg = "expression program: stack underflow at a STORE";
                    return DBG_ERR_INVALID;
                }
                if (vals[(size_t)stack.back()].dt.type == DBG_STRING) {
                    msg = "expression program: String results are not supported";
                    return DBG_ERR_UNSUPPORTED;
                }
                if (u.index < 0 || u.index >= P->n_outputs) {
                    msg = "expression program: output index out of range";
                    return DBG_ERR_INVALID;
                }
                if (stored[u.index]) {
                    msg = "expression program: output " + std::to_string(u.index) + " is stored twice";
                    return DBG_ERR_INVALID;
                }
                stored[u.index] = true;
                n.op = EX_STORE;
                n.idx = u.index;
                vals[(size_t)stack.back()].last_store = k;
                C.out_types[u.index] = vals[(size_t)stack.back()].dt;
                break;
            }
            default: msg = "expression program: unknown op"; return DBG_ERR_INVALID;
        }
    }
    for (int o = 0; o < P->n_outputs; ++o)
        if (!stored[o]) {
            msg = "expression program: output " + std::to_string(o) + " is never stored";
            return DBG_ERR_INVALID;
        }
    for (const Val& v : vals) {
        if (v.dt.type == DBG_DECIMAL128) C.wide = true;
        if (!v.consumed && v.last_store < 0) {
            msg = "expression program: a value is left over (neither stored nor used)";
            return DBG_ERR_INVALID;
        }
        // a stored value that no operator takes leaves the stack with its last STORE: nothing
        // under it could be reached any more, so every operator sees the operands it saw before
        if (!v.consumed) C.nodes[(size_t)v.last_store].flags |= EX_F_POP;
    }
    // a length() left nothing to run
    size_t kept = 0;
    for (const ENode& n : C.nodes)
        if (n.op != EX_NOP) C.nodes[kept++] = n;
    C.nodes.resize(kept);
    // depth of the live values
    int depth = 0;
    for (const ENode& n : C.nodes) {
        if (n.op == EX_COL || n.op == EX_CONST) depth++;
        else if (n.op == EX_STORE) depth -= (n.flags & EX_F_POP) ? 1 : 0;
        else if (n.op != EX_FUNC) depth--;
        if (depth > C.depth) C.depth = depth;
        if (depth > DBG_EXPR_STACK) {
            msg = "expression program: more than " + std::to_string(DBG_EXPR_STACK) + " live values on the stack";
            return DBG_ERR_UNSUPPORTED;
        }
    }
    return DBG_OK;
}
