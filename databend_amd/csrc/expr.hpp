// expr.hpp — scalar projection in front of the aggregate: plus / minus / multiply over numbers and
// Decimal128 (BlockOperator::Map -> Evaluator::run, SQL/evaluator/block_operator.rs:50-80).
//
// Two halves, both plain C++ so that a host build (tests/csrc/expr_host_main.cpp, under ASan and
// UBSan) runs the very source the kernel compiles, as like.hpp and zstd_dev.hpp do:
//  * expr_compile: the one place a program is checked and typed.  It walks the caller's postfix
//    dbg_expr_program, decides every node's type by the reference's rules and lowers it to ENodes
//    whose operand classes, power-of-ten factors and range limits are resolved.
//  * expr_num / expr_dec_add / expr_dec_mul: one operator on one row, called by expr_kernel
//    (expr.hip) and by the host build.  All wrapping arithmetic is done in unsigned types.
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
enum { EX_COL = 0, EX_CONST = 1, EX_NUM = 2, EX_DADD = 3, EX_DMUL = 4, EX_STORE = 5 };
enum { EX_PLUS = 0, EX_MINUS = 1, EX_MUL = 2 };
enum { EC_SINT = 0, EC_UINT = 1, EC_F64 = 2, EC_DEC = 3 };  // how a value sits in its 64 / 128 bits

// Values are canonical: integers sign- or zero-extended to 64 bits (to 128 where a program holds a
// Decimal128), floats as the bits of a double, decimals as i128.  Every operator leaves its result
// canonical (a number operator in a 128-bit program through expr_num_hi).
struct ENode {
    uint8_t op;       // EX_*
    uint8_t arith;    // EX_PLUS / EX_MINUS / EX_MUL
    uint8_t cls_a;    // EX_NUM into Float64: EC_* of each operand
    uint8_t cls_b;
    uint8_t to_f64;   // EX_NUM: the operation runs in Float64
    uint8_t flags;    // EX_DADD: EX_F_*;  EX_STORE: EX_F_POP
    uint8_t k;        // EX_DMUL: the divisor is 10^k
    uint8_t cls_r;    // EX_NUM: EC_* of the result (its extension to 128 bits in a wide program)
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

// ---- host: check, type and lower a program --------------------------------------------------
struct ExprCompiled {
    std::vector<ENode> nodes;
    dbg_datatype out_types[DBG_EXPR_MAX_OUTPUTS];
    int n_outs = 0;
    bool wide = false;  // some value is a Decimal128: the 128-bit instantiation runs it
    int depth = 0;      // most live values on the stack at once
};

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

// Why an operand type cannot be projected (nullptr: it can).
inline const char* expr_refuse_type(const dbg_datatype& t) {
    switch (t.type) {
        case DBG_DECIMAL256: return "Decimal256 operands are not supported";
        case DBG_STRING: return "String operands are not supported";
        case DBG_BOOLEAN: return "Boolean operands are not supported";
        case DBG_DATE: return "Date operands are not supported (date functions stay on the CPU path)";
        case DBG_TIMESTAMP: return "Timestamp operands are not supported (date functions stay on the CPU path)";
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
    struct Val {
        dbg_datatype dt;
        int last_store;  // node of its last STORE, -1: never stored
        bool consumed;
    };
    std::vector<Val> vals;   // every value the program makes
    std::vector<int> stack;  // indices into vals
    bool stored[DBG_EXPR_MAX_OUTPUTS] = {};
    C.nodes.assign((size_t)P->n_nodes, ENode{});
    C.n_outs = P->n_outputs;
    C.wide = false;
    C.depth = 0;
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
                if (const char* why = expr_refuse_type(t)) {
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
                vals.push_back({dt, -1, false});
                stack.push_back((int)vals.size() - 1);
                break;
            }
            case DBG_EXPR_CONST: {
                const dbg_datatype& t = u.dt;
                if (t.type < DBG_INT8 || t.type > DBG_DECIMAL256) {
                    msg = "expression program: bad constant type";
                    return DBG_ERR_INVALID;
                }
                if (const char* why = expr_refuse_type(t)) {
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
                vals.push_back({dt, -1, false});
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
                dbg_datatype dt;
                const int rc = expr_type_binary(arith, vals[(size_t)ia].dt, vals[(size_t)ib].dt, &dt, &n, msg);
                if (rc != DBG_OK) return rc;
                vals.push_back({dt, -1, false});
                stack.push_back((int)vals.size() - 1);
                break;
            }
            case DBG_EXPR_STORE: {
                if (stack.empty()) {
                    msg = "expression program: stack underflow at a STORE";
                    return DBG_ERR_INVALID;
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
    // depth of the live values
    int depth = 0;
    for (const ENode& n : C.nodes) {
        if (n.op == EX_COL || n.op == EX_CONST) depth++;
        else if (n.op == EX_STORE) depth -= (n.flags & EX_F_POP) ? 1 : 0;
        else depth--;
        if (depth > C.depth) C.depth = depth;
        if (depth > DBG_EXPR_STACK) {
            msg = "expression program: more than " + std::to_string(DBG_EXPR_STACK) + " live values on the stack";
            return DBG_ERR_UNSUPPORTED;
        }
    }
    return DBG_OK;
}
