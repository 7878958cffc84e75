// expr.hip — the device projection (dbg_expr_result_type / dbg_expr_eval): plus, minus and multiply
// over numbers and Decimal128, the date / time functions and length() in front of the aggregate
// (BlockOperator::Map, expr.hpp has the rules).
//
// A streaming element-wise kernel, memory-bound by intent.  The host lowers the program to ENodes
// (expr_compile); the kernel walks them per strip with wave-uniform dispatch and keeps the operand
// stack in register slots that shift on push and pop (static indices only: no scratch).
// One template, instantiated narrow and wide, each for a stack of two and of four slots (a program
// that never holds more than two live values needs half the slot registers: DESIGN.md §4.13):
//   narrow  every value fits 64 bits.  A lane owns 8 contiguous rows of a 256 x 8 strip, so a
//           column strip is one wide load per lane and the lane's output validity is one whole
//           byte, written with a plain store.
//   wide    some value is a Decimal128.  A lane takes one row per trip, loads and stores are 16
//           bytes per lane, the validity bytes of a wave's 64 rows come from a ballot.
// The last partial strip is read row by row behind a bound check.  An error (a decimal overflow on
// a valid, selected row) is raised with one plain store per workgroup.
// A third template flag, FUNC, compiles the date / time functions into the node loop (one more
// wave-uniform case, element-wise on the canonical value); a program without one runs the
// instantiation without them, whose code is what it was before the functions existed.
// length() is a pre-pass of its own (expr_length_kernel below): it writes a UInt64 column into a
// temporary of the call, which the node loop then reads as an ordinary column leaf.
#include "abi_internal.hpp"
#include "expr.hpp"

#define EXPR_BLOCK 256
#define EXPR_MAX_BLOCKS 2048

struct EOut {
    u8* data;
    u8* validity;  // nullptr: the result is not nullable
    u32 width;
    u32 is_f32;
};

struct EProg {
    u64 rows;
    int32_t n_nodes, n_cols;
    DCol cols[DBG_EXPR_MAX_COLUMNS];
    EOut outs[DBG_EXPR_MAX_OUTPUTS];
    ENode nodes[DBG_EXPR_MAX_NODES];
};

typedef u32 expr_u32x4 __attribute__((ext_vector_type(4)));
typedef u64 expr_u64x2 __attribute__((ext_vector_type(2)));

template <typename V>
__device__ __forceinline__ void gst(void* p, V v) {
    *(V __attribute__((address_space(1)))*)p = v;
}

// A value of the operand stack for the R rows of one lane: canonical bits and a validity bit per row.
template <bool WIDE, int R>
struct ESlot {
    u64 lo[R];
    u64 hi[R];  // wide programs only (never touched, so never allocated, in the narrow kernel)
    u32 valid;  // bit j: row j is not NULL
};

// Cells of the lane's R rows from r0 on, canonical; rows j >= n are not read.
template <bool WIDE, int R, bool FULL>
__device__ __forceinline__ void expr_load(const DCol& c, u64 r0, int n, ESlot<WIDE, R>& v) {
    const u8* p = c.data + r0 * (u64)c.width;
    if constexpr (WIDE) {
        v.lo[0] = 0;
        v.hi[0] = 0;
        if (n > 0) {
            switch (c.width) {
                case 1: v.lo[0] = gld<u8>(p); break;
                case 2: v.lo[0] = gld<u16>(p); break;
                case 4: v.lo[0] = gld<u32>(p); break;
                case 8: v.lo[0] = gld<u64>(p); break;
                default:
                    if (((uintptr_t)p & 15) == 0) {
                        const expr_u64x2 w = gld<expr_u64x2>(p);
                        v.lo[0] = w.x, v.hi[0] = w.y;
                    } else {
                        v.lo[0] = gld<u64>(p), v.hi[0] = gld<u64>(p + 8);
                    }
            }
        }
    } else if constexpr (FULL) {
        const bool al16 = ((uintptr_t)p & 15) == 0;
        switch (c.width) {
            case 1:
                if (((uintptr_t)p & 7) == 0) {
                    const u64 w = gld<u64>(p);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v.lo[j] = (w >> (8 * j)) & 0xff;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v.lo[j] = gld<u8>(p + j);
                }
                break;
            case 2:
                if (al16) {
                    const expr_u32x4 w = gld<expr_u32x4>(p);
                    v.lo[0] = w.x & 0xffff, v.lo[1] = w.x >> 16, v.lo[2] = w.y & 0xffff, v.lo[3] = w.y >> 16;
                    v.lo[4] = w.z & 0xffff, v.lo[5] = w.z >> 16, v.lo[6] = w.w & 0xffff, v.lo[7] = w.w >> 16;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v.lo[j] = gld<u16>(p + 2 * j);
                }
                break;
            case 4:
                if (al16) {
                    const expr_u32x4 w0 = gld<expr_u32x4>(p), w1 = gld<expr_u32x4>(p + 16);
                    v.lo[0] = w0.x, v.lo[1] = w0.y, v.lo[2] = w0.z, v.lo[3] = w0.w;
                    v.lo[4] = w1.x, v.lo[5] = w1.y, v.lo[6] = w1.z, v.lo[7] = w1.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v.lo[j] = gld<u32>(p + 4 * j);
                }
                break;
            default:
                if (al16) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const expr_u64x2 w = gld<expr_u64x2>(p + 16 * j);
                        v.lo[2 * j] = w.x, v.lo[2 * j + 1] = w.y;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v.lo[j] = gld<u64>(p + 8 * j);
                }
        }
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            u64 x = 0;
            if (j < n) {
                const u8* q = p + (u64)j * c.width;
                x = c.width == 1 ? (u64)gld<u8>(q) : c.width == 2 ? (u64)gld<u16>(q) : c.width == 4 ? (u64)gld<u32>(q) : gld<u64>(q);
            }
            v.lo[j] = x;
        }
    }
    // canonical form: widen Float32, sign-extend what is signed
    if (c.type == DBG_FLOAT32) {
#pragma unroll
        for (int j = 0; j < R; ++j) v.lo[j] = (u64)__double_as_longlong((double)__uint_as_float((u32)v.lo[j]));
    } else if (c.type <= DBG_INT64) {  // DBG_INT8 .. DBG_INT64
        const int sh = 64 - 8 * (int)c.width;
#pragma unroll
        for (int j = 0; j < R; ++j) v.lo[j] = (u64)((i64)(v.lo[j] << sh) >> sh);
        if constexpr (WIDE) v.hi[0] = (u64)((i64)v.lo[0] >> 63);
    }
    // validity of the R rows
    if (!c.nullable || c.validity == nullptr) {
        v.valid = (1u << R) - 1;
    } else if constexpr (!WIDE && FULL) {
        const u64 b0 = c.validity_offset + r0;
        const u32 sh = (u32)(b0 & 7);
        u32 w = gld<u8>(c.validity + (b0 >> 3));
        if (sh) w |= (u32)gld<u8>(c.validity + (b0 >> 3) + 1) << 8;  // row r0 + 7 exists and its bit is in that byte
        v.valid = (w >> sh) & 0xff;
    } else {
        u32 m = 0;
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (j < n) {
                const u64 b = c.validity_offset + r0 + j;
                m |= ((gld<u8>(c.validity + (b >> 3)) >> (b & 7)) & 1u) << j;
            }
        v.valid = m;
    }
}

__device__ __forceinline__ void expr_store_cell(u8* q, u32 width, u64 x) {
    if (width == 1) gst<u8>(q, (u8)x);
    else if (width == 2) gst<u16>(q, (u16)x);
    else if (width == 4) gst<u32>(q, (u32)x);
    else gst<u64>(q, x);
}

// Output cells of the lane's R rows from r0 on (rows j >= n are not written), and their validity.
template <bool WIDE, int R, bool FULL>
__device__ __forceinline__ void expr_store(const EOut& o, u64 rows, u64 r0, int n, const ESlot<WIDE, R>& v) {
    u8* p = o.data + r0 * (u64)o.width;
    u64 x[R];
#pragma unroll
    for (int j = 0; j < R; ++j)
        x[j] = o.is_f32 ? (u64)__float_as_uint((float)__longlong_as_double((long long)v.lo[j])) : v.lo[j];
    if constexpr (WIDE) {
        if (n > 0) {
            if (o.width != 16) {
                expr_store_cell(p, o.width, x[0]);
            } else if (((uintptr_t)p & 15) == 0) {
                expr_u64x2 w;
                w.x = x[0], w.y = v.hi[0];
                gst<expr_u64x2>(p, w);
            } else {
                gst<u64>(p, x[0]);
                gst<u64>(p + 8, v.hi[0]);
            }
        }
        if (o.validity) {
            // every lane of the wave is here (the caller keeps whole waves in the loop); the wave's
            // 64 rows start at a multiple of 64, so they are eight whole bytes: lanes 0..7 write
            // one each, as far as the column's ceil(rows / 8) bytes go
            const u64 bal = __ballot(n > 0 && (v.valid & 1u));
            const u32 lane = threadIdx.x & 63;
            const u64 byte_row = r0 - lane + 8 * (u64)lane;  // first row of this lane's byte
            if (lane < 8 && byte_row < rows) gst<u8>(o.validity + (byte_row >> 3), (u8)(bal >> (8 * lane)));
        }
    } else if constexpr (FULL) {
        const bool al16 = ((uintptr_t)p & 15) == 0;
        if (o.width == 8 && al16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                expr_u64x2 w;
                w.x = x[2 * j], w.y = x[2 * j + 1];
                gst<expr_u64x2>(p + 16 * j, w);
            }
        } else if (o.width == 4 && al16) {
            expr_u32x4 w0, w1;
            w0.x = (u32)x[0], w0.y = (u32)x[1], w0.z = (u32)x[2], w0.w = (u32)x[3];
            w1.x = (u32)x[4], w1.y = (u32)x[5], w1.z = (u32)x[6], w1.w = (u32)x[7];
            gst<expr_u32x4>(p, w0);
            gst<expr_u32x4>(p + 16, w1);
        } else if (o.width == 2 && al16) {
            expr_u32x4 w;
            w.x = (u32)(x[0] & 0xffff) | ((u32)x[1] << 16), w.y = (u32)(x[2] & 0xffff) | ((u32)x[3] << 16);
            w.z = (u32)(x[4] & 0xffff) | ((u32)x[5] << 16), w.w = (u32)(x[6] & 0xffff) | ((u32)x[7] << 16);
            gst<expr_u32x4>(p, w);
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) expr_store_cell(p + (u64)j * o.width, o.width, x[j]);
        }
        if (o.validity) gst<u8>(o.validity + (r0 >> 3), (u8)v.valid);
    } else {
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (j < n) expr_store_cell(p + (u64)j * o.width, o.width, x[j]);
        if (o.validity && n > 0) gst<u8>(o.validity + (r0 >> 3), (u8)(v.valid & ((1u << n) - 1)));
    }
}

template <bool WIDE, int R>
__device__ __forceinline__ void expr_copy(ESlot<WIDE, R>& d, const ESlot<WIDE, R>& s) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
        d.lo[j] = s.lo[j];
        if constexpr (WIDE) d.hi[j] = s.hi[j];
    }
    d.valid = s.valid;
}

// The program over the lane's rows [r0, r0 + n).  `sel`: bit j = row j passed the filter.  Returns
// 0, or 1 + the arithmetic op (EX_*) of an operator that failed on a valid, selected row.
template <bool WIDE, int R, bool FULL, int DEPTH, bool FUNC>
__device__ __forceinline__ u32 expr_run(const EProg* __restrict__ P, u64 r0, int n, u32 sel) {
    ESlot<WIDE, R> s0, s1, s2, s3;  // s0 is the top of the stack
#pragma unroll
    for (int j = 0; j < R; ++j) {
        s0.lo[j] = s1.lo[j] = s2.lo[j] = s3.lo[j] = 0;
        s0.hi[j] = s1.hi[j] = s2.hi[j] = s3.hi[j] = 0;
    }
    s0.valid = s1.valid = s2.valid = s3.valid = 0;
    u32 err = 0;
    const u64 rows = P->rows;
    const int nn = P->n_nodes;
    for (int k = 0; k < nn; ++k) {
        const ENode& nd = P->nodes[k];
        const int op = nd.op;
        if (op == EX_COL || op == EX_CONST) {
            if constexpr (DEPTH > 2) {
                expr_copy(s3, s2);
                expr_copy(s2, s1);
            }
            expr_copy(s1, s0);
            if (op == EX_COL) {
                expr_load<WIDE, R, FULL>(P->cols[nd.idx], r0, n, s0);
            } else {
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    s0.lo[j] = nd.c[0];
                    if constexpr (WIDE) s0.hi[j] = nd.c[1];
                }
                s0.valid = (1u << R) - 1;
            }
        } else if (op == EX_STORE) {
            expr_store<WIDE, R, FULL>(P->outs[nd.idx], rows, r0, n, s0);
            if (nd.flags & EX_F_POP) {
                expr_copy(s0, s1);
                if constexpr (DEPTH > 2) {
                    expr_copy(s1, s2);
                    expr_copy(s2, s3);
                }
            }
        } else if (FUNC && op == EX_FUNC) {
            // one value in, one out: validity and the slots below stay as they are
#pragma unroll
            for (int j = 0; j < R; ++j) s0.lo[j] = expr_func(nd, s0.lo[j]);
            if constexpr (WIDE) s0.hi[0] = expr_num_hi(nd, s0.lo[0]);
        } else {
            const u32 valid = s1.valid & s0.valid;
            if (op == EX_NUM) {
#pragma unroll
                for (int j = 0; j < R; ++j) s0.lo[j] = expr_num(nd, s1.lo[j], s0.lo[j]);
                if constexpr (WIDE) s0.hi[0] = expr_num_hi(nd, s0.lo[0]);  // canonical again for a decimal operator
            } else if constexpr (WIDE) {
                const EU128 a{s1.lo[0], s1.hi[0]}, b{s0.lo[0], s0.hi[0]};
                bool bad = false;
                const EU128 r = op == EX_DADD ? expr_dec_add(nd, a, b, &bad) : expr_dec_mul(nd, a, b, &bad);
                s0.lo[0] = r.lo, s0.hi[0] = r.hi;
                if (bad && (valid & sel & 1u)) err = 1u + nd.arith;
            }
            s0.valid = valid;
            if constexpr (DEPTH > 2) {
                expr_copy(s1, s2);
                expr_copy(s2, s3);
            }
        }
    }
    return err;
}

template <bool WIDE, int DEPTH, bool FUNC>
__global__ void __launch_bounds__(EXPR_BLOCK) expr_kernel(const EProg* __restrict__ P, const FilterDesc* __restrict__ F,
                                                           u32* __restrict__ err_out) {
    constexpr int R = WIDE ? 1 : 8;
    constexpr u64 STRIP = (u64)EXPR_BLOCK * R;
    __shared__ u32 s_err;
    if (threadIdx.x == 0) s_err = 0;
    __syncthreads();
    const u64 rows = P->rows;
    const u64 n_strips = (rows + STRIP - 1) / STRIP;
    u32 err = 0;
    for (u64 s = blockIdx.x; s < n_strips; s += gridDim.x) {
        const u64 r0 = s * STRIP + (u64)threadIdx.x * R;
        const int n = r0 >= rows ? 0 : (rows - r0 < (u64)R ? (int)(rows - r0) : R);
        u32 sel = (1u << R) - 1;
        if (F) {
            sel = 0;
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (j < n && eval_pred(F->nodes, F->n_nodes, F->cols, r0 + j)) sel |= 1u << j;
        }
        u32 e;
        if (WIDE || n < R) e = expr_run<WIDE, R, false, DEPTH, FUNC>(P, r0, n, sel);  // wide: whole waves stay together for the ballot
        else e = expr_run<WIDE, R, true, DEPTH, FUNC>(P, r0, n, sel);
        if (e) err = e;
    }
    if (err) s_err = err;  // any one of the workgroup's errors
    __syncthreads();
    if (threadIdx.x == 0 && s_err) *err_out = s_err;  // one plain store per workgroup
}

// ------------------------------------------------------------------------------------------
// length(String): the number of bytes that are not UTF-8 continuation bytes, one UInt64 per row
// ------------------------------------------------------------------------------------------
// A workgroup takes LEN_ROWS consecutive rows, whose bytes are one contiguous span of the blob, and
// streams the span in tiles of 256 aligned 16-byte chunks, one 16-byte load per lane.  Per chunk it
// keeps a 16-bit mask of the bytes that start a character (inside the span) and the exclusive prefix
// of their counts in LDS.  The count of start bytes from the span's first byte up to a row boundary
// x is then  (start bytes of the tiles before) + prefix[chunk of x] + popcount(mask[chunk of x]
// below x);  every boundary lies in exactly one tile, a lane resolves the boundaries it owns there,
// and a row's length is the difference of its two boundaries.  No lane ever walks a string: a long
// string only means more tiles for its workgroup, an empty one costs nothing.
// LDS: 256 masks + 256 prefixes (u32) + (LEN_ROWS + 1) boundary counts (u64) + 4 wave totals:
// 2 KiB + 8 KiB + 24 B.  Offsets are 64-bit and absolute, so a view may start at any row.
#define LEN_ROWS 1024
#define LEN_TILE (EXPR_BLOCK * 16)
#define LEN_BOUNDS ((LEN_ROWS + EXPR_BLOCK) / EXPR_BLOCK)  // boundaries a lane owns: 5 (the last one only lane 0's)

// bit k of the result: byte k of the four words starts a character
__device__ __forceinline__ u32 len_start_mask(expr_u32x4 w) {
    return expr_char_starts(w.x) | expr_char_starts(w.y) << 4 | expr_char_starts(w.z) << 8 | expr_char_starts(w.w) << 12;
}

__global__ void __launch_bounds__(EXPR_BLOCK) expr_length_kernel(const u8* __restrict__ data, const u64* __restrict__ offsets, u64 rows,
                                                                  u64* __restrict__ out) {
    __shared__ u32 s_mask[EXPR_BLOCK];
    __shared__ u32 s_pre[EXPR_BLOCK];
    __shared__ u32 s_wave[EXPR_BLOCK / 64];
    __shared__ u64 s_bound[LEN_ROWS + 1];
    const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64 r0 = (u64)blockIdx.x * LEN_ROWS;
    if (r0 >= rows) return;
    const u32 nr = (u32)(rows - r0 < (u64)LEN_ROWS ? rows - r0 : (u64)LEN_ROWS);  // rows of this workgroup: boundaries 0..nr
    // the boundaries this lane owns, as absolute addresses
    u64 x[LEN_BOUNDS];
#pragma unroll
    for (int k = 0; k < LEN_BOUNDS; ++k) {
        const u32 i = tid + (u32)k * EXPR_BLOCK;
        x[k] = i <= nr ? (u64)(uintptr_t)data + gld<u64>(offsets + r0 + i) : ~0ULL;
        if (i <= nr) s_bound[i] = 0;
    }
    const u64 a0 = (u64)(uintptr_t)data + gld<u64>(offsets + r0), a1 = (u64)(uintptr_t)data + gld<u64>(offsets + r0 + nr);
    u64 before = 0;  // start bytes of the tiles before this one
    for (u64 t0 = a0 & ~15ULL; t0 <= a1; t0 += LEN_TILE) {
        const u64 ca = t0 + 16ULL * tid;
        // the chunk's bytes [lo, hi) lie in the span; a chunk with none is not loaded
        const u32 lo = ca < a0 ? (u32)(a0 - ca) : 0u;
        const u32 hi = ca >= a1 ? 0u : (a1 - ca < 16 ? (u32)(a1 - ca) : 16u);
        u32 m = 0;
        if (hi > lo) m = len_start_mask(gld<expr_u32x4>((const void*)(uintptr_t)ca)) & ((1u << hi) - 1u) & ~((1u << lo) - 1u);
        const u32 cnt = (u32)__popc(m);
        u32 inc = cnt;  // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 y = (u32)__shfl_up((int)inc, d, 64);
            if (lane >= (u32)d) inc += y;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        u32 base = 0, total = 0;
#pragma unroll
        for (u32 w = 0; w < EXPR_BLOCK / 64; ++w) {
            const u32 t = s_wave[w];
            if (w < wave) base += t;
            total += t;
        }
        s_mask[tid] = m;
        s_pre[tid] = base + inc - cnt;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LEN_BOUNDS; ++k) {
            if (x[k] >= t0 && x[k] - t0 < LEN_TILE) {
                const u32 q = (u32)(x[k] - t0) >> 4, e = (u32)(x[k] - t0) & 15u;
                s_bound[tid + (u32)k * EXPR_BLOCK] = before + s_pre[q] + (u32)__popc(s_mask[q] & ((1u << e) - 1u));
            }
        }
        before += total;
        // the next trip writes s_wave only after every lane is past the second barrier, and s_mask /
        // s_pre only after its own first barrier, which every lane reaches after the loop above
    }
    __syncthreads();
    for (u32 i = tid; i < nr; i += EXPR_BLOCK) gst<u64>(out + r0 + i, s_bound[i + 1] - s_bound[i]);
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
// The device copies of one dbg_expr_eval call.
struct ExprLaunch {
    std::vector<DevBuf> consts;  // the filter's string constants and LIKE match bitmaps
    std::vector<FilterDesc> hf;  // host staging of the filter descriptor
    Buf<FilterDesc> dfd;
    Buf<EProg> dp;
    Buf<u32> derr;
    std::vector<Buf<u64>> lens;  // the columns length() pre-passes wrote
};

// Queue the filter's pre-passes, the uploads, the kernel and the read-back of the error word on s.
// The caller synchronises s whatever this returns.
static int expr_queue(const ExprCompiled& C, EProg& E, const dbg_filter* filter, u64 rows, hipStream_t s, ExprLaunch& L, u32* err) {
    // length(): every String column read through it becomes the UInt64 column of its lengths, the
    // String column's validity passing through
    for (int c = 0; c < E.n_cols; ++c) {
        if (!(C.len_cols >> c & 1u)) continue;
        L.lens.emplace_back();
        RETURN_IF(L.lens.back().ensure(rows));
        u64* out = L.lens.back().get();
        {
            prof::Scope ps("expr_length", s);
            const u64 grid = (rows + LEN_ROWS - 1) / LEN_ROWS;
            if (grid > 0x7fffffffULL) return fail(DBG_ERR_UNSUPPORTED, "expression program: too many rows for one length() pass");
            hipLaunchKernelGGL(expr_length_kernel, dim3((u32)grid), dim3(EXPR_BLOCK), 0, s, E.cols[c].data, E.cols[c].offsets, rows, out);
        }
        HIPCHECK(hipGetLastError());
        DCol& d = E.cols[c];
        d.type = DBG_UINT64;
        d.width = d.stride = 8;
        d.data = (const u8*)out;
        d.offsets = nullptr;
    }
    const bool filtered = filter && filter->n_nodes;
    if (filtered) {
        L.hf.resize(1);
        memset(&L.hf[0], 0, sizeof(FilterDesc));
        L.hf[0].rows = rows;
        for (int c = 0; c < filter->n_cols && c < DBG_MAX_FCOLS; ++c)
            if (filter->cols[c].len < rows) return fail(DBG_ERR_INVALID, "expression program: filter column shorter than rows");
        RETURN_IF(fill_filter({s, L.consts}, filter, 1, rows, L.hf[0].cols, &L.hf[0].n_cols, L.hf[0].nodes, &L.hf[0].n_nodes));
        RETURN_IF(L.dfd.ensure(1));
        HIPCHECK(hipMemcpyAsync(L.dfd, &L.hf[0], sizeof(FilterDesc), hipMemcpyHostToDevice, s));
    }
    RETURN_IF(L.dp.ensure(1));
    RETURN_IF(L.derr.ensure(4));
    HIPCHECK(hipMemcpyAsync(L.dp, &E, sizeof(E), hipMemcpyHostToDevice, s));
    HIPCHECK(hipMemsetAsync(L.derr, 0, 16, s));
    const u64 strip = (u64)EXPR_BLOCK * (C.wide ? 1 : 8);
    const u64 n_strips = (rows + strip - 1) / strip;
    const u32 grid = (u32)std::min<u64>(n_strips, EXPR_MAX_BLOCKS);
    {
        prof::Scope ps(C.wide ? "expr_eval_wide" : "expr_eval_narrow", s);
        const EProg* dp = L.dp.get();
        const FilterDesc* f = filtered ? L.dfd.get() : nullptr;
        u32* derr = L.derr.get();
        const bool shallow = C.depth <= 2;  // two stack slots instead of four: fewer registers, more waves per SIMD
#define EXPR_LAUNCH(W, D, F) hipLaunchKernelGGL((expr_kernel<W, D, F>), dim3(grid), dim3(EXPR_BLOCK), 0, s, dp, f, derr)
        if (C.has_func) {
            if (C.wide && shallow) EXPR_LAUNCH(true, 2, true);
            else if (C.wide) EXPR_LAUNCH(true, 4, true);
            else if (shallow) EXPR_LAUNCH(false, 2, true);
            else EXPR_LAUNCH(false, 4, true);
        } else {
            if (C.wide && shallow) EXPR_LAUNCH(true, 2, false);
            else if (C.wide) EXPR_LAUNCH(true, 4, false);
            else if (shallow) EXPR_LAUNCH(false, 2, false);
            else EXPR_LAUNCH(false, 4, false);
        }
#undef EXPR_LAUNCH
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(err, L.derr, 4, hipMemcpyDeviceToHost, s));
    return DBG_OK;
}

extern "C" {
int dbg_expr_result_type(const dbg_expr_program* program, int32_t k, dbg_datatype* out) {
    if (!program || !out) return fail(DBG_ERR_INVALID, "null argument");
    ExprCompiled C;
    std::string msg;
    const int rc = expr_compile(program, C, msg);
    if (rc != DBG_OK) return fail(rc, msg);
    if (k < 0 || k >= C.n_outs) return fail(DBG_ERR_INVALID, "expression program: output index out of range");
    *out = C.out_types[k];
    return DBG_OK;
}

int dbg_expr_eval(const dbg_expr_program* program, const dbg_filter* filter, uint64_t rows, dbg_out_column* outs, void* stream) {
    if (!program || !outs) return fail(DBG_ERR_INVALID, "null argument");
    ExprCompiled C;
    std::string msg;
    const int rc = expr_compile(program, C, msg);
    if (rc != DBG_OK) return fail(rc, msg);
    std::vector<EProg> hp(1);  // large: not on the stack
    EProg& E = hp[0];
    memset(&E, 0, sizeof(E));
    E.rows = rows;
    E.n_nodes = (int32_t)C.nodes.size();
    E.n_cols = program->n_cols;
    for (int c = 0; c < program->n_cols; ++c) {
        const dbg_column& col = program->cols[c];
        if (col.len < rows) return fail(DBG_ERR_INVALID, "expression program: column shorter than rows");
        if (col.dt.type == DBG_STRING) {
            if (rows && !col.offsets) return fail(DBG_ERR_INVALID, "expression program: String column without offsets");
        } else if (rows && !col.data) {
            return fail(DBG_ERR_INVALID, "expression program: column without data");
        }
        E.cols[c] = dcol_view(col);
    }
    for (size_t k = 0; k < C.nodes.size(); ++k) E.nodes[k] = C.nodes[k];
    for (int o = 0; o < C.n_outs; ++o) {
        const dbg_datatype& t = C.out_types[o];
        outs[o].dt = t;
        if (rows && (!outs[o].data || (t.nullable && !outs[o].validity))) return fail(DBG_ERR_INVALID, "expression program: output without a buffer");
        E.outs[o].data = (u8*)outs[o].data;
        E.outs[o].validity = t.nullable ? outs[o].validity : nullptr;
        E.outs[o].width = type_width(t.type);
        E.outs[o].is_f32 = t.type == DBG_FLOAT32;
    }
    if (rows == 0) return DBG_OK;
    hipStream_t s = (hipStream_t)stream;
    // Everything the queued work reads lives here, and every way out — an error after something
    // was queued included — waits for the stream before these buffers go.
    ExprLaunch L;
    u32 err = 0;
    int rc2 = expr_queue(C, E, filter, rows, s, L, &err);
    const hipError_t se = hipStreamSynchronize(s);  // the kernel has read the program, the filter and its constants
    if (rc2 != DBG_OK) return rc2;
    if (se != hipSuccess) return fail(DBG_ERR_DEVICE, std::string("expression program: ") + hipGetErrorString(se));
    if (err) {
        const int arith = (int)err - 1;
        return fail(DBG_ERR_OVERFLOW, std::string(arith == EX_MUL ? "Decimal multiply overflow" : "Decimal overflow") + " in " + expr_op_name(arith));
    }
    return DBG_OK;
}
}  // extern "C"
