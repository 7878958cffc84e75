// reduce.hip — aggregation without GROUP BY on gfx950: a streaming filter + reduce into one state
// (the reference's PartialSingleStateAggregator / FinalSingleStateAggregator,
// AGG/transform_single_key.rs: func.accumulate(place, columns, None, rows) and batch_merge_single).
//
// keyless_reduce_kernel: a workgroup takes tiles of KEYLESS_TILE rows grid-stride, a tile being
// KEYLESS_U strips of 256 x KEYLESS_R rows; a lane owns KEYLESS_R contiguous rows of every strip, so
// per strip a column is read with one to eight 16-byte loads per lane
// (any element offset: the loads are declared unaligned, gfx950 takes them at any byte address) and
// a validity or Boolean bitmap with one or two bytes at any bit offset.  The last, partial tile
// reads row by row with a bound check.  Per tile the predicate program runs once into a per-lane
// mask of its rows; then the aggregates are the outer loop (a wave-uniform switch on the state
// kind) and the lane's rows the inner loop into ONE register accumulator, which is reduced across
// the wave by a fixed xor-shuffle tree and folded by lane 0 into the wave's running state in LDS.
// After the last tile the four wave states are folded in wave order into partials[blockIdx]:
// plain stores, no atomics, no tickets, no spins.
// keyless_merge_kernel (one workgroup): lanes take the partial rows strided, reduce them in the
// same tree and fold the result into the handle's state with plain loads and stores; the kernel
// boundary orders it behind the reduce.  The same kernel folds decoded serialized states.
//
// Every mapping (row -> lane, tile -> workgroup, the trees) is a fixed function of the row count,
// so a float SUM over the same rows in the same batches has the same bits on every run.
#include "agg_dev.hpp"
#include "reduce.hpp"

namespace {

enum { R = KEYLESS_R, NT = KEYLESS_NT, NW = KEYLESS_NT / 64, U = KEYLESS_U, STRIP = KEYLESS_NT * KEYLESS_R };
static_assert(R == 8 && U * R <= 32, "a lane's rows of a tile are the bits of one 32-bit mask, a byte per strip");

// One aggregate's state in registers.  lo / hi: the sum or the extreme (hi: 128-bit kinds); cnt:
// COUNT's and AVG's count word (in the reduce kernel also: values that reached the state).
struct Acc {
    u64 lo, hi, cnt;
};
enum { OP_CNT, OP_ADD64, OP_ADDF, OP_ADD128, OP_MINS, OP_MAXS, OP_MINU, OP_MAXU, OP_MIN128, OP_MAX128 };

__device__ __forceinline__ int acc_op(const DAgg& A) {
    switch (A.kind) {
        case DBG_AGG_COUNT: return OP_CNT;
        case DBG_AGG_SUM: case DBG_AGG_AVG: return A.sumk == SUMK_I64 ? OP_ADD64 : (A.sumk == SUMK_F64 ? OP_ADDF : OP_ADD128);
        default: {
            const bool mn = A.kind == DBG_AGG_MIN;
            if (A.mmk == MMK_I128) return mn ? OP_MIN128 : OP_MAX128;
            if (A.mmk == MMK_I64) return mn ? OP_MINS : OP_MAXS;
            return mn ? OP_MINU : OP_MAXU;  // U64, and F64 through f64_order_key
        }
    }
}
__device__ __forceinline__ bool op_wide(int op) { return op == OP_ADD128 || op == OP_MIN128 || op == OP_MAX128; }

// the identities of Spec::slot_init (state_init_word)
__device__ __forceinline__ Acc acc_identity(int op) {
    switch (op) {
        case OP_MINS: return Acc{0x7fffffffffffffffULL, 0, 0};
        case OP_MAXS: return Acc{0x8000000000000000ULL, 0, 0};
        case OP_MINU: return Acc{~0ULL, 0, 0};
        case OP_MIN128: return Acc{~0ULL, 0x7fffffffffffffffULL, 0};
        case OP_MAX128: return Acc{0, 0x8000000000000000ULL, 0};
        default: return Acc{0, 0, 0};
    }
}

__device__ __forceinline__ void acc_value(int op, Acc& x, u64 lo, u64 hi) {
    switch (op) {
        case OP_ADD64: x.lo += lo; break;
        case OP_ADDF: x.lo = (u64)__double_as_longlong(__longlong_as_double((long long)x.lo) + __longlong_as_double((long long)lo)); break;
        case OP_ADD128: {
            const u64 s = x.lo + lo;
            x.hi += hi + (s < x.lo ? 1ULL : 0ULL);
            x.lo = s;
            break;
        }
        case OP_MINS: if ((i64)lo < (i64)x.lo) x.lo = lo; break;
        case OP_MAXS: if ((i64)lo > (i64)x.lo) x.lo = lo; break;
        case OP_MINU: if (lo < x.lo) x.lo = lo; break;
        case OP_MAXU: if (lo > x.lo) x.lo = lo; break;
        case OP_MIN128: if (i128_less(lo, hi, x.lo, x.hi)) { x.lo = lo; x.hi = hi; } break;
        case OP_MAX128: if (i128_less(x.lo, x.hi, lo, hi)) { x.lo = lo; x.hi = hi; } break;
        default: break;
    }
}
__device__ __forceinline__ void acc_combine(int op, Acc& x, const Acc& y) {
    acc_value(op, x, y.lo, y.hi);
    x.cnt += y.cnt;
}

// the fixed tree of a wave: after it every lane holds the wave's value
__device__ __forceinline__ Acc acc_wave(int op, Acc x) {
    const bool wide = op_wide(op);
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        Acc y;
        y.lo = __shfl_xor((unsigned long long)x.lo, off, 64);
        y.hi = wide ? __shfl_xor((unsigned long long)x.hi, off, 64) : 0;
        y.cnt = __shfl_xor((unsigned long long)x.cnt, off, 64);
        acc_combine(op, x, y);
    }
    return x;
}

// state words (slot layout) <-> Acc; P: a pointer type of any address space
template <typename P>
__device__ __forceinline__ Acc acc_load(int op, const DAgg& A, P st) {
    Acc x{0, 0, 0};
    const int w = A.w0;
    if (op == OP_CNT) {
        x.cnt = st[w];
    } else if (op == OP_MIN128 || op == OP_MAX128) {  // [seq, lo, hi]
        x.lo = st[w + 1];
        x.hi = st[w + 2];
    } else {
        x.lo = st[w];
        if (op == OP_ADD128) x.hi = st[w + 1];
        if (A.kind == DBG_AGG_AVG) x.cnt = st[w + (op == OP_ADD128 ? 2 : 1)];
    }
    return x;
}
template <typename P>
__device__ __forceinline__ void acc_store(int op, const DAgg& A, P st, const Acc& x) {
    const int w = A.w0;
    if (op == OP_CNT) {
        st[w] = x.cnt;
    } else if (op == OP_MIN128 || op == OP_MAX128) {
        st[w] = 0;  // the sequence word of the grouped path's seqlock: even
        st[w + 1] = x.lo;
        st[w + 2] = x.hi;
    } else {
        st[w] = x.lo;
        if (op == OP_ADD128) st[w + 1] = x.hi;
        if (A.kind == DBG_AGG_AVG) st[w + (op == OP_ADD128 ? 2 : 1)] = x.cnt;
    }
}

// ---- a lane's KEYLESS_R rows of a column ----
typedef u64 u64_u __attribute__((aligned(1)));
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));

// 8 bits of a bitmap from bit `bit` on; every one of them lies inside the bitmap (a full tile)
__device__ __forceinline__ u32 bits8(const u8* p, u64 bit) {
    const u32 sh = (u32)(bit & 7);
    u32 v = gld<u8>(p + (bit >> 3));
    if (sh) v |= (u32)gld<u8>(p + (bit >> 3) + 1) << 8;
    return (v >> sh) & 0xFFu;
}

// validity of the lane's rows as a mask (FULL: all R rows are rows of the batch)
template <bool FULL>
__device__ __forceinline__ u32 valid_mask(const DCol& c, u64 i0, u64 rows) {
    if (!c.nullable || c.validity == nullptr) return (1u << R) - 1;
    if (FULL) return bits8(c.validity, c.validity_offset + i0);
    u32 m = 0;
#pragma unroll
    for (int j = 0; j < R; ++j)
        if (i0 + j < rows && dcol_valid(c, i0 + j)) m |= 1u << j;
    return m;
}

// raw bits of the lane's rows, zero-extended (dcol_bits); a column of width <= 8
template <bool FULL>
__device__ __forceinline__ void load_bits(const DCol& c, u64 i0, u64 rows, u64 (&b)[R]) {
    if (!FULL) {
#pragma unroll
        for (int j = 0; j < R; ++j) b[j] = i0 + j < rows ? dcol_bits(c, i0 + j) : 0;
        return;
    }
    if (c.type == DBG_BOOLEAN) {
        const u32 v = bits8(c.data, c.data_offset + i0);
#pragma unroll
        for (int j = 0; j < R; ++j) b[j] = (v >> j) & 1u;
        return;
    }
    const u8* p = c.data + i0 * (u64)c.width;
    switch (c.width) {
        case 1: {
            const u64 v = *(const u64_u __attribute__((address_space(1)))*)p;
#pragma unroll
            for (int j = 0; j < R; ++j) b[j] = (v >> (8 * j)) & 0xFFu;
            break;
        }
        case 2: {
            const u32x4 v = *(const u32x4_u __attribute__((address_space(1)))*)p;
#pragma unroll
            for (int j = 0; j < R; ++j) b[j] = (v[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
            break;
        }
        case 4: {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const u32x4 v = *(const u32x4_u __attribute__((address_space(1)))*)(p + 16 * k);
#pragma unroll
                for (int j = 0; j < 4; ++j) b[4 * k + j] = v[j];
            }
            break;
        }
        default: {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const u32x4 v = *(const u32x4_u __attribute__((address_space(1)))*)(p + 16 * k);
                b[2 * k] = v[0] | ((u64)v[1] << 32);
                b[2 * k + 1] = v[2] | ((u64)v[3] << 32);
            }
        }
    }
}

// the value the state kinds take from raw bits: dcol_i64's sign extension, dcol_f64's widening
__device__ __forceinline__ u64 canon_value(int type, u64 b) {
    switch (type) {
        case DBG_INT8: return (u64)(i64)(int8_t)b;
        case DBG_INT16: return (u64)(i64)(int16_t)b;
        case DBG_INT32: case DBG_DATE: return (u64)(i64)(int32_t)b;
        case DBG_FLOAT32: return (u64)__double_as_longlong((double)__uint_as_float((u32)b));
        default: return b;
    }
}

// One aggregate over the lane's rows `vm` of argument column c into acc.
template <bool FULL>
__device__ __forceinline__ void lane_rows(const DAgg& A, int op, const DCol& c, u64 i0, u64 rows, u32 vm, Acc& acc) {
    if (c.width == 16) {  // Decimal128: [lo, hi] per row
#pragma unroll
        for (int j = 0; j < R; ++j) {
            u64 lo = 0, hi = 0;
            if (FULL) {
                const u32x4 v = *(const u32x4_u __attribute__((address_space(1)))*)(c.data + (i0 + j) * 16);
                lo = v[0] | ((u64)v[1] << 32);
                hi = v[2] | ((u64)v[3] << 32);
            } else if (i0 + j < rows) {
                lo = dcol_bits(c, i0 + j);
                hi = dcol_hi(c, i0 + j);
            }
            // (MMK_I64, precision <= 18: the low word is the value, as on the grouped path)
            if ((vm >> j) & 1u) acc_value(op, acc, lo, hi);
        }
        return;
    }
    u64 b[R];
    load_bits<FULL>(c, i0, rows, b);
    const bool fkey = op >= OP_MINS && A.mmk == MMK_F64;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        u64 v = canon_value(c.type, b[j]);
        if (fkey) v = f64_order_key(__longlong_as_double((long long)v));
        if ((vm >> j) & 1u) acc_value(op, acc, v, 0);
    }
}

// The same over all strips of a full tile for a column of width <= 8: every strip's loads are issued
// before the first value is used (no branch between them), so a lane has KEYLESS_U x its strip's
// loads in flight.  vm: bit 8 * u + j = row j of strip u.
__device__ __forceinline__ void lane_rows_full(const DAgg& A, int op, const DCol& c, u64 i0, u32 vm, Acc& acc) {
    const bool fkey = op >= OP_MINS && A.mmk == MMK_F64;
    const int type = c.type;
    auto step = [&](u64 bits, int k) {
        u64 v = canon_value(type, bits);
        if (fkey) v = f64_order_key(__longlong_as_double((long long)v));
        if ((vm >> k) & 1u) acc_value(op, acc, v, 0);
    };
    typedef const u32x4_u __attribute__((address_space(1)))* vptr;
    if (type == DBG_BOOLEAN) {
        u32 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = bits8(c.data, c.data_offset + i0 + (u64)u * STRIP);
#pragma unroll
        for (int k = 0; k < U * R; ++k) step((v[k / R] >> (k % R)) & 1u, k);
        return;
    }
    const u8* p = c.data + i0 * (u64)c.width;
    switch (c.width) {
        case 1: {
            u64 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = *(const u64_u __attribute__((address_space(1)))*)(p + (u64)u * STRIP);
#pragma unroll
            for (int k = 0; k < U * R; ++k) step((v[k / R] >> (8 * (k % R))) & 0xFFu, k);
            break;
        }
        case 2: {
            u32x4 v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = *(vptr)(p + (u64)u * STRIP * 2);
#pragma unroll
            for (int k = 0; k < U * R; ++k) step((v[k / R][(k % R) >> 1] >> (16 * (k & 1))) & 0xFFFFu, k);
            break;
        }
        case 4: {
            u32x4 v[U][2];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < 2; ++h) v[u][h] = *(vptr)(p + (u64)u * STRIP * 4 + 16 * h);
#pragma unroll
            for (int k = 0; k < U * R; ++k) step(v[k / R][(k % R) >> 2][k & 3], k);
            break;
        }
        default: {
            u32x4 v[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int h = 0; h < 4; ++h) v[u][h] = *(vptr)(p + (u64)u * STRIP * 8 + 16 * h);
#pragma unroll
            for (int k = 0; k < U * R; ++k) {
                const u32x4 w = v[k / R][(k % R) >> 1];
                step((k & 1) ? (w[2] | ((u64)w[3] << 32)) : (w[0] | ((u64)w[1] << 32)), k);
            }
        }
    }
}

// One tile: KEYLESS_U strips of NT * R rows; a lane owns R contiguous rows of every strip, bit
// 8 * u + j of its masks is row j of its part of strip u.  The strips of one aggregate are
// independent loads into the same accumulator, so a lane has up to KEYLESS_U of them in flight
// before the one wave reduction of the tile.
template <bool FULL>
__device__ __forceinline__ void reduce_tile(const Spec& S, const BatchDesc& B, u64 base, u64 rows, u64* ws /* LDS: this wave's state */) {
    const u32 lane = threadIdx.x & 63;
    const u64 i0 = base + (u64)threadIdx.x * R;  // strip u: i0 + u * STRIP
    u32 m = 0;
    if (B.n_nodes == 0) {
        if (FULL) {
            m = ~0u;
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const u64 r0 = i0 + (u64)u * STRIP;
                const u32 k = r0 >= rows ? 0u : (rows - r0 >= R ? (u32)R : (u32)(rows - r0));
                m |= ((1u << k) - 1) << (R * u);
            }
        }
    } else {
#pragma unroll 1
        for (int k = 0; k < U * R; ++k) {
            const u64 r = i0 + (u64)(k / R) * STRIP + (u64)(k % R);
            if ((FULL || r < rows) && eval_pred(B.nodes, B.n_nodes, B.fcols, r)) m |= 1u << k;
        }
    }
    if (__ballot(m != 0) == 0) return;  // no row of the wave's part of the tile reaches accumulate
    if (lane == 0) ws[S.flags_word] |= 1ULL << KEYLESS_SEEN_BIT;
#pragma unroll 1
    for (int a = 0; a < S.n_aggs; ++a) {
        const DAgg& A = S.aggs[a];
        const int op = acc_op(A);
        Acc acc = acc_identity(op);
        u32 vm = m;
        if (A.arg_type >= 0) {
            const DCol& c = B.args[a];
            if (A.arg_nullable) {
#pragma unroll
                for (int u = 0; u < U; ++u) vm &= (valid_mask<FULL>(c, i0 + (u64)u * STRIP, rows) << (R * u)) | ~(0xFFu << (R * u));
            }
            if (op != OP_CNT && __ballot(vm != 0) != 0) {
                if (FULL && c.width <= 8) {
                    lane_rows_full(A, op, c, i0, vm, acc);
                } else {  // Decimal128 (eight 16-byte loads per strip already), and the last, partial tile
#pragma unroll
                    for (int u = 0; u < U; ++u) lane_rows<FULL>(A, op, c, i0 + (u64)u * STRIP, rows, (vm >> (R * u)) & 0xFFu, acc);
                }
            }
        }
        acc.cnt = (u64)__popc(vm);
        acc = acc_wave(op, acc);
        if (lane == 0 && acc.cnt) {
            Acc cur = acc_load(op, A, ws);
            acc_combine(op, cur, acc);
            acc_store(op, A, ws, cur);  // (the count word of COUNT and AVG only)
            if (A.flag_bit >= 0) ws[S.flags_word] |= 1ULL << A.flag_bit;
        }
    }
}

__global__ void __launch_bounds__(KEYLESS_NT) keyless_reduce_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batch, u64 rows,
                                                                    u64* __restrict__ partials) {
    const Spec& S = *spec;
    const BatchDesc& B = *batch;
    __shared__ u64 wst[NW][DBG_MAX_WORDS];
    for (u32 k = threadIdx.x; k < NW * DBG_MAX_WORDS; k += NT) {
        const u32 w = k % DBG_MAX_WORDS;
        wst[k / DBG_MAX_WORDS][w] = (int)w <= S.n_words ? S.slot_init[w] : 0;
    }
    __syncthreads();
    u64* const ws = wst[threadIdx.x >> 6];
    const u64 tiles = (rows + KEYLESS_TILE - 1) / KEYLESS_TILE;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 base = t * KEYLESS_TILE;
        if (base + KEYLESS_TILE <= rows) reduce_tile<true>(S, B, base, rows, ws);
        else reduce_tile<false>(S, B, base, rows, ws);
    }
    __syncthreads();
    // the wave states in wave order -> this workgroup's partial row
    u64* const out = partials + (u64)blockIdx.x * (u64)S.stride_words;
    const int a = (int)threadIdx.x;
    if (a < S.n_aggs) {
        const DAgg& A = S.aggs[a];
        const int op = acc_op(A);
        Acc x = acc_load(op, A, wst[0]);
        for (int w = 1; w < NW; ++w) acc_combine(op, x, acc_load(op, A, wst[w]));
        acc_store(op, A, out, x);
    } else if (a == S.n_aggs) {
        u64 f = 0;
        for (int w = 0; w < NW; ++w) f |= wst[w][S.flags_word];
        out[S.flags_word] = f;
        out[0] = 0;
    }
}

__global__ void __launch_bounds__(KEYLESS_NT) keyless_merge_kernel(const Spec* __restrict__ spec, const u64* __restrict__ states, u64 n,
                                                                   u32 stride, u64* __restrict__ state) {
    const Spec& S = *spec;
    __shared__ Acc wacc[NW][DBG_MAX_AGGS];
    __shared__ u64 wflags[NW];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 f = 0;
    for (u64 p = threadIdx.x; p < n; p += NT) f |= states[p * stride + S.flags_word];
#pragma unroll
    for (int off = 32; off; off >>= 1) f |= __shfl_xor((unsigned long long)f, off, 64);
    if (lane == 0) wflags[wave] = f;
#pragma unroll 1
    for (int a = 0; a < S.n_aggs; ++a) {
        const DAgg& A = S.aggs[a];
        const int op = acc_op(A);
        Acc acc = acc_identity(op);
        for (u64 p = threadIdx.x; p < n; p += NT) acc_combine(op, acc, acc_load(op, A, states + p * stride));
        acc = acc_wave(op, acc);
        if (lane == 0) wacc[wave][a] = acc;
    }
    __syncthreads();
    const int a = (int)threadIdx.x;
    if (a < S.n_aggs) {
        const DAgg& A = S.aggs[a];
        const int op = acc_op(A);
        Acc x = acc_load(op, A, state);
        for (int w = 0; w < NW; ++w) acc_combine(op, x, wacc[w][a]);
        acc_store(op, A, state, x);
    } else if (a == S.n_aggs) {
        u64 g = state[S.flags_word];
        for (int w = 0; w < NW; ++w) g |= wflags[w];
        state[S.flags_word] = g;
    }
}

__global__ void keyless_init_kernel(const Spec* __restrict__ spec, u64* __restrict__ state) {
    const Spec& S = *spec;
    for (int w = (int)threadIdx.x; w < S.stride_words; w += (int)blockDim.x) state[w] = (w >= 1 && w <= S.n_words) ? S.slot_init[w] : 0;
}

// Serialized states -> word rows.  A state with OrNull flag 0 or None is what the reference's
// keyless partial writes for empty input (aggregate_ornull_adaptor.rs:108-126): it decodes to
// "nothing seen" (ERR_SER_UNREP is the grouped path's refusal, whose states cannot carry it).
__global__ void __launch_bounds__(256) keyless_decode_kernel(const Spec* __restrict__ spec, SerIngest in, u64 n, u64* __restrict__ words,
                                                             u64* __restrict__ err) {
    const Spec& S = *spec;
    u32 e = 0;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        u64* row = words + i * (u64)S.stride_words;
        for (int k = 0; k < S.stride_words; ++k) row[k] = (k >= 1 && k <= S.n_words) ? S.slot_init[k] : 0;
        u64 flags = 0;
        for (int a = 0; a < S.n_aggs; ++a) {
            const DAgg& A = S.aggs[a];
            const u64 o0 = gld<u64>(in.st_offs[a] + i), o1 = gld<u64>(in.st_offs[a] + i + 1);
            const u8* p = in.st_data[a] + o0;
            u32 r = ser_decode(S, A, p, o1 - o0, row + 1, &flags);
            if (r & ERR_SER_UNREP) {  // an OrNull-0 state that still holds a count: nothing seen
                for (int k = 0; k < A.nwords; ++k) row[A.w0 + k] = S.slot_init[A.w0 + k];
                r &= ~(u32)ERR_SER_UNREP;
            }
            if (!r && (A.ser_flags & SER_OR_NULL) && gld<u8>(p + (o1 - o0) - 1) > 0) flags |= 1ULL << KEYLESS_SEEN_BIT;
            e |= r;
        }
        row[S.flags_word] = flags;
    }
    if (e) atomicOr((unsigned long long*)err, (unsigned long long)e);
}

// The one result row through the grouped path's writers.  Serialized: agg_serialize writes the
// OrNull adaptor's byte as 1 (a group has rows); here it is the state's "rows seen" bit.
__global__ void keyless_write_kernel(const Spec* __restrict__ spec, const u64* __restrict__ state, OutDesc out, u64* __restrict__ err) {
    const Spec& S = *spec;
    const int a = (int)threadIdx.x;
    if (a >= S.n_aggs) return;
    const DAgg& A = S.aggs[a];
    // AVG over Decimal128 of precision > 18 (DecimalAvgState<OVERFLOW = true>, FUN/aggregate_avg.rs:
    // 141-153) range-checks its sum; build_spec marks it (dec_check) on a keyless spec, and like
    // SUM's the check is made on the final sum.  agg_result itself checks only the multiply.
    if (!out.ser && A.kind == DBG_AGG_AVG && !A.avg_round && A.dec_check && state[A.w0 + 2] != 0 &&
        dec38_out_of_range(state[A.w0], state[A.w0 + 1]))
        atomicOr((unsigned long long*)err, (unsigned long long)ERR_DEC_OVERFLOW);
    write_agg<false>(S, a, state, 0, out, err);
    if (out.ser && (A.ser_flags & SER_OR_NULL)) {
        const u32 len = out.agg_valid[a][0];
        ((u8*)out.agg_data[a])[len - 1] = (u8)((state[S.flags_word] >> KEYLESS_SEEN_BIT) & 1);
    }
}

}  // namespace

void launch_keyless_init(hipStream_t s, const Spec* dspec, u64* state) {
    hipLaunchKernelGGL(keyless_init_kernel, dim3(1), dim3(128), 0, s, dspec, state);
}

void launch_keyless_reduce(hipStream_t s, const Spec* dspec, const BatchDesc* batch, u64 rows, u64* partials, u32 blocks) {
    hipLaunchKernelGGL(keyless_reduce_kernel, dim3(blocks), dim3(KEYLESS_NT), 0, s, dspec, batch, rows, partials);
}

void launch_keyless_merge(hipStream_t s, const Spec* dspec, const u64* states, u64 n, u32 stride, u64* state) {
    if (!n) return;
    hipLaunchKernelGGL(keyless_merge_kernel, dim3(1), dim3(KEYLESS_NT), 0, s, dspec, states, n, stride, state);
}

void launch_keyless_decode(hipStream_t s, const Spec* dspec, const SerIngest& in, u64 n, u64* words, u64* err) {
    if (!n) return;
    u64 blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(keyless_decode_kernel, dim3((u32)blocks), dim3(256), 0, s, dspec, in, n, words, err);
}

void launch_keyless_write(hipStream_t s, const Spec* dspec, const u64* state, const OutDesc& out, u64* err) {
    hipLaunchKernelGGL(keyless_write_kernel, dim3(1), dim3(64), 0, s, dspec, state, out, err);
}
