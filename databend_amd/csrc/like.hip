// like.hip — the LIKE pre-pass: one match bitmap per LIKE node and batch (DBG_PRED_LIKE).
//
// eval_pred is inlined into every insert, scatter and filter kernel, several of them near their
// register limits, so no string search runs there: it reads one bit of a bitmap that a pre-pass on
// the same stream filled from the column (Arrow layout: offsets + bytes) just before.  Two kernels:
//
//  * like_rows_kernel — one lane per row, every pattern class (like.hpp's matchers): anchored
//    classes compare 8 bytes per step, the others run the per-row matcher with the pattern and its
//    segment table in LDS.  A wave ballots its 64 rows and lane 0 stores the mask word, so the mask
//    needs no memset and no atomics.
//  * like_scan_kernel — `%needle%` only: searches the column's contiguous byte blob
//    [offsets[0], offsets[rows]) in fixed tiles staged in LDS with 16-byte coalesced loads, instead
//    of the rows (whose lane-per-row byte loads are uncoalesced and length-skewed).  A hit is mapped
//    to its row by a binary search over the offsets of the tile's row range (staged in LDS when they
//    fit) and counts only when it ends inside that row; bits are OR-ed into the zeroed mask.
//
// Which of the two serves `%needle%`: launch_like_mask (rule and measurements: DESIGN.md §4.11).
#include "like.hpp"

#include <atomic>

typedef const u8 __attribute__((address_space(1)))* gbytes;
typedef const u8 __attribute__((address_space(3)))* lbytes;
typedef unsigned long long v2u64 __attribute__((ext_vector_type(2)));

#define LIKE_NT 256

__global__ void __launch_bounds__(LIKE_NT) like_rows_kernel(const u64* __restrict__ offsets, const u8* __restrict__ data, u64 rows,
                                                            LikeDesc L, const u8* __restrict__ dpat, u64* __restrict__ mask) {
    __shared__ u8 spat[DBG_LIKE_MAX_PATTERN];
    __shared__ uint16_t sseg[2 * DBG_LIKE_MAX_SEGMENTS];
    for (u32 t = threadIdx.x; t < L.pat_len; t += LIKE_NT) spat[t] = gld<u8>(dpat + t);
    if (threadIdx.x < DBG_LIKE_MAX_SEGMENTS) {
        sseg[threadIdx.x] = L.seg_off[threadIdx.x];
        sseg[DBG_LIKE_MAX_SEGMENTS + threadIdx.x] = L.seg_len[threadIdx.x];
    }
    __syncthreads();
    const u32 lane = threadIdx.x & 63;
    const u64 pl = L.pat_len;
    const lbytes lp = (lbytes)spat;
    // a wave owns 64 consecutive rows per step: `base` is the same in all its lanes
    for (u64 base = (u64)blockIdx.x * LIKE_NT + (threadIdx.x & ~63u); base < rows; base += (u64)gridDim.x * LIKE_NT) {
        const u64 i = base + lane;
        bool m = false;
        if (i < rows) {
            const u64 a = gld<u64>(offsets + i), hl = gld<u64>(offsets + i + 1) - a;
            const u8* h = data + a;
            switch (L.kind) {
                case DBG_LIKE_ORDINAL: m = hl == pl && bytes_equal(h, dpat, pl); break;
                case DBG_LIKE_END_OF_PERCENT: m = hl >= pl - 1 && bytes_equal(h, dpat, pl - 1); break;
                case DBG_LIKE_START_OF_PERCENT: m = hl >= pl - 1 && bytes_equal(h + (hl - (pl - 1)), dpat + 1, pl - 1); break;
                case DBG_LIKE_SURROUND_BY_PERCENT: m = pl > 2 ? like_find_end((gbytes)h, hl, lp + 1, pl - 2) >= 0 : true; break;
                case DBG_LIKE_SIMPLE:
                    m = like_simple((gbytes)h, hl, lp, L.has_start != 0, L.has_end != 0, sseg, sseg + DBG_LIKE_MAX_SEGMENTS, L.n_seg);
                    break;
                default: m = like_complex((gbytes)h, hl, lp, pl); break;
            }
        }
        const u64 b = __ballot(m);
        if (lane == 0) mask[base >> 6] = b;
    }
}

// ---- %needle% over the blob --------------------------------------------------------------------
// A tile is SCAN_TILE bytes of address space from a 16-byte aligned base; its workgroup stages them
// plus needle_len - 1 bytes of overhang, so every match that STARTS in the tile is found by it and by
// no other.  About 21 KB of LDS per workgroup (tile, overhang, needle, the tile's row offsets): LDS
// admits seven workgroups per CU, the wave slots eight.
#define SCAN_TILE 16384
#define SCAN_OVER 256  // >= DBG_LIKE_MAX_PATTERN - 2 - 1 bytes of overhang, rounded to 16
#define SCAN_PER (SCAN_TILE / 16 / LIKE_NT)  // whole 16-byte chunks per lane and tile
#define SCAN_ROWS 512  // offsets of a tile's rows held in LDS; a tile of more rows searches them in global memory

// bit 7 of every byte of x that is zero (exact: no carry between bytes)
__device__ __forceinline__ u64 zero_bytes(u64 x) {
    const u64 lo7 = 0x7F7F7F7F7F7F7F7FULL;
    return ~(((x & lo7) + lo7) | x | lo7);
}

// largest r in [lo, hi] with offsets[r] <= q (offsets[lo] <= q is the caller's)
__device__ __forceinline__ u64 row_of(const u64* __restrict__ offsets, u64 lo, u64 hi, u64 q) {
    while (lo < hi) {
        const u64 mid = lo + (hi - lo + 1) / 2;
        if (gld<u64>(offsets + mid) <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// The same by a whole wave, 64 probes per step (all 64 lanes call it, all get the result): four
// dependent loads instead of twenty-three for ten million rows.  offsets are non-decreasing, so the
// probes with offsets[p] <= q are a prefix of the lanes.
__device__ __forceinline__ u64 row_of_wave(const u64* __restrict__ offsets, u64 lo, u64 hi, u64 q, u32 lane) {
    while (hi - lo >= 64) {
        const u64 span = hi - lo;  // probe l = lo + span * (l + 1) / 64: strictly increasing, the last one hi
        const u32 c = (u32)__popcll(__ballot(gld<u64>(offsets + lo + ((span * (u64)(lane + 1)) >> 6)) <= q));
        const u64 nlo = c ? lo + ((span * (u64)c) >> 6) : lo;
        hi = c < 64 ? lo + ((span * (u64)(c + 1)) >> 6) - 1 : hi;
        lo = nlo;
    }
    const u64 p = lo + lane;
    const u32 c = (u32)__popcll(__ballot(p <= hi && gld<u64>(offsets + p) <= q));  // >= 1: offsets[lo] <= q
    return lo + c - 1;
}
// the same over offsets staged in LDS
__device__ __forceinline__ u32 row_of_lds(const u64* soff, u32 lo, u32 hi, u64 q) {
    while (lo < hi) {
        const u32 mid = lo + (hi - lo + 1) / 2;
        if (soff[mid] <= q) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// chunk k of the tile at T0 into LDS: a whole 16-byte chunk inside the blob [A, E) as loaded (w), the
// blob's first and last partial chunk byte by byte — nothing outside the blob is read
__device__ __forceinline__ void stage_chunk(u8* sb, u32 k, uintptr_t p, uintptr_t A, uintptr_t E, v2u64 w) {
    if (p >= A && p + 16 <= E) {
        *(v2u64*)(sb + 16 * k) = w;
    } else if (p < E && p + 16 > A) {
        for (u32 b = 0; b < 16; ++b) sb[16 * k + b] = (p + b >= A && p + b < E) ? gld<u8>((const u8*)p + b) : (u8)0;
    }
}

__global__ void __launch_bounds__(LIKE_NT) like_scan_kernel(const u64* __restrict__ offsets, const u8* __restrict__ data, u64 rows,
                                                            const u8* __restrict__ dneedle, u32 m, u32* __restrict__ mask) {
    __shared__ __attribute__((aligned(16))) u8 sb[SCAN_TILE + SCAN_OVER];
    __shared__ __attribute__((aligned(16))) u8 sneedle[DBG_LIKE_MAX_PATTERN];
    __shared__ u64 soff[SCAN_ROWS];
    __shared__ u64 srow[2];
    for (u32 t = threadIdx.x; t < m; t += LIKE_NT) sneedle[t] = gld<u8>(dneedle + t);
    const u64 o0 = gld<u64>(offsets), o1 = gld<u64>(offsets + rows);
    if (o1 - o0 < m) return;  // no row can hold the needle (uniform)
    // addresses: the blob is [A, E); tiles start at A rounded down to 16 bytes
    const uintptr_t A = (uintptr_t)data + o0, E = (uintptr_t)data + o1, T00 = A & ~(uintptr_t)15;
    const u64 n_tiles = (E - T00 + SCAN_TILE - 1) / SCAN_TILE;
    const u64 last_start = E - m;  // the last address a match can start at
    const u64 c0x8 = 0x0101010101010101ULL * gld<u8>(dneedle);
    const u64 c1x8 = 0x0101010101010101ULL * (m > 1 ? gld<u8>(dneedle + 1) : 0);
    const u32 n_chunks = (SCAN_TILE + m - 1 + 15) / 16;
    for (u64 t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uintptr_t T0 = T00 + t * SCAN_TILE;
        // the tile's whole chunks: all of a lane's loads in flight before the first is stored
        v2u64 w[SCAN_PER];
#pragma unroll
        for (u32 j = 0; j < SCAN_PER; ++j) {
            const uintptr_t p = T0 + 16 * (uintptr_t)(threadIdx.x + j * LIKE_NT);
            w[j] = (p >= A && p + 16 <= E) ? gld<v2u64>((const void*)p) : v2u64{0, 0};
        }
        __syncthreads();  // the previous tile's readers are done (and sneedle is written)
        // the tile's row range: the rows of its first and last blob byte, by the first two waves
        // (whose tile loads are in flight meanwhile)
        if (threadIdx.x < 128) {
            const u32 wv = threadIdx.x >> 6;
            const uintptr_t lo = T0 > A ? T0 : A, hi = (T0 + SCAN_TILE < E ? T0 + SCAN_TILE : E) - 1;
            const u64 r = row_of_wave(offsets, 0, rows - 1, (wv ? hi : lo) - (uintptr_t)data, threadIdx.x & 63);
            if ((threadIdx.x & 63) == 0) srow[wv] = r;
        }
#pragma unroll
        for (u32 j = 0; j < SCAN_PER; ++j) {
            const u32 k = threadIdx.x + j * LIKE_NT;
            stage_chunk(sb, k, T0 + 16 * (uintptr_t)k, A, E, w[j]);
        }
        for (u32 k = SCAN_TILE / 16 + threadIdx.x; k < n_chunks; k += LIKE_NT) {  // the overhang
            const uintptr_t p = T0 + 16 * (uintptr_t)k;
            stage_chunk(sb, k, p, A, E, (p >= A && p + 16 <= E) ? gld<v2u64>((const void*)p) : v2u64{0, 0});
        }
        __syncthreads();
        const u64 r_lo = srow[0], r_hi = srow[1];
        // offsets[r_lo .. r_hi + 1] into LDS when they fit: a hit then finds its row there
        const u32 n_off = r_hi - r_lo + 2 <= SCAN_ROWS ? (u32)(r_hi - r_lo + 2) : 0;  // uniform
        for (u32 i = threadIdx.x; i < n_off; i += LIKE_NT) soff[i] = gld<u64>(offsets + r_lo + i);
        __syncthreads();
        // every lane tests the 16 start positions of its chunks: first- and second-byte reject on two
        // words, then the rest of the needle from LDS
#pragma unroll
        for (u32 j = 0; j < SCAN_PER; ++j) {
            const u32 k = threadIdx.x + j * LIKE_NT;
            const uintptr_t p = T0 + 16 * (uintptr_t)k;
            if (p > last_start) break;
            const v2u64 v = *(const v2u64*)(sb + 16 * k);
            u64 z0 = zero_bytes(v.x ^ c0x8), z1 = zero_bytes(v.y ^ c0x8);
            if (m > 1) {  // byte i + 1 is the needle's second byte (the chunk's last byte: not known here)
                const u64 y0 = zero_bytes(v.x ^ c1x8), y1 = zero_bytes(v.y ^ c1x8);
                z0 &= (y0 >> 8) | (y1 << 56);
                z1 &= (y1 >> 8) | 0x8000000000000000ULL;
            }
            while (z0 | z1) {
                u32 b;
                if (z0) {
                    b = (u32)__builtin_ctzll(z0) >> 3;
                    z0 &= z0 - 1;
                } else {
                    b = 8 + ((u32)__builtin_ctzll(z1) >> 3);
                    z1 &= z1 - 1;
                }
                const uintptr_t q = p + b;
                if (q < A || q > last_start) continue;
                const u32 s = 16 * k + b;
                bool eq = true;
                for (u32 i = 1; i < m && eq; ++i) eq = sb[s + i] == sneedle[i];
                if (!eq) continue;
                // inside one row?  (a needle made of the end of one row and the start of the next is no match)
                const u64 off = q - (uintptr_t)data;
                u64 r, end;
                if (n_off) {
                    const u32 i = row_of_lds(soff, 0, n_off - 2, off);
                    r = r_lo + i;
                    end = soff[i + 1];
                } else {
                    r = row_of(offsets, r_lo, r_hi, off);
                    end = gld<u64>(offsets + r + 1);
                }
                if (off + m <= end) atomicOr(mask + (r >> 5), 1u << (r & 31));
            }
        }
    }
}

static std::atomic<u64> g_counts[LIKE_K_N];
static std::atomic<int> g_force{0};  // dbg_like_force_kernel: LIKE_K_ROWS / LIKE_K_SCAN, 0 = the rule below

void like_force_kernel(int k) { g_force = k; }

void like_kernel_counts(u64* out) {
    for (int k = 0; k < LIKE_K_N; ++k) out[k] = g_counts[k].load();
}

// `%needle%`: the scan kernel (DESIGN.md §4.11 has the measurements behind the rule).  Every other
// class, and the forced fallback, goes lane-per-row.
static bool scan_serves(const LikeDesc& L) {
    if (L.kind != DBG_LIKE_SURROUND_BY_PERCENT || L.pat_len <= 2) return false;
    if (g_force == LIKE_K_ROWS) return false;  // result-neutral test hook
    return true;
}

int launch_like_mask(hipStream_t s, const DCol& col, u64 rows, const LikeDesc& L, const u8* dpat, u64* mask) {
    const u64 words = (rows + 63) / 64;
    if (rows == 0) return LIKE_K_FILL;
    if (L.kind == DBG_LIKE_SURROUND_BY_PERCENT && L.pat_len <= 2) {  // '%%' matches every string
        (void)hipMemsetAsync(mask, 0xFF, words * 8, s);
        g_counts[LIKE_K_FILL]++;
        return LIKE_K_FILL;
    }
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1)
            v = 256;
        n_cu = v;
    }
    if (scan_serves(L)) {
        (void)hipMemsetAsync(mask, 0, words * 8, s);
        // the blob's size is on the device: a fixed grid of eight workgroups per CU strides the tiles
        hipLaunchKernelGGL(like_scan_kernel, dim3((u32)n_cu * 8), dim3(LIKE_NT), 0, s, col.offsets, col.data, rows, dpat + 1,
                           L.pat_len - 2, (u32*)mask);
        g_counts[LIKE_K_SCAN]++;
        return LIKE_K_SCAN;
    }
    u64 blocks = (rows + LIKE_NT - 1) / LIKE_NT;
    if (blocks > (u64)n_cu * 8) blocks = (u64)n_cu * 8;
    hipLaunchKernelGGL(like_rows_kernel, dim3((u32)blocks), dim3(LIKE_NT), 0, s, col.offsets, col.data, rows, L, dpat, mask);
    g_counts[LIKE_K_ROWS]++;
    return LIKE_K_ROWS;
}
