// like.hpp — SQL LIKE as Databend's select path evaluates it (EXP/filter/like.rs), restated.
//
// The reference classifies a constant pattern once per query (generate_like_pattern, like.rs:186-248)
// and runs one matcher per class over the column (select_column_like,
// select_value/select_column_scalar.rs:163-...).  Both are restated here byte for byte, quirks
// included — they are the contract, not bugs to fix:
//   * `_` anywhere, or `\` followed by `%`, `_` or `\`, makes the pattern Complex; a `\` elsewhere
//     only clears "simple".  So a pattern with such a backslash and no `%`, one leading or trailing
//     `%`, or one of each, is compared RAW, the backslash a byte like any other.
//   * SurroundByPercent with an empty needle (`%%`) matches everything, the empty string too.
//   * a SimplePattern never matches an empty haystack (`'' LIKE '%%%'` is false).
//   * ComplexPattern backtracks to the last `%`; `_` consumes one BYTE (decode_one is one byte); `\`
//     escapes the next pattern byte when one follows, and stands for itself at the pattern's end.
//
// One source for the device (like.hip) and the host (dbg_like_match_host; LIKE_HOST: a plain C++
// build for the stand-alone sanitizer program, tests/csrc/like_host_main.cpp).  The matchers are
// templates over the pointer types so that the device reads the haystack through a global and the
// pattern through an LDS pointer; they read haystack bytes [0, hl) and pattern bytes [0, pl) only.
#pragma once
#ifdef LIKE_HOST
#include <cstdint>
typedef uint64_t u64;
typedef int64_t i64;
typedef uint32_t u32;
typedef uint8_t u8;
#define LIKE_FN static inline
#include "../../include/dbgpu_agg.h"
#else
#include "device.hpp"
#define LIKE_FN __host__ __device__ __forceinline__
#endif

// A classified pattern as the kernels take it.  The pattern's bytes travel beside it; a
// SimplePattern's segments are (offset, length) pairs into them.
struct LikeDesc {
    int32_t kind;  // dbg_like_kind
    int32_t n_seg;
    uint8_t has_start, has_end, pad_[2];
    uint32_t pat_len;
    uint16_t seg_off[DBG_LIKE_MAX_SEGMENTS], seg_len[DBG_LIKE_MAX_SEGMENTS];
};

// generate_like_pattern.  Returns false when a SimplePattern has more segments than LikeDesc
// holds (L.kind is set either way); len <= DBG_LIKE_MAX_PATTERN is the caller's check.
inline bool like_classify(const u8* pat, u64 len, LikeDesc& L) {
    L = LikeDesc{};
    L.pat_len = (uint32_t)len;
    L.kind = DBG_LIKE_ORDINAL;
    if (len == 0) return true;
    u64 index = 0, first_non_percent = 0, percent_num = 0, n_seg = 0;
    const bool has_start = pat[0] == '%';
    bool has_end = false, simple = true;
    auto push = [&](u64 a, u64 b) {
        if (n_seg < DBG_LIKE_MAX_SEGMENTS) {
            L.seg_off[n_seg] = (uint16_t)a;
            L.seg_len[n_seg] = (uint16_t)(b - a);
        }
        ++n_seg;
    };
    if (has_start) index = first_non_percent = percent_num = 1;
    while (index < len) {
        const u8 c = pat[index];
        if (c == '_') {
            L.kind = DBG_LIKE_COMPLEX;
            return true;
        }
        if (c == '%') {
            ++percent_num;
            if (index > first_non_percent) push(first_non_percent, index);
            first_non_percent = index + 1;
            if (index == len - 1) has_end = true;
        } else if (c == '\\') {
            simple = false;
            if (index < len - 1) {
                ++index;
                if (pat[index] == '%' || pat[index] == '_' || pat[index] == '\\') {
                    L.kind = DBG_LIKE_COMPLEX;
                    return true;
                }
            }
        }
        ++index;
    }
    if (percent_num == 0) L.kind = DBG_LIKE_ORDINAL;
    else if (percent_num == 1 && has_start) L.kind = DBG_LIKE_START_OF_PERCENT;
    else if (percent_num == 1 && has_end) L.kind = DBG_LIKE_END_OF_PERCENT;
    else if (percent_num == 2 && has_start && has_end) L.kind = DBG_LIKE_SURROUND_BY_PERCENT;
    else if (!simple) L.kind = DBG_LIKE_COMPLEX;
    else {
        if (first_non_percent < len) push(first_non_percent, len);
        L.kind = DBG_LIKE_SIMPLE;
        L.has_start = has_start;
        L.has_end = has_end;
        L.n_seg = (int32_t)(n_seg < DBG_LIKE_MAX_SEGMENTS ? n_seg : DBG_LIKE_MAX_SEGMENTS);
        return n_seg <= DBG_LIKE_MAX_SEGMENTS;
    }
    return true;
}

template <class HP, class PP>
LIKE_FN bool like_bytes_eq(HP h, PP p, u64 n) {
    for (u64 i = 0; i < n; ++i)
        if (h[i] != p[i]) return false;
    return true;
}

// like.rs `find`: the first occurrence of needle (nl >= 1) in the haystack; the position just past
// it, or -1.  (The reference filters candidates by a rolling byte checksum before the same
// comparison; what it returns is the first occurrence.)
template <class HP, class PP>
LIKE_FN i64 like_find_end(HP h, u64 hl, PP needle, u64 nl) {
    if (nl > hl) return -1;
    const u8 c0 = needle[0];
    for (u64 i = 0; i + nl <= hl; ++i)
        if (h[i] == c0 && like_bytes_eq(h + i + 1, needle + 1, nl - 1)) return (i64)(i + nl);
    return -1;
}

// LikePattern::simple_pattern
template <class HP, class PP>
LIKE_FN bool like_simple(HP h, u64 hl, PP pat, bool has_start, bool has_end, const uint16_t* seg_off, const uint16_t* seg_len,
                         int n_seg) {
    if (hl == 0) return false;
    u64 start = 0;
    int si = 0;
    if (!has_start) {
        const u64 sl = seg_len[0];
        if (sl > hl) return false;
        if (!like_bytes_eq(h, pat + seg_off[0], sl)) return false;
        start = sl;
        si = 1;
    }
    for (; si < n_seg; ++si) {
        if (start >= hl) return false;
        const u64 sl = seg_len[si];
        if (si == n_seg - 1 && !has_end) {
            if (hl - start < sl) return false;
            if (!like_bytes_eq(h + (hl - sl), pat + seg_off[si], sl)) return false;
        } else {
            const i64 e = like_find_end(h + start, hl - start, pat + seg_off[si], sl);
            if (e < 0) return false;
            start += (u64)e;
        }
    }
    return true;
}

// LikePattern::complex_pattern
template <class HP, class PP>
LIKE_FN bool like_complex(HP h, u64 hl, PP pat, u64 pl) {
    u64 px = 0, tx = 0, next_px = 0, next_tx = 0;
    while (px < pl || tx < hl) {
        if (px < pl) {
            const u8 c = pat[px];
            if (c == '_') {
                if (tx < hl) {
                    ++px;
                    ++tx;
                    continue;
                }
            } else if (c == '%') {
                next_px = px;
                ++px;
                next_tx = tx + 1;
                continue;
            } else {
                if (c == '\\' && px + 1 < pl) ++px;
                if (tx < hl && h[tx] == pat[px]) {
                    ++tx;
                    ++px;
                    continue;
                }
            }
        }
        if (0 < next_tx && next_tx <= hl) {  // mismatch: back to the last %
            px = next_px;
            tx = next_tx;
            continue;
        }
        return false;
    }
    return true;
}

// One cell against a classified pattern (pat: the raw pattern bytes, L.pat_len of them).
template <class HP, class PP>
LIKE_FN bool like_match(const LikeDesc& L, HP h, u64 hl, PP pat) {
    const u64 pl = L.pat_len;
    switch (L.kind) {
        case DBG_LIKE_ORDINAL: return hl == pl && like_bytes_eq(h, pat, pl);
        case DBG_LIKE_END_OF_PERCENT: return hl >= pl - 1 && like_bytes_eq(h, pat, pl - 1);
        case DBG_LIKE_START_OF_PERCENT: return hl >= pl - 1 && like_bytes_eq(h + (hl - (pl - 1)), pat + 1, pl - 1);
        case DBG_LIKE_SURROUND_BY_PERCENT: return pl > 2 ? like_find_end(h, hl, pat + 1, pl - 2) >= 0 : true;
        case DBG_LIKE_SIMPLE: return like_simple(h, hl, pat, L.has_start != 0, L.has_end != 0, L.seg_off, L.seg_len, L.n_seg);
        default: return like_complex(h, hl, pat, pl);
    }
}

#ifndef LIKE_HOST
// ---- like.hip ----
// The match bitmap of one LIKE node over a batch's column (LAYOUT_ARROW, on the device): bit i of
// `mask` ((rows + 63) / 64 words) = row i matches, whatever its validity.  dpat: the device copy of
// the pattern.  Launched on s; the consumer kernel follows on the same stream.
enum { LIKE_K_FILL = 0, LIKE_K_ROWS = 1, LIKE_K_SCAN = 2, LIKE_K_N = 3 };
int launch_like_mask(hipStream_t s, const DCol& col, u64 rows, const LikeDesc& L, const u8* dpat, u64* mask);
void like_kernel_counts(u64* out /* [LIKE_K_N] */);
void like_force_kernel(int k);  // LIKE_K_ROWS / LIKE_K_SCAN for `%needle%`, 0: launch_like_mask's own rule
#endif
