// agg_export.hip — the table's groups as partial-state records (partitioned by hash % n or radix
// bits, or in fixed segments), the serialized-state compaction, and the String MIN/MAX result
// gather.  File map: agg_table.hpp.
#include "agg_table.hpp"
#include "agg_fin_small.hpp"

// ------------------------------------------------------------------------------------------
// Export partial-state records: [hash][key part][state words], partition-major.
// ------------------------------------------------------------------------------------------
// Key part of a record from an inline (packed) entry.
__device__ __forceinline__ void write_inline_key_part(const Spec& S, u64 key, u8* rec) {
    for (int c = 0; c < S.n_keys; ++c) {
        const dbg_datatype& ty = S.key_types[c];
        u32 w = type_width(ty.type);
        u64 b = (key >> (8 * S.koff[c])) & width_mask(w);
        if (ty.nullable) rec[S.rec_val_off[c]] = ((key >> (8 * S.voff[c])) & 0xff) != 0;
        for (u32 j = 0; j < w; ++j) rec[S.rec_key_off[c] + j] = (u8)(b >> (8 * j));
    }
}

__global__ void __launch_bounds__(BLOCK) export_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                      TableDesc t, u32 n_parts, int scheme, const u32* __restrict__ lpart,
                                                      const u64* pos, const u64* str_pos, u64 nblocks, u8* rec_out, u8* str_out,
                                                      const u64* part_str_base) {
    const Spec& S = *spec;
    __shared__ unsigned long long cur[MAX_PARTS_LDS];
    __shared__ unsigned long long scur[DBG_MAX_KEYS][MAX_PARTS_LDS];
    for (u32 p = threadIdx.x; p < n_parts; p += BLOCK) cur[p] = pos[(u64)p * nblocks + blockIdx.x];
    bool ref_strings = S.has_strings && !S.inline_keys;
    if (ref_strings)
        for (u32 p = threadIdx.x; p < n_parts; p += BLOCK)
            for (int c = 0; c < S.n_keys; ++c)
                if (S.key_types[c].type == DBG_STRING) scur[c][p] = str_pos[((u64)p * S.n_keys + c) * nblocks + blockIdx.x];
    __syncthreads();
    u64 base = (u64)blockIdx.x * SLOTS_PER_BLOCK;
    for (u32 k = threadIdx.x; k < SLOTS_PER_BLOCK; k += BLOCK) {
        u64 s = base + k;
        if (s > t.cap) break;
        const u64* st = t.slots + s * t.stride_words;
        u64 e = st[0];
        if (e == SLOT_EMPTY) continue;
        u64 h = entry_hash(S, batches, e, s == t.cap);
        u32 p = part_of(h, n_parts, scheme, lpart, s);
        u64 r = atomicAdd(&cur[p], 1ULL);
        u8* rec = rec_out + r * S.rec_width;
        *(u64*)rec = h;
        if (S.inline_keys) {
            write_inline_key_part(S, s == t.cap ? SLOT_EMPTY : e, rec);
        } else {
            const BatchDesc& RB = batches[ref_bid(e)];
            u64 row = ref_row(e);
            for (int c = 0; c < S.n_keys; ++c) {
                const DCol& kc = RB.keys[c];
                bool v = dcol_valid(kc, row);
                if (S.key_types[c].nullable) rec[S.rec_val_off[c]] = v ? 1 : 0;
                u8* kd = rec + S.rec_key_off[c];
                if (kc.type == DBG_STRING) {
                    StrRef sr = dcol_str(kc, row);
                    u64 o = atomicAdd(&scur[c][p], (unsigned long long)sr.len);
                    for (u64 j = 0; j < sr.len; ++j) str_out[o + j] = sr.p[j];
                    ((u64*)kd)[0] = o - part_str_base[p];  // relative to the partition's blob
                    ((u64*)kd)[1] = sr.len;
                } else {
                    u32 w = type_width(kc.type);
                    u64 lo = dcol_bits(kc, row);
                    u64 hi = w == 16 ? dcol_hi(kc, row) : 0;
                    for (u32 j = 0; j < w && j < 8; ++j) kd[j] = (u8)(lo >> (8 * j));
                    for (u32 j = 8; j < w; ++j) kd[j] = (u8)(hi >> (8 * (j - 8)));
                }
            }
        }
        u64* sw = (u64*)(rec + S.rec_state_off);
        for (int w = 1; w <= S.n_words; ++w) sw[w - 1] = st[w];
    }
}

void launch_export(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, const TableDesc& t, u32 n_parts,
                   int scheme, const u32* lpart, const u64* pos, const u64* str_pos, u8* rec_out, u8* str_out,
                   const u64* part_str_base) {
    u64 nb = finalize_blocks(t.cap);
    hipLaunchKernelGGL(export_kernel, dim3((u32)nb), dim3(BLOCK), 0, s, dspec, batches, t, n_parts, scheme, lpart, pos, str_pos, nb,
                       rec_out, str_out, part_str_base);
}


// ------------------------------------------------------------------------------------------
// export_fixed: the groups of a small inline-key table as records in a fixed-capacity buffer
// whose record 0 is the header [count][flags] — replicas + gather for low cardinality
// (SURVEY.md §8e): the count never leaves the device, so the exchange that follows (an RCCL
// all-gather of equal-size buffers) and the merge need no host round trip.  One workgroup, the
// same owned-slot scan as finalize_small.  flags = 1: incomplete (more groups than capacity, or
// inserts still deferred in the overflow lists); the merge turns that into a finalize error.
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FIN_NT) export_fixed_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                              TableDesc t, u8* buf, u64 cap_records, int recycle) {
    const Spec& S = *spec;
    __shared__ u64 wsum[FIN_NT / 64];
    const u64 n_slots = t.cap + 1;
    const u32 per = (u32)((n_slots + FIN_NT - 1) / FIN_NT);
    const u64 base = (u64)threadIdx.x * per;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 ent[FIN_MAXPER];
    u32 occ = 0, cnt = 0;
#pragma unroll
    for (u32 k = 0; k < FIN_MAXPER; ++k) {
        u64 s = base + k;
        ent[k] = (k < per && s < n_slots) ? gld<u64>(t.slots + s * t.stride_words) : SLOT_EMPTY;
    }
#pragma unroll
    for (u32 k = 0; k < FIN_MAXPER; ++k)
        if (ent[k] != SLOT_EMPTY) {
            occ |= 1u << k;
            cnt++;
        }
    u64 ic = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        u64 o = __shfl_up(ic, off, 64);
        if (lane >= off) ic += o;
    }
    if (lane == 63) wsum[wave] = ic;
    __syncthreads();
    u64 p = ic - cnt, total = 0;
    for (int w = 0; w < FIN_NT / 64; ++w) {
        if (w < wave) p += wsum[w];
        total += wsum[w];
    }
    const u32 rw = S.rec_width;
    while (occ && p < cap_records) {
        const u32 k = __builtin_ctz(occ);
        occ &= occ - 1;
        const u64 s = base + k;
        const u64* st = t.slots + s * t.stride_words;
        const u64 e = gld<u64>(st);
        u8* rec = buf + (1 + p) * rw;
        const u64 key = s == t.cap ? SLOT_EMPTY : e;
        *(u64*)rec = hash_packed(S, key);
        write_inline_key_part(S, key, rec);
        u64* sw = (u64*)(rec + S.rec_state_off);
        for (int w = 1; w <= S.n_words; ++w) sw[w - 1] = gld<u64>(st + w);
        p++;
    }
    if (threadIdx.x == 0) {
        const bool pending = ld_sc1(t.counters + CNT_OVF_ROWS) != 0 || ld_sc1(t.counters + CNT_OVF_RECS) != 0;
        ((u64*)buf)[0] = total < cap_records ? total : cap_records;
        ((u64*)buf)[1] = (total > cap_records || pending) ? 1 : 0;
    }
    if (recycle) {  // dbg_agg_set_recycle: table_init of the owned slots + counter reset (an
                    // incomplete export is flagged above, so nothing is lost silently)
        __syncthreads();  // every state word has been read
        if (threadIdx.x < CNT_WORDS) t.counters[threadIdx.x] = 0;
        const u32 sw = (u32)t.stride_words;
        for (u32 k = 0; k < per; ++k) {
            u64 s = base + k;
            if (s >= n_slots) break;
            u64* d = t.slots + s * sw;
            for (u32 w = 0; w < sw; ++w) d[w] = S.slot_init[w];
        }
    }
}

void launch_export_fixed(hipStream_t s, const Spec* dspec, const BatchDesc* batches, const TableDesc& t, u8* buf, u64 cap_records,
                         int recycle) {
    hipLaunchKernelGGL(export_fixed_kernel, dim3(1), dim3(FIN_NT), 0, s, dspec, batches, t, buf, cap_records, recycle);
}

// ------------------------------------------------------------------------------------------
// Serialized states (dbg_agg_result_serialized): rows written at a fixed stride with their
// lengths -> a Binary column (offsets from an exclusive scan of the lengths, then the bytes).
// ------------------------------------------------------------------------------------------
__global__ void ser_lengths_kernel(const u8* __restrict__ lens, u64 n, u64* __restrict__ offs) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i <= n; i += (u64)gridDim.x * blockDim.x)
        offs[i] = i < n ? lens[i] : 0;
}
__global__ void ser_copy_kernel(const u8* __restrict__ src, u32 stride, u64 n, const u64* __restrict__ offs,
                                u8* __restrict__ dst) {
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 o = offs[i], len = offs[i + 1] - o;
        for (u64 b = 0; b < len; ++b) dst[o + b] = src[i * stride + b];
    }
}
void launch_ser_compact(hipStream_t s, const u8* lens, const u8* src, u32 stride, u64 n, u64* offs, u8* dst, u64* total) {
    u64 blocks = (n + 256) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(ser_lengths_kernel, dim3((u32)blocks), dim3(256), 0, s, lens, n, offs);
    launch_exclusive_scan(s, offs, n + 1, total);
    if (n) hipLaunchKernelGGL(ser_copy_kernel, dim3((u32)blocks), dim3(256), 0, s, src, stride, n, offs, dst);
}

// ------------------------------------------------------------------------------------------
// String MIN/MAX results (MMK_STR): the state word of a group is a reference to the winning input
// row; the result column's offsets and bytes are gathered from the retained input.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ StrRef str_ref_value(const BatchDesc* batches, int a, u64 ref) {
    return dcol_str(batches[ref_bid(ref)].args[a], ref_row(ref));
}

// totals[a] (zeroed) += payload bytes of String aggregate a over the groups of the table; groups
// without a value (STR_REF_NONE: every argument NULL) count nothing
__global__ void __launch_bounds__(BLOCK) str_agg_bytes_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                             TableDesc t, u64* totals) {
    const Spec& S = *spec;
    for (int a = 0; a < S.n_aggs; ++a) {
        const DAgg& A = S.aggs[a];
        if ((A.kind != DBG_AGG_MIN && A.kind != DBG_AGG_MAX) || A.mmk != MMK_STR) continue;  // uniform
        u64 acc = 0;
        for (u64 s = blockIdx.x * (u64)BLOCK + threadIdx.x; s <= t.cap; s += (u64)gridDim.x * BLOCK) {
            const u64* st = t.slots + s * t.stride_words;
            if (st[0] == SLOT_EMPTY) continue;
            const u64 ref = st[A.w0];
            if (ref != STR_REF_NONE) acc += str_ref_value(batches, a, ref).len;
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if ((threadIdx.x & 63) == 0 && acc) atomicAdd((unsigned long long*)(totals + a), (unsigned long long)acc);
    }
}

void launch_str_agg_bytes(hipStream_t s, const Spec* dspec, const BatchDesc* batches, const TableDesc& t, u64* totals) {
    u64 blocks = (t.cap + 1 + BLOCK - 1) / BLOCK;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(str_agg_bytes_kernel, dim3((u32)blocks), dim3(BLOCK), 0, s, dspec, batches, t, totals);
}

// offs[i] = length of group i's value (0 for STR_REF_NONE), offs[n] = 0: scanned into offsets next
__global__ void __launch_bounds__(BLOCK) str_gather_lengths_kernel(const BatchDesc* __restrict__ batches, int a,
                                                                  const u64* __restrict__ refs, u64 n, u64* __restrict__ offs) {
    for (u64 i = blockIdx.x * (u64)BLOCK + threadIdx.x; i <= n; i += (u64)gridDim.x * BLOCK) {
        u64 len = 0;
        if (i < n) {
            const u64 ref = refs[i];
            if (ref != STR_REF_NONE) len = str_ref_value(batches, a, ref).len;
        }
        offs[i] = len;
    }
}

// The bytes: STR_GATHER_LANES consecutive lanes copy one string, a byte per lane and step
// (consecutive lanes, consecutive bytes on both sides; the strings start at any address).  A value
// that would pass cap_bytes (the total dbg_agg_finalize reported) is not written.
#define STR_GATHER_LANES 16
__global__ void __launch_bounds__(BLOCK) str_gather_bytes_kernel(const BatchDesc* __restrict__ batches, int a,
                                                                const u64* __restrict__ refs, u64 n, const u64* __restrict__ offs,
                                                                u8* __restrict__ data, u64 cap_bytes) {
    const u32 sub = threadIdx.x % STR_GATHER_LANES;
    const u64 per = (u64)gridDim.x * (BLOCK / STR_GATHER_LANES);
    for (u64 i = blockIdx.x * (u64)(BLOCK / STR_GATHER_LANES) + threadIdx.x / STR_GATHER_LANES; i < n; i += per) {
        const u64 ref = refs[i];
        if (ref == STR_REF_NONE) continue;
        const StrRef r = str_ref_value(batches, a, ref);
        const u64 o = offs[i];
        if (o + r.len > cap_bytes) continue;
        for (u64 k = sub; k < r.len; k += STR_GATHER_LANES) data[o + k] = gld<u8>(r.p + k);
    }
}

void launch_str_gather(hipStream_t s, const BatchDesc* batches, int a, const u64* refs, u64 n, u64* offs, u8* data, u64 cap_bytes) {
    u64 blocks = (n + BLOCK) / BLOCK;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(str_gather_lengths_kernel, dim3((u32)blocks), dim3(BLOCK), 0, s, batches, a, refs, n, offs);
    launch_exclusive_scan(s, offs, n + 1, nullptr);
    if (!n || !cap_bytes) return;
    u64 gblocks = (n + BLOCK / STR_GATHER_LANES - 1) / (BLOCK / STR_GATHER_LANES);
    if (gblocks > 16384) gblocks = 16384;
    hipLaunchKernelGGL(str_gather_bytes_kernel, dim3((u32)gblocks), dim3(BLOCK), 0, s, batches, a, refs, n, offs, data, cap_bytes);
}
