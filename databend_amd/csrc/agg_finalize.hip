// agg_finalize.hip — the table's groups into result columns: count / slot buckets / scan / write
// (merge_result + flush_column), the one-workgroup finalize_small, and the validity bit-packing
// of the outputs.  File map: agg_table.hpp.
#include "agg_table.hpp"
#include "agg_fin_small.hpp"

// ------------------------------------------------------------------------------------------
// Finalize / partition: per-block histograms over slot ranges.
// ------------------------------------------------------------------------------------------
u64 finalize_blocks(u64 cap) { return (cap + 1 + SLOTS_PER_BLOCK - 1) / SLOTS_PER_BLOCK; }

__global__ void __launch_bounds__(BLOCK) count_groups_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                            TableDesc t, u32 n_parts, int scheme, const u32* __restrict__ lpart,
                                                            u64* hist, u64* str_hist, u64 nblocks) {
    const Spec& S = *spec;
    __shared__ unsigned long long lh[MAX_PARTS_LDS];
    __shared__ unsigned long long ls[DBG_MAX_KEYS][MAX_PARTS_LDS];
    for (u32 p = threadIdx.x; p < n_parts; p += BLOCK) lh[p] = 0;
    if (S.has_strings && !S.inline_keys)
        for (u32 p = threadIdx.x; p < (u32)S.n_keys * MAX_PARTS_LDS; p += BLOCK) ls[p / MAX_PARTS_LDS][p % MAX_PARTS_LDS] = 0;
    __syncthreads();
    u64 base = (u64)blockIdx.x * SLOTS_PER_BLOCK;
    u32 mine = 0;  // n_parts == 1: count in registers, reduce once (no LDS atomics on one word)
    for (u32 k = threadIdx.x; k < SLOTS_PER_BLOCK; k += BLOCK) {
        u64 s = base + k;
        if (s > t.cap) break;
        u64 e = t.slots[s * t.stride_words];
        if (e == SLOT_EMPTY) continue;
        u32 p = 0;
        if (n_parts > 1) {
            p = part_of(scheme == 2 ? 0 : entry_hash(S, batches, e, s == t.cap), n_parts, scheme, lpart, s);
            atomicAdd(&lh[p], 1ULL);
        } else {
            mine++;
        }
        if (S.has_strings && !S.inline_keys)
            for (int c = 0; c < S.n_keys; ++c)
                if (S.key_types[c].type == DBG_STRING) atomicAdd(&ls[c][p], (unsigned long long)slot_str_len(S, batches, t, s, e, c));
    }
    if (n_parts == 1) {
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&lh[0], (unsigned long long)mine);
    }
    __syncthreads();
    for (u32 p = threadIdx.x; p < n_parts; p += BLOCK) {
        hist[(u64)p * nblocks + blockIdx.x] = lh[p];
        if (S.has_strings && !S.inline_keys)
            for (int c = 0; c < S.n_keys; ++c)
                if (S.key_types[c].type == DBG_STRING) str_hist[((u64)p * S.n_keys + c) * nblocks + blockIdx.x] = ls[c][p];
    }
}

void launch_count_groups(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, const TableDesc& t, u32 n_parts,
                         int scheme, const u32* lpart, u64* hist, u64* str_hist) {
    u64 nb = finalize_blocks(t.cap);
    hipLaunchKernelGGL(count_groups_kernel, dim3((u32)nb), dim3(BLOCK), 0, s, dspec, batches, t, n_parts, scheme, lpart, hist, str_hist, nb);
}

// Legacy bucket of every occupied slot (enable_experimental_aggregate_hashtable = 0): the
// FastHash of the group's FixedKeys / SingleBinary key (legacy.hpp), hash2bucket<bits, true>.
__global__ void __launch_bounds__(BLOCK) legacy_slot_bucket_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                                  TableDesc t, LegacyLayout L, u32* __restrict__ out) {
    const Spec& S = *spec;
    __shared__ u32 tab[256];
    crc_table_init(tab);
    for (u64 s = blockIdx.x * (u64)BLOCK + threadIdx.x; s <= t.cap; s += (u64)gridDim.x * BLOCK) {
        const u64 e = t.slots[s * t.stride_words];
        if (e == SLOT_EMPTY) continue;
        u64 h;
        if (L.binary) {
            const StrRef sr = dcol_str(batches[ref_bid(e)].keys[0], ref_row(e));
            h = legacy_bytes_hash(tab, sr.p, sr.len);
        } else if (L.serializer) {
            SerCrc sc;
            const u64 key = s == t.cap ? SLOT_EMPTY : e;
            for (int c = 0; c < S.n_keys; ++c) {
                const dbg_datatype& ty = S.key_types[c];
                bool v;
                u64 lo = 0, hi = 0;
                StrRef sr{nullptr, 0};
                if (S.inline_keys) {
                    v = !ty.nullable || ((key >> (8 * S.voff[c])) & 0xff) != 0;
                    lo = (key >> (8 * S.koff[c])) & width_mask(type_width(ty.type));
                } else {
                    const DCol& kc = batches[ref_bid(e)].keys[c];
                    const u64 row = ref_row(e);
                    v = dcol_valid(kc, row);
                    if (v && ty.type == DBG_STRING) sr = dcol_str(kc, row);
                    else if (v) {
                        lo = dcol_bits(kc, row);
                        if (ty.type == DBG_DECIMAL128) hi = dcol_hi(kc, row);
                    }
                }
                sc.column(tab, ty.type, ty.nullable, v, lo, hi, sr.p, sr.len);
            }
            h = sc.finish(tab);
        } else {
            u64 k[4] = {0, 0, 0, 0};
            const u64 key = s == t.cap ? SLOT_EMPTY : e;
            for (int c = 0; c < S.n_keys; ++c) {
                const dbg_datatype& ty = S.key_types[c];
                const u32 w = type_width(ty.type);
                bool v;
                u64 lo, hi = 0;
                if (S.inline_keys) {
                    v = !ty.nullable || ((key >> (8 * S.voff[c])) & 0xff) != 0;
                    lo = (key >> (8 * S.koff[c])) & width_mask(w);
                } else {
                    const DCol& kc = batches[ref_bid(e)].keys[c];
                    const u64 row = ref_row(e);
                    v = dcol_valid(kc, row);
                    lo = dcol_bits(kc, row);
                    if (w == 16) hi = dcol_hi(kc, row);
                }
                if (!v) {  // null byte 1, value bytes 0
                    const u32 o = (u32)L.null_off[c];
                    k[o >> 3] |= 1ULL << (8 * (o & 7));
                } else {
                    legacy_put(k, L.off[c], lo, hi, w);
                }
            }
            h = legacy_fixed_crc(tab, k, L.words);
        }
        out[s] = legacy_bucket(h, L.bits);
    }
}

// Bucket (scheme 0 or 1) of every occupied slot by the group hash of its first `nk` key columns: a
// DISTINCT aggregate's pair table (keys..., x) is bucketed by its group's keys alone, so each of
// its buckets holds exactly the pairs of the groups the same bucket of the main table holds
// (AggregateDistinctCombinator's set travels inside its group's state in the reference,
// FUN/aggregate_combinator_distinct.rs:94-105).
__global__ void __launch_bounds__(BLOCK) prefix_slot_bucket_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                                  TableDesc t, int nk, u32 n_parts, int scheme, u32* __restrict__ out) {
    const Spec& S = *spec;
    for (u64 s = blockIdx.x * (u64)BLOCK + threadIdx.x; s <= t.cap; s += (u64)gridDim.x * BLOCK) {
        const u64 e = t.slots[s * t.stride_words];
        if (e == SLOT_EMPTY) continue;
        const u64 h = S.inline_keys ? hash_packed(S, s == t.cap ? SLOT_EMPTY : e, nk) : group_hash(batches[ref_bid(e)].keys, nk, ref_row(e));
        out[s] = part_of(h, n_parts, scheme, nullptr, s);
    }
}

void launch_prefix_slot_bucket(hipStream_t s, const Spec* dspec, const BatchDesc* batches, const TableDesc& t, int nk, u32 n_parts,
                               int scheme, u32* out) {
    u64 blocks = (t.cap + 1 + BLOCK - 1) / BLOCK;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(prefix_slot_bucket_kernel, dim3((u32)blocks), dim3(BLOCK), 0, s, dspec, batches, t, nk, n_parts, scheme, out);
}

void launch_legacy_slot_bucket(hipStream_t s, const Spec* dspec, const BatchDesc* batches, const TableDesc& t, const LegacyLayout& L,
                               u32* out) {
    u64 blocks = (t.cap + 1 + BLOCK - 1) / BLOCK;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(legacy_slot_bucket_kernel, dim3((u32)blocks), dim3(BLOCK), 0, s, dspec, batches, t, L, out);
}

// Single-workgroup exclusive scan (in place) over n u64; *total = sum.
__global__ void __launch_bounds__(1024) exclusive_scan_kernel(u64* data, u64 n, u64* total) {
    __shared__ u64 sums[1024];
    u64 per = (n + 1023) / 1024;
    u64 a = threadIdx.x * per, b = a + per < n ? a + per : n;
    u64 acc = 0;
    for (u64 k = a; k < b; ++k) acc += data[k];
    sums[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        u64 v = threadIdx.x >= (u32)off ? sums[threadIdx.x - off] : 0;
        __syncthreads();
        sums[threadIdx.x] += v;
        __syncthreads();
    }
    u64 run = threadIdx.x ? sums[threadIdx.x - 1] : 0;
    for (u64 k = a; k < b; ++k) {
        u64 v = data[k];
        data[k] = run;
        run += v;
    }
    if (threadIdx.x == 1023 && total) *total = sums[1023];
}

void launch_exclusive_scan(hipStream_t s, u64* data, u64 n, u64* total) {
    hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, s, data, n, total);
}

// ------------------------------------------------------------------------------------------
// Results (merge_result + flush_column): deterministic order inside a workgroup via block scan.
// ------------------------------------------------------------------------------------------
// Slot order within the block: iteration k covers slots base + k*BLOCK + tid (coalesced entry
// reads); positions come from a block-wide exclusive scan per iteration (wave shuffles + one
// LDS exchange), with running totals carried across iterations.  Same per-block ownership of
// slots as count_groups, so the scanned block offsets line up.
__global__ void __launch_bounds__(BLOCK) write_results_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                             TableDesc t, const u64* pos, const u64* str_pos, u64 nblocks,
                                                             OutDesc out) {
    const Spec& S = *spec;
    // double-buffered per-wave sums: iteration k writes buffer k & 1, so one barrier per iteration
    // orders both its reads and the next iteration's writes
    __shared__ u64 wsum2[2][BLOCK / 64][1 + DBG_MAX_KEYS];
    const bool ref_strings = S.has_strings && !S.inline_keys;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64 base = (u64)blockIdx.x * SLOTS_PER_BLOCK;
    u64 run = pos[blockIdx.x];
    u64 srun[DBG_MAX_KEYS];
    if (ref_strings)
        for (int c = 0; c < S.n_keys; ++c)
            srun[c] = S.key_types[c].type == DBG_STRING ? str_pos[(u64)c * nblocks + blockIdx.x] : 0;
    auto wave_incl = [&](u64 v) {
        for (int off = 1; off < 64; off <<= 1) {
            u64 o = __shfl_up(v, off, 64);
            if (lane >= off) v += o;
        }
        return v;
    };
    // the next iteration's entry is loaded before this iteration's barrier
    auto entry_at = [&](u32 k) -> u64 {
        const u64 s = base + (u64)k * BLOCK + threadIdx.x;
        return s <= t.cap ? t.slots[s * t.stride_words] : SLOT_EMPTY;
    };
    u64 e_next = entry_at(0);
    for (u32 k = 0; k < SLOTS_PER_THREAD; ++k) {
        if (base + (u64)k * BLOCK > t.cap) break;  // uniform
        u64 (*wsum)[1 + DBG_MAX_KEYS] = wsum2[k & 1];
        const u64 s = base + (u64)k * BLOCK + threadIdx.x;
        const bool in = s <= t.cap;
        const u64* st = t.slots + (in ? s : 0) * t.stride_words;
        const u64 e = e_next;
        if (k + 1 < SLOTS_PER_THREAD) e_next = entry_at(k + 1);
        const u64 cnt = e != SLOT_EMPTY ? 1 : 0;
        u64 sb[DBG_MAX_KEYS];
        // inclusive count within the wave from one ballot (cnt is 0 / 1)
        const u64 ic = (u64)__popcll(__ballot(cnt != 0) & (lane == 63 ? ~0ULL : ((2ULL << lane) - 1)));
        if (lane == 63) wsum[wave][0] = ic;
        if (ref_strings)
            for (int c = 0; c < S.n_keys; ++c) {
                sb[c] = (cnt && S.key_types[c].type == DBG_STRING) ? slot_str_len(S, batches, t, s, e, c) : 0;
                u64 is = wave_incl(sb[c]);
                if (lane == 63) wsum[wave][1 + c] = is;
                sb[c] = is - sb[c];  // exclusive within the wave
            }
        __syncthreads();
        u64 p = run + ic - cnt, tot = 0;
        for (int w = 0; w < BLOCK / 64; ++w) {
            if (w < wave) p += wsum[w][0];
            tot += wsum[w][0];
        }
        u64 sp[DBG_MAX_KEYS];
        if (ref_strings)
            for (int c = 0; c < S.n_keys; ++c) {
                sp[c] = srun[c] + sb[c];
                u64 stot = 0;
                for (int w = 0; w < BLOCK / 64; ++w) {
                    if (w < wave) sp[c] += wsum[w][1 + c];
                    stot += wsum[w][1 + c];
                }
                srun[c] += stot;
            }
        run += tot;
        if (cnt && p < out.cap_groups) write_group(S, batches, t, s, st, e, p, sp, out);
    }
}

__global__ void __launch_bounds__(FIN_NT) finalize_small_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                                TableDesc t, OutDesc out, u64* totals, u64* host_mirror,
                                                                int recycle, u64 seq, int xfin) {
    if (kExperiments && (xfin & 8)) return;  // timing ablation (EXP=1 builds only)
    finalize_small_body<FIN_MAXPER>(*spec, batches, t, t.slots, out, totals, host_mirror, recycle, seq, nullptr, false, xfin);
}

void launch_finalize_small(hipStream_t s, const Spec* dspec, const BatchDesc* batches, const TableDesc& t, const OutDesc& out,
                           u64* totals, u64* host_mirror, int recycle, u64 seq) {
    static const int xfin = X_ENV("DBG_X_FIN") ? atoi(X_ENV("DBG_X_FIN")) : 0;
    hipLaunchKernelGGL(finalize_small_kernel, dim3(1), dim3(FIN_NT), 0, s, dspec, batches, t, out, totals, host_mirror, recycle,
                       seq, xfin);
}

// Fused finalize tail: bit-pack every nullable output's validity and close the string offsets,
// with the group count read from device memory (totals[0]; totals[1 + c] string bytes).
// 8 flag bytes (any nonzero = set) -> 8 bits, LSB first
__device__ __forceinline__ u32 pack8(u64 x) {
    const u64 hi = 0x8080808080808080ULL, lo7 = 0x7F7F7F7F7F7F7F7FULL;
    const u64 nz = (((x & lo7) + lo7) | x) & hi;  // bit 7 of every nonzero byte
    return (u32)(((nz >> 7) * 0x0102040810204080ULL) >> 56);
}

// bytes [8k, 8k + 8) -> bits byte k: one 8-byte load per lane (consecutive lanes, consecutive
// words) where whole and aligned
__device__ __forceinline__ void pack_bits_at(const u8* __restrict__ bytes, u64 n, u8* __restrict__ bits, u64 k) {
    const u64 i0 = k * 8;
    if (i0 >= n) return;
    u32 b = 0;
    if (i0 + 8 <= n && !((uintptr_t)(bytes + i0) & 7)) {
        b = pack8(*(const u64*)(bytes + i0));
    } else {
        for (u64 i = i0; i < n && i < i0 + 8; ++i)
            if (bytes[i]) b |= 1u << (i - i0);
    }
    bits[k] = (u8)b;
}

// Validity bitmaps of the result columns: flag bytes packed 64 at a time into one u64 of bits
// (eight 8-byte loads, one 8-byte store), all-valid columns filled a word at a time; the bytes
// past the last whole word, and bitmaps not 8-byte aligned, byte by byte.  (One byte per thread
// and column was 0.87 ms for C4's 1e9 groups: instruction-bound, SQ_INSTS_VALU.)
__global__ void finish_outputs_kernel(OutDesc out, const u64* totals, int n_keys, int n_aggs) {
    u64 n = totals[0];
    if (n > out.cap_groups) n = out.cap_groups;
    const u64 nb = (n + 7) / 8, nw = (n / 8) / 8;  // bitmap bytes; whole u64 words of whole bytes
    const u64 tid = blockIdx.x * (u64)blockDim.x + threadIdx.x, stride = (u64)gridDim.x * blockDim.x;
    for (int c = 0; c < n_keys + n_aggs; ++c) {
        const u8* bytes = c < n_keys ? out.key_valid[c] : out.agg_valid[c - n_keys];
        u8* bits = c < n_keys ? out.key_bits[c] : out.agg_bits[c - n_keys];
        const bool fill = !bytes && bits && c >= n_keys && ((out.all_valid >> (c - n_keys)) & 1);
        if (!bits || (!bytes && !fill)) continue;
        const bool wide = !((uintptr_t)bits & 7) && (fill || !((uintptr_t)bytes & 7));
        const u64 w_end = wide ? nw : 0;
        for (u64 w = tid; w < w_end; w += stride) {
            u64 v = ~0ULL;
            if (!fill) {
                const u64* src = (const u64*)(bytes + w * 64);
                v = 0;
#pragma unroll
                for (int j = 0; j < 8; ++j) v |= (u64)pack8(src[j]) << (8 * j);
            }
            ((u64*)bits)[w] = v;
        }
        for (u64 k = w_end * 8 + tid; k < nb; k += stride) {
            if (fill) bits[k] = all_valid_byte(n, k);
            else pack_bits_at(bytes, n, bits, k);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int c = 0; c < n_keys; ++c)
            if (out.key_offsets[c] && totals[0] <= out.cap_groups) out.key_offsets[c][n] = totals[1 + c];
}

void launch_finish_outputs(hipStream_t s, const OutDesc& out, const u64* totals, int n_keys, int n_aggs) {
    u64 nb = (out.cap_groups + 7) / 8;
    u64 blocks = (nb + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(finish_outputs_kernel, dim3((u32)blocks), dim3(256), 0, s, out, totals, n_keys, n_aggs);
}

void launch_write_results(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, const TableDesc& t,
                          const u64* pos, const u64* str_pos, const OutDesc& out) {
    u64 nb = finalize_blocks(t.cap);
    hipLaunchKernelGGL(write_results_kernel, dim3((u32)nb), dim3(BLOCK), 0, s, dspec, batches, t, pos, str_pos, nb, out);
}

__global__ void pack_bits_kernel(const u8* bytes, u64 n, u8* bits) {
    const u64 nb = (n + 7) / 8;
    for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < nb; k += (u64)gridDim.x * blockDim.x) pack_bits_at(bytes, n, bits, k);
}

__global__ void fill_valid_kernel(u64 n, u8* bits) {
    const u64 nb = (n + 7) / 8;
    for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < nb; k += (u64)gridDim.x * blockDim.x) bits[k] = all_valid_byte(n, k);
}

void launch_fill_valid(hipStream_t s, u64 n, u8* bits) {
    const u64 nb = (n + 7) / 8;
    u64 blocks = (nb + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (!blocks) return;
    hipLaunchKernelGGL(fill_valid_kernel, dim3((u32)blocks), dim3(256), 0, s, n, bits);
}

void launch_pack_bits(hipStream_t s, const u8* bytes, u64 n, u8* bits) {
    u64 nb = (n + 7) / 8;
    u64 blocks = (nb + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (!blocks) return;
    hipLaunchKernelGGL(pack_bits_kernel, dim3((u32)blocks), dim3(256), 0, s, bytes, n, bits);
}
