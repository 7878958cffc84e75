// agg_fin_small.hpp — the finalize of a small table in one workgroup (finalize_small_body) and the
// result helpers it writes with: shared by the stand-alone finalize_small_kernel
// (agg_finalize.hip), the fused finalize of agg_insert_fast_kernel (agg.hip)
// and, for part_of and the key lengths, the export kernels (agg_export.hip).  Included after
// agg_table.hpp.  File map: agg_table.hpp.
#pragma once

// scheme 2: the slot's legacy bucket, computed beforehand by legacy_slot_bucket_kernel
__device__ __forceinline__ u32 part_of(u64 h, u32 n_parts, int scheme, const u32* lpart, u64 s) {
    if (n_parts <= 1) return 0;
    if (scheme == 2) return lpart[s];
    if (scheme == 0) return (u32)(h % n_parts);  // Payload::scatter: hash % n (payload.rs:383)
    u32 rb = 31 - __clz(n_parts);                // radix bits [48 - r, 48) (partitioned_payload.rs:121)
    return (u32)((h >> (48 - rb)) & (n_parts - 1));
}

__device__ __forceinline__ u64 key_str_len(const Spec& S, const BatchDesc* batches, u64 e, int c) {
    StrRef r = dcol_str(batches[ref_bid(e)].keys[c], ref_row(e));
    return r.len;
}
// The same from slot s's key cache when it holds the key (published header, length <= 32): no
// read of the representative row.
__device__ __forceinline__ u64 slot_str_len(const Spec& S, const BatchDesc* batches, const TableDesc& t, u64 s, u64 e, int c) {
    if (S.kc_word && s < t.cap) {
        const u64 hv = t.slots[s * t.stride_words + S.kc_word];
        if ((hv & 1) && ((hv >> 1) & 0x7FFF) <= 8 * KC_KEY_WORDS) return (hv >> 1) & 0x7FFF;
    }
    return key_str_len(S, batches, e, c);
}

#define MAX_PARTS_LDS 256

// flush_column of one group (slot s, entry e, state words st) into output row p; sp[c] = string
// write cursor of key column c (advanced).
template <bool W256 = true>  // see write_agg
__device__ __forceinline__ void write_group(const Spec& S, const BatchDesc* batches, const TableDesc& t, u64 s, const u64* st,
                                           u64 e, u64 p, u64* sp, const OutDesc& out) {
    // group columns
    if (S.inline_keys) {
        u64 key = s == t.cap ? SLOT_EMPTY : e;
        for (int c = 0; c < S.n_keys; ++c) {
            const dbg_datatype& ty = S.key_types[c];
            u32 w = type_width(ty.type);
            u64 b = (key >> (8 * S.koff[c])) & width_mask(w);
            bool v = ty.nullable ? ((key >> (8 * S.voff[c])) & 0xff) != 0 : true;
            write_bytes(out.key_data[c], p, w, b, 0);
            if (out.key_valid[c]) out.key_valid[c][p] = v ? 1 : 0;
        }
    } else if (S.kc_word && s < t.cap && (st[S.kc_word] & 1) && ((st[S.kc_word] >> 1) & 0x7FFF) <= 8 * KC_KEY_WORDS) {
        // one String key held by the slot's key cache: no read of the representative row
        const u32 len = (u32)((st[S.kc_word] >> 1) & 0x7FFF);
        u64 w[KC_KEY_WORDS];
#pragma unroll
        for (int j = 0; j < KC_KEY_WORDS; ++j) w[j] = st[S.kc_word + 1 + j];
        out.key_offsets[0][p] = sp[0];
        if (out.key_valid[0]) out.key_valid[0][p] = 1;
        if (sp[0] + len <= out.cap_str[0]) {
            u8* d = (u8*)out.key_data[0] + sp[0];
#pragma unroll
            for (u32 j = 0; j < 8 * KC_KEY_WORDS; ++j)
                if (j < len) d[j] = (u8)(w[j >> 3] >> (8 * (j & 7)));
        }
        sp[0] += len;
    } else {
        const BatchDesc& RB = batches[ref_bid(e)];
        u64 row = ref_row(e);
        for (int c = 0; c < S.n_keys; ++c) {
            const DCol& kc = RB.keys[c];
            bool v = dcol_valid(kc, row);
            if (out.key_valid[c]) out.key_valid[c][p] = v ? 1 : 0;
            if (kc.type == DBG_STRING) {
                StrRef r = dcol_str(kc, row);
                out.key_offsets[c][p] = sp[c];
                if (sp[c] + r.len <= out.cap_str[c]) {
                    u8* d = (u8*)out.key_data[c] + sp[c];
                    for (u64 j = 0; j < r.len; ++j) d[j] = r.p[j];
                }
                sp[c] += r.len;
            } else {
                write_key_cell(out.key_data[c], p, kc, row);
            }
        }
    }
    for (int a = 0; a < S.n_aggs; ++a) write_agg<W256>(S, a, st, p, out, t.counters + CNT_ERR);
}

// ------------------------------------------------------------------------------------------
// finalize_small: count + scan + write + validity bits + string offsets in ONE workgroup, for
// tables of at most FIN_SMALL_SLOTS slots (low-cardinality queries: the four-launch finalize
// costs more than the work).  totals: [0] groups, [1 + c] string bytes of key column c.
//
// Each thread owns FIN_MAXPER consecutive slots whose entries it loads once, all in flight
// together, and keeps in registers for the write pass.  recycle != 0 (dbg_agg_set_recycle):
// the table is left re-initialised for the next batch (this kernel already holds every slot, so
// the reset costs no extra launch), unless an insert overflowed (the host then grows the table
// and finalizes again).  host_mirror (mapped pinned memory) receives the counters, the totals and
// finally `seq`, which the host polls instead of synchronising the stream.
// ------------------------------------------------------------------------------------------
#define FIN_NT 1024
#define FIN_MAXPER (FIN_SMALL_SLOTS / FIN_NT)
// The body, run by FIN_NT threads of one workgroup: the standalone kernel below, or the last
// workgroup of a fused insert (agg_insert_fast with FusedFin::on).  `view` holds the slots to
// read (t.slots, or a copy in LDS); the re-initialisation of a recycled table writes t.slots.
template <int MAXPER, bool W256 = true>
__device__ __forceinline__ bool finalize_small_body(const Spec& S, const BatchDesc* batches, const TableDesc& t, const u64* view,
                                                    const OutDesc& out, u64* totals, u64* host_mirror, int recycle, u64 seq,
                                                    u64* trace = nullptr, bool writeback = false, int xfin = 0) {
    __shared__ u64 wsum[FIN_NT / 64][1 + DBG_MAX_KEYS];
    __shared__ u64 cnts[CNT_WORDS];
    auto mark = [&](int k) { if (kPhaseTrace && trace && threadIdx.x == 0) trace[k] = __builtin_amdgcn_s_memrealtime(); };
    // Barriers here are LDS-only (no wait for this workgroup's global stores) unless a later
    // phase reads what other threads stored to global memory: every __syncthreads costs a
    // store round trip (vmcnt 0, ~1 us).
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    const u64 n_slots = t.cap + 1;
    const u32 per = (u32)((n_slots + FIN_NT - 1) / FIN_NT);  // <= MAXPER (host checks cap)
    const u64 base = (u64)threadIdx.x * per;
    const bool ref_strings = S.has_strings && !S.inline_keys;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool has_bits = false, dec_err = false;  // uniform
    for (int c = 0; c < S.n_keys; ++c) has_bits |= out.key_valid[c] && out.key_bits[c];
    for (int a = 0; a < S.n_aggs; ++a) {
        has_bits |= (out.agg_valid[a] || ((out.all_valid >> a) & 1)) && out.agg_bits[a];
        dec_err |= S.aggs[a].dec_check || (S.aggs[a].kind == DBG_AGG_AVG && S.aggs[a].sumk >= SUMK_I128);
    }
    // the table counters, in flight while the table is scanned (final: every inserting workgroup
    // has finished; write_group may still set decimal-overflow bits, reloaded below)
    u64 myc = threadIdx.x < CNT_WORDS ? ld_sc1(t.counters + threadIdx.x) : 0;
    u64 ent[MAXPER];
#pragma unroll
    for (u32 k = 0; k < MAXPER; ++k) {
        u64 s = base + k;
        ent[k] = (k < per && s < n_slots) ? view[s * t.stride_words] : SLOT_EMPTY;
    }
    u64 cnt = 0, sb[DBG_MAX_KEYS];
    u32 occ = 0;  // occupied owned slots (bit k = slot base + k)
    for (int c = 0; c < DBG_MAX_KEYS; ++c) sb[c] = 0;
#pragma unroll
    for (u32 k = 0; k < MAXPER; ++k) {
        if (ent[k] == SLOT_EMPTY) continue;
        cnt++;
        occ |= 1u << k;
        if (ref_strings)
            for (int c = 0; c < S.n_keys; ++c)
                if (S.key_types[c].type == DBG_STRING) sb[c] += key_str_len(S, batches, ent[k], c);
    }
    // block exclusive scan of cnt (and of the string bytes of each key column)
    auto wave_incl = [&](u64 v) {
        for (int off = 1; off < 64; off <<= 1) {
            u64 o = __shfl_up(v, off, 64);
            if (lane >= off) v += o;
        }
        return v;
    };
    u64 ic = wave_incl(cnt);
    u64 isb[DBG_MAX_KEYS];
    if (ref_strings)
        for (int c = 0; c < S.n_keys; ++c) isb[c] = wave_incl(sb[c]);
    if (lane == 63) {
        wsum[wave][0] = ic;
        if (ref_strings)
            for (int c = 0; c < S.n_keys; ++c) wsum[wave][1 + c] = isb[c];
    }
    lds_barrier();
    u64 p = ic - cnt, sp[DBG_MAX_KEYS];
    for (int w = 0; w < wave; ++w) p += wsum[w][0];
    if (ref_strings)
        for (int c = 0; c < S.n_keys; ++c) {
            sp[c] = isb[c] - sb[c];
            for (int w = 0; w < wave; ++w) sp[c] += wsum[w][1 + c];
        }
    u64 total = 0, stot[DBG_MAX_KEYS];
    for (int w = 0; w < FIN_NT / 64; ++w) total += wsum[w][0];
    for (int c = 0; c < S.n_keys; ++c) {
        stot[c] = 0;
        if (ref_strings)
            for (int w = 0; w < FIN_NT / 64; ++w) stot[c] += wsum[w][1 + c];
    }
    mark(7);
    // write pass over the occupied slots only (one write_group instance in the code; the entry
    // is re-read from the cache rather than indexed out of the register array)
    const u32 occ_all = occ;
    if (kExperiments && (xfin & 1)) occ = 0;  // timing ablation (EXP=1 builds only)
    while (occ && p < out.cap_groups) {
        const u32 k = __builtin_ctz(occ);
        occ &= occ - 1;
        const u64 s = base + k;
        const u64* st = view + s * t.stride_words;
        write_group<W256>(S, batches, t, s, st, st[0], p, sp, out);
        p++;
    }
    mark(8);
    u64 n = total < out.cap_groups ? total : out.cap_groups;
    if (has_bits && !(kExperiments && (xfin & 2))) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // validity bytes of every row are in global memory
        const u32 ncols = (u32)(S.n_keys + S.n_aggs);
        for (u64 f = threadIdx.x; f < (n + 7) / 8 * ncols; f += FIN_NT) {  // one (byte, column) per thread
            const u64 k = f / ncols;
            const int c = (int)(f % ncols);
            {
                const u8* bytes = c < S.n_keys ? out.key_valid[c] : out.agg_valid[c - S.n_keys];
                u8* bits = c < S.n_keys ? out.key_bits[c] : out.agg_bits[c - S.n_keys];
                if (!bytes && bits && c >= S.n_keys && ((out.all_valid >> (c - S.n_keys)) & 1)) {
                    bits[k] = all_valid_byte(n, k);
                    continue;
                }
                if (!bytes || !bits) continue;
                u8 b = 0;
                for (int j = 0; j < 8; ++j) {
                    u64 i = k * 8 + j;
                    if (i < n && bytes[i]) b |= (u8)(1u << j);
                }
                bits[k] = b;
            }
        }
    }
    if (threadIdx.x == 0) {
        totals[0] = total;
        for (int c = 0; c < S.n_keys; ++c) {
            totals[1 + c] = stot[c];
            if (out.key_offsets[c] && total <= out.cap_groups) out.key_offsets[c][total] = stot[c];
        }
    }
    if (dec_err) {
        __syncthreads();  // decimal-overflow bits of write_group are in the counters
        if (threadIdx.x == CNT_ERR) myc = ld_sc1(t.counters + CNT_ERR);
    }
    if (threadIdx.x < CNT_WORDS) cnts[threadIdx.x] = myc;
    lds_barrier();
    mark(9);
    // recycle only when the caller got every group (short buffers: the table must stay intact
    // for the retry with larger ones) and no insert overflowed (the host grows and finalizes again)
    bool rc = recycle && cnts[CNT_OVF_ROWS] == 0 && cnts[CNT_OVF_RECS] == 0 && total <= out.cap_groups;
    for (int c = 0; c < S.n_keys; ++c)
        if (ref_strings && S.key_types[c].type == DBG_STRING && stot[c] > out.cap_str[c]) rc = false;
    if (rc && threadIdx.x < CNT_WORDS) t.counters[threadIdx.x] = 0;  // dbg_agg_reset
    // zero-copy read-back: the table counters and the totals go straight to mapped pinned host
    // memory ([0, CNT_WORDS) counters, then totals), so finalize needs no copy launches
    // (system-scope stores: written through to host memory, never parked in the L2)
    auto put = [&](int w, u64 v) { __hip_atomic_store(host_mirror + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    if (threadIdx.x == 0) {
        if (host_mirror) {
            for (int w = 0; w < CNT_WORDS; ++w) put(w, cnts[w]);
            put(CNT_WORDS, total);
            for (int c = 0; c < S.n_keys; ++c) put(CNT_WORDS + 1 + c, stot[c]);
            put(CNT_WORDS + 1 + DBG_MAX_KEYS, rc ? 1 : 0);  // recycled
        }
    }
    mark(10);
    if (!rc && writeback)  // `view` is an LDS table the HBM table does not hold yet
        for (u64 i = threadIdx.x; i < n_slots * t.stride_words; i += FIN_NT) t.slots[i] = view[i];
    if (rc) {  // table_init of the owned slots that were claimed (an EMPTY slot is still in its
               // initial state: state words are only written after the entry is claimed)
        const u32 sw = (u32)t.stride_words;
        u32 o = occ_all;
        while (o) {
            const u32 k = __builtin_ctz(o);
            o &= o - 1;
            u64* d = t.slots + (base + k) * sw;
            for (u32 w = 0; w < sw; ++w) d[w] = S.slot_init[w];
        }
    }
    // `seq` last: thread 0 waits for its write-through mirror stores to complete before posting it.  No system-scope release: that would write
    // back the whole L2; the output columns are consumed in stream order on the device.
    if (host_mirror && threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(host_mirror + CNT_WORDS + 2 + DBG_MAX_KEYS, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return rc;
}
