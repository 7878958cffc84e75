// agg_table.hpp — the table layer of the hash GROUP BY path: the constants, key packing, probing
// of the HBM and LDS tables, the overflow lists and the end-of-launch flush.  agg.hip uses all of
// it, the other two units the constants and the key hashing.  Included only by these units
// (pp.hip and part.hip have BLOCK-like names of their own):
//
//   agg.hip          : the insert side: table_init, agg_insert and its specialised families
//                      (str1, short, fast), each with its eligibility and launch, agg_retry,
//                      agg_rehash, launch_insert; agg_chain.hpp holds the hand-offs by which the
//                      fast kernel's last workgroup finalizes the table in the same launch
//   agg_finalize.hip : count / write (merge_result + flush_column into output columns,
//                      EAGG/aggregate_hashtable.rs:427-451, payload_flush.rs), finalize_small,
//                      validity bit-packing; agg_fin_small.hpp is the body finalize_small shares
//                      with the fused finalize of agg.hip
//   agg_export.hip   : partial-state records partitioned by hash % n or radix bits (Payload::scatter,
//                      payload.rs:356-391; PartitionedPayload, partitioned_payload.rs), the
//                      serialized-state compaction and the String MIN/MAX result gather
//
// Bandwidth/atomic-bound integer work: no MFMA.  Every kernel is grid-strided over >= 2048
// workgroups of 256 threads (64-wide waves) or over contiguous row ranges per workgroup.
#pragma once
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>

#include "legacy.hpp"
#include "agg.hpp"
#include <hip/hip_ext.h>
#include "agg_dev.hpp"

#define BLOCK 256
#define SLOTS_PER_THREAD 8
#define SLOTS_PER_BLOCK (BLOCK * SLOTS_PER_THREAD)
#define LDS_BUDGET_BYTES (32 * 1024)
#define LDS_PROBE_CAP 64
#define FLUSH_ROUND 16  // rounds of BLOCK rows between checks for a full LDS table

// slot_mix (inline-key slot placement) lives in agg.hpp

// ------------------------------------------------------------------------------------------
// Key packing (inline mode): the row format of EAGG/payload.rs:100-129 in <= 8 bytes.
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ u64 pack_key(const Spec& S, const DCol* keys, u64 i) {
    u64 k = 0;
    for (int c = 0; c < S.n_keys; ++c) {
        const DCol& col = keys[c];
        bool v = dcol_valid(col, i);
        if (col.nullable) k |= (u64)(v ? 1 : 0) << (8 * S.voff[c]);
        if (v) {
            u64 b = dcol_bits(col, i);
            if (col.type == DBG_FLOAT32 || col.type == DBG_FLOAT64) b = canon_float_bits(col.type, b);
            k |= (b & width_mask(type_width(col.type))) << (8 * S.koff[c]);
        }
    }
    return k;
}


__device__ __forceinline__ u64 hash_packed(const Spec& S, u64 key, int nk = -1) {
    u64 h = 0;
    if (nk < 0) nk = S.n_keys;
    for (int c = 0; c < nk; ++c) {
        const dbg_datatype& t = S.key_types[c];
        bool v = t.nullable ? ((key >> (8 * S.voff[c])) & 0xff) != 0 : true;
        u64 b = (key >> (8 * S.koff[c])) & width_mask(type_width(t.type));
        u64 x = v ? hash_bits(t.type, b) : NULL_HASH_VAL;
        h = c == 0 ? x : (h * NULL_HASH_VAL) ^ x;
    }
    return h;
}


__device__ __forceinline__ bool ref_equal(const Spec& S, const BatchDesc* batches, const DCol* keys, u64 i, u64 e) {
    const DCol* other = batches[ref_bid(e)].keys;
    u64 j = ref_row(e);
    for (int c = 0; c < S.n_keys; ++c)
        if (!cell_equal(keys[c], i, other[c], j)) return false;
    return true;
}


// Reference group hash of the group an entry stands for.
__device__ __forceinline__ u64 entry_hash(const Spec& S, const BatchDesc* batches, u64 e, bool is_sentinel) {
    if (S.inline_keys) return hash_packed(S, is_sentinel ? SLOT_EMPTY : e);
    return group_hash(batches[ref_bid(e)].keys, S.n_keys, ref_row(e));
}


// ------------------------------------------------------------------------------------------
// Probing
// ------------------------------------------------------------------------------------------
// Find or claim the HBM slot of `key` (inline: packed key; ref: salt|bid|row entry).
// Returns the slot index or ~0 when the probe limit is hit (the caller records an overflow).
template <bool INLINE>
__device__ __forceinline__ u64 g_find(const Spec& S, const BatchDesc* batches, const DCol* keys, u64 i, u64 key,
                                      u64 h, const TableDesc& t, u32 probe_limit, bool& claimed) {
    claimed = false;
    if (INLINE && key == SLOT_EMPTY) {  // only possible for 8-byte packed keys: sentinel slot
        u64 old = at_cas<AS_GLB>(asp<AS_GLB>(t.slots + t.cap * t.stride_words), SLOT_EMPTY, 0ULL);
        claimed = old == SLOT_EMPTY;
        return t.cap;
    }
    u64 mask = t.cap - 1;
    u64 s = (INLINE ? slot_mix(key) : (h >> 16)) & mask;
    for (u32 p = 0; p < probe_limit; ++p) {
        wptr<AS_GLB> e = asp<AS_GLB>(t.slots + s * t.stride_words);
        u64 ev = vld<AS_GLB>(e);
        if (ev == SLOT_EMPTY) {
            u64 old = at_cas<AS_GLB>(e, SLOT_EMPTY, key);
            if (old == SLOT_EMPTY) {
                claimed = true;
                return s;
            }
            ev = old;
        }
        if (INLINE) {
            if (ev == key) return s;
        } else if ((ev >> 48) == (key >> 48) && ref_equal(S, batches, keys, i, ev)) {
            return s;
        }
        s = (s + 1) & mask;
    }
    return ~0ULL;
}

// Same against a table whose entries were claimed from a record/ovf entry that carries a
// foreign key (ref of another batch): compare through the batch table.
template <bool INLINE>
__device__ __forceinline__ u64 g_find_entry(const Spec& S, const BatchDesc* batches, u64 key, u64 h,
                                            const TableDesc& t, u32 probe_limit, bool& claimed) {
    const DCol* keys = INLINE ? nullptr : batches[ref_bid(key)].keys;
    return g_find<INLINE>(S, batches, keys, INLINE ? 0 : ref_row(key), key, h, t, probe_limit, claimed);
}

// LDS partial table: same probing, bounded occupancy; -1 = not staged (use HBM directly).
template <bool INLINE>
__device__ __forceinline__ int lds_find(const Spec& S, const BatchDesc* batches, const DCol* keys, u64 i, u64 key, u64 h,
                                        u64* lds, u32 lmask, u32 sw, u32* lcount, u32 llimit) {
    if (INLINE && key == SLOT_EMPTY) return -1;
    u32 s = (u32)((INLINE ? slot_mix(key) : (h >> 16)) & lmask);
    // Once the table is full (high cardinality), a key found within two probes is staged, any
    // other goes straight to HBM: a long probe through a full table of other keys is wasted LDS
    // traffic.  A key may then hold state both here and in HBM; the flush merges them.
    volatile __attribute__((address_space(3))) u32* lc = (volatile __attribute__((address_space(3))) u32*)lcount;
    const int cap = *lc >= llimit ? 2 : LDS_PROBE_CAP;
    for (int p = 0; p < cap; ++p) {
        wptr<AS_LDS> e = asp<AS_LDS>(lds + (u64)s * sw);
        u64 ev = vld<AS_LDS>(e);
        if (ev == SLOT_EMPTY) {
            if (*lc >= llimit) return -1;
            u64 old = at_cas<AS_LDS>(e, SLOT_EMPTY, key);
            if (old == SLOT_EMPTY) {
                __hip_atomic_fetch_add((__attribute__((address_space(3))) u32*)lcount, 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                return (int)s;
            }
            ev = old;
        }
        if (INLINE) {
            if (ev == key) return (int)s;
        } else if ((ev >> 48) == (key >> 48) && ref_equal(S, batches, keys, i, ev)) {
            return (int)s;
        }
        s = (s + 1) & lmask;
    }
    return -1;
}

__device__ __forceinline__ void push_ovf_row(const TableDesc& t, u32 bid, u64 row) {
    u64 k = atomicAdd((unsigned long long*)(t.counters + CNT_OVF_ROWS), 1ULL);
    if (k < t.ovf_rows_cap) t.ovf_rows[k] = ((u64)bid << 32) | row;
    else atomicOr((unsigned long long*)(t.counters + CNT_ERR), (unsigned long long)ERR_OVF_LOST);
}
template <bool SC1 = false, int RAS = AS_GLB>
__device__ __forceinline__ void push_ovf_rec(const Spec& S, const TableDesc& t, u64 key, const u64* words) {
    u64 k = atomicAdd((unsigned long long*)(t.counters + CNT_OVF_RECS), 1ULL);
    if (k >= t.ovf_recs_cap) {
        atomicOr((unsigned long long*)(t.counters + CNT_ERR), (unsigned long long)ERR_OVF_LOST);
        return;
    }
    u64* r = t.ovf_recs + k * t.stride_words;
    r[0] = key;
    for (int w = 1; w <= S.n_words; ++w) r[w] = rdw<SC1, RAS>(words + w);
}


// ------------------------------------------------------------------------------------------
// End of an insert launch: merge the workgroup's LDS partial table into the HBM table.
//
// Low cardinality is the hard case for the flush: every workgroup holds the same few hot groups,
// and G workgroups adding into the same HBM slots serialise at the memory side (device-scope
// atomics bypass the per-XCD L2).  So a workgroup whose LDS table holds <= SCR_ENTRIES groups
// parks it, compacted, in its scratch row; the last workgroup to finish (ticket) merges all
// parked rows in its own LDS table and flushes that once.  Larger tables (diverse keys, little
// contention) flush directly.  The combine of partial states follows combine_payload
// (EAGG/aggregate_hashtable.rs:383-425).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void st_sc1(u64* p, u64 v) {
    __hip_atomic_store((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool INLINE, bool RECORDS>
__device__ __forceinline__ u64 lds_entry_hash(const Spec& S, const BatchDesc& B, u64 e) {
    if (INLINE) return 0;
    if (RECORDS) return gld<u64>(B.rec_base + (u64)ref_row(e) * B.rec_width);
    return group_hash(B.keys, S.n_keys, ref_row(e));
}

template <bool INLINE, bool RECORDS, bool STR = true, bool W256 = true>  // STR, W256: see apply_row
__device__ __forceinline__ void flush_lds_direct(const Spec& S, const BatchDesc* batches, const BatchDesc& B, u64* lds,
                                                 u32 lds_slots, u32 sw, u32 nt, const TableDesc& t, u32& my_claims) {
    for (u32 s = threadIdx.x; s < lds_slots; s += nt) {
        u64* p = lds + (u64)s * sw;
        u64 e = p[0];
        if (e == SLOT_EMPTY) continue;
        u64 h = lds_entry_hash<INLINE, RECORDS>(S, B, e);
        bool claimed;
        u64 gs = g_find<INLINE>(S, batches, B.keys, INLINE ? 0 : ref_row(e), e, h, t, t.probe_limit, claimed);
        if (gs == ~0ULL) {
            push_ovf_rec<false, AS_LDS>(S, t, e, p);
            continue;
        }
        my_claims += claimed ? 1 : 0;
        apply_state<AS_GLB, false, AS_LDS, STR, W256>(S, asp<AS_GLB>(t.slots + gs * t.stride_words), p, batches);
    }
}

template <bool W256 = true>  // see apply_row
__device__ __forceinline__ void lds_table_init(const Spec& S, u64* lds, u32 lds_slots, u32 sw, u32 nt) {
    for (u32 s = threadIdx.x; s < lds_slots; s += nt) {
        u64* p = lds + (u64)s * sw;
        p[0] = SLOT_EMPTY;
        for (u32 w = 1; w < sw; ++w) p[w] = 0;
        for (int a = 0; a < S.n_aggs; ++a)
            if (S.aggs[a].kind == DBG_AGG_MIN || S.aggs[a].kind == DBG_AGG_MAX)
                for (int k = 0; k < S.aggs[a].nwords; ++k) p[S.aggs[a].w0 + k] = state_init_word<W256>(S.aggs[a], k);
    }
}

// lcount: [0] LDS claims, [1] HBM claims, [2] parked entries, [3] last-workgroup flag.
// Ends with the workgroup's HBM claims added to the table counter.
template <bool INLINE, bool RECORDS, bool STR = true, bool W256 = true>
__device__ __forceinline__ void block_flush(const Spec& S, const BatchDesc* batches, const BatchDesc& B, u64* lds, u32 lds_slots, u32 sw,
                            u32* lcount, u32 nt, const TableDesc& t, u32 my_claims) {
    const u32 lmask = lds_slots - 1;
    const u32 llimit = lds_slots - lds_slots / 4;
    const bool use_scr = t.scratch != nullptr && gridDim.x > 1 && gridDim.x <= t.scr_blocks;
    if (use_scr) {
        u64* counts = t.scratch;
        u64* tickets = t.scratch + t.scr_blocks;
        u64* rows = t.scratch + 2 * (u64)t.scr_blocks;
        u64* row = rows + (u64)blockIdx.x * SCR_ENTRIES * sw;
        if (lcount[0] <= SCR_ENTRIES) {  // park (uniform: lcount[0] is final after the barrier)
            for (u32 s = threadIdx.x; s < lds_slots; s += nt) {
                const u64* p = lds + (u64)s * sw;
                if (p[0] == SLOT_EMPTY) continue;
                u32 k = atomicAdd(&lcount[2], 1u);
                u64* d = row + (u64)k * sw;
                for (u32 w = 0; w <= (u32)S.n_words; ++w) st_sc1(d + w, p[w]);
            }
            __syncthreads();
            if (threadIdx.x == 0) st_sc1(counts + blockIdx.x, lcount[2]);
        } else {
            if (threadIdx.x == 0) st_sc1(counts + blockIdx.x, 0);
            flush_lds_direct<INLINE, RECORDS, STR, W256>(S, batches, B, lds, lds_slots, sw, nt, t, my_claims);
        }
        // Hand-off without release fences (MI355X_MICROARCH.md, inter-workgroup visibility, valid
        // forms): parked words are stored sc1 (write-through past the XCD's L2); every storing
        // wave drains them and the barrier orders all waves before lane 0's ticket add; the last
        // workgroup of each group of FLUSH_GROUP reads them back with sc1 loads behind one
        // agent-scope acquire.  Groups keep the merge tail short and parallel, and cut the
        // same-address atomics on the HBM table by FLUSH_GROUP (C1, 1464 workgroups of 4 groups:
        // FLUSH_GROUP 2 / 4 / 8 / 16 / 64 -> insert 0.470 / 0.432 / 0.439 / 0.467 / 0.649 ms: a
        // leader's serial merge of many parked tables costs more than the HBM atomics it saves).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const u32 g = blockIdx.x / FLUSH_GROUP;
        const u32 gsize = min((u32)FLUSH_GROUP, gridDim.x - g * FLUSH_GROUP);
        if (threadIdx.x == 0) {
            u64 tk = atomicAdd((unsigned long long*)(tickets + g), 1ULL);
            lcount[3] = tk == (u64)gsize - 1 ? 1u : 0u;
        }
        __syncthreads();
        if (lcount[3]) {  // the group's last workgroup: acquire, merge the group's parked rows, flush
            if (threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                tickets[g] = 0;  // ready for the next launch on this table (all members have added)
            }
            lds_table_init<W256>(S, lds, lds_slots, sw, nt);
            if (threadIdx.x == 0) lcount[0] = 0;
            __syncthreads();
            const u32 total = gsize * SCR_ENTRIES;
            for (u32 f = threadIdx.x; f < total; f += nt) {
                u64 b = (u64)g * FLUSH_GROUP + f / SCR_ENTRIES, k = f % SCR_ENTRIES;
                const u64* r = rows + (b * SCR_ENTRIES + k) * sw;
                u64 cnt = ld_sc1(counts + b);
                u64 e = ld_sc1(r);  // issued with the count: rows are allocated in full
                if (k >= cnt) continue;
                u64 h = lds_entry_hash<INLINE, RECORDS>(S, B, e);
                int ls = lds_find<INLINE>(S, batches, B.keys, INLINE ? 0 : ref_row(e), e, h, lds, lmask, sw, lcount, llimit);
                if (ls >= 0) {
                    apply_state<AS_LDS, true, AS_GLB, STR, W256>(S, asp<AS_LDS>(lds + (u64)ls * sw), r, batches);
                    continue;
                }
                bool claimed;
                u64 gs = g_find<INLINE>(S, batches, B.keys, INLINE ? 0 : ref_row(e), e, h, t, t.probe_limit, claimed);
                if (gs == ~0ULL) {
                    push_ovf_rec<true>(S, t, e, r);
                    continue;
                }
                my_claims += claimed ? 1 : 0;
                apply_state<AS_GLB, true, AS_GLB, STR, W256>(S, asp<AS_GLB>(t.slots + gs * t.stride_words), r, batches);
            }
            __syncthreads();
            flush_lds_direct<INLINE, RECORDS, STR, W256>(S, batches, B, lds, lds_slots, sw, nt, t, my_claims);
        }
    } else {
        flush_lds_direct<INLINE, RECORDS, STR, W256>(S, batches, B, lds, lds_slots, sw, nt, t, my_claims);
    }
    if (my_claims) atomicAdd(&lcount[1], my_claims);
    __syncthreads();
    if (threadIdx.x == 0 && lcount[1]) atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)lcount[1]);
}
