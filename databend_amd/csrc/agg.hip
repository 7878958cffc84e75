// agg.hip — gfx950 kernels of the hash GROUP BY path: the insert side.
//
//   table_init      : slots <- EMPTY entry + per-function initial state words
//   agg_insert      : fused  predicate -> group hash -> LDS-staged partial table -> HBM table
//                     (TransformFilter + AggregateHashTable::add_groups / combine_payload,
//                      EAGG/aggregate_hashtable.rs:128-425), with its specialised families
//                     agg_insert_str1, agg_insert_short and agg_insert_fast (whose last workgroup
//                     can finalize the table in the same launch)
//   agg_retry       : deferred overflow rows / partial records after the table has grown
//   agg_rehash      : grow the HBM table (AggregateHashTable::resize, :511-561)
//   launch_insert   : asks the four insert families in turn
//
// Each family's eligibility and launch function follow its kernel.  The other units of the path
// and the headers they share with this one: agg_table.hpp.
#include "agg_table.hpp"
#include "agg_fin_small.hpp"

// Host side: sizes the launches of more than one family use.
#define SHORT_MAX_SLOTS 65536  // HBM table slots up to which the short-key insert is taken
static u32 lds_slots_for(const Spec& S, u32 budget = LDS_BUDGET_BYTES) {
    u32 bytes_per = (u32)S.stride_words * 8;
    u32 n = 1;
    while ((n * 2) * bytes_per + 16 <= budget) n *= 2;
    return n;
}

// Grid of an insert whose workgroups each take one contiguous row range: workgroups of at least
// `min_rows` rows (`x_blocks` != 0: that many instead), at most DBG_INSERT_MAX_BLOCKS; `rpb`
// receives the rows per workgroup (`even_rpb`: rounded up to an even number), and workgroups
// whose range would be empty are left out.
static u32 row_range_grid(u64 rows, u64 min_rows, u64& rpb, bool even_rpb = false, u64 x_blocks = 0) {
    u64 blocks = (rows + min_rows - 1) / min_rows;
    if (x_blocks) blocks = x_blocks;
    if (blocks > DBG_INSERT_MAX_BLOCKS) blocks = DBG_INSERT_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    rpb = (rows + blocks - 1) / blocks;
    if (even_rpb) rpb = (rpb + 1) & ~1ULL;
    return (u32)((rows + rpb - 1) / rpb);
}

// ------------------------------------------------------------------------------------------
// table_init
// ------------------------------------------------------------------------------------------
// A memset of the table in 16-byte stores: chunk c is word pair (2k, 2k+1) of slot c / (sw / 2),
// its values from Spec::slot_init (stride_words is even: a power of two >= 2 or a multiple of 8).
typedef unsigned long long v2u64 __attribute__((ext_vector_type(2)));
__global__ void __launch_bounds__(BLOCK) table_init_kernel(const Spec* __restrict__ spec, u64* slots, u64 n_slots, u64* counters) {
    const Spec& S = *spec;
    if (counters && blockIdx.x == 0 && threadIdx.x < CNT_WORDS) counters[threadIdx.x] = 0;  // dbg_agg_reset
    const u32 half = (u32)S.tstride / 2;
    const u64 n_chunks = n_slots * half;
    v2u64 __attribute__((address_space(1)))* out = (v2u64 __attribute__((address_space(1)))*)slots;
    if (half == 1) {
        const v2u64 v = {S.slot_init[0], S.slot_init[1]};
        for (u64 c = blockIdx.x * (u64)BLOCK + threadIdx.x; c < n_chunks; c += (u64)gridDim.x * BLOCK) out[c] = v;
        return;
    }
    for (u64 c = blockIdx.x * (u64)BLOCK + threadIdx.x; c < n_chunks; c += (u64)gridDim.x * BLOCK) {
        u32 k = (u32)(c % half);
        out[c] = v2u64{S.slot_init[2 * k], S.slot_init[2 * k + 1]};
    }
}

void launch_table_init(hipStream_t s, const Spec* dspec, const Spec& hspec, u64* slots, u64 cap, u64* counters) {
    u64 n = (cap + 1) * (u64)(hspec.tstride / 2);
    u64 blocks = (n + BLOCK - 1) / BLOCK;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(table_init_kernel, dim3((u32)blocks), dim3(BLOCK), 0, s, dspec, slots, cap + 1, counters);
}

// ------------------------------------------------------------------------------------------
// agg_insert: one workgroup = one contiguous row range; LDS partial table, HBM fallback.
// ------------------------------------------------------------------------------------------
// One selected row (or partial record): group hash -> LDS table -> HBM table -> state update.
template <bool INLINE, bool RECORDS>
__device__ __forceinline__ void insert_one(const Spec& S, const BatchDesc* batches, const BatchDesc& B, u32 bid, u64 i,
                                           u64* lds, u32 lmask, u32 sw, u32* lcount, u32 llimit, const TableDesc& t,
                                           u32& my_claims) {
    u64 h, key;
    if (RECORDS) {
        h = gld<u64>(B.rec_base + i * (u64)B.rec_width);
    } else if (INLINE) {
        h = 0;
    } else {
        h = group_hash(B.keys, S.n_keys, i);
    }
    if (INLINE) key = pack_key(S, B.keys, i);
    else key = (h & 0xFFFF000000000000ULL) | ((u64)bid << 32) | i;

    int ls = lds_find<INLINE>(S, batches, B.keys, i, key, h, lds, lmask, sw, lcount, llimit);
    const u64* rec = RECORDS ? (const u64*)(B.rec_base + i * (u64)B.rec_width + S.rec_state_off) - 1 : nullptr;
    if (ls >= 0) {
        wptr<AS_LDS> st = asp<AS_LDS>(lds + (u64)ls * sw);
        if (RECORDS) apply_state<AS_LDS>(S, st, rec, batches);
        else apply_row<AS_LDS>(S, st, B, i, batches, bid);
        return;
    }
    bool claimed;
    u64 gs = g_find<INLINE>(S, batches, B.keys, i, key, h, t, t.probe_limit, claimed);
    if (gs == ~0ULL) {
        push_ovf_row(t, bid, i);
        return;
    }
    my_claims += claimed ? 1 : 0;
    wptr<AS_GLB> st = asp<AS_GLB>(t.slots + gs * t.stride_words);
    if (RECORDS) apply_state<AS_GLB>(S, st, rec, batches);
    else apply_row<AS_GLB>(S, st, B, i, batches, bid);
}

// Every FLUSH_ROUND rounds: a full LDS table is flushed to HBM and started over (the
// reference's clear_ht of a full partial table, aggregate_hashtable.rs:225-239), so hot keys of
// a skewed stream keep being combined in LDS instead of hammering one HBM slot (not once the HBM
// table overflows: the deferred-overflow lists are sized for two flushes of every workgroup's
// table).  Thread 0 decides, so the branch is uniform.  Called by every thread.
template <bool INLINE, bool RECORDS>
__device__ __forceinline__ void maybe_flush(const Spec& S, const BatchDesc* batches, const BatchDesc& B, u64* lds,
                                            u32 lds_slots, u32 sw, u32* lcount, u32 llimit, const TableDesc& t,
                                            u32& my_claims) {
    __shared__ u32 do_flush;
    if (threadIdx.x == 0)
        do_flush = lcount[0] >= llimit && ld_sc1(t.counters + CNT_OVF_ROWS) == 0 && ld_sc1(t.counters + CNT_OVF_RECS) == 0;
    __syncthreads();
    const bool flush_now = do_flush;
    __syncthreads();  // everyone has read the flag before thread 0 may rewrite it
    if (flush_now) {
        flush_lds_direct<INLINE, RECORDS>(S, batches, B, lds, lds_slots, sw, BLOCK, t, my_claims);
        __syncthreads();
        lds_table_init(S, lds, lds_slots, sw, BLOCK);
        if (threadIdx.x == 0) lcount[0] = 0;
        __syncthreads();
    }
}

template <bool INLINE, bool RECORDS>
__global__ void __launch_bounds__(BLOCK) agg_insert_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                          u32 bid, u64 rows, u64 rows_per_block, TableDesc t,
                                                          u32 lds_slots, u32 lenq) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const Spec& S = *spec;
    const BatchDesc& B = batches[bid];
    const u32 sw = S.stride_words;
    u32* lcount = (u32*)(lds + (u64)lds_slots * sw);  // [0] lds claims, [1] hbm claims
    const u32 lmask = lds_slots - 1;
    const u32 llimit = lds_slots - lds_slots / 4;

    lds_table_init(S, lds, lds_slots, sw, BLOCK);
    if (threadIdx.x < 4) lcount[threadIdx.x] = 0;
    __syncthreads();
    auto insert_row = [&](u64 i, u32& my_claims) {
        insert_one<INLINE, RECORDS>(S, batches, B, bid, i, lds, lmask, sw, lcount, llimit, t, my_claims);
    };

    u64 r0 = (u64)blockIdx.x * rows_per_block;
    u64 r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    u32 my_claims = 0;
    const u64 n_iter = r1 > r0 ? (r1 - r0 + BLOCK - 1) / BLOCK : 0;
    if (!RECORDS && B.n_nodes && rows_per_block < (1ULL << 32)) {
        // Filtered input (FilterExecutor::select then take, EXP/filter/filter_executor.rs:73-128):
        // every lane evaluates the predicate on its row, the selected rows are queued in LDS (wave
        // ballot + one LDS add per wave), and the hash / probe / state update runs on BLOCK queued
        // rows at a time with every lane busy — at 13% selectivity (ClickBench Q13) the
        // row-per-lane loop would run the long dependent chain of a string key with 1 lane in 8.
        // PU rounds of BLOCK rows are evaluated per step with all their loads issued together (one
        // row per lane per round, a single round in flight left the stream latency-bound: C5's
        // predicate pass ran at ~1.2 TB/s), queued together, and inserted BLOCK at a time.
        // `s <op> ''` on one non-null String column (ClickBench Q13: SearchPhrase <> ''): the
        // selection is a function of the row's length alone, read from the offsets; PU rounds of
        // BLOCK rows are evaluated per step with all their offset loads issued together (one row
        // per lane per round left C5's predicate pass latency-bound, ~1.2 TB/s)
        constexpr int PU = 4;
        static_assert(FLUSH_ROUND % PU == 0, "flush checks fall on step boundaries");
        __shared__ u32 selq[2 * BLOCK];
        __shared__ u32 qn;
        if (threadIdx.x == 0) qn = 0;
        __syncthreads();
        const u32 lane = __lane_id();
        const DNode& n0 = B.nodes[0];
        const DCol& c0 = B.fcols[n0.col];
        // its (PU + 1)-round queue lives in dynamic LDS after the table (lenq entries, host-sized
        // only for such a predicate: the other predicates keep the static 2-round queue and the
        // occupancy it allows — C1: 6 workgroups per CU, all 1464 resident at once)
        const bool lenpred = lenq >= (PU + 1) * BLOCK && B.n_nodes == 1 && n0.op == DBG_PRED_CMP_CONST && n0.str_len == 0 &&
                             c0.type == DBG_STRING && !c0.nullable && c0.layout == LAYOUT_ARROW;
        // the queue in use: the static one, or the multi-round one after the table (lenpred)
        u32* qbuf = lenpred ? (u32*)(lds + (u64)lds_slots * sw + 2) : selq;
        if (lenpred) {
            u32* selq = qbuf;
            const u64* __restrict__ offs = c0.offsets;
            for (u64 it = 0; it < n_iter; it += PU) {
                if (it && (it % FLUSH_ROUND) == 0) maybe_flush<INLINE, RECORDS>(S, batches, B, lds, lds_slots, sw, lcount, llimit, t, my_claims);
                u64 a[PU], b[PU];
#pragma unroll
                for (int k = 0; k < PU; ++k) {
                    const u64 i = r0 + (it + k) * BLOCK + threadIdx.x;
                    const u64 j = i < r1 ? i : r0;
                    a[k] = gld<u64>(offs + j);
                    b[k] = gld<u64>(offs + j + 1);
                }
                bool sel[PU];
                u32 cnt = 0;
                u64 mk[PU];
#pragma unroll
                for (int k = 0; k < PU; ++k) {
                    const u64 i = r0 + (it + k) * BLOCK + threadIdx.x;
                    sel[k] = i < r1 && apply_cmp(n0.cmp, b[k] != a[k] ? 1 : 0);
                    mk[k] = __ballot(sel[k]);
                    cnt += (u32)__popcll(mk[k]);
                }
                if (cnt) {  // queue the step's selected rows: one LDS add per wave
                    u32 wbase = 0;
                    if (lane == 0) wbase = atomicAdd(&qn, cnt);
                    wbase = __shfl(wbase, 0);
                    const u64 lt = (1ULL << lane) - 1;
#pragma unroll
                    for (int k = 0; k < PU; ++k) {
                        if (sel[k]) selq[wbase + (u32)__popcll(mk[k] & lt)] = (u32)((it + k) * BLOCK + threadIdx.x);
                        wbase += (u32)__popcll(mk[k]);
                    }
                }
                __syncthreads();
                const u32 n = qn;  // < (PU + 1) * BLOCK
                if (n >= BLOCK) {
                    const u32 full = n / BLOCK;
                    for (u32 c = 0; c < full; ++c) insert_row(r0 + selq[c * BLOCK + threadIdx.x], my_claims);
                    const u32 rem = n - full * BLOCK;  // < BLOCK: moved to the front
                    const u32 mv = threadIdx.x < rem ? selq[full * BLOCK + threadIdx.x] : 0u;
                    __syncthreads();
                    if (threadIdx.x < rem) selq[threadIdx.x] = mv;
                    if (threadIdx.x == 0) qn = rem;
                }
                __syncthreads();  // the queue is settled before the next step appends
            }
        } else {
            for (u64 it = 0; it < n_iter; ++it) {
                if (it && (it % FLUSH_ROUND) == 0) maybe_flush<INLINE, RECORDS>(S, batches, B, lds, lds_slots, sw, lcount, llimit, t, my_claims);
                const u64 i = r0 + it * BLOCK + threadIdx.x;
                const bool sel = i < r1 && eval_pred(B.nodes, B.n_nodes, B.fcols, i);
                const u64 m = __ballot(sel);
                if (m) {
                    u32 wbase = 0;
                    if (lane == 0) wbase = atomicAdd(&qn, (u32)__popcll(m));
                    wbase = __shfl(wbase, 0);
                    if (sel) selq[wbase + (u32)__popcll(m & ((1ULL << lane) - 1))] = (u32)(i - r0);
                }
                __syncthreads();
                const u32 n = qn;  // < 2 * BLOCK
                if (n >= BLOCK) {
                    const u32 off = selq[threadIdx.x];
                    const u32 rem = n - BLOCK;  // < BLOCK
                    const u32 mv = threadIdx.x < rem ? selq[BLOCK + threadIdx.x] : 0u;
                    __syncthreads();
                    if (threadIdx.x < rem) selq[threadIdx.x] = mv;
                    if (threadIdx.x == 0) qn = rem;
                    insert_row(r0 + off, my_claims);
                }
                __syncthreads();  // the queue is settled before the next round appends
            }
        }
        const u32 n = qn;  // < BLOCK
        if (threadIdx.x < n)
            insert_row(r0 + qbuf[threadIdx.x], my_claims);
    } else {
        for (u64 it = 0; it < n_iter; ++it) {
            if (it && (it % FLUSH_ROUND) == 0) maybe_flush<INLINE, RECORDS>(S, batches, B, lds, lds_slots, sw, lcount, llimit, t, my_claims);
            const u64 i = r0 + it * BLOCK + threadIdx.x;
            if (i >= r1) continue;
            if (!RECORDS && B.n_nodes && !eval_pred(B.nodes, B.n_nodes, B.fcols, i)) continue;
            if (RECORDS && B.seg_records) {  // fixed-capacity segments: record 0 is [count][flags]
                const u64 q = i % B.seg_records;
                const u8* hdr = B.rec_base + (i - q) * (u64)B.rec_width;
                if (q == 0) {
                    if (gld<u64>(hdr + 8)) atomicOr((unsigned long long*)(t.counters + CNT_ERR), (unsigned long long)ERR_FIXED_INCOMPLETE);
                    continue;
                }
                if (q > gld<u64>(hdr)) continue;
            }
            insert_row(i, my_claims);
        }
    }
    __syncthreads();
    block_flush<INLINE, RECORDS>(S, batches, B, lds, lds_slots, sw, lcount, BLOCK, t, my_claims);
}

// The generic insert takes every batch.
static InsertPath launch_insert_generic(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, u32 bid, u64 rows,
                                        bool records, const TableDesc& t, bool use_lds, const BatchDesc* hb) {
    u32 lslots = use_lds ? lds_slots_for(S, LDS_BUDGET_BYTES) : 1;
    // enough workgroups to fill 256 CUs several times over, each a contiguous row range
    u64 rpb;
    const u32 blocks = row_range_grid(rows, (u64)BLOCK * 16, rpb);
    size_t shmem = (size_t)lslots * S.stride_words * 8 + 16;
    // `string <op> ''` filter (one node on a non-null arrow String column): the kernel's
    // multi-round queue (5 rounds of BLOCK row indices) after the table
    u32 lenq = 0;
    if (hb && !records && hb->n_nodes == 1 && hb->nodes[0].op == DBG_PRED_CMP_CONST && hb->nodes[0].str_len == 0) {
        const DCol& c = hb->fcols[hb->nodes[0].col];
        if (c.type == DBG_STRING && !c.nullable && c.layout == LAYOUT_ARROW) lenq = 5 * BLOCK;
    }
    shmem += (size_t)lenq * 4;
    if (S.inline_keys) {
        if (records) hipLaunchKernelGGL((agg_insert_kernel<true, true>), dim3(blocks), dim3(BLOCK), shmem, s, dspec, batches, bid, rows, rpb, t, lslots, lenq);
        else hipLaunchKernelGGL((agg_insert_kernel<true, false>), dim3(blocks), dim3(BLOCK), shmem, s, dspec, batches, bid, rows, rpb, t, lslots, lenq);
    } else {
        if (records) hipLaunchKernelGGL((agg_insert_kernel<false, true>), dim3(blocks), dim3(BLOCK), shmem, s, dspec, batches, bid, rows, rpb, t, lslots, lenq);
        else hipLaunchKernelGGL((agg_insert_kernel<false, false>), dim3(blocks), dim3(BLOCK), shmem, s, dspec, batches, bid, rows, rpb, t, lslots, lenq);
    }
    return lenq ? INS_GENERIC_LENPRED : INS_GENERIC;
}

// ------------------------------------------------------------------------------------------
// agg_insert_str1: one non-null Arrow String key (ClickBench Q13: SearchPhrase), filtered by
// `key <op> ''` or not at all, into a table whose slots cache the key (Spec::kc_word).
//
// The generic kernel compares every probe against the representative row in global memory: an
// LDS hit reads that row's offsets and bytes, an LDS miss reads the HBM slot, then the row's
// offsets and bytes — three dependent random reads before the atomic (C5: 6x the algorithmic
// bytes).  Here the key's first 32 bytes and a header (hash bits 16..63, length, ready bit) sit
// beside the entry in LDS and HBM slots alike, so a probe decides inside the slot: an LDS hit
// touches no global memory, an HBM miss reads its slot's line and adds.  The stream reads two
// offsets per lane per 16-B load, keeps the selected rows' (byte offset, row, length) in an LDS
// queue and inserts them 256 at a time with every lane busy.
//
// Exactness: a different header means a different key (hash or length differ).  An equal header
// with equal cached bytes and a length <= 32 is the same key.  Anything else — a header not yet
// published (a claim in flight on this or another XCD, whose L2s are not coherent), equal headers
// with different bytes, a key longer than 32 bytes — compares against the representative row
// (ref_equal), as the generic kernel always does.  A claimer writes the key words with sc1 stores,
// drains them, then publishes the header sc1 (MI355X_MICROARCH.md, inter-workgroup visibility);
// readers load the slot with sc1 loads.  In LDS a slot whose header is not yet published is
// passed over (the row goes to HBM; the flush merges both states), so no lane ever waits.
// ------------------------------------------------------------------------------------------
typedef volatile __attribute__((address_space(3))) u64 vlds_u64;
typedef volatile __attribute__((address_space(3))) u32 vlds_u32;
// STR1_NT threads per workgroup, STR1_ROUNDS rounds of 2 x STR1_NT rows per stream step
#ifndef STR1_NT
#define STR1_NT 512
#endif
#ifndef STR1_ROUNDS
#define STR1_ROUNDS 2
#endif
#define STR1_QCAP ((2 * STR1_ROUNDS + 1) * STR1_NT)
#define STR1_LDS_BUDGET (56 * 1024)  // the key-caching LDS table (1024 slots for COUNT)

struct KcKey {
    u64 k[KC_KEY_WORDS];  // first 32 bytes, little-endian, zero-padded
    u64 h;                // group hash (hash_bytes)
    u64 hdr;              // (h & ~0xFFFF) | (len & 0x7FFF) << 1 | 1
    u32 len;
};

__device__ __forceinline__ void kc_key(const u8* p, u32 len, KcKey& q) {
    q.len = len;
    const u32 n = len < 8 * KC_KEY_WORDS ? len : 8 * KC_KEY_WORDS;
    const uintptr_t a = (uintptr_t)p;
    const u32 sh = (u32)(a & 7);
    const u64* base = (const u64*)(a - sh);
    const u32 nw = n ? (sh + n + 7) >> 3 : 0;  // aligned words covering [p, p + n): <= 5
    u64 w[KC_KEY_WORDS + 1];
#pragma unroll
    for (int j = 0; j <= KC_KEY_WORDS; ++j) w[j] = (u32)j < nw ? gld<u64>(base + j) : 0;
#pragma unroll
    for (int j = 0; j < KC_KEY_WORDS; ++j) {
        u64 v = sh ? (w[j] >> (8 * sh)) | (w[j + 1] << (64 - 8 * sh)) : w[j];
        const int rem = (int)n - 8 * j;
        q.k[j] = rem >= 8 ? v : (rem <= 0 ? 0 : v & ((1ULL << (8 * rem)) - 1));
    }
    if (len <= 8 * KC_KEY_WORDS) {  // hash_bytes over the register words (device.hpp)
        const u64 M = 0xc6a4a7935bd1e995ULL, R = 47;
        u64 h = 0xe17a1465ULL ^ ((u64)len * M);
        const u32 nb = len >> 3, tl = len & 7;
        u64 tail = 0;
#pragma unroll
        for (u32 i = 0; i < KC_KEY_WORDS; ++i) {
            if (i < nb) {
                u64 x = q.k[i] * M;
                x ^= x >> R;
                x *= M;
                h ^= x;
                h *= M;
            }
            if (i == nb) tail = q.k[i];
        }
        if (tl) h ^= __builtin_bswap64(tail) >> (8 * (8 - tl));
        h ^= h >> R;
        h *= M;
        h ^= h >> R;
        q.h = h;
    } else {
        q.h = hash_bytes(p, len);
    }
    q.hdr = (q.h & ~0xFFFFULL) | ((u64)(len < 0x7FFF ? len : 0x7FFF) << 1) | 1;
}

// LDS probe of the key-caching table; -1 = not staged here (use HBM).
__device__ __forceinline__ int lds_find_kc(u64* lds, u32 lmask, u32 lsw, u32 kc, u32* lcount, u32 llimit, u64 key, const KcKey& q) {
    if (q.len > 8 * KC_KEY_WORDS) return -1;
    vlds_u32* lc = (vlds_u32*)lcount;
    u32 s = (u32)(q.h >> 16) & lmask;
    const int cap = *lc >= llimit ? 2 : LDS_PROBE_CAP;
    for (int p = 0; p < cap; ++p) {
        vlds_u64* e = (vlds_u64*)(lds + (u64)s * lsw);
        u64 ev = e[0];
        if (ev == SLOT_EMPTY) {
            if (*lc >= llimit) return -1;
            u64 old = at_cas<AS_LDS>(asp<AS_LDS>(lds + (u64)s * lsw), SLOT_EMPTY, key);
            if (old == SLOT_EMPTY) {
                __hip_atomic_fetch_add((__attribute__((address_space(3))) u32*)lcount, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
                for (int j = 0; j < KC_KEY_WORDS; ++j) e[kc + 1 + j] = q.k[j];
                e[kc] = q.hdr;  // volatile LDS accesses stay in order: the words are visible first
                return (int)s;
            }
            ev = old;
        }
        if ((ev >> 48) == (key >> 48)) {
            const u64 hv = e[kc];
            if (!(hv & 1)) return -1;  // a claim in flight: not waited for
            if (hv == q.hdr) {
                bool eq = true;
#pragma unroll
                for (int j = 0; j < KC_KEY_WORDS; ++j) eq &= e[kc + 1 + j] == q.k[j];
                if (eq) return (int)s;
            }
        }
        s = (s + 1) & lmask;
    }
    return -1;
}

// HBM probe with the slot's key cache; exact (see above).  ~0 = probe limit reached.  The slot's
// entry and its cache words are loaded together (16-B loads of one 64-B slot); a stale copy (this
// CU's L1 or this XCD's L2 holding the line from before a claim) can only show EMPTY — the CAS
// then returns the real entry — or an unpublished header, which takes the representative row.
__device__ __forceinline__ u64 g_find_kc(const Spec& S, const BatchDesc* batches, const DCol* keys, u64 i, u64 key, const KcKey& q,
                                         const TableDesc& t, u32 probe_limit, bool& claimed) {
    claimed = false;
    const u32 kc = (u32)S.kc_word, kp = kc >> 1;
    const bool odd = kc & 1;
    const u64 mask = t.cap - 1;
    u64 s = (q.h >> 16) & mask;
    for (u32 p = 0; p < probe_limit; ++p) {
        u64* slot = t.slots + s * t.stride_words;
        const v2u64 __attribute__((address_space(1)))* sp = (const v2u64 __attribute__((address_space(1)))*)slot;
        const v2u64 p0 = sp[0], pa = sp[kp], pb = sp[kp + 1], pc = sp[kp + 2];
        u64 ev = p0[0];
        u64 hv = odd ? pa[1] : pa[0];
        u64 w[KC_KEY_WORDS] = {odd ? pb[0] : pa[1], odd ? pb[1] : pb[0], odd ? pc[0] : pb[1], odd ? pc[1] : pc[0]};
        if (ev == SLOT_EMPTY) {
            u64 old = at_cas<AS_GLB>(asp<AS_GLB>(slot), SLOT_EMPTY, key);
            if (old == SLOT_EMPTY) {
                claimed = true;
#pragma unroll
                for (int j = 0; j < KC_KEY_WORDS; ++j) st_sc1(slot + kc + 1 + j, q.k[j]);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                st_sc1(slot + kc, q.hdr);
                return s;
            }
            ev = old;
            hv = ld_sc1(slot + kc);  // the line was read before the claim: the cache again
#pragma unroll
            for (int j = 0; j < KC_KEY_WORDS; ++j) w[j] = ld_sc1(slot + kc + 1 + j);
        }
        if ((ev >> 48) == (key >> 48)) {
            if ((hv & 1) && hv != q.hdr) {  // published and different: another key
                s = (s + 1) & mask;
                continue;
            }
            bool eq = (hv & 1) && q.len <= 8 * KC_KEY_WORDS;
#pragma unroll
            for (int j = 0; j < KC_KEY_WORDS; ++j) eq = eq && w[j] == q.k[j];
            if (eq || ref_equal(S, batches, keys, i, ev)) return s;
        }
        s = (s + 1) & mask;
    }
    return ~0ULL;
}

// The key-caching LDS table into HBM (end of block, and whenever it fills: maybe_flush's rule).
__device__ __forceinline__ void flush_kc(const Spec& S, const BatchDesc* batches, const BatchDesc& B, u64* lds, u32 lds_slots, u32 lsw,
                                         u32 kc, const TableDesc& t, u32& my_claims) {
    for (u32 s = threadIdx.x; s < lds_slots; s += STR1_NT) {
        u64* p = lds + (u64)s * lsw;
        const u64 e = p[0];
        if (e == SLOT_EMPTY) continue;
        KcKey q;
        const u64 hv = p[kc];
        const u64 i = ref_row(e);
        u64 gs;
        bool claimed;
        if (hv & 1) {  // every claim has published its header before the flush's barrier
            q.hdr = hv;
            q.len = (u32)((hv >> 1) & 0x7FFF);
            for (int j = 0; j < KC_KEY_WORDS; ++j) q.k[j] = p[kc + 1 + j];
            // the slot index uses hash bits 16..: the header holds them; the salt is in the entry
            q.h = (hv & ~0xFFFFULL);
            gs = g_find_kc(S, batches, B.keys, i, e, q, t, t.probe_limit, claimed);
        } else {
            gs = g_find<false>(S, batches, B.keys, i, e, group_hash(B.keys, S.n_keys, i), t, t.probe_limit, claimed);
        }
        if (gs == ~0ULL) {
            push_ovf_rec<false, AS_LDS>(S, t, e, p);
            continue;
        }
        my_claims += claimed ? 1 : 0;
        apply_state<AS_GLB, false, AS_LDS>(S, asp<AS_GLB>(t.slots + gs * t.stride_words), p, batches);
    }
}

__device__ __forceinline__ void lds_init_kc(const Spec& S, u64* lds, u32 lds_slots, u32 lsw) {
    for (u32 s = threadIdx.x; s < lds_slots; s += STR1_NT) {
        u64* p = lds + (u64)s * lsw;
        p[0] = SLOT_EMPTY;
        for (u32 w = 1; w < lsw; ++w) p[w] = w < (u32)S.kc_word ? S.slot_init[w] : 0;
    }
}

template <bool PRED>
__global__ void __launch_bounds__(STR1_NT) agg_insert_str1_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                               u32 bid, u64 rows, u64 rows_per_block, TableDesc t, u32 lds_slots,
                                                               u32 fper, u32 xmode) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const Spec& S = *spec;
    const BatchDesc& B = batches[bid];
    const u32 kc = (u32)S.kc_word, lsw = kc + 1 + KC_KEY_WORDS;
    // [0] LDS claims, [1] HBM claims, [2] queue length, [3] flush flag, [4] LDS hits, [5] misses
    u32* lcount = (u32*)(lds + (u64)lds_slots * lsw);
    u32* qoff = lcount + 8;       // queue: key byte offset - offs[r0]
    u32* qrl = qoff + STR1_QCAP;  // (row - r0) << 6 | min(len, 63)
    const u32 lmask = lds_slots - 1, llimit = lds_slots - lds_slots / 4;
    lds_init_kc(S, lds, lds_slots, lsw);
    if (threadIdx.x < 8) lcount[threadIdx.x] = 0;
    __syncthreads();
    const DCol& kcol = B.keys[0];
    const u64* __restrict__ offs = kcol.offsets;
    const u8* __restrict__ data = kcol.data;
    const int pcmp = PRED ? B.nodes[0].cmp : 0;
    const u64 r0 = (u64)blockIdx.x * rows_per_block;
    const u64 r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    const u32 lane = __lane_id();
    const u64 lt = (1ULL << lane) - 1;
    const u64 off0 = r0 < rows ? gld<u64>(offs + r0) : 0;
    u32 my_claims = 0;

    auto insert = [&](u32 offr, u32 rl) {
        const u64 i = r0 + (rl >> 6);
        u64 off = off0 + offr;
        u32 len = rl & 63;
        if (len == 63 || offr == ~0u) {  // long key or far offset: read the row's offsets again
            off = gld<u64>(offs + i);
            len = (u32)(gld<u64>(offs + i + 1) - off);
        }
        // timing ablations (EXP=1 builds only, DBG_X_STR1): 1 stream + queue only, 2 + key loads
        // and hash, 4 misses dropped, 8 no LDS table
        if (kExperiments && (xmode & 1)) {
            if (off == ~0ULL) atomicAdd(&lcount[1], 1u);
            return;
        }
        KcKey q;
        kc_key(data + off, len, q);
        if (kExperiments && (xmode & 2)) {
            if (q.h == 0x1234567ULL) atomicAdd(&lcount[1], 1u);
            return;
        }
        const u64 key = (q.h & 0xFFFF000000000000ULL) | ((u64)bid << 32) | i;
        const int ls = (kExperiments && (xmode & 8)) ? -1 : lds_find_kc(lds, lmask, lsw, kc, lcount, llimit, key, q);
        const u64 hm = __ballot(ls >= 0), mm = __ballot(ls < 0);
        if (lane == 0) {  // the flush rule's hit rate: one LDS add per wave
            atomicAdd(&lcount[4], (u32)__popcll(hm));
            atomicAdd(&lcount[5], (u32)__popcll(mm));
        }
        if (ls >= 0) {
            apply_row<AS_LDS>(S, asp<AS_LDS>(lds + (u64)ls * lsw), B, i, batches, bid);
            return;
        }
        if (kExperiments && (xmode & 4)) return;
        bool claimed;
        const u64 gs = g_find_kc(S, batches, B.keys, i, key, q, t, t.probe_limit, claimed);
        if (gs == ~0ULL) {
            push_ovf_row(t, bid, i);
            return;
        }
        my_claims += claimed ? 1 : 0;
        apply_row<AS_GLB>(S, asp<AS_GLB>(t.slots + gs * t.stride_words), B, i, batches, bid);
    };

    // A full LDS table is flushed to HBM and started over only while it serves few rows (hit rate
    // below 1/4 since the last check): with Zipf keys (ClickBench Q13) the first keys a workgroup
    // meets are the hot ones and flushing them every few rounds cost more than it saved (C5 insert
    // 15.3 -> 13.0 ms without periodic flushes), while clustered input (a key's rows together)
    // would otherwise send a hot key's rows to one HBM slot for good.
    auto maybe_flush_kc = [&]() {
        if (threadIdx.x == 0) {
            lcount[3] = lcount[0] >= llimit && 3 * lcount[4] < lcount[5] && ld_sc1(t.counters + CNT_OVF_ROWS) == 0 &&
                        ld_sc1(t.counters + CNT_OVF_RECS) == 0;
            lcount[4] = lcount[5] = 0;
        }
        __syncthreads();
        const bool now = lcount[3];
        __syncthreads();
        if (now) {
            flush_kc(S, batches, B, lds, lds_slots, lsw, kc, t, my_claims);
            __syncthreads();
            lds_init_kc(S, lds, lds_slots, lsw);
            if (threadIdx.x == 0) lcount[0] = 0;
            __syncthreads();
        }
    };

    // the stream: two rows per lane per round, offs[i], offs[i + 1] in one 16-B load (i even,
    // offsets 16-B aligned: host-checked), offs[i + 2] from the next lane — or loaded, by the
    // wave's last lane and wherever the next lane's pair runs past the batch's last offset.  The
    // next step's loads are issued before this step's rows are queued and inserted.
    constexpr u64 STEP = (u64)STR1_ROUNDS * 2 * STR1_NT;
    u64 nv[STR1_ROUNDS][3];
    auto load_step = [&](u64 base) {
#pragma unroll
        for (int k = 0; k < STR1_ROUNDS; ++k) {
            const u64 i = base + (u64)k * 2 * STR1_NT + 2 * threadIdx.x;
            const u64 j = i + 1 <= rows ? i : 0;
            const v2u64 v = *(const v2u64 __attribute__((address_space(1)))*)(offs + j);
            nv[k][0] = v[0];
            nv[k][1] = v[1];
            nv[k][2] = ((lane == 63 || i + 3 > rows) && i + 2 <= rows) ? gld<u64>(offs + i + 2) : 0;
        }
    };
    if (r0 < r1) load_step(r0);
    u32 step = 0;
    for (u64 base = r0; base < r1; base += STEP, ++step) {
        if (fper && step && (step % fper) == 0) maybe_flush_kc();
        u64 a[STR1_ROUNDS][3];
#pragma unroll
        for (int k = 0; k < STR1_ROUNDS; ++k)
            for (int r = 0; r < 3; ++r) a[k][r] = nv[k][r];
        if (base + STEP < r1) load_step(base + STEP);
        u64 mk[STR1_ROUNDS][2];
        u32 cnt = 0;
#pragma unroll
        for (int k = 0; k < STR1_ROUNDS; ++k) {
            const u64 i = base + (u64)k * 2 * STR1_NT + 2 * threadIdx.x;
            const u64 nx = __shfl_down(a[k][0], 1);
            if (lane != 63 && i + 3 <= rows) a[k][2] = nx;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const u64 len = a[k][r + 1] - a[k][r];
                bool sel = i + r < r1;
                if (PRED) sel = sel && apply_cmp(pcmp, len != 0 ? 1 : 0);
                mk[k][r] = __ballot(sel);
                cnt += (u32)__popcll(mk[k][r]);
            }
        }
        if (cnt) {  // queue the step's selected rows: one LDS add per wave
            u32 wb = 0;
            if (lane == 0) wb = atomicAdd(&lcount[2], cnt);
            wb = __shfl(wb, 0);
#pragma unroll
            for (int k = 0; k < STR1_ROUNDS; ++k) {
                const u64 i = base + (u64)k * 2 * STR1_NT + 2 * threadIdx.x;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if ((mk[k][r] >> lane) & 1) {
                        const u32 q = wb + (u32)__popcll(mk[k][r] & lt);
                        const u64 d = a[k][r] - off0, len = a[k][r + 1] - a[k][r];
                        qoff[q] = d < 0xFFFFFFFFULL ? (u32)d : ~0u;
                        qrl[q] = (u32)(i + r - r0) << 6 | (u32)(len < 63 ? len : 63);
                    }
                    wb += (u32)__popcll(mk[k][r]);
                }
            }
        }
        __syncthreads();
        const u32 n = lcount[2];  // < STR1_QCAP
        if (n >= STR1_NT) {
            const u32 full = n / STR1_NT;
            for (u32 c = 0; c < full; ++c) insert(qoff[c * STR1_NT + threadIdx.x], qrl[c * STR1_NT + threadIdx.x]);
            const u32 rem = n - full * STR1_NT;  // < STR1_NT: moved to the front
            u32 mo = 0, mr = 0;
            if (threadIdx.x < rem) {
                mo = qoff[full * STR1_NT + threadIdx.x];
                mr = qrl[full * STR1_NT + threadIdx.x];
            }
            __syncthreads();
            if (threadIdx.x < rem) {
                qoff[threadIdx.x] = mo;
                qrl[threadIdx.x] = mr;
            }
            if (threadIdx.x == 0) lcount[2] = rem;
        }
        __syncthreads();  // the queue is settled before the next step appends
    }
    const u32 n = lcount[2];  // < STR1_NT
    if (threadIdx.x < n) insert(qoff[threadIdx.x], qrl[threadIdx.x]);
    __syncthreads();
    flush_kc(S, batches, B, lds, lds_slots, lsw, kc, t, my_claims);
    if (my_claims) atomicAdd(&lcount[1], my_claims);
    __syncthreads();
    if (threadIdx.x == 0 && lcount[1]) atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)lcount[1]);
}

// agg_insert_str1_kernel: one non-null Arrow String key (the Spec's key cache), no predicate or
// `key <op> ''` on that same column, offsets 16-B aligned, row offsets below 2^32 per workgroup.
static bool str1_eligible(const Spec& S, const BatchDesc& hb, u64 rows) {
    if (!S.kc_word || hb.is_records || S.n_keys != 1) return false;
    const DCol& k = hb.keys[0];
    if (k.type != DBG_STRING || k.nullable || k.layout != LAYOUT_ARROW || ((uintptr_t)k.offsets & 15)) return false;
    if (rows >= (1ULL << 32)) return false;  // queue entries hold (row - r0) << 6 in 32 bits: < 2^26 per workgroup
    if (hb.n_nodes == 0) return true;
    if (hb.n_nodes != 1) return false;
    const DNode& n = hb.nodes[0];
    const DCol& c = hb.fcols[n.col];
    return n.op == DBG_PRED_CMP_CONST && n.str_len == 0 && c.type == DBG_STRING && !c.nullable && c.layout == LAYOUT_ARROW &&
           c.offsets == k.offsets && c.data == k.data;
}

static InsertPath launch_insert_str1(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, u32 bid, u64 rows,
                                     bool records, const TableDesc& t, bool use_lds, const BatchDesc* hb) {
    // one non-null String key into a large key-caching table, filtered by `key <op> ''` or not
    const bool mine = !records && use_lds && hb && S.kc_word && t.cap + 1 > SHORT_MAX_SLOTS && str1_eligible(S, *hb, rows);
    if (!mine) return INS_NONE;
    const u32 lsw = (u32)S.kc_word + 1 + KC_KEY_WORDS;
    static const u32 x_mode = X_ENV("DBG_X_STR1") ? (u32)atoi(X_ENV("DBG_X_STR1")) : 0;
    static const u32 x_lds = X_ENV("DBG_X_STR1_LDS") ? (u32)atoi(X_ENV("DBG_X_STR1_LDS")) * 1024 : STR1_LDS_BUDGET;
    static const u32 fper = X_ENV("DBG_X_STR1_FLUSH") ? (u32)atoi(X_ENV("DBG_X_STR1_FLUSH")) : 4;
    u32 ls = 1;
    while ((ls * 2) * lsw * 8 <= x_lds) ls *= 2;
    const size_t shmem = (size_t)ls * lsw * 8 + 32 + (size_t)STR1_QCAP * 8;
    u64 rpb;
    const u32 blocks = row_range_grid(rows, (u64)STR1_NT * 16, rpb, true);  // even: 16-B offset loads
    if (hb->n_nodes) hipLaunchKernelGGL(agg_insert_str1_kernel<true>, dim3(blocks), dim3(STR1_NT), shmem, s, dspec, batches, bid, rows, rpb, t, ls, fper, x_mode);
    else hipLaunchKernelGGL(agg_insert_str1_kernel<false>, dim3(blocks), dim3(STR1_NT), shmem, s, dspec, batches, bid, rows, rpb, t, ls, fper, x_mode);
    return hb->n_nodes ? INS_STR1_PRED : INS_STR1;
}

// ------------------------------------------------------------------------------------------
// agg_insert_short: the generic insert specialised for short String keys and COUNT / SUM / AVG over
// non-nullable arguments (TPC-H Q1: GROUP BY l_returnflag, l_linestatus — 1-byte strings — with
// seven Decimal128 SUM / AVG).  The generic kernel's chain per queued row is: predicate -> LDS
// queue -> key offsets -> key bytes -> hash -> LDS probe -> the representative row's offsets ->
// its bytes -> the arguments -> LDS atomics, seven dependent global round trips.  Here the rows
// stay on their lanes (no queue): a row's key offsets and argument values are loaded together,
// then its key bytes with the predicate's column (fetching a row ahead costs two waves per SIMD
// of occupancy and measured slower: C1 insert 0.26 -> 0.32 ms).  Each key of <= 7 bytes is packed with its length into
// one word, and the LDS probe compares the packed words against a side array beside the table —
// the representative row is read only by the lane that claims a slot (for the group hash the HBM
// entry needs).
//
// Decimal SUM / AVG arguments of precision p with rows_per_block * 10^p < 2^63 (`narrow`, bit per
// aggregate) accumulate in the low state word alone, as a signed 64-bit partial (no carry, so a
// non-returning LDS add instead of add128's returning add + dependent high add); before the flush
// the high word is set to the partial's sign.  Slots are therefore either "short" (claimed here,
// packed keys in the side array, narrow representation) or "generic" (claimed by the fallback
// for longer keys or a full probe, marked PK_GEN, standard representation); each path matches only
// its own slots, so the two never mix (a key may hold a slot of each: the flush merges them).
// The end-of-block flush is the generic one.
// ------------------------------------------------------------------------------------------
#define SHORT_MAXA 8
#define PK_NONE (~0ULL)
#define PK_GEN (~0ULL - 1)
typedef __attribute__((address_space(3))) u64 lds_u64;
typedef volatile __attribute__((address_space(3))) u64 vlds_u64;
typedef volatile __attribute__((address_space(3))) u32 vlds_u32;
struct ShortRow {
    u64 o[4];               // key offsets [k0 begin, k0 end, k1 begin, k1 end]
    u64 lo[SHORT_MAXA];     // argument low words (or the whole value)
    u64 hi[SHORT_MAXA];     // Decimal128 high words of wide sums
};
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(6))) agg_insert_short_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                                u32 bid, u64 rows, u64 rows_per_block, TableDesc t, u32 lds_slots,
                                                                u32 rep_mask, int xmode, u32 narrow, u64* trace) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    // EXPERIMENT (TRACE=1 builds, DBG_X_TRACE_SHORT): [0] first workgroup start, [1] / [2] first /
    // last row loop end, [3] last flush start, [4] last workgroup end (s_memrealtime, 100 MHz)
    auto tmark = [&](int k, bool mx) {
        if (kPhaseTrace && trace && threadIdx.x == 0) {
            const unsigned long long v = __builtin_amdgcn_s_memrealtime();
            if (mx) atomicMax((unsigned long long*)trace + k, v);
            else atomicMin((unsigned long long*)trace + k, v);
        }
    };
    tmark(0, false);
    const Spec& S = *spec;
    const BatchDesc& B = batches[bid];
    const u32 sw = S.stride_words;
    u32* lcount = (u32*)(lds + (u64)lds_slots * sw);  // [0] lds claims, [1] hbm claims, [2..3] flush
    u64* pk0 = lds + (u64)lds_slots * sw + 4;          // packed keys of short slots (PK_NONE / PK_GEN)
    u64* pk1 = pk0 + lds_slots;
    const u32 lmask = lds_slots - 1;
    const u32 llimit = lds_slots - lds_slots / 4;
    lds_table_init<false>(S, lds, lds_slots, sw, BLOCK);
    for (u32 j = threadIdx.x; j < lds_slots; j += BLOCK) pk0[j] = pk1[j] = PK_NONE;
    if (threadIdx.x < 8) lcount[threadIdx.x] = 0;
    __syncthreads();
    const u64 r0 = (u64)blockIdx.x * rows_per_block;
    const u64 r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    u32 my_claims = 0;
    const int nk = S.n_keys;
    const int na = S.n_aggs;
    vlds_u32* lc = (vlds_u32*)lcount;
    auto fetch = [&](u64 i, ShortRow& r) __attribute__((always_inline)) {
        r.o[0] = gld<u64>(B.keys[0].offsets + i);
        r.o[1] = gld<u64>(B.keys[0].offsets + i + 1);
        r.o[2] = r.o[3] = 0;
        if (nk > 1) {
            r.o[2] = gld<u64>(B.keys[1].offsets + i);
            r.o[3] = gld<u64>(B.keys[1].offsets + i + 1);
        }
#pragma unroll
        for (int a = 0; a < SHORT_MAXA; ++a) {
            r.lo[a] = r.hi[a] = 0;
            if (a < na && S.aggs[a].arg_type >= 0 && S.aggs[a].kind != DBG_AGG_COUNT) {
                r.lo[a] = dcol_bits(B.args[a], i);
                if (S.aggs[a].sumk == SUMK_I128 && !((narrow >> a) & 1)) r.hi[a] = dcol_hi(B.args[a], i);
            }
        }
    };
    // the fallback: a generic slot (PK_GEN) of this workgroup's table, else the HBM table
    auto generic_row = [&](u64 i) __attribute__((always_inline)) {
        const u64 h = group_hash(B.keys, nk, i);
        const u64 key = (h & 0xFFFF000000000000ULL) | ((u64)bid << 32) | i;
        u32 s = (u32)((h >> 16) & lmask);
        const int cap = *lc >= llimit ? 2 : LDS_PROBE_CAP;
        int ls = -1;
        for (int p = 0; p < cap; ++p) {
            wptr<AS_LDS> e = asp<AS_LDS>(lds + (u64)s * sw);
            u64 ev = vld<AS_LDS>(e);
            if (ev == SLOT_EMPTY) {
                if (*lc >= llimit) break;
                const u64 old = at_cas<AS_LDS>(e, SLOT_EMPTY, key);
                if (old == SLOT_EMPTY) {
                    ((vlds_u64*)pk0)[s] = PK_GEN;
                    __hip_atomic_fetch_add((__attribute__((address_space(3))) u32*)lcount, 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                    ls = (int)s;
                    break;
                }
                ev = old;
            }
            // a slot whose marker is not written yet reads as not generic: at worst a second slot
            if (((vlds_u64*)pk0)[s] == PK_GEN && (ev >> 48) == (key >> 48) && ref_equal(S, batches, B.keys, i, ev)) {
                ls = (int)s;
                break;
            }
            s = (s + 1) & lmask;
        }
        if (ls >= 0) {
            apply_row<AS_LDS, true, false>(S, asp<AS_LDS>(lds + (u64)ls * sw), B, i, batches, bid);  // no Decimal256 (short_eligible)
            return;
        }
        bool claimed;
        const u64 gs = g_find<false>(S, batches, B.keys, i, key, h, t, t.probe_limit, claimed);
        if (gs == ~0ULL) {
            push_ovf_row(t, bid, i);
            return;
        }
        my_claims += claimed ? 1 : 0;
        apply_row<AS_GLB, true, false>(S, asp<AS_GLB>(t.slots + gs * t.stride_words), B, i, batches, bid);
    };
    auto process = [&](u64 i, const ShortRow& r) __attribute__((always_inline)) {
        const u64 l0 = r.o[1] - r.o[0], l1 = r.o[3] - r.o[2];
        const bool shortk = l0 <= 7 && l1 <= 7;
        // key bytes and the predicate's column: issued together, one wait
        u64 b0 = 0, b1 = 0;
        if (shortk && l0) b0 = load_partial(B.keys[0].data + r.o[0], l0);
        if (shortk && l1) b1 = load_partial(B.keys[1].data + r.o[2], l1);
        const bool pass = B.n_nodes == 0 || eval_pred(B.nodes, B.n_nodes, B.fcols, i);
        if (!pass) return;
        // timing ablation (EXP=1 builds only): the loads and the predicate alone (no probe, adds
        // or flush); the key bytes stay live through an improbable compare
        if (kExperiments && xmode == 5 && (b0 ^ b1) != 0x5A5A5A5A5A5A5A5AULL) return;
        if (!shortk) {
            generic_row(i);
            return;
        }
        const u64 k0 = (l0 << 56) | (b0 & width_mask((u32)l0));
        u64 k1 = nk > 1 ? ((l1 << 56) | (b1 & width_mask((u32)l1))) : 0;
        if (rep_mask && *lc < lds_slots / 8)
            k1 |= (u64)((threadIdx.x & rep_mask) + 1) << 59;  // a replica of the key's slot: fewer lanes per LDS address
        u32 pos = (u32)slot_mix(k0 ^ slot_mix(k1)) & lmask;
        int ls = -1;
        for (int p = 0; p < LDS_PROBE_CAP; ++p) {
            wptr<AS_LDS> e = asp<AS_LDS>(lds + (u64)pos * sw);
            u64 ev = vld<AS_LDS>(e);
            if (ev == SLOT_EMPTY) {
                if (*lc >= llimit) break;  // full: the generic path
                const u64 h = group_hash(B.keys, nk, i);
                const u64 key = (h & 0xFFFF000000000000ULL) | ((u64)bid << 32) | i;
                const u64 old = at_cas<AS_LDS>(e, SLOT_EMPTY, key);
                if (old == SLOT_EMPTY) {
                    ((vlds_u64*)pk0)[pos] = k0;
                    ((vlds_u64*)pk1)[pos] = k1;
                    __hip_atomic_fetch_add((__attribute__((address_space(3))) u32*)lcount, 1u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                    ls = (int)pos;
                    break;
                }
                ev = old;
            }
            // packed keys not written yet (or a generic slot) do not match: at worst a second slot
            if (((vlds_u64*)pk0)[pos] == k0 && ((vlds_u64*)pk1)[pos] == k1) {
                ls = (int)pos;
                break;
            }
            pos = (pos + 1) & lmask;
        }
        if (ls < 0) {
            generic_row(i);
            return;
        }
        if (kExperiments && (xmode == 2 || xmode == 4)) return;  // timing ablation (EXP=1 builds only)
        wptr<AS_LDS> st = asp<AS_LDS>(lds + (u64)ls * sw);
#pragma unroll
        for (int a = 0; a < SHORT_MAXA; ++a) {
            if (a >= na) break;
            const DAgg& A = S.aggs[a];
            wptr<AS_LDS> w = st + A.w0;
            if (A.kind == DBG_AGG_COUNT) {
                at_add<AS_LDS>(w, 1ULL);
                continue;
            }
            if (A.sumk == SUMK_I64) {
                u64 v = r.lo[a];
                switch (A.arg_type) {
                    case DBG_INT8: v = (u64)(i64)(int8_t)v; break;
                    case DBG_INT16: v = (u64)(i64)(int16_t)v; break;
                    case DBG_INT32: case DBG_DATE: v = (u64)(i64)(int32_t)v; break;
                    default: break;
                }
                at_add<AS_LDS>(w, v);
            } else if (A.sumk == SUMK_F64) {
                at_addf<AS_LDS>(w, A.arg_type == DBG_FLOAT32 ? (double)__uint_as_float((u32)r.lo[a]) : __longlong_as_double((long long)r.lo[a]));
            } else if ((narrow >> a) & 1) {
                at_add<AS_LDS>(w, r.lo[a]);  // signed 64-bit partial, widened before the flush
            } else {
                add128<AS_LDS>(w, r.lo[a], r.hi[a]);
            }
            if (A.kind == DBG_AGG_AVG) at_add<AS_LDS>(w + (A.sumk == SUMK_I128 ? 2 : 1), 1ULL);
        }
    };
    for (u64 i = r0 + threadIdx.x; i < r1; i += BLOCK) {
        ShortRow cur;
        fetch(i, cur);
        process(i, cur);
    }
    __syncthreads();
    tmark(1, false);
    tmark(2, true);
    if (kExperiments && xmode >= 3) return;  // timing ablation (EXP=1 builds only: no flush)
    if (narrow) {  // short slots: narrow partials -> Decimal128 state (high word = sign)
        for (u32 s = threadIdx.x; s < lds_slots; s += BLOCK) {
            const u64 pk = pk0[s];
            if (pk == PK_NONE || pk == PK_GEN) continue;
            u64* st = lds + (u64)s * sw;
            for (int a = 0; a < na; ++a)
                if ((narrow >> a) & 1) st[S.aggs[a].w0 + 1] = (u64)((i64)st[S.aggs[a].w0] >> 63);
        }
        __syncthreads();
    }
    tmark(3, true);
    block_flush<false, false, true, false>(S, batches, B, lds, lds_slots, sw, lcount, BLOCK, t, my_claims);
    tmark(4, true);
}

// host: the short-key specialisation applies (hb = host copy of the batch descriptor)
static bool short_eligible(const Spec& S, const BatchDesc& hb) {
    if (S.inline_keys || S.n_keys < 1 || S.n_keys > 2 || S.n_aggs > SHORT_MAXA || S.flags_word >= 0 || hb.is_records) return false;
    for (int c = 0; c < S.n_keys; ++c)
        if (S.key_types[c].type != DBG_STRING || S.key_types[c].nullable || hb.keys[c].layout != LAYOUT_ARROW) return false;
    for (int a = 0; a < S.n_aggs; ++a) {
        const DAgg& A = S.aggs[a];
        if (A.kind != DBG_AGG_COUNT && A.kind != DBG_AGG_SUM && A.kind != DBG_AGG_AVG) return false;
        if (A.arg_type >= 0 && A.arg_nullable) return false;
        if (A.arg_type == DBG_DECIMAL256) return false;  // compiled without the 256-bit updates: the generic insert
    }
    return true;
}

// EXPERIMENT (TRACE=1 builds, DBG_X_TRACE_SHORT): the phase-trace ring of the short-key insert, 8
// words per launch and 4096 launches, its medians dumped at exit.  Returns this launch's entry,
// initialised on `s` (nullptr: tracing is off).
static u64* exp_short_trace(hipStream_t s) {
    if (!(kPhaseTrace && X_ENV("DBG_X_TRACE_SHORT"))) return nullptr;
    static u64* buf = nullptr;
    static u32 launch = 0;
    static const u64 init[8] = {~0ULL, ~0ULL, 0, 0, 0, 0, 0, 0};
    if (!buf) {
        if (hipMalloc((void**)&buf, 4096 * 64) != hipSuccess) buf = nullptr;
        if (buf) hipMemset(buf, 0, 4096 * 64);
        atexit([] {
            std::vector<u64> hb(4096 * 8);
            (void)hipDeviceSynchronize();
            (void)hipMemcpy(hb.data(), buf, hb.size() * 8, hipMemcpyDeviceToHost);
            std::vector<std::vector<double>> d(4);
            for (int k = 0; k < 4096; ++k) {
                const u64* r = &hb[k * 8];
                if (r[0] == 0 || r[0] == ~0ULL || r[4] == 0) continue;
                for (int p = 1; p <= 4; ++p) d[p - 1].push_back((double)(r[p] - r[0]) * 0.01);
            }
            const char* nm[] = {"first row loop end", "last row loop end", "last flush start", "last workgroup end"};
            for (int p = 0; p < 4; ++p) {
                if (d[p].empty()) continue;
                std::sort(d[p].begin(), d[p].end());
                fprintf(stderr, "short trace %-20s median %7.2f us  (n=%zu)\n", nm[p], d[p][d[p].size() / 2], d[p].size());
            }
        });
    }
    if (!buf) return nullptr;
    u64* x_tr = buf + (u64)(launch++ & 4095) * 8;
    (void)hipMemcpyAsync(x_tr, init, sizeof(init), hipMemcpyHostToDevice, s);
    return x_tr;
}

static InsertPath launch_insert_short(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, u32 bid, u64 rows,
                                      bool records, const TableDesc& t, bool use_lds, const BatchDesc* hb) {
    static const int x_short = X_ENV("DBG_X_SHORT") ? atoi(X_ENV("DBG_X_SHORT")) : 1;
    static const u32 x_rep = X_ENV("DBG_X_SHORT_REP") ? (u32)atoi(X_ENV("DBG_X_SHORT_REP")) : 0;
    const bool x_noshort = x_short == 0;
    // low cardinality only: with a table already sized for many groups (the cardinality probe, or
    // earlier batches) most rows miss the workgroup's LDS table, and the generic kernel's queued
    // HBM path serves those far better than this kernel's per-row fallback (C5: 31 vs 95 ms)
    const bool mine = !records && use_lds && hb && !x_noshort && t.cap + 1 <= SHORT_MAX_SLOTS && short_eligible(S, *hb);
    if (!mine) return INS_NONE;
    const u32 lslots = lds_slots_for(S, LDS_BUDGET_BYTES);
    static const u64 x_blocks = X_ENV("DBG_X_SHORT_BLOCKS") ? (u64)atoll(X_ENV("DBG_X_SHORT_BLOCKS")) : 0;
    u64 rpb;
    const u32 blocks = row_range_grid(rows, (u64)BLOCK * 16, rpb, false, x_blocks);  // EXPERIMENT: grid size
    const size_t shmem = (size_t)lslots * S.stride_words * 8 + 32 + (size_t)lslots * 16;
    // narrow Decimal sums: rows_per_block * 10^p < 2^63 (a workgroup's partial fits in i64)
    u32 narrow = 0;
    for (int a = 0; a < S.n_aggs; ++a) {
        const DAgg& A = S.aggs[a];
        if (A.sumk != SUMK_I128 || A.kind == DBG_AGG_COUNT || A.arg_type != DBG_DECIMAL128) continue;
        const int p = hb->args[a].precision;
        double lim = 1.0;
        for (int k = 0; k < p; ++k) lim *= 10.0;
        if (p > 0 && p <= 18 && lim * (double)rpb < 9.0e18) narrow |= 1u << a;
    }
    static const bool x_wide = X_ENV("DBG_X_NARROW") && X_ENV("DBG_X_NARROW")[0] == '0';
    if (x_wide) narrow = 0;
    hipLaunchKernelGGL(agg_insert_short_kernel, dim3(blocks), dim3(BLOCK), shmem, s, dspec, batches, bid, rows, rpb, t, lslots,
                       x_rep ? x_rep - 1 : 0u, x_short, narrow, exp_short_trace(s));
    return INS_SHORT;
}

// ------------------------------------------------------------------------------------------
// Deferred overflow: rows (bid,row) and partial records [entry][words] re-inserted after growth.
// ------------------------------------------------------------------------------------------
template <bool INLINE>
__global__ void __launch_bounds__(BLOCK) agg_retry_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                         TableDesc t, u64 n_rows, u64 n_recs, const u64* rows_list,
                                                         const u64* recs_list) {
    const Spec& S = *spec;
    u64 total = n_rows + n_recs;
    for (u64 k = blockIdx.x * (u64)BLOCK + threadIdx.x; k < total; k += (u64)gridDim.x * BLOCK) {
        bool claimed;
        u64 gs;
        if (k < n_rows) {
            u64 it = rows_list[k];
            u32 bid = (u32)(it >> 32);
            u64 i = (u32)it;
            const BatchDesc& B = batches[bid];
            u64 h, key;
            if (B.is_records) h = gld<u64>(B.rec_base + i * (u64)B.rec_width);
            else h = INLINE ? 0 : group_hash(B.keys, S.n_keys, i);
            key = INLINE ? pack_key(S, B.keys, i) : ((h & 0xFFFF000000000000ULL) | ((u64)bid << 32) | i);
            gs = g_find<INLINE>(S, batches, B.keys, i, key, h, t, (u32)(t.cap < 0xFFFFFFFFull ? t.cap : 0xFFFFFFFFull), claimed);
            if (gs == ~0ULL) {
                atomicOr((unsigned long long*)(t.counters + CNT_ERR), (unsigned long long)ERR_OVF_LOST);
                continue;
            }
            wptr<AS_GLB> st = asp<AS_GLB>(t.slots + gs * t.stride_words);
            if (B.is_records) apply_state<AS_GLB>(S, st, (const u64*)(B.rec_base + i * (u64)B.rec_width + S.rec_state_off) - 1, batches);
            else apply_row<AS_GLB>(S, st, B, i, batches, bid);
        } else {
            const u64* r = recs_list + (k - n_rows) * t.stride_words;
            u64 key = r[0];
            if (INLINE && key == SLOT_EMPTY) continue;  // consumed by part_fixup (never a record key)
            u64 h = 0;
            if (!INLINE) {
                const BatchDesc& B = batches[ref_bid(key)];
                h = B.is_records ? gld<u64>(B.rec_base + (u64)ref_row(key) * B.rec_width) : group_hash(B.keys, S.n_keys, ref_row(key));
            }
            gs = g_find_entry<INLINE>(S, batches, key, h, t, (u32)(t.cap < 0xFFFFFFFFull ? t.cap : 0xFFFFFFFFull), claimed);
            if (gs == ~0ULL) {
                atomicOr((unsigned long long*)(t.counters + CNT_ERR), (unsigned long long)ERR_OVF_LOST);
                continue;
            }
            apply_state<AS_GLB>(S, asp<AS_GLB>(t.slots + gs * t.stride_words), r, batches);
        }
        if (claimed) atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), 1ULL);
    }
}

void launch_retry(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, const TableDesc& t, u64 n_rows,
                  u64 n_recs, const u64* rows_list, const u64* recs_list) {
    u64 total = n_rows + n_recs;
    if (!total) return;
    u64 blocks = (total + BLOCK - 1) / BLOCK;
    if (blocks > 4096) blocks = 4096;
    if (S.inline_keys)
        hipLaunchKernelGGL(agg_retry_kernel<true>, dim3((u32)blocks), dim3(BLOCK), 0, s, dspec, batches, t, n_rows, n_recs, rows_list, recs_list);
    else
        hipLaunchKernelGGL(agg_retry_kernel<false>, dim3((u32)blocks), dim3(BLOCK), 0, s, dspec, batches, t, n_rows, n_recs, rows_list, recs_list);
}

// ------------------------------------------------------------------------------------------
// Rehash into a larger table (groups are distinct: claim the first empty slot, copy the words).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) agg_rehash_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                          const u64* old_slots, u64 old_cap, TableDesc t) {
    const Spec& S = *spec;
    u64 sw = t.stride_words;
    u64 mask = t.cap - 1;
    for (u64 s = blockIdx.x * (u64)BLOCK + threadIdx.x; s <= old_cap; s += (u64)gridDim.x * BLOCK) {
        const u64* o = old_slots + s * sw;
        u64 e = o[0];
        if (e == SLOT_EMPTY) continue;
        u64 ns;
        if (s == old_cap) {
            ns = t.cap;  // sentinel slot
        } else {
            u64 h = S.inline_keys ? 0 : entry_hash(S, batches, e, false);
            ns = (S.inline_keys ? slot_mix(e) : (h >> 16)) & mask;
            for (;;) {
                u64 old = atomicCAS((unsigned long long*)(t.slots + ns * sw), SLOT_EMPTY, (unsigned long long)e);
                if (old == SLOT_EMPTY) break;
                ns = (ns + 1) & mask;
            }
        }
        u64* d = t.slots + ns * sw;
        if (s == old_cap) d[0] = e;
        for (u64 w = 1; w < sw; ++w) d[w] = o[w];
    }
}

void launch_rehash(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, const u64* old_slots, u64 old_cap,
                   const TableDesc& t) {
    u64 blocks = (old_cap + 1 + BLOCK - 1) / BLOCK;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(agg_rehash_kernel, dim3((u32)blocks), dim3(BLOCK), 0, s, dspec, batches, old_slots, old_cap, t);
}

// ------------------------------------------------------------------------------------------
// The hand-offs by which the last workgroup of an agg_insert_fast launch finalizes the table.
// ------------------------------------------------------------------------------------------
#include "agg_chain.hpp"

// ------------------------------------------------------------------------------------------
// agg_insert_fast: one non-null integer key column, optional `key <cmp> constant` predicate on
// that same column (GROUP BY x WHERE x <> c: ClickBench Q8; or no predicate: Q16).  Streams the
// key column with 16-byte loads (FAST_UNROLL per lane per grid round, the next round's issued
// before this one is filtered), evaluates the predicate on every value, and stages the selected
// rows in the LDS table exactly like agg_insert.
// ------------------------------------------------------------------------------------------
#ifndef FAST_UNROLL
// 16-byte loads per lane and round: C2 kernel (200 steps, three alternating rounds,
// scripts/gpu_c2_variants.sh) 1 / 2 / 3 / 4 / 8 -> 45.5 / 40.6 / 41.9 / 43.4 / 55 us: two rounds
// of two in flight keep each wave's window of the column to 2 x 2 grid strides
#define FAST_UNROLL 2
#endif
typedef unsigned int v4u __attribute__((ext_vector_type(4)));
// Column data reached through a descriptor is a generic pointer to the compiler, which then
// emits flat loads: those count against lgkmcnt too and retire out of order, so every LDS wait
// (and every use of a loaded value) drains ALL loads in flight and the prefetch pipeline
// collapses.  Streams read through this address-space-1 view compile to global_load.
typedef const v4u __attribute__((address_space(1)))* gv4p;

template <typename T>
__device__ __forceinline__ bool fast_pred(T v, int op, i64 c) {
    // the constant is in the column's domain (signed / unsigned by T)
    T k = (T)c;
    switch (op) {
        case DBG_CMP_EQ: return v == k;
        case DBG_CMP_NE: return v != k;
        case DBG_CMP_LT: return v < k;
        case DBG_CMP_LE: return v <= k;
        case DBG_CMP_GT: return v > k;
        default: return v >= k;
    }
}

// Element j of a 16-byte vector viewed as T[16 / sizeof(T)], from registers (no address taken).
template <typename T>
__device__ __forceinline__ T vget(const v4u& y, int j) {
    constexpr int W = sizeof(T);
    if constexpr (W == 8) {
        u32 lo = j ? y.z : y.x, hi = j ? y.w : y.y;
        return (T)(((u64)hi << 32) | lo);
    } else {
        int wi = (j * W) >> 2;
        u32 word = wi == 0 ? y.x : (wi == 1 ? y.y : (wi == 2 ? y.z : y.w));
        return (T)(word >> (((j * W) & 3) * 8));
    }
}

// Selected rows are appended to a per-wave LDS queue (ballot + mbcnt) and staged 64 at a time
// with every lane active: at low selectivity (Q8: 0.63 %) a lane-divergent insert per row would
// leave 63 of 64 lanes idle on every LDS round trip.
#define WQ 128  // queue entries per wave
#define WQW 384  // u64 words of per-wave queue space: rows (2 x WQ) or candidate vectors (WQ x (16 + 8) B)

template <typename T, bool PRED, int NT, bool CO>
__global__ void __launch_bounds__(NT) agg_insert_fast_kernel(const Spec* __restrict__ spec, const BatchDesc* __restrict__ batches,
                                                               u32 bid, u64 rows, TableDesc t, u32 lds_slots,
                                                               T lo, T hi, int negate, FusedFin ff, const void* key0,
                                                               u32 stride_words) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    constexpr int V = 16 / sizeof(T);
    const Spec& S = *spec;
    const BatchDesc& B = batches[bid];
    // The key column's base (B.keys[0].data) and S.stride_words come by value: the stream's first
    // loads then depend on the kernel arguments alone, not on two cold descriptor reads.
    const T* __restrict__ col = (const T*)key0;
    const u32 sw = stride_words;
    u32* lcount = (u32*)(lds + (u64)lds_slots * sw);
    const u32 lmask = lds_slots - 1;
    const u32 llimit = lds_slots - lds_slots / 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // per-wave queue (keys and rows) after the table and its 16 bytes of counters
    u64* qkey = lds + (u64)lds_slots * sw + 2 + (u64)wave * WQW;
    u64* qrow = qkey + WQ;
    // candidate-vector queue (the `<> c` path below) over the same per-wave space
    v4u* vq = (v4u*)qkey;
    u64* vqb = qkey + 2 * WQ;
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) atomicMin((unsigned long long*)ff.trace, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    // Grid-strided stream (all waves of the chip sweep one window of the column together: DRAM
    // rows stay open, scripts/micro/stream.hip): FAST_UNROLL unconditional 16-byte loads per lane
    // per round (an index past the end is clamped and its lane-slot masked off), so no branch
    // sits around the loads; other waves of the CU keep HBM busy while one filters.
    const u64 nvec = rows / V;
    gv4p vp = (gv4p)col;
    const u64 gstride = (u64)gridDim.x * NT;
    u64 k = (u64)blockIdx.x * NT + threadIdx.x;
    const u64 step = (u64)FAST_UNROLL * gstride;
    const u64 lastv = nvec ? nvec - 1 : 0;
    // The first round's loads go out before the LDS table is initialised: they need nothing but
    // the kernel arguments, and the barrier below waits for LDS only, so they stay in flight
    // across the initialisation (one memory trip earlier on every CU's hand-over between launches).
    v4u y[FAST_UNROLL];
#pragma unroll
    for (int u = 0; u < FAST_UNROLL; ++u) {
        u64 idx = k + u * gstride;
        y[u] = __builtin_nontemporal_load(vp + (idx < nvec ? idx : lastv));
    }
    lds_table_init<false>(S, lds, lds_slots, sw, NT);
    if (threadIdx.x < 4) lcount[threadIdx.x] = 0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // LDS only: the loads above stay in flight
    u32 my_claims = 0;
    u32 my_ovf = 0;  // overflow rows pushed (the fused chain reports them through its tickets)

    // predicate in range form: lo <= v <= hi, xor negate (host maps =, <>, <, <=, >, >=)
    auto pass = [&](T v) -> bool { return ((v >= lo) & (v <= hi)) ^ (negate != 0); };

    // stage one selected row (key bits, row index) — all callers have full or near-full lanes
    auto process = [&](u64 key, u64 i) {
        int ls = lds_find<true>(S, batches, nullptr, i, key, 0, lds, lmask, sw, lcount, llimit);
        if (ls >= 0) {
            wptr<AS_LDS> st = asp<AS_LDS>(lds + (u64)ls * sw);
            if (CO) at_add<AS_LDS>(st + 1, 1ULL);
            else apply_row<AS_LDS, false, false>(S, st, B, i, batches, bid);
            return;
        }
        bool claimed;
        u64 gs = g_find<true>(S, batches, nullptr, i, key, 0, t, t.probe_limit, claimed);
        if (gs == ~0ULL) {
            push_ovf_row(t, bid, i);
            my_ovf++;
            return;
        }
        my_claims += claimed ? 1 : 0;
        wptr<AS_GLB> gst = asp<AS_GLB>(t.slots + gs * t.stride_words);
        if (CO) at_add<AS_GLB>(gst + 1, 1ULL);
        else apply_row<AS_GLB, false, false>(S, gst, B, i, batches, bid);
    };

    u32 qn = 0;  // wave-uniform queue length
    auto drain64 = [&]() {  // process entries [0, 64), shift [64, qn) down
        vwptr<AS_LDS> qk = (vwptr<AS_LDS>)qkey, qr = (vwptr<AS_LDS>)qrow;
        u64 k = qk[lane], r = qr[lane];
        u64 k2 = 0, r2 = 0;
        bool mv = lane + 64 < (int)qn;
        if (mv) {
            k2 = qk[lane + 64];
            r2 = qr[lane + 64];
        }
        __builtin_amdgcn_wave_barrier();
        if (mv) {
            qk[lane] = k2;
            qr[lane] = r2;
        }
        __builtin_amdgcn_wave_barrier();
        qn -= 64;
        process(k, r);
    };

    // `key <> c` (ClickBench Q8: AdvEngineID <> 0) as a two-level compaction.  A row-level
    // queue pays the per-row mask + ballot-prefix VALU work on every lane (SQ counters: ~350
    // VALU per 32-row round, VALU ~60 % busy); instead each 16-byte vector is tested whole —
    // "some element differs from c" is three ORs of XORs — and only candidate vectors (4.9 % at
    // Q8's selectivity) are appended, whole, to a per-wave LDS queue; 64 at a time they are
    // expanded with every lane busy.  ~10 VALU per 8-row vector instead of ~90.
    const bool neq_fast = PRED && negate && lo == hi;
    u32 cc_lo, cc_hi;
    {
        typedef typename std::make_unsigned<T>::type UT;
        const u64 c = (u64)(UT)lo;
        if (sizeof(T) == 8) { cc_lo = (u32)c; cc_hi = (u32)(c >> 32); }
        else if (sizeof(T) == 4) { cc_lo = cc_hi = (u32)c; }
        else if (sizeof(T) == 2) { cc_lo = cc_hi = (u32)(c | (c << 16)); }
        else { cc_lo = cc_hi = (u32)(c * 0x01010101u); }
    }
    u32 vqn = 0;  // wave-uniform candidate count
    // expand candidate vectors [0, n) (n <= 64, one per lane), shift [64, vqn) down
    auto drain_vec = [&](u32 n) {
        v4u v = {0, 0, 0, 0};
        u64 bs = 0;
        const bool have = lane < (int)n;
        if (have) {
            v = ((volatile v4u*)vq)[lane];
            bs = ((volatile u64*)vqb)[lane];
        }
        const bool mv = lane + 64 < (int)vqn;
        v4u v2 = {0, 0, 0, 0};
        u64 b2 = 0;
        if (mv) {
            v2 = ((volatile v4u*)vq)[lane + 64];
            b2 = ((volatile u64*)vqb)[lane + 64];
        }
        __builtin_amdgcn_wave_barrier();
        if (mv) {
            ((volatile v4u*)vq)[lane] = v2;
            ((volatile u64*)vqb)[lane] = b2;
        }
        __builtin_amdgcn_wave_barrier();
        vqn -= n;
        u32 mm = 0;
        if (have)
#pragma unroll
            for (int j = 0; j < V; ++j) mm |= (pass(vget<T>(v, j)) ? 1u : 0u) << j;
        while (mm) {
            const int j = __builtin_ctz(mm);
            mm &= mm - 1;
            // element j of v from registers (j is lane-varying here): select over the dwords
            const int W = (int)sizeof(T);
            const int wi = (j * W) >> 2;
            const u32 w0 = wi == 0 ? v.x : (wi == 1 ? v.y : (wi == 2 ? v.z : v.w));
            u64 key;
            if (W == 8) {
                const u32 w1 = wi == 0 ? v.y : v.w;
                key = ((u64)w1 << 32) | w0;
            } else {
                const u32 sh = (u32)((j * W) & 3) * 8;
                key = (u64)((w0 >> sh) & (W == 4 ? 0xFFFFFFFFu : ((1u << (8 * W)) - 1u)));
            }
            process(key, bs + j);
        }
    };
    const u64 ltmask = (1ULL << lane) - 1;
    auto key_of = [&](const v4u& y, int j) -> u64 { return (u64)(typename std::make_unsigned<T>::type)vget<T>(y, j); };
    // Stage the selected rows of a group of NV vectors (one per lane and slot u), all lanes
    // together.  A lane's vector slots hold rows base[u] .. base[u] + V - 1.
    auto handle_group = [&](const v4u* y, const u64* base, int nv, u32 actm) {
        if (!PRED) {
            for (int u = 0; u < nv; ++u)
                if ((actm >> u) & 1)
#pragma unroll
                    for (int j = 0; j < V; ++j) process(key_of(y[u], j), base[u] + j);
            return;
        }
        if (neq_fast) {
#pragma unroll
            for (int u = 0; u < FAST_UNROLL; ++u) {
                const v4u& v = y[u];
                const bool any = (((v.x ^ cc_lo) | (v.y ^ cc_hi) | (v.z ^ cc_lo) | (v.w ^ cc_hi)) != 0) && ((actm >> u) & 1);
                const u64 b = __ballot(any);
                if (b == 0) continue;
                if (any) {
                    const u32 pos = vqn + (u32)__popcll(b & ltmask);
                    vq[pos] = v;
                    vqb[pos] = base[u];
                }
                vqn += (u32)__popcll(b);
                if (vqn >= 64) {
                    __builtin_amdgcn_wave_barrier();
                    drain_vec(64);
                }
            }
            return;
        }
        u32 m[FAST_UNROLL];
        u32 cnt = 0;
#pragma unroll
        for (int u = 0; u < FAST_UNROLL; ++u) {
            m[u] = 0;
            if (u < nv) {
#pragma unroll
                for (int j = 0; j < V; ++j) m[u] |= (pass(vget<T>(y[u], j)) ? 1u : 0u) << j;
            }
            if (!((actm >> u) & 1)) m[u] = 0;
            cnt += __popc(m[u]);
        }
        if (__ballot(cnt != 0) == 0) return;
        // exclusive prefix and wave total of cnt (<= 32 = 6 bits) from one ballot per bit
        u32 pre = 0, tot = 0;
#pragma unroll
        for (int bb = 0; bb < 6; ++bb) {
            u64 bal = __ballot((cnt >> bb) & 1);
            pre += (u32)__popcll(bal & ltmask) << bb;
            tot += (u32)__popcll(bal) << bb;
        }
        if (qn + tot <= WQ) {
            u32 pos = qn + pre;
#pragma unroll
            for (int u = 0; u < FAST_UNROLL; ++u) {
                u32 mm = m[u];
                while (mm) {
                    int j = __builtin_ctz(mm);
                    mm &= mm - 1;
                    qkey[pos] = key_of(y[u], j);
                    qrow[pos] = base[u] + j;
                    pos++;
                }
            }
            qn += tot;
            while (qn >= 64) {
                __builtin_amdgcn_wave_barrier();
                drain64();
            }
        } else {  // dense selection: lanes already busy, insert directly
#pragma unroll
            for (int u = 0; u < FAST_UNROLL; ++u) {
                u32 mm = m[u];
                while (mm) {
                    int j = __builtin_ctz(mm);
                    mm &= mm - 1;
                    process(key_of(y[u], j), base[u] + j);
                }
            }
        }
    };

    // Software pipeline: the next round's FAST_UNROLL loads are issued before this round is
    // filtered and queued (the first round's went out before the table's initialisation), so a
    // wave busy with its ballots and LDS queue writes still has 64 B/lane in flight (without it
    // the per-round processing sits on the load critical path).  The loop condition is
    // wave-uniform (ballot) because the queue needs all 64 lanes.
    while (__ballot(k < nvec) != 0) {
        const u64 kn = k + step;
        v4u yn[FAST_UNROLL];
#pragma unroll
        for (int u = 0; u < FAST_UNROLL; ++u) {
            u64 idx = kn + u * gstride;
            yn[u] = __builtin_nontemporal_load(vp + (idx < nvec ? idx : lastv));
        }
        u64 bases[FAST_UNROLL];
        u32 actm = 0;
#pragma unroll
        for (int u = 0; u < FAST_UNROLL; ++u) {
            u64 idx = k + u * gstride;
            actm |= (idx < nvec ? 1u : 0u) << u;
            bases[u] = idx * V;
        }
        handle_group(y, bases, FAST_UNROLL, actm);
#pragma unroll
        for (int u = 0; u < FAST_UNROLL; ++u) y[u] = yn[u];
        k = kn;
    }
    if (PRED && vqn) {
        __builtin_amdgcn_wave_barrier();
        drain_vec(vqn);
    }
    // drain the queue's rest (< 64 entries): lanes below qn take one each
    if (PRED && qn) {
        __builtin_amdgcn_wave_barrier();
        if (lane < (int)qn) process(((vwptr<AS_LDS>)qkey)[lane], ((vwptr<AS_LDS>)qrow)[lane]);
        qn = 0;
    }
    for (u64 i = nvec * V + (u64)blockIdx.x * NT + threadIdx.x; i < rows; i += gstride) {
        T v = gld<T>(col + i);
        if (!PRED || pass(v)) process((u64)(typename std::make_unsigned<T>::type)v, i);
    }
    __syncthreads();
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) {
        const u64 tm = __builtin_amdgcn_s_memrealtime();
        atomicMin((unsigned long long*)ff.trace + 1, (unsigned long long)tm);
        atomicMax((unsigned long long*)ff.trace + 2, (unsigned long long)tm);
    }
    if constexpr (CO && sizeof(T) <= 2) {
        if (ff.on && ff.dense && t.scratch != nullptr && gridDim.x > 1 && gridDim.x < 65536) {
            fused_dense<T>(S, batches, B, lds, lds_slots, sw, lcount, NT, t, my_claims, my_ovf, ff);
            return;
        }
    }
    if (ff.on && t.scratch != nullptr && gridDim.x > 1 && gridDim.x <= t.scr_blocks) {
        if constexpr (CO && sizeof(T) <= 2) {
            if (kChainTagged && ff.chain_tagged && lds_slots <= 4 * NT) {
                fused_chain_tagged<T>(S, batches, B, lds, lds_slots, sw, lcount, NT, t, my_claims, my_ovf, ff);
                return;
            }
        }
        fused_chain<T, CO>(S, batches, B, lds, lds_slots, sw, lcount, NT, t, my_claims, my_ovf, ff);
        return;
    }
    block_flush<true, false, false, false>(S, batches, B, lds, lds_slots, sw, lcount, NT, t, my_claims);
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) atomicMax((unsigned long long*)ff.trace + 3, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    if (ff.on) fused_finalize(S, batches, t, lds, ff);
}


bool prof_ext_events(hipEvent_t* a, hipEvent_t* b);  // abi.hip

static size_t fast_shmem(size_t table_bytes) { return table_bytes + (size_t)(1024 / 64) * WQW * 8; }
static size_t fast_table_bytes(const Spec& S) { return (size_t)lds_slots_for(S, 16 * 1024) * S.stride_words * 8 + 16; }

template <typename T>
static void launch_fast_t(hipStream_t s, const Spec* dspec, const Spec& S, const void* key0, const BatchDesc* batches, u32 bid, u64 rows,
                          const TableDesc& t, u32 lslots, size_t table_bytes, bool pred, int op, i64 c, int count_only,
                          const FusedFin* fused) {
    constexpr u64 V = 16 / sizeof(T);
    // `v <op> c` as `(lo <= v <= hi) ^ negate`, exact over T's range (constants outside it fold)
    typedef __int128 W;
    const W tmin = (W)std::numeric_limits<T>::min(), tmax = (W)std::numeric_limits<T>::max();
    const W C = std::is_signed<T>::value ? (W)c : (W)(u64)c;
    W lo = 1, hi = 0;  // empty range
    int neg = 0;
    auto all = [&]() { lo = tmin; hi = tmax; };
    switch (op) {
        case DBG_CMP_EQ: if (C >= tmin && C <= tmax) lo = hi = C; break;
        case DBG_CMP_NE: neg = 1; if (C >= tmin && C <= tmax) lo = hi = C; break;
        case DBG_CMP_LT: if (C > tmax) all(); else if (C > tmin) { lo = tmin; hi = C - 1; } break;
        case DBG_CMP_LE: if (C >= tmax) all(); else if (C >= tmin) { lo = tmin; hi = C; } break;
        case DBG_CMP_GT: if (C < tmin) all(); else if (C < tmax) { lo = C + 1; hi = tmax; } break;
        default: if (C <= tmin) all(); else if (C <= tmax) { lo = C; hi = tmax; } break;  // GE
    }
    if (lo > hi) { lo = 1; hi = 0; }  // stays empty in T (1 > 0 for every T)
    const int nt = 1024;
    static_assert(FIN_NT == 1024, "the fused finalize runs on the insert's workgroup");
    // one 1024-lane workgroup per CU (parked-row chain: 512 / 768 / 1024 / 2048 measured 52 / 55 / 63
    // / 90 us a C2 step); EXPERIMENT DBG_X_FAST_GRID for the dense hand-off, whose merge does not
    // grow with the grid
    static const u64 x_grid = X_ENV("DBG_X_FAST_GRID") ? (u64)atoll(X_ENV("DBG_X_FAST_GRID")) : 0;
    const u64 max_blocks = (x_grid && fused && fused->dense) ? x_grid : 256;
    size_t shmem = fast_shmem(table_bytes);
    FusedFin ff;
    if (fused) ff = *fused;
    else memset(&ff, 0, sizeof(ff));
    u64 quantum = V * (u64)nt * FAST_UNROLL;
    u64 blocks = (rows + quantum - 1) / quantum;
    if (blocks > max_blocks) blocks = max_blocks;
    if (blocks > DBG_INSERT_MAX_BLOCKS) blocks = DBG_INSERT_MAX_BLOCKS;
    if (blocks < 1) blocks = 1;
    // The tagged chain packs a workgroup's count of one key into CNT1_BITS: the workgroup's share
    // of the rows (its whole grid-stride rounds of nt vectors, one more round for the ragged end,
    // the scalar tail) must stay below that, or a count would carry into the tag; its readers
    // hold one item per thread, which bounds the grid.  Anything else takes the generic chain.
    static_assert(FAST_UNROLL >= 1 && V * 1024 * FAST_UNROLL < (1ULL << CNT1_BITS), "one grid round of a workgroup fits a level-1 count");
    ff.chain_tagged = blocks <= CHAIN_TAGGED_MAX_BLOCKS && rows / blocks + V * (u64)nt + V < (1ULL << CNT1_BITS);
    // profiling on: the kernel stamps the enclosing scope's events itself (abi.hip, prof_ext_events)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    const bool ext = prof_ext_events(&ev0, &ev1);
#define FAST_LAUNCH(P, N, F)                                                                                                     \
    do {                                                                                                                         \
        if (ext)                                                                                                                 \
            hipExtLaunchKernelGGL((agg_insert_fast_kernel<T, P, N, F>), dim3((u32)blocks), dim3(N), shmem, s, ev0, ev1, 0, dspec, \
                                  batches, bid, rows, t, lslots, (T)lo, (T)hi, neg, ff, key0, (u32)S.stride_words);             \
        else                                                                                                                     \
            hipLaunchKernelGGL((agg_insert_fast_kernel<T, P, N, F>), dim3((u32)blocks), dim3(N), shmem, s, dspec, batches, bid, \
                               rows, t, lslots, (T)lo, (T)hi, neg, ff, key0, (u32)S.stride_words);                               \
    } while (0)
    // CO: COUNT(*) is the only aggregate (ClickBench Q8/Q16 shape) — the kernel then carries no
    // apply_row code at all (smaller hot loop, fewer registers)
    if (count_only) {
        if (pred) FAST_LAUNCH(true, 1024, true); else FAST_LAUNCH(false, 1024, true);
    } else {
        if (pred) FAST_LAUNCH(true, 1024, false); else FAST_LAUNCH(false, 1024, false);
    }
#undef FAST_LAUNCH
}

// Host-side eligibility for the fast path (hb = host copy of the batch descriptor).
static bool fast_eligible(const Spec& S, const BatchDesc& hb, bool records) {
    if (records || !S.inline_keys || S.n_keys != 1 || S.key_types[0].nullable) return false;
    // String MIN/MAX: the kernel is compiled without that update (apply_row<AS, false>); the
    // generic insert stages and flushes such states
    for (int a = 0; a < S.n_aggs; ++a)
        if ((S.aggs[a].kind == DBG_AGG_MIN || S.aggs[a].kind == DBG_AGG_MAX) && S.aggs[a].mmk == MMK_STR) return false;
    // Decimal256 arguments likewise (apply_row<AS, false, false>, the fused finalize without the
    // four-word results)
    for (int a = 0; a < S.n_aggs; ++a)
        if (S.aggs[a].arg_type == DBG_DECIMAL256) return false;
    const DCol& k = hb.keys[0];
    int ty = k.type;
    bool intlike = (ty >= DBG_INT8 && ty <= DBG_UINT64) || ty == DBG_DATE || ty == DBG_TIMESTAMP;
    if (!intlike || k.layout != LAYOUT_ARROW || ((uintptr_t)k.data & 15)) return false;
    if (hb.n_nodes == 0) return true;
    if (hb.n_nodes != 1) return false;
    const DNode& n = hb.nodes[0];
    const DCol& f = hb.fcols[n.col];
    return n.op == DBG_PRED_CMP_CONST && f.data == k.data && f.type == ty && !f.nullable;
}

bool insert_can_fuse(const Spec& S, const BatchDesc& hb, u64 cap) {
    return hb.rows > 0 && fast_eligible(S, hb, false) && cap + 1 <= FUSED_FIN_SLOTS &&
           (cap + 1) * S.stride_words * 8 <= fast_shmem(fast_table_bytes(S));
}

static InsertPath launch_insert_fast(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, u32 bid, u64 rows,
                                     bool records, const TableDesc& t, bool use_lds, const BatchDesc* hb, const FusedFin* fused) {
    const bool mine = hb && use_lds && fast_eligible(S, *hb, records);
    if (!mine) return INS_NONE;
    u32 lslots = lds_slots_for(S, 16 * 1024);
    size_t shmem = fast_table_bytes(S);
    bool pred = hb->n_nodes == 1;
    int op = pred ? hb->nodes[0].cmp : 0;
    i64 c = pred ? hb->nodes[0].i64v : 0;
    int count_only = S.n_aggs == 1 && S.aggs[0].kind == DBG_AGG_COUNT && S.aggs[0].arg_type < 0 && S.aggs[0].w0 == 1;
    const InsertPath path = pred ? INS_FAST_PRED : INS_FAST;
#define FAST_KEY(T) \
    launch_fast_t<T>(s, dspec, S, hb->keys[0].data, batches, bid, rows, t, lslots, shmem, pred, op, c, count_only, fused); return path
    switch (hb->keys[0].type) {
        case DBG_INT8: FAST_KEY(int8_t);
        case DBG_UINT8: FAST_KEY(uint8_t);
        case DBG_INT16: FAST_KEY(int16_t);
        case DBG_UINT16: FAST_KEY(uint16_t);
        case DBG_INT32: case DBG_DATE: FAST_KEY(int32_t);
        case DBG_UINT32: FAST_KEY(uint32_t);
        case DBG_INT64: case DBG_TIMESTAMP: FAST_KEY(int64_t);
        case DBG_UINT64: FAST_KEY(uint64_t);
    }
#undef FAST_KEY
    return INS_NONE;
}

// ------------------------------------------------------------------------------------------
// launch_insert: the families are asked in the order fast, str1, short, generic.  Each takes the
// batch if it is its kind: the path launched, or INS_NONE (nothing launched).
// ------------------------------------------------------------------------------------------
InsertPath launch_insert(hipStream_t s, const Spec* dspec, const Spec& S, const BatchDesc* batches, u32 bid, u64 rows, bool records,
                         const TableDesc& t, bool use_lds, const BatchDesc* hb, const FusedFin* fused) {
    if (rows == 0) return INS_NONE;
    InsertPath p = launch_insert_fast(s, dspec, S, batches, bid, rows, records, t, use_lds, hb, fused);
    if (p == INS_NONE) p = launch_insert_str1(s, dspec, S, batches, bid, rows, records, t, use_lds, hb);
    if (p == INS_NONE) p = launch_insert_short(s, dspec, S, batches, bid, rows, records, t, use_lds, hb);
    if (p == INS_NONE) p = launch_insert_generic(s, dspec, S, batches, bid, rows, records, t, use_lds, hb);
    return p;
}
