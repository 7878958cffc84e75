// agg_chain.hpp — the cross-workgroup hand-offs of agg_insert_fast_kernel, by which the last
// workgroup of an insert launch finalizes the table: fused_finalize, the parked-row chains
// (fused_chain, fused_chain_tagged) and the direct-mapped fused_dense.  Included only by agg.hip,
// before the fast kernel, after agg_table.hpp and agg_fin_small.hpp.  File map: agg_table.hpp.
#pragma once

// The last workgroup of an insert launch finalizes the table (FusedFin).  Hand-off
// (MI355X_MICROARCH.md, inter-workgroup visibility, valid forms: agent atomics / sc1 stores on
// the producer side, the workgroup whose ticket add came last as the consumer, sc1 global loads
// of every handed-off byte): every table word of this launch was written by agent-scope atomics
// (g_find's CAS, apply_row / apply_state) and read back only by sc1 loads (g_find's volatile
// entry loads, ld_sc1 here); every wave drains its memory operations and the barrier orders
// them before lane 0's ticket add.  The last workgroup copies the table into LDS with sc1 loads
// and runs the finalize_small body on the copy (recycle re-initialises t.slots directly).
__device__ __forceinline__ void fused_finalize(const Spec& S, const BatchDesc* batches, const TableDesc& t, u64* lds,
                                               const FusedFin& ff) {
    __shared__ u32 is_last;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 tk = atomicAdd((unsigned long long*)(t.counters + CNT_FIN_TICKET), 1ULL);
        is_last = tk == (u64)gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[4] = __builtin_amdgcn_s_memrealtime();
    const u64 n = (t.cap + 1) * t.stride_words;  // host: <= the launch's dynamic LDS
    for (u64 i = threadIdx.x; i < n; i += FIN_NT) lds[i] = ld_sc1(t.slots + i);
    if (threadIdx.x == 0) atomicExch((unsigned long long*)(t.counters + CNT_FIN_TICKET), 0ULL);
    __syncthreads();
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[5] = __builtin_amdgcn_s_memrealtime();
    finalize_small_body<FUSED_FIN_SLOTS / FIN_NT, false>(S, batches, t, lds, ff.out, ff.totals, ff.host_mirror, ff.recycle, ff.seq,
                                                  ff.trace);
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[6] = __builtin_amdgcn_s_memrealtime();
}

// merge_states of a parked partial state (sc1 loads) into a slot; COUNT(*) alone (CO): one add
template <int AS, bool CO>
__device__ __forceinline__ void merge_parked(const Spec& S, const BatchDesc* batches, u64* st, const u64* r, u64 c1) {
    if constexpr (CO) {  // c1: the parked count, loaded with the entry
        if (c1) at_add<AS>(asp<AS>(st + 1), c1);
    } else {
        apply_state<AS, true, AS_GLB, false, false>(S, asp<AS>(st), r, batches);  // fast kernel: no String MIN/MAX, no Decimal256 (fast_eligible)
    }
}

// finalize_small_body for the COUNT(*)-only fast kernel (one non-null integer key of type T,
// slots [key][count]): the same outputs, counters, recycle and host mirror in a fraction of the
// code — this tail runs once per launch on whichever CU finishes last, from a cold instruction
// cache, so its length is latency.
template <typename T>
__device__ __forceinline__ void finalize_count_only(const TableDesc& t, const u64* view, const FusedFin& ff, bool known,
                                                    u32 view_claims, bool hbm_clean = false) {
    __shared__ u64 wsum[FIN_NT / 64];
    __shared__ u64 cnts[CNT_WORDS];
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    const OutDesc& out = ff.out;
    const u64 n_slots = t.cap + 1;
    constexpr u32 PER = FUSED_FIN_SLOTS / FIN_NT;
    const u64 base = (u64)threadIdx.x * PER;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 myc = (!known && threadIdx.x < CNT_WORDS) ? ld_sc1(t.counters + threadIdx.x) : 0;
    u64 ent[PER];
    u32 occ = 0, cnt = 0;
#pragma unroll
    for (u32 k = 0; k < PER; ++k) {
        const u64 s = base + k;
        ent[k] = s < n_slots ? view[s * 2] : SLOT_EMPTY;
        if (ent[k] != SLOT_EMPTY) {
            occ |= 1u << k;
            cnt++;
        }
    }
    u64 ic = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const u64 o = __shfl_up(ic, off, 64);
        if (lane >= off) ic += o;
    }
    if (lane == 63) wsum[wave] = ic;
    lds_barrier();
    u64 p = ic - cnt, total = 0;
    for (int w = 0; w < FIN_NT / 64; ++w) {
        if (w < wave) p += wsum[w];
        total += wsum[w];
    }
#pragma unroll
    for (u32 k = 0; k < PER; ++k) {
        if (!((occ >> k) & 1) || p >= out.cap_groups) continue;
        const u64 s = base + k;
        ((T*)out.key_data[0])[p] = (T)(s == t.cap ? SLOT_EMPTY : ent[k]);
        ((u64*)out.agg_data[0])[p] = view[s * 2 + 1];
        p++;
    }
    if (threadIdx.x == 0) ff.totals[0] = total;
    // known: every group of the table was claimed in this launch, nothing overflowed
    if (known) myc = threadIdx.x == CNT_CLAIMS ? total : 0;
    if (threadIdx.x < CNT_WORDS) cnts[threadIdx.x] = myc;
    lds_barrier();
    const bool rc = ff.recycle && cnts[CNT_OVF_ROWS] == 0 && cnts[CNT_OVF_RECS] == 0 && total <= out.cap_groups;
    if (rc && threadIdx.x < CNT_WORDS) t.counters[threadIdx.x] = 0;  // dbg_agg_reset
    // known counters: the view's claims were not added yet (fused_chain); a table that outlives
    // this finalize needs them
    if (known && !rc && threadIdx.x == 0 && view_claims)
        atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)view_claims);
    u64* hm = ff.host_mirror;
    auto put = [&](int w, u64 v) { __hip_atomic_store(hm + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    // known counters: one self-validating word ([seq | recycled | groups], MIRROR_COMPACT) instead
    // of the counter words and a seq posted behind a wait for them
    const bool compact = known && total < (1u << 24);
    if (hm && compact && threadIdx.x == 0)
        put(MIRROR_COMPACT, (ff.seq << 25) | ((rc ? 1ULL : 0ULL) << 24) | total);
    if (hm && !compact && threadIdx.x == 0) {
        for (int w = 0; w < CNT_WORDS; ++w) put(w, cnts[w]);
        put(CNT_WORDS, total);
        put(CNT_WORDS + 1, 0);  // string bytes of the (integer) key column
        put(CNT_WORDS + 1 + DBG_MAX_KEYS, rc ? 1 : 0);
    }
    if (!rc)  // the table outlives this finalize: the view holds groups the HBM table does not
        for (u64 i = threadIdx.x; i < n_slots * 2; i += FIN_NT) t.slots[i] = view[i];
    if (rc && !hbm_clean)  // table_init of the claimed slots of the view (the HBM copy may hold fewer: same
                           // values); hbm_clean: empty at launch and never written since — nothing to undo
#pragma unroll
        for (u32 k = 0; k < PER; ++k)
            if ((occ >> k) & 1) {
                u64* d = t.slots + (base + k) * 2;
                d[0] = SLOT_EMPTY;
                d[1] = 0;
            }
    if (hm && !compact && threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(hm + CNT_WORDS + 2 + DBG_MAX_KEYS, ff.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Find or claim `key` (inline) in an LDS copy of the HBM table (same slots, same probing as
// g_find).  false: the probe limit was hit.
__device__ __forceinline__ bool view_find(u64* view, const TableDesc& t, u64 key, u32& claims, u64& slot) {
    const u32 sw = t.stride_words;
    if (key == SLOT_EMPTY) {  // the all-ones 8-byte key: sentinel slot, entry 0 once claimed
        slot = t.cap;
        claims += at_cas<AS_LDS>(asp<AS_LDS>(view + t.cap * sw), SLOT_EMPTY, 0ULL) == SLOT_EMPTY ? 1u : 0u;
        return true;
    }
    const u64 mask = t.cap - 1;
    u64 s = slot_mix(key) & mask;
    for (u32 p = 0; p < t.probe_limit; ++p) {
        wptr<AS_LDS> e = asp<AS_LDS>(view + s * sw);
        u64 ev = vld<AS_LDS>(e);
        if (ev == SLOT_EMPTY) {
            const u64 old = at_cas<AS_LDS>(e, SLOT_EMPTY, key);
            if (old == SLOT_EMPTY) {
                claims++;
                slot = s;
                return true;
            }
            ev = old;
        }
        if (ev == key) {
            slot = s;
            return true;
        }
        s = (s + 1) & mask;
    }
    return false;
}

// The end of a fused COUNT(*) launch over keys of <= 16 bits (ClickBench Q8: Int16 AdvEngineID):
// a direct-mapped hand-off instead of the parked-row tree.  Every workgroup adds its LDS table's
// counts into a dense array indexed by the key (device atomics without return, issued as soon as
// it has streamed its share — overlapping the workgroups still streaming) and sets the key's bit
// in a presence bitmap, then takes the launch ticket; the last arrival reads the bitmap and the
// counts of the set bits (zeroing both behind it for the next launch), merges them into an LDS
// view of the table and runs the count-only finalize.  The critical path after the last workgroup
// streams is one atomic drain, one ticket and two dependent loads — against the tree's two park /
// ticket / reload levels — and the merge no longer grows with the grid.
template <typename T>
__device__ __forceinline__ void fused_dense(const Spec& S, const BatchDesc* batches, const BatchDesc& B, u64* lds, u32 lds_slots,
                                            u32 sw, u32* lcount, u32 nt, const TableDesc& t, u32 my_claims, u32 my_ovf,
                                            const FusedFin& ff) {
    __shared__ u32 role, bad, vcl, wg_ovf;
    __shared__ u64 hbm_claims, ovf_seen;
    const u32 dn = ff.dense_n, dmask = dn - 1;
    u64* dcnt = ff.dense;
    u64* dbits = ff.dense + dn;
    if (threadIdx.x == 0) wg_ovf = 0;
    // 1. the LDS table into the dense array (no return values: the stores drain before the ticket)
    for (u32 s = threadIdx.x; s < lds_slots; s += nt) {
        const u64* p = lds + (u64)s * sw;
        const u64 e = p[0];
        if (e == SLOT_EMPTY) continue;
        const u32 idx = (u32)e & dmask;
        __hip_atomic_fetch_add(dcnt + idx, p[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_or(dbits + (idx >> 6), 1ULL << (idx & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (my_claims) atomicAdd(&lcount[1], my_claims);
    if (my_ovf) atomicAdd(&wg_ovf, my_ovf);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        if (lcount[1]) {
            atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)lcount[1]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const u64 add = 1 + ((u64)lcount[1] << 16) + ((u64)wg_ovf << 40);
        const u64 tk = atomicAdd((unsigned long long*)(t.counters + CNT_FIN_TICKET), (unsigned long long)add) + add;
        role = (tk & 0xFFFF) == gridDim.x ? 1u : 0u;
        hbm_claims = (tk >> 16) & 0xFFFFFF;
        ovf_seen = tk >> 40;
    }
    __syncthreads();
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) atomicMax((unsigned long long*)ff.trace + 3, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    if (!role) return;
    // 2. the last arrival: view of the table, the dense groups merged into it, finalize
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        atomicExch((unsigned long long*)(t.counters + CNT_FIN_TICKET), 0ULL);
        bad = 0;
        vcl = 0;
        lcount[2] = 0;
        if (kPhaseTrace && ff.trace) ff.trace[4] = __builtin_amdgcn_s_memrealtime();
    }
    const u64 n = (t.cap + 1) * sw;  // host: <= the launch's dynamic LDS
    if (ff.table_empty && hbm_claims == 0)
        for (u64 i = threadIdx.x; i < n; i += nt) lds[i] = S.slot_init[i % sw];
    else
        for (u64 i = threadIdx.x; i < n; i += nt) lds[i] = ld_sc1(t.slots + i);
    __syncthreads();
    u32 vclaims = 0;
    for (u32 w = threadIdx.x; w < (dn >> 6); w += nt) {
        u64 b = ld_sc1(dbits + w);
        if (!b) continue;
        st_sc1(dbits + w, 0);
        while (b) {
            const u32 j = (u32)__builtin_ctzll(b);
            b &= b - 1;
            const u32 idx = (w << 6) | j;
            const u64 c = ld_sc1(dcnt + idx);
            st_sc1(dcnt + idx, 0);
            const u64 key = (u64)idx;  // the inline packed key of a <= 16-bit column: its raw bits
            u64 slot;
            if (view_find(lds, t, key, vclaims, slot)) {
                lds[slot * sw + 1] += c;  // one thread per key
            } else {  // an overflow record (the host grows the table and finalizes again)
                const u64 k = atomicAdd((unsigned long long*)(t.counters + CNT_OVF_RECS), 1ULL);
                if (k < t.ovf_recs_cap) {
                    u64* r = t.ovf_recs + k * t.stride_words;
                    r[0] = key;
                    r[1] = c;
                } else {
                    atomicOr((unsigned long long*)(t.counters + CNT_ERR), (unsigned long long)ERR_OVF_LOST);
                }
                bad = 1;
            }
        }
    }
    if (vclaims) atomicAdd(&vcl, vclaims);
    __syncthreads();
    const bool known = ff.table_empty && ovf_seen == 0 && !bad;
    if (threadIdx.x == 0 && vcl && !known) {
        atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)vcl);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[5] = __builtin_amdgcn_s_memrealtime();
    finalize_count_only<T>(t, lds, ff, known, vcl);
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[6] = __builtin_amdgcn_s_memrealtime();
}

// The low-cardinality end of a fused insert + finalize launch (ClickBench Q8: 32 groups in every
// workgroup's LDS table).  The HBM table is not written on the way: partial tables travel as
// parked rows up a two-level tree and are merged in LDS, and the last workgroup finalizes from
// an LDS view of the table with the group tables merged in.
//   1. every workgroup parks its LDS table (<= SCR_ENTRIES groups; a larger one flushes into the
//      HBM table as block_flush does) and takes its group's ticket;
//   2. the last workgroup of each group of SCR_GROUP merges the group's parked rows in LDS,
//      parks the merged table in the group's row and takes the launch ticket;
//   3. the last group leader copies the HBM table (groups of earlier launches and direct flushes)
//      into LDS, merges every group row into that view and runs the finalize body on it.  The
//      view goes back to HBM only when the table outlives the finalize (no recycle) or a key did
//      not fit the view (overflow record: the host grows the table and finalizes again).
// Each hand-off is a store drain + one ticket + sc1 loads (MI355X_MICROARCH.md, inter-workgroup
// visibility); against block_flush + fused_finalize this saves the HBM probe / CAS / atomic
// round trips of the group leaders' flush and one barrier + ticket level.
template <typename T, bool CO>
__device__ __forceinline__ void fused_chain(const Spec& S, const BatchDesc* batches, const BatchDesc& B, u64* lds, u32 lds_slots,
                                            u32 sw, u32* lcount, u32 nt, const TableDesc& t, u32 my_claims, u32 my_ovf,
                                            const FusedFin& ff) {
    __shared__ u32 role, bad, vcl, wg_ovf;  // (the view overwrites lcount: the table copy extends past lds_slots)
    const u32 lmask = lds_slots - 1;
    const u32 llimit = lds_slots - lds_slots / 4;
    u64* counts = t.scratch;
    u64* tickets = t.scratch + t.scr_blocks;
    u64* gmeta = tickets + t.scr_blocks / 2;  // [group] parked entries of the group row
    u64* rows = t.scratch + 2 * (u64)t.scr_blocks;
    u64* grows = rows + (u64)t.scr_blocks * SCR_ENTRIES * sw;
    const u32 n_groups = (gridDim.x + SCR_GROUP - 1) / SCR_GROUP;
    const u32 g = blockIdx.x / SCR_GROUP;
    const u32 gsize = min((u32)SCR_GROUP, gridDim.x - g * SCR_GROUP);
    if (threadIdx.x == 0) wg_ovf = 0;
    __syncthreads();
    // park the LDS table (compacted) in `dst` with sc1 stores, or flush it into the HBM table when
    // it holds more than a row takes (counted as a possible overflow: the flush may push
    // records); returns the parked entries (uniform)
    auto park = [&](u64* dst) -> u64 {
        if (lcount[0] > SCR_ENTRIES) {
            flush_lds_direct<true, false, false, false>(S, batches, B, lds, lds_slots, sw, nt, t, my_claims);
            my_ovf += threadIdx.x == 0 ? 1u : 0u;
            return 0;
        }
        for (u32 s = threadIdx.x; s < lds_slots; s += nt) {
            const u64* p = lds + (u64)s * sw;
            if (p[0] == SLOT_EMPTY) continue;
            const u32 k = atomicAdd(&lcount[2], 1u);
            u64* d = dst + (u64)k * sw;
            for (u32 w = 0; w <= (u32)S.n_words; ++w) st_sc1(d + w, p[w]);
        }
        __syncthreads();
        return lcount[2];
    };
    // HBM claims of this workgroup into the table counter, then a ticket (thread 0; both device
    // atomics complete in order: the ticket's taker sees the claims)
    // A ticket word carries, besides the arrivals (bits [0, 16)), the HBM claims (bits [16, 40))
    // and the possible overflow pushes (bits [40, 64)) of the workgroups that took it, so the last
    // arrival knows without another load whether this launch created groups in HBM or pushed
    // overflow records (the finalize then needs neither the table nor the counters).
    auto claims_and_ticket = [&](u64* ticket, u64 carried_claims, u64 carried_ovf) -> u64 {
        if (my_claims) atomicAdd(&lcount[1], my_claims);
        if (my_ovf) atomicAdd(&wg_ovf, my_ovf);
        my_claims = my_ovf = 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        u64 tk = 0;
        if (threadIdx.x == 0) {
            if (lcount[1]) {
                atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)lcount[1]);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            const u64 add = 1 + ((carried_claims + lcount[1]) << 16) + ((carried_ovf + wg_ovf) << 40);
            tk = atomicAdd((unsigned long long*)ticket, (unsigned long long)add) + add;  // inclusive
        }
        return tk;
    };
    // 1. park, group ticket
    const u64 np = park(rows + (u64)blockIdx.x * SCR_ENTRIES * sw);
    if (threadIdx.x == 0) st_sc1(counts + blockIdx.x, np);
    __shared__ u64 hbm_claims, ovf_seen;  // this launch's HBM claims / possible overflow pushes: the
                                          // group's (leader), all (last leader)
    {
        const u64 tk = claims_and_ticket(tickets + g, 0, 0);
        if (threadIdx.x == 0) {
            role = (tk & 0xFFFF) == gsize ? 1u : 0u;
            hbm_claims = (tk >> 16) & 0xFFFFFF;
            ovf_seen = tk >> 40;
            wg_ovf = 0;
        }
    }
    __syncthreads();
    if (!role) return;
    // 2. group leader: merge the group's parked rows in LDS, park the result in the group row
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        tickets[g] = 0;  // ready for the next launch on this table (all members have added)
        lcount[0] = lcount[1] = lcount[2] = 0;
    }
    lds_table_init<false>(S, lds, lds_slots, sw, nt);
    __syncthreads();
    for (u32 f = threadIdx.x; f < gsize * SCR_ENTRIES; f += nt) {
        const u64 b = (u64)g * SCR_GROUP + f / SCR_ENTRIES, k = f % SCR_ENTRIES;
        const u64* r = rows + (b * SCR_ENTRIES + k) * sw;
        const u64 cnt = ld_sc1(counts + b);
        const u64 e = ld_sc1(r);  // issued with the count: rows are allocated in full
        const u64 c1 = CO ? ld_sc1(r + 1) : 0;  // COUNT(*): the whole state, in the same round trip
        if (k >= cnt) continue;
        const int ls = lds_find<true>(S, batches, B.keys, 0, e, 0, lds, lmask, sw, lcount, llimit);
        if (ls >= 0) {
            merge_parked<AS_LDS, CO>(S, batches, lds + (u64)ls * sw, r, c1);
            continue;
        }
        bool claimed;
        const u64 gs = g_find<true>(S, batches, B.keys, 0, e, 0, t, t.probe_limit, claimed);
        if (gs == ~0ULL) {
            push_ovf_rec<true>(S, t, e, r);
            my_ovf++;
            continue;
        }
        my_claims += claimed ? 1 : 0;
        merge_parked<AS_GLB, CO>(S, batches, t.slots + gs * t.stride_words, r, c1);
    }
    __syncthreads();
    const u64 gp = park(grows + (u64)g * SCR_ENTRIES * sw);
    if (threadIdx.x == 0) st_sc1(gmeta + g, gp);
    {
        const u64 tk = claims_and_ticket(t.counters + CNT_FIN_TICKET, hbm_claims, ovf_seen);
        if (threadIdx.x == 0) {
            role = (tk & 0xFFFF) == n_groups ? 2u : 0u;
            hbm_claims = (tk >> 16) & 0xFFFFFF;
            ovf_seen = tk >> 40;
        }
    }
    __syncthreads();
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) atomicMax((unsigned long long*)ff.trace + 3, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    if (role != 2) return;
    // 3. the last group leader: view of the HBM table, group rows merged into it, finalize
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        atomicExch((unsigned long long*)(t.counters + CNT_FIN_TICKET), 0ULL);
        bad = 0;
        vcl = 0;
        if (kPhaseTrace && ff.trace) ff.trace[4] = __builtin_amdgcn_s_memrealtime();
    }
    // the view: the HBM table, or its initial state when it was empty at launch start (recycled
    // by the previous finalize) and no workgroup of this launch created a group in it
    const u64 n = (t.cap + 1) * sw;  // host: <= the launch's dynamic LDS
    if (ff.table_empty && hbm_claims == 0)
        for (u64 i = threadIdx.x; i < n; i += nt) lds[i] = S.slot_init[i % sw];
    else
        for (u64 i = threadIdx.x; i < n; i += nt) lds[i] = ld_sc1(t.slots + i);
    __syncthreads();
    u32 vclaims = 0;
    for (u32 f = threadIdx.x; f < n_groups * SCR_ENTRIES; f += nt) {
        const u64 gg = f / SCR_ENTRIES, k = f % SCR_ENTRIES;
        const u64* r = grows + (gg * SCR_ENTRIES + k) * sw;
        const u64 cnt = ld_sc1(gmeta + gg);
        const u64 e = ld_sc1(r);
        const u64 c1 = CO ? ld_sc1(r + 1) : 0;
        if (k >= cnt) continue;
        u64 slot;
        if (view_find(lds, t, e, vclaims, slot)) {
            merge_parked<AS_LDS, CO>(S, batches, lds + slot * sw, r, c1);
        } else {
            push_ovf_rec<true>(S, t, e, r);
            bad = 1;
        }
    }
    if (vclaims) atomicAdd(&vcl, vclaims);
    __syncthreads();
    const bool known = ff.table_empty && ovf_seen == 0 && !bad;
    // the view's claims into the table counter: before the finalize reads the counters, or — when
    // they are known (count-only) — only if the table outlives the finalize (finalize_count_only)
    if (threadIdx.x == 0 && vcl && !(CO && known)) {
        atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)vcl);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[5] = __builtin_amdgcn_s_memrealtime();
    // the finalize writes the view back when the table outlives it (no recycle: short buffers, an
    // overflow record, or a caller that keeps the table)
    // counters known without a load: an empty table at launch start, no overflow anywhere
    if constexpr (CO) finalize_count_only<T>(t, lds, ff, known, vcl);
    else finalize_small_body<FUSED_FIN_SLOTS / FIN_NT, false>(S, batches, t, lds, ff.out, ff.totals, ff.host_mirror, ff.recycle, ff.seq,
                                                       ff.trace, true);
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[6] = __builtin_amdgcn_s_memrealtime();
}

// The fused chain for COUNT(*) over a key of <= 16 bits (ClickBench Q8's Int16 AdvEngineID), with
// self-validating parked rows so that every hand-off costs one round trip instead of three.  The
// chain above parks a table, drains the stores, takes a ticket, and the last arrival then loads
// the rows: store drain + ticket + loads on the critical path at both levels.  Here all three are
// in flight together: a workgroup issues its ticket, parks its table without draining the stores,
// and loads its siblings' rows while the ticket is still outstanding.  A workgroup that the
// ticket says is not the last drops what it loaded and returns (it never waits on another
// workgroup); the last arrival already holds the rows that had landed, polls again only the
// items that had not, and merges them into its own LDS table in place (its own parked row is
// read by nobody).  The ticket elects the merger and carries the HBM claims; it vouches for no
// data, so nothing has to land before it.
// A parked entry is one word, [key 16 b | count 24 b (level 2: 28 b) | tag 24 b (level 2: 20 b)],
// the tag the low bits of the launch's sequence number, written by one sc1 store; the row's
// entry count is posted as [seq 44 b | entries 20 b].  Item k of a row is an entry only if the
// count word carries this launch's full sequence number and k is below its count, and it is
// accepted only once its own tag is this launch's: a reader spins (bounded) on an item until
// both hold — no acquire / release pair, no second round trip.
// A stale word never validates: the host keeps the low TAG2_BITS of the sequence number away
// from 0 and clears the whole scratch on the handle's stream whenever they wrap (fin_launch), and
// clears it when the handle is created, so every word in the rows is zero (tag 0: never a
// launch's), a word of the generic chain or the parked flush on this handle (a key of <= 16 bits
// or a row count below 2^40: tag 0 again), or a tagged word of a launch since the last clear,
// whose tag differs from this launch's.
// A count never carries into the tag: the host takes this chain only when a workgroup's share of
// the rows stays below 2^CNT1_BITS (launch_fast_t, from the grid, NT and FAST_UNROLL: with 256
// workgroups that is rows < 2^32 - 2^22); a group of SCR_GROUP then stays below 2^CNT2_BITS.
#ifndef CHAIN_TAGGED
#define CHAIN_TAGGED 1  // 0: the generic chain for these launches too (A/B builds: make EXP=1 EXTRA=-DCHAIN_TAGGED=0)
#endif
constexpr bool kChainTagged = CHAIN_TAGGED != 0;
#define TAG1_BITS 24
#define TAG2_BITS 20
#define CNT1_BITS (64 - 16 - TAG1_BITS)  // count bits of a level-1 entry
#define CNT2_BITS (64 - 16 - TAG2_BITS)
static_assert(FIN_SEQ_TAG_PERIOD == (1ULL << TAG2_BITS), "the host clears the scratch when the narrower tag wraps");
static_assert(TAG2_BITS <= TAG1_BITS, "the host keeps the low TAG2_BITS of the sequence number non-zero: both tags then are");
static_assert(((u64)SCR_GROUP << CNT1_BITS) <= (1ULL << CNT2_BITS), "a group's count fits a level-2 entry");
static_assert(SCR_GROUP * SCR_ENTRIES <= FIN_NT, "one parked item per thread at level 1");
#define CHAIN_TAGGED_MAX_BLOCKS (SCR_GROUP * (FIN_NT / SCR_ENTRIES))  // one group-row item per thread at level 2
__device__ __forceinline__ u64 chain_pack(u64 key, u64 cnt, u64 seq, int level) {
    const int tb = level == 1 ? TAG1_BITS : TAG2_BITS;
    return key | (cnt << 16) | ((seq & ((1ULL << tb) - 1)) << (64 - tb));
}

// The count-only finalize straight from the last leader's LDS table (every group of the launch
// merged into it, `total` of its lds_slots slots claimed), for a launch after which nothing
// outlives the finalize: the HBM table was empty and stays untouched, the counters are known, the
// table recycles.  No prefix scan: the order of result rows is free, so each entry takes its row
// from an LDS counter (`next`, zero on entry).  Host word and counters as finalize_count_only's
// known / recycled / compact case.
template <typename T, int OWN>
__device__ __forceinline__ void finalize_count_lds(const TableDesc& t, const u64* lds, u32 lds_slots, u32 sw, u32 nt, u32* next,
                                                   u32 total, const FusedFin& ff) {
    const OutDesc& out = ff.out;
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const u32 s = threadIdx.x + (u32)j * nt;
        if (s >= lds_slots) continue;
        const u64 e = lds[(u64)s * sw];
        if (e == SLOT_EMPTY) continue;
        const u32 p = atomicAdd(next, 1u);
        if (p >= out.cap_groups) continue;  // (total <= cap_groups: the caller's condition)
        ((T*)out.key_data[0])[p] = (T)e;
        ((u64*)out.agg_data[0])[p] = lds[(u64)s * sw + 1];
    }
    if (threadIdx.x < CNT_WORDS) t.counters[threadIdx.x] = 0;  // dbg_agg_reset
    if (threadIdx.x == 0) {
        ff.totals[0] = total;
        __hip_atomic_store(ff.host_mirror + MIRROR_COMPACT, (ff.seq << 25) | (1ULL << 24) | total, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <typename T>
__device__ __forceinline__ void fused_chain_tagged(const Spec& S, const BatchDesc* batches, const BatchDesc& B, u64* lds, u32 lds_slots,
                                                   u32 sw, u32* lcount, u32 nt, const TableDesc& t, u32 my_claims, u32 my_ovf,
                                                   const FusedFin& ff) {
    constexpr int OWN = 4;  // own slots per thread the last leader finalizes (lds_slots <= 4 x nt, checked by the caller)
    __shared__ u32 role, bad, vcl;
    __shared__ u64 hbm_claims, ovf_seen;
    const u32 lmask = lds_slots - 1;
    const u32 llimit = lds_slots - lds_slots / 4;
    u64* counts = t.scratch;
    u64* tickets = t.scratch + t.scr_blocks;
    u64* gmeta = tickets + t.scr_blocks / 2;
    u64* rows = t.scratch + 2 * (u64)t.scr_blocks;  // SCR_ENTRIES words per workgroup (one word per entry)
    u64* grows = rows + (u64)t.scr_blocks * SCR_ENTRIES * sw;
    const u32 n_groups = (gridDim.x + SCR_GROUP - 1) / SCR_GROUP;
    const u32 g = blockIdx.x / SCR_GROUP;
    const u32 gsize = min((u32)SCR_GROUP, gridDim.x - g * SCR_GROUP);
    const u64 seq = ff.seq & ((1ULL << 44) - 1);  // never 0: its low TAG2_BITS are not (host)
    // LDS words of the hand-offs: lcount[0] the table's claimed slots (lds_find), [1] the
    // workgroup's HBM claims not yet on a ticket, [2] parked entries, [3] possible overflow pushes
    // not yet on a ticket; [1..3] are zero when the stream ends and after every hand-off.
    auto lds_barrier = [] { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };  // loads and stores in flight stay there
    auto post_claims = [&]() {
        if (my_claims) atomicAdd(&lcount[1], my_claims);
        if (my_ovf) atomicOr(&lcount[3], 1u);
        my_claims = my_ovf = 0;
    };
    // The rare hand-off of a workgroup that wrote the HBM table or must: a table too large for a
    // row goes there (its possible overflow pushes counted), every HBM atomic of the workgroup is
    // drained and its claims are in the table counter before the ticket carries them (both device
    // atomics complete in order: the ticket's taker sees the claims).  Uniform; true = flushed.
    auto settle_hbm = [&]() -> bool {
        const bool large = lcount[0] > SCR_ENTRIES;
        if (large) {
            flush_lds_direct<true, false, false, false>(S, batches, B, lds, lds_slots, sw, nt, t, my_claims);
            if (threadIdx.x == 0) atomicOr(&lcount[3], 1u);
        }
        post_claims();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0 && lcount[1]) {
            atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)lcount[1]);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        return large;
    };
    // One hand-off, everything in flight together: every thread loads its item of the siblings'
    // rows (`m`, `w`; `others`: the item exists and is not this workgroup's own), thread 0 issues
    // the ticket (arrivals, HBM claims and possible overflow pushes of the workgroups that took
    // it, as the generic chain), every thread parks its slot's entry in `dst` (sc1, not drained);
    // the entry count follows as soon as the workgroup knows it, and only then does thread 0 wait
    // for the ticket.  Returns the inclusive ticket (thread 0).  Reads lcount[1], [3] before its
    // barrier, clears [1..3] behind it.
    // The ticket is an asm statement: a returning atomic the compiler can see is combined per wave,
    // which consumes its result — a full round trip — right where it is issued, ahead of wave 0's
    // loads and stores and of the barrier every other wave then waits at.  The asm's result
    // register is written when the atomic returns; the `s_waitcnt` that names it stands before
    // its first use.  (A memory operation the compiler does not count only makes its own waits
    // for older operations longer, never shorter: vmcnt retires in order.)
    auto hand_off = [&](u64* ticket, u64 carried_claims, u64 carried_ovf, bool flushed, u64* dst, u64* meta, int level,
                        bool others, const u64* o_meta, const u64* o_ent, u64& m, u64& w) -> u64 {
        m = w = 0;
        if (others) {
            m = ld_sc1(o_meta);
            w = ld_sc1(o_ent);
        }
        u64 old, add = 0;  // old: thread 0 only, written by the first asm, read behind the second
        if (threadIdx.x == 0) {
            add = 1 + ((carried_claims + lcount[1]) << 16) + ((u64)((carried_ovf || lcount[3]) ? 1 : 0) << 40);
            asm volatile("global_atomic_add_x2 %0, %1, %2, off sc0" : "=&v"(old) : "v"(ticket), "v"(add) : "memory");  // device scope, returns the old value
        }
        if (!flushed)
            for (u32 s = threadIdx.x; s < lds_slots; s += nt) {
                const u64* p = lds + (u64)s * sw;
                if (p[0] == SLOT_EMPTY) continue;
                const u32 k = atomicAdd(&lcount[2], 1u);
                st_sc1(dst + k, chain_pack(p[0], p[1], seq, level));
            }
        lds_barrier();
        u64 tk = 0;
        if (threadIdx.x == 0) {
            st_sc1(meta, (seq << 20) | lcount[2]);
            lcount[1] = lcount[2] = lcount[3] = 0;
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(old) : : "memory");  // the ticket is back
            tk = old + add;
        }
        return tk;
    };
    // an overflow record [key][count] (the host grows the table and finalizes again)
    auto push_kc = [&](u64 key, u64 c) {
        const u64 k = atomicAdd((unsigned long long*)(t.counters + CNT_OVF_RECS), 1ULL);
        if (k >= t.ovf_recs_cap) {
            atomicOr((unsigned long long*)(t.counters + CNT_ERR), (unsigned long long)ERR_OVF_LOST);
            return;
        }
        u64* r = t.ovf_recs + k * t.stride_words;
        r[0] = key;
        r[1] = c;
    };
    // The item (count word m, entry word w, as loaded under the ticket) a thread holds of a
    // sibling's row: an entry only if m is this launch's and k below its count, accepted once w
    // carries this launch's tag; only what is not current yet is loaded again (bounded: a spin
    // that does not settle raises ERR_CHAIN_SPIN).  false = no entry k.
    auto take_item = [&](const u64* meta, const u64* ent, u32 k, int level, u64 m, u64 w, u64& key, u64& cnt) -> bool {
        const int tb = level == 1 ? TAG1_BITS : TAG2_BITS;
        const u64 tag = seq & ((1ULL << tb) - 1);
        for (u32 it = 0; it < (1u << 22); ++it) {
            if ((m >> 20) == seq) {
                if (k >= (m & 0xFFFFF)) return false;
                if ((w >> (64 - tb)) == tag) {
                    key = w & 0xFFFF;
                    cnt = (w << tb) >> (tb + 16);
                    return true;
                }
            } else {
                m = ld_sc1(meta);
            }
            w = ld_sc1(ent);
            __builtin_amdgcn_s_sleep(1);
        }
        atomicOr((unsigned long long*)(t.counters + CNT_ERR), (unsigned long long)ERR_CHAIN_SPIN);
        bad = 1;
        // also onto the next ticket's overflow bit: the last leader — possibly another workgroup —
        // must not take its counters for known and zero the error word unread
        atomicOr(&lcount[3], 1u);
        return false;
    };
    // a sibling's entry into the own LDS table; one that does not fit goes to the HBM table
    auto merge_item = [&](u64 key, u64 c) {
        const int ls = lds_find<true>(S, batches, B.keys, 0, key, 0, lds, lmask, sw, lcount, llimit);
        if (ls >= 0) {
            at_add<AS_LDS>(asp<AS_LDS>(lds + (u64)ls * sw + 1), c);
            return;
        }
        bool claimed;
        const u64 gs = g_find<true>(S, batches, B.keys, 0, key, 0, t, t.probe_limit, claimed);
        if (gs == ~0ULL) {
            push_kc(key, c);
            my_ovf++;
            return;
        }
        my_claims += claimed ? 1 : 0;
        at_add<AS_GLB>(asp<AS_GLB>(t.slots + gs * t.stride_words + 1), c);
    };
    // the own LDS table went to the HBM table: empty again before rows are merged into it
    auto empty_own = [&]() {
        lds_table_init<false>(S, lds, lds_slots, sw, nt);
        if (threadIdx.x == 0) lcount[0] = 0;
        __syncthreads();
    };
    const u32 item_row = threadIdx.x / SCR_ENTRIES, item_k = threadIdx.x % SCR_ENTRIES;  // the thread's item of the siblings' rows
    // 1. level 1: ticket, park and the loads of the group's 15 other rows together.  (An add into
    //    an HBM slot another workgroup claimed leaves no claim behind: every thread drains what it
    //    has in flight before the barrier the ticket follows — nothing, unless it wrote HBM.)
    post_claims();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    bool flushed = false;
    if (lcount[1] | lcount[3] | (lcount[0] > SCR_ENTRIES ? 1u : 0u)) flushed = settle_hbm();
    const u64 b1 = (u64)g * SCR_GROUP + item_row;
    const bool has1 = item_row < gsize && b1 != blockIdx.x;
    const u64* meta1 = counts + b1;
    const u64* ent1 = rows + b1 * SCR_ENTRIES * sw + item_k;
    u64 m1, w1;
    {
        const u64 tk = hand_off(tickets + g, 0, 0, flushed, rows + (u64)blockIdx.x * SCR_ENTRIES * sw, counts + blockIdx.x, 1, has1,
                                meta1, ent1, m1, w1);
        if (threadIdx.x == 0) {
            role = (tk & 0xFFFF) == gsize ? 1u : 0u;
            hbm_claims = (tk >> 16) & 0xFFFFFF;
            ovf_seen = tk >> 40;
            bad = 0;
            vcl = 0;
        }
    }
    lds_barrier();
    if (!role) return;
    // 2. group leader: the members' rows merged into its own LDS table (emptied first when it went
    //    to the HBM table above); its level-1 claims are on the ticket already
    if (threadIdx.x == 0) tickets[g] = 0;  // all members have added
    if (flushed) empty_own();
    {
        u64 key, c;
        if (has1 && take_item(meta1, ent1, item_k, 1, m1, w1, key, c)) merge_item(key, c);
    }
    // 3. level 2: the same hand-off among the group leaders, over the group rows
    post_claims();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    flushed = false;
    if (lcount[1] | lcount[3] | (lcount[0] > SCR_ENTRIES ? 1u : 0u)) flushed = settle_hbm();
    const bool has2 = item_row < n_groups && item_row != g;
    const u64* meta2 = gmeta + item_row;
    const u64* ent2 = grows + (u64)item_row * SCR_ENTRIES * sw + item_k;
    u64 m2, w2;
    {
        const u64 tk = hand_off(t.counters + CNT_FIN_TICKET, hbm_claims, ovf_seen, flushed, grows + (u64)g * SCR_ENTRIES * sw, gmeta + g,
                                2, has2, meta2, ent2, m2, w2);
        if (threadIdx.x == 0) {
            role = (tk & 0xFFFF) == n_groups ? 2u : 0u;
            hbm_claims = (tk >> 16) & 0xFFFFFF;
            ovf_seen = tk >> 40;
        }
    }
    lds_barrier();
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) atomicMax((unsigned long long*)ff.trace + 3, (unsigned long long)__builtin_amdgcn_s_memrealtime());
    if (role != 2) return;
    // 4. the last leader: the other group rows merged into its own table, which then holds every
    //    group of the launch that is not in the HBM table
    if (threadIdx.x == 0) {
        atomicExch((unsigned long long*)(t.counters + CNT_FIN_TICKET), 0ULL);
        if (kPhaseTrace && ff.trace) ff.trace[4] = __builtin_amdgcn_s_memrealtime();
    }
    if (flushed) empty_own();
    {
        u64 key, c;
        if (has2 && take_item(meta2, ent2, item_k, 2, m2, w2, key, c)) merge_item(key, c);
    }
    post_claims();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the HBM atomics of entries that did not fit
    __syncthreads();
    // this merge's own HBM claims and possible overflow pushes (on no ticket), the table's groups;
    // read here: the view below overwrites lcount
    const u32 own_groups = lcount[0], spill_claims = lcount[1], spill_ovf = lcount[3];
    const bool ovf_any = ovf_seen != 0 || spill_ovf != 0;
    // Nothing outlives the launch (the common case): the HBM table was empty and no workgroup
    // touched it, no overflow, the table recycles and the result fits — finalize from the own
    // table; no view, no second copy of the entries.
    if (ff.table_empty && hbm_claims == 0 && spill_claims == 0 && !ovf_any && !bad && ff.recycle && ff.host_mirror &&
        own_groups <= ff.out.cap_groups) {
        if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[5] = __builtin_amdgcn_s_memrealtime();
        finalize_count_lds<T, OWN>(t, lds, lds_slots, sw, nt, &lcount[2], own_groups, ff);
        if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[6] = __builtin_amdgcn_s_memrealtime();
        return;
    }
    // 5. otherwise the view of the HBM table (a copy, or constants when it is still empty), the own
    //    table merged into it through registers, and the count-only finalize with its write-back
    if (threadIdx.x == 0 && spill_claims) {
        atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)spill_claims);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    u64 okey[OWN], ocnt[OWN];
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const u32 s = threadIdx.x + (u32)j * nt;
        okey[j] = SLOT_EMPTY;
        ocnt[j] = 0;
        if (s < lds_slots) {
            okey[j] = lds[(u64)s * sw];
            ocnt[j] = lds[(u64)s * sw + 1];
        }
    }
    __syncthreads();  // the view overwrites the table
    const u64 n = (t.cap + 1) * sw;  // host: <= the launch's dynamic LDS
    const bool hbm_clean = ff.table_empty && hbm_claims == 0 && spill_claims == 0;
    if (hbm_clean)  // COUNT(*) slots start [EMPTY][0]: no load of the Spec's initial slot
        for (u64 i = threadIdx.x; i < n; i += nt) lds[i] = (i % sw) == 0 ? SLOT_EMPTY : 0ULL;
    else
        for (u64 i = threadIdx.x; i < n; i += nt) lds[i] = ld_sc1(t.slots + i);
    __syncthreads();
    u32 vclaims = 0;
    auto to_view = [&](u64 key, u64 c) {
        u64 slot;
        if (view_find(lds, t, key, vclaims, slot)) {
            at_add<AS_LDS>(asp<AS_LDS>(lds + slot * sw + 1), c);
        } else {
            push_kc(key, c);
            bad = 1;
        }
    };
#pragma unroll
    for (int j = 0; j < OWN; ++j)
        if (okey[j] != SLOT_EMPTY) to_view(okey[j], ocnt[j]);
    if (vclaims) atomicAdd(&vcl, vclaims);
    __syncthreads();
    const bool known = ff.table_empty && !ovf_any && !bad;
    if (threadIdx.x == 0 && vcl && !known) {
        atomicAdd((unsigned long long*)(t.counters + CNT_CLAIMS), (unsigned long long)vcl);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[5] = __builtin_amdgcn_s_memrealtime();
    finalize_count_only<T>(t, lds, ff, known, vcl, hbm_clean && !bad);
    if (kPhaseTrace && ff.trace && threadIdx.x == 0) ff.trace[6] = __builtin_amdgcn_s_memrealtime();
}
