// serde.hip — ingest of serialized partial states (AggregateMeta::Serialized) on gfx950.
//
// The reference's final stage re-inserts a Serialized block [Binary state per aggregate...,
// group columns...] with AggregateHashTable::add_groups(.., agg_states) — probe, then
// AggregateFunction::batch_merge of each state column (EAGG/aggregate_function.rs:96-103) —
// from SerializedPayload::convert_to_aggregate_table (AGG/aggregate_meta.rs:57-101).  Here one
// pass turns every row into an exchange record ([group hash][key part][state words], the layout
// dbg_agg_record_layout describes): the group hash of its key columns and the borsh state bytes
// decoded into the table's state words.  The records then merge through the same record insert
// as dbg_agg_merge_records (merge_states), so a serialized row and an exported record of the same
// group are indistinguishable to the table.
//
// One thread per row: the work is a handful of dependent byte loads per aggregate, HBM-bound on
// the state bytes (≈ 9-26 B per aggregate per row) plus the record write.
#include "agg_dev.hpp"
#include "serde.hpp"

__global__ void __launch_bounds__(256) ser_ingest_kernel(const Spec* __restrict__ spec, SerIngest in, u64 n, u8* __restrict__ rec_out,
                                                         u64* __restrict__ err) {
    const Spec& S = *spec;
    u32 e = 0;
    for (u64 i = blockIdx.x * (u64)blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        u8* rec = rec_out + i * S.rec_width;
        *(u64*)rec = group_hash(in.keys, S.n_keys, i);
        for (int c = 0; c < S.n_keys; ++c) {
            const DCol& kc = in.keys[c];
            const bool v = dcol_valid(kc, i);
            if (S.key_types[c].nullable) rec[S.rec_val_off[c]] = v ? 1 : 0;
            u64* kd = (u64*)(rec + S.rec_key_off[c]);
            if (kc.type == DBG_STRING) {  // (offset into the column's own bytes, len)
                const u64 a = gld<u64>(kc.offsets + i), b = gld<u64>(kc.offsets + i + 1);
                kd[0] = a;
                kd[1] = b - a;
            } else {
                kd[0] = dcol_bits(kc, i);
                if (kc.type == DBG_DECIMAL128) kd[1] = dcol_hi(kc, i);
            }
        }
        u64* w = (u64*)(rec + S.rec_state_off);
        for (int k = 1; k <= S.n_words; ++k) w[k - 1] = S.slot_init[k];
        u64 flags = 0;
        for (int a = 0; a < S.n_aggs; ++a) {
            const u64 o0 = gld<u64>(in.st_offs[a] + i), o1 = gld<u64>(in.st_offs[a] + i + 1);
            e |= ser_decode(S, S.aggs[a], in.st_data[a] + o0, o1 - o0, w, &flags);
        }
        if (S.flags_word >= 0) w[S.flags_word - 1] = flags;
    }
    if (e) atomicOr((unsigned long long*)err, (unsigned long long)e);
}

void launch_ser_ingest(hipStream_t s, const Spec* dspec, const SerIngest& in, u64 n, u8* rec_out, u64* err) {
    if (!n) return;
    u64 blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(ser_ingest_kernel, dim3((u32)blocks), dim3(256), 0, s, dspec, in, n, rec_out, err);
}
