// abi_records.hip — a handle's groups as partial-state records: dbg_agg_partition and
// dbg_agg_export_records, the fixed-capacity exchange (export_fixed / merge_fixed), merging records
// and serialized states back into a table, key compaction and retained bytes.  Record layouts come
// from abi_spec.hip, the table and its batches from abi.hip, the RCCL transfers are exchange.hip's.
#include "abi_internal.hpp"

// The group key's legacy layout (legacy_method's FixedKeys packing or SingleBinary) by key column.
static int legacy_layout(const Spec& S, u32 bits, LegacyLayout* L) {
    memset(L, 0, sizeof(*L));
    int kind = 0;
    uint32_t kb = 0;
    RETURN_IF(legacy_method(S.key_types, S.n_keys, &kind, &kb));
    L->bits = bits;
    if (kind == DBG_LEGACY_SERIALIZER) {  // FastHash of the serialized key bytes (SerCrc, legacy.hpp)
        L->serializer = 1;
        return DBG_OK;
    }
    if (kind == DBG_LEGACY_SINGLE_BINARY) {
        L->binary = 1;
        return DBG_OK;
    }
    L->words = kb <= 8 ? 1 : (kb <= 16 ? 2 : 4);
    int order[DBG_MAX_KEYS];
    u32 off[DBG_MAX_KEYS];
    int32_t null_off[DBG_MAX_KEYS];
    legacy_fixed_order(S.key_types, S.n_keys, order, off, null_off);
    for (int j = 0; j < S.n_keys; ++j) {
        L->off[order[j]] = off[j];
        L->null_off[order[j]] = null_off[j];
    }
    return DBG_OK;
}

// A fresh batch descriptor as records at `base`: its key columns in the record layout.  strs[c]:
// the string bytes key column c's (offset, len) pairs point into (nullptr: fixed-width records).
static void record_key_cols(const Spec& S, const u8* base, const u8* const* strs, BatchDesc* st) {
    st->is_records = 1;
    st->rec_width = S.rec_width;
    st->rec_base = base;
    for (int c = 0; c < S.n_keys; ++c) {
        DCol& d = st->keys[c];
        const dbg_datatype& t = S.key_types[c];
        d.type = t.type;
        d.precision = t.precision;
        d.scale = t.scale;
        d.nullable = t.nullable;
        d.layout = LAYOUT_RECORD;
        d.width = type_width(t.type);
        d.stride = S.rec_width;
        d.data = base + S.rec_key_off[c];
        d.validity = t.nullable ? base + S.rec_val_off[c] : nullptr;
        if (strs) d.strings = strs[c];
    }
}

// One segment of state records -> the table (combine_payload's merge_states).
static int merge_record_batch(dbg_agg_handle* h, const u8* base, u64 n, const u8* const* strs) {
    const Spec& S = h->spec;
    if (n == 0) return DBG_OK;
    if (n >= 0xFFFFFFFFULL) return fail(DBG_ERR_UNSUPPORTED, "segment too large");
    BatchDesc* st;
    u32 bid;
    RETURN_IF(new_batch(h, &st, &bid));
    st->rows = n;
    record_key_cols(S, base, strs, st);
    RETURN_IF(upload_batch(h, st, bid));
    if (!h->pp) RETURN_IF(pp_maybe_switch(h, bid, n));
    if (h->pp) return pp_add_batch(h, st, bid, n, 1);
    h->table_rows += n;
    RETURN_IF(ensure_ovf(h, n, ovf_blocks(n) * 4096));
    prof::Scope ps("agg_merge", h->stream);
    note_insert(h, launch_insert(h->stream, h->dspec, S, h->dbatches, bid, n, true, table_desc(h), true));
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

// `rows` serialized states per aggregate -> the keyless handle's state (batch_merge_single,
// AGG/transform_single_key.rs:223-227): decoded into word rows, checked, then folded by the merge
// kernel.  The word rows are a temporary; nothing is retained.
static int keyless_merge_serialized(dbg_agg_handle* h, const SerIngest& in, u64 rows) {
    const Spec& S = h->spec;
    Buf<u64> words;
    RETURN_IF(words.ensure(rows * (u64)S.stride_words));
    if (!h->ser_err) RETURN_IF(h->ser_err.ensure(1));
    HIPCHECK(hipMemsetAsync(h->ser_err, 0, 8, h->stream));
    {
        prof::Scope ps("keyless_decode", h->stream);
        launch_keyless_decode(h->stream, h->dspec, in, rows, words, h->ser_err);
    }
    HIPCHECK(hipGetLastError());
    u64 e = 0;
    HIPCHECK(hipMemcpyAsync(&e, h->ser_err, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (e & ERR_SER_MALFORMED) return fail(DBG_ERR_INVALID, "serialized state bytes do not match the aggregate's state layout");
    {
        prof::Scope ps("keyless_merge", h->stream);
        launch_keyless_merge(h->stream, h->dspec, words, rows, (u32)S.stride_words, h->kstate);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(h->stream));  // the word rows are freed behind it
    h->kl_merged += rows;
    return DBG_OK;
}

extern "C" {
int dbg_agg_partition(dbg_agg_handle* h, uint32_t n_parts, int scheme, uint64_t* rec_counts, uint64_t* string_bytes) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    REFUSE_KEYLESS(h, "dbg_agg_partition");
    REFUSE_HANDLE_LOCAL(h, "dbg_agg_partition");
    if (n_parts < 1 || n_parts > 256) return fail(DBG_ERR_UNSUPPORTED, "1..256 partitions");
    if (scheme < 0 || scheme > 2) return fail(DBG_ERR_INVALID, "scheme 0 (hash % n), 1 (radix bits) or 2 (legacy buckets)");
    if (scheme >= 1 && (n_parts & (n_parts - 1))) return fail(DBG_ERR_INVALID, "radix partitions must be a power of two");
    LegacyLayout L;
    if (scheme == 2) RETURN_IF(legacy_layout(h->spec, 31 - __builtin_clz(n_parts), &L));
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    if (h->pp) RETURN_IF(pp_finalize(h, nullptr, nullptr));
    else RETURN_IF(resolve_overflow(h));
    const Spec& S = h->spec;
    u64 nb = h->pp ? pp_grec_blocks(std::max<u64>(h->n_groups, 1)) : finalize_blocks(h->cap);
    const u32* lpart = nullptr;
    const bool prefix = scheme != 2 && h->part_keys > 0 && h->part_keys < S.n_keys;
    if (prefix && h->pp) return fail(DBG_ERR_UNSUPPORTED, "partition keys: table strategy only");
    if (prefix && n_parts > 1) {  // buckets of the first part_keys key columns' group hash, per slot
        RETURN_IF(h->d_lpart.ensure((h->cap + 1) / 2 + 1, 1024));
        prof::Scope ps("prefix_bucket", h->stream);
        launch_prefix_slot_bucket(h->stream, h->dspec, h->dbatches, table_desc(h), h->part_keys, n_parts, scheme, (u32*)h->d_lpart.get());
        lpart = (const u32*)h->d_lpart.get();
        scheme = 2;  // count and export read lpart
    }
    if (scheme == 2 && n_parts > 1 && !prefix) {  // hash2bucket<bits, true> of each group's FastHash
        const u64 n = h->pp ? h->n_groups : h->cap + 1;
        RETURN_IF(h->d_lpart.ensure(n / 2 + 1, 1024));
        prof::Scope ps("legacy_bucket", h->stream);
        if (h->pp) launch_pp_grec_legacy_bucket(h->stream, h->dspec, h->dbatches, h->pp_grec, h->n_groups, L, (u32*)h->d_lpart.get());
        else launch_legacy_slot_bucket(h->stream, h->dspec, h->dbatches, table_desc(h), L, (u32*)h->d_lpart.get());
        lpart = (const u32*)h->d_lpart.get();
    }
    u64 nflat = (u64)n_parts * nb;
    RETURN_IF(h->d_part_pos.ensure(nflat + 8, 1024));
    RETURN_IF(h->d_part_str_pos.ensure(nflat * S.n_keys + 8, 1024));
    if (!h->d_part_str_base) RETURN_IF(h->d_part_str_base.ensure(257));
    HIPCHECK(hipMemsetAsync(h->d_part_str_pos, 0, (nflat * S.n_keys + 8) * 8, h->stream));
    {
        prof::Scope ps("count_groups", h->stream);
        if (h->pp)
            launch_pp_grec_count_parts(h->stream, h->dspec, h->dbatches, h->pp_grec, h->n_groups, n_parts, scheme, lpart,
                                       h->d_part_pos, h->d_part_str_pos, nb);
        else
            launch_count_groups(h->stream, h->dspec, S, h->dbatches, table_desc(h), n_parts, scheme, lpart, h->d_part_pos,
                                h->d_part_str_pos);
    }
    h->part_nb = nb;
    std::vector<u64> hist(nflat), shist(nflat * S.n_keys);
    HIPCHECK(hipMemcpyAsync(hist.data(), h->d_part_pos, nflat * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(shist.data(), h->d_part_str_pos, nflat * S.n_keys * 8, hipMemcpyDeviceToHost, h->stream));
    launch_exclusive_scan(h->stream, h->d_part_pos, nflat, h->d_part_pos + nflat);
    launch_exclusive_scan(h->stream, h->d_part_str_pos, nflat * S.n_keys, h->d_part_str_pos + nflat * S.n_keys);
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->part_counts.assign(n_parts, 0);
    h->part_strings.assign(n_parts, 0);
    for (u32 p = 0; p < n_parts; ++p) {
        for (u64 b = 0; b < nb; ++b) h->part_counts[p] += hist[(u64)p * nb + b];
        for (u64 k = 0; k < (u64)S.n_keys * nb; ++k) h->part_strings[p] += shist[(u64)p * S.n_keys * nb + k];
    }
    std::vector<u64> base(n_parts + 1, 0);
    for (u32 p = 0; p < n_parts; ++p) base[p + 1] = base[p] + h->part_strings[p];
    HIPCHECK(hipMemcpyAsync(h->d_part_str_base, base.data(), (n_parts + 1) * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->part_n = n_parts;
    h->part_scheme = scheme;
    for (u32 p = 0; p < n_parts; ++p) {
        if (rec_counts) rec_counts[p] = h->part_counts[p];
        if (string_bytes) string_bytes[p] = h->part_strings[p];
    }
    return DBG_OK;
}

int dbg_agg_export_records(dbg_agg_handle* h, void* dev_records, void* dev_strings) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    REFUSE_KEYLESS(h, "dbg_agg_export_records");
    REFUSE_HANDLE_LOCAL(h, "dbg_agg_export_records");
    if (!h->part_n) return fail(DBG_ERR_INVALID, "dbg_agg_partition must precede dbg_agg_export_records");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    prof::Scope ps("export_records", h->stream);
    if (h->pp)
        launch_pp_grec_export(h->stream, h->dspec, h->dbatches, h->pp_grec, h->n_groups, h->part_n, h->part_scheme,
                              (const u32*)h->d_lpart.get(), h->d_part_pos, h->d_part_str_pos, h->part_nb, (u8*)dev_records,
                              (u8*)dev_strings, h->d_part_str_base);
    else
        launch_export(h->stream, h->dspec, h->spec, h->dbatches, table_desc(h), h->part_n, h->part_scheme, (const u32*)h->d_lpart.get(),
                      h->d_part_pos, h->d_part_str_pos, (u8*)dev_records, (u8*)dev_strings, h->d_part_str_base);
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

// ---- fixed-capacity exchange (replicas + gather, low cardinality) ----
int dbg_agg_export_fixed(dbg_agg_handle* h, void* dev_buf, uint64_t cap_records) {
    if (!h) return fail(DBG_ERR_INVALID, "null argument");
    REFUSE_KEYLESS(h, "dbg_agg_export_fixed");
    if (!dev_buf) return fail(DBG_ERR_INVALID, "null argument");
    REFUSE_HANDLE_LOCAL(h, "dbg_agg_export_fixed");
    const Spec& S = h->spec;
    if (!S.inline_keys) return fail(DBG_ERR_UNSUPPORTED, "fixed export needs fixed-width (inline) group keys");
    if (h->cap + 1 > FIN_SMALL_SLOTS || h->pp) return fail(DBG_ERR_UNSUPPORTED, "fixed export is for small tables");
    if (S.rec_width < 16) return fail(DBG_ERR_INTERNAL, "record narrower than the fixed header");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    prof::Scope ps("export_fixed", h->stream);
    launch_export_fixed(h->stream, h->dspec, h->dbatches, table_desc(h), (u8*)dev_buf, cap_records, h->recycle);
    HIPCHECK(hipGetLastError());
    if (h->recycle) mark_recycled(h);  // the kernel re-initialised the table
    return DBG_OK;
}

int dbg_agg_merge_fixed(dbg_agg_handle* h, const void* dev_bufs, int32_t n_bufs, uint64_t cap_records) {
    if (!h) return fail(DBG_ERR_INVALID, "bad argument");
    REFUSE_KEYLESS(h, "dbg_agg_merge_fixed");
    if (!dev_bufs || n_bufs < 1) return fail(DBG_ERR_INVALID, "bad argument");
    REFUSE_HANDLE_LOCAL(h, "dbg_agg_merge_fixed");
    const Spec& S = h->spec;
    if (!S.inline_keys) return fail(DBG_ERR_UNSUPPORTED, "fixed merge needs fixed-width (inline) group keys");
    if (h->pp) return fail(DBG_ERR_UNSUPPORTED, "fixed merge: the handle runs partitioned (high cardinality)");
    const u64 n = (u64)n_bufs * (cap_records + 1);
    if (n >= 0xFFFFFFFFULL) return fail(DBG_ERR_UNSUPPORTED, "segment too large");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    h->finalized = false;
    h->clean = false;
    BatchDesc* st;
    u32 bid;
    RETURN_IF(new_batch(h, &st, &bid));
    h->table_rows += n;
    st->rows = n;
    st->seg_records = cap_records + 1;
    record_key_cols(S, (const u8*)dev_bufs, nullptr, st);
    RETURN_IF(submit_batch(h, &st, &bid, true));
    RETURN_IF(ensure_ovf(h, n, ovf_blocks(n) * 4096));
    prof::Scope ps("agg_merge", h->stream);
    note_insert(h, launch_insert(h->stream, h->dspec, S, h->dbatches, bid, n, true, table_desc(h), true));
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

int dbg_agg_merge_records(dbg_agg_handle* h, const void* dev_records, const void* dev_strings, int32_t n_segments,
                          const uint64_t* seg_records, const uint64_t* seg_string_bytes) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    REFUSE_KEYLESS(h, "dbg_agg_merge_records");
    REFUSE_HANDLE_LOCAL(h, "dbg_agg_merge_records");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    h->finalized = false;
    h->clean = false;
    const Spec& S = h->spec;
    u64 rec_off = 0, str_off = 0;
    for (int g = 0; g < n_segments; ++g) {
        u64 n = seg_records[g];
        const u8* base = (const u8*)dev_records + rec_off * S.rec_width;
        const u8* strs = (const u8*)dev_strings + str_off;
        rec_off += n;
        str_off += seg_string_bytes ? seg_string_bytes[g] : 0;
        const u8* per_col[DBG_MAX_KEYS];
        for (int c = 0; c < DBG_MAX_KEYS; ++c) per_col[c] = strs;
        RETURN_IF(merge_record_batch(h, base, n, per_col));
    }
    return DBG_OK;
}

// Key compaction (the reference copies only a new group's key into its payload arena,
// EAGG/payload_row.rs:111-130, so a partial's memory follows its groups, not the rows it saw):
// every group leaves as an exchange record (keys, string blob, states), the table restarts empty
// and merges the records back, so its ref-key entries point at one record batch of exactly the
// groups, and the inputs seen so far — the library's copies of host blocks and the caller's
// device columns — are no longer referenced.  O(groups); a no-op for inline keys (no references)
// and the partitioned payload (its records already hold the keys).
int dbg_agg_compact(dbg_agg_handle* h, int* compacted) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    if (compacted) *compacted = 0;
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    const Spec& S = h->spec;
    // a handle-local spec (String MIN/MAX states point into the retained input; Decimal256 has no
    // record format to re-merge from): nothing can be released (a no-op)
    if (h->pp || S.inline_keys || handle_local_reason(S)) return DBG_OK;
    u64 n = 0, sb = 0;
    RETURN_IF(dbg_agg_partition(h, 1, 0, &n, &sb));
    DevBuf rb, strb;
    RETURN_IF(rb.ensure(n * S.rec_width, 16));
    int rc = strb.ensure(sb, 16);
    if (rc == DBG_OK) rc = dbg_agg_export_records(h, rb, strb);
    if (rc == DBG_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(DBG_ERR_DEVICE, "compact: export failed");
    // the handle keeps its strategy: the re-merged batch (one record per group) must not be
    // probed again — on an AUTO handle with many groups the probe would see ratio ~1 and switch
    // to the partitioned payload, after which compaction does nothing
    const u64 rows_before = h->table_rows, remerged_before = h->remerged;
    if (rc == DBG_OK) rc = dbg_agg_reset(h);  // frees the copies of earlier inputs
    h->table_rows = rows_before ? rows_before : 1;
    h->remerged = remerged_before + n;  // merge_record_batch below counts the n records as rows
    RETURN_IF(rc);
    const u8* recs = rb;
    const u8* per_col[DBG_MAX_KEYS];
    for (int c = 0; c < DBG_MAX_KEYS; ++c) per_col[c] = strb;
    h->owned.push_back(std::move(rb));
    h->owned.push_back(std::move(strb));
    h->finalized = false;
    h->clean = false;
    RETURN_IF(merge_record_batch(h, recs, n, per_col));
    if (compacted) *compacted = 1;
    return DBG_OK;
}

// Device bytes the handle keeps for the inputs its table references: copies of host blocks and
// received / compacted records (the caller's own device columns are not counted).
int dbg_agg_retained_bytes(dbg_agg_handle* h, uint64_t* bytes) {
    if (!h || !bytes) return fail(DBG_ERR_INVALID, "null argument");
    u64 t = 0;
    for (const auto& b : h->owned) t += b.cap();
    *bytes = t;
    return DBG_OK;
}

// AggregateMeta::Serialized -> this table (SerializedPayload::convert_to_aggregate_table,
// AGG/aggregate_meta.rs:57-101; AggregateFunction::batch_merge, EAGG/aggregate_function.rs:96-103).
int dbg_agg_merge_serialized(dbg_agg_handle* h, const dbg_column* state_cols, const dbg_column* group_cols, uint64_t rows,
                             int on_device) {
    if (!h || (!state_cols && h->spec.n_aggs) || (!group_cols && h->spec.n_keys)) return fail(DBG_ERR_INVALID, "null argument");
    REFUSE_HANDLE_LOCAL(h, "dbg_agg_merge_serialized");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    h->finalized = false;
    h->clean = false;
    const Spec& S = h->spec;
    for (int a = 0; a < S.n_aggs; ++a)
        if (h->src_kinds[a] == DBG_AGG_AVG_SQL)
            return fail(DBG_ERR_UNSUPPORTED, "serialized states: SQL avg is sum and count in the reference plan");
    if (rows == 0) return DBG_OK;
    if (rows >= 0xFFFFFFFFULL) return fail(DBG_ERR_UNSUPPORTED, "a block holds fewer than 2^32 rows");
    SerIngest in;
    memset(&in, 0, sizeof(in));
    for (int c = 0; c < S.n_keys; ++c) {
        if (group_cols[c].len < rows) return fail(DBG_ERR_INVALID, "group column shorter than rows");
        RETURN_IF(to_dcol({h->stream, h->owned}, group_cols[c], S.key_types[c], true, on_device, in.keys[c]));
    }
    const dbg_datatype bin{DBG_STRING, 0, 0, 0, 0};
    for (int a = 0; a < S.n_aggs; ++a) {
        const dbg_column& sc = state_cols[a];
        if (sc.dt.type != DBG_STRING || sc.dt.nullable || !sc.offsets) return fail(DBG_ERR_INVALID, "a state column is a non-null Binary column");
        if (sc.len < rows) return fail(DBG_ERR_INVALID, "state column shorter than rows");
        DCol d;
        RETURN_IF(to_dcol({h->stream, h->owned}, sc, bin, true, on_device, d));
        in.st_data[a] = d.data;
        in.st_offs[a] = d.offsets;
    }
    if (is_keyless(S)) return keyless_merge_serialized(h, in, rows);
    // records are retained (the table's ref-key entries point at them) until reset
    RETURN_IF(own_alloc({h->stream, h->owned}, rows * S.rec_width));
    u8* const rb = h->owned.back();
    if (!h->ser_err) RETURN_IF(h->ser_err.ensure(1));
    HIPCHECK(hipMemsetAsync(h->ser_err, 0, 8, h->stream));
    {
        prof::Scope ps("ser_ingest", h->stream);
        launch_ser_ingest(h->stream, h->dspec, in, rows, rb, h->ser_err);
    }
    HIPCHECK(hipGetLastError());
    u64 e = 0;
    HIPCHECK(hipMemcpyAsync(&e, h->ser_err, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (e & ERR_SER_MALFORMED) return fail(DBG_ERR_INVALID, "serialized state bytes do not match the aggregate's state layout");
    if (e & ERR_SER_UNREP)
        return fail(DBG_ERR_UNSUPPORTED, "serialized state with a NULL result that the GPU state cannot carry "
                                         "(OrNull flag 0 or None without a nullable argument)");
    const u8* per_col[DBG_MAX_KEYS];
    for (int c = 0; c < DBG_MAX_KEYS; ++c) per_col[c] = c < S.n_keys ? in.keys[c].data : nullptr;
    return merge_record_batch(h, rb, rows, per_col);
}
}  // extern "C"
