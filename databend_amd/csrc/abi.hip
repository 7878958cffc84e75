// abi.hip — the handle of the C ABI of libdbgpu_agg.so (include/dbgpu_agg.h): the last-error slot,
// create / destroy / stream / reset, the table's allocation, growth and deferred overflow, batch
// descriptors and input upload, the inserts (dbg_agg_add_groups, host staging, the held-back and
// radix-partitioned launches) and the small setters and getters.  Everything else a handle does is
// in the other units listed in abi_internal.hpp, which also holds what they share.
//
// A handle is one AggregateHashTable (EAGG/aggregate_hashtable.rs:47) living in HBM.  It owns a
// HIP stream (or borrows the caller's) and its allocations; nothing here runs on the CPU except
// bookkeeping — there is no CPU fallback: a missing/unsupported case returns an error code.
#include "abi_internal.hpp"

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
// the other translation units (scan.hip) report through the same last-error slot
int abi_fail(int code, const std::string& msg) { return fail(code, msg); }

int err_bits_fail(u64 err, u64 mask) {
    err &= mask;
    if (err & ERR_OVF_LOST) return fail(DBG_ERR_INTERNAL, "overflow list exhausted");
    if (err & ERR_MINMAX_SPIN)
        return fail(DBG_ERR_INTERNAL, "Decimal128 MIN/MAX: a state update gave up after 2^20 contended attempts (the result would be wrong)");
    if (err & ERR_CHAIN_SPIN)
        return fail(DBG_ERR_INTERNAL, "fused finalize: a parked row was not posted in time (GPU hand-off stalled)");
    if (err & ERR_FIXED_INCOMPLETE)
        return fail(DBG_ERR_INVALID, "fixed-capacity exchange incomplete (a partial held more groups than the "
                                     "buffer, or unresolved overflow): use dbg_agg_partition + export_records");
    return DBG_OK;
}

int own_alloc(Owner o, size_t bytes) {
    DevBuf b;
    RETURN_IF(b.ensure(bytes));
    o.owned.push_back(std::move(b));
    return DBG_OK;
}

static int own_copy(Owner o, const void* src, size_t bytes, const void** out) {
    RETURN_IF(own_alloc(o, bytes));
    u8* const p = o.owned.back();
    if (bytes) HIPCHECK(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, o.stream));
    *out = p;
    return DBG_OK;
}

// ------------------------------------------------------------------------------------------
// table allocation / growth
// ------------------------------------------------------------------------------------------
static void table_init_now(dbg_agg_handle* h) {
    if (!h->init_pending) return;
    h->init_pending = false;
    prof::Scope ps("table_init", h->stream);
    launch_table_init(h->stream, h->dspec, h->spec, h->slots, h->cap, nullptr);
}

// The table as the kernels see it; a deferred initialisation, or a held-back partitioned table
// stage, is launched first (stream order).
TableDesc table_desc(dbg_agg_handle* h) {
    if (h->def_part) (void)part_flush(h);  // launch errors surface from the stream's next check
    table_init_now(h);
    TableDesc t;
    t.slots = h->slots;
    t.cap = h->cap;
    t.stride_words = (u32)h->spec.tstride;
    t.probe_limit = (u32)std::min<u64>(h->cap, 512);
    t.counters = h->counters;
    t.ovf_rows = h->ovf_rows;
    t.ovf_rows_cap = h->ovf_rows.cap();
    t.ovf_recs = h->ovf_recs;
    t.ovf_recs_cap = h->ovf_recs.cap() / (u64)h->spec.tstride;
    t.scratch = h->scratch;
    t.scr_blocks = h->scr_blocks;

    return t;
}

int flush_deferred(dbg_agg_handle* h) {
    if (h->def_part) RETURN_IF(part_flush(h));
    if (!h->def_on) return DBG_OK;
    h->def_on = false;
    {
        prof::Scope ps("agg_insert", h->stream);
        note_insert(h, launch_insert(h->stream, h->dspec, h->spec, h->dbatches, h->def_bid, h->def_rows, false, table_desc(h), true, &h->def_hb));
    }
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

static int alloc_table(dbg_agg_handle* h, u64 cap, Buf<u64>& out) {
    RETURN_IF(out.ensure((cap + 1) * (u64)h->spec.tstride));
    prof::Scope ps("table_init", h->stream);
    launch_table_init(h->stream, h->dspec, h->spec, out, cap);
    return DBG_OK;
}

int grow_table(dbg_agg_handle* h, u64 new_cap) {
    table_init_now(h);  // the old table is rehashed below
    Buf<u64> old;
    RETURN_IF(alloc_table(h, new_cap, old));
    std::swap(old, h->slots);
    u64 old_cap = h->cap;
    h->cap = new_cap;
    {
        prof::Scope ps("agg_rehash", h->stream);
        launch_rehash(h->stream, h->dspec, h->spec, h->dbatches, old, old_cap, table_desc(h));
    }
    HIPCHECK(hipStreamSynchronize(h->stream));  // the old table is freed behind it
    return DBG_OK;
}

static int read_counters(dbg_agg_handle* h) {
    HIPCHECK(hipMemcpyAsync(h->hcounters, h->counters, CNT_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return DBG_OK;
}

// Resolve deferred overflow: grow so that every pending group fits at <= 50% load, re-insert.
int resolve_overflow(dbg_agg_handle* h) {
    RETURN_IF(read_counters(h));
    bool grew = false;  // sized by overflowed rows this call: shrink to the groups once known
    for (int round = 0; round < 4; ++round) {
        u64 claims = h->hcounters[CNT_CLAIMS], orows = h->hcounters[CNT_OVF_ROWS], orecs = h->hcounters[CNT_OVF_RECS];
        RETURN_IF(err_bits_fail(h->hcounters[CNT_ERR], ERR_OVF_LOST));
        if (orows == 0 && orecs == 0) {
            h->pending_rows = h->pending_recs = 0;
            // keep the load factor sane for the next batch (the reference resizes at 1/1.5)
            const u64 fit = std::max<u64>(pow2_at_least((u64)(claims * 2.0) + 1), 1024);
            if ((double)claims * 1.5 > (double)h->cap) RETURN_IF(grow_table(h, fit));
            // overflow growth sizes by overflowed ROWS (an upper bound on the groups they hold):
            // once the groups are known, give back a table twice or more what they need at the
            // reference's load factor (get_capacity_for_count: next_pow2(1.5 x count),
            // EAGG/aggregate_hashtable.rs:567-569), so table_init, the finalize scans and
            // partitioned inserts touch what the groups need (C5: a first-step overflow left a
            // 2^25-slot, 2 GB table for 7e6 groups in every later step)
            else if (grew) {
                const u64 fit15 = std::max<u64>(pow2_at_least((u64)(claims * 1.5) + 1), 1024);
                if (h->cap >= 2 * fit15 && fit15 >= h->init_cap) RETURN_IF(grow_table(h, fit15));
            }
            return DBG_OK;
        }
        u64 need = pow2_at_least(2 * (claims + orows + orecs) + 1);
        if (need > h->cap) {
            RETURN_IF(grow_table(h, need));
            grew = true;
        }
        HIPCHECK(hipMemsetAsync(h->counters + CNT_OVF_ROWS, 0, 16, h->stream));
        {
            prof::Scope ps("agg_retry", h->stream);
            launch_retry(h->stream, h->dspec, h->spec, h->dbatches, table_desc(h), orows, orecs, h->ovf_rows, h->ovf_recs);
        }
        RETURN_IF(read_counters(h));
    }
    return fail(DBG_ERR_INTERNAL, "overflow did not converge");
}

// Make sure the deferred-overflow lists can hold everything the next launch may push.
int ensure_ovf(dbg_agg_handle* h, u64 add_rows, u64 add_recs) {
    u64 need_rows = h->pending_rows + add_rows, need_recs = h->pending_recs + add_recs;
    const u64 rec_words = (u64)h->spec.tstride;
    if (need_rows <= h->ovf_rows.cap() && need_recs * rec_words <= h->ovf_recs.cap()) {
        h->pending_rows = need_rows;
        h->pending_recs = need_recs;
        return DBG_OK;
    }
    // drain what is pending, then reallocate the lists at the new size
    RETURN_IF(resolve_overflow(h));
    need_rows = add_rows;
    need_recs = add_recs;
    if (need_rows > h->ovf_rows.cap()) RETURN_IF(h->ovf_rows.ensure(need_rows, 1024));
    if (need_recs * rec_words > h->ovf_recs.cap()) RETURN_IF(h->ovf_recs.ensure(need_recs * rec_words, 1024 * rec_words));
    h->pending_rows = need_rows;
    h->pending_recs = need_recs;
    return DBG_OK;
}

// ------------------------------------------------------------------------------------------
// batches
// ------------------------------------------------------------------------------------------
int new_batch(dbg_agg_handle* h, BatchDesc** staging, u32* bid) {
    if (h->n_batches >= 0xFFFE) return fail(DBG_ERR_UNSUPPORTED, "more than 65534 batches before reset");
    u32 id = h->n_batches + 1;
    if (id >= h->dbatches.cap())
        RETURN_IF(h->dbatches.grow_keep(std::max<u64>(64, h->dbatches.cap() * 2), h->dbatches.cap(), h->stream));
    // pinned staging descriptors are pooled: slot id is reused after dbg_agg_reset (which
    // synchronises the stream, so the previous upload from it has completed)
    while (h->pinned_descs.size() <= id) {
        PinnedBuf<BatchDesc> chunk;
        RETURN_IF(chunk.ensure(64));
        for (int k = 0; k < 64; ++k) h->pinned_descs.push_back(chunk + k);
        h->pinned_chunks.push_back(std::move(chunk));
    }
    BatchDesc* st = h->pinned_descs[id];
    memset(st, 0, sizeof(BatchDesc));
    h->n_batches = id;
    *staging = st;
    *bid = id;
    return DBG_OK;
}

static u64 desc_hash(const BatchDesc& d) {
    const u64* w = (const u64*)&d;
    u64 hv = 0x9E3779B97F4A7C15ULL;
    for (size_t k = 0; k < sizeof(BatchDesc) / 8; ++k) hv = (hv ^ w[k]) * 0xff51afd7ed558ccdULL;
    return hv;
}

int upload_batch(dbg_agg_handle* h, BatchDesc* st, u32 bid) {
    HIPCHECK(hipMemcpyAsync(h->dbatches + bid, st, sizeof(BatchDesc), hipMemcpyHostToDevice, h->stream));
    h->uploads_pending = true;
    return DBG_OK;
}

// Upload a filled batch descriptor, or reuse an identical cached one (device-resident inputs
// only: the descriptor is then pointers alone and immutable).  A cache hit needs no upload, so
// a steady stream of re-submitted device batches never forces dbg_agg_reset to synchronise.
int submit_batch(dbg_agg_handle* h, BatchDesc** pst, u32* pbid, bool cacheable) {
    BatchDesc* st = *pst;
    u32 bid = *pbid;
    if (cacheable && bid == h->n_cached + 1 && h->desc_cache.size() < 64) {
        u64 hv = desc_hash(*st);
        u32 hit = 0;
        for (u32 k = 0; k < h->desc_cache.size() && !hit; ++k)
            if (h->desc_cache[k].first == hv && memcmp(&h->desc_cache[k].second, st, sizeof(BatchDesc)) == 0) hit = k + 1;
        if (hit) {
            h->n_batches = bid - 1;  // give the fresh id back
            *pbid = hit;
            *pst = &h->desc_cache[hit - 1].second;
            return DBG_OK;
        }
        RETURN_IF(upload_batch(h, st, bid));
        h->desc_cache.push_back({hv, *st});
        h->n_cached = bid;
        return DBG_OK;
    }
    return upload_batch(h, st, bid);
}

// The validity of a non-nullable type is dropped: no kernel reads it (dcol_valid, device.hpp, and
// the sorts' has_nulls test `nullable` first); the bit offsets are read only with their bitmaps.
DCol dcol_view(const dbg_column& c) {
    DCol d;
    memset(&d, 0, sizeof(d));
    d.type = c.dt.type;
    d.precision = c.dt.precision;
    d.scale = c.dt.scale;
    d.nullable = c.dt.nullable;
    d.layout = LAYOUT_ARROW;
    d.width = type_width(c.dt.type);
    d.stride = d.width;
    d.data = (const u8*)c.data;
    d.offsets = c.offsets;
    d.validity = c.dt.nullable ? c.validity : nullptr;
    d.validity_offset = c.validity_offset;
    d.data_offset = c.data_offset;
    return d;
}

// dbg_column (host or device) -> DCol on device
int to_dcol(Owner o, const dbg_column& c, const dbg_datatype& want, bool check_type, int on_device, DCol& d) {
    if (!valid_type(c.dt.type)) return fail(DBG_ERR_INVALID, "bad column type");
    if (check_type && (c.dt.type != want.type || ((c.dt.type == DBG_DECIMAL128 || c.dt.type == DBG_DECIMAL256) && c.dt.scale != want.scale)))
        return fail(DBG_ERR_INVALID, "column type does not match the declared type");
    if (check_type && c.dt.nullable && !want.nullable) return fail(DBG_ERR_INVALID, "nullable column for a non-nullable declared type");
    d = dcol_view(c);
    if (check_type) d.nullable = want.nullable;
    if (on_device) return DBG_OK;
    // host: copy what the rows need and point at the copies (the bit offsets stay the caller's)
    d.data = d.validity = nullptr;
    d.offsets = nullptr;
    const u64 n = c.len;
    const void* p = nullptr;
    if (c.dt.type == DBG_STRING) {
        u64 lo = n ? c.offsets[0] : 0, hi = n ? c.offsets[n] : 0;
        // copy offsets rebased to 0 and the payload slice
        std::vector<uint64_t> offs(n + 1);
        for (u64 i = 0; i <= n; ++i) offs[i] = c.offsets[i] - lo;
        RETURN_IF(own_copy(o, offs.data(), (n + 1) * 8, &p));
        d.offsets = (const u64*)p;
        // the staging vector dies here: make the copy synchronous w.r.t. it
        HIPCHECK(hipStreamSynchronize(o.stream));
        RETURN_IF(own_copy(o, (const u8*)c.data + lo, hi - lo, &p));
        d.data = (const u8*)p;
    } else if (c.dt.type == DBG_BOOLEAN) {
        u64 bytes = (c.data_offset + n + 7) / 8;
        RETURN_IF(own_copy(o, c.data, bytes, &p));
        d.data = (const u8*)p;
    } else {
        RETURN_IF(own_copy(o, c.data, n * d.width, &p));
        d.data = (const u8*)p;
    }
    if (c.dt.nullable && c.validity) {
        u64 bytes = (c.validity_offset + n + 7) / 8;
        RETURN_IF(own_copy(o, c.validity, bytes, &p));
        d.validity = (const u8*)p;
    }
    return DBG_OK;
}

// A DBG_PRED_LIKE node's pattern, classified (the checks of the header, shared with the host entry
// points of abi_ops.hip)
int like_check(const uint8_t* pat, uint64_t len, LikeDesc& L) {
    if (!pat && len) return fail(DBG_ERR_INVALID, "LIKE: null pattern with a length");
    if (len > DBG_LIKE_MAX_PATTERN)
        return fail(DBG_ERR_UNSUPPORTED, "LIKE: patterns of at most " + std::to_string(DBG_LIKE_MAX_PATTERN) + " bytes");
    if (!like_classify(pat, len, L))
        return fail(DBG_ERR_UNSUPPORTED, "LIKE: at most " + std::to_string(DBG_LIKE_MAX_SEGMENTS) + " %-separated segments");
    return DBG_OK;
}

int fill_filter(Owner o, const dbg_filter* f, int on_device, u64 rows, DCol* cols, int* ncols, DNode* nodes, int* nnodes) {
    if (f->n_cols > DBG_MAX_FCOLS || f->n_nodes > DBG_MAX_NODES) return fail(DBG_ERR_UNSUPPORTED, "filter too large");
    // predicates compare at most two words (cmp3_i128): no Decimal256 filter columns
    for (int c = 0; c < f->n_cols; ++c) REFUSE_DECIMAL256(f->cols[c].dt.type, "filter");
    int depth = 0;
    LikeDesc likes[DBG_MAX_NODES];  // of the LIKE nodes, by node index
    for (int k = 0; k < f->n_nodes; ++k) {
        const dbg_pred_node& n = f->nodes[k];
        DNode& d = nodes[k];
        memset(&d, 0, sizeof(d));
        d.op = n.op;
        d.cmp = n.cmp;
        d.col = n.col;
        d.col2 = n.col2;
        d.i64v = n.i64;
        d.f64v = n.f64;
        d.lo = n.i128_lo;
        d.hi = n.i128_hi;
        if (n.op == DBG_PRED_CMP_CONST || n.op == DBG_PRED_CMP_COLS || n.op == DBG_PRED_IS_NULL || n.op == DBG_PRED_IS_NOT_NULL ||
            n.op == DBG_PRED_LIKE) {
            if (n.col < 0 || n.col >= f->n_cols || (n.op == DBG_PRED_CMP_COLS && (n.col2 < 0 || n.col2 >= f->n_cols)))
                return fail(DBG_ERR_INVALID, "predicate column index out of range");
            if (n.op == DBG_PRED_LIKE) {
                if (f->cols[n.col].dt.type != DBG_STRING) return fail(DBG_ERR_INVALID, "LIKE: the column is not a String column");
                // the pre-pass reads offsets[0 .. rows] whatever the consumer kernel goes on to read
                if (f->cols[n.col].len < rows) return fail(DBG_ERR_INVALID, "LIKE: filter column shorter than rows");
                RETURN_IF(like_check(n.str, n.str_len, likes[k]));
            }
            if (n.op == DBG_PRED_CMP_COLS) {  // cmp_cols reads both cells as the left column's type
                const dbg_datatype &a = f->cols[n.col].dt, &b = f->cols[n.col2].dt;
                if (a.type != b.type) return fail(DBG_ERR_INVALID, "column comparison: the two columns differ in type");
                if (a.type == DBG_DECIMAL128 && a.scale != b.scale)
                    return fail(DBG_ERR_INVALID, "column comparison: the two Decimal columns differ in scale");
            }
            depth++;
        } else if (n.op == DBG_PRED_TRUE) {
            depth++;
        } else if (n.op == DBG_PRED_AND || n.op == DBG_PRED_OR) {
            if (depth < 2) return fail(DBG_ERR_INVALID, "malformed predicate program");
            depth--;
        } else if (n.op == DBG_PRED_NOT) {
            if (depth < 1) return fail(DBG_ERR_INVALID, "malformed predicate program");
        } else {
            return fail(DBG_ERR_INVALID, "unknown predicate op");
        }
        if (depth > 15) return fail(DBG_ERR_UNSUPPORTED, "predicate too deep");
        if (n.op == DBG_PRED_CMP_CONST && f->cols[n.col].dt.type == DBG_STRING) {
            const void* p = nullptr;
            RETURN_IF(own_copy(o, n.str, n.str_len, &p));
            d.str = (const u8*)p;
            d.str_len = n.str_len;
        }
    }
    if (f->n_nodes && depth != 1) return fail(DBG_ERR_INVALID, "malformed predicate program");
    for (int c = 0; c < f->n_cols; ++c) RETURN_IF(to_dcol(o, f->cols[c], f->cols[c].dt, false, on_device, cols[c]));
    // LIKE nodes: the batch's match bitmap, rows / 8 bytes each, owned like the batch's other
    // device copies (a retry, a rehash or the partitioned payload reads the predicate again later),
    // filled on the stream before the kernel that evaluates the program
    for (int k = 0; k < f->n_nodes; ++k) {
        if (f->nodes[k].op != DBG_PRED_LIKE) continue;
        const dbg_pred_node& n = f->nodes[k];
        if (!cols[n.col].offsets) return fail(DBG_ERR_INVALID, "String column without offsets");
        const void* p = nullptr;
        RETURN_IF(own_copy(o, n.str, n.str_len, &p));
        nodes[k].str = (const u8*)p;
        nodes[k].str_len = n.str_len;
        RETURN_IF(own_alloc(o, std::max<u64>(1, (rows + 63) / 64) * 8));
        u64* const mask = (u64*)(u8*)o.owned.back();
        nodes[k].mask = (const u8*)mask;
        prof::Scope ps("like_mask", o.stream);
        launch_like_mask(o.stream, cols[n.col], rows, likes[k], nodes[k].str, mask);
        HIPCHECK(hipGetLastError());
    }
    *ncols = f->n_cols;
    *nnodes = f->n_nodes;
    return DBG_OK;
}

// Radix-partitioned COUNT(*) insert of a high-cardinality batch (part.hip); buffers grow only.
static int part_insert(dbg_agg_handle* h, const BatchDesc* st, u32 bid, u64 rows, u32 sb, bool on_device_insert, bool was_clean) {
    (void)bid;
    const int width = (int)st->keys[0].width;
    size_t tb = part_temp_bytes(width, rows, sb, h->cap);
    if (!tb) return fail(DBG_ERR_INTERNAL, "rocprim radix_sort_keys sizing failed");
    if (tb > h->part_temp.cap()) RETURN_IF(h->part_temp.ensure(tb));
    RETURN_IF(h->part_sorted.ensure(rows, 1024));
    RETURN_IF(h->part_bounds.ensure((h->cap >> sb) + 1, 1024));
    prof::Scope ps("agg_insert", h->stream);
    const char* step = "";
    // an empty table whose initialisation is still deferred: the slice kernel writes every slot
    const bool empty = h->init_pending;
    h->init_pending = false;
    hipError_t e = launch_part_sort(h->stream, *st, rows, h->cap, sb, h->part_temp, h->part_temp.cap(), h->part_sorted, h->part_bounds,
                                    &step);
    // EXPERIMENT (EXP=1 build): DBG_X_PART_DIRECT=0 keeps the table stage in the insert
    static const bool direct_on = !(X_ENV("DBG_X_PART_DIRECT") && X_ENV("DBG_X_PART_DIRECT")[0] == '0');
    // (was_clean: no group since the last reset or recycling finalize, the slots EMPTY or their
    // initialisation pending — the slices may start from EMPTY either way)
    if (e == hipSuccess && (empty || was_clean) && h->recycle && on_device_insert && direct_on) {  // the table stage waits for the next call
        h->def_part = true;
        h->def_part_sb = sb;
        h->def_part_kw = width;
        return DBG_OK;
    }
    if (e == hipSuccess) e = launch_part_slices(h->stream, table_desc(h), sb, h->part_sorted, h->part_bounds, empty, &step);
    if (e != hipSuccess) return fail(DBG_ERR_DEVICE, std::string("partitioned insert (") + step + "): " + hipGetErrorString(e));
    return DBG_OK;
}

// The held-back table stage of a partitioned insert into an empty table: the regular slices.
int part_flush(dbg_agg_handle* h) {
    if (!h->def_part) return DBG_OK;
    h->def_part = false;
    h->init_pending = false;  // part_slice<EMPTY> writes every slot
    prof::Scope ps("part_slice", h->stream);
    const char* step = "";
    hipError_t e = launch_part_slices(h->stream, table_desc(h), h->def_part_sb, h->part_sorted, h->part_bounds, true, &step);
    if (e != hipSuccess) return fail(DBG_ERR_DEVICE, std::string("partitioned insert (") + step + "): " + hipGetErrorString(e));
    return DBG_OK;
}

// A keyless handle's batch (func.accumulate(place, columns, None, rows), AGG/transform_single_key.rs:
// 104-106): the reduce into per-workgroup partial states, then their merge into the state.  Nothing
// reads the batch's rows after these two kernels.
static int keyless_add(dbg_agg_handle* h, u32 bid, u64 rows, int on_device) {
    const u32 blocks = keyless_grid(rows);
    {
        prof::Scope ps("keyless_reduce", h->stream);
        launch_keyless_reduce(h->stream, h->dspec, h->dbatches + bid, rows, h->kpartials, blocks);
    }
    {
        prof::Scope ps("keyless_merge", h->stream);
        launch_keyless_merge(h->stream, h->dspec, h->kpartials, blocks, (u32)h->spec.stride_words, h->kstate);
    }
    HIPCHECK(hipGetLastError());
    h->kl_reduces++;
    if (!on_device) HIPCHECK(hipStreamSynchronize(h->stream));  // host path: synchronous like the reference processor
    return DBG_OK;
}

static int add_groups_now(dbg_agg_handle* h, const dbg_column* group_cols, const dbg_column* arg_cols, const dbg_filter* filter,
                          uint64_t rows, int on_device) {
    if (rows >= 0xFFFFFFFFULL) return fail(DBG_ERR_UNSUPPORTED, "a batch holds fewer than 2^32 rows");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_deferred(h));
    h->finalized = false;
    if (rows == 0) return DBG_OK;
    const Spec& S = h->spec;
    BatchDesc* st;
    u32 bid;
    const size_t owned0 = h->owned.size();
    const Owner own{h->stream, h->owned};
    RETURN_IF(new_batch(h, &st, &bid));
    st->rows = rows;
    for (int c = 0; c < S.n_keys; ++c) {
        if (group_cols[c].len < rows) return fail(DBG_ERR_INVALID, "group column shorter than rows");
        RETURN_IF(to_dcol(own, group_cols[c], S.key_types[c], true, on_device, st->keys[c]));
    }
    for (int a = 0; a < S.n_aggs; ++a) {
        if (S.aggs[a].arg_type < 0) continue;
        if (!arg_cols) return fail(DBG_ERR_INVALID, "missing aggregate arguments");
        dbg_datatype want{S.aggs[a].arg_type, 0, arg_cols[a].dt.scale, (uint8_t)S.aggs[a].arg_nullable, 0};
        if (arg_cols[a].len < rows) return fail(DBG_ERR_INVALID, "argument column shorter than rows");
        RETURN_IF(to_dcol(own, arg_cols[a], want, true, on_device, st->args[a]));
    }
    if (filter && filter->n_nodes) RETURN_IF(fill_filter(own, filter, on_device, rows, st->fcols, &st->n_fcols, st->nodes, &st->n_nodes));
    RETURN_IF(submit_batch(h, &st, &bid, on_device && h->owned.size() == owned0));
    if (is_keyless(S)) return keyless_add(h, bid, rows, on_device);
    // high cardinality: the radix-partitioned payload instead of the HBM table (pp.hip)
    if (!h->pp) RETURN_IF(pp_maybe_switch(h, bid, rows));
    if (h->pp) return pp_add_batch(h, st, bid, rows, 0);
    // A first batch the probe puts at many groups gets a table sized for them before its insert:
    // the partitioned insert needs a large table, and growing by overflow afterwards costs the
    // whole batch again (C3's first 1e9-row batch into the initial table: 1.5 s + a retry pass)
    // (AggregateHashTable::get_capacity_for_count: next_pow2(count * LOAD_FACTOR 1.5),
    // EAGG/aggregate_hashtable.rs:567-569, mod.rs:49 — 2x, the earlier rule, put C3's 1.34e8 groups
    // 0.06 % below 2^28 and any estimator overshoot doubled the table, a radix pass and both
    // finalize scans).  Best-effort: capped at half the free device memory, and a failed
    // allocation keeps the current table (overflow growth then sizes it by the rows it meets).
    if (h->table_rows == 0 && h->pp_probed && h->est_groups > 65536.0) {
        u64 target = pow2_at_least((u64)std::min(1.5 * h->est_groups + 1.0, (double)(1ULL << 31)));
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            while (target > h->cap && (double)(target + 1) * h->spec.tstride * 8.0 > 0.5 * (double)free_b) target >>= 1;
        if (target > h->cap && grow_table(h, target) != DBG_OK) {
            (void)hipGetLastError();
            g_last_error.clear();
        }
    }
    h->table_rows += rows;
    const bool was_clean = h->clean;
    h->clean = false;
    if (part_slice_bits(S, *st, rows, h->cap)) {
        // radix-partitioned insert: every row may become an overflow record (probe left its
        // slice).  ensure_ovf may resolve pending overflow (and resize): shape after it.
        RETURN_IF(ensure_ovf(h, 0, rows));
    }
    if (u32 sb = part_slice_bits(S, *st, rows, h->cap)) {
        RETURN_IF(part_insert(h, st, bid, rows, sb, on_device != 0, was_clean));
        if (!on_device) RETURN_IF(resolve_overflow(h));
        return DBG_OK;
    }
    // worst-case pushes of this launch: every row, and every LDS slot of every workgroup
    RETURN_IF(ensure_ovf(h, rows, 2 * ovf_blocks(rows) * 4096));
    if (on_device && h->recycle && h->hcounters_dev && insert_can_fuse(S, *st, h->cap)) {  // held back: see def_on
        h->def_on = true;
        h->def_clean = was_clean;
        h->def_bid = bid;
        h->def_rows = rows;
        h->def_hb = *st;
        return DBG_OK;
    }
    {
        prof::Scope ps("agg_insert", h->stream);
        note_insert(h, launch_insert(h->stream, h->dspec, S, h->dbatches, bid, rows, false, table_desc(h), true, st));
    }
    HIPCHECK(hipGetLastError());
    if (!on_device) RETURN_IF(resolve_overflow(h));  // host path: synchronous like the reference processor
    return DBG_OK;
}

// Staged host blocks -> one batch (host_stage.hpp).  The host path is synchronous (it resolves
// overflow before returning), so the staging vectors are free again when this returns.
int stage_flush(dbg_agg_handle* h) {
    if (h->stage.empty()) return DBG_OK;
    std::vector<dbg_column> k, a, fc;
    std::vector<dbg_pred_node> nd;
    dbg_filter flt;
    h->stage.views(k, a, fc, nd, flt);
    int rc = add_groups_now(h, k.data(), a.data(), flt.n_nodes ? &flt : nullptr, h->stage.rows, 0);
    if (rc == DBG_OK && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(DBG_ERR_DEVICE, "stream synchronize");
    h->stage.clear();
    return rc;
}

int flush_pending(dbg_agg_handle* h) {
    RETURN_IF(stage_flush(h));
    return flush_deferred(h);
}

extern "C" {
const char* dbg_version(void) { return "dbgpu_agg 0.1 (gfx950)"; }
const char* dbg_last_error(void) { return g_last_error.c_str(); }

int dbg_device_count(int* n) {
    HIPCHECK(hipGetDeviceCount(n));
    return DBG_OK;
}

int dbg_agg_create(const dbg_agg_params* params, dbg_agg_handle** out) {
    if (!params || !out) return fail(DBG_ERR_INVALID, "null argument");
    auto* h = new dbg_agg_handle();
    int rc = build_spec(params, h->spec, h->result_types);
    if (rc != DBG_OK) {
        delete h;
        return rc;
    }
    for (int a = 0; a < params->n_aggs; ++a) h->src_kinds.push_back(params->aggs[a].kind);
    h->partial = params->partial != 0;
    if (params->device >= 0) h->device = params->device;
    else {
        hipError_t e = hipGetDevice(&h->device);
        if (e != hipSuccess) {
            delete h;
            return fail(DBG_ERR_DEVICE, std::string("hipGetDevice: ") + hipGetErrorString(e));
        }
    }
    auto cleanup = [&](int code) {
        dbg_agg_destroy(h);
        return code;
    };
    if (hipSetDevice(h->device) != hipSuccess) return cleanup(fail(DBG_ERR_DEVICE, "hipSetDevice failed"));
    if (hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) return cleanup(fail(DBG_ERR_DEVICE, "hipStreamCreate failed"));
    h->stream = h->own_stream;
    if ((rc = h->counters.ensure(CNT_WORDS)) != DBG_OK) return cleanup(rc);
    if (hipMemset(h->counters, 0, CNT_WORDS * 8) != hipSuccess) return cleanup(fail(DBG_ERR_DEVICE, "memset"));
    h->spec.err = h->counters + CNT_ERR;  // error bits raised from inside state updates
    {
        const char* cx = getenv("DBG_X_PPSPEC_CAP");
        const char* fd = getenv("DBG_X_PPSPEC_DESC");
        h->spec.x_pp_cap = cx ? std::max<u32>(64, (u32)atoi(cx) & ~3u) : ~0u;
        h->spec.x_pp_desc = (fd && fd[0] == '1') ? 1 : 0;
    }
    if ((rc = h->dspec.ensure(1)) != DBG_OK) return cleanup(rc);
    if (hipMemcpy(h->dspec, &h->spec, sizeof(Spec), hipMemcpyHostToDevice) != hipSuccess) return cleanup(fail(DBG_ERR_DEVICE, "spec upload"));
    if ((rc = h->hcounters.ensure(CNT_WORDS + DBG_MAX_KEYS + 8)) != DBG_OK) return cleanup(rc);
    if (hipHostGetDevicePointer((void**)&h->hcounters_dev, h->hcounters.get(), 0) != hipSuccess) h->hcounters_dev = nullptr;
    if (is_keyless(h->spec)) {  // one state and a launch's partial states instead of the table
        if ((rc = h->kstate.ensure((u64)h->spec.stride_words)) != DBG_OK) return cleanup(rc);
        if ((rc = h->kpartials.ensure((u64)KEYLESS_MAX_BLOCKS * (u64)h->spec.stride_words)) != DBG_OK) return cleanup(rc);
        launch_keyless_init(h->stream, h->dspec, h->kstate);
        BatchDesc* st0;
        u32 bid0;
        if ((rc = new_batch(h, &st0, &bid0)) != DBG_OK) return cleanup(rc);
        h->n_batches = 0;
        if (hipStreamSynchronize(h->stream) != hipSuccess) return cleanup(fail(DBG_ERR_DEVICE, "sync"));
        *out = h;
        return DBG_OK;
    }
    // initial capacity: 2x the hint, or 1024 slots (the CPU table starts at 32768 =
    // AggregateHashTable::initial_capacity(); on the GPU growth is a cheap rehash kernel and a
    // small table keeps init / finalize scans short for low-cardinality queries: 4096 -> 1024
    // slots took C2's fused finalize from 13.3 to 11.4 us and C1's from 58 to 50 us)
    h->hint_groups = params->capacity_hint;
    u64 hint = params->capacity_hint ? params->capacity_hint : 512;
    h->cap = pow2_at_least(std::max<u64>(hint * 2, 1024));
    h->init_cap = h->cap;
    if ((rc = alloc_table(h, h->cap, h->slots)) != DBG_OK) return cleanup(rc);
    // parking rows for every workgroup of an insert launch (launch_insert caps its grid here)
    h->scr_blocks = DBG_INSERT_MAX_BLOCKS;
    if ((rc = h->scratch.ensure(scr_words(h->scr_blocks, (u32)h->spec.stride_words))) != DBG_OK) return cleanup(rc);
    // all of it: tickets and counts start at zero, and a row word that was never written must not
    // look like a tagged entry (fused_chain_tagged)
    if (hipMemset(h->scratch, 0, scr_words(h->scr_blocks, (u32)h->spec.stride_words) * 8) != hipSuccess)
        return cleanup(fail(DBG_ERR_DEVICE, "memset"));

    // the (empty) batch table
    BatchDesc* st;
    u32 bid;
    if ((rc = new_batch(h, &st, &bid)) != DBG_OK) return cleanup(rc);
    h->n_batches = 0;  // slot 0 reserved: ref entries always carry bid >= 1
    if (hipStreamSynchronize(h->stream) != hipSuccess) return cleanup(fail(DBG_ERR_DEVICE, "sync"));
    *out = h;
    return DBG_OK;
}

void dbg_agg_destroy(dbg_agg_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->switch_ev) hipEventDestroy(h->switch_ev);
    if (h->own_stream) hipStreamDestroy(h->own_stream);
    delete h;  // frees every buffer: on the handle's device, behind the synchronisation above
}

int dbg_agg_set_stream(dbg_agg_handle* h, void* s) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_deferred(h));
    hipStream_t ns = s ? (hipStream_t)s : h->own_stream;
    if (ns != h->stream) {
        // device-side hand-off: work queued on the new stream waits for everything queued on the
        // old one (no host synchronisation, so a caller can alternate streams per launch)
        if (!h->switch_ev) HIPCHECK(hipEventCreateWithFlags(&h->switch_ev, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(h->switch_ev, h->stream));
        HIPCHECK(hipStreamWaitEvent(ns, h->switch_ev, 0));
        h->stream = ns;
    }
    return DBG_OK;
}

int dbg_agg_reset(dbg_agg_handle* h) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    HIPCHECK(hipSetDevice(h->device));
    h->def_on = false;  // the held-back insert is discarded with the groups
    h->def_part = false;
    h->stage.clear();   // and so are staged host rows
    // inputs copied by earlier batches, and the pinned batch descriptors reused below, may still
    // be read by queued work: wait if any were queued since the last synchronisation
    if (!h->owned.empty() || h->uploads_pending) {
        HIPCHECK(hipStreamSynchronize(h->stream));
        h->owned.clear();
        h->uploads_pending = false;
    }
    h->n_batches = h->n_cached;  // cached descriptors stay valid (immutable)
    h->pending_rows = h->pending_recs = 0;
    h->finalized = false;
    if (is_keyless(h->spec)) {  // the state back to its initial words, in stream order
        prof::Scope ps("keyless_init", h->stream);
        launch_keyless_init(h->stream, h->dspec, h->kstate);
        return DBG_OK;
    }
    h->table_rows = 0;
    h->remerged = 0;
    h->xrecv_busy = false;  // no group references the exchange's receive buffers any more
    h->xchunks.clear();  // an abandoned chunked shuffle (the last call never came): its buffers are the communicator's
    h->xfirst[0] = h->xfirst[1] = 0;
    for (auto& K : h->ppk) {  // partitioned payload: records dropped, buffers kept (the mode too)
        K.l1_n = 0;
        K.dig_n = 0;
        K.segs.clear();
    }
    h->pp_grec_ready = false;
    if (h->clean) return DBG_OK;  // the recycling finalize already re-initialised table + counters
    // the counters and the sentinel slot now; the slots when a kernel first touches the table
    // (table_desc), or never if a partitioned insert rewrites every slice first
    prof::Scope ps("table_init", h->stream);
    launch_table_init(h->stream, h->dspec, h->spec, h->slots + h->cap * (u64)h->spec.tstride, 0, h->counters);
    h->init_pending = true;
    h->clean = true;
    return DBG_OK;
}

int dbg_agg_add_groups(dbg_agg_handle* h, const dbg_column* group_cols, const dbg_column* arg_cols, const dbg_filter* filter,
                       uint64_t rows, int on_device) {
    if (!h || (!group_cols && h->spec.n_keys)) return fail(DBG_ERR_INVALID, "null argument");
    HIPCHECK(hipSetDevice(h->device));
    hstage::Stage& G = h->stage;
    if (on_device || !G.cap || rows >= G.cap) {
        RETURN_IF(stage_flush(h));
        return add_groups_now(h, group_cols, arg_cols, filter, rows, on_device);
    }
    const Spec& S = h->spec;
    // the checks add_groups_now would make, before the rows are accepted
    for (int c = 0; c < S.n_keys; ++c) {
        const dbg_column& g = group_cols[c];
        if (g.len < rows) return fail(DBG_ERR_INVALID, "group column shorter than rows");
        if (g.dt.type != S.key_types[c].type || (g.dt.type == DBG_DECIMAL128 && g.dt.scale != S.key_types[c].scale) ||
            (g.dt.nullable && !S.key_types[c].nullable))
            return fail(DBG_ERR_INVALID, "column type does not match the declared type");
    }
    for (int a = 0; a < S.n_aggs; ++a) {
        if (S.aggs[a].arg_type < 0) continue;
        if (!arg_cols) return fail(DBG_ERR_INVALID, "missing aggregate arguments");
        if (arg_cols[a].len < rows) return fail(DBG_ERR_INVALID, "argument column shorter than rows");
        if (arg_cols[a].dt.type != S.aggs[a].arg_type) return fail(DBG_ERR_INVALID, "column type does not match the declared type");
    }
    if (filter && filter->n_nodes)
        for (int c = 0; c < filter->n_cols; ++c)
            if (filter->cols[c].len < rows) return fail(DBG_ERR_INVALID, "filter column shorter than rows");
    if (!G.empty() && (G.rows + rows > G.cap || !G.same_filter(filter))) RETURN_IF(stage_flush(h));
    if (rows == 0) return DBG_OK;
    int32_t arg_types[DBG_MAX_AGGS];
    for (int a = 0; a < S.n_aggs; ++a) arg_types[a] = S.aggs[a].arg_type;
    G.append(S.n_keys, group_cols, S.n_aggs, arg_cols, arg_types, filter, rows);
    h->finalized = false;
    return DBG_OK;
}

int dbg_agg_set_host_staging(dbg_agg_handle* h, uint64_t rows) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(stage_flush(h));
    h->stage.cap = rows >= 0xFFFFFFFFULL ? 0xFFFFFFFEULL : rows;
    return DBG_OK;
}

int dbg_agg_set_strategy(dbg_agg_handle* h, int strategy) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    if (strategy < DBG_STRATEGY_AUTO || strategy > DBG_STRATEGY_PARTITIONED) return fail(DBG_ERR_INVALID, "unknown strategy");
    if (strategy == DBG_STRATEGY_PARTITIONED) REFUSE_KEYLESS(h, "dbg_agg_set_strategy(PARTITIONED)");
    if (strategy == DBG_STRATEGY_PARTITIONED) REFUSE_HANDLE_LOCAL(h, "dbg_agg_set_strategy(PARTITIONED)");
    if (h->table_rows || h->ppk[0].l1_n || h->ppk[1].l1_n)
        return fail(DBG_ERR_INVALID, "dbg_agg_set_strategy: the handle holds groups (call it after create or reset)");
    // AUTO switches only for records of <= 256 bytes (build_spec: pp_ok); a forced partitioned
    // payload runs up to the scatter's limit: a tile needs one wave of 64 rows in its 32 KiB
    // scratch (pp_direct_t > 0, i.e. records of <= 512 bytes) and <= 64 state words per group
    const Spec& PS = h->spec;
    const bool pp_fits = pp_direct_t(PS.pp_rw_raw) > 0 && pp_direct_t(PS.pp_rw_state) > 0 && PS.pp_sw <= 64;
    if (strategy == DBG_STRATEGY_PARTITIONED && !pp_fits)
        return fail(DBG_ERR_UNSUPPORTED, "dbg_agg_set_strategy: records too wide for the partitioned payload");
    h->strategy = strategy;
    h->pp = strategy == DBG_STRATEGY_PARTITIONED;
    // a new strategy starts a new query on the handle: forget the cardinality the last finalize saw
    h->obs_rows = h->obs_groups = 0;
    return DBG_OK;
}

int dbg_agg_get_strategy(dbg_agg_handle* h, int* partitioned, uint64_t* extra_rounds) {
    if (!h || !partitioned) return fail(DBG_ERR_INVALID, "null argument");
    *partitioned = h->pp ? (h->pp_spec >= 0 ? 2 : 1) : 0;
    if (extra_rounds) *extra_rounds = h->pp_stat_rounds;
    return DBG_OK;
}

int dbg_agg_get_pp_stats(dbg_agg_handle* h, uint32_t* final_bits, uint64_t* spilled_partitions) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    if (final_bits) *final_bits = h->pp_bits;
    if (spilled_partitions) *spilled_partitions = h->pp_stat_spilled;
    return DBG_OK;
}

int dbg_agg_insert_paths(dbg_agg_handle* h, uint64_t* counts, int32_t n) {
    if (!h || !counts || n < 0) return fail(DBG_ERR_INVALID, "null argument");
    for (int32_t i = 0; i < n; ++i) counts[i] = i < INS_N_PATHS ? h->insert_paths[i] : 0;
    return DBG_OK;
}

int dbg_agg_set_partition_keys(dbg_agg_handle* h, int n_keys) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    REFUSE_KEYLESS(h, "dbg_agg_set_partition_keys");
    if (n_keys < 0 || n_keys > h->spec.n_keys) return fail(DBG_ERR_INVALID, "partition keys: 0..n_group_cols");
    h->part_keys = n_keys;
    return DBG_OK;
}

int dbg_agg_set_recycle(dbg_agg_handle* h, int on) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    if (on) REFUSE_KEYLESS(h, "dbg_agg_set_recycle(1)");
    h->recycle = on ? 1 : 0;
    return DBG_OK;
}

int dbg_agg_capacity(dbg_agg_handle* h, uint64_t* slots) {
    if (!h || !slots) return fail(DBG_ERR_INVALID, "null argument");
    REFUSE_KEYLESS(h, "dbg_agg_capacity");
    *slots = h->cap;
    return DBG_OK;
}

int dbg_agg_keyless_stats(dbg_agg_handle* h, uint64_t* reduce_launches, uint64_t* merged_states) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    if (!is_keyless(h->spec)) return fail(DBG_ERR_INVALID, "dbg_agg_keyless_stats: the handle has group columns");
    if (reduce_launches) *reduce_launches = h->kl_reduces;
    if (merged_states) *merged_states = h->kl_merged;
    return DBG_OK;
}
}  // extern "C"
