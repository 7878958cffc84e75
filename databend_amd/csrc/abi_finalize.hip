// abi_finalize.hip — both finalize families of a handle: dbg_agg_finalize + dbg_agg_result[_serialized]
// (sizes first, then the columns), and dbg_agg_finalize_into[_async] / dbg_agg_finalize_wait (the
// caller's buffers, one fused round: fin_setup / fin_launch / fin_complete), with dbg_agg_step_async
// (reset + device batch + that round's launch in one call).  The table's growth
// and overflow are abi.hip's, the partitioned payload's ends of both families abi_pp.hip's.
#include "abi_exp.hpp"

static void note_observed(dbg_agg_handle* h) {
    // compaction's re-merged group records are not input rows: leave them out of the ratio
    const u64 rows = h->table_rows > h->remerged ? h->table_rows - h->remerged : 0;
    if (h->pp || !rows) return;
    h->obs_rows = rows;
    h->obs_groups = h->n_groups;
}

static void publish_groups(const dbg_agg_handle* h, uint64_t* n_groups, uint64_t* string_bytes) {
    if (n_groups) *n_groups = h->n_groups;
    if (string_bytes)
        for (int c = 0; c < h->spec.n_keys; ++c) string_bytes[c] = h->string_bytes[c];
}

bool groups_known(dbg_agg_handle* h, u64 groups, const u64* str_tot, const FinState* caps, uint64_t* n_groups,
                  uint64_t* string_bytes) {
    const Spec& S = h->spec;
    h->n_groups = groups;
    note_observed(h);
    h->string_bytes.assign(S.n_keys, 0);
    bool short_buf = caps && groups > caps->max_groups;
    for (int c = 0; c < S.n_keys; ++c) {
        if (S.key_types[c].type != DBG_STRING) continue;  // (String keys are never inline keys)
        h->string_bytes[c] = str_tot[c];
        if (caps && str_tot[c] > caps->cap_str[c]) short_buf = true;
    }
    publish_groups(h, n_groups, string_bytes);
    return short_buf;
}

// table mode: every claimed slot is a group
static int check_claims(const dbg_agg_handle* h) {
    if (h->n_groups == h->hcounters[CNT_CLAIMS]) return DBG_OK;
    return fail(DBG_ERR_INTERNAL, "group count mismatch: " + std::to_string(h->n_groups) + " vs claims " +
                                      std::to_string(h->hcounters[CNT_CLAIMS]));
}

// Before a table-wide write: per-block group counts and String key bytes, scanned into write
// positions; the totals land at d_pos + nb ([0] groups, [1 + c] bytes of String key column c).
static void count_and_scan(dbg_agg_handle* h, const TableDesc& t, u64 nb) {
    const Spec& S = h->spec;
    u64* totals = h->d_pos + nb;
    prof::Scope ps("count_groups", h->stream);
    launch_count_groups(h->stream, h->dspec, S, h->dbatches, t, 1, 0, nullptr, h->d_pos, h->d_str_pos);
    launch_exclusive_scan(h->stream, h->d_pos, nb, totals);
    if (S.has_strings && !S.inline_keys)
        for (int c = 0; c < S.n_keys; ++c)
            if (S.key_types[c].type == DBG_STRING) launch_exclusive_scan(h->stream, h->d_str_pos + (u64)c * nb, nb, totals + 1 + c);
}

// a result that is never NULL for a group: the aggregate's argument is never NULL (COUNT(*) or a
// non-nullable column), and SUM / AVG / MIN / MAX of one or more values is a value
static bool agg_always_valid(const DAgg& A) {
    return A.arg_type < 0 || !A.arg_nullable;
}

// Payload bytes of every String MIN/MAX result column (h->agg_string_bytes): one pass over the
// table's groups that follows each state's row reference to its length.
static int str_agg_totals(dbg_agg_handle* h) {
    const Spec& S = h->spec;
    if (!has_str_minmax(S)) return DBG_OK;
    h->agg_string_bytes.assign(S.n_aggs, 0);
    if (h->n_groups == 0) return DBG_OK;
    Buf<u64> dtot;
    RETURN_IF(dtot.ensure(S.n_aggs));
    hipError_t e = hipMemsetAsync(dtot, 0, 8ull * S.n_aggs, h->stream);
    if (e == hipSuccess) {
        prof::Scope ps("str_agg_bytes", h->stream);
        launch_str_agg_bytes(h->stream, h->dspec, h->dbatches, table_desc(h), dtot);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h->agg_string_bytes.data(), dtot, 8ull * S.n_aggs, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(DBG_ERR_DEVICE, std::string("string aggregate sizes: ") + hipGetErrorString(e));
    return DBG_OK;
}

static int result_impl(dbg_agg_handle* h, dbg_out_column* out_aggs, dbg_out_column* out_keys, int on_device, bool ser) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    if (!h->finalized) return fail(DBG_ERR_INVALID, "dbg_agg_finalize must precede dbg_agg_result");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    const Spec& S = h->spec;
    u64 n = h->n_groups;
    for (int a = 0; a < S.n_aggs; ++a) out_aggs[a].dt = ser ? dbg_datatype{DBG_STRING, 0, 0, 0, 0} : h->result_types[a];
    for (int c = 0; c < S.n_keys; ++c) out_keys[c].dt = S.key_types[c];
    if (n == 0) {  // no groups: every offsets column is its first offset
        auto zero_first_offset = [&](dbg_out_column& o) -> int {
            const u64 z = 0;
            if (o.offsets && on_device) HIPCHECK(hipMemcpy(o.offsets, &z, 8, hipMemcpyHostToDevice));
            else if (o.offsets) o.offsets[0] = 0;
            return DBG_OK;
        };
        for (int c = 0; c < S.n_keys; ++c)
            if (S.key_types[c].type == DBG_STRING) RETURN_IF(zero_first_offset(out_keys[c]));
        for (int a = 0; a < S.n_aggs; ++a)
            if (ser || is_str_minmax(S.aggs[a])) RETURN_IF(zero_first_offset(out_aggs[a]));
        return DBG_OK;
    }
    std::vector<DevBuf> temps;  // freed on every way out
    auto tmp = [&](size_t bytes, void** p) -> int {
        DevBuf b;
        RETURN_IF(b.ensure(bytes));
        *p = b.get();
        temps.push_back(std::move(b));
        return DBG_OK;
    };
    // a host caller's column, where it asked for one: copied out of its temporary
    auto to_host = [&](void* dst, const void* src, size_t bytes) {
        if (!on_device && dst && bytes) hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream);
    };
    // validity bytes (nullptr: every group valid) -> the column's validity bits
    auto pack_validity = [&](const u8* vbytes, const dbg_out_column& out) -> int {
        u8* bits = on_device ? out.validity : nullptr;
        if (!on_device && tmp((n + 7) / 8, (void**)&bits) != DBG_OK) return DBG_ERR_OOM;
        if (bits && vbytes) launch_pack_bits(h->stream, vbytes, n, bits);
        else if (bits) launch_fill_valid(h->stream, n, bits);
        to_host(out.validity, bits, (n + 7) / 8);
        return DBG_OK;
    };
    // where the device writes a column: the caller's device buffer, or a temporary copied out below
    auto dest = [&](void* callers, size_t bytes, void** p) -> int {
        *p = callers;
        return on_device ? DBG_OK : tmp(bytes, p);
    };
    OutDesc od;
    memset(&od, 0, sizeof(od));
    od.cap_groups = n;
    for (int c = 0; c < S.n_keys; ++c) od.cap_str[c] = h->string_bytes[c];
    int rc = DBG_OK;
    for (int c = 0; c < S.n_keys && rc == DBG_OK; ++c) {
        const dbg_datatype& t = S.key_types[c];
        rc = dest(out_keys[c].data, t.type == DBG_STRING ? h->string_bytes[c] : n * type_width(t.type), &od.key_data[c]);
        if (rc == DBG_OK && t.type == DBG_STRING) rc = dest(out_keys[c].offsets, (n + 1) * 8, (void**)&od.key_offsets[c]);
        if (rc == DBG_OK && t.nullable) rc = tmp(n, (void**)&od.key_valid[c]);
    }
    for (int a = 0; a < S.n_aggs && rc == DBG_OK; ++a) {
        const dbg_datatype& t = h->result_types[a];
        if (ser) {  // fixed-stride rows + lengths, compacted into Binary columns below
            od.ser = 1;
            od.ser_stride[a] = ser_stride_of(S.aggs[a]);
            rc = tmp(n * od.ser_stride[a], &od.agg_data[a]);
            if (rc == DBG_OK) rc = tmp(n, (void**)&od.agg_valid[a]);
            continue;
        }
        if (is_str_minmax(S.aggs[a])) rc = tmp(n * 8, &od.agg_data[a]);  // row references, gathered below
        else rc = dest(out_aggs[a].data, n * type_width(t.type), &od.agg_data[a]);
        if (rc == DBG_OK && t.nullable) {
            // (a keyless result is NULL for the empty input, whatever the argument)
            if (agg_always_valid(S.aggs[a]) && !is_keyless(S)) od.all_valid |= 1u << a;
            else rc = tmp(n, (void**)&od.agg_valid[a]);
        }
    }
    RETURN_IF(rc);
    if (is_keyless(S)) {
        prof::Scope ps("keyless_write", h->stream);
        launch_keyless_write(h->stream, h->dspec, h->kstate, od, h->counters + CNT_ERR);
    } else if (h->pp) {
        prof::Scope ps("pp_write", h->stream);
        launch_pp_grec_write(h->stream, h->dspec, h->dbatches, h->pp_grec, h->pp_tot, h->pp_blk, h->pp_nb, od,
                             h->counters + CNT_ERR);
    } else {
        prof::Scope ps("write_results", h->stream);
        launch_write_results(h->stream, h->dspec, S, h->dbatches, table_desc(h), h->d_pos, h->d_str_pos, od);
    }
    // offsets[n] and bit-packed validity
    for (int c = 0; c < S.n_keys; ++c) {
        const dbg_datatype& t = S.key_types[c];
        if (t.type == DBG_STRING) hipMemcpyAsync(od.key_offsets[c] + n, &h->string_bytes[c], 8, hipMemcpyHostToDevice, h->stream);
        if (t.nullable) RETURN_IF(pack_validity(od.key_valid[c], out_keys[c]));
    }
    std::vector<u64> ser_tot(S.n_aggs, 0);
    u64* dser_tot = nullptr;
    if (ser) {
        if (tmp(8ull * S.n_aggs, (void**)&dser_tot) != DBG_OK) return DBG_ERR_OOM;
        for (int a = 0; a < S.n_aggs; ++a) {
            u64* offs = nullptr;
            u8* data = nullptr;
            if (dest(out_aggs[a].offsets, (n + 1) * 8, (void**)&offs) != DBG_OK || dest(out_aggs[a].data, n * od.ser_stride[a], (void**)&data) != DBG_OK)
                return DBG_ERR_OOM;
            launch_ser_compact(h->stream, od.agg_valid[a], (const u8*)od.agg_data[a], od.ser_stride[a], n, offs, data, dser_tot + a);
            if (!on_device) od.agg_data[a] = data;  // copied out below with the totals known
            to_host(out_aggs[a].offsets, offs, (n + 1) * 8);
        }
        HIPCHECK(hipMemcpyAsync(ser_tot.data(), dser_tot, 8ull * S.n_aggs, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        for (int a = 0; a < S.n_aggs; ++a) to_host(out_aggs[a].data, od.agg_data[a], ser_tot[a]);
    }
    // String MIN/MAX: the row references the writers emitted -> offsets and bytes of the values
    for (int a = 0; a < S.n_aggs && !ser; ++a) {
        if (!is_str_minmax(S.aggs[a])) continue;
        const u64 total = (size_t)a < h->agg_string_bytes.size() ? h->agg_string_bytes[a] : 0;
        if (on_device && (!out_aggs[a].offsets || (total && !out_aggs[a].data)))
            return fail(DBG_ERR_INVALID, "dbg_agg_result: a String aggregate needs offsets and data buffers");
        u64* offs = nullptr;
        u8* data = nullptr;
        if (dest(out_aggs[a].offsets, (n + 1) * 8, (void**)&offs) != DBG_OK || dest(out_aggs[a].data, total, (void**)&data) != DBG_OK)
            return DBG_ERR_OOM;
        {
            prof::Scope ps("str_gather", h->stream);
            launch_str_gather(h->stream, h->dbatches, a, (const u64*)od.agg_data[a], n, offs, data, total);
        }
        to_host(out_aggs[a].offsets, offs, (n + 1) * 8);
        to_host(out_aggs[a].data, data, total);
    }
    for (int a = 0; a < S.n_aggs && !ser; ++a)
        if (h->result_types[a].nullable) RETURN_IF(pack_validity(od.agg_valid[a], out_aggs[a]));
    for (int c = 0; c < S.n_keys; ++c) {
        const dbg_datatype& t = S.key_types[c];
        to_host(out_keys[c].data, od.key_data[c], t.type == DBG_STRING ? h->string_bytes[c] : n * type_width(t.type));
        if (t.type == DBG_STRING) to_host(out_keys[c].offsets, od.key_offsets[c], (n + 1) * 8);
    }
    for (int a = 0; a < S.n_aggs && !ser; ++a)
        if (!is_str_minmax(S.aggs[a])) to_host(out_aggs[a].data, od.agg_data[a], n * type_width(h->result_types[a].type));
    HIPCHECK(hipMemcpyAsync(h->hcounters, h->counters, CNT_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
    hipError_t e = hipStreamSynchronize(h->stream);  // nothing reads the temporaries past it
    if (e != hipSuccess) return fail(DBG_ERR_DEVICE, std::string("result: ") + hipGetErrorString(e));
    if (h->hcounters[CNT_ERR] & ERR_DEC_OVERFLOW) {
        HIPCHECK(hipMemsetAsync(h->counters + CNT_ERR, 0, 8, h->stream));
        return fail(DBG_ERR_OVERFLOW, "Decimal overflow");
    }
    return DBG_OK;
}

// The next finalize's sequence number.  Its low bits tag the parked words of the tagged fused
// chain (agg.hip), where tag 0 belongs to no launch (a cleared word never validates): multiples of
// the tag period are skipped.
static u64 next_fin_seq(dbg_agg_handle* h) {
    if ((++h->fin_seq & (FIN_SEQ_TAG_PERIOD - 1)) == 0) ++h->fin_seq;
    return h->fin_seq;
}

// Fused finalize, split into launch and completion so a caller can overlap the device work with
// other launches (dbg_agg_finalize_into_async / dbg_agg_finalize_wait).
static int fin_launch(dbg_agg_handle* h) {
    FinState& F = h->fin;
    const Spec& S = h->spec;
    RETURN_IF(stage_flush(h));  // staged host rows first (this launches any held-back insert)
    u64 nb = finalize_blocks(h->cap);
    RETURN_IF(h->d_pos.ensure(nb + 16, 1024));
    RETURN_IF(h->d_str_pos.ensure((u64)S.n_keys * nb + 8, 1024));
    // the held-back partitioned insert's table stage writes the result columns directly (one
    // non-nullable integer key, COUNT(*): what part_slice_bits admits; the table stays empty)
    const bool direct = h->def_part && !h->pp && S.n_keys == 1 && S.n_aggs == 1 && !S.key_types[0].nullable &&
                        !h->result_types[0].nullable && type_width(h->result_types[0].type) == 8 && F.keys[0].data && F.aggs[0].data &&
                        type_width(S.key_types[0].type) == (u32)h->def_part_kw;
    if (direct) {
        h->def_part = false;
        RETURN_IF(h->part_status.ensure(part_direct_status_words(h->cap, h->def_part_sb), 1024));
    }
    TableDesc t = direct ? TableDesc{} : table_desc(h);
    const bool small = h->cap + 1 <= FIN_SMALL_SLOTS;
    const bool fuse = h->def_on && !h->pp && small && h->hcounters_dev && insert_can_fuse(S, h->def_hb, h->cap);
    if (!fuse) RETURN_IF(flush_deferred(h));
    u64* totals = h->d_pos + nb;
    F.direct = direct;
    if (!small && !h->pp && !direct) count_and_scan(h, t, nb);
    OutDesc od;
    memset(&od, 0, sizeof(od));
    od.cap_groups = F.max_groups;
    u8* vb = h->vbytes;
    for (int c = 0; c < S.n_keys; ++c) {
        od.key_data[c] = F.keys[c].data;
        od.key_offsets[c] = S.key_types[c].type == DBG_STRING ? F.keys[c].offsets : nullptr;
        od.cap_str[c] = (S.key_types[c].type == DBG_STRING && F.has_max_str) ? F.max_str[c] : 0;
        F.cap_str[c] = od.cap_str[c];
        if (S.key_types[c].nullable) {
            od.key_valid[c] = vb;
            od.key_bits[c] = F.keys[c].validity;
            vb += F.max_groups + 1;
        }
    }
    for (int a = 0; a < S.n_aggs; ++a) {
        od.agg_data[a] = F.aggs[a].data;
        if (h->result_types[a].nullable) {
            od.agg_bits[a] = F.aggs[a].validity;
            if (agg_always_valid(S.aggs[a])) {
                od.all_valid |= 1u << a;
            } else {
                od.agg_valid[a] = vb;
                vb += F.max_groups + 1;
            }
        }
    }
    if (h->pp) {
        F.zero_copy = false;
        F.seq = next_fin_seq(h);
        RETURN_IF(pp_fin_launch(h, od));
        F.active = true;
        return DBG_OK;
    }
    F.zero_copy = small && !direct && h->hcounters_dev != nullptr;
    F.seq = next_fin_seq(h);
    if (direct) {
        prof::Scope ps("part_direct", h->stream);
        TableDesc td{};
        td.slots = h->slots;
        td.cap = h->cap;
        hipError_t e = launch_part_direct(h->stream, td, h->def_part_sb, h->part_sorted, h->part_bounds, h->part_status,
                                          h->def_part_kw, od.key_data[0], (u64*)od.agg_data[0], od.cap_groups, totals);
        if (e != hipSuccess) return fail(DBG_ERR_DEVICE, std::string("partitioned insert (direct stage): ") + hipGetErrorString(e));
        launch_finish_outputs(h->stream, od, totals, S.n_keys, S.n_aggs);
    } else if (fuse) {  // the held-back insert and this finalize in one launch
        FusedFin ff;
        ff.out = od;
        ff.totals = totals;
        ff.host_mirror = h->hcounters_dev;
        ff.seq = F.seq;
        ff.recycle = h->recycle;
        ff.on = 1;
        ff.table_empty = h->def_clean ? 1 : 0;
        ff.chain_tagged = 0;  // launch_fast_t decides, from its grid
        ff.trace = nullptr;
        ff.dense = nullptr;
        ff.dense_n = 0;
        // The tagged chain accepts a parked word by its tag alone: when the tags have wrapped since
        // the scratch was last cleared, clear it again (behind every earlier launch of the handle),
        // so that no word of an earlier period can carry a current tag.
        if ((F.seq / FIN_SEQ_TAG_PERIOD) != h->scr_period) {
            HIPCHECK(hipMemsetAsync(h->scratch, 0, scr_words(h->scr_blocks, (u32)S.stride_words) * 8, h->stream));
            h->scr_period = F.seq / FIN_SEQ_TAG_PERIOD;
        }
        RETURN_IF(exp_fused_fin(h, F, ff));
        h->def_on = false;
        prof::Scope ps("agg_insert", h->stream);
        note_insert(h, launch_insert(h->stream, h->dspec, S, h->dbatches, h->def_bid, h->def_rows, false, t, true, &h->def_hb, &ff));
        exp_launch_returned();
    } else if (small) {
        prof::Scope ps("finalize_small", h->stream);
        launch_finalize_small(h->stream, h->dspec, h->dbatches, t, od, totals, F.zero_copy ? h->hcounters_dev : nullptr,
                              h->recycle && F.zero_copy, F.seq);
    } else {
        prof::Scope ps("write_results", h->stream);
        launch_write_results(h->stream, h->dspec, S, h->dbatches, t, h->d_pos, h->d_str_pos, od);
        launch_finish_outputs(h->stream, od, totals, S.n_keys, S.n_aggs);
    }
    if (!F.zero_copy) {
        HIPCHECK(hipMemcpyAsync(h->hcounters, h->counters, CNT_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipMemcpyAsync(h->hcounters + CNT_WORDS, totals, 8 * (S.n_keys + 1), hipMemcpyDeviceToHost, h->stream));
    }
    F.active = true;
    return DBG_OK;
}

// Wait for the launched round; *retry = the inserts had overflowed (now resolved: launch again).
static int fin_complete(dbg_agg_handle* h, bool* retry, uint64_t* n_groups, uint64_t* string_bytes) {
    FinState& F = h->fin;
    *retry = false;
    F.active = false;
    if (h->pp) return pp_fin_complete(h, n_groups, string_bytes);
    bool recycled = false;
    const bool direct_done = F.direct;
    if (!F.zero_copy) {
        HIPCHECK(hipStreamSynchronize(h->stream));
    } else {
        // the kernel posts `seq` last (after its write-through mirror stores): spin on it
        // instead of a stream synchronisation (whose wake-up costs several microseconds); after
        // ~20 ms fall back to the blocking wait (long queued inserts)
        volatile u64* hseq = h->hcounters + CNT_WORDS + 2 + DBG_MAX_KEYS;
        volatile u64* hcomp = h->hcounters + MIRROR_COMPACT;
        bool seen = false, compact = false;
        auto t0 = std::chrono::steady_clock::now();
        for (u64 it = 0;; ++it) {
            if (__atomic_load_n(hseq, __ATOMIC_ACQUIRE) == F.seq) {
                seen = true;
                break;
            }
            // the count-only fused finalize posts one word [seq | recycled | groups] when its
            // counters are known (every group claimed in the launch, no overflow)
            const u64 cw = __atomic_load_n(hcomp, __ATOMIC_ACQUIRE);
            if ((cw >> 25) == (F.seq & ((1ULL << 39) - 1))) {
                for (int w = 0; w < CNT_WORDS; ++w) h->hcounters[w] = 0;
                h->hcounters[CNT_CLAIMS] = cw & 0xFFFFFF;
                h->hcounters[CNT_WORDS] = cw & 0xFFFFFF;
                for (int c = 0; c < DBG_MAX_KEYS; ++c) h->hcounters[CNT_WORDS + 1 + c] = 0;
                h->hcounters[CNT_WORDS + 1 + DBG_MAX_KEYS] = (cw >> 24) & 1;
                seen = compact = true;
                break;
            }
            if ((it & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
            __builtin_ia32_pause();
        }
        if (seen) exp_completion_seen();
        else HIPCHECK(hipStreamSynchronize(h->stream));
        HIPCHECK(hipGetLastError());
        recycled = h->hcounters[CNT_WORDS + 1 + DBG_MAX_KEYS] != 0;
    }
    h->uploads_pending = false;
    if (F.direct) {
        F.direct = false;
        if (h->hcounters[CNT_WORDS] == ~0ULL) {
            // a slice held more keys than its slots, or the result columns are too short: the
            // regular table stage from the same sorted keys (the table was never written), then
            // the table finalize (which reports short buffers with the table intact)
            h->def_part = true;
            RETURN_IF(part_flush(h));
            *retry = true;
            return DBG_OK;
        }
        h->hcounters[CNT_CLAIMS] = h->hcounters[CNT_WORDS];  // the table's own counters were never touched
        recycled = true;
    }
    RETURN_IF(err_bits_fail(h->hcounters[CNT_ERR], ERR_OVF_LOST | ERR_MINMAX_SPIN | ERR_CHAIN_SPIN | ERR_FIXED_INCOMPLETE));
    if (h->hcounters[CNT_OVF_ROWS] || h->hcounters[CNT_OVF_RECS]) {
        RETURN_IF(resolve_overflow(h));
        *retry = true;
        return DBG_OK;
    }
    h->pending_rows = h->pending_recs = 0;
    const u64* tot = h->hcounters + CNT_WORDS;
    const bool short_buf = groups_known(h, tot[0], tot + 1, &F, n_groups, string_bytes);
    RETURN_IF(check_claims(h));
    h->finalized = true;
    if (recycled) {  // the table was re-initialised by the kernel, or never written (then its slots still wait)
        mark_recycled(h);
        h->init_pending = h->init_pending || direct_done;
    }
    if (h->hcounters[CNT_ERR] & ERR_DEC_OVERFLOW) {
        if (!recycled) HIPCHECK(hipMemsetAsync(h->counters + CNT_ERR, 0, 8, h->stream));
        return fail(DBG_ERR_OVERFLOW, "Decimal overflow");
    }
    if (short_buf) return fail(DBG_ERR_INVALID, "output buffers too small: " + std::to_string(h->n_groups) + " groups");
    return DBG_OK;
}

static int fin_setup(dbg_agg_handle* h, dbg_out_column* out_aggs, dbg_out_column* out_keys, uint64_t max_groups,
                     const uint64_t* max_string_bytes) {
    const Spec& S = h->spec;
    FinState& F = h->fin;
    for (int a = 0; a < S.n_aggs; ++a) out_aggs[a].dt = h->result_types[a];
    for (int c = 0; c < S.n_keys; ++c) out_keys[c].dt = S.key_types[c];
    F.aggs.assign(out_aggs, out_aggs + S.n_aggs);
    F.keys.assign(out_keys, out_keys + S.n_keys);
    F.max_groups = max_groups;
    F.has_max_str = max_string_bytes != nullptr;
    F.max_str.assign(S.n_keys, 0);
    if (max_string_bytes)
        for (int c = 0; c < S.n_keys; ++c) F.max_str[c] = max_string_bytes[c];
    // validity bytes staging (bit-packed into the caller's buffers by finish_outputs)
    int n_nullable = 0;
    for (int c = 0; c < S.n_keys; ++c) n_nullable += S.key_types[c].nullable ? 1 : 0;
    for (int a = 0; a < S.n_aggs; ++a) n_nullable += h->result_types[a].nullable ? 1 : 0;
    u64 need = (u64)n_nullable * (max_groups + 1);
    if (need > h->vbytes.cap()) RETURN_IF(h->vbytes.ensure(need, 4096));
    return DBG_OK;
}

extern "C" {
int dbg_agg_result_string_bytes(dbg_agg_handle* h, uint64_t* agg_string_bytes) {
    if (!h || !agg_string_bytes) return fail(DBG_ERR_INVALID, "null argument");
    if (!h->finalized) return fail(DBG_ERR_INVALID, "dbg_agg_finalize must precede dbg_agg_result_string_bytes");
    for (int a = 0; a < h->spec.n_aggs; ++a)
        agg_string_bytes[a] = (is_str_minmax(h->spec.aggs[a]) && (size_t)a < h->agg_string_bytes.size()) ? h->agg_string_bytes[a] : 0;
    return DBG_OK;
}

int dbg_agg_finalize(dbg_agg_handle* h, uint64_t* n_groups, uint64_t* string_bytes) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    if (is_keyless(h->spec)) {
        // one row always, from freshly initialised states when no row ever reached them
        // (FinalSingleStateAggregator::on_finish, AGG/transform_single_key.rs:212-245)
        h->n_groups = 1;
        h->string_bytes.clear();
        h->agg_string_bytes.assign(h->spec.n_aggs, 0);
        h->finalized = true;
        if (n_groups) *n_groups = 1;
        return DBG_OK;
    }
    if (h->pp) return pp_finalize(h, n_groups, string_bytes);
    const Spec& S = h->spec;
    // Optimistic single round trip: count + scan are enqueued behind the inserts and read back
    // together with the overflow counters; only when an insert overflowed does the table grow
    // (resolve_overflow) and the count run again.
    for (int round = 0; round < 3; ++round) {
        u64 nb = finalize_blocks(h->cap);
        RETURN_IF(h->d_pos.ensure(nb + 16, 1024));
        RETURN_IF(h->d_str_pos.ensure((u64)S.n_keys * nb + 8, 1024));
        count_and_scan(h, table_desc(h), nb);
        HIPCHECK(hipMemcpyAsync(h->hcounters, h->counters, CNT_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipMemcpyAsync(h->hcounters + CNT_WORDS, h->d_pos + nb, 8 * (S.n_keys + 1), hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        RETURN_IF(err_bits_fail(h->hcounters[CNT_ERR], ERR_OVF_LOST | ERR_MINMAX_SPIN | ERR_FIXED_INCOMPLETE));
        if (h->hcounters[CNT_OVF_ROWS] || h->hcounters[CNT_OVF_RECS]) {
            RETURN_IF(resolve_overflow(h));
            continue;
        }
        h->pending_rows = h->pending_recs = 0;
        const u64* tot = h->hcounters + CNT_WORDS;
        groups_known(h, tot[0], tot + 1, nullptr, nullptr, nullptr);  // the caller's outputs last, below
        RETURN_IF(check_claims(h));
        // keep the load factor sane for the next batch (the reference resizes at 1/1.5)
        if ((double)h->n_groups * 1.5 > (double)h->cap) {
            RETURN_IF(grow_table(h, pow2_at_least((u64)(h->n_groups * 2.0) + 1)));
            continue;  // positions depend on the slot layout: count again
        }
        RETURN_IF(str_agg_totals(h));
        h->finalized = true;
        publish_groups(h, n_groups, string_bytes);
        return DBG_OK;
    }
    return fail(DBG_ERR_INTERNAL, "finalize did not converge");
}

int dbg_agg_result(dbg_agg_handle* h, dbg_out_column* out_aggs, dbg_out_column* out_keys, int on_device) {
    return result_impl(h, out_aggs, out_keys, on_device, false);
}

int dbg_agg_serialized_stride(dbg_agg_handle* h, uint32_t* stride) {
    if (!h || !stride) return fail(DBG_ERR_INVALID, "null argument");
    REFUSE_HANDLE_LOCAL(h, "dbg_agg_serialized_stride");
    for (int a = 0; a < h->spec.n_aggs; ++a) {
        if (h->src_kinds[a] == DBG_AGG_AVG_SQL)
            return fail(DBG_ERR_UNSUPPORTED, "serialized states: SQL avg is sum and count in the reference plan");
        stride[a] = ser_stride_of(h->spec.aggs[a]);
    }
    return DBG_OK;
}

int dbg_agg_result_serialized(dbg_agg_handle* h, dbg_out_column* out_states, dbg_out_column* out_keys, int on_device) {
    if (!h) return fail(DBG_ERR_INVALID, "null handle");
    REFUSE_HANDLE_LOCAL(h, "dbg_agg_result_serialized");
    for (int a = 0; a < h->spec.n_aggs; ++a)
        if (h->src_kinds[a] == DBG_AGG_AVG_SQL)
            return fail(DBG_ERR_UNSUPPORTED, "serialized states: SQL avg is sum and count in the reference plan");
    return result_impl(h, out_states, out_keys, on_device, true);
}

int dbg_agg_finalize_into(dbg_agg_handle* h, dbg_out_column* out_aggs, dbg_out_column* out_keys, uint64_t max_groups,
                          const uint64_t* max_string_bytes, uint64_t* n_groups, uint64_t* string_bytes) {
    RETURN_IF(dbg_agg_finalize_into_async(h, out_aggs, out_keys, max_groups, max_string_bytes));
    return dbg_agg_finalize_wait(h, n_groups, string_bytes);
}

int dbg_agg_finalize_into_async(dbg_agg_handle* h, dbg_out_column* out_aggs, dbg_out_column* out_keys, uint64_t max_groups,
                                const uint64_t* max_string_bytes) {
    if (!h || !out_aggs) return fail(DBG_ERR_INVALID, "null argument");
    REFUSE_KEYLESS(h, "dbg_agg_finalize_into_async");
    if (!out_keys) return fail(DBG_ERR_INVALID, "null argument");
    // String MIN/MAX: no room for the aggregates' string sizes.  Decimal256 results go through the
    // same writers as dbg_agg_result, so that handle-local spec is served here.
    if (has_str_minmax(h->spec))
        return fail(DBG_ERR_UNSUPPORTED, std::string("dbg_agg_finalize_into_async: ") + handle_local_reason(h->spec));
    if (h->fin.active) return fail(DBG_ERR_INVALID, "a finalize is already in flight: dbg_agg_finalize_wait first");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(fin_setup(h, out_aggs, out_keys, max_groups, max_string_bytes));
    return fin_launch(h);
}

// One device batch into result columns: dbg_agg_reset + dbg_agg_add_groups(on_device = 1) +
// dbg_agg_finalize_into_async in one crossing.  What finalize_into_async would refuse is refused
// before the reset, so a refused call leaves the handle (and a finalize in flight) as it was.
int dbg_agg_step_async(dbg_agg_handle* h, const dbg_column* group_cols, const dbg_column* arg_cols, const dbg_filter* filter,
                       uint64_t rows, dbg_out_column* out_aggs, dbg_out_column* out_keys, uint64_t max_groups,
                       const uint64_t* max_string_bytes) {
    if (!h) return fail(DBG_ERR_INVALID, "null argument");
    REFUSE_KEYLESS(h, "dbg_agg_step_async");
    if (!group_cols || !out_aggs || !out_keys) return fail(DBG_ERR_INVALID, "null argument");
    if (has_str_minmax(h->spec))
        return fail(DBG_ERR_UNSUPPORTED, std::string("dbg_agg_step_async: ") + handle_local_reason(h->spec));
    if (h->fin.active) return fail(DBG_ERR_INVALID, "a finalize is already in flight: dbg_agg_finalize_wait first");
    RETURN_IF(dbg_agg_reset(h));
    RETURN_IF(dbg_agg_add_groups(h, group_cols, arg_cols, filter, rows, 1));
    RETURN_IF(fin_setup(h, out_aggs, out_keys, max_groups, max_string_bytes));
    return fin_launch(h);
}

int dbg_agg_finalize_wait(dbg_agg_handle* h, uint64_t* n_groups, uint64_t* string_bytes) {
    if (!h || !n_groups) return fail(DBG_ERR_INVALID, "null argument");
    if (!h->fin.active) return fail(DBG_ERR_INVALID, "no finalize in flight");
    HIPCHECK(hipSetDevice(h->device));
    RETURN_IF(flush_pending(h));
    for (int round = 0; round < 3; ++round) {
        if (round) RETURN_IF(fin_launch(h));
        bool retry = false;
        int rc = fin_complete(h, &retry, n_groups, string_bytes);
        if (rc != DBG_OK || !retry) return rc;
    }
    return fail(DBG_ERR_INTERNAL, "finalize did not converge");
}
}  // extern "C"
