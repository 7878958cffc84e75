// abi_ops.hip — the entry points that take no handle: the standalone filter (dbg_filter_select),
// LIKE's host entry points (dbg_like_*), take (dbg_take_*), the legacy hash methods (dbg_legacy_*),
// sort with limit (dbg_sort_limit_*) and the workload generator (dbg_datagen).  Each works on the caller's device columns and stream and
// keeps nothing; the kernels are filter.hip, like.hip, legacy.hip, sort.hip and datagen.hip.
#include "abi_internal.hpp"

// HashMethodKind::choose_hash_method_with_types (EXP/kernels/group_by.rs:48-97)
int legacy_method(const dbg_datatype* types, int n, int* kind, uint32_t* key_bytes) {
    if (n < 1 || n > DBG_MAX_KEYS) return fail(DBG_ERR_UNSUPPORTED, "1..8 group columns");
    if (n == 1 && types[0].type == DBG_STRING && !types[0].nullable) {
        *kind = DBG_LEGACY_SINGLE_BINARY;
        *key_bytes = 0;
        return DBG_OK;
    }
    for (int j = 0; j < n; ++j) REFUSE_DECIMAL256(types[j].type, "legacy hash methods");
    u32 len = 0;
    for (int j = 0; j < n; ++j) {
        const int t = types[j].type;
        if (t == DBG_STRING || t == DBG_BOOLEAN || !valid_type(t)) {
            *kind = DBG_LEGACY_SERIALIZER;
            *key_bytes = 0;
            return DBG_OK;
        }
        len += type_width(t) + (types[j].nullable ? 1 : 0);
    }
    *key_bytes = len;
    *kind = len == 1 ? DBG_LEGACY_KEYS_U8 : len == 2 ? DBG_LEGACY_KEYS_U16 : len <= 4 ? DBG_LEGACY_KEYS_U32
          : len <= 8 ? DBG_LEGACY_KEYS_U64 : len <= 16 ? DBG_LEGACY_KEYS_U128 : len <= 32 ? DBG_LEGACY_KEYS_U256
          : DBG_LEGACY_SERIALIZER;
    return DBG_OK;
}

// build_keys_vec: stable order by value width, widest first; null bytes after all values
void legacy_fixed_order(const dbg_datatype* types, int n, int* order, u32* off, int32_t* null_off) {
    for (int j = 0; j < n; ++j) {  // insertion keeps equal widths in column order
        int k = j;
        for (; k > 0 && type_width(types[order[k - 1]].type) < type_width(types[j].type); --k) order[k] = order[k - 1];
        order[k] = j;
    }
    u32 o = 0, noff = 0;
    for (int j = 0; j < n; ++j) noff += type_width(types[j].type);
    for (int j = 0; j < n; ++j) {
        const dbg_datatype& t = types[order[j]];
        off[j] = o;
        o += type_width(t.type);
        null_off[j] = t.nullable ? (int32_t)noff++ : -1;
    }
}

extern "C" {
// ---- standalone filter ----
int dbg_filter_select(const dbg_filter* filter, uint64_t rows, uint32_t* sel_out, uint64_t* n_sel, void* stream) {
    if (!filter || !sel_out || !n_sel) return fail(DBG_ERR_INVALID, "null argument");
    if (rows >= 0xFFFFFFFFULL) return fail(DBG_ERR_UNSUPPORTED, "selection indices are u32");
    hipStream_t s = (hipStream_t)stream;
    std::vector<DevBuf> consts;  // device copies of the predicates' string constants, and the LIKE nodes' match bitmaps
    FilterDesc fd;
    memset(&fd, 0, sizeof(fd));
    fd.rows = rows;
    RETURN_IF(fill_filter({s, consts}, filter, 1, rows, fd.cols, &fd.n_cols, fd.nodes, &fd.n_nodes));
    Buf<FilterDesc> dfd;
    Buf<u64> scratch;
    u64 nb = filter_blocks(rows);
    RETURN_IF(dfd.ensure(1));
    RETURN_IF(scratch.ensure(nb + 2));
    hipMemcpyAsync(dfd, &fd, sizeof(fd), hipMemcpyHostToDevice, s);
    {
        prof::Scope ps("filter_select", s);
        launch_filter_select(s, dfd, rows, scratch, scratch + nb, sel_out);
    }
    u64 tot = 0;
    if (nb) hipMemcpyAsync(&tot, scratch + nb, 8, hipMemcpyDeviceToHost, s);
    hipError_t e = hipStreamSynchronize(s);  // the kernel has read dfd, scratch and the constants
    *n_sel = tot;
    if (e != hipSuccess) return fail(DBG_ERR_DEVICE, std::string("filter: ") + hipGetErrorString(e));
    return DBG_OK;
}

// ---- LIKE on the host: the classification and the host build of the kernels' matcher (like.hpp) ----
int dbg_like_pattern_kind(const uint8_t* pat, uint64_t len, int32_t* kind) {
    if (!kind) return fail(DBG_ERR_INVALID, "null argument");
    LikeDesc L;
    RETURN_IF(like_check(pat, len, L));
    *kind = L.kind;
    return DBG_OK;
}

int dbg_like_match_host(const uint8_t* str, uint64_t len, const uint8_t* pat, uint64_t plen, int32_t* out) {
    if (!out || (!str && len)) return fail(DBG_ERR_INVALID, "null argument");
    LikeDesc L;
    RETURN_IF(like_check(pat, plen, L));
    *out = like_match(L, str, len, pat) ? 1 : 0;
    return DBG_OK;
}

int dbg_like_kernel_counts(uint64_t* counts, int32_t n) {
    if (!counts || n < 0) return fail(DBG_ERR_INVALID, "null argument");
    u64 c[LIKE_K_N];
    like_kernel_counts(c);
    for (int32_t i = 0; i < n; ++i) counts[i] = i < LIKE_K_N ? c[i] : 0;
    return DBG_OK;
}

int dbg_like_force_kernel(int32_t kernel) {
    if (kernel != 0 && kernel != LIKE_K_ROWS && kernel != LIKE_K_SCAN) return fail(DBG_ERR_INVALID, "dbg_like_force_kernel: 0, 1 (rows) or 2 (scan)");
    like_force_kernel(kernel);
    return DBG_OK;
}

int dbg_take_fixed(const dbg_column* col, const uint32_t* sel, uint64_t n_sel, void* out_data, uint8_t* out_validity, void* stream) {
    if (!col || !sel || !out_data) return fail(DBG_ERR_INVALID, "null argument");
    if (col->dt.type == DBG_STRING) return fail(DBG_ERR_UNSUPPORTED, "dbg_take_fixed: fixed-width columns only");
    REFUSE_DECIMAL256(col->dt.type, "dbg_take_fixed");
    hipStream_t s = (hipStream_t)stream;
    Buf<u8> vbytes;
    if (out_validity && col->dt.nullable) RETURN_IF(vbytes.ensure(n_sel + 1));
    launch_take_fixed(s, dcol_view(*col), sel, n_sel, (u8*)out_data, vbytes);
    if (vbytes) launch_pack_bits(s, vbytes, n_sel, out_validity);
    HIPCHECK(hipStreamSynchronize(s));
    return DBG_OK;
}

int dbg_take_string(const dbg_column* col, const uint32_t* sel, uint64_t n_sel, uint64_t* out_offsets, void* out_data,
                    uint64_t data_cap, uint8_t* out_validity, uint64_t* total_bytes, void* stream) {
    if (!col || !out_offsets || !total_bytes || (n_sel && !sel)) return fail(DBG_ERR_INVALID, "null argument");
    if (col->dt.type != DBG_STRING || !col->offsets) return fail(DBG_ERR_INVALID, "dbg_take_string: String columns only");
    hipStream_t s = (hipStream_t)stream;
    launch_take_string_offsets(s, col->offsets, sel, n_sel, out_offsets);
    // n_sel lengths + one zero -> exclusive scan -> n_sel + 1 offsets; the total lands in a pinned word
    HIPCHECK(hipMemsetAsync(out_offsets + n_sel, 0, 8, s));
    Buf<u64> dtot;
    RETURN_IF(dtot.ensure(1));
    u64 total = 0;
    hipError_t e = hipMemsetAsync(dtot, 0, 8, s);
    if (e == hipSuccess && n_sel) launch_exclusive_scan(s, out_offsets, n_sel + 1, dtot);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, dtot, 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(DBG_ERR_DEVICE, hipGetErrorString(e));
    *total_bytes = total;
    if (total > data_cap) return fail(DBG_ERR_INVALID, "dbg_take_string: data buffer too small (*total_bytes needed)");
    if (!n_sel) return DBG_OK;
    if (!out_data) return fail(DBG_ERR_INVALID, "null argument");
    Buf<u8> vbytes;
    if (out_validity && col->dt.nullable) RETURN_IF(vbytes.ensure(n_sel + 1));
    launch_take_string_bytes(s, dcol_view(*col), sel, n_sel, out_offsets, (u8*)out_data, vbytes);
    if (vbytes) launch_pack_bits(s, vbytes, n_sel, out_validity);
    HIPCHECK(hipStreamSynchronize(s));
    return DBG_OK;
}

int dbg_legacy_hash_method(const dbg_datatype* types, int n, int* kind, uint32_t* key_bytes) {
    if (!types || !kind || !key_bytes) return fail(DBG_ERR_INVALID, "null argument");
    return legacy_method(types, n, kind, key_bytes);
}

int dbg_legacy_group_hash(const dbg_column* cols, int n, uint64_t rows, uint64_t* out_hash, uint32_t* out_bucket,
                          int bucket_bits, void* stream) {
    if (!cols || !out_hash) return fail(DBG_ERR_INVALID, "null argument");
    if (out_bucket && (bucket_bits < 1 || bucket_bits > 31)) return fail(DBG_ERR_INVALID, "bucket bits 1..31");
    std::vector<dbg_datatype> types(n > 0 ? n : 1);
    for (int j = 0; j < n; ++j) types[j] = cols[j].dt;
    int kind = 0;
    uint32_t kb = 0;
    RETURN_IF(legacy_method(types.data(), n, &kind, &kb));
    for (int j = 0; j < n; ++j)
        if (cols[j].len < rows) return fail(DBG_ERR_INVALID, "column shorter than rows");
    hipStream_t s = (hipStream_t)stream;
    if (kind == DBG_LEGACY_SINGLE_BINARY) {
        launch_legacy_binary_hash(s, dcol_view(cols[0]), rows, out_hash, out_bucket, (u32)bucket_bits);
    } else if (kind == DBG_LEGACY_SERIALIZER) {
        LegacyKeyDesc d;
        memset(&d, 0, sizeof(d));
        d.n = n;
        for (int j = 0; j < n; ++j) d.cols[j] = dcol_view(cols[j]);  // key order: the serialized row
        launch_legacy_serializer_hash(s, d, rows, out_hash, out_bucket, (u32)bucket_bits);
    } else {
        LegacyKeyDesc d;
        memset(&d, 0, sizeof(d));
        d.n = n;
        const u32 width = kind == DBG_LEGACY_KEYS_U8 ? 1 : kind == DBG_LEGACY_KEYS_U16 ? 2 : kind == DBG_LEGACY_KEYS_U32 ? 4
                        : kind == DBG_LEGACY_KEYS_U64 ? 8 : kind == DBG_LEGACY_KEYS_U128 ? 16 : 32;
        d.words = width <= 8 ? 1 : width / 8;
        int order[DBG_MAX_KEYS];
        int32_t null_off[DBG_MAX_KEYS];
        legacy_fixed_order(types.data(), n, order, d.off, null_off);
        for (int j = 0; j < n; ++j) {  // key order: the packed key's
            d.cols[j] = dcol_view(cols[order[j]]);
            if (null_off[j] >= 0) d.null_off[j] = (u32)null_off[j];
        }
        launch_legacy_fixed_hash(s, d, rows, out_hash, out_bucket, (u32)bucket_bits);
    }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    return DBG_OK;
}

int dbg_sort_limit_indices(const dbg_column* col, uint64_t rows, int asc, int nulls_first, uint64_t limit,
                           uint32_t* idx_out, uint64_t* n_out, void* stream) {
    if (!col || !n_out || (!idx_out && limit && rows)) return fail(DBG_ERR_INVALID, "null argument");
    const int t = col->dt.type;
    REFUSE_DECIMAL256(t, "dbg_sort_limit_indices");
    if (t == DBG_STRING || t == DBG_DECIMAL128 || type_width(t) == 0)
        return fail(DBG_ERR_UNSUPPORTED, "dbg_sort_limit_indices: fixed-width number columns only");
    if (col->len < rows) return fail(DBG_ERR_INVALID, "column shorter than rows");
    std::string err;
    int rc = sort_limit_run((hipStream_t)stream, dcol_view(*col), rows, asc, nulls_first, limit, idx_out, n_out, err);
    return rc == DBG_OK ? rc : fail(rc, err);
}

int dbg_sort_limit_multi(const dbg_column* cols, int n_cols, const int* asc, const int* nulls_first, uint64_t rows,
                         uint64_t limit, uint32_t* idx_out, uint64_t* n_out, void* stream) {
    if (!cols || !asc || !nulls_first || !n_out || (!idx_out && limit && rows)) return fail(DBG_ERR_INVALID, "null argument");
    if (n_cols < 1 || n_cols > SORT_MAX_COLS) return fail(DBG_ERR_UNSUPPORTED, "dbg_sort_limit_multi: 1..8 sort columns");
    MKeyDesc K;
    memset(&K, 0, sizeof(K));
    K.n = n_cols;
    for (int c = 0; c < n_cols; ++c) {
        const dbg_column& col = cols[c];
        const int t = col.dt.type;
        REFUSE_DECIMAL256(t, "dbg_sort_limit_multi");
        if (!valid_type(t) || (t != DBG_STRING && type_width(t) == 0))
            return fail(DBG_ERR_UNSUPPORTED, "dbg_sort_limit_multi: number, Decimal128 and String columns");
        if (col.len < rows) return fail(DBG_ERR_INVALID, "column shorter than rows");
        if (t == DBG_STRING && !col.offsets) return fail(DBG_ERR_INVALID, "String column without offsets");
        K.cols[c] = dcol_view(col);
        K.desc[c] = asc[c] ? 0 : 1;
        K.nulls_first[c] = nulls_first[c] ? 1 : 0;
    }
    std::string err;
    int rc = sort_multi_limit_run((hipStream_t)stream, K, rows, limit, idx_out, n_out, err);
    return rc == DBG_OK ? rc : fail(rc, err);
}

// ---- workload generator ----
int dbg_datagen(int cfg, uint64_t seed, uint64_t row_start, uint64_t rows, void** outs, int n_outs, const uint64_t* aux,
                void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (launch_datagen(s, cfg, seed, row_start, rows, outs, n_outs, aux) != 0) return fail(DBG_ERR_INVALID, "bad datagen config");
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}
}  // extern "C"
