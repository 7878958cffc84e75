// abi_spec.hip — spec construction: AggregatorParams -> slot, record and payload layouts (+ result
// types, per the factory), and the entry points that only report them (dbg_agg_result_type,
// dbg_agg_record_layout, dbg_agg_record_width).  Pure host arithmetic: no handle state, no launch.
#include "abi_internal.hpp"

static bool is_signed_i(int t) { return t == DBG_INT8 || t == DBG_INT16 || t == DBG_INT32 || t == DBG_INT64; }
static bool is_unsigned_i(int t) { return t == DBG_UINT8 || t == DBG_UINT16 || t == DBG_UINT32 || t == DBG_UINT64; }
static bool is_float(int t) { return t == DBG_FLOAT32 || t == DBG_FLOAT64; }
// Decimal256 is what DecimalDataType::from_size gives for precision 39..76 (EXP/types/decimal.rs:903-921)
static int check_decimal256(const dbg_datatype& t) {
    if (t.type != DBG_DECIMAL256) return DBG_OK;
    if (t.precision < 39 || t.precision > 76 || t.scale > t.precision)
        return fail(DBG_ERR_INVALID, "Decimal256 needs precision 39..76 and scale <= precision");
    return DBG_OK;
}

// AggregateFunction::return_type() of the factory-built function.
static int result_type_of(const dbg_agg_spec& s, dbg_datatype* out) {
    int t = s.arg.type;
    dbg_datatype r{DBG_UINT64, 0, 0, 0, 0};
    if (s.kind == DBG_AGG_COUNT) {
        RETURN_IF(check_decimal256(s.arg));  // count(x): the argument's type is still declared
        *out = r;  // AggregateCountFunction: UInt64, never nullable
        return DBG_OK;
    }
    if (t < 0 || !valid_type(t)) return fail(DBG_ERR_INVALID, "aggregate needs an argument type");
    RETURN_IF(check_decimal256(s.arg));
    switch (s.kind) {
        case DBG_AGG_SUM:  // ResultTypeOfUnary::Sum
            if (is_signed_i(t)) r.type = DBG_INT64;
            else if (is_unsigned_i(t)) r.type = DBG_UINT64;
            else if (is_float(t)) r.type = DBG_FLOAT64;
            else if (t == DBG_DECIMAL128) r = dbg_datatype{DBG_DECIMAL128, 38, s.arg.scale, 0, 0};
            else if (t == DBG_DECIMAL256) r = dbg_datatype{DBG_DECIMAL256, 76, s.arg.scale, 0, 0};  // aggregate_sum.rs:224-250
            else return fail(DBG_ERR_UNSUPPORTED, "sum: unsupported argument type");
            break;
        case DBG_AGG_AVG:
            if (is_signed_i(t) || is_unsigned_i(t) || is_float(t)) r.type = DBG_FLOAT64;
            else if (t == DBG_DECIMAL128) r = dbg_datatype{DBG_DECIMAL128, 38, (uint8_t)std::max<int>(s.arg.scale, 4), 0, 0};
            else if (t == DBG_DECIMAL256)  // aggregate_avg.rs:261-270
                r = dbg_datatype{DBG_DECIMAL256, 76, (uint8_t)std::max<int>(s.arg.scale, 4), 0, 0};
            else return fail(DBG_ERR_UNSUPPORTED, "avg: unsupported argument type");
            break;
        case DBG_AGG_AVG_SQL:  // divide's result type (EXP/types/decimal.rs:1015-1037; numbers: Float64)
            if (is_signed_i(t) || is_unsigned_i(t) || is_float(t)) r.type = DBG_FLOAT64;
            else if (t == DBG_DECIMAL128)
                r = dbg_datatype{DBG_DECIMAL128, 38, (uint8_t)std::max<int>(s.arg.scale, std::min<int>(s.arg.scale + 6, 12)), 0, 0};
            else if (t == DBG_DECIMAL256) return fail(DBG_ERR_UNSUPPORTED, "avg (SQL) over Decimal256: the 256-bit rounding divide is not built");
            else return fail(DBG_ERR_UNSUPPORTED, "avg: unsupported argument type");
            break;
        case DBG_AGG_MIN: case DBG_AGG_MAX:
            // Boolean: MinMaxAnyState<BooleanType> (false < true; the 0/1 value in an i64 state word,
            // one byte per row in results and borsh Option<bool>); String: MinMaxAnyState<StringType>,
            // a reference to the winning input row as the state (MMK_STR)
            r = dbg_datatype{t, s.arg.precision, s.arg.scale, 0, 0};
            break;
        default: return fail(DBG_ERR_INVALID, "unknown aggregate kind");
    }
    r.nullable = (s.or_null || s.arg.nullable) ? 1 : 0;
    *out = r;
    return DBG_OK;
}

int build_spec(const dbg_agg_params* p, Spec& S, std::vector<dbg_datatype>& rtypes) {
    memset(&S, 0, sizeof(S));
    S.x_pp_cap = ~0u;  // no test hook (dbg_agg_create reads them)
    if (p->n_group_cols < 0 || p->n_group_cols > DBG_MAX_KEYS) return fail(DBG_ERR_UNSUPPORTED, "0..8 group columns supported");
    if (p->n_aggs < 0 || p->n_aggs > DBG_MAX_AGGS) return fail(DBG_ERR_UNSUPPORTED, "at most 32 aggregates");
    // no group columns: one state (reduce.hpp).  The register kernel carries states of at most two
    // words and no row references, and the empty input of an unwrapped function is not defined.
    const bool keyless = p->n_group_cols == 0;
    if (keyless) {
        if (p->n_aggs == 0) return fail(DBG_ERR_UNSUPPORTED, "no group columns: at least one aggregate is needed");
        for (int a = 0; a < p->n_aggs; ++a) {
            const dbg_agg_spec& s = p->aggs[a];
            if (s.kind != DBG_AGG_COUNT && !s.or_null)
                return fail(DBG_ERR_UNSUPPORTED, "no group columns: every aggregate but COUNT needs or_null (the factory always wraps)");
            if ((s.kind == DBG_AGG_MIN || s.kind == DBG_AGG_MAX) && s.arg.type == DBG_STRING)
                return fail(DBG_ERR_UNSUPPORTED, "no group columns: MIN/MAX of a String argument is not supported");
            if (s.arg.type == DBG_DECIMAL256) return fail(DBG_ERR_UNSUPPORTED, "no group columns: Decimal256 arguments are not supported");
        }
    }
    S.n_keys = p->n_group_cols;
    S.n_aggs = p->n_aggs;
    // inline packing: row format [validity bytes][values] (EAGG/payload.rs:100-129)
    int w = 0;
    bool fixed = true;
    for (int c = 0; c < S.n_keys; ++c) {
        dbg_datatype t = p->group_types[c];
        if (!valid_type(t.type)) return fail(DBG_ERR_INVALID, "bad group type");
        RETURN_IF(check_decimal256(t));
        S.key_types[c] = t;
        if (t.type == DBG_STRING) S.has_strings = 1;
        if (t.type == DBG_STRING || t.type == DBG_DECIMAL128 || t.type == DBG_DECIMAL256) fixed = false;  // reference keys
        if (t.nullable) S.voff[c] = (uint8_t)w++;
    }
    for (int c = 0; c < S.n_keys; ++c) {
        S.koff[c] = (uint8_t)w;
        w += type_width(S.key_types[c].type);
    }
    S.inline_keys = fixed && w <= 8;
    S.inline_width = w;
    // record layout: [hash][validity bytes][values, 8-aligned][state words]
    u32 off = 8;
    for (int c = 0; c < S.n_keys; ++c)
        if (S.key_types[c].nullable) S.rec_val_off[c] = off++;
    off = (off + 7) & ~7u;
    for (int c = 0; c < S.n_keys; ++c) {
        S.rec_key_off[c] = off;
        int t = S.key_types[c].type;
        off += (t == DBG_STRING || t == DBG_DECIMAL128) ? 16 : 8;  // Decimal256: no record format (handle-local spec)
    }
    // state words
    int word = 1, flag_bits = 0;
    rtypes.clear();
    for (int a = 0; a < S.n_aggs; ++a) {
        const dbg_agg_spec& s = p->aggs[a];
        DAgg& A = S.aggs[a];
        dbg_datatype rt;
        RETURN_IF(result_type_of(s, &rt));
        rtypes.push_back(rt);
        const bool sql_avg = s.kind == DBG_AGG_AVG_SQL;
        A.kind = sql_avg ? DBG_AGG_AVG : s.kind;  // same state; only the result differs
        A.arg_type = s.kind == DBG_AGG_COUNT && s.arg.type < 0 ? -1 : s.arg.type;
        A.arg_nullable = A.arg_type >= 0 ? s.arg.nullable : 0;
        int t = A.arg_type;
        A.sumk = t == DBG_DECIMAL256 ? SUMK_I256 : (t == DBG_DECIMAL128 ? SUMK_I128 : (is_float(t) ? SUMK_F64 : SUMK_I64));
        A.mmk = is_unsigned_i(t) ? MMK_U64 : (is_float(t) ? MMK_F64 : MMK_I64);
        if (t == DBG_DECIMAL128 && s.arg.precision > 18) A.mmk = MMK_I128;
        if (t == DBG_DECIMAL256) A.mmk = MMK_I256;
        if (t == DBG_STRING && (s.kind == DBG_AGG_MIN || s.kind == DBG_AGG_MAX)) A.mmk = MMK_STR;
        A.w0 = word;
        switch (A.kind) {
            case DBG_AGG_COUNT: A.nwords = 1; break;
            case DBG_AGG_SUM: A.nwords = sum_words(A.sumk); break;
            case DBG_AGG_AVG: A.nwords = sum_words(A.sumk) + 1; break;
            default: A.nwords = A.mmk == MMK_I256 ? 5 : (A.mmk == MMK_I128 ? 3 : 1);
        }
        word += A.nwords;
        A.flag_bit = -1;
        // (keyless: every one of them, since the empty input is NULL whatever the argument)
        if ((s.kind == DBG_AGG_SUM || s.kind == DBG_AGG_MIN || s.kind == DBG_AGG_MAX) && (A.arg_nullable || keyless)) A.flag_bit = flag_bits++;
        A.res_type = rt.type;
        A.res_precision = rt.precision;
        A.res_scale = rt.scale;
        A.res_nullable = rt.nullable;
        // SUM's range check (DecimalSumState<OVERFLOW>, p <= 18) also guards AVG_SQL's sum
        A.dec_check = ((s.kind == DBG_AGG_SUM || sql_avg) && t == DBG_DECIMAL128 && s.arg.precision <= 18) ? 1 : 0;
        // keyless: AVG's own range check at precision > 18 (DecimalAvgState<OVERFLOW = true>,
        // aggregate_avg.rs:141-153), made by keyless_write_kernel on the final sum; the grouped
        // writers read dec_check for SUM and AVG_SQL only
        if (keyless && s.kind == DBG_AGG_AVG && t == DBG_DECIMAL128 && s.arg.precision > 18) A.dec_check = 1;
        A.scale_add = (A.kind == DBG_AGG_AVG && (t == DBG_DECIMAL128 || t == DBG_DECIMAL256)) ? (int)rt.scale - (int)s.arg.scale : 0;
        A.avg_round = sql_avg && t == DBG_DECIMAL128;
        A.res_width = (int)type_width(rt.type);
        if (is_str_minmax(A)) A.res_width = 8;  // the result writers emit the row reference; dbg_agg_result gathers the bytes
        A.ser_flags = 0;
        if (s.kind != DBG_AGG_COUNT) {
            if (s.or_null) A.ser_flags |= SER_OR_NULL;
            if (A.arg_nullable) A.ser_flags |= SER_NULL_ADPT;
        }
    }
    if (flag_bits > 64) return fail(DBG_ERR_UNSUPPORTED, "too many nullable aggregates");
    S.flags_word = (flag_bits || keyless) ? word++ : -1;  // keyless: always, for KEYLESS_SEEN_BIT
    S.n_words = word - 1;
    if (word > DBG_MAX_WORDS) return fail(DBG_ERR_UNSUPPORTED, "aggregate states too wide");
    int sw = 1;
    while (sw < word && sw < 8) sw <<= 1;
    if (word > 8) sw = (word + 7) & ~7;
    S.stride_words = sw;
    // one non-null String key: the HBM slot also caches the key (agg_insert_str1_kernel), so a
    // probe compares in the slot's own line instead of reading the representative row
    S.tstride = sw;
    S.kc_word = 0;
    if (S.n_keys == 1 && S.key_types[0].type == DBG_STRING && !S.key_types[0].nullable) {
        const int need = word + 1 + KC_KEY_WORDS;  // entry + states (+ flags) + hdr + key words
        int ts = 1;
        while (ts < need && ts < 8) ts <<= 1;
        if (need > 8) ts = (need + 7) & ~7;
        if (ts <= DBG_MAX_WORDS) {
            S.tstride = ts;
            S.kc_word = word;
        }
    }
    for (int w = 0; w < DBG_MAX_WORDS; ++w) S.slot_init[w] = w == 0 ? SLOT_EMPTY : 0;
    for (int a = 0; a < S.n_aggs; ++a)
        if (S.aggs[a].kind == DBG_AGG_MIN || S.aggs[a].kind == DBG_AGG_MAX)
            for (int k = 0; k < S.aggs[a].nwords; ++k) S.slot_init[S.aggs[a].w0 + k] = state_init_word(S.aggs[a], k);
    S.rec_state_off = off;
    S.rec_width = off + 8 * (u32)S.n_words;
    // partitioned payload record formats (pp.hip): key part, then each argument value aligned to
    // its width, then one validity bit per nullable argument
    S.pp_str = S.has_strings;
    S.pp_kw = S.has_strings ? 48 : (u32)((S.inline_width + 7) & ~7);
    // raw records pack the arguments right after the key bytes (a 12-byte key + two Int16 = 16 B);
    // key words are compared / copied with the last one masked to the key bytes
    S.pp_klast_mask = (S.has_strings || (S.inline_width & 7) == 0) ? ~0ULL : ((1ULL << (8 * (S.inline_width & 7))) - 1);
    u32 po = S.has_strings ? S.pp_kw : (u32)S.inline_width;
    int vbits = 0;
    for (int a = 0; a < S.n_aggs; ++a) {
        const DAgg& A = S.aggs[a];
        S.pp_avbit[a] = -1;
        S.pp_aoff[a] = 0;
        if (A.arg_type < 0) continue;
        const u32 aw = A.arg_type == DBG_BOOLEAN ? 1 : type_width(A.arg_type);
        const u32 al = aw >= 8 ? 8 : aw;
        po = (po + al - 1) & ~(al - 1);
        S.pp_aoff[a] = (uint16_t)po;
        po += aw;
        if (A.arg_nullable) S.pp_avbit[a] = (int16_t)vbits++;
    }
    S.pp_avoff = po;
    po += (u32)(vbits + 7) / 8;
    S.pp_rw_raw = (po + 7) & ~7u;
    if (!vbits) S.pp_avoff = S.pp_rw_raw;
    S.pp_rw_state = S.pp_kw + 8 * (u32)S.n_words;
    S.pp_sw = 1 + S.pp_kw / 8 + (u32)S.n_words;
    // a handle-local spec (String MIN/MAX row references, Decimal256 keys or arguments) is never partitioned
    S.pp_ok = S.pp_rw_raw <= 256 && S.pp_rw_state <= 256 && vbits <= 64 && S.pp_sw <= 64 && !handle_local_reason(S);
    return DBG_OK;
}

// Upper bound of one group's serialized state of aggregate a (agg_serialize).
u32 ser_stride_of(const DAgg& A) {
    u32 n;
    switch (A.kind) {
        case DBG_AGG_COUNT: return 8;
        case DBG_AGG_SUM: n = A.sumk == SUMK_I128 ? 16 : 8; break;
        case DBG_AGG_AVG: n = A.sumk == SUMK_I128 ? 24 : 16; break;
        default: n = 1 + type_width(A.arg_type);
    }
    if (A.ser_flags & SER_NULL_ADPT) n++;
    if (A.ser_flags & SER_OR_NULL) n++;
    return n;
}

extern "C" {
int dbg_agg_result_type(const dbg_agg_spec* spec, dbg_datatype* out) {
    if (!spec || !out) return fail(DBG_ERR_INVALID, "null argument");
    return result_type_of(*spec, out);
}

int dbg_agg_record_width(dbg_agg_handle* h, uint32_t* width) {
    if (!h || !width) return fail(DBG_ERR_INVALID, "null argument");
    REFUSE_KEYLESS(h, "dbg_agg_record_width");
    *width = h->spec.rec_width;
    return DBG_OK;
}

int dbg_agg_record_layout(const dbg_agg_params* params, dbg_record_layout* out) {
    if (!params || !out) return fail(DBG_ERR_INVALID, "null argument");
    Spec S;
    std::vector<dbg_datatype> rt;
    RETURN_IF(build_spec(params, S, rt));
    if (is_keyless(S)) return fail(DBG_ERR_UNSUPPORTED, std::string("dbg_agg_record_layout: ") + keyless_reason());
    if (const char* why = handle_local_reason(S)) return fail(DBG_ERR_UNSUPPORTED, std::string("dbg_agg_record_layout: ") + why);
    memset(out, 0, sizeof(*out));
    out->width = S.rec_width;
    out->state_off = S.rec_state_off;
    for (int c = 0; c < S.n_keys; ++c) {
        out->key_off[c] = S.rec_key_off[c];
        out->validity_off[c] = S.key_types[c].nullable ? S.rec_val_off[c] : 0;
    }
    for (int a = 0; a < S.n_aggs; ++a) {
        out->agg_w0[a] = S.aggs[a].w0;
        out->agg_words[a] = S.aggs[a].nwords;
    }
    out->flags_word = S.flags_word;
    out->n_words = S.n_words;
    return DBG_OK;
}
}  // extern "C"
