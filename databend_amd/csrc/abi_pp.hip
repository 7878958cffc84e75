// abi_pp.hip — the host side of the partitioned payload (kernels: pp.hip), the handle's
// high-cardinality mode: the cardinality probe and the switch, level 1 on every batch
// (pp_add_batch), levels 2 / 3 and the LDS aggregation at finalize (pp_prepare, pp_agg), group
// records, and the payload's ends of both finalize families (pp_finalize; pp_fin_launch /
// pp_fin_complete).  Who calls them — inserts, finalize, partition — is in the other units.
#include "abi_exp.hpp"

#define PP_MIN_ROWS (1ULL << 22)
#define PP_MIN_GROUPS (1ULL << 20)
#define PP_SET_CAP (1ULL << 19)  // 2^18 samples at most: <= 50 % load

// Cardinality probe of the first batch into an empty handle (AggregateHashTable decides its
// partial strategy by observed cardinality too: clear_ht / maybe_repartition,
// EAGG/aggregate_hashtable.rs:225-239, 453-503).  Distinct group hashes among 2^20 evenly spaced
// selected rows give the estimate: the larger of twice the uniform-frequency solution of
// D = G (1 - exp(-s / G)) and Haas's GEE sqrt(N / s) f1 + (D - f1), capped at the selected rows.
int pp_maybe_switch(dbg_agg_handle* h, u32 bid, u64 rows) {
    const Spec& S = h->spec;
    h->est_groups = 0;  // set below only from this batch's probe or observation
    const int mode = h->strategy == DBG_STRATEGY_TABLE ? 0 : (h->strategy == DBG_STRATEGY_PARTITIONED ? 2 : 1);
    if (h->pp || !mode || !S.pp_ok || h->table_rows) return DBG_OK;
    if (mode == 1 && (rows < PP_MIN_ROWS || (!S.has_strings && S.inline_width <= 2))) return DBG_OK;
    if (mode == 1 && h->obs_rows >= PP_MIN_ROWS) {
        // the handle's last finalize saw this query's cardinality (groups per inserted row)
        const double ratio = std::min(1.0, (double)h->obs_groups / (double)h->obs_rows);
        h->pp_ratio = std::max(ratio, 1e-9);
        h->pp_probed = true;
        h->est_groups = ratio * (double)rows;
        if (ratio * (double)rows > (double)PP_MIN_GROUPS && ratio > 0.5) h->pp = true;
        return DBG_OK;
    }
    if (!h->pp_set) RETURN_IF(h->pp_set.ensure(PP_SET_CAP * 2 + 8));
    u64* out = h->pp_set + 2 * PP_SET_CAP;
    // 1/64 of the rows, between 2^16 and 2^18 samples; the set sized for them (<= 50 % load)
    const u64 ns = std::min<u64>(rows, std::max<u64>(1ULL << 16, std::min<u64>(rows / 64, 1ULL << 18)));
    const u64 set_cap = std::min<u64>(PP_SET_CAP, pow2_at_least(2 * ns));
    {
        prof::Scope ps("pp_probe", h->stream);
        launch_pp_sample(h->stream, h->dspec, h->dbatches, bid, rows, ns, h->pp_set, set_cap, out);
    }
    HIPCHECK(hipGetLastError());
    RETURN_IF(h->pp_hpart.ensure_after(h->stream, 1024, 1024));
    HIPCHECK(hipMemcpyAsync(h->pp_hpart, out, 32, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    const double sel = (double)h->pp_hpart[0], D = (double)h->pp_hpart[1], f1 = (double)h->pp_hpart[2];
    if (sel <= 0) return DBG_OK;
    const double nsel = (double)rows * sel / (double)ns;
    double gu = nsel;
    if (D < sel - 0.5) {  // bisection on G >= D of G (1 - exp(-sel / G)) = D (increasing in G)
        double lo = D, hi = 1e15;
        for (int it = 0; it < 200; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (mid * -std::expm1(-sel / mid) < D) lo = mid;
            else hi = mid;
        }
        gu = lo;
    }
    const double gee = std::sqrt(nsel / sel) * f1 + (D - f1);
    const double g = std::min(nsel, std::max(1.25 * gu, gee));
    h->pp_ratio = std::min(1.0, std::max(g / nsel, 1e-9));
    h->pp_probed = true;
    h->est_groups = g;
    // the partitioned payload beats the HBM table when keys are mostly unique (ClickBench Q33:
    // 1e9 groups in 1e9 rows); moderate cardinality stays on the table
    if (mode == 2 || (g > (double)PP_MIN_GROUPS && h->pp_ratio > 0.5)) h->pp = true;
    return DBG_OK;
}

// The pinned chunk staging is rewritten only after the stream has drained its last upload.
static int pp_upload_chunks(dbg_agg_handle* h, const std::vector<PPChunk>& ch, const std::vector<u32>& c0) {
    HIPCHECK(hipStreamSynchronize(h->stream));
    RETURN_IF(h->pp_hchunks.ensure_after(h->stream, ch.size(), 1024));
    RETURN_IF(h->pp_hc0.ensure_after(h->stream, c0.size(), 1024));
    RETURN_IF(h->pp_dchunks.ensure(ch.size(), 64));
    RETURN_IF(h->pp_dc0.ensure(c0.size(), 64));
    memcpy(h->pp_hchunks, ch.data(), ch.size() * sizeof(PPChunk));
    memcpy(h->pp_hc0, c0.data(), c0.size() * sizeof(u32));
    HIPCHECK(hipMemcpyAsync(h->pp_dchunks, h->pp_hchunks, ch.size() * sizeof(PPChunk), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->pp_dc0, h->pp_hc0, c0.size() * sizeof(u32), hipMemcpyHostToDevice, h->stream));
    return DBG_OK;
}

// count + scan of one level: part_out receives G * K + 1 partition offsets
static const char* const PP_COUNT_NAME[4] = {"", "pp_count_l1", "pp_count_l2", "pp_count_l3"};
static const char* const PP_SCAN_NAME[4] = {"", "pp_scan_l1", "pp_scan_l2", "pp_scan_l3"};
static const char* const PP_SCATTER_NAME[4] = {"", "pp_scatter_l1", "pp_scatter_l2", "pp_scatter_l3"};

// The specialised level-1 form of a raw batch (pp.hip pp_l1_*), or kind 0 for the generic kernels.
static PPFast pp_fast_desc(const Spec& S, const BatchDesc& B, u32 bid, int kind) {
    PPFast F;
    memset(&F, 0, sizeof(F));
    if (kind != 0 || B.is_records || B.n_nodes > 1) return F;
    const DNode* nd = B.n_nodes ? &B.nodes[0] : nullptr;
    if (nd && nd->op != DBG_PRED_CMP_CONST) return F;
    const DCol* pc = nd ? &B.fcols[nd->col] : nullptr;
    if (pc && (pc->nullable || pc->layout != LAYOUT_ARROW)) return F;
    auto fixed_ok = [](int t) { return t != DBG_STRING && t != DBG_DECIMAL128 && t != DBG_BOOLEAN && type_width(t) > 0; };
    if (!S.has_strings) {
        if (S.pp_rw_raw > 64) return F;
        u32 n = 0;
        for (int c = 0; c < S.n_keys; ++c) {
            const dbg_datatype& t = S.key_types[c];
            const DCol& d = B.keys[c];
            if (t.nullable || !fixed_ok(t.type) || d.layout != LAYOUT_ARROW) return F;
            F.ptr[n] = d.data;
            F.width[n] = (u8)type_width(t.type);
            F.type[n] = (u8)t.type;
            F.off[n] = S.koff[c];
            ++n;
        }
        F.nk = n;
        for (int a = 0; a < S.n_aggs; ++a) {
            const DAgg& A = S.aggs[a];
            if (A.arg_type < 0) continue;
            const DCol& d = B.args[a];
            if (A.arg_nullable || !fixed_ok(A.arg_type) || d.layout != LAYOUT_ARROW || n >= 8) return F;
            F.ptr[n] = d.data;
            F.width[n] = (u8)type_width(A.arg_type);
            F.type[n] = (u8)A.arg_type;
            F.off[n] = S.pp_aoff[a];
            ++n;
        }
        F.ncol = n;
        if (pc) {
            const int t = pc->type;
            if (!fixed_ok(t) || t == DBG_FLOAT32 || t == DBG_FLOAT64) return F;
            F.has_pred = 1;
            F.pcmp = nd->cmp;
            F.ptype = t;
            F.pwidth = type_width(t);
            F.pptr = pc->data;
            F.pconst = nd->i64v;
        }
        F.wpr = S.pp_rw_raw / 8;
        F.kind = 1;
        return F;
    }
    if (S.n_keys != 1 || S.key_types[0].type != DBG_STRING || S.key_types[0].nullable || S.pp_rw_raw != 48) return F;
    for (int a = 0; a < S.n_aggs; ++a)
        if (S.aggs[a].arg_type >= 0) return F;
    const DCol& k = B.keys[0];
    if (k.layout != LAYOUT_ARROW) return F;
    if (pc) {
        if (pc->type != DBG_STRING || pc->data != k.data || pc->offsets != k.offsets) return F;
        F.has_pred = 1;
        F.pcmp = nd->cmp;
        F.pstr = nd->str;
        F.pstr_len = nd->str_len;
    }
    F.soffs = k.offsets;
    F.sdata = k.data;
    F.bid = bid;
    F.wpr = 6;
    F.kind = 2;
    return F;
}


static int pp_count_scan(dbg_agg_handle* h, int level, int src, int kind, const u8* recs, const std::vector<PPChunk>& ch,
                         const std::vector<u32>& c0, u32 shift, u32 kbits, u64* part_out, const PPFast* F = nullptr,
                         bool counted = false, const u16* dig = nullptr) {
    const u64 K = 1ULL << kbits;
    RETURN_IF(pp_upload_chunks(h, ch, c0));
    if (counted && h->pp_cnt.cap() < ch.size() * K) return fail(DBG_ERR_INTERNAL, "fused counts: buffer too small");
    RETURN_IF(h->pp_cnt.ensure(ch.size() * K, 64));
    RETURN_IF(h->pp_off.ensure(ch.size() * K, 64));
    if (!counted) {
        prof::Scope ps(PP_COUNT_NAME[level], h->stream);
        if (F && F->kind)
            launch_pp_l1_fast(h->stream, *F, 1, h->pp_dchunks, (u32)ch.size(), h->pp_cnt, nullptr, nullptr, nullptr);
        else if (dig)
            launch_pp_count_dig(h->stream, h->pp_dchunks, (u32)ch.size(), dig, kbits, h->pp_cnt);
        else
            launch_pp_count(h->stream, h->dspec, h->dbatches, src, kind, recs, h->pp_dchunks, (u32)ch.size(), shift, kbits, h->pp_cnt,
                            (kind ? h->spec.pp_rw_state : h->spec.pp_rw_raw) / 8);
    }
    RETURN_IF(h->pp_scan_tmp.ensure(pp_scan_scratch_words((u32)(c0.size() - 1), kbits), 64));
    {
        prof::Scope ps(PP_SCAN_NAME[level], h->stream);
        launch_pp_scan(h->stream, h->pp_cnt, (u32)ch.size(), kbits, h->pp_dc0, (u32)(c0.size() - 1), h->pp_off, part_out,
                       h->pp_scan_tmp);
    }
    h->pp_last_part = part_out;
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

static int pp_scatter(dbg_agg_handle* h, int level, int src, int kind, const u8* recs, u32 n_chunks, u32 shift, u32 kbits,
                      u8* dst, const PPFast* F = nullptr, u32* cnt_next = nullptr, u32 sh_next = 0, u32 kb_next = 0) {
    prof::Scope ps(PP_SCATTER_NAME[level], h->stream);
    if (F && F->kind) {
        launch_pp_l1_fast(h->stream, *F, 0, h->pp_dchunks, n_chunks, nullptr, h->pp_off, h->pp_last_part, dst);
        HIPCHECK(hipGetLastError());
        return DBG_OK;
    }
    launch_pp_scatter(h->stream, h->dspec, h->spec, h->dbatches, src, kind, recs, h->pp_dchunks, n_chunks, shift, kbits, h->pp_off,
                      h->pp_last_part, dst, cnt_next, sh_next, kb_next);
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

// Level 1 (TransformPartialAggregate::transform in partitioned mode): the batch's selected rows
// become records appended to the payload, grouped into 256 partitions (PartitionedPayload::
// append_rows, EAGG/partitioned_payload.rs:100-143).
// EXPERIMENT (DBG_X_PPDIG=0): level 2 counts from the records instead of the digit array
static bool kX_no_dig() {
    static const bool off = X_ENV("DBG_X_PPDIG") && X_ENV("DBG_X_PPDIG")[0] == '0';
    return off;
}

int pp_add_batch(dbg_agg_handle* h, const BatchDesc* st, u32 bid, u64 rows, int kind) {
    const Spec& S = h->spec;
    auto& K = h->ppk[kind];
    PPFast F = pp_fast_desc(S, *st, bid, kind);
    F.dig = nullptr;
    if (kind == 0) note_insert(h, F.kind == 2 ? INS_PP_STR : (F.kind == 1 ? INS_PP_FIXED : INS_PP_GENERIC));
    const u32 rw = kind ? S.pp_rw_state : S.pp_rw_raw;
    std::vector<PPChunk> ch;
    for (u64 s = 0; s < rows; s += PP_CHUNK) ch.push_back(PPChunk{s, std::min<u64>(PP_CHUNK, rows - s), bid, 0});
    std::vector<u32> c0{0, (u32)ch.size()};
    RETURN_IF(h->pp_mid.ensure(257, 64));
    RETURN_IF(pp_count_scan(h, 1, 0, kind, nullptr, ch, c0, 64 - PP_L1_BITS, PP_L1_BITS, h->pp_mid, &F));
    RETURN_IF(h->pp_hpart.ensure_after(h->stream, 1024, 1024));
    HIPCHECK(hipMemcpyAsync(h->pp_hpart, h->pp_mid, 257 * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    const u64 total = h->pp_hpart[256];
    if (!total) return DBG_OK;
    const u64 l1_cap = pp_rec_cap(K.l1.cap(), rw);
    if (K.l1_n + total > l1_cap) {  // grow (x2), keeping the records already appended
        const u64 ncap = std::max<u64>(K.l1_n + total, K.l1_n ? 2 * l1_cap : 0);
        RETURN_IF(K.l1.grow_keep(ncap * rw + PP_SLACK, K.l1_n * rw, h->stream));
    }
    // the level-2 digits ride along while every record so far has them (fixed-shape raw batches)
    // (EXPERIMENT, DBG_X_PPDIG=0: no digits at all)
    const bool with_dig = F.kind == 1 && kind == 0 && K.dig_n == K.l1_n && !kX_no_dig();
    const u64 dig_cap = pp_rec_cap(K.dig.cap() * 2, 2);
    if (with_dig && K.l1_n + total > dig_cap) {
        const u64 ncap = std::max<u64>(K.l1_n + total, K.dig_n ? 2 * dig_cap : 0);
        RETURN_IF(K.dig.grow_keep(ncap + PP_SLACK / 2, K.dig_n, h->stream));
    }
    if (with_dig) F.dig = K.dig + K.l1_n;
    RETURN_IF(pp_scatter(h, 1, 0, kind, nullptr, (u32)ch.size(), 64 - PP_L1_BITS, PP_L1_BITS, K.l1 + K.l1_n * rw, &F));
    if (with_dig) K.dig_n = K.l1_n + total;
    K.segs.push_back(dbg_agg_handle::Seg{K.l1_n, total, std::vector<u64>(h->pp_hpart.get(), h->pp_hpart + 257)});
    K.l1_n += total;
    h->pp_grec_ready = false;
    return DBG_OK;
}

// the specialised aggregation's table load per LDS round (linear probing in a 96-slot window;
// records whose window is full wait for a further mini-round).  0.7 halves C4's rounds (4 -> 2)
// but the longer probes cost more: pp_agg 32 -> 45 ms
#ifndef PS_LOAD
#define PS_LOAD 0.45
#endif


// Levels 2 and 3 (NewTransformPartitionBucket + the final bucket split): every level-1 partition
// of both record kinds is re-scattered by the next hash bits until the estimated groups of a
// final partition fit half a workgroup's LDS table.
static int pp_prepare(dbg_agg_handle* h, bool spec_ok) {
    const Spec& S = h->spec;
    const u64 nr = h->ppk[0].l1_n, nsr = h->ppk[1].l1_n;
    // estimated groups: the probe's, raised to the capacity hint (a hint below what the probe saw
    // would leave too few partition bits: many LDS overflow rounds); without a probe the hint, else
    // every record its own group
    const double probed = h->pp_ratio * (double)nr + (double)nsr;
    const double est = h->pp_probed ? std::max((double)h->hint_groups, probed)
                                    : (h->hint_groups ? (double)h->hint_groups : probed);
    const double g = std::min((double)(nr + nsr), est);
    // 45 % load: a wave's probe runs as long as its longest lane's (64 lanes in lockstep)
    const double target = std::max(64.0, 0.45 * (double)pp_agg_slots(S));
    const double need = std::max(1.0, std::ceil(g / target));
    u32 B = PP_L1_BITS + 1;
    while ((double)(1ULL << B) < need && B < PP_L1_BITS + 16) ++B;
    // level 2 takes up to 10 bits (one pass instead of a 1-2 bit third level), level 3 the rest
    u32 k2 = std::min<u32>(B - PP_L1_BITS <= 10 ? 10 : 8, B - PP_L1_BITS), k3 = B - PP_L1_BITS - k2;
    // Compile-time specialised aggregation (result columns, raw records of a supported shape): a
    // partition is loaded once and aggregated in 2^sub LDS rounds, so partitions hold up to the
    // kernel's register budget of records and level 2 alone (<= 10 bits) sizes them — no level 3.
    h->pp_spec = -1;
    static const bool spec_on = !(X_ENV("DBG_X_PPSPEC") && X_ENV("DBG_X_PPSPEC")[0] == '0');
    u32 scap = 0, smax = 0;
    const int shape = (spec_on && spec_ok && nsr == 0 && nr > 0) ? pp_spec_shape(S, &scap, &smax) : -1;
    if (shape >= 0) {
        const double fill = 0.75 * (double)smax;  // average records per partition (the max stays below smax)
        u32 b2 = PP_L1_BITS + 1;
        while ((double)nr / (double)(1ULL << b2) > fill && b2 < PP_L1_BITS + 10) ++b2;
        const double gp = g / (double)(1ULL << b2);
        u32 sub = 0;
        while (gp / (double)(1u << sub) > PS_LOAD * (double)scap && sub < 5) ++sub;
        if ((double)nr / (double)(1ULL << b2) <= fill && gp / (double)(1u << sub) <= PS_LOAD * (double)scap && B >= b2) {
            B = b2;
            k2 = B - PP_L1_BITS;
            k3 = 0;
            h->pp_spec = shape;
            h->pp_spec_sub = sub;
        }
    }
    h->pp_bits = B;
    for (int kind = 0; kind < 2; ++kind) {
        auto& K = h->ppk[kind];
        if (!K.l1_n) continue;
        const u32 rw = kind ? S.pp_rw_state : S.pp_rw_raw;
        RETURN_IF(K.a.ensure(K.l1_n * rw + PP_SLACK));
        RETURN_IF(K.b.ensure(K.l1_n * rw + PP_SLACK));
        RETURN_IF(K.part.ensure((1ULL << B) + 1, 64));
        // level 2: units never straddle a level-1 partition (group = partition index)
        std::vector<PPChunk> ch;
        std::vector<u32> c0;
        for (u32 g1 = 0; g1 < (1u << PP_L1_BITS); ++g1) {
            c0.push_back((u32)ch.size());
            for (const auto& sg : K.segs) {
                const u64 lo = sg.base + sg.off[g1], hi = sg.base + sg.off[g1 + 1];
                for (u64 x = lo; x < hi; x += PP_CHUNK) ch.push_back(PPChunk{x, std::min<u64>(PP_CHUNK, hi - x), 0, g1});
            }
            if (c0.back() == ch.size()) ch.push_back(PPChunk{0, 0, 0, g1});
        }
        c0.push_back((u32)ch.size());
        const u32 sh2 = 64 - PP_L1_BITS - k2;
        u64* p2 = k3 ? nullptr : K.part;
        if (k3) {
            RETURN_IF(h->pp_mid.ensure((256ULL << k2) + 1, 64));
            p2 = h->pp_mid;
        }
        // the level-2 count reads the digit array (2 bytes per record) when level 1 wrote one
        const bool use_dig = K.dig && K.dig_n == K.l1_n && k2 <= 16 && !kX_no_dig();
        RETURN_IF(pp_count_scan(h, 2, 1, kind, K.l1, ch, c0, sh2, k2, p2, nullptr, false, use_dig ? K.dig : nullptr));
        const u64 G2 = 256ULL << k2;
        const u32 sh3 = sh2 - k3;
        // Level 3's counts ride on the level-2 scatter when every level-2 partition is one level-3
        // unit (<= PP_CHUNK records): one fewer pass over the records.
        bool fused3 = false;
        if (k3) {
            RETURN_IF(h->pp_hpart.ensure_after(h->stream, G2 + 1, 1024));
            HIPCHECK(hipMemcpyAsync(h->pp_hpart, p2, (G2 + 1) * 8, hipMemcpyDeviceToHost, h->stream));
            HIPCHECK(hipStreamSynchronize(h->stream));
            u64 mx = 0;
            for (u64 g2 = 0; g2 < G2; ++g2) mx = std::max<u64>(mx, h->pp_hpart[g2 + 1] - h->pp_hpart[g2]);
            fused3 = mx <= PP_CHUNK && ((1u << k2) << k3) <= PP_NEXT_HIST_MAX;
            if (fused3) {
                RETURN_IF(h->pp_cnt.ensure(G2 << k3, 64));
                HIPCHECK(hipMemsetAsync(h->pp_cnt, 0, (G2 << k3) * 4, h->stream));
            }
        }
        RETURN_IF(pp_scatter(h, 2, 1, kind, K.l1, (u32)ch.size(), sh2, k2, K.a, nullptr, fused3 ? h->pp_cnt : nullptr, sh3, k3));
        K.fin = K.a;
        K.alt = K.b;
        if (!k3) continue;
        // level 3: units inside level-2 partitions
        ch.clear();
        c0.clear();
        for (u64 g2 = 0; g2 < G2; ++g2) {
            c0.push_back((u32)ch.size());
            const u64 lo = h->pp_hpart[g2], hi = h->pp_hpart[g2 + 1];
            for (u64 x = lo; x < hi; x += PP_CHUNK) ch.push_back(PPChunk{x, std::min<u64>(PP_CHUNK, hi - x), 0, (u32)g2});
            if (c0.back() == ch.size()) ch.push_back(PPChunk{0, 0, 0, (u32)g2});
        }
        c0.push_back((u32)ch.size());
        if (fused3 && ch.size() != G2) return fail(DBG_ERR_INTERNAL, "fused level-3 counts: unit layout");
        RETURN_IF(pp_count_scan(h, 3, 1, kind, K.a, ch, c0, sh3, k3, K.part, nullptr, fused3));
        RETURN_IF(pp_scatter(h, 3, 1, kind, K.a, (u32)ch.size(), sh3, k3, K.b));
        K.fin = K.b;
        K.alt = K.a;
    }
    return DBG_OK;
}

static u64 pp_records(const dbg_agg_handle* h) { return h->ppk[0].l1_n + h->ppk[1].l1_n; }

// The LDS aggregation of every final partition: mode 0 writes the result columns of `od` (fixed-width
// keys), mode 1 the group records (state record format) into pp_grec.  Totals land in pp_tot.
static int pp_agg(dbg_agg_handle* h, int mode, const OutDesc* od) {
    const Spec& S = h->spec;
    if (!h->pp_tot) RETURN_IF(h->pp_tot.ensure(PPT_WORDS));
    HIPCHECK(hipMemsetAsync(h->pp_tot, 0, PPT_WORDS * 8, h->stream));
    const u64 N = pp_records(h);
    if (!N) return DBG_OK;
    RETURN_IF(pp_prepare(h, mode == 1 || (od && !od->ser)));
    PPAggOut o;
    memset(&o, 0, sizeof(o));
    o.tot = h->pp_tot;
    RETURN_IF(exp_pp_trace(h, o));
    if (mode == 0) {
        o.cols = *od;
    } else {
        RETURN_IF(h->pp_grec.ensure(N * S.pp_rw_state, 64));
        o.grec = h->pp_grec;
        o.grec_cap = N;
    }
    auto& R = h->ppk[0];
    auto& T = h->ppk[1];
    // every final partition may spill (skewed keys): room for all their ids (<= 1 MB)
    const u32 SPILL_CAP = 1u << h->pp_bits;
    if (h->pp_spec >= 0) {
        RETURN_IF(h->pp_spill.ensure(1 + (u64)SPILL_CAP));
        HIPCHECK(hipMemsetAsync(h->pp_spill, 0, 4, h->stream));
        prof::Scope ps("pp_agg", h->stream);
        launch_pp_agg_spec(h->stream, S, h->pp_spec, mode, 1u << h->pp_bits, R.part, R.fin, h->pp_spec_sub, o, h->pp_spill, SPILL_CAP);
        // partitions larger than its register budget (skewed keys): the generic kernel, spilled ids only
        launch_pp_agg(h->stream, h->dspec, S, h->dbatches, mode, 1u << h->pp_bits, R.part, nullptr, R.fin, R.alt, nullptr, nullptr,
                      o, h->pp_spill, SPILL_CAP);
    } else {
        prof::Scope ps("pp_agg", h->stream);
        launch_pp_agg(h->stream, h->dspec, S, h->dbatches, mode, 1u << h->pp_bits, R.l1_n ? R.part.get() : nullptr,
                      T.l1_n ? T.part.get() : nullptr, R.fin, R.alt, T.fin, T.alt, o);
    }
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

// Group records + per-block string lengths (scanned; totals in pp_tot[PPT_STR + c]).  Async.
static int pp_grec_build(dbg_agg_handle* h) {
    const Spec& S = h->spec;
    RETURN_IF(pp_agg(h, 1, nullptr));
    const u64 N = std::max<u64>(pp_records(h), 1);
    h->pp_nb = pp_grec_blocks(N);
    RETURN_IF(h->pp_blk.ensure((u64)S.n_keys * h->pp_nb + 8, 64));
    if (S.has_strings && pp_records(h)) {
        launch_pp_grec_lengths(h->stream, h->dspec, h->pp_grec, h->pp_tot, h->pp_blk, h->pp_nb, h->dbatches);
        for (int c = 0; c < S.n_keys; ++c)
            if (S.key_types[c].type == DBG_STRING)
                launch_exclusive_scan(h->stream, h->pp_blk + (u64)c * h->pp_nb, h->pp_nb, h->pp_tot + PPT_STR + c);
    }
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

static int pp_read_tot(dbg_agg_handle* h) {
    if (!h->pp_htot) RETURN_IF(h->pp_htot.ensure(PPT_WORDS));
    HIPCHECK(hipMemcpyAsync(h->pp_htot, h->pp_tot, PPT_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->pp_stat_rounds = h->pp_htot[PPT_ROUNDS];
    h->pp_stat_spilled = h->pp_htot[PPT_SPILLED];
    if (h->pp_htot[PPT_ERR] & ERR_OVF_LOST) return fail(DBG_ERR_INTERNAL, "partitioned aggregate: spill list exhausted");
    return DBG_OK;
}

// Decimal128 (precision > 18) and Decimal256 MIN/MAX states are the only updates that can give up
// (at_minmax128 / at_minmax256); handles without them skip the read-back.
static int check_minmax_spin(dbg_agg_handle* h) {
    bool any = false;
    for (int a = 0; a < h->spec.n_aggs; ++a) any |= (h->spec.aggs[a].mmk == MMK_I128 || h->spec.aggs[a].mmk == MMK_I256) &&
                                                    (h->spec.aggs[a].kind == DBG_AGG_MIN || h->spec.aggs[a].kind == DBG_AGG_MAX);
    if (!any) return DBG_OK;
    u64 e = 0;
    HIPCHECK(hipMemcpyAsync(&e, h->counters + CNT_ERR, 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    return err_bits_fail(e, ERR_MINMAX_SPIN);
}

// dbg_agg_finalize in partitioned mode: group records built, sizes known.
int pp_finalize(dbg_agg_handle* h, uint64_t* n_groups, uint64_t* string_bytes) {
    RETURN_IF(check_minmax_spin(h));
    if (!h->pp_grec_ready) {
        RETURN_IF(pp_grec_build(h));
        RETURN_IF(pp_read_tot(h));
        if (h->pp_htot[PPT_GROUPS] > pp_records(h)) return fail(DBG_ERR_INTERNAL, "partitioned aggregate: more groups than records");
        h->pp_grec_ready = true;
    }
    h->finalized = true;
    groups_known(h, h->pp_htot[PPT_GROUPS], h->pp_htot + PPT_STR, nullptr, n_groups, string_bytes);
    return DBG_OK;
}

// Fused finalize in partitioned mode: the LDS aggregation writes the result columns directly
// (fixed-width keys) or through group records (string keys: offsets need the scanned lengths).
int pp_fin_launch(dbg_agg_handle* h, const OutDesc& od) {
    const Spec& S = h->spec;
    if (!S.has_strings) {
        RETURN_IF(pp_agg(h, 0, &od));
    } else {
        RETURN_IF(pp_grec_build(h));
        if (pp_records(h)) {
            prof::Scope ps("pp_write", h->stream);
            launch_pp_grec_write(h->stream, h->dspec, h->dbatches, h->pp_grec, h->pp_tot, h->pp_blk, h->pp_nb, od,
                                 h->pp_tot + PPT_ERR);
        }
    }
    launch_finish_outputs(h->stream, od, h->pp_tot, S.n_keys, S.n_aggs);
    if (!h->pp_htot) RETURN_IF(h->pp_htot.ensure(PPT_WORDS));
    HIPCHECK(hipMemcpyAsync(h->pp_htot, h->pp_tot, PPT_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipGetLastError());
    return DBG_OK;
}

int pp_fin_complete(dbg_agg_handle* h, uint64_t* n_groups, uint64_t* string_bytes) {
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->uploads_pending = false;
    const u64* t = h->pp_htot;
    h->pp_stat_rounds = t[PPT_ROUNDS];
    h->pp_stat_spilled = t[PPT_SPILLED];
    const bool short_buf = groups_known(h, t[PPT_GROUPS], t + PPT_STR, &h->fin, n_groups, string_bytes);
    h->pp_grec_ready = h->spec.has_strings != 0;
    h->finalized = h->pp_grec_ready;
    if (t[PPT_ERR] & ERR_DEC_OVERFLOW) return fail(DBG_ERR_OVERFLOW, "Decimal overflow");
    if (t[PPT_ERR] & ERR_OVF_LOST) return fail(DBG_ERR_INTERNAL, "partitioned aggregate: spill list exhausted");
    RETURN_IF(check_minmax_spin(h));
    if (short_buf) return fail(DBG_ERR_INVALID, "output buffers too small: " + std::to_string(h->n_groups) + " groups");
    return DBG_OK;
}
