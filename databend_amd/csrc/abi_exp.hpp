// abi_exp.hpp — EXPERIMENT hooks of the host units, kept out of the product functions that call
// them (abi_finalize.hip: exp_fused_fin; abi_pp.hip: exp_pp_trace).  They act only in a library
// built with `make EXP=1` (X_ENV reads DBG_X_* knobs) or `make TRACE=1` (kPhaseTrace); in the
// shipped build X_ENV is a null constant and kPhaseTrace false, so each hook reduces to nothing.
#pragma once
#include "abi_internal.hpp"

// EXPERIMENT (DBG_X_TRACE): the phase-trace ring of the fused launches, 16 words per launch and
// 4096 launches, indexed by a process-wide launch count, and the host's two stamps around its turn
// between batches (completion word seen -> the next launch call has returned).
struct XTrace {
    u64* ring = nullptr;
    u64 launches = 0;
    std::vector<u64> init;
    std::chrono::steady_clock::time_point seen_at;
    bool seen = false;
    std::vector<double> host_us;
};
inline XTrace& x_tr() {
    static XTrace x;
    return x;
}
inline bool x_trace_on() {
    static const bool on = kPhaseTrace && X_ENV("DBG_X_TRACE");
    return on;
}
// fin_complete saw the launch's completion word
inline void exp_completion_seen() {
    if (!x_trace_on()) return;
    x_tr().seen_at = std::chrono::steady_clock::now();
    x_tr().seen = true;
}
// the fused launch call of fin_launch has returned (on whichever handle)
inline void exp_launch_returned() {
    XTrace& X = x_tr();
    if (!x_trace_on() || !X.seen) return;
    X.host_us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - X.seen_at).count());
    X.seen = false;
}
inline void x_trace_dump() {
    XTrace& X = x_tr();
    std::vector<u64> hb(4096 * 16);
    hipDeviceSynchronize();
    hipMemcpy(hb.data(), X.ring, hb.size() * 8, hipMemcpyDeviceToHost);
    auto median_line = [](const char* what, std::vector<double>& v) {
        if (v.empty()) return;
        std::sort(v.begin(), v.end());
        fprintf(stderr, "trace %-44s median %7.2f us  min %7.2f  max %7.2f  (n=%zu)\n", what, v[v.size() / 2], v.front(), v.back(),
                v.size());
    };
    auto whole = [](const u64* r) { return r[0] != 0 && r[0] != ~0ULL && r[1] != ~0ULL && r[6] != 0; };
    std::vector<std::vector<double>> d(14);
    for (int k = 0; k < 4096; ++k) {
        const u64* r = &hb[k * 16];
        if (!whole(r)) continue;
        for (int p = 1; p <= 14; ++p)
            if (r[p]) d[p - 1].push_back((double)(r[p] - r[0]) * 0.01);  // (a stamp this path never takes stays 0)
    }
    const char* nm[] = {"first WG stream end", "last WG stream end", "last block_flush end",
                        "ticket (last WG)", "table copied", "finalize end", "fin: scanned",
                        "fin: groups written", "fin: bits packed", "fin: counters read",
                        "tail: view+counts", "tail: prefix", "tail: t0 loads", "tail: t0 merged"};
    for (int p = 0; p < 14; ++p) {
        if (d[p].empty()) continue;
        std::sort(d[p].begin(), d[p].end());
        fprintf(stderr, "trace %-22s median %7.2f us  (n=%zu)\n", nm[p], d[p][d[p].size() / 2], d[p].size());
    }
    // consecutive launches j, j + 1 of the process (the clock is absolute): where j + 1's first
    // workgroup starts against j's first stream end and against j's finalize end (negative:
    // before it)
    std::vector<double> vs_stream, vs_fin;
    const u64 n = X.launches, first = n > 4096 ? n - 4096 : 0;
    for (u64 j = first; j + 1 < n; ++j) {
        const u64* a = &hb[(j & 4095) * 16];
        const u64* b = &hb[((j + 1) & 4095) * 16];
        if (!whole(a) || !whole(b)) continue;
        vs_stream.push_back((double)(int64_t)(b[0] - a[1]) * 0.01);
        vs_fin.push_back((double)(int64_t)(b[0] - a[6]) * 0.01);
    }
    median_line("next first WG start - first WG stream end", vs_stream);
    median_line("next first WG start - finalize end", vs_fin);
    median_line("host: completion seen -> next launch returned", X.host_us);
}

// The fused insert + finalize launch (fin_launch), after `ff` is filled: the direct-mapped
// hand-off (DBG_X_DENSE=1) and the per-launch phase trace (DBG_X_TRACE, dumped at exit).
static int exp_fused_fin(dbg_agg_handle* h, const FinState& F, FusedFin& ff) {
    const Spec& S = h->spec;
    {  // COUNT(*) over a <= 16-bit key into a recycled table: the direct-mapped hand-off
        // measured and not kept (C2 step 45.1 -> 138 us: 256 workgroups' device atomics on the
        // same ~33 addresses serialise at the memory side, profiles/r04/c2_dense_ab.json):
        // EXPERIMENT, DBG_X_DENSE=1
        static const bool dense_on = X_ENV("DBG_X_DENSE") && X_ENV("DBG_X_DENSE")[0] == '1';
        const int kt = S.key_types[0].type;
        const u32 kw = (kt == DBG_INT8 || kt == DBG_UINT8) ? 1 : ((kt == DBG_INT16 || kt == DBG_UINT16) ? 2 : 0);
        const bool co = S.n_aggs == 1 && S.aggs[0].kind == DBG_AGG_COUNT && S.aggs[0].arg_type < 0 && S.aggs[0].w0 == 1;
        if (dense_on && kw && co && h->def_clean && S.n_keys == 1) {
            if (!h->dense) {
                RETURN_IF(h->dense.ensure(65536 + 1024));
                HIPCHECK(hipMemsetAsync(h->dense, 0, (65536 + 1024) * 8, h->stream));
            }
            ff.dense = h->dense;
            ff.dense_n = kw == 1 ? 256u : 65536u;
        }
    }
    if (x_trace_on()) {
        XTrace& X = x_tr();
        if (!X.ring) {
            RETURN_IF(dev_alloc((void**)&X.ring, 4096 * 128));
            X.init.assign(16, 0);
            X.init[0] = X.init[1] = ~0ULL;
            atexit(x_trace_dump);
        }
        // one entry per launch of the process, whichever handle it is on: two handles' sequence
        // numbers would meet in the same entries
        ff.trace = X.ring + (X.launches++ & 4095) * 16;
        HIPCHECK(hipMemcpyAsync(ff.trace, X.init.data(), 128, hipMemcpyHostToDevice, h->stream));
    }
    return DBG_OK;
}

// The partitioned payload's aggregation (pp_agg): per-partition phase times of its kernels
// (DBG_X_PPTRACE, dumped at exit).
static int exp_pp_trace(dbg_agg_handle* h, PPAggOut& o) {
    static u64* x_pptrace = nullptr;  // EXPERIMENT (DBG_X_PPTRACE)
    if (kPhaseTrace && X_ENV("DBG_X_PPTRACE")) {
        if (!x_pptrace) {
            RETURN_IF(dev_alloc((void**)&x_pptrace, 64));
            HIPCHECK(hipMemset(x_pptrace, 0, 64));
            atexit([] {
                u64 v[8];
                hipDeviceSynchronize();
                hipMemcpy(v, x_pptrace, 64, hipMemcpyDeviceToHost);
                const double n = v[5] ? (double)v[5] : 1.0;
                fprintf(stderr, "pptrace raw us/partition [0..4] %.2f %.2f %.2f %.2f %.2f (spec kernel: load+hash, stage, insert, "
                                "emit, barriers)\n", v[0] * 0.01 / n, v[1] * 0.01 / n, v[2] * 0.01 / n, v[3] * 0.01 / n, v[4] * 0.01 / n);
                fprintf(stderr, "pptrace partitions %llu groups/partition %.0f  per partition us: insert %.2f sync %.2f "
                                "atomic %.2f write %.2f tail %.2f\n", (unsigned long long)v[5], v[6] / n, v[0] * 0.01 / n,
                        v[1] * 0.01 / n, v[2] * 0.01 / n, v[3] * 0.01 / n, v[4] * 0.01 / n);
            });
        }
        o.trace = x_pptrace;
    }
    return DBG_OK;
}
