// abi_internal.hpp — what the C-ABI translation units share: the handle (one AggregateHashTable in
// HBM), its finalize state, the error / HIP-check helpers, and the functions that cross units
// (declared at the end, by the unit that defines them; all hidden from the library's interface).
// The units: abi.hip the handle itself (error slot, table, batches, inserts), abi_spec.hip specs and
// layouts, abi_pp.hip the partitioned payload's host side, abi_finalize.hip both finalize families,
// abi_records.hip records / partition / merge / compact, abi_ops.hip the handle-free entry points,
// prof.hip the event profiler, exchange.hip the multi-GPU exchange over RCCL, expr.hip the projection
// (its kernel and its two entry points together).  A handle without group
// columns (is_keyless) is one state instead of a table: its kernels are reduce.hip's, its host steps
// sit in the same units beside the table's (keyless_add, keyless_merge_serialized, result_impl).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>
#include <chrono>

#include "agg.hpp"
#include "dev_buf.hpp"
#include "host_stage.hpp"
#include "legacy.hpp"
#include "serde.hpp"
#include "reduce.hpp"

#include "filter.hpp"
#include "like.hpp"
#include "sort.hpp"
#include "prof.hpp"

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
int fail(int code, const std::string& msg);

#define HIPCHECK(expr)                                                                         \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return fail(DBG_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)

#define RETURN_IF(rc) \
    do {              \
        int _r = (rc); \
        if (_r != DBG_OK) return _r; \
    } while (0)

// Entry points outside the hash aggregate (filter predicates, take, sort, legacy hash methods)
// carry values as at most two words: a Decimal256 column is refused, never read with a narrower width.
#define REFUSE_DECIMAL256(t, what)                                                                           \
    do {                                                                                                     \
        if ((t) == DBG_DECIMAL256) return fail(DBG_ERR_UNSUPPORTED, std::string(what) + ": Decimal256 columns are not supported"); \
    } while (0)

// ------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------
// Every buffer a handle owns is a Buf member (dev_buf.hpp), freed with the handle: a member that
// is a raw pointer aliases memory owned elsewhere and says so.
using DevBuf = Buf<u8>;  // device bytes; cap() = bytes

struct FinState {
    bool active = false;
    std::vector<dbg_out_column> aggs, keys;
    u64 max_groups = 0;
    bool has_max_str = false;
    std::vector<u64> max_str;
    u64 cap_str[DBG_MAX_KEYS] = {};
    bool zero_copy = false;
    u64 seq = 0;
    bool direct = false;  // the held-back partitioned insert's direct stage wrote the results (part_slice_direct)
};

// A record buffer of the partitioned payload ends in PP_SLACK bytes the records do not use (the
// aggregation reads whole words): the records of `rw` bytes a buffer of `cap` bytes holds.
constexpr u64 PP_SLACK = 64;
inline u64 pp_rec_cap(u64 cap, u64 rw) { return cap > PP_SLACK ? (cap - PP_SLACK) / rw : 0; }

struct dbg_agg_handle {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    Spec spec{};
    Buf<Spec> dspec;
    std::vector<dbg_datatype> result_types;
    std::vector<int> src_kinds;  // dbg_agg_kind as created (AVG_SQL is stored as AVG)
    bool partial = true;

    // table
    Buf<u64> slots;
    u64 cap = 0;       // slots of the table (the buffer holds cap + 1)
    u64 init_cap = 0;  // from the capacity hint: the table never shrinks below it
    // An on-device fast-path insert whose launch is held back until the next call: a
    // finalize_into_async of a small table then runs in the same launch (FusedFin); any other
    // call launches it first (flush_deferred).
    bool def_on = false;
    bool def_clean = false;  // the table was empty (recycled / reset) when the insert was held back
    u32 def_bid = 0;
    u64 def_rows = 0;
    BatchDesc def_hb;
    Buf<u64> counters;             // device, CNT_WORDS
    Buf<u64, MappedMem> hcounters;  // pinned; its tail mirrors what the finalize kernels post
    u64* hcounters_dev = nullptr;  // alias: its device mapping (finalize_small writes it directly)
    Buf<u64> dense;                // fused_dense's direct-mapped counts + presence bitmap (zero between launches)
    // overflow lists (deferred): rows, and records of tstride words
    Buf<u64> ovf_rows, ovf_recs;
    u64 pending_rows = 0, pending_recs = 0;
    // parking rows of per-workgroup partial tables (TableDesc::scratch)
    Buf<u64> scratch;
    u32 scr_blocks = 0;

    // batches (ids 1..n_batches); descs in device memory, staged through pinned memory
    Buf<BatchDesc> dbatches;
    u32 n_batches = 0;
    // descriptor cache: ids 1..n_cached hold immutable descriptors of device-resident inputs
    // (pointers only), kept across dbg_agg_reset so a re-submitted batch needs no upload
    u32 n_cached = 0;
    std::vector<std::pair<u64, BatchDesc>> desc_cache;  // (content hash, host copy); index = id - 1
    std::vector<BatchDesc*> pinned_descs;   // alias: pinned staging desc per batch id (pooled)
    std::vector<PinnedBuf<BatchDesc>> pinned_chunks;  // their allocations
    std::vector<DevBuf> owned;             // device copies of host inputs / filter constants
    // before_merge exchange receive buffers (records, string blobs) when this is the final table:
    // kept across resets and grown only, so a step allocates nothing; `xrecv_busy` while the table
    // may reference them (merged since the last reset) — an exchange then allocates fresh ones
    DevBuf xrecv[2];
    bool xrecv_busy = false;
    // chunked before-partial shuffle (dbg_agg_exchange_payload_chunk): level-1 segments from
    // xfirst[k] on are not shipped yet; what arrived per call waits in xchunks until the last call.
    // The receive buffers belong to the communicator (one grow-only pair per chunk slot, received
    // into on its stream), so no step allocates or frees them and the handle never frees memory a
    // transfer may still be writing.
    struct XChunk {
        std::vector<u64> pc;  // [n][2][P] counts of the chunk, every source
        const void* recv[2] = {nullptr, nullptr};  // alias: the communicator's slots
    };
    std::vector<XChunk> xchunks;
    u32 xfirst[2] = {0, 0};

    // finalize state
    bool finalized = false;
    u64 n_groups = 0;
    std::vector<u64> string_bytes;
    std::vector<u64> agg_string_bytes;  // payload bytes of each String MIN/MAX result column (dbg_agg_finalize)
    Buf<u64> d_pos;      // scanned per-block group counts
    Buf<u64> d_str_pos;  // [n_keys][blocks] scanned per column
    // partition state
    u32 part_n = 0;
    int part_scheme = 0;
    int part_keys = 0;  // dbg_agg_set_partition_keys: buckets by the first part_keys key columns (0 = all)
    u64 part_nb = 0;  // blocks of the partition histogram
    Buf<u64> d_part_pos, d_part_str_pos, d_part_str_base;
    Buf<u64> d_lpart;  // scheme 2: legacy bucket per slot / group record (u32)
    std::vector<u64> part_counts, part_strings;
    // fused finalize: validity bytes staging
    Buf<u8> vbytes;
    // fused finalize in flight (dbg_agg_finalize_into_async)
    FinState fin;
    hipEvent_t switch_ev = nullptr;  // dbg_agg_set_stream hand-off
    // recycle mode (dbg_agg_set_recycle): a small-table finalize_into leaves the table empty
    int recycle = 0;
    bool clean = false;           // table already re-initialised by the last finalize
    // dbg_agg_reset deferred the table's initialisation (counters and the sentinel slot are
    // initialised): table_desc() runs it before any kernel touches the table, except a
    // partitioned insert, whose slice kernel starts every slice EMPTY and writes the whole table
    bool init_pending = false;
    // sequence number the finalize kernel posts to host_mirror and the tagged fused chain tags its
    // parked words with (fin_launch skips the values whose low FIN_SEQ_TAG_PERIOD bits are 0).  It
    // starts just below the wrap of the chain's wider tag, so every handle crosses both tag wraps
    // within its first 32 finalizes instead of after a million.
    u64 fin_seq = (1ULL << 24) - 32;
    u64 scr_period = ((1ULL << 24) - 32) / FIN_SEQ_TAG_PERIOD;  // fin_seq's tag period when the scratch was last cleared
    bool uploads_pending = false; // descriptor uploads from pinned staging since the last sync
    // radix-partitioned insert (part.hip): sorted mixed keys, slice bounds, rocPRIM scratch
    Buf<u64> part_sorted, part_bounds;
    Buf<u8> part_temp;
    // A partitioned insert into an empty table in recycle mode holds back its table stage (the
    // keys are sorted already): a finalize_into that comes next runs the direct stage instead —
    // groups into the result columns without the table-wide count and write passes, the slots used
    // as scratch and left to be initialised like a reset table (launch_part_direct);
    // anything else that touches the table launches the regular slice stage first (part_flush).
    bool def_part = false;
    u32 def_part_sb = 0;
    int def_part_kw = 0;
    Buf<u64> part_status;  // the direct stage's look-back words
    u64 insert_paths[INS_N_PATHS] = {};  // launch_insert calls by the kernel they took, since create (dbg_agg_insert_paths)
    u64 table_rows = 0;  // rows / records inserted into the HBM table since the last reset
    u64 remerged = 0;    // of which records dbg_agg_compact merged back (groups, not input rows)
    int strategy = DBG_STRATEGY_AUTO;
    u64 hint_groups = 0;  // dbg_agg_params.capacity_hint
    // cardinality the last table-mode finalize observed (kept across reset): rows / records
    // inserted and the groups they formed.  A handle reused for the next batch of the same query
    // shape decides its strategy from it instead of probing again (no probe kernel, no host sync)
    u64 obs_rows = 0, obs_groups = 0;

    // ---- partitioned payload (pp.hip): high-cardinality mode ----
    bool pp = false;          // batches go to the radix-partitioned payload, not the HBM table
    double pp_ratio = 1.0;    // estimated groups per selected row (cardinality probe)
    double est_groups = 0;    // the probe's (or the last finalize's) group estimate for this batch
    bool pp_probed = false;   // pp_ratio comes from a probe (not the default upper bound)
    struct Seg {
        u64 base, n;
        std::vector<u64> off;  // level-1 partition offsets (257), relative to base
    };
    struct Kind {  // 0: raw records (add_groups), 1: state records (merge_records)
        Buf<u8> l1;
        u64 l1_n = 0;   // records
        Buf<u16> dig;   // level-2 digits of records [0, dig_n) (fixed-shape raw level 1)
        u64 dig_n = 0;
        std::vector<Seg> segs;
        Buf<u8> a, b;   // finalize levels: ping-pong buffers of one size, l1_n records each
        Buf<u64> part;  // final partition offsets (device)
        u8* fin = nullptr;  // alias: the final-level buffer (a or b) and its alternate (the aggregate's overflow)
        u8* alt = nullptr;  // alias
    } ppk[2];
    u32 pp_bits = 0;  // final partition bits
    int pp_spec = -1;   // >= 0: the compile-time specialised aggregation's shape (pp_agg_spec_kernel)
    u32 pp_spec_sub = 0;  // its rounds per partition: 2^pp_spec_sub
    // [count, partition ids...] spilled by the specialised kernel: an id per final partition, so
    // no spill is ever dropped
    Buf<u32> pp_spill;
    Buf<u32> pp_cnt;
    Buf<u64> pp_off;
    Buf<u64> pp_scan_tmp;  // scan scratch (group totals, block sums)
    u64* pp_last_part = nullptr;  // alias: partition offsets of the last count_scan (read by its scatter)
    Buf<u64> pp_mid;  // intermediate partition offsets (device)
    Buf<PPChunk> pp_dchunks;
    PinnedBuf<PPChunk> pp_hchunks;  // staging
    Buf<u32> pp_dc0;
    PinnedBuf<u32> pp_hc0;
    PinnedBuf<u64> pp_hpart;  // read-back of partition offsets
    Buf<u64> pp_tot;          // PPT_* (device)
    PinnedBuf<u64> pp_htot;
    Buf<u64> pp_set;          // cardinality probe hash set
    Buf<u8> pp_grec;          // group records (state record format)
    Buf<u64> pp_blk;          // per-block string lengths, scanned
    bool pp_grec_ready = false;
    u64 pp_nb = 0;            // blocks of the grec passes
    u64 pp_stat_rounds = 0;   // partitions that took more than one LDS round (last finalize)
    u64 pp_stat_spilled = 0;  // final partitions handed to the generic kernel (last finalize)
    Buf<u64> ser_err;         // serialized-state ingest error bits (serde.hip)

    // host-block staging (dbg_agg_set_host_staging, host_stage.hpp)
    hstage::Stage stage;

    // ---- keyless handle (no group columns, reduce.hpp): one state instead of the table ----
    Buf<u64> kstate;     // spec.stride_words words, slot layout (word 0 unused)
    Buf<u64> kpartials;  // KEYLESS_MAX_BLOCKS rows of stride_words: a reduce launch's per-workgroup states
    u64 kl_reduces = 0;  // reduce launches / serialized states merged since create (dbg_agg_keyless_stats)
    u64 kl_merged = 0;
};

// Handle-local specs.  Records, the partitioned payload, the exchanges and the serialized states
// carry keys and states of at most 16 bytes, and a String MIN/MAX state (MMK_STR) is a reference
// into this handle's retained input.  A spec with a String MIN/MAX, or with a Decimal256 key or
// argument, therefore runs the HBM table of its own handle only: every entry point that ships,
// re-encodes or compacts states refuses it (REFUSE_HANDLE_LOCAL) with the reason given here.
inline bool is_str_minmax(const DAgg& A) { return (A.kind == DBG_AGG_MIN || A.kind == DBG_AGG_MAX) && A.mmk == MMK_STR; }
inline bool has_str_minmax(const Spec& S) {
    for (int a = 0; a < S.n_aggs; ++a)
        if (is_str_minmax(S.aggs[a])) return true;
    return false;
}
inline bool has_decimal256(const Spec& S) {
    for (int c = 0; c < S.n_keys; ++c)
        if (S.key_types[c].type == DBG_DECIMAL256) return true;
    for (int a = 0; a < S.n_aggs; ++a)
        if (S.aggs[a].arg_type == DBG_DECIMAL256) return true;
    return false;
}
// nullptr: the spec's states and keys can leave the handle
inline const char* handle_local_reason(const Spec& S) {
    if (has_str_minmax(S)) return "String min/max states are row references local to the handle (dbg_agg_result only)";
    if (has_decimal256(S)) return "Decimal256 keys and states are wider than the record formats (the HBM table of one handle only)";
    return nullptr;
}
#define REFUSE_HANDLE_LOCAL(h, what)                                                          \
    do {                                                                                      \
        if (const char* why_ = handle_local_reason((h)->spec))                                \
            return fail(DBG_ERR_UNSUPPORTED, std::string(what) + ": " + why_);               \
    } while (0)

// A keyless handle (no group columns) has one state and no hash, table, records or partitions:
// every entry point that needs one of them refuses it (REFUSE_KEYLESS).
inline bool is_keyless(const Spec& S) { return S.n_keys == 0; }
inline const char* keyless_reason() { return "the handle has no group columns (one state: no hash table, records or partitions)"; }
#define REFUSE_KEYLESS(h, what)                                                                                     \
    do {                                                                                                            \
        if (is_keyless((h)->spec)) return fail(DBG_ERR_UNSUPPORTED, std::string(what) + ": " + keyless_reason()); \
    } while (0)

inline void note_insert(dbg_agg_handle* h, InsertPath p) {
    if (p >= 0 && p < INS_N_PATHS) h->insert_paths[p]++;
}

// ------------------------------------------------------------------------------------------
// what crosses units (dev_alloc: dev_buf.hpp), by the unit that defines it
// ------------------------------------------------------------------------------------------
int build_spec(const dbg_agg_params* p, Spec& S, std::vector<dbg_datatype>& rtypes);  // abi_spec.hip
// Everything a caller queued (staged host rows, a held-back insert) reaches the table.  abi.hip
extern "C" __attribute__((visibility("hidden"))) int flush_pending(dbg_agg_handle* h);

#pragma GCC visibility push(hidden)
inline bool valid_type(int t) { return t >= DBG_INT8 && t <= DBG_DECIMAL256; }
inline u64 pow2_at_least(u64 x) {
    u64 p = 1;
    while (p < x) p <<= 1;
    return p;
}
// worst-case overflow pushes of an insert launch over n rows: every LDS slot of every workgroup
inline u64 ovf_blocks(u64 n) { return std::min<u64>(2048, (n + 4095) / 4096) + 1; }
// A kernel left the table as dbg_agg_reset does (re-initialised, or never written).
inline void mark_recycled(dbg_agg_handle* h) {
    h->clean = true;
    h->finalized = false;
    h->n_batches = h->n_cached;
    h->pending_rows = h->pending_recs = 0;
}
// Where the device copy of a caller's host bytes goes: the stream that fills it and the list that
// keeps it alive ({h->stream, h->owned} for a handle).
struct Owner {
    hipStream_t stream;
    std::vector<DevBuf>& owned;
};

// ---- abi.hip ----
// CNT_ERR bits -> return code and last-error message; `mask`: the bits this caller tests
int err_bits_fail(u64 err, u64 mask);
int own_alloc(Owner o, size_t bytes);  // o.owned.back(): `bytes` of device memory
DCol dcol_view(const dbg_column& c);   // a caller's device-resident column as the kernels read it
int to_dcol(Owner o, const dbg_column& c, const dbg_datatype& want, bool check_type, int on_device, DCol& d);
// rows: the batch's rows (the match bitmap of every DBG_PRED_LIKE node is filled on o.stream, like.hip)
int fill_filter(Owner o, const dbg_filter* f, int on_device, u64 rows, DCol* cols, int* ncols, DNode* nodes, int* nnodes);
int like_check(const uint8_t* pat, uint64_t len, LikeDesc& L);  // a LIKE pattern within the header's caps, classified
TableDesc table_desc(dbg_agg_handle* h);
int flush_deferred(dbg_agg_handle* h);
int part_flush(dbg_agg_handle* h);
int stage_flush(dbg_agg_handle* h);
int grow_table(dbg_agg_handle* h, u64 new_cap);
int resolve_overflow(dbg_agg_handle* h);
int ensure_ovf(dbg_agg_handle* h, u64 add_rows, u64 add_recs);
int new_batch(dbg_agg_handle* h, BatchDesc** staging, u32* bid);
int upload_batch(dbg_agg_handle* h, BatchDesc* st, u32 bid);
int submit_batch(dbg_agg_handle* h, BatchDesc** pst, u32* pbid, bool cacheable);
// ---- abi_spec.hip ----
u32 ser_stride_of(const DAgg& A);
// ---- abi_pp.hip ----
int pp_maybe_switch(dbg_agg_handle* h, u32 bid, u64 rows);
int pp_add_batch(dbg_agg_handle* h, const BatchDesc* st, u32 bid, u64 rows, int kind);
int pp_finalize(dbg_agg_handle* h, uint64_t* n_groups, uint64_t* string_bytes);
int pp_fin_launch(dbg_agg_handle* h, const OutDesc& od);
int pp_fin_complete(dbg_agg_handle* h, uint64_t* n_groups, uint64_t* string_bytes);
// ---- abi_finalize.hip ----
// The groups of a finalize are known: h->n_groups / h->string_bytes from the totals (str_tot[c]:
// bytes of String key column c), the caller's outputs filled where given.  Returns whether the
// groups or a String column exceed `caps` (the buffers of a finalize_into; nullptr: none to check).
bool groups_known(dbg_agg_handle* h, u64 groups, const u64* str_tot, const FinState* caps, uint64_t* n_groups,
                  uint64_t* string_bytes);
// ---- abi_ops.hip ----
int legacy_method(const dbg_datatype* types, int n, int* kind, uint32_t* key_bytes);
// The FixedKeys packing (build_keys_vec) by position j in the key: the column there, its value's
// byte offset, and its null byte's offset (-1: not nullable).
void legacy_fixed_order(const dbg_datatype* types, int n, int* order, u32* off, int32_t* null_off);
#pragma GCC visibility pop
