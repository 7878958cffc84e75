// reduce.hpp — aggregation without GROUP BY (reduce.hip), shared with the abi_*.hip units.
//
// A handle created with no group columns has one state and no table: the state words of one slot
// (Spec::aggs[a].w0 / nwords, Spec::slot_init, Spec::flags_word; word 0, the entry, is unused) in a
// small device buffer.  A batch is reduced by keyless_reduce_kernel into one partial state per
// workgroup, and keyless_merge_kernel folds those rows (or decoded serialized states) into the
// handle's state.  Results and serialized states are written from that one state by the writers
// of the grouped path (write_agg, agg_dev.hpp).
#pragma once
#include "agg.hpp"
#include "serde.hpp"

#define KEYLESS_NT 256                           // threads of a workgroup
#define KEYLESS_R 8                              // contiguous rows per lane and strip
#define KEYLESS_U 4                              // strips per tile
#define KEYLESS_TILE (KEYLESS_NT * KEYLESS_R * KEYLESS_U)  // rows of one workgroup trip
#define KEYLESS_MAX_BLOCKS DBG_INSERT_MAX_BLOCKS  // grid cap of a reduce launch
// The flags word of a keyless state: bit Spec::aggs[a].flag_bit = a non-NULL value reached SUM /
// MIN / MAX a (every one of them has a bit, nullable argument or not: the empty input is NULL);
// bit KEYLESS_SEEN_BIT = a row reached accumulate (the OrNull adaptor's flag).
#define KEYLESS_SEEN_BIT 63

inline u32 keyless_grid(u64 rows) {
    const u64 tiles = (rows + KEYLESS_TILE - 1) / KEYLESS_TILE;
    return (u32)(tiles < KEYLESS_MAX_BLOCKS ? (tiles ? tiles : 1) : KEYLESS_MAX_BLOCKS);
}
// state: stride_words words, set to the initial state
void launch_keyless_init(hipStream_t s, const Spec* dspec, u64* state);
// `rows` rows of *batch (device) -> partials[blocks][stride_words], every word of every row written
void launch_keyless_reduce(hipStream_t s, const Spec* dspec, const BatchDesc* batch, u64 rows, u64* partials, u32 blocks);
// n states of `stride` words (slot layout) folded into *state, in stream order
void launch_keyless_merge(hipStream_t s, const Spec* dspec, const u64* states, u64 n, u32 stride, u64* state);
// n rows of borsh states -> words[n][stride_words]; err: ERR_SER_MALFORMED
void launch_keyless_decode(hipStream_t s, const Spec* dspec, const SerIngest& in, u64 n, u64* words, u64* err);
// the one result row (or, out.ser, the one row of serialized states) of *state
void launch_keyless_write(hipStream_t s, const Spec* dspec, const u64* state, const OutDesc& out, u64* err);
