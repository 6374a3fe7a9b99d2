// vf_where.h -- a metadata filter evaluated per row (vf_index_search_device with VF_SEARCH_WHERE: k_where_eval, k_where_scan, k_where_ids
// in vf_where.hip), as plain functions the kernels, their host side (vf_api.hip) and a host-compiled test (tests/test_where_plan.py:
// UBSan) share.  The grammar, the kinds and every ordering question live in veritasfi_amd/where.py; what arrives here is a PROGRAM over
// int64 key columns:
//   * columns: per field the keys [n] and a validity bitmap (bit r & 31 of word r >> 5; null = every row has the field);
//   * leaves:  kWhereInterval  valid && lo <= key <= hi  (lo > hi: the empty leaf, its column is not read)
//              kWhereSet       valid && key is in the strictly ascending run set_values[lo, lo + hi)
//              kWhereMissing   !valid
//   * ops:     postfix, one byte each: a value below 0x80 pushes that leaf's verdict; kWhereAnd / kWhereOr pop two and push one,
//              kWhereNot flips the top.  The program leaves exactly one value.
// The evaluation stack is the bits of ONE uint32_t (depth <= 32), so an evaluator needs no array and a kernel no scratch.
// The limits are design constants, not measurements; veritasfi_amd/where.py mirrors them and evaluates what exceeds them in NumPy.
// Output geometry: a bitmap in the BM25 filter's layout (uint32 words, bit r & 31 of word r >> 5, 2 * ceil(n / 64) words, zero at and
// past n), one passing-row count per TILE of tile_rows rows (a multiple of 64 in [64, 1024]; default 1024), their exclusive prefix,
// and the passing rows' ids: row r goes to prefix[tile of r] + (passing rows of its tile below r).
// No HIP header: the host compiler reads it as it stands.
#pragma once

#include <stdint.h>

#include "vf_scan_lds.h"   // VF_HD

namespace vf {

constexpr int kWhereMaxLeaves = 64;
constexpr int kWhereMaxOps = 128;
constexpr int kWhereMaxDepth = 32;
constexpr int kWhereMaxColumns = 16;
constexpr long long kWhereMaxSetValues = 65536;
constexpr int kWhereTileRows = 1024;         // the default tile; a wave step is 64 rows
constexpr int kWhereWaveRows = 64;

enum WhereOp { kWhereAnd = 0x80, kWhereOr = 0x81, kWhereNot = 0x82 };
enum WhereLeafKind { kWhereInterval = 0, kWhereSet = 1, kWhereMissing = 2 };

struct WhereLeaf {           // vf_where_leaf of include/veritasfi_hip.h
    int32_t kind, column;
    int64_t lo, hi;          // interval: the inclusive bounds; set: offset and length of the run in set_values; missing: unused
};
static_assert(sizeof(WhereLeaf) == 24, "the leaves are uploaded as they stand");

// ---- the checks ------------------------------------------------------------------------------------------------------------------
enum WhereVerdictKind {
    kWhereOk = 0,
    kWhereOverLimits = 1,     // a count above its limit, or a stack deeper than kWhereMaxDepth: `at` says which (WhereLimit) or the op
    kWhereEmpty = 2,          // no op, no leaf or no column
    kWhereBadOp = 3,          // ops[at] is neither a leaf of the program nor one of the three operators
    kWhereUnderflow = 4,      // ops[at] pops more than the stack holds
    kWhereLeftover = 5,       // the program leaves `at` values, not one
    kWhereBadLeaf = 6,        // leaves[at]: unknown kind, or a column outside the table
    kWhereBadSetRun = 7,      // leaves[at]: its run is not inside set_values
    kWhereSetNotAscending = 8 // set_values[at] is not above its predecessor in the run of a set leaf
};
enum WhereLimit { kWhereLimitLeaves = 0, kWhereLimitOps = 1, kWhereLimitColumns = 2, kWhereLimitSetValues = 3, kWhereLimitDepth = 4 };
struct WhereVerdict { int verdict; long long at; int limit; };

// the first offending position of a program, in the order: limits, emptiness, leaves (kind, column, run, ascending), ops (stack)
VF_HD WhereVerdict where_validate(const WhereLeaf* leaves, int n_leaves, const uint8_t* ops, int n_ops, int n_columns,
                                  const int64_t* set_values, long long n_set_values) {
    WhereVerdict v{kWhereOk, 0, -1};
    if (n_leaves > kWhereMaxLeaves) { v.verdict = kWhereOverLimits; v.at = n_leaves; v.limit = kWhereLimitLeaves; return v; }
    if (n_ops > kWhereMaxOps) { v.verdict = kWhereOverLimits; v.at = n_ops; v.limit = kWhereLimitOps; return v; }
    if (n_columns > kWhereMaxColumns) { v.verdict = kWhereOverLimits; v.at = n_columns; v.limit = kWhereLimitColumns; return v; }
    if (n_set_values > kWhereMaxSetValues) { v.verdict = kWhereOverLimits; v.at = n_set_values; v.limit = kWhereLimitSetValues; return v; }
    if (n_leaves < 1 || n_ops < 1 || n_columns < 1 || n_set_values < 0) { v.verdict = kWhereEmpty; return v; }
    for (int i = 0; i < n_leaves; ++i) {
        const WhereLeaf& l = leaves[i];
        if (l.kind < kWhereInterval || l.kind > kWhereMissing || l.column < 0 || l.column >= n_columns) { v.verdict = kWhereBadLeaf; v.at = i; return v; }
        if (l.kind != kWhereSet) continue;
        if (l.lo < 0 || l.hi < 0 || l.lo > n_set_values || l.hi > n_set_values - l.lo) { v.verdict = kWhereBadSetRun; v.at = i; return v; }
        for (int64_t j = l.lo + 1; j < l.lo + l.hi; ++j)
            if (set_values[j] <= set_values[j - 1]) { v.verdict = kWhereSetNotAscending; v.at = j; return v; }
    }
    int depth = 0;
    for (int i = 0; i < n_ops; ++i) {
        const int op = ops[i];
        if (op < 0x80) {
            if (op >= n_leaves) { v.verdict = kWhereBadOp; v.at = i; return v; }
            if (++depth > kWhereMaxDepth) { v.verdict = kWhereOverLimits; v.at = i; v.limit = kWhereLimitDepth; return v; }
        } else if (op == kWhereAnd || op == kWhereOr) {
            if (depth < 2) { v.verdict = kWhereUnderflow; v.at = i; return v; }
            --depth;
        } else if (op == kWhereNot) {
            if (depth < 1) { v.verdict = kWhereUnderflow; v.at = i; return v; }
        } else { v.verdict = kWhereBadOp; v.at = i; return v; }
    }
    if (depth != 1) { v.verdict = kWhereLeftover; v.at = depth; return v; }
    return v;
}

// ---- the interpreter ---------------------------------------------------------------------------------------------------------------
// key in the strictly ascending run [run, run + len): a halving search whose trip count depends on len alone (uniform across a wave)
template <class Run>
VF_HD bool where_in_run(Run run, long long len, int64_t key) {
    if (len <= 0) return false;
    long long at = 0;
    while (len > 1) {
        const long long half = len >> 1;
        if (run[at + half] <= key) at += half;
        len -= half;
    }
    return run[at] == key;
}

// One row through a program where_validate accepted.  key_of(column) / valid_of(column) read the row's key and validity; set_values
// is anything indexable.  Both the host driver and k_where_eval run exactly this.
template <class Leaves, class Ops, class Sets, class KeyOf, class ValidOf>
VF_HD bool where_eval_row(Leaves leaves, Ops ops, int n_ops, Sets set_values, KeyOf key_of, ValidOf valid_of) {
    uint32_t stack = 0;      // bit 0 is the top
    for (int i = 0; i < n_ops; ++i) {
        const uint32_t op = ops[i];
        if (op < 0x80u) {
            const int32_t kind = leaves[op].kind, column = leaves[op].column;
            const int64_t lo = leaves[op].lo, hi = leaves[op].hi;
            bool pass;
            if (kind == kWhereMissing) pass = !valid_of(column);
            else if (kind == kWhereInterval) {
                pass = false;
                if (lo <= hi) { const int64_t key = key_of(column); pass = valid_of(column) && lo <= key && key <= hi; }
            } else pass = valid_of(column) && where_in_run(set_values + lo, hi, key_of(column));
            stack = (stack << 1) | (pass ? 1u : 0u);
        } else if (op == (uint32_t)kWhereNot) {
            stack ^= 1u;
        } else {
            const uint32_t top = stack & 1u;
            stack >>= 1;
            stack = op == (uint32_t)kWhereAnd ? (stack & (top | ~1u)) : (stack | top);
        }
    }
    return (stack & 1u) != 0;
}

// ---- the output geometry -----------------------------------------------------------------------------------------------------------
VF_HD bool where_tile_rows_ok(int tile_rows) { return tile_rows >= kWhereWaveRows && tile_rows <= kWhereTileRows && tile_rows % kWhereWaveRows == 0; }
VF_HD long long where_groups(long long n) { return (n + kWhereWaveRows - 1) / kWhereWaveRows; }             // wave steps: 64 rows each
VF_HD long long where_bitmap_words(long long n) { return 2 * where_groups(n); }
VF_HD long long where_tiles(long long n, int tile_rows) { return (n + tile_rows - 1) / tile_rows; }
VF_HD long long where_tile_of(long long row, int tile_rows) { return row / tile_rows; }
VF_HD int where_popcount64(uint64_t v) { return __builtin_popcountll(v); }
// the 64 verdicts of group g as one word: bit i is row 64 g + i
template <class Words>
VF_HD uint64_t where_group_bits(Words bitmap, long long g) { return (uint64_t)bitmap[2 * g] | ((uint64_t)bitmap[2 * g + 1] << 32); }
VF_HD bool where_bit(const uint32_t* bitmap, long long row) { return (bitmap[row >> 5] >> (row & 31)) & 1u; }
// passing rows of `row`'s tile that lie below it: where the row's id goes, counted from its tile's prefix
VF_HD long long where_rank_in_tile(const uint32_t* bitmap, long long row, int tile_rows) {
    const long long g0 = where_tile_of(row, tile_rows) * (tile_rows / kWhereWaveRows), g = row / kWhereWaveRows;
    long long rank = 0;
    for (long long j = g0; j < g; ++j) rank += where_popcount64(where_group_bits(bitmap, j));
    const int lane = (int)(row % kWhereWaveRows);
    return rank + where_popcount64(where_group_bits(bitmap, g) & (lane ? (~0ull >> (64 - lane)) : 0ull));
}

// the uploaded descriptor block: the column table, the leaves, the ops, then the set values (each part padded to 256 bytes)
struct WhereColumnPtr { const int64_t* keys; const uint32_t* valid; };
static_assert(sizeof(WhereColumnPtr) == 16, "the column table is uploaded as it stands");
VF_HD long long where_pad256(long long bytes) { return (bytes + 255) & ~255ll; }
struct WhereBlock { long long columns_at, leaves_at, ops_at, sets_at, bytes; };
VF_HD WhereBlock where_block(int n_columns, int n_leaves, int n_ops, long long n_set_values) {
    WhereBlock b{};
    b.columns_at = 0;
    b.leaves_at = b.columns_at + where_pad256((long long)n_columns * (long long)sizeof(WhereColumnPtr));
    b.ops_at = b.leaves_at + where_pad256((long long)n_leaves * (long long)sizeof(WhereLeaf));
    b.sets_at = b.ops_at + where_pad256(n_ops);
    b.bytes = b.sets_at + where_pad256(n_set_values * 8);
    return b;
}

}  // namespace vf
