// vf_subset_multi.h -- a row list PER QUERY of a dense batch (vf_index_search / _device with VF_SEARCH_SUBSETS: k_subset_check_m,
// k_scan_subset_m, the ranking kernels of the exact path, k_subset_ids_m), as plain functions the kernels (vf_kernels.hip), their host
// side (vf_api.hip) and a host-compiled test (tests/test_subset_multi_plan.py: UBSan, every assignment of up to 5 queries to 3 lists
// of a 12-row index under shrunken blocking, then the arithmetic at the real constants) share.
//
// The rule: row i of such a call is what the one-list call (vf_subset.h) returns for query i alone under its own list, ids and score
// bits.  Canonical scores do not depend on what else is in the batch, so all that has to be arranged is WHICH list each workgroup reads.
//
// This mode serves lists of at most kSubsetRankRows (16 384) ids -- the lists that vf_subset.h ranks "straight into the result: no
// merge, any k".  A longer list is refused (VF_EUNSUPPORTED, naming the list and its length) and the Python layer routes it to the
// one-list call: the super-chunks, parts and merge buffers of vf_subset.h stay OUT of this mode on purpose.
//
// A PASS is at most pass_queries (256) consecutive queries of the call.  Inside a pass the queries are PERMUTED: grouped by list (stable
// in query order), the lists ordered by SIZE CLASS and then by their number.  A size class c is the row count n_rank(c) the ranking
// launch gives every query of the class: the smallest class bound >= m of the query's list.  The bounds -- 256 / 2048 / 8192 / 16 384 --
// are the issue's figures, NOT measured (no GPU timing exists for any other choice; tools/bench_subset_multi.py is the place to try one).
// A TILE is up to q_tile (4) consecutive queries of the permuted order that share one list: the tiles of a pass number the sum over its
// lists of ceil(queries of that list / q_tile).  Scores are query-major in permuted order: the queries of a class are contiguous, query
// p of class c owns n_rank(c) floats, so ONE launch_sort_rows(scores_c, n_rank, queries_c, n_rank, k, ...) ranks a whole class.
// The scan writes the SENTINEL -FLT_MAX at the positions [m, n_rank) of a query: every slot the ranking reads is written exactly once.
// Sentinels carry the highest positions of their row, so after ranking they come behind every real position (ties go to the lower
// position); the final map strikes them BY POSITION (pos >= m), never by score.
// Launches per pass: one query prep, one scan and one ranking launch per class in use (at most 4 each), one map -- whatever the number
// of distinct lists (subm_max_launches).  Score workspace: at most pass_queries x 16 384 x 4 = 16 MB (subm_score_bytes_bound; asserted
// below for the real constants).
// No HIP header: the host compiler reads it as it stands.
#pragma once

#include <stdint.h>

#include "vf_subset.h"   // kSubsetQ, kSubsetRowsPerWg, kSubsetRankRows, kSubsetMaxBatch, subset_ceil_div, subset_bad_at

namespace vf {

constexpr int kSubmMaxClasses = 4;
constexpr long long kSubmScoreBytes = 16ll << 20;   // scores of one pass

struct SubmConfig {          // the blocking; a test shrinks it
    int rows_per_wg;         // positions one workgroup of the scan scores (kSubsetRowsPerWg)
    int q_tile;              // queries per tile (kSubsetQ)
    long long rank_rows;     // the longest list served: the largest class bound
    int n_classes;           // 1 .. kSubmMaxClasses
    long long class_rows[kSubmMaxClasses];   // ascending; class_rows[n_classes - 1] == rank_rows
    int pass_queries;        // queries per pass (kSubsetMaxBatch)
};

VF_HD SubmConfig subm_config_default() {
    SubmConfig c{};
    c.rows_per_wg = kSubsetRowsPerWg; c.q_tile = kSubsetQ; c.rank_rows = kSubsetRankRows; c.n_classes = 4;
    c.class_rows[0] = 256; c.class_rows[1] = 2048; c.class_rows[2] = 8192; c.class_rows[3] = kSubsetRankRows;   // the issue's figures, not measured
    c.pass_queries = kSubsetMaxBatch;
    return c;
}
static_assert((long long)kSubsetMaxBatch * kSubsetRankRows * 4 == kSubmScoreBytes, "256 queries of the largest class are 16 MB of scores");

VF_HD bool subm_config_ok(const SubmConfig& c) {
    if (c.rows_per_wg < 1 || c.q_tile < 1 || c.q_tile > kSubsetQ || c.pass_queries < 1 || c.n_classes < 1 || c.n_classes > kSubmMaxClasses) return false;
    for (int i = 0; i < c.n_classes; ++i)
        if (c.class_rows[i] < 1 || (i > 0 && c.class_rows[i] <= c.class_rows[i - 1])) return false;
    return c.class_rows[c.n_classes - 1] == c.rank_rows && c.rank_rows <= kSubsetRankRows;
}

// the class of a list of m ids (m <= rank_rows): the first whose bound holds it
VF_HD int subm_class_of(const SubmConfig& c, long long m) {
    int k = 0;
    while (k < c.n_classes - 1 && c.class_rows[k] < m) ++k;
    return k;
}

// ---- the descriptors (uploaded as they stand) ------------------------------------------------------------------------------------
struct SubmTile {            // one per tile: k_scan_subset_m's blockIdx.y picks it
    const long long* ids;    // the tile's list (device; null when m == 0: never read then)
    long long m;             // its length
    long long score_base;    // float index of the score row of the tile's first query; query slot s owns [score_base + s * n_rank, + n_rank)
    int q[kSubsetQ];         // the pass-local caller-order indexes of the tile's queries (rows of qn); -1: absent
    int p0;                  // the tile's first permuted query
    int n_rank;              // the class's row count
    int pad[4];
};
static_assert(sizeof(SubmTile) == 64, "the tile table is uploaded as it stands");

struct SubmQuery {           // one per permuted query: k_subset_ids_m's blockIdx.y picks it
    const long long* ids;    // its list
    long long m;
    long long row;           // the caller's row of the CALL (not of the pass): where the result goes
};
static_assert(sizeof(SubmQuery) == 24, "the query table is uploaded as it stands");

struct SubmList {            // one per referenced list: k_subset_check_m's blockIdx.y picks it
    const long long* ids;
    long long m;
    long long list;          // its number in the caller's table: the high word of the check key
};
static_assert(sizeof(SubmList) == 24, "the list table is uploaded as it stands");

// the check word: the lowest (list, position) a list may not hold; ~0 = every list is good
VF_HD unsigned long long subm_check_key(long long list, long long pos) { return ((unsigned long long)list << 32) | (unsigned long long)pos; }
VF_HD long long subm_check_list(unsigned long long key) { return (long long)(key >> 32); }
VF_HD long long subm_check_pos(unsigned long long key) { return (long long)(key & 0xFFFFFFFFull); }

// ---- the call ----------------------------------------------------------------------------------------------------------------------
enum SubmVerdict { kSubmOk = 0, kSubmBadConfig = 1, kSubmBadListOf = 2, kSubmNegativeLength = 3, kSubmTooLong = 4 };

struct SubmCall {
    int verdict;             // SubmVerdict
    long long at;            // kSubmBadListOf: the query; kSubmNegativeLength / kSubmTooLong: the list
    long long value;         // the offending list_of entry, or length
    int passes;              // ceil(nq / pass_queries)
    long long rows;          // sum over the queries of their list's length (vf_search_stats.subset_rows)
};

// Refusals come in the order: list_of out of range (lowest query), then a referenced list of negative length or longer than rank_rows
// (lowest query that uses one).  Lists no query names are not looked at.
VF_HD SubmCall subm_call(int nq, const int32_t* list_of, int n_lists, const long long* m, const SubmConfig& c) {
    SubmCall r{};
    if (!subm_config_ok(c) || nq < 0 || n_lists < 0) { r.verdict = kSubmBadConfig; return r; }
    for (int q = 0; q < nq; ++q)
        if (list_of[q] < 0 || list_of[q] >= n_lists) { r.verdict = kSubmBadListOf; r.at = q; r.value = list_of[q]; return r; }
    for (int q = 0; q < nq; ++q) {
        const long long len = m[list_of[q]];
        if (len < 0) { r.verdict = kSubmNegativeLength; r.at = list_of[q]; r.value = len; return r; }
        if (len > c.rank_rows) { r.verdict = kSubmTooLong; r.at = list_of[q]; r.value = len; return r; }
        r.rows += len;
    }
    r.passes = (int)subset_ceil_div(nq, c.pass_queries);
    return r;
}

// ---- a pass ------------------------------------------------------------------------------------------------------------------------
struct SubmPass {
    int q0, nb;                              // the queries [q0, q0 + nb) of the call
    int n_tiles;
    int class_queries[kSubmMaxClasses];      // queries of the class ...
    int class_first[kSubmMaxClasses];        // ... the first of them in permuted order ...
    int class_tiles[kSubmMaxClasses];        // ... their tiles and the first of those
    int class_tile0[kSubmMaxClasses];
    long long class_base[kSubmMaxClasses];   // float index of the class's first score row
    long long score_floats;                  // the pass's scores: sum of class_queries * class_rows
    int launches;                            // prep + a scan and a ranking per class in use + map
};

VF_HD int subm_max_launches(const SubmConfig& c) { return 2 + 2 * c.n_classes; }
VF_HD long long subm_score_bytes_bound(const SubmConfig& c) { return 4ll * c.pass_queries * c.rank_rows; }
VF_HD long long subm_pass_tiles_bound(int nb) { return nb; }   // a tile holds at least one query

// Build pass `pass` of a call subm_call accepted.  perm [nb]: permuted order -> pass-local query; tiles [nb], qd [nb]: the two tables (the
// first n_tiles / nb entries are written).  list_ptr [n_lists]: where each list lies as the kernels will see it (may be null: the
// tables then hold null pointers, as the host test's do).
VF_HD SubmPass subm_build_pass(int pass, int nq, const int32_t* list_of, const long long* m, const long long* const* list_ptr, const SubmConfig& c,
                               int* perm, SubmTile* tiles, SubmQuery* qd) {
    SubmPass p{};
    p.q0 = pass * c.pass_queries;
    p.nb = nq - p.q0 < c.pass_queries ? nq - p.q0 : c.pass_queries;
    const int32_t* lo = list_of + p.q0;
    // stable insertion sort by (class, list): nb <= pass_queries, so at most a few thousand steps
    for (int i = 0; i < p.nb; ++i) {
        const int ci = subm_class_of(c, m[lo[i]]);
        int j = i;
        while (j > 0) {
            const int o = perm[j - 1], co = subm_class_of(c, m[lo[o]]);
            if (co < ci || (co == ci && lo[o] <= lo[i])) break;
            perm[j] = o;
            --j;
        }
        perm[j] = i;
    }
    for (int k = 0; k < kSubmMaxClasses; ++k) p.class_first[k] = p.class_tile0[k] = -1;
    long long base = 0;
    int t = -1;   // the open tile
    for (int pp = 0; pp < p.nb; ++pp) {
        const int q = perm[pp], list = lo[q], cls = subm_class_of(c, m[list]);
        const long long n_rank = c.class_rows[cls];
        if (p.class_first[cls] < 0) { p.class_first[cls] = pp; p.class_base[cls] = base; }
        const bool same = pp > 0 && lo[perm[pp - 1]] == list;
        int slot = same ? pp - tiles[t].p0 : 0;
        if (!same || slot >= c.q_tile) {   // a new tile
            ++t;
            slot = 0;
            SubmTile& T = tiles[t];
            T.ids = list_ptr ? list_ptr[list] : nullptr; T.m = m[list]; T.score_base = base; T.p0 = pp; T.n_rank = (int)n_rank;
            for (int s = 0; s < kSubsetQ; ++s) T.q[s] = -1;
            for (int s = 0; s < 4; ++s) T.pad[s] = 0;
            if (p.class_tile0[cls] < 0) p.class_tile0[cls] = t;
            ++p.class_tiles[cls];
        }
        tiles[t].q[slot] = q;
        qd[pp].ids = list_ptr ? list_ptr[list] : nullptr; qd[pp].m = m[list]; qd[pp].row = p.q0 + q;
        ++p.class_queries[cls];
        base += n_rank;
    }
    p.n_tiles = t + 1;
    p.score_floats = base;
    p.launches = 2;
    for (int k = 0; k < c.n_classes; ++k)
        if (p.class_queries[k] > 0) p.launches += 2;
    return p;
}

// ---- what a workgroup of k_scan_subset_m does ------------------------------------------------------------------------------------
// Workgroup bx of a tile owns the positions [bx * rows_per_wg, + rows_per_wg).  Past n_rank it returns at once; wholly inside
// [m, n_rank) it writes sentinels alone; otherwise it scores the positions < m and writes sentinels at the others below n_rank.
enum SubmWg { kSubmWgNothing = 0, kSubmWgSentinels = 1, kSubmWgScan = 2 };
VF_HD int subm_wg_kind(long long m, long long n_rank, long long bx, int rows_per_wg) {
    const long long first = bx * rows_per_wg;
    if (first >= n_rank) return kSubmWgNothing;
    return first >= m ? kSubmWgSentinels : kSubmWgScan;
}
VF_HD long long subm_scan_blocks(long long n_rank, int rows_per_wg) { return subset_ceil_div(n_rank, rows_per_wg); }
// where query slot s of a tile keeps the score of position pos
VF_HD long long subm_score_index(const SubmTile& t, int s, long long pos) { return t.score_base + (long long)s * t.n_rank + pos; }

}  // namespace vf
