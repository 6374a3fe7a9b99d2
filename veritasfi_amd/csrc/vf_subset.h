// vf_subset.h -- the plan of a search restricted to a chosen subset of rows (vf_index_search / _device with VF_SEARCH_SUBSET: k_scan_subset, then the ranking
// and merge kernels of the exact path), as plain functions the kernel (vf_kernels.hip), its host side (vf_api.hip) and a
// host-compiled test (tests/test_subset_plan.py: UBSan, every subset of up to 12 rows at every chunk size) share.
//
// The caller names m rows of the n the index holds: sel[0] < sel[1] < ... < sel[m - 1].  A POSITION is an index into sel.  The m
// positions are scored in SUPER-CHUNKS of at most super_rows positions per k_scan_subset launch, so that the score workspace
// stays within kSubsetScoreBytes whatever m is.  A super-chunk is ranked in RANK CHUNKS of at most rank_rows (16 384) positions; the
// k best positions of a chunk are a PART.  The kernel writes the scores chunk-major -- [chunk][query][rank_rows], subset_score_index --
// so that ONE launch_sort_rows ranks every whole chunk of a super-chunk (a "query" of that launch is a (chunk, query) pair; the short
// last chunk takes a second launch) and its output [chunk][query][k] is the part array the merge reads.  The parts of a super-chunk
// follow the running result in one buffer -- slot 0 the running result (all padding at first), slots 1 .. the parts in ascending
// position order -- and are folded in by launch_merge_topk, fan_in slots at a time: the result of a merge is copied over the last
// slot it consumed, which is the first slot of the next merge.  The merge breaks ties towards the earlier slot and the earlier rank,
// positions ascend with the rows they name, so "ties to the lower id" holds through every round.  After the last merge one kernel
// maps positions to ids through sel.  A list of one part (m <= rank_rows) is ranked straight into the result: no merge, any k.
// 64-bit arithmetic throughout (a shard holds up to 2^32 - 2 rows).  No HIP header: the host compiler reads it as it stands.
#pragma once

#include "vf_scan_lds.h"   // VF_HD, kSmallN

namespace vf {

// ---- k_scan_subset's blocking ------------------------------------------------------------------------------------
// A row is scored by a PAIR of lanes (lane half h holds the canonical partial sums 8h .. 8h + 7, as k_final's re-score does), a pair
// takes kSubsetR rows against kSubsetQ queries at once: every query value read from LDS feeds kSubsetR multiply-adds, every row value
// read from HBM kSubsetQ of them.  One wave per workgroup: 32 pairs x kSubsetR rows.
constexpr int kSubsetR = 2;             // rows per lane pair
constexpr int kSubsetQ = 4;             // queries per pass over the rows (the LDS query tile)
constexpr int kSubsetThreads = 64;
constexpr int kSubsetRowsPerWg = (kSubsetThreads / 2) * kSubsetR;
constexpr int kSubsetSlice = 1024;      // elements of a query the LDS holds at a time (a K-slice; a multiple of 16)
constexpr int kSubsetMaxD = 8192;       // the widest row the plan is checked for (the index itself sets the width)

// ---- the workspace -----------------------------------------------------------------------------------------------------------------
// 64 MB of scores per launch: the figure of the issue, NOT measured (no GPU timing exists for any other size; tools/bench_subset_search.py
// takes --super-rows to try one).  At 1 query that is 16.7M positions per launch, at 256 queries 65 536 -- fewer where the PARTS of that
// many rank chunks (12 bytes x queries x k each) would pass 64 MB themselves.  The record with it (round 16, profiles/r16_subset_search.log,
// 1M x 768 fp16, every list in one super-chunk): 500 000 rows, k = 100: 0.56 ms at 1 query, 0.61 at 4, 4.2 at 64.
constexpr long long kSubsetScoreBytes = 64ll << 20;
constexpr int kSubsetMaxBatch = 256;                 // queries per pass: bounds the merge buffer below
constexpr long long kSubsetRankRows = kSmallN;       // positions one launch_sort_rows ranks (its LDS holds that many keys)
constexpr int kSubsetMergeKeys = 16384;              // keys k_merge_topk sorts in LDS per query: next_pow2(fan_in * k) <= this
constexpr int kSubsetMaxK = 8192;                    // k beyond one rank chunk: two parts must fit a merge (the exact path's own limit)
constexpr long long kSubsetMaxRows = 0xFFFFFFFEll;   // rows of the largest shard, so the longest list

enum SubsetRoute {
    kSubsetEmpty = 0,     // m == 0: every result is (-1, -FLT_MAX), nothing is launched but the fill
    kSubsetAll = 1,       // m == n: the ordinary search, unchanged (exact: scores are canonical)
    kSubsetScan = 2,      // k_scan_subset
    kSubsetRefused = -1
};

struct SubsetPlan {
    int route;
    const char* why;        // route == kSubsetRefused: the limit that was hit
    int batch;              // queries per pass (<= kSubsetMaxBatch)
    long long super_rows;   // positions per k_scan_subset launch: the row stride of the score workspace (>= 1)
    long long supers;       // launches per pass
    long long rank_rows;    // positions per part
    long long parts;        // parts per pass, over all super-chunks
    long long super_parts;  // parts of a whole super-chunk: the part slots of the buffer, beside the running result's
    int fan_in;             // slots one merge takes: the running result and fan_in - 1 parts (0: a single part goes straight to the output)
    long long rounds;       // merges per pass
    int q_tile, slice, lds_bytes, rows_per_wg;   // the kernel's blocking: LDS = q_tile * slice * 4 bytes, whatever d is
    long long score_bytes, merge_bytes;          // the workspace: scores; running result + part slots + merge output
};

VF_HD long long subset_ceil_div(long long a, long long b) { return (a + b - 1) / b; }
VF_HD int subset_next_pow2(long long v) { int p = 1; while (p < v) p <<= 1; return p; }

// slots a merge of lists of k may take: the most whose keys k_merge_topk's LDS sort holds (0: not even two)
VF_HD int subset_fan_in(int k) {
    int f = 0;
    for (int c = 2; c <= 16 && subset_next_pow2((long long)c * k) <= kSubsetMergeKeys; ++c) f = c;
    return f;
}

// merges that fold the `parts` parts of one super-chunk into the running result, fan_in - 1 of them at a time
VF_HD long long subset_rounds(long long parts, int fan_in) { return fan_in < 2 ? 0 : subset_ceil_div(parts, fan_in - 1); }

// where the kernel writes the score of query q (of nq) at position i of a super-chunk: chunk-major, so that every chunk's scores of
// every query are rows of one [chunks * nq][rank_rows] matrix
VF_HD long long subset_score_index(long long i, int q, int nq, long long rank_rows) {
    return ((i / rank_rows) * nq + q) * rank_rows + i % rank_rows;
}

// super_rows_opt / rank_rows_opt: 0 = auto; tests and the bench lower them (rank_rows_opt at most kSubsetRankRows)
VF_HD SubsetPlan subset_plan(long long n, long long m, int nq, int k, long long super_rows_opt, long long rank_rows_opt) {
    SubsetPlan p{};
    p.q_tile = kSubsetQ; p.slice = kSubsetSlice; p.lds_bytes = kSubsetQ * kSubsetSlice * 4; p.rows_per_wg = kSubsetRowsPerWg;
    p.route = kSubsetRefused;
    if (n < 0 || m < 0 || m > n || nq < 0 || k < 0) { p.why = "negative size, or more ids than rows"; return p; }
    if (m > kSubsetMaxRows) { p.why = "more than 2^32 - 2 ids"; return p; }
    p.why = nullptr;
    if (m == 0) { p.route = kSubsetEmpty; return p; }
    if (m == n) { p.route = kSubsetAll; return p; }
    p.rank_rows = rank_rows_opt > 0 && rank_rows_opt < kSubsetRankRows ? rank_rows_opt : kSubsetRankRows;
    p.batch = nq < kSubsetMaxBatch ? (nq < 1 ? 1 : nq) : kSubsetMaxBatch;
    // every super-chunk but the last holds whole rank chunks, so the parts are the rank chunks of the list
    p.parts = subset_ceil_div(m, p.rank_rows);
    if (p.parts > 1) {
        p.fan_in = subset_fan_in(k);
        if (k > kSubsetMaxK || p.fan_in < 2) { p.route = kSubsetRefused; p.why = "k <= 8192 when more than 16384 ids are given"; return p; }
    }
    long long chunks = kSubsetScoreBytes / (4ll * p.batch * p.rank_rows);                     // rank chunks whose scores 64 MB hold (>= 4) ...
    const long long by_parts = kSubsetScoreBytes / (12ll * p.batch * (k < 1 ? 1 : k));        // ... and whose parts 64 MB hold
    if (p.parts > 1 && by_parts < chunks) chunks = by_parts < 1 ? 1 : by_parts;
    if (super_rows_opt > 0 && subset_ceil_div(super_rows_opt, p.rank_rows) < chunks) chunks = subset_ceil_div(super_rows_opt, p.rank_rows);
    if (chunks > p.parts) chunks = p.parts;
    p.super_parts = chunks;
    p.super_rows = chunks * p.rank_rows < m ? chunks * p.rank_rows : m;
    p.supers = subset_ceil_div(m, p.super_rows);
    if (p.parts > 1) {
        if (p.fan_in > p.super_parts + 1) p.fan_in = (int)p.super_parts + 1;
        const long long last = p.parts - (p.supers - 1) * p.super_parts;                      // parts of the last super-chunk
        p.rounds = (p.supers - 1) * subset_rounds(p.super_parts, p.fan_in) + subset_rounds(last, p.fan_in);
        p.merge_bytes = (p.super_parts + 2) * p.batch * k * 12;
    }
    p.score_bytes = p.super_parts * p.rank_rows * p.batch * 4;
    p.route = kSubsetScan;
    return p;
}

struct SubsetSpan { long long lo, hi; };   // positions [lo, hi)

VF_HD SubsetSpan subset_super(const SubsetPlan& p, long long m, long long c) {
    SubsetSpan s;
    s.lo = c * p.super_rows;
    s.hi = s.lo + p.super_rows < m ? s.lo + p.super_rows : m;
    return s;
}
// rank chunks of a super-chunk, and the r-th of them
VF_HD long long subset_rank_chunks(const SubsetPlan& p, const SubsetSpan& sup) { return subset_ceil_div(sup.hi - sup.lo, p.rank_rows); }
VF_HD SubsetSpan subset_rank_chunk(const SubsetPlan& p, const SubsetSpan& sup, long long r) {
    SubsetSpan s;
    s.lo = sup.lo + r * p.rank_rows;
    s.hi = s.lo + p.rank_rows < sup.hi ? s.lo + p.rank_rows : sup.hi;
    return s;
}

// The first position of ids[0 .. m) that a list may not hold -- out of [lo, hi), or not above its predecessor (descending or a
// duplicate) -- or -1 when the list is good.  The host form runs it before any HIP call; k_subset_check is the same test per position.
VF_HD bool subset_bad_at(const long long* ids, long long i, long long lo, long long hi) {
    return ids[i] < lo || ids[i] >= hi || (i > 0 && ids[i] <= ids[i - 1]);
}
// the same test on values already read (k_subset_check_m reads its list through a global-address-space pointer)
VF_HD bool subset_bad_value(long long v, bool has_prev, long long prev, long long lo, long long hi) { return v < lo || v >= hi || (has_prev && v <= prev); }
VF_HD long long subset_first_bad(const long long* ids, long long m, long long lo, long long hi) {
    for (long long i = 0; i < m; ++i) if (subset_bad_at(ids, i, lo, hi)) return i;
    return -1;
}

}  // namespace vf
