// vf_bm25_prepared.h -- the index arithmetic of a PREPARED row filter's statistics (vf_bm25_search with VF_BM25_PREPARED: the counting
// kernel k_bm25_sub_df_all, vf_sparse.hip), as plain functions the kernel and a host-compiled test (tests/test_bm25_prepared_plan.py:
// UBSan, every filter of a 12-row index at chunk sizes 1, 2, 3, 5 and 2048, then word, block and chunk boundaries) share.
//
// A prepared filter in subset mode holds idf for EVERY column of the vocabulary, so its df is counted for every column at once:
// df_s[c] = the postings of column c whose row the bitmap allows.  One pass over the flat posting array, cut into chunks of C postings
// as a live update cuts it (vf_bm25_live.h: live_chunk), one workgroup each, whatever columns they belong to -- a column of a posting
// per document and ten thousand columns of one posting cost the same per posting.  A workgroup
//   flags     its chunk's postings (bm25f_row_allowed) and leaves the exclusive prefix of the flags in LDS: rank[i] = allowed postings
//             among the chunk's first i, rank[cnt] = all of them;
//   finds     the columns that intersect the chunk: from the one that holds the chunk's first posting (bm25p_first_col, a binary
//             search) up to, not including, the first that starts at or past the chunk's end (bm25p_end_col); thread t takes the
//             columns first + t, first + t + 256, ...;
//   counts    column c's part of the chunk as rank[hi] - rank[lo] over the span bm25p_span cuts out of it;
//   writes    a column that lies wholly inside the chunk with a plain store (it has no other writer), and ADDS the part of a column
//             that crosses a chunk boundary with one integer atomic per (column, chunk): integers, so any order is exact.
// An empty column is written by nobody and keeps the zero of the memset before the launch.  Every posting is flagged exactly once.
// 64-bit positions throughout; rows are int32 (n_docs < 2^31), a column's count fits int32.  No HIP header: the host compiler reads
// it as it stands.
#pragma once

#include <stdint.h>

#include <vector>

#include "vf_bm25_filter.h"
#include "vf_bm25_live.h"

namespace vf {

constexpr int kBm25PrepThreads = 256;   // threads of the counting kernel (= kBmThreads, vf_sparse.hip)

// the column that holds the chunk's first posting (the chunk is not empty: nnz > 0)
VF_HD long long bm25p_first_col(const long long* indptr, long long V, long long nnz, const LiveChunk& ch) {
    return live_col_of(indptr, V, V, nnz, ch.lo);
}
// the first column that starts at or past the chunk's end: <= V, since indptr[V] = nnz >= ch.hi
VF_HD long long bm25p_end_col(const long long* indptr, long long V, long long nnz, const LiveChunk& ch) {
    return live_col_lower(indptr, V, V, nnz, ch.hi);
}

struct Bm25pSpan {
    int lo, hi;    // the column's postings inside the chunk are the chunk's [lo, hi): its count there is rank[hi] - rank[lo]
    bool owned;    // the column lies wholly inside the chunk: a plain store; else its part is added
};
// p0, p1: the column's flat postings [p0, p1), with p0 < ch.hi and (the column being first_col or later) p1 > ch.lo or p0 == p1
VF_HD Bm25pSpan bm25p_span(long long p0, long long p1, const LiveChunk& ch) {
    Bm25pSpan s;
    const long long a = p0 > ch.lo ? p0 : ch.lo, b = p1 < ch.hi ? p1 : ch.hi;
    s.lo = (int)(a - ch.lo);
    s.hi = (int)((b > a ? b : a) - ch.lo);
    s.owned = p0 >= ch.lo && p1 <= ch.hi;
    return s;
}

// the segment [b0, b1) of a chunk of cnt entries whose flags thread t sums before the workgroup's scan (the live kernels' split)
VF_HD void bm25p_thread_segment(int cnt, int t, int* b0, int* b1) {
    const int L = (cnt + kBm25PrepThreads - 1) / kBm25PrepThreads;
    *b0 = t * L < cnt ? t * L : cnt;
    *b1 = *b0 + L < cnt ? *b0 + L : cnt;
}

// ---- the launch on the CPU, chunk by chunk and thread by thread ---------------------------------------------------------------------
// df[V] (written whole); allow: the device bitmap; seen (nnz entries, zero on entry, or null) counts how often each posting was flagged;
// stores / adds ([V], zero on entry, or null) count the plain stores and the atomic adds each column received
inline void bm25p_cpu_df_all(const long long* indptr, const int* indices, long long V, long long nnz, const uint32_t* allow, int C,
                             int32_t* df, int* seen, int* stores, int* adds) {
    for (long long c = 0; c < V; ++c) df[c] = 0;                       // the memset
    if (nnz == 0) return;                                              // no launch
    std::vector<int> rank((size_t)kLiveMaxChunk + 1), part((size_t)kBm25PrepThreads);
    const long long chunks = live_chunks(nnz, C);
    for (long long x = 0; x < chunks; ++x) {
        const LiveChunk ch = live_chunk(nnz, C, x);
        const int cnt = (int)(ch.hi - ch.lo);
        for (int t = 0; t < kBm25PrepThreads; ++t)
            for (int i = t; i < cnt; i += kBm25PrepThreads) {
                if (seen) ++seen[ch.lo + i];
                rank[(size_t)i] = bm25f_row_allowed(allow, (uint32_t)indices[ch.lo + i]);
            }
        for (int t = 0; t < kBm25PrepThreads; ++t) {                   // each thread's sum, then the scan over the threads
            int b0, b1, s = 0;
            bm25p_thread_segment(cnt, t, &b0, &b1);
            for (int i = b0; i < b1; ++i) s += rank[(size_t)i];
            part[(size_t)t] = s;
        }
        int run = 0;
        for (int t = 0; t < kBm25PrepThreads; ++t) {
            int b0, b1;
            bm25p_thread_segment(cnt, t, &b0, &b1);
            for (int i = b0; i < b1; ++i) {
                const int f = rank[(size_t)i];
                rank[(size_t)i] = run;
                run += f;
            }
        }
        rank[(size_t)cnt] = run;
        const long long c0 = bm25p_first_col(indptr, V, nnz, ch), c1 = bm25p_end_col(indptr, V, nnz, ch);
        for (int t = 0; t < kBm25PrepThreads; ++t)
            for (long long c = c0 + t; c < c1; c += kBm25PrepThreads) {
                const Bm25pSpan s = bm25p_span(indptr[c], indptr[c + 1], ch);
                const int d = rank[(size_t)s.hi] - rank[(size_t)s.lo];
                if (s.owned) {
                    if (s.hi > s.lo) {
                        df[c] = d;
                        if (stores) ++stores[c];
                    }
                } else if (d) {
                    df[c] += d;
                    if (adds) ++adds[c];
                }
            }
    }
}

}  // namespace vf
