// vf_bm25_substats.h -- the index arithmetic of a filtered BM25 search scored by the SUBSET's own statistics (vf_bm25_search with
// VF_BM25_FILTER | VF_BM25_SUBSTATS: the counting kernels k_bm25_sub_len and k_bm25_sub_df and the scatter k_bm25_accum_s,
// vf_sparse.hip), as plain functions the kernels, the entry point and a host-compiled test (tests/test_bm25_substats_plan.py: UBSan,
// every filter of a 12-row index, then word and block boundaries) share.
//
// With m rows allowed, the result is what an index built from the allowed documents alone would return: N_s = m, df_s[c] = the
// postings of column c whose row is allowed, avgdl_s = (sum of the allowed rows' lengths) / m.  A request is two calls with the
// caller's logarithm between them (the library takes none):
//   the stage    counts.  The length sum walks the filter's bitmap in blocks of kBm25FilterBlockWords words, four words per thread
//                (bm25s_word_len); it is a sum of integers in 64 bits, so no launch order can change it.  The df count runs once per
//                DISTINCT column of the batch (bm25s_dedupe: a token two queries share, or one query repeats, is counted once):
//                workgroup (x, d) takes the postings p0 + x * T + i * gx * T + tid of column d (bm25s_df_plan, bm25s_df_base); a
//                wave counts by ballot, a workgroup adds once.  The counts go back per q_terms position through the dedupe map.
//   the search   scores a posting on the fly, live_score(idf[position], tf, doclen[row], avgdl, ...) of vf_bm25_live.h, where the
//                corpus mode reads the stored score; everything behind the scatter is the filtered call's.
// 64-bit positions throughout; rows are int32 (n_docs < 2^31), a column's count fits int32.  No HIP header: the host compiler reads
// it as it stands.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "vf_bm25_filter.h"

namespace vf {

constexpr int kBm25SubThreads = 256;          // threads of both counting kernels (= kBmThreads, vf_sparse.hip)
constexpr int kBm25SubWordsPerThread = 4;     // bitmap words a thread of the length sum takes: 256 * 4 = kBm25FilterBlockWords
constexpr int kBm25SubPostingsPerThread = 8;  // postings a thread of the df count takes before the grid is widened
constexpr int kBm25SubMaxChunks = 2048;       // most workgroups along a column
static_assert(kBm25SubThreads * kBm25SubWordsPerThread == kBm25FilterBlockWords, "the length sum walks the filter's bitmap blocks");

// ---- the distinct columns of a batch ---------------------------------------------------------------------------------------------
// distinct: the columns of q_terms[0 .. T) ascending, each once; pos2d[t]: where q_terms[t] stands in it.  Returns their number.
inline long long bm25s_dedupe(const int32_t* q_terms, long long T, std::vector<int32_t>& distinct, std::vector<int32_t>& pos2d) {
    distinct.assign(q_terms, q_terms + T);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    pos2d.resize((size_t)T);
    for (long long t = 0; t < T; ++t)
        pos2d[(size_t)t] = (int32_t)(std::lower_bound(distinct.begin(), distinct.end(), q_terms[t]) - distinct.begin());
    return (long long)distinct.size();
}

// ---- the df launch ---------------------------------------------------------------------------------------------------------------
// grid.x for columns of at most p postings: one chunk of kBm25SubThreads * kBm25SubPostingsPerThread postings per workgroup, at least
// one workgroup, at most kBm25SubMaxChunks (a longer column is walked in strides of the whole grid)
VF_HD unsigned bm25s_df_plan(long long p) {
    const long long per = (long long)kBm25SubThreads * kBm25SubPostingsPerThread;
    const long long g = (p + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : (g > kBm25SubMaxChunks ? kBm25SubMaxChunks : g));
}
// the first posting of workgroup x's i-th step over a column that starts at p0 (thread tid takes base + tid while below the end)
VF_HD long long bm25s_df_base(long long p0, unsigned x, unsigned gx, long long i) {
    return p0 + ((long long)x + i * (long long)gx) * kBm25SubThreads;
}

// ---- the length sum --------------------------------------------------------------------------------------------------------------
// the lengths of the allowed rows of the word whose first row is r0 (bits at or past n never count)
VF_HD unsigned long long bm25s_word_len(uint32_t allow_word, long long r0, long long n, const int* doclen) {
    unsigned long long s = 0;
    for (uint32_t m = allow_word & bm25f_valid_mask(r0, n); m; m &= m - 1) s += (unsigned long long)doclen[r0 + __builtin_ctz(m)];
    return s;
}
// the first word of thread tid of bitmap block b
VF_HD long long bm25s_len_word0(long long b, int tid) { return b * kBm25FilterBlockWords + (long long)tid * kBm25SubWordsPerThread; }

// ---- both counts on the CPU, launch for launch -------------------------------------------------------------------------------------
// allow: the device bitmap, `words` words (a multiple of kBm25FilterBlockWords), zero past the caller's
inline unsigned long long bm25s_cpu_len(const uint32_t* allow, long long words, long long n, const int* doclen) {
    unsigned long long total = 0;
    for (long long b = 0; b < words / kBm25FilterBlockWords; ++b) {
        unsigned long long block = 0;                       // one atomic per workgroup
        for (int tid = 0; tid < kBm25SubThreads; ++tid) {
            const long long w0 = bm25s_len_word0(b, tid);
            for (int j = 0; j < kBm25SubWordsPerThread; ++j) block += bm25s_word_len(allow[w0 + j], (w0 + j) * 32, n, doclen);
        }
        total += block;
    }
    return total;
}
// df[d] for the D distinct columns; `seen` (nnz entries, zero on entry, or null) counts how often each posting was looked at
inline void bm25s_cpu_df(const long long* indptr, const int* indices, const uint32_t* allow, const int32_t* distinct, long long D,
                         int32_t* df, int* seen) {
    long long most = 0;
    for (long long d = 0; d < D; ++d) most = std::max(most, indptr[distinct[d] + 1] - indptr[distinct[d]]);
    const unsigned gx = bm25s_df_plan(most);
    for (long long d = 0; d < D; ++d) {
        const long long p0 = indptr[distinct[d]], p1 = indptr[distinct[d] + 1];
        int32_t cnt = 0;
        for (unsigned x = 0; x < gx; ++x)
            for (long long i = 0; bm25s_df_base(p0, x, gx, i) < p1; ++i)
                for (int tid = 0; tid < kBm25SubThreads; ++tid) {
                    const long long p = bm25s_df_base(p0, x, gx, i) + tid;
                    if (p >= p1) break;
                    if (seen) ++seen[p];
                    cnt += bm25f_row_allowed(allow, (uint32_t)indices[p]);
                }
        df[d] = cnt;
    }
}

}  // namespace vf
