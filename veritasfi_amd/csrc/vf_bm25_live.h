// vf_bm25_live.h -- the index arithmetic of a live BM25 update (vf_bm25_create with VF_BM25_LIVE: documents leave, later rows move down,
// new documents are appended, every posting is re-scored), as plain functions the kernels (k_bm25_live_*, vf_sparse.hip) and a
// host-compiled test (tests/test_bm25_live_plan.py: every subset of 12 rows, chunk sizes 1, 4 and > nnz) share.
//
// The index is CSC: column c (a token) holds the postings [indptr[c], indptr[c + 1]) of the flat arrays, rows strictly ascending.
// An update writes a second set of arrays.  Of the old postings those whose row stays survive, in their order; S(p) is the number of
// survivors below flat position p.  The new documents' postings come as a delta CSC over Vn >= V columns (dptr, local rows, tf).
//   new start of column c      newptr[c] = S(start(c)) + dptr[c]            start(c) = indptr[c] for c <= V, nnz for the new columns
//   a survivor at p, column c  goes to S(p) + dptr[c]                       (= newptr[c] + its rank among the column's survivors)
//   delta posting q, column c  goes to newptr[c + 1] - dptr[c + 1] + q      (behind the column's survivors, in delta order)
// The flat array is cut into chunks of C postings, one workgroup each, so that a column holding a posting of nearly every document
// and ten thousand columns of one posting cost the same per posting.  A chunk recovers its postings' columns from the column that
// holds its first posting (a binary search) and the column starts inside it (marked, then a running maximum: of several columns that
// share a start only the last is not empty).  A chunk OWNS the column starts in [lo, hi); the last chunk also owns those at nnz (the
// trailing empty columns, the end sentinel and every new column), and with nnz == 0 there is one empty chunk that owns them all.
// 64-bit positions throughout; rows are int32 (n_docs < 2^31).  No HIP header: the host compiler reads it as it stands.
#pragma once

#include "vf_scan_lds.h"   // VF_HD

namespace vf {

constexpr int kLiveMaxChunk = 2048;   // postings per chunk: the default, and the most the kernels' LDS arrays hold

// the new row of old row r, or -1 when it leaves; rem[0] < rem[1] < ... < rem[m - 1] are the rows that leave
VF_HD long long live_new_row(long long r, const int* rem, long long m) {
    long long lo = 0, hi = m;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (rem[mid] < r) lo = mid + 1; else hi = mid;
    }
    return (lo < m && rem[lo] == r) ? -1 : r - lo;
}

// old start of column c of the new vocabulary, c in [0, Vn]
VF_HD long long live_old_start(const long long* indptr, long long V, long long nnz, long long c) { return c <= V ? indptr[c] : nnz; }

VF_HD long long live_chunks(long long nnz, long long C) {
    const long long k = (nnz + C - 1) / C;
    return k < 1 ? 1 : k;
}
struct LiveChunk { long long lo, hi; bool last; };   // flat positions [lo, hi)
VF_HD LiveChunk live_chunk(long long nnz, long long C, long long k) {
    LiveChunk ch;
    ch.lo = k * C < nnz ? k * C : nnz;
    ch.hi = ch.lo + C < nnz ? ch.lo + C : nnz;
    ch.last = k + 1 >= live_chunks(nnz, C);
    return ch;
}

// the first column in [0, Vn + 1] whose old start is >= p (Vn + 1: none)
VF_HD long long live_col_lower(const long long* indptr, long long V, long long Vn, long long nnz, long long p) {
    long long lo = 0, hi = Vn + 1;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (live_old_start(indptr, V, nnz, mid) < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// the column that holds flat position p < nnz: the last one whose old start is <= p
VF_HD long long live_col_of(const long long* indptr, long long V, long long Vn, long long nnz, long long p) {
    return live_col_lower(indptr, V, Vn, nnz, p + 1) - 1;
}
// the columns whose start a chunk owns: [first, end)
VF_HD long long live_owned_first(const long long* indptr, long long V, long long Vn, long long nnz, const LiveChunk& ch) {
    return live_col_lower(indptr, V, Vn, nnz, ch.lo);
}
VF_HD long long live_owned_end(const long long* indptr, long long V, long long Vn, long long nnz, const LiveChunk& ch) {
    return ch.last ? Vn + 1 : live_col_lower(indptr, V, Vn, nnz, ch.hi);
}

VF_HD long long live_dest(long long survivors_below, long long dptr_c) { return survivors_below + dptr_c; }
VF_HD long long live_delta_dest(long long newptr_c1, long long dptr_c1, long long q) { return newptr_c1 - dptr_c1 + q; }

// bm25_index_arrays' score of one posting: float64 in numpy's operation order, nothing contracted, rounded once to float32.
// idf comes from the host (numpy's log); one_minus_b = 1.0 - b.
VF_HD float live_score(double idf, int tf, int dl, double avgdl, double k1, double b, double one_minus_b) {
    const double t = (double)tf;
#if defined(__HIP_DEVICE_COMPILE__)
    const double len = __dadd_rn(one_minus_b, __ddiv_rn(__dmul_rn(b, (double)dl), avgdl));
    return (float)__ddiv_rn(__dmul_rn(idf, t), __dadd_rn(t, __dmul_rn(k1, len)));
#else
    volatile double bd = b * (double)dl;            // volatile: the host compiler forms no fused multiply-add across these
    volatile double len = one_minus_b + bd / avgdl;
    volatile double kl = k1 * len;
    volatile double num = idf * t;
    return (float)(num / (t + kl));
#endif
}

}  // namespace vf
