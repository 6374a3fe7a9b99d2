// vf_bm25_filter.h -- the word arithmetic of a BM25 search restricted to a chosen set of rows (vf_bm25_search with VF_BM25_FILTER: the
// filtered forms k_bm25_accum_f, k_bm25_tail_count_f, k_bm25_tail_write_f and the padding k_bm25_pad_out, vf_sparse.hip), as plain
// functions the kernels, the entry point and a host-compiled test (tests/test_bm25_filter_plan.py: UBSan, every filter and every
// touched set of up to 12 rows, then word and block boundaries) share.
//
// The filter is a bitmap `allow` of the n rows: bit (r & 31) of word r >> 5 set = row r may be returned.  Scores keep the whole
// corpus's statistics; the result is the unfiltered canonical ranking with the rows outside the set struck out:
//   the scatter   skips a posting whose row is out (bm25f_row_allowed), so the touched bitmap holds allowed rows only and the select,
//                 gather and sort kernels run unchanged over "allowed and touched";
//   the tail      (score 0, ascending rows) takes the bits ~touched & valid & allow of each word (bm25f_allowed_untouched).  Allowed
//                 untouched rows can lie in ANY bitmap block, so a filtered call counts, scans and writes the tail over all
//                 words / kBm25FilterBlockWords blocks at every k -- the unfiltered small-k call looks at block 0 alone;
//   the padding   with m rows allowed, ranks min(k, m) .. k - 1 are (-1, -FLT_MAX), the dense leg's convention.
// Rows are below 2^31 (vf_bm25_create), words are 32 bits.  No HIP header: the host compiler reads it as it stands.
#pragma once

#include <stdint.h>

#include "vf_scan_lds.h"   // VF_HD

namespace vf {

constexpr int kBm25FilterBlockWords = 1024;   // bitmap words one workgroup of the tail kernels takes (= kBmWordsPerBlock, vf_sparse.hip)

// the bits of the word whose first row is r0 that name rows below n
VF_HD uint32_t bm25f_valid_mask(long long r0, long long n) {
    return r0 >= n ? 0u : (n - r0 >= 32 ? 0xFFFFFFFFu : ((1u << (uint32_t)(n - r0)) - 1u));
}

// rows of a word that belong to the zero-score tail: allowed, below n, without a posting of the query
VF_HD uint32_t bm25f_allowed_untouched(uint32_t touched, uint32_t valid, uint32_t allow) { return ~touched & valid & allow; }

VF_HD bool bm25f_row_allowed(const uint32_t* allow, uint32_t row) { return (allow[row >> 5] >> (row & 31u)) & 1u; }

// words of a caller's bitmap over n rows
VF_HD long long bm25f_words(long long n) { return (n + 31) / 32; }

struct Bm25FilterCheck {
    long long bad_row;   // the first row at or past n whose bit is set (it can only lie in the last word), or -1
    long long m;         // rows allowed (bits set below n)
};

VF_HD int bm25f_popcount(uint32_t w) {
    w = w - ((w >> 1) & 0x55555555u);
    w = (w & 0x33333333u) + ((w >> 2) & 0x33333333u);
    return (int)((((w + (w >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24);
}

// what the entry point checks of allow[bm25f_words(n)] before any device work
VF_HD Bm25FilterCheck bm25f_check(const uint32_t* allow, long long n) {
    Bm25FilterCheck c{-1, 0};
    const long long words = bm25f_words(n);
    for (long long w = 0; w < words; ++w) {
        const uint32_t valid = bm25f_valid_mask(w * 32, n), over = allow[w] & ~valid;
        if (over && c.bad_row < 0) {
            int b = 0;
            while (!((over >> b) & 1u)) ++b;
            c.bad_row = w * 32 + b;
        }
        c.m += bm25f_popcount(allow[w] & valid);
    }
    return c;
}

struct Bm25FilterPlan {
    int tail_blocks;          // grid.x of the tail's count and write, and the blocks its scan runs over: every block of the bitmap
    long long tblk_entries;   // tblk entries per slot (= tail_blocks): the unfiltered small-k call holds one
    long long pad_from;       // first padded rank; k when there is no padding
};

// words: the handle's bitmap words per slot (a multiple of kBm25FilterBlockWords); m: rows allowed.  Whatever the query touches, the
// sort writes min(k, touched) ranks (touched counts allowed rows only, so touched <= m), the tail fills up to min(k, m) with the
// m - touched allowed untouched rows, and nothing but padding follows: where it starts does not depend on the query.
VF_HD Bm25FilterPlan bm25f_plan(long long words, long long m, long long k) {
    Bm25FilterPlan p{};
    p.tail_blocks = (int)(words / kBm25FilterBlockWords);
    p.tblk_entries = p.tail_blocks;
    p.pad_from = m < k ? m : k;
    return p;
}

}  // namespace vf
