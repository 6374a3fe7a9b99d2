// vf_bm25_multi.h -- a prepared row filter PER QUERY of a batch (vf_bm25_search with VF_BM25_PREPARED, phase VF_BM25_PREPARED_SEARCH and
// mode VF_BM25_PREPARED_PER_QUERY: the kernels k_bm25_accum_m, k_bm25_tail_count_m, k_bm25_tail_write_m and k_bm25_pad_out_m,
// vf_sparse.hip), as plain functions the kernels, the entry point and a host-compiled test (tests/test_bm25_multi_plan.py: UBSan, a
// two-slot group of a 12-row index under every filter, then the plan at the sizes where it changes) share.
//
// The rule: row i of such a batch is what the one-filter call returns for query i alone with filter i, ids and score bits; an entry
// without a filter is the unfiltered call.  A query owns a slot (its scores, touched bitmap, select state, output rows) and a prepared
// filter owns its bitmap and, in subset mode, its idf table, so all that differs between the slots of a group is WHICH filter the
// scatter, the tail and the padding read.  That is one Bm25Desc per query of the call, uploaded beside the query offsets and indexed by
// q0 + blockIdx.y: the same address for a whole workgroup, so its loads are scalar and the branch on it does not diverge.
//   the scatter   bm25m_form: no bitmap -> the stored score of every posting (k_bm25_accum); a bitmap and no idf table -> the stored
//                 score of the allowed postings (k_bm25_accum_f); both -> live_score from the posting's tf by the filter's idf, read per
//                 column (k_bm25_accum_sc).  One launch per token position, the same plain read-add-write: the fp32 order is the
//                 one-filter call's.
//   the tail      bm25m_tail_word: the filter's word, or all ones where there is no filter.  It runs over every bitmap block for every
//                 slot, as the filtered forms do; an unfiltered slot with fewer than k touched rows finds its tail in the first
//                 blocks and writes nothing past rank k, so it returns what its one-block form returns.
//   the padding   bm25m_pad_from: ranks min(m, k) .. k - 1 of a filtered slot, none of an unfiltered one; the grid of a group is sized
//                 by its longest span (bm25m_group_pad_span) and each slot starts at its own rank.
// A filter with m == 0 holds an all-zero bitmap: nothing is touched, the tail is empty and every rank is padding, without a special
// case.  Only a call in which NO query can return a row launches nothing.  No HIP header: the host compiler reads it as it stands.
#pragma once

#include <stdint.h>

#include "vf_bm25_filter.h"

namespace vf {

constexpr int kBm25mSmallK = 4096;   // = kBmSmallK, vf_sparse.hip: up to it one LDS sort per query and S queries per group

struct Bm25Desc {            // one per query of the call, on the device
    const uint32_t* allow;   // the filter's own bitmap [words], zero past n; null: every row may be returned
    const double* idf;       // subset mode: the filter's idf per column; null: the stored score of a posting is used
    double avgdl, k1, b, one_minus_b;   // subset mode: what live_score takes beside idf, tf and the document's length
    long long pad_from;      // first padded rank: min(m, k); k without a filter
    long long m;             // rows the filter allows (the host's plan; no kernel reads it)
};
static_assert(sizeof(Bm25Desc) == 64, "eight 8-byte members: the table is uploaded as it stands");

enum Bm25mForm { kBm25mPlain, kBm25mCorpus, kBm25mSubset };   // what k_bm25_accum, k_bm25_accum_f and k_bm25_accum_sc do

VF_HD Bm25mForm bm25m_form(const Bm25Desc& d) { return !d.allow ? kBm25mPlain : d.idf ? kBm25mSubset : kBm25mCorpus; }

// word w of the bitmap a slot's tail is cut by
VF_HD uint32_t bm25m_tail_word(const uint32_t* allow, long long w) { return allow ? allow[w] : 0xFFFFFFFFu; }

VF_HD long long bm25m_pad_from(bool filtered, long long m, long long k) { return filtered && m < k ? m : k; }

// the descriptor of a query without a filter, and of one whose prepared filter holds `allow` (and, in subset mode, `idf`) over m rows
VF_HD Bm25Desc bm25m_desc_none(long long k) { return Bm25Desc{nullptr, nullptr, 1.0, 0.0, 0.0, 1.0, k, 0}; }
VF_HD Bm25Desc bm25m_desc(const uint32_t* allow, const double* idf, double avgdl, double k1, double b, long long m, long long k) {
    return Bm25Desc{allow, idf, avgdl, k1, b, 1.0 - b, bm25m_pad_from(true, m, k), m};
}

// the query can return a row: it has no filter, or its filter allows one
VF_HD bool bm25m_can_return(const Bm25Desc& d) { return !d.allow || d.m > 0; }

struct Bm25MultiPlan {
    bool no_launch;          // no query of the call can return a row: the result is all padding
    bool small;              // k <= kBm25mSmallK: S queries per group; else the deep-k scratch, one query at a time
    int S;                   // slots per group
    int tail_blocks;         // every block of the bitmap, for every slot
    long long tblk_stride;   // tail counts per slot (= tail_blocks); 0 in the deep-k scratch, which holds one query
};

// desc: the call's nq descriptors; words: the handle's bitmap words per slot (a multiple of kBm25FilterBlockWords)
VF_HD Bm25MultiPlan bm25m_plan(const Bm25Desc* desc, long long k, int nq, int slot_cap, long long words) {
    Bm25MultiPlan p{};
    p.no_launch = true;
    for (int q = 0; q < nq; ++q)
        if (bm25m_can_return(desc[q])) p.no_launch = false;
    p.small = k <= kBm25mSmallK;
    p.S = p.small ? (nq < slot_cap ? nq : slot_cap) : 1;
    p.tail_blocks = (int)(words / kBm25FilterBlockWords);
    p.tblk_stride = p.small ? p.tail_blocks : 0;
    return p;
}

// ranks the padding kernel's grid must cover for the queries q0 .. q0 + g - 1: the longest of their spans k - pad_from; 0: no launch
VF_HD long long bm25m_group_pad_span(const Bm25Desc* desc, int q0, int g, long long k) {
    long long span = 0;
    for (int q = q0; q < q0 + g; ++q)
        if (k - desc[q].pad_from > span) span = k - desc[q].pad_from;
    return span;
}

}  // namespace vf
