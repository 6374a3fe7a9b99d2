// vf_bm25_call.h -- what kind of call a vf_bm25_search is and which kernels it launches, as two pure functions the entry point
// (vf_sparse.hip) and a host-compiled test (tests/test_bm25_call_plan.py: UBSan, every flag combination and phase, then the plan at
// the sizes where it changes) share.
//
//   bm25c_decode   the mode rides on `nq` as flag bits and on a phase member of the struct `q_offsets` then points to
//                  (include/veritasfi_hip.h: VF_BM25_FILTER, VF_BM25_SUBSTATS, VF_BM25_PREPARED): one of eight kinds and nq without the
//                  bits, or the first refusal in the entry point's order.  The texts of the refusals stay in vf_sparse.hip.
//   bm25c_plan     what the kind launches at (k, nq, the handle's slots and bitmap words, the m rows allowed): slots per group, which
//                  scatter kernel, plain or filtered tail and over how many bitmap blocks, where the padding starts -- or nothing at
//                  all, when no row is allowed.
// No HIP header and none of the ABI's: the host compiler reads it as it stands (vf_sparse.hip asserts the bits equal the ABI's).
#pragma once

#include <stdint.h>

#include "vf_bm25_filter.h"   // bm25f_plan; VF_HD

namespace vf {

constexpr int kBm25cFilter = 0x40000000, kBm25cSubstats = 0x20000000, kBm25cPrepared = 0x10000000;   // VF_BM25_FILTER, _SUBSTATS, _PREPARED
constexpr int kBm25cSmallK = 4096;                                                                     // = kBmSmallK, vf_sparse.hip

enum Bm25Kind { kBm25Plain, kBm25Filtered, kBm25SubStage, kBm25SubSearch, kBm25PrepPrepare, kBm25PrepArm, kBm25PrepRelease, kBm25PrepSearch };

// in the order the entry point meets them; kBm25NullPrepared and kBm25NullFilter are the null struct of either flag
enum Bm25Refusal { kBm25Accepted = 0, kBm25PreparedNotAlone, kBm25NullPrepared, kBm25PreparedPhase, kBm25NullFilter, kBm25SubstatsPhase, kBm25SubstatsAlone, kBm25Refusals };

struct Bm25Call {
    Bm25Kind kind;
    Bm25Refusal refusal;   // not kBm25Accepted: nothing else is meaningful
    int nq;                // without the flag bits
    bool subset;           // kBm25PrepSearch: the filter is in subset mode (scored by its own idf table); false out of the decoder, set by
                           // the entry point once it has found the filter the call's token names
};

// the struct of this call has a phase member that may be read (a vf_bm25_filter_query has none; a refused combination reads nothing)
VF_HD bool bm25c_has_phase(int nq_raw) {
    const int f = nq_raw & (kBm25cFilter | kBm25cSubstats | kBm25cPrepared);
    return f == kBm25cPrepared || f == (kBm25cFilter | kBm25cSubstats);
}

// phase: the struct's phase member (anything when the pointer is null or bm25c_has_phase is false)
VF_HD Bm25Call bm25c_decode(int nq_raw, bool null_struct, int phase) {
    const int flags = kBm25cFilter | kBm25cSubstats | kBm25cPrepared;
    Bm25Call c{kBm25Plain, kBm25Accepted, nq_raw & ~flags, false};
    if (nq_raw & kBm25cPrepared) {
        if (nq_raw & (kBm25cFilter | kBm25cSubstats)) c.refusal = kBm25PreparedNotAlone;
        else if (null_struct) c.refusal = kBm25NullPrepared;
        else if (phase < 1 || phase > 4) c.refusal = kBm25PreparedPhase;
        else c.kind = phase == 1 ? kBm25PrepPrepare : phase == 2 ? kBm25PrepArm : phase == 3 ? kBm25PrepSearch : kBm25PrepRelease;
    } else if (nq_raw & kBm25cFilter) {
        if (null_struct) c.refusal = kBm25NullFilter;
        else if (!(nq_raw & kBm25cSubstats)) c.kind = kBm25Filtered;
        else if (phase == 1) c.kind = kBm25SubStage;
        else if (phase == 2) c.kind = kBm25SubSearch;
        else c.refusal = kBm25SubstatsPhase;
    } else if (nq_raw & kBm25cSubstats) {
        c.refusal = kBm25SubstatsAlone;
    }
    return c;
}

enum Bm25Scatter { kBm25ScatterPlain, kBm25ScatterFiltered, kBm25ScatterSubPos, kBm25ScatterSubCol };   // k_bm25_accum, _f, _s, _sc

struct Bm25LaunchPlan {
    bool no_launch;          // nothing runs: no row is allowed (the result is all padding), or the kind is not a search's
    bool small;              // k <= kBm25cSmallK: one LDS sort per query, S queries per group; else the deep-k scratch, one at a time
    int S;                   // slots per group (the stage: the slots of the search that follows it)
    Bm25Scatter scatter;
    bool tail_f;             // the tail kernels are the _f forms, and the small-k tail's counts lie in the filtered call's own array
    int tail_blocks;         // bitmap blocks the tail counts: the first alone for the unfiltered small-k call (fewer than k touched rows
                             // means fewer than kBm25cSmallK, so its tail lies in block 0), every block otherwise
    long long tblk_stride;   // tail counts per slot; 0 in the deep-k scratch, which holds one query
    long long pad_from;      // first padded rank: min(m, k), k for an unfiltered call
    bool pad_out;            // k_bm25_pad_out runs: a filtered call of fewer than k rows
};

// words: the handle's bitmap words per slot (a multiple of kBm25FilterBlockWords); m: rows allowed (not read for kBm25Plain)
VF_HD Bm25LaunchPlan bm25c_plan(const Bm25Call& c, long long k, int nq, int slot_cap, long long words, long long m) {
    Bm25LaunchPlan p{};
    p.no_launch = true;
    if (c.kind == kBm25PrepPrepare || c.kind == kBm25PrepArm || c.kind == kBm25PrepRelease) return p;   // not a search's: nothing else is set
    const bool filtered = c.kind != kBm25Plain;
    const Bm25FilterPlan fp = bm25f_plan(words, filtered ? m : k, k);
    p.no_launch = filtered && m == 0;
    p.small = k <= kBm25cSmallK;
    p.S = (p.small || c.kind == kBm25SubStage) ? (nq < slot_cap ? nq : slot_cap) : 1;
    p.scatter = !filtered ? kBm25ScatterPlain : c.kind == kBm25SubSearch ? kBm25ScatterSubPos : (c.kind == kBm25PrepSearch && c.subset) ? kBm25ScatterSubCol : kBm25ScatterFiltered;
    p.tail_f = filtered;
    p.tail_blocks = (filtered || !p.small) ? fp.tail_blocks : 1;
    p.tblk_stride = !p.small ? 0 : (filtered ? fp.tblk_entries : 1);
    p.pad_from = fp.pad_from;
    p.pad_out = filtered && p.pad_from < k;
    return p;
}

}  // namespace vf
