// vf_compact.h -- the plan of a stable in-place row compaction (VF_INDEX_REMOVE: rows leave a live index and every later row moves
// down), as plain functions the mover (k_compact_rows), its host side (vf_api.hip) and a host-compiled test
// (tests/test_compact_plan.py: UBSan, every subset of up to 12 rows at every chunk size) share.
//
// n0 rows, of which the m rows rem[0] < rem[1] < ... < rem[m - 1] leave; n1 = n0 - m stay, in their order.  Destination row j of the
// result is source row compact_src(j) >= j of the array as it was.  Rows below first = rem[0] keep their place and are neither read
// nor written.  The rows [first, n1) are moved in chunks of at most `chunk_rows` destination rows, ascending, each in two steps:
// gather the chunk's source rows into a staging buffer, then copy the buffer onto the chunk's destination rows.  The sources of chunk
// c lie at or above its own first destination row (src(j) >= j), which is the destination end of chunk c - 1: a chunk never reads what
// an earlier one wrote, so the order of the launches on one stream is all the synchronisation there is.
// 64-bit arithmetic throughout (a shard holds up to 2^32 - 2 rows).  No HIP header: the host compiler reads it as it stands.
#pragma once

#include "vf_scan_lds.h"   // VF_HD

namespace vf {

constexpr long long kCompactStageBytes = 64ll << 20;   // the staging buffer of an automatic plan (capped at the bytes that move)

// source row of destination row j: j + the number of removed rows at or below it, i.e. the count of t with rem[t] - t <= j
// (rem[t] - t never decreases in t: a binary search)
VF_HD long long compact_src(long long j, const long long* rem, long long m) {
    long long lo = 0, hi = m;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (rem[mid] - mid <= j) lo = mid + 1; else hi = mid;
    }
    return j + lo;
}

struct CompactPlan {
    long long first;        // the first destination row that changes (rem[0], or n1 when only the last rows leave)
    long long end;          // n1: one past the last destination row
    long long chunk_rows;   // destination rows per chunk (>= 1): what the staging buffer must hold
    long long chunks;       // ceil((end - first) / chunk_rows); 0 when nothing moves
};
struct CompactChunk { long long lo, hi; };   // destination rows [lo, hi)

// rem0: the lowest removed row (ignored when m == 0); cap_rows: rows the staging buffer may hold (< 1 counts as 1)
VF_HD CompactPlan compact_plan(long long n0, long long m, long long rem0, long long cap_rows) {
    CompactPlan p;
    p.end = n0 - m;
    p.first = (m > 0 && rem0 < p.end) ? rem0 : p.end;
    const long long moved = p.end - p.first;
    long long c = cap_rows < 1 ? 1 : cap_rows;
    if (c > moved) c = moved;
    p.chunk_rows = c < 1 ? 1 : c;
    p.chunks = (moved + p.chunk_rows - 1) / p.chunk_rows;
    return p;
}

VF_HD CompactChunk compact_chunk(const CompactPlan& p, long long c) {
    CompactChunk k;
    k.lo = p.first + c * p.chunk_rows;
    k.hi = k.lo + p.chunk_rows < p.end ? k.lo + p.chunk_rows : p.end;
    return k;
}

// rows per chunk of an automatic plan: what kCompactStageBytes hold of the widest array that moves
VF_HD long long compact_auto_rows(long long widest_row_bytes) {
    const long long r = kCompactStageBytes / (widest_row_bytes < 1 ? 1 : widest_row_bytes);
    return r < 1 ? 1 : r;
}

// the widest access (16, 8, 4, 2 or 1 bytes) that both addresses and the row size allow: whole rows are then whole units
VF_HD int compact_unit(unsigned long long src, unsigned long long dst, long long row_bytes) {
    const unsigned long long x = src | dst | (unsigned long long)row_bytes;
    return (x & 15) == 0 ? 16 : (x & 7) == 0 ? 8 : (x & 3) == 0 ? 4 : (x & 1) == 0 ? 2 : 1;
}
// rows one workgroup moves: about 16 KB of them, 1 to 256
VF_HD int compact_rows_per_block(long long row_bytes) {
    const long long r = 16384 / (row_bytes < 1 ? 1 : row_bytes);
    return r < 1 ? 1 : r > 256 ? 256 : (int)r;
}

}  // namespace vf
