// vf_ksplit_geom.h -- the address geometry of k_scan_ksplit (rows of 2560 to 4096 padded elements), as plain functions the kernel, its
// launcher and a host-compiled test (tests/test_wide_rows_geometry.py: UBSan, every (n, grid, sample rows, wave, tile, lane)) share.
// The LDS budgets of the two kernels follow their geometry (the constants they share with the other scans: vf_scan_lds.h).
// No HIP header: the host compiler reads it as it stands.
#pragma once

#include "vf_scan_lds.h"   // VF_HD, kCtlBytes, stage_entries

namespace vf {

constexpr int kKsWaves = 4;        // one wave per SIMD; wave w owns a quarter of every row's 128-byte segments
constexpr int kKsThreads = kKsWaves * 64;
constexpr int kKsRegSegs = 10;     // query segments (64 elements x 32 queries = 16 registers per lane) a wave keeps in registers
constexpr int kKsMinDp = 2560;     // dp / 64 / 4 >= kKsRegSegs: every wave fills its register segments
constexpr int kKsMaxDp = 4096;     // (P - kKsRegSegs) * 4 waves * 4 KB = 96 KB of LDS for the rest of the image
constexpr int kKsSampWaves = 8;    // the sample part of a range is samp * 8 rows, whatever the kernel's wave count (k_sel0's slot map)
constexpr int kKsRowTile = 32;
constexpr int kKsSegBytes = 4096;  // one segment of a 32-query image
constexpr int kKsRedBytes = 2 * kKsWaves * 4096;   // partial accumulator tiles: [tile parity][wave][16 registers x 64 lanes] floats

VF_HD bool ks_serves(int dp) { return dp >= kKsMinDp && dp <= kKsMaxDp && dp % 128 == 0; }
VF_HD int ks_segs(int dp) { return dp >> 6; }
// wave w owns segments [ks_seg_begin(S, w), ks_seg_begin(S, w + 1)) of S: 10 to 16 of them, counts differ by at most one
VF_HD int ks_seg_begin(int S, int w) { return S * w / kKsWaves; }
// segments per wave the kernel is unrolled for (the last one may be absent in some waves)
VF_HD int ks_P(int S) { return (S + kKsWaves - 1) / kKsWaves; }
// ring depth (segments in flight per wave): divides P, so that segment j of every tile lands in ring slot j % D
VF_HD int ks_D(int P) { return P == 12 ? 6 : P == 14 ? 7 : P == 15 ? 5 : P == 16 ? 8 : P; }

struct KsPart { long long lo, hi; };
// rows of range v (of `grid`) in one mode: the sample part is its first swg rows, the main part the rest
VF_HD KsPart ks_part(long long n, long long grid, long long v, long long swg, bool sample) {
    const long long Ra = n * v / grid, Rb = n * (v + 1) / grid;
    const long long Rs = (Ra + swg < Rb) ? Ra + swg : Rb;
    KsPart p;
    p.lo = sample ? Ra : Rs;
    p.hi = sample ? Rs : Rb;
    return p;
}
// tiles a workgroup walks: every tile of the main part; ceil(swg / 32) of the sample part (those past a short range's end write nothing)
VF_HD int ks_ntiles(const KsPart& p, long long swg, bool sample) {
    return (int)(((sample ? swg : p.hi - p.lo) + kKsRowTile - 1) / kKsRowTile);
}
// the row lane (r31) of tile `tile` reads: inside the part where it has rows, and inside [0, n) always
VF_HD long long ks_row(const KsPart& p, long long n, int tile, int r31) {
    long long r = p.lo + (long long)tile * kKsRowTile + r31;
    if (r > p.hi - 1) r = p.hi - 1;
    if (r > n - 1) r = n - 1;
    if (r < 0) r = 0;
    return r;
}
// byte offset of the 16 bytes lane half h reads for step i (0..3) of segment sg of `row`
VF_HD long long ks_src(long long row, long long row_bytes, int sg, int h, int i) {
    return row * row_bytes + (long long)sg * 128 + h * 64 + i * 16;
}
// index into inv_scan ([n + 64]) of the reciprocal norm lane r31 fetches for the tile that starts at row t0
VF_HD long long ks_inv_index(long long t0, long long n, int r31) {
    const long long i = t0 + r31;
    return i < n + 63 ? (i < 0 ? 0 : i) : n + 63;
}
// LDS of k_scan_ksplit: the image segments the registers do not hold + the reduction area + control block + (main mode) candidate stage
VF_HD size_t scan_ksplit_lds_bytes(int dp, int stage_cap) {
    const int xs = ks_P(ks_segs(dp)) - kKsRegSegs;
    return (size_t)kKsWaves * (xs > 0 ? xs : 0) * kKsSegBytes + kKsRedBytes + kCtlBytes + (size_t)stage_cap * 16;
}
// candidate-stage entries that fit beside them; 0 = not this kernel
VF_HD int scan_ksplit_stage_cap(int dp) { return ks_serves(dp) ? stage_entries(scan_ksplit_lds_bytes(dp, 0)) : 0; }

// ---- k_scan_ksplit8: the same rows stored as e4m3 bytes (tests/test_wide_rows_fp8_geometry.py walks these) ------------------------------
// A row is dp bytes; a segment is 128 BYTES = 128 elements = eight matrix steps, so a row has dp / 128 segments (20 to 32), a wave 5 to 8.
// Ranges, sample parts, tiles, rows and reciprocal-norm indices are the functions above (ks_part, ks_ntiles, ks_row, ks_inv_index), and
// the 16 bytes a lane half reads are ks_src with row_bytes = dp.
constexpr int kKs8RegSegs = 5;      // query segments (128 elements x 32 queries = 32 registers per lane) a wave keeps in registers: 160
constexpr int kKs8MaxSegs = 8;      // segments per wave at dp = 4096; the ring holds the wave's whole share of a tile (16 registers each)
constexpr int kKs8SegBytes = 8192;  // one 128-element segment of a 32-query image: 16 k-groups x 32 queries x 16 bytes
constexpr int kKs8CtlBytes = kCtlBytes;   // the scans' control block, under the name tests/test_wide_rows_fp8_geometry.py knows it by

VF_HD int ks8_segs(int dp) { return dp >> 7; }
// wave w owns segments [ks8_seg_begin(S8, w), ks8_seg_begin(S8, w + 1)) of S8: 5 to 8 of them, counts differ by at most one
VF_HD int ks8_seg_begin(int S8, int w) { return S8 * w / kKsWaves; }
VF_HD int ks8_P(int S8) { return (S8 + kKsWaves - 1) / kKsWaves; }
// the k-group (8 elements, 16 bytes per query of the fp16 image) that meets the 8 bytes lane half h converts for step i (0..7) of segment
// sg: bytes [128 sg + 64 h + 8 i, + 8) of the row are elements of the same numbers
VF_HD int ks8_group(int sg, int h, int i) { return 16 * sg + 8 * h + i; }
// which of the four 16-byte loads (ks_src's i) holds step i's 8 bytes, and which half of it
VF_HD int ks8_step_load(int i) { return i >> 1; }
VF_HD int ks8_step_half(int i) { return i & 1; }
// LDS: [4 waves][P8 - 5] image segments + the reduction area + the control block + (main mode) the candidate stage
VF_HD long long ks8_lds_bytes(int dp, int stage_cap) {
    const int xs = ks8_P(ks8_segs(dp)) - kKs8RegSegs;
    return (long long)kKsWaves * (xs > 0 ? xs : 0) * kKs8SegBytes + kKsRedBytes + kCtlBytes + (long long)stage_cap * 16;
}
// candidate-stage entries that fit beside them in 160 KB (at most 32 KB of them); < 256 = not this kernel
VF_HD int ks8_stage_cap(int dp) {
    return ks_serves(dp) ? stage_entries((size_t)ks8_lds_bytes(dp, 0)) : 0;
}

}  // namespace vf
