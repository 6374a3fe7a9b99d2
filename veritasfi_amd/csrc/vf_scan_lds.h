// vf_scan_lds.h -- what the scan kernels take of a CU's LDS, as plain arithmetic: the design constants, the row forms and the LDS budget
// of every scan kernel but the two ksplit ones (those sit beside their geometry in vf_ksplit_geom.h, which builds on this header).
// The kernels and their launchers (vf_kernels.hip), the scan route (vf_route.h) and a host-compiled test (tests/test_scan_route.py:
// UBSan) share these definitions; each constant is defined here and nowhere else.
// No HIP header: the host compiler reads it as it stands.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__)
#define VF_HD __host__ __device__ __forceinline__
#else
#define VF_HD inline
#endif

namespace vf {

// ---- fixed design constants ------------------------------------------------------
constexpr int kQueryTile = 32;        // queries per MFMA N-tile (v_mfma_f32_32x32x16_f16)
constexpr int kMaxBatch = 64;         // queries per scan pass (2 N-tiles); larger nq loops
constexpr int kRowTile = 32;          // corpus rows per MFMA M-tile
constexpr int kScanThreads = 512;     // 8 waves per workgroup, one workgroup per CU
constexpr int kHistBins = 2048;       // threshold histogram over cosine in [-1, 1]
constexpr int kSmallN = 16384;        // <= this many rows: exact dense path (LDS sort)
constexpr int kMaxCap = 8192;         // candidate slots per query in the fused path (u64 each)
constexpr int kCntStride = 32;        // u32 elements between per-query counters: one 128-B line each
constexpr int kMaxKFused = 2048;      // largest k the fused path serves (k' <= 4096 <= cap/2)

constexpr int kLdsBytes = 160 * 1024;      // the LDS of a CU: what one workgroup of a scan kernel may take
constexpr int kStageMaxBytes = 32 * 1024;  // the candidate stage takes what the operands leave, up to this much (16 bytes per entry)
constexpr int kStageMinEntries = 256;      // a kernel whose stage would hold fewer entries does not serve the shape

// How a scan kernel reads a corpus row: the very integers the kernels' F8 template parameters take.
enum RowForm : int {
    kRowsF16 = 0,      // fp16 rows (or the fp16 scan copy of fp32 rows)
    kRowsE4m3 = 1,     // e4m3 codes, converted in registers (cvt8_e4m3)
    kRowsI8 = 2,       // the biased bytes of an int8 index or of the int8 row image, converted in registers (cvt8_i8b)
    kRowsI8Mfma1 = 3,  // ... on the int8 matrix instruction, the queries as one int8 plane (k_scan2r only)
    kRowsI8Mfma2 = 4,  // ... as two planes, hi + lo (k_scan2r only)
};
VF_HD bool row_form_bytes(RowForm f) { return f != kRowsF16; }   // one byte per element in HBM

// ---- LDS control block of k_scan (right after the query image) ---------------------------------
//   +0   u32 stage_cnt     candidates staged by this workgroup (main mode)
//   +4   u32 next_tile     next unclaimed tile of the workgroup's row range
//   +16  int tau_lds[64]   the workgroup's copy of the per-query threshold bins
//   +272 uint4 entries[stage_cap]
constexpr int kCtlBytes = 272;

// candidate-stage entries in what `fixed` bytes of operands and control block leave of the LDS
VF_HD int stage_entries(size_t fixed) {
    const size_t freeb = fixed < (size_t)kLdsBytes ? (size_t)kLdsBytes - fixed : 0;
    return (int)((freeb < (size_t)kStageMaxBytes ? freeb : (size_t)kStageMaxBytes) / 16);
}

// dynamic LDS of k_scan: query image + (main mode) candidate stage
VF_HD size_t scan_lds_bytes(int dp, int qn_tile) { return (size_t)dp * qn_tile * 2 + kCtlBytes; }
VF_HD int scan_stage_cap(int dp, int qn_tile) { return stage_entries(scan_lds_bytes(dp, qn_tile)); }

// k_scan2 / k_scan2r: four streaming waves (+ k_scan2's service wave in A/B builds), each with a ring of 4-KB row segments and a scratch
// of two 512-B halves (tile parity)
constexpr int kScan2Waves = 4, kRing = 3, kSegBytes = 4096, kScratchBytes = 1024;

VF_HD size_t scan2_lds_bytes(int dp, int qn_tile, int stage_cap) {
    const size_t img = (size_t)dp * qn_tile * 2;
    return img + (size_t)kScan2Waves * (kRing * kSegBytes + kScratchBytes) + kCtlBytes + (size_t)stage_cap * 16;
}
VF_HD int scan2_stage_cap(int dp, int qn_tile, RowForm rows) {   // candidate-stage entries that fit beside image + rings; < 256 = "does not fit"
    const size_t fixed = scan2_lds_bytes(dp, qn_tile, 0);
    if ((dp >> (rows ? 7 : 6)) < kRing) return 0;  // the ring holds three 128-byte segments of ONE row set at start-up
    if (fixed + kStageMinEntries * 16 > (size_t)kLdsBytes) return 0;
    return stage_entries(fixed);
}

// The shapes k_scan2r is built for -- (row bytes per 128-byte segment count S, register segments RB, ring depth RING):
//   fp16 rows, dp =  768: S = 12, RB = 6 (192 registers of B fragments at 64 queries), RING = 6
//   fp16 rows, dp = 1024: S = 16, RB = 6, RING = 4 (80 KB of image in LDS: k_scan2 has no room for this width at all)
//   fp16 rows, dp =  512: S =  8, RB = 4, RING = 6;   dp = 384: S = 6, RB = 3, RING = 6
//   e4m3 rows, dp =  768: S =  6, RB = 3 (a segment is 128 elements: 16 KB of image, 64 registers), RING = 6
//   e4m3 rows, dp = 1024: S =  8, RB = 3 (with the 32 accumulators the 256 accumulator registers hold no fourth), RING = 4
// (e4m3 rows are converted in registers like k_scan2's F8 variant: every e4m3 value is an fp16 value, the image is shared.)
// kRowsI8: the int8 row image of fp16 / fp32 rows of 768 elements (k_prep_image) -- one byte per element like e4m3 rows, so the e4m3
// shape; the bytes are converted by cvt8_i8b (exact), the row's scale rides in its inverse norm and its quantisation bound is added to
// every score (ScanArgs::off_scan).
struct Scan2rShape { int S, RB, RING; };
VF_HD Scan2rShape scan2r_shape(int dp, RowForm f8) {
    if (!f8 && dp == 768) return {12, 6, 6};
    if (!f8 && dp == 1024) return {16, 6, 4};   // (bge-m3 / bge-large rows: the reference's own width, config/example.yaml:3)
    if (!f8 && dp == 512) return {8, 4, 6};
    if (!f8 && dp == 384) return {6, 3, 6};
    if (f8 == kRowsI8Mfma1) return dp == 768 ? Scan2rShape{6, 6, 6} : Scan2rShape{0, 0, 0};   // one int8 query plane: every B fragment in registers
    if (f8 == kRowsI8Mfma2) return dp == 768 ? Scan2rShape{6, 3, 6} : Scan2rShape{0, 0, 0};   // hi + lo planes: half in registers, half in LDS, as the fp16 image
    if (f8 && dp == 768) return {6, 3, 6};
    if (f8 && dp == 1024) return {8, 3, 4};
    return {0, 0, 0};
}
VF_HD size_t scan2r_lds_bytes(int dp, int qn_tile, int stage_cap, RowForm f8) {
    const Scan2rShape sh = scan2r_shape(dp, f8);
    const size_t seg_img = (size_t)(f8 ? 128 : 64) * qn_tile * 2;
    return (size_t)(sh.S - sh.RB) * seg_img + (size_t)kScan2Waves * (sh.RING * kSegBytes + kScratchBytes) + kCtlBytes + (size_t)stage_cap * 16;
}
VF_HD int scan2r_stage_cap(int dp, int qn_tile, RowForm f8) {   // < 256 = "not this kernel"
    if (scan2r_shape(dp, f8).S == 0) return 0;
    const size_t fixed = scan2r_lds_bytes(dp, qn_tile, 0, f8);
    if (fixed + kStageMinEntries * 16 > (size_t)kLdsBytes) return 0;
    return stage_entries(fixed);
}

// k_scan_wide / k_scan_wide8: 256-query tiles, the query operand streaming through three LDS buffers of one 64-element chunk each
constexpr int kWideQ = 256, kWideKC = 64;
constexpr int kWideBuf = (kWideKC / 8) * kWideQ * 16;   // 32 KB per query chunk
constexpr int kWideCtl = 16 + 3 * kWideQ * 4;            // stage_cnt | tau_lds[256] | qcnt[256] | qbase[256]
constexpr int kWideStageCap = 3584;                      // 56 KB of candidate stage: the LDS the 96 KB of operand buffers and the control block leave

VF_HD size_t scan_wide_lds_bytes(int stage_cap) { return (size_t)3 * kWideBuf + kWideCtl + (size_t)stage_cap * 16; }
// waves = 8: a.jtiles 256-query tiles, one 512-thread workgroup per CU; waves = 4: a.jtiles 128-query tiles, two 256-thread workgroups per CU
VF_HD size_t scan_wide8_lds_bytes(int waves, int stage_cap) {
    return waves == 8 ? scan_wide_lds_bytes(stage_cap) : (size_t)65536 + (16 + 3 * 128 * 4) + (size_t)stage_cap * 16;
}
VF_HD int scan_wide8_stage_cap(int waves) { return waves == 8 ? kWideStageCap : 896; }   // what the operand stages and the control block leave of 160 / 80 KB

}  // namespace vf
