// vf_route.h -- which kernels serve a search: the one decision every search makes, as a pure function of the handle's shape and options.
// vf_api.hip fills a RouteIn from the handle (route_in), asks route_path / route_search once per search, route_batch or route_wide_pass
// once per pass (their answers carry what the pass is launched with beside its kernels: the publication block, whether the sample slots
// need clearing, the bytes a timed scan reads), and switches on the answer; allocation, streams, events and launches stay there.  Every threshold the choice rests on is
// defined here, beside the record of where it was measured.  Plain C++17: no HIP and no vf_index, so a host-compiled driver
// (tests/test_scan_route.py: UBSan, a table of pinned routes and an option sweep) evaluates it without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/veritasfi_hip.h"  // VF_DTYPE_*
#include "vf_ksplit_geom.h"               // + vf_scan_lds.h: the design constants, RowForm, every scan kernel's LDS budget
#include "vf_options.h"                   // the option table: names, defaults, accepted values

namespace vf {

// What the choice depends on: the option values as set (vf_options.h; -1 = auto where an option has one) and the handle's shape.
struct RouteIn : Options {
    int64_t n = 0;
    int d = 0, dp = 0, dtype = 0, n_cu = 256;
    bool has_scan = false;      // the scan copy and its inverse norms exist (corpora of up to kSmallN rows are built without them)
    bool has_image = false;     // an int8 row image exists ...
    float rho_mean = 0.0f;      // ... with this average relative residual
    bool group = false;         // a group handle (its shards route for themselves)
    int64_t aux_applied = -1;   // the CU split the first slot's streams were created with (-1: no slot yet)
    bool masked = false;        // this slot's scan stream is CU-masked
};

// the scan kernels, by the code vf_search_stats.scan_kernel reports (veritasfi_hip.h); a sample pass is named by the same codes
enum ScanKernel : int {
    kKernelNone = 0, kKernelScan = 1, kKernelScan2 = 2, kKernelWide = 3, kKernelWide8 = 4, kKernelScan2r = 5, kKernelKsplit = 6,
    kKernelKsplit8 = 7,   // k_scan_ksplit8 on e4m3 codes, k_scan_ksplit8i on int8 rows (as k_scan's and k_scan_wide's int8 forms report 1 and 3)
};

struct FusedPlan {
    int kprime, cap, total_waves, grid, samp;
    float eps;
    bool image;              // the scans read the int8 row image: kprime = k, thresholds and the re-score follow the eps band
    int tau_band, fine_band; // that band (2 eps, rounded up, + one bin) in threshold bins (1 / 1024) and in k_final's fine bins (1 / 16 384)
};

// One search of nq queries for the k best rows.
struct SearchRoute {
    int path = 2;            // -1: refused (force_path = 1 where the fused path cannot serve); 0 small dense, 1 fused, 2 chunked exact
    int per_pass = kMaxBatch;   // queries per pass: 32 or 64 (the widest query image the LDS holds), kWideMaxQueries for wide passes
    // path 1 only:
    bool wide = false;       // wide passes (route_wide_pass for each); else passes of `per_pass` (route_batch for each)
    bool image = false;      // the passes read the int8 row image ...
    int planes = 0;          // ... on the int8 matrix instruction with that many int8 query planes (0: converted, the fp16 instruction)
    FusedPlan plan{};
};

// One pass of nb <= per_pass queries of a search that is not wide.
struct BatchRoute {
    int tile;                // query tile: 32 or 64
    ScanKernel sample;       // the sample pass: kKernelScan, kKernelScan2r, kKernelKsplit or kKernelKsplit8 ...
    int sample_grid;         // ... its workgroups ...
    RowForm sample_rows;     // ... and how it reads a row
    ScanKernel main;         // the main scan
    RowForm main_rows;
    int stage_cap;           // its LDS candidate stage, in entries
    int refresh_every;       // staged entries per published block: a power of two (the kernels find a block's number with a shift)
    bool clear_sample;       // a wave range is shorter than the sample: the slots no wave writes must be cleared first
    int64_t scan_bytes;      // what the main scan reads from HBM (vf_index_profile's scan_bytes_per_launch)
};

// One wide pass of nb <= kWideMaxQueries queries.
struct WidePass {
    ScanKernel main;         // kKernelWide or kKernelWide8 (the sample pass is k_scan_wide's either way)
    RowForm rows;
    int waves;               // k_scan_wide8: 8 (256-query tiles, one workgroup per CU) or 4 (128-query tiles, two per CU)
    int qtot, jtiles, rgroups;   // queries padded to whole tiles of kWideTile, those tiles, row groups
    int main_jtiles;         // query tiles of the main pass: 128 wide for the two-workgroups-per-CU form
    int samp;                // sample rows per row group = samp * 8: 32768 / 65536 rows in all
    int stage_cap;           // the main pass's LDS candidate stage
    int cap;                 // candidate slots per query (the plan's, raised for deep k)
    int refresh_every;       // staged entries per published block: a power of two (block completion is tested with a mask)
    bool clear_sample;       // a row group is shorter than its sample: the slots no wave writes must be cleared first
    int64_t scan_bytes;      // what the main pass reads from HBM (vf_index_profile's scan_bytes_per_launch)
};

// One byte per element in HBM (e4m3 codes, or the biased bytes of an int8 index): scanned as bytes with the e4m3 geometry, converted in
// registers (cvt8_e4m3 / cvt8_i8b).  Everything that sizes a row, picks a byte-row kernel shape or counts traffic asks this.
inline bool byte_rows(int dtype) { return dtype == VF_DTYPE_FP8_E4M3 || dtype == VF_DTYPE_INT8; }
// how the kernels that scan the rows as stored read them (k_scan, k_scan_wide, k_scan_ksplit8)
inline RowForm stored_rows(int dtype) { return dtype == VF_DTYPE_INT8 ? kRowsI8 : (dtype == VF_DTYPE_FP8_E4M3 ? kRowsE4m3 : kRowsF16); }
inline int qn_tile_for(int nq_batch) { return nq_batch <= kQueryTile ? kQueryTile : kMaxBatch; }

// ---- CU split and scan overlap -------------------------------------------------------------------------------------------
// CU split and scan overlap, resolved.  Auto (-1): shards of up to 6M rows run their main scans on all but 32 CUs (one
// per shader engine: a mask that takes CUs from only some SEs leaves those SEs with more workgroups than CUs -- the
// dispatcher hands every SE the same number -- and a scan then takes two rounds; tools/ubench/cu_mask_probe.hip) and let
// consecutive scans overlap; larger shards keep the whole chip and ordered scans (measured, round 3: 1.25M rows 0.384 ->
// 0.362 ms per batch, 2.5M 0.717 -> 0.682, 5M 1.280 -> 1.269, 10M no change; profiles/r03_scan2_sweep.log).
constexpr int64_t kSplitMaxRows = 6'000'000;
constexpr int64_t kScan2rMinRows = 1'100'000;   // k_scan2r (where its shapes exist) above this many rows: below, the workgroup's longer start costs more than the ring gains
// Round 6: where k_scan2r serves the rows (fp16 rows of 384 / 512 / 768 / 1024 elements; a wave keeps 16-24 KB in flight there) the split + overlapping scans
// win at EVERY size -- 7.5M rows 1.878 -> 1.811 ms per batch, 10M rows 2.538 -> 2.466-2.473 (0.7585 -> 0.78 of 8 TB/s), whole chip +
// ordered scans with k_scan2 being the 2.538; k_scan2r on the whole chip with ordered scans LOSES (2.58-2.59): profiles/r06_scan2r_10m.log
// the widths on which k_scan2r was MEASURED against the kernel it replaces and is the default (its other shapes: scan_impl = 5)
// fp16 rows of 1024 / 512 / 384 elements (round 6, profiles/r06_scan2r_fp16_other_widths_ab.log; k_scan2r + its sample pass on the CU split
// with overlapping scans against the default before): 8M x 1024 2.725 -> 2.63-2.65 ms per batch (0.754 -> 0.774-0.781 of 8 TB/s; k_scan served
// that width: k_scan2's image does not fit), 1.25M x 1024 0.465-0.467 -> 0.430-0.444, 10M x 512 1.711 -> 1.620-1.643 (0.765 -> 0.785-0.796),
// 10M x 384 1.330 -> 1.262, 1.25M x 512 0.266-0.270 -> 0.260-0.265
inline bool scan2r_auto_width(int dp, bool f8) { return f8 ? (dp == 768 || dp == 1024) : (dp == 768 || dp == 1024 || dp == 512 || dp == 384); }
inline int64_t split_limit(const RouteIn& in) {
    const bool r_rows = !byte_rows(in.dtype) && in.scan_impl != 4 && in.scan_impl != 1 && in.scan_impl != 3 && !in.steal &&
                        scan2r_auto_width(in.dp, false) && scan2r_stage_cap(in.dp, kMaxBatch, kRowsF16) >= kStageMinEntries;
    return r_rows ? INT64_MAX : kSplitMaxRows;
}
// CUs the main scans leave to the small kernels of the other slots (0 = no split)
inline int64_t route_aux_cus(const RouteIn& in) {
    if (in.aux_applied >= 0) return in.aux_applied;   // what the existing scan streams are masked with (0 if masking failed)
    int64_t a = in.aux_cus >= 0 ? in.aux_cus : (in.n <= split_limit(in) ? 32 : 0);
    if (a <= 0 || in.n_cu < 64 || a * 2 > in.n_cu) return 0;
    return a;
}
inline bool route_overlap(const RouteIn& in) { return in.overlap_scans >= 0 ? in.overlap_scans != 0 : route_aux_cus(in) > 0; }
// what vf_search_stats reports of the two for a finished search
struct SplitReport { int aux_cus, scans_overlap; };
inline SplitReport route_split_report(const RouteIn& in, int path) {
    return {(path == 1 && in.masked) ? (int)route_aux_cus(in) : 0, (path == 1 && route_overlap(in)) ? 1 : 0};
}

// Rows of 2560 to 4096 padded elements (fp16, or the fp16 scan copy of fp32 rows; e4m3 rows: below): a 32-query image does not fit the LDS, so k_scan cannot
// serve them; k_scan_ksplit does (the contraction split over four waves, the image in registers + LDS).  Option wide_rows: 0 never, 2
// wherever the kernel serves the rows, 1 (auto) from kWideRowsMinRows rows.
// The count is measured (tools/bench_wide_rows.py, one box, the settings alternating, three windows of a second each;
// profiles/r08_wide_rows_threshold.log): the chunked exact path against this one at 32 768 / 65 536 / 131 072 / 262 144 / 1 048 576 rows,
// 1 / 4 / 64 queries, k = 100 / 2048.  At k = 100 the fused path wins everywhere (32 768 x 2560, one query: 0.139 against 0.329 ms).  At
// k = 2048 with one or four queries k_final's re-score of k' = 2 560+ rows per query is the step, and the fused path LOSES at 32 768 rows
// (2560: 0.579 / 0.619 against 0.357 / 0.479 ms; 4096: 0.912 / 0.975 against 0.520 / 0.571) and, for 4096-wide rows, at 65 536
// (1.231 / 1.287 against 1.025 / 1.104; 2560-wide rows are 1 to 4 % ahead there: a tie); from 131 072 rows it wins every cell at both widths
// (k = 2048, one query: 0.845 against 1.375 ms at 2560, 1.406 against 2.036 at 4096) and the margin grows with n (1M x 2560: 0.86
// against 10.1 ms).  So: 131 072 for every width.  Below it the existing behaviour stays (tests/test_gpu_retrieval.py::
// test_wide_rows_and_path_limits: 17 000 x 2560 on path 2).
constexpr int64_t kWideRowsMinRows = 131072;
inline bool ksplit_width(int dp) { return scan_lds_bytes(dp, kQueryTile) > (size_t)kLdsBytes; }   // no LDS-resident 32-query image: dp > 2432
// e4m3 rows of these widths: k_scan_ksplit8 (a row is dp bytes; the same split, image and reduction), under the same option.  Its count is
// measured the same way (tools/bench_wide_rows.py --dtype fp8, one box, the settings alternating, three windows;
// profiles/r10_wide_rows_fp8_threshold.log): 32 768 / 65 536 / 131 072 / 262 144 / 1 048 576 rows, 1 / 4 / 32 / 64 / 65 / 96 / 128 queries,
// k = 100 / 2048, d = 2560 and 4096.  Half the bytes per row halve the scan and the re-score of k' rows, so the fused path wins EVERY cell
// from the smallest row count of the grid: the closest are k = 2048 with one query at 32 768 rows, 0.339 against 0.364 ms at 2560 and
// 0.505 against 0.540 at 4096 (four queries: 0.345 / 0.475 and 0.518 / 0.670); at k = 100 it is 0.109 against 0.345 and 0.143 against
// 0.539 there, and 0.439 against 10.5 and 0.749 against 16.5 ms at 1M rows.  So: 32 768, for every width.
constexpr int64_t kWideRowsMinRows8 = 32768;
// int8 rows of these widths: k_scan_ksplit8i, which is k_scan_ksplit8 with cvt8_i8b at the matrix instruction (the device bytes of an int8
// index are the biased bytes it converts; geometry, LDS budget and stage cap are the byte-row kernel's).  They are served from 32 768 rows
// upward and that count is a FLOOR, not only the auto threshold: wide_rows = 2 and force_path = 1 do not go below it either.  32 768 is the
// smallest row count at which the byte-row kernel has ever been measured (profiles/r10_wide_rows_fp8_threshold.log: it won every cell
// there), and below it the behaviour of int8 rows is pinned by tests/test_gpu_int8_rows.py::
// test_int8_chunked_exact_path_and_rows_of_2560_elements (17 000 x 2560: path 2 under wide_rows = 1 and 2, force_path = 1 refused).
constexpr int64_t kWideRowsMinRowsI8 = 32768;
inline std::string wide_rows_refusal() {   // (declared in vf_options.h: the wide_rows row of the table)
    return std::string("wide_rows must be 0 (rows of more than 2432 padded elements never take the fused path), 1 (auto: from ") + std::to_string(kWideRowsMinRows) + " rows, e4m3 rows from " + std::to_string(kWideRowsMinRows8) + ", int8 rows from " + std::to_string(kWideRowsMinRowsI8) + ") or 2 (wherever k_scan_ksplit / k_scan_ksplit8 serve them; int8 rows: from " + std::to_string(kWideRowsMinRowsI8) + " rows)";
}
inline int ksplit_stage_cap(const RouteIn& in) { return byte_rows(in.dtype) ? ks8_stage_cap(in.dp) : scan_ksplit_stage_cap(in.dp); }
inline bool ksplit_serves(const RouteIn& in, bool forced) {
    if (in.wide_rows == 0 || ksplit_stage_cap(in) < kStageMinEntries) return false;
    // int8 rows return BEFORE `forced` and wide_rows = 2 are looked at: for them force_path = 1 and wide_rows = 2 do not reach below the
    // floor as they do for fp16 and e4m3 rows (kWideRowsMinRowsI8, above: a pinned test and no measurement below it)
    if (in.dtype == VF_DTYPE_INT8) return in.n >= kWideRowsMinRowsI8;
    return forced || in.wide_rows == 2 || in.n >= (in.dtype == VF_DTYPE_FP8_E4M3 ? kWideRowsMinRows8 : kWideRowsMinRows);
}

inline bool fused_possible(const RouteIn& in, int k, bool forced = false) {
    if (in.n <= 1024 || k > kMaxKFused || k <= 0) return false;
    // corpora of up to kSmallN rows are built WITHOUT the scan copy and its inverse norms (they never take the fused path on their
    // own): forcing path 1 on one must be refused, not run on null operands (round 4: found by the option fuzz -- a memory fault)
    if (!in.has_scan) return false;
    if (ksplit_width(in.dp)) return in.n > kSmallN && ksplit_serves(in, forced);
    return true;
}

// -1: force_path = 1 on a search the fused path cannot serve
inline int route_path(const RouteIn& in, int k) {
    if (in.force_path >= 0) {
        if (in.force_path == 1 && !fused_possible(in, k, true)) return -1;
        return (int)in.force_path;
    }
    if (in.n <= kSmallN) return 0;
    return fused_possible(in, k) ? 1 : 2;
}

inline int batch_limit(int dp) {
    // 64 queries need dp * 64 * 2 bytes of LDS; fall back to 32-query passes for wide rows
    // (k_scan_ksplit's rows: 32 as well)
    return scan_lds_bytes(dp, kMaxBatch) <= (size_t)kLdsBytes ? kMaxBatch : kQueryTile;
}

// ---- the int8 row image ---------------------------------------------------------------------------------
// fp16 / fp32 rows of 768 elements in a shard of at least kImageMinRows rows get a second copy at one byte per element (plus a float per
// row): the main scan of a batch with k <= kImageMaxK reads 772 instead of 1 540 bytes per row (768 wide) and k_final's band re-score
// keeps the results those of the canonical arithmetic.  Option scan_image: 0 off, 1 auto (default: only with kImageHeadroom of device
// memory left over after it), 2 force.  A shard whose worst row leaves more than kImageMaxRho of residual keeps no image: its eps band
// would hold a large part of the corpus (a row with one huge element and the rest near zero: tests/adversarial.py).
// k and width limits: the band must fit k_final's 4 096-entry survivor area.  Measured with the first band (2 rho_max wide,
// tests/test_gpu_scan_image.py): 4M x 768, k = 256 and 4M x 1024, k = 100 overflowed it for most queries; 768, k <= 128 did not
constexpr int kImageMaxK = 128;
constexpr int64_t kImageMinRows = 4'000'000;   // measured at 10M rows; the shards of a 4- or 8-GPU split (2.5M / 1.25M rows) keep the fp16 scan
constexpr int kImageMfmaAuto = 1;   // option image_mfma = -1
// An int8 index is the image itself (build_image): nothing is built or stored twice, so scan_image = 2 takes the int8-MFMA route at any
// size the fused path serves; auto keeps kImageMinRows, where the route was measured on these very bytes (the conversion route, k_scan's
// int8 form, below that) -- no threshold of its own has been measured yet.
// (whether build_image builds one under option scan_image = mode; the memory check and the residual test are its own)
inline bool image_eligible(const RouteIn& in, int64_t mode) {
    if (in.group || in.n >= (int64_t)0xFFFFFFFFll || in.dp != 768 || scan2r_stage_cap(in.dp, kMaxBatch, kRowsI8) < kStageMinEntries) return false;
    if (in.dtype == VF_DTYPE_INT8) return in.has_scan && (mode == 2 ? in.n > kSmallN : in.n >= kImageMinRows);
    return (in.dtype == VF_DTYPE_F16 || in.dtype == VF_DTYPE_F32) && in.n >= kImageMinRows;
}

// The int8 image's certificate.  The row the scan sees is s code / ||c|| = c / ||c|| + r with ||r|| = rho_row, so its
// approximate score moves by |q16 . r| <= ||q16|| rho_row <= (1 + 2^-11)(1 + 2^-20) rho_row more than on the fp16 path, and the scan's
// fp32 sum, whose terms now add up to at most 1 + rho_row, by d 2^-24 rho_row more: off_row (k_prep_image, rounded up).  The scan adds
// off_row to every score it forms, so canonical <= key + eps holds for every row with the fp16 path's eps (+ 10^-7 for that addition's
// rounding) -- the certificate k_final tests is the fp16 path's.  What the band must hold: the k-th canonical is ~ the k-th key minus
// that row's off, so every row whose key is within eps + off of the k-th best key must be re-scored.  The band is eps + 1.5 rho_mean c
// + 2^-9 (a top-k row up to ~1.75 x the average residual); a query whose rows lie further out fails the certificate and takes the exact
// path.  Widths in threshold bins (1 / 1024) and fine bins (1 / 16 384), rounded up + one bin.
inline void image_bound(int d, int dtype, float rho_mean, float* eps, int* tau_band, int* fine_band) {
    const double u16 = 1.0 / 2048.0;
    const double base = u16 * (dtype == VF_DTYPE_F32 ? 2.0 : 1.0) + sqrt((double)d) * ldexp(1.0, -24) + 2.0 * d * ldexp(1.0, -24) + 1e-6;
    const float e = (float)(base + 1e-7);
    const double band = (double)e + 1.5 * rho_mean * (1.0 + u16) * (1.0 + ldexp(1.0, -20)) + ldexp(1.0, -9);
    *eps = e;
    *tau_band = (int)ceil(band * (kHistBins / 2)) + 1;
    *fine_band = (int)ceil(band * (kHistBins / 2) * 16) + 1;
}

// Which matrix instruction scans the image (option image_mfma): 1 = v_mfma_i32_32x32x32_i8 on the codes as they are, the
// queries quantised to one int8 plane whose residual widens each query's certificate bound and band; 0 = the codes converted to fp16
// 2 = the same on hi + lo planes (the residual quantised again at step / 254: rho_q < 10^-4, the band of 0, twice the instructions of 1)
inline RowForm image_rows(int planes) { return planes == 2 ? kRowsI8Mfma2 : (planes == 1 ? kRowsI8Mfma1 : kRowsI8); }   // k_scan2r's row form of the image scans
inline int image_planes(const RouteIn& in, int qt) {   // 0: the fp16 instruction
    const int m = in.image_mfma < 0 ? kImageMfmaAuto : (int)in.image_mfma;
    return (m >= 1 && scan2r_stage_cap(in.dp, qt, image_rows(m)) >= kStageMinEntries) ? m : 0;
}

// the int8 image serves a fused batch when it exists, k is within kImageMaxK and the scans are k_scan2r's (the options that pick another
// kernel, the tile pool or k_scan's sample pass keep the rows as stored); wide passes never reach it (route_search decides them first)
inline bool image_serves(const RouteIn& in, int k, int qt) {
    return in.has_image && k <= kImageMaxK && (in.scan_impl == 2 || in.scan_impl == 5) && !in.steal && in.sample_impl != 0 &&
           scan2r_stage_cap(in.dp, qt, kRowsI8) >= kStageMinEntries;
}

inline FusedPlan make_plan(const RouteIn& in, int k, bool image = false) {
    FusedPlan p;
    p.image = image; p.tau_band = 0; p.fine_band = 0;
    // k' = k + margin, rounded up to a multiple of 32 (whole re-score rounds of 32 row groups)
    int margin = in.margin >= 0 ? (int)in.margin : std::max(24, k / 4);
    // Rows only k_scan_ksplit serves (2560 to 4096 padded elements): the certificate needs the k-th canonical score to clear the k'-th
    // approximate score by eps, and eps grows with d (2 d 2^-24: 4.9e-4 at d = 4096, beside 2^-11 per fp16 rounding) while the scores of
    // isotropic rows crowd together like 1 / sqrt(d).  Around rank k such rows lie k z sqrt(d) to the unit of score (z = the normal
    // quantile of k / n, <= sqrt(2 ln(n / k))), so k + k / 4 leaves a gap of 1.2 to 1.8 eps at d = 3072 .. 4096 and a fifth to a third of
    // the queries of an N(0, 1) corpus failed the certificate (40 000 rows, k = 100; exact through the repair, at its price).  The margin
    // is set for an expected gap of 2.5 eps on such rows -- the sum of `margin` spacings scatters by 1 / sqrt(margin) of itself, so 2.5 is
    // four to five deviations at margin >= 40; real embeddings spread wider and need less.  A speed setting: results do not depend on it.
    const double u16 = 1.0 / 2048.0;
    const float eps_plan = (float)(u16 * (in.dtype == VF_DTYPE_F32 ? 2.0 : 1.0) + sqrt((double)in.d) * ldexp(1.0, -24) +
                                   2.0 * in.d * ldexp(1.0, -24) + 1e-6);
    if (in.margin < 0 && ksplit_width(in.dp)) {
        const double z = sqrt(2.0 * log(std::max(3.0, (double)in.n / k)));
        margin = std::max(margin, (int)ceil(2.5 * eps_plan * k * z * sqrt((double)in.d)));
    }
    p.kprime = in.margin >= 0 ? k + margin : (k + margin + 31) / 32 * 32;
    p.kprime = std::min(p.kprime, 4096);  // k_final ranks into a fixed 4096-entry LDS array (k <= kMaxKFused = 2048)
    int cap = kMaxCap;
    while (cap < 4 * p.kprime && cap < 16384) cap <<= 1;
    if (in.cap > 0) { cap = 1; while (cap < in.cap) cap <<= 1; cap = std::min(cap, 16384); }
    while (cap < 2 * p.kprime) cap <<= 1;
    p.cap = cap;
    const int64_t scan_cus = in.n_cu - route_aux_cus(in);
    int64_t wgs = std::min<int64_t>(scan_cus, std::max<int64_t>(1, in.n / 512));
    if (in.waves > 0) wgs = std::max<int64_t>(1, in.waves / (kScanThreads / 64));
    p.grid = (int)wgs;
    p.total_waves = p.grid * (kScanThreads / 64);
    // sample rows per wave of the sample pass.  Auto: 16, but 4 for shards of up to 1.1M rows -- there a batch's own chain (k_final of
    // the slot's previous batch -> host turn-around -> prep -> sample pass -> seed -> main scan; two slots in flight) is longer than
    // two scans, so a shorter sample pass shortens the step although the looser seed admits 1.7 x the candidates: configs[1]
    // (1M x 768) 0.304 -> 0.290 ms per batch; from 1.25M rows on the step is the scan's and nothing changes, at 10M the larger
    // candidate lists cost 1.7 % (profiles/r04_sample_rows_sweep.log)
    // (only while the sample still holds 16 k' rows: a top-2048 search seeds its threshold from the k'-th best sample score)
    // Round 6, one box, fresh index per setting (profiles/r06_small_sweep_*.log): 1M rows 4 / 8 / 16 per wave = 0.2965 / 0.2915-0.2951 /
    // 0.3111 ms per batch, 1.25M rows 0.3559 / 0.3515-0.3534 / 0.3539-0.3550, 1.25M x 1024 0.4447 / 0.4479 / 0.4470: 8 is level with the best
    // of the other two at every small-shard size, so it is the rule up to 1.5M rows (16 beyond: the scan hides the pass there).
    p.samp = in.sample_rows > 0 ? (int)in.sample_rows : ((in.n <= 1500000 && 8ll * p.total_waves >= 16ll * p.kprime) ? 8 : 16);
    // A query's candidate list holds about k' (1 + ln(n / sample rows)) entries -- the k'-th best of a growing prefix moves up like that --
    // times the lag of the threshold refresh (measured 1.2-1.3 at k = 100 .. 2048).  The 4 k' rule above is short of that for deep
    // searches over large shards: round 6 found the reference's own call shape, k = 2048 with one to four queries
    // (src/utils/ensembleRetriever.py:64-66), overflowing its 16384-entry lists from 1M rows up and k = 1000 its 8192 -- correct results
    // through the exact re-run, at 56-72 ms instead of 2 (5M rows).  The list is sized for 1.6 x the expectation, up to 32768 entries
    // (what the wide passes use; k_final reads the list from global memory, so its length costs HBM, not LDS).
    if (in.cap <= 0) {
        const double sample_rows = (double)p.total_waves * p.samp;
        const double expect = p.kprime * (1.0 + log(std::max(1.0, (double)in.n / std::max(1.0, sample_rows))));
        while (p.cap < (int)(1.6 * expect) && p.cap < 32768) p.cap <<= 1;
    }
    // |approx - canonical| bound (DESIGN.md "Exactness certificate").  fp16 has an 11-bit significand, so
    // round-to-nearest moves an element by at most 2^-11 of its magnitude: rounding the normalised query moves the
    // dot product by <= 2^-11 * sum|q_j c_j| <= 2^-11 (Cauchy-Schwarz, both vectors of unit norm); rounding an fp32
    // corpus row to fp16 adds the same again.  Then the fp16 subnormal floor (2^-25 per element against a unit
    // vector: sqrt(d) * 2^-24 covers it twice) and the two fp32 dot products (d * 2^-24 each).
    // (k_scan_ksplit adds a row's dp products per quarter, then across quarters: still one sum of the same terms with dp - 1 additions, and
    // d 2^-24 times the sum of their magnitudes (<= 1 + 2^-11) bounds the error of ANY order -- tests/test_wide_rows_bound.py)
    p.eps = eps_plan;
    if (image) {
        image_bound(in.d, in.dtype, in.rho_mean, &p.eps, &p.tau_band, &p.fine_band);
        p.kprime = k;
        // a list holds ~ (rows in the band) x (1 + ln(n / sample rows)) x the refresh lag -- several thousand per query on ordinary data
        // (DESIGN.md 4): the largest list the fused path has, 256 KB per query, whatever the `cap` option says (that option sizes the
        // count-based lists only); its length costs memory, not time (k_final reads what was written)
        p.cap = 32768;
    }
    return p;
}

// ---- wide passes (k_scan_wide): up to 1024 queries share ONE read of the shard --------------------------------------
constexpr int kWideMinQueries = 129;   // e4m3 rows: below this the 64-query HBM-bound passes are faster (2 of them at most)
constexpr int kWideMinQueries16 = 65;  // fp16 (and fp32 -> fp16 scan copy) rows: TWO 64-query passes cost two reads of the shard (5.2 ms at 10M x 768), one wide pass 4.2-4.3 ms (round 4, profiles/r04_wide_threshold.log)
// rows of 2560 to 4096 padded elements: k_scan_ksplit reads the shard once per 32 queries, k_scan_wide (its query operand streams through
// LDS in 32-KB chunks, so its LDS does not grow with dp; exact at these widths, checked against the oracle) once per 256 at the matrix
// rate.  1M x 2560, k = 100, ms per batch, k_scan_ksplit / k_scan_wide: 4 queries 0.974 / 1.559, 32: 0.989 / 1.576, 64 (two passes): 1.739 /
// 1.483, 128: 3.475 / 1.583; 1M x 4096: 32: 1.545 / 2.452, 64: 2.738 / 2.308, 128: 5.475 / 2.413; at 64 queries k_scan_wide is ahead at
// every measured row count from 32 768 up and at k = 2048 too (profiles/r08_wide_rows_ab.log, r08_wide_rows_threshold.log).  So the
// boundary is the second pass: up to 32 queries k_scan_ksplit, from 33 k_scan_wide.
constexpr int kWideMinQueriesKsplit = 33;
// The same boundary for e4m3 rows of these widths (profiles/r10_wide_rows_fp8_threshold.log, r10_wide_rows_fp8_ab.log): a pass of
// k_scan_ksplit8 reads half the bytes of k_scan_ksplit's, k_scan_wide (fp16 instruction on converted rows) runs at the matrix rate as
// before, so TWO 32-query passes still beat it where the rows are many -- 64 queries, k = 100, ms per batch, k_scan_ksplit8 / k_scan_wide:
// 262 144 x 2560 0.354 / 0.369, 1M x 2560 0.923 / 1.138, 262 144 x 4096 0.511 / 0.516, 1M x 4096 1.536 / 1.730 (up to 131 072 rows and at
// k = 2048 the wide pass is ahead at 64 too) -- and three never do: 65 queries 1M x 2560 1.358 / 1.138, 1M x 4096 2.282 / 1.737,
// 32 768 x 2560 0.327 / 0.195; 96 and 128 queries likewise in every cell.  So the boundary is the third pass: from 65 the wide pass.
// Paddings it does not take (dp % 256 != 0) stay on 32-query passes of k_scan_ksplit8.
// int8 rows of these widths (k_scan_ksplit8i) take the same boundary: their wide pass is k_scan_wide<MODE, 2>, the fp16 instruction on
// converted rows like the kernel the figures above were measured against (k_scan_wide8 is an fp8-instruction kernel and does not apply).
constexpr int kWideMinQueriesKsplit8 = 65;
constexpr int kWideMaxQueries = 1024;  // 4 query tiles of 256 per pass: one workgroup per CU
constexpr int kWideTile = kWideQ;   // a wide pass pads its queries to whole tiles of the kernel
inline bool wide_possible(const RouteIn& in, int nq) {
    const bool ks = ksplit_width(in.dp);   // rows only k_scan_ksplit holds an image of (32 queries per pass)
    if (in.wide == 0 || nq < (in.wide > 1 ? (int)in.wide : ks ? (byte_rows(in.dtype) ? kWideMinQueriesKsplit8 : kWideMinQueriesKsplit) : (byte_rows(in.dtype) ? kWideMinQueries : kWideMinQueries16))) return false;
    // a register stage is 2 k-chunks of fp8 rows / 1 of fp16 rows and a tile alternates two stages
    return in.dp % (byte_rows(in.dtype) ? 256 : 128) == 0;
}

inline WidePass route_wide_pass(const RouteIn& in, const FusedPlan& p, int nb) {
    WidePass w;
    w.qtot = (nb + kWideTile - 1) / kWideTile * kWideTile;
    w.jtiles = w.qtot / kWideTile;
    w.rgroups = std::max(1, in.n_cu / w.jtiles);
    w.cap = p.cap;
    if (p.kprime > 256) w.cap = std::max(w.cap, 16384);   // k ~ 1000: ~k' (1 + ln(n / sample)) candidates per query
    // k_scan_wide8 (the fp8 matrix instruction): e4m3 rows, K-tiles of 64, a row group's bytes within a 32-bit lane offset
    // Rows of 2560 to 4096 padded elements take it on request only (wide_mfma = 1), auto keeps k_scan_wide: the query's hi + lo split
    // leaves a bound eps_q that grows with the width while make_plan's margin is sized for the fp16 bound, so on N(0, 1) rows queries
    // fail the certificate (2 of 64 at 1M x 2560, 25 of 64 at 1M x 4096) and each pays an exact repair of milliseconds over 1M rows -- 64
    // queries: 9.49 ms per batch against k_scan_wide's 1.12 at 2560, 57.0 against 1.74 at 4096 (the scans themselves: 0.90 against 0.96 ms,
    // 1.93 against 1.53; profiles/r10_wide_rows_fp8_ab.log).  Exact either way.
    const bool w8 = (in.wide_mfma > 0 || (in.wide_mfma < 0 && !ksplit_width(in.dp))) && in.dtype == VF_DTYPE_FP8_E4M3 && in.dp % 64 == 0 &&
                    (in.n / w.rgroups + 2 * 256) * (int64_t)in.dp < (int64_t)0xFFFFFFFFll;
    if (w8) {
        // the query's hi + lo split leaves ||delta|| ~ 6e-4 of the query's norm (eps_q ~ 1.1e-3 at dp = 1024 against the fp16 path's
        // 6.1e-4): the plan's k' = k + k / 4 still clears it on ordinary data (the k -> k' gap is ~2.4e-3); a deeper k' (k + k / 2) was the
        // first setting and cost 14 % more candidates for nothing (profiles/r04_wide8_kprime.log)
        if (p.kprime > 256) w.cap = std::max(w.cap, 32768);
    }
    w.main = w8 ? kKernelWide8 : kKernelWide;
    w.rows = stored_rows(in.dtype);   // (int8 rows: k_scan_wide converts the biased bytes, exact; the fp8 instruction is for e4m3 codes only)
    w.samp = w.jtiles >= 2 ? 64 : 32;
    w.waves = in.wide8_waves == 4 ? 4 : 8;
    w.main_jtiles = w8 && w.waves == 4 ? (nb + 127) / 128 : w.jtiles;
    w.stage_cap = !w8 ? kWideStageCap
                      : in.wide8_stage > 0 ? (int)std::min<int64_t>(in.wide8_stage, scan_wide8_stage_cap(w.waves)) : scan_wide8_stage_cap(w.waves);
    w.refresh_every = 1;
    while (w.refresh_every * 2 <= (int)std::min<int64_t>(256, std::max<int64_t>(1, in.refresh_every))) w.refresh_every *= 2;
    const int64_t group_rows = in.n / w.rgroups, group_samp = (int64_t)w.samp * 8;
    w.clear_sample = group_rows < group_samp;
    const int64_t sampled = std::min<int64_t>(in.n, (int64_t)w.rgroups * std::min(group_samp, group_rows));
    w.scan_bytes = (in.n - sampled) * ((int64_t)in.d * (row_form_bytes(w.rows) ? 1 : 2) + 4);
    return w;
}

// The search: its path, whether wide passes serve it (chosen BEFORE the image is considered), and whether its passes read the image.
// The image and its plane count are decided once per search, with the query tile of the first pass, min(batch limit, nq) queries;
// route_batch sizes each pass's stage with that pass's own tile.
inline SearchRoute route_search(const RouteIn& in, int nq, int k) {
    SearchRoute r;
    r.path = route_path(in, k);
    r.per_pass = batch_limit(in.dp);
    if (r.path != 1) return r;
    r.wide = wide_possible(in, nq);
    if (r.wide) r.per_pass = kWideMaxQueries;
    const int qt0 = qn_tile_for(std::min(batch_limit(in.dp), nq));
    r.image = !ksplit_width(in.dp) && !r.wide && image_serves(in, k, qt0);   // (path 1 on ksplit rows: route_path found that k_scan_ksplit serves them)
    r.planes = r.image ? image_planes(in, qt0) : 0;
    r.plan = make_plan(in, k, r.image);
    return r;
}

// One pass of nb queries of search `r` (path 1, not wide): the sample pass, then the main scan.
inline BatchRoute route_batch(const RouteIn& in, const SearchRoute& r, int nb) {
    BatchRoute b;
    const FusedPlan& p = r.plan;
    const int qt = b.tile = qn_tile_for(nb);
    const bool ks = ksplit_width(in.dp);
    const int64_t steal = in.steal, scan_impl = in.scan_impl;
    // A workgroup publishes its staged candidates (and refreshes one threshold) per BLOCK of refresh_every staged entries,
    // whatever query they belong to: the option is stated for a full 64-query batch and scales with the batch's query
    // count, so that a query sees the same publication granularity at nq = 1 as at nq = 64.  (Unscaled, a single
    // query over 5M rows staged ~76 entries per workgroup, never completed a 128-entry block, never raised its
    // threshold above the sample's and overflowed its candidate list: exact re-run, 38 ms instead of 1.5.)
    // (rounded down to a power of two: the kernels find a block's number with a shift)
    b.refresh_every = (int)std::min<int64_t>(256, std::max<int64_t>(4, std::max<int64_t>(1, in.refresh_every) * nb / kMaxBatch));
    while (b.refresh_every & (b.refresh_every - 1)) b.refresh_every &= b.refresh_every - 1;
    const int64_t per_wave = in.n / p.total_waves;   // (from n >= total_waves * samp on, no wave's range is shorter than its sample)
    b.clear_sample = per_wave < p.samp;
    const int64_t sampled = std::min<int64_t>(in.n, (int64_t)p.total_waves * std::min<int64_t>(p.samp, per_wave));
    b.scan_bytes = (in.n - sampled) * (p.image ? (int64_t)in.dp + 8 : (int64_t)in.d * (byte_rows(in.dtype) ? 1 : 2) + 4);
    // sample pass: a FEW workgroups walk the sample parts of all ranges (each stages the query image once)
    // (auto: 4 workgroups per spare CU when the CU split is on, one per range otherwise)
    // Round 6: where k_scan2r's operand path is the default (scan2r_auto_width) the sample pass takes it too -- ONE workgroup per spare
    // CU, each walking the sample parts of p.grid / 32 ranges with six-segment rings: the pass is bound by what a CU keeps in flight
    // (k_scan's register-staged loads: 68-71 us for 8 rows per wave in four rounds of 128 workgroups).  sample_impl: -1 auto, 0 k_scan, 1 k_scan2r
    const bool f8rows = in.dtype == VF_DTYPE_FP8_E4M3 || p.image;   // (image rows: one byte per element, the e4m3 shapes)
    // an int8 index off the image route: k_scan's int8 form only (k_scan2 / k_scan2r convert e4m3 codes; their int8 forms are the image's)
    const bool i8conv = in.dtype == VF_DTYPE_INT8 && !p.image;
    // e4m3 rows (768 / 1024 elements) take it wherever k_scan2r is their main scan (n > 1.1M: below), whole chip or split.
    const bool r_f8_auto = f8rows && scan_impl == 2 && in.n > kScan2rMinRows && !steal && scan2r_auto_width(in.dp, true);
    const bool sample_r = p.image || (!i8conv && in.sample_impl != 0 && scan_impl != 1 && scan2r_stage_cap(in.dp, qt, f8rows ? kRowsE4m3 : kRowsF16) >= kStageMinEntries &&
                          (in.sample_impl == 1 || (!f8rows && in.masked && scan2r_auto_width(in.dp, false)) || r_f8_auto));
    if (ks) {   // one workgroup per range: each loads its share of the image once and scores its range's sample part
        b.sample = byte_rows(in.dtype) ? kKernelKsplit8 : kKernelKsplit;
        b.sample_grid = p.grid;
        b.sample_rows = stored_rows(in.dtype);
    } else if (sample_r) {
        const int64_t sg_r = in.sample_grid > 0 ? in.sample_grid : (in.masked ? route_aux_cus(in) : p.grid);
        b.sample = kKernelScan2r;
        b.sample_grid = (int)std::min<int64_t>(std::max<int64_t>(sg_r, 1), p.grid);
        b.sample_rows = p.image ? image_rows(r.planes) : (f8rows ? kRowsE4m3 : kRowsF16);
    } else {
        const int64_t sg_opt = in.sample_grid >= 0 ? in.sample_grid : (in.masked ? 4 * route_aux_cus(in) : 0);
        b.sample = kKernelScan;
        b.sample_grid = sg_opt > 0 ? (int)std::min<int64_t>(sg_opt, p.grid) : p.grid;
        b.sample_rows = stored_rows(in.dtype);
    }
    // main scan
    const RowForm f8 = in.dtype == VF_DTYPE_FP8_E4M3 ? kRowsE4m3 : kRowsF16;
    if (ks) {   // e4m3 codes: k_scan_ksplit8; int8 rows: k_scan_ksplit8i, reported as 7 too
        b.main = byte_rows(in.dtype) ? kKernelKsplit8 : kKernelKsplit;
        b.main_rows = stored_rows(in.dtype);
        b.stage_cap = ksplit_stage_cap(in);
        return b;
    }
    if (p.image) {   // the int8 row image (image_serves: k_scan2r's e4m3 shapes, stage >= 256)
        b.main = kKernelScan2r;
        b.main_rows = image_rows(r.planes);
        b.stage_cap = scan2r_stage_cap(in.dp, qt, b.main_rows);
        return b;
    }
    // k_scan2 serves fp16 rows by default; e4m3 rows only on request (scan_impl = 3, or 5 for k_scan2r's e4m3 shapes): per byte they
    // carry twice the matrix work and the same LDS-DMA issues, and with ONE wave per SIMD nothing hides either -- measured 0.53
    // (k_scan2, round 3) and 0.55-0.60 (k_scan2r, round 6: B fragments in accumulator registers, rings of six) against k_scan's
    // 0.63-0.70 of peak at 10M x 768 / 1024 fp8 (profiles/r03_f8_sweep.log, r06_fp8_scan2r_ab.log)
    const int cap2 = i8conv ? 0 : (((scan_impl == 3 || ((scan_impl == 2 || scan_impl == 4 || scan_impl == 5) && !f8)) && !steal) ? scan2_stage_cap(in.dp, qt, f8) : 0);
    // k_scan2r (round 6): part of the query image in accumulator registers, deeper rings.  fp16 rows of 768 elements, measured against
    // k_scan2 in separate processes, alternating (profiles/r06_scan2r_ab.log): the 8-GPU rank's shard (1.25M rows) 0.3469-0.3528 ms
    // per batch against 0.3538-0.3602 (2.2 % faster: a wave keeps 24 KB in flight instead of 12), 10M rows level (2.538 vs 2.548 --
    // the scan sits on the copy ceiling there), configs[1] (1M rows) 3 % SLOWER (0.303-0.315 vs 0.293-0.303: that step is the
    // prologue chain's, and the workgroup's start is 2.3 us longer).  So: auto (scan_impl = 2) takes it above 1.1M rows wherever the
    // scans run on the CU split and overlap (which, for these rows, is every size: split_limit); 5 forces it, 4 forbids it.
    // e4m3 rows (round 6, after the filter rewrite): k_scan2r was 0.55-0.60 against k_scan's 0.63-0.70 while a tile's threshold filter
    // cost a lone wave 4 500 cycles; with the filter at ~1 000 it is 0.694-0.698 against 0.627-0.656 at 10M x 768 and 0.717-0.719
    // against 0.693-0.700 at 10M x 1024 (whole chip, ordered scans; split + overlap loses 3-5 % there), +2-3 % at 1.25M rows with its
    // own sample pass, level at 1M: the same row threshold as fp16 rows, no CU-split condition (profiles/r06_after_filter_kernel_choice.log)
    const bool r_auto = scan_impl == 2 && in.n > kScan2rMinRows && scan2r_auto_width(in.dp, f8 != 0) && (f8 || (in.masked && route_overlap(in)));   // (fp16 rows: with the CU split and overlapping scans only: above)
#ifdef VF_EXPERIMENTS
    const bool dbg_r = f8 || !(in.debug & (32 | 64));   // (bits 5 / 6 are k_scan2's experiments on fp16 rows, k_scan2r's on e4m3 rows)
#else
    const bool dbg_r = true;
#endif
    const int capr = ((scan_impl == 5 || r_auto) && !steal && dbg_r && !i8conv) ? scan2r_stage_cap(in.dp, qt, f8) : 0;
    if (capr >= kStageMinEntries) {
        b.main = kKernelScan2r; b.main_rows = f8; b.stage_cap = capr;
    } else if (cap2 >= kStageMinEntries) {   // whole-line LDS-DMA loads: image + four rings + a stage of >= 256 entries fit the 160 KB
        b.main = kKernelScan2; b.main_rows = f8; b.stage_cap = cap2;
    } else {
        b.main = kKernelScan; b.main_rows = stored_rows(in.dtype); b.stage_cap = scan_stage_cap(in.dp, qt);
    }
    return b;
}

}  // namespace vf
