// vf_options.h -- the integer options of an index handle (vf_index_set_option), ONE row each: the name, the default, the accepted values
// and the message a refused value gets.  Everything that knows an option by name is generated from this table: the struct the handle
// and the scan route hold (Options; RouteIn derives from it, vf_route.h), the check-and-store behind vf_index_set_option (option_set) and
// the key list of the host-compiled route driver (tests/scan_route_driver.py).  Plain C++17: no HIP and no vf_index
// (tests/test_options.py walks every row on the CPU).  "reserve_rows" and "profile" are actions on the handle, not stored values: they
// are vf_api.hip's.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>

namespace vf {

// the text that refuses a wide_rows value quotes the route's row thresholds: vf_route.h defines it beside them
inline std::string wide_rows_refusal();

// wide8_waves: the 4-wave form of k_scan_wide8 is built under -DVF_EXPERIMENTS only
#ifdef VF_EXPERIMENTS
#define VF_OPTION_WIDE8_WAVES(X) X(wide8_waves, 8, 4, 8, 5, 7, "wide8_waves must be 8 (one 512-thread workgroup per CU, 256-query tiles: the default) or 4 (two 256-thread workgroups, 128-query tiles: measured slower, DESIGN.md 4)")
#else
#define VF_OPTION_WIDE8_WAVES(X) X(wide8_waves, 8, 8, 8, 1, 0, "wide8_waves must be 8 (the 4-wave form was measured slower and is built with -DVF_EXPERIMENTS only: DESIGN.md 4)")
#endif

// X(name, default, lo, hi, hole_lo, hole_hi, refusal): a value is accepted when it lies in [lo, hi] and outside [hole_lo, hole_hi] (1, 0: no hole).
// -1 is "auto" where an option has one; what each value does: include/veritasfi_hip.h, and for the route's options vf_route.h.
#define VF_OPTIONS(X) \
    X(force_path, -1, -1, 2, 1, 0, "force_path must be -1 (auto), 0, 1 or 2") \
    X(sample_rows, -1, -1, 64, 0, 0, "sample_rows must be -1 (auto) or in [1, 64]") \
    X(margin, -1, -1, 2048, 1, 0, "margin must be -1 (auto) or in [0, 2048]") \
    X(cap, 0, 0, 16384, 1, 0, "cap must be in [0, 16384]") \
    X(waves, 0, 0, 8 * 1024, 1, 0, "waves must be in [0, 8192]") \
    X(scan_g, 0, 0, 4, 1, 0, "scan_g must be in [0, 4]") \
    X(refresh_every, 128, 1, 256, 1, 0, "refresh_every must be in [1, 256]") \
    /* steal: cross-workgroup tile pool in the main scan (measured slower: DESIGN.md 5) */ \
    X(steal, 0, 0, 1, 1, 0, "steal must be 0 or 1") \
    /* wide: 0 never, 1 auto (from kWideMinQueries* queries: vf_route.h), > 1 = from that many queries */ \
    X(wide, 1, 0, 4096, 1, 0,"wide must be 0 (off), 1 (auto) or a query count") \
    X(wide8_stage, 0, 0, 3584, 1, 63, "wide8_stage must be 0 (auto) or 64..3584 candidate-stage entries") \
    VF_OPTION_WIDE8_WAVES(X) \
    X(wide_mfma, -1, -1, 1, 1, 0, "wide_mfma must be -1 (auto: the fp8 instruction for e4m3 rows), 0 (fp16 matrix instruction on converted rows) or 1 (the fp8 instruction on the e4m3 row bytes: k_scan_wide8)") \
    /* wide_sync: -1 siblings of a wide row group run free (default: fastest), >= 0 = the slack in super-tiles */ \
    X(wide_sync, -1, -1, 8, 1, 0, "wide_sync must be -1 (off) or a slack of 0..8 super-tiles") \
    /* aux_cus: CUs the main scan leaves to the small kernels of the other slots (0 = no split); fixed once the first slot exists */ \
    X(aux_cus, -1, -1, 128, 1, 0, "aux_cus must be -1 (auto) or in [0, 128]") \
    X(sample_grid, -1, -1, 1024, 1, 0, "sample_grid must be -1 (auto), 0 (one workgroup per range) or a workgroup count") \
    X(scan_impl, 2, 1, 5, 1, 0, "scan_impl must be 1 (k_scan), 2 (auto: k_scan2 for fp16 rows, k_scan2r where it measured faster), 3 (k_scan2 wherever it fits, e4m3 rows converted), 4 (k_scan2 for fp16 rows, never k_scan2r) or 5 (k_scan2r wherever a shape of it exists: fp16 rows of 384 / 512 / 768 / 1024 elements, e4m3 rows of 768 / 1024)") \
    X(sample_impl, -1, -1, 1, 1, 0, "sample_impl must be -1 (auto: k_scan2r's operand path for the sample pass where it exists and the CU split is on), 0 (k_scan) or 1 (k_scan2r wherever it fits)") \
    X(overlap_scans, -1, -1, 1, 1, 0, "overlap_scans must be -1 (auto), 0 or 1") \
    X(scan_image, 1, 0, 2, 1, 0, "scan_image must be 0 (off), 1 (auto: when it fits with headroom) or 2 (force)") \
    X(image_mfma, -1, -1, 2, 1, 0, "image_mfma must be -1 (auto), 0 (the int8 row image on the fp16 matrix instruction, fp16 queries), 1 (on the int8 matrix instruction, the queries as one int8 plane) or 2 (as two planes, hi + lo: the band of 0)") \
    X(wide_rows, 1, 0, 2, 1, 0, wide_rows_refusal()) \
    /* the two row counts reach the shard limit: a shard holds fewer than 2^32 - 1 rows, a subset lists at most 2^32 - 2 (vf_subset.h) */ \
    X(compact_chunk_rows, 0, 0, 0xFFFFFFFFll, 1, 0, "compact_chunk_rows must be 0 (auto: 64 MB of staging) or the destination rows a removal moves per chunk") \
    X(subset_super_rows, 0, 0, 0xFFFFFFFEll, 1, 0, "subset_super_rows must be 0 (auto: 64 MB of scores) or the listed rows a subset search scores per launch") \
    X(debug, 0, INT64_MIN, INT64_MAX, 1, 0, "")   /* bits for experiments and stamps: unchecked */

struct Options {
#define X(name, dflt, lo, hi, hole_lo, hole_hi, refusal) int64_t name = dflt;
    VF_OPTIONS(X)
#undef X
};

enum OptionResult : int { kOptionStored = 0, kOptionUnknown, kOptionRefused };

// Looks `name` up, checks `value` against its row and stores it in `o`; *msg is what vf_last_error reports of the other two outcomes.
inline OptionResult option_set(Options& o, const char* name, int64_t value, std::string* msg) {
#define X(opt, dflt, lo, hi, hole_lo, hole_hi, refusal)                                                           \
    if (strcmp(name, #opt) == 0) {                                                                                \
        if (value < (lo) || value > (hi) || (value >= (hole_lo) && value <= (hole_hi))) { *msg = refusal; return kOptionRefused; } \
        o.opt = value;                                                                                            \
        return kOptionStored;                                                                                     \
    }
    VF_OPTIONS(X)
#undef X
    *msg = std::string("vf_index_set_option: unknown option ") + name;
    return kOptionUnknown;
}

}  // namespace vf
