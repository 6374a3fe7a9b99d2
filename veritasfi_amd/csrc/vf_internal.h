// vf_internal.h -- shared between the kernel TU (vf_kernels.hip) and the C-ABI TU (vf_api.hip).
// gfx950 only.  Not part of the public ABI (that is include/veritasfi_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/veritasfi_hip.h"  // VF_DTYPE_*

#include <string>

#include "vf_ksplit_geom.h"   // + vf_scan_lds.h: the design constants, RowForm and every scan kernel's LDS budget
#include "vf_compact.h"       // the plan of a removal's row compaction
#include "vf_subset.h"        // the plan of a search over a chosen subset of rows
#include "vf_subset_multi.h"  // ... and of a batch whose queries each bring their own list
#include "vf_where.h"         // a metadata filter as a program over key columns: its checks, interpreter and output geometry

namespace vf {

// records the thread-local message vf_last_error() returns; returns `code` (defined in vf_api.hip)
int set_error(int code, const std::string& msg);

typedef unsigned long long u64;
typedef unsigned int u32;

// Every entry point that selects a device (hipSetDevice is per-thread state) puts the caller's device back on return:
// a host application that drives its own HIP / torch work on another device must not find it changed by a vf_* call.
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// ---- device helpers shared by the kernel TUs (vf_kernels.hip, vf_sparse.hip) ----------------------
// orderkey: float -> u32 whose unsigned order is the float order; a ranking key is (orderkey(score) << 32) | ~row
__device__ __forceinline__ u32 orderkey(float f) {
    f = f + 0.0f;  // -0 -> +0 so equal floats have equal keys
    const u32 b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unorderkey(u32 k) {
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// workgroup bitonic sort, descending, n a power of two, keys in LDS
__device__ __forceinline__ void bitonic_sort_desc(u64* s, int n, int tid, int nthreads) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (n >> 1); i += nthreads) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                const int hi = lo | j;
                const bool desc = (lo & k) == 0;
                const u64 a = s[lo], b = s[hi];
                if ((a < b) == desc) { s[lo] = b; s[hi] = a; }
            }
            __syncthreads();
        }
    }
}

enum ScanMode { kModeSample = 0, kModeMain = 1 };

// What a query quantised to ONE int8 plane adds to its certificate bound and to its bands (k_scan2r, F8 = 3).  The scan sees
// q' = qn + r_q with ||r_q|| = rho_q against rows c' = c / ||c|| + r_row, ||c'|| <= 1 + rho_row <= 65 / 64 (an image exists only if
// every rho_row <= 1 / 64), so |r_q . c'| <= rho_q 65 / 64: one constant per query.  It moves all of that query's keys together, so it
// widens the query's certificate bound and its re-score band by itself, rounded up: in threshold bins (1 / 1024) and fine bins (1 / 16 384).
struct Q8Bound { float eps_add; int tau_bins, fine_bins; };
__host__ __device__ inline Q8Bound image_q8_bound(float rho_q) {
    Q8Bound b;
    if (!(rho_q < 1.0f)) { b.eps_add = INFINITY; b.tau_bins = kHistBins; b.fine_bins = 16 * kHistBins; return b; }   // (a NaN too)
    const double c = (double)rho_q * (65.0 / 64.0);
    b.eps_add = (float)c;
    if ((double)b.eps_add < c) b.eps_add = nextafterf(b.eps_add, INFINITY);
    b.tau_bins = (int)ceil(c * (kHistBins / 2));
    b.fine_bins = (int)ceil(c * (kHistBins / 2) * 16);
    return b;
}
// ... and the query's certificate bound: the image's + that term + 2^-20 -- the two fp32 multiplications (row inverse, query step) and the
// offset addition that form a key of magnitude <= 1 + 2 / 64 round by 2^-24 of it each; every step here rounds up
__host__ __device__ inline float image_q8_eps(float eps_img, float eps_add) {
    const float e = nextafterf(eps_img + eps_add, INFINITY) + 0x1p-20f;
    return nextafterf(e, INFINITY);
}

// Arguments of the fused scan kernel (k_scan).  Plain struct passed by value.
struct ScanArgs {
    const char* rows;        // fp16 scan copy, row-major, row_bytes per row (dp * 2)
    const float* inv_scan;   // [n] 1 / (canonical norm * row scale): approx score = acc * inv_scan
    const float* off_scan;   // int8 image only (k_scan2r, F8 = 2 / 3): [n + 64] per-row offset added to every approximate score; else null
    const float* q_scale;    // int8 image on the int8 matrix instruction only (k_scan2r, F8 = 3): [QN] the queries' code steps s_q (launch_prep_q8); else null
    const _Float16* qimg;    // query image [dp/8][QN][8] fp16 (normalised queries, zero padded)
    long long n;             // rows in this shard
    int dp;                  // padded dim, multiple of 64
    long long row_bytes;
    int total_waves;         // TW: rows are split evenly over TW waves
    int samp;                // sample rows at the head of each wave's range
    // sample mode output
    float* s0;               // [QN][TW * samp] approx scores of the sample rows (-inf = empty)
    const long long* wg_base; // [grid] first row of each scan workgroup's range (n * wg / grid)
    // main mode state (all zeroed / seeded per batch)
    u32* cnt;                // [QN * kCntStride] candidates appended (one counter per 128-B line)
    int* tau_bin;            // [QN] current threshold bin (monotone non-decreasing)
    u32* hist;               // [QN][kHistBins] counts of appended candidates per bin
    u32* hist_coarse;        // [QN][64] the same counts per 32 fine bins
    int stage_cap;           // LDS candidate-stage entries per workgroup (main mode)
    u64* cand;               // [QN][cap] (orderkey(approx) << 32) | local row
    int cap;
    int kprime;              // k + margin: the threshold keeps >= kprime rows above it
    int tau_band;            // bins every threshold is set below the one kprime rows reach (int8 image scan: 2 eps wide); 0 = none
    const int* band_q;       // optional [QN] per-query tau_band (set for k_scan2r's int8 query planes only, F8 = 3 / 4: the plan's band + the query's own quantisation term); null = tau_band
    int refresh_every;       // recompute tau when a query's count crosses a multiple of this
    int nq;                  // real queries (<= QN); padded queries never pass
    u32* tile_cnt;           // [grid] pool counters: tiles claimed from the shared tail of each workgroup's row range (k_sel0 zeroes them); null = no stealing
    int scan_grid;           // workgroups of the main scan (k_sel0 resets that many counters)
    // wide scan (k_scan_wide): queries in the global image, 256-query tiles per pass, row groups
    int qn_total, jtiles, rgroups;
    u32* sib;                // [rgroups][4] super-tiles finished by each query-tile workgroup of a row group (zeroed per launch), or null
    int sib_slack;           // a workgroup starts super-tile t + 1 once every sibling has finished t - sib_slack
    unsigned long long* dbg; // optional [grid][8 waves][4] wall-clock stamps (debug bit 7), else null
    int debug;               // bit 0: timing experiment -- seed tau so that nothing passes (results invalid)
};

struct FinalArgs {
    const u32* cnt; const u64* cand; int cap;
    int top_cap, sel_cap;    // LDS areas of k_final (set by launch_final)
    const int* tau_bin;      // final thresholds of the scan (validity check)
    const void* rows_orig; int orig_dtype; long long orig_row_elems;  // exact rows for rescoring (VF_DTYPE_*)
    const float* norm;       // canonical norms [n]
    const float* qn;         // canonical normalised queries [nq][d] fp32
    int d; int k; int kprime; float eps;
    const float* eps_q;      // optional [nq] per-query certificate bound (k_scan_wide8: the query's own quantisation residual); null = eps
    int band;                // > 0 (int8 image scan): re-score every candidate within `band` fine bins (1 / 16 384 each) of the k-th best
                             // approximate score (kprime = k then); 0: the best kprime candidates
    const int* band_q;       // optional [nq] per-query `band` (the int8 query plane: launch_prep_q8); null = band
    long long n_rows;        // rows in the shard (certificate is moot when all were re-scored)
    long long id_offset;
    long long* out_ids; float* out_scores;   // [nq][k]
    int* flags;              // [nq] 0 = certified exact, 1 = uncertified, 2 = overflow
    u32* cand_count_out;     // [nq] copy of cnt for stats
    unsigned long long* dbg; // optional [nq][8] wall-clock stamps of the phases (debug), else null
};

// ---- launchers (defined in vf_kernels.hip) -----------------------------------------------------
hipError_t launch_prep_rows(const void* rows, int dt /* VF_DTYPE_* */, long long n, int d, int dp,
                            void* scan /*fp16 [n][dp] (fp8 / int8 rows: bytes [n][dp]); null when rows are used in place*/,
                            float* norm, float* inv_scan, hipStream_t s);
// the int8 row image of fp16 / fp32 rows (after launch_prep_rows: it reads `norm`): bytes [n][dp], inv_img [n], max relative residual (float bits)
hipError_t launch_prep_image(const void* rows, int dt, long long n, int d, int dp, const float* norm, unsigned char* img,
                             float* inv_img, float* off_img, u32* rho_max_bits, float* rho_sum, hipStream_t s);
// k_append_rows: the index build for the m rows of one append, in one launch (VF_INDEX_APPEND).  Source row i becomes row n0 + i of the
// handle's arrays, which the caller has sized for n0 + m rows at least; optional outputs are null where the handle does not hold them.
struct AppendArgs {
    const void* src;         // [m][d] of dt as the caller gave them (int8: two's complement), on the handle's device
    int dt, d, dp;
    long long n0, m;
    void* rows;              // the handle's stored rows (int8: biased bytes)
    void* scan;              // its owned scan copy [.][dp], or null (none, or the rows are scanned in place)
    float* norm; float* inv_scan;
    float* cn;               // the small-corpus cache of normalised rows, or null
    unsigned char* img;      // an OWNED int8 row image's codes, or null
    float* inv_img; float* off_img;       // the image's inverses and offsets (an int8 index: the inverses alone, img = null); null without an image
    u32* rho_max_bits; float* rho_sum;    // with `img`: largest residual of the new rows (float bits) and their sum, zeroed by the caller
};
hipError_t launch_append_rows(const AppendArgs& a, hipStream_t s);
// k_compact_rows: one step of a removal's chunk (VF_INDEX_REMOVE; the plan: vf_compact.h).  Row j = j0 + t, t < count, is read at
// src + (source(j) - src_row0) * row_bytes and written at dst + (j - dst_row0) * row_bytes, where source(j) = compact_src(j, rem, m), or j
// itself when rem is null.  The launcher picks `unit` (compact_unit) and `rows_per_block` (compact_rows_per_block).
struct CompactArgs {
    const char* src; char* dst;
    long long row_bytes, j0, count;
    const long long* rem;    // device: the sorted removed rows [m], or null
    long long m, src_row0, dst_row0;
    int unit, rows_per_block;
};
hipError_t launch_compact_rows(const void* src, void* dst, long long row_bytes, long long j0, long long count, const long long* rem /*device*/,
                               long long m, long long src_row0, long long dst_row0, hipStream_t s);
hipError_t launch_prep_queries(const float* q, int nq, int d, int dp, int qn_tile /*32 or 64*/,
                               float* qn, _Float16* qimg, hipStream_t s);
hipError_t launch_normalize_rows(const void* rows, int dt /* VF_DTYPE_* */, long long row0, long long nrows, int d,
                                 const float* norm, float* out, hipStream_t s);
hipError_t launch_normalize_rows_gather(const void* rows, int dt, const long long* sel /*device, local row numbers*/, int nsel, int d,
                                        const float* norm, float* out, hipStream_t s);
hipError_t launch_dense_dot16(const float* qn, int nq, const float* cn, long long nrows, int d,
                              float* out, long long out_stride, hipStream_t s);
// k_scan_subset: canonical scores of the listed rows alone, read as the index holds them (VF_SEARCH_SUBSET; the plan: vf_subset.h)
struct SubsetArgs {
    const void* rows; const float* norm; long long n;   // the index: rows as held (rows_orig), canonical norms, row count
    const long long* ids; long long id_base;             // the list (device; global ids, strictly ascending): row = ids[i] - id_base
    long long pos0, count;                               // the positions [pos0, pos0 + count) of the list this launch scores
    const float* qn; int nq, d;                          // canonical queries of the pass [nq][d] (k_prep_queries)
    float* scores; long long rank_rows;                  // scores[subset_score_index(i, q, nq, rank_rows)], i = position - pos0: chunk-major
};
hipError_t launch_scan_subset(const SubsetArgs& a, int dt /* VF_DTYPE_* */, hipStream_t s);
// ids[p][j] += base0 + p * rank_rows where >= 0: the parts of one ranking launch over `parts` chunks, [parts][per_part]
hipError_t launch_subset_part_base(long long* ids, long long parts, long long per_part, long long base0, long long rank_rows, hipStream_t s);
// the device form's list check: *first_bad (preset to ~0) = the lowest position that is out of [lo, hi) or not above its predecessor
hipError_t launch_subset_check(const long long* ids, long long m, long long lo, long long hi, u64* first_bad, hipStream_t s);
// ranked positions -> ids through the list (-1 stays), scores copied; nothing is written when *first_bad != ~0 (first_bad may be null)
hipError_t launch_subset_ids(const long long* pos, const float* sc, long long total, const long long* ids, const u64* first_bad,
                             long long* out_ids, float* out_scores, hipStream_t s);
// k_scan_subset_m: k_scan_subset's body behind a tile table (VF_SEARCH_SUBSETS; the plan: vf_subset_multi.h).  One launch scores every
// tile of one size class: `tiles` points at the class's first descriptor, n_rank is the class's row count.
struct SubsetMArgs {
    const void* rows; const float* norm; long long n; long long id_base;   // the index, as SubsetArgs names it
    const float* qn; int d;                                                // canonical queries of the pass, caller order [nb][d]
    float* scores;                                                         // the pass's scores: subm_score_index
    const SubmTile* tiles; int n_rank;
};
hipError_t launch_scan_subset_m(const SubsetMArgs& a, int n_tiles, int dt /* VF_DTYPE_* */, hipStream_t s);
// every referenced list checked in one launch: *first_bad (preset to ~0) = the lowest subm_check_key(list, position) refused
hipError_t launch_subset_check_m(const SubmList* lists, int n_lists, long long longest, long long lo, long long hi, u64* first_bad, hipStream_t s);
// ranked positions [nb][k] in permuted order -> the caller's rows through each query's own list; sentinels (pos >= m) and padding become
// (-1, -FLT_MAX); nothing is written when *first_bad != ~0 (first_bad may be null)
hipError_t launch_subset_ids_m(const long long* pos, const float* sc, int nb, int k, const SubmQuery* qd, const u64* first_bad,
                               long long* out_ids, float* out_scores, hipStream_t s);
// k_where_eval, k_where_scan, k_where_ids (vf_where.hip; VF_SEARCH_WHERE; the program and the geometry: vf_where.h): the filter's bitmap,
// its tile counts and their prefix, the number of passing rows and -- when `ids` is not null -- their ids, ascending.  Everything is on
// the device; the caller has validated the program (where_validate) and sized bitmap [where_bitmap_words(n)], tile_counts and tile_prefix
// [where_tiles(n, tile_rows)] and ids [>= n].
struct WhereArgs {
    const WhereColumnPtr* columns; const WhereLeaf* leaves; const uint8_t* ops; int n_ops; const int64_t* sets;
    long long n; int tile_rows;
    u32* bitmap; u32* tile_counts; long long* tile_prefix; long long* m_out;
    long long* ids; long long id_offset;
};
hipError_t launch_where(const WhereArgs& a, hipStream_t s);
hipError_t launch_sort_rows(const float* scores, long long score_stride, int nq, int n, int k,
                            long long id_base, long long* out_ids, float* out_scores, int out_stride,
                            hipStream_t s);
// The RowForm a launcher takes says how its kernel reads a row (vf_scan_lds.h); each names the forms it is built for.
hipError_t launch_scan(const ScanArgs& a, int mode, int qn_tile, int grid, int want_g /*0 = auto*/,
                       RowForm rows /* kRowsF16, kRowsE4m3, kRowsI8 */, hipStream_t s);
// two's-complement int8 rows -> the biased bytes (code + 128) an int8 index holds; in place when in == out
hipError_t launch_rebias_i8(const void* in, void* out, long long bytes, hipStream_t s);
// test hook: the scan's hardware e4m3 -> fp16 conversion over `count` codes (device pointers)
hipError_t launch_debug_cvt_e4m3(const unsigned char* in, float* out, int count, hipStream_t s);
// test hook: one v_mfma_i32_32x32x32_i8 over A [32][32], B [32][32] int8 -> C [32][32] = A B^T with k_scan2r's operand map (device pointers)
hipError_t launch_debug_mfma_i8(const signed char* A, const signed char* B, int* C, hipStream_t s);
// k_scan2: the main scan with whole-line LDS-DMA corpus loads (fp16 or e4m3 rows); a.stage_cap = scan2_stage_cap(...) >= 256
hipError_t launch_scan2(const ScanArgs& a, int qn_tile, int grid, RowForm rows /* kRowsF16, kRowsE4m3 */, hipStream_t s);
// k_scan2r: k_scan2 with part of the query image in registers and deeper rings (fp16 rows of 768 elements, e4m3 rows of 768 / 1024); scan2r_stage_cap < 256 = not this kernel
// (+ the int8 row image in its three forms: kRowsI8, kRowsI8Mfma1, kRowsI8Mfma2)
hipError_t launch_scan2r(const ScanArgs& a, int qn_tile, int grid, RowForm rows, hipStream_t s);
hipError_t launch_scan2r_sample(const ScanArgs& a, int qn_tile, int grid, RowForm rows, hipStream_t s);
// k_scan_ksplit: the fused scan of fp16 rows with 2560 <= dp <= 4096 (32 queries; the contraction split over the workgroup's four waves,
// the query image in registers + LDS); scan_ksplit_stage_cap = 0: not this kernel
hipError_t launch_scan_ksplit(const ScanArgs& a, int mode, int grid, hipStream_t s);
// k_scan_ksplit8: the same for e4m3 rows (a.row_bytes = dp; segments of 128 bytes, 5 to 8 per wave); ks8_stage_cap = 0: not this kernel
// rows: kRowsE4m3 (k_scan_ksplit8) or kRowsI8, the biased bytes of an int8 index (k_scan_ksplit8i: the same kernel on cvt8_i8b)
hipError_t launch_scan_ksplit8(const ScanArgs& a, int mode, int grid, RowForm rows, hipStream_t s);
hipError_t launch_scan_wide(const ScanArgs& a, int mode, RowForm rows /* as launch_scan's */, hipStream_t s);
// k_scan_wide8: the wide main scan on the fp8 matrix instruction (e4m3 rows; a.qimg = the hi / lo code image of launch_prep_wide8)
hipError_t launch_prep_wide8(const float* qn, int nq, int d, int dp, int qtot, unsigned char* img8, float* eps_q, hipStream_t s);
hipError_t launch_scan_wide8(const ScanArgs& a, int waves /* 8: 256-query tiles, one workgroup per CU; 4: 128-query tiles, two per CU */, hipStream_t s);
int scan_wide8_occupancy(int waves, int stage_cap);
// The int8 query plane of the image scan on the int8 matrix instruction (k_scan2r, F8 = 3): codes in the B-operand order
// [dp / 16][qn_tile][16], the code step s_q, and per query what its own quantisation residual rho_q = ||qn - s_q code|| (fp64, rounded
// up) adds: eps_q = eps_img + rho_q 65 / 64 + 2^-20 and the two bands widened by rho_q 65 / 64 in their bins (image_q8_bound).
// band_q: [2][qn_tile] ints -- threshold bins, then k_final's fine bins.
hipError_t launch_prep_q8(const float* qn, int nq, int d, int dp, int qn_tile, int planes /* 1, or 2: hi + lo, [dp / 16][2][qn_tile][16] */, signed char* img8, float* q_scale, float* eps_q, int* band_q,
                          float eps_img, int tau_band, int fine_band, hipStream_t s);
hipError_t launch_sel0(const ScanArgs& a, int qn_tile, hipStream_t s);
hipError_t launch_final(FinalArgs a, int nq, hipStream_t s);
hipError_t launch_merge_topk(const long long* ids_parts, const float* score_parts, int nparts, int nq,
                             int k, long long* ids, float* scores, hipStream_t s);
hipError_t launch_merge_topk_packed(const void* parts, int nparts, int nq, int k, long long* ids, float* scores,
                                    hipStream_t s);
hipError_t launch_fuse_rank(const float* a, const float* b, int n, float* out, long long* order,
                            hipStream_t s);
// bytes of one packed per-shard result [ids nq*k int64][scores nq*k fp32], padded to 16 so that every part of an
// all-gathered buffer keeps its int64 ids 8-byte aligned (nq*k odd would otherwise put part 1 on a 4-byte boundary)
inline long long packed_part_bytes(int nq, int k) { return ((long long)nq * k * 12 + 15) / 16 * 16; }
hipError_t scan_configure();   // sets max dynamic LDS on the scan kernels (once per process/device)

}  // namespace vf
