// vf_api.hip -- the C ABI of libveritasfi_hip.so (include/veritasfi_hip.h): handle management,
// path selection and stream orchestration around the kernels in vf_kernels.hip.
//
// Reference surface replaced: faiss.IndexFlatIP build + search behind FaissRetriever
// (src/utils/faissRetriever.py:11-38), sklearn.cosine_similarity + argsort
// (experiments/retriever/step3_mul.py:233-289), compute_similarity_mtx
// (src/utils/ensembleRetriever.py:275-279), rank_chunk fusion (src/utils/vllmManager.py:454-457).
#include "../../include/veritasfi_hip.h"
#include "vf_internal.h"
#include "vf_route.h"

#include <fcntl.h>
#include <float.h>
#include <sys/stat.h>
#include <unistd.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

using namespace vf;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int vf::set_error(int code, const std::string& msg) { return fail(code, msg); }

#define VF_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return fail(VF_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (" + __FILE__ + \
                                     ":" + std::to_string(__LINE__) + ")");                            \
    } while (0)

#define VF_TRY(expr)             \
    do {                         \
        int _rc = (expr);        \
        if (_rc != VF_OK) return _rc; \
    } while (0)

extern "C" int vf_version(void) { return VF_VERSION; }
extern "C" const char* vf_last_error(void) { return g_err.c_str(); }

extern "C" int vf_device_count(int32_t* out) {
    if (!out) return fail(VF_EINVAL, "vf_device_count: null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *out = 0; return fail(VF_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
    *out = n;
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int kSlots = 4;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return VF_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, need);
        if (e != hipSuccess) return fail(VF_ENOMEM, std::string("hipMalloc(") + std::to_string(need) + "): " + hipGetErrorString(e));
        bytes = need;
        return VF_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return (T*)p; }
};

struct HostBuf {   // pinned host staging
    void* p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return VF_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipHostMalloc(&p, need, hipHostMallocDefault);
        if (e != hipSuccess) return fail(VF_ENOMEM, std::string("hipHostMalloc(") + std::to_string(need) + "): " + hipGetErrorString(e));
        bytes = need;
        return VF_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};

struct Slot {
    hipStream_t stream = nullptr;        // everything but the main scan (any CU)
    hipStream_t scan_stream = nullptr;   // the main k_scan launches: CU-masked to the scan partition when the split is on, else == stream
    hipEvent_t ev_pro = nullptr;         // this slot's prologue (queries, sample pass, threshold seed) is done
    hipEvent_t ev_in = nullptr, ev_done = nullptr, ev_scan = nullptr;  // ev_scan: after this slot's main k_scan
    hipEvent_t ev_t[4] = {nullptr, nullptr, nullptr, nullptr};  // profile: scan begin/end, pipeline begin/end
    bool timed = false;
    int wide_launches = 0, wide_queries = 0;   // k_scan_wide main passes of the pending search / queries they served
    int scan_kernel = 0;                       // main-scan kernel of the pending search: 1 k_scan, 2 k_scan2, 3 k_scan_wide, ... 7 k_scan_ksplit8 / k_scan_ksplit8i (veritasfi_hip.h)
    int scan_image = 0;                        // 1: the pending search's scans read the int8 row image
    DevBuf qn, qimg, s0, cnt, tau, hist, hist_coarse, cand, flags, counts;   // fused-path state
    DevBuf dbg, wgbase, tilecnt, sib;
    DevBuf qimg8, epsq;                  // k_scan_wide8: hi / lo e4m3 query image, per-query certificate bounds (the image scan's int8 query plane: the same two)
    DevBuf qscale, bandq;                // ... and that plane's code steps [64] and per-query bands [2][64] (launch_prep_q8)
    int image_i8 = 0;                    // 1 / 2: the pending search's image scans run on the int8 matrix instruction with that many query planes
    int64_t wgbase_n = -1; int wgbase_grid = -1;
    DevBuf dense_s, cn_tmp, parts_ids, parts_sc, run_ids, run_sc, qsel; // exact-path scratch
    int* h_flags = nullptr;      // pinned, [max batches * 64]
    u32* h_counts = nullptr;     // pinned
    int* d_flags = nullptr;      // device views of the two above
    u32* d_counts = nullptr;
    size_t h_cap = 0;
    // pending call
    bool pending = false;
    const float* d_queries = nullptr;
    int nq = 0, k = 0, path = 0;
    int64_t* d_ids = nullptr;
    float* d_scores = nullptr;
    hipStream_t user_stream = nullptr;
};

// per-slot state of a group search: one feed stream / staging set per shard, on the shard's device
struct GroupSlot {
    std::vector<hipStream_t> feed;       // [G] on shard g's device: query copy -> shard search -> result copy home
    std::vector<hipEvent_t> ev;          // [G] result of shard g has landed in `all` on the home device
    std::vector<DevBuf> dq, blob;        // [G] queries / packed result [ids | scores] on shard g's device
    DevBuf all;                          // home device: G packed parts, the merge kernel's input
    hipEvent_t ev_in = nullptr;          // home device: the caller's stream at _begin time
    // Host-staged exchange for shards WITHOUT peer access to the home device (hipDeviceEnablePeerAccess refused, or the test hook
    // vf_debug_force_no_peer): queries home -> pinned host -> shard, packed result shard -> pinned host -> home.  Every copy is issued
    // on a stream of the device that owns the DEVICE side of it; events carry the order across devices.  Created on first use.
    hipStream_t hq_stream = nullptr;     // home device: the query copy to the host (once per search, shared by the staged shards)
    hipEvent_t ev_hq = nullptr;          // home device: the queries are in `hq`
    HostBuf hq;                          // pinned: the batch's queries
    std::vector<hipStream_t> hfeed;      // [G] home device: shard g's result, host -> `all`
    std::vector<hipEvent_t> ev_hb;       // [G] shard device: shard g's result is in hb[g]
    std::vector<hipEvent_t> ev_home;     // [G] home device: ... and has landed in `all` (what the merge waits for instead of ev[g])
    std::vector<HostBuf> hb;             // [G] pinned: shard g's packed result
    std::vector<char> staged_last;       // [G] the last search of this slot took the staged way for shard g (ev_home[g] is recorded)
    bool pending = false;
    int nq = 0, k = 0;
    int64_t* d_ids = nullptr; float* d_scores = nullptr;
    hipStream_t user = nullptr;
};

}  // namespace

struct vf_index {
    int device = 0;
    int64_t n = 0;
    int64_t cap = 0;            // rows every row-side array below has room for (>= n; == n until "reserve_rows" or an append grows them).  Arrays the
                                // handle does not own (borrowed rows, rows scanned in place) have room for n only: an append takes an owned copy first
    int d = 0, dp = 0, dtype = 0;  // dtype: how rows are HELD in HBM (VF_DTYPE_F32 / _F16 / _FP8_E4M3 / _INT8: biased bytes, code + 128)
    int64_t id_offset = 0;
    int n_cu = 256;
    int64_t aux_applied = -1;   // the CU split the first slot's streams were created with (-1: no slot yet); fixed from then on
    bool owns_rows = false;
    void* rows_orig = nullptr;        // as given (fp32 or fp16), [n][d]
    void* rows_scan = nullptr;    // fp16 [n][dp]; may alias rows_orig
    bool owns_scan = false;
    float* norm = nullptr;            // canonical norms [cap + 64]
    float* inv_scan = nullptr;        // [cap + 64]
    float* cn_cache = nullptr;        // canonical normalised rows when n <= kSmallN ([min(cap, kSmallN)][d])
    unsigned char* rows_img = nullptr;   // int8 row image [cap][dp] (fp16 / fp32 rows, option scan_image): biased codes, k_prep_image
    bool owns_img = false;            // (an int8 index IS its image: rows_img = rows_scan, not owned, residuals and offsets 0)
    float* inv_img = nullptr;         // [cap + 64] row scale / canonical norm: the image's approx score = acc x inv_img, then [cap + 64] per-row
                                      // score offsets off_img (k_prep_image; the scan adds them: DESIGN.md 4)
    float rho_max = 0.0f;             // largest relative residual ||x - s code|| / ||x|| of a row of the image (rounded up)
    float rho_mean = 0.0f;            // their average: sets the re-score band
    bool image_refused = false;       // a row left more residual than an image may hold (kImageMaxRho): appends do not try again (setting scan_image does)
    float rho_sum = 0.0f;             // ... and their sum, which appended rows add to (rho_mean = rho_sum / n, as a fresh build forms it)
    std::mutex mu;
    Slot slots[kSlots];
    Options opt;                // every integer option, at the defaults of the table they are generated from (vf_options.h)
    vf_search_stats stats{};
    bool profile = false;
    double prof_scan_ms = 0.0, prof_pipe_ms = 0.0;
    int64_t prof_launches = 0, prof_bytes = 0;
    hipEvent_t ev_span = nullptr;     // profile: the first timed main scan since the option was set began here (scan stream)
    bool span_started = false;
    bool span_slot[4] = {false, false, false, false};   // slots whose ev_t[1] (end of their latest timed scan) belongs to this span
    // host-buffer entry (vf_index_search): per-handle device staging, grown on demand, reused across calls
    DevBuf st_q, st_ids, st_sc;
    DevBuf st_add, st_rho;            // appends: the new rows on their way in (host rows, rows of another device), the image's two residual words
    DevBuf st_cmp, st_rem;            // removals: the staging buffer of the row compaction, the sorted removed rows
    bool damaged = false;             // a HIP error struck a removal after its first row had moved: searches, appends and removals are refused from then on
    // ---- group handle (vf_index_create_sharded / vf_index_group): the corpus is row-sharded over `shards`, one per
    // device; this handle owns them.  device = the HOME device: queries arrive there and the merged result lands there.
    std::vector<vf_index*> shards;
    std::vector<int> peer_ok;         // [G] 1 = home <-> shard g peer access is on in both directions (or same device)
    GroupSlot gslots[kSlots];
};

// flags / candidate counts are written by k_final straight into host-mapped pinned memory
static int ensure_pinned(Slot& s, size_t nq_total) {
    if (nq_total <= s.h_cap) return VF_OK;
    if (s.h_flags) (void)hipHostFree(s.h_flags);
    if (s.h_counts) (void)hipHostFree(s.h_counts);
    s.h_flags = nullptr; s.h_counts = nullptr; s.h_cap = 0;
    size_t cap = std::max<size_t>(nq_total, 256);
    VF_HIP(hipHostMalloc((void**)&s.h_flags, cap * sizeof(int), hipHostMallocMapped));
    VF_HIP(hipHostMalloc((void**)&s.h_counts, cap * sizeof(u32), hipHostMallocMapped));
    VF_HIP(hipHostGetDevicePointer((void**)&s.d_flags, s.h_flags, 0));
    VF_HIP(hipHostGetDevicePointer((void**)&s.d_counts, s.h_counts, 0));
    s.h_cap = cap;
    return VF_OK;
}

static int build_image(vf_index* ix, int64_t mode);
static int image_alloc(vf_index* ix, int64_t mode);
static int image_fill(vf_index* ix);

static bool known_dtype(int64_t dtype) { return dtype >= VF_DTYPE_F32 && dtype <= VF_DTYPE_INT8; }
static size_t dtype_bytes(int dtype) { return dtype == VF_DTYPE_F32 ? 4 : (dtype == VF_DTYPE_F16 ? 2 : 1); }

// What the scan route (vf_route.h) decides from: the handle's shape and options and, for the passes of a search, whether the slot's scan
// stream is CU-masked.  Every routing question below goes through this.
static RouteIn route_in(const vf_index* ix, const Slot* s = nullptr) {
    RouteIn in;
    static_cast<Options&>(in) = ix->opt;
    in.n = ix->n; in.d = ix->d; in.dp = ix->dp; in.dtype = ix->dtype; in.n_cu = ix->n_cu;
    in.has_scan = ix->rows_scan && ix->inv_scan;
    in.has_image = ix->rows_img != nullptr; in.rho_mean = ix->rho_mean;
    in.group = !ix->shards.empty();
    in.aux_applied = ix->aux_applied;
    in.masked = s && s->scan_stream && s->scan_stream != s->stream;
    return in;
}

static int build_common(vf_index* ix) {
    hipDeviceProp_t prop;
    VF_HIP(hipGetDeviceProperties(&prop, ix->device));
    ix->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    VF_HIP(scan_configure());
    const int dt = ix->dtype;
    const size_t scan_esz = byte_rows(dt) ? 1 : 2;  // fp8 / int8 rows are scanned as bytes, everything else as fp16
    ix->dp = (ix->d + 127) / 128 * 128;  // whole 128-element segment pairs: see pick_G
    ix->cap = ix->n;
    const size_t npad = (size_t)ix->cap + 64;
    VF_HIP(hipMalloc((void**)&ix->norm, npad * sizeof(float)));
    VF_HIP(hipMalloc((void**)&ix->inv_scan, npad * sizeof(float)));
    VF_HIP(hipMemset(ix->norm, 0, npad * sizeof(float)));
    VF_HIP(hipMemset(ix->inv_scan, 0, npad * sizeof(float)));
    const bool need_scan = ix->n > kSmallN;  // small corpora never run the fused scan
    void* scan_out = nullptr;
    if (need_scan) {
        if (dt != VF_DTYPE_F32 && ix->dp == ix->d && ((uintptr_t)ix->rows_orig % 16) == 0) {
            ix->rows_scan = ix->rows_orig;  // fp16 / fp8 / int8 rows of a whole number of segments are scanned in place
            ix->owns_scan = false;
        } else {
            VF_HIP(hipMalloc((void**)&ix->rows_scan, (size_t)ix->cap * ix->dp * scan_esz));
            ix->owns_scan = true;
            scan_out = ix->rows_scan;
        }
    }
    VF_HIP(launch_prep_rows(ix->rows_orig, dt, ix->n, ix->d, ix->dp, scan_out, ix->norm, ix->inv_scan, nullptr));
    VF_TRY(build_image(ix, ix->opt.scan_image));
    if (ix->n > 0 && ix->n <= kSmallN) {
        VF_HIP(hipMalloc((void**)&ix->cn_cache, (size_t)std::min<int64_t>(ix->cap, kSmallN) * ix->d * sizeof(float)));
        VF_HIP(launch_normalize_rows(ix->rows_orig, dt, 0, ix->n, ix->d, ix->norm, ix->cn_cache, nullptr));
    }
    VF_HIP(hipDeviceSynchronize());
    return VF_OK;
}

// ---- the int8 row image (when one is built and when a search reads it: vf_route.h) ----------------------------------
// A shard whose worst row leaves more than kImageMaxRho of residual keeps no image; auto (scan_image = 1) builds one only with
// kImageHeadroom of device memory left over after it.
constexpr double kImageMaxRho = 1.0 / 64;
constexpr size_t kImageHeadroom = (size_t)8 << 30;
static float* image_offsets(const vf_index* ix) { return ix->inv_img ? ix->inv_img + ix->cap + 64 : nullptr; }   // (sized by capacity: appends fill both halves in place)
static void free_image(vf_index* ix) {
    if (ix->rows_img && ix->owns_img) (void)hipFree(ix->rows_img);
    if (ix->inv_img) (void)hipFree(ix->inv_img);
    ix->rows_img = nullptr; ix->inv_img = nullptr; ix->owns_img = false; ix->rho_max = ix->rho_mean = ix->rho_sum = 0.0f;
}
static int build_image(vf_index* ix, int64_t mode) {
    if (mode == 0 || ix->rows_img || !image_eligible(route_in(ix), mode)) return VF_OK;
    const size_t ibytes = 2 * ((size_t)ix->cap + 64) * sizeof(float);   // inverses + offsets
    if (ix->dtype == VF_DTYPE_INT8) {
        // the index's own bytes are the codes: row scale 1, so inv_img = 1 / ||c|| = inv_scan; no residual, so offsets, rho_max and rho_mean
        // are 0 and the band is the certificate's own (image_bound at rho_mean = 0)
        if (hipMalloc((void**)&ix->inv_img, ibytes) != hipSuccess) {
            (void)hipGetLastError();
            ix->inv_img = nullptr;
            return mode == 2 ? fail(VF_ENOMEM, "scan_image = 2: the row inverses and offsets do not fit in device memory") : VF_OK;
        }
        VF_HIP(hipMemset(ix->inv_img, 0, ibytes));
        VF_HIP(hipMemcpy(ix->inv_img, ix->inv_scan, (size_t)ix->n * sizeof(float), hipMemcpyDeviceToDevice));
        ix->rows_img = (unsigned char*)ix->rows_scan; ix->owns_img = false;
        return VF_OK;
    }
    VF_TRY(image_alloc(ix, mode));
    return ix->rows_img ? image_fill(ix) : VF_OK;
}
// the two arrays of an owned image, sized by the handle's capacity (a removal makes this call before it moves a row, image_fill
// after).  Auto (mode 1) without the room leaves the handle without an image and succeeds.
static int image_alloc(vf_index* ix, int64_t mode) {
    const size_t ibytes = 2 * ((size_t)ix->cap + 64) * sizeof(float), bytes = (size_t)ix->cap * ix->dp;
    if (mode == 1) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return VF_OK; }
        if (free_b < bytes + ibytes + kImageHeadroom) return VF_OK;   // auto: no room, the rows as stored are scanned
    }
    ix->owns_img = true;
    if (hipMalloc((void**)&ix->rows_img, bytes) != hipSuccess || hipMalloc((void**)&ix->inv_img, ibytes) != hipSuccess) {
        (void)hipGetLastError();
        free_image(ix);
        return mode == 2 ? fail(VF_ENOMEM, "scan_image = 2: the int8 row image does not fit in device memory") : VF_OK;
    }
    return VF_OK;
}
// codes, inverses, offsets and residual statistics of the handle's n rows into the owned image's arrays; an image whose worst row
// leaves too much residual is freed again and refused
static int image_fill(vf_index* ix) {
    const size_t ibytes = 2 * ((size_t)ix->cap + 64) * sizeof(float);
    VF_TRY(ix->st_rho.ensure(2 * sizeof(u32)));
    u32* d_rho = ix->st_rho.as<u32>();   // [0] largest rho (float bits), [1] sum of rho (float)
    VF_HIP(hipMemset(d_rho, 0, 2 * sizeof(u32)));
    VF_HIP(hipMemset(ix->inv_img, 0, ibytes));
    VF_HIP(launch_prep_image(ix->rows_orig, ix->dtype, ix->n, ix->d, ix->dp, ix->norm, ix->rows_img, ix->inv_img, image_offsets(ix), d_rho,
                             (float*)(d_rho + 1), nullptr));
    u32 bits[2] = {0u, 0u};
    VF_HIP(hipMemcpy(bits, d_rho, sizeof(bits), hipMemcpyDeviceToHost));
    float rho, sum;
    memcpy(&rho, &bits[0], sizeof(rho));
    memcpy(&sum, &bits[1], sizeof(sum));
    if (!(rho <= kImageMaxRho)) { free_image(ix); ix->image_refused = true; return VF_OK; }   // (a NaN fails the test too)
    ix->rho_max = rho;
    ix->rho_sum = sum;
    ix->rho_mean = sum / (float)ix->n;
    return VF_OK;
}

// A slot's stream and events are created on its first use: a one-shot index (the reference builds one per
// select_top_chunks call, step3_mul.py:233-253) only ever touches slot 0.
static int ensure_slot(vf_index* ix, Slot& s) {
    if (s.stream) return VF_OK;
    VF_HIP(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    // CU partition ("small shards"): a main-scan workgroup owns its CU (234 VGPRs x 8 waves, 128 KB LDS), so the
    // prologue and k_final of the OTHER slots used to queue behind it.  The main scans run on a stream whose CU mask
    // leaves `aux_cus` CUs alone (mask bits interleave over the 8 XCDs: bits [0, n_cu - aux) = all but the last aux / 8 CUs
    // of every XCD; tools/ubench/cu_mask_probe.hip); everything else runs on an unmasked stream and finds those CUs free.
    s.scan_stream = s.stream;
    int64_t aux = route_aux_cus(route_in(ix));
    if (aux) {
        const int words = (ix->n_cu + 31) / 32;
        std::vector<uint32_t> mask(words, 0u);
        for (int b = 0; b < ix->n_cu - (int)aux; ++b) mask[b / 32] |= 1u << (b % 32);
        hipStream_t ms = nullptr;
        if (hipExtStreamCreateWithCUMask(&ms, (uint32_t)words, mask.data()) == hipSuccess && ms) s.scan_stream = ms;
        else { (void)hipGetLastError(); if (ix->aux_applied < 0) aux = 0; }   // no CU masking on this stack: one stream, whole-chip grids
    }
    // the split is a property of the streams: plans, stats and the overlap decision use what was APPLIED here, whatever the
    // option is set to later (vf_index_set_option rejects a change once slots exist)
    if (ix->aux_applied < 0) ix->aux_applied = aux;
    VF_HIP(hipEventCreateWithFlags(&s.ev_in, hipEventDisableTiming));
    VF_HIP(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    VF_HIP(hipEventCreateWithFlags(&s.ev_scan, hipEventDisableTiming));
    VF_HIP(hipEventCreateWithFlags(&s.ev_pro, hipEventDisableTiming));
    for (int e = 0; e < 4; ++e) VF_HIP(hipEventCreate(&s.ev_t[e]));
    return VF_OK;
}

static void destroy_index(vf_index* ix) {
    if (!ix) return;
    if (!ix->shards.empty()) {  // group handle: per-slot staging on every shard's device, then the shards themselves
        for (int i = 0; i < kSlots; ++i) {
            GroupSlot& gs = ix->gslots[i];
            for (size_t g = 0; g < ix->shards.size(); ++g) {
                (void)hipSetDevice(ix->shards[g]->device);
                (void)hipDeviceSynchronize();
                if (g < gs.dq.size()) gs.dq[g].release();
                if (g < gs.blob.size()) gs.blob[g].release();
                if (g < gs.feed.size() && gs.feed[g]) (void)hipStreamDestroy(gs.feed[g]);
                if (g < gs.ev.size() && gs.ev[g]) (void)hipEventDestroy(gs.ev[g]);
                if (g < gs.ev_hb.size() && gs.ev_hb[g]) (void)hipEventDestroy(gs.ev_hb[g]);
                if (g < gs.hb.size()) gs.hb[g].release();
            }
            (void)hipSetDevice(ix->device);
            gs.all.release();
            gs.hq.release();
            for (hipStream_t st : gs.hfeed) if (st) (void)hipStreamDestroy(st);
            for (hipEvent_t ev : gs.ev_home) if (ev) (void)hipEventDestroy(ev);
            if (gs.hq_stream) (void)hipStreamDestroy(gs.hq_stream);
            if (gs.ev_hq) (void)hipEventDestroy(gs.ev_hq);
            if (gs.ev_in) (void)hipEventDestroy(gs.ev_in);
        }
        for (vf_index* sh : ix->shards) destroy_index(sh);
        ix->shards.clear();
    }
    (void)hipSetDevice(ix->device);
    (void)hipDeviceSynchronize();
    ix->st_q.release(); ix->st_ids.release(); ix->st_sc.release(); ix->st_add.release(); ix->st_rho.release(); ix->st_cmp.release(); ix->st_rem.release();
    for (int i = 0; i < kSlots; ++i) {
        Slot& s = ix->slots[i];
        DevBuf* bufs[] = {&s.qn, &s.qimg, &s.s0, &s.cnt, &s.tau, &s.hist, &s.hist_coarse, &s.cand, &s.flags, &s.counts, &s.dense_s,
                          &s.cn_tmp, &s.parts_ids, &s.parts_sc, &s.run_ids, &s.run_sc, &s.qsel, &s.dbg, &s.wgbase, &s.tilecnt, &s.sib};
        for (DevBuf* b : bufs) b->release();
        if (s.h_flags) (void)hipHostFree(s.h_flags);
        if (s.h_counts) (void)hipHostFree(s.h_counts);
        if (s.scan_stream && s.scan_stream != s.stream) (void)hipStreamDestroy(s.scan_stream);
        if (s.stream) (void)hipStreamDestroy(s.stream);
        if (s.ev_pro) (void)hipEventDestroy(s.ev_pro);
        if (s.ev_in) (void)hipEventDestroy(s.ev_in);
        if (s.ev_done) (void)hipEventDestroy(s.ev_done);
        if (s.ev_scan) (void)hipEventDestroy(s.ev_scan);
        for (int e = 0; e < 4; ++e) if (s.ev_t[e]) (void)hipEventDestroy(s.ev_t[e]);
    }
    if (ix->owns_scan && ix->rows_scan) (void)hipFree(ix->rows_scan);
    if (ix->owns_rows && ix->rows_orig) (void)hipFree(ix->rows_orig);
    if (ix->norm) (void)hipFree(ix->norm);
    if (ix->inv_scan) (void)hipFree(ix->inv_scan);
    if (ix->cn_cache) (void)hipFree(ix->cn_cache);
    if (ix->rows_img && ix->owns_img) (void)hipFree(ix->rows_img);
    if (ix->inv_img) (void)hipFree(ix->inv_img);
    if (ix->ev_span) (void)hipEventDestroy(ix->ev_span);
    delete ix;
}

// adopt: the device rows are the caller's own fresh allocation, handed over (the file loader): int8 rows are re-biased in place
static int create_impl(vf_index** out, const void* rows, bool rows_on_device, int64_t n, int32_t d, int32_t dtype,
                       int32_t device_id, int64_t id_offset, bool adopt = false) {
    if (!out) return fail(VF_EINVAL, "vf_index_create: null out");
    *out = nullptr;
    if (n < 0 || d <= 0 || (n > 0 && !rows)) return fail(VF_EINVAL, "vf_index_create: bad rows/n/d");
    if (!known_dtype(dtype)) return fail(VF_EINVAL, "vf_index_create: unknown dtype");
    if (n >= (int64_t)0xFFFFFFFFll) return fail(VF_EUNSUPPORTED, "vf_index_create: more than 2^32-1 rows per shard");
    int ndev = 0;
    VF_HIP(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(VF_EINVAL, "vf_index_create: bad device_id");
    VF_HIP(hipSetDevice(device_id));
    vf_index* ix = new (std::nothrow) vf_index();
    if (!ix) return fail(VF_ENOMEM, "vf_index_create: host allocation failed");
    ix->device = device_id; ix->n = n; ix->d = d; ix->id_offset = id_offset;
    ix->dtype = dtype;  // fp8 (OCP e4m3) rows stay fp8 in HBM: scanned as bytes, converted in registers
    const size_t esz = dtype_bytes(dtype);
    int rc = VF_OK;
    if (rows_on_device && dtype == VF_DTYPE_INT8 && !adopt && n > 0) {
        // int8 rows are held re-biased (code + 128), so the caller's device rows are copied, not borrowed: one pass, device to device
        hipError_t e = hipMalloc(&ix->rows_orig, (size_t)n * d);
        if (e != hipSuccess) rc = fail(VF_ENOMEM, std::string("hipMalloc(corpus): ") + hipGetErrorString(e));
        else {
            ix->owns_rows = true;
            e = launch_rebias_i8(rows, ix->rows_orig, (long long)n * d, nullptr);
            if (e != hipSuccess) rc = fail(VF_EHIP, std::string("re-biasing the int8 rows: ") + hipGetErrorString(e));
        }
    } else if (rows_on_device) {
        ix->rows_orig = const_cast<void*>(rows);
        ix->owns_rows = false;
        if (dtype == VF_DTYPE_INT8 && n > 0) {   // (adopt: the loader's own buffer, in place)
            const hipError_t e = launch_rebias_i8(ix->rows_orig, ix->rows_orig, (long long)n * d, nullptr);
            if (e != hipSuccess) rc = fail(VF_EHIP, std::string("re-biasing the int8 rows: ") + hipGetErrorString(e));
        }
    } else if (n > 0) {
        hipError_t e = hipMalloc(&ix->rows_orig, (size_t)n * d * esz);
        if (e != hipSuccess) rc = fail(VF_ENOMEM, std::string("hipMalloc(corpus): ") + hipGetErrorString(e));
        else {
            ix->owns_rows = true;
            e = hipMemcpy(ix->rows_orig, rows, (size_t)n * d * esz, hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = fail(VF_EHIP, std::string("hipMemcpy(corpus): ") + hipGetErrorString(e));
            else if (dtype == VF_DTYPE_INT8) {
                e = launch_rebias_i8(ix->rows_orig, ix->rows_orig, (long long)n * d, nullptr);
                if (e != hipSuccess) rc = fail(VF_EHIP, std::string("re-biasing the int8 rows: ") + hipGetErrorString(e));
            }
        }
    }
    if (rc == VF_OK) rc = build_common(ix);
    if (rc != VF_OK) { std::string keep = g_err; destroy_index(ix); g_err = keep; return rc; }
    *out = ix;
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------
// Appends (VF_INDEX_APPEND; DESIGN.md "Appending rows").  IndexFlatIP.add on an index that exists (src/utils/faissRetriever.py:18-24,
// fed in batches of 100 by src/load_data.py:98-128): the new rows are prepared by ONE kernel over them alone (k_append_rows) into the
// room behind row n of every array the handle holds, and the row count is raised last -- a search reads rows below n only, so a failure
// on the way leaves the handle as it was.  After it the handle is what vf_index_create over all the rows would have built: the
// transitions a fresh build makes at a row count (the scan copy instead of the small-corpus cache above kSmallN, the int8 row image at
// its threshold) are made when an append crosses it, and an image is dropped when a new row leaves more residual than it may hold.
// ------------------------------------------------------------------------------------------------
constexpr int64_t kMaxShardRows = 0xFFFFFFFFll;   // a shard holds fewer rows than this (candidate keys carry 32-bit row numbers)
// what every search, append and removal answers once a removal has failed half-way (remove_run)
static const char* kDamagedMsg = "the index was damaged by a HIP error in the middle of a removal (VF_INDEX_REMOVE): only vf_index_destroy works on it";

static bool search_pending(const vf_index* ix) {
    for (const Slot& s : ix->slots) if (s.pending) return true;
    for (const GroupSlot& g : ix->gslots) if (g.pending) return true;
    for (const vf_index* sh : ix->shards) if (search_pending(sh)) return true;
    return false;
}

// Every row-side array of the handle re-allocated for new_cap rows, its n rows copied device to device; borrowed rows (and rows scanned
// in place) become the handle's own copy.  The new arrays are complete before an old one is freed: on a failure they are freed and the
// handle is as it was.  The handle's device is current.
static int regrow(vf_index* ix, int64_t new_cap) {
    const size_t esz = dtype_bytes(ix->dtype), scan_esz = byte_rows(ix->dtype) ? 1 : 2;
    const size_t n = (size_t)ix->n, npad = (size_t)new_cap + 64, d = (size_t)ix->d, dp = (size_t)ix->dp;
    const bool scan_owned = ix->rows_scan && ix->owns_scan, scan_alias = ix->rows_scan && !ix->owns_scan;
    const bool img_owned = ix->rows_img && ix->owns_img, img_alias = ix->rows_img && !ix->owns_img;
    void *rows = nullptr, *scan = nullptr, *norm = nullptr, *inv = nullptr, *cn = nullptr, *img = nullptr, *iimg = nullptr;
    struct Want { void** p; size_t bytes; bool on; const void* from; size_t copy; bool zero; };
    const Want want[] = {
        {&rows, (size_t)new_cap * d * esz, true, ix->rows_orig, n * d * esz, false},
        {&scan, (size_t)new_cap * dp * scan_esz, scan_owned, ix->rows_scan, n * dp * scan_esz, false},
        {&norm, npad * sizeof(float), true, ix->norm, n * sizeof(float), true},            // (the zeroed tail of 64 and the room between)
        {&inv, npad * sizeof(float), true, ix->inv_scan, n * sizeof(float), true},
        {&cn, (size_t)std::min<int64_t>(new_cap, kSmallN) * d * sizeof(float), ix->cn_cache != nullptr, ix->cn_cache, n * d * sizeof(float), false},
        {&img, (size_t)new_cap * dp, img_owned, ix->rows_img, n * dp, false},
        {&iimg, 2 * npad * sizeof(float), ix->inv_img != nullptr, ix->inv_img, n * sizeof(float), true},
    };
    hipError_t e = hipSuccess;
    bool no_mem = false;
    for (const Want& w : want) {
        if (!w.on || e != hipSuccess) continue;
        e = hipMalloc(w.p, w.bytes);
        if (e != hipSuccess) { no_mem = true; *w.p = nullptr; break; }
        if (w.zero) e = hipMemsetAsync(*w.p, 0, w.bytes, nullptr);
        if (e == hipSuccess && w.copy && w.from) e = hipMemcpyAsync(*w.p, w.from, w.copy, hipMemcpyDeviceToDevice, nullptr);
    }
    if (e == hipSuccess && iimg && n)   // the offsets half starts behind the inverses' capacity, old and new
        e = hipMemcpyAsync((float*)iimg + npad, image_offsets(ix), n * sizeof(float), hipMemcpyDeviceToDevice, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();   // the copies are done, and so is every reader of the old arrays
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (const Want& w : want) if (*w.p) (void)hipFree(*w.p);
        return no_mem ? fail(VF_ENOMEM, std::string("growing the index to ") + std::to_string(new_cap) + " rows: " + hipGetErrorString(e))
                      : fail(VF_EHIP, std::string("growing the index: ") + hipGetErrorString(e));
    }
    if (ix->owns_rows && ix->rows_orig) (void)hipFree(ix->rows_orig);
    ix->rows_orig = rows; ix->owns_rows = true;
    if (scan_owned) { (void)hipFree(ix->rows_scan); ix->rows_scan = scan; }
    else if (scan_alias) ix->rows_scan = rows;   // still scanned in place: hipMalloc's alignment serves the scan
    (void)hipFree(ix->norm); ix->norm = (float*)norm;
    (void)hipFree(ix->inv_scan); ix->inv_scan = (float*)inv;
    if (ix->cn_cache) { (void)hipFree(ix->cn_cache); ix->cn_cache = (float*)cn; }
    if (img_owned) { (void)hipFree(ix->rows_img); ix->rows_img = (unsigned char*)img; }
    else if (img_alias) ix->rows_img = (unsigned char*)ix->rows_scan;
    if (ix->inv_img) { (void)hipFree(ix->inv_img); ix->inv_img = (float*)iimg; }
    ix->cap = new_cap;
    return VF_OK;
}

// m > 0 rows onto a plain handle: its mutex is held, no search is pending, n + m is in range.  src_device < 0: host rows.
static int append_rows(vf_index* ix, const void* rows, int src_device, int64_t m) {
    const int dt = ix->dtype;
    const int64_t n0 = ix->n, n1 = n0 + m;
    const size_t esz = dtype_bytes(dt), scan_esz = byte_rows(dt) ? 1 : 2;
    VF_HIP(hipSetDevice(ix->device));
    // room: 1.5 x the capacity at least, so that a run of appends without "reserve_rows" copies each row a bounded number of times
    if (!ix->owns_rows || n1 > ix->cap) VF_TRY(regrow(ix, std::max<int64_t>(n1, std::min<int64_t>(ix->cap + ix->cap / 2, kMaxShardRows - 1))));
    const void* src = rows;
    if (src_device != ix->device) {
        const size_t bytes = (size_t)m * ix->d * esz;
        VF_TRY(ix->st_add.ensure(bytes));
        if (src_device < 0) VF_HIP(hipMemcpy(ix->st_add.p, rows, bytes, hipMemcpyHostToDevice));
        else VF_HIP(hipMemcpyPeer(ix->st_add.p, ix->device, rows, src_device, bytes));
        src = ix->st_add.p;
    }
    // crossing kSmallN upward: the handle was built without the operands of the fused scan; a fresh build has them
    const bool cross = n0 <= kSmallN && n1 > kSmallN && !ix->rows_scan;
    const bool scan_in_place = dt != VF_DTYPE_F32 && ix->dp == ix->d;   // (the rows are the handle's own allocation by now: aligned)
    void* new_scan = nullptr;
    if (cross && !scan_in_place && hipMalloc(&new_scan, (size_t)ix->cap * ix->dp * scan_esz) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VF_ENOMEM, "append: the scan copy does not fit in device memory");
    }
    // (a handle created empty holds no small-corpus cache yet; a fresh build of these rows would)
    float* new_cn = nullptr;
    if (n0 == 0 && n1 <= kSmallN && !ix->cn_cache &&
        hipMalloc((void**)&new_cn, (size_t)std::min<int64_t>(ix->cap, kSmallN) * ix->d * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(VF_ENOMEM, "append: the cache of normalised rows does not fit in device memory");
    }
    auto drop_new = [&]() { if (new_scan) (void)hipFree(new_scan); if (new_cn) (void)hipFree(new_cn); };
    AppendArgs a{};
    a.src = src; a.dt = dt; a.d = ix->d; a.dp = ix->dp; a.n0 = n0; a.m = m;
    a.rows = ix->rows_orig; a.scan = (ix->rows_scan && ix->owns_scan) ? ix->rows_scan : nullptr;
    a.norm = ix->norm; a.inv_scan = ix->inv_scan;
    a.cn = new_cn ? new_cn : ((ix->cn_cache && n1 <= kSmallN) ? ix->cn_cache : nullptr);
    hipError_t e = hipSuccess;
    if (ix->rows_img) {
        a.inv_img = ix->inv_img; a.off_img = image_offsets(ix);
        if (ix->owns_img) {
            int rc = ix->st_rho.ensure(2 * sizeof(u32));
            if (rc != VF_OK) { drop_new(); return rc; }
            a.img = ix->rows_img; a.rho_max_bits = ix->st_rho.as<u32>(); a.rho_sum = (float*)(a.rho_max_bits + 1);
            e = hipMemsetAsync(ix->st_rho.p, 0, 2 * sizeof(u32), nullptr);
        }
    }
    if (e == hipSuccess) e = launch_append_rows(a, nullptr);
    // (the scan copy of ALL rows: one pass of the create-time kernel, which writes the norms it wrote before)
    if (e == hipSuccess && new_scan) e = launch_prep_rows(ix->rows_orig, dt, n1, ix->d, ix->dp, new_scan, ix->norm, ix->inv_scan, nullptr);
    u32 bits[2] = {0u, 0u};
    if (e == hipSuccess) e = a.img ? hipMemcpy(bits, ix->st_rho.p, sizeof(bits), hipMemcpyDeviceToHost) : hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        drop_new();
        return fail(VF_EHIP, std::string("append: ") + hipGetErrorString(e));
    }
    // commit: the rows exist from here on
    float* old_cn = ix->cn_cache;
    ix->n = n1;
    if (new_cn) ix->cn_cache = new_cn;
    if (cross) {
        ix->rows_scan = new_scan ? new_scan : ix->rows_orig; ix->owns_scan = new_scan != nullptr;
        ix->cn_cache = nullptr;
    }
    if (a.img) {
        float rho, sum;
        memcpy(&rho, &bits[0], sizeof(rho));
        memcpy(&sum, &bits[1], sizeof(sum));
        if (!(rho <= kImageMaxRho)) { free_image(ix); ix->image_refused = true; }   // a fresh build would have refused the image (a NaN fails the test too)
        else { ix->rho_max = std::max(ix->rho_max, rho); ix->rho_sum += sum; ix->rho_mean = ix->rho_sum / (float)ix->n; }
    }
    // the image a fresh build of this many rows would hold (it appears at a row count: image_eligible)
    if (!ix->rows_img && !ix->image_refused) {
        const int rc = build_image(ix, ix->opt.scan_image);
        if (rc != VF_OK) {   // back to the handle as it was
            const std::string keep = g_err;
            free_image(ix);
            ix->n = n0;
            if (new_cn) { (void)hipFree(new_cn); ix->cn_cache = nullptr; }
            if (cross) { ix->rows_scan = nullptr; ix->owns_scan = false; ix->cn_cache = old_cn; if (new_scan) (void)hipFree(new_scan); }
            g_err = keep;
            return rc;
        }
    }
    if (cross && old_cn) (void)hipFree(old_cn);
    if (ix->st_add.bytes > ((size_t)64 << 20)) ix->st_add.release();
    return VF_OK;
}

// vf_index_create / vf_index_create_device with VF_INDEX_APPEND in `dtype`.  Every argument error is reported before the first HIP call.
static int append_entry(vf_index** out, const void* rows, bool rows_on_device, int64_t n, int32_t d, int32_t dtype, int32_t device_id) {
    if (!out) return fail(VF_EINVAL, "vf_index_create: null out");
    const int32_t base = dtype & ~VF_INDEX_APPEND;
    if (!known_dtype(base)) return fail(VF_EINVAL, "vf_index_create: unknown dtype");
    if (n < 0 || d <= 0 || (n > 0 && !rows)) return fail(VF_EINVAL, "vf_index_create: bad rows/n/d");
    vf_index* ix = *out;
    if (!ix) return fail(VF_EINVAL, "vf_index_create: VF_INDEX_APPEND needs a live handle in *out");
    if (d != ix->d || base != ix->dtype)
        return fail(VF_EINVAL, "vf_index_create: VF_INDEX_APPEND: d and dtype must be the handle's (" + std::to_string(ix->d) + ", " + std::to_string(ix->dtype) + ")");
    if (device_id != ix->device) return fail(VF_EINVAL, "vf_index_create: VF_INDEX_APPEND: device_id must be the handle's device " + std::to_string(ix->device));
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->damaged) return fail(VF_EHIP, std::string("vf_index_create: VF_INDEX_APPEND: ") + kDamagedMsg);
    if (search_pending(ix)) return fail(VF_EINVAL, "vf_index_create: VF_INDEX_APPEND: search pending (a slot is between _begin and _end)");
    if (n == 0) return VF_OK;
    vf_index* target = ix->shards.empty() ? ix : ix->shards.back();   // a group: the rows go to its last shard, ids stay one range
    if (target->n + n >= kMaxShardRows) return fail(VF_EUNSUPPORTED, "vf_index_create: VF_INDEX_APPEND: more than 2^32-1 rows per shard");
    DeviceGuard restore_callers_device;
    const int src_device = rows_on_device ? device_id : -1;
    if (target == ix) return append_rows(ix, rows, src_device, n);
    std::lock_guard<std::mutex> lk(target->mu);
    VF_TRY(append_rows(target, rows, src_device, n));
    ix->n += n;
    return VF_OK;
}

// option "reserve_rows": room for `total` rows now, so that appends up to it move nothing (a group: in its last shard, where they go)
static int reserve_rows(vf_index* ix, int64_t total) {
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->damaged) return fail(VF_EHIP, std::string("reserve_rows: ") + kDamagedMsg);
    vf_index* target = ix->shards.empty() ? ix : ix->shards.back();
    if (target != ix) total -= ix->n - target->n;
    if (total >= kMaxShardRows) return fail(VF_EUNSUPPORTED, "reserve_rows: more than 2^32-1 rows per shard");
    if (total <= target->n) return VF_OK;
    if (search_pending(ix)) return fail(VF_EINVAL, "reserve_rows cannot change while a search is pending");
    std::unique_lock<std::mutex> lk;
    if (target != ix) lk = std::unique_lock<std::mutex>(target->mu);
    if (target->owns_rows && total <= target->cap) return VF_OK;
    DeviceGuard restore_callers_device;
    VF_HIP(hipSetDevice(target->device));
    return regrow(target, std::max(total, target->cap));
}

// ------------------------------------------------------------------------------------------------
// Removals (VF_INDEX_REMOVE; DESIGN.md 3.2 "Removing rows").  IndexFlat.remove_ids on a live index: the rows leave and every later
// row moves down, so ids stay the positions 0 .. n - 1 (what src/utils/ensembleRetriever.py:76 indexes its metadata with).  After it
// the handle is what vf_index_create over the remaining rows would have built.  A removal has two parts.  remove_prepare makes every
// allocation the call needs and changes nothing a search could see (a handle that borrows its rows takes its own copy, as an append
// does); a failure there leaves the handle as it was.  remove_run moves the rows (k_compact_rows, chunk by chunk through a staging
// buffer: vf_compact.h), brings every derived array to the bits of a fresh build, makes the transitions a fresh build makes at the
// new row count and lowers the row count; a HIP error there cannot be undone and marks the handle damaged.
//   rows_orig, an owned scan copy, norm, inv_scan: compacted by the mover -- each entry depends on its own row alone, so the moved
//   bits are the bits a fresh build computes.  The cache of normalised rows (n <= kSmallN) is small by definition: the create-time
//   kernel rewrites it from the first removed row on.  An owned int8 image is rebuilt by the create-time kernel on the rows that remain
//   (its residual statistics are sums and maxima over all rows); an int8 index copies its inverses from inv_scan.
// ------------------------------------------------------------------------------------------------
namespace {
enum ImageStep { kImageNone = 0, kImageDrop, kImageAlias, kImageRefill, kImageNew };
struct RemovePrep {
    vf_index* ix = nullptr;
    std::vector<long long> rem;        // the rows that leave: local row numbers, ascending, distinct, not empty
    CompactPlan plan{};
    bool to_small = false;             // the row count crosses kSmallN downward: the scan copy goes, the cache of normalised rows comes
    bool scan_moves = false;           // an owned scan copy that stays
    int image = kImageNone;
    float* new_cn = nullptr;           // allocations the commit hands to the handle
    unsigned char* new_img = nullptr;
    float* new_iimg = nullptr;
    void release() {
        if (new_cn) (void)hipFree(new_cn);
        if (new_img) (void)hipFree(new_img);
        if (new_iimg) (void)hipFree(new_iimg);
        new_cn = nullptr; new_img = nullptr; new_iimg = nullptr;
    }
};
}  // namespace


// p.ix (a plain handle: its mutex is held, no search is pending) and p.rem are set
static int remove_prepare(RemovePrep& p) {
    vf_index* ix = p.ix;
    const int64_t n0 = ix->n, m = (int64_t)p.rem.size(), n1 = n0 - m;
    const size_t esz = dtype_bytes(ix->dtype), scan_esz = byte_rows(ix->dtype) ? 1 : 2;
    VF_HIP(hipSetDevice(ix->device));
    VF_HIP(hipDeviceSynchronize());   // every reader of the arrays is done
    if (!ix->owns_rows) VF_TRY(regrow(ix, ix->cap));   // the caller's memory is never written
    p.to_small = n0 > kSmallN && n1 <= kSmallN;
    p.scan_moves = ix->rows_scan && ix->owns_scan && !p.to_small;
    long long widest = (long long)ix->d * (long long)esz;
    if (p.scan_moves) widest = std::max(widest, (long long)ix->dp * (long long)scan_esz);
    p.plan = compact_plan(n0, m, p.rem[0], ix->opt.compact_chunk_rows > 0 ? ix->opt.compact_chunk_rows : compact_auto_rows(widest));
    if (p.plan.chunks) {
        VF_TRY(ix->st_cmp.ensure((size_t)p.plan.chunk_rows * (size_t)widest));
        VF_TRY(ix->st_rem.ensure((size_t)m * sizeof(long long)));
    }
    if (n1 > 0 && n1 <= kSmallN && !ix->cn_cache &&
        hipMalloc((void**)&p.new_cn, (size_t)std::min<int64_t>(ix->cap, kSmallN) * ix->d * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        p.new_cn = nullptr;
        return fail(VF_ENOMEM, "remove: the cache of normalised rows does not fit in device memory");
    }
    // the image a fresh build of the remaining rows would hold
    RouteIn in = route_in(ix);
    in.n = n1; in.has_scan = in.has_scan && !p.to_small;
    const bool eligible = ix->opt.scan_image != 0 && image_eligible(in, ix->opt.scan_image);
    if (ix->rows_img) p.image = !eligible ? kImageDrop : ix->owns_img ? kImageRefill : kImageAlias;
    else if (eligible && ix->dtype != VF_DTYPE_INT8) {   // (it had refused its image, or had found no room for it)
        int rc = image_alloc(ix, ix->opt.scan_image);
        p.new_img = ix->rows_img; p.new_iimg = ix->inv_img;   // kept aside until the rows have moved
        ix->rows_img = nullptr; ix->inv_img = nullptr; ix->owns_img = false;
        if (rc != VF_OK) { p.release(); return rc; }
        if (p.new_img) p.image = kImageNew;
    }
    if (p.image == kImageRefill || p.image == kImageNew) {
        const int rc = ix->st_rho.ensure(2 * sizeof(u32));
        if (rc != VF_OK) { p.release(); return rc; }
    }
    return VF_OK;
}

static int remove_run(RemovePrep& p) {
    vf_index* ix = p.ix;
    const int dt = ix->dtype;
    const int64_t n0 = ix->n, m = (int64_t)p.rem.size(), n1 = n0 - m, first = p.plan.first;
    const size_t esz = dtype_bytes(dt), scan_esz = byte_rows(dt) ? 1 : 2;
    hipError_t e = hipSetDevice(ix->device);
    const long long* d_rem = ix->st_rem.as<long long>();
    if (e == hipSuccess && p.plan.chunks) e = hipMemcpy(ix->st_rem.p, p.rem.data(), (size_t)m * sizeof(long long), hipMemcpyHostToDevice);
    if (e != hipSuccess) {   // nothing has moved yet
        p.release();
        return fail(VF_EHIP, std::string("remove: ") + hipGetErrorString(e));
    }
    // ---- from here on a failure cannot be undone ----
    // Each array moves under a plan of its own: what the staging buffer (sized for the widest array's chunk) holds of ITS rows, so the
    // 4-byte arrays go in one chunk where the rows take many.  Option compact_chunk_rows fixes the rows per chunk for every array.
    auto move = [&](void* base, size_t row_bytes) {
        if (!base) return;
        const CompactPlan plan = compact_plan(n0, m, p.rem[0], ix->opt.compact_chunk_rows > 0 ? p.plan.chunk_rows : (long long)(ix->st_cmp.bytes / row_bytes));
        for (long long c = 0; c < plan.chunks && e == hipSuccess; ++c) {
            const CompactChunk k = compact_chunk(plan, c);
            e = launch_compact_rows(base, ix->st_cmp.p, (long long)row_bytes, k.lo, k.hi - k.lo, d_rem, m, 0, k.lo, nullptr);    // gather
            if (e == hipSuccess) e = launch_compact_rows(ix->st_cmp.p, base, (long long)row_bytes, k.lo, k.hi - k.lo, nullptr, 0, k.lo, 0, nullptr);   // scatter
        }
    };
    // the vacated entries [n1, n0) of a per-row float array: the zeroes a fresh build with room to spare leaves there
    auto vacate = [&](float* a) { if (e == hipSuccess && a) e = hipMemsetAsync(a + n1, 0, (size_t)m * sizeof(float), nullptr); };
    move(ix->rows_orig, (size_t)ix->d * esz);
    if (p.scan_moves) move(ix->rows_scan, (size_t)ix->dp * scan_esz);
    move(ix->norm, sizeof(float));
    move(ix->inv_scan, sizeof(float));
    vacate(ix->norm);
    vacate(ix->inv_scan);
    if (p.image == kImageAlias) {   // an int8 index: inv_img = inv_scan, offsets 0
        if (e == hipSuccess && n1 > first)
            e = hipMemcpyAsync(ix->inv_img + first, ix->inv_scan + first, (size_t)(n1 - first) * sizeof(float), hipMemcpyDeviceToDevice, nullptr);
        vacate(ix->inv_img);
    }
    if (e == hipSuccess && p.new_cn) e = launch_normalize_rows(ix->rows_orig, dt, 0, n1, ix->d, ix->norm, p.new_cn, nullptr);
    else if (e == hipSuccess && ix->cn_cache && n1 > first)
        e = launch_normalize_rows(ix->rows_orig, dt, first, n1 - first, ix->d, ix->norm, ix->cn_cache + (size_t)first * ix->d, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        p.release();
        ix->damaged = true;
        return fail(VF_EHIP, std::string("remove: ") + hipGetErrorString(e) + " -- " + kDamagedMsg);
    }
    // commit: the row count last among the arrays, then what a fresh build of n1 rows holds and does not hold
    ix->n = n1;
    if (p.to_small) {
        if (ix->owns_scan && ix->rows_scan) (void)hipFree(ix->rows_scan);
        ix->rows_scan = nullptr; ix->owns_scan = false;
    }
    if (p.new_cn) { ix->cn_cache = p.new_cn; p.new_cn = nullptr; }
    if (n1 == 0 && ix->cn_cache) { (void)hipFree(ix->cn_cache); ix->cn_cache = nullptr; }   // (a handle created empty holds none)
    ix->image_refused = false;
    if (p.image == kImageDrop) free_image(ix);
    if (p.image == kImageNew) {
        ix->rows_img = p.new_img; ix->inv_img = p.new_iimg; ix->owns_img = true;
        p.new_img = nullptr; p.new_iimg = nullptr;
    }
    if (p.image == kImageNew || p.image == kImageRefill) {
        const int rc = image_fill(ix);   // (a row that leaves too much residual: no image, as a fresh build decides)
        if (rc != VF_OK) { ix->damaged = true; g_err += std::string(" -- ") + kDamagedMsg; return VF_EHIP; }
    }
    if (ix->st_cmp.bytes > (size_t)kCompactStageBytes) ix->st_cmp.release();
    return VF_OK;
}

// vf_index_create with dtype == VF_INDEX_REMOVE.  Every argument error is reported before the first HIP call.
static int remove_entry(vf_index** out, const int64_t* ids, int64_t n_ids, int32_t d, int32_t device_id) {
    if (!out) return fail(VF_EINVAL, "vf_index_create: null out");
    vf_index* ix = *out;
    if (!ix) return fail(VF_EINVAL, "vf_index_create: VF_INDEX_REMOVE needs a live handle in *out");
    if (d != ix->d) return fail(VF_EINVAL, "vf_index_create: VF_INDEX_REMOVE: d must be the handle's (" + std::to_string(ix->d) + ")");
    if (device_id != ix->device) return fail(VF_EINVAL, "vf_index_create: VF_INDEX_REMOVE: device_id must be the handle's device " + std::to_string(ix->device));
    if (n_ids < 0 || (n_ids > 0 && !ids)) return fail(VF_EINVAL, "vf_index_create: VF_INDEX_REMOVE: bad ids/n_ids");
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->damaged) return fail(VF_EHIP, std::string("vf_index_create: VF_INDEX_REMOVE: ") + kDamagedMsg);
    if (search_pending(ix)) return fail(VF_EINVAL, "vf_index_create: VF_INDEX_REMOVE: search pending (a slot is between _begin and _end)");
    if (n_ids == 0) return VF_OK;
    const int64_t lo = ix->id_offset, hi = ix->id_offset + ix->n;
    for (int64_t i = 0; i < n_ids; ++i)
        if (ids[i] < lo || ids[i] >= hi)
            return fail(VF_EINVAL, "vf_index_create: VF_INDEX_REMOVE: ids[" + std::to_string(i) + "] = " + std::to_string(ids[i]) +
                                       " is outside the handle's ids [" + std::to_string(lo) + ", " + std::to_string(hi) + "): nothing was removed");
    std::vector<long long> all(ids, ids + n_ids);
    std::sort(all.begin(), all.end());
    all.erase(std::unique(all.begin(), all.end()), all.end());
    DeviceGuard restore_callers_device;
    if (ix->shards.empty()) {
        RemovePrep p;
        p.ix = ix;
        p.rem = std::move(all);
        for (long long& r : p.rem) r -= lo;
        VF_TRY(remove_prepare(p));
        return remove_run(p);
    }
    // a group: each id to the shard that holds it; every shard is validated and prepared before any is changed
    const size_t G = ix->shards.size();
    std::vector<RemovePrep> preps(G);
    size_t at = 0;
    for (size_t s = 0; s < G; ++s) {
        vf_index* sh = ix->shards[s];
        preps[s].ix = sh;
        while (at < all.size() && all[at] < sh->id_offset + sh->n) preps[s].rem.push_back(all[at++] - sh->id_offset);
        if (!preps[s].rem.empty() && (int64_t)preps[s].rem.size() == sh->n)
            return fail(VF_EUNSUPPORTED, "vf_index_create: VF_INDEX_REMOVE: the removal would leave shard " + std::to_string(s) +
                                             " of the group without rows (nothing re-balances a group): nothing was removed");
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    for (vf_index* sh : ix->shards) locks.emplace_back(sh->mu);
    for (size_t s = 0; s < G; ++s) {
        if (preps[s].rem.empty()) continue;
        const int rc = remove_prepare(preps[s]);
        if (rc != VF_OK) {
            const std::string keep = g_err;
            for (RemovePrep& q : preps) q.release();
            g_err = keep;
            return rc;
        }
    }
    int64_t gone = 0;
    for (size_t s = 0; s < G; ++s) {
        vf_index* sh = ix->shards[s];
        sh->id_offset -= gone;   // ids stay one contiguous range
        if (preps[s].rem.empty()) continue;
        const int rc = remove_run(preps[s]);
        if (rc != VF_OK) {       // (shards before this one have changed: the group cannot be searched as one range any more)
            const std::string keep = g_err;
            for (RemovePrep& q : preps) q.release();
            ix->damaged = sh->damaged || gone > 0;
            g_err = keep;
            return rc;
        }
        gone += (int64_t)preps[s].rem.size();
        ix->n -= (int64_t)preps[s].rem.size();
    }
    return VF_OK;
}

extern "C" int vf_index_create(vf_index** out, const void* rows, int64_t n, int32_t d, int32_t dtype,
                               int32_t device_id, int64_t id_offset) {
    if (dtype == VF_INDEX_REMOVE) return remove_entry(out, (const int64_t*)rows, n, d, device_id);
    if (dtype >= 0 && (dtype & VF_INDEX_APPEND)) return append_entry(out, rows, false, n, d, dtype, device_id);
    DeviceGuard restore_callers_device;
    return create_impl(out, rows, false, n, d, dtype, device_id, id_offset);
}

extern "C" int vf_index_create_device(vf_index** out, const void* d_rows, int64_t n, int32_t d, int32_t dtype,
                                      int32_t device_id, int64_t id_offset) {
    if (dtype >= 0 && (dtype & VF_INDEX_APPEND)) return append_entry(out, d_rows, true, n, d, dtype, device_id);
    DeviceGuard restore_callers_device;
    return create_impl(out, d_rows, true, n, d, dtype, device_id, id_offset);
}

// ------------------------------------------------------------------------------------------------
// Corpus file (.vfc): a 64-byte header followed by n * d elements, row-major.  Replaces "pull every
// embedding out of Chroma into Python lists at start-up" (src/utils/ensembleRetriever.py:39-43,
// src/utils/faissRetriever.py:14) for corpora that size cannot go through.
//   +0  char[8] "VFCORPUS"   +8 u32 version (1)   +12 u32 dtype (VF_DTYPE_*)   +16 u64 n   +24 u32 d
//   +28 u32 flags (bit 0: an int64[n] external-id table follows the rows)   +32 .. +63 reserved (0)
// ------------------------------------------------------------------------------------------------
struct VfcHeader {
    char magic[8];
    uint32_t version, dtype;
    uint64_t n;
    uint32_t d, flags;
    uint8_t reserved[32];
};
static_assert(sizeof(VfcHeader) == 64, "corpus file header is 64 bytes");

static int read_vfc_header(int fd, const char* path, VfcHeader* h, size_t* esz) {
    if (pread(fd, h, sizeof(*h), 0) != (ssize_t)sizeof(*h)) return fail(VF_EINVAL, std::string("corpus file too short: ") + path);
    if (memcmp(h->magic, "VFCORPUS", 8) != 0) return fail(VF_EINVAL, std::string("not a corpus file (bad magic): ") + path);
    if (h->version != 1) return fail(VF_EUNSUPPORTED, std::string("corpus file version not supported: ") + path);
    if (!known_dtype(h->dtype) || h->d == 0) return fail(VF_EINVAL, std::string("corpus file header is corrupt: ") + path);
    *esz = dtype_bytes((int)h->dtype);
    struct stat st;
    if (fstat(fd, &st) != 0) return fail(VF_EINVAL, std::string("cannot stat corpus file: ") + path);
    // n * d * element size (+ the id table) against the file's size, WITHOUT wrapping: a header with n = 2^61 and d = 16 would
    // otherwise multiply to a small number, pass this check and hand a huge row count to the loader (round 5: found by the header
    // fuzz of tools/host_sanitize_check.cc; unsigned wrap-around is not an error any sanitizer reports)
    unsigned long long payload = 0, ids = 0, need = 0;
    if (__builtin_mul_overflow((unsigned long long)h->n, (unsigned long long)h->d * (unsigned long long)*esz, &payload) ||
        __builtin_mul_overflow((unsigned long long)h->n, (h->flags & 1u) ? 8ull : 0ull, &ids) ||
        __builtin_add_overflow(payload, ids, &need) || __builtin_add_overflow(need, 64ull, &need))
        return fail(VF_EINVAL, std::string("corpus file header is corrupt (n x d overflows): ") + path);
    if ((unsigned long long)st.st_size < need) return fail(VF_EINVAL, std::string("corpus file is truncated: ") + path);
    if (h->n >= 0x7fffffffffffffffull / 2) return fail(VF_EINVAL, std::string("corpus file header is corrupt: ") + path);
    return VF_OK;
}

extern "C" int vf_corpus_file_info(const char* path, int64_t* n, int32_t* d, int32_t* dtype, int32_t* has_ids) {
    if (!path) return fail(VF_EINVAL, "vf_corpus_file_info: null path");
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(VF_EINVAL, std::string("cannot open corpus file: ") + path);
    VfcHeader h; size_t esz = 0;
    const int rc = read_vfc_header(fd, path, &h, &esz);
    close(fd);
    if (rc != VF_OK) return rc;
    if (n) *n = (int64_t)h.n;
    if (d) *d = (int32_t)h.d;
    if (dtype) *dtype = (int32_t)h.dtype;
    if (has_ids) *has_ids = (int32_t)(h.flags & 1u);
    return VF_OK;
}

// Rows [row_lo, row_hi) of the file become an index on `device_id` (a rank's shard: SURVEY.md 8e).  The rows are
// streamed through two pinned staging buffers (read() of one overlaps the H2D copy of the other).
extern "C" int vf_index_create_from_file(vf_index** out, const char* path, int64_t row_lo, int64_t row_hi,
                                         int32_t device_id, int64_t id_offset) {
    DeviceGuard restore_callers_device;
    if (!out || !path) return fail(VF_EINVAL, "vf_index_create_from_file: null argument");
    *out = nullptr;
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(VF_EINVAL, std::string("cannot open corpus file: ") + path);
    VfcHeader h; size_t esz = 0;
    int rc = read_vfc_header(fd, path, &h, &esz);
    if (rc == VF_OK && (row_lo < 0 || row_hi < row_lo || (uint64_t)row_hi > h.n))
        rc = fail(VF_EINVAL, "vf_index_create_from_file: row range outside the file");
    int ndev = 0;
    if (rc == VF_OK && (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev))
        rc = fail(VF_EINVAL, "vf_index_create_from_file: bad device_id");
    if (rc != VF_OK) { close(fd); return rc; }
    const int64_t n = row_hi - row_lo;
    const size_t row_bytes = (size_t)h.d * esz, total = (size_t)n * row_bytes;
    void* d_rows = nullptr;
    char* stage[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    const size_t chunk = 64u << 20;
    hipError_t e = hipSetDevice(device_id);
    if (e == hipSuccess && total) e = hipMalloc(&d_rows, total);
    for (int i = 0; i < 2 && e == hipSuccess && total; ++i) {
        e = hipHostMalloc((void**)&stage[i], chunk, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) rc = fail(VF_ENOMEM, std::string("vf_index_create_from_file: ") + hipGetErrorString(e));
    size_t done = 0;
    for (int i = 0; rc == VF_OK && done < total; i ^= 1) {
        const size_t len = std::min(chunk, total - done);
        if (hipEventSynchronize(ev[i]) != hipSuccess) { rc = fail(VF_EHIP, "vf_index_create_from_file: event wait failed"); break; }
        size_t got = 0;
        while (got < len) {
            const ssize_t r = pread(fd, stage[i] + got, len - got, (off_t)(64 + (size_t)row_lo * row_bytes + done + got));
            if (r <= 0) { rc = fail(VF_EINVAL, std::string("read error in corpus file: ") + path); break; }
            got += (size_t)r;
        }
        if (rc != VF_OK) break;
        e = hipMemcpyAsync((char*)d_rows + done, stage[i], len, hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess) e = hipEventRecord(ev[i], nullptr);
        if (e != hipSuccess) { rc = fail(VF_EHIP, std::string("vf_index_create_from_file: ") + hipGetErrorString(e)); break; }
        done += len;
    }
    close(fd);
    if (rc == VF_OK && hipDeviceSynchronize() != hipSuccess) rc = fail(VF_EHIP, "vf_index_create_from_file: copy failed");
    for (int i = 0; i < 2; ++i) {
        if (stage[i]) (void)hipHostFree(stage[i]);
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    if (rc == VF_OK) {
        rc = create_impl(out, d_rows, true, n, (int32_t)h.d, (int32_t)h.dtype, device_id, id_offset, true);
        // create_impl borrowed the device rows: hand them over to the index
        if (rc == VF_OK) { (*out)->owns_rows = true; d_rows = nullptr; }
    }
    if (d_rows) (void)hipFree(d_rows);
    return rc;
}

extern "C" int vf_index_destroy(vf_index* ix) {
    DeviceGuard restore_callers_device;
    if (!ix) return VF_OK;
    destroy_index(ix);
    return VF_OK;
}

extern "C" int vf_index_info(vf_index* ix, int64_t* n, int32_t* d, int32_t* dtype, int32_t* device_id) {
    if (!ix) return fail(VF_EINVAL, "vf_index_info: null handle");
    if (n) *n = ix->n;
    if (d) *d = ix->d;
    if (dtype) *dtype = ix->dtype;
    if (device_id) *device_id = ix->device;
    return VF_OK;
}

extern "C" int vf_index_stats(vf_index* ix, vf_search_stats* out) {
    if (!ix || !out) return fail(VF_EINVAL, "vf_index_stats: null argument");
    std::lock_guard<std::mutex> g(ix->mu);
    *out = ix->stats;
    return VF_OK;
}

extern "C" int vf_index_profile(vf_index* ix, double* scan_ms_total, int64_t* scan_launches, double* pipeline_ms_total,
                                int64_t* scan_bytes_per_launch) {
    if (!ix) return fail(VF_EINVAL, "vf_index_profile: null handle");
    std::lock_guard<std::mutex> g(ix->mu);
    double sm = ix->prof_scan_ms, pm = ix->prof_pipe_ms;
    int64_t nl = ix->prof_launches, nb = ix->prof_bytes;
    for (vf_index* sh : ix->shards) {  // group: totals over the shards (equal blocks: bytes per launch of the first)
        std::lock_guard<std::mutex> lk(sh->mu);
        sm += sh->prof_scan_ms; pm += sh->prof_pipe_ms; nl += sh->prof_launches;
        if (nb == 0) nb = sh->prof_bytes;
    }
    if (scan_ms_total) *scan_ms_total = sm;
    if (scan_launches) *scan_launches = nl;
    if (pipeline_ms_total) *pipeline_ms_total = pm;
    if (scan_bytes_per_launch) *scan_bytes_per_launch = nb;
    return VF_OK;
}

// Makespan of the timed main scans: first launch's begin -> last launch's end, on the streams the scans run on.  With
// ordered scans it is the sum of the brackets plus the gaps between launches; with overlapping scans (small shards) it is
// the only well-defined "time per launch": span / launches.  Call after the searches have ended.
extern "C" int vf_index_profile_span(vf_index* ix, double* span_ms, int64_t* launches) {
    if (!ix || !span_ms || !launches) return fail(VF_EINVAL, "vf_index_profile_span: null argument");
    DeviceGuard restore_callers_device;
    vf_index* t = ix->shards.empty() ? ix : ix->shards[0];   // a group: its first shard (equal blocks run in step)
    std::lock_guard<std::mutex> g(t->mu);
    *span_ms = 0.0; *launches = t->prof_launches;
    if (!t->span_started || !t->ev_span) return VF_OK;
    VF_HIP(hipSetDevice(t->device));
    for (int i = 0; i < kSlots; ++i) {
        if (!t->span_slot[i] || !t->slots[i].ev_t[1] || t->slots[i].pending) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, t->ev_span, t->slots[i].ev_t[1]) == hipSuccess && ms > *span_ms) *span_ms = ms;
        else (void)hipGetLastError();
    }
    return VF_OK;
}

// debug: copy the wall-clock stamps of slot's last main scan (option debug bit 7) to host
extern "C" int vf_index_debug_read(vf_index* ix, int32_t slot, unsigned long long* out, int64_t n_words) {
    DeviceGuard restore_callers_device;
    if (!ix || !out || slot < 0 || slot >= kSlots) return fail(VF_EINVAL, "vf_index_debug_read: bad argument");
    if (!ix->shards.empty()) return vf_index_debug_read(ix->shards[0], slot, out, n_words);
    std::lock_guard<std::mutex> g(ix->mu);
    Slot& s = ix->slots[slot];
    const size_t bytes = std::min<size_t>(s.dbg.bytes, (size_t)n_words * 8);
    VF_HIP(hipSetDevice(ix->device));
    VF_HIP(hipDeviceSynchronize());
    if (bytes) VF_HIP(hipMemcpy(out, s.dbg.p, bytes, hipMemcpyDeviceToHost));
    return (int)(bytes / 8);
}

extern "C" int vf_index_slots(vf_index* ix, int32_t* out) {
    if (!ix || !out) return fail(VF_EINVAL, "vf_index_slots: null argument");
    *out = kSlots;
    return VF_OK;
}

static_assert(kMaxShardRows == 0xFFFFFFFFll && kSubsetMaxRows == 0xFFFFFFFEll, "vf_options.h: the upper ends of compact_chunk_rows and subset_super_rows");
extern "C" int vf_index_set_option(vf_index* ix, const char* name, int64_t value) {
    if (!ix || !name) return fail(VF_EINVAL, "vf_index_set_option: null argument");
    if (strcmp(name, "reserve_rows") == 0) return reserve_rows(ix, value);
    for (vf_index* sh : ix->shards) VF_TRY(vf_index_set_option(sh, name, value));  // a group forwards to every shard
    std::lock_guard<std::mutex> g(ix->mu);
    if (strcmp(name, "profile") == 0) {
        ix->profile = value != 0; ix->prof_scan_ms = ix->prof_pipe_ms = 0.0; ix->prof_launches = 0;
        ix->span_started = false;
        for (bool& b : ix->span_slot) b = false;
        return VF_OK;
    }
    // the table's check (vf_options.h) runs on a copy: the handle takes the value once what it has to do for it has succeeded
    Options o = ix->opt;
    std::string msg;
    if (option_set(o, name, value, &msg) != kOptionStored) return fail(VF_EINVAL, msg);
    if (o.aux_cus != ix->opt.aux_cus && ix->aux_applied >= 0)   // takes effect for slots created afterwards (set it before the first search)
        return fail(VF_EINVAL, "aux_cus is fixed once the first search has created the scan streams: set it before searching");
    if (strcmp(name, "scan_image") == 0) {
        if (ix->damaged) return fail(VF_EHIP, std::string("scan_image: ") + kDamagedMsg);
        if (ix->shards.empty()) {   // (a group's shards have built or dropped theirs above)
            for (const Slot& sl : ix->slots) if (sl.pending) return fail(VF_EINVAL, "scan_image cannot change while a search is pending");
            DeviceGuard restore_callers_device;
            VF_HIP(hipSetDevice(ix->device));
            VF_HIP(hipDeviceSynchronize());
            ix->image_refused = false;
            if (value == 0) free_image(ix);
            else VF_TRY(build_image(ix, value));
        }
    }
    ix->opt = o;
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------
// exact path: canonical dense scores chunk by chunk + LDS sort + running merge.
// qn_dev: [nq][d] canonical normalised queries on device.  Writes [nq][k] at out_ids/out_scores.
// ------------------------------------------------------------------------------------------------
static int exact_search(vf_index* ix, Slot& s, const float* qn_dev, int nq, int k, int64_t* out_ids,
                        float* out_scores, hipStream_t st) {
    const int dt = ix->dtype;
    const int64_t chunk = kSmallN;
    const int64_t nchunks = ix->n == 0 ? 1 : (ix->n + chunk - 1) / chunk;
    if (nchunks > 1) {  // k_merge_topk sorts next_pow2(2k) 8-byte keys in LDS
        int64_t P = 1;
        while (P < 2 * (int64_t)k) P <<= 1;
        if (P * 8 > 160 * 1024) return fail(VF_EUNSUPPORTED, "exact chunked search supports k <= 8192 when n > 16384");
    }
    VF_TRY(s.dense_s.ensure((size_t)nq * chunk * sizeof(float)));
    if (nchunks == 1) {
        const float* cn = ix->cn_cache;
        if (!cn && ix->n > 0) {
            VF_TRY(s.cn_tmp.ensure((size_t)chunk * ix->d * sizeof(float)));
            VF_HIP(launch_normalize_rows(ix->rows_orig, dt, 0, ix->n, ix->d, ix->norm, s.cn_tmp.as<float>(), st));
            cn = s.cn_tmp.as<float>();
        }
        VF_HIP(launch_dense_dot16(qn_dev, nq, cn, ix->n, ix->d, s.dense_s.as<float>(), chunk, st));
        VF_HIP(launch_sort_rows(s.dense_s.as<float>(), chunk, nq, (int)ix->n, k, ix->id_offset, (long long*)out_ids,
                                out_scores, k, st));
        return VF_OK;
    }
    VF_TRY(s.cn_tmp.ensure((size_t)chunk * ix->d * sizeof(float)));
    const size_t part = (size_t)nq * k;
    VF_TRY(s.parts_ids.ensure(2 * part * sizeof(long long)));
    VF_TRY(s.parts_sc.ensure(2 * part * sizeof(float)));
    VF_TRY(s.run_ids.ensure(part * sizeof(long long)));
    VF_TRY(s.run_sc.ensure(part * sizeof(float)));
    long long* pid = s.parts_ids.as<long long>();
    float* psc = s.parts_sc.as<float>();
    VF_HIP(hipMemsetAsync(pid, 0xFF, part * sizeof(long long), st));  // running part = all -1
    VF_HIP(hipMemsetAsync(psc, 0, part * sizeof(float), st));
    for (int64_t c = 0; c < nchunks; ++c) {
        const int64_t r0 = c * chunk, nr = std::min(chunk, ix->n - r0);
        VF_HIP(launch_normalize_rows(ix->rows_orig, dt, r0, nr, ix->d, ix->norm, s.cn_tmp.as<float>(), st));
        VF_HIP(launch_dense_dot16(qn_dev, nq, s.cn_tmp.as<float>(), nr, ix->d, s.dense_s.as<float>(), chunk, st));
        VF_HIP(launch_sort_rows(s.dense_s.as<float>(), chunk, nq, (int)nr, k, ix->id_offset + r0, pid + part, psc + part,
                                k, st));
        VF_HIP(launch_merge_topk(pid, psc, 2, nq, k, s.run_ids.as<long long>(), s.run_sc.as<float>(), st));
        VF_HIP(hipMemcpyAsync(pid, s.run_ids.p, part * sizeof(long long), hipMemcpyDeviceToDevice, st));
        VF_HIP(hipMemcpyAsync(psc, s.run_sc.p, part * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    VF_HIP(hipMemcpyAsync(out_ids, s.run_ids.p, part * sizeof(long long), hipMemcpyDeviceToDevice, st));
    VF_HIP(hipMemcpyAsync(out_scores, s.run_sc.p, part * sizeof(float), hipMemcpyDeviceToDevice, st));
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------
// the fused pipeline (which path and which kernels serve a search: vf_route.h)
// ------------------------------------------------------------------------------------------------

// Test hook (not in the public header; exported by the test build only): the bound and bands above, for tests/test_scan_image_model.py
extern "C" int vf_debug_image_bound(int32_t d, int32_t dtype, float rho_mean, float* eps, int32_t* tau_band, int32_t* fine_band) {
    if (!eps || !tau_band || !fine_band || d <= 0) return fail(VF_EINVAL, "vf_debug_image_bound: bad argument");
    int tb = 0, fb = 0;
    image_bound(d, dtype, rho_mean, eps, &tb, &fb);
    *tau_band = tb; *fine_band = fb;
    return VF_OK;
}

// Test hook (not in the public header; exported by the test build only): what a query's int8 plane adds (image_q8_bound / image_q8_eps, the formulas k_prep_q8 runs on the device),
// for tests/test_scan_image_q8_model.py
extern "C" int vf_debug_image_q8_bound(float rho_q, float eps_img, int32_t tau_band, int32_t fine_band, float* eps_q, int32_t* tau_band_q,
                                       int32_t* fine_band_q) {
    if (!eps_q || !tau_band_q || !fine_band_q) return fail(VF_EINVAL, "vf_debug_image_q8_bound: bad argument");
    const Q8Bound b = image_q8_bound(rho_q);
    *eps_q = image_q8_eps(eps_img, b.eps_add);
    *tau_band_q = tau_band + b.tau_bins; *fine_band_q = fine_band + b.fine_bins;
    return VF_OK;
}

// ---- what the passes of a fused search share -----------------------------------------------------------------------------
// The fused path's per-query state for `slots` query slots: `slen` sample scores and a candidate list of `cap` entries each.
static int ensure_fused_bufs(Slot& s, size_t slots, size_t slen, size_t cap) {
    VF_TRY(s.s0.ensure(slots * slen * sizeof(float)));
    VF_TRY(s.cnt.ensure(slots * kCntStride * sizeof(u32)));
    VF_TRY(s.tau.ensure(slots * sizeof(int)));
    VF_TRY(s.hist.ensure(slots * kHistBins * sizeof(u32)));
    VF_TRY(s.hist_coarse.ensure(slots * 64 * sizeof(u32)));
    return s.cand.ensure(slots * cap * sizeof(u64));
}

// First row of every scan workgroup (k_sel0 maps sample slots back to rows) or, tagged with the negative count, of every row group of a
// wide pass: uploaded when (n, groups) changed.  The copy goes on the slot's stream, which is then synchronised (`base` is host memory):
// consecutive wide passes of one search can have different row-group counts, so the copy must be ordered behind the previous pass.
// The narrow passes keep one grid for the whole search and need no such order -- they used a blocking hipMemcpy here; for them only the
// synchronising call differs, on the first search after n or the grid changed.
static int upload_row_bases(vf_index* ix, Slot& s, int groups, bool wide, hipStream_t st) {
    const int tag = wide ? -groups : groups;
    if (s.wgbase_n == ix->n && s.wgbase_grid == tag) return VF_OK;
    std::vector<long long> base(groups);
    for (int w = 0; w < groups; ++w) base[w] = ix->n * (long long)w / groups;
    VF_TRY(s.wgbase.ensure((size_t)groups * sizeof(long long)));
    VF_HIP(hipMemcpyAsync(s.wgbase.p, base.data(), (size_t)groups * sizeof(long long), hipMemcpyHostToDevice, st));
    VF_HIP(hipStreamSynchronize(st));
    s.wgbase_n = ix->n; s.wgbase_grid = tag;
    return VF_OK;
}

// What every kernel of a pass of nb queries is given alike, wide or not: the rows as stored and their inverse norms, the fp16 query image,
// the slot's counters, thresholds, histograms and candidate lists.  The caller adds its geometry and the operands that are its own.
static ScanArgs scan_args(const vf_index* ix, const Slot& s, const FusedPlan& p, int nb) {
    ScanArgs a{};
    a.rows = (const char*)ix->rows_scan; a.inv_scan = ix->inv_scan; a.qimg = s.qimg.as<_Float16>();
    a.n = ix->n; a.dp = ix->dp; a.row_bytes = (long long)ix->dp * (byte_rows(ix->dtype) ? 1 : 2);
    a.s0 = s.s0.as<float>(); a.wg_base = s.wgbase.as<long long>(); a.cnt = s.cnt.as<u32>(); a.tau_bin = s.tau.as<int>();
    a.hist = s.hist.as<u32>(); a.hist_coarse = s.hist_coarse.as<u32>(); a.cand = s.cand.as<u64>(); a.cap = p.cap; a.kprime = p.kprime;
    a.nq = nb; a.debug = (int)ix->opt.debug;
    return a;
}

// ... and k_final: the candidate lists, the rows as given for the re-score, the pass's queries, where its results and flags go
static FinalArgs final_args(const vf_index* ix, const Slot& s, const FusedPlan& p, int k, const float* qn_b, int64_t* d_ids, float* d_scores,
                            int flag_off) {
    FinalArgs f{};
    f.cnt = s.cnt.as<u32>(); f.cand = s.cand.as<u64>(); f.cap = p.cap; f.tau_bin = s.tau.as<int>(); f.rows_orig = ix->rows_orig;
    f.orig_dtype = ix->dtype; f.orig_row_elems = ix->d; f.norm = ix->norm; f.qn = qn_b;
    f.d = ix->d; f.k = k; f.kprime = p.kprime; f.eps = p.eps; f.n_rows = ix->n; f.id_offset = ix->id_offset;
    f.out_ids = (long long*)d_ids; f.out_scores = d_scores;
    f.flags = s.d_flags + flag_off; f.cand_count_out = s.d_counts + flag_off;
    return f;
}

// The three ways a pending search (the slot's d_queries, nq, k, d_ids, d_scores) is enqueued on the slot's streams; begin_impl records
// ev_done behind whichever ran.
static int begin_exact(vf_index* ix, Slot& s, int per_pass) {
    hipStream_t st = s.stream;
    for (int b0 = 0; b0 < s.nq; b0 += per_pass) {
        const int nb = std::min(per_pass, s.nq - b0);
        float* qn_b = s.qn.as<float>() + (size_t)b0 * ix->d;
        VF_HIP(launch_prep_queries(s.d_queries + (size_t)b0 * ix->d, nb, ix->d, ix->dp, qn_tile_for(nb), qn_b, s.qimg.as<_Float16>(), st));
        VF_TRY(exact_search(ix, s, qn_b, nb, s.k, s.d_ids + (size_t)b0 * s.k, s.d_scores + (size_t)b0 * s.k, st));
    }
    return VF_OK;
}

// ---- wide passes (k_scan_wide): up to 1024 queries share ONE read of the shard --------------------------------------
static int begin_wide(vf_index* ix, int slot_id, const RouteIn& in, const SearchRoute& r) {
    Slot& s = ix->slots[slot_id];
    hipStream_t st = s.stream;
    const int64_t debug = ix->opt.debug;
    s.timed = ix->profile;
    if (s.timed) VF_HIP(hipEventRecord(s.ev_t[2], st));
    for (int b0 = 0; b0 < s.nq; b0 += r.per_pass) {
        const int nb = std::min(r.per_pass, s.nq - b0);
        const bool timed = s.timed && b0 == 0;
        const float* q_b = s.d_queries + (size_t)b0 * ix->d;
        float* qn_b = s.qn.as<float>() + (size_t)b0 * ix->d;
        const WidePass w = route_wide_pass(in, r.plan, nb);
        const int qtot = w.qtot, RG = w.rgroups;
        const bool w8 = w.main == kKernelWide8;
        FusedPlan p = r.plan;
        p.cap = w.cap;
        const size_t slen = (size_t)RG * w.samp * 8;
        VF_TRY(s.qimg.ensure((size_t)ix->dp * qtot * 2));
        VF_TRY(ensure_fused_bufs(s, (size_t)qtot, slen, (size_t)p.cap));
        VF_TRY(upload_row_bases(ix, s, RG, true, st));
        VF_HIP(launch_prep_queries(q_b, nb, ix->d, ix->dp, qtot, qn_b, s.qimg.as<_Float16>(), st));
        if (w8) {
            VF_TRY(s.qimg8.ensure((size_t)ix->dp * qtot * 2));
            VF_TRY(s.epsq.ensure((size_t)qtot * sizeof(float)));
            VF_HIP(launch_prep_wide8(qn_b, nb, ix->d, ix->dp, qtot, (unsigned char*)s.qimg8.p, s.epsq.as<float>(), st));
        }
        ScanArgs a = scan_args(ix, s, p, nb);
        a.total_waves = RG * 8; a.samp = w.samp; a.stage_cap = kWideStageCap; a.refresh_every = w.refresh_every;
        a.qn_total = qtot; a.jtiles = w.jtiles; a.rgroups = RG;
        if (w.clear_sample)   // sample slots no wave writes must read as empty (NaN)
            VF_HIP(hipMemsetAsync(a.s0, 0xFF, (size_t)qtot * slen * sizeof(float), st));
        VF_HIP(launch_scan_wide(a, kModeSample, w.rows, st));
        VF_HIP(launch_sel0(a, qtot, st));
        for (int o = 0; o < kSlots; ++o)
            if (o != slot_id && ix->slots[o].ev_scan) VF_HIP(hipStreamWaitEvent(st, ix->slots[o].ev_scan, 0));
        if (w.main_jtiles > 1 && ix->opt.wide_sync >= 0) {   // sibling progress words of the main pass (see k_scan_wide; eight per row group)
            VF_TRY(s.sib.ensure((size_t)RG * 8 * sizeof(u32)));
            VF_HIP(hipMemsetAsync(s.sib.p, 0, (size_t)RG * 8 * sizeof(u32), st));
            a.sib = s.sib.as<u32>(); a.sib_slack = (int)ix->opt.wide_sync;
        }
        if (timed) VF_HIP(hipEventRecord(s.ev_t[0], st));
        if (w8) {
            ScanArgs a8 = a;
            a8.qimg = (const _Float16*)s.qimg8.p;
            a8.jtiles = w.main_jtiles;
            a8.stage_cap = w.stage_cap;
            if (debug & 128) {   // per-wave phase times of k_scan_wide8 (vf_index_debug_read)
                VF_TRY(s.dbg.ensure((size_t)8 * w.main_jtiles * ((RG + 7) / 8) * w.waves * 16 * sizeof(u64)));
                VF_HIP(hipMemsetAsync(s.dbg.p, 0, s.dbg.bytes, st));
                a8.dbg = s.dbg.as<u64>();
            }
            VF_HIP(launch_scan_wide8(a8, w.waves, st));
        } else
            VF_HIP(launch_scan_wide(a, kModeMain, w.rows, st));
        VF_HIP(hipEventRecord(s.ev_scan, st));
        if (timed) {
            VF_HIP(hipEventRecord(s.ev_t[1], st));
            ix->prof_bytes = w.scan_bytes;
        }
        FinalArgs f = final_args(ix, s, p, s.k, qn_b, s.d_ids + (size_t)b0 * s.k, s.d_scores + (size_t)b0 * s.k, b0);
        f.eps_q = w8 ? s.epsq.as<float>() : nullptr;   // (the sample pass scored with fp16 queries: its bound is the smaller one)
        if (debug & 256) { VF_TRY(s.dbg.ensure((size_t)qtot * 8 * sizeof(u64))); f.dbg = s.dbg.as<u64>(); }
        VF_HIP(launch_final(f, nb, st));
        s.scan_kernel = w.main;
        ++s.wide_launches; s.wide_queries += nb;
    }
    if (s.timed) VF_HIP(hipEventRecord(s.ev_t[3], st));
    return VF_OK;
}

// ---- passes of up to 64 queries: sample pass, threshold seed, main scan (on the scan stream), k_final ---------------------------
static int begin_narrow(vf_index* ix, int slot_id, const RouteIn& in, const SearchRoute& r) {
    Slot& s = ix->slots[slot_id];
    hipStream_t st = s.stream, sst = s.scan_stream;
    const FusedPlan& p = r.plan;
    const int64_t debug = ix->opt.debug;
    VF_TRY(ensure_fused_bufs(s, kMaxBatch, (size_t)p.total_waves * p.samp, (size_t)p.cap));
    VF_TRY(s.tilecnt.ensure((size_t)p.grid * sizeof(u32)));
    s.timed = ix->profile;
    if (s.timed) VF_HIP(hipEventRecord(s.ev_t[2], st));
    VF_TRY(upload_row_bases(ix, s, p.grid, false, st));
    for (int b0 = 0; b0 < s.nq; b0 += r.per_pass) {
        const int nb = std::min(r.per_pass, s.nq - b0);
        const bool timed = s.timed && b0 == 0;
        const BatchRoute b = route_batch(in, r, nb);
        const int qt = b.tile;
        float* qn_b = s.qn.as<float>() + (size_t)b0 * ix->d;
        // (the int8 plane replaces the fp16 image: that one is not built)
        VF_HIP(launch_prep_queries(s.d_queries + (size_t)b0 * ix->d, nb, ix->d, ix->dp, qt, qn_b, s.image_i8 ? nullptr : s.qimg.as<_Float16>(), st));
        ScanArgs a = scan_args(ix, s, p, nb);
        if (s.image_i8) {
            VF_TRY(s.qimg8.ensure((size_t)ix->dp * kMaxBatch * 2));
            VF_TRY(s.epsq.ensure(kMaxBatch * sizeof(float)));
            VF_TRY(s.qscale.ensure(kMaxBatch * sizeof(float)));
            VF_TRY(s.bandq.ensure(2 * kMaxBatch * sizeof(int)));
            VF_HIP(launch_prep_q8(qn_b, nb, ix->d, ix->dp, qt, s.image_i8, (signed char*)s.qimg8.p, s.qscale.as<float>(), s.epsq.as<float>(), s.bandq.as<int>(),
                                  p.eps, p.tau_band, p.fine_band, st));
            a.qimg = (const _Float16*)s.qimg8.p; a.q_scale = s.qscale.as<float>(); a.band_q = s.bandq.as<int>();
        }
        if (p.image) { a.rows = (const char*)ix->rows_img; a.inv_scan = ix->inv_img; a.off_scan = image_offsets(ix); a.row_bytes = ix->dp; }   // every pass of the batch: sample, seed, main
        a.total_waves = p.total_waves; a.samp = p.samp; a.tau_band = p.tau_band; a.stage_cap = b.stage_cap; a.refresh_every = b.refresh_every;
        a.tile_cnt = ix->opt.steal ? s.tilecnt.as<u32>() : nullptr; a.scan_grid = p.grid;
        if (debug & 128) { VF_TRY(s.dbg.ensure((size_t)p.total_waves * ((debug & 512) ? 72 : 4) * sizeof(u64))); a.dbg = s.dbg.as<u64>(); if (debug & 512) VF_HIP(hipMemsetAsync(s.dbg.p, 0, s.dbg.bytes, st)); }
        // sample slots no wave writes (a wave range shorter than samp) must read as empty: 0xFF bytes
        // are a NaN, which k_sel0's "v > -inf" test skips.
        if (b.clear_sample)
            VF_HIP(hipMemsetAsync(a.s0, 0xFF, (size_t)qt * p.total_waves * p.samp * sizeof(float), st));
        switch (b.sample) {
        case kKernelKsplit: VF_HIP(launch_scan_ksplit(a, kModeSample, b.sample_grid, st)); break;
        case kKernelKsplit8: VF_HIP(launch_scan_ksplit8(a, kModeSample, b.sample_grid, b.sample_rows, st)); break;
        case kKernelScan2r: {
            ScanArgs as = a;
            as.stage_cap = 0;
            VF_HIP(launch_scan2r_sample(as, qt, b.sample_grid, b.sample_rows, st));
            break;
        }
        default: VF_HIP(launch_scan(a, kModeSample, qt, b.sample_grid, (int)ix->opt.scan_g, b.sample_rows, st));
        }
        VF_HIP(launch_sel0(a, qt, st));
        if (sst != st) {   // the main scan runs on the CU-masked stream, behind this slot's prologue
            VF_HIP(hipEventRecord(s.ev_pro, st));
            VF_HIP(hipStreamWaitEvent(sst, s.ev_pro, 0));
        }
        // Main scans of different slots run one after the other (a scan workgroup owns its CU); ordering them explicitly
        // keeps queueing time out of the timed bracket.  With overlap_scans they are left to the dispatcher: the next
        // scan's workgroups start on the CUs the previous one has finished with (no idle tail), at the price of that bracket.
        if (!route_overlap(in))
            for (int o = 0; o < kSlots; ++o)
                if (o != slot_id && ix->slots[o].ev_scan) VF_HIP(hipStreamWaitEvent(sst, ix->slots[o].ev_scan, 0));
        if (timed) {
            if (!ix->span_started) {   // makespan of the timed launches: from here to the last launch's end (vf_index_profile_span)
                if (!ix->ev_span) VF_HIP(hipEventCreate(&ix->ev_span));
                VF_HIP(hipEventRecord(ix->ev_span, sst));
                ix->span_started = true;
            }
            ix->span_slot[slot_id] = true;
            VF_HIP(hipEventRecord(s.ev_t[0], sst));
        }
        switch (b.main) {
        case kKernelKsplit8: VF_HIP(launch_scan_ksplit8(a, kModeMain, p.grid, b.main_rows, sst)); break;
        case kKernelKsplit: VF_HIP(launch_scan_ksplit(a, kModeMain, p.grid, sst)); break;
        case kKernelScan2r: VF_HIP(launch_scan2r(a, qt, p.grid, b.main_rows, sst)); break;
        case kKernelScan2: {
            ScanArgs a2 = a;
#ifdef VF_EXPERIMENTS
            if (debug & 32) {   // timing experiment: compute unit -> range table (k_scan2, debug bit 5)
                const bool fresh = s.sib.bytes < 4096;
                VF_TRY(s.sib.ensure(4096));
                if (fresh) VF_HIP(hipMemsetAsync(s.sib.p, 0xFF, 4096, st));
                a2.sib = s.sib.as<u32>();
            }
#endif
            VF_HIP(launch_scan2(a2, qt, p.grid, b.main_rows, sst));
            break;
        }
        default: VF_HIP(launch_scan(a, kModeMain, qt, p.grid, (int)ix->opt.scan_g, b.main_rows, sst));
        }
        s.scan_kernel = b.main;
        VF_HIP(hipEventRecord(s.ev_scan, sst));
        if (timed) {
            VF_HIP(hipEventRecord(s.ev_t[1], sst));
            ix->prof_bytes = b.scan_bytes;
        }
        if (sst != st) VF_HIP(hipStreamWaitEvent(st, s.ev_scan, 0));
        FinalArgs f = final_args(ix, s, p, s.k, qn_b, s.d_ids + (size_t)b0 * s.k, s.d_scores + (size_t)b0 * s.k, b0);
        f.band = p.fine_band;
        if (s.image_i8) { f.eps_q = s.epsq.as<float>(); f.band_q = s.bandq.as<int>() + qt; }
        if (debug & 256) { VF_TRY(s.dbg.ensure((size_t)std::max(p.total_waves * 4, 64 * 8) * sizeof(u64))); f.dbg = s.dbg.as<u64>(); }
        VF_HIP(launch_final(f, nb, st));
    }
    if (s.timed) VF_HIP(hipEventRecord(s.ev_t[3], st));
    return VF_OK;
}

static int begin_impl(vf_index* ix, int slot_id, const float* d_queries, int nq, int k, int64_t* d_ids,
                      float* d_scores, hipStream_t user) {
    Slot& s = ix->slots[slot_id];
    if (s.pending) return fail(VF_EINVAL, "vf_index_search_begin: slot already has a pending search");
    const int path = route_path(route_in(ix), k);
    if (path < 0) return fail(VF_EUNSUPPORTED, "forced fused path is not possible for this n / k / d");
    if (path != 1 && ix->n > kSmallN && k > 8192)  // checked before anything is enqueued (k_merge_topk's LDS sort)
        return fail(VF_EUNSUPPORTED, "exact chunked search supports k <= 8192 when n > 16384");
    VF_TRY(ensure_slot(ix, s));
    VF_HIP(hipEventRecord(s.ev_in, user));
    VF_HIP(hipStreamWaitEvent(s.stream, s.ev_in, 0));
    // (after ensure_slot: the plan's grid and the sample pass follow the CU split as it was applied to this slot's streams)
    const RouteIn in = route_in(ix, &s);
    const SearchRoute r = route_search(in, nq, k);
    VF_TRY(s.qn.ensure((size_t)std::max(nq, 1) * ix->d * sizeof(float)));
    VF_TRY(s.qimg.ensure(scan_lds_bytes(ix->dp, kMaxBatch)));
    VF_TRY(ensure_pinned(s, (size_t)nq));
    s.pending = true; s.d_queries = d_queries; s.nq = nq; s.k = k; s.d_ids = d_ids; s.d_scores = d_scores;
    s.path = path; s.user_stream = user; s.wide_launches = 0; s.wide_queries = 0; s.scan_kernel = 0;
    if (nq > 0 && k > 0) {
        if (path != 1) VF_TRY(begin_exact(ix, s, r.per_pass));
        else {
            s.scan_image = r.image ? 1 : 0;
            s.image_i8 = r.planes;
            VF_TRY(r.wide ? begin_wide(ix, slot_id, in, r) : begin_narrow(ix, slot_id, in, r));
        }
    }
    VF_HIP(hipEventRecord(s.ev_done, s.stream));
    return VF_OK;
}

// repair: exact chunked search for the flagged queries `redo` of the slot's search only (still on the GPU), waited for
static int repair_flagged(vf_index* ix, Slot& s, const std::vector<int>& redo) {
    const int m = (int)redo.size();
    hipStream_t st = s.stream;
    VF_TRY(s.qsel.ensure((size_t)m * ix->d * sizeof(float) + (size_t)m * s.k * (sizeof(long long) + sizeof(float))));
    float* qsel = s.qsel.as<float>();
    long long* rid = (long long*)(qsel + (size_t)m * ix->d);
    float* rsc = (float*)(rid + (size_t)m * s.k);
    for (int i = 0; i < m; ++i)
        VF_HIP(hipMemcpyAsync(qsel + (size_t)i * ix->d, s.qn.as<float>() + (size_t)redo[i] * ix->d,
                              (size_t)ix->d * sizeof(float), hipMemcpyDeviceToDevice, st));
    for (int i0 = 0; i0 < m; i0 += kMaxBatch) {
        const int nb = std::min(kMaxBatch, m - i0);
        VF_TRY(exact_search(ix, s, qsel + (size_t)i0 * ix->d, nb, s.k, (int64_t*)(rid + (size_t)i0 * s.k),
                            rsc + (size_t)i0 * s.k, st));
    }
    for (int i = 0; i < m; ++i) {
        VF_HIP(hipMemcpyAsync(s.d_ids + (size_t)redo[i] * s.k, rid + (size_t)i * s.k, (size_t)s.k * sizeof(long long),
                              hipMemcpyDeviceToDevice, st));
        VF_HIP(hipMemcpyAsync(s.d_scores + (size_t)redo[i] * s.k, rsc + (size_t)i * s.k, (size_t)s.k * sizeof(float),
                              hipMemcpyDeviceToDevice, st));
    }
    VF_HIP(hipEventRecord(s.ev_done, st));
    VF_HIP(hipEventSynchronize(s.ev_done));
    return VF_OK;
}

// (Round 6 measured a poll-then-block wait here -- hipEventQuery for up to 3 ms before hipEventSynchronize -- against the plain blocking
//  call, alternating processes, at 1M / 1.25M / 10M rows: no difference (0.2939-0.2943 vs 0.2933-0.2954 ms per batch at 1M): the
//  runtime's own wait already polls.  profiles/r06_spin_wait_ab.log)
static int end_impl(vf_index* ix, int slot_id) {
    Slot& s = ix->slots[slot_id];
    if (!s.pending) return fail(VF_EINVAL, "vf_index_search_end: slot has no pending search");
    s.pending = false;
    VF_HIP(hipEventSynchronize(s.ev_done));
    vf_search_stats stt{};
    stt.path = s.path; stt.n_queries = s.nq; stt.wide_launches = s.wide_launches; stt.wide_queries = s.wide_queries;
    const SplitReport split = route_split_report(route_in(ix, &s), s.path);
    stt.aux_cus = split.aux_cus;
    stt.scans_overlap = split.scans_overlap;
    stt.scan_kernel = s.scan_kernel;
    stt.scan_image = (s.path == 1) ? s.scan_image : 0;
    if (s.path == 1 && s.nq > 0 && s.k > 0) {
        if (s.timed) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, s.ev_t[0], s.ev_t[1]) == hipSuccess) { ix->prof_scan_ms += ms; ++ix->prof_launches; }
            if (hipEventElapsedTime(&ms, s.ev_t[2], s.ev_t[3]) == hipSuccess) ix->prof_pipe_ms += ms;
            s.timed = false;
        }
        std::vector<int> redo;
        for (int q = 0; q < s.nq; ++q) {
            stt.candidates += s.h_counts[q];
            stt.max_candidates = std::max<int64_t>(stt.max_candidates, s.h_counts[q]);
            if (s.h_flags[q] == 1) ++stt.uncertified;
            if (s.h_flags[q] == 2) ++stt.overflowed;
            if (s.h_flags[q] != 0) redo.push_back(q);
        }
        if (!redo.empty()) {
            VF_TRY(repair_flagged(ix, s, redo));
            stt.exact_reruns = (int)redo.size();
        }
    }
    // later work on the caller's stream sees the results
    VF_HIP(hipStreamWaitEvent(s.user_stream, s.ev_done, 0));
    ix->stats = stt;
    return VF_OK;
}

static int check_search_args(vf_index* ix, const void* q, int nq, int k, const void* ids, const void* sc) {
    if (!ix) return fail(VF_EINVAL, "search: null handle");
    if (nq < 0 || k < 0) return fail(VF_EINVAL, "search: negative nq / k");
    if (nq > 0 && k > 0 && (!q || !ids || !sc)) return fail(VF_EINVAL, "search: null buffer");
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------
// Group handle: ONE process, several devices (the reference's serve path is a single process: RAGManager singleton,
// src/utils/ragManager.py:17-30, building EnsembleRetriever -> FaissRetriever at ensembleRetriever.py:39-43).  Rows are
// split into contiguous blocks, one vf_index per device; a search copies the queries from the home
// device to every shard over xGMI peer copies, runs all shard searches concurrently (each on its own device streams),
// copies the packed per-shard top-k back to the home device and merges them there with k_merge_topk.  No host thread
// per device and no RCCL communicator are needed: the exchange is G small peer-to-peer copies (77 KB each at nq = 64,
// k = 100), which is what an all-gather over point-to-point xGMI links amounts to for one receiver.
// ------------------------------------------------------------------------------------------------
static int group_ensure_slot(vf_index* ix, GroupSlot& gs) {
    const size_t G = ix->shards.size();
    if (gs.feed.size() == G) return VF_OK;
    gs.feed.assign(G, nullptr); gs.ev.assign(G, nullptr);
    gs.dq.resize(G); gs.blob.resize(G);
    for (size_t g = 0; g < G; ++g) {
        VF_HIP(hipSetDevice(ix->shards[g]->device));
        VF_HIP(hipStreamCreateWithFlags(&gs.feed[g], hipStreamNonBlocking));
        VF_HIP(hipEventCreateWithFlags(&gs.ev[g], hipEventDisableTiming));
    }
    VF_HIP(hipSetDevice(ix->device));
    VF_HIP(hipEventCreateWithFlags(&gs.ev_in, hipEventDisableTiming));
    gs.hfeed.assign(G, nullptr); gs.ev_hb.assign(G, nullptr); gs.ev_home.assign(G, nullptr); gs.hb.resize(G); gs.staged_last.assign(G, 0);
    return VF_OK;
}

static bool shard_is_staged(const vf_index* ix, size_t g) { return g < ix->peer_ok.size() && !ix->peer_ok[g]; }

// streams / events of the host-staged exchange for shard g (first use)
static int group_ensure_staged(vf_index* ix, GroupSlot& gs, size_t g) {
    if (!gs.hq_stream) {
        VF_HIP(hipSetDevice(ix->device));
        VF_HIP(hipStreamCreateWithFlags(&gs.hq_stream, hipStreamNonBlocking));
        VF_HIP(hipEventCreateWithFlags(&gs.ev_hq, hipEventDisableTiming));
    }
    if (!gs.hfeed[g]) {
        VF_HIP(hipSetDevice(ix->device));
        VF_HIP(hipStreamCreateWithFlags(&gs.hfeed[g], hipStreamNonBlocking));
        VF_HIP(hipEventCreateWithFlags(&gs.ev_home[g], hipEventDisableTiming));
        VF_HIP(hipSetDevice(ix->shards[g]->device));
        VF_HIP(hipEventCreateWithFlags(&gs.ev_hb[g], hipEventDisableTiming));
    }
    return VF_OK;
}

static int group_begin(vf_index* ix, int slot_id, const float* d_queries, int nq, int k, int64_t* d_ids, float* d_scores,
                       hipStream_t user) {
    GroupSlot& gs = ix->gslots[slot_id];
    if (gs.pending) return fail(VF_EINVAL, "vf_index_search_begin: slot already has a pending search");
    const size_t G = ix->shards.size();
    if ((size_t)G * k > 16384) return fail(VF_EUNSUPPORTED, "sharded search: shards * k > 16384");
    VF_TRY(group_ensure_slot(ix, gs));
    gs.nq = nq; gs.k = k; gs.d_ids = d_ids; gs.d_scores = d_scores; gs.user = user;
    if (nq == 0 || k == 0) { gs.pending = true; return VF_OK; }
    const size_t qbytes = (size_t)nq * ix->d * sizeof(float);
    const size_t part = (size_t)packed_part_bytes(nq, k);
    VF_HIP(hipSetDevice(ix->device));
    VF_TRY(gs.all.ensure(G * part));
    VF_HIP(hipEventRecord(gs.ev_in, user));
    size_t started = 0;
    int rc = VF_OK;
    bool host_copy_issued = false;
    for (size_t g = 0; g < G && rc == VF_OK; ++g) {
        vf_index* sh = ix->shards[g];
        const bool staged = shard_is_staged(ix, g);
        hipError_t e = hipSuccess;
        if (staged) {   // home -> pinned host (once per search, on a home-device stream) -> shard g (on its feed stream)
            if ((rc = group_ensure_staged(ix, gs, g)) != VF_OK) break;
            if (!host_copy_issued) {
                if ((rc = gs.hq.ensure(qbytes)) != VF_OK) break;
                e = hipSetDevice(ix->device);
                if (e == hipSuccess) e = hipStreamWaitEvent(gs.hq_stream, gs.ev_in, 0);
                if (e == hipSuccess) e = hipMemcpyAsync(gs.hq.p, d_queries, qbytes, hipMemcpyDeviceToHost, gs.hq_stream);
                if (e == hipSuccess) e = hipEventRecord(gs.ev_hq, gs.hq_stream);
                if (e != hipSuccess) { rc = fail(VF_EHIP, std::string("sharded search: staged query copy (home -> host): ") + hipGetErrorString(e)); break; }
                host_copy_issued = true;
            }
        }
        e = hipSetDevice(sh->device);
        if (e == hipSuccess) e = hipStreamWaitEvent(gs.feed[g], staged ? gs.ev_hq : gs.ev_in, 0);
        if (e != hipSuccess) { rc = fail(VF_EHIP, std::string("sharded search: ") + hipGetErrorString(e)); break; }
        if ((rc = gs.dq[g].ensure(qbytes)) != VF_OK || (rc = gs.blob[g].ensure(part)) != VF_OK) break;
        if (staged) e = hipMemcpyAsync(gs.dq[g].p, gs.hq.p, qbytes, hipMemcpyHostToDevice, gs.feed[g]);
        else e = hipMemcpyPeerAsync(gs.dq[g].p, sh->device, d_queries, ix->device, qbytes, gs.feed[g]);
        if (e != hipSuccess) { rc = fail(VF_EHIP, std::string("sharded search: query ") + (staged ? "staged" : "peer") + " copy: " + hipGetErrorString(e)); break; }
        std::lock_guard<std::mutex> lk(sh->mu);
        rc = begin_impl(sh, slot_id, gs.dq[g].as<float>(), nq, k, (int64_t*)gs.blob[g].p,
                        (float*)((char*)gs.blob[g].p + (size_t)nq * k * 8), gs.feed[g]);
        if (rc == VF_OK) ++started; else sh->slots[slot_id].pending = false;
    }
    if (rc != VF_OK) {  // let the shards that did start finish, then report
        const std::string keep = g_err;
        for (size_t g = 0; g < started; ++g) {
            (void)hipSetDevice(ix->shards[g]->device);
            std::lock_guard<std::mutex> lk(ix->shards[g]->mu);
            (void)end_impl(ix->shards[g], slot_id);
        }
        g_err = keep;
        return rc;
    }
    gs.pending = true;
    return VF_OK;
}

static int group_end(vf_index* ix, int slot_id) {
    GroupSlot& gs = ix->gslots[slot_id];
    if (!gs.pending) return fail(VF_EINVAL, "vf_index_search_end: slot has no pending search");
    gs.pending = false;
    vf_search_stats tot{};
    tot.n_queries = gs.nq;
    if (gs.nq == 0 || gs.k == 0) { ix->stats = tot; return VF_OK; }
    const size_t G = ix->shards.size();
    const size_t part = (size_t)packed_part_bytes(gs.nq, gs.k);
    int rc = VF_OK;
    for (size_t g = 0; g < G; ++g) {  // every shard is ended even after a failure: no slot may stay pending
        vf_index* sh = ix->shards[g];
        (void)hipSetDevice(sh->device);
        int r;
        {
            std::lock_guard<std::mutex> lk(sh->mu);
            r = end_impl(sh, slot_id);  // waits for the shard, certifies, repairs; feed[g] is ordered after the result
            if (r == VF_OK) {
                const vf_search_stats& st = sh->stats;
                tot.path = std::max(tot.path, st.path);
                tot.candidates += st.candidates; tot.max_candidates = std::max(tot.max_candidates, st.max_candidates);
                tot.uncertified += st.uncertified; tot.overflowed += st.overflowed; tot.exact_reruns += st.exact_reruns;
                tot.wide_launches = std::max(tot.wide_launches, st.wide_launches); tot.wide_queries = std::max(tot.wide_queries, st.wide_queries);
                tot.aux_cus = std::max(tot.aux_cus, st.aux_cus); tot.scans_overlap = std::max(tot.scans_overlap, st.scans_overlap);
                tot.scan_kernel = std::max(tot.scan_kernel, st.scan_kernel);
                tot.scan_image = std::max(tot.scan_image, st.scan_image);
            }
        }
        if (r == VF_OK && !shard_is_staged(ix, g)) {
            hipError_t e = hipMemcpyPeerAsync((char*)gs.all.p + g * part, ix->device, gs.blob[g].p, sh->device, part, gs.feed[g]);
            if (e == hipSuccess) e = hipEventRecord(gs.ev[g], gs.feed[g]);
            if (e != hipSuccess) r = fail(VF_EHIP, std::string("sharded search: result peer copy: ") + hipGetErrorString(e));
            gs.staged_last[g] = 0;
        } else if (r == VF_OK) {   // shard -> pinned host on the shard's stream, host -> `all` on a home-device stream
            r = gs.hb[g].ensure(part);
            hipError_t e = hipSuccess;
            // hb[g] is free again once the PREVIOUS search's host -> home copy out of it has run
            if (r == VF_OK && gs.staged_last[g]) e = hipStreamWaitEvent(gs.feed[g], gs.ev_home[g], 0);
            if (r == VF_OK && e == hipSuccess) e = hipMemcpyAsync(gs.hb[g].p, gs.blob[g].p, part, hipMemcpyDeviceToHost, gs.feed[g]);
            if (r == VF_OK && e == hipSuccess) e = hipEventRecord(gs.ev_hb[g], gs.feed[g]);
            if (r == VF_OK && e == hipSuccess) e = hipSetDevice(ix->device);
            if (r == VF_OK && e == hipSuccess) e = hipStreamWaitEvent(gs.hfeed[g], gs.ev_hb[g], 0);
            if (r == VF_OK && e == hipSuccess) e = hipMemcpyAsync((char*)gs.all.p + g * part, gs.hb[g].p, part, hipMemcpyHostToDevice, gs.hfeed[g]);
            if (r == VF_OK && e == hipSuccess) e = hipEventRecord(gs.ev_home[g], gs.hfeed[g]);
            if (r == VF_OK && e != hipSuccess) r = fail(VF_EHIP, std::string("sharded search: staged result copy: ") + hipGetErrorString(e));
            if (r == VF_OK) gs.staged_last[g] = 1;
        }
        if (r != VF_OK && rc == VF_OK) rc = r;
    }
    if (rc != VF_OK) return rc;
    VF_HIP(hipSetDevice(ix->device));
    VF_HIP(scan_configure());
    for (size_t g = 0; g < G; ++g) VF_HIP(hipStreamWaitEvent(gs.user, shard_is_staged(ix, g) ? gs.ev_home[g] : gs.ev[g], 0));
    // parts are in ascending id-range order (shard order), which the merge's tie rule relies on
    VF_HIP(launch_merge_topk_packed(gs.all.p, (int)G, gs.nq, gs.k, (long long*)gs.d_ids, gs.d_scores, gs.user));
    ix->stats = tot;
    return VF_OK;
}

static int search_begin_locked(vf_index* ix, int slot, const float* d_queries, int nq, int k, int64_t* d_ids,
                               float* d_scores, hipStream_t stream) {
    if (ix->damaged) return fail(VF_EHIP, std::string("vf_index_search: ") + kDamagedMsg);
    if (!ix->shards.empty()) return group_begin(ix, slot, d_queries, nq, k, d_ids, d_scores, stream);
    VF_HIP(hipSetDevice(ix->device));
    int rc = begin_impl(ix, slot, d_queries, nq, k, d_ids, d_scores, stream);
    if (rc != VF_OK) ix->slots[slot].pending = false;
    return rc;
}

static int search_end_locked(vf_index* ix, int slot) {
    if (!ix->shards.empty()) return group_end(ix, slot);
    VF_HIP(hipSetDevice(ix->device));
    return end_impl(ix, slot);
}

static bool slot_pending(const vf_index* ix, int slot) {
    return ix->shards.empty() ? ix->slots[slot].pending : ix->gslots[slot].pending;
}

extern "C" int vf_index_search_begin(vf_index* ix, int32_t slot, const float* d_queries, int32_t nq, int32_t k,
                                     int64_t* d_ids, float* d_scores, void* stream) {
    DeviceGuard restore_callers_device;
    VF_TRY(check_search_args(ix, d_queries, nq, k, d_ids, d_scores));
    if (slot < 0 || slot >= kSlots) return fail(VF_EINVAL, "vf_index_search_begin: bad slot");
    std::lock_guard<std::mutex> g(ix->mu);
    return search_begin_locked(ix, slot, d_queries, nq, k, d_ids, d_scores, (hipStream_t)stream);
}

extern "C" int vf_index_search_end(vf_index* ix, int32_t slot) {
    DeviceGuard restore_callers_device;
    if (!ix) return fail(VF_EINVAL, "vf_index_search_end: null handle");
    if (slot < 0 || slot >= kSlots) return fail(VF_EINVAL, "vf_index_search_end: bad slot");
    std::lock_guard<std::mutex> g(ix->mu);
    return search_end_locked(ix, slot);
}

static int search_device_locked(vf_index* ix, const float* d_queries, int nq, int k, int64_t* d_ids, float* d_scores,
                                hipStream_t stream) {
    if (slot_pending(ix, 0)) return fail(VF_EINVAL, "vf_index_search_device: slot 0 busy (begin without end)");
    VF_TRY(search_begin_locked(ix, 0, d_queries, nq, k, d_ids, d_scores, stream));
    return search_end_locked(ix, 0);
}

// the subset forms of the two search entry points (nq carries VF_SEARCH_SUBSET, `queries` is a vf_subset_query): defined with the
// subset search, below
static int subset_entry_host(vf_index* ix, const vf_subset_query* sq, int32_t nq, int32_t k, int64_t* out_ids, float* out_scores);
static int subset_entry_device(vf_index* ix, const vf_subset_query* sq, int32_t nq, int32_t k, int64_t* d_out_ids, float* d_out_scores, void* stream);
// ... and the form with a list per query (VF_SEARCH_SUBSETS, `queries` is a vf_subsets_query); both flags together are refused there
static int subsets_entry(vf_index* ix, const vf_subsets_query* sq, int32_t nq_flags, int32_t k, int64_t* out_ids, float* out_scores, bool device, void* stream);
// ... and a metadata filter evaluated into a bitmap and an id list (VF_SEARCH_WHERE, `queries` is a vf_where_query; the device form only)
static int where_entry(vf_index* ix, vf_where_query* wq, int32_t nq_flags, bool device, void* stream);

extern "C" int vf_index_search_device(vf_index* ix, const float* d_queries, int32_t nq, int32_t k, int64_t* d_ids,
                                      float* d_scores, void* stream) {
    if (nq >= 0 && (nq & VF_SEARCH_WHERE)) return where_entry(ix, (vf_where_query*)d_queries, nq, true, stream);
    if (nq >= 0 && (nq & VF_SEARCH_SUBSETS)) return subsets_entry(ix, (const vf_subsets_query*)d_queries, nq, k, d_ids, d_scores, true, stream);
    if (nq >= 0 && (nq & VF_SEARCH_SUBSET)) return subset_entry_device(ix, (const vf_subset_query*)d_queries, nq & ~VF_SEARCH_SUBSET, k, d_ids, d_scores, stream);
    DeviceGuard restore_callers_device;
    VF_TRY(check_search_args(ix, d_queries, nq, k, d_ids, d_scores));
    std::lock_guard<std::mutex> g(ix->mu);
    return search_device_locked(ix, d_queries, nq, k, d_ids, d_scores, (hipStream_t)stream);
}

// Host buffers in and out: what FaissRetriever.invoke hands over (NumPy arrays, src/utils/faissRetriever.py:34-38).
// The device staging lives in the handle and is reused from call to call (no hipMalloc / hipFree per request); the
// handle's mutex is held for the whole call, so concurrent request threads take turns on it.
static int search_host_locked(vf_index* ix, const float* queries, int nq, int k, int64_t* out_ids, float* out_scores) {
    VF_HIP(hipSetDevice(ix->device));
    const size_t qb = (size_t)nq * ix->d * sizeof(float), ib = (size_t)nq * k * sizeof(int64_t), sb = (size_t)nq * k * sizeof(float);
    VF_TRY(ix->st_q.ensure(qb));
    VF_TRY(ix->st_ids.ensure(ib));
    VF_TRY(ix->st_sc.ensure(sb));
    VF_HIP(hipMemcpy(ix->st_q.p, queries, qb, hipMemcpyHostToDevice));
    VF_TRY(search_device_locked(ix, ix->st_q.as<float>(), nq, k, ix->st_ids.as<int64_t>(), ix->st_sc.as<float>(), nullptr));
    VF_HIP(hipSetDevice(ix->device));
    VF_HIP(hipStreamSynchronize(nullptr));
    VF_HIP(hipMemcpy(out_ids, ix->st_ids.p, ib, hipMemcpyDeviceToHost));
    VF_HIP(hipMemcpy(out_scores, ix->st_sc.p, sb, hipMemcpyDeviceToHost));
    return VF_OK;
}

extern "C" int vf_index_search(vf_index* ix, const float* queries, int32_t nq, int32_t k, int64_t* out_ids,
                               float* out_scores) {
    if (nq >= 0 && (nq & VF_SEARCH_WHERE)) return where_entry(ix, (vf_where_query*)queries, nq, false, nullptr);
    if (nq >= 0 && (nq & VF_SEARCH_SUBSETS)) return subsets_entry(ix, (const vf_subsets_query*)queries, nq, k, out_ids, out_scores, false, nullptr);
    if (nq >= 0 && (nq & VF_SEARCH_SUBSET)) return subset_entry_host(ix, (const vf_subset_query*)queries, nq & ~VF_SEARCH_SUBSET, k, out_ids, out_scores);
    DeviceGuard restore_callers_device;
    VF_TRY(check_search_args(ix, queries, nq, k, out_ids, out_scores));
    if (nq == 0 || k == 0) return VF_OK;
    std::lock_guard<std::mutex> g(ix->mu);
    return search_host_locked(ix, queries, nq, k, out_ids, out_scores);
}

static std::atomic<bool> g_force_no_peer{false};
// Test hook (not in the public header): handles grouped from now on treat EVERY shard as unreachable by peer copy.
extern "C" int vf_debug_force_no_peer(int32_t on) {
    return g_force_no_peer.exchange(on != 0) ? 1 : 0;
}

// Take ownership of per-device indexes (built with id_offset = first row of their block, in ascending block order)
// and present them as one index.  home = shards[0]'s device.
static int make_group(vf_index** out, std::vector<vf_index*>& shards) {
    vf_index* grp = new (std::nothrow) vf_index();
    if (!grp) return fail(VF_ENOMEM, "vf_index_group: host allocation failed");
    grp->device = shards[0]->device;
    grp->d = shards[0]->d; grp->dp = shards[0]->dp; grp->dtype = shards[0]->dtype; grp->id_offset = shards[0]->id_offset;
    grp->n_cu = shards[0]->n_cu;
    grp->n = 0;
    for (vf_index* sh : shards) grp->n += sh->n;
    grp->shards = shards;
    // peer access home <-> shard devices.  A link that cannot be enabled is not fatal -- hipMemcpyPeerAsync then stages
    // through the host -- but it is RECORDED (vf_index_peer_access) so that the slow exchange does not go unnoticed.
    auto enable = [](int from, int to) -> bool {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, from, to) != hipSuccess || !can) return false;
        if (hipSetDevice(from) != hipSuccess) return false;
        const hipError_t e = hipDeviceEnablePeerAccess(to, 0);
        (void)hipGetLastError();
        return e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
    };
    grp->peer_ok.assign(shards.size(), 1);
    const bool forced = g_force_no_peer.load(std::memory_order_relaxed);
    for (size_t g = 0; g < shards.size(); ++g) {
        // test hook: every shard -- the ones on the home device too -- takes the host-staged exchange, so that the path a refused
        // peer link falls to runs on a one-GPU box (device_ids = [0, 0]); nothing is enabled or disabled on the devices
        if (forced) { grp->peer_ok[g] = 0; continue; }
        if (shards[g]->device == grp->device) continue;
        const bool a = enable(grp->device, shards[g]->device), b = enable(shards[g]->device, grp->device);
        grp->peer_ok[g] = a && b ? 1 : 0;
    }
    (void)hipSetDevice(grp->device);
    *out = grp;
    return VF_OK;
}

extern "C" int vf_index_group(vf_index** out, vf_index** shards, int32_t n_shards) {
    DeviceGuard restore_callers_device;
    if (!out || !shards || n_shards <= 0) return fail(VF_EINVAL, "vf_index_group: bad argument");
    *out = nullptr;
    std::vector<vf_index*> v(shards, shards + n_shards);
    int64_t next = v[0] ? v[0]->id_offset : 0;
    for (vf_index* sh : v) {
        if (!sh || !sh->shards.empty()) return fail(VF_EINVAL, "vf_index_group: null or nested shard");
        if (sh->d != v[0]->d || sh->dtype != v[0]->dtype) return fail(VF_EINVAL, "vf_index_group: shards differ in d / dtype");
        if (sh->id_offset != next) return fail(VF_EINVAL, "vf_index_group: shards must be contiguous row blocks in ascending order");
        next += sh->n;
    }
    return make_group(out, v);
}

static int check_devices(const int32_t* device_ids, int32_t n_dev, const char* who) {
    if (!device_ids || n_dev <= 0 || n_dev > 64) return fail(VF_EINVAL, std::string(who) + ": bad device list");
    int ndev = 0;
    VF_HIP(hipGetDeviceCount(&ndev));
    for (int i = 0; i < n_dev; ++i)
        if (device_ids[i] < 0 || device_ids[i] >= ndev) return fail(VF_EINVAL, std::string(who) + ": bad device id");
    return VF_OK;
}

static void shard_block(int64_t n, int n_dev, int g, int64_t* lo, int64_t* hi) {  // SURVEY.md 8e partitioning
    const int64_t per = (n + n_dev - 1) / n_dev;
    *lo = std::min<int64_t>(n, (int64_t)g * per);
    *hi = std::min<int64_t>(n, *lo + per);
}

extern "C" int vf_index_create_sharded(vf_index** out, const void* rows, int64_t n, int32_t d, int32_t dtype,
                                       const int32_t* device_ids, int32_t n_dev) {
    DeviceGuard restore_callers_device;
    if (!out) return fail(VF_EINVAL, "vf_index_create_sharded: null out");
    *out = nullptr;
    VF_TRY(check_devices(device_ids, n_dev, "vf_index_create_sharded"));
    if (n < 0 || d <= 0 || (n > 0 && !rows)) return fail(VF_EINVAL, "vf_index_create_sharded: bad rows/n/d");
    if (!known_dtype(dtype)) return fail(VF_EINVAL, "vf_index_create_sharded: unknown dtype");
    const size_t esz = dtype_bytes(dtype);
    std::vector<vf_index*> shards;
    int rc = VF_OK;
    for (int g = 0; g < n_dev && rc == VF_OK; ++g) {
        int64_t lo, hi;
        shard_block(n, n_dev, g, &lo, &hi);
        vf_index* sh = nullptr;
        rc = create_impl(&sh, (const char*)rows + (size_t)lo * d * esz, false, hi - lo, d, dtype, device_ids[g], lo);
        if (rc == VF_OK) shards.push_back(sh);
    }
    if (rc == VF_OK) rc = make_group(out, shards);
    if (rc != VF_OK) { const std::string keep = g_err; for (vf_index* sh : shards) destroy_index(sh); g_err = keep; }
    return rc;
}

extern "C" int vf_index_create_sharded_from_file(vf_index** out, const char* path, const int32_t* device_ids, int32_t n_dev) {
    DeviceGuard restore_callers_device;
    if (!out || !path) return fail(VF_EINVAL, "vf_index_create_sharded_from_file: null argument");
    *out = nullptr;
    VF_TRY(check_devices(device_ids, n_dev, "vf_index_create_sharded_from_file"));
    int64_t n = 0;
    VF_TRY(vf_corpus_file_info(path, &n, nullptr, nullptr, nullptr));
    std::vector<vf_index*> shards;
    int rc = VF_OK;
    for (int g = 0; g < n_dev && rc == VF_OK; ++g) {
        int64_t lo, hi;
        shard_block(n, n_dev, g, &lo, &hi);
        vf_index* sh = nullptr;
        rc = vf_index_create_from_file(&sh, path, lo, hi, device_ids[g], lo);
        if (rc == VF_OK) shards.push_back(sh);
    }
    if (rc == VF_OK) rc = make_group(out, shards);
    if (rc != VF_OK) { const std::string keep = g_err; for (vf_index* sh : shards) destroy_index(sh); g_err = keep; }
    return rc;
}

extern "C" int vf_index_shards(vf_index* ix, int32_t* n_shards, int32_t* device_ids, int32_t cap) {
    if (!ix || !n_shards) return fail(VF_EINVAL, "vf_index_shards: null argument");
    const int G = (int)ix->shards.size();
    *n_shards = G;
    for (int g = 0; g < G && g < cap && device_ids; ++g) device_ids[g] = ix->shards[g]->device;
    return VF_OK;
}

extern "C" int vf_index_peer_access(vf_index* ix, int32_t* ok, int32_t cap, int32_t* n_missing) {
    if (!ix) return fail(VF_EINVAL, "vf_index_peer_access: null handle");
    int missing = 0;
    for (size_t g = 0; g < ix->peer_ok.size(); ++g) {
        if (ok && (int)g < cap) ok[g] = ix->peer_ok[g];
        missing += ix->peer_ok[g] ? 0 : 1;
    }
    if (n_missing) *n_missing = missing;
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------
// small dense cosine (compute_similarity_mtx / cosine_similarity restatements)
//
// These entry points sit on the serve chain (rank_chunk calls two of them per request) and used to pay 3 - 8 hipMalloc / hipFree
// pairs per call.  They now lease ONE arena from a small process-wide pool: a call pops an arena of its device (or makes one),
// carves its buffers out of it and pushes it back -- concurrent request threads each hold their own, none waits for another, and
// nothing hangs on thread-exit destructors.  Arenas above 64 MB and arenas beyond eight go back to the driver on release.
// ------------------------------------------------------------------------------------------------
namespace {
struct Arena { int device = -1; DevBuf buf; };
std::mutex g_arena_mu;
std::vector<Arena*> g_arena_free;
std::atomic<long long> g_arena_allocs{0};            // hipMalloc calls made for arenas (test hook: vf_debug_small_allocs)
constexpr size_t kArenaKeepBytes = (size_t)64 << 20, kArenaKeepCount = 8;

struct Lease {
    Arena* a = nullptr;
    size_t used = 0;
    // the caller has made `device` current
    int acquire(int device, size_t bytes) {
        {
            std::lock_guard<std::mutex> lk(g_arena_mu);
            int best = -1;
            for (int i = 0; i < (int)g_arena_free.size(); ++i)
                if (g_arena_free[i]->device == device && (best < 0 || g_arena_free[i]->buf.bytes > g_arena_free[best]->buf.bytes)) best = i;
            if (best >= 0) { a = g_arena_free[best]; g_arena_free.erase(g_arena_free.begin() + best); }
        }
        if (!a) { a = new (std::nothrow) Arena(); if (!a) return fail(VF_ENOMEM, "small-op arena: host allocation failed"); a->device = device; }
        if (bytes > a->buf.bytes) g_arena_allocs.fetch_add(1, std::memory_order_relaxed);
        const int rc = a->buf.ensure(bytes);
        if (rc != VF_OK) { a->buf.release(); delete a; a = nullptr; }
        return rc;
    }
    static size_t padded(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    template <class T> T* take(size_t count) {
        T* p = (T*)((char*)a->buf.p + used);
        used += padded(count * sizeof(T));
        return p;
    }
    ~Lease() {
        if (!a) return;
        std::unique_lock<std::mutex> lk(g_arena_mu);
        if (a->buf.bytes <= kArenaKeepBytes && g_arena_free.size() < kArenaKeepCount) { g_arena_free.push_back(a); return; }
        lk.unlock();
        a->buf.release();
        delete a;
    }
};
}  // namespace

// Test hook (not in the public header): resident workgroups per CU of k_scan_wide8<waves> with `stage_cap` candidate-stage entries
extern "C" int vf_debug_wide8_occupancy(int32_t waves, int32_t stage_cap) {
    if (scan_configure() != hipSuccess) return -1;
    return scan_wide8_occupancy(waves, stage_cap > 0 ? stage_cap : scan_wide8_stage_cap(waves));
}

// Test hook (not in the public header): arena allocations so far -- steady-state calls of the small entry points make none.
extern "C" long long vf_debug_small_allocs(void) { return g_arena_allocs.load(std::memory_order_relaxed); }

extern "C" int vf_cosine_scores(const float* a, int32_t na, const float* b, int64_t nb, int32_t d, float* out,
                                int32_t device_id) {
    DeviceGuard restore_callers_device;
    if (na < 0 || nb < 0 || d <= 0) return fail(VF_EINVAL, "vf_cosine_scores: bad sizes");
    if (na == 0 || nb == 0) return VF_OK;
    if (!a || !b || !out) return fail(VF_EINVAL, "vf_cosine_scores: null buffer");
    VF_HIP(hipSetDevice(device_id));
    const bool same = a == b && (int64_t)na == nb;       // vf_cosine_matrix: one operand, prepared once
    const size_t ea = (size_t)na * d, eb = same ? 0 : (size_t)nb * d;
    Lease ws;
    VF_TRY(ws.acquire(device_id, 2 * Lease::padded(ea * 4) + 2 * Lease::padded(eb * 4) + Lease::padded((size_t)na * 4) + Lease::padded((size_t)nb * 4) +
                                     Lease::padded((size_t)std::max<int64_t>(na, nb) * 4) + Lease::padded((size_t)na * nb * 4)));
    float* da = ws.take<float>(ea); float* an = ws.take<float>(ea);
    float* db = same ? da : ws.take<float>(eb); float* bn = same ? an : ws.take<float>(eb);
    float* norm_a = ws.take<float>(na); float* norm_b = same ? norm_a : ws.take<float>(nb);
    float* tmp = ws.take<float>(std::max<int64_t>(na, nb)); float* dout = ws.take<float>((size_t)na * nb);
    VF_HIP(hipMemcpy(da, a, ea * 4, hipMemcpyHostToDevice));
    if (!same) VF_HIP(hipMemcpy(db, b, eb * 4, hipMemcpyHostToDevice));
    VF_HIP(launch_prep_rows(da, 0, na, d, d, nullptr, norm_a, tmp, nullptr));
    if (!same) VF_HIP(launch_prep_rows(db, 0, nb, d, d, nullptr, norm_b, tmp, nullptr));
    VF_HIP(launch_normalize_rows(da, 0, 0, na, d, norm_a, an, nullptr));
    if (!same) VF_HIP(launch_normalize_rows(db, 0, 0, nb, d, norm_b, bn, nullptr));
    VF_HIP(launch_dense_dot16(an, na, bn, nb, d, dout, nb, nullptr));
    VF_HIP(hipMemcpy(out, dout, (size_t)na * nb * 4, hipMemcpyDeviceToHost));
    return VF_OK;
}

extern "C" int vf_cosine_matrix(const float* x, int32_t n, int32_t d, float* out, int32_t device_id) {
    return vf_cosine_scores(x, n, x, n, d, out, device_id);
}

// rows `sel` (local row numbers) of ONE device's index, canonically normalised, into xn [count][d] on that device (null stream)
static int gather_normalised(vf_index* sh, Lease& ws, const std::vector<long long>& sel, float* xn) {
    long long* dsel = ws.take<long long>(sel.size());
    VF_HIP(hipMemcpy(dsel, sel.data(), sel.size() * 8, hipMemcpyHostToDevice));
    VF_HIP(launch_normalize_rows_gather(sh->rows_orig, sh->dtype, dsel, (int)sel.size(), sh->d, sh->norm, xn, nullptr));
    return VF_OK;
}

// Cosine matrix of rows ALREADY in the index, picked by id (round 4): compute_similarity_mtx re-embeds the n retrieved chunk
// texts (src/utils/ensembleRetriever.py:265-281: n encoder forwards upstream, one batched forward here -- 19 ms for 100 chunks
// of 512 tokens); when the chunks came out of this index and the embedder treats documents and queries alike, their
// embeddings are rows of the HBM-resident corpus: gather + canonical normalise (the index's own norms) + dot16.
// A SHARDED handle (round 5): every shard normalises its own rows on its own device (the norms are per row, so the values are the
// single-device ones bit for bit), the blocks travel to the home device -- peer copy, or through the host where the link is
// missing -- and are put back into the caller's order there by the same gather kernel (norm 1: x * (float)(1.0 / 1.0) = x).
// Mixed form (round 6): ids[i] >= 0 picks a corpus row as above; ids[i] == -1 takes the next vector of `extra` ([n_extra][d] fp32
// host, in order of appearance) -- a chunk text the corpus does not hold, embedded by the caller.  Those vectors get the canonical
// norm of vf_cosine_matrix (k_prep_rows on fp32 values), so an all-extra call returns vf_cosine_matrix's bits and an all-row call
// vf_cosine_matrix_rows's.  This is what lets EnsembleRetriever.compute_similarity_mtx(texts) -- the reference's call, texts only
// (src/utils/vllmManager.py:462) -- serve known texts from HBM and embed only the unknown ones.
static int cosine_matrix_rows_impl(vf_index* ix, const int64_t* ids, int32_t n, const float* extra, int32_t n_extra, float* out,
                                   const char* who) {
    DeviceGuard restore_callers_device;
    if (!ix) return fail(VF_EINVAL, std::string(who) + ": null handle");
    if (ix->damaged) return fail(VF_EHIP, std::string(who) + ": " + kDamagedMsg);
    if (n < 0 || n_extra < 0) return fail(VF_EINVAL, std::string(who) + ": negative n");
    if (n == 0) return VF_OK;
    if (!ids || !out) return fail(VF_EINVAL, std::string(who) + ": null buffer");
    if (n > 4096) return fail(VF_EINVAL, std::string(who) + ": n must be <= 4096");
    if (n_extra > 0 && !extra) return fail(VF_EINVAL, std::string(who) + ": n_extra > 0 with a null extra buffer");
    const size_t nd = (size_t)n * ix->d;
    std::lock_guard<std::mutex> lk(ix->mu);
    int n_minus = 0;
    for (int i = 0; i < n; ++i) if (ids[i] == -1) ++n_minus;
    if (n_minus != n_extra) return fail(VF_EINVAL, std::string(who) + ": the ids hold " + std::to_string(n_minus) + " entries of -1 but n_extra is " + std::to_string(n_extra));
    if (ix->shards.empty() && n_extra == 0) {
        std::vector<long long> sel((size_t)n);
        for (int i = 0; i < n; ++i) {
            const int64_t r = ids[i] - ix->id_offset;
            if (r < 0 || r >= ix->n) return fail(VF_EINVAL, std::string(who) + ": id outside the index");
            sel[(size_t)i] = r;
        }
        VF_HIP(hipSetDevice(ix->device));
        Lease ws;
        VF_TRY(ws.acquire(ix->device, Lease::padded((size_t)n * 8) + Lease::padded(nd * 4) + Lease::padded((size_t)n * n * 4)));
        float* xn = ws.take<float>(nd); float* dout = ws.take<float>((size_t)n * n);
        VF_TRY(gather_normalised(ix, ws, sel, xn));
        VF_HIP(launch_dense_dot16(xn, n, xn, n, ix->d, dout, n, nullptr));
        VF_HIP(hipMemcpy(out, dout, (size_t)n * n * 4, hipMemcpyDeviceToHost));
        return VF_OK;
    }
    // general form: the blocks of the G shards (a plain handle is its own only shard), then the block of the extra vectors, meet in
    // `cat` on the home device and are put into the caller's order by one gather
    std::vector<vf_index*> parts = ix->shards;
    if (parts.empty()) parts.push_back(ix);
    const size_t G = parts.size();
    std::vector<std::vector<long long>> sel(G);
    std::vector<int> owner((size_t)n), rank_in((size_t)n);
    int seen_extra = 0;
    for (int i = 0; i < n; ++i) {
        if (ids[i] == -1) { owner[(size_t)i] = (int)G; rank_in[(size_t)i] = seen_extra++; continue; }
        size_t g = 0;
        while (g < G && !(ids[i] >= parts[g]->id_offset && ids[i] < parts[g]->id_offset + parts[g]->n)) ++g;
        if (g == G) return fail(VF_EINVAL, std::string(who) + ": id outside the index");
        owner[(size_t)i] = (int)g; rank_in[(size_t)i] = (int)sel[g].size();
        sel[g].push_back(ids[i] - parts[g]->id_offset);
    }
    std::vector<long long> start(G + 2, 0), where((size_t)n);   // block of shard g in the concatenation (block G: the extras); position i's row in it
    for (size_t g = 0; g < G; ++g) start[g + 1] = start[g] + (long long)sel[g].size();
    start[G + 1] = start[G] + n_extra;
    for (int i = 0; i < n; ++i) where[(size_t)i] = start[(size_t)owner[(size_t)i]] + rank_in[(size_t)i];
    const size_t ed = (size_t)n_extra * ix->d;
    VF_HIP(hipSetDevice(ix->device));
    Lease home;
    VF_TRY(home.acquire(ix->device, 2 * Lease::padded(nd * 4) + Lease::padded((size_t)n * 4) + Lease::padded((size_t)n * 8) + Lease::padded((size_t)n * n * 4) +
                                    Lease::padded(ed * 4) + 2 * Lease::padded((size_t)n_extra * 4)));
    float* cat = home.take<float>(nd); float* xn = home.take<float>(nd); float* ones = home.take<float>(n);
    long long* dwhere = home.take<long long>(n); float* dout = home.take<float>((size_t)n * n);
    std::vector<float> stage;
    for (size_t g = 0; g < G; ++g) {
        if (sel[g].empty()) continue;
        vf_index* sh = parts[g];
        const size_t cnt = sel[g].size(), bytes = cnt * ix->d * 4;
        float* dst = cat + (size_t)start[g] * ix->d;
        VF_HIP(hipSetDevice(sh->device));
        if (sh->device == ix->device && !shard_is_staged(ix, g)) {        // already at home: normalise straight into its block
            Lease ws;
            VF_TRY(ws.acquire(sh->device, Lease::padded(cnt * 8)));
            VF_TRY(gather_normalised(sh, ws, sel[g], dst));
            VF_HIP(hipStreamSynchronize(nullptr));
            continue;
        }
        Lease ws;
        VF_TRY(ws.acquire(sh->device, Lease::padded(cnt * 8) + Lease::padded(bytes)));
        float* part = ws.take<float>(cnt * ix->d);
        VF_TRY(gather_normalised(sh, ws, sel[g], part));
        VF_HIP(hipStreamSynchronize(nullptr));
        if (!shard_is_staged(ix, g)) {
            VF_HIP(hipMemcpyPeer(dst, ix->device, part, sh->device, bytes));
        } else {                                                          // no peer link: through the host
            stage.resize(cnt * ix->d);
            VF_HIP(hipMemcpy(stage.data(), part, bytes, hipMemcpyDeviceToHost));
            VF_HIP(hipSetDevice(ix->device));
            VF_HIP(hipMemcpy(dst, stage.data(), bytes, hipMemcpyHostToDevice));
        }
    }
    VF_HIP(hipSetDevice(ix->device));
    if (n_extra > 0) {   // the caller's vectors: canonical norms of their fp32 values (vf_cosine_matrix's arithmetic), normalised into block G
        float* raw = home.take<float>(ed); float* norm_e = home.take<float>(n_extra); float* tmp = home.take<float>(n_extra);
        VF_HIP(hipMemcpy(raw, extra, ed * 4, hipMemcpyHostToDevice));
        VF_HIP(launch_prep_rows(raw, 0, n_extra, ix->d, ix->d, nullptr, norm_e, tmp, nullptr));
        VF_HIP(launch_normalize_rows(raw, 0, 0, n_extra, ix->d, norm_e, cat + (size_t)start[G] * ix->d, nullptr));
    }
    const std::vector<float> one((size_t)n, 1.0f);
    VF_HIP(hipMemcpy(ones, one.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    VF_HIP(hipMemcpy(dwhere, where.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    VF_HIP(launch_normalize_rows_gather(cat, VF_DTYPE_F32, dwhere, n, ix->d, ones, xn, nullptr));
    VF_HIP(launch_dense_dot16(xn, n, xn, n, ix->d, dout, n, nullptr));
    VF_HIP(hipMemcpy(out, dout, (size_t)n * n * 4, hipMemcpyDeviceToHost));
    return VF_OK;
}

extern "C" int vf_cosine_matrix_rows(vf_index* ix, const int64_t* ids, int32_t n, float* out) {
    if (ids && n > 0 && n <= 4096)   // -1 is the mixed form's marker; here every id must name a row
        for (int i = 0; i < n; ++i) if (ids[i] == -1) return fail(VF_EINVAL, "vf_cosine_matrix_rows: id outside the index");
    return cosine_matrix_rows_impl(ix, ids, n, nullptr, 0, out, "vf_cosine_matrix_rows");
}

extern "C" int vf_cosine_matrix_rows_mixed(vf_index* ix, const int64_t* ids, int32_t n, const float* extra, int32_t n_extra, float* out) {
    return cosine_matrix_rows_impl(ix, ids, n, extra, n_extra, out, "vf_cosine_matrix_rows_mixed");
}

// ------------------------------------------------------------------------------------------------
// Search over a chosen subset of rows (round 16): vf_index_search / vf_index_search_device with VF_SEARCH_SUBSET in nq.  The reference promises metadata filtering and
// never delivers it (BM25Retriever.invoke raises NotImplementedError, src/utils/bm25Retriever.py:70-72; its sketch ranks everything
// and masks on the host, :91-132).  Here the listed rows alone are scored, by k_scan_subset, in the canonical arithmetic, so the
// result is exactly what an index over those rows would return, ids mapped back; cost follows the rows listed, not the rows held.
// The plan (super-chunks, rank chunks, merge rounds, limits, the two trivial routes): vf_subset.h.  The workspace is ONE lease of the
// small entry points' pool, so the search slots -- and a search pending in one -- are not touched.
// ------------------------------------------------------------------------------------------------
static std::string subset_bad_message(const char* who, int64_t i, int64_t v, bool has_prev, int64_t prev, int64_t lo, int64_t hi) {
    const std::string at = std::string(who) + ": ids[" + std::to_string(i) + "] = " + std::to_string(v);
    if (v < lo || v >= hi) return at + " is outside the index's ids [" + std::to_string(lo) + ", " + std::to_string(hi) + ")";
    if (has_prev && v == prev) return at + " is a duplicate of ids[" + std::to_string(i - 1) + "] (the list must be strictly ascending)";
    return at + " is not ascending: ids[" + std::to_string(i - 1) + "] = " + std::to_string(prev) + " (the list must be strictly ascending)";
}

static int check_subset_args(vf_index* ix, const void* q, int nq, int k, const void* list, int64_t m, const void* ids, const void* sc, const char* who) {
    if (!ix) return fail(VF_EINVAL, std::string(who) + ": null handle");
    if (nq < 0 || k < 0 || m < 0) return fail(VF_EINVAL, std::string(who) + ": negative nq / k / n_ids");
    if (m > 0 && !list) return fail(VF_EINVAL, std::string(who) + ": null id list");
    if (nq > 0 && k > 0 && (!q || !ids || !sc)) return fail(VF_EINVAL, std::string(who) + ": null buffer");
    return VF_OK;
}

static size_t subset_ws_bytes(const SubsetPlan& p, int d, int k) {
    const size_t part = (size_t)p.batch * k, slots = p.parts > 1 ? (size_t)p.super_parts + 1 : 1;
    size_t b = Lease::padded((size_t)p.batch * d * 4) + Lease::padded((size_t)p.score_bytes) + Lease::padded(slots * part * 8) + Lease::padded(slots * part * 4);
    if (p.parts > 1) b += Lease::padded(part * 8) + Lease::padded(part * 4);
    return b;
}

static void subset_stats(vf_index* ix, int nq, int64_t m) {
    vf_search_stats stt{};
    stt.path = 3; stt.n_queries = nq; stt.subset_rows = m;
    ix->stats = stt;
}

// every result (-1, -FLT_MAX): the ranking kernel over no score at all
static int subset_fill_empty(int nq, int k, int64_t* d_out_ids, float* d_out_sc, hipStream_t st) {
    VF_HIP(launch_sort_rows(nullptr, 0, nq, 0, k, 0, (long long*)d_out_ids, d_out_sc, k, st));
    return VF_OK;
}

// The scan route, enqueued on `st` (nothing is waited for): everything on the device of the plain handle ix, which is current.
// d_list: the m listed ids; d_flag: the device form's check word (nothing reaches the outputs unless it reads ~0), or null.
// Per super-chunk: one scan, one ranking launch over its whole chunks (+ one for a short last chunk), then the parts are folded into
// the running result, fan_in slots per merge (vf_subset.h).
static int subset_scan(vf_index* ix, const SubsetPlan& p, Lease& ws, const float* d_q, int nq, int k, const long long* d_list, int64_t m,
                       const u64* d_flag, int64_t* d_out_ids, float* d_out_sc, hipStream_t st) {
    const int d = ix->d;
    const bool merging = p.parts > 1;
    const size_t part = (size_t)p.batch * k, slots = merging ? (size_t)p.super_parts + 1 : 1;
    float* qn = ws.take<float>((size_t)p.batch * d);
    float* scores = ws.take<float>((size_t)p.score_bytes / 4);
    long long* buf_ids = ws.take<long long>(slots * part);     // slot 0: the running result; slots 1 ..: the parts of a super-chunk
    float* buf_sc = ws.take<float>(slots * part);
    long long* mrg_ids = merging ? ws.take<long long>(part) : nullptr;
    float* mrg_sc = merging ? ws.take<float>(part) : nullptr;
    for (int b0 = 0; b0 < nq; b0 += p.batch) {
        const int nb = std::min(p.batch, nq - b0);
        const size_t pb = (size_t)nb * k;   // one slot of this pass
        VF_HIP(launch_prep_queries(d_q + (size_t)b0 * d, nb, d, d, nb, qn, nullptr, st));
        if (merging) VF_HIP(hipMemsetAsync(buf_ids, 0xFF, pb * 8, st));   // the running result starts as padding (ids -1: their scores are not read)
        for (long long c = 0; c < p.supers; ++c) {
            const SubsetSpan sup = subset_super(p, m, c);
            const long long count = sup.hi - sup.lo;
            SubsetArgs a{};
            a.rows = ix->rows_orig; a.norm = ix->norm; a.n = ix->n; a.ids = d_list; a.id_base = ix->id_offset;
            a.pos0 = sup.lo; a.count = count; a.qn = qn; a.nq = nb; a.d = d; a.scores = scores; a.rank_rows = p.rank_rows;
            VF_HIP(launch_scan_subset(a, ix->dtype, st));
            if (!merging) {   // one part: ranked straight into the result, any k
                VF_HIP(launch_sort_rows(scores, p.rank_rows, nb, (int)count, k, 0, buf_ids, buf_sc, k, st));
                break;
            }
            const long long chunks = subset_rank_chunks(p, sup), full = count / p.rank_rows, tail = count - full * p.rank_rows;
            long long* part_ids = buf_ids + pb;
            float* part_sc = buf_sc + pb;
            // a "query" of the ranking launch is a (chunk, query) pair: the scores are [chunk][query][rank_rows], the parts come out [chunk][query][k]
            if (full > 0) VF_HIP(launch_sort_rows(scores, p.rank_rows, (int)(full * nb), (int)p.rank_rows, k, 0, part_ids, part_sc, k, st));
            if (tail > 0) VF_HIP(launch_sort_rows(scores + (size_t)full * nb * p.rank_rows, p.rank_rows, nb, (int)tail, k, 0, part_ids + (size_t)full * pb,
                                                  part_sc + (size_t)full * pb, k, st));
            VF_HIP(launch_subset_part_base(part_ids, chunks, (long long)pb, sup.lo, p.rank_rows, st));
            long long first = 0;   // the slot that holds the running result
            for (long long done = 0; done < chunks;) {
                const long long take = std::min<long long>(p.fan_in - 1, chunks - done);
                VF_HIP(launch_merge_topk(buf_ids + (size_t)first * pb, buf_sc + (size_t)first * pb, (int)take + 1, nb, k, mrg_ids, mrg_sc, st));
                first += take; done += take;
                // ... which moves to the last slot this merge consumed -- the first of the next merge -- or, at the end, back to slot 0
                const long long to = done < chunks ? first : 0;
                VF_HIP(hipMemcpyAsync(buf_ids + (size_t)to * pb, mrg_ids, pb * 8, hipMemcpyDeviceToDevice, st));
                VF_HIP(hipMemcpyAsync(buf_sc + (size_t)to * pb, mrg_sc, pb * 4, hipMemcpyDeviceToDevice, st));
                if (done >= chunks) first = 0;
            }
        }
        VF_HIP(launch_subset_ids(buf_ids, buf_sc, (long long)pb, d_list, d_flag, (long long*)d_out_ids + (size_t)b0 * k, d_out_sc + (size_t)b0 * k, st));
    }
    return VF_OK;
}

// host buffers, a plain handle, the caller holds the lock
static int subset_host_plain(vf_index* ix, const float* queries, int nq, int k, const int64_t* ids, int64_t m, int64_t* out_ids, float* out_sc,
                             const char* who) {
    if (ix->damaged) return fail(VF_EHIP, std::string(who) + ": " + kDamagedMsg);
    const int64_t lo = ix->id_offset, hi = ix->id_offset + ix->n;
    const long long bad = subset_first_bad((const long long*)ids, m, lo, hi);
    if (bad >= 0) return fail(VF_EINVAL, subset_bad_message(who, bad, ids[bad], bad > 0, bad > 0 ? ids[bad - 1] : 0, lo, hi));
    const SubsetPlan p = subset_plan(ix->n, m, nq, k, ix->opt.subset_super_rows, 0);
    if (p.route == kSubsetRefused) return fail(VF_EUNSUPPORTED, std::string(who) + ": " + p.why);
    if (p.route == kSubsetAll) return search_host_locked(ix, queries, nq, k, out_ids, out_sc);
    if (p.route == kSubsetEmpty) {
        std::fill(out_ids, out_ids + (size_t)nq * k, (int64_t)-1);
        std::fill(out_sc, out_sc + (size_t)nq * k, -FLT_MAX);
        subset_stats(ix, nq, 0);
        return VF_OK;
    }
    VF_HIP(hipSetDevice(ix->device));
    const size_t qe = (size_t)nq * ix->d, oe = (size_t)nq * k;
    Lease ws;
    VF_TRY(ws.acquire(ix->device, subset_ws_bytes(p, ix->d, k) + Lease::padded(qe * 4) + Lease::padded((size_t)m * 8) + Lease::padded(oe * 8) + Lease::padded(oe * 4)));
    float* dq = ws.take<float>(qe); long long* dlist = ws.take<long long>((size_t)m);
    int64_t* dout_ids = ws.take<int64_t>(oe); float* dout_sc = ws.take<float>(oe);
    VF_HIP(hipMemcpy(dq, queries, qe * 4, hipMemcpyHostToDevice));
    VF_HIP(hipMemcpy(dlist, ids, (size_t)m * 8, hipMemcpyHostToDevice));
    VF_TRY(subset_scan(ix, p, ws, dq, nq, k, dlist, m, nullptr, dout_ids, dout_sc, nullptr));
    VF_HIP(hipStreamSynchronize(nullptr));
    VF_HIP(hipMemcpy(out_ids, dout_ids, oe * 8, hipMemcpyDeviceToHost));
    VF_HIP(hipMemcpy(out_sc, dout_sc, oe * 4, hipMemcpyDeviceToHost));
    subset_stats(ix, nq, m);
    return VF_OK;
}

// A group: the list is split at the shards' id ranges on the host and the shards are searched ONE AFTER ANOTHER (no overlap: each
// call is the synchronous host form); a shard without a listed row gives an all-padding part.  The parts meet on the home device
// and one k_merge_topk ranks them (shard order = ascending ids, which its tie rule relies on).
static int subset_host_group(vf_index* ix, const float* queries, int nq, int k, const int64_t* ids, int64_t m, int64_t* out_ids, float* out_sc,
                             const char* who) {
    if (ix->damaged) return fail(VF_EHIP, std::string(who) + ": " + kDamagedMsg);
    const size_t G = ix->shards.size();
    if ((size_t)G * k > 16384) return fail(VF_EUNSUPPORTED, "sharded search: shards * k > 16384");
    const int64_t lo = ix->id_offset, hi = ix->id_offset + ix->n;
    const long long bad = subset_first_bad((const long long*)ids, m, lo, hi);
    if (bad >= 0) return fail(VF_EINVAL, subset_bad_message(who, bad, ids[bad], bad > 0, bad > 0 ? ids[bad - 1] : 0, lo, hi));
    const size_t oe = (size_t)nq * k;
    std::vector<int64_t> part_ids(G * oe);
    std::vector<float> part_sc(G * oe);
    const int64_t* at = ids;
    for (size_t g = 0; g < G; ++g) {
        vf_index* sh = ix->shards[g];
        const int64_t* end = std::lower_bound(at, ids + m, sh->id_offset + sh->n);
        VF_TRY(subset_host_plain(sh, queries, nq, k, at, end - at, part_ids.data() + g * oe, part_sc.data() + g * oe, who));
        at = end;
    }
    VF_HIP(hipSetDevice(ix->device));
    VF_HIP(scan_configure());
    Lease ws;
    VF_TRY(ws.acquire(ix->device, Lease::padded(G * oe * 8) + Lease::padded(G * oe * 4) + Lease::padded(oe * 8) + Lease::padded(oe * 4)));
    long long* dp_ids = ws.take<long long>(G * oe); float* dp_sc = ws.take<float>(G * oe);
    long long* d_ids = ws.take<long long>(oe); float* d_sc = ws.take<float>(oe);
    VF_HIP(hipMemcpy(dp_ids, part_ids.data(), G * oe * 8, hipMemcpyHostToDevice));
    VF_HIP(hipMemcpy(dp_sc, part_sc.data(), G * oe * 4, hipMemcpyHostToDevice));
    VF_HIP(launch_merge_topk(dp_ids, dp_sc, (int)G, nq, k, d_ids, d_sc, nullptr));
    VF_HIP(hipStreamSynchronize(nullptr));
    VF_HIP(hipMemcpy(out_ids, d_ids, oe * 8, hipMemcpyDeviceToHost));
    VF_HIP(hipMemcpy(out_sc, d_sc, oe * 4, hipMemcpyDeviceToHost));
    subset_stats(ix, nq, m);
    return VF_OK;
}

static int subset_entry_host(vf_index* ix, const vf_subset_query* sq, int32_t nq, int32_t k, int64_t* out_ids, float* out_scores) {
    static const char* who = "vf_index_search (VF_SEARCH_SUBSET)";
    if (!sq) return fail(VF_EINVAL, std::string(who) + ": null vf_subset_query");
    const float* queries = sq->queries; const int64_t* ids = sq->ids; const int64_t n_ids = sq->n_ids;
    DeviceGuard restore_callers_device;
    VF_TRY(check_subset_args(ix, queries, nq, k, ids, n_ids, out_ids, out_scores, who));
    std::lock_guard<std::mutex> g(ix->mu);
    if (nq == 0 || k == 0) {   // nothing to return, but a bad list is still a bad list
        const long long bad = subset_first_bad((const long long*)ids, n_ids, ix->id_offset, ix->id_offset + ix->n);
        if (bad >= 0) return fail(VF_EINVAL, subset_bad_message(who, bad, ids[bad], bad > 0, bad > 0 ? ids[bad - 1] : 0, ix->id_offset, ix->id_offset + ix->n));
        return VF_OK;
    }
    if (!ix->shards.empty()) return subset_host_group(ix, queries, nq, k, ids, n_ids, out_ids, out_scores, who);
    return subset_host_plain(ix, queries, nq, k, ids, n_ids, out_ids, out_scores, who);
}

static int subset_entry_device(vf_index* ix, const vf_subset_query* sq, int32_t nq, int32_t k, int64_t* d_out_ids, float* d_out_scores, void* stream) {
    static const char* who = "vf_index_search_device (VF_SEARCH_SUBSET)";
    if (!sq) return fail(VF_EINVAL, std::string(who) + ": null vf_subset_query");
    const float* d_queries = sq->queries; const int64_t* d_ids = sq->ids; const int64_t n_ids = sq->n_ids;
    DeviceGuard restore_callers_device;
    VF_TRY(check_subset_args(ix, d_queries, nq, k, d_ids, n_ids, d_out_ids, d_out_scores, who));
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->damaged) return fail(VF_EHIP, std::string(who) + ": " + kDamagedMsg);
    if (!ix->shards.empty()) return fail(VF_EUNSUPPORTED, std::string(who) + ": a group handle takes the host-buffer form only (vf_index_search with VF_SEARCH_SUBSET)");
    if (n_ids > ix->n) return fail(VF_EINVAL, std::string(who) + ": " + std::to_string(n_ids) + " ids for an index of " + std::to_string(ix->n) + " rows (the list must be strictly ascending)");
    const SubsetPlan p = subset_plan(ix->n, n_ids, nq, k, ix->opt.subset_super_rows, 0);
    if (p.route == kSubsetRefused) return fail(VF_EUNSUPPORTED, std::string(who) + ": " + p.why);
    hipStream_t st = (hipStream_t)stream;
    const int64_t m = n_ids, lo = ix->id_offset, hi = ix->id_offset + ix->n;
    VF_HIP(hipSetDevice(ix->device));
    if (p.route == kSubsetEmpty) {
        if (nq > 0 && k > 0) { VF_TRY(subset_fill_empty(nq, k, d_out_ids, d_out_scores, st)); VF_HIP(hipStreamSynchronize(st)); }
        subset_stats(ix, nq, 0);
        return VF_OK;
    }
    Lease ws;
    VF_TRY(ws.acquire(ix->device, Lease::padded(8) + (p.route == kSubsetScan && nq > 0 && k > 0 ? subset_ws_bytes(p, ix->d, k) : 0)));
    u64* d_flag = ws.take<u64>(1);
    VF_HIP(hipMemsetAsync(d_flag, 0xFF, 8, st));
    VF_HIP(launch_subset_check((const long long*)d_ids, m, lo, hi, d_flag, st));
    const bool scan = p.route == kSubsetScan && nq > 0 && k > 0;
    if (scan) VF_TRY(subset_scan(ix, p, ws, d_queries, nq, k, (const long long*)d_ids, m, d_flag, d_out_ids, d_out_scores, st));
    u64 first_bad = 0;
    VF_HIP(hipMemcpyAsync(&first_bad, d_flag, 8, hipMemcpyDeviceToHost, st));
    VF_HIP(hipStreamSynchronize(st));   // the one wait of the call: the results are final and the check word is here
    if (first_bad != ~0ull) {
        int64_t v[2] = {0, 0};
        const int64_t i = (int64_t)first_bad;
        VF_HIP(hipMemcpy(v, d_ids + (i > 0 ? i - 1 : 0), (i > 0 ? 2 : 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        return fail(VF_EINVAL, subset_bad_message(who, i, i > 0 ? v[1] : v[0], i > 0, v[0], lo, hi));
    }
    if (scan) { subset_stats(ix, nq, m); return VF_OK; }
    if (nq == 0 || k == 0) return VF_OK;
    return search_device_locked(ix, d_queries, nq, k, d_out_ids, d_out_scores, st);   // every row is listed: the ordinary search
}

// ------------------------------------------------------------------------------------------------
// A list per query of a batch (round 23): vf_index_search / vf_index_search_device with VF_SEARCH_SUBSETS in nq.  Row i is what the
// one-list call above returns for query i alone under its own list.  The plan -- passes, the permutation, tiles, size classes, the
// sentinel rule, the limits -- is vf_subset_multi.h; here are the argument checks, the tables' upload and subsets_enqueue_pass.
// The workspace is ONE lease of the small entry points' pool, as above.
// ------------------------------------------------------------------------------------------------
struct SubsetsBuffers {     // what a pass works in (all on the device)
    float* qn; float* scores; long long* rank_ids; float* rank_sc;
    const SubmTile* tiles; const SubmQuery* qd;   // of the whole call: a pass uses [tile0, + n_tiles) and [q0, + nb)
    const u64* flag;                               // the device form's check word, or null
};

// One pass, enqueued on `st` (nothing is waited for): the query prep, per size class in use one scan and one ranking launch, the map.
static int subsets_enqueue_pass(vf_index* ix, const SubmConfig& c, const SubmPass& p, int tile0, const float* d_q, int k, const SubsetsBuffers& b,
                                int64_t* d_out_ids, float* d_out_sc, hipStream_t st) {
    const int d = ix->d;
    VF_HIP(launch_prep_queries(d_q + (size_t)p.q0 * d, p.nb, d, d, p.nb, b.qn, nullptr, st));
    for (int cls = 0; cls < c.n_classes; ++cls) {
        if (p.class_queries[cls] == 0) continue;
        const int n_rank = (int)c.class_rows[cls];
        SubsetMArgs a{};
        a.rows = ix->rows_orig; a.norm = ix->norm; a.n = ix->n; a.id_base = ix->id_offset; a.qn = b.qn; a.d = d; a.scores = b.scores;
        a.tiles = b.tiles + tile0 + p.class_tile0[cls]; a.n_rank = n_rank;
        VF_HIP(launch_scan_subset_m(a, p.class_tiles[cls], ix->dtype, st));
        const size_t at = (size_t)p.class_first[cls] * k;
        VF_HIP(launch_sort_rows(b.scores + p.class_base[cls], n_rank, p.class_queries[cls], n_rank, k, 0, b.rank_ids + at, b.rank_sc + at, k, st));
    }
    VF_HIP(launch_subset_ids_m(b.rank_ids, b.rank_sc, p.nb, k, b.qd + p.q0, b.flag, (long long*)d_out_ids, d_out_sc, st));
    return VF_OK;
}

static int subsets_locked(vf_index* ix, const vf_subsets_query* sq, int nq, int k, int64_t* out_ids, float* out_sc, bool device, hipStream_t st,
                          const char* who) {
    if (ix->damaged) return fail(VF_EHIP, std::string(who) + ": " + kDamagedMsg);
    if (!ix->shards.empty()) return fail(VF_EUNSUPPORTED, std::string(who) + ": a group handle takes one list per call (VF_SEARCH_SUBSET, host buffers), not a list per query");
    const SubmConfig c = subm_config_default();
    const long long* m = (const long long*)sq->n_ids;
    const SubmCall call = subm_call(nq, sq->list_of, sq->n_lists, m, c);
    if (call.verdict == kSubmBadListOf)
        return fail(VF_EINVAL, std::string(who) + ": list_of[" + std::to_string(call.at) + "] = " + std::to_string(call.value) + " is outside [0, " + std::to_string(sq->n_lists) + "): query " + std::to_string(call.at) + " names no list");
    if (call.verdict == kSubmNegativeLength)
        return fail(VF_EINVAL, std::string(who) + ": lists[" + std::to_string(call.at) + "]: negative n_ids");
    if (call.verdict == kSubmTooLong)
        return fail(VF_EUNSUPPORTED, std::string(who) + ": lists[" + std::to_string(call.at) + "] holds " + std::to_string(call.value) + " ids; a list per query serves at most " +
                                         std::to_string(c.rank_rows) + " (send its queries through VF_SEARCH_SUBSET)");
    if (call.verdict != kSubmOk) return fail(VF_EINVAL, std::string(who) + ": bad sizes");
    // the referenced lists, ascending by their number
    std::vector<char> used((size_t)sq->n_lists, 0);
    for (int q = 0; q < nq; ++q) used[sq->list_of[q]] = 1;
    std::vector<int> ref;
    long long longest = 0, total = 0;
    for (int j = 0; j < sq->n_lists; ++j) {
        if (!used[j]) continue;
        if (m[j] > 0 && !sq->lists[j]) return fail(VF_EINVAL, std::string(who) + ": lists[" + std::to_string(j) + "]: null id list");
        ref.push_back(j);
        longest = std::max(longest, m[j]); total += m[j];
    }
    const int64_t lo = ix->id_offset, hi = ix->id_offset + ix->n;
    if (!device)   // before any HIP call
        for (int j : ref) {
            const long long bad = subset_first_bad((const long long*)sq->lists[j], m[j], lo, hi);
            if (bad >= 0) return fail(VF_EINVAL, subset_bad_message((std::string(who) + ": lists[" + std::to_string(j) + "]").c_str(), bad, sq->lists[j][bad], bad > 0,
                                                                    bad > 0 ? sq->lists[j][bad - 1] : 0, lo, hi));
        }
    if (nq == 0 || (k == 0 && !device)) return VF_OK;
    // the workspace: the largest pass's scores, the ranked positions of a pass, the three tables; the host form's staging
    long long score_floats = 0;
    for (int q0 = 0; q0 < nq; q0 += c.pass_queries) {
        long long f = 0;
        for (int q = q0; q < std::min(nq, q0 + c.pass_queries); ++q) f += c.class_rows[subm_class_of(c, m[sq->list_of[q]])];
        score_floats = std::max(score_floats, f);
    }
    if (score_floats * 4 > subm_score_bytes_bound(c)) return fail(VF_EINVAL, std::string(who) + ": the plan's score workspace exceeds its bound");
    const int nbmax = std::min(nq, c.pass_queries);
    const size_t qe = (size_t)nq * ix->d, oe = (size_t)nq * k, part = (size_t)nbmax * k;
    const size_t tiles_b = Lease::padded((size_t)nq * sizeof(SubmTile)), qd_b = Lease::padded((size_t)nq * sizeof(SubmQuery)), lists_b = Lease::padded(ref.size() * sizeof(SubmList));
    size_t bytes = Lease::padded(8) + Lease::padded((size_t)nbmax * ix->d * 4) + Lease::padded((size_t)score_floats * 4) + Lease::padded(part * 8) + Lease::padded(part * 4) +
                   tiles_b + qd_b + lists_b;
    if (!device) bytes += Lease::padded(qe * 4) + Lease::padded((size_t)total * 8) + Lease::padded(oe * 8) + Lease::padded(oe * 4);
    VF_HIP(hipSetDevice(ix->device));
    Lease ws;
    VF_TRY(ws.acquire(ix->device, bytes));
    u64* d_flag = ws.take<u64>(1);
    SubsetsBuffers b{};
    b.qn = ws.take<float>((size_t)nbmax * ix->d); b.scores = ws.take<float>((size_t)score_floats);
    b.rank_ids = ws.take<long long>(part); b.rank_sc = ws.take<float>(part);
    char* d_tables = ws.take<char>(tiles_b + qd_b + lists_b);
    b.tiles = (const SubmTile*)d_tables; b.qd = (const SubmQuery*)(d_tables + tiles_b); b.flag = device ? d_flag : nullptr;
    const SubmList* d_lists = (const SubmList*)(d_tables + tiles_b + qd_b);
    const float* d_q = sq->queries;
    int64_t* d_out_ids = out_ids; float* d_out_sc = out_sc;
    std::vector<const long long*> list_ptr((size_t)sq->n_lists, nullptr);
    if (device) {
        for (int j : ref) list_ptr[j] = (const long long*)sq->lists[j];
    } else {   // the queries and, in ONE copy, every referenced list go up
        float* dq = ws.take<float>(qe); long long* dl = ws.take<long long>((size_t)total);
        d_out_ids = ws.take<int64_t>(oe); d_out_sc = ws.take<float>(oe);
        std::vector<long long> all((size_t)total);
        size_t at = 0;
        for (int j : ref) {
            if (m[j] > 0) memcpy(all.data() + at, sq->lists[j], (size_t)m[j] * 8);
            list_ptr[j] = dl + at; at += (size_t)m[j];
        }
        VF_HIP(hipMemcpy(dq, sq->queries, qe * 4, hipMemcpyHostToDevice));
        if (total > 0) VF_HIP(hipMemcpy(dl, all.data(), (size_t)total * 8, hipMemcpyHostToDevice));
        d_q = dq;
    }
    // the tables of every pass, built on the host and uploaded in one copy
    std::vector<char> tables(tiles_b + qd_b + lists_b, 0);
    SubmTile* h_tiles = (SubmTile*)tables.data(); SubmQuery* h_qd = (SubmQuery*)(tables.data() + tiles_b); SubmList* h_lists = (SubmList*)(tables.data() + tiles_b + qd_b);
    std::vector<SubmPass> passes;
    std::vector<int> tile0s, perm((size_t)c.pass_queries);
    int n_tiles = 0;
    for (int ps = 0; ps < call.passes && k > 0; ++ps) {
        passes.push_back(subm_build_pass(ps, nq, sq->list_of, m, list_ptr.data(), c, perm.data(), h_tiles + n_tiles, h_qd + (size_t)ps * c.pass_queries));
        tile0s.push_back(n_tiles);
        n_tiles += passes.back().n_tiles;
    }
    for (size_t r = 0; r < ref.size(); ++r) h_lists[r] = SubmList{list_ptr[ref[r]], m[ref[r]], ref[r]};
    VF_HIP(hipMemcpyAsync(d_tables, tables.data(), tables.size(), hipMemcpyHostToDevice, st));   // (`tables` outlives the call's one wait)
    if (device) {
        VF_HIP(hipMemsetAsync(d_flag, 0xFF, 8, st));
        VF_HIP(launch_subset_check_m(d_lists, (int)ref.size(), longest, lo, hi, d_flag, st));
    }
    for (size_t ps = 0; ps < passes.size(); ++ps) VF_TRY(subsets_enqueue_pass(ix, c, passes[ps], tile0s[ps], d_q, k, b, d_out_ids, d_out_sc, st));
    if (device) {
        u64 first_bad = 0;
        VF_HIP(hipMemcpyAsync(&first_bad, d_flag, 8, hipMemcpyDeviceToHost, st));
        VF_HIP(hipStreamSynchronize(st));   // the one wait of the call: the results are final and the check word is here
        if (first_bad != ~0ull) {
            const long long j = subm_check_list(first_bad), i = subm_check_pos(first_bad);
            int64_t v[2] = {0, 0};
            VF_HIP(hipMemcpy(v, sq->lists[j] + (i > 0 ? i - 1 : 0), (i > 0 ? 2 : 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
            return fail(VF_EINVAL, subset_bad_message((std::string(who) + ": lists[" + std::to_string(j) + "]").c_str(), i, i > 0 ? v[1] : v[0], i > 0, v[0], lo, hi));
        }
        if (k == 0) return VF_OK;
    } else {
        VF_HIP(hipStreamSynchronize(st));
        VF_HIP(hipMemcpy(out_ids, d_out_ids, oe * 8, hipMemcpyDeviceToHost));
        VF_HIP(hipMemcpy(out_sc, d_out_sc, oe * 4, hipMemcpyDeviceToHost));
    }
    vf_search_stats stt{};
    stt.path = 4; stt.n_queries = nq; stt.subset_rows = call.rows; stt.subset_tiles = n_tiles;
    ix->stats = stt;
    return VF_OK;
}

// the argument checks that need no handle come first, in the order of the one-list form
static int subsets_entry(vf_index* ix, const vf_subsets_query* sq, int32_t nq_flags, int32_t k, int64_t* out_ids, float* out_scores, bool device, void* stream) {
    const char* who = device ? "vf_index_search_device (VF_SEARCH_SUBSETS)" : "vf_index_search (VF_SEARCH_SUBSETS)";
    if (nq_flags & VF_SEARCH_SUBSET) return fail(VF_EINVAL, std::string(who) + ": VF_SEARCH_SUBSET and VF_SEARCH_SUBSETS together (one list per call, or one per query)");
    const int nq = nq_flags & ~VF_SEARCH_SUBSETS;
    if (!sq) return fail(VF_EINVAL, std::string(who) + ": null vf_subsets_query");
    if (!ix) return fail(VF_EINVAL, std::string(who) + ": null handle");
    if (k < 0 || sq->n_lists < 0) return fail(VF_EINVAL, std::string(who) + ": negative k / n_lists");
    if (nq > 0 && (!sq->list_of || !sq->lists || !sq->n_ids)) return fail(VF_EINVAL, std::string(who) + ": null list table (lists / n_ids / list_of)");
    if (nq > 0 && k > 0 && (!sq->queries || !out_ids || !out_scores)) return fail(VF_EINVAL, std::string(who) + ": null buffer");
    DeviceGuard restore_callers_device;
    std::lock_guard<std::mutex> g(ix->mu);
    return subsets_locked(ix, sq, nq, k, out_ids, out_scores, device, (hipStream_t)stream, who);
}

// ------------------------------------------------------------------------------------------------
// A metadata filter evaluated on the device (round 24): vf_index_search_device with VF_SEARCH_WHERE in nq.  What turns a filter into a
// row set used to be host dictionaries and an upload of 8 bytes per passing row; here the program of vf_where.h runs over int64 key
// columns that live on the device and leaves the bitmap (the BM25 filter's layout) and the ascending id list (what VF_SEARCH_SUBSET
// takes) where the two legs want them.  Everything is checked before any device work; the descriptor block, the tile counts and
// their prefix are ONE lease of the small entry points' pool; three launches, one wait, at which m is read.
// ------------------------------------------------------------------------------------------------
static_assert(sizeof(vf_where_leaf) == sizeof(WhereLeaf) && sizeof(vf_where_column) == sizeof(WhereColumnPtr), "the public structs are the header's");
// vf_where.hip is the one kernel TU this file calls that a link of the host side alone leaves out (tests/test_host_sanitized.py links
// vf_kernels.o and vf_transformer.o): the reference is weak, and a library without the TU refuses the call instead of failing to link.
namespace vf { hipError_t launch_where(const WhereArgs& a, hipStream_t s) __attribute__((weak)); }

static std::string where_refusal(const WhereVerdict& v, const vf_where_query* wq) {
    switch (v.verdict) {
        case kWhereEmpty: return "an empty program (it needs at least one column, one leaf and one op)";
        case kWhereBadOp: return "ops[" + std::to_string(v.at) + "] = " + std::to_string((int)wq->ops[v.at]) + " is neither one of the " + std::to_string(wq->n_leaves) + " leaves nor an operator";
        case kWhereUnderflow: return "ops[" + std::to_string(v.at) + "] pops more than the stack holds";
        case kWhereLeftover: return "the program leaves " + std::to_string(v.at) + " values on the stack, not one";
        case kWhereBadLeaf: return "leaves[" + std::to_string(v.at) + "] has an unknown kind or names a column outside [0, " + std::to_string(wq->n_columns) + ")";
        case kWhereBadSetRun: return "leaves[" + std::to_string(v.at) + "]: its run lies outside the " + std::to_string(wq->n_set_values) + " set values";
        case kWhereSetNotAscending: return "set_values[" + std::to_string(v.at) + "] is not above its predecessor (a set leaf's run must be strictly ascending)";
        default: return "bad program";
    }
}

static int where_entry(vf_index* ix, vf_where_query* wq, int32_t nq_flags, bool device, void* stream) {
    static const char* who = "vf_index_search_device (VF_SEARCH_WHERE)";
    if (!device) return fail(VF_EINVAL, "vf_index_search (VF_SEARCH_WHERE): a filter is evaluated by the device form, vf_index_search_device");
    if (nq_flags & (VF_SEARCH_SUBSET | VF_SEARCH_SUBSETS)) return fail(VF_EINVAL, std::string(who) + ": VF_SEARCH_WHERE together with VF_SEARCH_SUBSET / VF_SEARCH_SUBSETS (a call evaluates a filter or searches, not both)");
    if (nq_flags & ~VF_SEARCH_WHERE) return fail(VF_EINVAL, std::string(who) + ": the count bits of nq must be 0");
    if (!wq) return fail(VF_EINVAL, std::string(who) + ": null vf_where_query");
    if (!ix) return fail(VF_EINVAL, std::string(who) + ": null handle");
    DeviceGuard restore_callers_device;
    std::lock_guard<std::mutex> g(ix->mu);
    if (ix->damaged) return fail(VF_EHIP, std::string(who) + ": " + kDamagedMsg);
    if (!ix->shards.empty()) return fail(VF_EUNSUPPORTED, std::string(who) + ": a group handle evaluates no filter (evaluate it on the host: WhereProgram.evaluate_numpy)");
    if (wq->n != ix->n) return fail(VF_EINVAL, std::string(who) + ": n = " + std::to_string(wq->n) + " but the index holds " + std::to_string(ix->n) + " rows (columns made before an append or a removal are stale)");
    const int tile_rows = wq->tile_rows == 0 ? kWhereTileRows : wq->tile_rows;
    if (!where_tile_rows_ok(tile_rows)) return fail(VF_EINVAL, std::string(who) + ": tile_rows = " + std::to_string(wq->tile_rows) + " must be 0 or a multiple of 64 in [64, 1024]");
    if (wq->n_columns < 0 || wq->n_leaves < 0 || wq->n_ops < 0 || wq->n_set_values < 0) return fail(VF_EINVAL, std::string(who) + ": a negative count");
    if ((wq->n_columns > 0 && !wq->columns) || (wq->n_leaves > 0 && !wq->leaves) || (wq->n_ops > 0 && !wq->ops) || (wq->n_set_values > 0 && !wq->set_values))
        return fail(VF_EINVAL, std::string(who) + ": null columns / leaves / ops / set_values");
    const WhereVerdict v = where_validate((const WhereLeaf*)wq->leaves, wq->n_leaves, wq->ops, wq->n_ops, wq->n_columns, wq->set_values, wq->n_set_values);
    if (v.verdict == kWhereOverLimits) {
        static const char* what[] = {"leaves", "ops", "columns", "set values", "stack depth"};
        static const long long cap[] = {kWhereMaxLeaves, kWhereMaxOps, kWhereMaxColumns, kWhereMaxSetValues, kWhereMaxDepth};
        const std::string got = v.limit == kWhereLimitDepth ? "ops[" + std::to_string(v.at) + "] takes the stack past" : std::to_string(v.at) + " " + what[v.limit] + ", above";
        return fail(VF_EUNSUPPORTED, std::string(who) + ": " + got + " the limit of " + std::to_string(cap[v.limit]) + (v.limit == kWhereLimitDepth ? " values" : "") + " (evaluate it on the host: WhereProgram.evaluate_numpy)");
    }
    if (v.verdict != kWhereOk) return fail(VF_EINVAL, std::string(who) + ": " + where_refusal(v, wq));
    for (int c = 0; c < wq->n_columns; ++c)
        if (!wq->columns[c].keys) return fail(VF_EINVAL, std::string(who) + ": columns[" + std::to_string(c) + "]: null keys");
    if (ix->n > 0 && !wq->d_bitmap) return fail(VF_EINVAL, std::string(who) + ": null d_bitmap");
    if (wq->d_ids && wq->ids_cap < ix->n) return fail(VF_EINVAL, std::string(who) + ": ids_cap = " + std::to_string(wq->ids_cap) + " is below the index's " + std::to_string(ix->n) + " rows");
    if (ix->n == 0) { wq->m = 0; return VF_OK; }
    if (!launch_where) return fail(VF_EINTERNAL, std::string(who) + ": this library was linked without vf_where.hip");
    hipStream_t st = (hipStream_t)stream;
    const long long tiles = where_tiles(ix->n, tile_rows);
    const WhereBlock blk = where_block(wq->n_columns, wq->n_leaves, wq->n_ops, wq->n_set_values);
    VF_HIP(hipSetDevice(ix->device));
    Lease ws;
    VF_TRY(ws.acquire(ix->device, Lease::padded((size_t)blk.bytes) + Lease::padded((size_t)tiles * 4) + Lease::padded((size_t)tiles * 8) + Lease::padded(8)));
    char* d_blk = ws.take<char>((size_t)blk.bytes);
    u32* d_counts = ws.take<u32>((size_t)tiles); long long* d_prefix = ws.take<long long>((size_t)tiles); long long* d_m = ws.take<long long>(1);
    std::vector<char> block((size_t)blk.bytes, 0);
    memcpy(block.data() + blk.columns_at, wq->columns, (size_t)wq->n_columns * sizeof(WhereColumnPtr));
    memcpy(block.data() + blk.leaves_at, wq->leaves, (size_t)wq->n_leaves * sizeof(WhereLeaf));
    memcpy(block.data() + blk.ops_at, wq->ops, (size_t)wq->n_ops);
    if (wq->n_set_values > 0) memcpy(block.data() + blk.sets_at, wq->set_values, (size_t)wq->n_set_values * 8);
    VF_HIP(hipMemcpyAsync(d_blk, block.data(), block.size(), hipMemcpyHostToDevice, st));   // (`block` outlives the call's one wait)
    WhereArgs a{};
    a.columns = (const WhereColumnPtr*)(d_blk + blk.columns_at); a.leaves = (const WhereLeaf*)(d_blk + blk.leaves_at);
    a.ops = (const uint8_t*)(d_blk + blk.ops_at); a.n_ops = wq->n_ops; a.sets = (const int64_t*)(d_blk + blk.sets_at);
    a.n = ix->n; a.tile_rows = tile_rows; a.bitmap = wq->d_bitmap; a.tile_counts = d_counts; a.tile_prefix = d_prefix; a.m_out = d_m;
    a.ids = (long long*)wq->d_ids; a.id_offset = ix->id_offset;
    VF_HIP(launch_where(a, st));
    long long m = 0;
    VF_HIP(hipMemcpyAsync(&m, d_m, 8, hipMemcpyDeviceToHost, st));
    VF_HIP(hipStreamSynchronize(st));   // the one wait of the call: the bitmap and the ids are final and m is here
    wq->m = m;
    return VF_OK;
}

extern "C" int vf_merge_topk_device(const int64_t* d_ids_parts, const float* d_score_parts, int32_t nparts, int32_t nq,
                                    int32_t k, int64_t* d_ids, float* d_scores, int32_t device_id, void* stream) {
    DeviceGuard restore_callers_device;
    if (nparts <= 0 || nq < 0 || k < 0) return fail(VF_EINVAL, "vf_merge_topk_device: bad sizes");
    if (nq == 0 || k == 0) return VF_OK;
    if (!d_ids_parts || !d_score_parts || !d_ids || !d_scores) return fail(VF_EINVAL, "vf_merge_topk_device: null buffer");
    if ((size_t)nparts * k > 16384) return fail(VF_EUNSUPPORTED, "vf_merge_topk_device: nparts * k > 16384");
    VF_HIP(hipSetDevice(device_id));
    VF_HIP(scan_configure());
    VF_HIP(launch_merge_topk((const long long*)d_ids_parts, d_score_parts, nparts, nq, k, (long long*)d_ids, d_scores,
                             (hipStream_t)stream));
    return VF_OK;
}

extern "C" int vf_merge_topk_packed_device(const void* d_parts, int32_t nparts, int32_t nq, int32_t k, int64_t* d_ids,
                                           float* d_scores, int32_t device_id, void* stream) {
    DeviceGuard restore_callers_device;
    if (nparts <= 0 || nq < 0 || k < 0) return fail(VF_EINVAL, "vf_merge_topk_packed_device: bad sizes");
    if (nq == 0 || k == 0) return VF_OK;
    if (!d_parts || !d_ids || !d_scores) return fail(VF_EINVAL, "vf_merge_topk_packed_device: null buffer");
    if ((size_t)nparts * k > 16384) return fail(VF_EUNSUPPORTED, "vf_merge_topk_packed_device: nparts * k > 16384");
    VF_HIP(hipSetDevice(device_id));
    VF_HIP(scan_configure());
    VF_HIP(launch_merge_topk_packed(d_parts, nparts, nq, k, (long long*)d_ids, d_scores, (hipStream_t)stream));
    return VF_OK;
}

extern "C" int vf_fuse_rank(const float* rerank_scores, const float* time_scores, int32_t n, float* out_scores,
                            int64_t* out_order, int32_t device_id) {
    DeviceGuard restore_callers_device;
    if (n < 0 || n > 4096) return fail(VF_EINVAL, "vf_fuse_rank: n must be in [0, 4096]");
    if (n == 0) return VF_OK;
    if (!rerank_scores || !time_scores || !out_scores || !out_order) return fail(VF_EINVAL, "vf_fuse_rank: null buffer");
    VF_HIP(hipSetDevice(device_id));
    Lease ws;
    VF_TRY(ws.acquire(device_id, 3 * Lease::padded((size_t)n * 4) + Lease::padded((size_t)n * 8)));
    float* a = ws.take<float>(n); float* b = ws.take<float>(n); float* o = ws.take<float>(n); long long* ord = ws.take<long long>(n);
    VF_HIP(hipMemcpy(a, rerank_scores, (size_t)n * 4, hipMemcpyHostToDevice));
    VF_HIP(hipMemcpy(b, time_scores, (size_t)n * 4, hipMemcpyHostToDevice));
    VF_HIP(launch_fuse_rank(a, b, n, o, ord, nullptr));
    VF_HIP(hipMemcpy(out_scores, o, (size_t)n * 4, hipMemcpyDeviceToHost));
    VF_HIP(hipMemcpy(out_order, ord, (size_t)n * 8, hipMemcpyDeviceToHost));
    return VF_OK;
}

// Test hook (not in the public header): k_prep_q8 on a batch of up to 64 canonical queries (host pointers): the codes as stored
// ([dp / 16][planes][64][16], dp = d padded to 128), the steps [64], the certificate bounds [64] and the bands [2][64], so that a test can hold
// the DEVICE's residual and bands against the NumPy model
extern "C" int vf_debug_prep_q8(const float* qn, int32_t nq, int32_t d, int32_t planes, float eps_img, int32_t tau_band, int32_t fine_band,
                                signed char* codes, float* q_scale, float* eps_q, int32_t* band_q) {
    DeviceGuard restore_callers_device;
    if (!qn || !codes || !q_scale || !eps_q || !band_q || nq < 1 || nq > kMaxBatch || d < 1 || planes < 1 || planes > 2)
        return fail(VF_EINVAL, "vf_debug_prep_q8: bad argument");
    const int dp = (d + 127) / 128 * 128;
    const size_t nimg = (size_t)dp * planes * kMaxBatch;
    float* d_q = nullptr; char* d_out = nullptr;   // d_out: codes | steps | bounds | bands
    VF_HIP(hipMalloc((void**)&d_q, (size_t)nq * d * sizeof(float)));
    hipError_t e = hipMalloc((void**)&d_out, nimg + 4 * kMaxBatch * 4);
    float* d_sc = (float*)(d_out + nimg);
    if (e == hipSuccess) e = hipMemcpy(d_q, qn, (size_t)nq * d * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_prep_q8(d_q, nq, d, dp, kMaxBatch, planes, (signed char*)d_out, d_sc, d_sc + kMaxBatch, (int*)(d_sc + 2 * kMaxBatch),
                                            eps_img, tau_band, fine_band, nullptr);
    if (e == hipSuccess) e = hipMemcpy(codes, d_out, nimg, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(q_scale, d_sc, kMaxBatch * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(eps_q, d_sc + kMaxBatch, kMaxBatch * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(band_q, d_sc + 2 * kMaxBatch, 2 * kMaxBatch * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_q); (void)hipFree(d_out);
    if (e != hipSuccess) return fail(VF_EHIP, std::string("vf_debug_prep_q8: ") + hipGetErrorString(e));
    return VF_OK;
}

// Test hook (not in the public header): k_prep_rows then k_prep_image on n host rows of d elements (VF_DTYPE_F16 / _F32; any n >= 1, no
// shard-size rule): the code bytes as stored [n][dp] (dp = d padded to 128), inv_img [n], off_img [n], the canonical norms [n], the
// largest rho and the sum of the rhos, so that a test can hold the DEVICE's row side of the certificate against the NumPy model
extern "C" int vf_debug_prep_image(const void* rows, int32_t dtype, int64_t n, int32_t d, unsigned char* codes, float* inv_img, float* off_img,
                                   float* norm, float* rho_max, float* rho_sum) {
    DeviceGuard restore_callers_device;
    if (!rows || !codes || !inv_img || !off_img || !norm || !rho_max || !rho_sum || (dtype != VF_DTYPE_F16 && dtype != VF_DTYPE_F32) || n < 1 ||
        n > (1 << 24) || d < 1 || d > 8192)
        return fail(VF_EINVAL, "vf_debug_prep_image: bad argument");
    const int dp = (d + 127) / 128 * 128;
    const size_t nn = (size_t)n, in_bytes = nn * d * (dtype == VF_DTYPE_F16 ? 2 : 4), img_bytes = nn * dp;
    char* d_in = nullptr; unsigned char* d_img = nullptr; float* d_f = nullptr;   // d_f: norm | inv_scan | inv_img | off_img | rho max bits, rho sum
    VF_HIP(hipMalloc((void**)&d_in, in_bytes));
    hipError_t e = hipMalloc((void**)&d_img, img_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&d_f, (4 * nn + 2) * sizeof(float));
    if (e == hipSuccess) e = hipMemset(d_f, 0, (4 * nn + 2) * sizeof(float));
    if (e == hipSuccess) e = hipMemset(d_img, 0xFF, img_bytes);   // (no code is 0xFF: a byte the kernel left alone shows)
    if (e == hipSuccess) e = hipMemcpy(d_in, rows, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_prep_rows(d_in, dtype, n, d, dp, nullptr, d_f, d_f + nn, nullptr);
    if (e == hipSuccess) e = launch_prep_image(d_in, dtype, n, d, dp, d_f, d_img, d_f + 2 * nn, d_f + 3 * nn, (u32*)(d_f + 4 * nn), d_f + 4 * nn + 1, nullptr);
    if (e == hipSuccess) e = hipMemcpy(codes, d_img, img_bytes, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(norm, d_f, nn * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(inv_img, d_f + 2 * nn, nn * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(off_img, d_f + 3 * nn, nn * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rho_max, d_f + 4 * nn, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rho_sum, d_f + 4 * nn + 1, 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_img); (void)hipFree(d_f);
    if (e != hipSuccess) return fail(VF_EHIP, std::string("vf_debug_prep_image: ") + hipGetErrorString(e));
    return VF_OK;
}

// Test hook (not in the public header): C [32][32] = A [32][32] B [32][32]^T through ONE int8 matrix instruction fed the way k_scan2r's
// int8 body feeds it (host pointers)
extern "C" int vf_debug_mfma_i8(const signed char* A, const signed char* B, int32_t* C) {
    DeviceGuard restore_callers_device;
    if (!A || !B || !C) return fail(VF_EINVAL, "vf_debug_mfma_i8: bad argument");
    signed char* d_in = nullptr; int* d_out = nullptr;
    VF_HIP(hipMalloc((void**)&d_in, 2048));
    hipError_t e = hipMalloc((void**)&d_out, 4096);
    if (e == hipSuccess) e = hipMemcpy(d_in, A, 1024, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in + 1024, B, 1024, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_debug_mfma_i8(d_in, d_in + 1024, d_out, nullptr);
    if (e == hipSuccess) e = hipMemcpy(C, d_out, 4096, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_out);
    if (e != hipSuccess) return fail(VF_EHIP, std::string("vf_debug_mfma_i8: ") + hipGetErrorString(e));
    return VF_OK;
}

// Test hook (not in the public header): the fused scan's HARDWARE e4m3 -> fp16 conversion applied to `count` codes,
// so that tests can pin it against the oracle's table instead of trusting the instruction's documentation.
extern "C" int vf_debug_cvt_e4m3(const unsigned char* codes, float* out, int32_t count) {
    DeviceGuard restore_callers_device;
    if (!codes || !out || count < 0) return fail(VF_EINVAL, "vf_debug_cvt_e4m3: bad argument");
    unsigned char* d_in = nullptr; float* d_out = nullptr;
    VF_HIP(hipMalloc((void**)&d_in, (size_t)count + 8));
    hipError_t e = hipMalloc((void**)&d_out, ((size_t)count + 8) * 4);
    if (e == hipSuccess) e = hipMemcpy(d_in, codes, count, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_debug_cvt_e4m3(d_in, d_out, count, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)count * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_in); (void)hipFree(d_out);
    if (e != hipSuccess) return fail(VF_EHIP, std::string("vf_debug_cvt_e4m3: ") + hipGetErrorString(e));
    return VF_OK;
}
