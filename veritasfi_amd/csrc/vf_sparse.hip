// vf_sparse.hip -- the ensemble's BM25 leg on gfx950: scoring of a bm25s CSC index (one column per token, per-posting
// precomputed float32 score) and an exact, canonically ordered top-k over every document.  Replaces bm25s's numpy scorer
// (np.add.at per query token) + its top-k (src/utils/bm25Retriever.py:74-87), which ranks all N chunks per request on the CPU.
//
// Contract: score(doc) = fp32 sum of the doc's postings over the query's tokens, added LEFT TO RIGHT in
// query-token order starting from 0.0f (bit-equal to the numpy scorer); rank by score descending, ties to the lower row;
// untouched rows score 0 and follow the touched ones in ascending row order.
//
// Kernels (one query per slot; gridDim.y = the slots of a group)
//   k_bm25_accum       one launch per query-token position: scores[row] += data[p] over the token's postings (plain
//                      read-add-write: a document appears once per column, positions run as successive launches, so no
//                      float atomic and a fixed order), touched rows marked in a bitmap (integer atomicOr)
//   k_bm25_hist / k_bm25_pick   multi-workgroup radix select over the touched rows' 64-bit keys (orderkey(score) << 32 | ~row),
//                      8-bit digits from the top; stops once a digit's bin is taken whole (or at once when k >= touched)
//   k_bm25_gather      the keys >= the selected prefix (exactly min(k, touched) of them)
//   k_bm25_sort_small  k <= 4096: LDS bitonic sort, write ids / scores
//   k_bitonic_*        k > 4096 (the reference's k = num_chunk call): bitonic sort of the selected keys in global memory
//   k_bm25_tail_*      the zero-score tail: untouched rows in ascending order (prefix sum over the bitmap's zero bits)
//   k_bm25_reset       clear what the query touched: its postings' score entries and bitmap words (O(postings), not O(N))
#include "vf_internal.h"

#include <float.h>
#include <mutex>
#include <string>
#include <vector>

namespace vf {

constexpr int kBmThreads = 256;
constexpr int kBmWordsPerThread = 4;
constexpr int kBmWordsPerBlock = kBmThreads * kBmWordsPerThread;   // 1024 bitmap words = 32768 rows per workgroup
constexpr int kBmSmallK = 4096;                                     // k up to this: one LDS sort per query
constexpr int kBmMaxSlots = 64;                                     // queries in flight per group
constexpr long long kBmScratchBudget = 3ll << 30;                   // bytes of per-query scratch a handle may hold
constexpr int kBmSortChunk = 4096;                                  // keys per LDS chunk of the global bitonic sort

struct BmState {          // per slot, rewritten by pass 0 of every query
    u64 prefix;           // selected keys are those >= prefix
    int need;             // keys still to take from the current digit's bin
    int done;
    u32 touched;          // rows with a posting
    u32 nsel;             // keys gathered
    u32 pad[2];
};

struct BmArgs {
    const long long* indptr; const int* indices; const float* data;   // CSC index
    const long long* q_off; const int* q_terms;                       // [nq + 1] offsets into q_terms (device)
    int q0;                                                           // query of slot 0
    long long n; int words;                                           // documents; bitmap words in use (padded to kBmWordsPerBlock)
    float* scores; long long score_stride;                            // [slot][n], zero outside a query
    u32* bits; long long bits_stride;                                 // [slot][words]
    u32* hist;                                                        // [slot][256]
    BmState* st;                                                      // [slot]
    u64* sel; long long sel_stride; long long sel_cap;                // [slot][sel_cap] gathered keys
    u32* tblk; long long tblk_stride;                                 // [slot][blocks] untouched rows per bitmap block, then their prefix
    int k;
    long long* out_ids; float* out_scores; long long out_stride;      // [slot][k]
};

__device__ __forceinline__ u64 bm_key(const float* sc, u32 row) {
    return ((u64)orderkey(sc[row]) << 32) | (u64)(0xFFFFFFFFu - row);
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_accum(BmArgs a, int t) {
    const int s = blockIdx.y, q = a.q0 + s;
    const long long b = a.q_off[q], e = a.q_off[q + 1];
    if (b + t >= e) return;
    const int col = a.q_terms[b + t];
    const long long p0 = a.indptr[col], p1 = a.indptr[col + 1];
    float* sc = a.scores + s * a.score_stride;
    u32* bits = a.bits + s * a.bits_stride;
    for (long long p = p0 + (long long)blockIdx.x * kBmThreads + threadIdx.x; p < p1; p += (long long)gridDim.x * kBmThreads) {
        const u32 row = (u32)a.indices[p];
        sc[row] = sc[row] + a.data[p];
        atomicOr(&bits[row >> 5], 1u << (row & 31u));
    }
}

// histogram of digit (key >> shift) & 255 over the touched keys whose upper digits equal the prefix
__global__ __launch_bounds__(kBmThreads) void k_bm25_hist(BmArgs a, int pass) {
    const int s = blockIdx.y, tid = threadIdx.x;
    const BmState* st = a.st + s;
    if (pass > 0 && st->done) return;
    __shared__ u32 h[256];
    h[tid] = 0;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const u64 hi_mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
    const u64 prefix = pass == 0 ? 0ull : st->prefix;
    const float* sc = a.scores + s * a.score_stride;
    const uint4 w4 = *(const uint4*)(a.bits + s * a.bits_stride + (long long)blockIdx.x * kBmWordsPerBlock + tid * 4);
    const u32 wv[4] = {w4.x, w4.y, w4.z, w4.w};
    const u32 w0 = (u32)blockIdx.x * kBmWordsPerBlock + tid * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        for (u32 m = wv[j]; m; m &= m - 1) {
            const u64 key = bm_key(sc, (w0 + j) * 32 + (u32)(__ffs(m) - 1));
            if ((key & hi_mask) == prefix) atomicAdd(&h[(u32)(key >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&a.hist[s * 256 + tid], h[tid]);
}

// one workgroup per slot: the digit that holds the need-th largest key (k_topk_rows' suffix scan), histogram cleared
__global__ __launch_bounds__(256) void k_bm25_pick(BmArgs a, int pass) {
    const int s = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    BmState* st = a.st + s;
    if (pass > 0 && st->done) return;
    __shared__ u32 wsum[4];
    __shared__ u32 pick[3];
    u32* hist = a.hist + s * 256;
    const u32 c = hist[tid];
    u32 sfx = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 v = __shfl_down(sfx, o, 64);
        if (lane + o < 64) sfx += v;
    }
    if (lane == 0) wsum[wid] = sfx;
    __syncthreads();
    for (int w = wid + 1; w < 4; ++w) sfx += wsum[w];
    const u32 total = wsum[0] + wsum[1] + wsum[2] + wsum[3];   // keys counted in this pass (pass 0: every touched row)
    int need;
    u64 prefix;
    if (pass == 0) {
        need = (u32)a.k < total ? a.k : (int)total;
        prefix = 0;
        if ((u32)need == total) {   // every touched row is wanted (or none was touched): no digit to pick
            hist[tid] = 0;
            if (tid == 0) { st->prefix = 0; st->need = 0; st->done = 1; st->touched = total; st->nsel = 0; }
            return;
        }
    } else {
        need = st->need;
        prefix = st->prefix;
    }
    if (sfx >= (u32)need && sfx - c < (u32)need) { pick[0] = (u32)tid; pick[1] = sfx - c; pick[2] = c; }
    __syncthreads();
    hist[tid] = 0;
    if (tid == 0) {
        const int shift = 56 - 8 * pass;
        need -= (int)pick[1];
        st->prefix = prefix | ((u64)pick[0] << shift);
        st->need = need;
        st->done = (int)pick[2] == need || shift == 0;   // the bin is taken whole: its lower digits do not matter
        if (pass == 0) { st->touched = total; st->nsel = 0; }
    }
}

// the touched keys >= prefix: exactly min(k, touched), keys are unique.  One global atomic per workgroup.
__global__ __launch_bounds__(kBmThreads) void k_bm25_gather(BmArgs a) {
    const int s = blockIdx.y, tid = threadIdx.x;
    BmState* st = a.st + s;
    const u64 prefix = st->prefix;
    const float* sc = a.scores + s * a.score_stride;
    const uint4 w4 = *(const uint4*)(a.bits + s * a.bits_stride + (long long)blockIdx.x * kBmWordsPerBlock + tid * 4);
    const u32 wv[4] = {w4.x, w4.y, w4.z, w4.w};
    const u32 w0 = (u32)blockIdx.x * kBmWordsPerBlock + tid * 4;
    __shared__ u32 cnt, base;
    if (tid == 0) cnt = 0;
    __syncthreads();
    u32 mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        for (u32 m = wv[j]; m; m &= m - 1) mine += bm_key(sc, (w0 + j) * 32 + (u32)(__ffs(m) - 1)) >= prefix;
    const u32 off = mine ? atomicAdd(&cnt, mine) : 0u;
    __syncthreads();
    if (tid == 0 && cnt) base = atomicAdd(&st->nsel, cnt);
    __syncthreads();
    if (!mine) return;
    u64* sel = a.sel + s * a.sel_stride;
    u32 i = base + off;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        for (u32 m = wv[j]; m; m &= m - 1) {
            const u64 key = bm_key(sc, (w0 + j) * 32 + (u32)(__ffs(m) - 1));
            if (key >= prefix) {
                if (i < a.sel_cap) sel[i] = key;
                ++i;
            }
        }
}

__device__ __forceinline__ void bm_emit(const BmArgs& a, int s, long long i, u64 key) {
    a.out_ids[s * a.out_stride + i] = (long long)(0xFFFFFFFFu - (u32)key);
    a.out_scores[s * a.out_stride + i] = unorderkey((u32)(key >> 32));
}

// k <= kBmSmallK: the gathered keys of one slot sorted in LDS (Pk = next power of two >= k), ranks [0, nsel) written
__global__ __launch_bounds__(512) void k_bm25_sort_small(BmArgs a, int Pk) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    u64* keys = (u64*)smem_raw;
    const int s = blockIdx.y, tid = threadIdx.x;
    const u32 n = min(a.st[s].nsel, (u32)Pk);
    const u64* sel = a.sel + s * a.sel_stride;
    for (int i = tid; i < Pk; i += 512) keys[i] = (u32)i < n ? sel[i] : 0ull;   // 0 sorts below every real key
    __syncthreads();
    bitonic_sort_desc(keys, Pk, tid, 512);
    for (int i = tid; i < (int)n; i += 512) bm_emit(a, s, i, keys[i]);
}

// zero bits (untouched rows < n) of the four words a thread owns in bitmap block b
__device__ __forceinline__ void bm_zero_words(const BmArgs& a, int s, int b, int tid, u32 z[4]) {
    const uint4 w4 = *(const uint4*)(a.bits + s * a.bits_stride + (long long)b * kBmWordsPerBlock + tid * 4);
    const u32 wv[4] = {w4.x, w4.y, w4.z, w4.w};
    const long long w0 = (long long)b * kBmWordsPerBlock + tid * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long r0 = (w0 + j) * 32;
        const u32 valid = r0 >= a.n ? 0u : (a.n - r0 >= 32 ? 0xFFFFFFFFu : ((1u << (u32)(a.n - r0)) - 1u));
        z[j] = ~wv[j] & valid;
    }
}

__device__ __forceinline__ u32 block_excl_scan(u32 v, u32* lds /* [kBmThreads / 64] */, u32* total) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    u32 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    u32 before = 0, all = 0;
    for (int w = 0; w < kBmThreads / 64; ++w) {
        before += w < wid ? lds[w] : 0u;
        all += lds[w];
    }
    __syncthreads();
    *total = all;
    return before + inc - v;
}

// the zero-score tail, only when fewer than k rows were touched: untouched rows per bitmap block ...
__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_count(BmArgs a) {
    const int s = blockIdx.y, tid = threadIdx.x;
    if (a.st[s].nsel >= (u32)a.k) return;
    u32 z[4];
    bm_zero_words(a, s, blockIdx.x, tid, z);
    __shared__ u32 lds[kBmThreads / 64];
    u32 total;
    block_excl_scan(__popc(z[0]) + __popc(z[1]) + __popc(z[2]) + __popc(z[3]), lds, &total);
    if (tid == 0) a.tblk[s * a.tblk_stride + blockIdx.x] = total;
}

// ... their exclusive prefix over the blocks (one workgroup per slot) ...
__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_scan(BmArgs a, int nblk) {
    const int s = blockIdx.y, tid = threadIdx.x;
    if (a.st[s].nsel >= (u32)a.k) return;
    __shared__ u32 lds[kBmThreads / 64];
    u32* t = a.tblk + s * a.tblk_stride;
    u32 carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += kBmThreads) {
        const u32 v = b0 + tid < nblk ? t[b0 + tid] : 0u;
        u32 total;
        const u32 ex = block_excl_scan(v, lds, &total);
        if (b0 + tid < nblk) t[b0 + tid] = carry + ex;
        carry += total;
    }
}

// ... and the rows themselves, in ascending order, at ranks nsel + (untouched rows before them), while < k
__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_write(BmArgs a) {
    const int s = blockIdx.y, tid = threadIdx.x;
    const long long nsel = a.st[s].nsel;
    if (nsel >= a.k) return;
    const long long start = nsel + a.tblk[s * a.tblk_stride + blockIdx.x];
    if (start >= a.k) return;
    u32 z[4];
    bm_zero_words(a, s, blockIdx.x, tid, z);
    __shared__ u32 lds[kBmThreads / 64];
    u32 total;
    long long pos = start + block_excl_scan(__popc(z[0]) + __popc(z[1]) + __popc(z[2]) + __popc(z[3]), lds, &total);
    const long long w0 = (long long)blockIdx.x * kBmWordsPerBlock + tid * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        for (u32 m = z[j]; m && pos < a.k; m &= m - 1, ++pos) {
            a.out_ids[s * a.out_stride + pos] = (w0 + j) * 32 + (__ffs(m) - 1);
            a.out_scores[s * a.out_stride + pos] = 0.0f;
        }
}

// every score entry and bitmap word the query touched back to zero (writes of zero only: overlaps are harmless)
__global__ __launch_bounds__(kBmThreads) void k_bm25_reset(BmArgs a) {
    const int s = blockIdx.y, q = a.q0 + s;
    float* sc = a.scores + s * a.score_stride;
    u32* bits = a.bits + s * a.bits_stride;
    for (long long t = a.q_off[q]; t < a.q_off[q + 1]; ++t) {
        const int col = a.q_terms[t];
        const long long p1 = a.indptr[col + 1];
        for (long long p = a.indptr[col] + (long long)blockIdx.x * kBmThreads + threadIdx.x; p < p1; p += (long long)gridDim.x * kBmThreads) {
            const u32 row = (u32)a.indices[p];
            sc[row] = 0.0f;
            bits[row >> 5] = 0u;
        }
    }
}

// ---- k > kBmSmallK: bitonic sort of one slot's P gathered keys in global memory (P a power of two) ----------------------------
__global__ __launch_bounds__(kBmThreads) void k_bm25_pad(u64* keys, long long from, long long P) {
    for (long long i = from + (long long)blockIdx.x * kBmThreads + threadIdx.x; i < P; i += (long long)gridDim.x * kBmThreads) keys[i] = 0ull;
}

__global__ __launch_bounds__(kBmThreads) void k_bitonic_global(u64* keys, long long P, long long kk, long long j) {
    for (long long i = (long long)blockIdx.x * kBmThreads + threadIdx.x; i < (P >> 1); i += (long long)gridDim.x * kBmThreads) {
        const long long lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
        const bool desc = (lo & kk) == 0;
        const u64 x = keys[lo], y = keys[hi];
        if ((x < y) == desc) { keys[lo] = y; keys[hi] = x; }
    }
}

// the steps j <= L / 2 of stages kk_lo .. kk_hi on L-key chunks in LDS (L = min(P, kBmSortChunk)); direction from the global index
__global__ __launch_bounds__(1024) void k_bitonic_lds(u64* keys, int L, long long kk_lo, long long kk_hi, long long j_first) {
    __shared__ u64 s[kBmSortChunk];
    const int tid = threadIdx.x;
    const long long off = (long long)blockIdx.x * L;
    for (int i = tid; i < L; i += 1024) s[i] = keys[off + i];
    __syncthreads();
    for (long long kk = kk_lo; kk <= kk_hi; kk <<= 1) {
        for (long long j = kk == kk_lo ? j_first : (kk >> 1); j > 0; j >>= 1) {
            for (int i = tid; i < (L >> 1); i += 1024) {
                const int lo = (int)(((i & ~(j - 1)) << 1) | (i & (j - 1))), hi = lo | (int)j;
                const bool desc = ((off + lo) & kk) == 0;
                const u64 x = s[lo], y = s[hi];
                if ((x < y) == desc) { s[lo] = y; s[hi] = x; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < L; i += 1024) keys[off + i] = s[i];
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_emit(BmArgs a) {
    const long long n = a.st[0].nsel;
    for (long long i = (long long)blockIdx.x * kBmThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kBmThreads) bm_emit(a, 0, i, a.sel[i]);
}

}  // namespace vf

using namespace vf;

static int bm_fail(int code, const std::string& msg) { return vf::set_error(code, msg); }

#define VFS_HIP(expr)                                                                                                   \
    do {                                                                                                                \
        hipError_t _e = (expr);                                                                                         \
        if (_e != hipSuccess)                                                                                           \
            return bm_fail(VF_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (vf_sparse.hip:" + std::to_string(__LINE__) + ")"); \
    } while (0)

struct vf_bm25 {
    int device = 0;
    long long n = 0, V = 0, nnz = 0;
    int words = 0;                          // bitmap words per slot, a multiple of kBmWordsPerBlock
    std::vector<long long> indptr;          // host copy: grid sizes
    long long* d_indptr = nullptr;
    int* d_indices = nullptr;
    float* d_data = nullptr;
    hipStream_t stream = nullptr;
    int slot_cap = 1;                       // slots the scratch budget allows
    int slots = 0;                          // slots allocated
    float* d_scores = nullptr;              // [slots][n]
    u32* d_bits = nullptr;                  // [slots][words]
    u32* d_hist = nullptr;                  // [slots][256]
    BmState* d_st = nullptr;                // [slots]
    u64* d_sel = nullptr;                   // [slots][kBmSmallK]
    u32* d_tblk = nullptr;                  // [slots]: one bitmap block serves a tail of < kBmSmallK rows
    long long* d_ids = nullptr;             // [slots][kBmSmallK]
    float* d_out = nullptr;
    u64* d_big = nullptr;                   // k > kBmSmallK: [next_pow2(n)] keys
    u32* d_big_tblk = nullptr;              // [words / kBmWordsPerBlock]
    long long* d_big_ids = nullptr;         // [n]
    float* d_big_out = nullptr;
    long long q_cap = 0, t_cap = 0;
    long long* d_qoff = nullptr;
    int* d_qterms = nullptr;
    const int32_t* qterms_host = nullptr;   // the caller's q_terms during a search (grid sizes)
    std::mutex mu;
};

static long long bm_pow2(long long v) {
    long long p = 1;
    while (p < v) p <<= 1;
    return p;
}

static long long bm_slot_bytes(const vf_bm25* h) {
    return h->n * 4 + (long long)h->words * 4 + 256 * 4 + (long long)sizeof(BmState) + 4 + (long long)kBmSmallK * (8 + 8 + 4);
}

static void bm_free_slots(vf_bm25* h) {
    void* ps[] = {h->d_scores, h->d_bits, h->d_hist, h->d_st, h->d_sel, h->d_tblk, h->d_ids, h->d_out};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    h->d_scores = nullptr; h->d_bits = nullptr; h->d_hist = nullptr; h->d_st = nullptr; h->d_sel = nullptr;
    h->d_tblk = nullptr; h->d_ids = nullptr; h->d_out = nullptr;
    h->slots = 0;
}

// the per-query scratch of `want` slots, zeroed (the reset keeps it zero between queries)
static int bm_ensure_slots(vf_bm25* h, int want) {
    if (want <= h->slots) return VF_OK;
    VFS_HIP(hipStreamSynchronize(h->stream));
    bm_free_slots(h);
    const size_t S = (size_t)want;
    hipError_t e = hipMalloc((void**)&h->d_scores, S * h->n * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_bits, S * h->words * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_hist, S * 256 * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_st, S * sizeof(BmState));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_sel, S * kBmSmallK * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_tblk, S * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_ids, S * kBmSmallK * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_out, S * kBmSmallK * 4);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_scores, 0, S * h->n * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_bits, 0, S * h->words * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_hist, 0, S * 256 * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_st, 0, S * sizeof(BmState), h->stream);
    if (e != hipSuccess) {
        bm_free_slots(h);
        return bm_fail(e == hipErrorOutOfMemory ? VF_ENOMEM : VF_EHIP, std::string("vf_bm25: query scratch: ") + hipGetErrorString(e));
    }
    h->slots = want;
    return VF_OK;
}

static int bm_ensure_big(vf_bm25* h) {
    if (h->d_big) return VF_OK;
    const long long P = bm_pow2(h->n);
    hipError_t e = hipMalloc((void**)&h->d_big, (size_t)P * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_big_tblk, (size_t)(h->words / kBmWordsPerBlock) * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_big_ids, (size_t)h->n * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_big_out, (size_t)h->n * 4);
    if (e != hipSuccess) {
        void* ps[] = {h->d_big, h->d_big_tblk, h->d_big_ids, h->d_big_out};
        for (void* p : ps)
            if (p) (void)hipFree(p);
        h->d_big = nullptr; h->d_big_tblk = nullptr; h->d_big_ids = nullptr; h->d_big_out = nullptr;
        return bm_fail(e == hipErrorOutOfMemory ? VF_ENOMEM : VF_EHIP, std::string("vf_bm25: deep-k scratch: ") + hipGetErrorString(e));
    }
    return VF_OK;
}

static unsigned bm_grid(long long work, long long per_block, long long cap) {
    long long g = (work + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

static int bm_destroy(vf_bm25* h) {
    if (!h) return VF_OK;
    DeviceGuard guard;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    bm_free_slots(h);
    void* ps[] = {h->d_indptr, h->d_indices, h->d_data, h->d_big, h->d_big_tblk, h->d_big_ids, h->d_big_out, h->d_qoff, h->d_qterms};
    for (void* p : ps)
        if (p) (void)hipFree(p);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return VF_OK;
}

extern "C" int vf_bm25_create(const int64_t* indptr, int64_t V, const int32_t* indices, const float* data, int64_t nnz,
                              int64_t n_docs, int32_t device_id, vf_bm25** out, int32_t* slots) {
    if (!out) return bm_fail(VF_EINVAL, "vf_bm25_create: null out");
    if (!indptr) {   // release (realloc-style): the handle *out is destroyed
        bm_destroy(*out);
        *out = nullptr;
        return VF_OK;
    }
    *out = nullptr;
    if (!indptr || V < 0 || nnz < 0 || (nnz > 0 && (!indices || !data))) return bm_fail(VF_EINVAL, "vf_bm25_create: null or negative argument");
    if (n_docs <= 0 || n_docs > 0x7FFFFFFFll) return bm_fail(VF_EINVAL, "vf_bm25_create: n_docs must be in [1, 2^31 - 1]");
    if (indptr[0] != 0 || indptr[V] != nnz) return bm_fail(VF_EINVAL, "vf_bm25_create: indptr must start at 0 and end at nnz");
    for (int64_t c = 0; c < V; ++c) {   // the kernels rely on these: rows in range, each row once per column (ascending), scores > 0
        if (indptr[c + 1] < indptr[c]) return bm_fail(VF_EINVAL, "vf_bm25_create: indptr is not non-decreasing");
        for (int64_t p = indptr[c]; p < indptr[c + 1]; ++p) {
            if (indices[p] < 0 || indices[p] >= n_docs) return bm_fail(VF_EINVAL, "vf_bm25_create: a document row is out of range");
            if (p > indptr[c] && indices[p] <= indices[p - 1])
                return bm_fail(VF_EINVAL, "vf_bm25_create: rows of a column must be strictly ascending (one posting per document)");
            if (!(data[p] > 0.0f) || !(data[p] <= FLT_MAX)) return bm_fail(VF_EINVAL, "vf_bm25_create: posting scores must be finite and > 0");
        }
    }
    int ndev = 0;
    VFS_HIP(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return bm_fail(VF_EINVAL, "vf_bm25_create: bad device_id");
    DeviceGuard guard;
    VFS_HIP(hipSetDevice(device_id));
    vf_bm25* h = new (std::nothrow) vf_bm25();
    if (!h) return bm_fail(VF_ENOMEM, "host allocation failed");
    h->device = device_id; h->n = n_docs; h->V = V; h->nnz = nnz;
    h->words = (int)(((n_docs + 31) / 32 + kBmWordsPerBlock - 1) / kBmWordsPerBlock * kBmWordsPerBlock);
    h->indptr.assign(indptr, indptr + V + 1);
    const long long per_slot = bm_slot_bytes(h);
    h->slot_cap = (int)std::max(1ll, std::min((long long)kBmMaxSlots, kBmScratchBudget / per_slot));
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_indptr, (size_t)(V + 1) * 8);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_indices, (size_t)std::max<int64_t>(nnz, 1) * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_data, (size_t)std::max<int64_t>(nnz, 1) * 4);
    if (e == hipSuccess) e = hipMemcpy(h->d_indptr, indptr, (size_t)(V + 1) * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(h->d_indices, indices, (size_t)nnz * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && nnz) e = hipMemcpy(h->d_data, data, (size_t)nnz * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        const std::string msg = std::string("vf_bm25_create: ") + hipGetErrorString(e);
        bm_destroy(h);
        return bm_fail(e == hipErrorOutOfMemory ? VF_ENOMEM : VF_EHIP, msg);
    }
    if (slots) *slots = h->slot_cap;
    *out = h;
    return VF_OK;
}

// the scoring and the radix select of the group's queries (slots 0 .. g-1); sel / tblk / out set by the caller
static int bm_score_select(vf_bm25* h, BmArgs& a, const int64_t* q_off, int g) {
    hipStream_t st = h->stream;
    long long maxlen = 0;
    for (int s = 0; s < g; ++s) maxlen = std::max<long long>(maxlen, q_off[a.q0 + s + 1] - q_off[a.q0 + s]);
    for (long long t = 0; t < maxlen; ++t) {   // token positions in order: the fp32 sum runs left to right
        long long post = 0;
        for (int s = 0; s < g; ++s) {
            const long long b = q_off[a.q0 + s], e = q_off[a.q0 + s + 1];
            if (b + t < e) {
                const long long c = h->qterms_host[b + t];
                post = std::max(post, h->indptr[c + 1] - h->indptr[c]);
            }
        }
        if (post == 0) continue;
        hipLaunchKernelGGL(k_bm25_accum, dim3(bm_grid(post, kBmThreads, 4096), g), dim3(kBmThreads), 0, st, a, (int)t);
        VFS_HIP(hipGetLastError());
    }
    const unsigned wblk = (unsigned)(h->words / kBmWordsPerBlock);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(k_bm25_hist, dim3(wblk, g), dim3(kBmThreads), 0, st, a, pass);
        hipLaunchKernelGGL(k_bm25_pick, dim3(1, g), dim3(256), 0, st, a, pass);
    }
    hipLaunchKernelGGL(k_bm25_gather, dim3(wblk, g), dim3(kBmThreads), 0, st, a);
    VFS_HIP(hipGetLastError());
    return VF_OK;
}

static int bm_tail_and_reset(vf_bm25* h, BmArgs& a, const int64_t* q_off, int g, int tail_blocks) {
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(k_bm25_tail_count, dim3(tail_blocks, g), dim3(kBmThreads), 0, st, a);
    hipLaunchKernelGGL(k_bm25_tail_scan, dim3(1, g), dim3(kBmThreads), 0, st, a, tail_blocks);
    hipLaunchKernelGGL(k_bm25_tail_write, dim3(tail_blocks, g), dim3(kBmThreads), 0, st, a);
    long long post = 0;
    for (int s = 0; s < g; ++s) {
        long long p = 0;
        for (long long t = q_off[a.q0 + s]; t < q_off[a.q0 + s + 1]; ++t) {
            const long long c = h->qterms_host[t];
            p = std::max(p, h->indptr[c + 1] - h->indptr[c]);
        }
        post = std::max(post, p);
    }
    if (post > 0) hipLaunchKernelGGL(k_bm25_reset, dim3(bm_grid(post, kBmThreads, 4096), g), dim3(kBmThreads), 0, st, a);
    VFS_HIP(hipGetLastError());
    return VF_OK;
}

extern "C" int vf_bm25_search(vf_bm25* h, const int64_t* q_offsets, const int32_t* q_terms, int32_t nq, int32_t k,
                              int64_t* out_ids, float* out_scores) {
    if (!h) return bm_fail(VF_EINVAL, "vf_bm25_search: null handle");
    if (nq < 0) return bm_fail(VF_EINVAL, "vf_bm25_search: negative nq");
    if (nq == 0) return VF_OK;
    if (!q_offsets || !out_ids || !out_scores) return bm_fail(VF_EINVAL, "vf_bm25_search: null buffer");
    if (k < 1 || (long long)k > h->n) return bm_fail(VF_EINVAL, "vf_bm25_search: k must be in [1, n_docs]");
    if (q_offsets[0] != 0) return bm_fail(VF_EINVAL, "vf_bm25_search: q_offsets[0] must be 0");
    for (int q = 0; q < nq; ++q)
        if (q_offsets[q + 1] < q_offsets[q]) return bm_fail(VF_EINVAL, "vf_bm25_search: q_offsets must be non-decreasing");
    const long long T = q_offsets[nq];
    if (T > 0 && !q_terms) return bm_fail(VF_EINVAL, "vf_bm25_search: null q_terms");
    for (long long t = 0; t < T; ++t)
        if (q_terms[t] < 0 || q_terms[t] >= h->V) return bm_fail(VF_EINVAL, "vf_bm25_search: a token column is out of range");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard guard;
    VFS_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if (nq + 1 > h->q_cap) {
        if (h->d_qoff) (void)hipFree(h->d_qoff);
        h->d_qoff = nullptr; h->q_cap = 0;
        VFS_HIP(hipMalloc((void**)&h->d_qoff, (size_t)(nq + 1) * 8));
        h->q_cap = nq + 1;
    }
    if (std::max<long long>(T, 1) > h->t_cap) {
        if (h->d_qterms) (void)hipFree(h->d_qterms);
        h->d_qterms = nullptr; h->t_cap = 0;
        VFS_HIP(hipMalloc((void**)&h->d_qterms, (size_t)std::max<long long>(T, 1) * 4));
        h->t_cap = std::max<long long>(T, 1);
    }
    VFS_HIP(hipMemcpyAsync(h->d_qoff, q_offsets, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    if (T > 0) VFS_HIP(hipMemcpyAsync(h->d_qterms, q_terms, (size_t)T * 4, hipMemcpyHostToDevice, st));
    h->qterms_host = q_terms;

    BmArgs a{};
    a.indptr = h->d_indptr; a.indices = h->d_indices; a.data = h->d_data;
    a.q_off = h->d_qoff; a.q_terms = h->d_qterms;
    a.n = h->n; a.words = h->words;
    a.k = k;
    const bool small = k <= kBmSmallK;
    const int S = small ? std::min<int>(nq, h->slot_cap) : 1;
    {
        const int rc = bm_ensure_slots(h, std::max(S, h->slots));
        if (rc != VF_OK) return rc;
    }
    if (!small) {
        const int rc = bm_ensure_big(h);
        if (rc != VF_OK) return rc;
    }
    a.scores = h->d_scores; a.score_stride = h->n;
    a.bits = h->d_bits; a.bits_stride = h->words;
    a.hist = h->d_hist; a.st = h->d_st;
    for (int q0 = 0; q0 < nq; q0 += S) {
        const int g = std::min(S, nq - q0);
        a.q0 = q0;
        if (small) {
            a.sel = h->d_sel; a.sel_stride = kBmSmallK; a.sel_cap = kBmSmallK;
            a.tblk = h->d_tblk; a.tblk_stride = 1;
            a.out_ids = h->d_ids; a.out_scores = h->d_out; a.out_stride = k;
            int rc = bm_score_select(h, a, q_offsets, g);
            if (rc != VF_OK) return rc;
            const int Pk = (int)bm_pow2(k);
            hipLaunchKernelGGL(k_bm25_sort_small, dim3(1, g), dim3(512), (size_t)Pk * 8, st, a, Pk);
            // fewer than k touched rows means fewer than kBmSmallK: the tail lies in the first 2 * kBmSmallK rows, one bitmap block
            rc = bm_tail_and_reset(h, a, q_offsets, g, 1);
            if (rc != VF_OK) return rc;
        } else {
            a.sel = h->d_big; a.sel_stride = 0; a.sel_cap = bm_pow2(h->n);
            a.tblk = h->d_big_tblk; a.tblk_stride = 0;
            a.out_ids = h->d_big_ids; a.out_scores = h->d_big_out; a.out_stride = 0;
            int rc = bm_score_select(h, a, q_offsets, 1);
            if (rc != VF_OK) return rc;
            BmState bs;
            VFS_HIP(hipMemcpyAsync(&bs, h->d_st, sizeof(bs), hipMemcpyDeviceToHost, st));
            VFS_HIP(hipStreamSynchronize(st));
            const long long P = bm_pow2(std::max<long long>(bs.nsel, 1));
            if (P > bs.nsel) hipLaunchKernelGGL(k_bm25_pad, dim3(bm_grid(P - bs.nsel, kBmThreads, 4096)), dim3(kBmThreads), 0, st, h->d_big, (long long)bs.nsel, P);
            const int L = (int)std::min<long long>(P, kBmSortChunk);
            const unsigned chunks = (unsigned)(P / L), pairs = bm_grid(P / 2, kBmThreads, 8192);
            hipLaunchKernelGGL(k_bitonic_lds, dim3(chunks), dim3(1024), 0, st, h->d_big, L, 2ll, (long long)L, 1ll);
            for (long long kk = 2ll * L; kk <= P; kk <<= 1) {
                for (long long j = kk >> 1; j >= L; j >>= 1) hipLaunchKernelGGL(k_bitonic_global, dim3(pairs), dim3(kBmThreads), 0, st, h->d_big, P, kk, j);
                hipLaunchKernelGGL(k_bitonic_lds, dim3(chunks), dim3(1024), 0, st, h->d_big, L, kk, kk, (long long)(L / 2));
            }
            if (bs.nsel > 0) hipLaunchKernelGGL(k_bm25_emit, dim3(bm_grid(bs.nsel, kBmThreads, 8192)), dim3(kBmThreads), 0, st, a);
            VFS_HIP(hipGetLastError());
            rc = bm_tail_and_reset(h, a, q_offsets, 1, h->words / kBmWordsPerBlock);
            if (rc != VF_OK) return rc;
        }
        VFS_HIP(hipMemcpyAsync(out_ids + (size_t)q0 * k, a.out_ids, (size_t)g * k * 8, hipMemcpyDeviceToHost, st));
        VFS_HIP(hipMemcpyAsync(out_scores + (size_t)q0 * k, a.out_scores, (size_t)g * k * 4, hipMemcpyDeviceToHost, st));
    }
    VFS_HIP(hipStreamSynchronize(st));
    h->qterms_host = nullptr;
    return VF_OK;
}
