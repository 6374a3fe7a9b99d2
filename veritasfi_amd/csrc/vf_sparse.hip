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
//   k_bm25_*_f, k_bm25_pad_out   a search restricted to a set of rows (VF_BM25_FILTER; the word arithmetic is vf_bm25_filter.h): the scatter
//                      skips rows outside the set, the tail takes allowed rows only from every bitmap block, ranks past the set are padded
//   k_bm25_sub_len, k_bm25_sub_df, k_bm25_accum_s   a filtered search scored by the subset's own statistics (VF_BM25_SUBSTATS; the index
//                      arithmetic is vf_bm25_substats.h): the allowed rows' lengths summed and the allowed postings of each distinct query
//                      column counted (the stage), then a scatter that scores each posting from its tf by the caller's idf and avgdl
//   k_bm25_sub_df_all, k_bm25_accum_sc   a PREPARED row filter (VF_BM25_PREPARED; the index arithmetic is vf_bm25_prepared.h): its bitmap stays
//                      on the device, and in subset mode df is counted once for EVERY column in one pass over the flat posting array,
//                      so that the scatter reads idf per column from the filter's own table and a request uploads only its query
//   k_bm25_accum_m, k_bm25_tail_count_m, k_bm25_tail_write_m, k_bm25_pad_out_m   a prepared filter PER QUERY (VF_BM25_PREPARED_PER_QUERY; the
//                      descriptors and the plan are vf_bm25_multi.h): each slot reads which bitmap, idf table and first padded rank are
//                      its own from a table indexed by its query, and then runs the body of the form that filter means
//   k_bm25_live_*      a live handle's update: documents leave and arrive, every posting is re-scored into a second set of
//                      arrays (described where they stand; the index arithmetic is vf_bm25_live.h)
#include "vf_internal.h"
#include "vf_bm25_live.h"
#include "vf_bm25_filter.h"
#include "vf_bm25_substats.h"
#include "vf_bm25_prepared.h"
#include "vf_bm25_multi.h"

#include <float.h>
#include <algorithm>
#include <mutex>
#include <new>
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
static_assert(kBmWordsPerBlock == kBm25FilterBlockWords, "vf_bm25_filter.h plans the tail over blocks of kBmWordsPerBlock words");
static_assert(kBmThreads == kBm25SubThreads && kBmWordsPerThread == kBm25SubWordsPerThread, "vf_bm25_substats.h plans the counting kernels");
static_assert(kBmThreads == kBm25PrepThreads, "vf_bm25_prepared.h plans the all-columns count");
static_assert(kBmSmallK == kBm25mSmallK, "vf_bm25_multi.h plans the group loop of a filter per query");

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

// kFilt: `allow` is the filter's bitmap; a posting whose row is out is skipped, so it is neither scored nor marked as touched
template <bool kFilt>
__device__ __forceinline__ void bm_accum(const BmArgs& a, int t, const u32* allow) {
    const int s = blockIdx.y, q = a.q0 + s;
    const long long b = a.q_off[q], e = a.q_off[q + 1];
    if (b + t >= e) return;
    const int col = a.q_terms[b + t];
    const long long p0 = a.indptr[col], p1 = a.indptr[col + 1];
    float* sc = a.scores + s * a.score_stride;
    u32* bits = a.bits + s * a.bits_stride;
    for (long long p = p0 + (long long)blockIdx.x * kBmThreads + threadIdx.x; p < p1; p += (long long)gridDim.x * kBmThreads) {
        const u32 row = (u32)a.indices[p];
        if (kFilt && !bm25f_row_allowed(allow, row)) continue;
        sc[row] = sc[row] + a.data[p];
        atomicOr(&bits[row >> 5], 1u << (row & 31u));
    }
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_accum(BmArgs a, int t) { bm_accum<false>(a, t, nullptr); }
__global__ __launch_bounds__(kBmThreads) void k_bm25_accum_f(BmArgs a, int t, const u32* allow) { bm_accum<true>(a, t, allow); }

// ---- a filtered search by the subset's own statistics (vf_bm25_substats.h) ----------------------------------------------------------
struct SubArgs {
    const long long* indptr; const int* indices; const int* tf; const int* doclen;   // the live handle's arrays
    const u32* allow; long long n;                                                    // the filter, [words], zero past n
    const int* dcols; int* df;                                                        // the batch's distinct columns and their counts
    unsigned long long* total;                                                        // the allowed rows' lengths, summed
    const double* idf; double avgdl, k1, b, one_minus_b;                              // the search: idf per q_terms position
};

// the lengths of the allowed rows: one bitmap block per workgroup, a wave reduction, one integer atomic per workgroup (exact: any order)
__global__ __launch_bounds__(kBmThreads) void k_bm25_sub_len(SubArgs a) {
    const int tid = threadIdx.x;
    const long long w0 = bm25s_len_word0(blockIdx.x, tid);
    const uint4 f4 = *(const uint4*)(a.allow + w0);
    const u32 fv[4] = {f4.x, f4.y, f4.z, f4.w};
    unsigned long long s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) s += bm25s_word_len(fv[j], (w0 + j) * 32, a.n, a.doclen);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    __shared__ unsigned long long wsum[kBmThreads / 64];
    if ((tid & 63) == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kBmThreads / 64; ++w) t += wsum[w];
        if (t) atomicAdd(a.total, t);
    }
}

// the allowed postings of distinct column d0 + blockIdx.y: a wave counts by ballot, a workgroup adds once
__global__ __launch_bounds__(kBmThreads) void k_bm25_sub_df(SubArgs a, int d0) {
    const int tid = threadIdx.x, d = d0 + blockIdx.y;
    const int col = a.dcols[d];
    const long long p0 = a.indptr[col], p1 = a.indptr[col + 1];
    int cnt = 0;   // lane 0 of each wave holds the wave's count
    for (long long i = 0;; ++i) {
        const long long base = bm25s_df_base(p0, blockIdx.x, gridDim.x, i);   // the same for the whole workgroup: every lane votes
        if (base >= p1) break;
        const long long p = base + tid;
        const bool in = p < p1 && bm25f_row_allowed(a.allow, (u32)a.indices[p]);
        cnt += __popcll(__ballot(in));
    }
    __shared__ int wsum[kBmThreads / 64];
    if ((tid & 63) == 0) wsum[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < kBmThreads / 64; ++w) t += wsum[w];
        if (t) atomicAdd(&a.df[d], t);
    }
}

// k_bm25_accum_f with the posting's score computed from its tf by the subset's statistics in place of the stored one; idf is indexed
// by the token's position in q_terms.  The same plain read-add-write, one launch per position: the fp32 order is fixed.
// kByCol: idf is a prepared filter's table over the whole vocabulary, indexed by the token's column (k_bm25_accum_sc)
template <bool kByCol>
__device__ __forceinline__ void bm_accum_s(const BmArgs& a, int t, const SubArgs& sa) {
    const int s = blockIdx.y, q = a.q0 + s;
    const long long b = a.q_off[q], e = a.q_off[q + 1];
    if (b + t >= e) return;
    const int col = a.q_terms[b + t];
    const double idf = kByCol ? sa.idf[col] : sa.idf[b + t];
    const long long p0 = a.indptr[col], p1 = a.indptr[col + 1];
    float* sc = a.scores + s * a.score_stride;
    u32* bits = a.bits + s * a.bits_stride;
    for (long long p = p0 + (long long)blockIdx.x * kBmThreads + threadIdx.x; p < p1; p += (long long)gridDim.x * kBmThreads) {
        const u32 row = (u32)a.indices[p];
        if (!bm25f_row_allowed(sa.allow, row)) continue;
        sc[row] = sc[row] + live_score(idf, sa.tf[p], sa.doclen[row], sa.avgdl, sa.k1, sa.b, sa.one_minus_b);
        atomicOr(&bits[row >> 5], 1u << (row & 31u));
    }
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_accum_s(BmArgs a, int t, SubArgs sa) { bm_accum_s<false>(a, t, sa); }
__global__ __launch_bounds__(kBmThreads) void k_bm25_accum_sc(BmArgs a, int t, SubArgs sa) { bm_accum_s<true>(a, t, sa); }

// ---- a prepared filter per query (vf_bm25_multi.h) ----------------------------------------------------------------------------------
// The slot's descriptor: one address per workgroup, read before the kernel's first store, so the loads are scalar
__device__ __forceinline__ Bm25Desc bm_desc(const BmArgs& a, const Bm25Desc* __restrict__ desc) { return desc[a.q0 + blockIdx.y]; }

// bm_accum_s with its filter taken from the slot's descriptor: the bitmap, the idf table (per column) and the scoring parameters
__device__ __forceinline__ void bm_accum_s(const BmArgs& a, int t, const Bm25Desc& d, const int* tf, const int* doclen) {
    SubArgs sa{};
    sa.tf = tf; sa.doclen = doclen; sa.allow = d.allow;
    sa.idf = d.idf; sa.avgdl = d.avgdl; sa.k1 = d.k1; sa.b = d.b; sa.one_minus_b = d.one_minus_b;
    bm_accum_s<true>(a, t, sa);
}

// The scatter of a group whose slots differ in their filter: per slot k_bm25_accum's, k_bm25_accum_f's or k_bm25_accum_sc's body, chosen by
// a branch the whole workgroup takes alike.  tf, doclen: the live handle's (null on a frozen one, which holds no subset-mode filter)
__global__ __launch_bounds__(kBmThreads) void k_bm25_accum_m(BmArgs a, int t, const Bm25Desc* __restrict__ desc, const int* tf, const int* doclen) {
    const Bm25Desc d = bm_desc(a, desc);
    switch (bm25m_form(d)) {
        case kBm25mPlain: bm_accum<false>(a, t, nullptr); break;
        case kBm25mCorpus: bm_accum<true>(a, t, d.allow); break;
        case kBm25mSubset: bm_accum_s(a, t, d, tf, doclen); break;
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

// zero bits (untouched rows < n) of the four words a thread owns in bitmap block b; kFilt: those of them `allow` [words] lets through;
// kSlot: `allow` is the slot's own and may be null, which lets every row through (bm25m_tail_word, word by word)
template <bool kFilt, bool kSlot = false>
__device__ __forceinline__ void bm_zero_words(const BmArgs& a, int s, int b, int tid, const u32* allow, u32 z[4]) {
    const long long w0 = (long long)b * kBmWordsPerBlock + tid * 4;
    const uint4 w4 = *(const uint4*)(a.bits + s * a.bits_stride + w0);
    const u32 wv[4] = {w4.x, w4.y, w4.z, w4.w};
    uint4 f4 = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (kFilt && !kSlot) f4 = *(const uint4*)(allow + w0);
    if (kSlot) f4 = make_uint4(bm25m_tail_word(allow, w0), bm25m_tail_word(allow, w0 + 1), bm25m_tail_word(allow, w0 + 2), bm25m_tail_word(allow, w0 + 3));
    const u32 fv[4] = {f4.x, f4.y, f4.z, f4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) z[j] = bm25f_allowed_untouched(wv[j], bm25f_valid_mask((w0 + j) * 32, a.n), fv[j]);
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
template <bool kFilt, bool kSlot = false>
__device__ __forceinline__ void bm_tail_count(const BmArgs& a, const u32* allow) {
    const int s = blockIdx.y, tid = threadIdx.x;
    if (a.st[s].nsel >= (u32)a.k) return;
    u32 z[4];
    bm_zero_words<kFilt, kSlot>(a, s, blockIdx.x, tid, allow, z);
    __shared__ u32 lds[kBmThreads / 64];
    u32 total;
    block_excl_scan(__popc(z[0]) + __popc(z[1]) + __popc(z[2]) + __popc(z[3]), lds, &total);
    if (tid == 0) a.tblk[s * a.tblk_stride + blockIdx.x] = total;
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_count(BmArgs a) { bm_tail_count<false>(a, nullptr); }
__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_count_f(BmArgs a, const u32* allow) { bm_tail_count<true>(a, allow); }
__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_count_m(BmArgs a, const Bm25Desc* __restrict__ desc) { bm_tail_count<true, true>(a, bm_desc(a, desc).allow); }

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
template <bool kFilt, bool kSlot = false>
__device__ __forceinline__ void bm_tail_write(const BmArgs& a, const u32* allow) {
    const int s = blockIdx.y, tid = threadIdx.x;
    const long long nsel = a.st[s].nsel;
    if (nsel >= a.k) return;
    const long long start = nsel + a.tblk[s * a.tblk_stride + blockIdx.x];
    if (start >= a.k) return;
    u32 z[4];
    bm_zero_words<kFilt, kSlot>(a, s, blockIdx.x, tid, allow, z);
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

__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_write(BmArgs a) { bm_tail_write<false>(a, nullptr); }
__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_write_f(BmArgs a, const u32* allow) { bm_tail_write<true>(a, allow); }
__global__ __launch_bounds__(kBmThreads) void k_bm25_tail_write_m(BmArgs a, const Bm25Desc* __restrict__ desc) { bm_tail_write<true, true>(a, bm_desc(a, desc).allow); }

// a filter that allows fewer than k rows: ranks from .. k - 1 of every slot are padding, written before the sort and the tail write theirs
__global__ __launch_bounds__(kBmThreads) void k_bm25_pad_out(BmArgs a, long long from) {
    const int s = blockIdx.y;
    for (long long i = from + (long long)blockIdx.x * kBmThreads + threadIdx.x; i < a.k; i += (long long)gridDim.x * kBmThreads) {
        a.out_ids[s * a.out_stride + i] = -1;
        a.out_scores[s * a.out_stride + i] = -FLT_MAX;
    }
}

// ... and where every slot has its own filter, from its own rank: the grid covers the group's longest span, a slot without padding starts at k
__global__ __launch_bounds__(kBmThreads) void k_bm25_pad_out_m(BmArgs a, const Bm25Desc* __restrict__ desc) {
    const int s = blockIdx.y;
    for (long long i = bm_desc(a, desc).pad_from + (long long)blockIdx.x * kBmThreads + threadIdx.x; i < a.k; i += (long long)gridDim.x * kBmThreads) {
        a.out_ids[s * a.out_stride + i] = -1;
        a.out_scores[s * a.out_stride + i] = -FLT_MAX;
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

// ---- the live index: one update = remove rows, renumber, append documents, re-score every posting (vf_bm25_live.h) -----------------
// A second set of arrays is written from the old set and the delta; nothing is moved in place.  One workgroup per chunk of C flat
// postings (C <= kLiveMaxChunk), whatever columns they belong to.  Every output element has exactly one writer: no float atomics,
// and the LDS atomicMax that marks column starts is on integers.
//   k_bm25_live_rowmap   old row -> new row or -1 (binary search in the removed rows); document lengths compacted, new ones appended
//   k_bm25_live_count    survivors per chunk
//   k_bm25_live_scan     exclusive prefix of the chunk counts (one workgroup)
//   k_bm25_live_indptr   S(start(c)) + dptr[c] for the column starts each chunk owns: the new indptr
//   k_bm25_live_rewrite  every survivor to S(p) + dptr[col(p)] with its new row, its tf and its new score
//   k_bm25_live_append   the delta's postings behind their columns' survivors
struct LiveArgs {
    const long long* indptr; const int* indices; const int* tf;   // the old set
    long long V, Vn, nnz, n0, n1, n_new; int C;
    const int* rem; long long m;                                  // rows that leave, ascending and distinct
    int* map;                                                     // [n0] new row or -1
    const int* doclen0; int* doclen1; const int* delta_dl;        // [n0], [n1 + n_new], [n_new]
    long long* csum;                                              // [chunks + 1] survivors per chunk, then their exclusive prefix
    const long long* dptr; const int* drows; const int* dtf; long long dnnz;   // the delta CSC over Vn columns, local rows
    long long* newptr;                                            // [Vn + 1]
    int* indices1; int* tf1; float* data1;                        // the new set
    const double* idf; double avgdl, k1, b, one_minus_b;
};

// exclusive prefix over the workgroup's kBmThreads values (Op: sum, or maximum with identity `id`); total = the whole workgroup's
template <typename T, bool kMax>
__device__ __forceinline__ T live_block_scan(T v, T id, T* part, T* total) {
    const int t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (int d = 1; d < kBmThreads; d <<= 1) {
        const T x = t >= d ? part[t - d] : id;
        __syncthreads();
        part[t] = kMax ? (x > part[t] ? x : part[t]) : part[t] + x;
        __syncthreads();
    }
    const T excl = t > 0 ? part[t - 1] : id;
    *total = part[kBmThreads - 1];
    __syncthreads();
    return excl;
}

// the flags rank[0 .. cnt) of a chunk (0 or 1, all written, not yet fenced) to their exclusive prefix: rank[i] = flags set below i,
// rank[cnt] = all of them
__device__ __forceinline__ void live_flags_to_ranks(int cnt, int* rank, int* part) {
    const int t = threadIdx.x;
    __syncthreads();
    const int L = (cnt + kBmThreads - 1) / kBmThreads;
    const int b0 = min(t * L, cnt), b1 = min(b0 + L, cnt);
    int s = 0;
    for (int i = b0; i < b1; ++i) s += rank[i];
    int total;
    int run = live_block_scan<int, false>(s, 0, part, &total);
    for (int i = b0; i < b1; ++i) {
        const int f = rank[i];
        rank[i] = run;
        run += f;
    }
    if (t == 0) rank[cnt] = total;
    __syncthreads();
}

// rows[i] = the new row of the chunk's posting i (or -1); rank[i] = survivors among the postings below i, rank[cnt] = all of them
__device__ __forceinline__ void live_chunk_ranks(const LiveArgs& a, long long lo, int cnt, int* rows, int* rank, int* part) {
    const int t = threadIdx.x;
    for (int i = t; i < cnt; i += kBmThreads) {
        const int r = a.map[a.indices[lo + i]];
        if (rows) rows[i] = r;
        rank[i] = r >= 0;
    }
    live_flags_to_ranks(cnt, rank, part);
}

// ---- a prepared filter's df for EVERY column (vf_bm25_prepared.h): one workgroup per chunk of C flat postings ---------------------------
struct PrepArgs {
    const long long* indptr; const int* indices; long long V, nnz; int C;   // the handle's index
    const u32* allow;                                                       // the prepared filter's own bitmap
    int* df;                                                                // [V], zeroed before the launch
};

// The chunk's postings are flagged by the bitmap and the flags' exclusive prefix is left in LDS; every column that intersects the chunk
// then takes the difference of two prefix entries.  A column wholly inside the chunk has this workgroup as its only writer (a plain
// store); one that crosses a chunk boundary is added to, one integer atomic per (column, chunk).  Empty columns keep the memset's zero.
__global__ __launch_bounds__(kBmThreads) void k_bm25_sub_df_all(PrepArgs a) {
    __shared__ int rank[kLiveMaxChunk + 1];
    __shared__ int part[kBmThreads];
    const LiveChunk ch = live_chunk(a.nnz, a.C, blockIdx.x);
    const int cnt = (int)(ch.hi - ch.lo), t = threadIdx.x;
    if (cnt == 0) return;
    for (int i = t; i < cnt; i += kBmThreads) rank[i] = bm25f_row_allowed(a.allow, (u32)a.indices[ch.lo + i]);
    live_flags_to_ranks(cnt, rank, part);
    const long long c0 = bm25p_first_col(a.indptr, a.V, a.nnz, ch), c1 = bm25p_end_col(a.indptr, a.V, a.nnz, ch);
    for (long long c = c0 + t; c < c1; c += kBmThreads) {   // c < c1 <= V: indptr[c + 1] and df[c] exist
        const Bm25pSpan s = bm25p_span(a.indptr[c], a.indptr[c + 1], ch);
        const int d = rank[s.hi] - rank[s.lo];
        if (s.owned) {
            if (s.hi > s.lo) a.df[c] = d;
        } else if (d) {
            atomicAdd(&a.df[c], d);
        }
    }
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_live_rowmap(LiveArgs a) {
    const long long top = a.n0 > a.n_new ? a.n0 : a.n_new;
    for (long long r = (long long)blockIdx.x * kBmThreads + threadIdx.x; r < top; r += (long long)gridDim.x * kBmThreads) {
        if (r < a.n0) {
            const long long nr = live_new_row(r, a.rem, a.m);
            a.map[r] = (int)nr;
            if (nr >= 0) a.doclen1[nr] = a.doclen0[r];
        }
        if (r < a.n_new) a.doclen1[a.n1 + r] = a.delta_dl[r];
    }
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_live_count(LiveArgs a) {
    __shared__ int wsum[kBmThreads / 64];
    const LiveChunk ch = live_chunk(a.nnz, a.C, blockIdx.x);
    int s = 0;
    for (long long p = ch.lo + threadIdx.x; p < ch.hi; p += kBmThreads) s += a.map[a.indices[p]] >= 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);   // a sum only: one wave reduction and one barrier
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kBmThreads / 64; ++w) total += wsum[w];
        a.csum[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_live_scan(LiveArgs a, long long chunks) {
    __shared__ long long part[kBmThreads];
    const long long L = (chunks + kBmThreads - 1) / kBmThreads;
    const long long b0 = min((long long)threadIdx.x * L, chunks), b1 = min(b0 + L, chunks);
    long long s = 0;
    for (long long i = b0; i < b1; ++i) s += a.csum[i];
    long long total;
    long long run = live_block_scan<long long, false>(s, 0ll, part, &total);
    for (long long i = b0; i < b1; ++i) {
        const long long f = a.csum[i];
        a.csum[i] = run;
        run += f;
    }
    if (threadIdx.x == 0) a.csum[chunks] = total;
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_live_indptr(LiveArgs a) {
    __shared__ int rank[kLiveMaxChunk + 1];
    __shared__ int part[kBmThreads];
    const LiveChunk ch = live_chunk(a.nnz, a.C, blockIdx.x);
    live_chunk_ranks(a, ch.lo, (int)(ch.hi - ch.lo), nullptr, rank, part);
    const long long c0 = live_owned_first(a.indptr, a.V, a.Vn, a.nnz, ch), c1 = live_owned_end(a.indptr, a.V, a.Vn, a.nnz, ch);
    const long long below = a.csum[blockIdx.x];
    for (long long c = c0 + threadIdx.x; c < c1; c += kBmThreads)
        a.newptr[c] = live_dest(below + rank[live_old_start(a.indptr, a.V, a.nnz, c) - ch.lo], a.dptr[c]);
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_live_rewrite(LiveArgs a) {
    __shared__ int rank[kLiveMaxChunk + 1];
    __shared__ int rows[kLiveMaxChunk];
    __shared__ int col[kLiveMaxChunk];
    __shared__ int part[kBmThreads];
    const LiveChunk ch = live_chunk(a.nnz, a.C, blockIdx.x);
    const int cnt = (int)(ch.hi - ch.lo), t = threadIdx.x;
    if (cnt == 0) return;
    // the column of every posting: the one that holds the chunk's first posting, then the last column that starts at or below it
    const long long cfirst = live_col_of(a.indptr, a.V, a.Vn, a.nnz, ch.lo), cend = live_col_lower(a.indptr, a.V, a.Vn, a.nnz, ch.hi);
    for (int i = t; i < cnt; i += kBmThreads) col[i] = i == 0 ? (int)cfirst : -1;
    __syncthreads();
    for (long long c = cfirst + 1 + t; c < cend; c += kBmThreads) atomicMax(&col[a.indptr[c] - ch.lo], (int)c);   // c < cend <= V: starts in (lo, hi)
    __syncthreads();
    {
        const int L = (cnt + kBmThreads - 1) / kBmThreads;
        const int b0 = min(t * L, cnt), b1 = min(b0 + L, cnt);
        int mx = -1;
        for (int i = b0; i < b1; ++i) mx = max(mx, col[i]);
        int total;
        int run = live_block_scan<int, true>(mx, -1, part, &total);
        for (int i = b0; i < b1; ++i) {
            run = max(run, col[i]);
            col[i] = run;
        }
    }
    live_chunk_ranks(a, ch.lo, cnt, rows, rank, part);
    const long long below = a.csum[blockIdx.x];
    for (int i = t; i < cnt; i += kBmThreads) {
        const int r = rows[i];
        if (r < 0) continue;
        const int c = col[i], f = a.tf[ch.lo + i];
        const long long d = live_dest(below + rank[i], a.dptr[c]);
        a.indices1[d] = r;
        a.tf1[d] = f;
        a.data1[d] = live_score(a.idf[c], f, a.doclen1[r], a.avgdl, a.k1, a.b, a.one_minus_b);
    }
}

__global__ __launch_bounds__(kBmThreads) void k_bm25_live_append(LiveArgs a) {
    for (long long q = (long long)blockIdx.x * kBmThreads + threadIdx.x; q < a.dnnz; q += (long long)gridDim.x * kBmThreads) {
        long long lo = 0, hi = a.Vn;   // the delta column of q: the last c with dptr[c] <= q
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (a.dptr[mid + 1] <= q) lo = mid + 1; else hi = mid;
        }
        const long long d = live_delta_dest(a.newptr[lo + 1], a.dptr[lo + 1], q);
        const int r = (int)(a.n1 + a.drows[q]), f = a.dtf[q];
        a.indices1[d] = r;
        a.tf1[d] = f;
        a.data1[d] = live_score(a.idf[lo], f, a.doclen1[r], a.avgdl, a.k1, a.b, a.one_minus_b);
    }
}

}  // namespace vf

// ---- the host path ---------------------------------------------------------------------------------------------------------------
// Everything above is device code; from here on the host decides what runs.
//   the mode of a call     vf_bm25_call.h: bm25c_decode turns `nq`'s flag bits and the struct's phase into one of eight kinds or a
//                          refusal, bm25c_plan turns (kind, k, nq, slots, words, m) into the kernels of the group loop.  vf_bm25_search
//                          is decode, the checks every kind shares, the filter resolved into a BmFilter (bm_filter_check, then
//                          bm_filter_bind once the slots exist), one group loop.  A prepared search whose mode is
//                          VF_BM25_PREPARED_PER_QUERY resolves one filter per query instead (bm_multi_check): vf_bm25_multi.h holds its
//                          descriptors and its plan, bm_multi_launch_plan puts that plan into the group loop's terms.
//   the checks             each written once: bm_check_allow (a caller's bitmap), bm_check_scoring (idf, avgdl, k1, b), bm_all_padding,
//                          bm_sub_args (the SubArgs of the stage, the prepare and both scored searches).
//   device memory          bm_free frees and nulls, bm_alloc makes a list of buffers or none of them, bm_grow serves the buffers that
//                          follow a call's size.  The handle owns the index arrays, the query buffers, d_sub and d_sidf for its whole
//                          life; the slots' scratch with d_allow and d_ftblk (bm_free_slots) and the deep-k scratch (bm_free_big) until
//                          an update changes n; a BmStage owns an update's second set of arrays until the commit swaps them in; a
//                          BmPrepared owns its bitmap and idf table until it is released or an update makes it stale.
#include "vf_bm25_call.h"

#include <initializer_list>

using namespace vf;

static_assert(kBm25cFilter == VF_BM25_FILTER && kBm25cSubstats == VF_BM25_SUBSTATS && kBm25cPrepared == VF_BM25_PREPARED, "vf_bm25_call.h decodes the ABI's flag bits");
static_assert(kBm25cSmallK == kBmSmallK, "vf_bm25_call.h plans the small-k arm");
static_assert(VF_BM25_SUBSTATS_STAGE == 1 && VF_BM25_SUBSTATS_SEARCH == 2 && VF_BM25_PREPARED_PREPARE == 1 && VF_BM25_PREPARED_ARM == 2 &&
              VF_BM25_PREPARED_SEARCH == 3 && VF_BM25_PREPARED_RELEASE == 4, "vf_bm25_call.h decodes the ABI's phases");

static int bm_fail(int code, const std::string& msg) { return vf::set_error(code, msg); }
static int bm_hip_fail(const char* what, hipError_t e) { return bm_fail(e == hipErrorOutOfMemory ? VF_ENOMEM : VF_EHIP, std::string(what) + ": " + hipGetErrorString(e)); }

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
    // a filtered search (VF_BM25_FILTER) also holds these from the first such call on; they go with the slots
    u32* d_allow = nullptr;                 // [words] the filter of the call in flight, zero past n
    u32* d_ftblk = nullptr;                 // [slots][words / kBmWordsPerBlock]: the filtered small-k tail counts every bitmap block
    // a live handle (VF_BM25_LIVE) also keeps what a re-scoring needs
    bool live = false;
    bool born = true;                       // false between the stage and the commit that create a live handle
    int* d_tf = nullptr;                    // [nnz] term frequency of each posting
    int* d_doclen = nullptr;                // [n] tokens per document
    struct BmStage* stage = nullptr;        // a staged update: the second set of arrays, not yet swapped in
    unsigned long long gen = 1;             // the update generation: every commit makes it the next one
    // a search by the subset's statistics (VF_BM25_SUBSTATS) also holds these from the first such call on
    unsigned long long* d_sub = nullptr;    // the stage's counts: the length sum (8 B), then df [sub_cap] and the distinct columns [sub_cap]
    long long sub_cap = 0;
    double* d_sidf = nullptr;               // [sidf_cap] the search's idf per q_terms position
    long long sidf_cap = 0;
    std::vector<u32> staged_allow;          // the bitmap the last stage left in d_allow, while allow_staged: its search does not upload it again
    bool allow_staged = false;
    // prepared filters (VF_BM25_PREPARED): each owns its device memory; none aliases d_allow
    std::vector<struct BmPrepared*> prepared;
    unsigned long long next_token = 1;
    // a prepared filter per query (VF_BM25_PREPARED_PER_QUERY) also holds these from the first such call on
    Bm25Desc* d_desc = nullptr;             // [desc_cap] the descriptors of the call in flight, one per query
    long long desc_cap = 0;
    std::vector<Bm25Desc> desc_host;        // what goes up to d_desc: it outlives the copy
    std::mutex mu;
};

// One prepared filter.  A committed update frees its device memory and leaves the entry (stale) so that its token is refused by
// generation; a release or the handle's end removes it.
struct BmPrepared {
    unsigned long long token = 0, gen = 0;
    bool subset = false, armed = false, stale = false;
    long long m = 0, total_len = 0, V = 0, bytes = 0;
    u32* d_allow = nullptr;                 // [words] the filter's own bitmap, zero past n
    double* d_idf = nullptr;                // subset mode: [V] the subset's idf per column
    double avgdl = 1.0, k1 = 0.0, b = 0.0;  // subset mode, from the arm
};

// What a stage leaves for its commit.  Everything an update allocates is allocated here, before the first kernel.
struct BmStage {
    long long n1 = 0, n_new = 0, Vn = 0, dnnz = 0, cap = 0, chunks = 0;
    int C = kLiveMaxChunk;
    int* d_rem = nullptr; int* d_map = nullptr; int* d_doclen1 = nullptr; int* d_delta_dl = nullptr;
    long long* d_csum = nullptr; long long* d_dptr = nullptr; int* d_drows = nullptr; int* d_dtf = nullptr;
    long long* d_newptr = nullptr; int* d_indices1 = nullptr; int* d_tf1 = nullptr; float* d_data1 = nullptr;
    double* d_idf = nullptr;
    long long m = 0;
    std::vector<long long> newptr;          // host copy of the new indptr
};

static long long bm_pow2(long long v) {
    long long p = 1;
    while (p < v) p <<= 1;
    return p;
}

static long long bm_slot_bytes(const vf_bm25* h) {
    return h->n * 4 + (long long)h->words * 4 + 256 * 4 + (long long)sizeof(BmState) + 4 + (long long)kBmSmallK * (8 + 8 + 4);
}

// ---- device buffers: every hipMalloc and hipFree of the BM25 leg goes through these three ---------------------------------------------
template <class... T>
static void bm_free(T*&... p) {   // free and null
    ((p ? (void)hipFree((void*)p) : (void)0, p = nullptr), ...);
}

struct BmBuf { void** p; size_t bytes; };
template <class T>
static BmBuf bm_buf(T*& p, size_t bytes) { return BmBuf{(void**)&p, bytes}; }

// Makes every buffer of the list (all null on entry; an entry of 0 bytes is not wanted and stays null) or, on a failure, none of them: what
// it made is freed and null again.  `what` opens the message.
static int bm_alloc(const char* what, std::initializer_list<BmBuf> bufs) {
    for (const BmBuf& b : bufs) {
        const hipError_t e = b.bytes ? hipMalloc(b.p, b.bytes) : hipSuccess;
        if (e == hipSuccess) continue;
        *b.p = nullptr;
        for (const BmBuf& made : bufs) bm_free(*made.p);   // the entries past the failure are null still
        return bm_hip_fail(what, e);
    }
    return VF_OK;
}

// a buffer that follows a call's size: made again (its contents are the call's own) when `want` entries exceed what it holds
template <class T>
static int bm_grow(const char* what, T*& p, long long& cap, long long want, size_t bytes) {
    if (want <= cap) return VF_OK;
    bm_free(p);
    cap = 0;
    const int rc = bm_alloc(what, {bm_buf(p, bytes)});
    if (rc == VF_OK) cap = want;
    return rc;
}

static void bm_free_slots(vf_bm25* h) {
    // d_allow and d_ftblk are sized by the slots and the words that go here: the next filtered call makes them again
    bm_free(h->d_scores, h->d_bits, h->d_hist, h->d_st, h->d_sel, h->d_tblk, h->d_ids, h->d_out, h->d_allow, h->d_ftblk);
    h->allow_staged = false;
    h->slots = 0;
}

static void bm_free_big(vf_bm25* h) { bm_free(h->d_big, h->d_big_tblk, h->d_big_ids, h->d_big_out); }

// what a filtered call holds beyond the slots (after bm_ensure_slots: h->slots and h->words are the call's)
static int bm_ensure_filter(vf_bm25* h) {
    if (h->d_allow) return VF_OK;   // made and dropped together: d_allow stands for both
    const size_t wbytes = (size_t)h->words * 4;
    const int rc = bm_alloc("vf_bm25: filter scratch", {bm_buf(h->d_allow, wbytes), bm_buf(h->d_ftblk, (size_t)h->slots * (size_t)(h->words / kBmWordsPerBlock) * 4)});
    if (rc != VF_OK) return rc;
    const hipError_t e = hipMemsetAsync(h->d_allow, 0, wbytes, h->stream);   // the words past n stay zero
    if (e == hipSuccess) return VF_OK;
    bm_free(h->d_allow, h->d_ftblk);
    return bm_hip_fail("vf_bm25: filter scratch", e);
}

// the per-query scratch of `want` slots, zeroed (the reset keeps it zero between queries)
static int bm_ensure_slots(vf_bm25* h, int want) {
    if (want <= h->slots) return VF_OK;
    VFS_HIP(hipStreamSynchronize(h->stream));
    bm_free_slots(h);
    const size_t S = (size_t)want;
    const int rc = bm_alloc("vf_bm25: query scratch", {bm_buf(h->d_scores, S * h->n * 4), bm_buf(h->d_bits, S * h->words * 4), bm_buf(h->d_hist, S * 256 * 4),
                                                        bm_buf(h->d_st, S * sizeof(BmState)), bm_buf(h->d_sel, S * kBmSmallK * 8), bm_buf(h->d_tblk, S * 4),
                                                        bm_buf(h->d_ids, S * kBmSmallK * 8), bm_buf(h->d_out, S * kBmSmallK * 4)});
    if (rc != VF_OK) return rc;
    hipError_t e = hipMemsetAsync(h->d_scores, 0, S * h->n * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_bits, 0, S * h->words * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_hist, 0, S * 256 * 4, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_st, 0, S * sizeof(BmState), h->stream);
    if (e != hipSuccess) { bm_free_slots(h); return bm_hip_fail("vf_bm25: query scratch", e); }
    h->slots = want;
    return VF_OK;
}

static int bm_ensure_big(vf_bm25* h) {   // all four or none: d_big stands for them
    return h->d_big ? VF_OK : bm_alloc("vf_bm25: deep-k scratch", {bm_buf(h->d_big, (size_t)bm_pow2(h->n) * 8), bm_buf(h->d_big_tblk, (size_t)(h->words / kBmWordsPerBlock) * 4),
                                                bm_buf(h->d_big_ids, (size_t)h->n * 8), bm_buf(h->d_big_out, (size_t)h->n * 4)});
}

static unsigned bm_grid(long long work, long long per_block, long long cap) {
    long long g = (work + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

static void bm_drop_stage(vf_bm25* h) {
    BmStage* s = h->stage;
    if (!s) return;
    bm_free(s->d_rem, s->d_map, s->d_doclen1, s->d_delta_dl, s->d_csum, s->d_dptr, s->d_drows, s->d_dtf, s->d_newptr, s->d_indices1, s->d_tf1,
            s->d_data1, s->d_idf);
    delete s;
    h->stage = nullptr;
}

static void bm_prepared_free_device(BmPrepared* f) {
    bm_free(f->d_allow, f->d_idf);
    f->bytes = 0;
}

// a committed update: no prepared filter may search again (rows have moved); the tokens stay known until they are released
static void bm_prepared_invalidate(vf_bm25* h) {
    for (BmPrepared* f : h->prepared) {
        bm_prepared_free_device(f);
        f->stale = true; f->armed = false;
    }
}

static void bm_prepared_free_all(vf_bm25* h) {
    for (BmPrepared* f : h->prepared) {
        bm_prepared_free_device(f);
        delete f;
    }
    h->prepared.clear();
}

static LiveArgs bm_live_args(const vf_bm25* h, const BmStage* s) {
    LiveArgs a{};
    a.indptr = h->d_indptr; a.indices = h->d_indices; a.tf = h->d_tf;
    a.V = h->V; a.Vn = s->Vn; a.nnz = h->nnz; a.n0 = h->n; a.n1 = s->n1; a.n_new = s->n_new; a.C = s->C;
    a.rem = s->d_rem; a.m = s->m; a.map = s->d_map;
    a.doclen0 = h->d_doclen; a.doclen1 = s->d_doclen1; a.delta_dl = s->d_delta_dl;
    a.csum = s->d_csum;
    a.dptr = s->d_dptr; a.drows = s->d_drows; a.dtf = s->d_dtf; a.dnnz = s->dnnz;
    a.newptr = s->d_newptr; a.indices1 = s->d_indices1; a.tf1 = s->d_tf1; a.data1 = s->d_data1;
    return a;
}

static int bm_destroy(vf_bm25* h) {
    if (!h) return VF_OK;
    DeviceGuard guard;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    bm_free_slots(h);
    bm_free_big(h);
    bm_drop_stage(h);
    bm_prepared_free_all(h);
    bm_free(h->d_indptr, h->d_indices, h->d_data, h->d_qoff, h->d_qterms, h->d_tf, h->d_doclen, h->d_sub, h->d_sidf, h->d_desc);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return VF_OK;
}

static void bm_set_docs(vf_bm25* h, long long n) {   // what depends on the document count
    h->n = n;
    h->words = (int)(((n + 31) / 32 + kBmWordsPerBlock - 1) / kBmWordsPerBlock * kBmWordsPerBlock);
    h->slot_cap = (int)std::max(1ll, std::min((long long)kBmMaxSlots, kBmScratchBudget / bm_slot_bytes(h)));
}

// A handle on device `dev` with its stream and nothing else; the caller's DeviceGuard puts the thread's device back.
static int bm_new_handle(int dev, vf_bm25** out) {
    int ndev = 0;
    VFS_HIP(hipGetDeviceCount(&ndev));
    if (dev < 0 || dev >= ndev) return bm_fail(VF_EINVAL, "vf_bm25_create: bad device_id");
    VFS_HIP(hipSetDevice(dev));
    vf_bm25* h = new (std::nothrow) vf_bm25();
    if (!h) return bm_fail(VF_ENOMEM, "host allocation failed");
    h->device = dev;
    const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { bm_destroy(h); return bm_hip_fail("vf_bm25_create", e); }
    *out = h;
    return VF_OK;
}

// ---- live updates (include/veritasfi_hip.h: VF_BM25_LIVE) ---------------------------------------------------------------------
// Phase 1.  Validates, allocates all the update needs, uploads the delta, runs the row map, the survivor count and the scan, and
// returns the new per-column counts.  The handle's arrays are only read.
static int bm_live_stage(vf_bm25* h, vf_bm25_delta* d) {
    bm_drop_stage(h);
    if (!h->live) return bm_fail(VF_EINVAL, "vf_bm25_create: VF_BM25_LIVE on a handle that was not created live (it keeps no term frequencies)");
    const long long Vn = d->vocab, n_new = d->n_new, n0 = h->n;
    if (Vn < h->V) return bm_fail(VF_EINVAL, "vf_bm25_create: the delta's vocabulary is smaller than the handle's (columns never disappear)");
    if (Vn > 0x7FFFFFFEll) return bm_fail(VF_EINVAL, "vf_bm25_create: the vocabulary must stay below 2^31 - 1 columns (the kernels keep columns as int32)");
    if (n_new > 0x7FFFFFFFll) return bm_fail(VF_EINVAL, "vf_bm25_create: n_docs must stay in [1, 2^31 - 1]");
    if (n_new < 0 || d->n_remove < 0 || !d->indptr || !d->counts || (d->n_remove > 0 && !d->remove))
        return bm_fail(VF_EINVAL, "vf_bm25_create: null or negative field in vf_bm25_delta");
    const int C = d->chunk == 0 ? kLiveMaxChunk : d->chunk;
    if (C < 1 || C > kLiveMaxChunk) return bm_fail(VF_EINVAL, "vf_bm25_create: vf_bm25_delta.chunk must be 0 or in [1, " + std::to_string(kLiveMaxChunk) + "]");
    const long long dnnz = d->indptr[Vn];
    if (d->indptr[0] != 0 || dnnz < 0 || (dnnz > 0 && (!d->rows || !d->tf))) return bm_fail(VF_EINVAL, "vf_bm25_create: the delta's indptr must start at 0 and end at its posting count");
    std::vector<int> delta_dl((size_t)n_new, 0);
    for (long long c = 0; c < Vn; ++c) {   // what vf_bm25_create checks of an index, with tf >= 1 in place of score > 0
        if (d->indptr[c + 1] < d->indptr[c] || d->indptr[c + 1] > dnnz) return bm_fail(VF_EINVAL, "vf_bm25_create: the delta's indptr is not non-decreasing");
        for (long long p = d->indptr[c]; p < d->indptr[c + 1]; ++p) {
            if (d->rows[p] < 0 || d->rows[p] >= n_new) return bm_fail(VF_EINVAL, "vf_bm25_create: a document row of the delta is out of range");
            if (p > d->indptr[c] && d->rows[p] <= d->rows[p - 1])
                return bm_fail(VF_EINVAL, "vf_bm25_create: rows of a delta column must be strictly ascending (one posting per document)");
            if (d->tf[p] < 1) return bm_fail(VF_EINVAL, "vf_bm25_create: a term frequency of the delta is below 1");
            if ((long long)delta_dl[d->rows[p]] + d->tf[p] > 0x7FFFFFFFll) return bm_fail(VF_EINVAL, "vf_bm25_create: a document of the delta is longer than 2^31 - 1 tokens");
            delta_dl[d->rows[p]] += d->tf[p];
        }
    }
    std::vector<int> rem((size_t)d->n_remove);
    for (long long i = 0; i < d->n_remove; ++i) {
        if (d->remove[i] < 0 || d->remove[i] >= n0)
            return bm_fail(VF_EINVAL, "vf_bm25_create: remove[" + std::to_string(i) + "] = " + std::to_string(d->remove[i]) + " is outside 0 .. " + std::to_string(n0 - 1));
        rem[i] = (int)d->remove[i];
    }
    std::sort(rem.begin(), rem.end());
    rem.erase(std::unique(rem.begin(), rem.end()), rem.end());
    const long long m = (long long)rem.size(), n1 = n0 - m;
    if (n1 + n_new < 1) return bm_fail(VF_EINVAL, "vf_bm25_create: the update would leave no document (n_docs >= 1)");
    if (n1 + n_new > 0x7FFFFFFFll) return bm_fail(VF_EINVAL, "vf_bm25_create: n_docs must stay in [1, 2^31 - 1]");

    BmStage* s = new (std::nothrow) BmStage();
    if (!s) return bm_fail(VF_ENOMEM, "host allocation failed");
    h->stage = s;
    s->n1 = n1; s->n_new = n_new; s->Vn = Vn; s->dnnz = dnnz; s->C = C; s->m = m;
    s->cap = h->nnz + dnnz;                       // survivors <= nnz: known exactly only after the count, and allocations come first
    s->chunks = live_chunks(h->nnz, C);
    try { s->newptr.resize((size_t)Vn + 1); } catch (const std::bad_alloc&) { bm_drop_stage(h); return bm_fail(VF_ENOMEM, "host allocation failed"); }
    const auto some = [](long long count) { return (size_t)std::max(1ll, count); };
    const int rc = bm_alloc("vf_bm25_create (stage)", {bm_buf(s->d_rem, some(m) * 4), bm_buf(s->d_map, some(n0) * 4), bm_buf(s->d_doclen1, (size_t)(n1 + n_new) * 4),
                                                       bm_buf(s->d_delta_dl, some(n_new) * 4), bm_buf(s->d_csum, (size_t)(s->chunks + 1) * 8),
                                                       bm_buf(s->d_dptr, (size_t)(Vn + 1) * 8), bm_buf(s->d_drows, some(dnnz) * 4), bm_buf(s->d_dtf, some(dnnz) * 4),
                                                       bm_buf(s->d_newptr, (size_t)(Vn + 1) * 8), bm_buf(s->d_indices1, some(s->cap) * 4),
                                                       bm_buf(s->d_tf1, some(s->cap) * 4), bm_buf(s->d_data1, some(s->cap) * 4), bm_buf(s->d_idf, some(Vn) * 8)});
    if (rc != VF_OK) { bm_drop_stage(h); return rc; }
    hipStream_t st = h->stream;
    hipError_t e = hipSuccess;
    if (m) e = hipMemcpyAsync(s->d_rem, rem.data(), (size_t)m * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_new) e = hipMemcpyAsync(s->d_delta_dl, delta_dl.data(), (size_t)n_new * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_dptr, d->indptr, (size_t)(Vn + 1) * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && dnnz) e = hipMemcpyAsync(s->d_drows, d->rows, (size_t)dnnz * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && dnnz) e = hipMemcpyAsync(s->d_dtf, d->tf, (size_t)dnnz * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        LiveArgs a = bm_live_args(h, s);
        hipLaunchKernelGGL(k_bm25_live_rowmap, dim3(bm_grid(std::max(n0, n_new), kBmThreads, 8192)), dim3(kBmThreads), 0, st, a);
        hipLaunchKernelGGL(k_bm25_live_count, dim3((unsigned)s->chunks), dim3(kBmThreads), 0, st, a);
        hipLaunchKernelGGL(k_bm25_live_scan, dim3(1), dim3(kBmThreads), 0, st, a, s->chunks);
        hipLaunchKernelGGL(k_bm25_live_indptr, dim3((unsigned)s->chunks), dim3(kBmThreads), 0, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(s->newptr.data(), s->d_newptr, (size_t)(Vn + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { bm_drop_stage(h); return bm_hip_fail("vf_bm25_create (stage)", e); }
    for (long long c = 0; c < Vn; ++c) d->counts[c] = s->newptr[c + 1] - s->newptr[c];
    d->n_removed = m;
    return VF_OK;
}

// Phase 2.  Re-scores and rewrites every posting into the staged arrays, then swaps them in.
static int bm_live_commit(vf_bm25* h, const vf_bm25_delta* d) {
    BmStage* s = h->stage;
    if (!s) return bm_fail(VF_EINVAL, "vf_bm25_create: VF_BM25_COMMIT without a staged update");
    if (!d->idf || d->vocab != s->Vn || !(d->avgdl > 0.0) || !(d->k1 >= 0.0) || !(d->b >= 0.0 && d->b <= 1.0)) {
        bm_drop_stage(h);
        return bm_fail(VF_EINVAL, "vf_bm25_create: the commit needs idf[vocab] of the staged vocabulary, avgdl > 0, k1 >= 0 and b in [0, 1]");
    }
    hipStream_t st = h->stream;
    LiveArgs a = bm_live_args(h, s);
    a.idf = s->d_idf; a.avgdl = d->avgdl; a.k1 = d->k1; a.b = d->b; a.one_minus_b = 1.0 - d->b;
    hipError_t e = hipSuccess;
    if (s->Vn) e = hipMemcpyAsync(s->d_idf, d->idf, (size_t)s->Vn * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        if (h->nnz) hipLaunchKernelGGL(k_bm25_live_rewrite, dim3((unsigned)s->chunks), dim3(kBmThreads), 0, st, a);
        if (s->dnnz) hipLaunchKernelGGL(k_bm25_live_append, dim3(bm_grid(s->dnnz, kBmThreads, 8192)), dim3(kBmThreads), 0, st, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { bm_drop_stage(h); return bm_fail(VF_EHIP, std::string("vf_bm25_create (commit): ") + hipGetErrorString(e)); }
    // the swap: from here nothing can fail
    bm_free(h->d_indptr, h->d_indices, h->d_data, h->d_tf, h->d_doclen);
    h->d_indptr = s->d_newptr; h->d_indices = s->d_indices1; h->d_data = s->d_data1; h->d_tf = s->d_tf1; h->d_doclen = s->d_doclen1;
    s->d_newptr = nullptr; s->d_indices1 = nullptr; s->d_data1 = nullptr; s->d_tf1 = nullptr; s->d_doclen1 = nullptr;
    h->indptr.swap(s->newptr);
    h->V = s->Vn; h->nnz = h->indptr[(size_t)s->Vn];
    const long long n = s->n1 + s->n_new;
    if (n != h->n) {   // the per-query scratch is sized by n: dropped, and made again (zeroed) by the next search
        bm_free_slots(h);
        bm_free_big(h);
        bm_set_docs(h, n);
    }
    h->born = true;
    ++h->gen;                  // what a VF_BM25_SUBSTATS stage counted is no longer this index's
    h->allow_staged = false;
    bm_prepared_invalidate(h); // ... and no prepared filter's bits are this index's rows
    bm_drop_stage(h);
    return VF_OK;
}

static int bm_live_fetch(vf_bm25* h, const vf_bm25_delta* d) {
    if (!h->live || !h->born) return bm_fail(VF_EINVAL, "vf_bm25_create: VF_BM25_FETCH needs a live handle");
    hipStream_t st = h->stream;
    if (d->out_indptr) VFS_HIP(hipMemcpyAsync(d->out_indptr, h->d_indptr, (size_t)(h->V + 1) * 8, hipMemcpyDeviceToHost, st));
    if (d->out_indices && h->nnz) VFS_HIP(hipMemcpyAsync(d->out_indices, h->d_indices, (size_t)h->nnz * 4, hipMemcpyDeviceToHost, st));
    if (d->out_data && h->nnz) VFS_HIP(hipMemcpyAsync(d->out_data, h->d_data, (size_t)h->nnz * 4, hipMemcpyDeviceToHost, st));
    if (d->out_tf && h->nnz) VFS_HIP(hipMemcpyAsync(d->out_tf, h->d_tf, (size_t)h->nnz * 4, hipMemcpyDeviceToHost, st));
    if (d->out_doc_len) VFS_HIP(hipMemcpyAsync(d->out_doc_len, h->d_doclen, (size_t)h->n * 4, hipMemcpyDeviceToHost, st));
    VFS_HIP(hipStreamSynchronize(st));
    return VF_OK;
}

static int bm_live_call(vf_bm25_delta* d, int32_t device_id, vf_bm25** out, int32_t* slots) {
    const int phase = device_id & (VF_BM25_LIVE | VF_BM25_COMMIT | VF_BM25_DISCARD | VF_BM25_FETCH);
    const int dev = device_id & 0xFFF;
    if (phase != VF_BM25_LIVE && phase != VF_BM25_COMMIT && phase != VF_BM25_DISCARD && phase != VF_BM25_FETCH)
        return bm_fail(VF_EINVAL, "vf_bm25_create: exactly one of VF_BM25_LIVE, VF_BM25_COMMIT, VF_BM25_DISCARD and VF_BM25_FETCH");
    vf_bm25* h = *out;
    if (!h) {   // a stage on no handle starts one: it is born by its commit
        if (phase != VF_BM25_LIVE) return bm_fail(VF_EINVAL, "vf_bm25_create: null handle");
        DeviceGuard guard;
        int rc = bm_new_handle(dev, &h);
        if (rc != VF_OK) return rc;
        h->live = true; h->born = false;
        rc = bm_alloc("vf_bm25_create", {bm_buf(h->d_indptr, 8)});
        if (rc == VF_OK) {
            const hipError_t e = hipMemset(h->d_indptr, 0, 8);
            if (e != hipSuccess) rc = bm_hip_fail("vf_bm25_create", e);
        }
        if (rc != VF_OK) { bm_destroy(h); return rc; }
        try {   // the host vectors of a stage allocate: no exception leaves the C ABI
            h->indptr.assign(1, 0);
            rc = bm_live_stage(h, d);
        } catch (const std::bad_alloc&) {
            rc = bm_fail(VF_ENOMEM, "host allocation failed");
        }
        if (rc != VF_OK) { bm_destroy(h); return rc; }
        *out = h;
        return VF_OK;
    }
    if (dev != h->device) return bm_fail(VF_EINVAL, "vf_bm25_create: device_id is not the handle's device");
    int rc;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        DeviceGuard guard;
        VFS_HIP(hipSetDevice(h->device));
        if (phase == VF_BM25_LIVE) {
            try {
                rc = bm_live_stage(h, d);
            } catch (const std::bad_alloc&) {   // as every refusal of a stage: the handle is as it was
                bm_drop_stage(h);
                rc = bm_fail(VF_ENOMEM, "host allocation failed");
            }
        } else if (phase == VF_BM25_COMMIT) rc = bm_live_commit(h, d);
        else if (phase == VF_BM25_FETCH) rc = bm_live_fetch(h, d);
        else { bm_drop_stage(h); rc = VF_OK; }
        if (rc == VF_OK && slots) *slots = h->slot_cap;
        if (h->born) return rc;
    }
    if (rc != VF_OK || phase == VF_BM25_DISCARD) {   // a handle that was never born does not outlive its failed or discarded creation
        bm_destroy(h);
        *out = nullptr;
    }
    return rc;
}

extern "C" int vf_bm25_create(const int64_t* indptr, int64_t V, const int32_t* indices, const float* data, int64_t nnz,
                              int64_t n_docs, int32_t device_id, vf_bm25** out, int32_t* slots) {
    if (!out) return bm_fail(VF_EINVAL, "vf_bm25_create: null out");
    if (!indptr) {   // release (realloc-style): the handle *out is destroyed
        bm_destroy(*out);
        *out = nullptr;
        return VF_OK;
    }
    if (device_id >= 0 && (device_id & ~0xFFF))   // a live update: `indptr` is a vf_bm25_delta
        return bm_live_call((vf_bm25_delta*)(void*)indptr, device_id, out, slots);
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
    DeviceGuard guard;
    vf_bm25* h = nullptr;
    int rc = bm_new_handle(device_id, &h);
    if (rc != VF_OK) return rc;
    h->V = V; h->nnz = nnz;
    bm_set_docs(h, n_docs);
    h->indptr.assign(indptr, indptr + V + 1);
    const size_t pbytes = (size_t)std::max<int64_t>(nnz, 1) * 4;
    rc = bm_alloc("vf_bm25_create", {bm_buf(h->d_indptr, (size_t)(V + 1) * 8), bm_buf(h->d_indices, pbytes), bm_buf(h->d_data, pbytes)});
    if (rc == VF_OK) {
        hipError_t e = hipMemcpy(h->d_indptr, indptr, (size_t)(V + 1) * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess && nnz) e = hipMemcpy(h->d_indices, indices, (size_t)nnz * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess && nnz) e = hipMemcpy(h->d_data, data, (size_t)nnz * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = bm_hip_fail("vf_bm25_create", e);
    }
    if (rc != VF_OK) { bm_destroy(h); return rc; }
    if (slots) *slots = h->slot_cap;
    *out = h;
    return VF_OK;
}

// ---- a search by the subset's own statistics (include/veritasfi_hip.h: VF_BM25_SUBSTATS) --------------------------------------------
// ---- the checks the modes share, each written once ---------------------------------------------------------------------------------
// a caller's bitmap (`who`: the flag or phase it came with): not null, made for this document count, no bit at or past it; fc->m: rows allowed
static int bm_check_allow(const vf_bm25* h, const uint32_t* allow, long long n_docs, Bm25FilterCheck* fc, const char* who) {
    if (!allow) return bm_fail(VF_EINVAL, std::string("vf_bm25_search: ") + who + " with a null allow bitmap");
    if (n_docs != h->n)
        return bm_fail(VF_EINVAL, "vf_bm25_search: the filter was made for " + std::to_string(n_docs) + " documents, the handle holds " +
                                      std::to_string(h->n) + " (a live handle may have changed since the bitmap was made: make it again)");
    *fc = bm25f_check(allow, h->n);
    if (fc->bad_row >= 0)
        return bm_fail(VF_EINVAL, "vf_bm25_search: the filter allows row " + std::to_string(fc->bad_row) + ", at or past n_docs = " + std::to_string(h->n));
    return VF_OK;
}

// what a scored search takes from its caller (`who`: the phase that brought it): idf[count] finite and >= 0, avgdl > 0, k1 >= 0, b in [0, 1]
static int bm_check_scoring(const double* idf, long long count, double avgdl, double k1, double b, const char* who) {
    for (long long i = 0; i < count; ++i)
        if (!(idf[i] >= 0.0) || !(idf[i] <= DBL_MAX)) return bm_fail(VF_EINVAL, "vf_bm25_search: idf[" + std::to_string(i) + "] is negative or not finite");
    if (!(avgdl > 0.0) || !(avgdl <= DBL_MAX) || !(k1 >= 0.0) || !(b >= 0.0 && b <= 1.0))
        return bm_fail(VF_EINVAL, std::string("vf_bm25_search: ") + who + " needs avgdl > 0, k1 >= 0 and b in [0, 1]");
    return VF_OK;
}

// nothing may be returned: every rank of every query is padding (a stage's outputs may be absent)
static void bm_all_padding(int64_t* out_ids, float* out_scores, int nq, int k) {
    if (!out_ids || !out_scores || k < 1) return;
    std::fill(out_ids, out_ids + (size_t)nq * k, (int64_t)-1);
    std::fill(out_scores, out_scores + (size_t)nq * k, -FLT_MAX);
}

// the SubArgs of the counting kernels (counts: the length sum, then df as int32) and of the scoring scatters (idf and what follows it)
static SubArgs bm_sub_args(const vf_bm25* h, const u32* allow, unsigned long long* counts, const double* idf = nullptr, double avgdl = 1.0, double k1 = 0.0, double b = 0.0) {
    SubArgs sa{};
    sa.indptr = h->d_indptr; sa.indices = h->d_indices; sa.tf = h->d_tf; sa.doclen = h->d_doclen;
    sa.allow = allow; sa.n = h->n;
    sa.total = counts; sa.df = counts ? (int*)(counts + 1) : nullptr;
    sa.idf = idf; sa.avgdl = avgdl; sa.k1 = k1; sa.b = b; sa.one_minus_b = 1.0 - b;
    return sa;
}

// The stage.  Every check has passed and m > 0.  Uploads the bitmap (it stays for the search that follows), sums the allowed rows'
// lengths, counts the allowed postings of the batch's distinct columns, and writes the struct's out members last.  S: that search's slots
static int bm_substats_stage(vf_bm25* h, vf_bm25_substats_query* sq, long long m, const int32_t* q_terms, int S, long long T) {
    const uint32_t* allow_host = sq->allow;
    std::vector<int32_t> distinct, pos2d;
    std::vector<unsigned long long> back;   // the length sum, then the counts (two int32 per word)
    long long D = 0;
    const size_t aw = (size_t)bm25f_words(h->n);
    try {
        D = bm25s_dedupe(q_terms, T, distinct, pos2d);
        back.assign((size_t)(1 + (D + 1) / 2), 0ull);
        h->staged_allow.assign(allow_host, allow_host + aw);
    } catch (const std::bad_alloc&) {
        h->allow_staged = false;
        return bm_fail(VF_ENOMEM, "host allocation failed");
    }
    h->allow_staged = false;
    DeviceGuard guard;
    VFS_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    int rc = bm_ensure_slots(h, std::max(S, h->slots));   // the slots of the search that follows, so that it does not make d_allow again
    if (rc == VF_OK) rc = bm_ensure_filter(h);
    const long long cap = std::max<long long>(D, 1) + (std::max<long long>(D, 1) & 1);   // even: the columns start on 8 bytes as well
    if (rc == VF_OK) rc = bm_grow("vf_bm25: subset counts", h->d_sub, h->sub_cap, cap, 8 + (size_t)cap * 8);
    if (rc != VF_OK) return rc;
    SubArgs sa = bm_sub_args(h, h->d_allow, h->d_sub);
    sa.dcols = sa.df + h->sub_cap;
    VFS_HIP(hipMemcpyAsync(h->d_allow, allow_host, aw * 4, hipMemcpyHostToDevice, st));
    VFS_HIP(hipMemsetAsync(h->d_sub, 0, 8 + (size_t)h->sub_cap * 4, st));
    if (D > 0) VFS_HIP(hipMemcpyAsync((void*)sa.dcols, distinct.data(), (size_t)D * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bm25_sub_len, dim3((unsigned)(h->words / kBmWordsPerBlock)), dim3(kBmThreads), 0, st, sa);
    long long most = 0;
    for (long long d = 0; d < D; ++d) most = std::max(most, h->indptr[(size_t)distinct[d] + 1] - h->indptr[(size_t)distinct[d]]);
    if (most > 0) {
        const unsigned gx = bm25s_df_plan(most);
        for (long long d0 = 0; d0 < D; d0 += 32768)   // grid.y holds fewer than 65 536
            hipLaunchKernelGGL(k_bm25_sub_df, dim3(gx, (unsigned)std::min<long long>(32768, D - d0)), dim3(kBmThreads), 0, st, sa, (int)d0);
    }
    VFS_HIP(hipGetLastError());
    VFS_HIP(hipMemcpyAsync(back.data(), h->d_sub, 8 + (size_t)D * 4, hipMemcpyDeviceToHost, st));
    VFS_HIP(hipStreamSynchronize(st));
    const int32_t* df = (const int32_t*)(back.data() + 1);
    for (long long t = 0; t < T; ++t) sq->df[t] = df[pos2d[(size_t)t]];
    sq->total_len = (int64_t)back[0]; sq->m = m; sq->generation = h->gen;
    h->allow_staged = true;
    return VF_OK;
}

// ---- prepared filters (include/veritasfi_hip.h: VF_BM25_PREPARED) -----------------------------------------------------------------
static BmPrepared* bm_prepared_find(vf_bm25* h, unsigned long long token) {
    for (BmPrepared* f : h->prepared)
        if (f->token == token) return f;
    return nullptr;
}

static int bm_prepared_stale(const vf_bm25* h, const BmPrepared* f, const char* what) {
    return bm_fail(VF_EINVAL, std::string("vf_bm25_search: ") + what + ": the filter was prepared at update generation " + std::to_string(f->gen) +
                                  ", the handle is at " + std::to_string(h->gen) + " (the live index was updated since: prepare the filter again)");
}

// PREPARE.  Everything is checked and allocated before the first device write; the filter joins the handle and the struct's out members
// are written last, so a failure leaves the handle and every other filter as they were.
static int bm_prepared_prepare(vf_bm25* h, vf_bm25_prepared_query* pq) {
    if (pq->mode != VF_BM25_PREPARED_CORPUS && pq->mode != VF_BM25_PREPARED_SUBSET)
        return bm_fail(VF_EINVAL, "vf_bm25_search: vf_bm25_prepared_query.mode must be VF_BM25_PREPARED_CORPUS or VF_BM25_PREPARED_SUBSET");
    const bool subset = pq->mode == VF_BM25_PREPARED_SUBSET;
    Bm25FilterCheck fc{};
    int rc = bm_check_allow(h, pq->allow, pq->n_docs, &fc, "VF_BM25_PREPARED_PREPARE");
    if (rc != VF_OK) return rc;
    const int C = pq->chunk == 0 ? kLiveMaxChunk : pq->chunk;
    if (subset) {
        if (!h->live || !h->born)
            return bm_fail(VF_EUNSUPPORTED, "vf_bm25_search: a prepared filter in subset mode needs a live handle (VF_BM25_LIVE): only it keeps the term frequencies and the document lengths");
        if (pq->vocab != h->V || (h->V > 0 && !pq->df))
            return bm_fail(VF_EINVAL, "vf_bm25_search: VF_BM25_PREPARED_PREPARE in subset mode needs df[vocab] with vocab = the handle's " + std::to_string(h->V) + " columns");
        if (C < 1 || C > kLiveMaxChunk) return bm_fail(VF_EINVAL, "vf_bm25_search: vf_bm25_prepared_query.chunk must be 0 or in [1, " + std::to_string(kLiveMaxChunk) + "]");
    }
    BmPrepared* f = new (std::nothrow) BmPrepared();
    if (!f) return bm_fail(VF_ENOMEM, "host allocation failed");
    const long long V = h->V;
    std::vector<unsigned long long> back;   // the length sum, then the counts (two int32 per word)
    try {
        h->prepared.reserve(h->prepared.size() + 1);
        if (subset) back.assign((size_t)(1 + (V + 1) / 2), 0ull);
    } catch (const std::bad_alloc&) {
        delete f;
        return bm_fail(VF_ENOMEM, "host allocation failed");
    }
    DeviceGuard guard;
    hipError_t e = hipSetDevice(h->device);
    hipStream_t st = h->stream;
    const size_t aw = (size_t)bm25f_words(h->n), wbytes = (size_t)h->words * 4, ventries = (size_t)std::max<long long>(V, 1), cbytes = 8 + ventries * 4;
    unsigned long long* d_cnt = nullptr;    // subset mode, for this call only: the length sum (8 B), then df [V] as int32
    rc = e != hipSuccess ? bm_hip_fail("vf_bm25_search (prepare)", e)
                         : bm_alloc("vf_bm25_search (prepare)", {bm_buf(f->d_allow, wbytes), bm_buf(f->d_idf, subset ? ventries * 8 : 0), bm_buf(d_cnt, subset ? cbytes : 0)});
    if (rc != VF_OK) { delete f; return rc; }
    e = hipMemsetAsync(f->d_allow, 0, wbytes, st);   // the words past n stay zero
    if (e == hipSuccess) e = hipMemcpyAsync(f->d_allow, pq->allow, aw * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && subset && fc.m > 0) {
        e = hipMemsetAsync(d_cnt, 0, cbytes, st);
        if (e == hipSuccess) {
            const SubArgs sa = bm_sub_args(h, f->d_allow, d_cnt);
            hipLaunchKernelGGL(k_bm25_sub_len, dim3((unsigned)(h->words / kBmWordsPerBlock)), dim3(kBmThreads), 0, st, sa);
            if (h->nnz > 0) {
                PrepArgs pa{};
                pa.indptr = h->d_indptr; pa.indices = h->d_indices; pa.V = V; pa.nnz = h->nnz; pa.C = C;
                pa.allow = f->d_allow; pa.df = (int*)(d_cnt + 1);
                hipLaunchKernelGGL(k_bm25_sub_df_all, dim3((unsigned)live_chunks(h->nnz, C)), dim3(kBmThreads), 0, st, pa);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(back.data(), d_cnt, 8 + (size_t)V * 4, hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    bm_free(d_cnt);
    if (e != hipSuccess) { bm_prepared_free_device(f); delete f; return bm_hip_fail("vf_bm25_search (prepare)", e); }
    f->token = h->next_token++; f->gen = h->gen; f->subset = subset; f->m = fc.m; f->V = V;
    f->total_len = subset ? (long long)back[0] : 0;
    f->bytes = (long long)wbytes + (subset ? std::max<long long>(V, 1) * 8 : 0);
    h->prepared.push_back(f);   // reserved above: does not allocate
    if (subset) {
        const int32_t* df = (const int32_t*)(back.data() + 1);
        for (long long c = 0; c < V; ++c) pq->df[c] = df[c];
        pq->total_len = f->total_len;
    }
    pq->token = f->token; pq->m = f->m; pq->generation = f->gen; pq->bytes = f->bytes;
    return VF_OK;
}

static int bm_prepared_arm(vf_bm25* h, const vf_bm25_prepared_query* pq) {
    BmPrepared* f = bm_prepared_find(h, pq->token);
    if (!f) return bm_fail(VF_EINVAL, "vf_bm25_search: VF_BM25_PREPARED_ARM: token " + std::to_string(pq->token) + " names no prepared filter of this handle (unknown or released)");
    if (!f->subset) return bm_fail(VF_EINVAL, "vf_bm25_search: VF_BM25_PREPARED_ARM: the filter was prepared in corpus mode (it has no idf table)");
    if (f->stale || f->gen != h->gen) return bm_prepared_stale(h, f, "VF_BM25_PREPARED_ARM");
    if (pq->vocab != f->V || (f->V > 0 && !pq->idf))
        return bm_fail(VF_EINVAL, "vf_bm25_search: VF_BM25_PREPARED_ARM needs idf[vocab] with vocab = the filter's " + std::to_string(f->V) + " columns");
    const int rc = bm_check_scoring(pq->idf, f->V, pq->avgdl, pq->k1, pq->b, "VF_BM25_PREPARED_ARM");
    if (rc != VF_OK) return rc;
    DeviceGuard guard;
    VFS_HIP(hipSetDevice(h->device));
    if (f->V > 0) VFS_HIP(hipMemcpyAsync(f->d_idf, pq->idf, (size_t)f->V * 8, hipMemcpyHostToDevice, h->stream));
    VFS_HIP(hipStreamSynchronize(h->stream));
    f->avgdl = pq->avgdl; f->k1 = pq->k1; f->b = pq->b; f->armed = true;
    return VF_OK;
}

static int bm_prepared_release(vf_bm25* h, const vf_bm25_prepared_query* pq) {
    BmPrepared* f = bm_prepared_find(h, pq->token);
    if (!f) return bm_fail(VF_EINVAL, "vf_bm25_search: VF_BM25_PREPARED_RELEASE: token " + std::to_string(pq->token) + " names no prepared filter of this handle (unknown or released)");
    DeviceGuard guard;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->prepared.erase(std::find(h->prepared.begin(), h->prepared.end(), f));
    bm_prepared_free_device(f);
    delete f;
    return VF_OK;
}

// ---- the search --------------------------------------------------------------------------------------------------------------------
static const char* const kBmRefusalText[kBm25Refusals] = {
    "",
    "vf_bm25_search: VF_BM25_PREPARED goes alone (the prepared filter carries its rows and its mode)",
    "vf_bm25_search: VF_BM25_PREPARED with a null vf_bm25_prepared_query",
    "vf_bm25_search: vf_bm25_prepared_query.phase must be one of the four VF_BM25_PREPARED_* phases",
    "vf_bm25_search: VF_BM25_FILTER with a null vf_bm25_filter_query",
    "vf_bm25_search: vf_bm25_substats_query.phase must be VF_BM25_SUBSTATS_STAGE or VF_BM25_SUBSTATS_SEARCH",
    "vf_bm25_search: VF_BM25_SUBSTATS goes with VF_BM25_FILTER (the statistics are those of the allowed rows)",
};

// What `q_offsets` points to in a flagged call, as the one struct type its flags say it is; the two others stay null.
struct BmCallArg {
    const vf_bm25_filter_query* fq = nullptr;   // VF_BM25_FILTER alone
    vf_bm25_substats_query* sq = nullptr;       // VF_BM25_FILTER | VF_BM25_SUBSTATS
    vf_bm25_prepared_query* pq = nullptr;       // VF_BM25_PREPARED
    BmCallArg(const void* p, int nq_raw) {
        if (nq_raw & VF_BM25_PREPARED) pq = (vf_bm25_prepared_query*)p;
        else if (nq_raw & VF_BM25_SUBSTATS) sq = (vf_bm25_substats_query*)p;
        else fq = (const vf_bm25_filter_query*)p;
    }
    const int64_t* q_offsets() const { return pq ? pq->q_offsets : sq ? sq->q_offsets : fq->q_offsets; }
    const uint32_t* allow() const { return sq ? sq->allow : fq->allow; }
    long long n_docs() const { return sq ? sq->n_docs : fq->n_docs; }
};

// The filter of a call, resolved: what the scatter and the tail read.  bm_filter_check fills m from the host's side, before any device
// work; bm_filter_bind, once the slots exist, sets the device bitmap and the scoring scatters' arguments.
struct BmFilter {
    const u32* allow = nullptr;       // device bitmap; null: every row may be returned
    long long m = 0;                  // rows allowed
    const BmPrepared* pf = nullptr;   // kBm25PrepSearch: the filter its token names
    SubArgs sub{};                    // read by the scatters that score from tf (the plan's kBm25ScatterSubPos and kBm25ScatterSubCol)
    const Bm25Desc* desc = nullptr;   // a filter per query: the call's descriptors on the device (the _m kernels read them; allow, m, pf and sub
                                      // are then not used) and, host_desc, the same on the host for the padding's grid
    const Bm25Desc* host_desc = nullptr;
};

// Every check of the call's filter, in the order of include/veritasfi_hip.h.  A prepared search's filter is found here, under the lock, and with it
// its mode: c.subset is set for the plan (the decoder cannot know it).
// A prepared search with a filter per query (mode VF_BM25_PREPARED_PER_QUERY): tokens[i] names query i's filter, 0 none.  Checked in query
// order, each as the one-token search checks its own; then the descriptors are written into the handle's host table (pointers into the
// filters' own device memory: nothing of a filter is copied).  A refusal leaves the table unread.
static int bm_multi_check(vf_bm25* h, const vf_bm25_prepared_query* pq, int nq, int k, BmFilter* f) {
    if (!pq->tokens) return bm_fail(VF_EINVAL, "vf_bm25_search: VF_BM25_PREPARED_PER_QUERY with a null tokens (one token per query, 0 for a query without a filter)");
    try {
        h->desc_host.resize((size_t)nq);
    } catch (const std::bad_alloc&) {
        return bm_fail(VF_ENOMEM, "host allocation failed");
    }
    for (int i = 0; i < nq; ++i) {
        const unsigned long long token = pq->tokens[i];
        if (token == 0) { h->desc_host[(size_t)i] = bm25m_desc_none(k); continue; }
        const std::string who = "tokens[" + std::to_string(i) + "] = " + std::to_string(token);
        const BmPrepared* pf = bm_prepared_find(h, token);
        if (!pf) return bm_fail(VF_EINVAL, "vf_bm25_search: " + who + " names no prepared filter of this handle (unknown or released)");
        if (pf->stale || pf->gen != h->gen) return bm_prepared_stale(h, pf, ("VF_BM25_PREPARED_SEARCH, " + who).c_str());
        if (pf->subset && !pf->armed)
            return bm_fail(VF_EINVAL, "vf_bm25_search: " + who + ": the prepared filter is in subset mode and was never armed (VF_BM25_PREPARED_ARM gives it its idf)");
        h->desc_host[(size_t)i] = bm25m_desc(pf->d_allow, pf->subset ? pf->d_idf : nullptr, pf->avgdl, pf->k1, pf->b, pf->m, k);
    }
    f->host_desc = h->desc_host.data();
    return VF_OK;
}

static int bm_filter_check(vf_bm25* h, Bm25Call& c, const BmCallArg& arg, long long T, int k, BmFilter* f) {
    if (c.kind == kBm25Plain) return VF_OK;
    if (c.kind == kBm25PrepSearch && arg.pq->mode == VF_BM25_PREPARED_PER_QUERY) return bm_multi_check(h, arg.pq, c.nq, k, f);
    if (c.kind == kBm25PrepSearch) {   // the filter's own checks were made when it was prepared: only that it is still this index's is looked at here
        const unsigned long long token = arg.pq->token;
        const BmPrepared* pf = bm_prepared_find(h, token);
        if (!pf) return bm_fail(VF_EINVAL, "vf_bm25_search: token " + std::to_string(token) + " names no prepared filter of this handle (unknown or released)");
        if (pf->stale || pf->gen != h->gen) return bm_prepared_stale(h, pf, "VF_BM25_PREPARED_SEARCH");
        if (pf->subset && !pf->armed)
            return bm_fail(VF_EINVAL, "vf_bm25_search: the prepared filter is in subset mode and was never armed (VF_BM25_PREPARED_ARM gives it its idf)");
        f->pf = pf; f->m = pf->m; c.subset = pf->subset;
        return VF_OK;
    }
    Bm25FilterCheck fc{};
    const int rc = bm_check_allow(h, arg.allow(), arg.n_docs(), &fc, "VF_BM25_FILTER");
    if (rc != VF_OK) return rc;
    f->m = fc.m;
    if (c.kind == kBm25Filtered) return VF_OK;
    const vf_bm25_substats_query* sq = arg.sq;
    if (!h->live || !h->born)
        return bm_fail(VF_EUNSUPPORTED, "vf_bm25_search: VF_BM25_SUBSTATS needs a live handle (VF_BM25_LIVE): only it keeps the term frequencies and the document lengths");
    if (c.kind == kBm25SubStage) return T > 0 && !sq->df ? bm_fail(VF_EINVAL, "vf_bm25_search: VF_BM25_SUBSTATS_STAGE with a null df") : VF_OK;
    if (sq->generation != h->gen)
        return bm_fail(VF_EINVAL, "vf_bm25_search: the statistics were staged at update generation " + std::to_string(sq->generation) + ", the handle is at " +
                                      std::to_string(h->gen) + " (the live index was updated between the stage and the search: stage again)");
    if (T > 0 && !sq->idf) return bm_fail(VF_EINVAL, "vf_bm25_search: VF_BM25_SUBSTATS_SEARCH with a null idf");
    return bm_check_scoring(sq->idf, T, sq->avgdl, sq->k1, sq->b, "VF_BM25_SUBSTATS_SEARCH");
}

static int bm_filter_bind(vf_bm25* h, const Bm25Call& c, const BmCallArg& arg, long long T, BmFilter* f) {
    if (c.kind == kBm25Plain) return VF_OK;
    int rc = bm_ensure_filter(h);   // d_allow, and the tail's scratch over every bitmap block
    if (rc != VF_OK) return rc;
    if (f->host_desc) {   // a filter per query: c.nq descriptors go up beside the query, nothing of any filter (d_allow is not touched)
        rc = bm_grow("vf_bm25: query descriptors", h->d_desc, h->desc_cap, c.nq, (size_t)c.nq * sizeof(Bm25Desc));
        if (rc != VF_OK) return rc;
        VFS_HIP(hipMemcpyAsync(h->d_desc, f->host_desc, (size_t)c.nq * sizeof(Bm25Desc), hipMemcpyHostToDevice, h->stream));
        f->desc = h->d_desc;
        return VF_OK;
    }
    if (f->pf) {   // nothing goes up: the bitmap is the filter's own (d_allow and what a stage left in it are not touched)
        f->allow = f->pf->d_allow;
        if (c.subset) f->sub = bm_sub_args(h, f->allow, nullptr, f->pf->d_idf, f->pf->avgdl, f->pf->k1, f->pf->b);
        return VF_OK;
    }
    // the bitmap goes up with every filtered call (n / 8 bytes): no filter is kept on the device between calls ...
    // ... except from a VF_BM25_SUBSTATS stage to its search: the stage's copy serves when it holds these very words
    const bool scored = c.kind == kBm25SubSearch;
    const size_t aw = (size_t)bm25f_words(h->n);
    const bool staged = scored && h->allow_staged && h->staged_allow.size() == aw && std::equal(h->staged_allow.begin(), h->staged_allow.end(), arg.allow());
    h->allow_staged = false;
    if (!staged) VFS_HIP(hipMemcpyAsync(h->d_allow, arg.allow(), aw * 4, hipMemcpyHostToDevice, h->stream));
    f->allow = h->d_allow;
    if (!scored) return VF_OK;
    rc = bm_grow("vf_bm25: idf of the query positions", h->d_sidf, h->sidf_cap, std::max<long long>(T, 1), (size_t)std::max<long long>(T, 1) * 8);
    if (rc != VF_OK) return rc;
    if (T > 0) VFS_HIP(hipMemcpyAsync(h->d_sidf, arg.sq->idf, (size_t)T * 8, hipMemcpyHostToDevice, h->stream));
    f->sub = bm_sub_args(h, f->allow, nullptr, h->d_sidf, arg.sq->avgdl, arg.sq->k1, arg.sq->b);
    return VF_OK;
}

// the plan of a call with a filter per query (vf_bm25_multi.h) in the group loop's terms: the tail's buffers are the filtered call's, the
// scatter and the padding are chosen per slot on the device (the _m kernels), so `scatter`, `pad_from` and `pad_out` are not read
static Bm25LaunchPlan bm_multi_launch_plan(const Bm25MultiPlan& mp, long long k) {
    Bm25LaunchPlan p{};
    p.no_launch = mp.no_launch; p.small = mp.small; p.S = mp.S;
    p.scatter = kBm25ScatterFiltered; p.tail_f = true; p.tail_blocks = mp.tail_blocks; p.tblk_stride = mp.tblk_stride;
    p.pad_from = k; p.pad_out = false;
    return p;
}

// the scoring and the radix select of the group's queries (slots 0 .. g-1); sel / tblk / out set by the caller
static int bm_score_select(vf_bm25* h, BmArgs& a, const int64_t* q_off, int g, const Bm25LaunchPlan& p, const BmFilter& f) {
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
        const dim3 grid(bm_grid(post, kBmThreads, 4096), g), block(kBmThreads);
        if (f.desc) hipLaunchKernelGGL(k_bm25_accum_m, grid, block, 0, st, a, (int)t, f.desc, (const int*)h->d_tf, (const int*)h->d_doclen);   // each slot its own form
        else switch (p.scatter) {   // the filtered forms skip the rows outside the set; the two last score each posting from its tf
            case kBm25ScatterPlain: hipLaunchKernelGGL(k_bm25_accum, grid, block, 0, st, a, (int)t); break;
            case kBm25ScatterFiltered: hipLaunchKernelGGL(k_bm25_accum_f, grid, block, 0, st, a, (int)t, f.allow); break;
            case kBm25ScatterSubPos: hipLaunchKernelGGL(k_bm25_accum_s, grid, block, 0, st, a, (int)t, f.sub); break;       // idf per q_terms position
            case kBm25ScatterSubCol: hipLaunchKernelGGL(k_bm25_accum_sc, grid, block, 0, st, a, (int)t, f.sub); break;      // idf per column
        }
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

// k > kBmSmallK, one query: the search's one read-back (how many keys the select gathered), then the global bitonic sort of that many
static int bm_sort_deep(vf_bm25* h, BmArgs& a) {
    hipStream_t st = h->stream;
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
    return VF_OK;
}

static int bm_tail_and_reset(vf_bm25* h, BmArgs& a, const int64_t* q_off, int g, const Bm25LaunchPlan& p, const BmFilter& f) {
    hipStream_t st = h->stream;
    const dim3 grid(p.tail_blocks, g), block(kBmThreads);
    if (f.desc) hipLaunchKernelGGL(k_bm25_tail_count_m, grid, block, 0, st, a, f.desc);
    else if (p.tail_f) hipLaunchKernelGGL(k_bm25_tail_count_f, grid, block, 0, st, a, f.allow);
    else hipLaunchKernelGGL(k_bm25_tail_count, grid, block, 0, st, a);
    hipLaunchKernelGGL(k_bm25_tail_scan, dim3(1, g), block, 0, st, a, p.tail_blocks);
    if (f.desc) hipLaunchKernelGGL(k_bm25_tail_write_m, grid, block, 0, st, a, f.desc);
    else if (p.tail_f) hipLaunchKernelGGL(k_bm25_tail_write_f, grid, block, 0, st, a, f.allow);
    else hipLaunchKernelGGL(k_bm25_tail_write, grid, block, 0, st, a);
    long long post = 0;
    for (int s = 0; s < g; ++s)
        for (long long t = q_off[a.q0 + s]; t < q_off[a.q0 + s + 1]; ++t) {
            const long long c = h->qterms_host[t];
            post = std::max(post, h->indptr[c + 1] - h->indptr[c]);
        }
    if (post > 0) hipLaunchKernelGGL(k_bm25_reset, dim3(bm_grid(post, kBmThreads, 4096), g), block, 0, st, a);
    VFS_HIP(hipGetLastError());
    return VF_OK;
}

extern "C" int vf_bm25_search(vf_bm25* h, const int64_t* q_offsets, const int32_t* q_terms, int32_t nq, int32_t k,
                              int64_t* out_ids, float* out_scores) {
    if (!h) return bm_fail(VF_EINVAL, "vf_bm25_search: null handle");
    if (nq < 0) return bm_fail(VF_EINVAL, "vf_bm25_search: negative nq");
    // 1. the kind of call: `arg` is a flagged call's struct
    const BmCallArg arg(q_offsets, nq);
    Bm25Call c = bm25c_decode(nq, !q_offsets, q_offsets && bm25c_has_phase(nq) ? (arg.pq ? arg.pq->phase : arg.sq->phase) : 0);
    if (c.refusal) return bm_fail(VF_EINVAL, kBmRefusalText[c.refusal]);
    if (c.kind == kBm25PrepPrepare || c.kind == kBm25PrepArm || c.kind == kBm25PrepRelease) {
        std::lock_guard<std::mutex> lk(h->mu);
        return c.kind == kBm25PrepPrepare ? bm_prepared_prepare(h, arg.pq) : c.kind == kBm25PrepArm ? bm_prepared_arm(h, arg.pq) : bm_prepared_release(h, arg.pq);
    }
    if (c.kind != kBm25Plain) q_offsets = arg.q_offsets();
    nq = c.nq;
    const bool stage = c.kind == kBm25SubStage;   // it reads neither k nor the outputs
    // 2. the checks every kind shares
    if (nq == 0) return VF_OK;
    if (!q_offsets || (!stage && (!out_ids || !out_scores))) return bm_fail(VF_EINVAL, "vf_bm25_search: null buffer");
    std::lock_guard<std::mutex> lk(h->mu);   // before n_docs and the vocabulary are read: a live handle's update changes both
    if (!stage && (k < 1 || (long long)k > h->n)) return bm_fail(VF_EINVAL, "vf_bm25_search: k must be in [1, n_docs]");
    if (q_offsets[0] != 0) return bm_fail(VF_EINVAL, "vf_bm25_search: q_offsets[0] must be 0");
    for (int q = 0; q < nq; ++q)
        if (q_offsets[q + 1] < q_offsets[q]) return bm_fail(VF_EINVAL, "vf_bm25_search: q_offsets must be non-decreasing");
    const long long T = q_offsets[nq];
    if (T > 0 && !q_terms) return bm_fail(VF_EINVAL, "vf_bm25_search: null q_terms");
    for (long long t = 0; t < T; ++t)
        if (q_terms[t] < 0 || q_terms[t] >= h->V) return bm_fail(VF_EINVAL, "vf_bm25_search: a token column is out of range");
    // 3. the filter, and with its m the plan
    BmFilter f;
    int rc = bm_filter_check(h, c, arg, T, k, &f);
    if (rc != VF_OK) return rc;
    Bm25LaunchPlan p = bm25c_plan(c, k, nq, h->slot_cap, h->words, f.m);
    if (f.host_desc) p = bm_multi_launch_plan(bm25m_plan(f.host_desc, k, nq, h->slot_cap, h->words), k);
    if (p.no_launch) {   // no row is allowed
        bm_all_padding(out_ids, out_scores, nq, k);
        if (stage) {
            std::fill(arg.sq->df, arg.sq->df + T, (int64_t)0);
            arg.sq->total_len = 0; arg.sq->m = 0; arg.sq->generation = h->gen;
        }
        return VF_OK;
    }
    if (stage) return bm_substats_stage(h, arg.sq, f.m, q_terms, p.S, T);
    DeviceGuard guard;
    VFS_HIP(hipSetDevice(h->device));
    hipStream_t st = h->stream;
    rc = bm_grow("vf_bm25: query offsets", h->d_qoff, h->q_cap, nq + 1, (size_t)(nq + 1) * 8);
    if (rc == VF_OK) rc = bm_grow("vf_bm25: query tokens", h->d_qterms, h->t_cap, std::max<long long>(T, 1), (size_t)std::max<long long>(T, 1) * 4);
    if (rc != VF_OK) return rc;
    VFS_HIP(hipMemcpyAsync(h->d_qoff, q_offsets, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, st));
    if (T > 0) VFS_HIP(hipMemcpyAsync(h->d_qterms, q_terms, (size_t)T * 4, hipMemcpyHostToDevice, st));
    h->qterms_host = q_terms;
    rc = bm_ensure_slots(h, std::max(p.S, h->slots));
    if (rc == VF_OK && !p.small) rc = bm_ensure_big(h);
    if (rc == VF_OK) rc = bm_filter_bind(h, c, arg, T, &f);
    if (rc != VF_OK) return rc;
    // 4. one loop over groups of S queries; the two arms differ in their buffers and their sort
    BmArgs a{};
    a.indptr = h->d_indptr; a.indices = h->d_indices; a.data = h->d_data;
    a.q_off = h->d_qoff; a.q_terms = h->d_qterms;
    a.n = h->n; a.words = h->words; a.k = k;
    a.scores = h->d_scores; a.score_stride = h->n;
    a.bits = h->d_bits; a.bits_stride = h->words;
    a.hist = h->d_hist; a.st = h->d_st;
    a.sel = p.small ? h->d_sel : h->d_big; a.sel_stride = p.small ? kBmSmallK : 0; a.sel_cap = p.small ? kBmSmallK : bm_pow2(h->n);
    a.tblk = !p.small ? h->d_big_tblk : p.tail_f ? h->d_ftblk : h->d_tblk; a.tblk_stride = p.tblk_stride;
    a.out_ids = p.small ? h->d_ids : h->d_big_ids; a.out_scores = p.small ? h->d_out : h->d_big_out; a.out_stride = p.small ? k : 0;
    const unsigned pad_grid = bm_grid(k - p.pad_from, kBmThreads, 64);   // a filtered call of fewer than k rows pads ranks pad_from .. k - 1
    const int Pk = (int)bm_pow2(k);
    for (int q0 = 0; q0 < nq; q0 += p.S) {
        const int g = std::min(p.S, nq - q0);
        a.q0 = q0;
        rc = bm_score_select(h, a, q_offsets, g, p, f);
        if (rc != VF_OK) return rc;
        if (p.pad_out) hipLaunchKernelGGL(k_bm25_pad_out, dim3(pad_grid, g), dim3(kBmThreads), 0, st, a, p.pad_from);
        const long long span = f.desc ? bm25m_group_pad_span(f.host_desc, q0, g, k) : 0;   // a filter per query: the group's longest padding
        if (span > 0) hipLaunchKernelGGL(k_bm25_pad_out_m, dim3(bm_grid(span, kBmThreads, 64), g), dim3(kBmThreads), 0, st, a, f.desc);
        if (p.small) hipLaunchKernelGGL(k_bm25_sort_small, dim3(1, g), dim3(512), (size_t)Pk * 8, st, a, Pk);
        else rc = bm_sort_deep(h, a);
        if (rc == VF_OK) rc = bm_tail_and_reset(h, a, q_offsets, g, p, f);
        if (rc != VF_OK) return rc;
        VFS_HIP(hipMemcpyAsync(out_ids + (size_t)q0 * k, a.out_ids, (size_t)g * k * 8, hipMemcpyDeviceToHost, st));
        VFS_HIP(hipMemcpyAsync(out_scores + (size_t)q0 * k, a.out_scores, (size_t)g * k * 4, hipMemcpyDeviceToHost, st));
    }
    VFS_HIP(hipStreamSynchronize(st));
    h->qterms_host = nullptr;
    return VF_OK;
}

