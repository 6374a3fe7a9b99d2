// vf_transformer.hip -- encoder forward for the embedding model and the cross-encoder re-ranker,
// hand-written for gfx950 (wave64, v_mfma_f32_32x32x16_f16).  Replaces what the reference delegates to
//   * HuggingFaceEmbeddings.embed_query / embed_documents (src/utils/ragManager.py:50;
//     src/utils/faissRetriever.py:33; src/load_data.py:99,124) -- BERT / XLM-R encoder + pooling
//   * get_embeddings (experiments/retriever/step3_mul.py:191-209, continuous_retrieval.py:127-152)
//   * the re-ranker's compute_score (src/utils/vllmManager.py:450-452), encoder-style cross-encoder
//     (XLM-R + RobertaClassificationHead: BASELINE.json configs[3], [4])
//
// Post-LN BERT-family layer, inference only:
//   x   = LN(word[ids] + pos[p] + type[tt])
//   qkv = x Wqkv^T + b ;  ctx = softmax(q k^T / sqrt(dh) + mask) v
//   x   = LN(ctx Wo^T + b + x) ;  x = LN(gelu(x W1^T + b) W2^T + b + x)
// fp16 weights and activations, fp32 accumulation (MFMA), fp32 LayerNorm / softmax / GELU / pooling.
//
// Kernels
//   k_embed_ln        gather three embeddings, add, LayerNorm (half a wave per row, 16-byte chunks)
//   k_gemm_dma16_tn<E> C = A[M,K] W[N,K]^T + bias (+GELU | +residual): 128x256x32 tiles, LDS-DMA ring, TWO workgroups
//                     per CU, 16x16x32 MFMAs -- the large-problem kernel (100 pairs x 512 tokens);
//                     k_gemm_dma_tn<E> is the same with 32x32x16 MFMAs (selectable)
//   k_gemm_tn<E>      128x128x64 tiles, register-staged LDS double buffer -- everything smaller
//   k_gemm_splitk<E>  64x64 tiles split over K with a deterministic slab reduction -- a single short query's FFN-down
//   k_gemm256_tn<E>   256x256x64 tiles, one workgroup per CU -- kept selectable for experiments (VF_GEMM_KIND=2)
//   k_attention       fused q k^T -> online softmax -> p v per (sequence, head); K and V^T in LDS
//   k_layernorm       row LayerNorm (half a wave per row)
//   k_pool            CLS / mean / last-token pooling (+ L2 normalise)  or  RoBERTa classification head
#include "../../include/veritasfi_hip.h"
#include "vf_internal.h"
#include "vf_gemm_route.h"   // tile geometry, the EPI_* codes the route reads, route_gemm and the small decisions beside it

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <utility>
#include <atomic>
#include <vector>

namespace vft {

typedef _Float16 half_t;
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));

static int fail(int code, const std::string& msg) { return vf::set_error(code, msg); }

#define VFT_HIP(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return fail(VF_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e) + " (vf_transformer.hip:" + \
                                     std::to_string(__LINE__) + ")");                                     \
    } while (0)

#define VFT_TRY(expr)               \
    do {                            \
        int _rc = (expr);           \
        if (_rc != VF_OK) return _rc; \
    } while (0)

// ------------------------------------------------------------------------------------------------
// wave helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------------------------------------
// position ids: BERT 0..t-1; RoBERTa cumsum(mask) * mask + pad_idx  (pos_offset = pad_idx = 1)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_position_ids(const int* mask, int B, int T, int roberta_pad, int* pos) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int run = 0;
    for (int t0 = 0; t0 < T; t0 += 64) {
        const int t = t0 + lane;
        const int m = t < T ? (mask[b * T + t] != 0) : 0;
        int inc = m;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        if (t < T) pos[b * T + t] = roberta_pad >= 0 ? (m ? run + inc + roberta_pad : roberta_pad) : t;
        run += __shfl(inc, 63);
    }
}

// ------------------------------------------------------------------------------------------------
// Row kernels (embeddings + LayerNorm, LayerNorm): HALF a wave per row, 8 rows per 256-thread workgroup.  A row is
// moved as 16-byte chunks of 8 halves; lane l of the half takes chunks l, l + 32, ... (H <= 1024: at most 4), so a
// load instruction of the half-wave covers 512 contiguous bytes.  fp32 statistics, two passes over registers;
// reductions stay inside the 32-lane half (xor offsets < 32).  H % 8 == 0.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float half_wave_sum(float v) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ void ln_finish(float (&v)[4][8], float s, int l32, int nch, int H, const float* g, const float* bta,
                                          float eps, half_t* dst_row) {
    const float mean = half_wave_sum(s) / H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (l32 + 32 * i < nch) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[i][e] - mean; q += d * d; }
        }
    const float rstd = rsqrtf(half_wave_sum(q) / H + eps);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = l32 + 32 * i;
        if (c < nch) {
            const float4 g0 = *(const float4*)(g + c * 8), g1 = *(const float4*)(g + c * 8 + 4);
            const float4 b0 = *(const float4*)(bta + c * 8), b1 = *(const float4*)(bta + c * 8 + 4);
            const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
            const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
            h8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)((v[i][e] - mean) * rstd * gg[e] + bb[e]);
            *(h8*)(dst_row + c * 8) = o;
        }
    }
}

__global__ __launch_bounds__(256) void k_embed_ln(const int* ids, const int* pos, const int* tts, const half_t* word,
                                                   const half_t* posw, const half_t* typew, const float* g,
                                                   const float* bta, float eps, int M, int H, half_t* out) {
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), l32 = threadIdx.x & 31;
    if (row >= M) return;
    const h8* w = (const h8*)(word + (long long)ids[row] * H);
    const h8* p = (const h8*)(posw + (long long)pos[row] * H);
    const h8* t = (const h8*)(typew + (long long)(tts ? tts[row] : 0) * H);
    const int nch = H >> 3;
    float v[4][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = l32 + 32 * i;
        if (c < nch) {
            const h8 a = w[c], b = p[c], d = t[c];
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[i][e] = (float)a[e] + (float)b[e] + (float)d[e]; s += v[i][e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
        }
    }
    ln_finish(v, s, l32, nch, H, g, bta, eps, out + (long long)row * H);
}

// row LayerNorm of y -> x
__global__ __launch_bounds__(256) void k_layernorm(const half_t* y, const float* g, const float* bta, float eps, int M,
                                                    int H, half_t* x) {
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), l32 = threadIdx.x & 31;
    if (row >= M) return;
    const h8* src = (const h8*)(y + (long long)row * H);
    const int nch = H >> 3;
    float v[4][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = l32 + 32 * i;
        if (c < nch) {
            const h8 a = src[c];
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[i][e] = (float)a[e]; s += v[i][e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[i][e] = 0.f;
        }
    }
    ln_finish(v, s, l32, nch, H, g, bta, eps, x + (long long)row * H);
}

// ------------------------------------------------------------------------------------------------
// GEMM  C[M,N] = A[M,K] * W[N,K]^T + bias (+ epilogue).  Both operands K-contiguous ("TN"), which is
// how nn.Linear stores W.  128x128 tile per 256-thread workgroup (4 waves as 2x2, 64x64 each = 2x2
// MFMA 32x32 tiles), BK = 64, two LDS buffers, register-staged global->LDS with the next tile's loads
// issued before the MFMAs of the current one and written to the other buffer after them (one barrier
// per K-tile).  LDS rows padded to 144 B: ds_read_b128 fragment reads are conflict-free.
// Requires M % 128 == 0 (buffers are padded), N % 128 == 0, K % 64 == 0.
// ------------------------------------------------------------------------------------------------
// EPI_RESIDUAL_F32: C and R are FP32 buffers, C = R + acc (+ bias): the decoder family's residual stream is kept in fp32 (the
// reference runs those models in the checkpoint's wider dtype: experiments/retriever/step3_mul.py:62-64), only the
// GEMM operands are fp16.
// EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_RESIDUAL = 2, EPI_RESIDUAL_F32 = 3 and EPI_BIAS_QGELU = 11 (C = quick_gelu(A.W^T + b): x sigmoid(1.702 x), the
// vision tower's activation (CLIP)) are the codes gemm()'s route reads: vf_gemm_route.h.  The codes of the kernels' other epilogues:
enum { EPI_GATED_SILU = 4, EPI_GATED_GELU = 5,   // k_gemm8p_tn only: C[M][N/2] = act(A.Wgate^T) * (A.Wup^T), W = [gate rows | up rows]
       /* 6: was the LayerNorm-in-the-tail experiment (deleted in round 4) */
       // LayerNorm folded into the products around it (k_gemm8p_tn only; LnFold, DESIGN.md 7 "LayerNorm without a launch"):
       EPI_LNA = 7,            // C = rstd_m (A.W'^T - mean_m colsum(W')_n) + c_n : A is the RAW pre-LayerNorm sum, W' = W diag(gamma)
       EPI_LNA_GELU = 8,       // ... + GELU
       EPI_RES_STATS = 9,      // C = A.W^T + b + R (R already normalised), and the row sums (sum, sum of squares) of C
       EPI_LNRES_STATS = 10 }; // C = A.W^T + b + LayerNorm(R) from the raw R and its row sums, and the row sums of C

// exact-GELU x Phi(x) = max(x, 0) - (|x| / 2) erfc(|x| / sqrt 2), with the complementary error function as
// exp2 of a polynomial:  -log2 erfc(a / sqrt 2) = a (c1 + a (c2 + a (c3 + a (c4 + a c5)))), fitted on [0, 6] with the
// weight of the term it multiplies (tools/fit_gelu.py).  |error| <= 7e-7 over every fp16 input (checked exhaustively
// there; the A&S 7.1.26 form used before: 1.5e-7 x |x| / 2), all terms of one sign up to the small c4 -- no cancellation --
// and the polynomial keeps rising beyond the fitted range, so large |x| needs no clamp (exp2 underflows to 0).
// ONE transcendental (exp2) instead of rcp + exp, 6 FMAs: 45 issue cycles per element against 82 (the epilogue of the
// FFN-up product is VALU-bound: one workgroup per CU, nothing runs under it).
constexpr float kGeluC1 = 1.151000500e+00f, kGeluC2 = 4.595957994e-01f, kGeluC3 = 5.214668810e-02f,
                kGeluC4 = -7.198743522e-03f, kGeluC5 = 4.881057539e-04f;
__device__ __forceinline__ float gelu_erf(float x) {
    const float a = fabsf(x);
    float h = __builtin_fmaf(kGeluC5, a, kGeluC4);
    h = __builtin_fmaf(h, a, kGeluC3);
    h = __builtin_fmaf(h, a, kGeluC2);
    h = __builtin_fmaf(h, a, kGeluC1);
    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(-a, h, -1.0f));     // erfc(a / sqrt 2) / 2
    return __builtin_fmaf(-a, e, fmaxf(x, 0.0f));
}
// tanh-GELU (gemma's gelu_pytorch_tanh: x sigmoid(2 * 0.79788456 (x + 0.044715 x^3))) in the same form:
// log2(1 + exp(2 u(a))) - 1 = a h(a), degree 5, |error| <= 5.4e-6 over every fp16 input (tools/fit_gelu.py --tanh),
// rising beyond the fitted range [0, 5.5]: one exp2 and 6 FMAs instead of the cubic, exp, add, rcp and two multiplies.
constexpr float kGeluT1 = 1.150273800e+00f, kGeluT2 = 4.617776871e-01f, kGeluT3 = 5.021990836e-02f,
                kGeluT4 = -9.723095223e-03f, kGeluT5 = 2.106440719e-03f;
__device__ __forceinline__ float gelu_tanh(float x) {
    const float a = fabsf(x);
    float h = __builtin_fmaf(kGeluT5, a, kGeluT4);
    h = __builtin_fmaf(h, a, kGeluT3);
    h = __builtin_fmaf(h, a, kGeluT2);
    h = __builtin_fmaf(h, a, kGeluT1);
    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(-a, h, -1.0f));     // sigmoid(-2 u(a))
    return __builtin_fmaf(-a, e, fmaxf(x, 0.0f));
}
// The same arithmetic on TWO values at once: the multiplies / FMAs are written on 2-vectors so that they issue as
// v_pk_mul_f32 / v_pk_fma_f32 (one slot for two lanes' worth of work); exp2, |x| and max stay scalar.
typedef float f2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2v gelu_erf2(f2v x) {
    const f2v a = {fabsf(x[0]), fabsf(x[1])};
    f2v h = a * kGeluC5 + kGeluC4;
    h = h * a + kGeluC3;
    h = h * a + kGeluC2;
    h = h * a + kGeluC1;
    const f2v s = -(a * h) - 1.0f;
    const f2v e = {__builtin_amdgcn_exp2f(s[0]), __builtin_amdgcn_exp2f(s[1])};
    const f2v relu = {fmaxf(x[0], 0.0f), fmaxf(x[1], 0.0f)};
    return relu - a * e;
}
// quick-GELU x sigmoid(1.702 x) = max(x, 0) - |x| sigmoid(-1.702 |x|): the same shape as the forms above (no cancellation,
// large |x| needs no clamp: exp2 overflows to +inf, its reciprocal is 0)
constexpr float kQGelu = 1.702f * 1.4426950408889634f;
__device__ __forceinline__ float quick_gelu(float x) {
    const float a = fabsf(x);
    const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kQGelu * a));
    return __builtin_fmaf(-a, s, fmaxf(x, 0.0f));
}
__device__ __forceinline__ f2v quick_gelu2(f2v x) { return f2v{quick_gelu(x[0]), quick_gelu(x[1])}; }
constexpr int GBK = 64, GLD = GBK + 8;

template <int EPI>
__global__ __launch_bounds__(256) void k_gemm_tn(const half_t* __restrict__ A, const half_t* __restrict__ W,
                                                  const float* __restrict__ bias, const half_t* __restrict__ R,
                                                  half_t* __restrict__ C, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* As = (half_t*)smem;              // [2][GBM][GLD]
    half_t* Ws = As + 2 * GBM * GLD;         // [2][GBN][GLD]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r31 = lane & 31, h = lane >> 5, wr = wid >> 1, wc = wid & 1;
    // Tile order (speed only): blocks are dealt round-robin over the 8 XCDs, each with a private 4 MB L2.
    // Give every XCD a CONTIGUOUS run of the tile sequence (bijective remap), and order that sequence in
    // groups of 8 m-tiles x all n-tiles, n-major inside a group: the 64 workgroups an XCD runs at once then
    // share 8 A row-panels and 8 W row-panels (~3 MB at K=768), so operands are fetched into L2 once.
    int mt_idx, nt_idx;
    {
        const int Mt = M / GBM, Nt = N / GBN, nwg = Mt * Nt;
        const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
        const int p = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
        constexpr int GM = 8;
        const int g = p / (GM * Nt), r = p - g * (GM * Nt);
        const int gm = (Mt - g * GM) < GM ? (Mt - g * GM) : GM;
        nt_idx = r / gm;
        mt_idx = g * GM + (r - nt_idx * gm);
    }
    const long long m0 = (long long)mt_idx * GBM, n0 = (long long)nt_idx * GBN;
    // register staging of the next K-tile: thread t moves chunks t, t+256, t+512, t+768 (16 B each;
    // chunk c = row c>>3, k-chunk c&7) of both operands.  Plain named registers + macros: arrays captured
    // by a lambda are not promoted to registers by hipcc and end up in scratch.
    const int srow = tid >> 3, skc = tid & 7;
    const half_t* Ag = A + (m0 + srow) * K + skc * 8;
    const half_t* Wg = W + (n0 + srow) * K + skc * 8;
    half_t* Asw = As + srow * GLD + skc * 8;
    half_t* Wsw = Ws + srow * GLD + skc * 8;
    uint4 ra0, ra1, ra2, ra3, rw0, rw1, rw2, rw3;
#define VFT_GLOAD(KT)                                                          \
    {                                                                          \
        const long long ko = (long long)(KT) * GBK;                            \
        ra0 = *(const uint4*)(Ag + ko);                                        \
        ra1 = *(const uint4*)(Ag + ko + 32LL * K);                             \
        ra2 = *(const uint4*)(Ag + ko + 64LL * K);                             \
        ra3 = *(const uint4*)(Ag + ko + 96LL * K);                             \
        rw0 = *(const uint4*)(Wg + ko);                                        \
        rw1 = *(const uint4*)(Wg + ko + 32LL * K);                             \
        rw2 = *(const uint4*)(Wg + ko + 64LL * K);                             \
        rw3 = *(const uint4*)(Wg + ko + 96LL * K);                             \
    }
#define VFT_LSTORE(BUF)                                                        \
    {                                                                          \
        half_t* a_ = Asw + (BUF) * GBM * GLD;                                  \
        half_t* w_ = Wsw + (BUF) * GBN * GLD;                                  \
        *(uint4*)(a_) = ra0;                                                   \
        *(uint4*)(a_ + 32 * GLD) = ra1;                                        \
        *(uint4*)(a_ + 64 * GLD) = ra2;                                        \
        *(uint4*)(a_ + 96 * GLD) = ra3;                                        \
        *(uint4*)(w_) = rw0;                                                   \
        *(uint4*)(w_ + 32 * GLD) = rw1;                                        \
        *(uint4*)(w_ + 64 * GLD) = rw2;                                        \
        *(uint4*)(w_ + 96 * GLD) = rw3;                                        \
    }
    f16v acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    const int nk = K / GBK;
    VFT_GLOAD(0)
    VFT_LSTORE(0)
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        const int ktn = kt + 1 < nk ? kt + 1 : kt;  // unconditional (clamped) prefetch
        VFT_GLOAD(ktn)
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ABOVE the MFMAs (the scheduler sinks it otherwise)
        const half_t* a_base = As + (buf * GBM + wr * 64 + r31) * GLD + h * 8;
        const half_t* w_base = Ws + (buf * GBN + wc * 64 + r31) * GLD + h * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            h8 af[2], wf[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                af[t] = *(const h8*)(a_base + t * 32 * GLD + ks * 16);
                wf[t] = *(const h8*)(w_base + t * 32 * GLD + ks * 16);
            }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[mt], wf[nt], acc[mt][nt], 0, 0, 0);
        }
        VFT_LSTORE(buf ^ 1)
        __syncthreads();
    }
#undef VFT_GLOAD
#undef VFT_LSTORE
    // epilogue: acc[mt][nt][reg] -> row m0 + wr*64 + mt*32 + (reg&3) + 8*(reg>>2) + 4*h, col n0 + wc*64 + nt*32 + r31
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const long long n = n0 + wc * 64 + nt * 32 + r31;
        const float bv = bias ? bias[n] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const long long m = m0 + wr * 64 + mt * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                float v = acc[mt][nt][reg] + bv;
                if (EPI == EPI_BIAS_GELU) v = gelu_erf(v);
                if (EPI == EPI_BIAS_QGELU) v = quick_gelu(v);
                if (EPI == EPI_BIAS_RESIDUAL) v += (float)R[m * N + n];
                if (EPI == EPI_RESIDUAL_F32) ((float*)C)[m * N + n] = v + ((const float*)R)[m * N + n];
                else C[m * N + n] = (half_t)v;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// k_gemm_splitk: the same product for FEW rows and LONG K (a single short query's FFN-down: M <= 64, K = ffn).  At that size
// the tiled kernels launch a dozen workgroups that each walk the whole K serially (26 us for K = 3072) while 240
// CUs idle; here a 64 x 64 output tile is computed by S workgroups, each over K / S, so the weight matrix
// streams through the whole chip.  Deterministic: every split writes its fp32 partial tile to its own slab
// part[s][M][N]; the workgroup that arrives LAST at the tile's counter sums the slabs in split order, applies
// the epilogue and resets the counter (slabs cross XCDs, whose L2s are not coherent: see the hand-off below).
// 256 threads = 4 waves, one 32 x 32 MFMA tile each; BK = 64, two register-staged LDS buffers.
// Requires M % 64 == 0, N % 64 == 0, (K / S) % 64 == 0.
// ------------------------------------------------------------------------------------------------
constexpr int SLD = SBK + 8;

template <int EPI>
__global__ __launch_bounds__(256) void k_gemm_splitk(const half_t* __restrict__ A, const half_t* __restrict__ W,
                                                      const float* __restrict__ bias, const half_t* __restrict__ R,
                                                      half_t* __restrict__ C, int M, int N, int K, int S,
                                                      float* __restrict__ part, unsigned* __restrict__ counters) {
    __shared__ __attribute__((aligned(16))) half_t As[2][SBM][SLD];
    __shared__ __attribute__((aligned(16))) half_t Ws[2][SBN][SLD];
    __shared__ unsigned s_old;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r31 = lane & 31, h = lane >> 5, wr = wid >> 1, wc = wid & 1;
    const int Nt = N / SBN;
    const int sp = blockIdx.x % S, t = blockIdx.x / S, nt = t % Nt, mt = t / Nt;
    const long long m0 = (long long)mt * SBM, n0 = (long long)nt * SBN;
    const int klen = K / S, k0 = sp * klen, nk = klen / SBK;
    // a K-tile of A / W is 64 rows x 128 B = 512 chunks of 16 B: two per thread (rows c >> 3, chunk c & 7)
    const int row0 = tid >> 3, kc = tid & 7;
    const half_t* ap = A + (m0 + row0) * K + k0 + kc * 8;
    const half_t* wp = W + (n0 + row0) * K + k0 + kc * 8;
    h8 ra[2], rw[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ra[j] = *(const h8*)(ap + (long long)(32 * j) * K);
        rw[j] = *(const h8*)(wp + (long long)(32 * j) * K);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        *(h8*)(&As[0][row0 + 32 * j][kc * 8]) = ra[j];
        *(h8*)(&Ws[0][row0 + 32 * j][kc * 8]) = rw[j];
    }
    __syncthreads();
    f16v acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                ra[j] = *(const h8*)(ap + (long long)(32 * j) * K + (kt + 1) * SBK);
                rw[j] = *(const h8*)(wp + (long long)(32 * j) * K + (kt + 1) * SBK);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const h8 af = *(const h8*)(&As[cur][wr * 32 + r31][ks * 16 + h * 8]);
            const h8 wf = *(const h8*)(&Ws[cur][wc * 32 + r31][ks * 16 + h * 8]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, wf, acc, 0, 0, 0);
        }
        if (kt + 1 < nk) {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                *(h8*)(&As[cur ^ 1][row0 + 32 * j][kc * 8]) = ra[j];
                *(h8*)(&Ws[cur ^ 1][row0 + 32 * j][kc * 8]) = rw[j];
            }
        }
        __syncthreads();
    }
    // this split's partial tile -> its slab
    float* slab = part + ((long long)sp * M + m0) * N + n0;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        // agent-scope store: written through the (per-XCD, mutually non-coherent) L2 to memory
        __hip_atomic_store(slab + (long long)row * N + wc * 32 + r31, acc[reg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // The slab must have reached memory before the arrival is counted.  A full release fence would write back AND
    // (on the acquire side) invalidate the whole L2 per workgroup -- measured 2-3x slower than no split at all, it
    // evicts the weights; the partials alone bypass L2 instead (agent-scope stores above, agent-scope loads below),
    // and all this needs is that the stores have completed: vmcnt(0), then the barrier, then the counter.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_old = __hip_atomic_fetch_add(counters + t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_old != (unsigned)(S - 1)) return;  // not the last split of this tile
    // the last arrival reduces in split order (deterministic) and applies the epilogue: thread -> row tid >> 2,
    // 16 consecutive columns
    const int row = tid >> 2, c0 = (tid & 3) * 16;
    float v[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.f;
    for (int s2 = 0; s2 < S; ++s2) {
        const float* src = part + ((long long)s2 * M + m0 + row) * N + n0 + c0;
        float x[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) x[e] = __hip_atomic_load(src + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] += x[e];
    }
    const long long off = (m0 + row) * N + n0 + c0;
    h8 o[2];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        float x = v[e] + (bias ? bias[n0 + c0 + e] : 0.f);
        if (EPI == EPI_BIAS_GELU) x = gelu_erf(x);
        if (EPI == EPI_BIAS_QGELU) x = quick_gelu(x);
        o[e >> 3][e & 7] = (half_t)x;
    }
    if (EPI == EPI_BIAS_RESIDUAL) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const h8 r = *(const h8*)(R + off + 8 * q);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[q][e] = (half_t)((float)o[q][e] + (float)r[e]);
        }
    }
    *(h8*)(C + off) = o[0];
    *(h8*)(C + off + 8) = o[1];
    if (tid == 0) __hip_atomic_store(counters + t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
}

// ------------------------------------------------------------------------------------------------
// k_gemm_dma16_tn: 128 (M) x 256 (N) tile, 4 waves (2 x 2, wave tile 64 x 128 = 2 x 4 MFMA tiles), BK = 32,
// THREE 24 KB LDS slots filled by LDS-DMA (72 KB per workgroup), so that TWO workgroups share a CU.
// The two are independent: one's barrier bubbles, DMA tail and whole epilogue (the output's HBM write) run
// under the other's MFMAs -- the overlap a single lock-stepped 128 KB workgroup per CU cannot have.
// Iteration t: issue the DMA of stage t+1 into slot (t+1) % 3 (last read in iteration t-2, which every wave
// finished before the barrier of iteration t-1), wait with a COUNTED vmcnt(6) (this wave's 6 DMA instructions
// of stage t+1 stay in flight), one raw s_barrier, 16 MFMAs per wave on slot t % 3.
// LDS rows are 64 B (4 chunks of 16 B); chunk c of row r sits at physical chunk c ^ ((r >> 2) & 3): the DMA
// lanes fetch the matching logical chunk, and a ds_read_b128 lane group (16 rows) touches 16 distinct slots.
// ------------------------------------------------------------------------------------------------
constexpr int DTHREADS = 256, DSLOT = 24576, DLDS = 3 * DSLOT;

// The kernel described above, with 16x16x32 MFMAs (the guide measures that MFMA shape at 1.12-1.15x the FLOP/s of 32x32x16 with
// operands from LDS; the 32x32x16 form of round 1 measured 4-6 % slower and is gone).  Lane (r = lane & 15, kb = lane >> 4) reads rows r of a 16-row tile at k-block kb, so the chunk
// swizzle is re-derived for that map: physical chunk = c ^ f(row), f = {0, 3, 2, 1}[(row >> 2) & 3], which gives every
// ds_read_b128 lane group ({0-3, 12-15, 20-27} ...) 16 distinct 16-byte slots.
__device__ __forceinline__ int swz16(int row) { return (0x6C >> (2 * ((row >> 2) & 3))) & 3; }   // 0b01'10'11'00 -> 0, 3, 2, 1

template <int EPI, int BN>
__global__ __launch_bounds__(DTHREADS, 2) void k_gemm_dma16_tn(const half_t* __restrict__ A, const half_t* __restrict__ W,
                                                          const float* __restrict__ bias, const half_t* __restrict__ R,
                                                          half_t* __restrict__ C, int M, int N, int K) {
    extern __shared__ __attribute__((aligned(16))) char smem[];  // 3 slots x [A 128x32 | W BNx32] fp16
    constexpr int NTW = BN / 32;            // 16-column MFMA tiles per wave (wave tile 64 x BN/2): 8 or 4
    constexpr int WJ = BN / 64;             // W-tile DMA instructions per wave per stage: 4 or 2
    constexpr int SLOT = (DBM + BN) * 64;   // bytes per LDS slot: 24 KB or 16 KB
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r15 = lane & 15, kb = lane >> 4, wr = wid >> 1, wc = wid & 1;   // MFMA 16x16x32: row / col lane & 15, k-block lane >> 4
    int mt_idx, nt_idx;
    {   // XCD-contiguous, n-major groups of 8 m-tiles (64 workgroups resident per XCD)
        const int Mt = M / DBM, Nt = N / BN, nwg = Mt * Nt;
        const int orig = blockIdx.x, xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
        const int p = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
        constexpr int GM = 8;
        const int g = p / (GM * Nt), r = p - g * (GM * Nt);
        const int gm = (Mt - g * GM) < GM ? (Mt - g * GM) : GM;
        nt_idx = r / gm;
        mt_idx = g * GM + (r - nt_idx * gm);
    }
    const long long m0 = (long long)mt_idx * DBM, n0 = (long long)nt_idx * BN;
    // one DMA instruction fills 16 rows x 64 B; the A tile is 8 of them (wave w: rows [32w, 32w+32)), the W tile 16
    // (wave w: rows [64w, 64w+64)).  lane l -> row l >> 2 of the 16, physical chunk l & 3.
    const half_t* a_src[2];
    const half_t* w_src[WJ];
    const int drow = lane >> 2, dpc = lane & 3;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int row = wid * 32 + j * 16 + drow;
        a_src[j] = A + (m0 + row) * K + (dpc ^ swz16(row)) * 8;
    }
#pragma unroll
    for (int j = 0; j < WJ; ++j) {
        const int row = wid * (BN / 4) + j * 16 + drow;
        w_src[j] = W + (n0 + row) * K + (dpc ^ swz16(row)) * 8;
    }
    auto stage = [&](int slot, int kt) {
        char* abase = smem + slot * SLOT + (wid * 32) * 64;
        char* wbase = smem + slot * SLOT + 8192 + (wid * (BN / 4)) * 64;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a_src[j] + (long long)kt * DBK),
                                             (__attribute__((address_space(3))) void*)(abase + j * 1024), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < WJ; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(w_src[j] + (long long)kt * DBK),
                                             (__attribute__((address_space(3))) void*)(wbase + j * 1024), 16, 0, 0);
    };
    f4v acc[4][NTW];   // wave tile 64 x BN/2 = 4 x NTW MFMA tiles of 16 x 16
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NTW; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[a][b][e] = 0.f;
    const int pc = (kb ^ swz16(r15)) * 16;  // tile offsets are multiples of 16 rows: they do not change (row >> 2) & 3
    const char* a_row = smem + (wr * 64 + r15) * 64 + pc;
    const char* w_row = smem + 8192 + (wc * (BN / 2) + r15) * 64 + pc;
    const int nk = K / DBK;
    stage(0, 0);
    int slot = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const int nslot = slot == 2 ? 0 : slot + 1;
        stage(nslot, kt + 1 < nk ? kt + 1 : nk - 1);            // past the end: re-reads the last tile (unused)
        if (BN == 256) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");  // stage kt landed (this wave's DMA: 2 + WJ stay in flight)
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        __builtin_amdgcn_s_barrier();                           // ... and every wave's
        const char* ab = a_row + slot * SLOT;
        const char* wb = w_row + slot * SLOT;
        {   // BK = 32 is ONE k-step of the 16x16x32 MFMA: 4 + NTW fragment reads, 4 * NTW MFMAs
            h8 af[4], wf[NTW];
#pragma unroll
            for (int t = 0; t < 4; ++t) af[t] = *(const h8*)(ab + t * 16 * 64);
#pragma unroll
            for (int t = 0; t < NTW; ++t) wf[t] = *(const h8*)(wb + t * 16 * 64);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], wf[nt], acc[mt][nt], 0, 0, 0);
        }
        slot = nslot;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // retire the trailing dummy stage before LDS is reused
    __syncthreads();
    if constexpr (EPI == EPI_RESIDUAL_F32) {
        // fp32 residual stream: straight from the accumulators (16 lanes cover 64 contiguous bytes of a row; an fp32
        // image of the tile would not fit the three operand slots)
        const float* R32 = (const float*)R;
        float* C32 = (float*)C;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
            const long long col = n0 + wc * (BN / 2) + nt * 16 + r15;
            const float bv = bias ? bias[col] : 0.f;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const long long off = (m0 + wr * 64 + mt * 16 + 4 * kb + reg) * N + col;
                    C32[off] = acc[mt][nt][reg] + bv + R32[off];
                }
        }
        return;
    }
    // epilogue through LDS: fp16(acc + bias [+GELU]) into a [128][BN] fp16 image (inside the three slots), then 16-byte
    // row chunks out (residual added in fp32 on the vector side)
    half_t* Es = (half_t*)smem;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int col = wc * (BN / 2) + nt * 16 + r15;
        const float bv = bias ? bias[n0 + col] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = wr * 64 + mt * 16 + 4 * kb + reg;
                float v = acc[mt][nt][reg] + bv;
                if (EPI == EPI_BIAS_GELU) v = gelu_erf(v);
                if (EPI == EPI_BIAS_QGELU) v = quick_gelu(v);
                Es[row * BN + col] = (half_t)v;
            }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < BN / 16; ++i) {
        const int c = tid + DTHREADS * i, row = c / (BN / 8), cc = c % (BN / 8);  // BN / 8 chunks of 8 halves per row
        h8 o = *(const h8*)(Es + row * BN + cc * 8);
        const long long off = (m0 + row) * N + n0 + cc * 8;
        if (EPI == EPI_BIAS_RESIDUAL) {
            const h8 r = *(const h8*)(R + off);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)o[e] + (float)r[e]);
        }
        *(h8*)(C + off) = o;
    }
}

// ------------------------------------------------------------------------------------------------
// k_gemm_skinny: C[M <= 64, N] = A[., K] . W[N, K]^T + bias (+ epilogue) for ONE short sequence (a query string:
// src/utils/faissRetriever.py:33 embeds one per request).  Such a product is a weight stream: a workgroup owns 16 output
// columns (N / 16 workgroups: 48 .. 192), its eight waves split K into eighths and stream their slice of W straight
// into MFMA 16x16x32 B operands (16 rows x 64 contiguous bytes per instruction), the activations (L2-resident) into A
// operands (a batch of 6 k-steps in flight); the fp32 partial tiles meet in LDS, the epilogue writes M x 16 halves.  No split-K hand-off between
// workgroups, no padding rows computed beyond the next multiple of 16.  Requires N % 16 == 0, K % 256 == 0; A has at
// least 64 rows (the workspace is padded and zero-filled).
// ------------------------------------------------------------------------------------------------
constexpr int kSkinnyWaves = 8, kSkinnyBatch = 6;

// S > 1 (long K, few column tiles: the N = hidden products with K = ffn): S workgroups share a column tile, each taking
// K / S; their fp32 partial tiles meet in `part` ([S][64][N], agent-scope stores and loads: the XCDs' L2s are not coherent
// with each other) and the last to arrive (counters[tile]) sums them in split order and runs the epilogue -- the protocol
// of k_gemm_splitk.  With 48 workgroups each streaming all of A (M x 3072) the product took 15-26 us; with 192 it is one
// memory round trip per wave.
template <int EPI, int MT>
__global__ __launch_bounds__(kSkinnyWaves * 64) void k_gemm_skinny(const half_t* __restrict__ A, const half_t* __restrict__ W,
                                                                   const float* __restrict__ bias, const half_t* __restrict__ R,
                                                                   half_t* __restrict__ C, int M, int N, int K, int S,
                                                                   float* __restrict__ part, unsigned* __restrict__ counters) {
    __shared__ float red[kSkinnyWaves][MT * 16][17];
    __shared__ unsigned s_old;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r15 = lane & 15, kb = lane >> 4;
    const int tile = blockIdx.x / S, sp = blockIdx.x - tile * S;
    const int n0 = tile * 16;
    const int Ks = K / S;                                     // this workgroup's K range: [sp Ks, (sp + 1) Ks)
    const int steps = Ks >> 5, per = steps / kSkinnyWaves;   // k-steps of 32; per wave (Ks % 256 == 0)
    const half_t* wp = W + (long long)(n0 + r15) * K + kb * 8 + (long long)sp * Ks + (long long)wid * per * 32;
    const half_t* ap = A + (long long)r15 * K + kb * 8 + (long long)sp * Ks + (long long)wid * per * 32;
    f4v acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.f;
    // the epilogue's residual (thread -> row tid >> 2, columns 4 (tid & 3) .. + 3) is fetched before the weight stream starts:
    // loaded after the reduction it costs one more dependent memory round trip per product (10.7 vs 7.5 us measured)
    h4 rpre = {(half_t)0.f, (half_t)0.f, (half_t)0.f, (half_t)0.f};
    if (EPI == EPI_BIAS_RESIDUAL) {
        const int row = tid >> 2, c0 = (tid & 3) * 4;
        if (row < M && row < MT * 16) rpre = *(const h4*)(R + (long long)row * N + n0 + c0);
    }
    for (int s0 = 0; s0 < per; s0 += kSkinnyBatch) {
        h8 bf[kSkinnyBatch], af[kSkinnyBatch][MT];
#pragma unroll
        for (int u = 0; u < kSkinnyBatch; ++u) {        // all loads of the batch in flight at once; the tail is clamped
            const int s = s0 + u < per ? s0 + u : per - 1;
            bf[u] = *(const h8*)(wp + s * 32);
#pragma unroll
            for (int t = 0; t < MT; ++t) af[u][t] = *(const h8*)(ap + (long long)t * 16 * K + s * 32);
        }
#pragma unroll
        for (int u = 0; u < kSkinnyBatch; ++u) {
            if (s0 + u < per) {
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u][t], bf[u], acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) red[wid][t * 16 + 4 * kb + reg][r15] = acc[t][reg];
    __syncthreads();
    // thread -> row tid >> 2, columns 4 (tid & 3) .. + 3   (the first 4 * 16 MT threads have a row)
    const int row = tid >> 2, c0 = (tid & 3) * 4;
    const bool has_row = row < M && row < MT * 16;
    float sum[4] = {0.f, 0.f, 0.f, 0.f};
    if (has_row) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int w = 0; w < kSkinnyWaves; ++w) sum[e] += red[w][row][c0 + e];
    }
    if (S > 1) {
        if (has_row) {
            float* slab = part + ((long long)sp * 64 + row) * N + n0 + c0;
#pragma unroll
            for (int e = 0; e < 4; ++e) __hip_atomic_store(slab + e, sum[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the slab has reached memory before the arrival is counted
        __syncthreads();
        if (tid == 0) s_old = __hip_atomic_fetch_add(counters + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (s_old != (unsigned)(S - 1)) return;             // not the last split of this column tile
        if (has_row) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sum[e] = 0.f;
            for (int s2 = 0; s2 < S; ++s2) {                // split order: deterministic
                const float* src = part + ((long long)s2 * 64 + row) * N + n0 + c0;
#pragma unroll
                for (int e = 0; e < 4; ++e) sum[e] += __hip_atomic_load(src + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (tid == 0) __hip_atomic_store(counters + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
    if (has_row) {
        h4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v = sum[e];
            v += bias ? bias[n0 + c0 + e] : 0.f;
            if (EPI == EPI_BIAS_GELU) v = gelu_erf(v);
                if (EPI == EPI_BIAS_QGELU) v = quick_gelu(v);
            if (EPI == EPI_BIAS_RESIDUAL) v += (float)rpre[e];
            o[e] = (half_t)v;
        }
        *(h4*)(C + (long long)row * N + n0 + c0) = o;
    }
}

// ------------------------------------------------------------------------------------------------
// Buffer-resource accesses with explicit cache policy (the hand-over forms of MI355X_MICROARCH.md): 16- / 8-byte loads and
// stores with sc1 (memory side), used by the split-K tail of the 8-phase products.  (The persistent all-layers one-query
// forward these were written for -- k_sq_forward, rounds 2-3: correct, 20-40 % slower than a launch per product -- is gone;
// its measurements stay in DESIGN.md section 7.)
// ------------------------------------------------------------------------------------------------
typedef int i4v __attribute__((ext_vector_type(4)));
typedef int i2v __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t sq_rsrc_t;
__device__ __forceinline__ sq_rsrc_t sq_rsrc(const void* q) { return __builtin_amdgcn_make_buffer_rsrc((void*)q, 0, 0x7ffffff0, 0x00020000); }
__device__ __forceinline__ h8 sq_ld8(sq_rsrc_t r, int off) { return __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16)); }
__device__ __forceinline__ void sq_st8(sq_rsrc_t r, int off, h8 v) { __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, v), r, off, 0, 16); }

// ------------------------------------------------------------------------------------------------
// LayerNorm folded into the neighbouring products: a residual product (EPI_RES_STATS / EPI_LNRES_STATS) leaves, per 256-column
// tile, the sums (sum y, sum y^2) of every row of its fp16 output y; the consumers read the raw y and the n_parts partial
// sums: the next product as its A operand (EPI_LNA*: the LayerNorm's gamma is folded into the weights, its mean / beta
// terms enter through colsum(W') and c), the next residual product as its residual (normalised element by element).
struct LnFold {
    const float* stats_in;   // [n_parts][Mp][2] partial row sums of the raw operand (A for EPI_LNA*, R for EPI_LNRES_STATS)
    float* stats_out;        // [N / 256][Mp][2] (EPI_*_STATS)
    const float* colsum;     // [N] column sums of the folded weights (EPI_LNA*)
    const float* gR;         // [N] gamma / beta of the LayerNorm applied to R (EPI_LNRES_STATS)
    const float* bR;
    int n_parts;             // hidden / 256
    int Mp;                  // rows of the stats arrays
    float inv_h, eps;        // 1 / hidden
    // Split-K TAIL (independent of the fold; rides in this struct so that every launch site passes one extra argument): the
    // tiles of the partial last round -- dispatch indices >= sk_nfull -- are cut into sk_S slices along K, one workgroup each
    // (600 tiles on 256 CUs are 2.34 rounds of work in 3; with the 88 tail tiles cut in two the third round is 176 half-length
    // workgroups).  Co-operative finish (round 4): a slice leaves the 16-row blocks it does NOT own in sk_ws (write-through), counts
    // itself in sk_cnt[tile], waits for the other slices and adds their partials of ITS blocks IN SLICE ORDER (deterministic), runs
    // the epilogue on its rows; the last slice to finish reading resets the counters.  (Until round 4 the last arrival read all S
    // partials back and finished the whole tile alone: 3 % slower on a 600-tile product, 10 % on a product cut whole.)
    // The slices of one tile sit at dispatch indices that are congruent modulo 8 -- one XCD under the round-robin placement
    // -- and every slice notes the XCD it really ran on (HW_REG_XCC_ID): when they all match the reader's, the partials are
    // still in THAT L2 (the write-through stores went through it) and the read-backs use L1-bypassing loads that hit it;
    // otherwise it falls back to memory-side (sc1) loads.  Placement decides the speed, never the result.
    float* sk_ws;            // [tail tiles][sk_S][256 x 256] fp32
    unsigned* sk_cnt;        // [tail tiles][2]: arrivals, XCD mask; zero between launches
    int sk_nfull, sk_S;      // sk_S == 0: no split
    int sk_ntail;            // tail tiles (the sliced part of the grid is padded to 8 tiles x sk_S: the excess workgroups leave)
    unsigned* sk_stat;       // [4] read-backs through L2 / from memory, (timing experiments: bit 0 of sk_dbg skips the partial stores, bit 1 the read-back)
    int sk_dbg;
    int loop2;               // main loop in TWO phases of 32 MFMAs per K-tile instead of four of 16 (see k_gemm8p_tn)
};

// split-K tail workspace of one handle (see gws_ensure)
struct GemmWs {
    float* ws = nullptr;
    unsigned* cnt = nullptr;     // [kSkMaxTiles][2] arrivals + XCD mask, then 4 statistics words
    size_t bytes = 0;
};

// geometry of the 256 x 256 x 64 kernels (k_gemm8p_tn, k_gemm9_tn): 512 threads, eight 16-KB half-tile slots + a dump slot
constexpr int PTHREADS = 512, PSLOT = 16384, PLDS = 2 * 4 * PSLOT + PSLOT;
// ------------------------------------------------------------------------------------------------
// The co-operative split-K finish, shared by the 8-phase kernel's tail tiles and the persistent kernel's whole-product cut (round 5):
// `acc` holds this slice's partial sums of the tile in the kernel's own register layout (both kernels: acc[mi][ni], 16-row block mi of
// the wave's 128 rows), `flag` is 16 bytes of LDS nobody else is using, every thread of the workgroup calls it behind a barrier with
// no vector-memory access of its own pending.  Returns true when the workgroup has handed its share over and must leave; otherwise
// sk_own names the blocks it has to finish (bias, activation, residual, store).
struct SkCtx { float* ws; unsigned* cnt; unsigned* stat; int S; int dbg; };

__device__ __forceinline__ bool sk_coop_finish(f4v (&acc)[8][4], const SkCtx& sk, int sk_tile, int me, unsigned& sk_own, unsigned* flag, int tid) {
    // Split-K, co-operative finish (round 4).  Until then the LAST slice to arrive read all S partials back (one CU pulls 50-60
    // GB/s: ~9 us per 256 KB) and finished the tile alone.  Now slice s owns the 16-row blocks mi in [8 s / S, 8 (s + 1) / S) of
    // both 128-row halves: it leaves only the blocks it does not own in sk_ws ((S - 1) / S of a partial), counts itself, waits
    // until all S slices have done so, adds the others' partials of ITS blocks in slice order (its own term comes from the
    // registers, at its place in the order: bit for bit the old sum) and runs the epilogue on its rows only.
    // The wait is BOUNDED.  Slices of one launch alone cannot block one another (they are the last workgroups of the grid, at
    // most one round of the CUs, one per CU, and nothing ahead of them waits) -- but two such launches on different streams,
    // or in two processes sharing the GPU, could each hold the CUs the other's missing slices need.  So a slice that has
    // waited kSkWaitTicks (300 us; partners normally arrive within one tile's time) hands ITS blocks over as well, marks
    // itself in the tile's state word and leaves its CU; the slice that arrives LAST sees the marks in the value its own
    // arrival returns and finishes those blocks too.  One 32-bit word per tile orders everything: bits 0-7 arrivals, 8-15
    // "has handed over" per slice, 16-23 finished; a slice whose mark lands after the last arrival learns that from the
    // returned value and carries on itself (the word is then harmlessly marked).  vf_debug_splitk_stats(.., 16) sets the bound
    // to zero: every slice but the last hands over at once -- the old last-arrival scheme, through the take-over code (tests).
    constexpr unsigned long long kSkWaitTicks = 30000ull;   // of the 100 MHz real-time counter
    const sq_rsrc_t rw = sq_rsrc(sk.ws);
    const int S = sk.S;
    const int lo_me = 8 * me / S, hi_me = 8 * (me + 1) / S;
    sk_own = ((1u << hi_me) - 1u) & ~((1u << lo_me) - 1u);
    const int my = ((sk_tile * S + me) * 32) * PTHREADS * 16;   // byte offset: [tile][slice][mi * 4 + ni][thread] x 16 B
    unsigned* const w0 = sk.cnt + 2 * sk_tile;               // the state word; w0[1]: slices per XCD, 3 bits each
    auto finished = [&](bool same_xcd) {   // tid 0: this slice needs nothing from the workspace any more
        const unsigned v = __hip_atomic_fetch_add(w0, 1u << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (((v >> 16) & 0xffu) == (unsigned)(S - 1)) {   // the last to finish leaves the words at zero for the next launch
            __hip_atomic_store(w0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(w0 + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            atomicAdd(sk.stat + (same_xcd ? 0 : 1), 1u);
        }
    };
    // one block (16 rows of either half) summed in slice order: any slice's share, one block at a time (take-over only)
    auto take_block = [&](auto MI, bool) {
        constexpr int mi = decltype(MI)::value;
        f4v t[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) t[ni] = f4v{0.f, 0.f, 0.f, 0.f};
        for (int sl = 0; sl < S; ++sl) {
            if (sl == me) {
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[ni][e] += acc[mi][ni][e];
            } else {
                const int off = ((sk_tile * S + sl) * 32) * PTHREADS * 16;
                f4v v[4];
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    v[ni] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rw, off + ((mi * 4 + ni) * PTHREADS + tid) * 16, 0, 16));
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[ni][e] += v[ni][e];
            }
        }
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = t[ni];
    };
    auto coop = [&](auto LO, auto HI) -> bool {   // true: the share has been handed over, the workgroup leaves
        constexpr int lo = decltype(LO)::value, hi = decltype(HI)::value;
        if (!(sk.dbg & 1)) {
#pragma unroll
            for (int mi = 0; mi < 8; ++mi)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
                    if (mi < lo || mi >= hi)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, acc[mi][ni]), rw, my + ((mi * 4 + ni) * PTHREADS + tid) * 16, 0, 16);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // write-through stores have reached memory ...
        __syncthreads();
        if (tid == 0) {
            unsigned xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            xcc &= 7u;
            (void)__hip_atomic_fetch_add(w0 + 1, 1u << (3 * xcc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // ... before the slice counts.  Round 5: RELAXED, here and in the poll.  An agent-scope release is a buffer_wbl2 (a
            // write-back of this XCD's whole L2), an acquiring poll a buffer_inv per turn -- and neither is needed: the partials are
            // stored sc1 (write-through) and every wave has waited for its stores (above, then the barrier); they are read sc1
            // (past this CU's L1, every load of them), by the polling lane after its poll has matched and by the other waves behind
            // the barrier it then joins -- the hand-off form MI355X_MICROARCH.md lists as valid without fences.  Worth 6-7 us of
            // the FFN-down launch at 6 656 rows (53.7 -> 46-47 us; profiles/r05_splitk_relaxed_arrival_l2_vs_writethrough.log).
            const unsigned a = __hip_atomic_fetch_add(w0, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool last = (a & 0xffu) == (unsigned)(S - 1);
            unsigned give_up = 0u;
            if (!last) {
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime(), bound = (sk.dbg & 16) ? 0ull : kSkWaitTicks;
                for (;;) {
                    if ((__hip_atomic_load(w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 0xffu) >= (unsigned)S) break;
                    if (__builtin_amdgcn_s_memrealtime() - t0 >= bound) { give_up = 1u; break; }
                    __builtin_amdgcn_s_sleep(4);
                }
            }
            flag[0] = give_up;
            flag[2] = last ? ((a >> 8) & 0xffu) : 0u;   // the last arrival: whose blocks are left for it
            flag[3] = xcc;
        }
        __syncthreads();
        if (flag[0]) {   // waited long enough: my own blocks go to the workspace too, then the mark
            if (!(sk.dbg & 1)) {
#pragma unroll
                for (int mi = lo; mi < hi; ++mi)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, acc[mi][ni]), rw, my + ((mi * 4 + ni) * PTHREADS + tid) * 16, 0, 16);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) {
                const unsigned b = __hip_atomic_fetch_or(w0, 1u << (8 + me), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                flag[0] = (b & 0xffu) >= (unsigned)S ? 0u : 1u;   // everybody is here after all: nobody will finish my blocks for me
                if (flag[0]) finished(false);
            }
            __syncthreads();
            if (flag[0]) return true;
        }
        // two blocks at a time (64 more registers beside the 128 accumulators; the whole share at once spilled)
        auto reduce2 = [&](auto B0, auto NB) {
            constexpr int b0 = decltype(B0)::value, nb = decltype(NB)::value;
            f4v t[nb][4];
#pragma unroll
            for (int m = 0; m < nb; ++m)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) t[m][ni] = f4v{0.f, 0.f, 0.f, 0.f};
            auto add_slice = [&](int sl) {
                const int off = ((sk_tile * S + sl) * 32) * PTHREADS * 16;
                f4v v[nb][4];
                // sc1 loads, all of them (sc0 loads may be served by this CU's L1 like plain ones)
#pragma unroll
                for (int m = 0; m < nb; ++m)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni)
                        v[m][ni] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rw, off + (((b0 + m) * 4 + ni) * PTHREADS + tid) * 16, 0, 16));
#pragma unroll
                for (int m = 0; m < nb; ++m)
#pragma unroll
                    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                        for (int e = 0; e < 4; ++e) t[m][ni][e] += v[m][ni][e];
            };
            if (!(sk.dbg & 2))
                for (int sl = 0; sl < me; ++sl) add_slice(sl);
#pragma unroll
            for (int m = 0; m < nb; ++m)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[m][ni][e] += acc[b0 + m][ni][e];
            if (!(sk.dbg & 2))
                for (int sl = me + 1; sl < S; ++sl) add_slice(sl);
#pragma unroll
            for (int m = 0; m < nb; ++m)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[b0 + m][ni] = t[m][ni];
        };
        using std::integral_constant;
        reduce2(integral_constant<int, lo>{}, integral_constant<int, (hi - lo >= 2 ? 2 : 1)>{});
        if constexpr (hi - lo == 3) reduce2(integral_constant<int, lo + 2>{}, integral_constant<int, 1>{});
        if constexpr (hi - lo == 4) reduce2(integral_constant<int, lo + 2>{}, integral_constant<int, 2>{});
        return false;
    };
    using std::integral_constant;
    bool leave = false;
    switch (lo_me * 16 + hi_me) {   // the eight (first block, end) pairs of S = 2, 3, 4
        case 0 * 16 + 4: leave = coop(integral_constant<int, 0>{}, integral_constant<int, 4>{}); break;
        case 4 * 16 + 8: leave = coop(integral_constant<int, 4>{}, integral_constant<int, 8>{}); break;
        case 0 * 16 + 2: leave = coop(integral_constant<int, 0>{}, integral_constant<int, 2>{}); break;
        case 2 * 16 + 5: leave = coop(integral_constant<int, 2>{}, integral_constant<int, 5>{}); break;
        case 5 * 16 + 8: leave = coop(integral_constant<int, 5>{}, integral_constant<int, 8>{}); break;
        case 2 * 16 + 4: leave = coop(integral_constant<int, 2>{}, integral_constant<int, 4>{}); break;
        case 4 * 16 + 6: leave = coop(integral_constant<int, 4>{}, integral_constant<int, 6>{}); break;
        case 6 * 16 + 8: leave = coop(integral_constant<int, 6>{}, integral_constant<int, 8>{}); break;
        default: __builtin_trap();   // the host only launches S in {2, 3, 4}
    }
    if (leave) return true;
    const bool same_xcd = false;   // (take_block's second argument: every read of a partial is an sc1 load wherever its slice ran)
    const unsigned gone = flag[2];
    if (gone) {   // the last arrival finishes the blocks of the slices that have left (their whole partial is in the workspace)
        unsigned take = 0u;
        for (int x = 0; x < S; ++x)
            if ((gone >> x) & 1u) take |= ((1u << (8 * (x + 1) / S)) - 1u) & ~((1u << (8 * x / S)) - 1u);
        take &= ~sk_own;
        if (take & 1u) take_block(integral_constant<int, 0>{}, same_xcd);
        if (take & 2u) take_block(integral_constant<int, 1>{}, same_xcd);
        if (take & 4u) take_block(integral_constant<int, 2>{}, same_xcd);
        if (take & 8u) take_block(integral_constant<int, 3>{}, same_xcd);
        if (take & 16u) take_block(integral_constant<int, 4>{}, same_xcd);
        if (take & 32u) take_block(integral_constant<int, 5>{}, same_xcd);
        if (take & 64u) take_block(integral_constant<int, 6>{}, same_xcd);
        if (take & 128u) take_block(integral_constant<int, 7>{}, same_xcd);
        sk_own |= take;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {   // statistics only: did every slice of this tile run on this XCD (the placement both callers arrange)?
        const unsigned per_xcd = __hip_atomic_load(w0 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        finished(((per_xcd >> (3 * flag[3])) & 7u) == (unsigned)S);
    }
    return false;
}

// ------------------------------------------------------------------------------------------------
// k_gemm8p_tn: 256 x 256 x 64 tiles, 8 waves (2 (M) x 4 (N), wave tile 128 x 64 = 8 x 4 MFMA 16x16x32 tiles,
// 128 accumulator VGPRs), ONE workgroup per CU, LDS-DMA staging with a counted vmcnt and raw barriers --
// the "8-phase" schedule of the CDNA GEMM playbook, derived here for this operand layout:
//
//  * a K-tile (64 deep) is FOUR half-tiles of 16 KB (128 rows x 128 B), in the order they are first needed:
//      g % 4 = 0  A_m0: A rows {0..63, 128..191}   (each wave's first 64 rows)
//              1  B_n0: W rows {64 wc + 0..31}      (each wave's first 32 columns)
//              2  B_n1: W rows {64 wc + 32..63}
//              3  A_m1: A rows {64..127, 192..255}
//    two K-tiles of LDS (128 KB) + a 16 KB dump slot for the stage instructions past the end of K;
//  * a K-tile is FOUR phases of 16 MFMAs per wave, one 64 x 32 quadrant of the wave tile each, in the order
//    (m0,n0) (m0,n1) (m1,n1) (m1,n0); phase 0 reads A_m0 + B_n0 from LDS (12 ds_read_b128), phase 1 B_n1 (4),
//    phase 2 A_m1 (8), phase 3 nothing (B_n0 is still in registers);
//  * phase P (counted over the whole K loop) issues the DMA of half-tile P + 6: its slot was last read in phase
//    P - 2; it waits, with vmcnt(6), until half-tiles <= P + 2 of this wave's own DMA have landed (3 half-tiles
//    = 6 instructions stay in flight);
//  * waves 4..7 (the partner of wave w on its SIMD is wave w + 4) run ONE barrier behind waves 0..3: while one
//    half reads LDS / issues DMA, the other half issues its 16 MFMAs, so each SIMD's matrix pipe always has work.
//    With the one-barrier stagger a half-tile read in phase P was waited for by every wave in phase P - 1 or
//    earlier (the +1 in "P + 2" above), and the slot written in phase P was read no later than phase P - 2.
//  LDS rows are 128 B = 8 chunks of 16 B; chunk c of row r sits at physical chunk c ^ ((r >> 1) & 7) (the DMA lanes
//  fetch the matching logical chunk): a ds_read_b128 lane group of the 16x16x32 operand read (8 rows at k-block kb,
//  8 rows at kb + 1) then touches 16 distinct 16-byte slots of the 256-byte bank row.
//  Round 3: the default main loop runs TWO phases per K-tile instead of four -- quadrants (m0,n0) (m0,n1), then (m1,n1) (m1,n0):
//  32 MFMAs behind every hand-over between the wave halves, four barriers per K-tile instead of eight (LnFold::loop2; the
//  invariants are written out at the loop).  The four-phase loop described above stays selectable (VF_GEMM_8P_LOOP2=0) and
//  is what the LayerNorm-fold instances run.
//  Requires M % 256 == 0, N % 256 == 0, K % 64 == 0, K >= 128.
// ------------------------------------------------------------------------------------------------

template <int EPI>
__global__ __launch_bounds__(PTHREADS) void k_gemm8p_tn(const half_t* __restrict__ A, const half_t* __restrict__ W,
                                                          const float* __restrict__ bias, const half_t* __restrict__ R,
                                                          half_t* __restrict__ C, int M, int N, int K, LnFold lf) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // ONE array: [2 K-tiles][4 half-tiles][16 KB] + dump
    const int tid = threadIdx.x, lane = tid & 63;
    constexpr bool RES16 = EPI == EPI_BIAS_RESIDUAL || EPI == EPI_RES_STATS || EPI == EPI_LNRES_STATS;
    // Operands swapped (D = W_frag x A_frag): a lane then owns FOUR CONSECUTIVE COLUMNS of one output row instead of one column
    // of four rows, and the epilogue moves the tile into its LDS image with 32 eight-byte writes per lane instead of 128
    // two-byte ones (round 3; the fp32-residual form always worked this way, straight from the registers).
#ifdef VF_8P_SWAP_EPILOGUE   // A/B builds only: measured SLOWER inside the forward ("operand order and power")
    constexpr bool SWAP16 = EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_QGELU || EPI == EPI_BIAS_RESIDUAL;
#else
    constexpr bool SWAP16 = false;
#endif
    constexpr bool SWAP = SWAP16 || EPI == EPI_RESIDUAL_F32;
    constexpr bool LNA = EPI == EPI_LNA || EPI == EPI_LNA_GELU, STATS = EPI == EPI_RES_STATS || EPI == EPI_LNRES_STATS;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r15 = lane & 15, kb = lane >> 4, wr = wid >> 2, wc = wid & 3;
    int mt_idx, nt_idx;
    int sk_tile = -1, sk_slice = 0;
    unsigned sk_own = 0xffu;    // bit mi: THIS workgroup finishes and stores the 16-row blocks mi of both 128-row halves (all, or a split-K slice's share)
    {   // XCD-contiguous, n-major groups of 4 m-tiles
        const int Mt = M / PBM, Nt = N / PBN, nwg = Mt * Nt;
        int orig = blockIdx.x;
        if (lf.sk_S > 1 && orig >= lf.sk_nfull) {   // a slice of a tail tile: indices congruent mod 8 (one XCD) share a tile
            const int j = orig - lf.sk_nfull, i = j >> 3;
            sk_tile = (i / lf.sk_S) * 8 + (j & 7); sk_slice = i % lf.sk_S;
            if (sk_tile >= lf.sk_ntail) return;     // padding of the sliced part (before any barrier)
            orig = lf.sk_nfull + sk_tile;
        }
        const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
        const int p = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
        constexpr int GM = 4;
        const int g = p / (GM * Nt), r = p - g * (GM * Nt);
        const int gm = (Mt - g * GM) < GM ? (Mt - g * GM) : GM;
        nt_idx = r / gm;
        mt_idx = g * GM + (r - nt_idx * gm);
    }
    const long long m0 = (long long)mt_idx * PBM, n0 = (long long)nt_idx * PBN;
    // ---- staging: wave w issues DMA instructions 2w, 2w+1 of every half-tile: LDS rows 16 w + 8 j + (lane >> 3)
    const half_t* src[4][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = 16 * wid + 8 * j + (lane >> 3);          // LDS row of the half-tile
        const int lc = (lane & 7) ^ ((i >> 1) & 7);            // logical 16-byte chunk this lane fetches
        const int am0 = i < 64 ? i : 64 + i, am1 = am0 + 64;   // A_m0: rows {0..63, 128..191}; A_m1: + 64
        const int bn0 = (i >> 5) * 64 + (i & 31), bn1 = bn0 + 32;
        src[0][j] = A + (m0 + am0) * K + lc * 8;
        if ((EPI == EPI_GATED_SILU || EPI == EPI_GATED_GELU)) {
            // gated product: the tile's 256 columns are 128 gate columns and the SAME 128 up columns, laid out so that a wave's
            // first 32 columns (half-tile B_n0) are gate rows and its second 32 (B_n1) the matching up rows of W
            const long long gr = (long long)nt_idx * 128 + (i >> 5) * 32 + (i & 31);
            src[1][j] = W + gr * K + lc * 8;
            src[2][j] = W + ((long long)(N >> 1) + gr) * K + lc * 8;
        } else {
            src[1][j] = W + (n0 + bn0) * K + lc * 8;
            src[2][j] = W + (n0 + bn1) * K + lc * 8;
        }
        src[3][j] = A + (m0 + am1) * K + lc * 8;
    }
    // K range of this workgroup: all of K, or slice sk_slice of sk_S (whole K-tiles, >= 2 each: the host checks)
    const int nk_all = K / PBK;
    const int kt_lo = sk_tile >= 0 ? nk_all * sk_slice / lf.sk_S : 0;
    const int nk = (sk_tile >= 0 ? nk_all * (sk_slice + 1) / lf.sk_S : nk_all) - kt_lo, G = 4 * nk;   // K-tiles, half-tiles
    auto stage = [&](int g) {             // g: half-tile counted over the whole K loop (wave-uniform)
        const int s = g & 3;
        const int kt = g < G ? (g >> 2) : nk - 1;                                // past the end: re-read the last K-tile ...
        const int slot = g < G ? ((g >> 2) & 1) * 4 + s : 8;                     // ... into the dump slot
        char* dst = smem + slot * PSLOT + (16 * wid) * 128;
        const half_t* s0 = s == 0 ? src[0][0] : s == 1 ? src[1][0] : s == 2 ? src[2][0] : src[3][0];
        const half_t* s1 = s == 0 ? src[0][1] : s == 1 ? src[1][1] : s == 2 ? src[2][1] : src[3][1];
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s0 + (long long)(kt_lo + kt) * PBK),
                                         (__attribute__((address_space(3))) void*)(dst), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(s1 + (long long)(kt_lo + kt) * PBK),
                                         (__attribute__((address_space(3))) void*)(dst + 1024), 16, 0, 0);
    };
    f4v acc[8][4];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[a][b][e] = 0.f;
    // fragment addresses inside a half-tile: row = (wave's 64 / 32 rows) + tile * 16 + r15; chunk (4 ks + kb) ^ ((r15 >> 1) & 7)
    const int swz = (r15 >> 1) & 7;
    const int a_off = (wr * 64 + r15) * 128, b_off = (wc * 32 + r15) * 128;
    const int c0 = ((0 + kb) ^ swz) * 16, c1 = ((4 + kb) ^ swz) * 16;   // k-steps 0 and 1
    h8 Af[4][2], B0f[2][2], B1f[2][2];
#define VFT_READ_A(SLOTBASE)                                                              \
    _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                        \
        Af[t][0] = *(const h8*)((SLOTBASE) + a_off + t * 2048 + c0);                       \
        Af[t][1] = *(const h8*)((SLOTBASE) + a_off + t * 2048 + c1);                       \
    }
#define VFT_READ_B(DSTF, SLOTBASE)                                                         \
    _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                        \
        DSTF[t][0] = *(const h8*)((SLOTBASE) + b_off + t * 2048 + c0);                     \
        DSTF[t][1] = *(const h8*)((SLOTBASE) + b_off + t * 2048 + c1);                     \
    }
#ifdef VF_8P_QUAD_T_INNER   /* A/B builds: consecutive MFMAs share the W fragment instead of the A fragment */
#define VFT_QUAD_LOOPS _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) _Pragma("unroll") for (int u = 0; u < 2; ++u) _Pragma("unroll") for (int t = 0; t < 4; ++t)
#else
#define VFT_QUAD_LOOPS _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) _Pragma("unroll") for (int t = 0; t < 4; ++t) _Pragma("unroll") for (int u = 0; u < 2; ++u)
#endif
#define VFT_QUAD(MQ, NQ, BF)                                                               \
    VFT_QUAD_LOOPS                                                                         \
                acc[(MQ) * 4 + t][(NQ) * 2 + u] = SWAP                                                                        \
                    ? __builtin_amdgcn_mfma_f32_16x16x32_f16(BF[u][ks], Af[t][ks], acc[(MQ) * 4 + t][(NQ) * 2 + u], 0, 0, 0) \
                    : __builtin_amdgcn_mfma_f32_16x16x32_f16(Af[t][ks], BF[u][ks], acc[(MQ) * 4 + t][(NQ) * 2 + u], 0, 0, 0);
#define VFT_PHASE_HEAD(G)                                                                  \
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");                                       \
    __builtin_amdgcn_s_barrier();                                                          \
    stage(G);
#define VFT_PHASE_MID()                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    __builtin_amdgcn_s_barrier();                                                          \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                     \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    __builtin_amdgcn_s_setprio(1);
#define VFT_PHASE_TAIL()                                                                   \
    __builtin_amdgcn_s_setprio(0);                                                         \
    __builtin_amdgcn_sched_barrier(0);
    if (lf.loop2) {
        // TWO phases per K-tile (round 3): X = quadrants (m0,n0) (m0,n1) on A_m0, B_n0, B_n1 (16 fragment reads, 32 MFMAs),
        // Y = (m1,n1) (m1,n0) on A_m1 (8 reads, 32 MFMAs): four barriers per K-tile instead of eight, twice the matrix work
        // behind each hand-over between the wave halves.  Every fragment read has COMPLETED before the barrier that follows it
        // (lgkmcnt(0) in front of the barrier, in the shadow of the partner half's 32 MFMAs), so a slot may be restaged by
        // whoever passes the next barrier: X(kt) restages half-tile 4 kt + 7 (its slot, A_m1 of the other buffer, was read in
        // Y(kt - 1)), Y(kt) the three half-tiles 4 kt + 8 .. + 10 (read in X(kt)).  Landed-guarantees, one phase ahead for the
        // half that reads one barrier later: X waits until half-tiles <= 4 kt + 3 of this wave's DMA are in (vmcnt(6): 4 kt + 4
        // .. + 6 may fly), Y until <= 4 kt + 6 (vmcnt(2): only 4 kt + 7 may fly).
        for (int g = 0; g < 7; ++g) stage(g);
        if (wr == 1) {
            asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // 14 issued, 8 may fly: half-tiles 0 .. 2 of this wave landed
            __builtin_amdgcn_s_barrier();
        }
        for (int kt = 0; kt < nk; ++kt) {
            const char* base = smem + (kt & 1) * (4 * PSLOT);
            asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            stage(4 * kt + 7);
            VFT_READ_B(B0f, base + 1 * PSLOT)
            VFT_READ_B(B1f, base + 2 * PSLOT)
            VFT_READ_A(base + 0 * PSLOT)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
            VFT_QUAD(0, 0, B0f)
            VFT_QUAD(0, 1, B1f)
            VFT_PHASE_TAIL()
            asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            stage(4 * kt + 8);
            stage(4 * kt + 9);
            stage(4 * kt + 10);
            VFT_READ_A(base + 3 * PSLOT)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
            VFT_QUAD(1, 1, B1f)
            VFT_QUAD(1, 0, B0f)
            VFT_PHASE_TAIL()
        }
    } else {
    for (int g = 0; g < 6; ++g) stage(g);
    if (wr == 1) {   // waves 4..7 run one barrier behind; the other half reads half-tiles 0 and 1 right after this barrier
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // 12 issued, 8 may still fly: half-tiles 0, 1 of this wave landed
        __builtin_amdgcn_s_barrier();
    }
    for (int kt = 0; kt < nk; ++kt) {
        const char* base = smem + (kt & 1) * (4 * PSLOT);
        const int g0 = 4 * kt + 6;
        // phase 0: quadrant (m0, n0); reads B_n0 then A_m0
        VFT_PHASE_HEAD(g0)
        VFT_READ_B(B0f, base + 1 * PSLOT)
        VFT_READ_A(base + 0 * PSLOT)
        VFT_PHASE_MID()
        VFT_QUAD(0, 0, B0f)
        VFT_PHASE_TAIL()
        // phase 1: quadrant (m0, n1); reads B_n1
        VFT_PHASE_HEAD(g0 + 1)
        VFT_READ_B(B1f, base + 2 * PSLOT)
        VFT_PHASE_MID()
        VFT_QUAD(0, 1, B1f)
        VFT_PHASE_TAIL()
        // phase 2: quadrant (m1, n1); reads A_m1
        VFT_PHASE_HEAD(g0 + 2)
        VFT_READ_A(base + 3 * PSLOT)
        VFT_PHASE_MID()
        VFT_QUAD(1, 1, B1f)
        VFT_PHASE_TAIL()
        // phase 3: quadrant (m1, n0); nothing to read
        VFT_PHASE_HEAD(g0 + 3)
        VFT_PHASE_MID()
        VFT_QUAD(1, 0, B0f)
        VFT_PHASE_TAIL()
    }
    }
#undef VFT_READ_A
#undef VFT_READ_B
#undef VFT_QUAD
#undef VFT_PHASE_HEAD
#undef VFT_PHASE_MID
#undef VFT_PHASE_TAIL
    if (wr == 0) __builtin_amdgcn_s_barrier();   // balance the stagger
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the dump-slot DMAs
    __syncthreads();
    if constexpr (EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_RESIDUAL) {
        if (sk_tile >= 0) {
            const SkCtx skc{lf.sk_ws, lf.sk_cnt, lf.sk_stat, lf.sk_S, lf.sk_dbg};
            if (sk_coop_finish(acc, skc, sk_tile, sk_slice, sk_own, (unsigned*)(smem + 8 * PSLOT), tid)) return;
        }
    }
    if (EPI == EPI_RESIDUAL_F32) {
        // fp32 residual stream (decoder): the MFMA operands were swapped (W fragment first), so a lane holds 4 consecutive
        // COLUMNS of one row -- out = R + acc as one 16-byte read-modify-write per tile, straight from the registers
        const float* Rf = (const float*)R;
        float* Cf = (float*)C;
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const long long off = (m0 + wr * 128 + mi * 16 + r15) * N + n0 + wc * 64 + ni * 16 + 4 * kb;
                const f4v rv = *(const f4v*)(Rf + off);
                f4v o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = rv[e] + acc[mi][ni][e];
                *(f4v*)(Cf + off) = o;
            }
        return;
    }
    if ((EPI == EPI_GATED_SILU || EPI == EPI_GATED_GELU)) {
        // gated epilogue: out[row][32 wc + 16 ni + r15] = act(gate) * up with gate = acc[.][ni], up = acc[.][ni + 2] (ni = 0, 1),
        // fp32 throughout (the unfused path rounds both products to fp16 first); a [256][128] fp16 image, then 16-byte chunks
        half_t* Eg = (half_t*)smem;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int col = wc * 32 + ni * 16 + r15;
#pragma unroll
            for (int mi = 0; mi < 8; ++mi)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int row = wr * 128 + mi * 16 + 4 * kb + reg;
                    const float g = acc[mi][ni][reg], u = acc[mi][ni + 2][reg];
                    // tanh-GELU = x * sigmoid(2 * 0.7978845608 * (x + 0.044715 x^3)) (gelu_tanh);  SiLU = x * sigmoid(x)
                    Eg[row * 128 + col] = (half_t)((EPI == EPI_GATED_GELU ? gelu_tanh(g) : g / (1.0f + __expf(-g))) * u);
                }
        }
        __syncthreads();
        const int NO = N >> 1;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = tid + PTHREADS * i, row = c >> 4, cc = c & 15;   // 16 chunks of 8 halves per 128-wide row
            *(h8*)(C + (m0 + row) * NO + (long long)nt_idx * 128 + cc * 8) = *(const h8*)(Eg + row * 128 + cc * 8);
        }
        return;
    }
    if constexpr (SWAP16) {
        // swapped layout: lane (r15, kb) of tile (mi, ni) holds row wr 128 + mi 16 + r15, columns wc 64 + ni 16 + 4 kb .. + 3.
        // Image rows are 528 bytes (256 halves + 8): the 16 lanes of a ds_write_b64 group (one kb, rows r15 = 0 .. 15) land 16
        // bytes apart, and the 16-byte row reads below stay aligned.  135 KB of the 144.
        constexpr int ES = PBN + 8;
        half_t* Es2 = (half_t*)smem;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int col = wc * 64 + ni * 16 + 4 * kb;
            f4v bv = {0.f, 0.f, 0.f, 0.f};
            if (bias) bv = *(const f4v*)(bias + n0 + col);
#pragma unroll
            for (int mi = 0; mi < 8; ++mi) {
                const int row = wr * 128 + mi * 16 + r15;
                f2v v0 = {acc[mi][ni][0] + bv[0], acc[mi][ni][1] + bv[1]};
                f2v v1 = {acc[mi][ni][2] + bv[2], acc[mi][ni][3] + bv[3]};
                if (EPI == EPI_BIAS_GELU) { v0 = gelu_erf2(v0); v1 = gelu_erf2(v1); }
                if (EPI == EPI_BIAS_QGELU) { v0 = quick_gelu2(v0); v1 = quick_gelu2(v1); }
                const h4 o = {(half_t)v0[0], (half_t)v0[1], (half_t)v1[0], (half_t)v1[1]};
                *(h4*)(Es2 + row * ES + col) = o;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = tid + PTHREADS * i, row = c >> 5, cc = c & 31;  // 32 chunks of 8 halves per 256-wide row
            h8 o = *(const h8*)(Es2 + row * ES + cc * 8);
            const long long off = (m0 + row) * N + n0 + cc * 8;
            if (EPI == EPI_BIAS_RESIDUAL) {
                const h8 r = *(const h8*)(R + off);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)o[e] + (float)r[e]);
            }
            *(h8*)(C + off) = o;
        }
        return;
    }
    // epilogue through LDS: fp16(acc + bias [+GELU]) into a [256][256] fp16 image (the two K-tile buffers), then
    // 16-byte row chunks out (residual added in fp32 on the vector side)
    half_t* Es = (half_t*)smem;
    float2* rowst = (float2*)(smem + 8 * PSLOT);   // the dump slot: (mean, rstd) of the tile's 256 rows (LnFold)
    if constexpr (LNA || EPI == EPI_LNRES_STATS) {
        if (tid < PBM) {
            float sm = 0.f, sq = 0.f;
            for (int pz = 0; pz < lf.n_parts; ++pz) {
                const float2 v = *(const float2*)(lf.stats_in + ((long long)pz * lf.Mp + m0 + tid) * 2);
                sm += v.x; sq += v.y;
            }
            const float mean = sm * lf.inv_h;
            const float var = fmaxf(sq * lf.inv_h - mean * mean, 0.f);
            rowst[tid] = make_float2(mean, rsqrtf(var + lf.eps));
        }
        __syncthreads();
    }
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
        const int col = wc * 64 + ni * 16 + r15;
        const float bv = bias ? bias[n0 + col] : 0.f;
        float csv = 0.f;
        if constexpr (LNA) csv = lf.colsum[n0 + col];
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
#pragma unroll
            for (int reg = 0; reg < 4; reg += 2) {
                const int row = wr * 128 + mi * 16 + 4 * kb + reg;
                f2v v;
                if constexpr (LNA) {   // rstd (acc - mean colsum) + c   (c arrives as `bias`)
                    const float2 s0 = rowst[row], s1 = rowst[row + 1];
                    v[0] = s0.y * (acc[mi][ni][reg] - s0.x * csv) + bv;
                    v[1] = s1.y * (acc[mi][ni][reg + 1] - s1.x * csv) + bv;
                } else {
                    v[0] = acc[mi][ni][reg] + bv; v[1] = acc[mi][ni][reg + 1] + bv;
                }
                if (EPI == EPI_BIAS_GELU || EPI == EPI_LNA_GELU) v = gelu_erf2(v);
                if (EPI == EPI_BIAS_QGELU) v = quick_gelu2(v);
                Es[row * PBN + col] = (half_t)v[0];
                Es[(row + 1) * PBN + col] = (half_t)v[1];
            }
    }
    __syncthreads();
    float gr[8], br[8];
    if constexpr (EPI == EPI_LNRES_STATS) {   // a thread's 16 chunks all sit in the same 8 columns
        const int cc0 = tid & 31;
#pragma unroll
        for (int e = 0; e < 8; ++e) { gr[e] = lf.gR[n0 + cc0 * 8 + e]; br[e] = lf.bR[n0 + cc0 * 8 + e]; }
    }
    // pass i covers rows 16 i .. 16 i + 15 = block mi = i & 7 of half i >> 3.  A co-operative split-K slice stores its own blocks only:
    // its passes over the others repeat an owned block (every load stays unconditional, so all sixteen are in flight together) and
    // their stores go out of the buffer's bounds, where the hardware drops them -- no branch in either form of the loop (with a
    // branch around each store the compiler issued one pass's loads after the previous pass's store: + 2 % on a 600-tile product)
    auto store_tile = [&](auto SPLIT) {
        constexpr bool split = decltype(SPLIT)::value;
        const sq_rsrc_t rc = sq_rsrc(C + m0 * N + n0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            bool own = true;
            int ie = i;
            if constexpr (split) { own = (sk_own >> (i & 7)) & 1u; ie = own ? i : ((i & 8) | __builtin_ctz(sk_own)); }
            const int c = tid + PTHREADS * ie, row = c >> 5, cc = c & 31;  // 32 chunks of 8 halves per 256-wide row
            h8 o = *(const h8*)(Es + row * PBN + cc * 8);
            const long long off = (m0 + row) * N + n0 + cc * 8;
            if (RES16) {
                const h8 r = *(const h8*)(R + off);
                if constexpr (EPI == EPI_LNRES_STATS) {
                    const float2 st = rowst[row];
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)o[e] + (((float)r[e] - st.x) * st.y * gr[e] + br[e]));
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)o[e] + (float)r[e]);
                }
            }
            if constexpr (STATS) {   // row sums of the ROUNDED output: the 32 lanes of a half-wave hold one row's 32 chunks
                float sm = 0.f, sq = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) { const float y = (float)o[e]; sm += y; sq += y * y; }
#pragma unroll
                for (int d_ = 16; d_; d_ >>= 1) { sm += __shfl_xor(sm, d_, 32); sq += __shfl_xor(sq, d_, 32); }
                if (cc == 0) *(float2*)(lf.stats_out + ((long long)nt_idx * lf.Mp + m0 + row) * 2) = make_float2(sm, sq);
            }
            if constexpr (split) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, o), rc, own ? (int)((row * N + cc * 8) * 2) : 0x7ffffff0, 0, 0);
            else *(h8*)(C + off) = o;
        }
    };
    if (sk_tile >= 0) store_tile(std::true_type{});
    else store_tile(std::false_type{});
}


// ------------------------------------------------------------------------------------------------
// One LDS-DMA instruction (1 KB per wave) from inline asm, so that the compiler never sees an LDS-DMA and puts no vmcnt(0) in front of
// LDS traffic; every wait is written by hand.  LDS byte address and 64-bit global base are scalars (k_gemm9_tn keeps both as running
// state); the s_nop covers the M0 write -> LDS-DMA hazard the compiler's recognizer cannot see inside asm.
__device__ __forceinline__ void dma16u(unsigned long long ua, unsigned voff, unsigned lds_addr) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(ua), "s"(lds_addr)
                 : "memory");
}

// tile of a dispatch index: XCD-contiguous, n-major groups of 4 m-tiles (as k_gemm8p_tn)
__device__ __forceinline__ void q_tile_of(int orig, int Mt, int Nt, int& mt, int& nt) {
    const int ntiles = Mt * Nt, xcd = orig & 7, q8 = ntiles >> 3, r8 = ntiles & 7;
    const int p = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    constexpr int GM = 4;
    const int g = p / (GM * Nt), r = p - g * (GM * Nt);
    const int gm = (Mt - g * GM) < GM ? (Mt - g * GM) : GM;
    nt = r / gm;
    mt = g * GM + (r - nt * gm);
}

// ------------------------------------------------------------------------------------------------
// k_gemm9_tn (round 4): the PERSISTENT two-phase kernel with an LDS-FREE, BARRIER-FREE epilogue.
//
// What the numbers of round 3 say: a 256 x 256 tile of k_gemm8p_tn costs T(K) = 10 us + 0.0217 us x K -- the main
// loop moves its 64 KB per K-tile at 47 GB/s per CU = 12 TB/s chip-wide, i.e. AT the L2 -> LDS ceiling, and the fixed 10 us per
// tile (37 % of a K = 768 tile) are the epilogue: every workgroup of a round reaches it together, 256 x 128 KB of output
// meet the memory system as one burst (32 MB at ~4 TB/s = 8 us) while every matrix pipe idles, then 256 new workgroups are
// dispatched and wait for their first loads.  The persistent 8-phase experiment (k_gemm8q_tn) kept the loads of the next
// tile in flight but still moved the tile through LDS in four barrier-separated passes.  Here:
//  * the tile leaves STRAIGHT FROM THE ACCUMULATORS: operands swapped (D = W_frag x A_frag), and the W rows a wave stages
//    are PERMUTED so that lane (r15, kb) owns, for row r15 of every 16-row block, columns 8 kb .. 8 kb + 7 and 32 + 8 kb ..
//    + 7 of the wave's 64: two 16-byte stores per 16 x 64 block whose four kb lanes write one aligned 64-byte segment
//    each.  No LDS image, no barrier: the epilogue is ~200 VALU instructions and 16 fire-and-forget stores per lane;
//  * the stores DRAIN UNDER THE NEXT TILE'S MAIN LOOP: the stage sequence runs on into the next tile (its first seven
//    half-tiles are issued before the epilogue, as in k_gemm8q_tn), the first K-tile's counted waits leave the 16 stores in
//    flight (vmcnt is in order and counts stores);
//  * the one-barrier stagger between the two wave halves is never rebalanced: a half runs its epilogue while the other
//    still issues the last (or already the first) 32 MFMAs -- no wave waits for another one between tiles;
//  * residual rows are fetched into the (dead) fragment registers at the start of the epilogue; the bias of a tile arrives
//    by one LDS-DMA during its first K-tile, double-buffered by tile parity.
// Main loop, slot discipline and landed-guarantees are k_gemm8p_tn's two-phase loop (see there); q_stage maps half-tiles past
// the end of K to the next tile (or the dump slot).  Requires M, N % 256 == 0, K % 64 == 0, K >= 256; gridDim.x a multiple of
// 8 or the tile count.
// ------------------------------------------------------------------------------------------------
constexpr int RLDS = PLDS + 2048 + 1024;   // + two tiles' bias (2 x 256 floats) + wall-clock stamps of 16 tiles (debug)
constexpr int k9StampTiles = 16, k9Stamps = 6;

template <int EPI, int MODE = 0>   // MODE 0: whole tiles, data-parallel; 1: the whole product cut along K (one slice per workgroup); 2: stream-K
__global__ __launch_bounds__(PTHREADS) void k_gemm9_tn(const half_t* __restrict__ A, const half_t* __restrict__ W,
                                                         const float* __restrict__ bias, const half_t* __restrict__ R,
                                                         half_t* __restrict__ C, int M, int N, int K, int stagger_ticks, unsigned long long* __restrict__ dbg,
                                                         SkCtx sk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // [2 K-tiles][4 half-tiles][16 KB] + dump + 2 x bias + stamps
    constexpr bool SPLIT = MODE == 1, STREAMK = MODE == 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r15 = lane & 15, kb = lane >> 4, wr = wid >> 2, wc = wid & 3;
    const int Mt = M / PBM, Nt = N / PBN, ntiles = Mt * Nt;
    float* bias_lds = (float*)(smem + PLDS);
    // Per-lane byte offsets of the first DMA instruction of A_m0 and of B_n0 inside a tile's A / W panel.  The second instruction of
    // a half-tile fetches the rows 8 further down, whose swizzle differs: it keeps its own offset; A_m1 (+ 64 rows) and B_n1 (+ 32
    // rows) enter through the scalar base.
    unsigned voffA[2], voffW[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = 16 * wid + 8 * j + (lane >> 3);          // LDS row of the half-tile
        const int lc = (lane & 7) ^ ((i >> 1) & 7);            // logical 16-byte chunk this lane fetches
        const int am0 = i < 64 ? i : 64 + i;                   // A_m0: rows {0..63, 128..191}; A_m1: + 64
        // W rows, permuted: LDS row 32 w' + 16 u + jj of B_n0 (n-block u, MFMA column jj) holds column 8 (jj >> 2) + 4 u + (jj & 3)
        // of wave w''s first 32; B_n1 the same of its second 32
        const int jj = i & 15, u = (i >> 4) & 1;
        const int bn0 = (i >> 5) * 64 + 8 * (jj >> 2) + 4 * u + (jj & 3);
        voffA[j] = (unsigned)((am0 * K + lc * 8) * 2);
        voffW[j] = (unsigned)((bn0 * K + lc * 8) * 2);
    }
    const unsigned long long a_m1_bytes = (unsigned long long)64 * K * 2, b_n1_bytes = (unsigned long long)32 * K * 2;
    const int nk = K / PBK;
    // ---- WORK ITEMS of this workgroup: its tiles b, b + G, ... (an item = a tile and a range of its K-tiles; today always all of them.
    // Round 4 also built the remainder tiles of long-K products as K-slices inside this kernel -- partials through the handle's workspace,
    // last arriver reduces in slice order -- correct and deterministic, and SLOWER in the forward than handing those products to the
    // 8-phase kernel's split-K tail: 11.67 vs 11.48 ms at 768 wide, 36.4 vs 35.6 at 1024; profiles/r04_gemm9_tail_slices.log.  Removed.)
    // Round 5, sk.S in {2, 3, 4}: a product of LESS than a round with a long K (FFN-down of a data-parallel rank's 13 pairs: 78 tiles,
    // K = 3072 -- a third of the CUs at work for 63 us) is cut whole: the grid is 8 x ceil(tiles / 8) x S workgroups, ONE item each --
    // slice i % S of the tile at XCD-local index i / S, i = blockIdx / 8 (the slices of a tile share blockIdx % 8 = one XCD under the
    // round-robin placement: their partials meet in that L2) -- and the tile leaves through sk_coop_finish (the 8-phase kernel's
    // co-operative finish) instead of the plain epilogue, each slice finishing the 16-row blocks it owns.
    const int G_ = (int)gridDim.x, wg = (int)blockIdx.x;
    const int sk_S = SPLIT && sk.S > 1 ? sk.S : 1;   // (SPLIT is its own instantiation: the multi-item kernel's loop and registers stay as they were)
    int sk_tile = -1, sk_slice = 0;
    if (sk_S > 1) {
        const int i = wg >> 3;
        sk_slice = i % sk_S;
        const int t_local = i / sk_S, xcd = wg & 7;
        if (t_local >= (ntiles >> 3) + (xcd < (ntiles & 7) ? 1 : 0)) return;   // padding of the sliced grid (before any barrier)
        sk_tile = t_local * 8 + xcd;
    }
    // ---- STREAM-K (MODE 2, round 5).  The K-tiles of an XCD's tiles (the contiguous chunk q_tile_of gives it), laid end to end, are
    // dealt out EVENLY to the XCD's workgroups: a workgroup's range [lo, hi) starts and ends anywhere inside a tile, so a product
    // of 1.2 or 2.3 rounds costs 1.2 or 2.3 tiles' time per workgroup instead of 2 or 3.  A range is cut at the tile boundaries into
    // SEGMENTS (its items); one that does not reach its tile's last K-tile leaves the accumulators in the workgroup's slot of the
    // handle's workspace (write-through stores, then one count on the finisher's word) -- a DUMP --, the one that does reach it
    // without having started the tile waits for those counts, adds the partials in ascending-K order (a fixed order: bit-equal
    // from run to run) and runs the epilogue -- the FINISH.  A workgroup walks its segments from the END of its range to the
    // start: its dump (the head of a tile other workgroups complete) comes FIRST, its finish (the tail of a tile started by
    // workgroups with LOWER indices) LAST -- so a finisher only ever waits for workgroups dispatched before it, which dump
    // before they do anything else: no circular wait, whatever else occupies the chip.  Range ends are nudged off a tile's
    // first and last K-tile (every segment >= 2 K-tiles: the loop's counted waits assume it).  The order of an XCD's tiles is
    // transposed so that, as in the data-parallel walk, the tiles in flight at any moment are neighbours that share
    // operand panels in L2.
    // Everything a workgroup needs to know about its range is worked out ONCE, in front of the loop, lane-parallel, and kept in two
    // vector registers (x_t0, x_t1: lane i < 16 = the i-th segment walked -- tile coordinates, first K-tile, K-tiles; lane 32 = the
    // workgroup whose word this one's dump counts on; lane 33 = how many partials its finish waits for): the loop reads them with
    // v_readlane.  (Kept as scalars, this state -- a dozen values and the divisions behind them -- overflowed the scalar file, and
    // the spill code around the loop pushed 70-230 vector registers to scratch.)
    int x_t0 = 0, x_t1 = 0, x_items = 0;
    bool x_dump0 = false, x_fin = false;
    if constexpr (STREAMK) {
        const int xcd = wg & 7, wl = wg >> 3, GL = G_ >> 3;
        const int q8 = ntiles >> 3, r8 = ntiles & 7;
        const int nx = q8 + (xcd < r8 ? 1 : 0), base = xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8;
        auto bound = [&](int w) -> int {   // (32-bit: w nx nk < 2^21 for any product the host sends here)
            unsigned bb = (unsigned)w * (unsigned)(nx * nk) / (unsigned)GL;
            const unsigned r = bb % (unsigned)nk;
            if (r == 1u) bb -= 1u; else if (r == (unsigned)nk - 1u) bb += 1u;
            return (int)bb;
        };
        const int lo = bound(wl), hi = bound(wl + 1);
        const int first_t = lo / nk, last_t = hi > lo ? (hi - 1) / nk : first_t;
        x_items = hi > lo ? last_t - first_t + 1 : 0;
        // roles: the first segment walked is a DUMP when it stops short of its tile's end (hi inside a tile); the last one a FINISH when it
        // starts inside its tile (lo inside a tile) and reaches the end; a lone segment can be either, or a whole tile
        x_dump0 = (hi % nk) != 0;
        x_fin = (lo % nk) != 0 && !(x_items == 1 && x_dump0);
        {
            int tl = last_t - (lane & 15);
            if (tl < first_t) tl = first_t;
            const int s_ = lo > tl * nk ? lo : tl * nk, e_ = hi < (tl + 1) * nk ? hi : (tl + 1) * nk;
            // tl-th tile of this XCD in stream order -> tile coordinates: a ragged R x GL grid walked column-major, tiles numbered row-major
            const int R = (nx + GL - 1) / GL, lastc = nx - (R - 1) * GL, Rm1 = R > 1 ? R - 1 : 1;
            int col, row;
            if (tl < lastc * R) { col = tl / R; row = tl - col * R; }
            else { const int v2 = tl - lastc * R; col = lastc + v2 / Rm1; row = v2 - (col - lastc) * Rm1; }
            const int pt = base + row * GL + col;
            constexpr int GM = 4;
            const int g = pt / (GM * Nt), r = pt - g * (GM * Nt);
            const int gm = (Mt - g * GM) < GM ? (Mt - g * GM) : GM;
            const int nt_ = r / gm, mt_ = g * GM + (r - nt_ * gm);
            x_t0 = mt_ | (nt_ << 16);
            x_t1 = (s_ - tl * nk) | ((e_ - s_) << 16);
        }
        if (x_dump0) {   // the workgroup that reaches the end of the tile this one dumps the head (or a middle) of
            const int tile_end = (last_t + 1) * nk;
            int f = wl + 1;
            while (bound(f + 1) < tile_end) ++f;
            if (lane == 32) x_t0 = f * 8 + xcd;
        }
        if (x_fin) {     // the workgroups below that hold the rest of the tile this one finishes
            const int tile_start = first_t * nk;
            int P = 1;
            while (bound(wl - P) > tile_start) ++P;
            if (lane == 33) x_t0 = P;
        }
    }
    const int n_items = STREAMK ? x_items : sk_S > 1 ? 1 : (wg < ntiles ? (ntiles - wg + G_ - 1) / G_ : 0);
    if (n_items == 0) return;                                   // (before any barrier)
    auto item = [&](int idx, int& mt_, int& nt_, int& klo_, int& nk_) {
        if (STREAMK) {
            const int a_ = __builtin_amdgcn_readlane(x_t0, idx), b_ = __builtin_amdgcn_readlane(x_t1, idx);
            mt_ = a_ & 0xffff; nt_ = a_ >> 16; klo_ = b_ & 0xffff; nk_ = b_ >> 16;
        }
        else if (sk_S > 1) { q_tile_of(sk_tile, Mt, Nt, mt_, nt_); klo_ = nk * sk_slice / sk_S; nk_ = nk * (sk_slice + 1) / sk_S - klo_; }
        else { q_tile_of(wg + idx * G_, Mt, Nt, mt_, nt_); klo_ = 0; nk_ = nk; }
    };
    const sq_rsrc_t x_rw = sq_rsrc(sk.ws);
    auto x_dump = [&](f4v (&acc_)[8][4]) {   // every thread: the accumulators to this workgroup's slot, [mi * 4 + ni][thread] x 16 B
        int my = wg * 32 * PTHREADS * 16;   // (scalar offset + one per-thread offset: no address registers)
        asm volatile("" : "+s"(my));           // (opaque: left visible, the 32 scalar offsets are hoisted out of the main loop and spilled)
#pragma unroll
        for (int mi = 0; mi < 8; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i4v, acc_[mi][ni]), x_rw, tid * 16, my + (mi * 4 + ni) * PTHREADS * 16, 16);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    // (read in UNIFORM control flow, all lanes enabled: a cross-lane read inside `if (tid == 0)` can meet a register the allocator has
    //  just reloaded from scratch for the active lanes only -- lane 32 of it is then whatever was there: the first build of this
    //  faulted on exactly that address)
    const int x_tgt = STREAMK ? __builtin_amdgcn_readlane(x_t0, 32) : 0, x_P = STREAMK && x_fin ? __builtin_amdgcn_readlane(x_t0, 33) : 0;
    auto x_count = [&]() {   // tid 0, behind a rendezvous of all waves: one count on the word of the workgroup that finishes the dumped tile
        (void)__hip_atomic_fetch_add(sk.cnt + x_tgt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    int mt_c, nt_c, klo_c, nk_c;
    item(0, mt_c, nt_c, klo_c, nk_c);
    int ktg = 0;   // K-tiles consumed by this workgroup so far: LDS buffer of local K-tile kt is (ktg + kt) & 1
    // ---- the STAGE CURSOR: half-tiles are staged strictly in sequence (A_m0, B_n0, B_n1, A_m1 of K-tile 0, then of K-tile 1, ...,
    // running on into the workgroup's next item), 1.75 K-tiles ahead of the MFMAs.  Its state lives in scalar registers and
    // moves by a few scalar adds per half-tile (the first version recomputed tile, K-tile and slot of every half-tile from its
    // index: ~45 scalar instructions per stage call, 180 in front of every K-tile's first barrier).
    unsigned long long st_a, st_w;          // byte addresses of the K-tile being staged: row 0 of the tile's A / W panel, its first k
    int st_kt = 0, st_nk = nk_c, st_item = 0;   // that K-tile's index in its item, the item's K-tiles, the item
    unsigned st_slot;                       // LDS byte address of that K-tile's buffer + this wave's 2 KB piece (toggles by 64 KB)
    bool st_dump = false;                   // past the workgroup's last item: the stage calls go on re-reading into the dump slot
    const unsigned lds_smem = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(__attribute__((address_space(3))) const char*)smem);
    const unsigned lds0 = lds_smem + (unsigned)(16 * wid * 128);
    auto panel = [&](int mt_, int nt_, int klo_) {
        const unsigned long long a0 = (unsigned long long)A + ((unsigned long long)((long long)mt_ * PBM * K) + (unsigned long long)klo_ * PBK) * 2ull;
        const unsigned long long w0 = (unsigned long long)W + ((unsigned long long)((long long)nt_ * PBN * K) + (unsigned long long)klo_ * PBK) * 2ull;
        st_a = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a0);
        st_w = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(w0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)w0);
    };
    panel(mt_c, nt_c, klo_c);
    st_slot = lds0;
    auto stage_advance = [&]() {            // after A_m1: on to the next K-tile (of this item, of the next one, or of the dump)
        st_slot = lds0 + ((st_slot - lds0) ^ (4u * PSLOT));
        if (st_dump) return;
        if (++st_kt < st_nk) { st_a += PBK * 2; st_w += PBK * 2; return; }
        st_kt = 0;
        if (++st_item < n_items) {
            int mt_, nt_, klo_;
            item(st_item, mt_, nt_, klo_, st_nk);
            panel(mt_, nt_, klo_);
        } else {
            st_dump = true;                 // keep the last K-tile's addresses: valid memory, landing in the dump slot
        }
    };
#define VF9_STAGE(S_)                                                                                                  \
    {                                                                                                                  \
        const unsigned dst_ = st_dump ? lds0 + 8u * PSLOT : st_slot + (unsigned)(S_) * PSLOT;                          \
        const unsigned long long b_ = (S_) == 0 ? st_a : (S_) == 3 ? st_a + a_m1_bytes : (S_) == 1 ? st_w : st_w + b_n1_bytes; \
        dma16u(b_, ((S_) == 0 || (S_) == 3) ? voffA[0] : voffW[0], dst_);                                              \
        dma16u(b_, ((S_) == 0 || (S_) == 3) ? voffA[1] : voffW[1], dst_ + 1024u);                                      \
        if ((S_) == 3) stage_advance();                                                                                \
    }
    f4v acc[8][4];
    const int swz = (r15 >> 1) & 7;
    const int a_off = (wr * 64 + r15) * 128, b_off = (wc * 32 + r15) * 128;
    const int c0 = ((0 + kb) ^ swz) * 16, c1 = ((4 + kb) ^ swz) * 16;   // k-steps 0 and 1
    h8 Af[4][2], B0f[2][2], B1f[2][2];
#define VF9_READ_A(SLOTBASE)                                                              \
    _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                        \
        Af[t][0] = *(const h8*)((SLOTBASE) + a_off + t * 2048 + c0);                       \
        Af[t][1] = *(const h8*)((SLOTBASE) + a_off + t * 2048 + c1);                       \
    }
#define VF9_READ_B(DSTF, SLOTBASE)                                                         \
    _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                        \
        DSTF[t][0] = *(const h8*)((SLOTBASE) + b_off + t * 2048 + c0);                     \
        DSTF[t][1] = *(const h8*)((SLOTBASE) + b_off + t * 2048 + c1);                     \
    }
    // operands swapped (W fragment first): block (m-block MQ 4 + t, n-block NQ 2 + u) comes out TRANSPOSED -- lane (r15, kb) holds
    // C[row 16 (MQ 4 + t) + r15][the four columns of n-block NQ 2 + u that MFMA rows 4 kb .. 4 kb + 3 stand for].  Consecutive MFMAs share
    // the W fragment (the FIRST operand) over four A fragments; the other order (VF9_ORDER 0) measured level (profiles/r04_gemm9_k_sweep.log).
#ifndef VF9_ORDER
#define VF9_ORDER 1
#endif
#if VF9_ORDER == 0
#define VF9_QUAD_LOOPS _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) _Pragma("unroll") for (int t = 0; t < 4; ++t) _Pragma("unroll") for (int u = 0; u < 2; ++u)
#else
#define VF9_QUAD_LOOPS _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) _Pragma("unroll") for (int u = 0; u < 2; ++u) _Pragma("unroll") for (int t = 0; t < 4; ++t)
#endif
#define VF9_QUAD(MQ, NQ, BF)                                                               \
    VF9_QUAD_LOOPS                                                                         \
                acc[(MQ) * 4 + t][(NQ) * 2 + u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(BF[u][ks], Af[t][ks], acc[(MQ) * 4 + t][(NQ) * 2 + u], 0, 0, 0);
#define VF9_MID()                                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                     \
    __builtin_amdgcn_s_barrier();                                                          \
    __builtin_amdgcn_sched_barrier(0);                                                     \
    __builtin_amdgcn_s_setprio(1);
#define VF9_TAIL()                                                                         \
    __builtin_amdgcn_s_setprio(0);                                                         \
    __builtin_amdgcn_sched_barrier(0);
    VF9_STAGE(0) VF9_STAGE(1) VF9_STAGE(2) VF9_STAGE(3) VF9_STAGE(0) VF9_STAGE(1) VF9_STAGE(2)
    // DESYNCHRONISE the workgroups.  Tiles take the same time everywhere, so workgroups that start together reach every epilogue
    // together: 256 x 128 KB of stores meet the memory system as one burst.  Spread over a tile's time, a third of the chip writes
    // while two thirds compute and the write-back cache absorbs each tile.  The workgroups with the SMALLER tile count
    // (blockIdx >= ntiles % grid) take their offsets for free: they end before the others anyway (profiles/r04_gemm9_stagger.log).
    if (stagger_ticks > 0) {
        const int rem = ntiles % G_;
        int num = 0, den = 1;
        if (rem != 0) { if (wg >= rem) { num = ((wg - rem) >> 3) + 1; den = ((G_ - rem + 7) >> 3) + 1; } }
        else if (ntiles >= 2 * G_) { num = wg >> 3; den = 2 * ((G_ + 7) >> 3); }       // equal work: half a tile's spread
        const unsigned long long wait = (unsigned long long)stagger_ticks * (unsigned)num / (unsigned)den;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < wait) __builtin_amdgcn_s_sleep(16);
    }
    if (wr == 1) {   // waves 4..7 run one barrier behind, from here to the end of the kernel
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");   // 14 issued, 8 may fly: half-tiles 0 .. 2 of this wave landed
        __builtin_amdgcn_s_barrier();
    }
    unsigned long long* stamps = (unsigned long long*)(smem + PLDS + 2048);   // [16 tiles][6], written by lane 0 of wave 0 (LDS: no vmcnt traffic)
#define VF9_STAMP(SLOT_)                                                                                              \
    if (dbg && wid == 0 && lane == 0 && it < k9StampTiles) stamps[it * k9Stamps + (SLOT_)] = __builtin_amdgcn_s_memrealtime();
    if (dbg && wid == 0) { for (int i = lane; i < k9StampTiles * k9Stamps; i += 64) stamps[i] = 0ull; }
    // ---- the epilogue, straight from the accumulators, in two halves.  Phase X of a K-tile touches only the accumulators of the wave's
    // first 64 rows (acc[0..3]), phase Y only those of its second 64 (acc[4..7]).  BOTH halves of an item's epilogue run in the NEXT
    // item's first K-tile, each in front of the barrier of the phase that is about to overwrite its accumulators: acc[0..3] (final
    // since X of the last K-tile) in front of X(0), acc[4..7] in front of Y(0); each half clears what it has stored (the MFMAs always
    // accumulate in place).  Placements measured (first K-tile of a tile in the steady state, a normal K-tile 1.45 us;
    // profiles/r04_gemm9_*.log): the whole epilogue between two tiles 4.4 us + 2.2 us -- the one-barrier stagger makes the wave halves take
    // turns at it; each half right behind the MFMAs that finish it 4.9 us (it waits for them to drain through the pipe it shares
    // with the other wave half); waves 0..3 behind their MFMAs, waves 4..7 in front of the barrier 5.6 us; this one 5.3 + 2.7 us with
    // the steady K-tile at 1.32 us.  The cost is the stores themselves: a tile's 128 KB leave the CU at ~32 GB/s wherever they are
    // issued.  Threading conversions and stores BETWEEN the 32 MFMAs of a phase would hide them and does not fit the register allocator:
    // 128 accumulators + 64 fragment registers + the half in flight spill 60-120 registers around the block in every arrangement
    // tried (peeled K-tiles, C = 0 starts, opaque zeros), and scratch accesses drain the DMA queue.
    // lane (r15, kb) of block mi holds row wr 128 + mi 16 + r15 and, for hf = 0, 1, the eight columns wc 64 + hf 32 + 8 kb .. + 7:
    // acc[mi][2 hf][0..3], acc[mi][2 hf + 1][0..3].  Residual rows are loaded and consumed in front of the phase's stage DMAs (vmcnt is
    // in order: loads issued behind them would wait for them).
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    h8 rr[4][2];
    unsigned sk_own = 0xffu;   // 16-row blocks this workgroup finishes and stores: all of them, or a split-K slice's share (wave-uniform)
#define VF9_EPI_LOAD_R(MH_, M0_, N0_)                                                                                  \
    if constexpr (EPI == EPI_BIAS_RESIDUAL) {                                                                          \
        _Pragma("unroll") for (int t_ = 0; t_ < 4; ++t_)                                                               \
            _Pragma("unroll") for (int hf_ = 0; hf_ < 2; ++hf_)                                                        \
                if (!SPLIT || ((sk_own >> (4 * (MH_) + t_)) & 1u))                                                      \
                    rr[t_][hf_] = *(const h8*)(R + ((M0_) + wr * 128 + (4 * (MH_) + t_) * 16 + r15) * N + (N0_) + wc * 64 + 8 * kb + hf_ * 32); \
    }
#define VF9_EPI_HALF(MH_, M0_, N0_, PAR_)                                                                              \
    {                                                                                                                  \
        f2v bv_[2][4];                                                                                                 \
        _Pragma("unroll") for (int hf_ = 0; hf_ < 2; ++hf_) {                                                          \
            f4v b0_ = {0.f, 0.f, 0.f, 0.f}, b1_ = b0_;                                                                 \
            if (bias) {                                                                                                \
                const float* bl_ = bias_lds + (PAR_) * 256 + wc * 64 + hf_ * 32 + 8 * kb;                              \
                b0_ = *(const f4v*)bl_; b1_ = *(const f4v*)(bl_ + 4);                                                  \
            }                                                                                                          \
            bv_[hf_][0] = f2v{b0_[0], b0_[1]}; bv_[hf_][1] = f2v{b0_[2], b0_[3]};                                      \
            bv_[hf_][2] = f2v{b1_[0], b1_[1]}; bv_[hf_][3] = f2v{b1_[2], b1_[3]};                                      \
        }                                                                                                              \
        half_t* cbase_ = C + ((M0_) + wr * 128 + (4 * (MH_)) * 16 + r15) * N + (N0_) + wc * 64 + 8 * kb;               \
        _Pragma("unroll") for (int t_ = 0; t_ < 4; ++t_) {                                                             \
            const int mi_ = 4 * (MH_) + t_;                                                                            \
            _Pragma("unroll") for (int hf_ = 0; hf_ < 2; ++hf_) {                                                      \
                u4v o_;                                                                                                \
                _Pragma("unroll") for (int q_ = 0; q_ < 2; ++q_) {                                                     \
                    const f4v a4_ = acc[mi_][2 * hf_ + q_];                                                            \
                    f2v v0_ = f2v{a4_[0], a4_[1]} + bv_[hf_][2 * q_], v1_ = f2v{a4_[2], a4_[3]} + bv_[hf_][2 * q_ + 1]; \
                    if (EPI == EPI_BIAS_GELU) { v0_ = gelu_erf2(v0_); v1_ = gelu_erf2(v1_); }                          \
                    if (EPI == EPI_BIAS_QGELU) { v0_ = quick_gelu2(v0_); v1_ = quick_gelu2(v1_); }                     \
                    h2v p0_ = __builtin_convertvector(v0_, h2v), p1_ = __builtin_convertvector(v1_, h2v);              \
                    if constexpr (EPI == EPI_BIAS_RESIDUAL) {   /* (the LDS-image epilogues round acc + bias to fp16 before the residual joins: same order) */ \
                        const h8 r8_ = rr[t_][hf_];                                                                    \
                        p0_ = __builtin_convertvector(__builtin_convertvector(p0_, f2v) + f2v{(float)r8_[4 * q_ + 0], (float)r8_[4 * q_ + 1]}, h2v); \
                        p1_ = __builtin_convertvector(__builtin_convertvector(p1_, f2v) + f2v{(float)r8_[4 * q_ + 2], (float)r8_[4 * q_ + 3]}, h2v); \
                    }                                                                                                  \
                    o_[2 * q_] = __builtin_bit_cast(unsigned, p0_); o_[2 * q_ + 1] = __builtin_bit_cast(unsigned, p1_); \
                }                                                                                                      \
                if (!SPLIT || ((sk_own >> mi_) & 1u)) *(u4v*)(cbase_ + (long long)t_ * 16 * N + hf_ * 32) = o_;   /* (a split-K slice stores the blocks it owns) */ \
            }                                                                                                          \
            _Pragma("unroll") for (int b_ = 0; b_ < 4; ++b_) acc[mi_][b_] = f4v{0.f, 0.f, 0.f, 0.f};                   \
        }                                                                                                              \
    }
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = f4v{0.f, 0.f, 0.f, 0.f};
    // One loop body for every K-tile (first / second are wave-uniform run-time flags: peeling the first K-tile into a copy of its own let
    // the compiler fold the cleared accumulators into C = 0 MFMAs with fresh destinations, and the allocator spilled).
    long long m0p = 0, n0p = 0;   // the previous item's tile
    int it = 0;
    bool x_pend = false;          // stream-K: the previous item left a tile whose epilogue is due (not so behind a dump)
    for (;; ++it) {
        const long long m0 = (long long)mt_c * PBM, n0 = (long long)nt_c * PBN;
        VF9_STAMP(0)
        for (int kt = 0; kt < nk_c; ++kt) {
            if (kt == 1) { VF9_STAMP(1) }
            if (kt == 2) { VF9_STAMP(2) }
            const char* base = smem + ((ktg + kt) & 1) * (4 * PSLOT);
            const bool pend = STREAMK ? x_pend : it > 0;
            const bool first = kt == 0 && pend, second = kt == 1 && pend;
            // Counted waits (vmcnt is in order and counts the epilogue's stores).  Queue around an item boundary, oldest first:
            // X(last): 2 DMAs | Y(last): 6 DMAs | X(0): 2 DMAs, 8 stores | Y(0): 6 DMAs, 8 stores | X(1): 2 DMAs | Y(1): 6 DMAs ...
            //   X(0) needs the DMAs of X(last): as ever (6);   Y(0) those of Y(last) -> 2 + 8 may fly;   X(1) those of X(0) -> 8 + 6 + 8;
            //   Y(1) those of Y(0) -> 8 + 2 (the first eight stores are older: three phases old);   X(2): as ever (the second eight: three phases).
            // (the residual form stores BEFORE it stages -- X(0): 8 stores, 2 DMAs | Y(0): 8 stores, 6 DMAs -- so X(1) may leave 8 + 6 in
            // flight and Y(1) is as ever)
            if (second) { if constexpr (EPI == EPI_BIAS_RESIDUAL) asm volatile("s_waitcnt vmcnt(14)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(22)" ::: "memory"); }
            else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if constexpr (EPI == EPI_BIAS_RESIDUAL) {   // residual rows first, consumed at once: nothing younger to wait behind, no register held across the stage
                if (!SPLIT && first) { VF9_EPI_LOAD_R(0, m0p, n0p) VF9_EPI_HALF(0, m0p, n0p, (it - 1) & 1) }
                __builtin_amdgcn_sched_barrier(0);
            }
            VF9_STAGE(3)
            if (kt == 0 && wid == 0 && bias) dma16u((unsigned long long)(bias + n0), (unsigned)lane * 16u, lds_smem + (unsigned)PLDS + (unsigned)(it & 1) * 1024u);
            if constexpr (EPI != EPI_BIAS_RESIDUAL) {
                if (!SPLIT && first) { VF9_EPI_HALF(0, m0p, n0p, (it - 1) & 1) }   // (before the fragment reads: their 64 registers are dead here)
                __builtin_amdgcn_sched_barrier(0);
            }
            VF9_READ_B(B0f, base + 1 * PSLOT)
            VF9_READ_B(B1f, base + 2 * PSLOT)
            VF9_READ_A(base + 0 * PSLOT)
            VF9_MID()
            VF9_QUAD(0, 0, B0f)
            VF9_QUAD(0, 1, B1f)
            VF9_TAIL()
            if (first || (second && EPI != EPI_BIAS_RESIDUAL)) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if constexpr (EPI == EPI_BIAS_RESIDUAL) {
                if (!SPLIT && first) { VF9_EPI_LOAD_R(1, m0p, n0p) VF9_EPI_HALF(1, m0p, n0p, (it - 1) & 1) }
                __builtin_amdgcn_sched_barrier(0);
            }
            VF9_STAGE(0)
            VF9_STAGE(1)
            VF9_STAGE(2)
            if constexpr (EPI != EPI_BIAS_RESIDUAL) {
                if (!SPLIT && first) { VF9_EPI_HALF(1, m0p, n0p, (it - 1) & 1) }   // (the A fragments are dead here)
            }
            __builtin_amdgcn_sched_barrier(0);
            VF9_READ_A(base + 3 * PSLOT)
            VF9_MID()
            VF9_QUAD(1, 1, B1f)
            VF9_QUAD(1, 0, B0f)
            VF9_TAIL()
        }
        ktg += nk_c;
        VF9_STAMP(3)
        m0p = m0; n0p = n0;
        if (it + 1 >= n_items) break;
        if (STREAMK) {
            x_pend = true;
            if (it == 0 && x_dump0) {   // the head of a tile other workgroups complete: out with it, and on with cleared accumulators
                x_dump(acc);
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) acc[a][b] = f4v{0.f, 0.f, 0.f, 0.f};
                // waves 4..7 run one barrier behind: wave 0 has seen THEIR stores land once it is through the second of two barriers
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_s_barrier();
                if (tid == 0) x_count();
                x_pend = false;
            }
        }
        item(it + 1, mt_c, nt_c, klo_c, nk_c);
    }
    if (wr == 0) __builtin_amdgcn_s_barrier();   // balance the stagger
    if (STREAMK) {
        if (n_items == 1 && x_dump0) {   // a lone segment that stops short of its tile's end: dump, count, done
            x_dump(acc);                 // (its wait covers the dump-slot DMAs as well)
            __syncthreads();
            if (tid == 0) x_count();
            return;
        }
        {   // a FINISH: the tail of a tile begun by the P workgroups below -- their partials, in ascending K, onto this one's own.
            // (Written without a branch around it -- P = 0 for everybody else -- because a conditional update of the 128
            // accumulators in front of the epilogue made the allocator keep two copies of them: 125-230 registers in scratch.)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the dump-slot DMAs
            __syncthreads();
            const int P = x_P;
            if (tid == 0 && P > 0) {
                unsigned* const w0 = sk.cnt + wg;
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                while (__hip_atomic_load(w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)P) {
                    // cannot happen (the P workgroups were dispatched before this one and dump first); if it ever does, say so and go on
                    if (__builtin_amdgcn_s_memrealtime() - t0 > 200000000ull) { atomicAdd(sk.stat + 3, 1u); break; }
                    __builtin_amdgcn_s_sleep(4);
                }
                __hip_atomic_store(w0, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // for the next launch
            }
            __syncthreads();
            // ((own + lowest) + next ...): a fixed order.  A quarter of a partial (32 registers) per trip.
            constexpr int XB = 2;
            for (int j = P; j >= 1; --j) {
                int off = (wg - 8 * j) * 32 * PTHREADS * 16;   // (the workgroups below on this XCD)
                asm volatile("" : "+s"(off));
#pragma unroll
                for (int b0 = 0; b0 < 8; b0 += XB) {
                    f4v v[XB][4];
#pragma unroll
                    for (int m = 0; m < XB; ++m)
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni)
                            v[m][ni] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(x_rw, tid * 16, off + ((b0 + m) * 4 + ni) * PTHREADS * 16, 16));
#pragma unroll
                    for (int m = 0; m < XB; ++m)
#pragma unroll
                        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[b0 + m][ni][e] += v[m][ni][e];
                }
            }
        }
    }
    if (SPLIT && sk_S > 1) {   // a slice: partials out, partners' partials of the owned blocks in (the dump slot's first bytes are the flag words)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the dump-slot DMAs
        __syncthreads();
        if (sk_coop_finish(acc, sk, sk_tile, sk_slice, sk_own, (unsigned*)(smem + 8 * PSLOT), tid)) return;
    }
    // the last item's epilogue
    VF9_EPI_LOAD_R(0, m0p, n0p)
    VF9_EPI_HALF(0, m0p, n0p, it & 1)
    VF9_EPI_LOAD_R(1, m0p, n0p)
    VF9_EPI_HALF(1, m0p, n0p, it & 1)
    VF9_STAMP(4)
#undef VF9_EPI_HALF
#undef VF9_EPI_LOAD_R
#undef VF9_STAMP
#undef VF9_READ_A
#undef VF9_READ_B
#undef VF9_QUAD
#undef VF9_QUAD_LOOPS
#undef VF9_MID
#undef VF9_TAIL
#undef VF9_STAGE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the dump-slot DMAs
    if (dbg && wid == 0) {                           // every store acknowledged: the workgroup's end; then the stamps leave LDS
        if (lane == 0) stamps[(k9StampTiles - 1) * k9Stamps + 5] = __builtin_amdgcn_s_memrealtime();
        __builtin_amdgcn_s_waitcnt(0);
        for (int i = lane; i < k9StampTiles * k9Stamps; i += 64) dbg[(long long)blockIdx.x * (k9StampTiles * k9Stamps) + i] = stamps[i];
    }
}

// ------------------------------------------------------------------------------------------------
// Fused attention.  grid (ceil(T/128), heads, B), 256 threads; wave w handles queries
// [qb*128 + 32w, +32) of sequence b, head hd; K [T][64] and V^T [64][T] of that (b, head) live in LDS.
// S^T = K Q^T is computed with the KEY on the MFMA row, so a lane holds 16 key scores of ONE query
// (its partner lane + 32 the other 16): softmax reductions are in-lane plus one lane^32 exchange, and
// the probabilities are already the B operand of O^T = V^T P^T (k-slot order (j&3) + 8*(j>>2) + 4*h,
// matched by reading V^T as two 8-byte groups).  Online softmax over 32-key tiles.
// dh = 64, T % 32 == 0, T <= 512.
// ------------------------------------------------------------------------------------------------
constexpr int ADH = 64;
[[maybe_unused]] constexpr int AKLD = ADH + 8, ATHREADS = 512;

// Both 32-lane halves of v in every lane, without an LDS round trip: gfx950's v_permlane32_swap exchanges lanes
// [32, 64) of its first operand with lanes [0, 32) of its second, so two copies of v become (lower half everywhere,
// upper half everywhere).  Written as inline asm on two distinct registers: the compiler builtin, fed the same value
// twice, returned the first result for both (measured), and the instruction needs one wait state after a VALU write.
__device__ __forceinline__ void halves(float v, float& lo, float& hi) {
    float a = v, b = v;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    lo = a;
    hi = b;
}

// weight preparation: the attention kernels take scores in log2 units, so log2(e) / sqrt(dh) is folded into the query
// projection (rows [0, H) of Wqkv and of its bias) once, when the weights are loaded
__global__ void k_scale_half(half_t* __restrict__ w, long long n, float s) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = (half_t)((float)w[i] * s);
}
__global__ void k_scale_float(float* __restrict__ w, long long n, float s) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] *= s;
}

// ------------------------------------------------------------------------------------------------
// k_attention2: resident attention, second generation (dh = 64, T % 32 == 0, T <= 512).
// PERSISTENT workgroups (as many as stay co-resident: one per CU at T = 512), 64 * ceil(T / 64) threads, each walking
// (sequence, head) pairs blockIdx.x, + gridDim.x, ...; wave w owns queries [64w, 64w + 64) as two 32-query blocks (a, b)
// that share every K / V fragment read.  Scores arrive in LOG2 units: the caller has folded log2(e) / sqrt(64) into Q.
//  * K and V of the pair are staged verbatim ([key][64] rows of 128 B) by LDS-DMA; the XOR swizzles live in the
//    per-lane SOURCE address.  K: chunk ^ ((key >> 1) & 7) -- the ds_read_b128 A-operand reads of 32 keys are
//    conflict-free.  V: chunk ^ (((key >> 1) & 1) << 2) -- the 4-key x 16-dh blocks of ds_read_b64_tr_b16 (which
//    delivers V^T fragments without a transposing staging pass) are.
//  * Next-pair prefetch: the key range is cut into chunks of 128 keys; once every wave has left a chunk (one barrier per
//    chunk) its LDS rows are refilled with the NEXT pair's keys, so staging runs under the tile loop instead of in front
//    of it.  Fully masked chunks are neither staged nor visited.  (a2_dma16 and the pair loop say what it takes to keep
//    the compiler's own s_waitcnt vmcnt(0) out of the tile loop.)
//  * S^T = K Q^T with the key on the MFMA row (a lane owns 16 scores of one query).  The running reference maximum
//    m_ref AND the key padding mask enter through the matrix pipe as a fifth k-step (A = (1, mask_key), B = (-m_ref, 1),
//    m_ref kept fp16-representable so the products are exact): the scores come out already masked and relative to
//    m_ref, and p = exp2(s) needs no per-element arithmetic.  (As the MFMA's initial accumulator the same bias costs 16
//    register copies per tile.)
//  * Lazy maximum: m_ref moves only when a probability overflows fp16, which the (infinite) row sum reveals; the
//    rescale of O, l and the bias fragment is a rare wave-uniform branch.  l is kept per lane (its half of the keys)
//    and combined once at the end.
//  * In-wave software pipeline (a2_phase): the two query blocks run half a tile apart; each phase issues one block's
//    nine MFMAs with the other block's softmax in the gaps.
//  * O is staged 16 queries at a time through the wave's own 2 KiB of LDS and stored as whole 128-byte rows.
// Cost anatomy (tools/attention_clock.py, tools/ubench/issue_cost.hip): the loop is bound by vector ISSUE, not by the
// matrix pipe -- v_exp_f32 13.9 cycles, v_dot2c 7.5, v_cvt_pk 4, an MFMA's issue 8 of its 32 -- about 800 cycles per
// (64 queries x 32 keys) against 576 of MFMA time.
// ------------------------------------------------------------------------------------------------
typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
constexpr float A2_THR = 8.0f;

__device__ __forceinline__ int a2_koff(int row, int ch) { return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int a2_voff(int row, int ch) { return row * 128 + ((ch ^ (((row >> 1) & 1) << 2)) << 4); }

__device__ __forceinline__ void a2_tr_read(h8& dst, const char* lo, const char* hi) {
    const fp16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)lo);
    const fp16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)hi);
#pragma unroll
    for (int e = 0; e < 4; ++e) { dst[e] = (half_t)a[e]; dst[4 + e] = (half_t)b[e]; }
}

// the rare path: move the reference maximum of one query block (first tile: to the tile's maximum; later: up to the
// maximum of the queries whose scores ran more than A2_THR ahead of it) and bring s, O, l and the bias fragment to the
// new reference.  m_ref stays representable in fp16, so the bias k-step (1 x -m_ref, fp32 accumulation) subtracts it exactly.
__device__ __forceinline__ void a2_move_ref(f16v& s, f16v (&o)[2], float& l, float& mref, h8& mq, bool first, int h) {
    float tmax = s[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) tmax = fmaxf(tmax, s[e]);
    {
        float lo, hi;
        halves(tmax, lo, hi);
        tmax = fmaxf(lo, hi);
    }
    const float want = mref + (first ? tmax : (tmax > A2_THR ? tmax : 0.f));
    const float mnew = (float)(half_t)fminf(fmaxf(want, -60000.f), 60000.f);
    const float delta = mnew - mref;
    const float alpha = first ? 1.f : __builtin_amdgcn_exp2f(-delta);
    mref = mnew;
    l *= alpha;
    mq[0] = h == 0 ? (half_t)(-mnew) : (half_t)0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        s[e] -= delta;
        o[0][e] *= alpha;
        o[1][e] *= alpha;
    }
}

// p = exp2(s) -> fp16 B-operand fragments; returns the lane's partial row sum, taken over the ROUNDED probabilities
// (v_dot2_f32_f16 against (1, 1)), so that O / l is a weighted mean with consistently perturbed weights: a dominant
// key then reproduces its value row exactly, as it does when the largest probability is exactly 1.  A probability
// past the fp16 range makes the sum infinite: the overflow signal that moves the reference (a2_move_ref).
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float a2_probs(const f16v& s, h8 (&pf)[2]) {
    const h2 one2 = {(half_t)1.f, (half_t)1.f};
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int e = 0; e < 16; e += 4) {
        const h2 p01 = {(half_t)__builtin_amdgcn_exp2f(s[e]), (half_t)__builtin_amdgcn_exp2f(s[e + 1])};
        const h2 p23 = {(half_t)__builtin_amdgcn_exp2f(s[e + 2]), (half_t)__builtin_amdgcn_exp2f(s[e + 3])};
        s0 = __builtin_amdgcn_fdot2(p01, one2, s0, false);
        s1 = __builtin_amdgcn_fdot2(p23, one2, s1, false);
        pf[e >> 3][e & 7] = p01[0];
        pf[e >> 3][(e & 7) + 1] = p01[1];
        pf[e >> 3][(e & 7) + 2] = p23[0];
        pf[e >> 3][(e & 7) + 3] = p23[1];
    }
    return s0 + s1;
}

// ---- in-wave software pipeline -------------------------------------------------------------------------------
// Two waves of a SIMD do NOT fill each other's matrix-pipe gaps here (measured: the loop ran as long as its MFMA time
// plus its VALU time; a wave whose next MFMA waits for the pipe keeps the issue slot).  The overlap has to be inside
// one wave's instruction stream: the two query blocks run half a tile apart, and each phase issues one block's nine
// MFMAs (P.V of this tile, then the bias step and QK^T of the next tile) with the OTHER block's softmax spread over
// the gaps -- two v_exp, one pack, one row-sum step per MFMA.
//   phase A(i): MFMA  P.V(a, i), QK(a, i+1)      VALU  probabilities(b, i)      then the overflow check of b
//   phase B(i): MFMA  P.V(b, i), QK(b, i+1)      VALU  probabilities(a, i+1)    then the overflow check of a
// The key padding mask rides the bias k-step (A = (1, mask_key), B = (-m_ref, 1)): no branch, no per-score arithmetic.

// half of a slice: two scores -> exp2 -> one packed pair -> row-sum step
#define A2_HALF_SLICE(S, PF, ACC, E)                                                                                   \
    {                                                                                                                  \
        const h2 p_ = {(half_t)__builtin_amdgcn_exp2f(S[E]), (half_t)__builtin_amdgcn_exp2f(S[(E) + 1])};             \
        ACC = __builtin_amdgcn_fdot2(p_, one2, ACC, false);                                                            \
        PF[(E) >> 3][(E) & 7] = p_[0];                                                                                 \
        PF[(E) >> 3][((E) & 7) + 1] = p_[1];                                                                           \
    }

// One phase.  MFMA: o += V^T(vf) . P(pv_p) for this tile [4], then (QK) s_next = bias + K(kf) . Q(q) for the next
// tile [5].  VALU: pr_p = exp2(pr_s), returns the lane's partial row sum.
template <bool QK>
__device__ __forceinline__ float a2_phase(f16v (&o)[2], const h8 (&pv_p)[2], const h8 (&vf)[2][2], f16v& s_next, const h8 (&kf)[4],
                                          const h8 (&q)[4], const h8& ba, const h8& mq, const f16v& pr_s, h8 (&pr_p)[2]) {
    const h2 one2 = {(half_t)1.f, (half_t)1.f};
    float s0 = 0.f, s1 = 0.f;
    f16v zero;
#pragma unroll
    for (int e = 0; e < 16; ++e) zero[e] = 0.f;
    o[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[0][0], pv_p[0], o[0], 0, 0, 0);
    A2_HALF_SLICE(pr_s, pr_p, s0, 0)
    o[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[0][1], pv_p[0], o[1], 0, 0, 0);
    A2_HALF_SLICE(pr_s, pr_p, s1, 2)
    o[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[1][0], pv_p[1], o[0], 0, 0, 0);
    A2_HALF_SLICE(pr_s, pr_p, s0, 4)
    o[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[1][1], pv_p[1], o[1], 0, 0, 0);
    A2_HALF_SLICE(pr_s, pr_p, s1, 6)
    if (QK) s_next = __builtin_amdgcn_mfma_f32_32x32x16_f16(ba, mq, zero, 0, 0, 0);
    A2_HALF_SLICE(pr_s, pr_p, s0, 8)
    if (QK) s_next = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[0], q[0], s_next, 0, 0, 0);
    A2_HALF_SLICE(pr_s, pr_p, s1, 10)
    if (QK) s_next = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[1], q[1], s_next, 0, 0, 0);
    A2_HALF_SLICE(pr_s, pr_p, s0, 12)
    if (QK) s_next = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[2], q[2], s_next, 0, 0, 0);
    A2_HALF_SLICE(pr_s, pr_p, s1, 14)
    if (QK) s_next = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[3], q[3], s_next, 0, 0, 0);
    // one MFMA, two transcendentals, two other vector ops per gap
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
    }
    return s0 + s1;
}

// the bias k-step's A operand for key tile kt: (1, mask_key) in the h = 0 lanes (mh[key] = packed {1.0h, 0 or -30000h})
__device__ __forceinline__ h8 a2_bias_a(const unsigned* mh, int kt, int r31, int h) {
    const unsigned w = h == 0 ? mh[kt * 32 + r31] : 0u;
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    const u4v v = {w, 0u, 0u, 0u};
    h8 r;
    __builtin_memcpy(&r, &v, 16);
    return r;
}

__device__ __forceinline__ void a2_read_k(h8 (&kf)[4], const char* Ks, int kt, int r31, int h) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const h8*)(Ks + a2_koff(kt * 32 + r31, 2 * ks + h));
}

// V^T fragments of key tile kt: k-slot j of half h <-> key 16 st + (j & 3) + 8 (j >> 2) + 4 h.  Transposed read: lane
// 4q + p of its 16-lane group addresses key (base + q), dh chunk 4 mt + 2 (group & 1) + (p >> 1), byte 8 (p & 1).
__device__ __forceinline__ void a2_read_v(h8 (&vf)[2][2], const char* Vs, int kt, int lane) {
    const int h = lane >> 5, vq = (lane >> 2) & 3, vp = lane & 3, vg = (lane >> 4) & 1;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int key = kt * 32 + 16 * st + 4 * h + vq, ch = 4 * mt + 2 * vg + (vp >> 1);
            a2_tr_read(vf[st][mt], Vs + a2_voff(key, ch) + 8 * (vp & 1), Vs + a2_voff(key + 8, ch) + 8 * (vp & 1));
        }
}

// 16 bytes per lane global -> LDS (lds: wave-uniform base, lane i lands at base + 16 i), as inline asm ON PURPOSE.  With the
// builtin the compiler knows an LDS-DMA is pending and, unable to prove that a later LDS read does not alias it, puts
// s_waitcnt vmcnt(0) in front of every ds_read -- in k_attention2's tile loop that drains the next pair's prefetch at
// every tile (measured: +45 % loop time).  Here the kernel orders DMA against reads itself (vmcnt(0) + barrier at the
// chunk boundaries).  M0 is saved and restored around the transfer.
__device__ __forceinline__ void a2_dma16(const void* g, const char* lds) {
    const unsigned base = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)lds;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(base)
                 : "memory");
}

// O of one 16-query group of a block: the owning lanes write their 8 x 8 bytes into the wave's 2 KiB staging rows
// (swizzled like K), then every lane moves 32 bytes of whole rows to global memory
__device__ __forceinline__ void a2_store_group(const f16v (&o)[2], float inv, int hh, char* Os, half_t* dst_rows, int H, int nrows,
                                               int lane) {
    const int r31 = lane & 31, h = lane >> 5;
    if ((r31 >> 4) == hh) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                h4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (half_t)(o[mt][g4 * 4 + e] * inv);
                // dh = 32 mt + 8 g4 + 4 h + e  ->  chunk 4 mt + g4, byte 8 h
                *(h4*)(Os + a2_koff(r31 & 15, 4 * mt + g4) + 8 * h) = v;
            }
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int c = lane + 64 * it, row = c >> 3, ch = c & 7;
        const uint4 v = *(const uint4*)(Os + a2_koff(row, ch));
        if (row < nrows) *(uint4*)(dst_rows + (long long)row * H + ch * 8) = v;
    }
}

// MODE 0: the kernel; 6: diagnostic build that also appends per-wave clock stamps after ctx (tools/attention_clock.py).
// seq_off != nullptr: PACKED sequences -- sequence b occupies rows [seq_off[b], seq_off[b + 1]) of qkv / mask / ctx (its
// length rounded up to 32; T is then the longest, which sizes LDS and the workgroup).  Pairs differ in length: a wave
// whose queries lie past the pair's end sits the pair out but keeps every barrier, and the chunk hand-over below works
// with the two pairs' own chunk counts.
template <int MODE>
__global__ __launch_bounds__(512) void k_attention2(const half_t* __restrict__ qkv, const int* __restrict__ mask, int B, int T, int H,
                                                    int ct, const int* __restrict__ seq_off, half_t* __restrict__ ctx, int nsplit) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ks = smem;                                  // [T] rows of 128 B, swizzled (a2_koff)
    char* Vs = smem + (size_t)T * 128;                // [T] rows of 128 B, swizzled (a2_voff)
    unsigned* mbuf = (unsigned*)(Vs + (size_t)T * 128);   // [2][T] packed {1.0h, mask_h}: this pair's and the next one's
    const int tid = threadIdx.x, lane = tid & 63, nthreads = blockDim.x;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* Os = (char*)(mbuf + 2 * T) + wid * 2048;    // the wave's O staging rows
    const int r31 = lane & 31, h = lane >> 5;
    const int heads = H / ADH, npairs = B * heads, ld = 3 * H;
    const int cts = ct == 16 ? 4 : ct == 8 ? 3 : 2;                  // ct: tiles per chunk (4, 8 or 16) = 1 << cts
    const unsigned cmask = ct >= 32 ? 0xffffffffu : ((1u << ct) - 1u);
    const unsigned MASK_ON = 0x00003c00u, MASK_OFF = 0xf7533c00u;   // {1.0h, 0h} / {1.0h, -30000h}
    constexpr int ALL_PUBLISHED = 1 << 20;
    // Round 5: the LAST nsplit pairs are walked as two HALF items each -- the same keys and values staged, the first half of the
    // workgroup's waves active in one, the second half in the other -- so that the partial last round of a batch (300 pairs on 256
    // CUs: 44 of them alone on the chip for a whole pair's time) runs one wave per SIMD on twice the CUs, in little more than half
    // the time.  An item index vp < npairs - nsplit is that pair; beyond, pair (npairs - nsplit) + (vp - ...) / 2, half (vp - ...) & 1.
    const int nfullp = npairs - nsplit, nitems = npairs + nsplit, hwaves = (int)(blockDim.x >> 7);
    auto pair_of = [&](int v) { return v < nfullp ? v : nfullp + ((v - nfullp) >> 1); };
    auto wave_on = [&](int v) { return v < nfullp || (wid >= hwaves) == (bool)((v - nfullp) & 1); };
    int vp = blockIdx.x;
    if (vp >= nitems) return;
    int pair = pair_of(vp);
    unsigned long long tk_start = 0, rt_start = 0;
    if (MODE == 6) { tk_start = __builtin_amdgcn_s_memtime(); rt_start = __builtin_amdgcn_s_memrealtime(); }

    // first row and length of pair p's sequence
    auto seq_of = [&](int p, long long& row0, int& Tb) {
        const int b = p / heads;
        if (seq_off) {
            const int o0 = seq_off[b], o1 = seq_off[b + 1];
            row0 = o0;
            Tb = o1 - o0;
        } else {
            row0 = (long long)b * T;
            Tb = T;
        }
    };
    // 16-byte chunk c of an image <- key c >> 3, source chunk (c & 7) ^ swizzle(key); a wave-instruction fills 1 KiB (8 keys)
    auto stage_chunk = [&](long long prow, int Tb, int hd, int g) {
        const half_t* Kg = qkv + prow * ld + H + hd * ADH;
        const half_t* Vg = Kg + H;
        const int cper = ct * 256;   // 16-byte pieces per chunk and image
        const int cend = (g + 1) * cper < Tb * 8 ? (g + 1) * cper : Tb * 8;
        for (int c0 = g * cper + wid * 64; c0 < cend; c0 += nthreads) {
            const int c = c0 + lane, key = c >> 3, chp = c & 7;
            const half_t* ks = Kg + (long long)key * ld + ((chp ^ ((key >> 1) & 7)) << 3);
            const half_t* vs = Vg + (long long)key * ld + ((chp ^ (((key >> 1) & 1) << 2)) << 3);
            a2_dma16(ks, Ks + c0 * 16);
            a2_dma16(vs, Vs + c0 * 16);
        }
    };
    // tile classes (bit j = 32-key tile j has a valid key); a sequence without any valid key keeps every tile
    auto classify = [&](const unsigned* mh, int ntl) {
        unsigned act = 0;
        for (int j = 0; j < ntl; ++j) act |= (__ballot((mh[j * 32 + r31] >> 16) == 0u) != 0ull ? 1u : 0u) << j;
        return act ? act : (ntl >= 32 ? 0xffffffffu : ((1u << ntl) - 1u));
    };
    // Q fragments (B operand) of both query blocks: lane (query r31, half h) holds q[8h + j + 16 ks].  A query past the
    // end of the sequence re-reads its last one (computed, never stored).
    const int qa0 = wid * 64, qb0 = qa0 + 32;
    h8 qa[4], qb[4];
    auto load_q = [&](long long prow, int Tb, int hd) {
        const int ra = qa0 + r31 < Tb ? qa0 + r31 : Tb - 1, rb = qb0 + r31 < Tb ? qb0 + r31 : Tb - 1;
        const half_t* Qa = qkv + (prow + ra) * ld + hd * ADH + h * 8;
        const half_t* Qb = qkv + (prow + rb) * ld + hd * ADH + h * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qa[ks] = *(const h8*)(Qa + ks * 16);
            qb[ks] = *(const h8*)(Qb + ks * 16);
        }
    };

    long long row0, row0n = 0;
    int Tb, Tbn = 0;
    seq_of(pair, row0, Tb);
    // ---- first pair: its first chunk (and the mask of the second pair), waited for; the other chunks are issued right
    //      behind the barrier and land under the first chunk's tiles (published by the first boundary, or on demand)
    stage_chunk(row0, Tb, pair % heads, 0);
    if (tid < Tb) mbuf[tid] = mask[row0 + tid] ? MASK_ON : MASK_OFF;
    if (vp + (int)gridDim.x < nitems) {
        seq_of(pair_of(vp + gridDim.x), row0n, Tbn);
        if (tid < Tbn) mbuf[T + tid] = mask[row0n + tid] ? MASK_ON : MASK_OFF;
    }
    load_q(row0, Tb, pair % heads);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    __syncthreads();
    for (int g = 1; g < (((Tb >> 5) + ct - 1) >> cts); ++g) stage_chunk(row0, Tb, pair % heads, g);
    unsigned act = classify(mbuf, Tb >> 5);
    int pub_from = 1;                      // chunks >= pub_from are not yet known to have landed (no barrier published them)
    unsigned long long tk_loop = 0, tk_tail = 0, tk_bar = 0;

    // Pair loop.  No vector-memory LOAD with a register destination is pending while tiles run: the wait the compiler
    // places before such a register's first use is vmcnt(0) -- the counter is in order -- and inside the tile loop
    // that would drain the LDS-DMA prefetch at every tile.  The next pair's Q fragments and the mask of the pair after
    // it are therefore loaded in the quiet window at the pair's end (after the closing barrier, nothing else in flight)
    // and settled there, under the O epilogue.
    for (int cur = 0;; cur ^= 1) {
        const int nxt_vp = vp + gridDim.x, nxt2_vp = nxt_vp + gridDim.x;
        const bool has_next = nxt_vp < nitems;
        const int nxt_pair = pair_of(nxt_vp), nxt2_pair = pair_of(nxt2_vp);
        const int hd = pair % heads, hdn = nxt_pair % heads;
        const int nchunks = ((Tb >> 5) + ct - 1) >> cts;            // of this pair
        const int nchunks_n = has_next ? (((Tbn >> 5) + ct - 1) >> cts) : 0;
        const bool wact = qa0 < Tb && wave_on(vp);                  // this wave has queries in this pair (and, of a half item, in its half)
        const unsigned* mh = mbuf + cur * T;
        const unsigned* mhn = mbuf + (cur ^ 1) * T;
        unsigned act_n = 0;
        int g_nb = 0;                      // next inner chunk boundary to run
        // An inner boundary: every wave has left chunk g (and every LDS read of it has returned); the transfers issued a
        // chunk ago have landed.  After the barrier the chunk's rows take the NEXT pair's keys (LDS-DMA, in flight under
        // the following chunks).
        auto boundary = [&](int g) {
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
            __syncthreads();
            pub_from = ALL_PUBLISHED;
            if (has_next) {
                if (g == 0) act_n = classify(mhn, Tbn >> 5);        // the next pair's mask: written a pair ago
                if (g < nchunks_n && ((act_n >> (ct * g)) & cmask)) stage_chunk(row0n, Tbn, hdn, g);
            }
        };
        // reads may run ahead of the boundaries, but not into a chunk that no barrier has published yet
        auto publish_for = [&](int tile) {
            if ((tile >> cts) >= pub_from) {
                __builtin_amdgcn_s_waitcnt(0x0F70);
                __syncthreads();
                pub_from = ALL_PUBLISHED;
            }
        };
        unsigned long long t0 = 0;
        if (MODE == 6) t0 = __builtin_amdgcn_s_memtime();

        f16v oa[2], ob[2], sa, sb, zero;
#pragma unroll
        for (int e = 0; e < 16; ++e) oa[0][e] = oa[1][e] = ob[0][e] = ob[1][e] = zero[e] = 0.f;
        // the bias k-step's B operand: (-m_ref, 1, 0, ...) per query, in the h = 0 lanes
        h8 mqa, mqb;
#pragma unroll
        for (int e = 0; e < 8; ++e) mqa[e] = mqb[e] = (half_t)0.f;
        mqa[1] = mqb[1] = h == 0 ? (half_t)1.f : (half_t)0.f;
        float la = 0.f, lb = 0.f, mra = 0.f, mrb = 0.f;
        h8 pa[2], pb[2], vf[2][2], kf[4], ba;

        // ---- prologue of the pipeline: scores of the first active tile for both blocks, references, a's probabilities
        unsigned rest = act;
        int t = __builtin_ctz(rest);
        rest &= rest - 1;
        int tn = rest ? __builtin_ctz(rest) : -1;
        publish_for(t);
        if (tn >= 0) publish_for(tn);
        if (wact) {
            a2_read_k(kf, Ks, t, r31, h);
            ba = a2_bias_a(mh, t, r31, h);
            a2_read_v(vf, Vs, t, lane);
            sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ba, mqa, zero, 0, 0, 0);
            sb = __builtin_amdgcn_mfma_f32_32x32x16_f16(ba, mqb, zero, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                sa = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qa[ks], sa, 0, 0, 0);
                sb = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[ks], qb[ks], sb, 0, 0, 0);
            }
            if (tn >= 0) {
                a2_read_k(kf, Ks, tn, r31, h);
                ba = a2_bias_a(mh, tn, r31, h);
            }
            a2_move_ref(sa, oa, la, mra, mqa, true, h);
            a2_move_ref(sb, ob, lb, mrb, mqb, true, h);
            la += a2_probs(sa, pa);
        }
        // ---- steady state: here pa(t), sb(t), vf(t) are ready, and kf / ba hold tile tn
        while (tn >= 0) {
            rest &= rest - 1;
            const int tn2 = rest ? __builtin_ctz(rest) : -1;
            if (tn2 >= 0) publish_for(tn2);
            if (wact) {
                // phase A: P.V(a, t), QK(a, tn)  ||  probabilities(b, t)
                float sum = a2_phase<true>(oa, pa, vf, sa, kf, qa, ba, mqa, sb, pb);
                if (__ballot(!(sum < 1e30f)) != 0ull) {
                    a2_move_ref(sb, ob, lb, mrb, mqb, false, h);
                    sum = a2_probs(sb, pb);
                }
                lb += sum;
                // phase B: P.V(b, t), QK(b, tn)  ||  probabilities(a, tn); then the fragment reads of the tiles ahead
                sum = a2_phase<true>(ob, pb, vf, sb, kf, qb, ba, mqb, sa, pa);
                a2_read_v(vf, Vs, tn, lane);
                if (tn2 >= 0) {
                    a2_read_k(kf, Ks, tn2, r31, h);
                    ba = a2_bias_a(mh, tn2, r31, h);
                }
                if (__ballot(!(sum < 1e30f)) != 0ull) {
                    a2_move_ref(sa, oa, la, mra, mqa, false, h);
                    sum = a2_probs(sa, pa);
                }
                la += sum;
            }
            // chunk boundaries between tile t and tile tn
            while (g_nb < (tn >> cts)) boundary(g_nb++);
            t = tn;
            tn = tn2;
        }
        // ---- drain: P.V(a, t) || probabilities(b, t), then P.V(b, t)
        if (wact) {
            float sum = a2_phase<false>(oa, pa, vf, sa, kf, qa, ba, mqa, sb, pb);
            if (__ballot(!(sum < 1e30f)) != 0ull) {
                a2_move_ref(sb, ob, lb, mrb, mqb, false, h);
                sum = a2_probs(sb, pb);
            }
            lb += sum;
#pragma unroll
            for (int st = 0; st < 2; ++st)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) ob[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf[st][mt], pb[st], ob[mt], 0, 0, 0);
        }
        while (g_nb < nchunks - 1) boundary(g_nb++);
        unsigned long long t1 = 0;
        if (MODE == 6) { t1 = __builtin_amdgcn_s_memtime(); tk_loop += t1 - t0; }
        int rmask = 1;
        long long row0n2 = 0;
        int Tbn2 = 0;
        if (has_next) {
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
            __syncthreads();                                        // the pair is done in every wave
            if (MODE == 6) tk_bar += __builtin_amdgcn_s_memtime() - t1;
            if (nchunks == 1) act_n = classify(mhn, Tbn >> 5);
            load_q(row0n, Tbn, hdn);                                // quiet window: nothing else in flight
            if (nxt2_vp < nitems) {
                seq_of(nxt2_pair, row0n2, Tbn2);
                if (tid < Tbn2) rmask = mask[row0n2 + tid];
            }
        }
        // ---- O: normalise (the halves' partial row sums combine here), stage 16 queries at a time, store whole rows
        if (wact) {
            float inva, invb;
            {
                float lo, hi;
                halves(la, lo, hi);
                inva = 1.0f / (lo + hi);
                halves(lb, lo, hi);
                invb = 1.0f / (lo + hi);
            }
            half_t* dst = ctx + (row0 + qa0) * H + hd * ADH;
            const int nrows = Tb - qa0;   // >= 32
            a2_store_group(oa, inva, 0, Os, dst, H, nrows, lane);
            a2_store_group(oa, inva, 1, Os, dst + 16LL * H, H, nrows - 16, lane);
            a2_store_group(ob, invb, 0, Os, dst + 32LL * H, H, nrows - 32, lane);
            a2_store_group(ob, invb, 1, Os, dst + 48LL * H, H, nrows - 48, lane);
        }
        if (MODE == 6) {
            tk_tail += __builtin_amdgcn_s_memtime() - t1;
            if (!has_next && lane == 0) {
                unsigned long long* out = (unsigned long long*)(ctx + (long long)B * T * H) + ((long long)blockIdx.x * 8 + wid) * 8;
                out[0] = tk_bar; out[1] = tk_loop; out[2] = tk_tail;
                out[3] = __builtin_amdgcn_s_memtime() - tk_start;
                out[4] = __builtin_amdgcn_s_memrealtime() - rt_start;
                out[5] = (unsigned long long)(vp / gridDim.x + 1);
                out[6] = rt_start;
                out[7] = __builtin_amdgcn_s_memrealtime();
            }
        }
        // Settle the window's loads here: a real S_WAITCNT (the builtin), which the compiler's own wait insertion accounts
        // for -- and BEFORE the loop exit, because the structurised control flow routes the exit through the loop
        // header's predecessor: a load still pending on the exit path would put the waits back into the tile loop.
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
        asm volatile("" : "+v"(rmask));       // (keeps the mask's compare-and-select below the wait)
        if (!has_next) break;
        if (nxt2_vp < nitems && tid < Tbn2) mbuf[cur * T + tid] = rmask ? MASK_ON : MASK_OFF;   // read (as mhn) after a barrier of the next pair
        // the pair's last chunk, and the chunks only the next pair has, refill now
        for (int g = nchunks - 1; g < nchunks_n; ++g)
            if ((act_n >> (ct * g)) & cmask) stage_chunk(row0n, Tbn, hdn, g);
        pub_from = nchunks - 1;
        if (nchunks == 1) {   // a single chunk: the refill must land before the next pair starts
            __builtin_amdgcn_s_waitcnt(0x0F70);
            __syncthreads();
            pub_from = ALL_PUBLISHED;
        }
        vp = nxt_vp;
        pair = nxt_pair;
        act = act_n;
        row0 = row0n;
        Tb = Tbn;
        row0n = row0n2;
        Tbn = Tbn2;
    }
}

// ------------------------------------------------------------------------------------------------
// k_attention_stream<DH, CAUSAL>: the same fused attention with K / V STREAMED through LDS in 64-key tiles instead of
// held whole (head dim 128 with T = 512 would need 270 KB; and a 37 KB workgroup lets four share a CU).
// grid (ceil(T / 128), heads, B), 256 threads = 4 waves, wave w owns queries [qb*128 + 32w, +32).  Grouped-query
// attention: head hd reads K / V of kv head hd / (heads / kv_heads).  Per tile: the next tile's K rows and V block
// (transposed in registers) are fetched into registers before the current tile is consumed and written to the other
// LDS buffer afterwards -- one barrier per tile.  S^T = K Q^T as in k_attention (a lane owns one query's scores),
// two 32-key score tiles per iteration share one max / exchange / rescale.  CAUSAL: tiles past the workgroup's
// last query are never visited, tiles past a wave's last query are skipped by that wave (it still stages), the
// diagonal tile is masked per element.  Key padding mask as in k_attention (additive -30000).
// qkv rows: [q (heads*DH) | k (kv_heads*DH) | v (kv_heads*DH)], row stride ld.  T % 32 == 0.
// ------------------------------------------------------------------------------------------------
constexpr int SKT = 64;  // keys per tile

// (This first, register-staged generation of the streaming kernel was deleted in round 4; k_attention_stream2 below is the kernel that
// runs.  The description above is kept because the tile loop, the online softmax and the masks are the ones it introduced.)

// ------------------------------------------------------------------------------------------------
// k_attention_stream2<CAUSAL>: k_attention_stream at head dim 128 with the operand path of k_attention2 -- K and V tiles
// go global -> LDS VERBATIM by LDS-DMA (no register staging, no 8 x 8 register transposes by the first two waves, 48
// fewer live registers), 256-byte rows whose 16-byte chunks are XOR-swizzled through the SOURCE addresses of the DMA
// lanes: K chunk c of row r sits at c ^ (r & 15) (a ds_read_b128 lane group = 16 rows at one logical chunk -> 16 distinct
// slots), V chunk c at c ^ ((r & 3) << 2) (a transposing read's 32-lane half covers 4 keys x 64 B -> 4 distinct 64-byte
// groups).  V^T fragments come from ds_read_b64_tr_b16 (a2_tr_read) in the key order the score tiles already have.
// Everything else (tile loop, one barrier per 64-key tile, online softmax, causal / padding masks, packed rows) is
// k_attention_stream's.
// ------------------------------------------------------------------------------------------------
// Head dim 128: 64-key tiles; head dim 256 (gemma): 32-key tiles, the wave's Q fragments in registers (64 of them) instead
// of a 66 KB LDS tile, so that two workgroups share a CU (the register-staged kernel it replaces: one workgroup, one wave
// per SIMD, two LDS reads per QK^T MFMA -- 0.13 PFLOP/s); head dim 64 (the encoder beyond 512 tokens: bge-m3 documents):
// 128-key tiles of 128-byte rows with k_attention2's swizzles.  A tile is 16 KB of K and 16 KB of V in every case.
template <int DH>
struct AttnStream2Lds {
    static constexpr int KT = DH == 256 ? 32 : DH == 128 ? 64 : 128;
    char k[2][KT * DH * 2];
    char v[2][KT * DH * 2];
    float mb[2][KT];
    int padded[2][2];    // per buffer and staging wave: the wave's keys hold a masked one (or run past the sequence's end)
};
// chunk swizzles (16-byte chunks of a row): rows of 256 / 512 bytes sit on the same banks, rows of 128 bytes alternate
template <int DH> __device__ __forceinline__ int s2_kswz(int row) { return DH == 64 ? (row >> 1) & 7 : row & 15; }
template <int DH> __device__ __forceinline__ int s2_vswz(int row) { return DH == 64 ? ((row >> 1) & 1) << 2 : (row & 3) << 2; }
template <int DH> __device__ __forceinline__ int s2_koff(int row, int ch) { return row * (DH * 2) + ((ch ^ s2_kswz<DH>(row)) << 4); }
template <int DH> __device__ __forceinline__ int s2_voff(int row, int ch) { return row * (DH * 2) + ((ch ^ s2_vswz<DH>(row)) << 4); }

template <int DH, bool CAUSAL>
__global__ __launch_bounds__(256, 2) void k_attention_stream2(const half_t* __restrict__ qkv, const int* __restrict__ mask, int Targ,
                                                            int ld, int heads, int kv_heads, float scale,
                                                            half_t* __restrict__ ctx, int ctx_ld, const int* __restrict__ seq_off = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    AttnStream2Lds<DH>& L = *reinterpret_cast<AttnStream2Lds<DH>*>(smem);
    constexpr int KS = DH / 16, MT = DH / 32, KT = AttnStream2Lds<DH>::KT, NS = KT / 32, CPR = DH / 8;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r31 = lane & 31, h = lane >> 5;
    const int qb = blockIdx.x, hd = blockIdx.y, b = blockIdx.z;
    const int hk = hd / (heads / kv_heads);
    const long long row0 = seq_off ? (long long)seq_off[b] : (long long)b * Targ;
    const int T = seq_off ? seq_off[b + 1] - seq_off[b] : Targ;
    if (qb * 128 >= T) return;
    const int q_dim = heads * DH, kv_dim = kv_heads * DH;
    const half_t* Kg = qkv + row0 * ld + q_dim + hk * DH;
    const half_t* Vg = qkv + row0 * ld + q_dim + kv_dim + hk * DH;
    const int q0 = qb * 128 + wid * 32;
    const bool wave_active = q0 < T;
    const int last_q = (qb * 128 + 127 < T - 1) ? qb * 128 + 127 : T - 1;
    const int ntiles = CAUSAL ? (last_q / KT + 1) : (T + KT - 1) / KT;
    // ---- staging: a tile of K (and of V) is 1024 chunks of 16 B; DMA round j of thread t fills physical chunk t + 256 j
    //      = row t / CPR + (256 / CPR) j, slot t % CPR, with the LOGICAL chunk that the swizzle puts there
    const int srow = tid / CPR, slot = tid % CPR;
    constexpr int RSTEP = 256 / CPR;      // rows between a thread's DMA rounds: 16 (head dim 128) or 8 (256)
    float rmb = 0.f;
    // The source address of a DMA is a SCALAR base (the sequence's K / V column block) + a 32-bit lane offset, recomputed per tile from
    // the key index (a sequence is <= 4096 rows of <= 64 KB: the offset fits 32 bits).  As eight 64-bit per-lane pointers the compiler
    // kept them -- loop invariants -- across the tile loop, and at head dim 256 (128 output accumulators + 64 query-fragment registers:
    // gemma, the reference's configured re-ranker) parked 14 registers in scratch, reloaded in EVERY tile in front of the hand-written
    // wait (round 5: ScratchSize 60 -> 0).
    const unsigned long long kbase = (unsigned long long)Kg, vbase = (unsigned long long)Vg;
    const unsigned ld2 = (unsigned)ld * 2u;
    const unsigned lds_k0 = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)L.k[0] + (unsigned)(64 * wid) * 16u;
    const unsigned lds_v0 = (unsigned)(size_t)(__attribute__((address_space(3))) const char*)L.v[0] + (unsigned)(64 * wid) * 16u;
    constexpr unsigned kBufBytes = (unsigned)(KT * DH * 2);
    auto stage = [&](int tile, int buf) {
        const int kt = tile * KT;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = srow + RSTEP * j;
            const unsigned key = (unsigned)(kt + row < T ? kt + row : T - 1);
            const unsigned klc = (unsigned)(slot ^ s2_kswz<DH>(row)), vlc = (unsigned)(slot ^ s2_vswz<DH>(row));
            const unsigned rowoff = key * ld2;
            dma16u(kbase, rowoff + klc * 16u, lds_k0 + (unsigned)buf * kBufBytes + (unsigned)(256 * j) * 16u);
            dma16u(vbase, rowoff + vlc * 16u, lds_v0 + (unsigned)buf * kBufBytes + (unsigned)(256 * j) * 16u);
        }
        if (tid < KT) rmb = (kt + tid < T && mask[row0 + kt + tid]) ? 0.f : -30000.f;
    };
    auto stash_mask = [&](int buf) {
        if (tid < 128) {   // (waves 0 and 1 exactly; lanes >= KT carry 0)
            if (tid < KT) L.mb[buf][tid] = rmb;
            const bool any = __ballot(tid < KT && rmb != 0.f) != 0ull;
            if (lane == 0) L.padded[buf][wid] = any ? 1 : 0;
        }
    };
    h8 qf[KS];
    {
        const int qrow = q0 + r31 < T ? q0 + r31 : T - 1;
        const half_t* Qg = qkv + (row0 + qrow) * ld + hd * DH + h * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            h8 v = *(const h8*)(Qg + ks * 16);
            if (scale > 0.f) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (half_t)((float)v[e] * scale);
            }
            qf[ks] = v;
        }
    }
    f16v o[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[mt][e] = 0.f;
    float m_run = -1e30f, l_run = 0.f;
    const float LOG2E = scale > 0.f ? 1.4426950408889634f : 1.0f;
    const int vq = (lane >> 2) & 3, vp = lane & 3, vg = (lane >> 4) & 1;     // transposing-read coordinates (a2_read_v)
    stage(0, 0);
    stash_mask(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int tile = 0; tile < ntiles; ++tile) {
        const int buf = tile & 1, kt = tile * KT;
        if (tile + 1 < ntiles) stage(tile + 1, buf ^ 1);     // every wave left buffer buf ^ 1 before the last barrier
        const bool visit = wave_active && (!CAUSAL || kt <= q0 + 31);
        if (visit) {
            const char* Kb = L.k[buf];
            const char* Vb = L.v[buf];
            // (head dim 256 only: the fragment addresses below -- 16 swizzled K offsets, 16 V address pairs, all functions of the lane --
            //  are recomputed in every tile from an opaque copy of the lane id, a few VALU operations beside 32 MFMAs; hoisted out of the
            //  tile loop they were the other ten registers the allocator could not hold beside 128 accumulators and 64 query registers)
            int lane_t = lane;
            if constexpr (DH == 256) asm volatile("" : "+v"(lane_t));
            const int r31 = lane_t & 31, h = lane_t >> 5, vq = (lane_t >> 2) & 3, vp = lane_t & 3, vg = (lane_t >> 4) & 1;
            f16v s[NS];
#pragma unroll
            for (int sx = 0; sx < NS; ++sx) {
                f16v z;
#pragma unroll
                for (int e = 0; e < 16; ++e) z[e] = 0.f;
                s[sx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const h8*)(Kb + s2_koff<DH>(sx * 32 + r31, h)), qf[0], z, 0, 0, 0);
#pragma unroll
                for (int ks = 1; ks < KS; ++ks)
                    s[sx] = __builtin_amdgcn_mfma_f32_32x32x16_f16(*(const h8*)(Kb + s2_koff<DH>(sx * 32 + r31, 2 * ks + h)), qf[ks], s[sx], 0, 0, 0);
            }
            const bool diag = CAUSAL && (kt + KT - 1 > q0);
            if (L.padded[buf][0] | L.padded[buf][1]) {
#pragma unroll
                for (int sx = 0; sx < NS; ++sx)
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) s[sx][reg] += L.mb[buf][sx * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h];
            }
            if (diag) {
#pragma unroll
                for (int sx = 0; sx < NS; ++sx)
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int kl = sx * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                        if (kt + kl > q0 + r31) s[sx][reg] = -30000.f;
                    }
            }
            float tmax = -1e30f;
#pragma unroll
            for (int sx = 0; sx < NS; ++sx)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) tmax = fmaxf(tmax, s[sx][reg]);
            {
                float lo, hi;
                halves(tmax, lo, hi);
                tmax = fmaxf(lo, hi);
            }
            const float m_new = fmaxf(m_run, tmax);
            const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * LOG2E);
            const float mneg = -m_new * LOG2E;
            float psum = 0.f;
            h8 pf[2 * NS];
#pragma unroll
            for (int sx = 0; sx < NS; ++sx)
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const float p = __builtin_amdgcn_exp2f(fmaf(s[sx][reg], LOG2E, mneg));
                    psum += p;
                    pf[sx * 2 + (reg >> 3)][reg & 7] = (half_t)p;
                }
            {
                float lo, hi;
                halves(psum, lo, hi);
                psum = lo + hi;
            }
            l_run = l_run * alpha + psum;
            m_run = m_new;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[mt][e] *= alpha;
            // O^T[dh, q] += V^T[dh, keys] P^T[keys, q]; k-slot j of half h of 16-key group st <-> key 16 st + (j&3) + 8 (j>>2) + 4 h
#pragma unroll
            for (int st = 0; st < 2 * NS; ++st)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) {
                    const int key = 16 * st + 4 * h + vq, ch = 4 * mt + 2 * vg + (vp >> 1);
                    h8 vf;
                    a2_tr_read(vf, Vb + s2_voff<DH>(key, ch) + 8 * (vp & 1), Vb + s2_voff<DH>(key + 8, ch) + 8 * (vp & 1));
                    o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[st], o[mt], 0, 0, 0);
                }
        }
        if (tile + 1 < ntiles) stash_mask(buf ^ 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's DMA of the next tile has landed
        __syncthreads();
    }
    if (wave_active && q0 + r31 < T) {
        const float inv = 1.0f / l_run;
        half_t* dst = ctx + (row0 + q0 + r31) * ctx_ld + hd * DH;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                h4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (half_t)(o[mt][g4 * 4 + e] * inv);
                *(h4*)(dst + mt * 32 + 8 * g4 + 4 * h) = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// pooling / heads: one 256-thread block per sequence -> out[b, :]
//   pooling 0 CLS (token 0), 1 unmasked mean over T (continuous_retrieval.py:148 quirk), 3 MASKED mean (sentence-transformers'
//   Pooling module with pooling_mode_mean_tokens: what HuggingFaceEmbeddings(model_name) of ragManager.py:50 runs for a model
//   whose 1_Pooling/config.json says so, or that ships no modules.json at all), 2 last
//   token per last_token_pool (step3_mul.py:181-188: position T-1 if EVERY row's last mask bit is 1,
//   else sum(mask)-1);  normalize: L2 (sentence-transformers Normalize module)
//   head 1: RobertaClassificationHead  logit = out_proj(tanh(dense(x_cls)))
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pool(const half_t* x, const int* mask, int T, int Tv, int H, int pooling,
                                               int normalize, int all_last_set, int head, const half_t* Wd,
                                               const float* bd, const half_t* Wp, const float* bp, float* out,
                                               const int* seq_off = nullptr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* v = (float*)smem;        // [H]
    float* red = v + H;             // [256]
    const int b = blockIdx.x, tid = threadIdx.x;
    // packed sequences (CLS or last-token pooling): sequence b occupies rows [seq_off[b], seq_off[b + 1]), valid tokens first
    const long long base = seq_off ? (long long)seq_off[b] : (long long)b * T;
    if (seq_off) { Tv = seq_off[b + 1] - seq_off[b]; all_last_set = 0; }
    const half_t* xb = x + base * H;
    int tok = 0;
    if (pooling == 2) {
        if (all_last_set) tok = Tv - 1;
        else {
            int c = 0;
            for (int t = 0; t < Tv; ++t) c += mask[base + t] != 0;
            tok = c > 0 ? c - 1 : 0;
        }
    }
    for (int j = tid; j < H; j += 256) {
        float s = 0.f;
        if (pooling == 1) {
            for (int t = 0; t < Tv; ++t) s += (float)xb[(long long)t * H + j];
            s /= Tv;
        } else if (pooling == 3) {   // sentence-transformers' pooling_mode_mean_tokens: sum of the unmasked tokens / max(count, 1e-9)
            float cnt = 0.f;
            for (int t = 0; t < Tv; ++t)
                if (mask[base + t] != 0) { s += (float)xb[(long long)t * H + j]; cnt += 1.f; }
            s /= fmaxf(cnt, 1e-9f);
        } else {
            s = (float)xb[(long long)tok * H + j];
        }
        v[j] = s;
    }
    __syncthreads();
    if (head == 1) {
        // dense + tanh -> red-free second stage: each thread computes some outputs of dense
        float* y = red + 256;  // [H]
        // each thread owns some outputs and walks its weight row (independent loads, deep in flight).  Coalesced
        // one-row-per-wave variants were measured 2-4x SLOWER here (dependent L2 round trips per row); the head is
        // 0.4 % of a 100-pair forward, so the simple form stays.
        for (int o = tid; o < H; o += 256) {
            // 16-byte loads of the weight row, four independent partial sums (H % 32 == 0: hidden is a multiple of 128)
            const h8* wr8 = (const h8*)(Wd + (long long)o * H);
            float s4[4] = {bd[o], 0.f, 0.f, 0.f};
            for (int j8 = 0; j8 < (H >> 3); j8 += 4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const h8 w8 = wr8[j8 + q];
                    const float* vv = v + (j8 + q) * 8;
#pragma unroll
                    for (int e = 0; e < 8; ++e) s4[q] += (float)w8[e] * vv[e];
                }
            }
            y[o] = tanhf((s4[0] + s4[1]) + (s4[2] + s4[3]));
        }
        __syncthreads();
        float part = 0.f;
        for (int j = tid; j < H; j += 256) part += (float)Wp[j] * y[j];
        red[tid] = part;
        __syncthreads();
        for (int s2 = 128; s2; s2 >>= 1) { if (tid < s2) red[tid] += red[tid + s2]; __syncthreads(); }
        if (tid == 0) out[b] = red[0] + bp[0];
        return;
    }
    float scale = 1.f;
    if (normalize) {
        float part = 0.f;
        for (int j = tid; j < H; j += 256) part += v[j] * v[j];
        red[tid] = part;
        __syncthreads();
        for (int s2 = 128; s2; s2 >>= 1) { if (tid < s2) red[tid] += red[tid + s2]; __syncthreads(); }
        const float nrm = sqrtf(red[0]);
        scale = 1.0f / fmaxf(nrm, 1e-12f);
    }
    for (int j = tid; j < H; j += 256) out[(long long)b * H + j] = v[j] * scale;
}

__global__ void k_to_f32(const half_t* x, long long n, float* out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = (float)x[i];
}

// returns 1 if mask[:, T-1] is all ones (last_token_pool's left-padding test)
__global__ void k_all_last_set(const int* mask, int B, int T, int Tv, int* out) {
    int ok = 1;
    for (int b = threadIdx.x; b < B; b += blockDim.x) ok &= mask[b * T + Tv - 1] != 0;
    ok = __all(ok);
    if (threadIdx.x == 0) *out = ok;
}

// ------------------------------------------------------------------------------------------------
// Decoder-only (pre-norm, RMSNorm, RoPE, grouped-query attention, SwiGLU) layer pieces: the family of the models the
// reference configures by default -- Qwen3-Embedding with last_token_pool (experiments/retriever/step3_mul.py:181-209,
// :384) and "Yes"-logit LLM re-rankers (experiments/profile/stress_test.py:197,212-225).  GEMMs and the streaming
// attention are the kernels above; these are the small row kernels around them (half a wave per row, 16-byte chunks).
// ------------------------------------------------------------------------------------------------
// token embeddings (times the model's embedding scale) into the FP32 residual stream
__global__ __launch_bounds__(256) void k_gather_rows(const int* ids, const half_t* table, int M, int H, float scale, float* out) {
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), l32 = threadIdx.x & 31;
    if (row >= M) return;
    const h8* src = (const h8*)(table + (long long)ids[row] * H);
    float4* dst = (float4*)(out + (long long)row * H);
    for (int c = l32; c < (H >> 3); c += 32) {
        const h8 v = src[c];   // gemma: embeddings times sqrt(hidden)
        dst[2 * c] = make_float4((float)v[0] * scale, (float)v[1] * scale, (float)v[2] * scale, (float)v[3] * scale);
        dst[2 * c + 1] = make_float4((float)v[4] * scale, (float)v[5] * scale, (float)v[6] * scale, (float)v[7] * scale);
    }
}

// y = x * rsqrt(mean(x^2) + eps) * (w + woff)   (woff = 1 for gemma's zero-centred gains; fp32 statistics; chunks are
// re-read in the second pass).  x is the fp32 residual stream; y is fp16 (the next GEMM's operand) or fp32 (exported
// hidden states).
template <typename TOUT>
__global__ __launch_bounds__(256) void k_rmsnorm(const float* x, const float* w, float woff, float eps, int M, int H, TOUT* y) {
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), l32 = threadIdx.x & 31;
    if (row >= M) return;
    const float4* src = (const float4*)(x + (long long)row * H);
    const int nch = H >> 2;
    float q = 0.f;
    for (int c = l32; c < nch; c += 32) {
        const float4 a = src[c];
        q += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
    }
    const float r = rsqrtf(half_wave_sum(q) / H + eps);
    const float4* wv = (const float4*)w;
    for (int c = l32; c < nch; c += 32) {
        const float4 a = src[c], g = wv[c];
        const float o0 = a.x * r * (g.x + woff), o1 = a.y * r * (g.y + woff), o2 = a.z * r * (g.z + woff), o3 = a.w * r * (g.w + woff);
        if constexpr (sizeof(TOUT) == 4) {
            ((float4*)(y + (long long)row * H))[c] = make_float4(o0, o1, o2, o3);
        } else {
            h4 o;
            o[0] = (half_t)o0; o[1] = (half_t)o1; o[2] = (half_t)o2; o[3] = (half_t)o3;
            ((h4*)(y + (long long)row * H))[c] = o;
        }
    }
}

// cos / sin of pos * theta^(-2i/dh), i < dh/2, pos < T  ->  tab[pos][i] = (cos, sin)
__global__ void k_rope_table(float theta, int T, int dh, float2* tab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, half_dh = dh >> 1;
    if (i >= T * half_dh) return;
    const int pos = i / half_dh, j = i - pos * half_dh;
    const float inv_freq = powf(theta, -2.0f * (float)j / (float)dh);
    float sn, cs;
    sincosf((float)pos * inv_freq, &sn, &cs);
    tab[i] = make_float2(cs, sn);
}

// In place on the q and k parts of a qkv row: optional per-head RMSNorm over head_dim (weights qw / kw), then rotary
// embedding in the "rotate half" convention (element i pairs with i + dh/2).  dh/16 lanes per TOKEN; lane j owns elements
// [8j, 8j+8) of the first half and their partners in the second half of EVERY head of its token (two 16-byte accesses per
// head: no cross-lane traffic for the rotation), so the token's (cos, sin) row and the norm weights are fetched once per
// token instead of once per head -- per head they were twice the bytes of the data itself (39 us per layer at Qwen3-0.6B's
// 16 x 512 tokens against a 20 us read-modify-write floor).  dh in {64, 128, 256}.
__global__ __launch_bounds__(256) void k_qknorm_rope(half_t* qkv, int M, int T, int ld, int heads, int kv_heads, int dh,
                                                      const float* qw, const float* kw, float eps, int qk_norm,
                                                      const float2* tab, const int* pos_ids = nullptr) {
    const int lpu = dh >> 4;                       // lanes per token: 16 (dh 256), 8 (dh 128) or 4 (dh 64)
    const int tpw = 256 / lpu;                     // tokens per workgroup
    const int tokx = blockIdx.x * tpw + threadIdx.x / lpu, j = threadIdx.x % lpu;
    const bool live = tokx < M;
    const int tok = live ? tokx : 0;
    const int half_dh = dh >> 1, pos = pos_ids ? pos_ids[tok] : tok % T;   // packed rows carry their own positions
    float cc[8], ss[8];
    {
        const float4* tp = (const float4*)(tab + pos * half_dh + 8 * j);   // (cos, sin) pairs of elements 8j .. 8j + 7
#pragma unroll
        for (int e2 = 0; e2 < 4; ++e2) {
            const float4 c = tp[e2];
            cc[2 * e2] = c.x; ss[2 * e2] = c.y; cc[2 * e2 + 1] = c.z; ss[2 * e2 + 1] = c.w;
        }
    }
    half_t* row = qkv + (long long)tok * ld;
    {   // blockIdx.y: the first half of the q heads, the second half, the k heads (three times the lanes in flight)
        const int part = blockIdx.y == 2, h0 = blockIdx.y == 1 ? heads / 2 : 0;
        const int nh = part ? kv_heads : (blockIdx.y == 1 ? heads - heads / 2 : heads / 2);
        half_t* base = row + (part ? heads * dh : h0 * dh);
        const float* w = part ? kw : qw;
        float wl[8], wh[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { wl[e] = qk_norm ? w[8 * j + e] : 1.f; wh[e] = qk_norm ? w[half_dh + 8 * j + e] : 1.f; }
        for (int hh = 0; hh < nh; ++hh) {
            half_t* v = base + hh * dh;
            const h8 lo = *(const h8*)(v + 8 * j), hi = *(const h8*)(v + half_dh + 8 * j);
            float a[8], b[8], q = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { a[e] = (float)lo[e]; b[e] = (float)hi[e]; q += a[e] * a[e] + b[e] * b[e]; }
            float r = 1.f;
            if (qk_norm) {
                for (int o = lpu >> 1; o > 0; o >>= 1) q += __shfl_xor(q, o);
                r = rsqrtf(q / dh + eps);
            }
            h8 olo, ohi;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // HF casts the normalised value to the activation dtype before the weight multiply and again before RoPE
                float x1 = a[e] * r, x2 = b[e] * r;
                if (qk_norm) { x1 = (float)(half_t)x1 * wl[e]; x2 = (float)(half_t)x2 * wh[e]; }
                x1 = (float)(half_t)x1; x2 = (float)(half_t)x2;
                olo[e] = (half_t)(x1 * cc[e] - x2 * ss[e]);
                ohi[e] = (half_t)(x2 * cc[e] + x1 * ss[e]);
            }
            if (live) {
                *(h8*)(v + 8 * j) = olo;
                *(h8*)(v + half_dh + 8 * j) = ohi;
            }
        }
    }
}

// act[m][f] = act_fn(gu[m][f]) * gu[m][F + f];  act_fn = SiLU (0) or tanh-GELU (1: gemma's gelu_pytorch_tanh).
// grid (ceil(F / 8 / 256), rows): no index division on the per-chunk path.
__global__ __launch_bounds__(256) void k_swiglu(const half_t* gu, long long M, int F, int act_kind, half_t* act) {
    const int fc = blockIdx.x * 256 + threadIdx.x;
    if (fc >= (F >> 3)) return;
    for (long long m = blockIdx.y; m < M; m += gridDim.y) {
        const h8 g = *(const h8*)(gu + m * 2 * F + fc * 8);
        const h8 u = *(const h8*)(gu + m * 2 * F + F + fc * 8);
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float x = (float)g[e];
            // tanh-GELU = x * sigmoid(2 * 0.7978845608 * (x + 0.044715 x^3)) (gelu_tanh);  SiLU = x * sigmoid(x)
            o[e] = (half_t)((act_kind == 1 ? gelu_tanh(x) : x / (1.0f + __expf(-x))) * (float)u[e]);
        }
        *(h8*)(act + m * F + fc * 8) = o;
    }
}

// one vocabulary token's logit at the pooled (last) position: out[b] = x[last_b] . row     (the "Yes" score)
__global__ __launch_bounds__(64) void k_token_logit(const half_t* x, const int* mask, int T, int Tv, int H, int all_last_set,
                                                    const half_t* row, float* out, const int* seq_off = nullptr) {
    const int b = blockIdx.x, lane = threadIdx.x;
    // packed sequences: rows [seq_off[b], seq_off[b + 1]), valid tokens first -- the last valid one is the count - 1
    const long long base = seq_off ? (long long)seq_off[b] : (long long)b * T;
    if (seq_off) { Tv = seq_off[b + 1] - seq_off[b]; all_last_set = 0; }
    int tok = Tv - 1;
    if (!all_last_set) {
        int c = 0;
        for (int t = 0; t < Tv; ++t) c += mask[base + t] != 0;
        tok = c > 0 ? c - 1 : 0;
    }
    const half_t* xr = x + (base + tok) * H;
    float s = 0.f;
    for (int j = lane; j < H; j += 64) s += (float)xr[j] * (float)row[j];
    s = wave_sum(s);
    if (lane == 0) out[b] = s;
}

}  // namespace vft

// ------------------------------------------------------------------------------------------------
// handle + C ABI
// ------------------------------------------------------------------------------------------------
using namespace vft;
static hipError_t gws_ensure(GemmWs& g, hipStream_t zero_on = nullptr);
static void gws_free(GemmWs& g);

// ------------------------------------------------------------------------------------------------
// Opt every kernel into its dynamic LDS size (idempotent; cheap).
// The library holds ONE kernel per operation and shape class.  The measured-and-rejected kernels of rounds 1-3 (k_gemm256_tn,
// k_gemm_dma_tn with 32x32x16 MFMAs, the 128-wide DMA instance, the four-wave k_gemm4w_tn, the persistent k_gemm8q_tn, the all-layers
// k_sq_forward, LayerNorm in the tail of the residual products, first-generation attention) were deleted in round 4; their
// measurements stay in DESIGN.md section 7 and profiles/.
static hipError_t configure_once() {
    hipError_t er = hipSuccess;
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_tn<EPI_BIAS>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_tn<EPI_BIAS_GELU>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_tn<EPI_BIAS_QGELU>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_tn<EPI_BIAS_RESIDUAL>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_dma16_tn<EPI_BIAS, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, DLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_dma16_tn<EPI_BIAS_GELU, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, DLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_dma16_tn<EPI_BIAS_QGELU, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, DLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_dma16_tn<EPI_BIAS_RESIDUAL, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, DLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS_GELU>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS_QGELU>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS_RESIDUAL>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
#ifdef VF_EXPERIMENTS
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
#endif
#ifdef VF_EXPERIMENTS
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS_GELU, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
#endif
#ifdef VF_EXPERIMENTS
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS_RESIDUAL, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
#endif
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS, true>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS_GELU, true>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm9_tn<EPI_BIAS_RESIDUAL, true>, hipFuncAttributeMaxDynamicSharedMemorySize, RLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_BIAS>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_BIAS_GELU>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_BIAS_QGELU>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_BIAS_RESIDUAL>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_RESIDUAL_F32>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
#ifdef VF_EXPERIMENTS
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_LNA>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
#endif
#ifdef VF_EXPERIMENTS
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_LNA_GELU>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
#endif
#ifdef VF_EXPERIMENTS
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_RES_STATS>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
#endif
#ifdef VF_EXPERIMENTS
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_LNRES_STATS>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
#endif
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_GATED_SILU>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm8p_tn<EPI_GATED_GELU>, hipFuncAttributeMaxDynamicSharedMemorySize, PLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_tn<EPI_RESIDUAL_F32>, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_gemm_dma16_tn<EPI_RESIDUAL_F32, 256>, hipFuncAttributeMaxDynamicSharedMemorySize, DLDS);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_attention2<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_attention2<6>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_attention_stream2<64, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AttnStream2Lds<64>));
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_attention_stream2<64, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AttnStream2Lds<64>));
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_attention_stream2<128, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AttnStream2Lds<128>));
    if (er == hipSuccess) er = hipFuncSetAttribute((const void*)k_attention_stream2<256, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(AttnStream2Lds<256>));
    return er;
}


// k_attention2 launcher: persistent workgroups, as many as stay co-resident (LDS: K, V, two masks, O staging; registers:
// two waves per SIMD), each walking (sequence, head) pairs blockIdx.x, + gridDim.x, ...
static std::atomic<int> g_att_halves{1};
extern "C" int vf_debug_attention_halves(int on) { return g_att_halves.exchange(on ? 1 : 0); }   // A/B and parity: half items of k_attention2 on / off
template <int MODE>
static void launch_attention2(const half_t* qkv, const int* mask, int B, int T, int heads, half_t* ctx, hipStream_t st,
                              const int* seq_off = nullptr) {
    static const int n_cu = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        return n;
    }();
    const int waves = (T + 63) / 64;
    const size_t lds = (size_t)T * 256 + (size_t)T * 8 + (size_t)waves * 2048;   // K, V, two masks, O staging
    int per_cu = (int)((160 * 1024) / lds);
    if (per_cu > 8 / waves) per_cu = 8 / waves;
    if (per_cu < 1) per_cu = 1;
    const int npairs = B * heads;
    // half items (see the kernel): the pairs of a partial last round that fills at most half the CUs; a batch of at most half the CUs
    // altogether.  One workgroup per CU, an even number of waves (T > 192).  VF_ATT_HALVES=0 switches it off (A/B).
    static const int halves_on = getenv("VF_ATT_HALVES") ? atoi(getenv("VF_ATT_HALVES")) : 1;
    int nsplit = 0;
    if (halves_on && g_att_halves.load(std::memory_order_relaxed) && per_cu == 1 && waves >= 4 && waves % 2 == 0) {
        const int rem = npairs % n_cu;
        if (npairs > n_cu ? (rem > 0 && 2 * rem <= n_cu) : 2 * npairs <= n_cu) nsplit = npairs > n_cu ? rem : npairs;
    }
    const int nitems = npairs + nsplit;
    const int grid = nitems < n_cu * per_cu ? nitems : n_cu * per_cu;
    static const int ct = [] { const char* e = getenv("VF_ATT_CHUNK"); const int v = e ? atoi(e) : 4; return (v == 8 || v == 16) ? v : 4; }();
    hipLaunchKernelGGL(k_attention2<MODE>, dim3(grid), dim3(64 * waves), lds, st, qkv, mask, B, T, heads * ADH, ct, seq_off, ctx, nsplit);
}

constexpr int kEncResidentT = 512;   // longest sequence whose K / V^T fit the resident-attention kernel's LDS
constexpr int kEncMaxT = 8192;       // longest sequence the encoder takes (streaming attention beyond kEncResidentT)

// Every handle works on a stream of its OWN (created non-blocking on first use), never on the legacy NULL stream: two handles used
// from two threads on one device (a replica per request thread; ReplicaSet with a device listed twice) otherwise serialise on the NULL
// stream -- and an operation on it while ANOTHER handle's thread is capturing its small-batch graph fails outright ("operation would
// make the legacy stream depend on a capturing blocking stream": round 5, found by the from_config test with device_ids [0, 0]).
static hipError_t handle_stream(hipStream_t* s) {
    return *s ? hipSuccess : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

// ------------------------------------------------------------------------------------------------
// What the four model handles (vf_encoder, vf_decoder, vf_vit, vf_clip_text) share: the state, the create / destroy steps, the size
// formulas and the configuration check of the BERT-shaped layer.  Every entry point that selects a handle's device holds a
// vf::DeviceGuard (vf_internal.h) while it does.
// ------------------------------------------------------------------------------------------------
namespace vft {

// A handle's workspace: device buffers known by the address of the field that names each, so that one line allocates a buffer (and says
// whether it starts zeroed) and free_all() frees and nulls them all -- no second list to keep in step.
struct DevPool {
    std::vector<void**> fields;
    template <typename T>
    hipError_t get(T** field, size_t bytes, bool zero, hipStream_t st) {   // zero: filled on the handle's stream, in front of its forward
        const hipError_t e = hipMalloc((void**)field, bytes);
        if (e != hipSuccess) return e;
        fields.push_back((void**)field);
        return zero ? hipMemsetAsync(*field, 0, bytes, st) : hipSuccess;
    }
    void free_all() {   // the owner has synchronised its device
        for (void** f : fields) { (void)hipFree(*f); *f = nullptr; }
        fields.clear();
    }
};

struct ModelBase {
    hipStream_t stream = nullptr;   // this handle's own stream (handle_stream)
    GemmWs gws;
    int device = 0;
    half_t* w16 = nullptr;   // all fp16 matrices
    float* w32 = nullptr;    // all fp32 vectors (biases, norms)
    DevPool ws;              // the workspace, grown on demand (*_ensure_ws)
    std::mutex mu;
};

static int model_check_device(int device_id, const std::string& who) {
    int ndev = 0;
    VFT_HIP(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev) return fail(VF_EINVAL, who + ": bad device_id");
    return VF_OK;
}
// the two weight blobs onto the current device (= m.device), and every kernel opted into its LDS
static hipError_t model_upload(ModelBase& m, const void* w16, int64_t n16, const float* w32, int64_t n32) {
    hipError_t er = hipMalloc((void**)&m.w16, (size_t)n16 * 2);
    if (er == hipSuccess) er = hipMalloc((void**)&m.w32, (size_t)n32 * 4);
    if (er == hipSuccess) er = hipMemcpy(m.w16, w16, (size_t)n16 * 2, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = hipMemcpy(m.w32, w32, (size_t)n32 * 4, hipMemcpyHostToDevice);
    if (er == hipSuccess) er = configure_once();
    return er;
}
// a create that failed on the device: the message is built before the destroy's own HIP calls
template <typename H>
static int model_create_failed(H* h, int (*destroy)(H*), const char* who, hipError_t er) {
    const std::string msg = std::string(who) + ": " + hipGetErrorString(er);
    destroy(h);
    return fail(VF_EHIP, msg);
}
// everything ModelBase owns (current device = m.device); a handle that never ran a forward has no stream and an empty pool
static void model_release(ModelBase& m) {
    (void)hipDeviceSynchronize();
    m.ws.free_all();
    gws_free(m.gws);
    if (m.stream) (void)hipStreamDestroy(m.stream);
    if (m.w16) (void)hipFree(m.w16);
    if (m.w32) (void)hipFree(m.w32);
}

// elements of one BERT-shaped layer (encoder, vision tower, CLIP text tower): fp16 Wqkv, Wo, W1, W2; the fp32 vectors in the order of the
// post-LayerNorm layer (bqkv, bo, LN1, b1, b2, LN2) and of the pre-LayerNorm one (LN1, bqkv, bo, LN2, b1, b2)
static size_t bert_layer16(size_t H, size_t F) { return 3 * H * H + H * H + F * H + H * F; }
static size_t postln_layer32(size_t H, size_t F) { return 3 * H + H + 2 * H + F + H + 2 * H; }
static size_t preln_layer32(size_t H, size_t F) { return 2 * H + 3 * H + H + 2 * H + F + H; }
// ... and what the kernels ask of its widths; prefix: "", "vit: " or "clip text: "
static int bert_check_dims(int hidden, int heads, int ffn, const std::string& prefix) {
    if (hidden <= 0 || hidden % 128 != 0 || hidden > 1024) return fail(VF_EUNSUPPORTED, prefix + "hidden must be a multiple of 128, <= 1024");
    if (heads <= 0 || hidden % heads || hidden / heads != 64) return fail(VF_EUNSUPPORTED, prefix + "head dim must be 64");
    if (ffn <= 0 || ffn % 128 != 0) return fail(VF_EUNSUPPORTED, prefix + "ffn must be a multiple of 128");
    return VF_OK;
}

}  // namespace vft

struct vf_encoder : ModelBase {
    vf_encoder_config cfg{};
    bool q_folded = true;    // log2(e) / sqrt(dh) folded into the query projection (k_scale_half at load)
    // fp16 offsets (elements)
    size_t o_word = 0, o_pos = 0, o_type = 0, o_layers = 0, o_head_dense = 0, o_head_out = 0, layer16 = 0;
    // fp32 offsets
    size_t f_emb_g = 0, f_emb_b = 0, f_layers = 0, f_head_bd = 0, f_head_bp = 0, layer32 = 0;
    // workspace (grown on demand)
    int cap_tokens = 0, cap_b = 0;
    half_t *x = nullptr, *y = nullptr, *qkv = nullptr, *ctx = nullptr, *hbuf = nullptr;
    int *d_ids = nullptr, *d_mask = nullptr, *d_tt = nullptr, *d_pos = nullptr, *d_flag = nullptr;
    int* d_seq = nullptr;            // [cap_b + 1] row offsets of the packed (ragged-batch) forward
    std::vector<int32_t> pk;         // host staging of the packed ids / mask / position ids / type ids / offsets
    float* d_out = nullptr;
    float* d_hidden = nullptr;  // [cap_tokens, H] fp32, for vf_encoder_forward_hidden
    // split-K GEMM (forwards of <= kSplitMaxRows tokens): fp32 slabs [kSplitMax][kSplitMaxRows][max(3H, F)] + tile counters
    float* sk_part = nullptr;
    unsigned* sk_cnt = nullptr;
    // LayerNorm folded into the products (LnFold): gamma-folded copies of Wqkv (layers >= 1) and W1 (fp16, per layer
    // [3H][H] + [F][H]), their column sums and the folded bias vectors (fp32, per layer 3H + 3H + F + F); built on first use.
    // Row-sum partials of the two raw residual sums [H / 256][cap_tokens][2] live with the workspace.
    half_t* fold16 = nullptr;
    float* fold32 = nullptr;
    float *stats_a = nullptr, *stats_b = nullptr;
    // Small forwards (one query string: faissRetriever.py:33) are ~90 dependent launches of a few microseconds each and
    // run host-bound when launched one by one: they are captured once per shape into a hipGraph and replayed.
    struct GraphKey { int B, T, Tv, tt, pooling, normalize; bool operator==(const GraphKey& o) const { return B == o.B && T == o.T && Tv == o.Tv && tt == o.tt && pooling == o.pooling && normalize == o.normalize; } };
    struct GraphEntry { GraphKey key; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs;
};

static size_t enc_n16(const vf_encoder_config& c) {
    const size_t H = c.hidden, F = c.ffn;
    size_t n = (size_t)c.vocab * H + (size_t)c.max_pos * H + (size_t)c.type_vocab * H;
    n += (size_t)c.layers * bert_layer16(H, F);
    if (c.head == 1) n += H * H + H;
    return n;
}
static size_t enc_n32(const vf_encoder_config& c) {
    const size_t H = c.hidden, F = c.ffn;
    size_t n = 2 * H + (size_t)c.layers * postln_layer32(H, F);
    if (c.head == 1) n += H + 1;
    return n;
}

extern "C" int vf_encoder_weight_sizes(const vf_encoder_config* cfg, int64_t* n_fp16, int64_t* n_fp32) {
    if (!cfg || !n_fp16 || !n_fp32) return fail(VF_EINVAL, "vf_encoder_weight_sizes: null argument");
    *n_fp16 = (int64_t)enc_n16(*cfg);
    *n_fp32 = (int64_t)enc_n32(*cfg);
    return VF_OK;
}

static void enc_drop_graphs(vf_encoder* e) {
    for (auto& g : e->graphs) (void)hipGraphExecDestroy(g.exec);
    e->graphs.clear();
}

extern "C" int vf_encoder_destroy(vf_encoder* e) {
    if (!e) return VF_OK;
    vf::DeviceGuard guard;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    enc_drop_graphs(e);   // before the workspace goes: captured launches hold its pointers
    model_release(*e);
    if (e->d_flag) (void)hipFree(e->d_flag);
    if (e->sk_part) (void)hipFree(e->sk_part);
    if (e->sk_cnt) (void)hipFree(e->sk_cnt);
    if (e->fold16) (void)hipFree(e->fold16);
    if (e->fold32) (void)hipFree(e->fold32);
    delete e;
    return VF_OK;
}

extern "C" int vf_encoder_create(vf_encoder** out, const vf_encoder_config* cfg, const void* w16, int64_t n16,
                                 const float* w32, int64_t n32, int32_t device_id) {
    if (!out) return fail(VF_EINVAL, "vf_encoder_create: null out");
    *out = nullptr;
    if (!cfg || !w16 || !w32) return fail(VF_EINVAL, "vf_encoder_create: null argument");
    const vf_encoder_config& c = *cfg;
    VFT_TRY(bert_check_dims(c.hidden, c.heads, c.ffn, ""));
    if (c.layers <= 0 || c.vocab <= 0 || c.max_pos <= 0 || c.type_vocab <= 0) return fail(VF_EINVAL, "bad encoder config");
    if (c.pooling < 0 || c.pooling > 3 || c.head < 0 || c.head > 1) return fail(VF_EINVAL, "bad pooling / head");
    if ((size_t)n16 != enc_n16(c) || (size_t)n32 != enc_n32(c))
        return fail(VF_EINVAL, "vf_encoder_create: weight blob sizes do not match the config (see vf_encoder_weight_sizes)");
    VFT_TRY(model_check_device(device_id, "vf_encoder_create"));
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(device_id));
    vf_encoder* e = new (std::nothrow) vf_encoder();
    if (!e) return fail(VF_ENOMEM, "host allocation failed");
    e->cfg = c; e->device = device_id;
    const size_t H = c.hidden, F = c.ffn;
    e->o_word = 0; e->o_pos = e->o_word + (size_t)c.vocab * H; e->o_type = e->o_pos + (size_t)c.max_pos * H;
    e->o_layers = e->o_type + (size_t)c.type_vocab * H;
    e->layer16 = bert_layer16(H, F);
    e->o_head_dense = e->o_layers + (size_t)c.layers * e->layer16;
    e->o_head_out = e->o_head_dense + H * H;
    e->f_emb_g = 0; e->f_emb_b = H; e->f_layers = 2 * H;
    e->layer32 = postln_layer32(H, F);
    e->f_head_bd = e->f_layers + (size_t)c.layers * e->layer32;
    e->f_head_bp = e->f_head_bd + H;
    hipError_t er = model_upload(*e, w16, n16, w32, n32);
    if (er == hipSuccess) er = hipMalloc((void**)&e->d_flag, 4);
    {
        const size_t nmax = std::max<size_t>(3 * (size_t)cfg->hidden, (size_t)cfg->ffn);
        if (er == hipSuccess) er = hipMalloc((void**)&e->sk_part, (size_t)kSplitMax * kSplitMaxRows * nmax * sizeof(float));
        if (er == hipSuccess) er = hipMalloc((void**)&e->sk_cnt, 4096 * sizeof(unsigned));
        if (er == hipSuccess) er = handle_stream(&e->stream);
        if (er == hipSuccess) er = hipMemsetAsync(e->sk_cnt, 0, 4096 * sizeof(unsigned), e->stream);   // (not the legacy stream: see handle_stream)
    }
    if (er == hipSuccess && e->q_folded) {
        const float qs = 0.125f * 1.4426950408889634f;   // log2(e) / sqrt(64)
        for (int l = 0; l < c.layers; ++l) {
            hipLaunchKernelGGL(k_scale_half, dim3((unsigned)((H * H + 255) / 256)), dim3(256), 0, 0,
                               e->w16 + e->o_layers + (size_t)l * e->layer16, (long long)(H * H), qs);
            hipLaunchKernelGGL(k_scale_float, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, 0,
                               e->w32 + e->f_layers + (size_t)l * e->layer32, (long long)H, qs);
        }
        er = hipDeviceSynchronize();
    }
    if (er != hipSuccess) return model_create_failed(e, vf_encoder_destroy, "vf_encoder_create", er);
    *out = e;
    return VF_OK;
}

// Every *_ensure_ws below: the zero fills run on the handle's stream, in front of its forward; the capacity is set once every buffer
// exists, so a call after an allocation that failed half-way frees what there is and starts over.
static int enc_ensure_ws(vf_encoder* e, int B, int T) {
    VFT_HIP(handle_stream(&e->stream));
    int tokens = (B * T + 255) / 256 * 256;
    if (tokens <= e->cap_tokens && B <= e->cap_b) return VF_OK;
    // grow monotonically on BOTH axes: alternating call shapes (100 x 512 re-rank, then 256 x 64 embed) must not free and
    // rebuild the workspace -- and drop every captured graph -- on each call
    tokens = std::max(tokens, e->cap_tokens); B = std::max(B, e->cap_b);
    enc_drop_graphs(e);   // captured launches hold the workspace pointers
    e->ws.free_all();
    e->cap_tokens = e->cap_b = 0;
    const size_t H = e->cfg.hidden, F = e->cfg.ffn, Mp = tokens;
    const int out_dim = e->cfg.head == 1 ? 1 : (int)H;
    DevPool& ws = e->ws;
    hipStream_t st = e->stream;
    // (zeroed: padded rows are read by the GEMMs, keep them finite)
    VFT_HIP(ws.get(&e->x, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&e->y, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&e->qkv, Mp * 3 * H * 2, true, st));
    VFT_HIP(ws.get(&e->ctx, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&e->hbuf, Mp * F * 2, true, st));
    VFT_HIP(ws.get(&e->d_ids, Mp * 4, false, st));
    VFT_HIP(ws.get(&e->d_mask, Mp * 4, false, st));
    VFT_HIP(ws.get(&e->d_tt, Mp * 4, false, st));
    VFT_HIP(ws.get(&e->d_pos, Mp * 4, false, st));
    VFT_HIP(ws.get(&e->d_seq, ((size_t)B + 1) * 4, false, st));
    VFT_HIP(ws.get(&e->d_out, (size_t)B * out_dim * 4, false, st));
    VFT_HIP(ws.get(&e->d_hidden, Mp * H * 4, false, st));
    if (H % 256 == 0) {
        VFT_HIP(ws.get(&e->stats_a, (H / 256) * Mp * 2 * sizeof(float), true, st));
        VFT_HIP(ws.get(&e->stats_b, (H / 256) * Mp * 2 * sizeof(float), true, st));
    }
    e->cap_tokens = tokens; e->cap_b = B;
    VFT_HIP(gws_ensure(e->gws, st));
    return VF_OK;
}

// compute units of the current device (256 on MI355X)
static int device_cus() {
    static const int n = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 256;
        return v;
    }();
    return n;
}

template <int EPI>
static hipError_t gemm_splitk(const half_t* A, const half_t* W, const float* bias, const half_t* R, half_t* C, int Mrows,
                              int N, int K, float* part, unsigned* cnt, hipStream_t st) {
    const int tiles = (Mrows / SBM) * (N / SBN);
    const int sp = pick_splits(tiles, K);
    hipLaunchKernelGGL(k_gemm_splitk<EPI>, dim3(tiles * sp), dim3(256), 0, st, A, W, bias, R, C, Mrows, N, K, sp, part, cnt);
    return hipGetLastError();
}

static std::atomic<int> g_loop2{getenv("VF_GEMM_8P_LOOP2") ? atoi(getenv("VF_GEMM_8P_LOOP2")) : 1};   // default: the two-phase loop (round 3: 2-7 % on the products, 0.7-2 % on the forward)
extern "C" int vf_debug_gemm_8p_loop2(int on) { return on >= 0 ? g_loop2.exchange(on ? 1 : 0) : g_loop2.load(); }   // A/B: two-phase main loop of k_gemm8p_tn
static std::atomic<unsigned long long*> g_gemm9_dbg{nullptr};
// test hook: device buffer [workgroups][16 tiles][6] for k_gemm9_tn's wall-clock stamps (100 MHz), or null (tools/gemm9_stamps.py)
extern "C" void vf_debug_gemm9_stamps(void* buf) { g_gemm9_dbg.store((unsigned long long*)buf); }
static std::atomic<long long> g_gemm9_split_launches{0};
extern "C" long long vf_debug_gemm9_split_launches(void) { return g_gemm9_split_launches.load(std::memory_order_relaxed); }   // products cut whole along K so far
static std::atomic<long long> g_gemm9_streamk_launches{0};
extern "C" long long vf_debug_gemm9_streamk_launches(void) { return g_gemm9_streamk_launches.load(std::memory_order_relaxed); }   // stream-K launches so far
static std::atomic<int> g_gemm9_streamk{-1};   // -1: VF_GEMM_9_STREAMK decides; 0 / 1: forced by the test hook
extern "C" int vf_debug_gemm9_streamk(int on) { return g_gemm9_streamk.exchange(on < 0 ? -1 : (on ? 1 : 0)); }
static std::atomic<int> g_gemm9_split{-1};   // -1: VF_GEMM_9_SPLIT decides; 0 / 1: forced by the test hook
extern "C" int vf_debug_gemm9_split(int on) { return g_gemm9_split.exchange(on < 0 ? -1 : (on ? 1 : 0)); }   // A/B: the whole-product K cut inside the persistent kernel
static std::atomic<int> g_gemm9{-1};   // -1: VF_GEMM_9 decides; 0 / 1: forced by the test hook
extern "C" int vf_debug_gemm9(int on) { return g_gemm9.exchange(on < 0 ? -1 : (on ? 1 : 0)); }   // A/B: the persistent register-epilogue kernel as the default large product
static std::atomic<long long> g_p8_min_override{-1};
// Test hook: lower the tile count from which the 8-phase kernel (and with it the folded LayerNorm) is used, so that a small model
// exercises that path.
extern "C" long long vf_debug_gemm_8p_min_wgs(long long v) { return g_p8_min_override.exchange(v); }
static LnFold lf_plain() { LnFold l{}; l.loop2 = g_loop2.load(std::memory_order_relaxed); return l; }

// Split-K tail of the 8-phase products: fp32 partials + arrival counters.  The workspace belongs to a HANDLE (round 4: it
// used to be process-global, which raced between handles on different threads / devices): each encoder / decoder / vision
// handle allocates its own in *_ensure_ws -- never inside gemm(), so a forward under stream capture never allocates --
// and passes it down; launches of one handle are serialised by its mutex and stream, and the buffer is freed only at destroy.
// Sized for the largest cut gemm() makes: tail tiles x slices <= the CU count, 256 KB of partials each.
static std::atomic<int> g_splitk_tail{getenv("VF_NO_SPLITK_TAIL") ? 0 : getenv("VF_SPLITK_TAIL") ? std::min(2, std::max(0, atoi(getenv("VF_SPLITK_TAIL")))) : 1};
extern "C" int vf_debug_splitk_tail(int on) { return on >= 0 ? g_splitk_tail.exchange(on > 2 ? 2 : on) : g_splitk_tail.load(); }   // 0 off, 1 long-K products only (default), 2 every product with a partial last round
static std::atomic<int> g_sk_dbg{getenv("VF_SK_DBG") ? atoi(getenv("VF_SK_DBG")) : 0};   // sk_coop_finish's experiment / test bits
static std::mutex g_gws_mu;
static std::vector<GemmWs*> g_gws_all;    // every live workspace (statistics hook only)
static hipError_t gws_ensure(GemmWs& g, hipStream_t zero_on) {   // current device = the handle's; zero_on: the handle's stream (the counters are zeroed in front of its first product)
    if (g.ws) return hipSuccess;
    const size_t nb = gemm_ws_bytes(device_cus());
    hipError_t e = hipMalloc((void**)&g.ws, nb);
    if (e == hipSuccess) e = hipMalloc((void**)&g.cnt, ((size_t)kSkMaxTiles * 2 + 4) * sizeof(unsigned));
    if (e == hipSuccess) e = zero_on ? hipMemsetAsync(g.cnt, 0, ((size_t)kSkMaxTiles * 2 + 4) * sizeof(unsigned), zero_on) : hipMemset(g.cnt, 0, ((size_t)kSkMaxTiles * 2 + 4) * sizeof(unsigned));
    if (e != hipSuccess) {
        if (g.ws) (void)hipFree(g.ws);
        if (g.cnt) (void)hipFree(g.cnt);
        g.ws = nullptr; g.cnt = nullptr;
        return e;
    }
    g.bytes = nb;
    std::lock_guard<std::mutex> lk(g_gws_mu);
    g_gws_all.push_back(&g);
    return hipSuccess;
}
static void gws_free(GemmWs& g) {           // the owner has synchronised its device
    {
        std::lock_guard<std::mutex> lk(g_gws_mu);
        g_gws_all.erase(std::remove(g_gws_all.begin(), g_gws_all.end(), &g), g_gws_all.end());
    }
    if (g.ws) (void)hipFree(g.ws);
    if (g.cnt) (void)hipFree(g.cnt);
    g.ws = nullptr; g.cnt = nullptr; g.bytes = 0;
}
// read-backs served by the slices' own L2 / from memory since the last call, summed over the live workspaces of the current
// device (and the timing-experiment switches of LnFold::sk_dbg)
extern "C" int vf_debug_splitk_stats(unsigned* out2, int dbg) {
    if (dbg >= 0) g_sk_dbg.store(dbg);
    if (!out2) return 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    std::lock_guard<std::mutex> lk(g_gws_mu);
    out2[0] = out2[1] = 0;
    int seen = 0;
    for (GemmWs* g : g_gws_all) {
        hipPointerAttribute_t at{};
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipPointerGetAttributes(&at, g->cnt) != hipSuccess || at.device != dev) { (void)hipGetLastError(); continue; }
        unsigned v[2] = {0, 0};
        unsigned* p = g->cnt + 2 * (size_t)kSkMaxTiles;
        if (hipMemcpy(v, p, sizeof v, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        if (hipMemset(p, 0, 4 * sizeof(unsigned)) != hipSuccess) return -1;
        out2[0] += v[0]; out2[1] += v[1]; ++seen;
    }
    return seen ? 1 : 0;
}

// The knobs of a product's route (vf_gemm_route.h): the environment, read once per process, under the test hooks, read on each call.
static GemmKnobs gemm_knobs(int force_kind = 0) {
    static const GemmKnobs env = [] {
        const auto i = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        const auto ll = [](const char* name, long long dflt) { const char* e = getenv(name); return e ? atoll(e) : dflt; };
        GemmKnobs k;
        k.kind = i("VF_GEMM_KIND", k.kind);
        k.dma_min_wgs = ll("VF_GEMM_DMA_MIN_WGS", k.dma_min_wgs);
        k.p8_min_wgs = ll("VF_GEMM_8P_MIN_WGS", k.p8_min_wgs);
        k.p8_f32_min_wgs = ll("VF_GEMM_8P_F32_MIN_WGS", k.p8_f32_min_wgs);
        k.gemm9 = i("VF_GEMM_9", k.gemm9);
        k.gemm9_min_wgs = ll("VF_GEMM_9_MIN_WGS", k.gemm9_min_wgs);
        k.gemm9_split = i("VF_GEMM_9_SPLIT", k.gemm9_split);
        k.split_min_k = i("VF_GEMM_9_SPLIT_MINK", k.split_min_k);
        k.split_min_kt = i("VF_GEMM_9_SPLIT_MINKT", k.split_min_kt);
        k.gemm9_streamk = i("VF_GEMM_9_STREAMK", k.gemm9_streamk);
        k.streamk_min_saved = i("VF_GEMM_9_STREAMK_MIN_SAVED", k.streamk_min_saved);
        k.stagger_pct = i("VF_GEMM_9_STAGGER", k.stagger_pct);
#ifdef VF_EXPERIMENTS
        k.experiments = true;
#endif
        return k;
    }();
    GemmKnobs k = env;
    if (force_kind) k.kind = force_kind;
    const long long p8 = g_p8_min_override.load(std::memory_order_relaxed);
    if (p8 >= 0) { k.p8_min_wgs = p8; k.p8_forced = true; }
    const int h9 = g_gemm9.load(std::memory_order_relaxed), hsplit = g_gemm9_split.load(std::memory_order_relaxed),
              hsk = g_gemm9_streamk.load(std::memory_order_relaxed);
    if (h9 >= 0) k.gemm9 = h9;
    if (hsplit >= 0) k.gemm9_split = hsplit;
    if (hsk >= 0) k.gemm9_streamk = hsk;
    k.splitk_tail = g_splitk_tail.load(std::memory_order_relaxed);   // (VF_SPLITK_TAIL / VF_NO_SPLITK_TAIL are its initial value)
    return k;
}

static GemmIn gemm_in(int epi, int M, int N, int K, int force_kind, bool has_ws, size_t ws_bytes) {
    GemmIn in;
    in.epi = epi; in.M = M; in.N = N; in.K = K; in.n_cu = device_cus();
    in.has_ws = has_ws; in.ws_bytes = has_ws ? ws_bytes : 0;
    in.knobs = gemm_knobs(force_kind);
    return in;
}

// One product C = epi(A W^T): route_gemm (vf_gemm_route.h) picks the kernel, its grid and its cut; this launches it.
template <int EPI>
static hipError_t gemm(const half_t* A, const half_t* W, const float* bias, const half_t* R, half_t* C, int M, int N,
                       int K, hipStream_t st, int force_kind = 0, GemmWs* gws = nullptr) {
    const bool has_ws = gws && gws->ws;
    const GemmRoute r = route_gemm(gemm_in(EPI, M, N, K, force_kind, has_ws, has_ws ? gws->bytes : 0));
    constexpr bool epi9 = EPI == EPI_BIAS || EPI == EPI_BIAS_GELU || EPI == EPI_BIAS_QGELU || EPI == EPI_BIAS_RESIDUAL;   // the epilogues k_gemm9_tn is built for ...
    constexpr bool epi9_cut = epi9 && EPI != EPI_BIAS_QGELU;                                                               // ... and its cut forms
    const dim3 grid(r.grid);
    switch (r.kernel) {
    case kGemmTn128:
        hipLaunchKernelGGL(k_gemm_tn<EPI>, grid, dim3(256), (size_t)2 * (GBM + GBN) * GLD * sizeof(half_t), st, A, W, bias, R, C, M, N, K);
        return hipGetLastError();
    case kGemmDma16:
        hipLaunchKernelGGL((k_gemm_dma16_tn<EPI, 256>), grid, dim3(DTHREADS), DLDS, st, A, W, bias, R, C, M, N, K);
        return hipGetLastError();
    case kGemm8p: {
        LnFold lf = lf_plain();
        if (r.slices) {   // the split-K tail (LnFold::sk_*): `tail_tiles` tiles behind `full_tiles` whole ones, each in `slices` slices
            lf.sk_ws = gws->ws; lf.sk_cnt = gws->cnt; lf.sk_nfull = r.full_tiles; lf.sk_S = r.slices; lf.sk_ntail = r.tail_tiles;
            lf.sk_stat = gws->cnt + 2 * (size_t)kSkMaxTiles; lf.sk_dbg = g_sk_dbg.load(std::memory_order_relaxed);
        }
        hipLaunchKernelGGL(k_gemm8p_tn<EPI>, grid, dim3(PTHREADS), PLDS, st, A, W, bias, R, C, M, N, K, lf);
        return hipGetLastError();
    }
    case kGemm9:
        if constexpr (epi9) {
            hipLaunchKernelGGL(k_gemm9_tn<EPI>, grid, dim3(PTHREADS), RLDS, st, A, W, bias, R, C, M, N, K, r.stagger_ticks, g_gemm9_dbg.load(std::memory_order_relaxed), SkCtx{nullptr, nullptr, nullptr, 0, 0});
            return hipGetLastError();
        }
        break;
    case kGemm9Split:
        if constexpr (epi9_cut) {
            const SkCtx sk{gws->ws, gws->cnt, gws->cnt + 2 * (size_t)kSkMaxTiles, r.slices, g_sk_dbg.load(std::memory_order_relaxed)};
            g_gemm9_split_launches.fetch_add(1, std::memory_order_relaxed);
            hipLaunchKernelGGL((k_gemm9_tn<EPI, true>), grid, dim3(PTHREADS), RLDS, st, A, W, bias, R, C, M, N, K, 0, g_gemm9_dbg.load(std::memory_order_relaxed), sk);
            return hipGetLastError();
        }
        break;
    case kGemm9StreamK:
#ifdef VF_EXPERIMENTS   // (the default build does not carry the kernel, and says so to the route: GemmKnobs::experiments)
        if constexpr (epi9_cut) {
            const SkCtx sk{gws->ws, gws->cnt, gws->cnt + 2 * (size_t)kSkMaxTiles, 0, g_sk_dbg.load(std::memory_order_relaxed)};
            g_gemm9_streamk_launches.fetch_add(1, std::memory_order_relaxed);
            hipLaunchKernelGGL((k_gemm9_tn<EPI, 2>), grid, dim3(PTHREADS), RLDS, st, A, W, bias, R, C, M, N, K, 0, g_gemm9_dbg.load(std::memory_order_relaxed), sk);
            return hipGetLastError();
        }
#endif
        break;
    }
    return hipErrorInvalidValue;   // a route to a kernel this epilogue (or this build) does not have: never a quiet substitute
}

// Test hook: what gemm() would decide right now for one product -- the live knobs, the device's CU count and a workspace sized as
// gws_ensure sizes it -- as {kernel, grid, slices, tail tiles, full tiles, stagger ticks} (GemmRoute).  Launches nothing.
extern "C" int vf_debug_gemm_route(int M, int N, int K, int epi, int kind, int* out6) {
    if (!out6 || M <= 0 || N <= 0 || K <= 0 || M % 128 || N % 128 || K % 32) return -2;
    const GemmRoute r = route_gemm(gemm_in(epi, M, N, K, kind, true, gemm_ws_bytes(device_cus())));
    out6[0] = (int)r.kernel; out6[1] = r.grid; out6[2] = r.slices; out6[3] = r.tail_tiles; out6[4] = r.full_tiles; out6[5] = r.stagger_ticks;
    return 0;
}

// Gated MLP front half in one launch: C[M][F] = act(A . Wgate^T) * (A . Wup^T), Wgu = [gate rows (F) | up rows (F)] x K.  Returns
// false when the shape does not fill the 8-phase kernel (the caller then runs the plain product + k_swiglu).
static bool gemm_gated(const half_t* A, const half_t* Wgu, half_t* C, int M, int F, int K, int act_kind, hipStream_t st, hipError_t* er) {
    static const bool off = getenv("VF_NO_GATED_GEMM") != nullptr;   // A/B switch
    const int N = 2 * F;
    *er = hipSuccess;
    if (off || !gated_ok(M, F, K)) return false;
    if (act_kind == 1)
        hipLaunchKernelGGL(k_gemm8p_tn<EPI_GATED_GELU>, dim3((N / PBN) * (M / PBM)), dim3(PTHREADS), PLDS, st, A, Wgu, nullptr, nullptr, C, M, N, K, lf_plain());
    else
        hipLaunchKernelGGL(k_gemm8p_tn<EPI_GATED_SILU>, dim3((N / PBN) * (M / PBM)), dim3(PTHREADS), PLDS, st, A, Wgu, nullptr, nullptr, C, M, N, K, lf_plain());
    *er = hipGetLastError();
    return true;
}

template <int EPI>
static hipError_t gemm_skinny(const half_t* A, const half_t* W, const float* bias, const half_t* R, half_t* C, int Mvalid, int N,
                              int K, hipStream_t st, float* part = nullptr, unsigned* counters = nullptr) {
    // K split over workgroups when K is long and the column tiles alone leave most of the chip idle (see the kernel)
    static const bool no_split = getenv("VF_NO_SKINNY_SPLIT") != nullptr;
    const int S = skinny_slices(N, K, part && counters && !no_split);
    const dim3 grid((N / 16) * S), block(kSkinnyWaves * 64);
    switch ((Mvalid + 15) >> 4) {   // 16-row tiles that hold real rows
    case 1: hipLaunchKernelGGL((k_gemm_skinny<EPI, 1>), grid, block, 0, st, A, W, bias, R, C, Mvalid, N, K, S, part, counters); break;
    case 2: hipLaunchKernelGGL((k_gemm_skinny<EPI, 2>), grid, block, 0, st, A, W, bias, R, C, Mvalid, N, K, S, part, counters); break;
    case 3: hipLaunchKernelGGL((k_gemm_skinny<EPI, 3>), grid, block, 0, st, A, W, bias, R, C, Mvalid, N, K, S, part, counters); break;
    default: hipLaunchKernelGGL((k_gemm_skinny<EPI, 4>), grid, block, 0, st, A, W, bias, R, C, Mvalid, N, K, S, part, counters); break;
    }
    return hipGetLastError();
}

// (the measured-and-rejected experiment kernels of rounds 1-3 were deleted in round 4; DESIGN.md section 7 keeps their numbers)
extern "C" int vf_debug_experiments(void) { return 0; }

// ---- LayerNorm folded into the products (LnFold) ---------------------------------------------------------------------
// W'[n][k] = fp16(W[n][k] * gamma[k]);  colsum[n] = sum_k W'[n][k] (of the ROUNDED values: what the MFMA multiplies);
// c[n] = sum_k W[n][k] * beta[k] + b[n].  One wave per output row.
__global__ __launch_bounds__(256) void k_fold_ln(const half_t* __restrict__ W, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, const float* __restrict__ b, int N, int K,
                                                 half_t* __restrict__ Wf, float* __restrict__ colsum, float* __restrict__ cvec) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    float cs = 0.f, cv = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float w = (float)W[(long long)n * K + k];
        const half_t wf = (half_t)(w * gamma[k]);
        Wf[(long long)n * K + k] = wf;
        cs += (float)wf;
        cv += w * beta[k];
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) { cs += __shfl_xor(cs, o); cv += __shfl_xor(cv, o); }
    if (lane == 0) { colsum[n] = cs; cvec[n] = cv + b[n]; }
}

static std::atomic<long long> g_ln_fold_forwards{0};
// MEASURED SLOWER, so off unless asked for (VF_LN_FOLD=1 / vf_debug_ln_fold(1)): the two k_layernorm launches of a layer cost
// 2 x 29.5 us; the folded form removes them and adds their arithmetic to four epilogues that run on the MFMA waves with
// nothing beside them on the CU -- re-rank p50 12.14 vs 11.94 ms (XLM-R-base shape), 37.2 vs 35.7 (large), same box
// (tools/gpu_r03_fold.sh).  It is exact to the same tolerances (errors vs HF fp32 slightly smaller: x is never rounded to fp16).
static std::atomic<int> g_ln_fold{getenv("VF_LN_FOLD") ? 1 : 0};
extern "C" int vf_debug_ln_fold(int on) { return on >= 0 ? g_ln_fold.exchange(on ? 1 : 0) : g_ln_fold.load(); }
// Test hook: forwards that took the folded path so far (vf_debug_gemm_8p_min_wgs lowers the tile count from which a small model takes it).
extern "C" long long vf_debug_ln_fold_forwards() { return g_ln_fold_forwards.load(std::memory_order_relaxed); }

static size_t fold16_layer(const vf_encoder_config& c) { return (size_t)3 * c.hidden * c.hidden + (size_t)c.ffn * c.hidden; }
static size_t fold32_layer(const vf_encoder_config& c) { return (size_t)6 * c.hidden + 2 * (size_t)c.ffn; }

// the folded path serves a forward whose four products per layer all take the 8-phase kernel
static bool enc_fold_ok(const vf_encoder* e, int Mp) {
    const bool off = g_ln_fold.load(std::memory_order_relaxed) == 0;
    const GemmKnobs kn = gemm_knobs();
    const vf_encoder_config& c = e->cfg;
    if (off || kn.kind != 0) return false;
    if (Mp % PBM || c.hidden % PBN || c.ffn % PBN || c.hidden < 2 * PBK || !e->stats_a) return false;
    return (long long)(Mp / PBM) * (c.hidden / PBN) >= kn.p8_min_wgs;
}

static int enc_ensure_fold(vf_encoder* e, hipStream_t st) {
    if (e->fold16) return VF_OK;
    const vf_encoder_config& c = e->cfg;
    const int H = c.hidden, F = c.ffn;
    VFT_HIP(hipMalloc((void**)&e->fold16, (size_t)c.layers * fold16_layer(c) * sizeof(half_t)));
    VFT_HIP(hipMalloc((void**)&e->fold32, (size_t)c.layers * fold32_layer(c) * sizeof(float)));
    for (int l = 0; l < c.layers; ++l) {
        const half_t* w = e->w16 + e->o_layers + (size_t)l * e->layer16;
        const float* f = e->w32 + e->f_layers + (size_t)l * e->layer32;
        const half_t *Wqkv = w, *W1 = Wqkv + (size_t)4 * H * H;
        const float *bqkv = f, *g1 = f + 4 * H, *b1n = g1 + H, *b1 = b1n + H;
        half_t* d16 = e->fold16 + (size_t)l * fold16_layer(c);
        float* d32 = e->fold32 + (size_t)l * fold32_layer(c);
        if (l > 0) {   // the LayerNorm in front of this layer's QKV projection is the previous layer's second one
            const float* fp = e->w32 + e->f_layers + (size_t)(l - 1) * e->layer32;
            const float *g2p = fp + 7 * H + F, *b2np = g2p + H;
            hipLaunchKernelGGL(k_fold_ln, dim3((3 * H + 3) / 4), dim3(256), 0, st, Wqkv, g2p, b2np, bqkv, 3 * H, H, d16, d32, d32 + 3 * H);
        }
        hipLaunchKernelGGL(k_fold_ln, dim3((F + 3) / 4), dim3(256), 0, st, W1, g1, b1n, b1, F, H, d16 + (size_t)3 * H * H,
                           d32 + 6 * H, d32 + 6 * H + F);
    }
    VFT_HIP(hipGetLastError());
    return VF_OK;
}

template <int EPI>
static hipError_t gemm8p_fold(const half_t* A, const half_t* W, const float* bias, const half_t* R, half_t* C, int M, int N, int K,
                              const LnFold& lf, hipStream_t st) {
    hipLaunchKernelGGL(k_gemm8p_tn<EPI>, dim3((N / PBN) * (M / PBM)), dim3(PTHREADS), PLDS, st, A, W, bias, R, C, M, N, K, lf);
    return hipGetLastError();
}

// ids / mask / type ids already in e->d_ids / d_mask / d_tt; result lands in e->d_out
// seq_off != nullptr: PACKED rows (forward_impl's ragged-batch path) -- Mpk rows in all, sequence b in rows
// [seq_off[b], seq_off[b + 1]), T = the longest; ids / mask / position ids are already packed on the device.
static int enc_forward_device(vf_encoder* e, int B, int T, int Tv, bool has_tt, hipStream_t st, const int* seq_off = nullptr,
                              int Mpk = 0) {
    const vf_encoder_config& c = e->cfg;
    const int H = c.hidden, F = c.ffn, M = seq_off ? Mpk : B * T, Mp = (M + 255) / 256 * 256;
    const int Ms = (M + 63) / 64 * 64;
    static const bool no_splitk = getenv("VF_NO_SPLITK") != nullptr;  // A/B switch
    static const bool no_skinny = getenv("VF_NO_SKINNY") != nullptr;  // A/B switch
    // the product class (vf_gemm_route.h): skinny = one short sequence, weight-streaming GEMMs; split-K for the long-K product of a
    // single short sequence; everything else through gemm()
    const bool skinny = enc_product_class(M, H, F, false, !no_skinny, !no_splitk) == kEncSkinny;
    const bool ffn_down_splitk = enc_product_class(M, H, F, true, !no_skinny, !no_splitk) == kEncSplitK;
    if (!seq_off) hipLaunchKernelGGL(k_position_ids, dim3(B), dim3(64), 0, st, e->d_mask, B, T, c.roberta_pad_idx, e->d_pos);
    hipLaunchKernelGGL(k_embed_ln, dim3((M + 7) / 8), dim3(256), 0, st, e->d_ids, e->d_pos, has_tt ? e->d_tt : nullptr,
                       e->w16 + e->o_word, e->w16 + e->o_pos, e->w16 + e->o_type, e->w32 + e->f_emb_g, e->w32 + e->f_emb_b,
                       c.ln_eps, M, H, e->x);
    // V^T row stride: (T + pad) halves with (T + pad) / 2 == 2 (mod 64) -> conflict-free 8-byte reads
    // (rows must also be 16-byte aligned for the transposed staging writes -> multiple of 8 halves; a
    //  row stride of 4 (mod 64) dwords keeps the 8-byte reads of 32 lanes within a 2-way conflict)
    int pad = 8;
    while ((((T + pad) / 2) & 63) != 4) pad += 8;
    const int vt_ld = T + pad;
    const size_t att_lds = (size_t)T * AKLD * 2 + (size_t)ADH * vt_ld * 2 + (size_t)T * 4 + 64;  // K, V^T, mask, tile states
    // LayerNorm without a launch (LnFold): when every product of a layer takes the 8-phase kernel, the two LayerNorm sweeps of
    // the layer (2 x 29.5 us of 970 at 100 x 512 tokens) disappear into the products around them -- the residual products
    // write the RAW sums and their row sums, the next product reads the raw sum as its A operand through gamma-folded
    // weights, the next residual product normalises its residual element by element.  e->y holds y1 (attention sum),
    // e->x holds y2 (FFN sum) of the previous layer; the last layer writes y2 over y1 and one k_layernorm produces e->x.
#ifdef VF_EXPERIMENTS
    const bool fold = !skinny && !(!no_splitk && enc_short(M, H, F)) && enc_fold_ok(e, Mp);
    if (fold) { VFT_TRY(enc_ensure_fold(e, st)); g_ln_fold_forwards.fetch_add(1, std::memory_order_relaxed); }
#else
    constexpr bool fold = false;   // measured slower at every batch size: the folded epilogues are built with -DVF_EXPERIMENTS only
#endif
    LnFold lf0{};
    lf0.n_parts = H / 256; lf0.Mp = e->cap_tokens; lf0.inv_h = 1.0f / (float)H; lf0.eps = c.ln_eps;
    for (int l = 0; l < c.layers; ++l) {
        const half_t* w = e->w16 + e->o_layers + (size_t)l * e->layer16;
        const float* f = e->w32 + e->f_layers + (size_t)l * e->layer32;
        const half_t *Wqkv = w, *Wo = Wqkv + (size_t)3 * H * H, *W1 = Wo + (size_t)H * H, *W2 = W1 + (size_t)F * H;
        const float *bqkv = f, *bo = bqkv + 3 * H, *g1 = bo + H, *b1n = g1 + H, *b1 = b1n + H, *b2 = b1 + F, *g2 = b2 + H,
                    *b2n = g2 + H;
        const half_t* f16 = fold ? e->fold16 + (size_t)l * fold16_layer(c) : nullptr;
        const float* f32 = fold ? e->fold32 + (size_t)l * fold32_layer(c) : nullptr;
        if (skinny) VFT_HIP(gemm_skinny<EPI_BIAS>(e->x, Wqkv, bqkv, nullptr, e->qkv, M, 3 * H, H, st));
#ifdef VF_EXPERIMENTS
        else if (fold && l > 0) {   // A = the previous layer's raw FFN sum; its LayerNorm sits in the folded weights + epilogue
            LnFold lf = lf0;
            lf.stats_in = e->stats_b; lf.colsum = f32;
            VFT_HIP(gemm8p_fold<EPI_LNA>(e->x, f16, f32 + 3 * H, nullptr, e->qkv, Mp, 3 * H, H, lf, st));
        }
#endif
        else VFT_HIP(gemm<EPI_BIAS>(e->x, Wqkv, bqkv, nullptr, e->qkv, Mp, 3 * H, H, st, 0, &e->gws));
        static const bool att_stream = getenv("VF_ATT_STREAM") != nullptr;  // A/B switch: streaming kernel on the BERT path
        // Sequences longer than 512 tokens (bge-m3 = XLM-R-large with an 8194-entry position table: config/example.yaml:3,
        // src/utils/ragManager.py:50) cannot keep K and V^T of a head resident in LDS: they take the streaming kernel
        // (64-key tiles through LDS, online softmax), which has no length limit.
        if (att_stream || T > kEncResidentT) {
                hipLaunchKernelGGL((k_attention_stream2<64, false>), dim3((T + 127) / 128, c.heads, B), dim3(256),
                                   sizeof(AttnStream2Lds<64>), st, e->qkv, e->d_mask, T, 3 * H, c.heads, c.heads,
                                   e->q_folded ? -1.f : 0.125f, e->ctx, H, seq_off);
        } else {
            (void)att_lds;
            if (!e->q_folded) return fail(VF_EUNSUPPORTED, "the resident attention kernel needs the softmax scale folded into the query projection");
            launch_attention2<0>(e->qkv, e->d_mask, B, T, c.heads, e->ctx, st, seq_off);
        }
#ifdef VF_EXPERIMENTS
        if (fold) {
            LnFold lf = lf0;
            lf.stats_out = e->stats_a;
            if (l == 0) VFT_HIP(gemm8p_fold<EPI_RES_STATS>(e->ctx, Wo, bo, e->x, e->y, Mp, H, H, lf, st));   // residual = the embedding LayerNorm's output
            else {
                const float* fp = e->w32 + e->f_layers + (size_t)(l - 1) * e->layer32;
                lf.stats_in = e->stats_b; lf.gR = fp + 7 * H + F; lf.bR = fp + 8 * H + F;                    // previous layer's g2 / b2n
                VFT_HIP(gemm8p_fold<EPI_LNRES_STATS>(e->ctx, Wo, bo, e->x, e->y, Mp, H, H, lf, st));
            }
            LnFold lu = lf0;
            lu.stats_in = e->stats_a; lu.colsum = f32 + 6 * H;
            VFT_HIP(gemm8p_fold<EPI_LNA_GELU>(e->y, f16 + (size_t)3 * H * H, f32 + 6 * H + F, nullptr, e->hbuf, Mp, F, H, lu, st));
            LnFold ld = lf0;
            ld.stats_in = e->stats_a; ld.gR = g1; ld.bR = b1n; ld.stats_out = e->stats_b;
            half_t* dst = l + 1 < c.layers ? e->x : e->y;      // the last layer's sum goes over y1 (same chunk read and written by a thread)
            VFT_HIP(gemm8p_fold<EPI_LNRES_STATS>(e->hbuf, W2, b2, e->y, dst, Mp, H, F, ld, st));
            if (l + 1 == c.layers) hipLaunchKernelGGL(k_layernorm, dim3((M + 7) / 8), dim3(256), 0, st, e->y, g2, b2n, c.ln_eps, M, H, e->x);
            continue;
        }
#else
        (void)f16; (void)f32; (void)lf0;
#endif
        if (skinny) VFT_HIP(gemm_skinny<EPI_BIAS_RESIDUAL>(e->ctx, Wo, bo, e->x, e->y, M, H, H, st));
        else VFT_HIP(gemm<EPI_BIAS_RESIDUAL>(e->ctx, Wo, bo, e->x, e->y, Mp, H, H, st, 0, &e->gws));
        hipLaunchKernelGGL(k_layernorm, dim3((M + 7) / 8), dim3(256), 0, st, e->y, g1, b1n, c.ln_eps, M, H, e->x);
        if (skinny) VFT_HIP(gemm_skinny<EPI_BIAS_GELU>(e->x, W1, b1, nullptr, e->hbuf, M, F, H, st));
        else VFT_HIP(gemm<EPI_BIAS_GELU>(e->x, W1, b1, nullptr, e->hbuf, Mp, F, H, st, 0, &e->gws));
        if (skinny) {
            VFT_HIP(gemm_skinny<EPI_BIAS_RESIDUAL>(e->hbuf, W2, b2, e->x, e->y, M, H, F, st, e->sk_part, e->sk_cnt));
        } else if (ffn_down_splitk) {   // a single short sequence: the long-K product (K = ffn) is split over K across the chip
            VFT_HIP(gemm_splitk<EPI_BIAS_RESIDUAL>(e->hbuf, W2, b2, e->x, e->y, Ms, H, F, e->sk_part, e->sk_cnt, st));
        } else {
            VFT_HIP(gemm<EPI_BIAS_RESIDUAL>(e->hbuf, W2, b2, e->x, e->y, Mp, H, F, st, 0, &e->gws));
        }
        hipLaunchKernelGGL(k_layernorm, dim3((M + 7) / 8), dim3(256), 0, st, e->y, g2, b2n, c.ln_eps, M, H, e->x);
    }
    int all_last = 0;
    if (c.pooling == 2) {
        hipLaunchKernelGGL(k_all_last_set, dim3(1), dim3(64), 0, st, e->d_mask, B, T, Tv, e->d_flag);
        VFT_HIP(hipMemcpyAsync(&all_last, e->d_flag, 4, hipMemcpyDeviceToHost, st));
        VFT_HIP(hipStreamSynchronize(st));
    }
    const size_t pool_lds = ((size_t)H * 2 + 256) * sizeof(float);
    hipLaunchKernelGGL(k_pool, dim3(B), dim3(256), pool_lds, st, e->x, e->d_mask, T, Tv, H, c.pooling, c.normalize, all_last,
                       c.head, e->w16 + e->o_head_dense, e->w32 + e->f_head_bd, e->w16 + e->o_head_out,
                       e->w32 + e->f_head_bp, e->d_out, seq_off);
    VFT_HIP(hipGetLastError());
    return VF_OK;
}


static std::atomic<long long> g_packed_forwards{0};
// Test hook: how many forwards took the packed (ragged-batch) path in this process.
extern "C" long long vf_debug_packed_forwards() { return g_packed_forwards.load(std::memory_order_relaxed); }

// Token ids index the embedding table on the device: an id outside [0, vocab) (a tokenizer that does not belong to the model, a -1
// used as padding) would be an out-of-bounds read there -- a GPU memory fault, not an exception.  Checked here, on the host copy
// the caller hands over (b * t compares: ~15 us for 100 x 512 tokens); padded positions are looked up too, so they count.
static long long first_id_out_of_range(const int32_t* ids, size_t n, int32_t hi) {
    for (size_t i = 0; i < n; ++i)
        if ((uint32_t)ids[i] >= (uint32_t)hi) return (long long)i;
    return -1;
}

static int forward_impl(vf_encoder* e, const int32_t* ids, const int32_t* mask, const int32_t* type_ids, int32_t b,
                        int32_t t, int32_t t_valid, int32_t pooling, int32_t normalize, float* out) {
    if (!e) return fail(VF_EINVAL, "vf_encoder_forward: null handle");
    if (b < 0 || t < 0) return fail(VF_EINVAL, "vf_encoder_forward: negative sizes");
    if (b == 0) return VF_OK;
    if (!ids || !mask || !out) return fail(VF_EINVAL, "vf_encoder_forward: null buffer");
    if (t == 0 || t % 32 != 0 || t > kEncMaxT) return fail(VF_EINVAL, "vf_encoder_forward: t must be a multiple of 32 in [32, 8192] (pad with mask 0)");
    if (t_valid <= 0 || t_valid > t) return fail(VF_EINVAL, "vf_encoder_forward: t_valid must be in [1, t]");
    if (t > e->cfg.max_pos - (e->cfg.roberta_pad_idx >= 0 ? e->cfg.roberta_pad_idx + 1 : 0))
        return fail(VF_EINVAL, "vf_encoder_forward: t exceeds the position table");
    {
        const long long bad = first_id_out_of_range(ids, (size_t)b * t, e->cfg.vocab);
        if (bad >= 0) return fail(VF_EINVAL, "vf_encoder_forward: token id " + std::to_string(ids[bad]) + " at [" + std::to_string(bad / t) + ", " + std::to_string(bad % t) + "] is outside the vocabulary [0, " + std::to_string(e->cfg.vocab) + ")");
        const long long badt = type_ids ? first_id_out_of_range(type_ids, (size_t)b * t, e->cfg.type_vocab) : -1;
        if (badt >= 0) return fail(VF_EINVAL, "vf_encoder_forward: token type id " + std::to_string(type_ids[badt]) + " is outside [0, " + std::to_string(e->cfg.type_vocab) + ")");
    }
    std::lock_guard<std::mutex> g(e->mu);
    // per-call pooling / normalisation: swapped in under the handle's lock, restored on every exit path
    struct Restore {
        vf_encoder_config& c; int p, n;
        ~Restore() { c.pooling = p; c.normalize = n; }
    } restore{e->cfg, e->cfg.pooling, e->cfg.normalize};
    if (pooling >= 0) e->cfg.pooling = pooling;
    if (normalize >= 0) e->cfg.normalize = normalize;
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(e->device));
    int rc = enc_ensure_ws(e, b, t);
    if (rc != VF_OK) return rc;
    const size_t n = (size_t)b * t;
    const int out_dim = e->cfg.head == 1 ? 1 : e->cfg.hidden;
    static const bool no_graph = getenv("VF_NO_GRAPH") != nullptr;   // A/B switch
    VFT_HIP(handle_stream(&e->stream));
    hipStream_t es = e->stream;
    if (!no_graph && n <= 256 && e->cfg.pooling != 2) {   // (last-token pooling reads a flag back mid-forward: not capturable)
        hipStream_t gs = es;
        const vf_encoder::GraphKey key{b, t, t_valid, type_ids != nullptr, e->cfg.pooling, e->cfg.normalize};
        hipGraphExec_t exec = nullptr;
        for (auto& g : e->graphs) if (g.key == key) { exec = g.exec; break; }
        VFT_HIP(hipMemcpyAsync(e->d_ids, ids, n * 4, hipMemcpyHostToDevice, gs));
        VFT_HIP(hipMemcpyAsync(e->d_mask, mask, n * 4, hipMemcpyHostToDevice, gs));
        if (type_ids) VFT_HIP(hipMemcpyAsync(e->d_tt, type_ids, n * 4, hipMemcpyHostToDevice, gs));
        if (!exec) {
            hipGraph_t graph = nullptr;
            VFT_HIP(hipStreamBeginCapture(gs, hipStreamCaptureModeThreadLocal));
            rc = enc_forward_device(e, b, t, t_valid, type_ids != nullptr, gs);
            const hipError_t ce = hipStreamEndCapture(gs, &graph);
            if (rc != VF_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
            if (ce != hipSuccess) return fail(VF_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
            const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) return fail(VF_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
            if (e->graphs.size() >= 32) enc_drop_graphs(e);   // bounded cache: request shapes are few (t = 32, 64, ...)
            e->graphs.push_back({key, exec});
        }
        VFT_HIP(hipGraphLaunch(exec, gs));
        VFT_HIP(hipMemcpyAsync(out, e->d_out, (size_t)b * out_dim * 4, hipMemcpyDeviceToHost, gs));
        VFT_HIP(hipStreamSynchronize(gs));
        return VF_OK;
    }
    // Ragged batch (right-padded, CLS pooling or a classification head): the rows are PACKED -- every
    // sequence keeps ceil32(length) rows -- so the GEMMs, LayerNorms and attention only see the tokens that exist.  A row's
    // output does not depend on its neighbours or its padding (masked keys weigh exactly 0), so this is the same forward
    // on fewer rows; FlagEmbedding sorts by length for the same reason (the reference's compute_score / encode).
    static const bool no_pack = getenv("VF_NO_PACKED") != nullptr;   // A/B switch
    if (!no_pack && e->q_folded && b >= 2 && (e->cfg.head == 1 || e->cfg.pooling == 0)) {   // (any width: the streaming attention packs too)
        std::vector<int32_t>& pk = e->pk;
        pk.resize((size_t)b + 1);
        long long rows = 0;
        int tmax = 0;
        bool ok = true;
        for (int i = 0; i < b && ok; ++i) {
            const int32_t* m = mask + (size_t)i * t;
            int len = 0;
            while (len < t && m[len]) ++len;
            for (int j = len; j < t; ++j) if (m[j]) { ok = false; break; }   // not right-padded
            if (len == 0) ok = false;                                         // a sequence without tokens: the padded path
            const int l32 = (len + 31) / 32 * 32;
            pk[i] = (int32_t)rows;
            rows += l32;
            tmax = l32 > tmax ? l32 : tmax;
        }
        pk[b] = (int32_t)rows;
        if (ok && rows * 100 <= (long long)n * 85) {   // at least 15 % fewer rows
            const size_t R = (size_t)rows;
            pk.resize((size_t)b + 1 + 4 * R);
            int32_t *off = pk.data(), *pid = off + b + 1, *pmk = pid + R, *ppos = pmk + R, *ptt = ppos + R;
            const int rp = e->cfg.roberta_pad_idx;
            for (int i = 0; i < b; ++i) {
                const int r0 = off[i], l32 = off[i + 1] - off[i];
                const int32_t *si = ids + (size_t)i * t, *sm = mask + (size_t)i * t;
                for (int j = 0; j < l32; ++j) {
                    pid[r0 + j] = si[j];
                    pmk[r0 + j] = sm[j] != 0;
                    ppos[r0 + j] = rp >= 0 ? (sm[j] ? j + 1 + rp : rp) : j;      // k_position_ids on a right-padded row
                    if (type_ids) ptt[r0 + j] = type_ids[(size_t)i * t + j];
                }
            }
            VFT_HIP(hipMemcpyAsync(e->d_seq, off, ((size_t)b + 1) * 4, hipMemcpyHostToDevice, es));
            VFT_HIP(hipMemcpyAsync(e->d_ids, pid, R * 4, hipMemcpyHostToDevice, es));
            VFT_HIP(hipMemcpyAsync(e->d_mask, pmk, R * 4, hipMemcpyHostToDevice, es));
            VFT_HIP(hipMemcpyAsync(e->d_pos, ppos, R * 4, hipMemcpyHostToDevice, es));
            if (type_ids) VFT_HIP(hipMemcpyAsync(e->d_tt, ptt, R * 4, hipMemcpyHostToDevice, es));
            rc = enc_forward_device(e, b, tmax, tmax, type_ids != nullptr, es, e->d_seq, (int)rows);
            if (rc != VF_OK) return rc;
            g_packed_forwards.fetch_add(1, std::memory_order_relaxed);
            VFT_HIP(hipMemcpyAsync(out, e->d_out, (size_t)b * out_dim * 4, hipMemcpyDeviceToHost, es));
            VFT_HIP(hipStreamSynchronize(es));
            return VF_OK;
        }
    }
    VFT_HIP(hipMemcpyAsync(e->d_ids, ids, n * 4, hipMemcpyHostToDevice, es));
    VFT_HIP(hipMemcpyAsync(e->d_mask, mask, n * 4, hipMemcpyHostToDevice, es));
    if (type_ids) VFT_HIP(hipMemcpyAsync(e->d_tt, type_ids, n * 4, hipMemcpyHostToDevice, es));
    rc = enc_forward_device(e, b, t, t_valid, type_ids != nullptr, es);
    if (rc != VF_OK) return rc;
    VFT_HIP(hipMemcpyAsync(out, e->d_out, (size_t)b * out_dim * 4, hipMemcpyDeviceToHost, es));
    VFT_HIP(hipStreamSynchronize(es));
    return VF_OK;
}

extern "C" int vf_encoder_forward(vf_encoder* e, const int32_t* ids, const int32_t* mask, const int32_t* type_ids,
                                  int32_t b, int32_t t, int32_t t_valid, float* out) {
    return forward_impl(e, ids, mask, type_ids, b, t, t_valid, -1, -1, out);
}

// Same forward with the pooling / normalisation chosen per call (-1 keeps the handle's setting): get_embeddings'
// callers pick "last token" or "unmasked mean" per call site (step3_mul.py:203-207, continuous_retrieval.py:146-149)
// on one loaded model.  Only for embedding handles (head == 0).
extern "C" int vf_encoder_forward_pooled(vf_encoder* e, const int32_t* ids, const int32_t* mask, const int32_t* type_ids,
                                         int32_t b, int32_t t, int32_t t_valid, int32_t pooling, int32_t normalize,
                                         float* out) {
    if (!e) return fail(VF_EINVAL, "vf_encoder_forward_pooled: null handle");
    if (e->cfg.head != 0) return fail(VF_EINVAL, "vf_encoder_forward_pooled: handle is a re-ranker");
    if (pooling < -1 || pooling > 3 || normalize < -1 || normalize > 1)
        return fail(VF_EINVAL, "vf_encoder_forward_pooled: pooling must be -1..3, normalize -1..1");
    return forward_impl(e, ids, mask, type_ids, b, t, t_valid, pooling, normalize, out);
}

// last_hidden_state [b, t, hidden] fp32 (what the reference's get_embeddings pools itself:
// experiments/retriever/step3_mul.py:203-207, continuous_retrieval.py:146-149)
extern "C" int vf_encoder_forward_hidden(vf_encoder* e, const int32_t* ids, const int32_t* mask, const int32_t* type_ids,
                                         int32_t b, int32_t t, float* out_hidden) {
    if (!e) return fail(VF_EINVAL, "vf_encoder_forward_hidden: null handle");
    if (b < 0 || t < 0) return fail(VF_EINVAL, "vf_encoder_forward_hidden: negative sizes");
    if (b == 0) return VF_OK;
    if (!ids || !mask || !out_hidden) return fail(VF_EINVAL, "vf_encoder_forward_hidden: null buffer");
    if (t == 0 || t % 32 != 0 || t > kEncMaxT) return fail(VF_EINVAL, "vf_encoder_forward_hidden: t must be a multiple of 32 in [32, 8192]");
    if (t > e->cfg.max_pos - (e->cfg.roberta_pad_idx >= 0 ? e->cfg.roberta_pad_idx + 1 : 0))
        return fail(VF_EINVAL, "vf_encoder_forward_hidden: t exceeds the position table");
    {
        const long long bad = first_id_out_of_range(ids, (size_t)b * t, e->cfg.vocab);
        if (bad >= 0) return fail(VF_EINVAL, "vf_encoder_forward_hidden: token id " + std::to_string(ids[bad]) + " is outside the vocabulary [0, " + std::to_string(e->cfg.vocab) + ")");
        const long long badt = type_ids ? first_id_out_of_range(type_ids, (size_t)b * t, e->cfg.type_vocab) : -1;
        if (badt >= 0) return fail(VF_EINVAL, "vf_encoder_forward_hidden: token type id " + std::to_string(type_ids[badt]) + " is outside [0, " + std::to_string(e->cfg.type_vocab) + ")");
    }
    std::lock_guard<std::mutex> g(e->mu);
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(e->device));
    int rc = enc_ensure_ws(e, b, t);
    if (rc != VF_OK) return rc;
    const size_t n = (size_t)b * t;
    VFT_HIP(handle_stream(&e->stream));
    hipStream_t es = e->stream;
    VFT_HIP(hipMemcpyAsync(e->d_ids, ids, n * 4, hipMemcpyHostToDevice, es));
    VFT_HIP(hipMemcpyAsync(e->d_mask, mask, n * 4, hipMemcpyHostToDevice, es));
    if (type_ids) VFT_HIP(hipMemcpyAsync(e->d_tt, type_ids, n * 4, hipMemcpyHostToDevice, es));
    rc = enc_forward_device(e, b, t, t, type_ids != nullptr, es);
    if (rc != VF_OK) return rc;
    const long long tot = (long long)n * e->cfg.hidden;
    hipLaunchKernelGGL(k_to_f32, dim3(1024), dim3(256), 0, es, e->x, tot, e->d_hidden);
    VFT_HIP(hipMemcpyAsync(out_hidden, e->d_hidden, (size_t)tot * 4, hipMemcpyDeviceToHost, es));
    VFT_HIP(hipStreamSynchronize(es));
    return VF_OK;
}

extern "C" int vf_encoder_info(vf_encoder* e, vf_encoder_config* out) {
    if (!e || !out) return fail(VF_EINVAL, "vf_encoder_info: null argument");
    *out = e->cfg;
    return VF_OK;
}

// the re-ranker is an encoder with head == 1: same object, named entry points for the reference's
// compute_score (src/utils/vllmManager.py:451)
extern "C" int vf_reranker_create(vf_encoder** out, const vf_encoder_config* cfg, const void* w16, int64_t n16,
                                  const float* w32, int64_t n32, int32_t device_id) {
    if (cfg && cfg->head != 1) return fail(VF_EINVAL, "vf_reranker_create: config.head must be 1");
    return vf_encoder_create(out, cfg, w16, n16, w32, n32, device_id);
}
extern "C" int vf_reranker_score(vf_encoder* e, const int32_t* ids, const int32_t* mask, const int32_t* type_ids,
                                 int32_t b, int32_t t, float* out_scores) {
    if (e && e->cfg.head != 1) return fail(VF_EINVAL, "vf_reranker_score: handle is not a re-ranker");
    return vf_encoder_forward(e, ids, mask, type_ids, b, t, t, out_scores);
}
extern "C" int vf_reranker_destroy(vf_encoder* e) { return vf_encoder_destroy(e); }


// ------------------------------------------------------------------------------------------------
// Decoder-only model handle (vf_decoder_*): see the kernel block above and include/veritasfi_hip.h.
// ------------------------------------------------------------------------------------------------
constexpr int kDecMaxT = 4096;  // the reference truncates at max_length=4096 (step3_mul.py:200); streaming attention has no residency limit, the RoPE table is sized for this

struct vf_decoder : ModelBase {
    vf_decoder_config cfg{};
    size_t o_embed = 0, o_layers = 0, layer16 = 0, o_head_row = 0;  // fp16 offsets (elements)
    size_t f_layers = 0, layer32 = 0, f_final = 0;                   // fp32 offsets
    int cap_tokens = 0, cap_b = 0, rope_T = 0;
    float *x = nullptr, *y = nullptr;   // the residual stream, FP32 (ping-pong)
    half_t *n = nullptr, *qkv = nullptr, *ctx = nullptr, *gu = nullptr, *act = nullptr;
    int *d_ids = nullptr, *d_mask = nullptr, *d_flag = nullptr;
    int *d_seq = nullptr, *d_pos = nullptr;   // packed (ragged-batch) forward: row offsets [cap_b + 1], RoPE positions [cap_tokens]
    std::vector<int32_t> pk;                  // its host staging
    float* d_out = nullptr;
    float* d_hidden = nullptr;   // [cap_tokens, H] fp32 final hidden states (vf_decoder_forward_hidden)
    float2* rope = nullptr;
};

static size_t dec_qd(const vf_decoder_config& c) { return (size_t)c.heads * c.head_dim; }
static size_t dec_kd(const vf_decoder_config& c) { return (size_t)c.kv_heads * c.head_dim; }
static size_t dec_layer16(const vf_decoder_config& c) {
    const size_t H = c.hidden, F = c.ffn, QD = dec_qd(c), KD = dec_kd(c);
    return (QD + 2 * KD) * H + H * QD + 2 * F * H + H * F;
}
static size_t dec_layer32(const vf_decoder_config& c) { return 2 * (size_t)c.hidden + 2 * (size_t)c.head_dim; }
static size_t dec_n16(const vf_decoder_config& c) {
    return (size_t)c.vocab * c.hidden + (size_t)c.layers * dec_layer16(c) + (c.head == 2 ? (size_t)c.hidden : 0);
}
static size_t dec_n32(const vf_decoder_config& c) { return (size_t)c.layers * dec_layer32(c) + (size_t)c.hidden; }

static int dec_check_cfg(const vf_decoder_config* c) {
    if (!c) return fail(VF_EINVAL, "vf_decoder: null config");
    if (c->vocab <= 0 || c->layers <= 0 || c->heads <= 0 || c->kv_heads <= 0 || c->heads % c->kv_heads != 0)
        return fail(VF_EINVAL, "vf_decoder: bad vocab / layers / heads / kv_heads");
    if (c->head_dim != 64 && c->head_dim != 128 && c->head_dim != 256)
        return fail(VF_EUNSUPPORTED, "vf_decoder: head_dim must be 64, 128 or 256");
    if (c->act != 0 && c->act != 1) return fail(VF_EINVAL, "vf_decoder: act must be 0 (SiLU) or 1 (tanh-GELU)");
    if (c->hidden <= 0 || c->hidden % 128 != 0 || c->ffn <= 0 || c->ffn % 64 != 0)
        return fail(VF_EUNSUPPORTED, "vf_decoder: hidden must be a multiple of 128, ffn of 64");
    if ((dec_qd(*c) + 2 * dec_kd(*c)) % 128 != 0 || dec_qd(*c) % 64 != 0)
        return fail(VF_EUNSUPPORTED, "vf_decoder: (heads + 2 kv_heads) * head_dim must be a multiple of 128");
    if (c->pooling < 0 || c->pooling > 2 || (c->head != 0 && c->head != 2)) return fail(VF_EINVAL, "vf_decoder: bad pooling / head");
    if (!(c->rope_theta > 0.f) || !(c->rms_eps > 0.f)) return fail(VF_EINVAL, "vf_decoder: rope_theta and rms_eps must be positive");
    return VF_OK;
}

extern "C" int vf_decoder_weight_sizes(const vf_decoder_config* cfg, int64_t* n_fp16, int64_t* n_fp32) {
    if (!n_fp16 || !n_fp32) return fail(VF_EINVAL, "vf_decoder_weight_sizes: null argument");
    const int rc = dec_check_cfg(cfg);
    if (rc != VF_OK) return rc;
    *n_fp16 = (int64_t)dec_n16(*cfg);
    *n_fp32 = (int64_t)dec_n32(*cfg);
    return VF_OK;
}

extern "C" int vf_decoder_destroy(vf_decoder* d) {
    if (!d) return VF_OK;
    vf::DeviceGuard guard;
    (void)hipSetDevice(d->device);
    model_release(*d);
    if (d->d_flag) (void)hipFree(d->d_flag);
    delete d;
    return VF_OK;
}

extern "C" int vf_decoder_create(vf_decoder** out, const vf_decoder_config* cfg, const void* w16, int64_t n16,
                                 const float* w32, int64_t n32, int32_t device_id) {
    if (!out) return fail(VF_EINVAL, "vf_decoder_create: null out");
    *out = nullptr;
    int rc = dec_check_cfg(cfg);
    if (rc != VF_OK) return rc;
    if (!w16 || !w32 || n16 != (int64_t)dec_n16(*cfg) || n32 != (int64_t)dec_n32(*cfg))
        return fail(VF_EINVAL, "vf_decoder_create: weight blobs do not match vf_decoder_weight_sizes");
    VFT_TRY(model_check_device(device_id, "vf_decoder_create"));
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(device_id));
    vf_decoder* d = new (std::nothrow) vf_decoder();
    if (!d) return fail(VF_ENOMEM, "vf_decoder_create: host allocation failed");
    d->cfg = *cfg; d->device = device_id;
    d->o_embed = 0;
    d->o_layers = (size_t)cfg->vocab * cfg->hidden;
    d->layer16 = dec_layer16(*cfg);
    d->o_head_row = d->o_layers + (size_t)cfg->layers * d->layer16;
    d->f_layers = 0; d->layer32 = dec_layer32(*cfg); d->f_final = (size_t)cfg->layers * d->layer32;
    hipError_t er = model_upload(*d, w16, n16, w32, n32);
    if (er == hipSuccess) er = hipMalloc((void**)&d->d_flag, 4);
    if (er != hipSuccess) return model_create_failed(d, vf_decoder_destroy, "vf_decoder_create", er);
    *out = d;
    return VF_OK;
}

// ---- the launches of the decoder's kernels: grid and block arithmetic in ONE place each, shared by the forward below and by the
//      vf_debug_dec_* test hooks (tests/test_gpu_decoder_kernels.py), so that a test of one kernel runs production's launch ----
static void dec_launch_rope_table(float theta, int T, int dh, float2* tab, hipStream_t st) {
    const int cells = T * (dh / 2);
    hipLaunchKernelGGL(k_rope_table, dim3((cells + 255) / 256), dim3(256), 0, st, theta, T, dh, tab);
}
static void dec_launch_gather_rows(const int* ids, const half_t* table, int M, int H, float scale, float* out, hipStream_t st) {
    hipLaunchKernelGGL(k_gather_rows, dim3((M + 7) / 8), dim3(256), 0, st, ids, table, M, H, scale, out);
}
template <typename TOUT>
static void dec_launch_rmsnorm(const float* x, const float* w, float woff, float eps, int M, int H, TOUT* y, hipStream_t st) {
    hipLaunchKernelGGL(k_rmsnorm<TOUT>, dim3((M + 7) / 8), dim3(256), 0, st, x, w, woff, eps, M, H, y);
}
static void dec_launch_qknorm_rope(half_t* qkv, int M, int T, int ld, int heads, int kv_heads, int DH, const float* qw, const float* kw,
                                   float eps, int qk_norm, const float2* tab, const int* pos, hipStream_t st) {
    const int tpw = 256 / (DH / 16);   // tokens per workgroup: 64, 32 or 16
    hipLaunchKernelGGL(k_qknorm_rope, dim3((M + tpw - 1) / tpw, 3), dim3(256), 0, st, qkv, M, T, ld, heads, kv_heads, DH, qw, kw, eps,
                       qk_norm, tab, pos);
}
// causal grouped-query attention over qkv rows of ld elements; false: no kernel for this head dim (nothing launched)
static bool dec_launch_attention(const half_t* qkv, const int* mask, const int* seq_off, int b, int t, int ld, int heads, int kv_heads,
                                 int DH, float scale, half_t* ctx, int ctx_ld, hipStream_t st) {
    const dim3 agrid((t + 127) / 128, heads, b);
    if (DH == 64) {
        hipLaunchKernelGGL((k_attention_stream2<64, true>), agrid, dim3(256), sizeof(AttnStream2Lds<64>), st, qkv, mask, t, ld, heads,
                           kv_heads, scale, ctx, ctx_ld, seq_off);
    } else if (DH == 128) {
        hipLaunchKernelGGL((k_attention_stream2<128, true>), agrid, dim3(256), sizeof(AttnStream2Lds<128>), st, qkv, mask, t, ld, heads,
                           kv_heads, scale, ctx, ctx_ld, seq_off);
    } else if (DH == 256) {
        hipLaunchKernelGGL((k_attention_stream2<256, true>), agrid, dim3(256), sizeof(AttnStream2Lds<256>), st, qkv, mask, t, ld, heads,
                           kv_heads, scale, ctx, ctx_ld, seq_off);
    } else {
        return false;
    }
    return true;
}
static void dec_launch_swiglu(const half_t* gu, int M, int F, int act_kind, half_t* act, hipStream_t st) {
    hipLaunchKernelGGL(k_swiglu, dim3(((F >> 3) + 255) / 256, M < 32768 ? M : 32768), dim3(256), 0, st, gu, (long long)M, F, act_kind, act);
}
static void dec_launch_token_logit(const half_t* x, const int* mask, int b, int T, int Tv, int H, int all_last, const half_t* row,
                                   float* out, const int* seq_off, hipStream_t st) {
    hipLaunchKernelGGL(k_token_logit, dim3(b), dim3(64), 0, st, x, mask, T, Tv, H, all_last, row, out, seq_off);
}
static void dec_launch_pool(const half_t* x, const int* mask, int b, int T, int Tv, int H, int pooling, int normalize, int all_last,
                            float* out, const int* seq_off, hipStream_t st) {
    const size_t pool_lds = ((size_t)H * 2 + 256) * sizeof(float);
    hipLaunchKernelGGL(k_pool, dim3(b), dim3(256), pool_lds, st, x, mask, T, Tv, H, pooling, normalize, all_last, 0, nullptr, nullptr,
                       nullptr, nullptr, out, seq_off);
}

static int dec_ensure_ws(vf_decoder* d, int B, int T) {
    VFT_HIP(handle_stream(&d->stream));
    int tokens = (B * T + 255) / 256 * 256;
    if (tokens <= d->cap_tokens && B <= d->cap_b && T <= d->rope_T) return VF_OK;
    tokens = std::max(tokens, d->cap_tokens); B = std::max(B, d->cap_b);   // monotone growth (see enc_ensure_ws)
    d->ws.free_all();
    d->cap_tokens = d->cap_b = d->rope_T = 0;
    const vf_decoder_config& c = d->cfg;
    const size_t H = c.hidden, F = c.ffn, QKV = dec_qd(c) + 2 * dec_kd(c), QD = dec_qd(c), Mp = tokens;
    DevPool& ws = d->ws;
    hipStream_t st = d->stream;
    // (zeroed: padded rows are read by the GEMMs, keep them finite)
    VFT_HIP(ws.get(&d->x, Mp * H * 4, true, st));
    VFT_HIP(ws.get(&d->y, Mp * H * 4, true, st));
    VFT_HIP(ws.get(&d->d_hidden, Mp * H * 4, false, st));
    VFT_HIP(ws.get(&d->n, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&d->qkv, Mp * QKV * 2, true, st));
    VFT_HIP(ws.get(&d->ctx, Mp * QD * 2, true, st));
    VFT_HIP(ws.get(&d->gu, Mp * 2 * F * 2, true, st));
    VFT_HIP(ws.get(&d->act, Mp * F * 2, true, st));
    VFT_HIP(ws.get(&d->d_ids, Mp * 4, false, st));
    VFT_HIP(ws.get(&d->d_mask, Mp * 4, false, st));
    VFT_HIP(ws.get(&d->d_pos, Mp * 4, false, st));
    VFT_HIP(ws.get(&d->d_seq, ((size_t)B + 1) * 4, false, st));
    VFT_HIP(ws.get(&d->d_out, (size_t)B * (c.head == 2 ? 1 : H) * 4, false, st));
    VFT_HIP(ws.get(&d->rope, (size_t)kDecMaxT * (c.head_dim / 2) * sizeof(float2), false, st));
    // on the handle's own stream, like the zero fills: the forwards run there, and a non-blocking stream does not order itself behind
    // the NULL stream (round-5 advisor: the first forward after a (re)allocation could read a table not written yet)
    dec_launch_rope_table(c.rope_theta, kDecMaxT, c.head_dim, d->rope, st);
    VFT_HIP(hipGetLastError());
    d->cap_tokens = tokens; d->cap_b = B; d->rope_T = kDecMaxT;
    VFT_HIP(gws_ensure(d->gws, st));
    return VF_OK;
}

// The layers: ids / mask already in d->d_ids / d->d_mask.  Returns the final residual stream (fp32, device) in *xfinal.
// seq_off != nullptr: PACKED rows (vf_decoder_forward's ragged-batch path) -- Mpk rows in all, sequence i in rows
// [seq_off[i], seq_off[i + 1]) with its valid tokens first, t = the longest; pos = each row's RoPE position.
static int dec_layers_device(vf_decoder* d, int b, int t, hipStream_t st, float** xfinal, const int* seq_off = nullptr, int Mpk = 0,
                             const int* pos = nullptr) {
    const vf_decoder_config& c = d->cfg;
    const int H = c.hidden, F = c.ffn, DH = c.head_dim, QD = (int)dec_qd(c), KD = (int)dec_kd(c), QKV = QD + 2 * KD;
    const int M = seq_off ? Mpk : b * t, Mp = (M + 255) / 256 * 256;
    dec_launch_gather_rows(d->d_ids, d->w16 + d->o_embed, M, H, c.embed_scale > 0.f ? c.embed_scale : 1.0f, d->x, st);
    float *px = d->x, *py = d->y;   // residual stream in fp32; GEMM operands (d->n, d->ctx, d->act) in fp16
    const float scale = 1.0f / sqrtf((float)DH);
    const float woff = c.norm_plus_one ? 1.0f : 0.0f;
    for (int l = 0; l < c.layers; ++l) {
        const half_t* W = d->w16 + d->o_layers + (size_t)l * d->layer16;
        const half_t *Wqkv = W, *Wo = Wqkv + (size_t)QKV * H, *Wgu = Wo + (size_t)H * QD, *Wdn = Wgu + (size_t)2 * F * H;
        const float* P = d->w32 + d->f_layers + (size_t)l * d->layer32;
        const float *ln1 = P, *ln2 = P + H, *qn = P + 2 * H, *kn = qn + DH;
        dec_launch_rmsnorm<half_t>(px, ln1, woff, c.rms_eps, M, H, d->n, st);
        VFT_HIP(gemm<EPI_BIAS>(d->n, Wqkv, nullptr, nullptr, d->qkv, Mp, QKV, H, st, 0, &d->gws));
        dec_launch_qknorm_rope(d->qkv, M, t, QKV, c.heads, c.kv_heads, DH, qn, kn, c.rms_eps, c.qk_norm, d->rope, pos, st);
        dec_launch_attention(d->qkv, d->d_mask, seq_off, b, t, QKV, c.heads, c.kv_heads, DH, scale, d->ctx, QD, st);   // (head dim checked at create)
        VFT_HIP(gemm<EPI_RESIDUAL_F32>(d->ctx, Wo, nullptr, (const half_t*)px, (half_t*)py, Mp, H, QD, st));
        std::swap(px, py);
        dec_launch_rmsnorm<half_t>(px, ln2, woff, c.rms_eps, M, H, d->n, st);
        hipError_t ger = hipSuccess;
        if (!gemm_gated(d->n, Wgu, d->act, Mp, F, H, c.act, st, &ger)) {   // gate / up products and the activation in one launch
            VFT_HIP(gemm<EPI_BIAS>(d->n, Wgu, nullptr, nullptr, d->gu, Mp, 2 * F, H, st, 0, &d->gws));
            dec_launch_swiglu(d->gu, M, F, c.act, d->act, st);
        }
        VFT_HIP(ger);
        VFT_HIP(gemm<EPI_RESIDUAL_F32>(d->act, Wdn, nullptr, (const half_t*)px, (half_t*)py, Mp, H, F, st));
        std::swap(px, py);
    }
    VFT_HIP(hipGetLastError());
    *xfinal = px;
    return VF_OK;
}

static int dec_check_call(vf_decoder* d, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t, const void* out, const char* who) {
    if (!d) return fail(VF_EINVAL, std::string(who) + ": null handle");
    if (b < 0 || t < 0) return fail(VF_EINVAL, std::string(who) + ": negative sizes");
    if (b > 0 && (!ids || !mask || !out)) return fail(VF_EINVAL, std::string(who) + ": null buffer");
    if (b > 0 && (t == 0 || t % 32 != 0 || t > kDecMaxT))
        return fail(VF_EINVAL, std::string(who) + ": t must be a multiple of 32 in [32, 4096] (pad with mask 0)");
    if (b > 0) {
        const long long bad = first_id_out_of_range(ids, (size_t)b * t, d->cfg.vocab);
        if (bad >= 0) return fail(VF_EINVAL, std::string(who) + ": token id " + std::to_string(ids[bad]) + " at [" + std::to_string(bad / t) + ", " + std::to_string(bad % t) + "] is outside the vocabulary [0, " + std::to_string(d->cfg.vocab) + ")");
    }
    return VF_OK;
}

// ids / mask [b, t] int32 host (t % 32 == 0, t <= 4096; right- or left-padded with mask 0); t_valid = columns the
// tokenizer produced.  out: [b, hidden] fp32 (head 0) or [b] fp32 (head 2).
static int dec_forward_impl(vf_decoder* d, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t, int32_t t_valid, int32_t normalize,
                            float* out);

extern "C" int vf_decoder_forward(vf_decoder* d, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t,
                                  int32_t t_valid, float* out) {
    return dec_forward_impl(d, ids, mask, b, t, t_valid, -1, out);
}

// The same forward with the L2 normalisation of the pooled row chosen per call (-1: the handle's, 0 / 1): an embedder wrapper
// (HipDecoderEmbeddings: last_token_pool + normalize, continuous_retrieval.py:55-60) gets unit vectors out of the pooling kernel
// whatever the handle was created with, instead of a NumPy pass on the host.  Head 2 (the token logit) has nothing to normalise.
extern "C" int vf_decoder_forward_pooled(vf_decoder* d, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t, int32_t t_valid,
                                         int32_t normalize, float* out) {
    if (normalize < -1 || normalize > 1) return fail(VF_EINVAL, "vf_decoder_forward_pooled: normalize must be -1, 0 or 1");
    return dec_forward_impl(d, ids, mask, b, t, t_valid, normalize, out);
}

static int dec_forward_impl(vf_decoder* d, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t, int32_t t_valid, int32_t normalize,
                            float* out) {
    VFT_TRY(dec_check_call(d, ids, mask, b, t, out, "vf_decoder_forward"));
    if (b == 0) return VF_OK;
    if (t_valid <= 0 || t_valid > t) return fail(VF_EINVAL, "vf_decoder_forward: t_valid must be in [1, t]");
    std::lock_guard<std::mutex> g(d->mu);
    struct Restore {   // per-call normalisation: swapped in under the handle's lock, restored on every exit path
        vf_decoder_config& c; int n;
        ~Restore() { c.normalize = n; }
    } restore{d->cfg, d->cfg.normalize};
    if (normalize >= 0 && d->cfg.head != 2) d->cfg.normalize = normalize;
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(d->device));
    int rc = dec_ensure_ws(d, b, t);
    if (rc != VF_OK) return rc;
    const vf_decoder_config& c = d->cfg;
    const int H = c.hidden, M = b * t;
    VFT_HIP(handle_stream(&d->stream));
    hipStream_t st = d->stream;
    const size_t ntok = (size_t)b * t;
    // Ragged batch, padded on ONE side throughout (the tokenizer's left or right padding), last-token pooling or the
    // token-logit head: the rows are PACKED -- a sequence keeps ceil32(length) rows, valid tokens first, each carrying its
    // original column as RoPE position -- and the layers only see the tokens that exist (as the encoder's forward_impl).
    // The pooled row is the last valid token, which is what last_token_pool (step3_mul.py:181-188) and logits[:, -1]
    // (stress_test.py:212-225) select on one-sided padding.
    static const bool no_pack = getenv("VF_NO_PACKED") != nullptr;   // A/B switch
    if (!no_pack && b >= 4 && (c.pooling == 2 || c.head == 2)) {
        std::vector<int32_t>& pk = d->pk;
        pk.assign((size_t)3 * b + 1, 0);
        int32_t *off = pk.data(), *first = off + b + 1, *lens = first + b;
        long long rows = 0;
        int tmax = 0;
        bool ok = true, all_left = true, all_right = true;
        for (int i = 0; i < b && ok; ++i) {
            const int32_t* m = mask + (size_t)i * t;
            int f = 0;
            while (f < t_valid && !m[f]) ++f;
            int e2 = f;
            while (e2 < t_valid && m[e2]) ++e2;
            for (int j = e2; j < t; ++j) if (m[j]) { ok = false; break; }   // more than one run of tokens
            if (e2 == f) ok = false;                                         // no token at all: the padded path
            all_right = all_right && f == 0;
            // LEFT padding is judged against the columns the tokenizer produced (t_valid), not the 32-aligned t: the
            // caller's alignment columns sit on the right of a left-padded batch whose width is not a multiple of 32
            all_left = all_left && e2 == t_valid;
            const int l32 = (e2 - f + 31) / 32 * 32;
            off[i] = (int32_t)rows; first[i] = f; lens[i] = e2 - f;
            rows += l32;
            tmax = l32 > tmax ? l32 : tmax;
        }
        off[b] = (int32_t)rows;
        if (ok && (all_left || all_right) && rows * 100 <= (long long)ntok * 85) {
            const size_t R = (size_t)rows;
            const size_t head = (size_t)3 * b + 1;
            pk.resize(head + 3 * R);
            off = pk.data(); first = off + b + 1; lens = first + b;
            int32_t *pid = pk.data() + head, *pmk = pid + R, *ppos = pmk + R;
            for (int i = 0; i < b; ++i) {
                const int r0 = off[i], l32 = off[i + 1] - off[i], f = first[i], n = lens[i];
                const int32_t* si = ids + (size_t)i * t;
                for (int j = 0; j < l32; ++j) {
                    const bool v = j < n;
                    pid[r0 + j] = si[v ? f + j : f];
                    pmk[r0 + j] = v;
                    ppos[r0 + j] = v ? f + j : 0;
                }
            }
            VFT_HIP(hipMemcpyAsync(d->d_seq, off, ((size_t)b + 1) * 4, hipMemcpyHostToDevice, st));
            VFT_HIP(hipMemcpyAsync(d->d_ids, pid, R * 4, hipMemcpyHostToDevice, st));
            VFT_HIP(hipMemcpyAsync(d->d_mask, pmk, R * 4, hipMemcpyHostToDevice, st));
            VFT_HIP(hipMemcpyAsync(d->d_pos, ppos, R * 4, hipMemcpyHostToDevice, st));
            float* pxp = nullptr;
            VFT_TRY(dec_layers_device(d, b, tmax, st, &pxp, d->d_seq, (int)rows, d->d_pos));
            const float woffp = c.norm_plus_one ? 1.0f : 0.0f;
            dec_launch_rmsnorm<half_t>(pxp, d->w32 + d->f_final, woffp, c.rms_eps, (int)rows, H, d->n, st);
            if (c.head == 2) dec_launch_token_logit(d->n, d->d_mask, b, tmax, tmax, H, 0, d->w16 + d->o_head_row, d->d_out, d->d_seq, st);
            else dec_launch_pool(d->n, d->d_mask, b, tmax, tmax, H, c.pooling, c.normalize, 0, d->d_out, d->d_seq, st);
            VFT_HIP(hipGetLastError());
            VFT_HIP(hipMemcpyAsync(out, d->d_out, (size_t)b * (c.head == 2 ? 1 : H) * 4, hipMemcpyDeviceToHost, st));
            VFT_HIP(hipStreamSynchronize(st));
            g_packed_forwards.fetch_add(1, std::memory_order_relaxed);
            return VF_OK;
        }
    }
    VFT_HIP(hipMemcpyAsync(d->d_ids, ids, ntok * 4, hipMemcpyHostToDevice, st));
    VFT_HIP(hipMemcpyAsync(d->d_mask, mask, ntok * 4, hipMemcpyHostToDevice, st));
    float* px = nullptr;
    VFT_TRY(dec_layers_device(d, b, t, st, &px));
    const float woff = c.norm_plus_one ? 1.0f : 0.0f;
    dec_launch_rmsnorm<half_t>(px, d->w32 + d->f_final, woff, c.rms_eps, M, H, d->n, st);
    int all_last = 0;
    if (c.pooling == 2 || c.head == 2) {
        hipLaunchKernelGGL(k_all_last_set, dim3(1), dim3(64), 0, st, d->d_mask, b, t, t_valid, d->d_flag);
        VFT_HIP(hipMemcpyAsync(&all_last, d->d_flag, 4, hipMemcpyDeviceToHost, st));
        VFT_HIP(hipStreamSynchronize(st));
    }
    if (c.head == 2) dec_launch_token_logit(d->n, d->d_mask, b, t, t_valid, H, all_last, d->w16 + d->o_head_row, d->d_out, nullptr, st);
    else dec_launch_pool(d->n, d->d_mask, b, t, t_valid, H, c.pooling, c.normalize, all_last, d->d_out, nullptr, st);
    VFT_HIP(hipGetLastError());
    VFT_HIP(hipMemcpyAsync(out, d->d_out, (size_t)b * (c.head == 2 ? 1 : H) * 4, hipMemcpyDeviceToHost, st));
    VFT_HIP(hipStreamSynchronize(st));
    return VF_OK;
}

// last_hidden_state [b, t, hidden] fp32 host: the final RMSNorm of the fp32 residual stream, what HF's model(**inputs)
// returns and the reference's generic route pools itself (experiments/retriever/step3_mul.py:203-207:
// outputs.last_hidden_state -> last_token_pool).
extern "C" int vf_decoder_forward_hidden(vf_decoder* d, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t,
                                         float* out_hidden) {
    VFT_TRY(dec_check_call(d, ids, mask, b, t, out_hidden, "vf_decoder_forward_hidden"));
    if (b == 0) return VF_OK;
    std::lock_guard<std::mutex> g(d->mu);
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(d->device));
    int rc = dec_ensure_ws(d, b, t);
    if (rc != VF_OK) return rc;
    const vf_decoder_config& c = d->cfg;
    const int H = c.hidden, M = b * t;
    VFT_HIP(handle_stream(&d->stream));
    hipStream_t st = d->stream;
    const size_t ntok = (size_t)b * t;
    VFT_HIP(hipMemcpyAsync(d->d_ids, ids, ntok * 4, hipMemcpyHostToDevice, st));
    VFT_HIP(hipMemcpyAsync(d->d_mask, mask, ntok * 4, hipMemcpyHostToDevice, st));
    float* px = nullptr;
    VFT_TRY(dec_layers_device(d, b, t, st, &px));
    dec_launch_rmsnorm<float>(px, d->w32 + d->f_final, c.norm_plus_one ? 1.0f : 0.0f, c.rms_eps, M, H, d->d_hidden, st);
    VFT_HIP(hipGetLastError());
    VFT_HIP(hipMemcpyAsync(out_hidden, d->d_hidden, ntok * H * 4, hipMemcpyDeviceToHost, st));
    VFT_HIP(hipStreamSynchronize(st));
    return VF_OK;
}

// ------------------------------------------------------------------------------------------------
// Vision tower (CLIP-style ViT): the "figure encoder" BASELINE configs[3] names next to the text encoder.  The reference
// holds no image model (grep -ri "clip\|vit" /root/reference: nothing), so the contract is the third-party model the
// config names -- transformers' CLIPVisionModelWithProjection: patch embedding (a strided convolution = a product over
// unfolded patches), class token + learned positions, LayerNorm, PRE-LayerNorm transformer layers (x += Wo attn(LN1 x);
// x += W2 act(W1 LN2 x)), LayerNorm of the class token, linear projection to the joint space (768 for ViT-L/14).
// Everything runs on the encoder's kernels: the products (gemm<EPI>), k_attention2 with the key-padding mask for the
// rows that pad 257 / 197 / 50 tokens to a multiple of 32, k_layernorm.  New here: the patch unfold, the embedding
// assembly + first LayerNorm, the quick-GELU epilogue of the products (EPI_BIAS_QGELU: x sigmoid(1.702 x), CLIP's
// activation), and the class-token head.
// ------------------------------------------------------------------------------------------------
struct vf_vit : ModelBase {
    vf_vit_config cfg{};
    int P = 0, T = 0, Tp = 0, Kp = 0;     // patches per image, tokens (P + 1), tokens padded to 32, patch length padded to 64
    size_t o_patch = 0, o_cls = 0, o_pos = 0, o_layers = 0, o_proj = 0, layer16 = 0;
    size_t f_zero = 0, f_pre = 0, f_layers = 0, f_post = 0, layer32 = 0;
    int cap_b = 0;
    float* d_pix = nullptr;
    half_t *patches = nullptr, *emb = nullptr, *x = nullptr, *y = nullptr, *t = nullptr, *qkv = nullptr, *ctx = nullptr, *hbuf = nullptr;
    int* d_mask = nullptr;
    float* d_out = nullptr;
};

static size_t vit_n16(const vf_vit_config& c) {
    const size_t H = c.hidden, F = c.ffn, g = c.image / c.patch, P = g * g, Kp = ((size_t)c.channels * c.patch * c.patch + 63) / 64 * 64;
    return H * Kp + H + (P + 1) * H + (size_t)c.layers * bert_layer16(H, F) + (size_t)c.proj_dim * H;
}
static size_t vit_n32(const vf_vit_config& c) {
    const size_t H = c.hidden, F = c.ffn;
    return 2 * H + (size_t)c.layers * preln_layer32(H, F) + 2 * H;
}
extern "C" int vf_vit_weight_sizes(const vf_vit_config* cfg, int64_t* n_fp16, int64_t* n_fp32) {
    if (!cfg || !n_fp16 || !n_fp32) return fail(VF_EINVAL, "vf_vit_weight_sizes: null argument");
    if (cfg->patch <= 0 || cfg->image <= 0) return fail(VF_EINVAL, "vf_vit_weight_sizes: bad config");
    *n_fp16 = (int64_t)vit_n16(*cfg);
    *n_fp32 = (int64_t)vit_n32(*cfg);
    return VF_OK;
}

// pixels [B][C][S][S] fp32 -> patches [B P][Kp] fp16, element (c, i, j) of a patch at c p p + i p + j (the Conv2d weight's own
// flattening); columns >= C p p and rows >= B P (up to rows_p) are zero
// (PIX = unsigned char: raw 0..255 pixels, normalised here as (x / 255 - mean[c]) / std[c] = x * sc[c] + sh[c] -- a quarter of the
// PCIe bytes of fp32 pixels, which at 200 images per call is a fifth of the whole forward)
template <typename PIX>
__global__ __launch_bounds__(256) void k_vit_unfold(const PIX* __restrict__ pix, int B, int C, int S, int p, int Kp, int rows_p,
                                                    float sc0, float sc1, float sc2, float sh0, float sh1, float sh2,
                                                    half_t* __restrict__ out) {
    const int g = S / p, P = g * g, K = C * p * p;
    const long long n = (long long)rows_p * Kp;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int row = (int)(i / Kp), k = (int)(i - (long long)row * Kp);
        float v = 0.f;
        if (row < B * P && k < K) {
            const int b = row / P, pi = row - b * P, py = pi / g, px = pi - py * g;
            const int c = k / (p * p), r = k - c * p * p, iy = r / p, ix = r - iy * p;
            v = (float)pix[(((long long)b * C + c) * S + (py * p + iy)) * S + (px * p + ix)];
            if constexpr (sizeof(PIX) == 1) v = v * (c == 0 ? sc0 : c == 1 ? sc1 : sc2) + (c == 0 ? sh0 : c == 1 ? sh1 : sh2);
        }
        out[i] = (half_t)v;
    }
}

// token rows: [cls + pos 0 | patch embeddings + pos 1..P | zero rows up to Tp], then the first LayerNorm (half a wave per row,
// k_layernorm's arithmetic: fp32 statistics over the fp32 sums); mask[b][t] = t < T
__global__ __launch_bounds__(256) void k_vit_embed(const half_t* __restrict__ emb, const half_t* __restrict__ cls,
                                                   const half_t* __restrict__ pos, const float* __restrict__ g,
                                                   const float* __restrict__ bta, float eps, int B, int P, int Tp, int H,
                                                   half_t* __restrict__ x, int* __restrict__ mask) {
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), l32 = threadIdx.x & 31;
    if (row >= B * Tp) return;
    const int b = row / Tp, t = row - b * Tp;
    if (l32 == 0) mask[row] = t <= P ? 1 : 0;
    half_t* dst = x + (long long)row * H;
    if (t > P) {
        for (int c = l32; c < H; c += 32) dst[c] = (half_t)0.f;
        return;
    }
    const half_t* src = t == 0 ? cls : emb + ((long long)b * P + (t - 1)) * H;
    float sum = 0.f, sq = 0.f;
    for (int c = l32; c < H; c += 32) {
        const float v = (float)src[c] + (float)pos[(long long)t * H + c];
        sum += v;
    }
#pragma unroll
    for (int o = 16; o; o >>= 1) sum += __shfl_xor(sum, o, 32);
    const float mean = sum / (float)H;
    for (int c = l32; c < H; c += 32) {
        const float v = (float)src[c] + (float)pos[(long long)t * H + c] - mean;
        sq += v * v;
    }
#pragma unroll
    for (int o = 16; o; o >>= 1) sq += __shfl_xor(sq, o, 32);
    const float rstd = rsqrtf(sq / (float)H + eps);
    for (int c = l32; c < H; c += 32) {
        const float v = (float)src[c] + (float)pos[(long long)t * H + c];
        dst[c] = (half_t)((v - mean) * rstd * g[c] + bta[c]);
    }
}

// one workgroup per image: LayerNorm of the class token's row, then out[d] = <Wproj[d], ln> (no bias), optionally L2-normalised
__global__ __launch_bounds__(256) void k_vit_head(const half_t* __restrict__ x, int Tp, int H, const float* __restrict__ g,
                                                  const float* __restrict__ bta, float eps, const half_t* __restrict__ Wp, int D,
                                                  int normalize, float* __restrict__ out, const int* __restrict__ rowsel = nullptr) {
    extern __shared__ float sm[];   // [H] normalised class token, [256] reduction
    float* red = sm + H;
    const int tid = threadIdx.x;
    // the pooled row: the class token (row 0) of an image, or row rowsel[b] of a text sequence (CLIP's EOS-token pooling)
    const half_t* row = x + ((long long)blockIdx.x * Tp + (rowsel ? rowsel[blockIdx.x] : 0)) * H;
    float s = 0.f;
    for (int c = tid; c < H; c += 256) s += (float)row[c];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const float mean = red[0] / (float)H;
    __syncthreads();
    float q = 0.f;
    for (int c = tid; c < H; c += 256) { const float v = (float)row[c] - mean; q += v * v; }
    red[tid] = q;
    __syncthreads();
    for (int o = 128; o; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const float rstd = rsqrtf(red[0] / (float)H + eps);
    __syncthreads();
    for (int c = tid; c < H; c += 256) sm[c] = ((float)row[c] - mean) * rstd * g[c] + bta[c];
    __syncthreads();
    float nrm = 0.f;
    float* o_ = out + (long long)blockIdx.x * D;
    for (int d = tid; d < D; d += 256) {
        const half_t* w = Wp + (long long)d * H;
        float acc = 0.f;
        for (int c = 0; c < H; c += 8) {
            const h8 wv = *(const h8*)(w + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf((float)wv[e], sm[c + e], acc);
        }
        o_[d] = acc;
        nrm += acc * acc;
    }
    if (!normalize) return;
    red[tid] = nrm;
    __syncthreads();
    for (int o = 128; o; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const float inv = red[0] > 0.f ? rsqrtf(red[0]) : 0.f;
    for (int d = tid; d < D; d += 256) o_[d] *= inv;
}

extern "C" int vf_vit_destroy(vf_vit* v) {
    if (!v) return VF_OK;
    vf::DeviceGuard guard;
    (void)hipSetDevice(v->device);
    model_release(*v);
    delete v;
    return VF_OK;
}

extern "C" int vf_vit_create(vf_vit** out, const vf_vit_config* cfg, const void* w16, int64_t n16, const float* w32, int64_t n32,
                             int32_t device_id) {
    if (!out) return fail(VF_EINVAL, "vf_vit_create: null out");
    *out = nullptr;
    if (!cfg || !w16 || !w32) return fail(VF_EINVAL, "vf_vit_create: null argument");
    const vf_vit_config& c = *cfg;
    VFT_TRY(bert_check_dims(c.hidden, c.heads, c.ffn, "vit: "));
    if (c.layers <= 0 || c.channels <= 0 || c.patch <= 0 || c.image <= 0 || c.image % c.patch) return fail(VF_EINVAL, "vit: bad image / patch / layers");
    if (c.proj_dim <= 0 || c.act < 0 || c.act > 1 || c.normalize < 0 || c.normalize > 1) return fail(VF_EINVAL, "vit: bad proj_dim / act / normalize");
    const int g = c.image / c.patch, P = g * g, T = P + 1, Tp = (T + 31) / 32 * 32;
    if (Tp > kEncResidentT) return fail(VF_EUNSUPPORTED, "vit: more than 511 patches per image");
    if ((size_t)n16 != vit_n16(c) || (size_t)n32 != vit_n32(c))
        return fail(VF_EINVAL, "vf_vit_create: weight blob sizes do not match the config (see vf_vit_weight_sizes)");
    VFT_TRY(model_check_device(device_id, "vf_vit_create"));
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(device_id));
    vf_vit* v = new (std::nothrow) vf_vit();
    if (!v) return fail(VF_ENOMEM, "host allocation failed");
    v->cfg = c; v->device = device_id; v->P = P; v->T = T; v->Tp = Tp;
    v->Kp = (c.channels * c.patch * c.patch + 63) / 64 * 64;
    const size_t H = c.hidden, F = c.ffn;
    v->o_patch = 0; v->o_cls = H * (size_t)v->Kp; v->o_pos = v->o_cls + H; v->o_layers = v->o_pos + (size_t)T * H;
    v->layer16 = bert_layer16(H, F);
    v->o_proj = v->o_layers + (size_t)c.layers * v->layer16;
    v->f_pre = 0; v->f_layers = 2 * H; v->layer32 = preln_layer32(H, F);
    v->f_post = v->f_layers + (size_t)c.layers * v->layer32;
    hipError_t er = model_upload(*v, w16, n16, w32, n32);
    if (er == hipSuccess) {   // log2(e) / sqrt(64) into the query projection, as the text encoder does (k_attention2 expects it)
        const float qs = 0.125f * 1.4426950408889634f;
        for (int l = 0; l < c.layers; ++l) {
            hipLaunchKernelGGL(k_scale_half, dim3((unsigned)((H * H + 255) / 256)), dim3(256), 0, 0, v->w16 + v->o_layers + (size_t)l * v->layer16, (long long)(H * H), qs);
            hipLaunchKernelGGL(k_scale_float, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, 0, v->w32 + v->f_layers + (size_t)l * v->layer32 + 2 * H, (long long)H, qs);
        }
        er = hipDeviceSynchronize();
    }
    if (er != hipSuccess) return model_create_failed(v, vf_vit_destroy, "vf_vit_create", er);
    *out = v;
    return VF_OK;
}

static int vit_ensure_ws(vf_vit* v, int B) {
    VFT_HIP(handle_stream(&v->stream));
    if (B <= v->cap_b) return VF_OK;
    v->ws.free_all();
    v->cap_b = 0;
    const vf_vit_config& c = v->cfg;
    const size_t H = c.hidden, F = c.ffn;
    const size_t Mp = ((size_t)B * v->Tp + 255) / 256 * 256, Rp = ((size_t)B * v->P + 255) / 256 * 256;
    DevPool& ws = v->ws;
    hipStream_t st = v->stream;
    // (zeroed: rows past B Tp are read by the products, keep them finite)
    VFT_HIP(ws.get(&v->d_pix, (size_t)B * c.channels * c.image * c.image * 4, false, st));
    VFT_HIP(ws.get(&v->patches, Rp * v->Kp * 2, false, st));
    VFT_HIP(ws.get(&v->emb, Rp * H * 2, false, st));
    VFT_HIP(ws.get(&v->x, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&v->y, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&v->t, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&v->qkv, Mp * 3 * H * 2, true, st));
    VFT_HIP(ws.get(&v->ctx, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&v->hbuf, Mp * F * 2, true, st));
    VFT_HIP(ws.get(&v->d_mask, Mp * 4, true, st));
    VFT_HIP(ws.get(&v->d_out, (size_t)B * c.proj_dim * 4, false, st));
    v->cap_b = B;
    VFT_HIP(gws_ensure(v->gws, st));
    return VF_OK;
}

// The PRE-LayerNorm layers of a tower (vf_vit or vf_clip_text: same fields) over the M rows of v->x: x += Wo attn(LN1 x); x += W2 act(W1 LN2 x).
// attention(): the tower's own launch, v->qkv -> v->ctx.
template <typename Tower, typename Attention>
static int preln_layers(Tower* v, int M, hipStream_t st, Attention attention) {
    const auto& c = v->cfg;
    const int H = c.hidden, F = c.ffn, Mp = (M + 255) / 256 * 256;
    for (int l = 0; l < c.layers; ++l) {
        const half_t* w = v->w16 + v->o_layers + (size_t)l * v->layer16;
        const float* f = v->w32 + v->f_layers + (size_t)l * v->layer32;
        const half_t *Wqkv = w, *Wo = Wqkv + (size_t)3 * H * H, *W1 = Wo + (size_t)H * H, *W2 = W1 + (size_t)F * H;
        const float *g1 = f, *b1n = g1 + H, *bqkv = b1n + H, *bo = bqkv + 3 * H, *g2 = bo + H, *b2n = g2 + H, *b1 = b2n + H, *b2 = b1 + F;
        hipLaunchKernelGGL(k_layernorm, dim3((M + 7) / 8), dim3(256), 0, st, v->x, g1, b1n, c.ln_eps, M, H, v->t);
        VFT_HIP(gemm<EPI_BIAS>(v->t, Wqkv, bqkv, nullptr, v->qkv, Mp, 3 * H, H, st, 0, &v->gws));
        attention();
        VFT_HIP(gemm<EPI_BIAS_RESIDUAL>(v->ctx, Wo, bo, v->x, v->y, Mp, H, H, st, 0, &v->gws));
        hipLaunchKernelGGL(k_layernorm, dim3((M + 7) / 8), dim3(256), 0, st, v->y, g2, b2n, c.ln_eps, M, H, v->t);
        if (c.act == 0) VFT_HIP(gemm<EPI_BIAS_GELU>(v->t, W1, b1, nullptr, v->hbuf, Mp, F, H, st, 0, &v->gws));
        else VFT_HIP(gemm<EPI_BIAS_QGELU>(v->t, W1, b1, nullptr, v->hbuf, Mp, F, H, st, 0, &v->gws));
        VFT_HIP(gemm<EPI_BIAS_RESIDUAL>(v->hbuf, W2, b2, v->y, v->x, Mp, H, F, st, 0, &v->gws));
    }
    return VF_OK;
}

// pixels [b][channels][image][image] host -> out [b][proj_dim]: fp32 already resized / normalised by the caller's image
// processor (u8 == nullptr), or raw bytes normalised on the device with the processor's mean / std (three channels)
static int vit_forward_impl(vf_vit* v, const float* pixels, const unsigned char* u8, const float* mean, const float* stdv, int32_t b,
                            float* out) {
    if (!v) return fail(VF_EINVAL, "vf_vit_forward: null handle");
    if (b < 0) return fail(VF_EINVAL, "vf_vit_forward: negative batch");
    if (b == 0) return VF_OK;
    if ((!pixels && !u8) || !out) return fail(VF_EINVAL, "vf_vit_forward: null buffer");
    float sc[3] = {1.f, 1.f, 1.f}, sh[3] = {0.f, 0.f, 0.f};
    if (u8) {
        if (v->cfg.channels != 3 || !mean || !stdv) return fail(VF_EINVAL, "vf_vit_forward_u8: three channels with mean / std");
        for (int c = 0; c < 3; ++c) {
            if (!(stdv[c] > 0.f)) return fail(VF_EINVAL, "vf_vit_forward_u8: std must be positive");
            sc[c] = 1.0f / (255.0f * stdv[c]); sh[c] = -mean[c] / stdv[c];
        }
    }
    std::lock_guard<std::mutex> lk(v->mu);
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(v->device));
    VFT_TRY(vit_ensure_ws(v, b));
    const vf_vit_config& c = v->cfg;
    const int H = c.hidden, P = v->P, Tp = v->Tp, Kp = v->Kp;
    const int M = b * Tp, Rp = (b * P + 255) / 256 * 256;
    VFT_HIP(handle_stream(&v->stream));
    hipStream_t st = v->stream;
    const size_t npix = (size_t)b * c.channels * c.image * c.image;
    if (u8) {
        VFT_HIP(hipMemcpyAsync(v->d_pix, u8, npix, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_vit_unfold<unsigned char>, dim3(2048), dim3(256), 0, st, (const unsigned char*)v->d_pix, b, c.channels, c.image, c.patch, Kp, Rp,
                           sc[0], sc[1], sc[2], sh[0], sh[1], sh[2], v->patches);
    } else {
        VFT_HIP(hipMemcpyAsync(v->d_pix, pixels, npix * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_vit_unfold<float>, dim3(2048), dim3(256), 0, st, (const float*)v->d_pix, b, c.channels, c.image, c.patch, Kp, Rp,
                           1.f, 1.f, 1.f, 0.f, 0.f, 0.f, v->patches);
    }
    VFT_HIP(gemm<EPI_BIAS>(v->patches, v->w16 + v->o_patch, nullptr, nullptr, v->emb, Rp, H, Kp, st, 0, &v->gws));
    hipLaunchKernelGGL(k_vit_embed, dim3((M + 7) / 8), dim3(256), 0, st, v->emb, v->w16 + v->o_cls, v->w16 + v->o_pos, v->w32 + v->f_pre,
                       v->w32 + v->f_pre + H, c.ln_eps, b, P, Tp, H, v->x, v->d_mask);
    VFT_TRY(preln_layers(v, M, st, [&] { launch_attention2<0>(v->qkv, v->d_mask, b, Tp, c.heads, v->ctx, st); }));
    hipLaunchKernelGGL(k_vit_head, dim3(b), dim3(256), (size_t)(H + 256) * sizeof(float), st, v->x, Tp, H, v->w32 + v->f_post, v->w32 + v->f_post + H,
                       c.ln_eps, v->w16 + v->o_proj, c.proj_dim, c.normalize, v->d_out, (const int*)nullptr);
    VFT_HIP(hipGetLastError());
    VFT_HIP(hipMemcpyAsync(out, v->d_out, (size_t)b * c.proj_dim * 4, hipMemcpyDeviceToHost, st));
    VFT_HIP(hipStreamSynchronize(st));
    return VF_OK;
}
extern "C" int vf_vit_forward(vf_vit* v, const float* pixels, int32_t b, float* out) {
    return vit_forward_impl(v, pixels, nullptr, nullptr, nullptr, b, out);
}
extern "C" int vf_vit_forward_u8(vf_vit* v, const unsigned char* pixels, const float* mean3, const float* std3, int32_t b, float* out) {
    if (!pixels) return fail(VF_EINVAL, "vf_vit_forward_u8: null buffer");
    return vit_forward_impl(v, nullptr, pixels, mean3, std3, b, out);
}

// ------------------------------------------------------------------------------------------------
// CLIP TEXT tower (round 4): the query side of the figure leg.  Figure rows live in CLIP's joint space (vf_vit_* above); a
// text query reaches them only through the SAME model's text tower -- transformers' CLIPTextModelWithProjection:
// token + learned position embeddings (no LayerNorm), PRE-LayerNorm layers with CAUSAL attention (and the key-padding
// mask), final_layer_norm, the hidden state at the EOS token, text_projection (no bias) into the joint space (768 for
// ViT-L/14).  Kernels: the vision tower's products / k_layernorm / quick-GELU epilogue, the decoder family's causal
// streaming attention at head dim 64 (k_attention_stream2<64, true>: softmax scale passed, nothing folded into Wq), and
// k_vit_head reading row eos[b] instead of row 0.
// ------------------------------------------------------------------------------------------------
struct vf_clip_text : ModelBase {
    vf_clip_text_config cfg{};
    size_t o_tok = 0, o_pos = 0, o_layers = 0, o_proj = 0, layer16 = 0;
    size_t f_layers = 0, f_final = 0, layer32 = 0;
    int cap_tokens = 0, cap_b = 0;
    half_t *x = nullptr, *y = nullptr, *t = nullptr, *qkv = nullptr, *ctx = nullptr, *hbuf = nullptr;
    int *d_ids = nullptr, *d_mask_in = nullptr, *d_mask = nullptr, *d_eos = nullptr;
    float* d_out = nullptr;
};

static size_t ct_n16(const vf_clip_text_config& c) {
    const size_t H = c.hidden, F = c.ffn;
    return (size_t)c.vocab * H + (size_t)c.max_pos * H + (size_t)c.layers * bert_layer16(H, F) + (size_t)c.proj_dim * H;
}
static size_t ct_n32(const vf_clip_text_config& c) {
    const size_t H = c.hidden, F = c.ffn;
    return (size_t)c.layers * preln_layer32(H, F) + 2 * H;
}
extern "C" int vf_clip_text_weight_sizes(const vf_clip_text_config* cfg, int64_t* n_fp16, int64_t* n_fp32) {
    if (!cfg || !n_fp16 || !n_fp32) return fail(VF_EINVAL, "vf_clip_text_weight_sizes: null argument");
    if (cfg->vocab <= 0 || cfg->max_pos <= 0 || cfg->hidden <= 0 || cfg->layers <= 0 || cfg->ffn <= 0 || cfg->proj_dim <= 0)
        return fail(VF_EINVAL, "vf_clip_text_weight_sizes: bad config");
    *n_fp16 = (int64_t)ct_n16(*cfg);
    *n_fp32 = (int64_t)ct_n32(*cfg);
    return VF_OK;
}

// rows [b][Tp]: x = fp16(token[id] + position[t]) for t < T, zero rows and mask 0 beyond; mask[b][t] = the caller's mask
__global__ __launch_bounds__(256) void k_clip_text_embed(const int* __restrict__ ids, const int* __restrict__ mask_in,
                                                         const half_t* __restrict__ tok, const half_t* __restrict__ pos, int B, int T,
                                                         int Tp, int H, int vocab, half_t* __restrict__ x, int* __restrict__ mask) {
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), l32 = threadIdx.x & 31;
    if (row >= B * Tp) return;
    const int b = row / Tp, t = row - b * Tp;
    half_t* dst = x + (long long)row * H;
    if (t >= T) {
        if (l32 == 0) mask[row] = 0;
        for (int c = l32 * 8; c < H; c += 256) *(h8*)(dst + c) = h8{0, 0, 0, 0, 0, 0, 0, 0};
        return;
    }
    int id = ids[b * T + t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    if (l32 == 0) mask[row] = mask_in[b * T + t] ? 1 : 0;
    const half_t* e = tok + (long long)id * H;
    const half_t* p = pos + (long long)t * H;
    for (int c = l32 * 8; c < H; c += 256) {
        const h8 ev = *(const h8*)(e + c), pv = *(const h8*)(p + c);
        h8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (half_t)((float)ev[i] + (float)pv[i]);
        *(h8*)(dst + c) = o;
    }
}

extern "C" int vf_clip_text_destroy(vf_clip_text* v) {
    if (!v) return VF_OK;
    vf::DeviceGuard guard;
    (void)hipSetDevice(v->device);
    model_release(*v);
    delete v;
    return VF_OK;
}

extern "C" int vf_clip_text_create(vf_clip_text** out, const vf_clip_text_config* cfg, const void* w16, int64_t n16, const float* w32,
                                   int64_t n32, int32_t device_id) {
    if (!out) return fail(VF_EINVAL, "vf_clip_text_create: null out");
    *out = nullptr;
    if (!cfg || !w16 || !w32) return fail(VF_EINVAL, "vf_clip_text_create: null argument");
    const vf_clip_text_config& c = *cfg;
    VFT_TRY(bert_check_dims(c.hidden, c.heads, c.ffn, "clip text: "));
    if (c.layers <= 0 || c.vocab <= 0 || c.max_pos <= 0 || c.max_pos > 512) return fail(VF_EINVAL, "clip text: bad layers / vocab / max_pos (<= 512)");
    if (c.proj_dim <= 0 || c.act < 0 || c.act > 1 || c.normalize < 0 || c.normalize > 1) return fail(VF_EINVAL, "clip text: bad proj_dim / act / normalize");
    if ((size_t)n16 != ct_n16(c) || (size_t)n32 != ct_n32(c))
        return fail(VF_EINVAL, "vf_clip_text_create: weight blob sizes do not match the config (see vf_clip_text_weight_sizes)");
    VFT_TRY(model_check_device(device_id, "vf_clip_text_create"));
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(device_id));
    vf_clip_text* v = new (std::nothrow) vf_clip_text();
    if (!v) return fail(VF_ENOMEM, "host allocation failed");
    v->cfg = c; v->device = device_id;
    const size_t H = c.hidden, F = c.ffn;
    v->o_tok = 0; v->o_pos = (size_t)c.vocab * H; v->o_layers = v->o_pos + (size_t)c.max_pos * H;
    v->layer16 = bert_layer16(H, F);
    v->o_proj = v->o_layers + (size_t)c.layers * v->layer16;
    v->f_layers = 0; v->layer32 = preln_layer32(H, F);
    v->f_final = (size_t)c.layers * v->layer32;
    const hipError_t er = model_upload(*v, w16, n16, w32, n32);
    if (er != hipSuccess) return model_create_failed(v, vf_clip_text_destroy, "vf_clip_text_create", er);
    *out = v;
    return VF_OK;
}

static int ct_ensure_ws(vf_clip_text* v, int B, int Tp) {
    VFT_HIP(handle_stream(&v->stream));
    int tokens = (B * Tp + 255) / 256 * 256;
    if (tokens <= v->cap_tokens && B <= v->cap_b) return VF_OK;
    tokens = std::max(tokens, v->cap_tokens); B = std::max(B, v->cap_b);
    v->ws.free_all();
    v->cap_tokens = v->cap_b = 0;
    const size_t H = v->cfg.hidden, F = v->cfg.ffn, Mp = tokens;
    DevPool& ws = v->ws;
    hipStream_t st = v->stream;
    // (zeroed: rows past B Tp are read by the products, keep them finite)
    VFT_HIP(ws.get(&v->x, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&v->y, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&v->t, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&v->qkv, Mp * 3 * H * 2, true, st));
    VFT_HIP(ws.get(&v->ctx, Mp * H * 2, true, st));
    VFT_HIP(ws.get(&v->hbuf, Mp * F * 2, true, st));
    VFT_HIP(ws.get(&v->d_ids, Mp * 4, false, st));
    VFT_HIP(ws.get(&v->d_mask_in, Mp * 4, false, st));
    VFT_HIP(ws.get(&v->d_mask, Mp * 4, true, st));
    VFT_HIP(ws.get(&v->d_eos, (size_t)B * 4, false, st));
    VFT_HIP(ws.get(&v->d_out, (size_t)B * v->cfg.proj_dim * 4, false, st));
    v->cap_tokens = tokens; v->cap_b = B;
    VFT_HIP(gws_ensure(v->gws, st));
    return VF_OK;
}

// ids / mask [b][t] int32 host (right-padded, as CLIP's tokenizer pads; mask == nullptr: every token valid -- what the HF
// pipeline does, its tokenizer pads with the EOS id and passes no mask) -> out [b][proj_dim] fp32 host.
// The pooled position follows transformers: eos_token_id == 2 (the published checkpoints' legacy config): argmax of the ids,
// first maximum; otherwise the FIRST position holding eos_token_id (a row without one pools position 0, as argmax of zeros does).
extern "C" int vf_clip_text_forward(vf_clip_text* v, const int32_t* ids, const int32_t* mask, int32_t b, int32_t t, float* out) {
    if (!v) return fail(VF_EINVAL, "vf_clip_text_forward: null handle");
    if (b < 0 || t < 0) return fail(VF_EINVAL, "vf_clip_text_forward: negative sizes");
    if (b == 0) return VF_OK;
    if (!ids || !out) return fail(VF_EINVAL, "vf_clip_text_forward: null buffer");
    const vf_clip_text_config& c = v->cfg;
    if (t == 0 || t > c.max_pos) return fail(VF_EINVAL, "vf_clip_text_forward: t must be in [1, max_pos]");
    {   // refused on the host like the encoder's and the decoder's ids: the pooled position below is computed from these very values
        const long long bad = first_id_out_of_range(ids, (size_t)b * t, c.vocab);
        if (bad >= 0) return fail(VF_EINVAL, "vf_clip_text_forward: token id " + std::to_string(ids[bad]) + " at [" + std::to_string(bad / t) + ", " + std::to_string(bad % t) + "] is outside the vocabulary [0, " + std::to_string(c.vocab) + ")");
    }
    std::vector<int> eos((size_t)b), ones;
    for (int i = 0; i < b; ++i) {
        const int32_t* r = ids + (size_t)i * t;
        int at = 0;
        if (c.eos_token_id == 2) { for (int j = 1; j < t; ++j) if (r[j] > r[at]) at = j; }
        else { for (int j = 0; j < t; ++j) if (r[j] == c.eos_token_id) { at = j; break; } }
        eos[(size_t)i] = at;
    }
    if (!mask) { ones.assign((size_t)b * t, 1); mask = ones.data(); }
    std::lock_guard<std::mutex> lk(v->mu);
    vf::DeviceGuard guard;
    VFT_HIP(hipSetDevice(v->device));
    const int Tp = (t + 31) / 32 * 32;
    VFT_TRY(ct_ensure_ws(v, b, Tp));
    const int H = c.hidden, M = b * Tp;
    VFT_HIP(handle_stream(&v->stream));
    hipStream_t st = v->stream;
    VFT_HIP(hipMemcpyAsync(v->d_ids, ids, (size_t)b * t * 4, hipMemcpyHostToDevice, st));
    VFT_HIP(hipMemcpyAsync(v->d_mask_in, mask, (size_t)b * t * 4, hipMemcpyHostToDevice, st));
    VFT_HIP(hipMemcpyAsync(v->d_eos, eos.data(), (size_t)b * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_clip_text_embed, dim3((M + 7) / 8), dim3(256), 0, st, v->d_ids, v->d_mask_in, v->w16 + v->o_tok, v->w16 + v->o_pos, b, t,
                       Tp, H, c.vocab, v->x, v->d_mask);
    const dim3 agrid((Tp + 127) / 128, c.heads, b);
    VFT_TRY(preln_layers(v, M, st, [&] {
        hipLaunchKernelGGL((k_attention_stream2<64, true>), agrid, dim3(256), sizeof(AttnStream2Lds<64>), st, v->qkv, v->d_mask, Tp, 3 * H, c.heads,
                           c.heads, 0.125f, v->ctx, H, (const int*)nullptr);
    }));
    hipLaunchKernelGGL(k_vit_head, dim3(b), dim3(256), (size_t)(H + 256) * sizeof(float), st, v->x, Tp, H, v->w32 + v->f_final, v->w32 + v->f_final + H,
                       c.ln_eps, v->w16 + v->o_proj, c.proj_dim, c.normalize, v->d_out, (const int*)v->d_eos);
    VFT_HIP(hipGetLastError());
    VFT_HIP(hipMemcpyAsync(out, v->d_out, (size_t)b * c.proj_dim * 4, hipMemcpyDeviceToHost, st));
    VFT_HIP(hipStreamSynchronize(st));
    return VF_OK;
}

// Test hook (not part of the public header; tools/bench_gemm.py and the GEMM parity test bind it):
// C[M][N] = epi(A[M][K] . W[N][K]^T + bias [, + R]) on device pointers, fp16 in/out, fp32 accumulation.
extern "C" int vf_debug_gemm(const void* A, const void* W, const float* bias, const void* R, void* C, int M, int N, int K,
                             int epi, void* stream, int kind /* 0 auto, 1 DMA 128x256, 2 256x256, 3 128x128 */) {
    hipError_t er = configure_once();
    if (er != hipSuccess) return -1;
    if (M % 128 || N % 128 || K % 64) return -2;
    if ((kind == 1 || kind == 5) && (M % DBM || N % DBN)) return -2;
    if (kind == 6 && (M % DBM || N % 128)) return -2;
    if ((kind == 2 || kind == 7 || kind == 8 || kind == 10) && (M % LBM || N % LBN)) return -2;
    if ((kind == 7 || kind == 8) && K < 128) return -2;
    if ((kind == 11 || kind == 12) && (M % LBM || N % LBN || K < 256)) return -2;   // 11: the whole-product K cut, 12: stream-K (where their gates admit the shape)
    if (kind == 10 && (K < 256 || (epi != EPI_BIAS && epi != EPI_BIAS_GELU && epi != EPI_BIAS_QGELU && epi != EPI_BIAS_RESIDUAL))) return -2;
    hipStream_t st = (hipStream_t)stream;
    const half_t *a = (const half_t*)A, *w = (const half_t*)W, *r = (const half_t*)R;
    half_t* c = (half_t*)C;
    // the hook's own split-K workspace: one per device, never freed, calls serialised (a test hook, not a serving path)
    static std::mutex hook_mu;
    static GemmWs hook_ws[16];
    std::lock_guard<std::mutex> hook_lk(hook_mu);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16 || gws_ensure(hook_ws[dev]) != hipSuccess) return -1;
    GemmWs* gws = &hook_ws[dev];
    if (epi == EPI_GATED_SILU || epi == EPI_GATED_GELU) {   // W = [gate rows (N / 2) | up rows (N / 2)], C is M x N / 2
        if (!gemm_gated(a, w, c, M, N / 2, K, epi == EPI_GATED_GELU, st, &er)) return -2;
        return er == hipSuccess ? 0 : -1;
    }
    if (epi == EPI_RESIDUAL_F32) {   // R and C are fp32 [M][N] here (the decoder's residual stream), no bias
        er = gemm<EPI_RESIDUAL_F32>(a, w, nullptr, r, c, M, N, K, st, kind);
        return er == hipSuccess ? 0 : -1;
    }
    if (epi == EPI_BIAS) er = gemm<EPI_BIAS>(a, w, bias, r, c, M, N, K, st, kind, gws);
    else if (epi == EPI_BIAS_GELU) er = gemm<EPI_BIAS_GELU>(a, w, bias, r, c, M, N, K, st, kind, gws);
    else if (epi == EPI_BIAS_QGELU) er = gemm<EPI_BIAS_QGELU>(a, w, bias, r, c, M, N, K, st, kind, gws);
    else er = gemm<EPI_BIAS_RESIDUAL>(a, w, bias, r, c, M, N, K, st, kind, gws);
    return er == hipSuccess ? 0 : -1;
}

// Test hook (tools/bench_attention.py, tests/test_gpu_encoder.py): one attention pass over qkv [B*T][3*64*heads]
// (Q already carrying log2(e) / 8) with the key padding mask [B*T]; kind 1 = first-generation resident kernel,
// 2 = k_attention2, 3 = streaming kernel.
extern "C" int vf_debug_attention(const void* qkv, const int* mask, int B, int T, int heads, void* ctx, void* stream, int kind) {
    hipError_t er = configure_once();
    if (er != hipSuccess) return -1;
    if (B <= 0 || heads <= 0 || T <= 0 || T % 32) return -2;
    if (kind != 3 && kind != 4 && T > kEncResidentT) return -2;
    hipStream_t st = (hipStream_t)stream;
    const int H = heads * ADH;
    if (kind == 1 || kind == 3) {
        return -3;   // first-generation kernels: deleted in round 4
    } else if (kind == 2) {
        launch_attention2<0>((const half_t*)qkv, mask, B, T, heads, (half_t*)ctx, st);
    } else if (kind == 26) {
        launch_attention2<6>((const half_t*)qkv, mask, B, T, heads, (half_t*)ctx, st);
    } else if (kind == 4) {
        hipLaunchKernelGGL((k_attention_stream2<64, false>), dim3((T + 127) / 128, heads, B), dim3(256), sizeof(AttnStream2Lds<64>), st,
                           (const half_t*)qkv, mask, T, 3 * H, heads, heads, -1.f, (half_t*)ctx, H);
    } else {
        return -2;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Test hook: k_attention2 over PACKED sequences -- sequence b in rows [seq_off[b], seq_off[b + 1]) (lengths multiples of 32,
// at most Tmax <= 512) of qkv [rows][3*64*heads] / mask [rows] / ctx [rows][64*heads]; seq_off is a device array of B + 1 ints.
extern "C" int vf_debug_attention_packed(const void* qkv, const int* mask, const int* seq_off, int B, int Tmax, int heads, void* ctx,
                                         void* stream) {
    hipError_t er = configure_once();
    if (er != hipSuccess) return -1;
    if (B <= 0 || heads <= 0 || Tmax <= 0 || Tmax % 32 || Tmax > kEncResidentT || !seq_off) return -2;
    launch_attention2<0>((const half_t*)qkv, mask, B, Tmax, heads, (half_t*)ctx, (hipStream_t)stream, seq_off);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// Test hooks (tests/test_gpu_decoder_kernels.py): ONE decoder kernel each, on the caller's device buffers and stream, through the launch
// helper the forward uses (dec_launch_*).  Every refusal (-2) returns before anything is launched.
// The causal grouped-query attention of dec_layers_device: qkv rows [q (heads*dh) | k (kv_heads*dh) | v (kv_heads*dh)], mask per row,
// seq_off (device, B + 1 ints) or null, ctx rows of ctx_ld elements.  Packed: T is the longest sequence, every length a multiple of 32.
extern "C" int vf_debug_dec_attention(const void* qkv, const int* mask, const int* seq_off, int B, int T, int heads, int kv_heads,
                                      int head_dim, float scale, void* ctx, int ctx_ld, void* stream) {
    if (configure_once() != hipSuccess) return -1;
    if (!qkv || !mask || !ctx || B <= 0 || heads <= 0 || kv_heads <= 0 || heads % kv_heads != 0) return -2;
    if (T <= 0 || T % 32 != 0 || T > kDecMaxT) return -2;
    if (head_dim != 64 && head_dim != 128 && head_dim != 256) return -2;
    if (ctx_ld < heads * head_dim || ctx_ld % 4 != 0) return -2;
    if (!dec_launch_attention((const half_t*)qkv, mask, seq_off, B, T, (heads + 2 * kv_heads) * head_dim, heads, kv_heads, head_dim, scale,
                              (half_t*)ctx, ctx_ld, (hipStream_t)stream))
        return -2;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int vf_debug_dec_rope_table(float theta, int T, int dh, void* tab, void* stream) {
    if (!tab || !(theta > 0.f) || T <= 0 || T > kDecMaxT || (dh != 64 && dh != 128 && dh != 256)) return -2;
    dec_launch_rope_table(theta, T, dh, (float2*)tab, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// qkv [M][(heads + 2 kv_heads) * dh] in place; tab: kDecMaxT rows of k_rope_table; pos_ids (device, M ints in [0, 4096)) or null: tok % T
extern "C" int vf_debug_dec_qknorm_rope(void* qkv, int M, int T, int heads, int kv_heads, int dh, const float* qw, const float* kw, float eps,
                                        int qk_norm, const void* tab, const int* pos_ids, void* stream) {
    if (!qkv || !tab || M <= 0 || T <= 0 || T > kDecMaxT || heads <= 0 || kv_heads <= 0 || (dh != 64 && dh != 128 && dh != 256)) return -2;
    if (qk_norm && (!qw || !kw)) return -2;
    dec_launch_qknorm_rope((half_t*)qkv, M, T, (heads + 2 * kv_heads) * dh, heads, kv_heads, dh, qw, kw, eps, qk_norm, (const float2*)tab,
                           pos_ids, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int vf_debug_dec_rmsnorm(const float* x, const float* w, float woff, float eps, int M, int H, void* y, int out_fp32, void* stream) {
    if (!x || !w || !y || M <= 0 || H <= 0 || H % 4 != 0) return -2;
    if (out_fp32) dec_launch_rmsnorm<float>(x, w, woff, eps, M, H, (float*)y, (hipStream_t)stream);
    else dec_launch_rmsnorm<half_t>(x, w, woff, eps, M, H, (half_t*)y, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int vf_debug_dec_swiglu(const void* gu, int M, int F, int act_kind, void* act, void* stream) {
    if (!gu || !act || M <= 0 || F <= 0 || F % 8 != 0 || (act_kind != 0 && act_kind != 1)) return -2;
    dec_launch_swiglu((const half_t*)gu, M, F, act_kind, (half_t*)act, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int vf_debug_dec_gather_rows(const int* ids, const void* table, int M, int H, float scale, float* out, void* stream) {
    if (!ids || !table || !out || M <= 0 || H <= 0 || H % 8 != 0) return -2;
    dec_launch_gather_rows(ids, (const half_t*)table, M, H, scale, out, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// the pooled position's "Yes" logit / the last-token row (k_pool, pooling 2): x [rows][H] fp16, out [B] / [B][H] fp32
extern "C" int vf_debug_dec_token_logit(const void* x, const int* mask, const int* seq_off, int B, int T, int Tv, int H, int all_last,
                                        const void* row, float* out, void* stream) {
    if (!x || !mask || !row || !out || B <= 0 || T <= 0 || Tv <= 0 || Tv > T || H <= 0) return -2;
    dec_launch_token_logit((const half_t*)x, mask, B, T, Tv, H, all_last, (const half_t*)row, out, seq_off, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
extern "C" int vf_debug_dec_pool_last(const void* x, const int* mask, const int* seq_off, int B, int T, int Tv, int H, int all_last,
                                      int normalize, float* out, void* stream) {
    if (!x || !mask || !out || B <= 0 || T <= 0 || Tv <= 0 || Tv > T || H <= 0 || H > 4096) return -2;
    dec_launch_pool((const half_t*)x, mask, B, T, Tv, H, 2, normalize, all_last, out, seq_off, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
