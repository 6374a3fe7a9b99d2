// vf_gemm_route.h -- which kernel serves a matrix product: the one decision every product of the encoder, the cross-encoder, the decoder
// re-ranker, ViT and the CLIP text tower makes, as a pure function of its shape, the chip and the knobs.
// vf_transformer.hip reads the knobs (gemm_knobs: the environment once, the test hooks on each call), fills a GemmIn, asks route_gemm once
// per product and switches on the answer; workspaces, launches and counters stay there.  Every threshold the choice rests on is defined
// here, beside the record of where it was measured.  Plain C++17: no HIP and no getenv, so a host-compiled driver
// (tests/test_gemm_route.py: UBSan, a table of pinned routes and an option sweep) evaluates it without a GPU.
#pragma once
#include <stddef.h>

#include <algorithm>

namespace vft {

// ---- tile geometry -------------------------------------------------------------------------------------------------------------------
constexpr int GBM = 128, GBN = 128;             // k_gemm_tn: 128 x 128 x 64, register-staged
constexpr int SBM = 64, SBN = 64, SBK = 64;     // k_gemm_splitk: 64 x 64 tiles split over K
constexpr int DBM = 128, DBN = 256, DBK = 32;   // k_gemm_dma16_tn: 128 x 256 x 32, LDS-DMA ring, two workgroups per CU
constexpr int LBM = 256, LBN = 256;             // the 256 x 256 tile of the 8-phase / persistent kernels
constexpr int PBM = 256, PBN = 256, PBK = 64;   // k_gemm8p_tn, k_gemm9_tn: 256 x 256 x 64
constexpr int kSkMaxTiles = 256;                // tiles a co-operative split-K finish keeps arrival counters for
constexpr int kSplitMax = 8, kSplitMaxRows = 64;  // split-K only for single short sequences (measured: slower from 256 tokens)

// the epilogues the route reads (the rest, k_gemm8p_tn's gated and folded forms, never pass through gemm(): vf_transformer.hip)
enum { EPI_BIAS = 0, EPI_BIAS_GELU = 1, EPI_BIAS_RESIDUAL = 2, EPI_RESIDUAL_F32 = 3, EPI_BIAS_QGELU = 11 };

// ---- knobs ---------------------------------------------------------------------------------------------------------------------------
// Every value the choice reads from the environment or a test hook, with the defaults.
// kind (VF_GEMM_KIND, or the caller's force_kind) overrides for A/B runs: 0 auto, 3 = 128 x 128, 5 = the 128 x 256 DMA kernel, 7 = the
// 8-phase kernel, 10 = the persistent kernel (whole tiles), 11 = its whole-product K cut, 12 = stream-K (the last two where their gates
// admit the shape).
struct GemmKnobs {
    int kind = 0;
    long long dma_min_wgs = 384;      // VF_GEMM_DMA_MIN_WGS
    long long p8_min_wgs = 384;       // VF_GEMM_8P_MIN_WGS, or what vf_debug_gemm_8p_min_wgs set ...
    bool p8_forced = false;           // ... and whether it did: the same gate then applies to k_gemm9_tn, and no cut is taken on its own
    long long p8_f32_min_wgs = 256;   // VF_GEMM_8P_F32_MIN_WGS (Qwen3-4B shape, 320 tiles: 66.4 vs 68.9 ms per forward)
    int gemm9 = 1;                    // VF_GEMM_9 / vf_debug_gemm9
    long long gemm9_min_wgs = 128;    // VF_GEMM_9_MIN_WGS
    int gemm9_split = 1;              // VF_GEMM_9_SPLIT / vf_debug_gemm9_split
    int split_min_k = 2048;           // VF_GEMM_9_SPLIT_MINK      (experiments)
    int split_min_kt = 8;             // VF_GEMM_9_SPLIT_MINKT
    int gemm9_streamk = 0;            // VF_GEMM_9_STREAMK / vf_debug_gemm9_streamk
    int streamk_min_saved = 5;        // VF_GEMM_9_STREAMK_MIN_SAVED
    int splitk_tail = 1;              // VF_SPLITK_TAIL, VF_NO_SPLITK_TAIL / vf_debug_splitk_tail: 0 off, 1 long-K products only, 2 every product with a partial last round
    int stagger_pct = 100;            // VF_GEMM_9_STAGGER: per cent of a tile's time; 0 = off
    bool experiments = false;         // the stream-K kernel is compiled in (-DVF_EXPERIMENTS; the product build does not carry it)
};

struct GemmIn {
    int epi = EPI_BIAS, M = 0, N = 0, K = 0, n_cu = 256;
    bool has_ws = false;      // the handle's split-K workspace exists ...
    size_t ws_bytes = 0;      // ... with this many bytes of fp32 partials
    GemmKnobs knobs;
};

enum GemmKernel : int {
    kGemmTn128 = 0,          // k_gemm_tn
    kGemmDma16 = 1,          // k_gemm_dma16_tn
    kGemm8p = 2,             // k_gemm8p_tn, with a split-K tail when slices >= 2
    kGemm9 = 3,              // k_gemm9_tn, whole tiles
    kGemm9Split = 4,         // k_gemm9_tn, the whole product cut along K
    kGemm9StreamK = 5,       // k_gemm9_tn, stream-K
};

struct GemmRoute {
    GemmKernel kernel = kGemmTn128;
    int grid = 0;            // workgroups
    int slices = 0;          // K slices per cut tile (kGemm8p with a tail, kGemm9Split), else 0
    int tail_tiles = 0;      // kGemm8p with a tail: the tiles that are cut ...
    int full_tiles = 0;      // ... and the whole tiles in front of them
    int stagger_ticks = 0;   // kGemm9: a tile's time in ticks of the 100 MHz real-time counter, over which the workgroups start
};

constexpr size_t kSkTileBytes = (size_t)PBM * PBN * sizeof(float);   // a slice leaves 256 KB of fp32 partials
// The split-K workspace of a handle: sized for the largest cut route_gemm makes, tail tiles x slices <= the CU count, 256 KB of partials each.
inline size_t gemm_ws_bytes(int n_cu) { return (size_t)std::max(n_cu, kSkMaxTiles) * kSkTileBytes; }

constexpr int kLongK = 2048;       // "long K": where a partial last round, or an idle chip, is worth a cut along K (FFN-down; the records below)
constexpr int kSubSplitMinK = 4096;   // the 8-phase kernel's sub-round cut (its record below)
inline int pad8(int tiles) { return (tiles + 7) & ~7; }   // tiles padded to one per XCD

// One to two rounds' remainder "can be cut at least in two": a partial last round of a long-K product whose tiles, padded to the XCDs,
// fill at most half the CUs, with the split-K tail on and a workspace to finish through.  The persistent kernel's gate (such a product of
// up to two rounds goes to the 8-phase kernel) and the 8-phase kernel's (it takes it) are this one condition.
inline bool tail_cuttable(const GemmIn& in, int tiles, int ncu8) {
    return in.K >= kLongK && ncu8 > 0 && tiles > ncu8 && tiles % ncu8 != 0 && 2 * pad8(tiles % ncu8) <= ncu8 && in.knobs.splitk_tail != 0 && in.has_ws;
}

// The 8-phase kernel's cut, before the mode is looked at: the tiles of the partial last round (a product of less than one round -- tiles <=
// CUs: the per-rank batches of a data-parallel re-rank -- is cut whole), S slices per tile so that the slices still fit one round, each
// at least two K-tiles long.
struct Cut8 { int ntail, pad, S; };
inline Cut8 cut8(int tiles, int cus, int nk) {
    Cut8 c;
    c.ntail = cus <= 0 ? 0 : (tiles > cus ? tiles % cus : tiles);
    c.pad = pad8(c.ntail);
    c.S = c.ntail > 0 ? std::min(std::min(cus / c.pad, nk / 2), 4) : 0;
    return c;
}
// a cut of `ntail` tiles in S slices can be finished: the tail is on, the workspace holds the partials, the counters the tiles
inline bool cut_fits(const GemmIn& in, int ntail, int S) {
    return S >= 2 && in.knobs.splitk_tail != 0 && in.has_ws && ntail <= kSkMaxTiles && (size_t)ntail * S * kSkTileBytes <= in.ws_bytes;
}

inline GemmRoute route_gemm(const GemmIn& in) {
    // Tile choice (VF_GEMM_KIND overrides for A/B runs: 5 = DMA 128x256 with 16x16x32 MFMAs (the default large-problem
    // kernel), 6 = its 128-wide instance, 1 = 128x256 with 32x32x16 MFMAs, 2 = 256x256, 3 = 128x128):
    //  * 128 x 256 DMA tiles, two workgroups per CU, when they give at least VF_GEMM_DMA_MIN_WGS workgroups
    //    (16x16x32 MFMAs: 4 % faster in isolation, 6 % on the 100-pair forward than the 32x32x16 form);
    //  * 128 x 128 register-staged tiles for everything smaller (micro-batches of 8 pairs, single queries).
    // The 256 x 256 single-workgroup-per-CU kernel measured equal in isolation and 6 % slower inside the forward
    // (its GELU epilogue has nothing to hide under); it stays selectable for experiments.
    const GemmKnobs& kn = in.knobs;
    const int M = in.M, N = in.N, K = in.K, kind = kn.kind, epi = in.epi;
    const bool dma_ok = M % DBM == 0 && N % DBN == 0 && K % DBK == 0;
    const bool big_ok = M % LBM == 0 && N % LBN == 0 && K % PBK == 0;   // whole 256 x 256 x 64 tiles
    const long long tiles_ll = (long long)(M / PBM) * (N / PBN);       // 256 x 256 tiles: what every rule below counts
    const int tiles = (int)tiles_ll, nkt = K / PBK;
    const int cus = in.n_cu, ncu8 = in.n_cu & ~7;                       // (the persistent kernel runs on whole XCD rows of workgroups)
    const bool forced = kn.p8_forced;
    GemmRoute r;
    const auto small_tiles = [&] {   // the 128 x 256 DMA kernel where it fills the chip (kind 5: wherever it divides), else 128 x 128
        const long long dma_wgs = (long long)(M / DBM) * (N / DBN);
        const bool dma = epi == EPI_RESIDUAL_F32 ? (dma_wgs >= kn.dma_min_wgs && kind != 3) : (kind == 5 || (kind == 0 && dma_wgs >= kn.dma_min_wgs));
        if (dma_ok && dma) { r.kernel = kGemmDma16; r.grid = (int)dma_wgs; }
        else { r.kernel = kGemmTn128; r.grid = (N / GBN) * (M / GBM); }
        return r;
    };
    if (epi == EPI_RESIDUAL_F32) {   // fp32 residual epilogue: 8-phase, the 128 x 256 DMA kernel or the 128 x 128 one
        if (big_ok && K >= 2 * PBK && (kind == 7 || (kind == 0 && tiles_ll >= kn.p8_f32_min_wgs))) { r.kernel = kGemm8p; r.grid = tiles; return r; }
        return small_tiles();
    }
    const bool epi9 = epi == EPI_BIAS || epi == EPI_BIAS_GELU || epi == EPI_BIAS_QGELU || epi == EPI_BIAS_RESIDUAL;   // k_gemm9_tn's epilogues
    const bool epi_cut = epi == EPI_BIAS || epi == EPI_BIAS_GELU || epi == EPI_BIAS_RESIDUAL;                        // the ones a co-operative finish serves
    // 256 x 256 8-phase tiles (one workgroup per CU) once they fill the chip 1.5 times over (p8_min_wgs); measured against the
    // 128 x 256 DMA kernel at M = 51200: 225 / 79 / 265 / 246 us vs 278 / 79 / 296 / 295 us (QKV / out / FFN-up / FFN-down
    // shapes of a 768-wide encoder; the vendor library: 210 / 66 / 234 / 217)
    if (epi9) {
        // round 4: the persistent two-phase kernel with the register-direct epilogue (k_gemm9_tn)
        // Default (VF_GEMM_9=0 switches it off) wherever the partial last round does not matter: K < 2048, or whole rounds.  In the 100-pair
        // forward, per layer (profiles/r04_rerank_layer_8p_vs_gemm9.txt): 768 wide: QKV 167 vs 188 us, out projection 82 vs 87, FFN-up + GELU
        // 235 vs 271; 1024 wide: 277 vs 281, 129 vs 127, 408 vs 408.  Long-K products with a remainder (FFN-down: K = 3072 / 4096, 600 / 800
        // tiles) keep the 8-phase kernel, whose split-K tail is worth more there than the persistent pipeline (391 vs 360 us at K = 4096).
        //
        // Mid-size products (the per-rank batches of a data-parallel re-rank: 13 / 25 / 50 pairs x 512 tokens = 78 ... 1200 tiles): every
        // kernel forced on every shape of the layer (tools/gpu_r04_midsize.sh, profiles/r04_midsize_kernels.log) -- the 256 x 256
        // persistent kernel wins from ~128 tiles on (gemm9_min_wgs), partial round or not: 12 800 x 768 x 3072 59.6 us against 89.8 (128 x 256 DMA kernel)
        // and 94.4 (128 x 128), 0.91 x the vendor library; 6 656 x 2304 x 768 27.6 against 34.8 / 41.4.  Below that (78 tiles: out
        // projection and FFN-down of a 13-pair batch) the small-tile kernels are level or ahead (62.8 vs 56.1 us inside the forward).
        // The old gate (1.5 rounds of tiles, shared with the 8-phase kernel) left 10-50 % on mid-size batches.
        //
        // Round 5: LESS than a round of tiles with a long K -- FFN-down of the 13 pairs one rank of an 8-GPU data-parallel re-rank scores
        // (6 656 x 768 x 3072: 78 tiles = a third of the CUs busy for 62.8 us where the vendor library takes 36.5) -- is cut whole
        // along K inside the persistent kernel: S slices per tile (8 x ceil(tiles / 8) x S workgroups <= the CUs, each slice >= 8
        // K-tiles), finished co-operatively through the handle's workspace (sk_coop_finish).  VF_GEMM_9_SPLIT=0 switches it off (A/B).
        if (epi != EPI_BIAS_QGELU && big_ok && K >= kn.split_min_k && (kind == 0 || kind == 11) && kn.gemm9 && kn.gemm9_split && !forced &&
            kn.splitk_tail != 0 && in.has_ws && tiles_ll <= kSkMaxTiles) {
            const int pad = pad8(tiles);
            for (int c = 4; c >= 2; --c)
                if (pad * c <= ncu8 && nkt / c >= kn.split_min_kt && (size_t)tiles * c * kSkTileBytes <= in.ws_bytes) {
                    r.kernel = kGemm9Split; r.grid = pad * c; r.slices = c;
                    return r;
                }
        }
        // Round 5, stream-K (k_gemm9_tn<EPI, 2>): a product whose LAST round is mostly empty -- 1.2 rounds of FFN-up at 13 pairs, 2.3 of
        // FFN-up / 0.6 of FFN-down at 25, 2.3 of FFN-down at 100 -- deals the K-tiles out evenly instead of the tiles, when that saves at
        // least VF_GEMM_9_STREAMK_MIN_SAVED K-tiles of a workgroup's time over whole tiles.  Built, exact, deterministic -- and SLOWER on
        // every shape of the forward, so OFF unless asked for (VF_GEMM_9_STREAMK=1, vf_debug_gemm9_streamk(1), kind 12): nearly every
        // workgroup dumps one 256-KB fp32 partial and reads one back -- 64 MB written through and 64 MB read per launch, ~27 us at what the
        // chip sustains for that -- against the 10-20 us the even deal saves: 6 656 x 3072 x 768 64.7 us against 49.7 with whole tiles,
        // 12 800 x 768 x 3072 90.8 against 79.0, the 13- / 25- / 100-pair forwards 2.62 / 4.38 / 13.0 ms against 2.39 / 3.77 / 11.3, same
        // box, same call (profiles/r05_streamk.log).  The whole-product cut above pays the same toll per slice but only where two thirds of
        // the chip would otherwise idle.
        // (off even in the experiments build unless asked for; the default build does not carry the kernel)
        if (kn.experiments && epi != EPI_BIAS_QGELU && big_ok && K >= 4 * PBK && (kind == 12 || (kind == 0 && kn.gemm9 && kn.gemm9_streamk && !forced)) &&
            in.has_ws && ncu8 >= 8 && ncu8 <= kSkMaxTiles) {
            const long long dp_len = (tiles_ll + ncu8 - 1) / ncu8 * nkt, sk_len = (tiles_ll * nkt + ncu8 - 1) / ncu8;
            if ((kind == 12 || dp_len - sk_len >= kn.streamk_min_saved) && tiles_ll >= 8 && tiles_ll <= 12ll * ncu8 /* <= 16 segments per workgroup */ &&
                (tiles_ll / 8) * nkt / (ncu8 / 8) >= 6 && (size_t)ncu8 * kSkTileBytes <= in.ws_bytes) {
                r.kernel = kGemm9StreamK; r.grid = ncu8;
                return r;
            }
        }
        const bool p9_size = tiles_ll >= (forced ? kn.p8_min_wgs : kn.gemm9_min_wgs);
        if (big_ok && K >= 4 * PBK && ncu8 > 0 && (kind == 10 || (kind == 0 && kn.gemm9 && p9_size))) {
            const int G = tiles < ncu8 ? tiles : ncu8;
            // long-K products of MORE than two rounds with a remainder keep the 8-phase kernel (split-K tail): 800 tiles at K = 4096 360 vs
            // 391 us, 600 at K = 3072 231 vs 235; up to two rounds the persistent kernel is level or ahead (400 tiles at K = 4096: 178 vs
            // 188 us; 300 at K = 3072: 131 vs 126; profiles/r04_midsize_kernels.log, r04_midsize_large.log)
            // Round 5, after the relaxed arrival made the finish cheaper: between one and two rounds, when the remainder can be cut at least
            // in two (<= half the CUs), the 8-phase kernel's tail wins as well -- 300 tiles at K = 3072 (FFN-down of 50 pairs) 136 vs
            // 145-147 us; a remainder too large to cut stays here (450 tiles: 180-183 vs 186-187; profiles/r05_tail8p_vs_gemm9.log)
            // (under an epilogue no co-operative finish serves there is no tail to win with: a workspace then changes nothing)
            if (kind == 10 || K < kLongK || tiles % G == 0 || (tiles <= 2 * ncu8 && !(epi_cut && tail_cuttable(in, tiles, ncu8)))) {
                // a tile's time in ticks of the 100 MHz real-time counter: ~1.5 us per K-tile + 2 (the stagger spreads the workgroups over it)
                r.kernel = kGemm9; r.grid = G;
                r.stagger_ticks = tiles > ncu8 ? (int)((150ll * nkt + 200) * kn.stagger_pct / 100) : 0;
                return r;
            }
        }
    }
    const Cut8 c8 = cut8(tiles, cus, nkt);
    // Less than HALF a round of 256 x 256 tiles with a very long K (FFN-down of a 13-pair batch at 1024 wide: 104 tiles, K = 4096): the
    // 8-phase kernel with EVERY tile cut along K (2-4 slices, co-operative finish) -- 6656 x 1024 x 4096 67-68 us against 78-80 (128 x 128
    // tiles) and 80 (persistent kernel, 104 workgroups); the 13-pair forward 6.36 -> 6.17 ms.  At K = 3072 (78 tiles, 768 wide) the cut wins
    // 3 % in isolation (55-56 us against 56-58) and LOSES 4 % inside the forward (2.52 against 2.42 ms: 40 MB of partials through a cold
    // L2), so the gate is K >= 4096 (profiles/r04_skcoop.log, r04_skcoop_forward.log)
    // (tiles <= CUs: the whole product is the tail, so c8.S is the slice count the launch uses)
    const bool sub_split = epi_cut && kind == 0 && !forced && big_ok && K >= kSubSplitMinK && tiles_ll <= cus && cut_fits(in, c8.ntail, c8.S);
    // one to two rounds, long K, a remainder that can be cut at least in two: this kernel's split-K tail (see the persistent kernel's gate above)
    const bool tail8 = epi_cut && kind == 0 && !forced && big_ok && tiles_ll <= 2ll * ncu8 && tail_cuttable(in, tiles, ncu8);
    if (big_ok && K >= 2 * PBK &&
        (kind == 7 || sub_split || tail8 || (kind == 0 && (tiles_ll >= kn.p8_min_wgs || (K >= kLongK && tiles_ll > 2 * ncu8 && !forced))))) {
        // (Peeling the rows of a partial last round -- 600 tiles on 256 CUs are 2.34 rounds of work in 3 -- into the 128 x 256
        // kernel was measured: no gain, the half-size workgroups alone on their CUs run at a quarter of the MFMA rate.)
        // Round 3: the tiles of the partial last round are cut along K instead (LnFold::sk_*): S slices per tail tile so that
        // the slices still fit one round, each at least two K-tiles long.
        r.kernel = kGemm8p; r.grid = tiles;
        if (epi_cut) {
            // Measured (tools/gpu_r03_splitk.sh): a slice pays ~5 us to leave its 256 KB of partials and the last arrival ~9 us per
            // 256 KB it reads back from memory (one CU pulls 50-60 GB/s), so the cut only pays where half a tile's main loop is
            // worth more: long-K products (K >= 2048: FFN-down), two slices.  Cutting the K = 768 products (S = 2..4) made the
            // forward SLOWER (12.53 vs 12.26 ms); the general form stays reachable through vf_debug_splitk_tail(2).
            int S = c8.S;
            if (kn.splitk_tail == 1 && !sub_split) S = (nkt >= kLongK / PBK && S >= 2 && tiles > cus) ? 2 : 0;
            if (cut_fits(in, c8.ntail, S)) {
                r.slices = S; r.tail_tiles = c8.ntail; r.full_tiles = tiles - c8.ntail;
                r.grid = r.full_tiles + c8.pad * S;
            }
        }
        return r;
    }
    return small_tiles();
}

// ---- the small decisions beside gemm() -------------------------------------------------------------------------------------------------
// Gated MLP front half in one launch of the 8-phase kernel (C[M][F] = act(A . Wgate^T) * (A . Wup^T), N = 2 F columns): only where the shape
// fills that kernel; the caller runs the plain product + k_swiglu otherwise.
constexpr long long kGatedMinWgs = 384;
inline bool gated_ok(int M, int F, int K) {
    const int N = 2 * F;
    return !(M % PBM || N % PBN || F % 128 || K % PBK || K < 2 * PBK || (long long)(M / PBM) * (N / PBN) < kGatedMinWgs);
}

// k_gemm_skinny: K split over workgroups when K is long and the column tiles alone leave most of the chip idle (see the kernel)
inline int skinny_slices(int N, int K, bool can_split) {
    int S = 1;
    if (can_split && K >= kLongK && N / 16 <= 64 && N / 16 <= 4096)
        for (int c = 2; c <= kSplitMax; ++c)
            if (K % (c * 256) == 0 && (N / 16) * c <= 256) S = c;
    return S;
}

// split count for the small-M kernel (k_gemm_splitk): enough workgroups to cover the chip, at least two K-steps per split
inline int pick_splits(int tiles, int K) {
    const int steps = K / SBK;
    int best = 1;
    for (int sp = 1; sp <= kSplitMax; ++sp)
        if (steps % sp == 0 && steps / sp >= 2 && tiles * sp <= 512) best = sp;
    return best;
}

// The encoder forward's product class.  Skinny: one short sequence (M <= 64 rows), weight-streaming products for all four of a layer.
// Short: a single short sequence (its rows padded to 64 within kSplitMaxRows) -- the long-K product (FFN-down, K = ffn >= 2048) is split
// over K across the chip (1.17 -> 1.00 ms per forward); the K = hidden products are not (the split's extra dependent memory round trips
// cost more than 12 short K-steps), nor anything from 256 tokens up (measured slower).  Everything else: route_gemm.
enum EncProduct : int { kEncGeneral = 0, kEncSkinny = 1, kEncSplitK = 2 };
inline bool enc_skinny(int M, int H, int F) { return M <= 64 && H % 256 == 0 && F % 256 == 0; }
inline bool enc_short(int M, int H, int F) { return (M + 63) / 64 * 64 <= kSplitMaxRows && H % 64 == 0 && F % 64 == 0; }
inline EncProduct enc_product_class(int M, int H, int F, bool ffn_down, bool allow_skinny, bool allow_splitk) {
    if (allow_skinny && enc_skinny(M, H, F)) return kEncSkinny;
    if (ffn_down && allow_splitk && enc_short(M, H, F) && F >= kLongK) return kEncSplitK;
    return kEncGeneral;
}

}  // namespace vft
