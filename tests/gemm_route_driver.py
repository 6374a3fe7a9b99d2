"""A host-compiled driver of the GEMM route (veritasfi_amd/csrc/vf_gemm_route.h), shared by tests/test_gemm_route.py (no GPU) and
tests/test_gpu_gemm_route.py (what the library would decide against the driver's prediction).

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone:

  driver eval    reads one question per line of stdin ("key=value key=value ..."), prints the answer as one line of "key=value"
  driver sweep   walks the shape / knob grid and holds every route to what the kernels rely on; prints the count and the failures

A question is a product for route_gemm (fn=0, the default) or one of the small decisions beside it: fn=1 gated_ok, fn=2 skinny_slices,
fn=3 pick_splits, fn=4 enc_product_class."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "vf_gemm_route.h"
using namespace vft;

static int eval_lines() {
    char line[4096];
    while (std::fgets(line, sizeof line, stdin)) {
        std::map<std::string, double> kv;
        for (char* tok = std::strtok(line, " \n"); tok; tok = std::strtok(nullptr, " \n")) {
            char* eq = std::strchr(tok, '=');
            if (!eq) { std::printf("error=bad-token\n"); return 2; }
            kv[std::string(tok, eq - tok)] = std::atof(eq + 1);
        }
        auto get = [&](const char* name, double dflt) { auto it = kv.find(name); if (it == kv.end()) return dflt; double v = it->second; kv.erase(it); return v; };
        const int fn = (int)get("fn", 0);
        GemmIn in;
        in.epi = (int)get("epi", 0); in.M = (int)get("M", 0); in.N = (int)get("N", 0); in.K = (int)get("K", 0); in.n_cu = (int)get("n_cu", 256);
        in.has_ws = get("ws", 1) != 0;
        const bool ws_auto = get("ws_auto", 0) != 0;   // sized as the library sizes a handle's workspace for that many CUs
        in.ws_bytes = in.has_ws ? (ws_auto ? gemm_ws_bytes(in.n_cu) : (size_t)get("ws_bytes", 64.0 * 1048576.0)) : 0;
        GemmKnobs& k = in.knobs;
#define KNOB(f, T) k.f = (T)get(#f, (double)k.f);
        KNOB(kind, int) KNOB(dma_min_wgs, long long) KNOB(p8_min_wgs, long long) KNOB(p8_forced, bool) KNOB(p8_f32_min_wgs, long long)
        KNOB(gemm9, int) KNOB(gemm9_min_wgs, long long) KNOB(gemm9_split, int) KNOB(split_min_k, int) KNOB(split_min_kt, int)
        KNOB(gemm9_streamk, int) KNOB(streamk_min_saved, int) KNOB(splitk_tail, int) KNOB(stagger_pct, int) KNOB(experiments, bool)
#undef KNOB
        const int F = (int)get("F", 0), H = (int)get("H", 0), tiles = (int)get("tiles", 0);
        const bool can_split = get("can_split", 1) != 0, ffn_down = get("ffn_down", 0) != 0, allow_skinny = get("allow_skinny", 1) != 0,
                   allow_splitk = get("allow_splitk", 1) != 0;
        if (!kv.empty()) { std::printf("error=unknown-key:%s\n", kv.begin()->first.c_str()); return 2; }
        if (fn == 1) std::printf("ok=%d\n", (int)gated_ok(in.M, F, in.K));
        else if (fn == 2) std::printf("slices=%d\n", skinny_slices(in.N, in.K, can_split));
        else if (fn == 3) std::printf("splits=%d\n", pick_splits(tiles, in.K));
        else if (fn == 4) std::printf("cls=%d\n", (int)enc_product_class(in.M, H, F, ffn_down, allow_skinny, allow_splitk));
        else {
            const GemmRoute r = route_gemm(in);
            std::printf("kernel=%d grid=%d slices=%d tail=%d full=%d ticks=%d\n", (int)r.kernel, r.grid, r.slices, r.tail_tiles, r.full_tiles, r.stagger_ticks);
        }
    }
    return 0;
}

static long long failures = 0, checked = 0, seen[6];
static GemmIn cur;
#define CHECK(c) do { if (!(c)) { if (failures < 20) std::printf("FAIL %s: epi=%d M=%d N=%d K=%d n_cu=%d kind=%d splitk_tail=%d ws=%d gemm9=%d gemm9_split=%d " \
    "p8_min_wgs=%lld p8_forced=%d gemm9_streamk=%d experiments=%d\n", #c, cur.epi, cur.M, cur.N, cur.K, cur.n_cu, cur.knobs.kind, cur.knobs.splitk_tail, (int)cur.has_ws, \
    cur.knobs.gemm9, cur.knobs.gemm9_split, cur.knobs.p8_min_wgs, (int)cur.knobs.p8_forced, cur.knobs.gemm9_streamk, (int)cur.knobs.experiments); ++failures; } } while (0)

static void check(const GemmIn& in) {
    cur = in;
    const GemmRoute r = route_gemm(in);
    ++checked; ++seen[r.kernel];
    const int M = in.M, N = in.N, K = in.K, tiles = (M / 256) * (N / 256), nkt = K / 64, ncu8 = in.n_cu & ~7;
    const bool whole256 = M % 256 == 0 && N % 256 == 0 && K % 64 == 0;
    CHECK(r.grid >= 1);
    switch (r.kernel) {
    case kGemmTn128: CHECK(M % 128 == 0 && N % 128 == 0 && K % 64 == 0 && r.grid == (M / 128) * (N / 128)); break;
    case kGemmDma16: CHECK(M % 128 == 0 && N % 256 == 0 && K % 32 == 0 && r.grid == (M / 128) * (N / 256)); break;
    case kGemm8p: CHECK(whole256 && K >= 128); break;
    case kGemm9: CHECK(whole256 && K >= 256 && r.grid <= ncu8 && r.grid == std::min(tiles, ncu8)); break;
    case kGemm9Split: CHECK(whole256 && K >= 256 && r.grid <= ncu8); break;
    case kGemm9StreamK: CHECK(whole256 && K >= 256 && r.grid == ncu8 && in.has_ws && (size_t)r.grid * 262144 <= in.ws_bytes); break;
    default: CHECK(!"a kernel code"); }
    if (r.kernel != kGemm9) CHECK(r.stagger_ticks == 0);
    if (r.kernel == kGemm9 || r.kernel == kGemm9Split || r.kernel == kGemm9StreamK) CHECK(in.epi == 0 || in.epi == 1 || in.epi == 2 || in.epi == 11);
    if (r.kernel == kGemm9Split) {
        CHECK(r.slices >= 2 && r.slices <= 4 && r.grid == ((tiles + 7) & ~7) * r.slices && r.tail_tiles == 0 && r.full_tiles == 0);
        CHECK(nkt / r.slices >= in.knobs.split_min_kt && tiles <= kSkMaxTiles && (size_t)tiles * r.slices * 262144 <= in.ws_bytes);
    } else if (r.kernel == kGemm8p && r.slices) {
        const int padt = (r.tail_tiles + 7) & ~7;
        CHECK(r.slices >= 2 && r.slices <= 4 && nkt / r.slices >= 2 && r.tail_tiles >= 1 && r.tail_tiles + r.full_tiles == tiles);
        CHECK(r.grid == r.full_tiles + padt * r.slices && padt * r.slices <= in.n_cu);
        CHECK(r.tail_tiles <= kSkMaxTiles && (size_t)r.tail_tiles * r.slices * 262144 <= in.ws_bytes);
    } else {
        CHECK(r.slices == 0 && r.tail_tiles == 0 && r.full_tiles == 0);
        if (r.kernel == kGemm8p) CHECK(r.grid == tiles);
    }
    // no cut of any kind without a workspace, with the tail off, or under an epilogue no co-operative finish serves
    if (!in.has_ws || in.knobs.splitk_tail == 0 || in.epi == 3 || in.epi == 11) CHECK(r.slices == 0 && r.kernel != kGemm9Split);
    if (in.epi == 3 || in.epi == 11) CHECK(r.kernel != kGemm9StreamK);
    // ... so under those two a workspace changes nothing at all: a caller may pass one to every product (the pre-LayerNorm layer loop does)
    if ((in.epi == 3 || in.epi == 11) && in.has_ws) {
        GemmIn bare = in;
        bare.has_ws = false; bare.ws_bytes = 0;
        const GemmRoute b = route_gemm(bare);
        CHECK(b.kernel == r.kernel && b.grid == r.grid && b.slices == r.slices && b.tail_tiles == r.tail_tiles && b.full_tiles == r.full_tiles &&
              b.stagger_ticks == r.stagger_ticks);
    }
    // stream-K only where it is compiled in AND asked for
    if (r.kernel == kGemm9StreamK) CHECK(in.knobs.experiments && (in.knobs.gemm9_streamk || in.knobs.kind == 12));
}

static int sweep() {
    const int epis[] = {0, 1, 2, 3, 11};
    const int Ms[] = {128, 256, 3328, 4096, 6528, 6656, 12800, 25600, 32512, 32768, 38400, 51200};
    const int Ns[] = {128, 256, 768, 1024, 2304, 2560, 3072, 4096};
    const int Ks[] = {64, 128, 192, 256, 320, 768, 1024, 1984, 2048, 2112, 3072, 4096};
    const int cus[] = {8, 64, 256, 304};
    const int kinds[] = {0, 3, 5, 7, 10, 11, 12};
    const long long p8s[] = {-1, 1, 1ll << 40};   // the 8-phase gate: unforced, forced to 1, forced to 2^40
    for (int epi : epis) for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int n_cu : cus) for (int kind : kinds)
    for (int tail = 0; tail <= 2; ++tail) for (int ws = 0; ws < 2; ++ws) for (int g9 = 0; g9 < 2; ++g9) for (int g9s = 0; g9s < 2; ++g9s)
    for (long long p8 : p8s) for (int sk = 0; sk < 2; ++sk) for (int ex = 0; ex < 2; ++ex) {
        GemmIn in;
        in.epi = epi; in.M = M; in.N = N; in.K = K; in.n_cu = n_cu;
        in.has_ws = ws != 0; in.ws_bytes = ws ? gemm_ws_bytes(n_cu) : 0;
        in.knobs.kind = kind; in.knobs.splitk_tail = tail; in.knobs.gemm9 = g9; in.knobs.gemm9_split = g9s;
        if (p8 >= 0) { in.knobs.p8_min_wgs = p8; in.knobs.p8_forced = true; }
        in.knobs.gemm9_streamk = sk; in.knobs.experiments = ex != 0;
        check(in);
    }
    std::printf("gemm route sweep: %lld products checked (tn128 %lld, dma16 %lld, 8p %lld, gemm9 %lld, gemm9-split %lld, gemm9-streamk %lld), %lld failure(s)\n",
                checked, seen[0], seen[1], seen[2], seen[3], seen[4], seen[5], failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "eval")) return eval_lines();
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    std::printf("usage: %s eval|sweep\n", argv[0]);
    return 2;
}
"""

KERNELS = {"tn128": 0, "dma16": 1, "8p": 2, "gemm9": 3, "gemm9-split": 4, "gemm9-streamk": 5}
FNS = {"gemm": 0, "gated": 1, "skinny": 2, "splits": 3, "enc": 4}
_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "gemm_route.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "gemm_route")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def evaluate(exe: str, cases) -> list:
    """cases: dicts of the driver's keys (fn by name or number).  Returns one dict of ints per case."""
    lines = []
    for c in cases:
        c = dict(c)
        if isinstance(c.get("fn"), str):
            c["fn"] = FNS[c["fn"]]
        lines.append(" ".join(f"{k}={v}" for k, v in c.items()))
    run = subprocess.run([exe, "eval"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=_ENV)
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    out = [dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in ln.split()) for ln in run.stdout.strip().split("\n")]
    assert len(out) == len(cases), run.stdout[-2000:]
    return out


def sweep(exe: str):
    return subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=900, env=_ENV)
