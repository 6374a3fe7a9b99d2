"""A host-compiled driver of a prepared filter's all-columns count (veritasfi_amd/csrc/vf_bm25_prepared.h), used by
tests/test_bm25_prepared_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone.  It reads
a CSC index, a list of chunk sizes and a list of filters from a text file and REPLAYS the launch of k_bm25_sub_df_all chunk by chunk
and thread by thread with the header's own functions (bm25p_cpu_df_all: live_chunk, the flags and their exclusive prefix, bm25p_first_col,
bm25p_end_col, bm25p_span), over the device bitmap zero-padded to whole blocks.  It checks on its own that every posting was flagged
exactly once, that a column received a plain store at most once and never both a store and an add, and that a column was added to at
most once per chunk it crosses; it prints df for every column, and the test compares that with numpy.

  input   n V nnz NC F / indptr [V + 1] / indices [nnz] / NC chunk sizes / F lines: the filter's row count, then its rows
  output  per (chunk size, filter) "c <C> f <i> m <rows> df <V counts>", last "prepared: <failures> failure(s)"
"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "vf_bm25_prepared.h"
using namespace vf;

static long long failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long n, V, nnz, NC, F;
    if (std::fscanf(f, "%lld %lld %lld %lld %lld", &n, &V, &nnz, &NC, &F) != 5) return 2;
    std::vector<long long> indptr((size_t)V + 1);
    std::vector<int> indices((size_t)nnz), chunk((size_t)NC);
    for (auto& v : indptr) if (std::fscanf(f, "%lld", &v) != 1) return 2;
    for (auto& v : indices) if (std::fscanf(f, "%d", &v) != 1) return 2;
    for (auto& v : chunk) if (std::fscanf(f, "%d", &v) != 1 || v < 1 || v > kLiveMaxChunk) return 2;

    const long long cw = bm25f_words(n);
    const long long words = (cw + kBm25FilterBlockWords - 1) / kBm25FilterBlockWords * kBm25FilterBlockWords;   // the handle's `words`
    std::vector<uint32_t> allow((size_t)words, 0u);   // the device copy: zero past the caller's words
    std::vector<int32_t> df((size_t)(V > 0 ? V : 1));
    std::vector<int> seen((size_t)(nnz > 0 ? nnz : 1)), stores((size_t)(V > 0 ? V : 1)), adds((size_t)(V > 0 ? V : 1));
    for (long long i = 0; i < F; ++i) {
        long long cnt;
        if (std::fscanf(f, "%lld", &cnt) != 1) return 2;
        std::fill(allow.begin(), allow.end(), 0u);
        for (long long j = 0; j < cnt; ++j) {
            long long r;
            if (std::fscanf(f, "%lld", &r) != 1 || r < 0 || r >= n) return 2;
            allow[(size_t)(r >> 5)] |= 1u << (r & 31);
        }
        const Bm25FilterCheck fc = bm25f_check(allow.data(), n);
        CHECK(fc.bad_row == -1, "filter %lld: refused at row %lld", i, fc.bad_row);
        for (int C : chunk) {
            std::fill(seen.begin(), seen.end(), 0);
            std::fill(stores.begin(), stores.end(), 0);
            std::fill(adds.begin(), adds.end(), 0);
            bm25p_cpu_df_all(indptr.data(), indices.data(), V, nnz, allow.data(), C, df.data(), seen.data(), stores.data(), adds.data());
            for (long long p = 0; p < nnz; ++p) CHECK(seen[p] == 1, "C %d filter %lld: posting %lld was flagged %d times", C, i, p, seen[p]);
            for (long long c = 0; c < V; ++c) {
                const long long p0 = indptr[c], p1 = indptr[c + 1];
                const long long crossed = p1 > p0 ? (p1 - 1) / C - p0 / C + 1 : 0;   // chunks the column has a posting in
                CHECK(stores[c] <= 1 && !(stores[c] && adds[c]), "C %d filter %lld: column %lld got %d stores and %d adds", C, i, c, stores[c], adds[c]);
                CHECK(stores[c] == (crossed == 1 ? 1 : 0), "C %d filter %lld: column %lld in %lld chunk(s) got %d stores", C, i, c, crossed, stores[c]);
                CHECK(adds[c] <= (crossed > 1 ? crossed : 0), "C %d filter %lld: column %lld in %lld chunk(s) got %d adds", C, i, c, crossed, adds[c]);
            }
            std::printf("c %d f %lld m %lld df", C, i, fc.m);
            for (long long c = 0; c < V; ++c) std::printf(" %d", df[(size_t)c]);
            std::printf("\n");
        }
    }
    std::fclose(f);
    std::printf("prepared: %lld failure(s)\n", failures);
    return failures ? 1 : 0;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "bm25_prepared.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "bm25_prepared")
    subprocess.check_call([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def write_input(path, n, indptr, indices, chunks, filters) -> str:
    """The driver's input file; ``filters`` is a list of row lists."""
    with open(path, "w") as f:
        f.write(f"{n} {len(indptr) - 1} {len(indices)} {len(chunks)} {len(filters)}\n")
        for arr in (indptr, indices, chunks):
            f.write(" ".join(str(int(v)) for v in arr) + "\n")
        for rows in filters:
            f.write(" ".join(str(int(v)) for v in [len(rows)] + list(rows)) + "\n")
    return str(path)


def run(exe: str, input_path: str):
    return subprocess.run([exe, input_path], capture_output=True, text=True, timeout=600, env=_ENV)


def parse(stdout: str):
    """-> {(C, filter index): (m, [df per column])}."""
    out = {}
    for line in stdout.splitlines():
        if line.startswith("c "):
            w = line.split()
            out[(int(w[1]), int(w[3]))] = (int(w[5]), [int(v) for v in w[7:]])
    return out
