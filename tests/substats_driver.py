"""A host-compiled driver of the subset-statistics counts (veritasfi_amd/csrc/vf_bm25_substats.h), used by
tests/test_bm25_substats_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone.  It reads
a CSC index, the document lengths, a batch's q_terms and a list of filters from a text file and EXECUTES the stage of a
VF_BM25_SUBSTATS request the way the entry point and the kernels do, with the header's own functions: the de-duplication of the batch's
columns (bm25s_dedupe), the device bitmap zero-padded to whole blocks, the length sum block by block and thread by thread
(bm25s_len_word0, bm25s_word_len), and the df count over the launch's grid (bm25s_df_plan, bm25s_df_base), where every posting of a
distinct column must be looked at exactly once.  It prints what the stage would return; the test compares that with numpy.

  input   n V nnz T F / indptr [V + 1] / indices [nnz] / doclen [n] / q_terms [T] / F lines: the filter's row count, then its rows
  output  "distinct <D> : <columns>", "pos2d : <T indices>", then per filter "f <i> m <rows> len <sum> df <T counts, per position>",
          last "substats: <failures> failure(s)" (a posting looked at twice or never, a bitmap the check refuses)"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "vf_bm25_substats.h"
using namespace vf;

static long long failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    long long n, V, nnz, T, F;
    if (std::fscanf(f, "%lld %lld %lld %lld %lld", &n, &V, &nnz, &T, &F) != 5) return 2;
    std::vector<long long> indptr((size_t)V + 1);
    std::vector<int> indices((size_t)nnz), doclen((size_t)n);
    std::vector<int32_t> q_terms((size_t)T);
    for (auto& v : indptr) if (std::fscanf(f, "%lld", &v) != 1) return 2;
    for (auto& v : indices) if (std::fscanf(f, "%d", &v) != 1) return 2;
    for (auto& v : doclen) if (std::fscanf(f, "%d", &v) != 1) return 2;
    for (auto& v : q_terms) if (std::fscanf(f, "%d", &v) != 1) return 2;

    std::vector<int32_t> distinct, pos2d;
    const long long D = bm25s_dedupe(q_terms.data(), T, distinct, pos2d);
    std::printf("distinct %lld :", D);
    for (int32_t c : distinct) std::printf(" %d", c);
    std::printf("\npos2d :");
    for (int32_t d : pos2d) std::printf(" %d", d);
    std::printf("\n");

    const long long cw = bm25f_words(n);
    const long long words = (cw + kBm25FilterBlockWords - 1) / kBm25FilterBlockWords * kBm25FilterBlockWords;   // the handle's `words`
    std::vector<uint32_t> allow((size_t)words, 0u);   // the device copy: zero past the caller's words
    std::vector<int32_t> df((size_t)(D > 0 ? D : 1));
    std::vector<int> seen((size_t)(nnz > 0 ? nnz : 1));
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
        const unsigned long long total = bm25s_cpu_len(allow.data(), words, n, doclen.data());
        std::fill(seen.begin(), seen.end(), 0);
        bm25s_cpu_df(indptr.data(), indices.data(), allow.data(), distinct.data(), D, df.data(), seen.data());
        std::vector<char> asked((size_t)V + 1, 0);
        for (int32_t c : distinct) asked[(size_t)c] = 1;
        for (long long c = 0; c < V; ++c)
            for (long long p = indptr[c]; p < indptr[c + 1]; ++p)
                CHECK(seen[p] == (asked[c] ? 1 : 0), "filter %lld: posting %lld of column %lld was looked at %d times", i, p, c, seen[p]);
        std::printf("f %lld m %lld len %llu df", i, fc.m, total);
        for (long long t = 0; t < T; ++t) std::printf(" %d", df[(size_t)pos2d[(size_t)t]]);
        std::printf("\n");
    }
    std::fclose(f);
    // the grid plan: at least one workgroup, never more than the cap, and enough for one pass up to the cap
    for (long long p : {0ll, 1ll, 2047ll, 2048ll, 2049ll, 1000000ll, 4194304ll, 4194305ll, 3000000000ll}) {
        const unsigned g = bm25s_df_plan(p);
        const long long per = (long long)kBm25SubThreads * kBm25SubPostingsPerThread;
        CHECK(g >= 1 && g <= (unsigned)kBm25SubMaxChunks, "plan(%lld) = %u", p, g);
        CHECK(g == (unsigned)kBm25SubMaxChunks || (long long)g * per >= p, "plan(%lld) = %u workgroups of %lld postings", p, g, per);
        CHECK(bm25s_df_base(7, 0, g, 0) == 7 && bm25s_df_base(7, 1, g, 1) == 7 + (1 + (long long)g) * kBm25SubThreads, "base of plan(%lld)", p);
    }
    std::printf("substats: %lld failure(s)\n", failures);
    return failures ? 1 : 0;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "bm25_substats.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "bm25_substats")
    subprocess.check_call([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def write_input(path, n, indptr, indices, doclen, q_terms, filters) -> str:
    """The driver's input file; ``filters`` is a list of row lists."""
    with open(path, "w") as f:
        f.write(f"{n} {len(indptr) - 1} {len(indices)} {len(q_terms)} {len(filters)}\n")
        for arr in (indptr, indices, doclen, q_terms):
            f.write(" ".join(str(int(v)) for v in arr) + "\n")
        for rows in filters:
            f.write(" ".join(str(int(v)) for v in [len(rows)] + list(rows)) + "\n")
    return str(path)


def run(exe: str, input_path: str):
    return subprocess.run([exe, input_path], capture_output=True, text=True, timeout=600, env=_ENV)


def parse(stdout: str):
    """-> (distinct columns, pos2d, [(m, len, [df per position])] per filter)."""
    distinct = pos2d = None
    rows = []
    for line in stdout.splitlines():
        w = line.split()
        if line.startswith("distinct "):
            distinct = [int(v) for v in w[3:]]
        elif line.startswith("pos2d :"):
            pos2d = [int(v) for v in w[2:]]
        elif line.startswith("f "):
            rows.append((int(w[3]), int(w[5]), [int(v) for v in w[7:]]))
    return distinct, pos2d, rows
