"""A host-compiled driver of the removal's compaction plan (veritasfi_amd/csrc/vf_compact.h), used by tests/test_compact_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone:

  driver small   every n <= 12, every subset of removed rows, every chunk size 1 .. n: the plan is EXECUTED on an integer array the
                 way the library executes it on the device (per chunk: gather into a staging array, then scatter) and held to the
                 plain deletion and to what makes the scheme safe without any synchronisation but launch order
  driver large   seeded random cases of up to 2^32 - 2 rows: plan arithmetic only, no arrays (overflow)
  driver units   the access width and rows-per-workgroup the launcher picks

Each prints the number of cases and the first failures, and returns 1 if there was one."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <random>
#include <vector>
#include "vf_compact.h"
using namespace vf;

static long long failures = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

static int small() {
    for (int n = 0; n <= 12; ++n)
    for (unsigned mask = 0; mask < (1u << n); ++mask)
    for (int cap = 1; cap <= std::max(n, 1); ++cap) {
        ++cases;
        std::vector<long long> rem, want, a(n), stage(cap, -1);
        for (int i = 0; i < n; ++i) { a[i] = 1000 + i; if (mask >> i & 1) rem.push_back(i); else want.push_back(1000 + i); }
        const long long m = (long long)rem.size(), n1 = n - m;
        const CompactPlan p = compact_plan(n, m, m ? rem[0] : 0, cap);
        CHECK(p.end == n1 && p.first <= p.end && p.chunk_rows >= 1 && p.chunk_rows <= cap, "n=%d mask=%u cap=%d", n, mask, cap);
        CHECK(m == 0 ? p.chunks == 0 : p.first == std::min(rem[0], n1), "n=%d mask=%u cap=%d first=%lld", n, mask, cap, p.first);
        CHECK((p.chunks == 0) == (p.first == p.end), "n=%d mask=%u cap=%d chunks=%lld", n, mask, cap, p.chunks);
        std::vector<char> read(n, 0), written(n, 0);
        long long prev_hi = p.first;
        for (long long c = 0; c < p.chunks; ++c) {
            const CompactChunk k = compact_chunk(p, c);
            // chunks are disjoint, ascending and tile [first, end); the staging array holds each
            CHECK(k.lo == prev_hi && k.hi > k.lo && k.hi <= p.end && k.hi - k.lo <= cap, "n=%d mask=%u cap=%d chunk %lld = [%lld, %lld)", n, mask, cap, c, k.lo, k.hi);
            for (long long j = k.lo; j < k.hi; ++j) {          // gather
                const long long s = compact_src(j, rem.data(), m);
                // no chunk reads a row below the previous chunk's destination end (= its own first row), nor past the array
                CHECK(s >= k.lo && s >= j && s < n, "n=%d mask=%u cap=%d j=%lld src=%lld", n, mask, cap, j, s);
                if (s < 0 || s >= n) return 1;
                read[s] = 1;
                stage[j - k.lo] = a[s];
            }
            for (long long j = k.lo; j < k.hi; ++j) { a[j] = stage[j - k.lo]; written[j] = 1; }   // scatter
            prev_hi = k.hi;
        }
        CHECK(prev_hi == p.end, "n=%d mask=%u cap=%d: the chunks end at %lld", n, mask, cap, prev_hi);
        for (long long i = 0; i < n; ++i) {
            if (m && i < rem[0]) CHECK(!read[i] && !written[i], "n=%d mask=%u cap=%d: row %lld below the first removed row was touched", n, mask, cap, i);
            if (i >= n1) CHECK(!written[i], "n=%d mask=%u cap=%d: row %lld past the new end was written", n, mask, cap, i);
        }
        a.resize(n1);
        CHECK(a == want, "n=%d mask=%u cap=%d: the result differs from the plain deletion", n, mask, cap);
    }
    std::printf("compact plan, small: %lld cases executed, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

static int large() {
    std::mt19937_64 rng(20261020);
    const long long kMax = 0xFFFFFFFEll;   // rows of the largest shard
    for (int it = 0; it < 20000; ++it) {
        ++cases;
        const long long n0 = it % 4 == 0 ? kMax - (long long)(rng() % 1000) : 1 + (long long)(rng() % kMax);
        const long long mm = 1 + (long long)(rng() % std::min<long long>(n0, 48));
        std::vector<long long> rem;
        const int shape = it % 3;   // scattered over the whole range / near its end / one run from a random row
        const long long run0 = (long long)(rng() % (unsigned long long)(n0 - mm + 1));
        for (long long t = 0; t < mm; ++t)
            rem.push_back(shape == 0 ? (long long)(rng() % (unsigned long long)n0) : shape == 1 ? n0 - 1 - (long long)(rng() % std::min<long long>(n0, 100000)) : run0 + t);
        std::sort(rem.begin(), rem.end());
        rem.erase(std::unique(rem.begin(), rem.end()), rem.end());
        const long long m = (long long)rem.size(), n1 = n0 - m;
        const long long cap = it % 5 == 0 ? 1 + (long long)(rng() % 8) : it % 5 == 1 ? compact_auto_rows(1 + (long long)(rng() % 16384)) : 1 + (long long)(rng() % kMax);
        const CompactPlan p = compact_plan(n0, m, rem[0], cap);
        const long long moved = p.end - p.first;
        CHECK(p.end == n1 && p.first == std::min(rem[0], n1) && p.chunk_rows >= 1 && p.chunk_rows <= cap, "n0=%lld m=%lld cap=%lld", n0, m, cap);
        CHECK(p.chunks >= 0 && (moved == 0) == (p.chunks == 0), "n0=%lld m=%lld cap=%lld chunks=%lld", n0, m, cap, p.chunks);
        if (p.chunks) {
            CHECK((p.chunks - 1) * p.chunk_rows < moved && moved <= p.chunks * p.chunk_rows, "n0=%lld m=%lld cap=%lld chunks=%lld x %lld for %lld rows", n0, m, cap, p.chunks, p.chunk_rows, moved);
            const long long pick[] = {0, p.chunks - 1, (long long)(rng() % (unsigned long long)p.chunks), p.chunks / 2};
            for (long long c : pick) {
                const CompactChunk k = compact_chunk(p, c), nx = compact_chunk(p, c + 1 < p.chunks ? c + 1 : c);
                CHECK(k.lo >= p.first && k.lo < k.hi && k.hi <= p.end && k.hi - k.lo <= p.chunk_rows, "n0=%lld cap=%lld chunk %lld = [%lld, %lld)", n0, cap, c, k.lo, k.hi);
                CHECK(c + 1 == p.chunks ? k.hi == p.end : nx.lo == k.hi, "n0=%lld cap=%lld chunk %lld ends at %lld", n0, cap, c, k.hi);
                CHECK(c != 0 || k.lo == p.first, "n0=%lld cap=%lld: the first chunk starts at %lld", n0, cap, k.lo);
                const long long js[] = {k.lo, k.hi - 1, k.lo + (long long)(rng() % (unsigned long long)(k.hi - k.lo))};
                for (long long j : js) {
                    const long long s = compact_src(j, rem.data(), m);
                    long long below = 0;   // the definition: s is the j-th row (from 0) that stays
                    for (long long r : rem) below += r < s;
                    CHECK(s >= j && s >= k.lo && s < n0 && s - below == j && !std::binary_search(rem.begin(), rem.end(), s), "n0=%lld j=%lld src=%lld", n0, j, s);
                }
            }
            CHECK(compact_src(p.end - 1, rem.data(), m) < n0, "n0=%lld: the last row's source", n0);
        }
    }
    std::printf("compact plan, large: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

static int units() {
    const long long rbs[] = {1, 2, 4, 100, 101, 200, 202, 400, 768, 1536, 3072, 5120, 16384, 16385, 1 << 20};
    for (long long rb : rbs) for (unsigned long long sa = 0; sa < 32; ++sa) for (unsigned long long da = 0; da < 32; ++da) {
        ++cases;
        const int u = compact_unit(0x10000 + sa, 0x20000 + da, rb);
        CHECK((u == 16 || u == 8 || u == 4 || u == 2 || u == 1) && rb % u == 0 && sa % u == 0 && da % u == 0, "rb=%lld sa=%llu da=%llu unit=%d", rb, sa, da, u);
        const int wider = u * 2;
        CHECK(u == 16 || rb % wider || sa % wider || da % wider, "rb=%lld sa=%llu da=%llu: unit %d where %d would do", rb, sa, da, u, wider);
        const int rpb = compact_rows_per_block(rb);
        CHECK(rpb >= 1 && rpb <= 256 && (rpb == 1 || rpb * rb <= 16384), "rb=%lld rows per block %d", rb, rpb);
    }
    CHECK(compact_unit(0x10000, 0x20000, 1536) == 16 && compact_unit(0x10000, 0x20000, 100) == 4 && compact_unit(0x10000, 0x20000, 101) == 1 &&
          compact_unit(0x10000, 0x20000, 200) == 8, "the widths of the issue's row sizes");
    std::printf("compact plan, units: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "small")) return small();
    if (argc == 2 && !std::strcmp(argv[1], "large")) return large();
    if (argc == 2 && !std::strcmp(argv[1], "units")) return units();
    std::printf("usage: %s small|large|units\n", argv[0]);
    return 2;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "compact_plan.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "compact_plan")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def run(exe: str, what: str):
    return subprocess.run([exe, what], capture_output=True, text=True, timeout=600, env=_ENV)
