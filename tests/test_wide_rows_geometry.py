"""k_scan_ksplit's address geometry (veritasfi_amd/csrc/vf_ksplit_geom.h), enumerated on the CPU under UBSan.

The kernel takes every address it forms from the `__host__ __device__` functions of that header, so a host-compiled driver can
walk them: for every row count, grid (option `waves` / 8), sample rows per wave (option `sample_rows`), both modes, every
workgroup, tile, wave, lane and segment, every 16 bytes a load would read lie inside [0, n * row_bytes), every segment belongs to
exactly one wave, every reciprocal-norm index lies in [0, n + 64), and every sample slot that is written lies inside its range's
slots.  n = 21 845 with 2 048 ranges is the shape of round 6's memory fault (a range shorter than its sample part).  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "veritasfi_amd", "csrc", "vf_ksplit_geom.h")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vf_ksplit_geom.h"
using namespace vf;
static long long failures = 0, checked = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) std::printf("FAIL %s: n=%lld grid=%lld samp=%d dp=%d mode=%d v=%lld tile=%d\n", #c, n, grid, samp, dp, mode, v, tile); ++failures; } } while (0)
int main() {
    const long long ns[] = {1025, 16385, 17000, 20000, 21845, 32768, 40000, 65537, 262147};
    const long long grids[] = {1, 2, 7, 32, 78, 128, 256, 1024, 2048};
    const int samps[] = {1, 4, 8, 16, 64};
    const int dps[] = {2560, 2688, 2816, 2944, 3072, 3200, 3328, 3456, 3584, 3712, 3840, 3968, 4096};
    for (int dp : dps) {
        const int S = ks_segs(dp), P = ks_P(S);
        long long n = 0, grid = 0, v = 0; int samp = 0, mode = 0, tile = 0;
        CHECK(ks_serves(dp));
        CHECK(P >= kKsRegSegs && P <= 16 && P % ks_D(P) == 0);
        // the four waves' segments tile [0, S): contiguous, each wave holds 10 .. P of them
        CHECK(ks_seg_begin(S, 0) == 0 && ks_seg_begin(S, kKsWaves) == S);
        for (int w = 0; w < kKsWaves; ++w) {
            const int cnt = ks_seg_begin(S, w + 1) - ks_seg_begin(S, w);
            CHECK(cnt >= kKsRegSegs && cnt <= P && cnt >= P - 1);
        }
        // LDS: the image segments beyond the registers + the reduction area + a 256-entry stage fit 160 KB
        CHECK((long long)kKsWaves * (P - kKsRegSegs) * kKsSegBytes + kKsRedBytes + 272 + 256 * 16 <= 160 * 1024);
    }
    for (long long n : ns) for (long long grid : grids) for (int samp : samps) for (int mode = 0; mode < 2; ++mode) {
        const int dp = (n % 2) ? 2560 : 4096;   // the row geometry does not depend on dp beyond row_bytes; segments are checked per dp below
        const long long row_bytes = (long long)dp * 2, total = n * row_bytes, swg = (long long)samp * kKsSampWaves;
        const bool sample = mode == 0;
        std::vector<unsigned char> seen(sample ? 0 : (size_t)n, 0);
        for (long long v = 0; v < grid; ++v) {
            const KsPart p = ks_part(n, grid, v, swg, sample);
            int tile = -1;
            CHECK(p.lo >= 0 && p.lo <= p.hi && p.hi <= n);
            const int nt = ks_ntiles(p, swg, sample);
            CHECK(nt >= 0);
            for (tile = 0; tile < nt + 1; ++tile) {   // (+ 1: the refill past the last tile re-reads the last tile's rows)
                const int tt = tile < nt ? tile : (nt > 0 ? nt - 1 : 0);
                const long long t0 = p.lo + (long long)tt * kKsRowTile;
                for (int r = 0; r < 32; ++r) {
                    const long long row = ks_row(p, n, tt, r);
                    CHECK(row >= 0 && row < n);
                    if (t0 + r < p.hi) { CHECK(row == t0 + r); if (!sample && tile < nt) { CHECK(!seen[(size_t)row]); seen[(size_t)row] = 1; } }
                    const long long ii = ks_inv_index(t0, n, r);
                    CHECK(ii >= 0 && ii < n + 64);
                    if (t0 + r < p.hi) CHECK(ii == t0 + r);
                    // first and last 16 bytes any lane of any wave reads of this row (every segment is walked per dp below)
                    CHECK(ks_src(row, row_bytes, 0, 0, 0) >= 0 && ks_src(row, row_bytes, ks_segs(dp) - 1, 1, 3) + 16 <= total);
                    ++checked;
                }
                if (sample && tile < nt)   // slots written: blockIdx * swg + tile * 32 + r for rows below the part's end
                    for (int r = 0; r < 32; ++r) if (t0 + r < p.hi) CHECK((long long)tt * kKsRowTile + r < swg);
            }
        }
        if (!sample) {   // main parts + sample parts cover every row exactly once
            long long v = -1; int tile = -1;
            for (long long vv = 0; vv < grid; ++vv) {
                const KsPart s = ks_part(n, grid, vv, swg, true);
                for (long long r = s.lo; r < s.hi; ++r) { CHECK(!seen[(size_t)r]); seen[(size_t)r] = 1; }
            }
            for (long long r = 0; r < n; ++r) CHECK(seen[(size_t)r]);
        }
    }
    // every (dp, wave, segment of the wave, lane half, step): inside the row, 16-byte pieces disjoint and covering the row
    for (int dp : dps) {
        long long n = 3, grid = 1, v = 0; int samp = 1, mode = 1, tile = 0;
        const int S = ks_segs(dp), P = ks_P(S);
        const long long row_bytes = (long long)dp * 2;
        std::vector<unsigned char> piece((size_t)(row_bytes / 16), 0);
        for (int w = 0; w < kKsWaves; ++w) {
            const int sbeg = ks_seg_begin(S, w), send = ks_seg_begin(S, w + 1);
            for (int j = 0; j < P; ++j) {
                if (sbeg + j >= send) { CHECK(j == P - 1); continue; }   // the absent last segment: the kernel skips it
                for (int h = 0; h < 2; ++h) for (int i = 0; i < 4; ++i) {
                    const long long off = ks_src(2, row_bytes, sbeg + j, h, i) - 2 * row_bytes;
                    CHECK(off >= 0 && off + 16 <= row_bytes && off % 16 == 0);
                    CHECK(!piece[(size_t)(off / 16)]);
                    piece[(size_t)(off / 16)] = 1;
                    // the query image's 16 bytes of the same k-slots: group 8 (sbeg + j) + 4 h + i of dp / 8
                    CHECK(8 * (sbeg + j) + 4 * h + i < dp / 8);
                }
            }
        }
        for (unsigned char c : piece) CHECK(c);
    }
    std::printf("geometry: %lld lane addresses checked, %lld failure(s)\n", checked, failures);
    return failures ? 1 : 0;
}
"""


def test_every_address_of_the_ksplit_scan_lies_inside_its_buffers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = tmp_path / "ks_geom.cc"
    src.write_text(DRIVER)
    exe = str(tmp_path / "ks_geom")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.dirname(HEADER), str(src), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    print(run.stdout[-3000:], run.stderr[-3000:])
    assert run.returncode == 0 and " 0 failure(s)" in run.stdout and "runtime error" not in run.stderr
