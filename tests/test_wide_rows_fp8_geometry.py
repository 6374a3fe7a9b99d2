"""k_scan_ksplit8's address geometry (the ks8_* functions of veritasfi_amd/csrc/vf_ksplit_geom.h and the range / tile / row functions it
shares with k_scan_ksplit), enumerated on the CPU under UBSan.

The kernel takes every address it forms from those `__host__ __device__` functions, so a host-compiled driver walks them: every padded
width 2560 .. 4096, row count, grid (option `waves` / 8), sample rows per wave (option `sample_rows`), both modes, every workgroup, tile
(plus the refill past the last tile), wave, segment, lane half and step.  Every 16 bytes read lie inside [0, n * dp); the four waves'
segments tile [0, dp / 128) with 5 .. P8 each; the 16-byte pieces of a row are disjoint and cover it; every query-image k-group is below
dp / 8 and used exactly once per row, and meets the bytes of the same element numbers; every reciprocal-norm index lies in [0, n + 64);
main plus sample parts cover every row exactly once; the LDS budget leaves >= 256 stage entries within 160 KB.  n = 21 845 with 2 048
ranges is the shape of round 6's memory fault (a range shorter than its sample part).  A byte address is row * dp + an offset inside
the row, so the offsets of every (wave, segment, lane half, load, step) are walked once per width, every row of every tile is held to
[0, n) and to the row's two ends at the narrowest and widest rows, and the full per-load walk at every width runs for the lowest and
the highest row each workgroup reads.  No GPU."""
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
    for (int dp = 2560; dp <= 4096; dp += 128) {   // ---- per width: segments, pieces, k-groups, LDS ----
        const int S8 = ks8_segs(dp), P8 = ks8_P(S8);
        const long long row_bytes = dp;
        long long n = 3, grid = 1, v = 0; int samp = 1, mode = 1, tile = 0;
        CHECK(ks_serves(dp) && S8 * 128 == dp);
        CHECK(P8 >= kKs8RegSegs && P8 <= kKs8MaxSegs);
        CHECK(ks8_seg_begin(S8, 0) == 0 && ks8_seg_begin(S8, kKsWaves) == S8);
        std::vector<unsigned char> piece((size_t)(row_bytes / 16), 0);
        std::vector<int> group((size_t)(dp / 8), 0);
        for (int w = 0; w < kKsWaves; ++w) {
            const int sbeg = ks8_seg_begin(S8, w), send = ks8_seg_begin(S8, w + 1);
            CHECK(send - sbeg >= kKs8RegSegs && send - sbeg <= P8 && send - sbeg >= P8 - 1);
            for (int j = 0; j < P8; ++j) {
                if (sbeg + j >= send) { CHECK(j == P8 - 1); continue; }   // the absent last segment: the kernel skips it
                for (int h = 0; h < 2; ++h) {
                    for (int i = 0; i < 4; ++i) {
                        const long long off = ks_src(2, row_bytes, sbeg + j, h, i) - 2 * row_bytes;
                        CHECK(off >= 0 && off + 16 <= row_bytes && off % 16 == 0);
                        CHECK(!piece[(size_t)(off / 16)]);
                        piece[(size_t)(off / 16)] = 1;
                    }
                    for (int i = 0; i < 8; ++i) {   // the 8 bytes step i converts are the elements of its k-group
                        const int g = ks8_group(sbeg + j, h, i);
                        CHECK(g >= 0 && g < dp / 8);
                        if (g >= 0 && g < dp / 8) ++group[(size_t)g];
                        CHECK(ks8_step_load(i) >= 0 && ks8_step_load(i) < 4 && (ks8_step_half(i) == 0 || ks8_step_half(i) == 1));
                        const long long byte0 = ks_src(0, row_bytes, sbeg + j, h, ks8_step_load(i)) + 8 * ks8_step_half(i);
                        CHECK(byte0 == 8ll * g);
                    }
                }
            }
        }
        for (unsigned char c : piece) CHECK(c);
        for (int c : group) CHECK(c == 1);
        // LDS: the image segments beyond the registers + the reduction area + control block + a stage of >= 256 entries fit 160 KB
        const int cap = ks8_stage_cap(dp);
        CHECK(cap >= 256 && cap <= 2048);
        CHECK(ks8_lds_bytes(dp, cap) <= 160 * 1024);
        CHECK(ks8_lds_bytes(dp, 0) == (long long)kKsWaves * (P8 - kKs8RegSegs) * kKs8SegBytes + kKsRedBytes + kKs8CtlBytes);
        CHECK((long long)kKsWaves * (P8 - kKs8RegSegs) * kKs8SegBytes <= 96 * 1024);
    }
    // ---- per (n, grid, sample rows, mode): every workgroup, tile and lane row; under each row every width, wave, segment, lane half, load ----
    for (long long n : ns) for (long long grid : grids) for (int samp : samps) for (int mode = 0; mode < 2; ++mode) {
        int dp = 0;
        const long long swg = (long long)samp * kKsSampWaves;
        const bool sample = mode == 0;
        std::vector<unsigned char> seen(sample ? 0 : (size_t)n, 0);
        for (long long v = 0; v < grid; ++v) {
            const KsPart p = ks_part(n, grid, v, swg, sample);
            int tile = -1;
            CHECK(p.lo >= 0 && p.lo <= p.hi && p.hi <= n);
            const int nt = ks_ntiles(p, swg, sample);
            CHECK(nt >= 0);
            if (nt == 0) continue;   // the kernel issues nothing
            for (tile = 0; tile < nt + 1; ++tile) {   // (+ 1: the refill past the last tile re-reads the last tile's rows)
                const int tt = tile < nt ? tile : nt - 1;
                const long long t0 = p.lo + (long long)tt * kKsRowTile;
                for (int r = 0; r < 32; ++r) {
                    dp = 0;
                    const long long row = ks_row(p, n, tt, r);
                    CHECK(row >= 0 && row < n);
                    if (t0 + r < p.hi) { CHECK(row == t0 + r); if (!sample && tile < nt) { CHECK(!seen[(size_t)row]); seen[(size_t)row] = 1; } }
                    const long long ii = ks_inv_index(t0, n, r);
                    CHECK(ii >= 0 && ii < n + 64);
                    if (t0 + r < p.hi) CHECK(ii == t0 + r);
                    // ks_src is row * row_bytes + (an offset the per-width walk above has placed inside the row).  Every load of every wave is
                    // walked at every width for the first lane row of a part's first tile and the last lane row of its refill (the lowest and
                    // the highest row the workgroup reads); for the rest the row's two ends at the narrowest and the widest rows (the byte
                    // offsets are linear in dp between them).
                    const bool walk = (r == 0 && tile == 0) || (r == 31 && tile == nt);
                    for (dp = 2560; dp <= 4096; dp += walk ? 128 : 4096 - 2560) {
                        const long long row_bytes = dp, total = n * row_bytes;
                        const int S8 = ks8_segs(dp);
                        CHECK(ks_src(row, row_bytes, 0, 0, 0) >= 0 && ks_src(row, row_bytes, S8 - 1, 1, 3) + 16 <= total);
                        ++checked;
                        if (!walk) continue;
                        for (int w = 0; w < kKsWaves; ++w)
                            for (int sg = ks8_seg_begin(S8, w); sg < ks8_seg_begin(S8, w + 1); ++sg)
                                for (int h = 0; h < 2; ++h) for (int i = 0; i < 4; ++i) {
                                    const long long b = ks_src(row, row_bytes, sg, h, i);
                                    CHECK(b >= 0 && b + 16 <= total);
                                    ++checked;
                                }
                    }
                }
                dp = 0;
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
    std::printf("geometry: %lld lane addresses checked, %lld failure(s)\n", checked, failures);
    return failures ? 1 : 0;
}
"""


def test_every_address_of_the_fp8_ksplit_scan_lies_inside_its_buffers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = tmp_path / "ks8_geom.cc"
    src.write_text(DRIVER)
    exe = str(tmp_path / "ks8_geom")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.dirname(HEADER), str(src), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                         env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    print(run.stdout[-3000:], run.stderr[-3000:])
    assert run.returncode == 0 and " 0 failure(s)" in run.stdout and "runtime error" not in run.stderr
