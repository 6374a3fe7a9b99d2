"""The option table (veritasfi_amd/csrc/vf_options.h) as the tests expect it, and a host-compiled driver of it, shared by
tests/test_options.py (no GPU: every row through option_set) and tests/test_gpu_set_option.py (the same rows through a live handle).

`rows()` is the expectation: one entry per integer option with its default, values at the edges of what it accepts, values just past
them and in its holes, and the refusal message -- a literal copy of the text vf_index_set_option's if / else chain held before the table
replaced it.  The driver (UBSan, stand-alone like tests/scan_route_driver.py) reads "name value" lines and prints what option_set made of
each, starting from a default-constructed RouteIn every time:

  driver defaults   one line per option: name, Options' default, a default-constructed RouteIn's
  driver set        per line of stdin: "<result> <the option's value afterwards>|<message>" (result 0 stored, 1 unknown, 2 refused)"""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
STORED, UNKNOWN, REFUSED = 0, 1, 2
UNKNOWN_MESSAGE = "vf_index_set_option: unknown option %s"

_WIDE8_WAVES = "wide8_waves must be 8 (the 4-wave form was measured slower and is built with -DVF_EXPERIMENTS only: DESIGN.md 4)"
_WIDE8_WAVES_X = ("wide8_waves must be 8 (one 512-thread workgroup per CU, 256-query tiles: the default) or 4 (two 256-thread workgroups, "
                  "128-query tiles: measured slower, DESIGN.md 4)")
_WIDE_ROWS = ("wide_rows must be 0 (rows of more than 2432 padded elements never take the fused path), 1 (auto: from 131072 rows, e4m3 rows "
              "from 32768, int8 rows from 32768) or 2 (wherever k_scan_ksplit / k_scan_ksplit8 serve them; int8 rows: from 32768 rows)")


def rows(experiments: bool = False):
    """(name, default, accepted edge values, refused values: one past each edge and the holes, message).  experiments: a -DVF_EXPERIMENTS build."""
    return [
        ("force_path", -1, [-1, 2], [-2, 3], "force_path must be -1 (auto), 0, 1 or 2"),
        ("sample_rows", -1, [-1, 1, 64], [-2, 65, 0], "sample_rows must be -1 (auto) or in [1, 64]"),
        ("margin", -1, [-1, 2048], [-2, 2049], "margin must be -1 (auto) or in [0, 2048]"),
        ("cap", 0, [0, 16384], [-1, 16385], "cap must be in [0, 16384]"),
        ("waves", 0, [0, 8192], [-1, 8193], "waves must be in [0, 8192]"),
        ("scan_g", 0, [0, 4], [-1, 5], "scan_g must be in [0, 4]"),
        ("refresh_every", 128, [1, 256], [0, 257], "refresh_every must be in [1, 256]"),
        ("steal", 0, [0, 1], [-1, 2], "steal must be 0 or 1"),
        ("wide", 1, [0, 4096], [-1, 4097], "wide must be 0 (off), 1 (auto) or a query count"),
        ("wide8_stage", 0, [0, 64, 3584], [-1, 3585, 1, 63], "wide8_stage must be 0 (auto) or 64..3584 candidate-stage entries"),
        ("wide8_waves", 8, [4, 8], [3, 9, 5, 6, 7], _WIDE8_WAVES_X) if experiments else ("wide8_waves", 8, [8], [7, 9, 4], _WIDE8_WAVES),
        ("wide_mfma", -1, [-1, 1], [-2, 2], "wide_mfma must be -1 (auto: the fp8 instruction for e4m3 rows), 0 (fp16 matrix instruction on "
         "converted rows) or 1 (the fp8 instruction on the e4m3 row bytes: k_scan_wide8)"),
        ("wide_sync", -1, [-1, 8], [-2, 9], "wide_sync must be -1 (off) or a slack of 0..8 super-tiles"),
        ("aux_cus", -1, [-1, 128], [-2, 129], "aux_cus must be -1 (auto) or in [0, 128]"),
        ("sample_grid", -1, [-1, 1024], [-2, 1025], "sample_grid must be -1 (auto), 0 (one workgroup per range) or a workgroup count"),
        ("scan_impl", 2, [1, 5], [0, 6], "scan_impl must be 1 (k_scan), 2 (auto: k_scan2 for fp16 rows, k_scan2r where it measured faster), "
         "3 (k_scan2 wherever it fits, e4m3 rows converted), 4 (k_scan2 for fp16 rows, never k_scan2r) or 5 (k_scan2r wherever a shape of it "
         "exists: fp16 rows of 384 / 512 / 768 / 1024 elements, e4m3 rows of 768 / 1024)"),
        ("sample_impl", -1, [-1, 1], [-2, 2], "sample_impl must be -1 (auto: k_scan2r's operand path for the sample pass where it exists and "
         "the CU split is on), 0 (k_scan) or 1 (k_scan2r wherever it fits)"),
        ("overlap_scans", -1, [-1, 1], [-2, 2], "overlap_scans must be -1 (auto), 0 or 1"),
        ("scan_image", 1, [0, 2], [-1, 3], "scan_image must be 0 (off), 1 (auto: when it fits with headroom) or 2 (force)"),
        ("image_mfma", -1, [-1, 2], [-2, 3], "image_mfma must be -1 (auto), 0 (the int8 row image on the fp16 matrix instruction, fp16 "
         "queries), 1 (on the int8 matrix instruction, the queries as one int8 plane) or 2 (as two planes, hi + lo: the band of 0)"),
        ("wide_rows", 1, [0, 2], [-1, 3], _WIDE_ROWS),
        ("compact_chunk_rows", 0, [0, 0xFFFFFFFF], [-1, 0x100000000], "compact_chunk_rows must be 0 (auto: 64 MB of staging) or the "
         "destination rows a removal moves per chunk"),
        ("subset_super_rows", 0, [0, 0xFFFFFFFE], [-1, 0xFFFFFFFF], "subset_super_rows must be 0 (auto: 64 MB of scores) or the listed rows "
         "a subset search scores per launch"),
        ("debug", 0, [I64_MIN, I64_MAX], [], ""),   # unchecked
    ]


def library_is_test_build() -> bool:
    """The loaded library is the -DVF_EXPERIMENTS build (it exports the test hooks): its wide8_waves row is the other one."""
    from veritasfi_amd import _ffi
    return hasattr(_ffi.lib(), "vf_debug_gemm")


DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "vf_route.h"
using namespace vf;

static int64_t value_of(const Options& o, const char* name) {
#define X(opt, ...) if (!std::strcmp(name, #opt)) return o.opt;
    VF_OPTIONS(X)
#undef X
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "defaults")) {
        const Options o; const RouteIn in;
#define X(opt, ...) std::printf("%s %" PRId64 " %" PRId64 "\n", #opt, o.opt, in.opt);
        VF_OPTIONS(X)
#undef X
        return 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "set")) {
        char name[256]; long long value;
        while (std::scanf("%255s %lld", name, &value) == 2) {
            RouteIn in;
            std::string msg;
            const OptionResult r = option_set(in, name, value, &msg);
            std::printf("%d %" PRId64 "|%s\n", (int)r, value_of(in, name), msg.c_str());
        }
        return 0;
    }
    std::printf("usage: %s defaults|set\n", argv[0]);
    return 2;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir, experiments: bool = False) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    stem = os.path.join(str(tmp_dir), "option_table_x" if experiments else "option_table")
    with open(stem + ".cc", "w") as f:
        f.write(DRIVER)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"] +
                          (["-DVF_EXPERIMENTS"] if experiments else []) + ["-I", CSRC, stem + ".cc", "-o", stem])
    return stem


def _run(exe, mode, text=""):
    run = subprocess.run([exe, mode], input=text, capture_output=True, text=True, timeout=120, env=_ENV)
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    return run.stdout.split("\n")[:-1]


def defaults(exe) -> list:
    """[(name, Options' default, RouteIn's default)] in the table's order."""
    return [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in _run(exe, "defaults")]


def set_each(exe, pairs) -> list:
    """pairs: (name, value).  Returns (result, the option's value afterwards, message) for each, set on fresh defaults."""
    out = []
    lines = _run(exe, "set", "".join(f"{n} {v}\n" for n, v in pairs))
    assert len(lines) == len(pairs), lines[-5:]
    for ln in lines:
        head, msg = ln.split("|", 1)
        out.append((int(head.split()[0]), int(head.split()[1]), msg))
    return out
