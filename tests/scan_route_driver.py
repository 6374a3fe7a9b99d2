"""A host-compiled driver of the scan route (veritasfi_amd/csrc/vf_route.h + vf_options.h + vf_scan_lds.h), shared by tests/test_scan_route.py (no GPU)
and tests/test_gpu_scan_route.py (the library's reported values against the driver's prediction).

The headers are plain C++17 without HIP, so the host compiler reads them as they stand (the way tests/test_wide_rows_geometry.py
compiles its header), under UBSan.  The program is stand-alone:

  driver eval    reads one search per line of stdin ("key=value key=value ..."), prints its route as one line of "key=value"
  driver sweep   walks the option grid and holds every route to the invariants; prints the count and the failures

A search is routed the way vf_api.hip does it: the path first (no slot yet), then the CU split as ensure_slot applies it (masking = 1:
the stack masks streams; aux_applied = N: what a live handle reports instead), then the search and each of its passes."""
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
#include "vf_route.h"
using namespace vf;

struct Case {
    RouteIn in;
    int nq = 1, k = 100;
    bool masking = true;          // the stack can CU-mask a stream
    long long aux_applied = -1;   // >= 0: the split a live handle reports (masked iff > 0)
};
struct Routed {
    SearchRoute r; SplitReport split{0, 0};
    int passes = 0, wide_launches = 0, wide_queries = 0, scan_kernel = 0;
    BatchRoute first{}, last{};   // passes of a search that is not wide
    WidePass wfirst{}, wlast{};
};

static Routed route(Case c) {
    Routed o;
    RouteIn& in = c.in;
    in.aux_applied = -1; in.masked = false;
    const int path = route_path(in, c.k);   // before the slot's streams exist
    if (path < 0) { o.r.path = -1; return o; }
    if (c.aux_applied >= 0) { in.aux_applied = c.aux_applied; in.masked = c.aux_applied > 0; }
    else { const long long a = c.masking ? route_aux_cus(in) : 0; in.aux_applied = a; in.masked = a > 0; }   // ensure_slot
    o.r = route_search(in, c.nq, c.k);
    o.split = route_split_report(in, o.r.path);
    if (o.r.path != 1 || c.nq <= 0 || c.k <= 0) return o;
    for (int b0 = 0; b0 < c.nq; b0 += o.r.per_pass) {
        const int nb = std::min(o.r.per_pass, c.nq - b0);
        // (a pass's route depends on its query count only: the first and the last pass stand for all)
        if (b0 != 0 && b0 + o.r.per_pass < c.nq) { ++o.passes; if (o.r.wide) { ++o.wide_launches; o.wide_queries += nb; } continue; }
        ++o.passes;
        if (o.r.wide) { o.wlast = route_wide_pass(in, o.r.plan, nb); if (b0 == 0) o.wfirst = o.wlast; ++o.wide_launches; o.wide_queries += nb; o.scan_kernel = o.wlast.main; }
        else { o.last = route_batch(in, o.r, nb); if (b0 == 0) o.first = o.last; o.scan_kernel = o.last.main; }
    }
    return o;
}

static int dp_of(int d) { return (d + 127) / 128 * 128; }

static int eval_lines() {
    char line[4096];
    while (std::fgets(line, sizeof line, stdin)) {
        std::map<std::string, double> kv;
        for (char* tok = std::strtok(line, " \n"); tok; tok = std::strtok(nullptr, " \n")) {
            char* eq = std::strchr(tok, '=');
            if (!eq) { std::printf("error=bad-token\n"); return 2; }
            kv[std::string(tok, eq - tok)] = std::atof(eq + 1);
        }
        Case c;
        RouteIn& in = c.in;
        auto get = [&](const char* name, double dflt) { auto it = kv.find(name); if (it == kv.end()) return dflt; double v = it->second; kv.erase(it); return v; };
        in.n = (int64_t)get("n", 0); in.d = (int)get("d", 0); in.dp = dp_of(in.d); in.dtype = (int)get("dtype", VF_DTYPE_F16);
        in.n_cu = (int)get("n_cu", 256);
        in.has_scan = get("has_scan", in.n > kSmallN) != 0; in.has_image = get("has_image", 0) != 0; in.rho_mean = (float)get("rho_mean", 0.0);
        in.group = get("group", 0) != 0;
        c.nq = (int)get("nq", 1); c.k = (int)get("k", 100); c.masking = get("masking", 1) != 0; c.aux_applied = (long long)get("aux_applied", -1);
#define OPT(f, ...) in.f = (int64_t)get(#f, (double)in.f);   // every option of the table (vf_options.h), by its name
        VF_OPTIONS(OPT)
#undef OPT
        if (!kv.empty()) { std::printf("error=unknown-key:%s\n", kv.begin()->first.c_str()); return 2; }
        const Routed o = route(c);
        const bool fused = o.r.path == 1, narrow = fused && !o.r.wide && o.passes > 0;
        std::printf("path=%d wide=%d per_pass=%d passes=%d scan_image=%d planes=%d aux_cus=%d scans_overlap=%d scan_kernel=%d wide_launches=%d "
                    "wide_queries=%d tile=%d sample=%d sample_grid=%d sample_rows=%d main_rows=%d stage_cap=%d kprime=%d cap=%d grid=%d samp=%d total_waves=%d "
                    "refresh_every=%d clear_sample=%d scan_bytes=%lld\n",
                    o.r.path, (int)o.r.wide, o.r.per_pass, o.passes, fused && o.r.image ? 1 : 0, o.r.planes, o.split.aux_cus, o.split.scans_overlap,
                    o.scan_kernel, o.wide_launches, o.wide_queries, narrow ? o.first.tile : 0, narrow ? (int)o.first.sample : 0,
                    narrow ? o.first.sample_grid : 0, narrow ? (int)o.first.sample_rows : -1,
                    narrow ? (int)o.last.main_rows : (fused && o.passes ? (int)o.wlast.rows : -1), narrow ? o.last.stage_cap : (fused && o.passes ? o.wlast.stage_cap : 0),
                    fused ? o.r.plan.kprime : 0, fused ? (o.r.wide && o.passes ? o.wlast.cap : o.r.plan.cap) : 0, fused ? o.r.plan.grid : 0, fused ? o.r.plan.samp : 0, fused ? o.r.plan.total_waves : 0,
                    // the first pass's (the one a profiled search times)
                    narrow ? o.first.refresh_every : (fused && o.passes ? o.wfirst.refresh_every : 0),
                    narrow ? (int)o.first.clear_sample : (fused && o.passes ? (int)o.wfirst.clear_sample : 0),
                    narrow ? (long long)o.first.scan_bytes : (fused && o.passes ? (long long)o.wfirst.scan_bytes : 0ll));
    }
    return 0;
}

static long long failures = 0, checked = 0;
static Case cur; static int cur_k, cur_nq;
#define CHECK(c) do { if (!(c)) { if (failures < 20) std::printf("FAIL %s: dtype=%d n=%lld d=%d nq=%d k=%d scan_impl=%d sample_impl=%d wide_rows=%d scan_image=%d image=%d steal=%d force_path=%d\n", #c, \
    cur.in.dtype, (long long)cur.in.n, cur.in.d, cur_nq, cur_k, (int)cur.in.scan_impl, (int)cur.in.sample_impl, (int)cur.in.wide_rows, (int)cur.in.scan_image, (int)cur.in.has_image, (int)cur.in.steal, (int)cur.in.force_path); ++failures; } } while (0)

static void check_batch(const RouteIn& in, const BatchRoute& b) {
    CHECK(b.tile == 32 || b.tile == 64);
    CHECK(in.dp <= 2432 || b.tile == 32);
    CHECK(b.sample_grid >= 1);
    if (b.main == kKernelScan2 || b.main == kKernelScan2r || b.main == kKernelKsplit || b.main == kKernelKsplit8) CHECK(b.stage_cap >= 256);
    CHECK(b.main == kKernelScan || b.main == kKernelScan2 || b.main == kKernelScan2r || b.main == kKernelKsplit || b.main == kKernelKsplit8);
    CHECK(b.sample == kKernelScan || b.sample == kKernelScan2r || b.sample == kKernelKsplit || b.sample == kKernelKsplit8);
    if (b.main == kKernelScan2r) CHECK(scan2r_shape(in.dp, b.main_rows).S != 0);
    if (b.sample == kKernelScan2r) CHECK(scan2r_shape(in.dp, b.sample_rows).S != 0);
    if (b.main == kKernelScan2) CHECK(b.main_rows == kRowsF16 || b.main_rows == kRowsE4m3);
    if (b.main == kKernelKsplit8) CHECK(b.main_rows == kRowsE4m3 || b.main_rows == kRowsI8);
}

static int sweep() {
    const int dtypes[] = {VF_DTYPE_F32, VF_DTYPE_F16, VF_DTYPE_FP8_E4M3, VF_DTYPE_INT8};
    const int ds[] = {384, 512, 640, 768, 1024, 2432, 2560, 2688, 4096, 4097};
    const long long ns[] = {1024, 16384, 16385, 32767, 32768, 131071, 131072, 1100000, 1100001, 1500000, 4000000, 6000000, 6000001};
    const int nqs[] = {1, 32, 33, 64, 65, 128, 129, 1024, 1025};
    const int ks[] = {1, 128, 129, 2048, 2049};
    for (int dtype : dtypes) for (int d : ds) for (long long n : ns)
    for (int scan_impl = 1; scan_impl <= 5; ++scan_impl) for (int sample_impl = -1; sample_impl <= 1; ++sample_impl)
    for (int wide_rows = 0; wide_rows <= 2; ++wide_rows) for (int scan_image = 0; scan_image <= 2; ++scan_image) for (int image = 0; image < 2; ++image)
    for (int steal = 0; steal < 2; ++steal) for (int force_path = -1; force_path <= 1; force_path += 2) {
        Case c;
        RouteIn& in = c.in;
        in.n = n; in.d = d; in.dp = dp_of(d); in.dtype = dtype; in.has_scan = n > kSmallN;
        in.scan_impl = scan_impl; in.sample_impl = sample_impl; in.wide_rows = wide_rows; in.scan_image = scan_image; in.steal = steal;
        in.force_path = force_path;
        // an image exists only where build_image builds one: the option on and the shape eligible (the memory and residual tests aside)
        in.has_image = image && scan_image != 0 && image_eligible(in, scan_image);
        for (int nq : nqs) for (int k : ks) {
            c.nq = nq; c.k = k; cur = c; cur_k = k; cur_nq = nq;
            const Routed o = route(c);
            ++checked;
            CHECK(o.r.path >= -1 && o.r.path <= 2);
            CHECK(o.r.path != -1 || force_path == 1);
            if (o.r.path != 1) continue;
            CHECK(in.has_scan);
            CHECK(k <= kMaxKFused && n > 1024);
            CHECK(o.passes == (nq + o.r.per_pass - 1) / o.r.per_pass);
            CHECK(o.r.plan.kprime >= k && o.r.plan.kprime <= 4096 && o.r.plan.cap >= 2 * o.r.plan.kprime && o.r.plan.grid >= 1 && o.r.plan.grid <= in.n_cu);
            if (o.r.image) { CHECK(k <= 128 && in.dp == 768 && in.has_image && !o.r.wide); CHECK(o.r.planes >= 0 && o.r.planes <= 2); }
            else CHECK(o.r.planes == 0);
            if (o.r.wide) {
                CHECK(o.wlast.main == kKernelWide || o.wlast.main == kKernelWide8);
                CHECK(o.wlast.main != kKernelWide8 || dtype == VF_DTYPE_FP8_E4M3);
                CHECK(o.wlast.jtiles >= 1 && o.wlast.jtiles <= 4 && o.wlast.rgroups >= 1 && o.wlast.stage_cap >= 256);
                CHECK(scan_wide8_lds_bytes(o.wlast.waves, o.wlast.stage_cap) <= (size_t)kLdsBytes);
            } else {
                check_batch(in, o.first);
                check_batch(in, o.last);
                CHECK(!o.r.image || (o.last.main == kKernelScan2r && o.last.sample == kKernelScan2r && o.last.main_rows == image_rows(o.r.planes)));
            }
        }
    }
    std::printf("route sweep: %lld searches checked, %lld failure(s)\n", checked, failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "eval")) return eval_lines();
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    std::printf("usage: %s eval|sweep\n", argv[0]);
    return 2;
}
"""

DTYPES = {"f32": 0, "f16": 1, "e4m3": 2, "int8": 3}
_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "scan_route.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "scan_route")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def evaluate(exe: str, cases) -> list:
    """cases: dicts of the driver's keys (dtype by name or number).  Returns one dict of ints per case."""
    lines = []
    for c in cases:
        c = dict(c)
        if isinstance(c.get("dtype"), str):
            c["dtype"] = DTYPES[c["dtype"]]
        lines.append(" ".join(f"{k}={v}" for k, v in c.items()))
    run = subprocess.run([exe, "eval"], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120, env=_ENV)
    assert run.returncode == 0 and "runtime error" not in run.stderr, (run.stdout[-2000:], run.stderr[-2000:])
    out = [dict((kv.split("=")[0], int(kv.split("=")[1])) for kv in ln.split()) for ln in run.stdout.strip().split("\n")]
    assert len(out) == len(cases), run.stdout[-2000:]
    return out


def sweep(exe: str):
    return subprocess.run([exe, "sweep"], capture_output=True, text=True, timeout=900, env=_ENV)
