"""A host-compiled driver of the BM25 call decoder and launch plan (veritasfi_amd/csrc/vf_bm25_call.h), used by
tests/test_bm25_call_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone and takes
no input.  It calls the header's two functions over a fixed crossing of arguments and prints one line per case; it judges nothing
itself -- what each line must say is written out in the test.

  D <flags> <null> <phase> <nq> -> <kind> <refusal> <nq> <subset>
      bm25c_decode: flags = the three bits of `nq` (1 VF_BM25_PREPARED, 2 VF_BM25_FILTER, 4 VF_BM25_SUBSTATS), every combination x the
      struct pointer null or not x phase -1 .. 5 x nq in {0, 1, 64}; a refused call prints kind -1; subset is never set by the decoder
  P <n> <k> <nq> <kind> <subset> <m> -> <no_launch> <small> <S> <scatter> <tail_f> <tail_blocks> <tblk_stride> <pad_from> <pad_out>
      bm25c_plan: n in {1, 31, 4096, 4097, 32768, 32769, 70001} with the handle's bitmap words x the k of {1, 2, 4096, 4097, n} that
      fit x nq in {1, slot_cap, slot_cap + 1} x every kind (a prepared search in both modes) x m in {0, 1, k - 1, k, n}

It ends with the number of cases of each part."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

SIZES = (1, 31, 4096, 4097, 32768, 32769, 70001)
PHASES = tuple(range(-1, 6))
NQS = (0, 1, 64)


def slot_cap(n: int) -> int:
    """The slots the driver gives a handle of n rows: 64, the most a handle has, and a small one at the largest size."""
    return 7 if n == 70001 else 64


def words(n: int) -> int:
    """Bitmap words per slot of a handle of n rows: whole blocks of 1024."""
    return ((n + 31) // 32 + 1023) // 1024 * 1024


def ks(n: int):
    return sorted({k for k in (1, 2, 4096, 4097, n) if k <= n})


def ms(n: int, k: int):
    return sorted({m for m in (0, 1, k - 1, k, n) if 0 <= m <= n})


DRIVER = r"""
#include <cstdio>
#include <set>
#include "vf_bm25_call.h"
using namespace vf;

int main() {
    long long cases = 0;
    for (int flags = 0; flags < 8; ++flags)
        for (int null_struct = 0; null_struct < 2; ++null_struct)
            for (int phase = -1; phase <= 5; ++phase)
                for (int nq : {0, 1, 64}) {
                    const int raw = nq | (flags & 1 ? kBm25cPrepared : 0) | (flags & 2 ? kBm25cFilter : 0) | (flags & 4 ? kBm25cSubstats : 0);
                    const Bm25Call c = bm25c_decode(raw, null_struct != 0, phase);
                    std::printf("D %d %d %d %d -> %d %d %d %d\n", flags, null_struct, phase, nq, c.refusal ? -1 : (int)c.kind, (int)c.refusal, c.refusal ? -1 : c.nq, (int)c.subset);
                    ++cases;
                }
    std::printf("decode: %lld cases\n", cases);
    cases = 0;
    for (long long n : {1ll, 31ll, 4096ll, 4097ll, 32768ll, 32769ll, 70001ll}) {
        const long long words = ((n + 31) / 32 + kBm25FilterBlockWords - 1) / kBm25FilterBlockWords * kBm25FilterBlockWords;
        const int slot_cap = n == 70001 ? 7 : 64;
        std::set<long long> ks;
        for (long long k : {1ll, 2ll, 4096ll, 4097ll, n})
            if (k <= n) ks.insert(k);
        for (long long k : ks)
            for (int nq : {1, slot_cap, slot_cap + 1})
                for (int kind = kBm25Plain; kind <= kBm25PrepSearch; ++kind)
                    for (int subset = 0; subset < (kind == kBm25PrepSearch ? 2 : 1); ++subset) {
                        std::set<long long> ms;
                        for (long long m : {0ll, 1ll, k - 1, k, n})
                            if (m >= 0 && m <= n) ms.insert(m);
                        for (long long m : ms) {
                            const Bm25Call c{(Bm25Kind)kind, kBm25Accepted, nq, subset != 0};
                            const Bm25LaunchPlan p = bm25c_plan(c, k, nq, slot_cap, words, m);
                            std::printf("P %lld %lld %d %d %d %lld -> %d %d %d %d %d %d %lld %lld %d\n", n, k, nq, kind, subset, m, (int)p.no_launch, (int)p.small, p.S,
                                        (int)p.scatter, (int)p.tail_f, p.tail_blocks, p.tblk_stride, p.pad_from, (int)p.pad_out);
                            ++cases;
                        }
                    }
    }
    std::printf("plan: %lld cases\n", cases);
    return 0;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "bm25_call_plan.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "bm25_call_plan")
    subprocess.check_call([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def run(exe: str):
    return subprocess.run([exe], capture_output=True, text=True, timeout=600, env=_ENV)
