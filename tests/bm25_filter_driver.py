"""A host-compiled driver of the filtered BM25 search's word arithmetic (veritasfi_amd/csrc/vf_bm25_filter.h), used by
tests/test_bm25_filter_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone and takes
no input.  It EXECUTES a filtered call the way the entry point and the kernels do, with the header's own functions -- the bitmap
check and the popcount m, the launch plan, the device bitmap zero-padded to whole blocks, the scatter that skips a row outside the
set (bm25f_row_allowed), the sort's ranks, the padding written first, then the tail per bitmap block (count, exclusive scan over
the blocks, write: bm25f_valid_mask and bm25f_allowed_untouched word by word, the per-block cut-offs of k_bm25_tail_write) -- and
holds the outcome to the plain definition: the allowed rows sorted by (touched first, score descending, row ascending), cut to k,
then (-1, -FLT_MAX).  Every rank must have exactly one writer.

  exhaustive  every n <= 12, every filter, every touched set, k in {1, 2, n}
  random      n in {31, 32, 33, 63, 64, 65, 32767, 32768, 32769, 65537} (word and block boundaries on the edges), seeded filters and
              touched sets of several densities, k in {1, 2, 100, 4096, 4097, n}
  check       the bitmap check names the FIRST bit at or past n, whatever else is set, and counts the rows below n

The select, gather and sort kernels are not modelled (a filtered call runs them unchanged): the model sorts the touched bitmap's
rows.  In the exhaustive part the tail walks the words that hold rows and one word past them instead of all 1024 of the block (the
rest are the same all-zero words); the random part walks every word of every block.

It prints the number of cases per part and the first failures, and returns 1 if there was one."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

DRIVER = r"""
#include <cfloat>
#include <cstdio>
#include <cstdint>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>
#include "vf_bm25_filter.h"
using namespace vf;

static std::atomic<long long> failures{0};
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

static const long long kUnwritten = -7;
static float score_of(long long r) { return (float)((r * 7 + 3) % 5 + 1) * 0.5f; }   // ties on purpose: the lower row wins them

struct Case {
    long long n, k;
    std::vector<uint32_t> allow;      // the caller's bitmap: bm25f_words(n) words
    std::vector<uint32_t> postings;   // bitmap of the rows the query has a posting for, filter or not
    long long walk_words;             // words of a block the tail walks (0 = all)
};

static thread_local std::vector<uint32_t> d_allow, bits;   // reused across cases: the device bitmap and the touched bitmap, zero between cases
static thread_local std::vector<long long> out_ids, sel, tblk;
static thread_local std::vector<float> out_scores;

static void run(const Case& c, const char* tag) {
    const long long n = c.n, k = c.k, cw = bm25f_words(n);
    const long long words = (cw + kBm25FilterBlockWords - 1) / kBm25FilterBlockWords * kBm25FilterBlockWords;   // the handle's `words`
    // the entry point: check, popcount, plan
    const Bm25FilterCheck fc = bm25f_check(c.allow.data(), n);
    CHECK(fc.bad_row == -1, "%s: a good bitmap was refused at row %lld", tag, fc.bad_row);
    long long m_plain = 0;
    for (long long r = 0; r < n; ++r) m_plain += (c.allow[r >> 5] >> (r & 31)) & 1u;
    CHECK(fc.m == m_plain, "%s: m = %lld, %lld rows are allowed", tag, fc.m, m_plain);
    const Bm25FilterPlan p = bm25f_plan(words, fc.m, k);
    CHECK(p.tail_blocks * (long long)kBm25FilterBlockWords == words && p.tblk_entries == p.tail_blocks, "%s: %d tail blocks over %lld words", tag, p.tail_blocks, words);
    CHECK(p.pad_from == std::min(k, fc.m), "%s: padding from %lld", tag, p.pad_from);
    if ((long long)d_allow.size() < words) { d_allow.assign((size_t)words, 0u); bits.assign((size_t)words, 0u); }
    for (long long w = 0; w < cw; ++w) d_allow[w] = c.allow[w];   // the upload: the words past the caller's stay zero
    // k_bm25_accum_f: a posting whose row is out is neither scored nor marked
    sel.clear();
    for (long long w = 0; w < cw; ++w)
        for (uint32_t b = c.postings[w]; b; b &= b - 1) {
            const uint32_t row = (uint32_t)(w * 32 + __builtin_ctz(b));
            if (!bm25f_row_allowed(d_allow.data(), row)) continue;
            bits[row >> 5] |= 1u << (row & 31u);
        }
    // the select, the gather and the sort, unchanged: min(k, touched) rows of the touched bitmap, score descending, ties to the lower row
    for (long long w = 0; w < cw; ++w)
        for (uint32_t b = bits[w]; b; b &= b - 1) sel.push_back(w * 32 + __builtin_ctz(b));
    std::sort(sel.begin(), sel.end(), [](long long x, long long y) { return score_of(x) != score_of(y) ? score_of(x) > score_of(y) : x < y; });
    const long long nsel = std::min<long long>(k, (long long)sel.size());
    out_ids.assign((size_t)k, kUnwritten);
    out_scores.assign((size_t)k, 0.0f);
    // k_bm25_pad_out, before the sort and the tail write
    for (long long i = p.pad_from; i < k; ++i) { out_ids[i] = -1; out_scores[i] = -FLT_MAX; }
    for (long long i = 0; i < nsel; ++i) {
        CHECK(out_ids[i] == kUnwritten, "%s: the sort writes rank %lld over the padding", tag, i);
        out_ids[i] = sel[i]; out_scores[i] = score_of(sel[i]);
    }
    // k_bm25_tail_count_f, k_bm25_tail_scan, k_bm25_tail_write_f over plan.tail_blocks blocks
    if (nsel < k) {
        const long long walk = c.walk_words ? std::min<long long>(c.walk_words, kBm25FilterBlockWords) : kBm25FilterBlockWords;
        tblk.assign((size_t)p.tblk_entries, 0);
        for (int b = 0; b < p.tail_blocks; ++b)
            for (long long j = 0; j < walk; ++j) {
                const long long w = (long long)b * kBm25FilterBlockWords + j;
                tblk[b] += bm25f_popcount(bm25f_allowed_untouched(bits[w], bm25f_valid_mask(w * 32, n), d_allow[w]));
            }
        long long carry = 0;
        for (int b = 0; b < p.tail_blocks; ++b) { const long long v = tblk[b]; tblk[b] = carry; carry += v; }
        CHECK(nsel + carry == fc.m, "%s: %lld sorted + %lld tail rows, %lld allowed", tag, nsel, carry, fc.m);
        for (int b = 0; b < p.tail_blocks; ++b) {
            long long pos = nsel + tblk[b];
            if (pos >= k) continue;
            for (long long j = 0; j < walk; ++j) {
                const long long w = (long long)b * kBm25FilterBlockWords + j;
                for (uint32_t z = bm25f_allowed_untouched(bits[w], bm25f_valid_mask(w * 32, n), d_allow[w]); z && pos < k; z &= z - 1, ++pos) {
                    CHECK(out_ids[pos] == kUnwritten, "%s: the tail writes rank %lld, which holds %lld", tag, pos, out_ids[pos]);
                    out_ids[pos] = w * 32 + __builtin_ctz(z); out_scores[pos] = 0.0f;
                }
            }
        }
    }
    // the plain definition
    long long rank = 0, bad = -1;
    for (long long i = 0; i < nsel && bad < 0; ++i, ++rank)   // sel is already the plain sort of the allowed rows with a posting, if the scatter was right
        if (!((c.allow[sel[i] >> 5] >> (sel[i] & 31)) & 1u) || !((c.postings[sel[i] >> 5] >> (sel[i] & 31)) & 1u)) bad = rank;
    long long want_touched = 0;
    for (long long w = 0; w < cw; ++w) want_touched += bm25f_popcount(c.allow[w] & c.postings[w]);
    CHECK((long long)sel.size() == want_touched, "%s: %zu rows touched, %lld allowed rows have a posting", tag, sel.size(), want_touched);
    for (long long r = 0; r < n && rank < k && bad < 0; ++r) {
        if (!((c.allow[r >> 5] >> (r & 31)) & 1u) || ((c.postings[r >> 5] >> (r & 31)) & 1u)) continue;
        if (out_ids[rank] != r || out_scores[rank] != 0.0f) bad = rank;
        ++rank;
    }
    for (; rank < k && bad < 0; ++rank)
        if (out_ids[rank] != -1 || out_scores[rank] != -FLT_MAX) bad = rank;
    CHECK(bad < 0, "%s: rank %lld holds row %lld", tag, bad, out_ids[bad]);
    // k_bm25_reset: the touched bitmap back to zero for the next case
    for (long long w = 0; w < cw; ++w) bits[w] = 0u;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static std::vector<uint32_t> random_bits(long long n, double density) {
    std::vector<uint32_t> v((size_t)bm25f_words(n), 0u);
    for (long long r = 0; r < n; ++r)
        if ((double)(rng() >> 11) / 9007199254740992.0 < density) v[r >> 5] |= 1u << (r & 31);
    return v;
}

int main() {
    char tag[128];
    // every n <= 12, every filter, every touched set, k in {1, 2, n}: the filters dealt out to four threads
    std::atomic<long long> done{0};
    auto stripe = [&done](unsigned part, unsigned parts) {
        char tag[128];
        tag[0] = 0;
        long long mine = 0;
        for (long long n = 1; n <= 12; ++n) {
            const long long ks[3] = {1, 2, n};
            Case c;
            c.n = n; c.allow.assign(1, 0u); c.postings.assign(1, 0u); c.walk_words = 2;
            for (uint32_t f = part; f < (1u << n); f += parts)
                for (uint32_t t = 0; t < (1u << n); ++t)
                    for (int ki = 0; ki < 3; ++ki) {
                        if (ks[ki] > n || (ki == 2 && n <= 2)) continue;
                        c.k = ks[ki]; c.allow[0] = f; c.postings[0] = t;
                        if (failures < 20) std::snprintf(tag, sizeof tag, "n=%lld filter=%x touched=%x k=%lld", n, f, t, c.k);
                        run(c, tag);
                        ++mine;
                    }
        }
        done += mine;
    };
    {
        std::vector<std::thread> pool;
        for (unsigned i = 0; i < 4; ++i) pool.emplace_back(stripe, i, 4u);
        for (std::thread& t : pool) t.join();
    }
    long long cases = done;
    std::printf("exhaustive: %lld cases\n", cases);
    // word and block boundaries
    cases = 0;
    const long long ns[] = {31, 32, 33, 63, 64, 65, 32767, 32768, 32769, 65537};
    const double fdens[] = {0.5, 0.01, 1.0, 0.0003}, tdens[] = {0.0, 0.002, 0.3, 1.0};
    for (long long n : ns)
        for (double fd : fdens)
            for (double td : tdens) {
                Case c;
                c.n = n; c.walk_words = 0;
                c.allow = random_bits(n, fd);
                c.postings = random_bits(n, td);
                if (fd == 0.0003) {   // ... and the last row alone next to a few: the last word's last valid bit
                    c.allow[(n - 1) >> 5] |= 1u << ((n - 1) & 31);
                }
                const long long ks[] = {1, 2, 100, 4096, 4097, n};
                for (long long k : ks) {
                    if (k > n) continue;
                    c.k = k;
                    std::snprintf(tag, sizeof tag, "n=%lld filter density %g touched density %g k=%lld", n, fd, td, k);
                    run(c, tag);
                    ++cases;
                }
            }
    std::printf("random: %lld cases\n", cases);
    // the bitmap check: the first bit at or past n
    cases = 0;
    for (long long n : {1ll, 5ll, 31ll, 33ll, 63ll, 70001ll}) {
        const long long cw = bm25f_words(n), last0 = (cw - 1) * 32;
        for (long long first = n; first < cw * 32; ++first)
            for (int more = 0; more < 2; ++more) {
                std::vector<uint32_t> v = random_bits(n, 0.5);
                long long m = 0;
                for (long long w = 0; w < cw; ++w) m += bm25f_popcount(v[w]);
                v[first >> 5] |= 1u << (first & 31);
                if (more) v[cw - 1] |= ~0u << (first & 31);   // every later bit of the last word as well
                const Bm25FilterCheck fc = bm25f_check(v.data(), n);
                CHECK(fc.bad_row == first && first >= last0, "n=%lld: bit %lld set, the check names %lld", n, first, fc.bad_row);
                CHECK(fc.m == m, "n=%lld: m = %lld with a bit past the end, %lld rows are allowed", n, fc.m, m);
                ++cases;
            }
        CHECK(bm25f_valid_mask(last0, n) == (n - last0 >= 32 ? 0xFFFFFFFFu : (1u << (n - last0)) - 1u) && bm25f_valid_mask(cw * 32, n) == 0u, "n=%lld: the last word's mask", n);
    }
    std::printf("check: %lld cases\n", cases);
    std::printf("bm25 filter plan: %lld failure(s)\n", failures.load());
    return failures ? 1 : 0;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def expected_exhaustive_cases() -> int:
    return sum(4 ** n * len({k for k in (1, 2, n) if k <= n}) for n in range(1, 13))


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "bm25_filter_plan.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "bm25_filter_plan")
    subprocess.check_call([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-pthread", "-I", CSRC, src, "-o", exe])
    return exe


def run(exe: str):
    return subprocess.run([exe], capture_output=True, text=True, timeout=600, env=_ENV)
