"""A host-compiled driver of the subset search's plan (veritasfi_amd/csrc/vf_subset.h), used by tests/test_subset_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone:

  driver small   every n <= 12, every subset of the rows, every super-chunk and rank-chunk size 1 .. n, k in {1, 2, 3, n + 2}: the plan
                 is EXECUTED on integer arrays the way the library executes it on the device -- score a super-chunk into the chunk-major
                 workspace, rank every chunk from its row of that matrix into a part slot, add the chunk bases, fold the parts into
                 the running result, map positions to ids at the end -- with 2 .. 4 slots per merge so that several rounds happen,
                 and held to a plain sort of the listed rows
  driver large   seeded random cases of up to 2^32 - 2 rows: plan arithmetic only, no arrays (overflow, workspace, merge keys, LDS)
  driver lists   the list check: the first offending position of out-of-range, descending and duplicate entries

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
#include "vf_subset.h"
using namespace vf;

static long long failures = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

struct Hit { long long score, pos; };                       // higher score first, ties to the lower position
static bool better(const Hit& a, const Hit& b) { return a.score != b.score ? a.score > b.score : a.pos < b.pos; }
typedef std::vector<Hit> Part;                              // at most k hits, ranked (the padding of a short part is simply absent)

// what k_merge_topk does: the k best of the slots' hits; on equal scores the earlier slot, then the earlier rank
static Part merge(const std::vector<Part>& slots, int k) {
    struct Key { long long score; size_t slot, rank; };
    std::vector<Key> keys;
    for (size_t s = 0; s < slots.size(); ++s) for (size_t r = 0; r < slots[s].size(); ++r) keys.push_back({slots[s][r].score, s, r});
    std::stable_sort(keys.begin(), keys.end(), [](const Key& a, const Key& b) { return a.score != b.score ? a.score > b.score : (a.slot != b.slot ? a.slot < b.slot : a.rank < b.rank); });
    Part out;
    for (size_t i = 0; i < keys.size() && (int)i < k; ++i) out.push_back(slots[keys[i].slot][keys[i].rank]);
    return out;
}

static int small() {
    for (int n = 0; n <= 12; ++n)
    for (unsigned mask = 0; mask < (1u << n); ++mask) {
        std::vector<long long> sel, score(n);
        for (int i = 0; i < n; ++i) { score[i] = (i * 7 + 3) % 5; if (mask >> i & 1) sel.push_back(i); }   // many equal scores
        const long long m = (long long)sel.size();
        const int ks[] = {1, 2, 3, n + 2};
        for (long long sup = 1; sup <= std::max(n, 1); ++sup)
        for (long long rank = 1; rank <= std::max(n, 1); ++rank)
        for (int k : ks) {
            ++cases;
            SubsetPlan p = subset_plan(n, m, 3, k, sup, rank);
            if (m == 0) { CHECK(p.route == kSubsetEmpty, "n=%d mask=%u", n, mask); continue; }
            if (m == n) { CHECK(p.route == kSubsetAll, "n=%d mask=%u", n, mask); continue; }
            CHECK(p.route == kSubsetScan, "n=%d mask=%u sup=%lld rank=%lld k=%d route=%d", n, mask, sup, rank, k, p.route);
            if (p.route != kSubsetScan) return 1;
            CHECK(p.rank_rows == rank && p.super_rows >= 1 && p.super_rows <= m && (p.super_rows % rank == 0 || p.super_rows == m) && p.super_rows <= (sup + rank - 1) / rank * rank &&
                  p.super_parts == (p.super_rows + rank - 1) / rank, "n=%d mask=%u sup=%lld rank=%lld: super_rows=%lld rank_rows=%lld super_parts=%lld", n, mask, sup, rank, p.super_rows, p.rank_rows, p.super_parts);
            const bool merging = p.parts > 1;
            long long want_rounds = 0;
            if (merging) p.fan_in = (int)std::min<long long>(p.super_parts + 1, 2 + (long long)((mask + k) % 3));   // few slots per merge: several rounds
            const int nq = 3, q = (int)(mask % 3);                               // the plan was made for three queries: this is one of them
            std::vector<Part> buf(merging ? p.super_parts + 1 : 1);             // slot 0: the running result (empty = all padding)
            std::vector<char> scored(m, 0);
            long long prev_hi = 0, parts = 0, rounds = 0;
            for (long long c = 0; c < p.supers; ++c) {
                const SubsetSpan s = subset_super(p, m, c);
                // the super-chunks tile the list, each fits the score workspace
                CHECK(s.lo == prev_hi && s.hi > s.lo && s.hi <= m && s.hi - s.lo <= p.super_rows, "n=%d mask=%u super %lld = [%lld, %lld)", n, mask, c, s.lo, s.hi);
                std::vector<long long> ws(p.score_bytes / 4, -99);
                for (long long i = s.lo; i < s.hi; ++i) {                        // what the kernel writes, where it writes it
                    const long long at = subset_score_index(i - s.lo, q, nq, p.rank_rows);
                    CHECK(at >= 0 && at < (long long)ws.size() && ws[at] == -99, "n=%d mask=%u: position %lld lands at %lld of %zu", n, mask, i, at, ws.size());
                    if (at < 0 || at >= (long long)ws.size()) return 1;
                    ws[at] = score[sel[i]]; scored[i] = 1;
                }
                long long prev = s.lo;
                const long long chunks = subset_rank_chunks(p, s);
                CHECK(chunks <= p.super_parts, "n=%d mask=%u: %lld chunks in a buffer of %lld part slots", n, mask, chunks, p.super_parts);
                for (long long r = 0; r < chunks; ++r) {
                    const SubsetSpan ch = subset_rank_chunk(p, s, r);
                    CHECK(ch.lo == prev && ch.hi > ch.lo && ch.hi <= s.hi && ch.hi - ch.lo <= p.rank_rows && (ch.hi - ch.lo == p.rank_rows || r == chunks - 1),
                          "n=%d mask=%u chunk %lld of super %lld = [%lld, %lld)", n, mask, r, c, ch.lo, ch.hi);
                    // the ranking launch: "query" r * nq + q reads one row of the [chunks * nq][rank_rows] matrix and ranks positions INSIDE the chunk ...
                    Part part;
                    for (long long t = 0; t < ch.hi - ch.lo; ++t) part.push_back({ws[(r * nq + q) * p.rank_rows + t], t});
                    std::sort(part.begin(), part.end(), better);
                    if ((int)part.size() > k) part.resize(k);
                    for (Hit& h : part) h.pos += s.lo + r * p.rank_rows;         // ... and the base is added afterwards
                    buf[merging ? 1 + r : 0] = part;
                    ++parts;
                    prev = ch.hi;
                }
                CHECK(prev == s.hi, "n=%d mask=%u: the chunks of super %lld end at %lld", n, mask, c, prev);
                prev_hi = s.hi;
                if (!merging) continue;
                want_rounds += subset_rounds(chunks, p.fan_in);
                long long first = 0;
                for (long long done = 0; done < chunks;) {                      // the fold, as the library runs it
                    const long long take = std::min<long long>(p.fan_in - 1, chunks - done);
                    const std::vector<Part> in(buf.begin() + first, buf.begin() + first + take + 1);
                    const Part f = merge(in, k);
                    ++rounds; first += take; done += take;
                    CHECK(first < (long long)buf.size(), "n=%d mask=%u: the running result moves to slot %lld of %zu", n, mask, first, buf.size());
                    buf[done < chunks ? first : 0] = f;
                    if (done >= chunks) first = 0;
                }
            }
            std::vector<Part> slots(1, buf[0]);
            CHECK(prev_hi == m && parts == p.parts && rounds == want_rounds && (merging ? rounds >= 1 : rounds == 0), "n=%d mask=%u sup=%lld rank=%lld k=%d: end %lld, %lld parts (plan %lld), %lld rounds (%lld)",
                  n, mask, sup, rank, k, prev_hi, parts, p.parts, rounds, want_rounds);
            for (long long i = 0; i < m; ++i) CHECK(scored[i], "n=%d mask=%u: position %lld was never scored", n, mask, i);
            // the reference: the listed rows ranked by (score desc, id asc), the first k; positions map to ids through sel
            Part want;
            for (long long i = 0; i < m; ++i) want.push_back({score[sel[i]], sel[i]});
            std::sort(want.begin(), want.end(), better);
            if ((int)want.size() > k) want.resize(k);
            bool same = slots.size() == 1 && slots[0].size() == want.size();
            for (size_t i = 0; same && i < want.size(); ++i) same = sel[slots[0][i].pos] == want[i].pos && slots[0][i].score == want[i].score;
            CHECK(same, "n=%d mask=%u sup=%lld rank=%lld k=%d: the result differs from a plain sort of the listed rows", n, mask, sup, rank, k);
        }
    }
    std::printf("subset plan, small: %lld cases executed, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

static int large() {
    std::mt19937_64 rng(20261020);
    for (int it = 0; it < 40000; ++it) {
        ++cases;
        const long long n = it % 4 == 0 ? kSubsetMaxRows + 1 - (long long)(rng() % 1000) : 2 + (long long)(rng() % kSubsetMaxRows);
        const long long m = it % 3 == 0 ? std::min(n - 1, kSubsetMaxRows) - (long long)(rng() % std::min<long long>(n - 1, 1000)) : 1 + (long long)(rng() % (unsigned long long)std::min(n - 1, kSubsetMaxRows));
        const int nq = it % 7 == 0 ? 1 + (int)(rng() % 100000) : 1 + (int)(rng() % 300);
        const int k = it % 5 == 0 ? kSubsetMaxK - (int)(rng() % 3) : 1 + (int)(rng() % kSubsetMaxK);
        const long long sup = it % 6 == 0 ? 1 + (long long)(rng() % 100000) : 0;
        const SubsetPlan p = subset_plan(n, m, nq, k, sup, 0);
        CHECK(p.route == kSubsetScan, "n=%lld m=%lld nq=%d k=%d: route %d", n, m, nq, k, p.route);
        if (p.route != kSubsetScan) continue;
        CHECK(p.batch >= 1 && p.batch <= kSubsetMaxBatch && p.batch <= nq, "nq=%d batch=%d", nq, p.batch);
        CHECK(p.rank_rows == kSubsetRankRows && p.super_rows >= 1 && p.super_rows <= m && (p.super_rows == m || p.super_rows % p.rank_rows == 0) &&
              p.super_parts == (p.super_rows + p.rank_rows - 1) / p.rank_rows, "m=%lld super_rows=%lld super_parts=%lld", m, p.super_rows, p.super_parts);
        CHECK(p.score_bytes == 4ll * p.batch * p.super_parts * p.rank_rows && p.score_bytes <= kSubsetScoreBytes && p.score_bytes >= 4ll * p.batch * p.super_rows, "m=%lld nq=%d: %lld bytes of scores", m, nq, p.score_bytes);
        CHECK(subset_score_index(p.super_rows - 1, p.batch - 1, p.batch, p.rank_rows) < p.score_bytes / 4, "m=%lld: the last score lands past the workspace", m);
        CHECK((p.supers - 1) * p.super_rows < m && m <= p.supers * p.super_rows, "m=%lld: %lld supers of %lld", m, p.supers, p.super_rows);
        CHECK((p.parts - 1) * p.rank_rows < m && m <= p.parts * p.rank_rows && p.parts <= 262144, "m=%lld: %lld parts", m, p.parts);
        CHECK(p.super_parts * (long long)p.batch <= 0x7FFFFFFF, "the ranking launch's grid: %lld x %d", p.super_parts, p.batch);
        if (p.parts > 1) {
            CHECK(p.fan_in >= 2 && p.fan_in <= 16 && p.fan_in <= p.super_parts + 1 && subset_next_pow2((long long)p.fan_in * k) <= kSubsetMergeKeys && (long long)p.fan_in * k <= 16384, "k=%d fan_in=%d", k, p.fan_in);
            const long long last = p.parts - (p.supers - 1) * p.super_parts;
            CHECK(last >= 1 && last <= p.super_parts && p.rounds == (p.supers - 1) * ((p.super_parts + p.fan_in - 2) / (p.fan_in - 1)) + (last + p.fan_in - 2) / (p.fan_in - 1) && p.rounds >= 1,
                  "parts=%lld super_parts=%lld fan_in=%d rounds=%lld", p.parts, p.super_parts, p.fan_in, p.rounds);
            CHECK(p.merge_bytes == 12ll * (p.super_parts + 2) * p.batch * k && p.merge_bytes <= kSubsetScoreBytes + 2 * 12ll * kSubsetMaxBatch * kSubsetMaxK, "merge bytes %lld", p.merge_bytes);
        } else {
            CHECK(p.fan_in == 0 && p.rounds == 0 && p.merge_bytes == 0, "one part: fan_in=%d rounds=%lld", p.fan_in, p.rounds);
        }
        const SubsetSpan last = subset_super(p, m, p.supers - 1);
        CHECK(last.hi == m && last.lo < m && last.lo == (p.supers - 1) * p.super_rows, "m=%lld: the last super-chunk [%lld, %lld)", m, last.lo, last.hi);
        const SubsetSpan lc = subset_rank_chunk(p, last, subset_rank_chunks(p, last) - 1);
        CHECK(lc.hi == m && lc.lo < m && lc.hi - lc.lo <= p.rank_rows, "m=%lld: the last rank chunk [%lld, %lld)", m, lc.lo, lc.hi);
    }
    // the limits, at their edges
    CHECK(subset_plan(100000, 16384, 1, 100000, 0, 0).route == kSubsetScan, "any k while the list is short");
    CHECK(subset_plan(100000, 16385, 1, 8192, 0, 0).route == kSubsetScan && subset_plan(100000, 16385, 1, 8193, 0, 0).route == kSubsetRefused, "k <= 8192 beyond one part");
    CHECK(subset_plan(kSubsetMaxRows + 2, kSubsetMaxRows + 1, 1, 10, 0, 0).route == kSubsetRefused && subset_plan(kSubsetMaxRows + 2, kSubsetMaxRows, 1, 10, 0, 0).route == kSubsetScan, "2^32 - 2 ids");
    CHECK(subset_plan(10, 11, 1, 1, 0, 0).route == kSubsetRefused && subset_plan(10, -1, 1, 1, 0, 0).route == kSubsetRefused, "more ids than rows");
    { const SubsetPlan p = subset_plan(150000, 147457, 2, 2048, 0, 0); CHECK(p.parts == 10 && p.fan_in == 8 && p.rounds == 2 && p.supers == 1, "the ten-part case: %lld parts, fan-in %d, %lld rounds", p.parts, p.fan_in, p.rounds); }
    // the kernel's LDS: one query tile of one K-slice, whatever d and the dtype are (the rows never pass through LDS)
    for (int d = 1; d <= kSubsetMaxD; ++d) for (int esz : {4, 2, 1, 1}) {
        ++cases;
        const SubsetPlan p = subset_plan(1000, 10, 64, 10, 0, 0);
        const int slices = (d + p.slice - 1) / p.slice;
        CHECK(p.lds_bytes == p.q_tile * p.slice * 4 && p.lds_bytes <= 160 * 1024 && p.slice % 16 == 0 && slices * p.slice >= d && esz >= 1, "d=%d: %d bytes of LDS", d, p.lds_bytes);
        CHECK(p.rows_per_wg == (kSubsetThreads / 2) * kSubsetR, "rows per workgroup %d", p.rows_per_wg);
    }
    std::printf("subset plan, large: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

static int lists() {
    const long long good[] = {10, 11, 15, 19};
    CHECK(subset_first_bad(good, 4, 10, 20) == -1 && subset_first_bad(good, 0, 10, 20) == -1, "a good list");
    const long long low[] = {9, 11}, high[] = {10, 20}, desc[] = {10, 12, 11, 30}, dup[] = {10, 12, 12, 5};
    CHECK(subset_first_bad(low, 2, 10, 20) == 0 && subset_first_bad(high, 2, 10, 20) == 1, "out of range");
    CHECK(subset_first_bad(desc, 4, 10, 20) == 2 && subset_first_bad(dup, 4, 10, 20) == 2, "descending / duplicate: the first offender");
    cases += 6;
    std::printf("subset plan, lists: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "small")) return small();
    if (argc == 2 && !std::strcmp(argv[1], "large")) return large();
    if (argc == 2 && !std::strcmp(argv[1], "lists")) return lists();
    std::printf("usage: %s small|large|lists\n", argv[0]);
    return 2;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "subset_plan.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "subset_plan")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def run(exe: str, what: str):
    return subprocess.run([exe, what], capture_output=True, text=True, timeout=600, env=_ENV)
