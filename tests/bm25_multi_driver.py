"""A host-compiled driver of a BM25 batch with a prepared filter per query (veritasfi_amd/csrc/vf_bm25_multi.h), used by
tests/test_bm25_multi_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone.  It reads a
CSC index of at most 32 rows, two queries and a list of ranks k, and REPLAYS a two-slot group as the kernels k_bm25_accum_m,
k_bm25_tail_count_m / k_bm25_tail_write_m and k_bm25_pad_out_m run it, with the header's own functions: each slot reads its descriptor,
the scatter marks the rows bm25m_form lets through, the tail takes bm25f_allowed_untouched of bm25m_tail_word, the padding starts at the
descriptor's pad_from.  The ranks a slot is left with -- the touched rows (in ascending order: the select and the sort are not the
subject), then the tail, then the padding -- must equal the replay of that slot ALONE by vf_bm25_filter.h's one-filter functions
(bm25f_row_allowed, bm25f_allowed_untouched, bm25f_plan; no launch at all for a filter of no row), and no rank may stay unwritten or be
written twice.  Slot 0 runs through every filter of the index; slot 1 holds a fixed other filter in corpus form, the same in subset
form, no filter, and the empty filter.  Then the plan (bm25m_plan, bm25m_group_pad_span) at the sizes the input lists, against
vf_bm25_call.h's plan of the one-filter prepared search.

  input   n V nnz / indptr [V + 1] / indices [nnz] / two lines "<count> <columns>": the queries of slot 0 and slot 1 / the fixed filter
          of slot 1 as a bit mask / NK, then NK ranks / NP, then NP lines "n k nq slot_cap"
  output  per filter f of slot 0 and rank k (slot 1 holding the fixed filter) "f <f> k <k> s0 <k ids> s1 <k ids>"; per plan line
          "plan <n> <k> <nq> <cap> S <S> small <0|1> blocks <tail blocks> stride <tblk stride> groups <groups>"; last
          "multi: <failures> failure(s)"
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
#include "vf_bm25_multi.h"
#include "vf_bm25_call.h"
using namespace vf;

static long long failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

static long long n, V, nnz, words;
static std::vector<long long> indptr;
static std::vector<int> indices;
static const long long kUnwritten = -2;

// the ranks one slot ends with: touched rows ascending (cut to k), the tail, the padding; each rank written once
struct Slot {
    std::vector<uint32_t> touched;
    std::vector<long long> out;
    std::vector<int> writes;
    void begin(long long k) { touched.assign((size_t)words, 0u); out.assign((size_t)k, kUnwritten); writes.assign((size_t)k, 0); }
    void put(long long rank, long long id) { out[(size_t)rank] = id; ++writes[(size_t)rank]; }
    long long emit_touched(long long k) {   // the select, the gather and the sort: min(k, touched) ranks
        long long r = 0;
        for (long long row = 0; row < n && r < k; ++row)
            if ((touched[(size_t)(row >> 5)] >> (row & 31)) & 1u) put(r++, row);
        return r;
    }
};

// the _m kernels on one slot: everything the slot's filter decides is read from its descriptor
static void multi_slot(const Bm25Desc* desc, int q, const std::vector<int>& query, long long k, Slot& s, int* subset_adds) {
    const Bm25Desc& d = desc[q];
    s.begin(k);
    for (int col : query)                                                  // k_bm25_accum_m, one launch per token position
        for (long long p = indptr[(size_t)col]; p < indptr[(size_t)col + 1]; ++p) {
            const uint32_t row = (uint32_t)indices[(size_t)p];
            const Bm25mForm form = bm25m_form(d);
            if (form != kBm25mPlain && !bm25f_row_allowed(d.allow, row)) continue;
            if (form == kBm25mSubset) ++*subset_adds;                      // live_score(idf[col], tf, ...) in place of the stored score
            s.touched[row >> 5] |= 1u << (row & 31u);
        }
    for (long long r = d.pad_from; r < k; ++r) s.put(r, -1);               // k_bm25_pad_out_m
    long long pos = s.emit_touched(k);
    if (pos >= k) return;                                                  // k_bm25_tail_*_m over ALL blocks: nsel < k
    for (long long w = 0; w < words; ++w)
        for (uint32_t z = bm25f_allowed_untouched(s.touched[(size_t)w], bm25f_valid_mask(w * 32, n), bm25m_tail_word(d.allow, w)); z && pos < k; z &= z - 1, ++pos) {
            int b = 0;
            while (!((z >> b) & 1u)) ++b;
            s.put(pos, w * 32 + b);
        }
}

// the one-filter call on the same query alone (vf_bm25_filter.h); allow null: the unfiltered call
static void single_slot(const uint32_t* allow, const std::vector<int>& query, long long k, Slot& s) {
    s.begin(k);
    if (allow) {
        const Bm25FilterCheck fc = bm25f_check(allow, n);
        if (fc.m == 0) {                                                   // no launch: bm_all_padding
            for (long long r = 0; r < k; ++r) s.put(r, -1);
            return;
        }
        for (long long r = bm25f_plan(words, fc.m, k).pad_from; r < k; ++r) s.put(r, -1);
    }
    for (int col : query)
        for (long long p = indptr[(size_t)col]; p < indptr[(size_t)col + 1]; ++p) {
            const uint32_t row = (uint32_t)indices[(size_t)p];
            if (allow && !bm25f_row_allowed(allow, row)) continue;
            s.touched[row >> 5] |= 1u << (row & 31u);
        }
    long long pos = s.emit_touched(k);
    for (long long w = 0; w < words && pos < k; ++w)
        for (uint32_t z = bm25f_allowed_untouched(s.touched[(size_t)w], bm25f_valid_mask(w * 32, n), allow ? allow[w] : 0xFFFFFFFFu); z && pos < k; z &= z - 1, ++pos) {
            int b = 0;
            while (!((z >> b) & 1u)) ++b;
            s.put(pos, w * 32 + b);
        }
}

static void same(const Slot& got, const Slot& want, long long k, const char* what, long long f, int variant) {
    for (long long r = 0; r < k; ++r) {
        CHECK(got.writes[(size_t)r] == 1, "%s filter %lld variant %d k %lld: rank %lld written %d times", what, f, variant, k, r, got.writes[(size_t)r]);
        CHECK(got.out[(size_t)r] == want.out[(size_t)r], "%s filter %lld variant %d k %lld: rank %lld is %lld, the one-filter call has %lld", what, f, variant, k, r,
              got.out[(size_t)r], want.out[(size_t)r]);
    }
}

static void fill(std::vector<uint32_t>& w, unsigned long long mask) {
    std::fill(w.begin(), w.end(), 0u);
    w[0] = (uint32_t)mask;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    if (std::fscanf(f, "%lld %lld %lld", &n, &V, &nnz) != 3 || n < 1 || n > 32) return 2;
    indptr.resize((size_t)V + 1);
    indices.resize((size_t)nnz);
    for (auto& v : indptr) if (std::fscanf(f, "%lld", &v) != 1) return 2;
    for (auto& v : indices) if (std::fscanf(f, "%d", &v) != 1 || v < 0 || v >= n) return 2;
    std::vector<int> query[2];
    for (auto& q : query) {
        long long cnt;
        if (std::fscanf(f, "%lld", &cnt) != 1) return 2;
        q.resize((size_t)cnt);
        for (auto& c : q) if (std::fscanf(f, "%d", &c) != 1 || c < 0 || c >= V) return 2;
    }
    unsigned long long fixed;
    long long NK, NP;
    if (std::fscanf(f, "%llu %lld", &fixed, &NK) != 2) return 2;
    std::vector<long long> ks((size_t)NK);
    for (auto& k : ks) if (std::fscanf(f, "%lld", &k) != 1 || k < 1 || k > n) return 2;

    words = (bm25f_words(n) + kBm25FilterBlockWords - 1) / kBm25FilterBlockWords * kBm25FilterBlockWords;   // the handle's `words`
    std::vector<uint32_t> allow0((size_t)words, 0u), allow1((size_t)words, 0u), none((size_t)words, 0u);
    std::vector<double> idf((size_t)(V > 0 ? V : 1), 1.0);   // a subset-mode filter's table: only that it is there is read here
    fill(allow1, fixed);
    Slot got[2], want[2];
    const long long m1 = bm25f_check(allow1.data(), n).m;
    for (unsigned long long mask = 0; mask < (1ull << n); ++mask) {
        fill(allow0, mask);
        const long long m0 = bm25f_check(allow0.data(), n).m;
        for (long long k : ks) {
            // slot 1: the fixed filter in corpus form, the same in subset form, no filter, the empty filter; slot 0 in corpus form, and in
            // subset form beside variant 1
            for (int variant = 0; variant < 4; ++variant) {
                const bool sub = variant == 1;
                Bm25Desc desc[2];
                desc[0] = bm25m_desc(allow0.data(), sub ? idf.data() : nullptr, 2.5, 1.5, 0.75, m0, k);
                desc[1] = variant == 0   ? bm25m_desc(allow1.data(), nullptr, 1.0, 0.0, 0.0, m1, k)
                          : variant == 1 ? bm25m_desc(allow1.data(), idf.data(), 2.5, 1.5, 0.75, m1, k)
                          : variant == 2 ? bm25m_desc_none(k)
                                         : bm25m_desc(none.data(), nullptr, 1.0, 0.0, 0.0, 0, k);
                CHECK(bm25m_form(desc[0]) == (sub ? kBm25mSubset : kBm25mCorpus), "slot 0's form");
                CHECK(bm25m_form(desc[1]) == (variant == 1 ? kBm25mSubset : variant == 2 ? kBm25mPlain : kBm25mCorpus), "slot 1's form in variant %d", variant);
                CHECK(desc[0].pad_from == bm25f_plan(words, m0, k).pad_from && desc[1].pad_from == (variant == 2 ? k : bm25f_plan(words, variant == 3 ? 0 : m1, k).pad_from),
                      "pad_from of filter %llu variant %d k %lld", mask, variant, k);
                int adds[2] = {0, 0};
                multi_slot(desc, 0, query[0], k, got[0], &adds[0]);
                multi_slot(desc, 1, query[1], k, got[1], &adds[1]);
                single_slot(allow0.data(), query[0], k, want[0]);
                single_slot(variant == 2 ? nullptr : variant == 3 ? none.data() : allow1.data(), query[1], k, want[1]);
                same(got[0], want[0], k, "slot 0", (long long)mask, variant);
                same(got[1], want[1], k, "slot 1", (long long)mask, variant);
                CHECK(sub || (adds[0] == 0 && adds[1] == 0), "a slot without an idf table scored from tf");
                const Bm25MultiPlan p = bm25m_plan(desc, k, 2, 64, words);
                CHECK(p.no_launch == (m0 == 0 && (variant == 3 || (variant != 2 && m1 == 0))), "no_launch of filter %llu variant %d", mask, variant);
                const long long s0 = k - desc[0].pad_from, s1 = k - desc[1].pad_from;
                CHECK(bm25m_group_pad_span(desc, 0, 2, k) == (s0 > s1 ? s0 : s1) && bm25m_group_pad_span(desc, 1, 1, k) == s1, "the group's padding span");
                if (variant == 0) {
                    std::printf("f %llu k %lld s0", mask, k);
                    for (long long r = 0; r < k; ++r) std::printf(" %lld", got[0].out[(size_t)r]);
                    std::printf(" s1");
                    for (long long r = 0; r < k; ++r) std::printf(" %lld", got[1].out[(size_t)r]);
                    std::printf("\n");
                }
            }
        }
    }

    // the plan at other sizes: a batch of one filter must plan as vf_bm25_call.h plans the one-filter prepared search
    if (std::fscanf(f, "%lld", &NP) != 1) return 2;
    for (long long i = 0; i < NP; ++i) {
        long long pn, k;
        int nq, cap;
        if (std::fscanf(f, "%lld %lld %d %d", &pn, &k, &nq, &cap) != 4 || k < 1 || k > pn || nq < 1 || cap < 1) return 2;
        const long long pw = (bm25f_words(pn) + kBm25FilterBlockWords - 1) / kBm25FilterBlockWords * kBm25FilterBlockWords;
        const uint32_t some = 1u;   // a non-null bitmap pointer: the plan does not read through it
        for (int shape = 0; shape < 4; ++shape) {   // one filter of m >= k rows on every query; one of m < k; filters of no row; a mix with unfiltered queries
            const long long m = shape == 0 ? pn : shape == 1 ? (k > 1 ? k - 1 : 0) : shape == 2 ? 0 : k / 2;
            std::vector<Bm25Desc> desc((size_t)nq);
            for (int q = 0; q < nq; ++q) desc[(size_t)q] = (shape == 3 && q % 2 == 0) ? bm25m_desc_none(k) : bm25m_desc(&some, nullptr, 1.0, 0.0, 0.0, m, k);
            const Bm25MultiPlan p = bm25m_plan(desc.data(), k, nq, cap, pw);
            Bm25Call c = bm25c_decode(nq | kBm25cPrepared, false, 3);
            CHECK(c.kind == kBm25PrepSearch && c.refusal == kBm25Accepted, "the decoder on a prepared search");
            const Bm25LaunchPlan one = bm25c_plan(c, k, nq, cap, pw, m);
            CHECK(p.small == one.small && p.S == one.S && p.tail_blocks == one.tail_blocks && p.tblk_stride == one.tblk_stride,
                  "n %lld k %lld nq %d cap %d shape %d: S %d/%d blocks %d/%d stride %lld/%lld", pn, k, nq, cap, shape, p.S, one.S, p.tail_blocks, one.tail_blocks, p.tblk_stride, one.tblk_stride);
            if (shape != 3) {
                CHECK(p.no_launch == one.no_launch, "n %lld k %lld shape %d: no_launch", pn, k, shape);
                CHECK(desc[0].pad_from == one.pad_from && (bm25m_group_pad_span(desc.data(), 0, nq < p.S ? nq : p.S, k) > 0) == one.pad_out, "n %lld k %lld shape %d: padding", pn, k, shape);
            } else {
                CHECK(!p.no_launch, "a batch with an unfiltered query launches");
                CHECK(desc[0].pad_from == k && bm25m_group_pad_span(desc.data(), 0, 1, k) == 0, "an unfiltered query has no padding");
                if (nq > 1) CHECK(bm25m_group_pad_span(desc.data(), 0, 2, k) == k - m, "the span of a mixed pair");
            }
            long long groups = 0;
            for (int q0 = 0; q0 < nq; q0 += p.S) ++groups;
            if (shape == 0) std::printf("plan %lld %lld %d %d S %d small %d blocks %d stride %lld groups %lld\n", pn, k, nq, cap, p.S, (int)p.small, p.tail_blocks, p.tblk_stride, groups);
        }
    }
    // the decoder still refuses what it refused: phase 5, and the flag beside another
    CHECK(bm25c_decode(1 | kBm25cPrepared, false, 5).refusal == kBm25PreparedPhase, "phase 5");
    CHECK(bm25c_decode(1 | kBm25cPrepared | kBm25cFilter, false, 3).refusal == kBm25PreparedNotAlone, "VF_BM25_PREPARED | VF_BM25_FILTER");
    CHECK(bm25c_decode(1 | kBm25cPrepared | kBm25cSubstats, false, 3).refusal == kBm25PreparedNotAlone, "VF_BM25_PREPARED | VF_BM25_SUBSTATS");
    CHECK(bm25c_decode(1 | kBm25cPrepared, true, 3).refusal == kBm25NullPrepared, "a null struct");
    std::fclose(f);
    std::printf("multi: %lld failure(s)\n", failures);
    return failures ? 1 : 0;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "bm25_multi.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "bm25_multi")
    subprocess.check_call([cxx, "-O2", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def write_input(path, n, indptr, indices, queries, fixed_mask, ks, plans) -> str:
    """The driver's input file; ``queries``: the two slots' column lists; ``plans``: (n, k, nq, slot_cap) tuples."""
    with open(path, "w") as f:
        f.write(f"{n} {len(indptr) - 1} {len(indices)}\n")
        for arr in (indptr, indices):
            f.write(" ".join(str(int(v)) for v in arr) + "\n")
        for q in queries:
            f.write(" ".join(str(int(v)) for v in [len(q)] + list(q)) + "\n")
        f.write(f"{int(fixed_mask)}\n")
        f.write(" ".join(str(int(v)) for v in [len(ks)] + list(ks)) + "\n")
        f.write(f"{len(plans)}\n")
        for p in plans:
            f.write(" ".join(str(int(v)) for v in p) + "\n")
    return str(path)


def run(exe: str, input_path: str):
    return subprocess.run([exe, input_path], capture_output=True, text=True, timeout=600, env=_ENV)


def parse(stdout: str):
    """-> ({(filter mask, k): (slot 0's ids, slot 1's ids)}, {(n, k, nq, cap): (S, small, blocks, stride, groups)})."""
    rows, plans = {}, {}
    for line in stdout.splitlines():
        w = line.split()
        if line.startswith("f "):
            k = int(w[3])
            rows[(int(w[1]), k)] = ([int(v) for v in w[5:5 + k]], [int(v) for v in w[6 + k:6 + 2 * k]])
        elif line.startswith("plan "):
            plans[tuple(int(v) for v in w[1:5])] = (int(w[6]), int(w[8]), int(w[10]), int(w[12]), int(w[14]))
    return rows, plans
