"""A host-compiled driver of the live BM25 update's index arithmetic (veritasfi_amd/csrc/vf_bm25_live.h), used by
tests/test_bm25_live_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under ASan + UBSan.  The program is stand-alone:

  driver IN OUT   IN holds a small CSC index with term frequencies, a few deltas (new documents as CSC) and a table of idf values
                  (numpy's log: the program takes no logarithm, as the library takes none).  For EVERY subset of removed rows that
                  leaves a document, every delta and the chunk sizes 1, 4 and nnz + 5 it EXECUTES the update the way the kernels do
                  -- row map, survivors per chunk, scan, the new indptr from the column starts each chunk owns, the rewrite with
                  the columns recovered from marked starts and a running maximum, the append -- and holds it to what the scheme
                  relies on: every column start has one owner, every output position one writer, the recovered column is the
                  posting's column, and the chunk size changes nothing.  OUT gets each case's arrays for the test to compare with
                  bm25_index_arrays.

It prints the number of cases and the first failures, and returns 1 if there was one."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <algorithm>
#include <vector>
#include "vf_bm25_live.h"
using namespace vf;

static long long failures = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

typedef std::vector<long long> VL;
typedef std::vector<int> VI;
struct Delta { long long n_new, Vn; VL ptr; VI rows, tf, dl; };
struct Result { VL newptr; VI indices, tf; std::vector<uint32_t> bits; VI doclen; };

static VL read_vl(FILE* f) {
    long long n = 0;
    if (std::fread(&n, 8, 1, f) != 1) { std::printf("short input\n"); std::exit(2); }
    VL v((size_t)n);
    if (n && std::fread(v.data(), 8, (size_t)n, f) != (size_t)n) { std::printf("short input\n"); std::exit(2); }
    return v;
}
static VI to_vi(const VL& v) { return VI(v.begin(), v.end()); }

// one update, executed chunk by chunk as the kernels execute it
static Result run(long long n0, long long V, const VL& indptr, const VI& indices, const VI& tf, const VI& doclen, const VI& rem, const Delta& d,
                  long long C, const std::vector<double>& idf_table, long long table_n, double k1, double b, const char* tag) {
    const long long nnz = indptr[V], m = (long long)rem.size(), n1 = n0 - m, Vn = d.Vn, dnnz = d.ptr[Vn];
    Result r;
    // k_bm25_live_rowmap
    VI map((size_t)n0);
    r.doclen.assign((size_t)(n1 + d.n_new), -1);
    for (long long row = 0; row < n0; ++row) {
        const long long nr = live_new_row(row, rem.data(), m);
        CHECK(nr >= -1 && nr < n1, "%s: row %lld -> %lld", tag, row, nr);
        map[row] = (int)nr;
        if (nr >= 0) { CHECK(r.doclen[nr] == -1, "%s: new row %lld written twice", tag, nr); r.doclen[nr] = doclen[row]; }
    }
    for (long long i = 0; i < d.n_new; ++i) r.doclen[n1 + i] = d.dl[i];
    for (int x : r.doclen) CHECK(x >= 0, "%s: a document length was not written", tag);
    // k_bm25_live_count, k_bm25_live_scan
    const long long chunks = live_chunks(nnz, C);
    VL csum((size_t)chunks + 1, 0);
    long long covered = 0;
    for (long long k = 0; k < chunks; ++k) {
        const LiveChunk ch = live_chunk(nnz, C, k);
        CHECK(ch.lo == covered && ch.hi >= ch.lo && ch.hi - ch.lo <= C && ch.hi <= nnz && ch.last == (k + 1 == chunks), "%s: chunk %lld = [%lld, %lld)", tag, k, ch.lo, ch.hi);
        covered = ch.hi;
        for (long long p = ch.lo; p < ch.hi; ++p) csum[k] += map[indices[p]] >= 0;
    }
    CHECK(covered == nnz, "%s: the chunks end at %lld of %lld", tag, covered, nnz);
    long long runsum = 0;
    for (long long k = 0; k <= chunks; ++k) { const long long f = csum[k]; csum[k] = runsum; runsum += f; }
    // k_bm25_live_indptr
    r.newptr.assign((size_t)Vn + 1, -1);
    for (long long k = 0; k < chunks; ++k) {
        const LiveChunk ch = live_chunk(nnz, C, k);
        const long long cnt = ch.hi - ch.lo;
        VI rank((size_t)cnt + 1, 0);
        for (long long i = 0; i < cnt; ++i) rank[i + 1] = rank[i] + (map[indices[ch.lo + i]] >= 0);
        const long long c0 = live_owned_first(indptr.data(), V, Vn, nnz, ch), c1 = live_owned_end(indptr.data(), V, Vn, nnz, ch);
        for (long long c = c0; c < c1; ++c) {
            const long long s = live_old_start(indptr.data(), V, nnz, c);
            CHECK(c >= 0 && c <= Vn && s >= ch.lo && s - ch.lo <= cnt && (s < ch.hi || ch.last), "%s: chunk %lld owns column %lld at %lld", tag, k, c, s);
            if (c < 0 || c > Vn || s < ch.lo || s - ch.lo > cnt) return r;
            CHECK(r.newptr[c] == -1, "%s: column %lld has two owners", tag, c);
            r.newptr[c] = live_dest(csum[k] + rank[s - ch.lo], d.ptr[c]);
        }
    }
    for (long long c = 0; c <= Vn; ++c) CHECK(r.newptr[c] >= 0 && (c == 0 || r.newptr[c] >= r.newptr[c - 1]), "%s: new indptr[%lld] = %lld", tag, c, r.newptr[c]);
    CHECK(r.newptr[0] == 0 && r.newptr[Vn] == csum[chunks] + dnnz, "%s: the new indptr ends at %lld", tag, r.newptr[Vn]);
    const long long nnz1 = r.newptr[Vn], N = n1 + d.n_new;
    if (nnz1 < 0 || nnz1 > nnz + dnnz) return r;
    long long total = 0;
    for (int x : r.doclen) total += x;
    const double avgdl = total > 0 ? (double)total / (double)N : 1.0;
    std::vector<double> idf((size_t)Vn);
    for (long long c = 0; c < Vn; ++c) idf[c] = idf_table[(size_t)(N * table_n + (r.newptr[c + 1] - r.newptr[c]))];
    // k_bm25_live_rewrite
    r.indices.assign((size_t)nnz1, -1); r.tf.assign((size_t)nnz1, -1); r.bits.assign((size_t)nnz1, 0);
    for (long long k = 0; k < chunks; ++k) {
        const LiveChunk ch = live_chunk(nnz, C, k);
        const long long cnt = ch.hi - ch.lo;
        if (cnt == 0) continue;
        const long long cfirst = live_col_of(indptr.data(), V, Vn, nnz, ch.lo), cend = live_col_lower(indptr.data(), V, Vn, nnz, ch.hi);
        VI col((size_t)cnt, -1);
        col[0] = (int)cfirst;
        for (long long c = cfirst + 1; c < cend; ++c) {
            CHECK(c < V && indptr[c] > ch.lo && indptr[c] < ch.hi, "%s: chunk %lld marks column %lld", tag, k, c);
            if (!(c < V && indptr[c] > ch.lo && indptr[c] < ch.hi)) return r;
            col[indptr[c] - ch.lo] = std::max(col[indptr[c] - ch.lo], (int)c);
        }
        for (long long i = 1; i < cnt; ++i) col[i] = std::max(col[i], col[i - 1]);
        long long rank = 0;
        for (long long i = 0; i < cnt; ++i) {
            const long long p = ch.lo + i, c = col[i];
            CHECK(c >= 0 && c < V && indptr[c] <= p && p < indptr[c + 1], "%s: posting %lld recovered column %lld", tag, p, c);
            const int nr = map[indices[p]];
            if (nr < 0) continue;
            const long long dst = live_dest(csum[k] + rank, d.ptr[c]);
            ++rank;
            CHECK(dst >= 0 && dst < nnz1 && r.indices[dst] == -1, "%s: posting %lld -> %lld", tag, p, dst);
            if (dst < 0 || dst >= nnz1) return r;
            r.indices[dst] = nr; r.tf[dst] = tf[p];
            const float sc = live_score(idf[c], tf[p], r.doclen[nr], avgdl, k1, b, 1.0 - b);
            std::memcpy(&r.bits[dst], &sc, 4);
        }
    }
    // k_bm25_live_append
    for (long long q = 0; q < dnnz; ++q) {
        long long lo = 0, hi = Vn;
        while (lo < hi) { const long long mid = lo + (hi - lo) / 2; if (d.ptr[mid + 1] <= q) lo = mid + 1; else hi = mid; }
        const long long dst = live_delta_dest(r.newptr[lo + 1], d.ptr[lo + 1], q);
        CHECK(dst >= 0 && dst < nnz1 && r.indices[dst] == -1, "%s: delta posting %lld -> %lld", tag, q, dst);
        if (dst < 0 || dst >= nnz1) return r;
        const int nr = (int)(n1 + d.rows[q]);
        r.indices[dst] = nr; r.tf[dst] = d.tf[q];
        const float sc = live_score(idf[lo], d.tf[q], r.doclen[nr], avgdl, k1, b, 1.0 - b);
        std::memcpy(&r.bits[dst], &sc, 4);
    }
    for (long long p = 0; p < nnz1; ++p) CHECK(r.indices[p] >= 0, "%s: position %lld has no writer", tag, p);
    for (long long c = 0; c < Vn; ++c)
        for (long long p = r.newptr[c] + 1; p < r.newptr[c + 1]; ++p) CHECK(r.indices[p] > r.indices[p - 1], "%s: column %lld is not strictly ascending at %lld", tag, c, p);
    return r;
}

static void put(FILE* f, const void* p, size_t n) { if (n && std::fwrite(p, 4, n, f) != n) { std::printf("short write\n"); std::exit(2); } }

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: %s IN OUT\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    const VL head = read_vl(f);   // n0, V, table_n, deltas
    const long long n0 = head[0], V = head[1], table_n = head[2], nd = head[3];
    const VL indptr = read_vl(f);
    const VI indices = to_vi(read_vl(f)), tf = to_vi(read_vl(f)), doclen = to_vi(read_vl(f));
    std::vector<Delta> deltas;
    for (long long i = 0; i < nd; ++i) {
        Delta d;
        const VL h = read_vl(f);
        d.n_new = h[0]; d.Vn = h[1];
        d.ptr = read_vl(f); d.rows = to_vi(read_vl(f)); d.tf = to_vi(read_vl(f)); d.dl = to_vi(read_vl(f));
        deltas.push_back(d);
    }
    std::vector<double> table((size_t)(table_n * table_n)), kb(2);
    if (std::fread(table.data(), 8, table.size(), f) != table.size() || std::fread(kb.data(), 8, 2, f) != 2) { std::printf("short input\n"); return 2; }
    std::fclose(f);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::printf("cannot open %s\n", argv[2]); return 2; }
    const long long nnz = indptr[V], chunk_sizes[] = {1, 4, nnz + 5};
    for (unsigned mask = 0; mask < (1u << n0); ++mask)
    for (size_t di = 0; di < deltas.size(); ++di) {
        VI rem;
        for (int i = 0; i < n0; ++i) if (mask >> i & 1) rem.push_back(i);
        if (n0 - (long long)rem.size() < 1) continue;   // every subset that leaves at least one document
        Result first;
        for (int ci = 0; ci < 3; ++ci) {
            ++cases;
            char tag[96];
            std::snprintf(tag, sizeof tag, "mask=%u delta=%zu chunk=%lld", mask, di, chunk_sizes[ci]);
            Result r = run(n0, V, indptr, indices, tf, doclen, rem, deltas[di], chunk_sizes[ci], table, table_n, kb[0], kb[1], tag);
            if (ci == 0) first = r;
            else CHECK(r.newptr == first.newptr && r.indices == first.indices && r.tf == first.tf && r.bits == first.bits && r.doclen == first.doclen, "%s: differs from chunk size 1", tag);
        }
        const int32_t hdr[4] = {(int32_t)mask, (int32_t)di, (int32_t)deltas[di].Vn, (int32_t)first.indices.size()};
        put(out, hdr, 4);
        const VI np32(first.newptr.begin(), first.newptr.end());
        put(out, np32.data(), np32.size()); put(out, first.indices.data(), first.indices.size());
        put(out, first.tf.data(), first.tf.size()); put(out, first.bits.data(), first.bits.size());
    }
    std::fclose(out);
    std::printf("bm25 live plan: %lld cases executed, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", ASAN_OPTIONS="detect_leaks=0")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "bm25_live_plan.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "bm25_live_plan")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", CSRC, src, "-o", exe])
    return exe


def run(exe: str, inp: str, out: str):
    return subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=600, env=_ENV)
