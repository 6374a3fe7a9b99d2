"""A host-compiled driver of the plan of a dense batch whose queries each bring their own row list
(veritasfi_amd/csrc/vf_subset_multi.h), used by tests/test_subset_multi_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone:

  driver small   a 12-row index, three lists of every length triple from {0, 1, 2, 3, 5, 12}, every list_of in {0, 1, 2}^nq for
                 nq = 1 .. 5, under four shrunken blockings (rows per workgroup 2 and 64, tiles of 2 and 4 queries, size classes such
                 as 2 / 4 / 16, passes of 2 and 256 queries) and k in {1, 3, 12, 20}: the plan is EXECUTED on integer arrays the way the
                 library executes it on the device -- walk the scan's grid tile by tile and workgroup by workgroup (subm_wg_kind), rank
                 every class's score rows, map positions through each query's own list -- and held to a plain sort of the listed rows
  driver large   seeded random calls at the real constants (up to 600 queries, lists of up to 16 384 ids): the tables' invariants, the
                 launch and workspace bounds, the refusals; no score arrays

Each prints the number of cases and the first failures, and returns 1 if there was one."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

DRIVER = r"""
#include <climits>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <random>
#include <vector>
#include "vf_subset_multi.h"
using namespace vf;

static long long failures = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

static const long long SENT = LLONG_MIN;   // stands for -FLT_MAX: below every real score
static long long fake(long long query, long long row) { return (query * 3 + row * 7 + 3) % 5; }   // many equal scores

struct Tables { std::vector<int> perm; std::vector<SubmTile> tiles; std::vector<SubmQuery> qd; };

// the invariants of one pass's tables; returns the pass
static SubmPass build_and_check(int pass, int nq, const std::vector<int32_t>& list_of, const std::vector<long long>& m,
                                const std::vector<const long long*>& ptr, const SubmConfig& c, Tables& t) {
    const int nb = std::min(nq - pass * c.pass_queries, c.pass_queries);
    t.perm.assign(nb, -1); t.tiles.assign(nb, SubmTile{}); t.qd.assign(nb, SubmQuery{});
    const SubmPass p = subm_build_pass(pass, nq, list_of.data(), m.data(), ptr.data(), c, t.perm.data(), t.tiles.data(), t.qd.data());
    CHECK(p.q0 == pass * c.pass_queries && p.nb == nb, "pass %d: q0 %d nb %d", pass, p.q0, p.nb);
    std::vector<int> seen(nb, 0);
    for (int pp = 0; pp < nb; ++pp) { CHECK(t.perm[pp] >= 0 && t.perm[pp] < nb, "perm[%d] = %d", pp, t.perm[pp]); if (t.perm[pp] >= 0 && t.perm[pp] < nb) ++seen[t.perm[pp]]; }
    for (int q = 0; q < nb; ++q) CHECK(seen[q] == 1, "query %d appears %d times in the permutation", q, seen[q]);
    // grouped by list, lists by (class, number), stable in query order
    for (int pp = 1; pp < nb; ++pp) {
        const int a = list_of[p.q0 + t.perm[pp - 1]], b = list_of[p.q0 + t.perm[pp]];
        const int ca = subm_class_of(c, m[a]), cb = subm_class_of(c, m[b]);
        CHECK(ca < cb || (ca == cb && (a < b || (a == b && t.perm[pp - 1] < t.perm[pp]))), "order at %d", pp);
    }
    // the tile count: the sum over the lists of ceil(queries of that list / q_tile)
    std::vector<int> per_list(m.size(), 0);
    for (int q = 0; q < nb; ++q) ++per_list[list_of[p.q0 + q]];
    long long want_tiles = 0;
    for (size_t j = 0; j < m.size(); ++j) want_tiles += subset_ceil_div(per_list[j], c.q_tile);
    CHECK(p.n_tiles == want_tiles && p.n_tiles <= subm_pass_tiles_bound(nb), "tiles %d, formula %lld", p.n_tiles, want_tiles);
    // a tile: one list, at most q_tile queries, consecutive in permuted order; every query in exactly one tile slot
    std::vector<int> in_tile(nb, 0);
    int next_p = 0;
    for (int ti = 0; ti < p.n_tiles; ++ti) {
        const SubmTile& T = t.tiles[ti];
        CHECK(T.p0 == next_p, "tile %d starts at %d, expected %d", ti, T.p0, next_p);
        int cnt = 0;
        for (int s = 0; s < kSubsetQ; ++s) {
            if (T.q[s] < 0) { for (int s2 = s; s2 < kSubsetQ; ++s2) CHECK(T.q[s2] < 0, "a gap in tile %d", ti); break; }
            CHECK(s < c.q_tile, "tile %d holds more than q_tile queries", ti);
            CHECK(T.q[s] == t.perm[T.p0 + s], "tile %d slot %d", ti, s);
            const int list = list_of[p.q0 + T.q[s]];
            CHECK(T.m == m[list] && T.ids == ptr[list], "tile %d slot %d is of another list", ti, s);
            ++in_tile[T.q[s]]; ++cnt;
        }
        CHECK(cnt >= 1, "tile %d is empty", ti);
        const int cls = subm_class_of(c, T.m);
        CHECK(T.n_rank == c.class_rows[cls] && T.n_rank >= T.m, "tile %d: n_rank %d for m %lld", ti, T.n_rank, T.m);
        CHECK(T.score_base == p.class_base[cls] + (long long)(T.p0 - p.class_first[cls]) * T.n_rank, "tile %d: score base", ti);
        CHECK(ti >= p.class_tile0[cls] && ti < p.class_tile0[cls] + p.class_tiles[cls], "tile %d outside its class's tiles", ti);
        next_p += cnt;
    }
    CHECK(next_p == nb, "tiles cover %d of %d queries", next_p, nb);
    for (int q = 0; q < nb; ++q) CHECK(in_tile[q] == 1, "query %d is in %d tile slots", q, in_tile[q]);
    // the classes: contiguous, in order, and the bounds
    long long floats = 0; int launches = 2, qsum = 0, tsum = 0;
    for (int k = 0; k < c.n_classes; ++k) {
        if (p.class_queries[k] == 0) { CHECK(p.class_tiles[k] == 0, "class %d has tiles and no query", k); continue; }
        CHECK(p.class_first[k] == qsum && p.class_tile0[k] == tsum && p.class_base[k] == floats, "class %d: first %d tile0 %d base %lld", k, p.class_first[k], p.class_tile0[k], p.class_base[k]);
        qsum += p.class_queries[k]; tsum += p.class_tiles[k]; floats += (long long)p.class_queries[k] * c.class_rows[k]; launches += 2;
    }
    CHECK(qsum == nb && tsum == p.n_tiles && floats == p.score_floats, "class sums");
    CHECK(p.launches == launches && p.launches <= subm_max_launches(c) && subm_max_launches(c) <= 10, "launches %d (bound %d)", p.launches, subm_max_launches(c));
    CHECK(p.score_floats * 4 <= subm_score_bytes_bound(c), "score bytes %lld over %lld", p.score_floats * 4, subm_score_bytes_bound(c));
    for (int pp = 0; pp < nb; ++pp) {
        const int list = list_of[p.q0 + t.perm[pp]];
        CHECK(t.qd[pp].row == p.q0 + t.perm[pp] && t.qd[pp].m == m[list] && t.qd[pp].ids == ptr[list], "query descriptor %d", pp);
    }
    return p;
}

struct Hit { long long score, id; };

static void execute(int nq, const std::vector<int32_t>& list_of, const std::vector<long long>& m, const std::vector<std::vector<long long>>& lists,
                    const SubmConfig& c, int k, const char* tag) {
    std::vector<const long long*> ptr;
    for (auto& l : lists) ptr.push_back(l.empty() ? nullptr : l.data());
    const SubmCall call = subm_call(nq, list_of.data(), (int)m.size(), m.data(), c);
    CHECK(call.verdict == kSubmOk && call.passes == subset_ceil_div(nq, c.pass_queries), "%s: verdict %d passes %d", tag, call.verdict, call.passes);
    long long rows = 0;
    for (int q = 0; q < nq; ++q) rows += m[list_of[q]];
    CHECK(call.rows == rows, "%s: rows %lld", tag, call.rows);
    std::vector<Hit> out((size_t)nq * k, Hit{1, -7});   // what the map writes; (1, -7) = never written
    Tables t;
    for (int ps = 0; ps < call.passes; ++ps) {
        const SubmPass p = build_and_check(ps, nq, list_of, m, ptr, c, t);
        std::vector<long long> scores((size_t)p.score_floats, 0);
        std::vector<int> written((size_t)p.score_floats, 0);
        // the scans: one launch per class in use, grid (blocks of n_rank, tiles of the class)
        for (int cls = 0; cls < c.n_classes; ++cls) {
            if (!p.class_queries[cls]) continue;
            const long long n_rank = c.class_rows[cls], blocks = subm_scan_blocks(n_rank, c.rows_per_wg);
            for (int ty = 0; ty < p.class_tiles[cls]; ++ty) {
                const SubmTile& T = t.tiles[p.class_tile0[cls] + ty];
                CHECK(T.n_rank == n_rank, "%s: a tile of another class in the launch", tag);
                for (long long bx = 0; bx < blocks; ++bx) {
                    const int kind = subm_wg_kind(T.m, T.n_rank, bx, c.rows_per_wg);
                    if (kind == kSubmWgNothing) continue;
                    for (int i = 0; i < c.rows_per_wg; ++i) {
                        const long long pos = bx * c.rows_per_wg + i;
                        if (kind == kSubmWgSentinels) CHECK(pos >= T.m, "%s: a sentinel workgroup holds a real position", tag);
                        if (pos >= T.n_rank) continue;
                        for (int s = 0; s < kSubsetQ; ++s) {
                            if (T.q[s] < 0) continue;
                            const long long at = subm_score_index(T, s, pos);
                            CHECK(at >= 0 && at < p.score_floats, "%s: score index %lld outside %lld", tag, at, p.score_floats);
                            if (at < 0 || at >= p.score_floats) continue;
                            const bool real = kind == kSubmWgScan && pos < T.m;
                            scores[at] = real ? fake(p.q0 + T.q[s], T.ids[pos]) : SENT;
                            ++written[at];
                        }
                    }
                }
            }
        }
        for (long long i = 0; i < p.score_floats; ++i) CHECK(written[i] == 1, "%s: score slot %lld written %d times", tag, i, written[i]);
        // the rankings: a class's rows are contiguous; each gives min(k, n_rank) positions, the rest -1
        std::vector<long long> rank_pos((size_t)p.nb * k, -1), rank_sc((size_t)p.nb * k, SENT);
        for (int cls = 0; cls < c.n_classes; ++cls) {
            const long long n_rank = c.class_rows[cls];
            for (int j = 0; j < p.class_queries[cls]; ++j) {
                const long long* row = scores.data() + p.class_base[cls] + j * n_rank;
                std::vector<long long> order(n_rank);
                for (long long i = 0; i < n_rank; ++i) order[i] = i;
                std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) { return row[a] != row[b] ? row[a] > row[b] : a < b; });
                for (long long i = 0; i < k && i < n_rank; ++i) { rank_pos[(size_t)(p.class_first[cls] + j) * k + i] = order[i]; rank_sc[(size_t)(p.class_first[cls] + j) * k + i] = row[order[i]]; }
            }
        }
        // the map: by position, never by score
        for (int pp = 0; pp < p.nb; ++pp)
            for (int i = 0; i < k; ++i) {
                const long long pos = rank_pos[(size_t)pp * k + i];
                const bool real = pos >= 0 && pos < t.qd[pp].m;
                Hit& h = out[(size_t)t.qd[pp].row * k + i];
                CHECK(h.id == -7, "%s: output (%lld, %d) written twice", tag, t.qd[pp].row, i);
                h = real ? Hit{rank_sc[(size_t)pp * k + i], t.qd[pp].ids[pos]} : Hit{SENT, -1};
            }
    }
    // brute force per query
    for (int q = 0; q < nq; ++q) {
        std::vector<Hit> want;
        for (long long id : lists[list_of[q]]) want.push_back(Hit{fake(q, id), id});
        std::stable_sort(want.begin(), want.end(), [](const Hit& a, const Hit& b) { return a.score != b.score ? a.score > b.score : a.id < b.id; });
        for (int i = 0; i < k; ++i) {
            const Hit w = i < (int)want.size() ? want[i] : Hit{SENT, -1};
            const Hit g = out[(size_t)q * k + i];
            CHECK(g.id == w.id && g.score == w.score, "%s: query %d rank %d: got (%lld, %lld), want (%lld, %lld)", tag, q, i, g.id, g.score, w.id, w.score);
        }
    }
}

static SubmConfig shrunk(int rows_per_wg, int q_tile, std::vector<long long> classes, int pass_queries) {
    SubmConfig c{};
    c.rows_per_wg = rows_per_wg; c.q_tile = q_tile; c.n_classes = (int)classes.size(); c.pass_queries = pass_queries;
    for (size_t i = 0; i < classes.size(); ++i) c.class_rows[i] = classes[i];
    c.rank_rows = classes.back();
    return c;
}

static int small() {
    const SubmConfig cfgs[] = {shrunk(2, 2, {2, 4, 16}, 2), shrunk(2, 4, {2, 4, 16}, 256), shrunk(64, 4, {4, 16}, 256), shrunk(64, 2, {2, 4, 8, 16}, 2), shrunk(2, 4, {12}, 256)};
    const long long lens[] = {0, 1, 2, 3, 5, 12}, mult[] = {5, 7, 11};
    const int ks[] = {1, 3, 12, 20};
    for (const SubmConfig& c : cfgs) CHECK(subm_config_ok(c), "a shrunken config is refused");
    for (long long la : lens) for (long long lb : lens) for (long long lc : lens) {
        const std::vector<long long> m = {la, lb, lc};
        std::vector<std::vector<long long>> lists(3);
        for (int j = 0; j < 3; ++j)
            for (long long r = 0; r < 12; ++r)
                if ((r * mult[j] + j) % 12 < m[j]) lists[j].push_back(r);   // r -> r * mult + j is a bijection mod 12: exactly m[j] rows, ascending
        for (int j = 0; j < 3; ++j) CHECK((long long)lists[j].size() == m[j], "list %d has %zu rows", j, lists[j].size());
        for (int nq = 1; nq <= 5; ++nq) {
            int total = 1;
            for (int i = 0; i < nq; ++i) total *= 3;
            for (int code = 0; code < total; ++code) {
                std::vector<int32_t> list_of(nq);
                for (int i = 0, v = code; i < nq; ++i, v /= 3) list_of[i] = v % 3;
                for (size_t ci = 0; ci < sizeof(cfgs) / sizeof(cfgs[0]); ++ci) {
                    for (int k : ks) {
                        ++cases;
                        char tag[96];
                        std::snprintf(tag, sizeof tag, "m=%lld/%lld/%lld nq=%d code=%d cfg=%zu k=%d", la, lb, lc, nq, code, ci, k);
                        execute(nq, list_of, m, lists, cfgs[ci], k, tag);
                    }
                }
            }
        }
    }
    // the same list appears under two numbers (equal content, different objects): each is scanned for itself
    for (size_t ci = 0; ci < sizeof(cfgs) / sizeof(cfgs[0]); ++ci)
        for (int k : ks) {
            std::vector<std::vector<long long>> lists = {{2, 5, 7}, {2, 5, 7}, {}};
            ++cases;
            execute(5, {0, 1, 0, 2, 1}, {3, 3, 0}, lists, cfgs[ci], k, "twins");
        }
    std::printf("subset multi plan, small: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

static int large() {
    const SubmConfig c = subm_config_default();
    CHECK(subm_config_ok(c) && c.rows_per_wg == 64 && c.q_tile == 4 && c.rank_rows == 16384 && c.pass_queries == 256 && c.n_classes <= 4, "the real constants");
    CHECK(subm_score_bytes_bound(c) == (16ll << 20) && subm_score_bytes_bound(c) == kSubmScoreBytes, "16 MB of scores");
    CHECK(subm_max_launches(c) == 10, "launches per pass: 1 + 4 + 4 + 1");
    CHECK(sizeof(SubmTile) == 64, "the tile descriptor");
    std::mt19937_64 rng(23);
    Tables t;
    for (int it = 0; it < 400; ++it) {
        const int nq = 1 + (int)(rng() % 600), n_lists = 1 + (int)(rng() % 40);
        std::vector<long long> m(n_lists);
        for (auto& v : m) {
            const int kind = (int)(rng() % 6);
            v = kind == 0 ? 0 : kind == 1 ? (long long)(rng() % 257) : kind == 2 ? 16384 - (long long)(rng() % 3) : (long long)(rng() % 16385);
        }
        if (it % 7 == 0) for (auto& v : m) v = 16384;   // every query in the largest class: the workspace bound is met exactly at 256
        std::vector<int32_t> list_of(nq);
        for (auto& v : list_of) v = (int32_t)(rng() % n_lists);
        std::vector<const long long*> ptr(n_lists, nullptr);
        const SubmCall call = subm_call(nq, list_of.data(), n_lists, m.data(), c);
        ++cases;
        CHECK(call.verdict == kSubmOk && call.passes == (nq + 255) / 256, "case %d: verdict %d", it, call.verdict);
        for (int ps = 0; ps < call.passes; ++ps) build_and_check(ps, nq, list_of, m, ptr, c, t);
        // the refusals: the lowest query that names no list; a referenced list that is too long (an unreferenced one is not looked at)
        std::vector<int32_t> bad_of = list_of;
        const int at = (int)(rng() % nq);
        bad_of[at] = (rng() & 1) ? n_lists : -1;
        const SubmCall r1 = subm_call(nq, bad_of.data(), n_lists, m.data(), c);
        CHECK(r1.verdict == kSubmBadListOf && r1.at == at && r1.value == bad_of[at], "case %d: list_of refusal", it);
        std::vector<long long> m2 = m;
        m2.push_back(16385);
        CHECK(subm_call(nq, list_of.data(), n_lists + 1, m2.data(), c).verdict == kSubmOk, "case %d: an unreferenced long list", it);
        bad_of = list_of; bad_of[at] = n_lists;
        const SubmCall r2 = subm_call(nq, bad_of.data(), n_lists + 1, m2.data(), c);
        CHECK(r2.verdict == kSubmTooLong && r2.at == n_lists && r2.value == 16385, "case %d: too-long refusal", it);
    }
    CHECK(subm_class_of(c, 0) == 0 && subm_class_of(c, 256) == 0 && subm_class_of(c, 257) == 1 && subm_class_of(c, 16384) == c.n_classes - 1, "class bounds");
    CHECK(subm_check_list(subm_check_key(70000, 16383)) == 70000 && subm_check_pos(subm_check_key(70000, 16383)) == 16383, "the check key");
    CHECK(subm_check_key(0, 5) < subm_check_key(1, 0) && subm_check_key(3, 4) < subm_check_key(3, 5) && subm_check_key(65535, 16383) < ~0ull, "the check key's order");
    std::printf("subset multi plan, large: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "small")) return small();
    if (argc == 2 && !std::strcmp(argv[1], "large")) return large();
    std::printf("usage: %s small|large\n", argv[0]);
    return 2;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "subset_multi_plan.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "subset_multi_plan")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def run(exe: str, what: str):
    return subprocess.run([exe, what], capture_output=True, text=True, timeout=600, env=_ENV)
