"""A host-compiled driver of the metadata filter's program and output geometry (veritasfi_amd/csrc/vf_where.h), used by
tests/test_where_plan.py.

The header is plain C++17 without HIP, so the host compiler reads it as it stands, under UBSan.  The program is stand-alone:

  driver programs   every program shape of up to 3 leaves (with and without NOT, both operators, both bracketings) over a pool of interval,
                    empty-interval, set and missing leaves, run by where_eval_row -- the interpreter the kernel runs -- on each row of a
                    12-row, 2-column table under all 4096 validity patterns (keys vary with the pattern), and held to a recursive
                    evaluation of the same expression on plain bools; every program also passes where_validate
  driver tiles      tiles of 64, 128 and 1024 rows at n = 1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025 under five row patterns: the
                    kernels' walk (a ballot word per 64 rows, a count per tile, the exclusive prefix, ids through where_rank_in_tile) is
                    held to a plain loop: word count, zero tail bits, counts, prefix, m, every id's position
  driver validate   where_validate: stack underflow, leftover stack, depth 33 (and 32), a leaf naming column 16, a set run that is not
                    ascending or leaves set_values, an unknown op, a leaf index past the program's, every limit

Each prints the number of cases and the first failures, and returns 1 if there was one."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "veritasfi_amd", "csrc")

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "vf_where.h"
using namespace vf;

static long long failures = 0, cases = 0;
#define CHECK(c, ...) do { if (!(c)) { if (failures < 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

static const int64_t SETS[] = {0, 2, /**/ 1, /**/ -1, 1, 3};   // three runs: [0, 2), [2, 3), [3, 6)
static const WhereLeaf POOL[] = {
    {kWhereInterval, 0, 0, 1}, {kWhereInterval, 1, 2, 2}, {kWhereInterval, 0, 1, 0} /* empty */, {kWhereSet, 1, 0, 2}, {kWhereMissing, 0, 0, 0},
    {kWhereSet, 0, 3, 3}, {kWhereMissing, 1, 0, 0}, {kWhereInterval, 1, INT64_MIN, 0}, {kWhereSet, 0, 2, 1}, {kWhereInterval, 0, -1, INT64_MAX},
};
static const int NPOOL = 10;

struct Row { int64_t key[2]; bool valid[2]; };

static bool leaf_plain(const WhereLeaf& l, const Row& r) {
    if (l.kind == kWhereMissing) return !r.valid[l.column];
    if (!r.valid[l.column]) return false;
    if (l.kind == kWhereInterval) return l.lo <= r.key[l.column] && r.key[l.column] <= l.hi;
    for (int64_t j = l.lo; j < l.lo + l.hi; ++j) if (SETS[j] == r.key[l.column]) return true;
    return false;
}

// an expression over up to three pool leaves: shape 0: a; 1: a o1 b; 2: (a o1 b) o2 c; 3: a o1 (b o2 c); nots: bit 0 negates a, 1 b, 2 c, 3 the whole
struct Expr { int shape, a, b, c, o1, o2, nots; };

static bool plain(const Expr& e, const Row& r) {
    bool A = leaf_plain(POOL[e.a], r) ^ bool(e.nots & 1), B = false, C = false, v;
    if (e.shape >= 1) B = leaf_plain(POOL[e.b], r) ^ bool(e.nots & 2);
    if (e.shape >= 2) C = leaf_plain(POOL[e.c], r) ^ bool(e.nots & 4);
    auto ap = [](int o, bool x, bool y) { return o == kWhereAnd ? (x && y) : (x || y); };
    if (e.shape == 0) v = A;
    else if (e.shape == 1) v = ap(e.o1, A, B);
    else if (e.shape == 2) v = ap(e.o2, ap(e.o1, A, B), C);
    else v = ap(e.o1, A, ap(e.o2, B, C));
    return v ^ bool(e.nots & 8);
}

static std::vector<uint8_t> postfix(const Expr& e) {
    std::vector<uint8_t> p;
    auto leaf = [&](int i, int bit) { p.push_back((uint8_t)i); if (e.nots & bit) p.push_back((uint8_t)kWhereNot); };
    leaf(e.a, 1);
    if (e.shape == 1) { leaf(e.b, 2); p.push_back((uint8_t)e.o1); }
    if (e.shape == 2) { leaf(e.b, 2); p.push_back((uint8_t)e.o1); leaf(e.c, 4); p.push_back((uint8_t)e.o2); }
    if (e.shape == 3) { leaf(e.b, 2); leaf(e.c, 4); p.push_back((uint8_t)e.o2); p.push_back((uint8_t)e.o1); }
    if (e.nots & 8) p.push_back((uint8_t)kWhereNot);
    return p;
}

static void run_expr(const Expr& e, const std::vector<Row>& tables) {
    const std::vector<uint8_t> ops = postfix(e);
    const WhereVerdict v = where_validate(POOL, NPOOL, ops.data(), (int)ops.size(), 2, SETS, 6);
    CHECK(v.verdict == kWhereOk, "shape %d leaves %d %d %d: verdict %d at %lld", e.shape, e.a, e.b, e.c, v.verdict, v.at);
    for (size_t i = 0; i < tables.size(); ++i) {
        const Row& r = tables[i];
        const bool got = where_eval_row(POOL, ops.data(), (int)ops.size(), SETS, [&](int c) { return r.key[c]; }, [&](int c) { return r.valid[c]; });
        ++cases;
        CHECK(got == plain(e, r), "shape %d leaves %d %d %d ops %x %x nots %d, table row %zu", e.shape, e.a, e.b, e.c, e.o1, e.o2, e.nots, i);
    }
}

static int programs() {
    // 4096 validity patterns of a 12-row, 2-column table: bit r of p is column 0's validity of row r, column 1's is a mix of p; keys in -1 .. 3
    std::vector<Row> tables;
    for (unsigned p = 0; p < 4096; ++p)
        for (unsigned r = 0; r < 12; ++r) {
            Row row;
            row.valid[0] = (p >> r) & 1u;
            row.valid[1] = ((p * 2654435761u) >> (7 + r)) & 1u;
            row.key[0] = (int64_t)(((p >> (r % 7)) + r * 2u) % 5u) - 1;
            row.key[1] = (int64_t)(((p >> (r % 5)) + r * 3u + 1u) % 5u) - 1;
            tables.push_back(row);
        }
    const int ops2[2] = {kWhereAnd, kWhereOr};
    for (int a = 0; a < NPOOL; ++a)
        for (int nots = 0; nots < 16; nots += 1) if (!(nots & 6)) run_expr(Expr{0, a, 0, 0, 0, 0, nots}, tables);
    for (int a = 0; a < 6; ++a) for (int b = 0; b < 6; ++b) for (int o = 0; o < 2; ++o)
        for (int nots = 0; nots < 16; ++nots) if (!(nots & 4)) run_expr(Expr{1, a, b, 0, ops2[o], 0, nots}, tables);
    for (int shape = 2; shape <= 3; ++shape)
        for (int a = 0; a < 5; ++a) for (int b = 0; b < 5; ++b) for (int c = 3; c < 8; ++c) for (int o = 0; o < 4; ++o)
            run_expr(Expr{shape, a, b, c, ops2[o & 1], ops2[o >> 1], (a + 2 * b + 3 * c + o) & 15}, tables);
    std::printf("where programs: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

static bool pattern_bit(int pattern, long long r, long long n) {
    switch (pattern) {
        case 0: return true;
        case 1: return false;
        case 2: return r & 1;
        case 3: return r == 0 || r == n - 1 || r % 64 == 63 || r % 64 == 0;
        default: return ((r * 2654435761ull) >> 13) % 3 == 0;
    }
}

static int tiles() {
    const int tile_rows[] = {64, 128, 1024};
    const long long ns[] = {1, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025};
    for (int tr : tile_rows) for (long long n : ns) for (int pattern = 0; pattern < 5; ++pattern) {
        ++cases;
        CHECK(where_tile_rows_ok(tr), "tile_rows %d", tr);
        // the column: key 1 where the pattern passes, key 0 elsewhere, every third row invalid under pattern 4 (then it fails)
        std::vector<int64_t> keys(n); std::vector<char> valid(n, 1), want(n);
        for (long long r = 0; r < n; ++r) {
            keys[r] = pattern_bit(pattern, r, n) ? 1 : 0;
            if (pattern == 4 && r % 3 == 1) valid[r] = 0;
            want[r] = keys[r] == 1 && valid[r];
        }
        const WhereLeaf leaf{kWhereInterval, 0, 1, 1};
        const uint8_t ops[1] = {0};
        // k_where_eval's walk: a workgroup per tile, a ballot per 64 rows, steps wholly past n write nothing
        const long long words = where_bitmap_words(n), tiles_n = where_tiles(n, tr), steps = tr / kWhereWaveRows;
        CHECK(words == 2 * ((n + 63) / 64) && tiles_n == (n + tr - 1) / tr, "n %lld tile %d: geometry", n, tr);
        std::vector<uint32_t> bitmap(words, 0xDEADBEEFu);
        std::vector<char> written(words, 0);
        std::vector<uint32_t> counts(tiles_n, 0xDEADBEEFu);
        for (long long t = 0; t < tiles_n; ++t) {
            uint32_t count = 0;
            for (long long s = 0; s < steps; ++s) {
                const long long g = t * steps + s;
                if (g * kWhereWaveRows >= n) break;
                uint64_t bits = 0;
                for (int lane = 0; lane < 64; ++lane) {
                    const long long row = g * kWhereWaveRows + lane;
                    bool pass = false;
                    if (row < n) pass = where_eval_row(&leaf, ops, 1, (const int64_t*)nullptr, [&](int) { return keys[row]; }, [&](int) { return valid[row] != 0; });
                    if (pass) bits |= 1ull << lane;
                }
                CHECK(2 * g + 1 < words, "n %lld tile %d: word %lld of %lld", n, tr, 2 * g + 1, words);
                bitmap[2 * g] = (uint32_t)bits; bitmap[2 * g + 1] = (uint32_t)(bits >> 32);
                ++written[2 * g]; ++written[2 * g + 1];
                count += (uint32_t)where_popcount64(bits);
            }
            counts[t] = count;
        }
        // k_where_scan
        std::vector<long long> prefix(tiles_n);
        long long m = 0;
        for (long long t = 0; t < tiles_n; ++t) { prefix[t] = m; m += counts[t]; }
        // held to the plain loop
        std::vector<long long> plain_ids;
        for (long long r = 0; r < n; ++r) if (want[r]) plain_ids.push_back(1000 + r);
        CHECK(m == (long long)plain_ids.size(), "n %lld tile %d pattern %d: m %lld, plain %zu", n, tr, pattern, m, plain_ids.size());
        for (long long w = 0; w < words; ++w) CHECK(written[w] == 1, "n %lld tile %d: word %lld written %d times", n, tr, w, (int)written[w]);
        for (long long r = 0; r < words * 32; ++r)
            CHECK(where_bit(bitmap.data(), r) == (r < n && want[r]), "n %lld tile %d pattern %d: bit %lld", n, tr, pattern, r);
        for (long long t = 0; t < tiles_n; ++t) {
            long long c = 0;
            for (long long r = t * tr; r < n && r < (t + 1) * tr; ++r) c += want[r];
            CHECK(counts[t] == c, "n %lld tile %d: count of tile %lld", n, tr, t);
        }
        // k_where_ids: the rank rule
        std::vector<long long> ids(m > 0 ? m : 1, -1);
        for (long long r = 0; r < n; ++r) {
            if (!where_bit(bitmap.data(), r)) continue;
            const long long at = prefix[where_tile_of(r, tr)] + where_rank_in_tile(bitmap.data(), r, tr);
            CHECK(at >= 0 && at < m, "n %lld tile %d: row %lld goes to %lld of %lld", n, tr, r, at, m);
            if (at >= 0 && at < m) { CHECK(ids[at] == -1, "position %lld written twice", at); ids[at] = 1000 + r; }
        }
        for (long long i = 0; i < m; ++i) CHECK(ids[i] == plain_ids[i], "n %lld tile %d pattern %d: ids[%lld] = %lld, plain %lld", n, tr, pattern, i, ids[i], plain_ids[i]);
    }
    CHECK(!where_tile_rows_ok(0) && !where_tile_rows_ok(32) && !where_tile_rows_ok(96 + 1) && !where_tile_rows_ok(2048) && where_tile_rows_ok(192), "tile_rows rule");
    const WhereBlock b = where_block(16, 64, 128, 65536);
    CHECK(b.columns_at == 0 && b.leaves_at == 256 && b.ops_at == 256 + 1536 && b.sets_at == 256 + 1536 + 128 + 128 && b.bytes == b.sets_at + 65536 * 8, "the descriptor block");
    std::printf("where tiles: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

static WhereVerdict val(const std::vector<WhereLeaf>& l, const std::vector<uint8_t>& o, int cols, const std::vector<int64_t>& s) {
    ++cases;
    return where_validate(l.data(), (int)l.size(), o.data(), (int)o.size(), cols, s.data(), (long long)s.size());
}

static int validate() {
    const uint8_t A = kWhereAnd, O = kWhereOr, N = kWhereNot;
    const std::vector<WhereLeaf> two = {{kWhereInterval, 0, 0, 5}, {kWhereMissing, 1, 0, 0}};
    const std::vector<int64_t> none;
    WhereVerdict v = val(two, {0, 1, A, N}, 2, none);
    CHECK(v.verdict == kWhereOk, "a good program: %d", v.verdict);
    v = val(two, {0, A}, 2, none);
    CHECK(v.verdict == kWhereUnderflow && v.at == 1, "AND on one value: %d at %lld", v.verdict, v.at);
    v = val(two, {N, 0}, 2, none);
    CHECK(v.verdict == kWhereUnderflow && v.at == 0, "NOT on nothing: %d at %lld", v.verdict, v.at);
    v = val(two, {0, 1, O, O}, 2, none);
    CHECK(v.verdict == kWhereUnderflow && v.at == 3, "a second OR: %d at %lld", v.verdict, v.at);
    v = val(two, {0, 1}, 2, none);
    CHECK(v.verdict == kWhereLeftover && v.at == 2, "leftover stack: %d at %lld", v.verdict, v.at);
    v = val(two, {0, 1, 0, A}, 2, none);
    CHECK(v.verdict == kWhereLeftover && v.at == 2, "leftover stack after an op: %d at %lld", v.verdict, v.at);
    // depth: 32 pushes then 31 ANDs is the deepest program; one more push is refused at that push
    std::vector<uint8_t> deep(32, 0);
    for (int i = 0; i < 31; ++i) deep.push_back(A);
    v = val(two, deep, 2, none);
    CHECK(v.verdict == kWhereOk, "depth 32: %d at %lld", v.verdict, v.at);
    deep.assign(33, 0);
    for (int i = 0; i < 32; ++i) deep.push_back(A);
    v = val(two, deep, 2, none);
    CHECK(v.verdict == kWhereOverLimits && v.limit == kWhereLimitDepth && v.at == 32, "depth 33: %d limit %d at %lld", v.verdict, v.limit, v.at);
    // leaves
    v = val({{kWhereInterval, 16, 0, 0}}, {0}, 16, none);
    CHECK(v.verdict == kWhereBadLeaf && v.at == 0, "a leaf naming column 16 of 16: %d", v.verdict);
    v = val({{kWhereInterval, 0, 0, 0}, {kWhereInterval, -1, 0, 0}}, {0}, 16, none);
    CHECK(v.verdict == kWhereBadLeaf && v.at == 1, "a leaf naming column -1: %d", v.verdict);
    v = val({{3, 0, 0, 0}}, {0}, 1, none);
    CHECK(v.verdict == kWhereBadLeaf, "a leaf of kind 3: %d", v.verdict);
    v = val({{kWhereSet, 0, 0, 3}}, {0}, 1, {1, 5, 5});
    CHECK(v.verdict == kWhereSetNotAscending && v.at == 2, "a run that repeats: %d at %lld", v.verdict, v.at);
    v = val({{kWhereSet, 0, 1, 2}}, {0}, 1, {9, 5, 4});
    CHECK(v.verdict == kWhereSetNotAscending && v.at == 2, "a run that descends: %d at %lld", v.verdict, v.at);
    v = val({{kWhereSet, 0, 0, 2}, {kWhereSet, 0, 2, 2}}, {0}, 1, {1, 5, 0, 3});
    CHECK(v.verdict == kWhereOk, "two ascending runs, the second starting lower: %d", v.verdict);
    v = val({{kWhereSet, 0, 2, 2}}, {0}, 1, {1, 5, 7});
    CHECK(v.verdict == kWhereBadSetRun && v.at == 0, "a run past set_values: %d", v.verdict);
    v = val({{kWhereSet, 0, INT64_MAX, INT64_MAX}}, {0}, 1, {1});
    CHECK(v.verdict == kWhereBadSetRun, "a run whose end overflows: %d", v.verdict);
    v = val({{kWhereSet, 0, -1, 1}}, {0}, 1, {1});
    CHECK(v.verdict == kWhereBadSetRun, "a run before set_values: %d", v.verdict);
    // ops
    v = val(two, {0, 2, A}, 2, none);
    CHECK(v.verdict == kWhereBadOp && v.at == 1, "leaf 2 of 2: %d at %lld", v.verdict, v.at);
    v = val(two, {0, 0x83}, 2, none);
    CHECK(v.verdict == kWhereBadOp && v.at == 1, "op 0x83: %d at %lld", v.verdict, v.at);
    // emptiness and the limits
    CHECK(val(two, {}, 2, none).verdict == kWhereEmpty && val({}, {0}, 2, none).verdict == kWhereEmpty && val(two, {0}, 0, none).verdict == kWhereEmpty, "empty programs");
    const std::vector<WhereLeaf> many(65, WhereLeaf{kWhereInterval, 0, 0, 0});
    v = val(many, {0}, 1, none);
    CHECK(v.verdict == kWhereOverLimits && v.limit == kWhereLimitLeaves && v.at == 65, "65 leaves: %d", v.verdict);
    CHECK(val(std::vector<WhereLeaf>(64, WhereLeaf{kWhereInterval, 0, 0, 0}), {63}, 1, none).verdict == kWhereOk, "64 leaves");
    std::vector<uint8_t> long_ops = {0};
    for (int i = 0; i < 128; ++i) long_ops.push_back(N);
    v = val(two, long_ops, 2, none);
    CHECK(v.verdict == kWhereOverLimits && v.limit == kWhereLimitOps && v.at == 129, "129 ops: %d", v.verdict);
    long_ops.pop_back();
    CHECK(val(two, long_ops, 2, none).verdict == kWhereOk, "128 ops");
    v = val(two, {0}, 17, none);
    CHECK(v.verdict == kWhereOverLimits && v.limit == kWhereLimitColumns, "17 columns: %d", v.verdict);
    std::vector<int64_t> big(65537);
    for (size_t i = 0; i < big.size(); ++i) big[i] = (int64_t)i;
    v = val({{kWhereSet, 0, 0, 65537}}, {0}, 1, big);
    CHECK(v.verdict == kWhereOverLimits && v.limit == kWhereLimitSetValues, "65537 set values: %d", v.verdict);
    big.pop_back();
    CHECK(val({{kWhereSet, 0, 0, 65536}}, {0}, 1, big).verdict == kWhereOk, "65536 set values");
    CHECK(kWhereMaxLeaves == 64 && kWhereMaxOps == 128 && kWhereMaxDepth == 32 && kWhereMaxColumns == 16 && kWhereMaxSetValues == 65536 && kWhereTileRows == 1024, "the limits");
    // where_in_run at every length up to 9 and a long run
    for (int len = 0; len <= 9; ++len) {
        std::vector<int64_t> run(len);
        for (int i = 0; i < len; ++i) run[i] = 3 * i - 4;
        for (int64_t key = -6; key < 3 * len; ++key) {
            bool in = false;
            for (int i = 0; i < len; ++i) in |= run[i] == key;
            ++cases;
            CHECK(where_in_run(run.data(), len, key) == in, "run of %d, key %lld", len, (long long)key);
        }
    }
    CHECK(where_in_run(big.data(), 65536, 65535) && where_in_run(big.data(), 65536, 0) && !where_in_run(big.data(), 65536, 65536) && !where_in_run(big.data(), 65536, -1), "a long run");
    std::printf("where validate: %lld cases, %lld failure(s)\n", cases, failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "programs")) return programs();
    if (argc == 2 && !std::strcmp(argv[1], "tiles")) return tiles();
    if (argc == 2 && !std::strcmp(argv[1], "validate")) return validate();
    std::printf("usage: %s programs|tiles|validate\n", argv[0]);
    return 2;
}
"""

_ENV = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(tmp_dir) -> str:
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    assert os.path.exists(cxx), "no host C++ compiler (g++, clang++ or ROCm's clang++)"
    src = os.path.join(str(tmp_dir), "where_plan.cc")
    with open(src, "w") as f:
        f.write(DRIVER)
    exe = os.path.join(str(tmp_dir), "where_plan")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe])
    return exe


def run(exe: str, what: str):
    return subprocess.run([exe, what], capture_output=True, text=True, timeout=600, env=_ENV)
