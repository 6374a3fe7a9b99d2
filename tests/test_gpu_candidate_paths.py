"""Every narrow main-scan kernel driven through the three regimes of the candidate path it shares with the others (tile_epilogue's
stage in vf_kernels.hip: LDS stage -> direct append to the query's global list when the stage is full -> flag 2 and the exact repair
when the list is full), at 20 037 to 40 037 rows.  Every search is compared bit for bit (ids and score bits) with oracle.search on the
stored values, and every cell carries a WITNESS that the regime it names really ran -- the results alone cannot tell, because the exact
repair makes a wrong overflow invisible and a row lost in the direct append shows only if that branch is reached.

The witnesses use what the host knows of a search: grid, stage_cap, cap, kprime, passes, samp and total_waves come from the
host-compiled route driver (tests/scan_route_driver.py = vf_route.h, with the CU count of the device and the CU split the library
reports), none is re-derived here.

Regime 1, the stage fills, the lists hold, nothing is repaired.  k_scan, k_scan2, k_scan2r, k_scan_ksplit and ks8_body (k_scan_ksplit8 /
k_scan_ksplit8i) flush a workgroup's stage ONCE, after the tile loop (read in vf_kernels.hip: the `MODE == kModeMain` block that ends
k_scan and k_scan_ksplit, ks_flush as ks8_body's last statement, the blocks "flush the staged candidates" that end k_scan2 and
k_scan2r; no narrow kernel flushes early -- only k_scan_wide / k_scan_wide8 do, and they are not in this table).  So a workgroup moves at
most stage_cap entries through its stage per pass, and
    candidates > passes x grid x stage_cap                                               (the witness as the issue states it)
means by pigeonhole that some workgroup staged more than its stage holds.  But `candidates` also counts the rows k_sel0 emits from the
sample pass as each list's first entries, and those never pass through a stage.  They are sample rows, at most total_waves x samp per
query, so the STRICT witness is
    candidates - n_queries x total_waves x samp > passes x grid x stage_cap.
With the default sampling (a quarter of 20 037 rows is sample) that subtraction leaves nothing provable, so every regime-1 cell runs
twice: (A) the default plan with the witness as stated, (B) options waves = 128 and sample_rows = 1 (16 workgroups, 128 sample rows per
query: both are speed settings the fuzz draws too) with the strict witness (k_scan_ksplit8i has no (B) at deep k: CELLS says why; the
ramp below is its strict witness).  For both, the inequality is first asserted on the CPU from
a lower bound on `candidates` that holds for ANY correct scan:
  * count-based routes, k = 2048: every row at or above a query's true k'-th best score is a candidate whatever the thresholds did, so
    candidates >= nq x kprime.  N(0, 1) rows, so no certificate fails.
  * image route (k <= 128, band-based): T identical rows that are the best match of every query of a near-identical family all tie with
    the k-th best, so all lie in the band: candidates >= nq x T.  The block sits at the corpus's start, at its end (across the ragged
    last tile) and scattered.
A third data shape, rows in ascending score order (the thresholds rise through the scan), has no CPU bound -- its count depends on what
the sample saw -- and asserts the strict witness on the GPU's own figures only, under waves = 64.

Regime 2, a list overflows and the repair answers: a duplicate block larger than cap (33 000 rows of 40 037 on the image route, whose
lists hold 32 768; cap + 800 on the count-based routes at k = 100) that is the best match of a family at the edges of the query tiles
(0, 31, 32, 63), among queries that see the block BELOW every other row (random directions bent to a cosine of -0.3 with it, so that the
block is no candidate of theirs: otherwise their lists overflow as well and `overflowed` counts nothing).
Regime 3, two passes with overflow in both (byte rows, 70 queries = 64 + 6, family at 63, 64, 69).
Both assert max_candidates > cap, overflowed == the family's size, exact_reruns == uncertified + overflowed, and every query's result.

The second part runs a FIXED number of cases of tools/fuzz_search.py's `int8` and `wide_rows` profiles (seeds chosen with the route
driver so that the routes named there are all met)."""
import importlib.util
import os

import numpy as np
import pytest

import scan_route_driver as drv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20_037          # not a whole number of 32-row tiles
N_OVER = 40_037     # the image route's regime 2 / 3: 33 000 copies beside 7 037 other rows
T_BLOCK = 3000      # the image route's regime-1 block: below k_final's 4096-entry survivor area (see test_stage_fills_lists_hold)
STAT_KEYS = ("path", "scan_kernel", "scan_image", "candidates", "max_candidates", "uncertified", "overflowed", "exact_reruns")
STRICT = {"waves": 128, "sample_rows": 1}   # variant (B): 16 workgroups, 128 sample rows per query


class Cell:
    def __init__(self, name, dtype, d, options, route, n=N, deep=None):
        self.name, self.dtype, self.d, self.options, self.route, self.n = name, dtype, d, options, route, n
        self.image = route[2] == 1
        self.deep = deep or ({}, STRICT)    # the options of the deep-k search's variants (A) and (B)

    def __repr__(self):
        return self.name


# (stats path, scan_kernel, scan_image) as the issue's table names them
CELLS = [
    Cell("k_scan-f16-100", "f16", 100, {"scan_impl": 1}, (1, 1, 0)),
    Cell("k_scan-f16-768", "f16", 768, {"scan_impl": 1}, (1, 1, 0)),
    Cell("k_scan-e4m3-768", "e4m3", 768, {}, (1, 1, 0)),
    Cell("k_scan-int8-768", "int8", 768, {"scan_image": 0}, (1, 1, 0)),
    Cell("k_scan2-f16-768", "f16", 768, {}, (1, 2, 0)),
    Cell("k_scan2r-f16-768", "f16", 768, {"scan_impl": 5}, (1, 5, 0)),
    Cell("k_scan2r-f16-1024", "f16", 1024, {"scan_impl": 5}, (1, 5, 0)),
    Cell("k_scan2r-e4m3-768", "e4m3", 768, {"scan_impl": 5}, (1, 5, 0)),
    Cell("k_scan2r-image-mfma0", "int8", 768, {"scan_image": 2, "image_mfma": 0}, (1, 5, 1)),
    Cell("k_scan2r-image-mfma1", "int8", 768, {"scan_image": 2, "image_mfma": 1}, (1, 5, 1)),
    Cell("k_scan2r-image-mfma2", "int8", 768, {"scan_image": 2, "image_mfma": 2}, (1, 5, 1)),
    Cell("k_scan_ksplit-f16-2560", "f16", 2560, {"wide_rows": 2}, (1, 6, 0)),
    Cell("k_scan_ksplit8-e4m3-2560", "e4m3", 2560, {"wide_rows": 2}, (1, 7, 0)),
    # 32 773 rows (the kernel serves int8 rows from 32 768): 64 workgroups by default, and 32 x k' = 81 920 entries do not exceed 64 stages;
    # they exceed 32 (waves = 256).  With that option alone the plan sizes the lists at 16 384 and 18 of the 32 overflowed (max 21 448,
    # measured: repaired, so exact, but not this regime); sample_rows = 64 seeds tighter thresholds and the lists hold (max 5 437).
    # NO variant (B) at deep k for this kernel: its CPU bound needs fewer sample rows than k', and a scan that starts without a seeded
    # threshold may append every row of the shard to a list (the other cells show max_candidates = n under (B)) -- 32 773 rows, five
    # more than the longest list holds.  Measured: max_candidates = 32 773 with 32 workgroups, 31 796 with 8, 29 635 with one, so
    # whether a list overflows is a matter of timing there.  This kernel's strict witness is the ramp's (seeded, k = 100).
    Cell("k_scan_ksplit8i-int8-2560", "int8", 2560, {}, (1, 7, 0), n=32_773, deep=({"waves": 256, "sample_rows": 64}, None)),
]
BYTE_CELLS = [c for c in CELLS if c.image or c.name == "k_scan2r-e4m3-768"]   # regime 3


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()  # raises if the HIP library is missing: no fallback
    n = _ffi.c_i32(0)
    _ffi.check(_ffi.lib().vf_device_count(n), "vf_device_count")
    assert n.value >= 1, "no GPU visible"
    return m


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("scan_route"))


@pytest.fixture(scope="module")
def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(want, got, what):
    (wi, ws), (gi, gs) = want, got
    assert wi.shape == gi.shape and ws.shape == gs.shape, (what, wi.shape, gi.shape)
    bad = np.nonzero((wi != gi).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:8].tolist()} (first: got {gi[bad[0]][:8]}, want {wi[bad[0]][:8]})"
    assert np.array_equal(_bits(ws), _bits(gs)), f"{what}: score bits differ, max |diff| = {float(np.max(np.abs(ws - gs)))}"


def _store(vf, dtype, x):
    """fp32 values -> (what the index is built from, the stored values the oracle scores)."""
    if dtype == "f16":
        r = x.astype(np.float16)
        return r, r
    if dtype == "int8":
        c = vf.quantize_int8(x)
        return c, c.astype(np.float32)
    import torch
    from oracle import ref_numpy
    codes = torch.from_numpy(np.clip(x * 0.5, -400, 400)).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    return codes, ref_numpy.decode_e4m3(codes).astype(np.float16)   # exact: the decoded values ARE the corpus


def _open(vf, cell, payload, options):
    ix = vf.DenseIndex.from_e4m3(payload) if cell.dtype == "e4m3" else (vf.DenseIndex.from_int8(payload) if cell.dtype == "int8" else vf.DenseIndex(payload))
    for name, value in {**cell.options, **options}.items():
        ix.set_option(name, value)
    return ix


def _routed(driver, n_cu, cell, n, nq, k, options, st):
    case = dict(dtype=cell.dtype, n=n, d=cell.d, nq=nq, k=k, n_cu=n_cu, has_image=1 if cell.image else 0, aux_applied=st["aux_cus"],
                **{**cell.options, **options})
    return drv.evaluate(driver, [case])[0]


def _tiles(driver, n_cu, cell):
    """Query counts to run: the 32-query tile, and the 64-query tile where a pass serves 64 (the driver's per_pass)."""
    r = drv.evaluate(driver, [dict(dtype=cell.dtype, n=cell.n, d=cell.d, nq=32, k=100, n_cu=n_cu, has_image=1 if cell.image else 0, **cell.options)])[0]
    assert r["path"] == 1 and not r["wide"] and r["per_pass"] in (32, 64), r
    return (32, 64) if r["per_pass"] == 64 else (32,)


def _search(vf, driver, n_cu, cell, payload, n, q, k, options, what):
    with _open(vf, cell, payload, options) as ix:
        got = ix.search(q, k)
        st = ix.stats()
    r = _routed(driver, n_cu, cell, n, q.shape[0], k, options, st)
    assert (st["path"], st["scan_kernel"], st["scan_image"]) == cell.route, (what, st)
    assert (r["path"], r["scan_kernel"], r["scan_image"]) == cell.route and not r["wide"], (what, r)
    return got, st, r


def _figures(what, st, r, nq):
    seeds = nq * r["total_waves"] * r["samp"]
    print(f"{what}: candidates={st['candidates']} max_candidates={st['max_candidates']} passes x grid x stage_cap={r['passes']}x{r['grid']}x{r['stage_cap']}"
          f"={r['passes'] * r['grid'] * r['stage_cap']} seeds<={seeds} cap={r['cap']} kprime={r['kprime']} uncertified={st['uncertified']} "
          f"overflowed={st['overflowed']} exact_reruns={st['exact_reruns']}")
    return seeds


def _assert_stage_filled(what, st, r, nq, strict, cpu_bound=None):
    """Regime 1's witness (see the module's text), on the CPU's lower bound first where there is one, then on the GPU's count."""
    seeds = _figures(what, st, r, nq)
    stages = r["passes"] * r["grid"] * r["stage_cap"]
    through = (lambda c: c - seeds) if strict else (lambda c: c)
    if cpu_bound is not None:
        assert through(cpu_bound) > stages, f"{what}: the construction does not prove a full stage ({cpu_bound} - {seeds if strict else 0} <= {stages})"
        assert st["candidates"] >= cpu_bound, f"{what}: fewer candidates than any correct scan appends ({st['candidates']} < {cpu_bound})"
    assert through(st["candidates"]) > stages, f"{what}: no workgroup's stage need have filled ({st['candidates']}, seeds <= {seeds}, stages {stages})"
    assert st["max_candidates"] <= r["cap"], f"{what}: a list overflowed ({st['max_candidates']} > {r['cap']})"
    assert st["overflowed"] == 0 and st["exact_reruns"] == 0, f"{what}: the scan did not answer alone: {st}"


# ---- the corpora, built once each ----------------------------------------------------------------------------------------------------------
_cache = {}


def _base(n, d):
    key = ("base", n, d)
    if key not in _cache:
        _cache[key] = np.random.default_rng(5000 + d).standard_normal((n, d)).astype(np.float32)
    return _cache[key]


def _family(d, m, seed):
    """q0 and m distinct near-copies of it: q0 + 0.02 noise."""
    rng = np.random.default_rng(seed)
    q0 = rng.standard_normal(d).astype(np.float32)
    return q0, (q0[None, :] + 0.02 * rng.standard_normal((m, d)).astype(np.float32)).astype(np.float32)


def _deep_case(vf, oracle, cell):
    """N(0, 1) rows and 64 N(0, 1) queries with the oracle's top 2048 (the best k of them are the result for a smaller k)."""
    key = ("deep", cell.dtype, cell.d, cell.n)
    if key not in _cache:
        payload, stored = _store(vf, cell.dtype, _base(cell.n, cell.d))
        q = np.random.default_rng(6000 + cell.d).standard_normal((64, cell.d)).astype(np.float32)
        _cache[key] = (payload, q, oracle.search(stored, q, 2048))
    return _cache[key]


def _block_case(vf, oracle, cell, n, size, where, m):
    """`size` identical rows -- q0's own values -- among N(0, 1) rows, and the family of q0 (m queries) whose best match they are."""
    key = ("block", cell.dtype, cell.d, n, size, where)
    if key not in _cache:
        q0, fam = _family(cell.d, 64, 7000 + cell.d)
        x = _base(n, cell.d).copy()
        at = {"start": np.arange(size), "end": np.arange(n - size, n),
              "scattered": np.sort(np.random.default_rng(7100).choice(n, size, replace=False))}[where]
        x[at] = q0
        payload, stored = _store(vf, cell.dtype, x)
        stored32 = stored.astype(np.float32)
        assert (stored32[at] == stored32[at[0]]).all()                      # the copies are identical as stored
        cos = oracle.cosine(fam, stored32)
        others = np.ones(n, bool)
        others[at] = False
        assert (cos[:, at[0]] > cos[:, others].max(axis=1)).all(), "the block must outrank every other row for each family query"
        _cache[key] = (payload, stored32, at, q0, fam)
    payload, stored32, at, q0, fam = _cache[key]
    return payload, stored32, at, q0, fam[:m]


def _ramp_case(vf, oracle, cell):
    """N(0, 1) rows in ascending order of their score for q0, and q0's family."""
    key = ("ramp", cell.dtype, cell.d, cell.n)
    if key not in _cache:
        q0, fam = _family(cell.d, 64, 8000 + cell.d)
        _, stored = _store(vf, cell.dtype, _base(cell.n, cell.d))
        order = np.argsort(oracle.cosine(q0[None, :], stored.astype(np.float32))[0], kind="stable")
        payload, stored = _store(vf, cell.dtype, _base(cell.n, cell.d)[order])
        _cache[key] = (payload, fam, oracle.search(stored, fam, 100))
    return _cache[key]


def _cut(full, sel, k):
    return np.ascontiguousarray(full[0][sel, :k]), np.ascontiguousarray(full[1][sel, :k])


# ---- regime 1 -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS, ids=repr)
def test_stage_fills_lists_hold_nothing_repaired(vf, oracle, driver, n_cu, cell):
    """The image route's T is 3000: chosen against k_final's 4096-entry survivor area (the band must hold the T ties), and kept -- no
    search needed a repair, so it was never lowered.  Observed on an MI355X (256 CUs, CU split 32; 64-query tile, the ksplit kernels 32;
    `stages` = passes x grid x stage_cap, candidates / max_candidates against it and against cap):
      kernel                      (A) candidates / max  stages  cap    | (B) candidates / max    stages  seeds <=  cap
      k_scan f16 100              656 164 / 10 546      79 872  16 384 | 1 256 354 / 20 037      32 768  8 192     32 768
      k_scan f16 768              661 858 / 10 936      79 872  16 384 | 1 256 206 / 20 037      32 768  8 192     32 768
      k_scan e4m3                 660 293 / 10 841      79 872  16 384 | 1 256 151 / 20 037      32 768  8 192     32 768
      k_scan int8                 659 735 / 10 938      79 872  16 384 | 1 255 856 / 20 037      32 768  8 192     32 768
      k_scan2                     655 542 / 10 936      29 289  16 384 | 1 242 434 / 20 037      12 016  8 192     32 768
      k_scan2r f16 768            656 223 / 10 936      29 289  16 384 | 1 243 197 / 20 037      12 016  8 192     32 768
      k_scan2r f16 1024           656 929 / 10 869      29 289  16 384 | 1 241 461 / 20 037      12 016  8 192     32 768
      k_scan2r e4m3               655 051 / 10 841      29 289  16 384 | 1 243 552 / 20 037      12 016  8 192     32 768
      k_scan2r image, mfma 0      192 000 /  3 000      29 289  32 768 |   948 371 / 16 274      12 016  8 192     32 768   (block at the end)
      k_scan2r image, mfma 1      192 000 /  3 000      79 872  32 768 | 1 001 502 / 17 205      32 768  8 192     32 768
      k_scan2r image, mfma 2      192 000 /  3 000      29 289  32 768 |   970 335 / 16 398      12 016  8 192     32 768
      k_scan_ksplit               309 807 / 10 901      79 872  16 384 |   549 184 / 20 037      32 768  4 096     32 768
      k_scan_ksplit8              314 716 / 10 889      79 872  16 384 |   549 796 / 20 037      32 768  4 096     32 768
      k_scan_ksplit8i             159 255 /  5 369      65 536  16 384 |   none (see CELLS)
    uncertified = overflowed = exact_reruns = 0 in every one.  Under (A) the image route appends exactly nq x T: the block and nothing else."""
    tiles = _tiles(driver, n_cu, cell)
    if not cell.image:   # deep k: candidates >= nq x kprime for any data
        payload, q, full = _deep_case(vf, oracle, cell)
        for nq in tiles:
            for tag, options, strict in (("A", cell.deep[0], False), ("B", cell.deep[1], True)):
                if options is None:   # (k_scan_ksplit8i: see CELLS)
                    continue
                what = f"{cell} deep-k nq={nq} ({tag})"
                got, st, r = _search(vf, driver, n_cu, cell, payload, cell.n, q[:nq], 2048, options, what)
                _assert_stage_filled(what, st, r, nq, strict, cpu_bound=nq * r["kprime"])
                _same(_cut(full, slice(0, nq), 2048), got, what)
    else:                # an exact-duplicate block: candidates >= nq x T
        for where in ("start", "end", "scattered"):
            payload, stored32, at, _, fam = _block_case(vf, oracle, cell, cell.n, T_BLOCK, where, 64)
            full = oracle.search(stored32, fam, 100)
            assert all(np.array_equal(full[0][i], at[:100]) for i in range(64))   # the 100 lowest ids of the block, for every query
            for nq in tiles:
                for tag, options, strict in (("A", {}, False), ("B", STRICT, True)):
                    what = f"{cell} block of {T_BLOCK} at the {where} nq={nq} ({tag})"
                    got, st, r = _search(vf, driver, n_cu, cell, payload, cell.n, fam[:nq], 100, options, what)
                    _assert_stage_filled(what, st, r, nq, strict, cpu_bound=nq * T_BLOCK)
                    _same(_cut(full, slice(0, nq), 100), got, what)


@pytest.mark.parametrize("cell", CELLS, ids=repr)
def test_stage_fills_on_a_score_ascending_ramp(vf, oracle, driver, n_cu, cell):
    """Rows in ascending score order for a family of near-identical queries, eight workgroups (waves = 64), k = 100: the thresholds rise
    through every range.  No CPU bound is claimed: the strict witness is asserted on the GPU's own count.  Observed (64 queries, the
    ksplit kernels 32): candidates 172 672 to 174 757 on the count-based routes of 768 / 1024 / 100 elements (max 2 869 of cap 8 192),
    194 842 / 257 486 / 202 770 on the image route with 0 / 1 / 2 planes (max 4 233 of 32 768), 98 425 / 97 952 / 147 836 on k_scan_ksplit /
    ksplit8 / ksplit8i (max 5 054 of 8 192); seeds <= 65 536 (32 768 at 32 queries), stages 16 384 (6 008 where the stage holds 751)."""
    payload, fam, full = _ramp_case(vf, oracle, cell)
    for nq in _tiles(driver, n_cu, cell):
        what = f"{cell} ramp nq={nq}"
        got, st, r = _search(vf, driver, n_cu, cell, payload, cell.n, fam[:nq], 100, {"waves": 64}, what)
        _assert_stage_filled(what, st, r, nq, strict=True)
        _same(_cut(full, slice(0, nq), 100), got, what)


# ---- regimes 2 and 3 ----------------------------------------------------------------------------------------------------------------------
def _overflow_case(vf, oracle, driver, n_cu, cell):
    """The corpus with a block larger than the lists, 70 block-averse queries and 6 family queries, and the oracle's top 100 of all 76."""
    n = N_OVER if cell.image else cell.n
    cap = drv.evaluate(driver, [dict(dtype=cell.dtype, n=n, d=cell.d, nq=64, k=100, n_cu=n_cu, has_image=1 if cell.image else 0, **cell.options)])[0]["cap"]
    size = 33_000 if cell.image else cap + 800
    assert size > cap and n - size >= 7000
    payload, stored32, at, q0, fam = _block_case(vf, oracle, cell, n, size, "scattered", 6)
    key = ("over", cell.dtype, cell.d, n, size)
    if key not in _cache:
        rng = np.random.default_rng(9000 + cell.d)
        plain = rng.standard_normal((70, cell.d)).astype(np.float32)
        u = stored32[at[0]] / np.linalg.norm(stored32[at[0]])
        plain -= np.outer(plain @ u, u)
        plain -= 0.3 * np.outer(np.linalg.norm(plain, axis=1), u)           # cosine with the block: -0.29
        cos = oracle.cosine(plain, stored32)
        others = np.ones(n, bool)
        others[at] = False
        assert (cos[:, at[0]] < np.quantile(cos[:, others], 0.02, axis=1)).all(), "the block must rank below the other rows for these queries"
        pool = np.concatenate([plain, fam])
        _cache[key] = (pool, oracle.search(stored32, pool, 100))
    pool, full = _cache[key]
    return payload, n, cap, pool, full


def _batch(nq, family_at):
    """Indices into the pool of 70 plain + 6 family queries: family members at `family_at`, plain queries elsewhere."""
    sel = np.arange(nq)
    sel[list(family_at)] = 70 + np.arange(len(family_at))
    return sel


def _assert_overflow_accounted(what, st, r, nq, family, cap):
    _figures(what, st, r, nq)
    assert r["cap"] == cap, (what, r)
    assert st["max_candidates"] > cap, f"{what}: no list overflowed ({st['max_candidates']} <= {cap})"
    assert st["overflowed"] == family, f"{what}: {st['overflowed']} queries flagged as overflowed, the family has {family}"
    assert st["exact_reruns"] == st["uncertified"] + st["overflowed"], f"{what}: {st}"


@pytest.mark.parametrize("cell", CELLS, ids=repr)
def test_list_overflows_and_the_repair_answers(vf, oracle, driver, n_cu, cell):
    """Observed: max_candidates = 8 992 against cap 8 192 on every count-based route, 33 000 against 32 768 on the image route;
    overflowed = exact_reruns = the family's size (4 of 64, 2 of 32), uncertified = 0; candidates 93 840 to 98 387 (64 queries,
    768 / 1024 / 100 elements), 34 952 to 45 409 (ksplit kernels, 32 queries), 191 255 / 212 409 / 193 482 (image, 0 / 1 / 2 planes)."""
    payload, n, cap, pool, full = _overflow_case(vf, oracle, driver, n_cu, cell)
    for nq in _tiles(driver, n_cu, cell):
        family_at = (0, 31, 32, 63) if nq == 64 else (0, 31)
        sel = _batch(nq, family_at)
        what = f"{cell} overflow nq={nq}"
        got, st, r = _search(vf, driver, n_cu, cell, payload, n, pool[sel], 100, {}, what)
        assert r["passes"] == 1, r
        _assert_overflow_accounted(what, st, r, nq, len(family_at), cap)
        _same(_cut(full, sel, 100), got, what)


@pytest.mark.parametrize("cell", BYTE_CELLS, ids=repr)
def test_two_passes_with_overflow_in_both(vf, oracle, driver, n_cu, cell):
    """Observed: overflowed = exact_reruns = 3, uncertified = 0; max_candidates 8 992 (e4m3, cap 8 192) and 33 000 (image, cap 32 768);
    candidates 95 986 (e4m3), 164 950 / 190 106 / 168 167 (image, 0 / 1 / 2 planes)."""
    payload, n, cap, pool, full = _overflow_case(vf, oracle, driver, n_cu, cell)
    sel = _batch(70, (63, 64, 69))
    what = f"{cell} overflow nq=64+6"
    got, st, r = _search(vf, driver, n_cu, cell, payload, n, pool[sel], 100, {}, what)
    assert r["passes"] == 2 and r["per_pass"] == 64, r
    _assert_overflow_accounted(what, st, r, 70, 3, cap)
    _same(_cut(full, sel, 100), got, what)


# ---- a fixed number of fuzz cases of the int8 and wide-rows profiles -------------------------------------------------------------------------
FUZZ = {   # profile: (seed, cases, max_work, routes (path, scan_kernel or None = any, scan_image) that must be met)
    "int8": (37, 24, 4e9, [(0, None, 0), (2, None, 0), (1, 1, 0), (1, 5, 1), (1, 3, 0)]),
    "wide_rows": (23, 10, 4e9, [(1, 6, 0), (1, 7, 0)]),
}


@pytest.mark.parametrize("profile", sorted(FUZZ))
def test_fuzz_profiles_a_fixed_number_of_cases(vf, oracle, profile):
    spec = importlib.util.spec_from_file_location("fuzz_search", os.path.join(ROOT, "tools", "fuzz_search.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    seed, cases, max_work, must = FUZZ[profile]
    rng = np.random.default_rng(seed)
    fails, seen = [], set()
    for _ in range(cases):
        case = fz.draw_case(rng, max_work, profile)
        ok, st, why = fz.run_case(vf, oracle, case, repeat=2)
        seen.add((st.get("path"), st.get("scan_kernel"), st.get("scan_image")))
        print("OK  " if ok else "FAIL", case, {x: st.get(x) for x in STAT_KEYS})
        if not ok:
            fails.append((case, why, st))
    print(f"fuzz profile {profile}: {cases} cases; (path, scan kernel, scan image) seen:", sorted(seen, key=str))
    assert not fails, fails[:3]
    for path, kernel, image in must:
        assert any(p == path and (kernel is None or kn == kernel) and im == image for p, kn, im in seen), ((path, kernel, image), sorted(seen, key=str))
