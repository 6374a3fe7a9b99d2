"""The int8 scan image (option scan_image) on the GPU: fp16 / fp32 rows of 768 elements in shards of 4M rows and more
are scanned through a per-row-scaled int8 copy (rows of 1024 keep the fp16 scan), and k_final's band re-score keeps ids and score bits those of the canonical
arithmetic -- the oracle's, and the fp16 scan's (scan_image = 0) on the same index.

The ROW side of the certificate (key = approx + off_row >= canonical - eps) is held on the device too: k_prep_image's codes, inverses,
offsets and residual statistics against the NumPy model (through the test build's hook), a search over a shard whose best matches are
rows the image understates by their whole offset (tests/test_scan_image_model.py: hostile_case) at every position of the 32-row tile,
and the edges: a shard that is not a whole number of tiles, zero rows, exact ties at the k-th place, a shard that must refuse the image."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4_000_000   # the image's smallest shard (kImageMinRows)


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _shard(n, d, seed=0):
    """N(0, 1) fp16 rows generated where they live (bench.make_shard's generator, shifted by `seed` chunks)."""
    import torch
    import bench
    lo = seed * bench.GEN_CHUNK
    return bench.make_shard(torch, lo, lo + n, d, torch.device("cuda", 0), "f16")


@pytest.fixture(scope="module")
def c768():
    return _shard(N, 768)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _search_both(ix, q, k):
    """(image result, its stats), (fp16-path result, its stats) on one index; the image is dropped and rebuilt."""
    ix.set_option("scan_image", 1)
    got = ix.search(q, k)
    st = ix.stats()
    ix.set_option("scan_image", 0)
    ref = ix.search(q, k)
    st0 = ix.stats()
    ix.set_option("scan_image", 1)
    return got, st, ref, st0


@pytest.mark.parametrize("nq,k", [(64, 100), (1, 1), (128, 100), (64, 1), (7, 128), (7, 256)])
def test_image_768_matches_oracle_and_fp16_path(vf, oracle, c768, nq, k):
    q = np.random.default_rng(7002 + nq + k).standard_normal((nq, 768)).astype(np.float32)
    with vf.DenseIndex(c768) as ix:
        got, st, ref, st0 = _search_both(ix, q, k)
        image = nq <= 64 and k <= 128
        if image:
            assert st["path"] == 1 and st["scan_image"] == 1 and st["scan_kernel"] == 5, st
        elif nq > 64:                                            # 128 queries of fp16 rows: one wide pass, never the image
            assert st["scan_image"] == 0 and st["wide_launches"] == 1, st
        else:                                                    # k above the image's limit: the rows as stored
            assert st["scan_image"] == 0 and st["scan_kernel"] == 5, st
        assert st["exact_reruns"] == 0 and st["overflowed"] == 0, st
        assert st0["scan_image"] == 0 and st0["exact_reruns"] == 0, st0
        assert _same(got, ref)
        if (nq, k) == (64, 100):
            assert _same(got, oracle.search(c768.cpu().numpy(), q, k))
        # the same index again after the image was dropped and rebuilt: bit for bit
        assert _same(ix.search(q, k), ref) and ix.stats()["scan_image"] == (1 if image else 0)


def test_rows_of_1024_keep_the_fp16_scan(vf):
    """1024-wide rows: the 2 eps band of a top-100 over 4M rows overflows k_final's survivor area for most queries (measured with an
    image: 40 of 64 queries re-run exactly), so no image is built for them."""
    c = _shard(N, 1024, seed=3)
    q = np.random.default_rng(7102).standard_normal((64, 1024)).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        ix.set_option("scan_image", 2)
        ix.search(q, 100)
        st = ix.stats()
        assert st["scan_image"] == 0 and st["scan_kernel"] == 5 and st["exact_reruns"] == 0, st


def test_fp32_rows_take_the_image(vf, c768):
    c = c768.float() * 3.0
    q = np.random.default_rng(7202).standard_normal((16, 768)).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        got, st, ref, _ = _search_both(ix, q, 100)
        assert st["scan_image"] == 1 and st["exact_reruns"] == 0, st
        assert _same(got, ref)


def test_clustered_corpus_fails_the_certificate_and_is_repaired(vf, oracle):
    """Rows that are one direction plus a little noise: every score lies within the eps band of the k-th best, the band does not fit
    k_final's survivor area, the certificate fails and the exact path answers -- with the oracle's ids and score bits."""
    import torch
    d = 768
    g = torch.Generator(device="cuda")
    g.manual_seed(7301)
    base = torch.randn(d, generator=g, device="cuda")
    c = torch.empty((N, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, N, 500_000):
        c[r0:r0 + 500_000] = (base + 0.02 * torch.randn((500_000, d), generator=g, device="cuda")).half()
    q = (base.cpu().numpy() + 0.5 * np.random.default_rng(7302).standard_normal((4, d))).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        i, s = ix.search(q, 100)
        st = ix.stats()
        assert st["scan_image"] == 1 and st["exact_reruns"] > 0, st
        assert _same((i, s), oracle.search(c.cpu().numpy(), q, 100))


def test_sharded_group_and_corpus_file(vf, c768, tmp_path):
    from veritasfi_amd import corpus_file
    c1 = _shard(N, 768, seed=40)
    q = np.random.default_rng(7402).standard_normal((64, 768)).astype(np.float32)
    with vf.DenseIndex(c768) as a, vf.DenseIndex(c1, id_offset=N) as b:
        a.set_option("scan_image", 0)
        b.set_option("scan_image", 0)
        ref = [a.search(q, 100), b.search(q, 100)]
    with vf.DenseIndex.group([vf.DenseIndex(c768), vf.DenseIndex(c1, id_offset=N)]) as ix:   # two 4M-row shards, one device
        got = ix.search(q, 100)
        assert ix.stats()["scan_image"] == 1, ix.stats()
        ix.set_option("scan_image", 0)
        assert _same(ix.search(q, 100), got)
    ids = np.concatenate([ref[0][0], ref[1][0]], axis=1)
    sc = np.concatenate([ref[0][1], ref[1][1]], axis=1)
    order = np.lexsort((ids, -sc.astype(np.float64)), axis=1)[:, :100]
    assert np.array_equal(np.take_along_axis(ids, order, 1), got[0])
    p = str(tmp_path / "img.vfc")
    corpus_file.write(p, c768.cpu().numpy())
    with vf.DenseIndex.from_file(p) as ix:
        i, s = ix.search(q, 100)
        assert ix.stats()["scan_image"] == 1 and ix.stats()["exact_reruns"] == 0
        assert _same((i, s), ref[0])


def test_option_values_and_smaller_shards(vf):
    c = _shard(2_500_000, 768, seed=80)                      # a 4-GPU rank's shard of the headline corpus: no image
    q = np.random.default_rng(7502).standard_normal((64, 768)).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        with pytest.raises(Exception):
            ix.set_option("scan_image", 3)
        ix.set_option("scan_image", 2)                          # forced: still only for shards of 4M rows and more
        ix.search(q, 100)
        st = ix.stats()
        assert st["scan_image"] == 0 and st["scan_kernel"] == 5, st


# ---- the row side of the certificate on the device --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,d,per_kind", [("f16", 768, 37), ("f32", 768, 37), ("f16", 700, 21), ("f32", 700, 21), ("f16", 768, 557)])
def test_device_prep_image_matches_the_model(vf, dtype, d, per_kind):
    """vf_debug_prep_image: k_prep_rows + k_prep_image on every row kind of tests/test_scan_image_model.py (fp16: all but the two
    fp32-range kinds), row counts that are no multiple of the kernel's 16 rows per workgroup (the last case: 5 013 rows, 314 workgroups
    meeting in the two atomics; d = 700: 68 padding bytes per row).  Codes, canonical norms, inv_img, off_img and rho_max are the model's
    BIT FOR BIT; rho_sum is within (workgroups + 16) 2^-24 relative of the fp64 sum (one fp32 atomic add per workgroup, 16 inside it).
    An offset the kernel halved, or a residual reduced over half of a row's lanes, fails here.  "tie" rows (x / s exactly on .5) may
    fall back to: codes within 1 of the model's and off_img >= the offset formula of the residual of the codes AS STORED -- the test
    prints which rows needed that (none where the device's fp32 division is correctly rounded, as NumPy's is)."""
    import test_scan_image_model as M
    from veritasfi_amd import _ffi
    L = _ffi.lib()
    L.vf_debug_prep_image.restype = ctypes.c_int
    L.vf_debug_prep_image.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32] + [ctypes.c_void_p] * 6
    dp = (d + 127) // 128 * 128
    np_t = np.float16 if dtype == "f16" else np.float32

    def device(x):
        n = x.shape[0]
        codes = np.zeros((n, dp), dtype=np.uint8)
        inv, off, norm = (np.zeros(n, dtype=np.float32) for _ in range(3))
        rmax, rsum = np.zeros(1, dtype=np.float32), np.zeros(1, dtype=np.float32)
        _ffi.check(L.vf_debug_prep_image(x.ctypes.data, 1 if dtype == "f16" else 0, n, d, codes.ctypes.data, inv.ctypes.data, off.ctypes.data,
                                         norm.ctypes.data, rmax.ctypes.data, rsum.ctypes.data), "vf_debug_prep_image")
        return codes, inv, off, norm, rmax[0], rsum[0]

    kinds = ["gauss", "clustered", "heavy"] + [k for k in M.EDGE_KINDS if dtype == "f32" or k not in ("f32big", "f32small")]
    with np.errstate(over="ignore"):
        x = np.ascontiguousarray(np.concatenate([M._rows(kind, per_kind, d, 300 + i) for i, kind in enumerate(kinds)]).astype(np_t))
    is_tie = np.repeat(np.array([k == "tie" for k in kinds]), per_kind)
    n = x.shape[0]
    assert n % 16 != 0
    codes, inv, off, norm, rmax, rsum = device(x)
    xs = x.astype(np.float32)                                    # the rows as stored
    code, s, inv_m, rho, norm_m, res = M.quantise(xs, full=True)
    off_m = M.offsets(res, d)
    assert np.all(codes[:, d:] == 128)                           # padding: code 0
    got = codes[:, :d].astype(np.int16) - 128
    assert np.array_equal(_bits(norm), _bits(norm_m))
    row_ok = (got == code).all(axis=1) & (_bits(inv) == _bits(inv_m)) & (_bits(off) == _bits(off_m))
    weak = np.nonzero(~row_ok & is_tie)[0]
    assert row_ok[~is_tie].all(), np.nonzero(~row_ok & ~is_tie)[0][:10]
    print(f"{dtype} d={d} n={n}: tie rows held to the weaker rule: {weak.tolist()}")
    rho_dev = rho.copy()
    for r in weak:                                               # the weaker rule (tie rows only)
        assert np.abs(got[r] - code[r]).max() <= 1 and _bits(inv[r:r + 1])[0] == _bits(inv_m[r:r + 1])[0]
        real = np.sqrt(((xs[r].astype(np.float64) - float(s[r]) * got[r]) ** 2).sum()) / float(norm_m[r])
        assert float(off[r]) >= real * (1 + 2.0 ** -11) * (1 + 2.0 ** -20) + d * 2.0 ** -24 * real
        rho_dev[r] = np.nextafter(np.float32(real), np.float32(np.inf))
    if weak.size == 0:
        assert _bits(np.float32(rmax)) == _bits(rho.max())
    else:
        assert float(rmax) >= float(rho_dev.max()) * (1 - 2.0 ** -23)
    total = float(rho_dev.astype(np.float64).sum())
    assert abs(float(rsum) - total) <= ((n + 15) // 16 + 16) * 2.0 ** -24 * total, (rsum, total)
    # a row that is not finite: the shard's rho_max must not be either (build_image then keeps no image)
    if per_kind == 37:
        for bad in (np.inf, -np.inf, np.nan):
            y = np.ascontiguousarray(M._rows("gauss", 19, d, 77).astype(np_t))
            y[11, 5] = bad
            assert not np.isfinite(device(y)[4]), bad


def _exact_shard(n, d, seed):
    """"exact" rows (tests/test_scan_image_model.py) generated where they live: integer codes in [-126, 126], one element of each row
    +-127, times a power of two -- the image holds them without residual (rho = 0, off = 0)."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    c = torch.empty((n, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, n, 500_000):
        m = min(500_000, n - r0)
        code = torch.randint(-126, 127, (m, d), generator=g, device="cuda").float()
        peak = torch.randint(0, d, (m,), generator=g, device="cuda")
        code[torch.arange(m, device="cuda"), peak] = 127.0 * (2.0 * torch.randint(0, 2, (m,), generator=g, device="cuda").float() - 1.0)
        c[r0:r0 + m] = (code * torch.exp2(torch.randint(-9, -3, (m, 1), generator=g, device="cuda").float())).half()
    return c


def test_rows_the_image_understates_by_their_whole_offset(vf, oracle):
    """The hostile search.  Background: 4 000 037 "exact" rows (rho = 0: the band is eps + 2^-9).  Four sign-vector queries (rho_q ~ 0
    with one int8 plane) at batch positions 0, 31, 32 and 63 among N(0, 1) queries, each with 32 "aligned" victims -- its 32 best
    canonical matches, understated by the image by rho_row = 0.011 .. 0.015 -- at every residue of the 32-row tile, the first row, the
    last whole tile and row n - 1 of the last, partial one among them, every victim among exact rows (offset 0); and 220 exact decoys
    between the victims' canonical scores and their keys without offset.  On the model (asserted before the GPU is touched), a victim's
    key without its offset or with half of it lies more than a coarse bin below the cut: a scan that lost, halved or misrouted an
    offset drops the victim, keeps a k-th key among the decoys and certifies a wrong top 100.  Ids and score bits must be the
    oracle's, with no exact re-run (the image answered, not the repair), for every image_mfma form, in the batch and alone."""
    import torch
    import test_scan_image_model as M
    n, d, k = N + 37, 768, 100
    assert n % 32 == 5
    at = (0, 31, 32, 63)
    cases = [M.hostile_case(oracle, 7900 + i) for i in range(4)]
    margins, (rho_lo, rho_hi), band = M.hostile_margins(oracle, cases, n, k)
    print(f"victims' rho_row {rho_lo:.5f} .. {rho_hi:.5f}, band {band:.5f}; smallest margins to the cut (key without offset, with half of it, "
          f"with all of it), image_mfma 0 / 1 / 2: {margins}")
    assert 0.010 <= rho_lo and rho_hi <= 1.0 / 64
    for form in (0, 1, 2):
        none, half, full = margins[form]
        assert none >= 2.0 ** -10 and half >= 2.0 ** -10 and full > 0, (form, margins[form])
    # where the planted rows go: victims in even tiles (any two at least 33 rows apart), decoys in odd ones
    rng = np.random.default_rng(7910)
    tiles = n // 32                                              # whole tiles; tile `tiles` is the partial one
    vt = 2 * rng.choice(np.arange(1, tiles // 2), size=(4, 32), replace=False)
    vt[0, 0], vt[1, 31] = 0, tiles - (tiles % 2)                 # row 0; residue 31 of the last whole even tile
    vpos = vt * 32 + np.arange(32)[None, :]
    vpos[0, 4] = n - 1                                           # residue 4 of the partial tile: the shard's last row
    nd = cases[0]["decoys"].shape[0]
    dpos = (2 * rng.choice(np.arange(1, tiles // 2 - 1), size=(4, nd), replace=False) + 1) * 32 + rng.integers(0, 32, (4, nd))
    assert np.array_equal(np.sort(vpos % 32, axis=1), np.tile(np.arange(32), (4, 1))) and vpos.max() == n - 1
    allv = np.sort(vpos.ravel())
    assert np.diff(allv).min() >= 5 and not np.intersect1d(allv, dpos.ravel()).size and np.unique(dpos).size == dpos.size
    c = _exact_shard(n, d, 7920)
    for i, case in enumerate(cases):
        c[torch.from_numpy(vpos[i]).cuda()] = torch.from_numpy(case["victims"].astype(np.float16)).cuda()
        c[torch.from_numpy(dpos[i]).cuda()] = torch.from_numpy(case["decoys"].astype(np.float16)).cuda()
    q = np.random.default_rng(7930).standard_normal((64, d)).astype(np.float32)
    for i, case in enumerate(cases):
        q[at[i]] = case["query"]
    host = c.cpu().numpy()
    want = oracle.search(host, q, k)
    want1 = oracle.search(host, q[:1], k)
    for i in range(4):                                           # the construction holds on the rows as stored, background included
        ids = want[0][at[i]]
        assert set(ids[:32].tolist()) == set(vpos[i].tolist()) and set(ids[32:].tolist()) <= set(dpos[i].tolist()), i
    with vf.DenseIndex(c) as ix:
        for form in (1, 2, 0):
            ix.set_option("image_mfma", form)
            for qq, ww in ((q, want), (q[:1], want1)):
                got = ix.search(qq, k)
                st = ix.stats()
                print(f"image_mfma={form} nq={qq.shape[0]}:", {key: st[key] for key in ("scan_image", "scan_kernel", "exact_reruns", "uncertified", "overflowed", "candidates")})
                assert st["scan_image"] == 1 and st["scan_kernel"] == 5 and st["exact_reruns"] == 0 and st["uncertified"] == 0, (form, st)
                bad = np.nonzero((got[0] != ww[0]).any(axis=1) | (_bits(got[1]) != _bits(ww[1])).any(axis=1))[0]
                assert bad.size == 0, (form, qq.shape[0], bad.tolist())


def test_edges_through_the_image(vf, oracle, c768):
    """The N(0, 1) shard extended to 4 000 037 rows (5 rows in the last tile) with an id offset above 2^32, and planted: zero rows (norm
    -> 1, step -> 1, every key 0); 150 copies of one strong row for query 0 -- exact ties across the k-th place: after the three best
    the top k is the LOWEST ids among the copies; and query 0's three best matches at the last three row ids.  k = 100 and 128, every
    image_mfma form, against the fp16 scan of the same index, bit for bit; k = 100 against the oracle."""
    import torch
    import bench
    n, d, id0 = N + 37, 768, 5_000_000_000
    c = torch.empty((n, d), dtype=torch.float16, device="cuda")
    c[:N] = c768
    c[N:] = bench.make_shard(torch, 90 * bench.GEN_CHUNK, 90 * bench.GEN_CHUNK + 37, d, torch.device("cuda", 0), "f16")
    rng = np.random.default_rng(8001)
    q = rng.standard_normal((8, d)).astype(np.float32)
    zeros = np.array([5, 1_000_003, n - 20])
    copies = np.sort(rng.choice(np.arange(100, n - 100), size=150, replace=False))
    strong = (q[0] + 0.3 * rng.standard_normal(d)).astype(np.float16)
    best = (q[0][None, :] + 0.05 * rng.standard_normal((3, d))).astype(np.float16)
    assert not np.intersect1d(zeros, copies).size
    c[torch.from_numpy(zeros).cuda()] = 0
    c[torch.from_numpy(copies).cuda()] = torch.from_numpy(strong).cuda()
    c[n - 3:] = torch.from_numpy(best).cuda()
    want = oracle.search(c.cpu().numpy(), q, 100, id0)
    with vf.DenseIndex(c, id_offset=id0) as ix:
        for k in (100, 128):
            ix.set_option("scan_image", 0)
            ref = ix.search(q, k)
            st0 = ix.stats()
            assert st0["scan_image"] == 0, st0                       # (150 ties across its k'-th place: the fp16 scan may repair query 0)
            ix.set_option("scan_image", 1)
            assert set(ref[0][0, :3].tolist()) == {id0 + n - 3, id0 + n - 2, id0 + n - 1}
            assert np.array_equal(ref[0][0, 3:], id0 + copies[:k - 3]) and np.unique(_bits(ref[1][0, 3:])).size == 1
            if k == 100:
                assert _same(ref, want)
            for form in (1, 2, 0):
                ix.set_option("image_mfma", form)
                got = ix.search(q, k)
                st = ix.stats()
                assert st["scan_image"] == 1 and st["scan_kernel"] == 5 and st["exact_reruns"] == 0 and st["overflowed"] == 0, (k, form, st)
                assert _same(got, ref), (k, form)


def test_a_shard_with_one_heavy_row_refuses_the_image(vf, oracle, c768):
    """One row with a few large elements (rho_row > 1/64: the 65/64 of eps_q is proven below that only) among 4M ordinary ones: no
    image is kept even when it is forced, and the fp16 scan answers with the oracle's ids and score bits."""
    import test_scan_image_model as M
    import torch
    heavy = M._rows("heavy", 1, 768, 5).astype(np.float16)
    rho = M.quantise(heavy.astype(np.float32))[3]
    assert rho[0] > 1.0 / 64
    c = c768.clone()
    c[1_234_567] = torch.from_numpy(heavy[0]).cuda()
    q = np.random.default_rng(8101).standard_normal((8, 768)).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        ix.set_option("scan_image", 2)
        got = ix.search(q, 100)
        st = ix.stats()
        assert st["scan_image"] == 0 and st["scan_kernel"] == 5 and st["exact_reruns"] == 0, st
        assert _same(got, oracle.search(c.cpu().numpy(), q, 100))
