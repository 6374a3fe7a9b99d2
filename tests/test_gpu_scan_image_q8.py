"""The int8 row image scanned with the int8 matrix instruction (option image_mfma = 1: one int8 query plane; 2: hi + lo planes;
DESIGN.md 2, 4): the sums are exact integers, and each query's own quantisation residual widens ITS certificate bound and re-score
band.  Ids and score bits must be those of the fp16 scan (scan_image = 0) on the same index -- for ordinary queries without an exact
re-run in either form, for queries with one dominant element (a coarse step: a large one-plane residual) through the exact re-run with
one plane and without it with two, and for a clustered corpus through the repair.  image_mfma = 0 (the codes converted to fp16, fp16
queries) is run beside them.  The operand map of the instruction and the prep kernel's residuals, steps, codes and bands are pinned
through test-build hooks."""
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


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


@pytest.fixture(scope="module")
def c768():
    import torch
    import bench
    return bench.make_shard(torch, 0, N, 768, torch.device("cuda", 0), "f16")


def _reference(ix, q, k):
    ix.set_option("scan_image", 0)
    ref = ix.search(q, k)
    st0 = ix.stats()
    ix.set_option("scan_image", 1)
    assert st0["scan_image"] == 0 and st0["exact_reruns"] == 0, st0
    return ref


@pytest.mark.parametrize("nq,k", [(64, 100), (1, 1), (128, 100), (64, 1), (7, 128), (7, 256)])
def test_int8_instruction_matches_the_fp16_path_bit_for_bit(vf, c768, nq, k):
    q = np.random.default_rng(7002 + nq + k).standard_normal((nq, 768)).astype(np.float32)
    with vf.DenseIndex(c768) as ix:
        ref = _reference(ix, q, k)
        image = nq <= 64 and k <= 128
        cands = {}
        for form in (1, 2, 0):
            ix.set_option("image_mfma", form)
            got = ix.search(q, k)
            st = ix.stats()
            cands[form] = st["candidates"] / nq
            assert st["scan_image"] == (1 if image else 0), st
            if image:
                assert st["path"] == 1 and st["scan_kernel"] == 5, st
            assert st["exact_reruns"] == 0 and st["overflowed"] == 0 and st["uncertified"] == 0, (form, st)
            assert _same(got, ref), form
        print(f"nq={nq} k={k}: candidates per query, one int8 plane {cands[1]:.0f}, two planes {cands[2]:.0f}, fp16 instruction {cands[0]:.0f}")
        ix.set_option("image_mfma", -1)
        assert _same(ix.search(q, k), ref)
        with pytest.raises(Exception):
            ix.set_option("image_mfma", 3)


def test_queries_with_one_dominant_element_stay_exact(vf, c768):
    """One element 40 x the others: the query's step is set by it, the rest quantise coarsely, and with ONE plane rho_q ~ 0.05: a band of
    ~0.07 holds tens of thousands of rows of a 4M-row N(0, 1) shard (cos ~ N(0, 1 / 768)), not the 4 096 of k_final's survivor area, so
    every such query is flagged and the exact path answers it.  Two planes leave rho_q < 10^-3 (band as the fp16 form's): no re-run.
    The result is the fp16 path's every way, and a flagged query is always re-run."""
    rng = np.random.default_rng(7602)
    q = rng.standard_normal((16, 768)).astype(np.float32)
    q[np.arange(16), rng.integers(0, 768, 16)] = 40.0
    with vf.DenseIndex(c768) as ix:
        ref = _reference(ix, q, 100)
        for form in (1, 2, 0):
            ix.set_option("image_mfma", form)
            got = ix.search(q, 100)
            st = ix.stats()
            print(f"dominant-element queries, image_mfma={form}:", {k: st[k] for k in ("exact_reruns", "uncertified", "overflowed", "candidates")})
            assert st["scan_image"] == 1 and st["scan_kernel"] == 5, st
            assert st["exact_reruns"] == st["uncertified"] + st["overflowed"], st     # what is flagged is re-run, nothing else
            assert (st["exact_reruns"] == 16) if form == 1 else (st["exact_reruns"] == 0), (form, st)
            assert _same(got, ref), form


def test_clustered_corpus_is_still_repaired_exactly(vf, oracle):
    import torch
    d = 768
    g = torch.Generator(device="cuda")
    g.manual_seed(7301)
    base = torch.randn(d, generator=g, device="cuda")
    c = torch.empty((N, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, N, 500_000):
        c[r0:r0 + 500_000] = (base + 0.02 * torch.randn((500_000, d), generator=g, device="cuda")).half()
    q = (base.cpu().numpy() + 0.5 * np.random.default_rng(7302).standard_normal((4, d))).astype(np.float32)
    want = oracle.search(c.cpu().numpy(), q, 100)
    with vf.DenseIndex(c) as ix:
        for form in (1, 2):
            ix.set_option("image_mfma", form)
            i, s = ix.search(q, 100)
            st = ix.stats()
            assert st["scan_image"] == 1 and st["exact_reruns"] > 0, (form, st)
            assert _same((i, s), want), form


def test_operand_map_of_the_int8_matrix_instruction(vf):
    """vf_debug_mfma_i8: C = A B^T from one v_mfma_i32_32x32x32_i8 fed as k_scan2r feeds it.  Exact integers over the whole int8 range,
    A and B unrelated (a transposed or half-swapped map cannot pass), and a B with a single non-zero entry per probe."""
    from veritasfi_amd import _ffi
    L = _ffi.lib()
    L.vf_debug_mfma_i8.restype = ctypes.c_int
    L.vf_debug_mfma_i8.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    rng = np.random.default_rng(7701)

    def run(A, B):
        C = np.zeros((32, 32), dtype=np.int32)
        _ffi.check(L.vf_debug_mfma_i8(A.ctypes.data, B.ctypes.data, C.ctypes.data), "vf_debug_mfma_i8")
        return C

    A = rng.integers(-128, 128, (32, 32)).astype(np.int8)
    B = rng.integers(-128, 128, (32, 32)).astype(np.int8)
    assert np.array_equal(run(A, B), A.astype(np.int32) @ B.astype(np.int32).T)
    for n, kk in ((0, 0), (5, 17), (31, 31), (13, 16), (20, 15)):
        B1 = np.zeros((32, 32), dtype=np.int8)
        B1[n, kk] = 3
        want = np.zeros((32, 32), dtype=np.int32)
        want[:, n] = 3 * A[:, kk].astype(np.int32)
        assert np.array_equal(run(A, B1), want), (n, kk)


@pytest.mark.parametrize("planes", [1, 2])
def test_prep_kernel_matches_the_model(vf, oracle, planes):
    """vf_debug_prep_q8: k_prep_q8's codes, steps, certificate bounds and bands as the DEVICE wrote them, against the NumPy model of
    tests/test_scan_image_q8_model.py -- ordinary, half-way and dominant-element queries, and the padding slots.  A residual the kernel
    understated (a reduction bug) would leave every search test on N(0, 1) data passing and the certificate unsound."""
    import test_scan_image_q8_model as Q
    from veritasfi_amd import _ffi
    L = _ffi.lib()
    L.vf_debug_prep_q8.restype = ctypes.c_int
    L.vf_debug_prep_q8.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_int32, ctypes.c_int32,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    q = np.concatenate([Q._queries("gauss", 20, 1), Q._queries("halfway", 2, 2), Q._queries("dominant", 20, 3)])
    qn = np.ascontiguousarray(oracle.normalize(q), dtype=np.float32)
    nq, d = qn.shape
    eps_img, tb0, fb0 = np.float32(Q.M.image_eps(d)), 16, 231
    codes = np.zeros((d // 16, planes, 64, 16), dtype=np.int8)
    step, eps, band = np.zeros(64, np.float32), np.zeros(64, np.float32), np.zeros((2, 64), np.int32)
    _ffi.check(L.vf_debug_prep_q8(qn.ctypes.data, nq, d, planes, ctypes.c_float(float(eps_img)), tb0, fb0, codes.ctypes.data, step.ctypes.data,
                                  eps.ctypes.data, band.ctypes.data), "vf_debug_prep_q8")
    hi, lo, s, rho, real = Q.quantise_query(qn, planes)
    got_hi = codes[:, 0].transpose(1, 0, 2).reshape(64, d)
    assert np.array_equal(got_hi[:nq], hi) and not got_hi[nq:].any()
    want_step = s if planes == 1 else (s / np.float32(254.0)).astype(np.float32)
    assert np.array_equal(step[:nq], want_step) and not step[nq:].any()
    seen = s[:, None].astype(np.float64) * got_hi[:nq]
    if planes == 2:
        got_lo = codes[:, 1].transpose(1, 0, 2).reshape(64, d)
        assert np.abs(got_lo[:nq].astype(np.int32) - lo).max() <= 1 and not got_lo[nq:].any()   # (the device divides in fp32, the model in fp64)
        seen = seen + want_step[:, None].astype(np.float64) * got_lo[:nq]
    real_dev = np.sqrt(((qn.astype(np.float64) - seen) ** 2).sum(axis=1))       # the residual of the codes AS STORED
    for i in range(nq):
        # the device's bound covers the realised residual, and is the model's formula of a rho within a rounding of the realised one
        lo_b = Q.q8_bound(np.float32(real_dev[i]), eps_img, tb0, fb0)
        hi_b = Q.q8_bound(np.nextafter(np.float32(real_dev[i] * (1 + 1e-6)), np.float32(np.inf)), eps_img, tb0, fb0)
        assert eps[i] >= float(eps_img) + real_dev[i] * 65.0 / 64.0 + 2.0 ** -20
        assert lo_b[0] <= eps[i] <= hi_b[0] and lo_b[1] <= band[0, i] <= hi_b[1] and lo_b[2] <= band[1, i] <= hi_b[2], (i, eps[i], lo_b, hi_b)
    assert np.all(eps[nq:] == Q.q8_bound(0.0, eps_img, tb0, fb0)[0]) and np.all(band[0, nq:] == tb0) and np.all(band[1, nq:] == fb0)
