"""The int8 scan image's certificate, modelled in NumPy on the CPU: the quantiser k_prep_image applies, the score key
k_scan2r forms from it (approximate score + the row's offset), and the bound the library uses (vf_debug_image_bound) -- canonical <= key
+ eps for every row, with the fp16 path's eps, on random, clustered and hostile rows; and the key is never more than 2 off + eps above."""
import numpy as np
import pytest

import adversarial as ADV


def quantise(x):
    """k_prep_image: per row s = absmax / 127 (fp32), code = rint(x / s) clamped to +-127, rho = ||x - s code|| / norm (fp64, rounded
    UP to fp32), inv = s / norm; returns (codes int8, s, inv fp32, rho fp32, norm fp32 -- the canonical norm)."""
    x = np.asarray(x, dtype=np.float32)
    mx = np.abs(x).max(axis=1)
    s = np.where(mx > 0, mx / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    code = np.clip(np.rint(x / s[:, None]), -127, 127).astype(np.int8)
    norm = canonical_norm(x)
    res = np.sqrt(((x.astype(np.float64) - s[:, None].astype(np.float64) * code) ** 2).sum(axis=1)) / norm
    rho = res.astype(np.float32)
    rho = np.where(rho.astype(np.float64) < res, np.nextafter(rho, np.float32(np.inf)), rho)
    inv = (s.astype(np.float64) / norm).astype(np.float32)
    return code, s, inv, rho, norm


def offsets(rho, d):
    """off_img: rho (1 + 2^-11)(1 + 2^-20) + d 2^-24 rho, in fp64, rounded up to fp32."""
    od = rho.astype(np.float64) * (1 + 2.0 ** -11) * (1 + 2.0 ** -20) + d * 2.0 ** -24 * rho.astype(np.float64)
    off = od.astype(np.float32)
    return np.where(off.astype(np.float64) < od, np.nextafter(off, np.float32(np.inf)), off)


def canonical_norm(x):
    """sqrt in fp64 of dot16(x, x) (16 interleaved fp32 partial sums, fixed tree); zero -> 1."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    acc = np.zeros((n, 16), dtype=np.float32)
    for j in range(d):
        acc[:, j & 15] = (x[:, j] * x[:, j] + acc[:, j & 15]).astype(np.float32)
    for h in (8, 4, 2, 1):
        acc = (acc[:, :h] + acc[:, h:2 * h]).astype(np.float32)
    nm = np.sqrt(acc[:, 0].astype(np.float64)).astype(np.float32)
    return np.where(nm == 0, np.float32(1.0), nm)


def biased_bytes(code):
    return (code.astype(np.int16) + 128).astype(np.uint8)


def cvt_i8b(b):
    """cvt8_i8b: v_perm_b32 puts byte b under 0x64 (the fp16 1024 + b), v_pk_add_f16 adds -1152."""
    h = (np.uint16(0x6400) | b.astype(np.uint16)).view(np.float16)
    return (h + np.float16(-1152.0)).astype(np.float16)


def approx_scores(qn, code, inv):
    """What the scan forms: fp16 query image x the exact fp16 codes, summed in fp32, times the fp32 inverse (scale / norm)."""
    q16 = qn.astype(np.float16).astype(np.float32)
    acc = code.astype(np.float32) @ q16
    return (acc.astype(np.float32) * inv).astype(np.float32)


def image_eps(d, fp32_rows=False):
    return ADV.eps_bound(d, 2.0 ** -11, fp32_rows) + 1e-7


def image_band(d, rho_mean, fp32_rows=False):
    return np.float32(image_eps(d, fp32_rows)) + 1.5 * rho_mean * (1 + 2.0 ** -11) * (1 + 2.0 ** -20) + 2.0 ** -9


def test_conversion_is_exact_for_every_code():
    code = np.arange(-127, 128, dtype=np.int16).astype(np.int8)
    assert np.array_equal(cvt_i8b(biased_bytes(code)).astype(np.float32), code.astype(np.float32))


def _rows(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)
    if kind == "clustered":
        base = rng.standard_normal(d)
        return (base + 0.03 * rng.standard_normal((n, d))).astype(np.float16).astype(np.float32)
    if kind == "heavy":   # a few large elements per row: the scale is set by them, the rest quantise coarsely
        x = rng.standard_normal((n, d)) * 0.1
        x[np.arange(n), rng.integers(0, d, n)] = 8.0
        return x.astype(np.float32)
    raise ValueError(kind)


@pytest.mark.parametrize("kind,d", [("gauss", 768), ("gauss", 1024), ("clustered", 768), ("heavy", 768)])
def test_rho_bounds_the_residual_and_eps_bounds_the_score_error(oracle, kind, d):
    x = _rows(kind, 3000, d, 11 + d)
    code, s, inv, rho, norm = quantise(x)
    # rho is an upper bound of the realised residual (fp64) and the codes are in range
    real = np.sqrt(((x.astype(np.float64) - s[:, None].astype(np.float64) * code) ** 2).sum(axis=1)) / norm
    assert np.all(rho.astype(np.float64) >= real) and np.abs(code.astype(np.int32)).max() <= 127
    q = np.random.default_rng(5).standard_normal((16, d)).astype(np.float32)
    qn = oracle.normalize(q)
    key = (approx_scores(qn.T, code, inv[:, None]) + offsets(rho, d)[:, None]).astype(np.float32)
    can = oracle.cosine(q, x).T
    eps = image_eps(d)
    assert (can - key.astype(np.float64)).max() <= eps
    assert (key.astype(np.float64) - can - 2 * offsets(rho, d)[:, None]).max() <= eps
    # N(0, 1) rows: rho ~ 7.8e-3 on average, the shard's maximum well above it (a row's absmax sets its step): DESIGN.md 2
    if kind == "gauss":
        assert 0.006 < rho.mean() < 0.009 and rho.max() < 1.0 / 64


def test_eps_on_hostile_rows(oracle):
    """The half-way query of tests/adversarial.py against rows parallel to it: the fp16 query rounding all one way plus the rows'
    quantisation, still inside the bound."""
    q, _ = ADV.halfway_query()
    qn = oracle.normalize(q[None, :])[0]
    rows = np.stack([qn * (1 + 1e-3 * i) for i in range(64)]).astype(np.float16).astype(np.float32)
    code, s, inv, rho, norm = quantise(rows)
    key = (approx_scores(qn[:, None], code, inv[:, None])[:, 0] + offsets(rho, 768)).astype(np.float32)
    can = oracle.cosine(q[None, :], rows)[0]
    assert (can - key.astype(np.float64)).max() <= image_eps(768)


@pytest.mark.parametrize("d,dtype,rho", [(768, 1, 0.0075), (1024, 1, 0.008), (768, 0, 0.0), (768, 0, 0.015)])
def test_library_bound_matches_the_model(d, dtype, rho):
    """vf_debug_image_bound: the test build's hook onto the bound make_plan uses (host code only: no GPU needed)."""
    import ctypes
    from veritasfi_amd import build as B
    lib = ctypes.CDLL(B.TEST_LIB)
    eps, tb, fb = ctypes.c_float(), ctypes.c_int32(), ctypes.c_int32()
    rc = lib.vf_debug_image_bound(ctypes.c_int32(d), ctypes.c_int32(dtype), ctypes.c_float(rho), ctypes.byref(eps), ctypes.byref(tb),
                                  ctypes.byref(fb))
    assert rc == 0
    want = image_eps(d, fp32_rows=dtype == 0)
    assert abs(eps.value - want) <= 1e-7 * want + 1e-9 and eps.value >= np.float32(want) * (1 - 2 ** -23)
    band = image_band(d, float(np.float32(rho)), fp32_rows=dtype == 0)
    assert tb.value == int(np.ceil(band * 1024)) + 1 and fb.value == int(np.ceil(band * 16384)) + 1
