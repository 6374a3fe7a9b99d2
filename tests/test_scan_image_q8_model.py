"""The int8 row image scanned with the int8 matrix instruction (k_scan2r, F8 = 3), modelled in NumPy on the CPU: int8 row
codes x int8 query planes, the exact integer sum, the two fp32 multiplications (query step, row inverse) and the row's offset -- and the
per-query bound eps_q = eps_image + rho_q 65 / 64 + 2^-20: canonical <= key + eps_q for EVERY (query, row) pair, on the row kinds of
tests/test_scan_image_model.py, on tests/adversarial.py's half-way query and on queries with one dominant element (a coarse step: a
large rho_q).  One plane is the library's default (k_prep_q8, option image_mfma = 1); the two-plane form (image_mfma = 2: hi + lo, the
residual quantised again at s / 254) is modelled beside it with the same assertions: its rho_q is a hundredth of one plane's and its band
the fp16 form's.  The library's host formula for the per-query bound and bands (the one k_prep_q8 runs on the device) is checked
against the model through the test build's hook."""
import ctypes

import numpy as np
import pytest

import adversarial as ADV
import test_scan_image_model as M

D = 768


def quantise_query(qn, planes=1):
    """k_prep_q8: s = absmax / 127 (fp32), code = rint(qn / s) clamped to +-127; rho_q = ||qn - q'|| in fp64, rounded UP to fp32, q' the
    vector the scan sees.  Two planes: lo = rint((qn - s hi) / (s / 254)) clamped, q' = s hi + (s / 254) lo.
    Returns (hi int32 [nq, d], lo or None, s fp32 [nq], rho fp32 [nq])."""
    qn = np.asarray(qn, dtype=np.float32)
    mx = np.abs(qn).max(axis=1)
    s = np.where(mx > 0, mx / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    hi = np.clip(np.rint(qn / s[:, None]), -127, 127).astype(np.int32)
    seen = s[:, None].astype(np.float64) * hi
    lo = None
    if planes == 2:
        s2 = (s / np.float32(254.0)).astype(np.float32)
        lo = np.clip(np.rint((qn.astype(np.float64) - seen) / s2[:, None]), -127, 127).astype(np.int32)
        seen = seen + s2[:, None].astype(np.float64) * lo
    res = np.sqrt(((qn.astype(np.float64) - seen) ** 2).sum(axis=1))
    rho = res.astype(np.float32)
    rho = np.where(rho.astype(np.float64) < res, np.nextafter(rho, np.float32(np.inf)), rho)
    return hi, lo, s, rho, res


def keys(code, inv, off, hi, lo, s):
    """The scan's key for every (row, query): the exact int32 sum -> fp32 (exact: |sum| < 2^24) x the query's step x the row's inverse
    + the row's offset, each operation rounded to fp32.  Two planes: hi x 254 + lo combined in fp32, step s / 254.  Returns the key with
    the last multiplication and the addition rounded separately and as one fma (the compiler may contract them)."""
    acc = code.astype(np.int64) @ hi.T.astype(np.int64)
    assert np.abs(acc).max() < 2 ** 24
    accf = acc.astype(np.float32)
    assert np.array_equal(accf.astype(np.int64), acc)
    step = s
    if lo is not None:
        acc_lo = code.astype(np.int64) @ lo.T.astype(np.int64)
        assert np.abs(acc_lo).max() < 2 ** 24
        accf = (accf * np.float32(254.0)).astype(np.float32)            # (up to 3.1e9: this product and the sum below round; int32 would overflow)
        accf = (accf + acc_lo.astype(np.float32)).astype(np.float32)
        step = (s / np.float32(254.0)).astype(np.float32)
    m = (accf * step[None, :]).astype(np.float32)
    two = ((m * inv[:, None]).astype(np.float32) + off[:, None]).astype(np.float32)
    fma = (m.astype(np.float64) * inv[:, None].astype(np.float64) + off[:, None].astype(np.float64)).astype(np.float32)
    return two, fma


def q8_bound(rho_q, eps_img, tau_band, fine_band):
    """image_q8_bound / image_q8_eps (csrc/vf_internal.h): c = rho_q 65 / 64 in fp64; eps_q = up(up(eps_img + up(c)) + 2^-20), the
    bands + ceil(c x 1024) and + ceil(c x 16 384)."""
    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))
    c = float(np.float32(rho_q)) * (65.0 / 64.0)
    add = np.float32(c)
    if float(add) < c:
        add = up(add)
    e = up(np.float32(np.float32(eps_img) + add)) + np.float32(2.0 ** -20)
    return up(np.float32(e)), tau_band + int(np.ceil(c * 1024)), fine_band + int(np.ceil(c * 16384))


def _queries(kind, nq, seed):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, D)).astype(np.float32)
    if kind == "dominant":                                       # one element 40 x the rest: the step is set by it
        q[np.arange(nq), rng.integers(0, D, nq)] = 40.0
    elif kind == "halfway":
        q[0] = ADV.halfway_query()[0]
    return q


def _check_all_pairs(oracle, x, q, planes):
    code, s_row, inv, rho_row, norm, res_row = M.quantise(x, full=True)
    off = M.offsets(res_row, D)
    qn = oracle.normalize(q)
    hi, lo, s, rho_q, real = quantise_query(qn, planes)
    assert np.all(rho_q.astype(np.float64) >= real)              # rho_q as computed bounds the realised residual
    assert np.abs(hi).max() <= 127 and (lo is None or np.abs(lo).max() <= 127)
    can = oracle.cosine(q, x).T                                  # [rows, queries]
    eps_img = np.float32(M.image_eps(D))
    eps_q = np.array([q8_bound(r, eps_img, 0, 0)[0] for r in rho_q], dtype=np.float64)
    worst = 0.0
    for key in keys(code.astype(np.int32), inv, off, hi, lo, s):
        # every pair, whatever the row: the 65 / 64 is PROVEN for rows with rho_row <= 1 / 64 only (the library keeps no image of a shard
        # with a worse row: kImageMaxRho) -- "heavy" rows lie above it (rho_row ~ 0.1) and pass on Cauchy-Schwarz's slack
        gap = can - key.astype(np.float64) - eps_q[None, :]
        worst = max(worst, float(gap.max()))
        assert gap.max() <= 0.0, (planes, float(gap.max()))
    return rho_q, worst


@pytest.mark.parametrize("planes", [1, 2])
@pytest.mark.parametrize("kind", ["gauss", "clustered", "heavy"])
@pytest.mark.parametrize("qkind", ["gauss", "halfway", "dominant"])
def test_eps_q_bounds_every_pair(oracle, kind, qkind, planes):
    x = M._rows(kind, 3000, D, 11 + D)
    q = _queries(qkind, 16, 5)
    rho_q, _ = _check_all_pairs(oracle, x, q, planes)
    if planes == 1 and qkind == "gauss":
        assert 0.006 < rho_q.mean() < 0.009 and rho_q.max() < 0.013   # the issue's 7.66e-3 mean, 1.2e-2 max
    if planes == 1 and qkind == "dominant":
        assert rho_q.min() > 0.03                                    # a coarse step: several times an ordinary query's residual
    if planes == 2 and qkind != "dominant":
        assert rho_q.max() < 1e-4


@pytest.mark.parametrize("planes", [1, 2])
def test_eps_q_on_hostile_rows(oracle, planes):
    """Rows parallel to the half-way query (tests/test_scan_image_model.py's hostile case): the query's and the rows' quantisation
    residuals add up along the same direction."""
    q, _ = ADV.halfway_query()
    qn = oracle.normalize(q[None, :])[0]
    rows = np.stack([qn * (1 + 1e-3 * i) for i in range(64)]).astype(np.float16).astype(np.float32)
    _check_all_pairs(oracle, rows, q[None, :], planes)


@pytest.mark.parametrize("rho_q", [0.0, 4.8e-5, 0.00766, 0.012, 0.0525, 0.5])
def test_library_bound_and_bands_match_the_model(rho_q):
    """vf_debug_image_q8_bound: the test build's hook onto image_q8_bound / image_q8_eps (host code only: no GPU needed)."""
    from veritasfi_amd import build as B
    lib = ctypes.CDLL(B.TEST_LIB)
    eps_img, tb0, fb0 = np.float32(M.image_eps(D)), 16, 231
    eps, tb, fb = ctypes.c_float(), ctypes.c_int32(), ctypes.c_int32()
    rc = lib.vf_debug_image_q8_bound(ctypes.c_float(rho_q), ctypes.c_float(float(eps_img)), ctypes.c_int32(tb0), ctypes.c_int32(fb0),
                                     ctypes.byref(eps), ctypes.byref(tb), ctypes.byref(fb))
    assert rc == 0
    want = q8_bound(rho_q, eps_img, tb0, fb0)
    assert np.float32(eps.value) == want[0] and (tb.value, fb.value) == want[1:]
    assert eps.value >= float(eps_img) + float(np.float32(rho_q)) * 65.0 / 64.0 + 2.0 ** -20 - 1e-12


def test_a_residual_without_a_bound_gives_no_certificate():
    from veritasfi_amd import build as B
    lib = ctypes.CDLL(B.TEST_LIB)
    eps, tb, fb = ctypes.c_float(), ctypes.c_int32(), ctypes.c_int32()
    for bad in (float("inf"), float("nan"), 1.0):
        assert lib.vf_debug_image_q8_bound(ctypes.c_float(bad), ctypes.c_float(6e-4), ctypes.c_int32(16), ctypes.c_int32(231),
                                           ctypes.byref(eps), ctypes.byref(tb), ctypes.byref(fb)) == 0
        assert eps.value == float("inf") and tb.value >= 2048
