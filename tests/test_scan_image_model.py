"""The int8 scan image's certificate, modelled in NumPy on the CPU: the quantiser k_prep_image applies, the score key
k_scan2r forms from it (approximate score + the row's offset), and the bound the library uses (vf_debug_image_bound) -- canonical <= key
+ eps for every row, with the fp16 path's eps, on random, clustered and hostile rows; and the key is never more than 2 off + eps above.
Rows on the quantiser's own lattice ("exact": no residual at all) and rows whose residual is parallel to a sign-vector query ("aligned":
the approximate score understates the canonical one by rho_row itself) show that the offset is tight, i.e. that such data can SEE an
offset the scan lost or halved; hostile_case builds the planted rows tests/test_gpu_scan_image.py searches through the device's image."""
import numpy as np
import pytest

import adversarial as ADV


def quantise(x, full=False):
    """k_prep_image: per row s = absmax / 127 (fp32), code = rint(x / s) clamped to +-127, rho = ||x - s code|| / norm (fp64, rounded
    UP to fp32), inv = s / norm; returns (codes int8, s, inv fp32, rho fp32, norm fp32 -- the canonical norm), and with `full` the
    residual in fp64 before its rounding as well: what the kernel forms the offset from."""
    x = np.asarray(x, dtype=np.float32)
    mx = np.abs(x).max(axis=1)
    s = np.where(mx > 0, mx / np.float32(127.0), np.float32(1.0)).astype(np.float32)
    code = np.clip(np.rint(x / s[:, None]), -127, 127).astype(np.int8)
    norm = canonical_norm(x)
    res = np.sqrt(((x.astype(np.float64) - s[:, None].astype(np.float64) * code) ** 2).sum(axis=1)) / norm
    rho = res.astype(np.float32)
    rho = np.where(rho.astype(np.float64) < res, np.nextafter(rho, np.float32(np.inf)), rho)
    inv = (s.astype(np.float64) / norm).astype(np.float32)
    return (code, s, inv, rho, norm, res) if full else (code, s, inv, rho, norm)


def offsets(res, d):
    """off_img: r (1 + 2^-11)(1 + 2^-20) + d 2^-24 r in fp64, rounded up to fp32 -- of the fp64 residual r itself (quantise(x, full=True)),
    as k_prep_image forms it, NOT of rho, its fp32 form rounded up (that offset is the same or one ulp larger: the device prep test of
    tests/test_gpu_scan_image.py told the two apart)."""
    od = np.asarray(res, dtype=np.float64) * (1 + 2.0 ** -11) * (1 + 2.0 ** -20) + d * 2.0 ** -24 * np.asarray(res, dtype=np.float64)
    off = od.astype(np.float32)
    return np.where(off.astype(np.float64) < od, np.nextafter(off, np.float32(np.inf)), off)


def canonical_norm(x):
    """sqrt in fp64 of dot16(x, x) (16 interleaved fp32 partial sums, fixed tree); zero -> 1."""
    x = np.asarray(x, dtype=np.float32)
    n, d = x.shape
    acc = np.zeros((n, 16), dtype=np.float32)
    with np.errstate(over="ignore", under="ignore"):             # (fp32 rows of 1e30 / 1e-30: the squares overflow to inf / vanish, as on the device)
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
    if kind == "exact":
        return exact_rows(lattice(n, d, rng), rng)
    if kind == "aligned":   # against the query sign_vector(d, seed)
        sigma = sign_vector(d, seed)
        return aligned_rows(lattice(n, d, rng, sigma, 0.9, rms_for_rho(rng.uniform(0.010, 0.015, n), d)), sigma, rng)
    if kind == "zero":      # every third row all zero (norm -> 1, step -> 1, every score 0), among ordinary ones
        x = rng.standard_normal((n, d)).astype(np.float16).astype(np.float32)
        x[::3] = 0.0
        return x
    if kind == "single":    # one non-zero element: code +-127 there, no residual
        x = np.zeros((n, d), dtype=np.float32)
        x[np.arange(n), rng.integers(0, d, n)] = rng.standard_normal(n).astype(np.float16).astype(np.float32) + np.float32(0.001)
        return x
    if kind == "subnormal":  # every element an fp16 subnormal, m 2^-24 with |m| < 1024
        return (rng.integers(-1023, 1024, (n, d)) * 2.0 ** -24).astype(np.float32)
    if kind in ("f32big", "f32small"):   # fp32 rows whose squares overflow (norm inf: score 0) / vanish (norm 0 -> 1)
        return (rng.standard_normal((n, d)) * (1e30 if kind == "f32big" else 1e-30)).astype(np.float32)
    if kind == "tie":       # x / s exactly on .5 for every element but the one that sets the step: rint's tie, to even
        c, peak = lattice(n, d, rng)
        h = c + np.where(c >= 0, 0.5, -0.5)
        h[np.arange(n), peak] = c[np.arange(n), peak]
        return (h * 2.0 ** rng.integers(-9, -3, n)[:, None]).astype(np.float32)
    raise ValueError(kind)


EDGE_KINDS = ("exact", "aligned", "zero", "single", "subnormal", "f32big", "f32small", "tie")


def sign_vector(d, seed):
    """A query whose normalised entries all have one magnitude: sigma / sqrt(d)."""
    return np.random.default_rng(1000 + seed).choice(np.array([-1.0, 1.0], dtype=np.float32), size=d)


def rms_for_rho(rho, d):
    """The element rms at which an "aligned" row has residual rho: ||delta|| = (7/16) sqrt(d - 1) against ||c + delta|| = rms sqrt(d)."""
    return 0.4375 * np.sqrt((d - 1.0) / d) / np.asarray(rho, dtype=np.float64)


def lattice(n, d, rng, sigma=None, cos=None, rms=None):
    """Integer codes c [n, d] in [-126, 126] with ONE element per row exactly +-127 (it sets the row's step), and where it sits.  Without
    sigma: uniform.  With sigma: c ~ rint(sigma a + t N(0, 1)) with a = cos rms, t = sqrt(1 - cos^2) rms -- a row of that element rms whose
    cosine to sigma is about cos (callers SELECT on the values as stored)."""
    if sigma is None:
        c = rng.integers(-126, 127, (n, d)).astype(np.float64)
        top = rng.choice([-127.0, 127.0], n)
    else:
        cos = np.broadcast_to(np.asarray(cos, dtype=np.float64), (n,))
        rms = np.broadcast_to(np.asarray(rms, dtype=np.float64), (n,))
        c = sigma[None, :] * (cos * rms)[:, None] + (np.sqrt(1.0 - cos ** 2) * rms)[:, None] * rng.standard_normal((n, d))
        c = np.clip(np.rint(c), -126, 126)
    peak = rng.integers(0, d, n)
    c[np.arange(n), peak] = top if sigma is None else 127.0 * sigma[peak]
    return c, peak


def exact_rows(lat, rng):
    """Rows s c, s a power of two: on the quantiser's own lattice, so codes = c, rho = 0 and off = 0 (fp16 holds them exactly)."""
    c, _ = lat
    return (c * 2.0 ** rng.integers(-9, -3, c.shape[0])[:, None]).astype(np.float32)


def aligned_rows(lat, sigma, rng):
    """Rows s (c + delta), delta = (7/16) sigma except 0 on the +-127 element: codes = c, and the residual s delta is parallel to the
    query sigma / sqrt(d) (but for that one element), so the approximate score understates the canonical one by rho_row (Cauchy-Schwarz
    with equality).  16 |c + delta| <= 2023 < 2^11: every value is an fp16 number."""
    c, peak = lat
    delta = np.broadcast_to(0.4375 * sigma.astype(np.float64), c.shape).copy()
    delta[np.arange(c.shape[0]), peak] = 0.0
    x = ((c + delta) * 2.0 ** rng.integers(-9, -3, c.shape[0])[:, None]).astype(np.float32)
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
    return x


def hostile_case(oracle, seed, d=768, k=100, victims=32, decoys=220):
    """Planted rows for ONE sign-vector query (returned unnormalised: sigma): `victims` aligned rows with rho_row in [0.011, 0.0153]
    (<= 1/64: the image stays) whose canonical scores are the best of the shard, and `decoys` exact rows (off = 0) just below them -- far
    above the victims' keys without their offsets.  The top k is then the victims plus the best k - victims decoys; a victim whose offset
    the scan lost, halved or took from a neighbour (an exact row: 0) falls out of the re-score band while the k-th key stays with the
    decoys, and the certificate passes on a wrong answer.  Both kinds are SELECTED on their values as stored (as adversarial.build_case
    does): decoys with canonical score in [V - 5e-4, V - 1e-4], victims in [V + 5e-5, V + 5.5e-4], V = 0.9.  The background must lie far
    below (uniform lattice rows against a sign vector: cos ~ N(0, 1 / d), 0.2 at most over millions of rows)."""
    V = 0.9
    rng = np.random.default_rng(seed)
    sigma = sign_vector(d, seed)
    q = sigma[None, :].astype(np.float32)

    def pick(make, lo, hi, want, tries, rho_range=None):
        got = []
        for _ in range(8):
            x = make(tries)
            can = oracle.cosine(q, x)[0].astype(np.float64)
            ok = (can > lo) & (can < hi)
            if rho_range is not None:
                rho = quantise(x)[3]
                ok &= (rho >= rho_range[0]) & (rho <= rho_range[1])
            got.append(x[ok])
            if sum(g.shape[0] for g in got) >= want:
                return np.concatenate(got)[:want]
        raise AssertionError(f"only {sum(g.shape[0] for g in got)} of {want} rows met the window")

    spread = lambda m: V + rng.uniform(-0.004, 0.004, m)
    vic = pick(lambda m: aligned_rows(lattice(m, d, rng, sigma, spread(m), rms_for_rho(rng.uniform(0.0113, 0.0150, m), d)), sigma, rng),
               V + 5e-5, V + 5.5e-4, victims, 4000, (0.011, 0.0153))
    dec = pick(lambda m: exact_rows(lattice(m, d, rng, sigma, spread(m), rng.uniform(28.0, 40.0, m)), rng), V - 5e-4, V - 1e-4, decoys, 8000)
    return {"query": q[0], "victims": vic, "decoys": dec}


def hostile_margins(oracle, cases, n_shard, k=100, d=768):
    """The biting check on the model, for every image_mfma form: for each case's query, over ALL planted rows (the background lies far
    below), cut = (k-th best key) - B - eps_q with B = image_band of the shard's modelled rho_mean (background rows: rho = 0).  Returns
    per form the smallest margins (cut - key without offset, cut - key with half the offset, key with the offset - cut) over every
    victim of every case, and the victims' rho range."""
    import test_scan_image_q8_model as Q
    rows = np.concatenate([np.concatenate([c["victims"], c["decoys"]]) for c in cases])
    code, s, inv, rho, norm, res = quantise(rows, full=True)
    off = offsets(res, d)
    B = float(image_band(d, float(rho.astype(np.float64).sum() / n_shard)))
    eps_img = np.float32(image_eps(d))
    out = {}
    at = 0
    for ci, c in enumerate(cases):
        nv, per = c["victims"].shape[0], c["victims"].shape[0] + c["decoys"].shape[0]
        vsel = np.arange(at, at + nv)
        at += per
        qn = oracle.normalize(c["query"][None, :])
        assert rho[vsel].max() <= 1.0 / 64 and not rho[vsel[-1] + 1:vsel[0] + per].any()     # victims keep the image; decoys have no residual
        for form in (0, 1, 2):
            if form == 0:
                raw = approx_scores(qn.T, code, inv[:, None])[:, 0]
                eps_q = float(eps_img)
            else:
                hi, lo, sq, rho_q, _ = Q.quantise_query(qn, form)
                raw = Q.keys(code.astype(np.int32), inv, np.zeros_like(off), hi, lo, sq)[0][:, 0]
                eps_q = float(Q.q8_bound(rho_q[0], eps_img, 0, 0)[0])
            full = (raw + off).astype(np.float32).astype(np.float64)
            cut = np.sort(full)[::-1][k - 1] - B - eps_q
            half = raw.astype(np.float64) + 0.5 * off
            m = out.setdefault(form, [np.inf, np.inf, np.inf])
            m[0] = min(m[0], float((cut - raw[vsel]).min()))
            m[1] = min(m[1], float((cut - half[vsel]).min()))
            m[2] = min(m[2], float((full[vsel] - cut).min()))
    return out, (float(rho[rho > 0].min()), float(rho.max())), B


@pytest.mark.parametrize("kind,d", [("gauss", 768), ("gauss", 1024), ("clustered", 768), ("heavy", 768)] + [(kind, 768) for kind in EDGE_KINDS])
def test_rho_bounds_the_residual_and_eps_bounds_the_score_error(oracle, kind, d):
    x = _rows(kind, 3000, d, 11 + d)
    code, s, inv, rho, norm, res = quantise(x, full=True)
    # rho is an upper bound of the realised residual (fp64) and the codes are in range
    real = np.sqrt(((x.astype(np.float64) - s[:, None].astype(np.float64) * code) ** 2).sum(axis=1)) / norm
    assert np.all(rho.astype(np.float64) >= real) and np.abs(code.astype(np.int32)).max() <= 127
    q = np.random.default_rng(5).standard_normal((16, d)).astype(np.float32)
    qn = oracle.normalize(q)
    key = (approx_scores(qn.T, code, inv[:, None]) + offsets(res, d)[:, None]).astype(np.float32)
    can = oracle.cosine(q, x).T
    eps = image_eps(d)
    assert (can - key.astype(np.float64)).max() <= eps
    assert (key.astype(np.float64) - can - 2 * offsets(res, d)[:, None]).max() <= eps
    # N(0, 1) rows: rho ~ 7.8e-3 on average, the shard's maximum well above it (a row's absmax sets its step): DESIGN.md 2
    if kind == "gauss":
        assert 0.006 < rho.mean() < 0.009 and rho.max() < 1.0 / 64
    if kind == "exact":                                          # on the lattice: no residual, no offset
        assert not rho.any() and not offsets(res, d).any()
    if kind == "single":                                         # (127 x fp32(x / 127) is x to a rounding)
        assert rho.max() < 2.0 ** -23
    if kind == "aligned":
        assert 0.0095 < rho.min() and rho.max() < 1.0 / 64


def test_aligned_rows_make_the_offset_tight(oracle):
    """The sign-vector query against rows whose residual is parallel to it: the approximate score understates the canonical one by
    u >= rho_row (sqrt((d - 1) / d) - 2^-11) - 2^-11 - d 2^-23 (the residual's one zero element, the fp16 rounding of the query, the two
    fp32 sums), so key + eps - canonical = eps + off_row - u <= 2 eps + 2e-3 off_row: an eighth of off_row at rho_row = 0.010.  The key
    WITHOUT the offset, and with half of it, violates canonical <= key + eps on every such row: data on which a lost offset shows."""
    d, seed = 768, 21
    x = _rows("aligned", 512, d, seed)
    code, s, inv, rho, norm, res = quantise(x, full=True)
    off = offsets(res, d).astype(np.float64)
    q = sign_vector(d, seed)[None, :]
    qn = oracle.normalize(q)
    assert np.abs(np.abs(qn) - np.abs(qn[0, 0])).max() == 0       # one magnitude
    raw = approx_scores(qn.T, code, inv[:, None])[:, 0].astype(np.float64)
    key = (raw + off).astype(np.float32).astype(np.float64)
    can = oracle.cosine(q, x)[0].astype(np.float64)
    eps = image_eps(d)
    slack = key + eps - can
    print(f"aligned rows: rho {rho.min():.4f}..{rho.max():.4f}, (key + eps - canonical) / off {(slack / off).min():.3f}..{(slack / off).max():.3f}, "
          f"canonical - (key without offset + eps) >= {(can - raw - eps).min():.4f}")
    assert slack.min() >= 0
    assert np.all(slack <= 2 * eps + 2e-3 * off) and np.all(slack < off / 7)
    assert np.all(raw + eps < can) and np.all(raw + 0.5 * off + eps < can)


def test_hostile_case_bites_on_the_model(oracle):
    """hostile_case / hostile_margins as tests/test_gpu_scan_image.py uses them (one query here): a victim's key without its offset and
    with half of it lies more than a coarse bin (2^-10) below the cut of every image_mfma form, its key with the offset above it."""
    cases = [hostile_case(oracle, 7801)]
    margins, (rho_lo, rho_hi), band = hostile_margins(oracle, cases, 4_000_037)
    print(f"victims' rho {rho_lo:.5f}..{rho_hi:.5f}, band {band:.5f}, margins (no offset, half, full) per form: {margins}")
    assert 0.011 <= rho_lo and rho_hi <= 1.0 / 64
    for form, (none, half, full) in margins.items():
        assert none >= 2.0 ** -10 and half >= 2.0 ** -10 and full > 0, (form, none, half, full)
    can_v = oracle.cosine(cases[0]["query"][None, :], cases[0]["victims"])[0]
    can_d = oracle.cosine(cases[0]["query"][None, :], cases[0]["decoys"])[0]
    assert can_v.min() > can_d.max() and cases[0]["decoys"].shape[0] >= 200


def test_eps_on_hostile_rows(oracle):
    """The half-way query of tests/adversarial.py against rows parallel to it: the fp16 query rounding all one way plus the rows'
    quantisation, still inside the bound."""
    q, _ = ADV.halfway_query()
    qn = oracle.normalize(q[None, :])[0]
    rows = np.stack([qn * (1 + 1e-3 * i) for i in range(64)]).astype(np.float16).astype(np.float32)
    code, s, inv, rho, norm, res = quantise(rows, full=True)
    key = (approx_scores(qn[:, None], code, inv[:, None])[:, 0] + offsets(res, 768)).astype(np.float32)
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
