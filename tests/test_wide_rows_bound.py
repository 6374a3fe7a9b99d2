"""The certificate's summation term covers k_scan_ksplit's order of additions (make_plan in vf_route.h; tests/adversarial.py's
eps_bound restates the bound).

The kernel adds a row's dp products in fp32 per wave -- a quarter of the row's 64-element segments each, 16 k-slots per matrix
instruction -- and then the four partial sums in the fixed order ((p0 + p1) + p2) + p3.  That is one sum of the same dp terms
with dp - 1 additions, so the classical bound |fl(sum) - sum| <= (dp - 1) 2^-24 sum |x_i| (1 + O(dp 2^-24)) holds whatever the
order; with unit vectors rounded to fp16, sum |x_i| <= 1 + 2^-11 and the scan's share of eps, d 2^-24, is the bound.  This test
models the order in NumPy (fp32 adds, sequential inside a 16-slot group as the harshest reading of the instruction, groups and
segments in the kernel's order, the quarters last) and measures the error against the fp64 dot product of the SAME fp16 operands:
random unit vectors, and vectors whose products all have one sign (every addition rounds a growing sum: the worst case for a
sequential order).  No GPU."""
import numpy as np
import pytest

from adversarial import eps_bound

SEG = 64


def _seg_begin(S, w):
    return S * w // 4


def ksplit_sum(q16, r16):
    """fp32 model of the kernel's sum for one (query, row) pair of fp16 vectors of dp elements."""
    dp = q16.shape[0]
    S = dp // SEG
    prod = q16.astype(np.float32) * r16.astype(np.float32)          # an fp16 x fp16 product is exact in fp32
    parts = []
    for w in range(4):
        acc = np.float32(0.0)
        for sg in range(_seg_begin(S, w), _seg_begin(S, w + 1)):
            seg = prod[sg * SEG:(sg + 1) * SEG].reshape(8, 8)       # element group c = 4 h + i, j
            for i in range(4):                                       # one matrix instruction: k-slots (h, j) of step i
                for h in range(2):
                    for j in range(8):
                        acc = np.float32(acc + seg[4 * h + i, j])
        parts.append(acc)
    return np.float32(np.float32(np.float32(parts[0] + parts[1]) + parts[2]) + parts[3])


def _unit16(v):
    v = v / np.linalg.norm(v)
    return v.astype(np.float32).astype(np.float16)


@pytest.mark.parametrize("d", [2560, 4096, 2500, 3000])
def test_the_quartered_sum_stays_within_the_scan_share_of_eps(d):
    dp = (d + 127) // 128 * 128
    rng = np.random.default_rng(d)
    share = d * 2.0 ** -24 * (1.0 + 2.0 ** -11)                      # the scan's fp32 sum in make_plan's eps (the other d 2^-24 is the canonical sum's)
    assert share < eps_bound(d, 2.0 ** -11) - 2.0 ** -11             # ... and it is inside the bound the library uses
    worst = 0.0
    cases = []
    for _ in range(6):                                               # random directions
        cases.append((rng.standard_normal(d), rng.standard_normal(d)))
    for _ in range(3):                                               # all products positive: |q| . |r|, the sum of magnitudes itself
        a = np.abs(rng.standard_normal(d))
        cases.append((a, a * np.exp(rng.uniform(-0.3, 0.3, d))))
    flat = np.ones(d)                                                # equal entries: cosine 1, every addition rounds a growing sum
    cases.append((flat, flat))
    cases.append((flat, -flat))
    for a, b in cases:
        q16, r16 = np.zeros(dp, np.float16), np.zeros(dp, np.float16)
        q16[:d], r16[:d] = _unit16(a), _unit16(b)
        exact = float(q16.astype(np.float64) @ r16.astype(np.float64))
        mags = float(np.abs(q16.astype(np.float64)) @ np.abs(r16.astype(np.float64)))
        assert mags <= (1.0 + 2.0 ** -11) ** 2
        err = abs(float(ksplit_sum(q16, r16)) - exact)
        worst = max(worst, err)
        assert err <= share, (d, err, share)
    print(f"d = {d}: worst |fp32 quartered sum - fp64| = {worst:.3e}, the scan's share of eps = {share:.3e}")
