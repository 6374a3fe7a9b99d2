"""What the library reports of a search against the route the host-compiled driver (tests/scan_route_driver.py, vf_route.h) predicts for
the same inputs: path, scan_kernel, scan_image, wide_launches, wide_queries, aux_cus and scans_overlap -- and, with the profile on, the
bytes the library says a timed main scan reads (scan_bytes_per_launch) against the driver's scan_bytes of the search's first pass.

20 000 rows (the smallest kind of index the fused path serves on its own) of 768 elements as fp16, e4m3 and int8 (scan_image = 2: the
index is its own image), and of 2560 elements as fp16 and e4m3 under wide_rows = 2, each with 1, 33, 65 and 130 queries: every branch of
the route but the row-count thresholds, which tests/test_scan_route.py walks on the CPU.  The driver takes the CU count from the device
and the CU split from what the library reports it applied."""
import numpy as np
import pytest

import scan_route_driver as drv

pytestmark = pytest.mark.gpu

N, K = 20000, 100
KEYS = ("path", "scan_kernel", "scan_image", "wide_launches", "wide_queries", "aux_cus", "scans_overlap")
# (dtype, d, options set before the first search)
INDEXES = [("f16", 768, {}), ("e4m3", 768, {}), ("int8", 768, {"scan_image": 2}), ("f16", 2560, {"wide_rows": 2}), ("e4m3", 2560, {"wide_rows": 2})]


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


def _index(vf, dtype, d, rng):
    if dtype == "f16":
        return vf.DenseIndex(rng.standard_normal((N, d), dtype=np.float32).astype(np.float16))
    if dtype == "int8":
        return vf.DenseIndex.from_int8(rng.integers(-128, 128, size=(N, d), dtype=np.int8))
    codes = rng.integers(0, 0x7F, size=(N, d), dtype=np.uint8) | (rng.integers(0, 2, size=(N, d), dtype=np.uint8) << 7)   # no NaN code
    return vf.DenseIndex.from_e4m3(codes)


@pytest.mark.parametrize("dtype,d,options", INDEXES, ids=[f"{t}-{d}" for t, d, _ in INDEXES])
def test_reported_route_is_the_predicted_one(vf, driver, dtype, d, options):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(7)
    with _index(vf, dtype, d, rng) as ix:
        for name, value in options.items():
            ix.set_option(name, value)
        ix.set_option("profile", 1)
        got, got_bytes = [], []
        for nq in (1, 33, 65, 130):
            ix.search(rng.standard_normal((nq, d), dtype=np.float32), K)
            got.append(ix.stats())
            got_bytes.append(ix.profile()["scan_bytes_per_launch"])   # (of the latest timed search's first pass)
    has_image = 1 if options.get("scan_image") == 2 else 0   # (the int8 index is its own image; 20 000 rows of fp16 / e4m3 build none)
    cases = [dict(dtype=dtype, n=N, d=d, nq=nq, k=K, n_cu=n_cu, has_image=has_image, aux_applied=g["aux_cus"], **options)
             for nq, g in zip((1, 33, 65, 130), got)]
    want = drv.evaluate(driver, cases)
    for nq, g, gb, w in zip((1, 33, 65, 130), got, got_bytes, want):
        print(dtype, d, nq, {k: g[k] for k in KEYS}, "scan_bytes_per_launch", gb, w)
        assert {k: g[k] for k in KEYS} == {k: w[k] for k in KEYS}, f"{dtype} {N} x {d}, {nq} queries"
        assert gb == w["scan_bytes"] and gb > 0, f"{dtype} {N} x {d}, {nq} queries: scan bytes"
        assert g["path"] == 1   # every one of these searches is the fused path's: the comparison above is about its kernels
