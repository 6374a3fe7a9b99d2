"""What the library would decide for a matrix product (vf_debug_gemm_route: the live knobs, the device's CU count, a workspace sized as a
handle's) against the route the host-compiled driver (tests/gemm_route_driver.py, vf_gemm_route.h) predicts for the same inputs.

A dozen of tests/test_gemm_route.py's pinned products under the default knobs, then the same products with each dispatch hook toggled
once.  Nothing is launched: the hook only asks.  (The knobs are assumed to come from a clean environment: no VF_GEMM_* variable set.)"""
import ctypes

import pytest

import gemm_route_driver as drv

pytestmark = pytest.mark.gpu

KEYS = ("kernel", "grid", "slices", "tail", "full", "ticks")
# (M, N, K, epi, kind)
PRODUCTS = [
    (51200, 768, 768, 2, 0), (51200, 3072, 768, 11, 0), (51200, 768, 3072, 2, 0), (25600, 768, 3072, 2, 0), (6656, 3072, 3072, 1, 0),
    (38400, 768, 3072, 2, 0), (12800, 768, 3072, 2, 0), (32512, 256, 768, 0, 0), (6656, 768, 3072, 2, 0), (6656, 1024, 4096, 2, 0),
    (6656, 768, 3072, 2, 10), (25600, 768, 768, 0, 7), (12288, 1024, 96, 0, 0), (8192, 2560, 2560, 3, 0),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("gemm_route"))


@pytest.fixture(scope="module")
def lib():
    from veritasfi_amd import _ffi
    L = _ffi.lib()  # raises if the HIP library is missing: no fallback
    n = _ffi.c_i32(0)
    _ffi.check(L.vf_device_count(n), "vf_device_count")
    assert n.value >= 1, "no GPU visible"
    L.vf_debug_gemm_route.restype = ctypes.c_int
    L.vf_debug_gemm_route.argtypes = [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    L.vf_debug_gemm_8p_min_wgs.restype = ctypes.c_longlong
    L.vf_debug_gemm_8p_min_wgs.argtypes = [ctypes.c_longlong]
    for name in ("vf_debug_gemm9", "vf_debug_gemm9_split", "vf_debug_splitk_tail"):
        getattr(L, name).restype = ctypes.c_int
        getattr(L, name).argtypes = [ctypes.c_int]
    return L


def _library(L):
    got = []
    for M, N, K, epi, kind in PRODUCTS:
        out = (ctypes.c_int * 6)()
        assert L.vf_debug_gemm_route(M, N, K, epi, kind, out) == 0
        got.append(dict(zip(KEYS, out)))
    return got


def test_the_library_decides_what_the_driver_predicts(lib, driver):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    # (what the driver is told, the hook call that sets it, the hook call that puts the default back)
    settings = [
        ({}, None, None),
        (dict(gemm9=0), lambda: lib.vf_debug_gemm9(0), lambda: lib.vf_debug_gemm9(-1)),
        (dict(gemm9_split=0), lambda: lib.vf_debug_gemm9_split(0), lambda: lib.vf_debug_gemm9_split(-1)),
        (dict(splitk_tail=0), lambda: lib.vf_debug_splitk_tail(0), lambda: lib.vf_debug_splitk_tail(1)),
        (dict(splitk_tail=2), lambda: lib.vf_debug_splitk_tail(2), lambda: lib.vf_debug_splitk_tail(1)),
        (dict(p8_min_wgs=1, p8_forced=1), lambda: lib.vf_debug_gemm_8p_min_wgs(1), lambda: lib.vf_debug_gemm_8p_min_wgs(-1)),
    ]
    assert lib.vf_debug_splitk_tail(-1) == 1   # the default the settings above go back to
    kernels = set()
    for knobs, set_hook, restore in settings:
        if set_hook:
            set_hook()
        try:
            got = _library(lib)
        finally:
            if restore:
                restore()
        want = drv.evaluate(driver, [dict(M=M, N=N, K=K, epi=epi, kind=kind, n_cu=n_cu, ws_auto=1, experiments=1, **knobs)
                                     for M, N, K, epi, kind in PRODUCTS])
        for p, g, w in zip(PRODUCTS, got, want):
            print(knobs, p, g, w)
            assert g == w, f"{p} under {knobs}"
            kernels.add(g["kernel"])
    assert _library(lib) == drv.evaluate(driver, [dict(M=M, N=N, K=K, epi=epi, kind=kind, n_cu=n_cu, ws_auto=1, experiments=1)
                                                  for M, N, K, epi, kind in PRODUCTS])   # every hook is back at its default
    if n_cu == 256:   # (the products were picked on the MI355X's count: there they reach every kernel of the product build)
        assert kernels >= {drv.KERNELS[k] for k in ("tn128", "dma16", "8p", "gemm9", "gemm9-split")}
    out = (ctypes.c_int * 6)()
    assert lib.vf_debug_gemm_route(100, 768, 768, 0, 0, out) == -2   # not a shape gemm() takes
