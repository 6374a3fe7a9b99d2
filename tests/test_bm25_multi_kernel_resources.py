"""The kernels of a BM25 batch with a prepared filter per query (k_bm25_accum_m, k_bm25_tail_count_m, k_bm25_tail_write_m and
k_bm25_pad_out_m; csrc/vf_sparse.hip): no scratch memory, no register spills, no dynamic stack, at most 64 VGPRs and no AGPRs (8 waves
per SIMD as far as registers go), the standard of tests/test_bm25_prepared_kernel_resources.py -- the scatter holds the three forms'
bodies behind one uniform branch, so it needs what the widest of them needs; the others add a scalar read to their one-filter forms.
hipcc's own remarks on the product's flags, through tools/resource_usage.py; hipcc cross-compiles: no GPU needed."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MULTI = ("k_bm25_accum_m", "k_bm25_tail_count_m", "k_bm25_tail_write_m", "k_bm25_pad_out_m")


def test_multi_kernels_use_no_scratch_and_at_most_64_registers():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in ru.usage(os.path.join(vf_build.CSRC, "vf_sparse.hip"))}
    for name in MULTI:
        k = kernels[name]
        print(k)
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert str(k.get("dynamic_stack", "False")) != "True", k
        assert k.get("vgprs", 0) <= 64 and k.get("agprs", 0) == 0, k
