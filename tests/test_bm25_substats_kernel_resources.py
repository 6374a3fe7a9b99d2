"""The kernels of a BM25 search scored by the subset's own statistics (k_bm25_sub_len, k_bm25_sub_df, k_bm25_accum_s,
csrc/vf_sparse.hip): no scratch memory, no register spills, at most 64 VGPRs and no AGPRs (8 waves per SIMD as far as registers go)
-- the two counting kernels are traffic and a reduction, the scatter adds a handful of float64 operations per posting.  hipcc's own
remarks on the product's flags, through tools/resource_usage.py; hipcc cross-compiles: no GPU needed."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSTATS = ("k_bm25_sub_len", "k_bm25_sub_df", "k_bm25_accum_s")


def test_substats_kernels_use_no_scratch_and_at_most_64_registers():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in ru.usage(os.path.join(vf_build.CSRC, "vf_sparse.hip"))}
    for name in SUBSTATS:
        k = kernels[name]
        print(k)
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert str(k.get("dynamic_stack", "False")) != "True", k
        assert k.get("vgprs", 0) <= 64 and k.get("agprs", 0) == 0, k
