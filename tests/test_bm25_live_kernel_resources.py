"""The six kernels of a live BM25 update (k_bm25_live_*, csrc/vf_sparse.hip) stay free of scratch memory and register spills (hipcc's
own remarks on the product's flags, through tools/resource_usage.py; hipcc cross-compiles: no GPU needed).  They are passes over the
whole posting array that are nothing but traffic, and the two that rank a chunk in LDS must leave room for several workgroups per CU:
the rewrite holds three int arrays of kLiveMaxChunk entries and the scan's partials."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE = ("k_bm25_live_rowmap", "k_bm25_live_count", "k_bm25_live_scan", "k_bm25_live_indptr", "k_bm25_live_rewrite", "k_bm25_live_append")


def test_live_kernels_use_no_scratch_few_registers_and_a_quarter_of_the_lds_at_most():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in ru.usage(os.path.join(vf_build.CSRC, "vf_sparse.hip"))}
    for name in LIVE:
        k = kernels[name]
        print(k)
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert str(k.get("dynamic_stack", "False")) != "True", k
        assert k.get("vgprs", 0) <= 64 and k.get("agprs", 0) == 0, k      # 8 waves per SIMD as far as registers go
        assert k.get("lds", 0) <= 40 * 1024, k                            # 4 workgroups per CU of 160 KB at least
    need = (3 * 2048 + 1 + 256) * 4                                       # rank [C + 1], rows [C], col [C], part [256]
    assert need <= kernels["k_bm25_live_rewrite"]["lds"] <= need + 64, kernels["k_bm25_live_rewrite"]
