"""The registers and scratch of the three kernels that evaluate a metadata filter (hipcc's remarks, tools/resource_usage.py: no GPU).

k_where_eval keeps its evaluation stack in the bits of one register and reads leaves, ops and column pointers at uniform addresses, so
nothing is indexed per lane: no scratch, no spills, no dynamic stack, at most 64 VGPRs, no AGPRs -- the standard of the recent kernels.
k_where_scan and k_where_ids are a prefix sum and a ranked scatter under the same standard.  (profiles/r24_where_resources.txt holds the
table.)"""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_where_kernel_resources():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    ru = _tool()
    from veritasfi_amd import build as vf_build
    assert "vf_where.hip" in vf_build.SOURCES and "vf_where.h" in vf_build.HEADERS
    kernels = {k["pretty"]: k for k in ru.usage(os.path.join(vf_build.CSRC, "vf_where.hip"))}
    assert sorted(kernels) == ["k_where_eval", "k_where_ids", "k_where_scan"], sorted(kernels)
    for name, k in kernels.items():
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert str(k.get("dynamic_stack", "False")) == "False", k
        assert k["vgprs"] <= 64 and k.get("agprs", 0) == 0, k
