"""k_compact_rows, the mover of a removal (VF_INDEX_REMOVE), stays free of scratch memory and register spills and keeps full occupancy
(hipcc's own remarks on the product's flags, through tools/resource_usage.py; hipcc cross-compiles: no GPU needed).  It is a copy loop
with four loads in flight per thread: a scratch access in it would double the traffic of a kernel that is nothing but traffic, and a
register count above 64 would halve the waves that hide its latency."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compact_kernel_uses_no_scratch_and_few_registers():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in ru.usage(os.path.join(vf_build.CSRC, "vf_kernels.hip"))}
    k = kernels["k_compact_rows"]
    print(k)
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
    assert str(k.get("dynamic_stack", "False")) != "True", k
    assert k.get("vgprs", 0) <= 64 and k.get("agprs", 0) == 0, k      # 8 waves per SIMD
    assert k.get("lds", 0) <= 4096, k                                 # the source rows of one workgroup: 256 x 8 bytes
