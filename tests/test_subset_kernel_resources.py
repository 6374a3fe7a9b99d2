"""k_scan_subset's registers and LDS are the ones DESIGN.md section 4.2 states (hipcc's remarks, tools/resource_usage.py: no GPU).

Why each figure is pinned.  The kernel keeps 2 rows x 4 queries x 8 partial sums = 64 accumulators per lane beside the row vectors in
flight, all indexed by fully unrolled loops: one index the compiler cannot resolve and the arrays go to scratch, which turns every
multiply-add into a memory access -- so no scratch, no spills, no dynamic stack (the existing tests/test_kernel_resources.py holds the
same for every kernel whose name starts with k_scan; this test says it for each of the four row types by name).  The design counts on
two waves per SIMD, eight one-wave workgroups per CU, to keep 64 KB of row loads in flight per CU: that is at most 256 registers.  The
LDS is one tile of 4 queries x one K-slice of 1024 elements x 4 bytes = 16 384 bytes whatever d is, which is what lets those eight
workgroups (128 KB) share a CU's 160 KB -- the plan (vf_subset.h) states the same number and tests/test_subset_plan.py holds it there."""
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


def test_k_scan_subset_resources():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    ru = _tool()
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in ru.usage(os.path.join(vf_build.CSRC, "vf_kernels.hip"))}
    for dt in (0, 1, 2, 3):   # VF_DTYPE_F32, _F16, _FP8_E4M3, _INT8
        k = kernels.get(f"k_scan_subset<{dt}>")
        assert k is not None, (dt, sorted(n for n in kernels if "subset" in n))
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert str(k.get("dynamic_stack", "False")) == "False", k
        assert k["lds"] == 4 * 1024 * 4, k
        assert k["vgprs"] + k.get("agprs", 0) <= 256 and k["occupancy"] >= 2, k
    for name in ("k_subset_check", "k_subset_ids"):
        assert kernels[name].get("scratch", 0) == 0 and kernels[name].get("lds", 0) == 0, kernels[name]
