"""The registers and LDS of the kernels behind a dense batch with a row list per query (hipcc's remarks, tools/resource_usage.py: no GPU).

k_scan_subset_m runs k_scan_subset's body behind a tile table, so what tests/test_subset_kernel_resources.py pins for that kernel is
pinned here for each of the four row types by name: 2 rows x 4 queries x 8 partial sums per lane live in registers, all indexed by
fully unrolled loops -- one index the compiler cannot resolve (the tile's four query indexes are selected, not indexed, for that
reason) and the arrays go to scratch -- so no scratch, no spills, no dynamic stack; two waves per SIMD, which is at most 256
registers; LDS is one tile of 4 queries x one K-slice of 1024 elements x 4 bytes = 16 384 bytes whatever d is.  The check and map
kernels are plain grid loops: no scratch, no LDS.  (profiles/r23_subset_multi_resources.txt holds the tables of this and the parent
commit; k_scan_subset itself is held by the existing test.)"""
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


def test_k_scan_subset_m_resources():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    ru = _tool()
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in ru.usage(os.path.join(vf_build.CSRC, "vf_kernels.hip"))}
    for dt in (0, 1, 2, 3):   # VF_DTYPE_F32, _F16, _FP8_E4M3, _INT8
        k = kernels.get(f"k_scan_subset_m<{dt}>")
        assert k is not None, (dt, sorted(n for n in kernels if "subset" in n))
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert str(k.get("dynamic_stack", "False")) == "False", k
        assert k["lds"] == 4 * 1024 * 4, k
        assert k["vgprs"] + k.get("agprs", 0) <= 256 and k["occupancy"] >= 2, k
    for name in ("k_subset_check_m", "k_subset_ids_m"):
        assert kernels[name].get("scratch", 0) == 0 and kernels[name].get("lds", 0) == 0, kernels[name]
