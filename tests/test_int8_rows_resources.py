"""The int8-row forms of the scans -- k_scan<NT, G, MODE, 2> in every (NT, G, MODE) shape the e4m3 form has and k_scan_wide<MODE, 2>, the
biased bytes converted by cvt8_i8b -- exist, use no scratch, spill no vector register, have no dynamic stack and fit the register budget
of their launch bounds (512 threads: two waves per SIMD, 256 registers a lane).  k_final, which gained the int8 re-score, stays without
scratch, and the re-biasing pass is a kernel of its own.  hipcc's own remarks through tools/resource_usage.py: cross-compiled, no GPU."""
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


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc"), "hipcc is needed (it cross-compiles: no GPU)"
    from veritasfi_amd import build as vf_build
    return {k["pretty"]: k for k in _tool().usage(os.path.join(vf_build.CSRC, "vf_kernels.hip"))}


def _clean(kernels, name, budget=256, min_occupancy=2):
    assert name in kernels, name
    k = kernels[name]
    print(name, {x: k.get(x) for x in ("vgprs", "agprs", "sgpr_spill", "scratch", "vgpr_spill", "occupancy")})
    assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0, (name, k)
    assert str(k.get("dynamic_stack", "False")) != "True", name
    assert k.get("vgprs", 0) + k.get("agprs", 0) <= budget and k["occupancy"] >= min_occupancy, (name, k)


def test_int8_forms_of_k_scan_exist_in_every_e4m3_shape_without_scratch(kernels):
    e4m3 = sorted(n for n in kernels if n.startswith("k_scan<") and n.endswith(",1>"))
    assert len(e4m3) == 16, e4m3                              # NT 1 / 2 x G 1 .. 4 x sample / main
    for nt in (1, 2):
        for g in (1, 2, 3, 4):
            for mode in (0, 1):
                assert f"k_scan<{nt},{g},{mode},1>" in kernels
                _clean(kernels, f"k_scan<{nt},{g},{mode},2>")
    assert len([n for n in kernels if n.startswith("k_scan<") and n.endswith(",2>")]) == 16


def test_int8_forms_of_k_scan_wide_exist_without_scratch(kernels):
    for mode in (0, 1):
        _clean(kernels, f"k_scan_wide<{mode},2>")


def test_k_final_with_the_int8_rescore_and_the_rebias_pass(kernels):
    _clean(kernels, "k_final", budget=256, min_occupancy=2)
    _clean(kernels, "k_rebias_i8", budget=64, min_occupancy=8)
