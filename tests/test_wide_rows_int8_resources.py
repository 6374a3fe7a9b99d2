"""k_scan_ksplit8i's eight instantiations (both modes, 5 .. 8 segments per wave) exist, use no scratch, spill no vector register, have no
dynamic stack and run one wave per SIMD.  hipcc's own remarks through tools/resource_usage.py: cross-compiled, no GPU.  (The kernel
shares its body with k_scan_ksplit8, whose own figures tests/test_wide_rows_fp8_resources.py holds.)"""
import importlib.util
import os
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [5, 6, 7, 8]   # segments of 128 bytes per wave: VF_KSPLIT8_SHAPES


def _tool():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_int8_ksplit_scan_has_no_scratch_and_one_wave_per_simd():
    assert os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc"), "hipcc is needed (it cross-compiles: no GPU)"
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in _tool().usage(os.path.join(vf_build.CSRC, "vf_kernels.hip"))}
    for mode in (0, 1):
        for p in SHAPES:
            name = f"k_scan_ksplit8i<{mode},{p}>"
            assert name in kernels, name
            k = kernels[name]
            print(name, {x: k.get(x) for x in ("vgprs", "agprs", "sgpr_spill", "scratch", "vgpr_spill", "occupancy")})
            assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k["occupancy"] == 1, (name, k)
            assert str(k.get("dynamic_stack", "False")) != "True", name
    assert len([n for n in kernels if n.startswith("k_scan_ksplit8i<")]) == 2 * len(SHAPES)
