"""k_scan_ksplit's instantiations (both modes, segments per wave 10 .. 16) exist, use no scratch, spill no vector register and run
one wave per SIMD; the two k_scan instantiations tests/test_kernel_resources.py tolerates scratch in are still there, unchanged in
that respect.  hipcc's own remarks through tools/resource_usage.py: cross-compiled, no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(10, 10), (11, 11), (12, 6), (13, 13), (14, 7), (15, 5), (16, 8)]   # (segments per wave, ring depth): VF_KSPLIT_SHAPES


def _tool():
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_ksplit_scan_has_no_scratch_and_one_wave_per_simd():
    assert os.path.exists("/opt/rocm/bin/hipcc") or __import__("shutil").which("hipcc"), "hipcc is needed (it cross-compiles: no GPU)"
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in _tool().usage(os.path.join(vf_build.CSRC, "vf_kernels.hip"))}
    for mode in (0, 1):
        for p, d in SHAPES:
            name = f"k_scan_ksplit<{mode},{p},{d}>"
            assert name in kernels, name
            k = kernels[name]
            print(name, {x: k.get(x) for x in ("vgpr", "agpr", "sgpr_spill", "scratch", "vgpr_spill", "occupancy")})
            assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k["occupancy"] == 1, (name, k)
            assert str(k.get("dynamic_stack", "False")) != "True", name
    assert len([n for n in kernels if n.startswith("k_scan_ksplit<")]) == 2 * len(SHAPES)
    for name in ("k_scan<2,4,1,0>", "k_scan<2,4,0,0>"):   # allow-listed there: they must keep matching kernels that have scratch
        assert name in kernels and kernels[name].get("scratch", 0) > 0, name
