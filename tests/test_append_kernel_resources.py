"""k_append_rows and the create-time kernels it shares its device functions with stay free of scratch memory and register spills
(hipcc's own remarks on the product's flags, through tools/resource_usage.py; hipcc cross-compiles: no GPU needed).  The append runs once
per ingest batch of 100 rows, so its one launch is the whole device cost of a call: a scratch access in it would be most of that."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_append_and_create_time_kernels_use_no_scratch():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    spec = importlib.util.spec_from_file_location("resource_usage", os.path.join(ROOT, "tools", "resource_usage.py"))
    ru = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ru)
    from veritasfi_amd import build as vf_build
    kernels = {k["pretty"]: k for k in ru.usage(os.path.join(vf_build.CSRC, "vf_kernels.hip"))}
    for name in ("k_append_rows", "k_prep_rows", "k_prep_image", "k_normalize_rows", "k_rebias_i8"):
        k = kernels[name]
        assert k.get("scratch", 0) == 0 and k.get("vgpr_spill", 0) == 0 and k.get("sgpr_spill", 0) == 0, k
        assert str(k.get("dynamic_stack", "False")) != "True", k
