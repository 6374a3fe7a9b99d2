#!/usr/bin/env python3
"""Repeat-run stress: the SAME search many times over (index built once), every run compared bit for bit with the oracle -- finds
timing-dependent faults a single run of a fuzz case can miss (round 4: the fuzz had found an intermittent wrong score in the narrow
fp8-MFMA scan variant; this loop showed 12 of 40 runs losing one row, and that none of the shipped kernels do).
    python tools/stress_repeat.py [--runs 40]"""
import argparse, importlib.util, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

CASES = [
    # (what, case, options)
    ("narrow fp8 rows, 2 queries, k = 2048 (k_scan)", dict(dtype="fp8", d=1536, nq=2, n=54938, k=2048, data="normal", seed=982935475), {}),
    ("narrow fp8 rows, same, k_scan2 with converted rows", dict(dtype="fp8", d=1536, nq=2, n=54938, k=2048, data="normal", seed=982935475), {"scan_impl": 3}),
    ("narrow fp16 rows, 64 queries (k_scan2)", dict(dtype="f16", d=768, nq=64, n=120000, k=100, data="normal", seed=11), {}),
    ("narrow fp16 rows, 3 queries, clustered data", dict(dtype="f16", d=1024, nq=3, n=200000, k=1000, data="clusters", seed=12), {}),
    ("wide fp8 rows, 200 queries (k_scan_wide8)", dict(dtype="fp8", d=1024, nq=200, n=60000, k=1000, data="normal", seed=13), {}),
    ("wide fp8 rows, 300 queries, duplicates (k_scan_wide8)", dict(dtype="fp8", d=768, nq=300, n=40000, k=100, data="dupes", seed=14), {}),
    ("wide fp8 rows, 1024 queries, k = 1000: the configs[4] call shape (k_scan_wide8)", dict(dtype="fp8", d=1024, nq=1024, n=150000, k=1000, data="normal", seed=17), {}),
    ("wide fp8 rows on the fp16 instruction (k_scan_wide)", dict(dtype="fp8", d=1024, nq=200, n=60000, k=1000, data="normal", seed=13), {"wide_mfma": 0}),
    ("wide fp16 rows, 96 queries (k_scan_wide)", dict(dtype="f16", d=768, nq=96, n=80000, k=100, data="normal", seed=15), {}),
    ("sharded handle, 3 row blocks, fp16", dict(dtype="f16", d=768, nq=64, n=150000, k=100, data="normal", seed=16, shards=3), {}),
    ("narrow fp16 rows, 64 queries: k_scan2r for the scan and the sample pass (round 6)", dict(dtype="f16", d=768, nq=64, n=200000, k=100, data="normal", seed=18), {"scan_impl": 5, "sample_impl": 1}),
    ("narrow fp16 rows, 20 queries, clustered data: k_scan2r<1>", dict(dtype="f16", d=768, nq=20, n=150000, k=1000, data="clusters", seed=19), {"scan_impl": 5, "sample_impl": 1}),
    ("narrow fp32 rows (fp16 scan copy), 64 queries, duplicates: k_scan2r", dict(dtype="f32", d=768, nq=64, n=100000, k=100, data="dupes", seed=20), {"scan_impl": 5, "sample_impl": 1}),
    # rounds 7 to 12: the int8 image route on an int8 index's own bytes (k_scan2r on the int8 matrix instruction), the conversion route, k_scan_ksplit
    ("int8 rows, 64 queries: the int8 matrix instruction, one query plane (k_scan2r, image route)", dict(dtype="int8", d=768, nq=64, n=120000, k=100, data="normal", seed=21), {"scan_image": 2, "image_mfma": 1}),
    ("int8 rows, same, hi + lo query planes", dict(dtype="int8", d=768, nq=64, n=120000, k=100, data="normal", seed=21), {"scan_image": 2, "image_mfma": 2}),
    ("int8 rows, same, converted in registers (k_scan's int8 form)", dict(dtype="int8", d=768, nq=64, n=120000, k=100, data="normal", seed=21), {"scan_image": 0}),
    ("int8 rows, 64 queries, duplicates: the image route", dict(dtype="int8", d=768, nq=64, n=120000, k=100, data="dupes", seed=22), {"scan_image": 2, "image_mfma": 1}),
    ("fp16 rows of 2560 elements, 32 queries (k_scan_ksplit)", dict(dtype="f16", d=2560, nq=32, n=40000, k=100, data="normal", seed=23), {"wide_rows": 2}),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=40)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("fz", os.path.join(ROOT, "tools", "fuzz_search.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    import veritasfi_amd as vf
    from oracle import canonical
    canonical.build()
    total_bad = 0
    for what, case, opts in CASES:
        codes, rows, q = fz.make_data(case)
        oi, os_ = canonical.search(rows, q, case["k"])
        dev_ids = [0] * case.get("shards", 1) if case.get("shards", 1) > 1 else None
        ix = fz.make_index(vf, case, codes, rows, dev_ids)
        for key, val in opts.items():
            ix.set_option(key, val)
        bad = 0
        for _ in range(a.runs):
            ids, sc = ix.search(q, case["k"])
            if not (np.array_equal(oi, ids) and np.array_equal(os_.view(np.uint32), sc.view(np.uint32))):
                bad += 1
        st = ix.stats()
        ix.close()
        total_bad += bad
        print(json.dumps({"what": what, "runs": a.runs, "failures": bad, "scan_kernel": st.get("scan_kernel"), "scan_image": st.get("scan_image"), "path": st.get("path"),
                          "exact_reruns": st.get("exact_reruns")}), flush=True)
    return 1 if total_bad else 0


if __name__ == "__main__":
    sys.exit(main())
