#!/usr/bin/env python3
"""A/B of an int8 index (VF_DTYPE_INT8) against the fp16 and e4m3 indexes of the same seeded values, and of its two scan routes.

    python tools/bench_int8_rows.py --n 10000000 --d 768 --nq 64 --k 100                    # fp16 (+ image on auto) / e4m3 / int8
    python tools/bench_int8_rows.py --routes --n 32768,131072,1048576,4194304 --nq 1,4,64 --k 100,128

Every measurement runs in a FRESH process (this script calls itself with --child, one `timeout`-bounded child per setting and window),
the settings alternate, --rounds windows each (default three), and the driver stops at the first child that fails.  A child builds the
values on the device from the seed -- N(0, 1) rows; fp16: cast; e4m3: cast (|x| < 448); int8: the quantize_int8 recipe, absmax / 127
per row -- creates ONE index, records the device memory the index holds (what its creation allocated, plus the rows an fp16 / e4m3
index borrows), warms up, then times windows of at least --window seconds of batches pipelined two deep through the slots with
resident inputs, as bench.py does.  It prints one JSON line per (nq, k) cell: ms per batch, the path and kernel that ran, repairs of the last
batch.  The driver prints one line per cell and setting: median, min and max over the windows.
--routes: the int8 index only, conversion route (scan_image = 0: k_scan's int8 form) against the int8-MFMA route (scan_image = 2: k_scan2r
on the index's own bytes); the auto rule's row threshold is read off this grid.
--quality (no GPU): the quality table -- python tools/bench_int8_rows.py --quality --n 50000 --nq 64 --k 100."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_rows(torch, n, d, dtype, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out_dt = {"f16": torch.float16, "fp8": torch.uint8, "int8": torch.int8}[dtype]
    rows = torch.empty((n, d), dtype=out_dt, device=dev)
    for lo in range(0, n, 100_000):
        hi = min(n, lo + 100_000)
        x = torch.randn((hi - lo, d), generator=g, device=dev, dtype=torch.float32)
        if dtype == "f16":
            rows[lo:hi] = x.to(torch.float16)
        elif dtype == "fp8":
            rows[lo:hi] = x.to(torch.float8_e4m3fn).view(torch.uint8)
        else:
            sc = x.abs().amax(dim=1, keepdim=True) / 127.0
            sc = torch.where(sc > 0, sc, torch.ones_like(sc))
            rows[lo:hi] = torch.clamp(torch.round(x / sc), -127, 127).to(torch.int8)
    return rows.view(torch.float8_e4m3fn) if dtype == "fp8" else rows


def quality(args):
    """Host arithmetic only (no GPU): how far the three storage types move the ranking of N(0, 1)-based SYNTHETIC rows (not a real
    embedder's) -- top-k overlap with the fp32 ranking, the largest score error, the mean relative row residual."""
    import numpy as np
    import torch
    import veritasfi_amd as vf
    from oracle import ref_numpy
    rng = np.random.default_rng(args.seed)
    n, d, nq, k = int(args.n), args.d, int(args.nq), int(args.k)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = x[rng.choice(n, nq, replace=False)] + 0.5 * rng.standard_normal((nq, d)).astype(np.float32)   # noisy copies of rows
    peak = np.abs(x).max(axis=1, keepdims=True).astype(np.float64)                                     # the fp8 recipe of FaissRetriever
    xs = np.clip(x * np.exp2(np.floor(np.log2(448.0 / np.where(peak > 0, peak, 448.0)))).astype(np.float32), -448.0, 448.0)
    held = {"f16": (x.astype(np.float16).astype(np.float32), x),
            "e4m3": (ref_numpy.decode_e4m3(torch.from_numpy(xs).to(torch.float8_e4m3fn).view(torch.uint8).numpy()).astype(np.float32), xs),
            "int8": (vf.quantize_int8(x).astype(np.float32), None)}

    def cos(rows):
        r = rows.astype(np.float64)
        r /= np.maximum(np.linalg.norm(r, axis=1, keepdims=True), 1e-300)
        qq = q.astype(np.float64)
        return (qq / np.linalg.norm(qq, axis=1, keepdims=True)) @ r.T

    ref = cos(x)
    top = np.argsort(-ref, axis=1, kind="stable")[:, :k]
    for name, (rows, base) in held.items():
        s = cos(rows)
        got = np.argsort(-s, axis=1, kind="stable")[:, :k]
        overlap = np.mean([len(set(a.tolist()) & set(b.tolist())) / k for a, b in zip(top, got)])
        if name == "int8":
            sc = np.abs(x).max(axis=1, keepdims=True).astype(np.float64) / 127.0
            rho = np.linalg.norm(x - sc * rows, axis=1) / np.linalg.norm(x, axis=1)
        else:
            rho = np.linalg.norm(base.astype(np.float64) - rows, axis=1) / np.linalg.norm(base.astype(np.float64), axis=1)
        print(json.dumps({"quality": name, "n": n, "d": d, "nq": nq, "k": k, "data": "synthetic N(0, 1) rows, noisy-copy queries",
                          "mean_rho": round(float(rho.mean()), 5), "max_score_error": float(f"{np.abs(s - ref).max():.3g}"),
                          "topk_overlap_with_fp32": round(float(overlap), 4)}), flush=True)
    return 0


def child(args):
    import torch
    import veritasfi_amd as vf
    dev = torch.device("cuda:0")
    n, d = int(args.n), args.d
    rows = make_rows(torch, n, d, args.dtype, args.seed, dev)
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    index = vf.DenseIndex(rows)
    free1, _ = torch.cuda.mem_get_info()
    held = free0 - free1                                    # what creation allocated: norms, scan copies, an image ...
    if args.dtype == "int8":
        del rows                                            # (an int8 index copies its rows)
        torch.cuda.empty_cache()
    else:
        held += rows.numel() * rows.element_size()          # ... + the rows an fp16 / e4m3 index borrows from the tensor
    for opt in args.option:
        name, val = opt.split("=")
        index.set_option(name, int(val))
    free2, _ = torch.cuda.mem_get_info()
    held += max(0, free1 - free2) if args.option else 0     # (scan_image = 2 on an int8 index: two floats per row)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed + 1)
    stream = torch.cuda.Stream(device=dev)
    try:
        for k in [int(x) for x in args.k.split(",")]:
            for nq in [int(x) for x in args.nq.split(",")]:
                qpool = [torch.randn((nq, d), generator=g, device=dev, dtype=torch.float32) for _ in range(2)]
                ids = [torch.empty((nq, k), dtype=torch.int64, device=dev) for _ in range(2)]
                sc = [torch.empty((nq, k), dtype=torch.float32, device=dev) for _ in range(2)]

                def run(steps):
                    for i in range(steps + 1):
                        if i < steps:
                            index.search_begin(i & 1, qpool[i & 1], k, ids[i & 1], sc[i & 1])
                        if i >= 1:
                            index.search_end((i - 1) & 1)

                with torch.cuda.stream(stream):
                    run(4)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    run(4)
                    torch.cuda.synchronize()
                    per = (time.perf_counter() - t0) / 4
                    steps = max(4, int(args.window / max(per, 1e-6)) + 1)
                    t0 = time.perf_counter()
                    run(steps)
                    torch.cuda.synchronize()
                    el = time.perf_counter() - t0
                st = index.stats()
                print(json.dumps({"setting": args.setting, "dtype": args.dtype, "n": n, "d": d, "nq": nq, "k": k, "ms_per_batch": round(1e3 * el / steps, 4),
                                  "q_per_s": round(nq * steps / el, 1), "path": st["path"], "scan_kernel": st["scan_kernel"], "scan_image": st["scan_image"],
                                  "exact_reruns_last_batch": st["exact_reruns"], "candidates_per_query_last_batch": round(st["candidates"] / max(nq, 1), 1), "index_bytes": int(held), "index_bytes_per_row": round(held / max(n, 1), 2)}),
                      flush=True)
    finally:
        index.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="10000000", help="rows; a comma list runs every value (a process per value, setting and window)")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", default="64", help="queries per batch; a comma list runs every value on the same index")
    ap.add_argument("--k", default="100", help="results per query; a comma list runs every value")
    ap.add_argument("--routes", action="store_true", help="the int8 index only: conversion route against the int8-MFMA route")
    ap.add_argument("--quality", action="store_true", help="host arithmetic only: top-k overlap with the fp32 ranking for fp16 / e4m3 / int8 (single --n / --nq / --k)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window, at least")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dtype", default="int8", help=argparse.SUPPRESS)
    ap.add_argument("--setting", default="", help=argparse.SUPPRESS)
    ap.add_argument("--option", action="append", default=[], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.quality:
        return quality(args)
    if args.routes:
        settings = [("int8_convert", "int8", ["scan_image=0"]), ("int8_mfma", "int8", ["scan_image=2"])]
    else:
        settings = [("f16_image_auto", "f16", []), ("e4m3", "fp8", []), ("int8", "int8", [])]
    cells = {}
    for n in [int(x) for x in args.n.split(",")]:
        for rnd in range(args.rounds):
            for name, dtype, opts in settings:
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--n", str(n), "--d", str(args.d),
                       "--nq", args.nq, "--k", args.k, "--window", str(args.window), "--seed", str(args.seed), "--dtype", dtype, "--setting", name]
                for o in opts:
                    cmd += ["--option", o]
                proc = subprocess.run(cmd, capture_output=True, text=True)
                if proc.returncode != 0:
                    print(f"# {name} n={n} window {rnd}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}", flush=True)
                    return 1
                for line in proc.stdout.splitlines():
                    if line.startswith("{"):
                        rec = json.loads(line)
                        print(line, flush=True)
                        cells.setdefault((n, rec["nq"], rec["k"], name), []).append(rec)
    for (n, nq, k, name), recs in cells.items():
        t = [r["ms_per_batch"] for r in recs]
        print(f"# n={n:9d} nq={nq:3d} k={k:4d} {name:15s} {statistics.median(t):9.4f} ms/batch (min {min(t):.4f} max {max(t):.4f}) "
              f"{nq / statistics.median(t) * 1e3:10.0f} q/s path {recs[-1]['path']} kernel {recs[-1]['scan_kernel']} image {recs[-1]['scan_image']} candidates/query {recs[-1]['candidates_per_query_last_batch']} "
              f"index {recs[-1]['index_bytes'] / 2**30:.2f} GiB ({recs[-1]['index_bytes_per_row']} B/row)", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
