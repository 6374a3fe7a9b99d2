#!/usr/bin/env python3
"""A/B of the search paths for rows of 2560 to 4096 padded elements, on ONE index in ONE process.

    python tools/bench_wide_rows.py --n 1000000 --d 2560 --nq 4 --k 100 [--dtype f16|f32|fp8|int8] [--scan-wide] [--f16-control] [--e4m3-control] [--verify 2]

Settings: `path2` (option wide_rows = 0: the chunked exact path, what these rows took before k_scan_ksplit existed), `ksplit`
(wide_rows = 2, wide = 0: the fused path on k_scan_ksplit, 32-query passes at every batch size) and, with --scan-wide, `scan_wide` (wide_rows = 2 and
wide = 2: the batch goes to k_scan_wide's 256-query tiles; only for nq >= 2).  Every setting is warmed up; then timed windows
of at least --window seconds each, the settings ALTERNATING, --rounds rounds; the spread over the rounds is printed.  Batches are
pipelined two deep through the slots (vf_index_search_begin / _end) with resident inputs, as bench.py does; on the fused path
HIP events around the main scan launches give the launch time (vf_index_profile) and the launch interval (vf_index_profile_span).
One JSON line: ms per batch per setting (median, min, max over the rounds), the byte rate n (2 dp + 4) / launch interval of the
ksplit setting as a fraction of 8 TB/s, and `verified`: ids and score bits of --verify queries against the CPU oracle.
--dtype fp8: the rows are e4m3 codes cast from N(0, 1) (k_scan_ksplit8; the wide pass is k_scan_wide8, or k_scan_wide with --wide-mfma 0);
a pass then reads n (dp + 4) bytes.  --f16-control adds `ksplit_f16`: a second index in the same process holding the same decoded values
as fp16 rows, on k_scan_ksplit, timed in the same alternation; its results must equal the e4m3 index's bit for bit.
--dtype int8: the rows are quantize_int8 of N(0, 1), built on the device in chunks (k_scan_ksplit8i; the wide pass is k_scan_wide's int8
form); a pass reads n (dp + 4) bytes as for e4m3 rows.  --e4m3-control adds `ksplit_e4m3`: a second index in the same process of the same
shape holding e4m3 codes cast from N(0, 1), on k_scan_ksplit8, timed in the same alternation (other values: its results are not compared)."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=2560)
    ap.add_argument("--nq", default="4", help="queries per batch; a comma list runs every value on the same index")
    ap.add_argument("--k", default="100", help="results per query; a comma list runs every value")
    ap.add_argument("--dtype", choices=["f16", "f32", "fp8", "int8"], default="f16")
    ap.add_argument("--f16-control", action="store_true", help="with --dtype fp8: also time an fp16 index of the same decoded values on k_scan_ksplit")
    ap.add_argument("--e4m3-control", action="store_true", help="with --dtype int8: also time an e4m3 index of the same shape on k_scan_ksplit8")
    ap.add_argument("--only", default="", help="time this one setting only (path2, ksplit, scan_wide or the control): a fresh process per setting and window; "
                    "`result_crc` in the JSON line lets the settings' results be compared across processes (same --seed: same rows and queries)")
    ap.add_argument("--wide-mfma", type=int, default=-1, help="with --dtype fp8: option wide_mfma for the scan_wide setting (1 k_scan_wide8, 0 k_scan_wide)")
    ap.add_argument("--scan-wide", action="store_true", help="also time k_scan_wide forced onto these rows (nq >= 2)")
    ap.add_argument("--scan-wide-from", type=int, default=2, help="with --scan-wide: only for batches of at least this many queries")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window, at least")
    ap.add_argument("--verify", type=int, default=2, help="queries checked against the CPU oracle (0 = none)")
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()

    import torch
    import veritasfi_amd as vf
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed)
    tdt = {"f16": torch.float16, "f32": torch.float32, "fp8": torch.float8_e4m3fn, "int8": torch.int8}[args.dtype]
    fp8, i8 = args.dtype == "fp8", args.dtype == "int8"
    corpus = torch.empty((args.n, args.d), dtype=torch.uint8 if fp8 else tdt, device=dev)   # (e4m3: filled as bytes, viewed as e4m3 below)
    for lo in range(0, args.n, 100_000):
        hi = min(args.n, lo + 100_000)
        block = torch.randn((hi - lo, args.d), generator=g, device=dev, dtype=torch.float32)
        if i8:   # vf.quantize_int8's recipe in fp32: one scale per row, absmax / 127, round to nearest even, not kept
            mx = block.abs().amax(dim=1, keepdim=True)
            sc = torch.where(mx > 0, mx / 127.0, torch.ones_like(mx))
            corpus[lo:hi] = torch.clamp(torch.round(block / sc), -127.0, 127.0).to(torch.int8)
            continue
        block = block.to(tdt)
        corpus[lo:hi] = block.view(torch.uint8) if fp8 else block
    if fp8:
        corpus = corpus.view(tdt)
    dp = (args.d + 127) // 128 * 128
    host = None

    index = vf.DenseIndex(corpus)
    control = None
    if args.dtype == "fp8" and args.f16_control:   # the same values as fp16 rows (every e4m3 value is an fp16 value)
        corpus16 = torch.empty((args.n, args.d), dtype=torch.float16, device=dev)
        for lo in range(0, args.n, 100_000):
            corpus16[lo:lo + 100_000] = corpus[lo:lo + 100_000].to(torch.float16)
        control = vf.DenseIndex(corpus16)
    if i8 and args.e4m3_control and args.only in ("", "ksplit_e4m3"):   # an e4m3 index of the same shape (its own N(0, 1) draw: the byte-row kernel it is measured against)
        g8 = torch.Generator(device=dev)   # (a generator of its own: the queries below do not depend on whether this index is built)
        g8.manual_seed(args.seed + 1)
        corpus8 = torch.empty((args.n, args.d), dtype=torch.uint8, device=dev)
        for lo in range(0, args.n, 100_000):
            hi = min(args.n, lo + 100_000)
            corpus8[lo:hi] = torch.randn((hi - lo, args.d), generator=g8, device=dev, dtype=torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)
        control = vf.DenseIndex(corpus8.view(torch.float8_e4m3fn))
    if args.dtype == "fp8" and args.wide_mfma >= 0:
        index.set_option("wide_mfma", args.wide_mfma)
    ok_all = True
    try:
        for k in [int(x) for x in args.k.split(",")]:
            for nq in [int(x) for x in args.nq.split(",")]:
                out, host = cell(args, torch, vf, index, corpus, g, dev, dp, nq, k, host, control, "ksplit_e4m3" if i8 else "ksplit_f16")
                print(json.dumps(out), flush=True)
                ok_all = ok_all and out.get("verified", out["settings_agree_bitwise"])
    finally:
        index.close()
        if control is not None:
            control.close()
    return 0 if ok_all else 1


def cell(args, torch, vf, index, corpus, g, dev, dp, nq, k, host, control=None, control_name="ksplit_f16"):
    qpool = [torch.randn((nq, args.d), generator=g, device=dev, dtype=torch.float32) for _ in range(2)]
    ids = [torch.empty((nq, k), dtype=torch.int64, device=dev) for _ in range(2)]
    sc = [torch.empty((nq, k), dtype=torch.float32, device=dev) for _ in range(2)]
    settings = [("path2", {"wide_rows": 0, "wide": 1}), ("ksplit", {"wide_rows": 2, "wide": 0})]
    if args.scan_wide and nq >= max(2, args.scan_wide_from):
        settings.append(("scan_wide", {"wide_rows": 2, "wide": 2}))
    if control is not None:
        settings.append((control_name, {"wide_rows": 2, "wide": 0}))
    if args.only:
        settings = [(n_, o_) for n_, o_ in settings if n_ == args.only]
        if not settings:   # (scan_wide below its first batch size, a control that was not asked for)
            return {"n": args.n, "d": args.d, "nq": nq, "k": k, "dtype": args.dtype, "only": args.only, "settings": {}, "settings_agree_bitwise": True}, host
    row_bytes = dp if args.dtype in ("fp8", "int8") else 2 * dp
    out = {"n": args.n, "d": args.d, "dp": dp, "nq": nq, "k": k, "dtype": args.dtype, "rounds": args.rounds, "window_s": args.window, "settings": {}}
    try:
        stream = torch.cuda.Stream(device=dev)

        cur = [index]

        def apply(opts, name=""):
            cur[0] = control if name == control_name else index
            for opt, val in opts.items():
                cur[0].set_option(opt, val)

        def run(steps):
            for i in range(steps + 1):
                if i < steps:
                    cur[0].search_begin(i & 1, qpool[i & 1], k, ids[i & 1], sc[i & 1])
                if i >= 1:
                    cur[0].search_end((i - 1) & 1)

        per_step, stats, results = {}, {}, {}
        with torch.cuda.stream(stream):
            for name, opts in settings:          # warm-up of every setting; the step count of a window from a first timing
                apply(opts, name)
                run(2)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(4)
                torch.cuda.synchronize()
                per_step[name] = (time.perf_counter() - t0) / 4
                stats[name] = cur[0].stats()
                results[name] = (ids[1].cpu().numpy().copy(), sc[1].cpu().numpy().copy())   # (4 steps: the last batch is qpool[1])
            times = {name: [] for name, _ in settings}
            launch = {name: [] for name, _ in settings}
            interval = {name: [] for name, _ in settings}
            for _ in range(args.rounds):
                for name, opts in settings:
                    apply(opts, name)
                    steps = max(4, int(args.window / max(per_step[name], 1e-6)) + 1)
                    run(2)
                    torch.cuda.synchronize()
                    cur[0].set_option("profile", 1)
                    t0 = time.perf_counter()
                    run(steps)
                    torch.cuda.synchronize()
                    el = time.perf_counter() - t0
                    prof = cur[0].profile()
                    cur[0].set_option("profile", 0)
                    times[name].append(1e3 * el / steps)
                    if prof["scan_launches"] > 0:
                        launch[name].append(prof["scan_ms_total"] / prof["scan_launches"])
                        if prof["span_ms"] > 0:
                            interval[name].append(prof["span_ms"] / prof["scan_launches"])
        for name, _ in settings:
            t = times[name]
            rec = {"ms_per_batch": round(statistics.median(t), 4), "min": round(min(t), 4), "max": round(max(t), 4),
                   "spread": round((max(t) - min(t)) / statistics.median(t), 4), "path": stats[name]["path"], "scan_kernel": stats[name]["scan_kernel"],
                   "exact_reruns_last_batch": stats[name]["exact_reruns"], "overflowed_last_batch": stats[name]["overflowed"]}
            rec["result_crc"] = zlib.crc32(results[name][1].tobytes(), zlib.crc32(results[name][0].tobytes()))
            if launch[name]:
                rec["scan_launch_ms"] = round(statistics.median(launch[name]), 4)
            if interval[name]:
                iv = statistics.median(interval[name])
                rec["launch_interval_ms"] = round(iv, 4)
                # one pass reads the shard once, rows + reciprocal norms (k_scan_ksplit: a pass per 32 queries; the events bracket a
                # batch's first pass, the interval is per batch)
                # (k_scan_ksplit8 / k_scan_ksplit8i the same on rows of dp bytes; the fp16 control reads 2 dp, the e4m3 control dp)
                passes = (nq + 31) // 32 if stats[name]["scan_kernel"] in (6, 7) else 1
                rb = 2 * dp if name == "ksplit_f16" else row_bytes
                rec["passes_per_batch"] = passes
                rec["bytes_per_pass"] = args.n * (rb + 4)
                rec["byte_rate_TBps"] = round(passes * args.n * (rb + 4) / (iv * 1e-3) / 1e12, 3)
                rec["frac_of_8TBps"] = round(passes * args.n * (rb + 4) / (iv * 1e-3) / 8e12, 4)
            out["settings"][name] = rec
            print(f"# {name:11s} {rec['ms_per_batch']:9.4f} ms/batch (min {rec['min']:.4f} max {rec['max']:.4f}) path {rec['path']} kernel {rec['scan_kernel']}"
                  + (f" launch {rec.get('scan_launch_ms')} ms interval {rec.get('launch_interval_ms')} ms {rec.get('frac_of_8TBps')} of 8 TB/s" if launch[name] else ""),
                  file=sys.stderr, flush=True)
        base = results[settings[0][0]]
        compared = [n_ for n_, _ in settings if n_ != "ksplit_e4m3"]   # (the e4m3 control holds other values)
        same = all(np.array_equal(results[n_][0], base[0]) and np.array_equal(results[n_][1].view(np.uint32), base[1].view(np.uint32)) for n_ in compared)
        out["settings_agree_bitwise"] = bool(same)
        if control is not None and control_name == "ksplit_f16" and not args.only:
            out["fp8_over_f16_time"] = round(out["settings"]["ksplit"]["ms_per_batch"] / out["settings"]["ksplit_f16"]["ms_per_batch"], 4)
        if control is not None and control_name == "ksplit_e4m3" and not args.only:
            out["int8_over_e4m3_time"] = round(out["settings"]["ksplit"]["ms_per_batch"] / out["settings"]["ksplit_e4m3"]["ms_per_batch"], 4)
        if args.verify > 0:
            from oracle import canonical as oracle
            oracle.build()
            nv = min(args.verify, nq)
            if host is None:
                host = (corpus.to(torch.float16) if args.dtype in ("fp8", "int8") else corpus).cpu().numpy()   # (both exact in fp16)
            wi, ws = oracle.search(host, qpool[1][:nv].cpu().numpy(), k)
            out["verified"] = bool(same and all(np.array_equal(results[n_][0][:nv], wi) and np.array_equal(results[n_][1][:nv].view(np.uint32), ws.view(np.uint32))
                                                for n_ in compared))
            out["verified_queries"] = nv
    finally:
        for ix_ in (index, control):
            for name, val in (("wide_rows", 1), ("wide", 1), ("profile", 0)):
                if ix_ is not None:
                    ix_.set_option(name, val)
    return out, host


if __name__ == "__main__":
    sys.exit(main())
