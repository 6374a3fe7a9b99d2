#!/usr/bin/env python3
"""What searching a chosen subset of rows costs (DenseIndex.search(subset=RowSubset): vf_index_search_device with VF_SEARCH_SUBSET, k_scan_subset),
beside three yardsticks taken in the same process.

    python tools/bench_subset_search.py                     # every setting, written to profiles/r16_subset_search.log as well
    python tools/bench_subset_search.py --m 10000 --nq 1,4  # a part of it

One index of --n fp16 rows of --d elements (N(0, 1) from a seed, generated on the device).  A SETTING is a subset size and a layout
-- `contiguous`: one run of m rows in the middle; `scattered`: m rows drawn uniformly -- and runs in a FRESH process (this script calls
itself with --child, one `timeout`-bounded child per setting), the settings alternate over --rounds passes, and the driver stops at the
first child that fails.  In a child, for every nq of --nq and k of --k, --calls calls each (after 3 warm-up calls), p50 of a host clock
around the call (every call returns after a device synchronise; queries, the id list and the outputs are resident on the device):

  subset     the subset search itself
  rebuild    the parent commit's only exact route: index_select of the listed rows into a second matrix, vf_index_create_device over it,
             one search, ids mapped back through the list; + the HBM the second matrix takes
  whole      an unfiltered search of the whole index (what a host-side filter would start from; not exact for the subset)
  floor      the listed rows' bytes (m x d x 2) divided by --hbm-tbs TB/s: what reading them once costs at the HBM peak

Every subset result is compared with the rebuild route's (ids and score bits) before anything is timed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_rows(torch, n, d, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    rows = torch.empty((n, d), dtype=torch.float16, device=dev)
    for lo in range(0, n, 100_000):
        hi = min(n, lo + 100_000)
        rows[lo:hi] = torch.randn((hi - lo, d), generator=g, device=dev, dtype=torch.float32).to(torch.float16)
    return rows


def p50(fn, calls, torch):
    for _ in range(3):
        fn()
    t = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(t), 4), round(min(t), 4)


def child(args):
    import numpy as np
    import torch
    import veritasfi_amd as vf
    from veritasfi_amd import _ffi
    dev = torch.device("cuda:0")
    n, d, m = args.n, args.d, args.m_one
    rows = make_rows(torch, n, d, args.seed, dev)
    index = vf.DenseIndex(rows)
    if args.super_rows:
        index.set_option("subset_super_rows", args.super_rows)
    rng = np.random.default_rng(args.seed + m)
    sel = np.arange(n // 2 - m // 2, n // 2 - m // 2 + m) if args.layout == "contiguous" else np.sort(rng.choice(n, m, replace=False))
    rs = index.row_subset(sel)
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed + 1)
    L = _ffi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for nq in args.nqs:
        q = torch.randn((nq, d), generator=g, device=dev, dtype=torch.float32)
        for k in args.ks:
            ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
            sc = torch.empty((nq, k), dtype=torch.float32, device=dev)

            def subset():
                _ffi.check(_ffi.search_subset_device(L, index._h, q.data_ptr(), nq, k, rs.tensor.data_ptr(), len(rs), ids.data_ptr(), sc.data_ptr(), stream),
                           "vf_index_search_device (subset)")

            def rebuild():
                second = rows.index_select(0, rs.tensor)
                other = vf.DenseIndex(second)
                i2, s2 = other.search_device(q, k)
                mapped = torch.where(i2 >= 0, rs.tensor[i2.clamp(min=0)], i2)
                other.close()
                return mapped, s2

            def whole():
                index.search_device(q, k)

            subset()
            st = index.stats()
            want_ids, want_sc = rebuild()
            assert torch.equal(ids, want_ids) and torch.equal(sc.view(torch.int32), want_sc.view(torch.int32)), "the subset search differs from the rebuild route"
            t_sub, min_sub = p50(subset, args.calls, torch)
            t_reb, _ = p50(rebuild, max(5, args.calls // 3), torch)
            t_whole, _ = p50(whole, args.calls, torch)
            floor_ms = m * d * 2 / (args.hbm_tbs * 1e12) * 1e3
            print(json.dumps({"m": m, "layout": args.layout, "n": n, "d": d, "nq": nq, "k": k, "path": st["path"], "subset_p50_ms": t_sub, "subset_min_ms": min_sub,
                              "rebuild_p50_ms": t_reb, "rebuild_extra_MB": round(m * d * 2 / 1e6, 1), "whole_p50_ms": t_whole, "floor_ms": round(floor_ms, 5),
                              "hbm_fraction": round(floor_ms / t_sub, 4), "subset_GBps": round(m * d * 2 / 1e9 / (t_sub / 1e3), 1)}), flush=True)
    index.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--m", default="1000,10000,100000,500000", help="subset sizes (comma list)")
    ap.add_argument("--nq", default="1,4,64")
    ap.add_argument("--k", default="100,2048")
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--super-rows", type=int, default=0, help="option subset_super_rows (0 = auto: 64 MB of scores per launch)")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="the HBM peak the floor is computed from, TB/s")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_subset_search.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--layout", default="", help=argparse.SUPPRESS)
    ap.add_argument("--m-one", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.nqs = [int(x) for x in args.nq.split(",")]
    args.ks = [int(x) for x in args.k.split(",")]
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def run(m, layout):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--m-one", str(m), "--layout", layout,
               "--n", str(args.n), "--d", str(args.d), "--nq", args.nq, "--k", args.k, "--calls", str(args.calls), "--seed", str(args.seed),
               "--super-rows", str(args.super_rows), "--hbm-tbs", str(args.hbm_tbs)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            say(f"# m={m} {layout}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}")
            return None
        recs = []
        for line in proc.stdout.splitlines():
            if line.startswith("{"):
                say(line)
                recs.append(json.loads(line))
        return recs

    say("# " + " ".join(sys.argv))
    ms = [int(x) for x in args.m.split(",")]
    settings = [(m, layout) for m in ms for layout in ("contiguous", "scattered")]
    got = {}
    for rnd in range(args.rounds):
        for m, layout in (settings if rnd % 2 == 0 else settings[::-1]):    # the settings alternate: no setting always follows the same one
            recs = run(m, layout)
            if recs is None:
                return 1
            for r in recs:
                got.setdefault((m, layout, r["nq"], r["k"]), []).append(r)
    say("# medians over the rounds: subset | rebuild (extra HBM) | whole index | floor at the HBM peak = fraction of the peak the subset search reaches")
    for (m, layout, nq, k), v in sorted(got.items()):
        med = {key: statistics.median(r[key] for r in v) for key in ("subset_p50_ms", "rebuild_p50_ms", "whole_p50_ms")}
        say(f"# m={m:7d} {layout:10s} nq={nq:3d} k={k:5d}  subset {med['subset_p50_ms']:9.4f} ms | rebuild {med['rebuild_p50_ms']:9.4f} ms (+{v[0]['rebuild_extra_MB']} MB) "
            f"= {med['rebuild_p50_ms'] / med['subset_p50_ms']:6.2f} x | whole {med['whole_p50_ms']:9.4f} ms = {med['whole_p50_ms'] / med['subset_p50_ms']:6.2f} x | "
            f"floor {v[0]['floor_ms']:8.5f} ms = {v[0]['floor_ms'] / med['subset_p50_ms']:6.4f} of peak")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
