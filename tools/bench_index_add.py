#!/usr/bin/env python3
"""What an append to a live index costs (DenseIndex.add: vf_index_create* with VF_INDEX_APPEND), against the only other route to the same
state -- building a second index over all the rows -- and whether a handle grown by appends searches like one built at once.

    python tools/bench_index_add.py                      # every measurement, written to profiles/r13_index_add.log as well
    python tools/bench_index_add.py --only append        # append / rebuild costs only;  --only search: the search comparison only

Every measurement runs in a FRESH process (this script calls itself with --child, one `timeout`-bounded child per setting and window),
the settings of a comparison alternate, and the driver stops at the first child that fails.  fp16 rows of --d elements, N(0, 1) from a
seed, generated on the device.  A call's time is a host clock around it: add() and the index constructor return after a device
synchronise.

  append     --calls appends of --m rows into an index of n rows with room reserved (option reserve_rows), rows resident on the
             device and rows in host memory: p50 / p90 / max per call, at every --n.  Cost should follow the rows added, not n.
  rebuild    the same state by vf_index_create_device over all n + m rows (resident, borrowed: the cheapest form), p50 of --rebuilds.
  growing    the appends again at the largest n WITHOUT a reservation: the calls that grow the arrays by half are the expensive ones.
  search     --search-n rows, 64 queries, k = 100, batches pipelined two deep: a handle grown from --search-n0 rows in appends of
             --search-m against a handle built at once; --rounds windows each, the two alternating."""
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


def pct(t, p):
    s = sorted(t)
    return s[min(len(s) - 1, int(p * len(s)))]


def child_append(args, torch, vf, dev):
    n, d, m, calls = args.n, args.d, args.m, args.calls
    rows = make_rows(torch, n + (calls + 8) * m, d, args.seed, dev)
    host = rows[n:].cpu().numpy() if args.setting.endswith("host") else None
    index = vf.DenseIndex(rows[:n])
    if not args.setting.startswith("growing"):
        index.reserve(n + (calls + 8) * m)
    torch.cuda.synchronize()
    t = []
    for i in range(calls + 8):
        blk = host[i * m:(i + 1) * m] if host is not None else rows[n + i * m:n + (i + 1) * m]
        t0 = time.perf_counter()
        index.add(blk)
        t.append(1e3 * (time.perf_counter() - t0))
    t = t[8:] if not args.setting.startswith("growing") else t      # (a reserved index: the first calls warm the kernel and the staging up)
    ids, _ = index.search_device(rows[index.n - 1:index.n].float(), 1)
    assert int(ids[0, 0]) == index.n - 1 and index.n == n + (calls + 8) * m, "the last appended row is not its own best match"
    rec = {"setting": args.setting, "n": n, "d": d, "m": m, "calls": len(t), "p50_ms": round(statistics.median(t), 4), "p90_ms": round(pct(t, 0.9), 4),
           "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}
    if args.setting.startswith("growing"):
        rec["calls_over_10x_p50"] = [(i, round(x, 3)) for i, x in enumerate(t) if x > 10 * statistics.median(t)]
    print(json.dumps(rec), flush=True)
    index.close()


def child_rebuild(args, torch, vf, dev):
    n, d, m = args.n, args.d, args.m
    rows = make_rows(torch, n + m, d, args.seed, dev)
    t = []
    for i in range(args.rebuilds + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index = vf.DenseIndex(rows)
        t.append(1e3 * (time.perf_counter() - t0))
        index.close()
    t = t[2:]
    print(json.dumps({"setting": args.setting, "n": n, "d": d, "m": m, "calls": len(t), "p50_ms": round(statistics.median(t), 4), "p90_ms": round(pct(t, 0.9), 4),
                      "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}), flush=True)


def child_search(args, torch, vf, dev):
    n, d, nq, k = args.n, args.d, 64, 100
    rows = make_rows(torch, n, d, args.seed, dev)
    if args.setting == "search_grown":
        index = vf.DenseIndex(rows[:args.search_n0].clone())
        for lo in range(args.search_n0, n, args.search_m):
            index.add(rows[lo:min(n, lo + args.search_m)])
        del rows
        torch.cuda.empty_cache()
    else:
        index = vf.DenseIndex(rows)
    assert index.n == n
    g = torch.Generator(device=dev)
    g.manual_seed(args.seed + 1)
    qpool = [torch.randn((nq, d), generator=g, device=dev, dtype=torch.float32) for _ in range(2)]
    ids = [torch.empty((nq, k), dtype=torch.int64, device=dev) for _ in range(2)]
    sc = [torch.empty((nq, k), dtype=torch.float32, device=dev) for _ in range(2)]

    def run(steps):
        for i in range(steps + 1):
            if i < steps:
                index.search_begin(i & 1, qpool[i & 1], k, ids[i & 1], sc[i & 1])
            if i >= 1:
                index.search_end((i - 1) & 1)

    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        run(8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run(8)
        torch.cuda.synchronize()
        steps = max(8, int(args.window / max((time.perf_counter() - t0) / 8, 1e-6)) + 1)
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
    st = index.stats()
    print(json.dumps({"setting": args.setting, "n": n, "d": d, "nq": nq, "k": k, "ms_per_batch": round(1e3 * el / steps, 4), "steps": steps, "path": st["path"],
                      "scan_kernel": st["scan_kernel"], "scan_image": st["scan_image"], "exact_reruns_last_batch": st["exact_reruns"],
                      "checksum_ids": int(ids[0].sum().item())}), flush=True)
    index.close()


def child(args):
    import torch
    import veritasfi_amd as vf
    dev = torch.device("cuda:0")
    if args.setting.startswith("search"):
        child_search(args, torch, vf, dev)
    elif args.setting == "rebuild":
        child_rebuild(args, torch, vf, dev)
    else:
        child_append(args, torch, vf, dev)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100000,1000000", help="rows in the index before the appends (comma list)")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--m", type=int, default=100, help="rows per append")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rebuilds", type=int, default=20)
    ap.add_argument("--search-n", type=int, default=1_000_000)
    ap.add_argument("--search-n0", type=int, default=100_000)
    ap.add_argument("--search-m", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed search window, at least")
    ap.add_argument("--timeout", type=int, default=180, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--only", choices=["append", "search"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_index_add.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--setting", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        args.n = int(args.n)
        return child(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def run(setting, n):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--setting", setting, "--n", str(n),
               "--d", str(args.d), "--m", str(args.m), "--calls", str(args.calls), "--rebuilds", str(args.rebuilds), "--seed", str(args.seed),
               "--window", str(args.window), "--search-n0", str(args.search_n0), "--search-m", str(args.search_m)]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        if proc.returncode != 0:
            say(f"# {setting} n={n}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}")
            return None
        rec = None
        for line in proc.stdout.splitlines():
            if line.startswith("{"):
                say(line)
                rec = json.loads(line)
        return rec

    say("# " + " ".join(sys.argv))
    ns = [int(x) for x in args.n.split(",")]
    if args.only in (None, "append"):
        p50 = {}
        for rnd in range(2):                                         # two passes over the settings, alternating
            for n in ns:
                for setting in ("append_reserved_device", "rebuild", "append_reserved_host"):
                    rec = run(setting, n)
                    if rec is None:
                        return 1
                    p50.setdefault((setting, n), []).append(rec["p50_ms"])
        rec = run("growing_device", ns[-1])
        if rec is None:
            return 1
        for (setting, n), v in sorted(p50.items()):
            say(f"# {setting:24s} n={n:9d}  p50 per call {min(v):9.4f} .. {max(v):9.4f} ms over {len(v)} processes")
        for setting in ("append_reserved_device", "append_reserved_host"):
            a, b = statistics.median(p50[(setting, ns[0])]), statistics.median(p50[(setting, ns[-1])])
            say(f"# {setting}: p50 at n={ns[-1]} / p50 at n={ns[0]} = {b / a:.3f}")
        for n in ns:
            say(f"# n={n}: rebuild p50 / append p50 (device rows) = {statistics.median(p50[('rebuild', n)]) / statistics.median(p50[('append_reserved_device', n)]):.1f}")
    if args.only in (None, "search"):
        t = {"search_grown": [], "search_built": []}
        for rnd in range(args.rounds):
            for setting in (("search_grown", "search_built") if rnd % 2 == 0 else ("search_built", "search_grown")):
                rec = run(setting, args.search_n)
                if rec is None:
                    return 1
                t[setting].append(rec)
        for setting, recs in t.items():
            v = [r["ms_per_batch"] for r in recs]
            say(f"# {setting:13s} n={args.search_n} nq=64 k=100: median {statistics.median(v):.4f} ms/batch (min {min(v):.4f} max {max(v):.4f}), kernel "
                f"{recs[-1]['scan_kernel']} image {recs[-1]['scan_image']}, ids checksum {recs[-1]['checksum_ids']}")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
