#!/usr/bin/env python3
"""What removing rows from a live index costs (DenseIndex.remove: vf_index_create with VF_INDEX_REMOVE, k_compact_rows), against two
yardsticks taken in the same process, and whether a handle shrunk by a removal searches like one built at its size.

    python tools/bench_index_remove.py                     # every measurement, written to profiles/r14_index_remove.log as well
    python tools/bench_index_remove.py --only remove       # removal costs only;  --only search: the search comparison only

Every measurement runs in a FRESH process (this script calls itself with --child, one `timeout`-bounded child per setting and window),
the settings alternate, and the driver stops at the first child that fails.  fp16 rows of --d elements, N(0, 1) from a seed, generated
on the device.  A call's time is a host clock around it: remove(), add() and the index constructor return after a device synchronise.

  remove     --calls removals from an index of n rows, the removed rows put back by add() between calls (so n stays), p50 / p90 / max:
               tail      --m rows drawn from the last 1000 (an amended filing that was ingested last: almost nothing moves)
               scatter   --m rows drawn uniformly (everything behind the lowest of them moves)
               filing    one contiguous run of --filing rows in the middle (half the index moves)
  rebuild    the parent commit's only route to the same state: index_select of the surviving rows on the device into a second matrix
             and vf_index_create_device over it; its time and the extra HBM the second matrix takes while both exist.
  memcpy     a plain device-to-device copy of the bytes the removal moves (rows, norms and inverses behind the first removed row),
             to a scratch buffer and back: the floor of a staged mover.
  search     --search-n rows, 64 queries, k = 100, batches pipelined two deep: a handle shrunk from --search-n0 rows by one removal of
             scattered rows against a handle built over the same remaining rows; --rounds windows each, the two alternating."""
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


def summary(t):
    return {"calls": len(t), "p50_ms": round(statistics.median(t), 4), "p90_ms": round(pct(t, 0.9), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}


def draw(np, rng, pattern, n, m, filing):
    if pattern == "tail":
        return np.sort(rng.choice(np.arange(n - 1000, n), m, replace=False))
    if pattern == "scatter":
        return np.sort(rng.choice(n, m, replace=False))
    return np.arange(n // 2, n // 2 + filing)


def child_remove(args, torch, vf, dev):
    import numpy as np
    n, d, pattern = args.n, args.d, args.setting.split("_", 1)[1]
    rng = np.random.default_rng(args.seed)
    rows = make_rows(torch, n, d, args.seed, dev)
    cur = rows.clone()                                              # what the index holds, in its order (rows: the first build's input)
    index = vf.DenseIndex(rows)
    index.reserve(n + 1)                                            # its own copy now, so that no call pays for it
    row_bytes = d * 2 + 8                                           # the row, its norm and its inverse
    t_rm, t_add, t_rb, t_cp, moved = [], [], [], [], []
    for i in range(args.calls + 4):
        gone = draw(np, rng, pattern, n, args.m, args.filing)
        gone_t = torch.from_numpy(gone).to(dev)
        back = cur.index_select(0, gone_t)
        keep = torch.ones(n, dtype=torch.bool, device=dev)
        keep[gone_t] = False
        keep_idx = keep.nonzero().squeeze(1)
        torch.cuda.synchronize()
        # yardstick 1: a second matrix of the surviving rows and a second index over it
        t0 = time.perf_counter()
        second = cur.index_select(0, keep_idx)
        other = vf.DenseIndex(second)
        torch.cuda.synchronize()
        t_rb.append(1e3 * (time.perf_counter() - t0))
        other.close()
        # yardstick 2: the bytes the removal moves, copied away and back
        nbytes = (n - len(gone) - int(gone[0])) * row_bytes
        moved.append(nbytes)
        flat = cur.view(torch.uint8).view(-1)
        if nbytes > 0:
            scratch = torch.empty(min(nbytes, flat.numel()), dtype=torch.uint8, device=dev)
            src = flat[flat.numel() - scratch.numel():]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scratch.copy_(src)
            src.copy_(scratch)
            torch.cuda.synchronize()
            t_cp.append(1e3 * (time.perf_counter() - t0))
            del scratch
        else:
            t_cp.append(0.0)
        # the removal, then the rows put back
        t0 = time.perf_counter()
        got = index.remove(gone)
        t_rm.append(1e3 * (time.perf_counter() - t0))
        assert got == len(gone) and index.n == n - len(gone)
        t0 = time.perf_counter()
        index.add(back)
        t_add.append(1e3 * (time.perf_counter() - t0))
        cur = torch.cat([second, back])
        del second, back, keep, keep_idx
    probe = torch.tensor([0, n // 3, n - 1], device=dev)
    ids, _ = index.search_device(cur.index_select(0, probe).float(), 1)
    assert ids[:, 0].tolist() == probe.tolist(), "a row is not its own best match under its id after the removals"
    rec = {"setting": args.setting, "n": n, "d": d, "removed_per_call": int(len(gone)), "moved_MB_p50": round(statistics.median(moved[4:]) / 1e6, 2),
           "remove": summary(t_rm[4:]), "add_back": summary(t_add[4:]), "rebuild": summary(t_rb[4:]), "memcpy_twice": summary(t_cp[4:]),
           "rebuild_extra_MB": round((n - len(gone)) * d * 2 / 1e6, 1)}
    rec["rebuild_over_remove"] = round(rec["rebuild"]["p50_ms"] / rec["remove"]["p50_ms"], 2)
    rec["remove_over_memcpy"] = round(rec["remove"]["p50_ms"] / rec["memcpy_twice"]["p50_ms"], 2) if rec["memcpy_twice"]["p50_ms"] > 0 else None
    print(json.dumps(rec), flush=True)
    index.close()


def child_search(args, torch, vf, dev):
    import numpy as np
    n, n0, d, nq, k = args.n, args.search_n0, args.d, 64, 100
    rows = make_rows(torch, n0, d, args.seed, dev)
    gone = np.sort(np.random.default_rng(args.seed).choice(n0, n0 - n, replace=False))
    if args.setting == "search_shrunk":
        index = vf.DenseIndex(rows)
        assert index.remove(gone) == n0 - n
    else:
        keep = torch.ones(n0, dtype=torch.bool, device=dev)
        keep[torch.from_numpy(gone).to(dev)] = False
        index = vf.DenseIndex(rows[keep].contiguous())
    del rows
    torch.cuda.empty_cache()
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
                      "checksum_ids": int(ids[0].sum().item()), "checksum_scores": float(sc[0].double().sum().item())}), flush=True)
    index.close()


def child(args):
    import torch
    import veritasfi_amd as vf
    dev = torch.device("cuda:0")
    if args.setting.startswith("search"):
        child_search(args, torch, vf, dev)
    else:
        child_remove(args, torch, vf, dev)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="100000,1000000", help="rows in the index (comma list)")
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--m", type=int, default=100, help="rows per removal of the tail and scatter patterns")
    ap.add_argument("--filing", type=int, default=10_000, help="rows of the contiguous run")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--search-n", type=int, default=1_000_000)
    ap.add_argument("--search-n0", type=int, default=1_100_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed search window, at least")
    ap.add_argument("--timeout", type=int, default=180, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--only", choices=["remove", "search"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_index_remove.log"))
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
               "--d", str(args.d), "--m", str(args.m), "--filing", str(args.filing), "--calls", str(args.calls), "--seed", str(args.seed),
               "--window", str(args.window), "--search-n0", str(args.search_n0)]
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
    if args.only in (None, "remove"):
        recs = {}
        for rnd in range(2):                                         # two passes over the settings, alternating
            for n in ns:
                for setting in ("remove_tail", "remove_scatter", "remove_filing"):
                    rec = run(setting, n)
                    if rec is None:
                        return 1
                    recs.setdefault((setting, n), []).append(rec)
        for (setting, n), v in sorted(recs.items()):
            rm, rb, cp = ([r[key]["p50_ms"] for r in v] for key in ("remove", "rebuild", "memcpy_twice"))
            say(f"# {setting:15s} n={n:9d}  remove p50 {min(rm):8.4f} .. {max(rm):8.4f} ms | rebuild p50 {min(rb):8.4f} .. {max(rb):8.4f} ms "
                f"(+{v[0]['rebuild_extra_MB']} MB) = {statistics.median(rb) / statistics.median(rm):6.2f} x | two copies of the {v[0]['moved_MB_p50']} MB moved "
                f"{min(cp):8.4f} .. {max(cp):8.4f} ms: remove = {statistics.median(rm) / max(statistics.median(cp), 1e-9):6.2f} x")
    if args.only in (None, "search"):
        t = {"search_shrunk": [], "search_built": []}
        for rnd in range(args.rounds):
            for setting in (("search_shrunk", "search_built") if rnd % 2 == 0 else ("search_built", "search_shrunk")):
                rec = run(setting, args.search_n)
                if rec is None:
                    return 1
                t[setting].append(rec)
        for setting, rs in t.items():
            v = [r["ms_per_batch"] for r in rs]
            say(f"# {setting:13s} n={args.search_n} nq=64 k=100: median {statistics.median(v):.4f} ms/batch (min {min(v):.4f} max {max(v):.4f}), kernel "
                f"{rs[-1]['scan_kernel']} image {rs[-1]['scan_image']}, ids checksum {rs[-1]['checksum_ids']}, scores checksum {rs[-1]['checksum_scores']}")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
