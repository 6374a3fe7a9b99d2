#!/usr/bin/env python3
"""What a row list PER QUERY buys the dense leg (DenseIndex.search(queries, k, subsets=[...]): vf_index_search_device with
VF_SEARCH_SUBSETS, one device call for a batch whose queries belong to different tenants), beside the only route there was before it:
group the queries by list, one search(subset=<RowSubset>) per distinct list, the rows put back in order.

    python tools/bench_subset_multi.py                        # every setting, written to profiles/r23_subset_multi.log as well
    python tools/bench_subset_multi.py --m 1000 --f 1,64      # a part of it

tools/bench_bm25_multi.py's method: one box; a SETTING is a list length m and runs in a FRESH process (this script calls itself with
--child, one `timeout`-bounded child per setting); the settings alternate over --rounds passes, and the driver stops at the first child
that fails.  A child builds an n x d fp16 index of N(0, 1) rows, makes max(F) device-resident lists (RowSubset) of m scattered rows each
and, for every F of --f, gives query i of --nq queries the list i mod F; at k = --k, --calls calls each after 3 warm-up calls, p50 of a
host clock around the call, per BATCH:

  multi       search(queries, k, subsets=[...]): the one call
  grouped     the queries grouped by list, search(group, k, subset=<RowSubset>) per distinct list, rows scattered back
  one_list    F = 1 only: search(queries, k, subset=<the one RowSubset>), to show what the tile table and the sentinels cost

The multi result is compared with the grouped one (ids and score bits) before anything is timed.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def p50(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(t), 4)


def child(args):
    import numpy as np
    import veritasfi_amd as vf
    n, d, m, k, nq = args.n, args.d, args.m_one, args.k, args.nq
    rng = np.random.default_rng(args.seed)
    rows = np.empty((n, d), np.float16)
    for r0 in range(0, n, 100_000):      # in pieces: no fp32 copy of the whole corpus
        rows[r0:r0 + 100_000] = rng.standard_normal((min(100_000, n - r0), d), dtype=np.float32)
    queries = rng.standard_normal((nq, d), dtype=np.float32)
    ix = vf.DenseIndex(rows)
    lrng = np.random.default_rng(args.seed + m)
    lists = [ix.row_subset(np.sort(lrng.choice(n, m, replace=False)).astype(np.int64)) for _ in range(max(args.fs))]
    for F in args.fs:
        subsets = [lists[i % F] for i in range(nq)]
        groups = [(lists[f], list(range(f, nq, F))) for f in range(F)]
        group_queries = [np.ascontiguousarray(queries[rows_]) for _, rows_ in groups]

        def multi():
            return ix.search(queries, k, subsets=subsets)

        def grouped():
            ids, sc = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
            for (s, rows_), qs in zip(groups, group_queries):
                ids[rows_], sc[rows_] = ix.search(qs, k, subset=s)
            return ids, sc

        a, b = multi(), grouped()
        assert ix.stats()["path"] == 3, ix.stats()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "the multi call differs from the grouped route"
        multi()
        st = ix.stats()
        assert st["path"] == 4, st
        rec = {"m": m, "F": F, "n": n, "d": d, "nq": nq, "k": k, "tiles": st["subset_tiles"], "multi_p50_ms": p50(multi, args.calls),
               "grouped_p50_ms": p50(grouped, args.calls)}
        if F == 1:
            rec["one_list_p50_ms"] = p50(lambda: ix.search(queries, k, subset=lists[0]), args.calls)
        print(json.dumps(rec), flush=True)
    ix.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--m", default="1000,10000", help="list lengths (comma list; at most 16 384)")
    ap.add_argument("--f", default="1,4,16,64", help="distinct lists among the batch's queries (comma list)")
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_subset_multi.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--m-one", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.fs = [int(x) for x in args.f.split(",")]
    if args.child:
        return child(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say("# " + " ".join(["tools/bench_subset_multi.py"] + sys.argv[1:]))
    common = ["--n", str(args.n), "--d", str(args.d), "--seed", str(args.seed), "--f", args.f, "--nq", str(args.nq), "--k", str(args.k), "--calls", str(args.calls)]
    settings = [int(m) for m in args.m.split(",")]
    got = {}
    for rnd in range(args.rounds):
        for m in (settings if rnd % 2 == 0 else settings[::-1]):    # the settings alternate: no setting always follows the same one
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--m-one", str(m)] + common
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:
                say(f"# m={m}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}")
                return 1
            for line in proc.stdout.splitlines():
                if line.startswith("{"):
                    say(line)
                    rec = json.loads(line)
                    got.setdefault((m, rec["F"]), []).append(rec)
    say(f"# medians over the rounds, per batch of {args.nq} queries at k={args.k}: the one multi call | one call per distinct list, rows put back")
    for (m, F), v in sorted(got.items()):
        med = {key: statistics.median(rec[key] for rec in v) for key in v[0] if key.endswith("_ms")}
        one = f"   one-list call {med['one_list_p50_ms']:7.4f} ms" if "one_list_p50_ms" in med else ""
        say(f"# m={m:6d} F={F:2d} tiles={v[0]['tiles']:3d}  multi {med['multi_p50_ms']:7.4f} ms | grouped {med['grouped_p50_ms']:8.4f} ms = "
            f"{med['grouped_p50_ms'] / med['multi_p50_ms']:5.2f} x{one}")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
