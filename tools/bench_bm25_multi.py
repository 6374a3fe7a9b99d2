#!/usr/bin/env python3
"""What a prepared BM25 filter PER QUERY buys (search_columns(queries, k, subsets=[...]): vf_bm25_search with VF_BM25_PREPARED in mode
VF_BM25_PREPARED_PER_QUERY, one device call for a batch whose queries belong to different tenants), beside the only route there was
before it: group the queries by filter, one prepared call per distinct filter, the rows put back in order.

    python tools/bench_bm25_multi.py                        # every setting, written to profiles/r22_bm25_multi.log as well
    python tools/bench_bm25_multi.py --m 1000 --f 1,64      # a part of it

tools/bench_bm25_prepared.py's method and data: one Zipf index of --n documents (vocabulary 200 000, mean length 8, 10-token queries from
the same law), built ONCE by the driver into a temporary directory.  A SETTING is (filter size m, statistics mode) and runs in a FRESH
process (this script calls itself with --child, one `timeout`-bounded child per setting) on a LIVE retriever; the settings alternate over
--rounds passes, and the driver stops at the first child that fails.  A child prepares max(F) distinct filters of m scattered rows each and,
for every F of --f, gives query i of --nq queries the filter i mod F; at k = --k, --calls calls each after 3 warm-up calls, p50 of a
host clock around the call, per BATCH:

  multi       search_columns(queries, k, subsets=[...]): the one call
  grouped     the queries grouped by filter, search_columns(group, k, subset=<BM25Subset>) per distinct filter, rows scattered back
  one_token   F = 1 only: search_columns(queries, k, subset=<the one BM25Subset>), to show what reading the descriptors costs

The multi result is compared with the grouped one (ids and score bits) before anything is timed.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
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
    n, m, k, nq, mode = args.n, args.m_one, args.k, args.nq, args.mode_one
    r = vf.BM25Retriever(args.index_dir, stemmer=None, load_corpus=False, live=True)
    assert r.num_docs == n
    rng = np.random.default_rng(args.seed + m)
    prepared = [r.prepare_subset(np.sort(rng.choice(n, m, replace=False)).astype(np.int64), stats=mode) for _ in range(max(args.fs))]
    qrng = np.random.default_rng(args.seed)
    queries = [((qrng.zipf(1.25, size=args.query_len) - 1) % args.vocab).astype(np.int32) for _ in range(nq)]

    for F in args.fs:
        subsets = [prepared[i % F] for i in range(nq)]
        groups = [(prepared[f], list(range(f, nq, F))) for f in range(F)]
        group_queries = [[queries[i] for i in rows] for _, rows in groups]

        def multi():
            return r.search_columns(queries, k, subsets=subsets)

        def grouped():
            ids, sc = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
            for (s, rows), qs in zip(groups, group_queries):
                ids[rows], sc[rows] = r.search_columns(qs, k, subset=s)
            return ids, sc

        a, b = multi(), grouped()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "the multi call differs from the grouped route"
        rec = {"m": m, "mode": mode, "F": F, "n": n, "nq": nq, "k": k, "multi_p50_ms": p50(multi, args.calls), "grouped_p50_ms": p50(grouped, args.calls)}
        if F == 1:
            rec["one_token_p50_ms"] = p50(lambda: r.search_columns(queries, k, subset=prepared[0]), args.calls)
        print(json.dumps(rec), flush=True)
    r.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--doc-len", type=float, default=8.0)
    ap.add_argument("--query-len", type=int, default=10)
    ap.add_argument("--m", default="1000,100000", help="filter sizes (comma list)")
    ap.add_argument("--modes", default="corpus,subset")
    ap.add_argument("--f", default="1,4,16,64", help="distinct filters among the batch's queries (comma list)")
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_bm25_multi.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--m-one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--mode-one", default="corpus", help=argparse.SUPPRESS)
    ap.add_argument("--index-dir", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.fs = [int(x) for x in args.f.split(",")]
    if args.child:
        return child(args)
    import numpy as np
    from veritasfi_amd import bm25 as B
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say("# " + " ".join(["tools/bench_bm25_multi.py"] + sys.argv[1:]))
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        rng = np.random.default_rng(0)
        lens = rng.poisson(args.doc_len, size=args.n)
        off = np.zeros(args.n + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        toks = (rng.zipf(1.25, size=int(off[-1])) - 1) % args.vocab
        B.build_bm25_index_from_ids(off, toks, args.vocab, d)
        say(f"# index: n_docs={args.n} vocab={args.vocab} tokens={toks.size} built in {time.perf_counter() - t0:.1f} s")
        del toks
        common = ["--n", str(args.n), "--vocab", str(args.vocab), "--query-len", str(args.query_len), "--seed", str(args.seed), "--index-dir", d,
                  "--f", args.f, "--nq", str(args.nq), "--k", str(args.k), "--calls", str(args.calls)]
        settings = [(int(m), mode) for m in args.m.split(",") for mode in args.modes.split(",")]
        got = {}
        for rnd in range(args.rounds):
            for m, mode in (settings if rnd % 2 == 0 else settings[::-1]):    # the settings alternate: no setting always follows the same one
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--m-one", str(m), "--mode-one", mode] + common
                proc = subprocess.run(cmd, capture_output=True, text=True)
                if proc.returncode != 0:
                    say(f"# m={m} {mode}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}")
                    return 1
                for line in proc.stdout.splitlines():
                    if line.startswith("{"):
                        say(line)
                        rec = json.loads(line)
                        got.setdefault((m, mode, rec["F"]), []).append(rec)
        say(f"# medians over the rounds, per batch of {args.nq} queries at k={args.k}: the one multi call | one prepared call per distinct filter, rows put back")
        for (m, mode, F), v in sorted(got.items()):
            med = {key: statistics.median(rec[key] for rec in v) for key in v[0] if key.endswith("_ms")}
            one = f"   one-token call {med['one_token_p50_ms']:7.4f} ms" if "one_token_p50_ms" in med else ""
            say(f"# m={m:7d} {mode:6s} F={F:2d}  multi {med['multi_p50_ms']:7.4f} ms | grouped {med['grouped_p50_ms']:8.4f} ms = "
                f"{med['grouped_p50_ms'] / med['multi_p50_ms']:5.2f} x{one}")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
