#!/usr/bin/env python3
"""What a BM25 search restricted to a set of rows costs (BM25Retriever.search_columns(subset=): vf_bm25_search with VF_BM25_FILTER), beside
the unfiltered call and the route the ensemble took before the kernels could filter.

    python tools/bench_bm25_filter.py                      # every setting, written to profiles/r17_bm25_filter.log as well
    python tools/bench_bm25_filter.py --m 1000 --nq 1      # a part of it

One Zipf index of --n documents in tools/bench_bm25.py's shape (vocabulary 200 000, mean length 8, 10-token queries from the same law),
built ONCE by the driver into a temporary directory.  A SETTING is a filter size and a layout -- `contiguous`: one run of m rows in
the middle; `scattered`: m rows drawn uniformly -- and runs in a FRESH process (this script calls itself with --child, one
`timeout`-bounded child per setting), the settings alternate over --rounds passes, and the driver stops at the first child that
fails.  In a child, for every nq of --nq at k = --k, --calls calls each after 3 warm-up calls, p50 of a host clock around the call
(every call ends in a stream synchronise), per CALL, not per query:

  filtered    search_columns(queries, k, subset=ids): packing the sorted ids into the bitmap (also timed alone: pack), its upload
              (n / 8 bytes), the filtered scatter, select, sort, tail over every bitmap block
  unfiltered  search_columns(queries, k)
  parent      the ensemble's former route to the same answer, one query at a time as the ensemble runs it: the device's full ranking
              search_columns([q], n) (parent_device) and then, on the host, the list of n ints BM25Retriever._result builds and
              EnsembleRetriever._bm25_branch's loop over n pairs against the set of passing rows (parent_host).  Timed on --parent-queries
              queries with --parent-calls calls each; for nq > 1 the figure is per query, times nq.

Every filtered result is compared with the parent route's (ids and score bits) before anything is timed.  Needs a GPU."""
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
    from veritasfi_amd import bm25 as B
    n, m, k = args.n, args.m_one, args.k_one
    r = vf.BM25Retriever(args.index_dir, stemmer=None, load_corpus=False)
    assert r.num_docs == n
    rng = np.random.default_rng(args.seed + m)
    ids = np.arange(n // 2 - m // 2, n // 2 - m // 2 + m, dtype=np.int64) if args.layout == "contiguous" else np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    allow = set(ids.tolist())
    qrng = np.random.default_rng(args.seed)
    queries = [((qrng.zipf(1.25, size=args.query_len) - 1) % args.vocab).astype(np.int32) for _ in range(max(args.nqs))]

    def parent_device(q):
        return r.search_columns([q], n)

    def parent_host(full):
        b_ids, b_scores = r._result(full[0][0], full[1][0])
        return [(int(row), s) for row, s in zip(b_ids, b_scores) if int(row) in allow][:k]

    for nq in args.nqs:
        qs = queries[:nq]
        got_ids, got_sc = r.search_columns(qs, k, subset=ids)
        for i in range(min(nq, args.parent_queries)):
            kept = parent_host(parent_device(qs[i]))
            keep = min(k, m)
            assert got_ids[i][:keep].tolist() == [row for row, _ in kept], "the filtered call differs from the parent route"
            assert np.array_equal(got_sc[i][:keep].view(np.uint32), np.asarray([s for _, s in kept], np.float32).view(np.uint32))
            assert (got_ids[i][keep:] == -1).all()
        t_filtered = p50(lambda: r.search_columns(qs, k, subset=ids), args.calls)
        t_pack = p50(lambda: B.filter_words(ids, n), args.calls)
        t_plain = p50(lambda: r.search_columns(qs, k), args.calls)
        dev, host = [], []
        for q in qs[:args.parent_queries]:
            dev.append(p50(lambda: parent_device(q), args.parent_calls, warm=1))
            full = parent_device(q)
            host.append(p50(lambda: parent_host(full), args.parent_calls, warm=1))
        t_dev, t_host = statistics.median(dev) * nq, statistics.median(host) * nq
        print(json.dumps({"m": m, "layout": args.layout, "n": n, "nq": nq, "k": k, "filtered_p50_ms": t_filtered, "pack_p50_ms": t_pack,
                          "unfiltered_p50_ms": t_plain, "parent_device_ms": round(t_dev, 3), "parent_host_ms": round(t_host, 3),
                          "parent_ms": round(t_dev + t_host, 3), "bitmap_bytes": (n + 31) // 32 * 4}), flush=True)
    r.close()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--doc-len", type=float, default=8.0)
    ap.add_argument("--query-len", type=int, default=10)
    ap.add_argument("--m", default="1000,10000,100000,500000", help="filter sizes (comma list)")
    ap.add_argument("--nq", default="1,64")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--parent-calls", type=int, default=3)
    ap.add_argument("--parent-queries", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_bm25_filter.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--layout", default="", help=argparse.SUPPRESS)
    ap.add_argument("--m-one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--k-one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--index-dir", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.nqs = [int(x) for x in args.nq.split(",")]
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

    say("# " + " ".join(["tools/bench_bm25_filter.py"] + sys.argv[1:]))
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

        def run(m, layout):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--m-one", str(m), "--layout", layout,
                   "--n", str(args.n), "--vocab", str(args.vocab), "--query-len", str(args.query_len), "--nq", args.nq, "--k-one", str(args.k),
                   "--calls", str(args.calls), "--parent-calls", str(args.parent_calls), "--parent-queries", str(args.parent_queries),
                   "--seed", str(args.seed), "--index-dir", d]
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

        settings = [(m, layout) for m in (int(x) for x in args.m.split(",")) for layout in ("contiguous", "scattered")]
        got = {}
        for rnd in range(args.rounds):
            for m, layout in (settings if rnd % 2 == 0 else settings[::-1]):    # the settings alternate: no setting always follows the same one
                recs = run(m, layout)
                if recs is None:
                    return 1
                for rec in recs:
                    got.setdefault((m, layout, rec["nq"]), []).append(rec)
    say("# medians over the rounds, per call: filtered (of which packing the ids) | unfiltered | the parent route = device full ranking + host list and loop")
    for (m, layout, nq), v in sorted(got.items()):
        med = {key: statistics.median(rec[key] for rec in v) for key in ("filtered_p50_ms", "pack_p50_ms", "unfiltered_p50_ms", "parent_device_ms", "parent_host_ms", "parent_ms")}
        say(f"# m={m:7d} {layout:10s} nq={nq:3d} k={args.k}  filtered {med['filtered_p50_ms']:9.4f} ms (pack {med['pack_p50_ms']:7.4f}) | unfiltered {med['unfiltered_p50_ms']:9.4f} ms "
            f"= {med['unfiltered_p50_ms'] / med['filtered_p50_ms']:5.2f} x | parent {med['parent_ms']:10.3f} ms (device {med['parent_device_ms']:9.3f} + host {med['parent_host_ms']:10.3f}) "
            f"= {med['parent_ms'] / med['filtered_p50_ms']:8.1f} x")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
