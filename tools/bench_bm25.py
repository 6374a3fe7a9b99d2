"""Time the BM25 leg (BM25Retriever.search_columns: vf_bm25_search) at 1M and 10M documents beside bm25s's numpy scorer.

``python tools/bench_bm25.py [--sizes 1000000,10000000] [--reps 30]`` builds a Zipf-distributed token-id index per size (Lucene
weights, bm25.build_bm25_index_from_ids), draws 10-token queries from the same Zipf law, and prints one line per
(size, batch, k): per-query p50 / p99 of the device call (host clock around the whole call, which ends in a stream
synchronise), postings scored per second, and the numpy scorer's time for the same call (np.add.at per token in order, then
an exact canonical top-k).  Every device result is checked against the numpy one.  Needs a GPU.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import veritasfi_amd as vf  # noqa: E402
from veritasfi_amd import bm25 as B  # noqa: E402


def numpy_call(ix, queries, k):
    out = []
    for cols in queries:
        sc = np.zeros(ix.num_docs, np.float32)
        for c in cols:
            seg = slice(ix.indptr[c], ix.indptr[c + 1])
            np.add.at(sc, ix.indices[seg], ix.data[seg])
        n = sc.size
        cand = np.arange(n) if k >= n else np.flatnonzero(sc >= np.partition(sc, n - k)[n - k])
        o = cand[np.lexsort((cand, -sc[cand]))][:k]
        out.append((o, sc[o]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000")
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--doc-len", type=float, default=8.0)
    ap.add_argument("--query-len", type=int, default=10)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--numpy-reps", type=int, default=1)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    for n in (int(s) for s in args.sizes.split(",")):
        with tempfile.TemporaryDirectory() as d:
            t0 = time.perf_counter()
            lens = rng.poisson(args.doc_len, size=n)
            off = np.zeros(n + 1, np.int64)
            np.cumsum(lens, out=off[1:])
            toks = (rng.zipf(1.25, size=int(off[-1])) - 1) % args.vocab
            B.build_bm25_index_from_ids(off, toks, args.vocab, d)
            del toks
            ix = B.load_bm25_index(d, load_corpus=False)
            t1 = time.perf_counter()
            r = vf.BM25Retriever(d, stemmer=None)
            t2 = time.perf_counter()
            print(f"n_docs={n} vocab={args.vocab} nnz={ix.data.size} build {t1 - t0:.1f} s, device load {t2 - t1:.1f} s, "
                  f"slots {r.info()['slots']}", flush=True)
            queries = [((rng.zipf(1.25, size=args.query_len) - 1) % args.vocab).astype(np.int32) for _ in range(64)]
            plen = np.diff(ix.indptr)
            for batch, k in ((1, 100), (1, 2048), (1, n), (64, 100), (64, 2048)):
                qs = queries[:batch]
                postings = int(sum(plen[c].sum() for c in qs))
                r.search_columns(qs, k)   # warm-up (scratch allocation, code load)
                reps = args.reps if k < n else max(3, args.reps // 10)
                times = []
                for _ in range(reps):
                    a = time.perf_counter()
                    ids, sc = r.search_columns(qs, k)
                    times.append(time.perf_counter() - a)
                times = np.asarray(times) / batch
                a = time.perf_counter()
                for _ in range(args.numpy_reps):
                    ref = numpy_call(ix, qs if batch == 1 else qs[:4], k)
                t_np = (time.perf_counter() - a) / args.numpy_reps / (1 if batch == 1 else 4)
                ok = all(np.array_equal(ids[i], ref[i][0]) and np.array_equal(sc[i].view(np.uint32), ref[i][1].view(np.uint32))
                         for i in range(len(ref)))
                print(f"  batch={batch:3d} k={k:9d}: device per query p50 {np.percentile(times, 50) * 1e3:8.3f} ms "
                      f"p99 {np.percentile(times, 99) * 1e3:8.3f} ms, {postings / batch / 1e6:6.2f} M postings/query, "
                      f"{postings / (times.mean() * batch) / 1e9:6.2f} G postings/s | numpy {t_np * 1e3:9.1f} ms/query "
                      f"| {'bit-equal' if ok else 'MISMATCH'}", flush=True)
                if not ok:
                    raise SystemExit("device result differs from the numpy scorer")
            r.close()


if __name__ == "__main__":
    main()
