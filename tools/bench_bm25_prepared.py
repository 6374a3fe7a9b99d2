#!/usr/bin/env python3
"""What a PREPARED BM25 row filter buys (BM25Retriever.prepare_subset -> search_columns(subset=<BM25Subset>): vf_bm25_search with
VF_BM25_PREPARED, one device call that uploads only the query), beside the unprepared calls with the same rows on the same handle, the
unfiltered call, and what the one-time prepare costs.

    python tools/bench_bm25_prepared.py                      # every setting, written to profiles/r20_bm25_prepared.log as well
    python tools/bench_bm25_prepared.py --m 1000 --nq 1      # a part of it

tools/bench_bm25_substats.py's method and data: one Zipf index of --n documents (vocabulary 200 000, mean length 8, 10-token queries from
the same law), built ONCE by the driver into a temporary directory.  A SETTING is a filter size (m rows drawn uniformly) and runs in a
FRESH process (this script calls itself with --child, one `timeout`-bounded child per setting) on a LIVE retriever; the settings
alternate over --rounds passes, and the driver stops at the first child that fails.  In a child, for every nq of --nq at k = --k,
--calls calls each after 3 warm-up calls, p50 of a host clock around the call, per CALL, not per query:

  prepared_corpus / prepared_subset   search_columns(queries, k, subset=<BM25Subset of that mode>)
  corpus / subset                     the unprepared calls, search_columns(queries, k, subset=ids[, stats="subset"]): the baseline
  unfiltered                          search_columns(queries, k)
  prepare                             prepare_subset + close, --prepare-calls calls per mode, and the medians of the retriever's own clocks
                                      (last_prepare_ms): pack (ids -> bitmap), prepare (corpus mode: the upload; subset mode: the upload,
                                      the length sum, the all-columns df count and the counts' way back, so count = the difference), host
                                      (numpy's log over the vocabulary), arm (the idf table's upload)

Every prepared result is compared with the unprepared one (ids and score bits) before anything is timed.  Last, in a process of its own,
EnsembleRetriever.invoke at n/2 passing rows with a dict against a PreparedWhere, per where_statistics value (--ensemble-calls calls; the
dense leg, d = 32, and the BM25 leg are on, the title-summary leg is off).  Needs a GPU."""
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
    n, m, k = args.n, args.m_one, args.k_one
    r = vf.BM25Retriever(args.index_dir, stemmer=None, load_corpus=False, live=True)
    assert r.num_docs == n
    rng = np.random.default_rng(args.seed + m)
    ids = np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    qrng = np.random.default_rng(args.seed)
    queries = [((qrng.zipf(1.25, size=args.query_len) - 1) % args.vocab).astype(np.int32) for _ in range(max(args.nqs))]

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))

    prep = {}
    for mode in ("corpus", "subset"):
        split = []

        def prepare():
            s = r.prepare_subset(ids, stats=mode)
            split.append(dict(r.last_prepare_ms))
            s.close()

        total = p50(prepare, args.prepare_calls, warm=1)
        prep[mode] = dict({key: round(statistics.median(s[key] for s in split[1:]), 4) for key in ("pack", "prepare", "host", "arm")}, total=total)
    pc, ps = r.prepare_subset(ids), r.prepare_subset(ids, stats="subset")
    for nq in args.nqs:
        qs = queries[:nq]
        assert same(r.search_columns(qs, k, subset=pc), r.search_columns(qs, k, subset=ids)), "a prepared corpus-mode search differs"
        assert same(r.search_columns(qs, k, subset=ps), r.search_columns(qs, k, subset=ids, stats="subset")), "a prepared subset-mode search differs"
        rec = {"m": m, "n": n, "nq": nq, "k": k,
               "prepared_corpus_p50_ms": p50(lambda: r.search_columns(qs, k, subset=pc), args.calls),
               "prepared_subset_p50_ms": p50(lambda: r.search_columns(qs, k, subset=ps), args.calls),
               "corpus_p50_ms": p50(lambda: r.search_columns(qs, k, subset=ids), args.calls),
               "subset_p50_ms": p50(lambda: r.search_columns(qs, k, subset=ids, stats="subset"), args.calls),
               "unfiltered_p50_ms": p50(lambda: r.search_columns(qs, k), args.calls)}
        for mode in ("corpus", "subset"):
            for key, v in prep[mode].items():
                rec[f"prepare_{mode}_{key}_ms"] = v
        rec["prepared_bytes"] = r.info()["prepared_bytes"]
        print(json.dumps(rec), flush=True)
    r.close()
    return 0


class _Store:
    def __init__(self, n, metas, embs):
        self.n, self.metas, self.embs = n, metas, embs

    def get(self, ids=None, include=()):
        if ids is None:
            return {"documents": None, "metadatas": self.metas, "embeddings": self.embs}
        return {"documents": [f"chunk {i}" for i in ids], "metadatas": [self.metas[int(i[1:])] for i in ids]}


class _Emb:
    def __init__(self, d):
        self.d = d

    def embed_query(self, text):
        import zlib
        import numpy as np
        return np.random.default_rng(zlib.crc32(text.encode())).standard_normal(self.d).astype(np.float32)


def ensemble_child(args):
    import numpy as np
    import veritasfi_amd as vf
    from veritasfi_amd.ensemble import EnsembleRetriever
    n, d = args.n, 32
    rng = np.random.default_rng(args.seed)
    embs = rng.standard_normal((n, d)).astype(np.float32)
    metas = [{"doc_id": f"d{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": "t", "tenant": "a" if i % 2 == 0 else "b"} for i in range(n)]
    ts = _Store(1, [None], np.ones((1, d), np.float32))
    ts.get = lambda ids=None, include=(): {"documents": ["t"], "embeddings": np.ones((1, d), np.float32)}
    qrng = np.random.default_rng(args.seed)
    query = " ".join(f"t{int(c)}" for c in (qrng.zipf(1.25, size=args.query_len) - 1) % args.vocab)
    where = {"tenant": "a"}
    with vf.BM25Retriever(args.index_dir, stemmer=None, load_corpus=False, live=True) as bm:
        for mode in ("corpus", "subset"):
            er = EnsembleRetriever("unused", _Store(n, metas, embs), ts, 5, _Emb(d), bm25_k=12, faiss_ts_k=0, bm25_retriever=bm, where_statistics=mode)
            t0 = time.perf_counter()
            pw = er.prepare_where(where)
            t_prepare = 1e3 * (time.perf_counter() - t0)
            assert er.invoke(query, [], where=pw) == er.invoke(query, [], where=where) and pw.passing.size == (n + 1) // 2
            rec = {"ensemble": mode, "n": n, "passing": int(pw.passing.size), "legs": "dense (faiss_k=5, d=32) + BM25 (bm25_k=12); title-summary leg off",
                   "prepared_where_p50_ms": p50(lambda: er.invoke(query, [], where=pw), args.ensemble_calls),
                   "dict_p50_ms": p50(lambda: er.invoke(query, [], where=where), args.ensemble_calls),
                   "unfiltered_p50_ms": p50(lambda: er.invoke(query, []), args.ensemble_calls), "prepare_where_ms": round(t_prepare, 3)}
            pw.close()
            print(json.dumps(rec), flush=True)
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
    ap.add_argument("--prepare-calls", type=int, default=5)
    ap.add_argument("--ensemble-calls", type=int, default=15)
    ap.add_argument("--no-ensemble", action="store_true")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_bm25_prepared.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--ensemble-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--m-one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--k-one", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--index-dir", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.nqs = [int(x) for x in args.nq.split(",")]
    if args.child:
        return child(args)
    if args.ensemble_child:
        return ensemble_child(args)
    import numpy as np
    from veritasfi_amd import bm25 as B
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    say("# " + " ".join(["tools/bench_bm25_prepared.py"] + sys.argv[1:]))
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
        common = ["--n", str(args.n), "--vocab", str(args.vocab), "--query-len", str(args.query_len), "--seed", str(args.seed), "--index-dir", d]

        def run(extra, what):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__)] + extra + common
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:
                say(f"# {what}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}")
                return None
            recs = []
            for line in proc.stdout.splitlines():
                if line.startswith("{"):
                    say(line)
                    recs.append(json.loads(line))
            return recs

        settings = [int(x) for x in args.m.split(",")]
        got = {}
        for rnd in range(args.rounds):
            for m in (settings if rnd % 2 == 0 else settings[::-1]):    # the settings alternate: no setting always follows the same one
                recs = run(["--child", "--m-one", str(m), "--nq", args.nq, "--k-one", str(args.k), "--calls", str(args.calls),
                            "--prepare-calls", str(args.prepare_calls)], f"m={m}")
                if recs is None:
                    return 1
                for rec in recs:
                    got.setdefault((m, rec["nq"]), []).append(rec)
        say("# medians over the rounds, per call: prepared | unprepared (the baseline) | unfiltered; then the one-time prepare per mode")
        for (m, nq), v in sorted(got.items()):
            med = {key: statistics.median(rec[key] for rec in v) for key in v[0] if key.endswith("_ms")}
            say(f"# m={m:7d} nq={nq:3d} k={args.k}  corpus: prepared {med['prepared_corpus_p50_ms']:7.4f} ms | unprepared {med['corpus_p50_ms']:7.4f} ms = "
                f"{med['corpus_p50_ms'] / med['prepared_corpus_p50_ms']:5.2f} x   subset: prepared {med['prepared_subset_p50_ms']:7.4f} ms | unprepared "
                f"{med['subset_p50_ms']:7.4f} ms = {med['subset_p50_ms'] / med['prepared_subset_p50_ms']:5.2f} x   unfiltered {med['unfiltered_p50_ms']:7.4f} ms")
        for (m, nq), v in sorted(got.items()):
            if nq != min(args.nqs):
                continue
            med = {key: statistics.median(rec[key] for rec in v) for key in v[0] if key.endswith("_ms")}
            upload = med["prepare_corpus_prepare_ms"]
            say(f"# m={m:7d} prepare, once per (filter, generation)  corpus {med['prepare_corpus_total_ms']:7.3f} ms (pack {med['prepare_corpus_pack_ms']:6.3f} + upload "
                f"{upload:6.3f})   subset {med['prepare_subset_total_ms']:7.3f} ms (pack {med['prepare_subset_pack_ms']:6.3f} + upload {upload:6.3f} + count "
                f"{med['prepare_subset_prepare_ms'] - upload:6.3f} + host log {med['prepare_subset_host_ms']:6.3f} + arm {med['prepare_subset_arm_ms']:6.3f})")
        if not args.no_ensemble:
            say(f"# EnsembleRetriever.invoke, host clock, p50 of {args.ensemble_calls} calls, one query, where = half of the chunks")
            if run(["--ensemble-child", "--ensemble-calls", str(args.ensemble_calls)], "ensemble") is None:
                return 1
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
