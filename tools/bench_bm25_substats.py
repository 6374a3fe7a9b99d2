#!/usr/bin/env python3
"""What a filtered BM25 search scored by the subset's own statistics costs (BM25Retriever.search_columns(subset=, stats="subset"):
vf_bm25_search with VF_BM25_FILTER | VF_BM25_SUBSTATS, two device calls with numpy's log between them), beside the corpus mode on the
same handle and the only route to the same answer there was before: an index built from the subset's documents.

    python tools/bench_bm25_substats.py                      # every setting, written to profiles/r19_bm25_substats.log as well
    python tools/bench_bm25_substats.py --m 1000 --nq 1      # a part of it

One Zipf index of --n documents in tools/bench_bm25_filter.py's shape (vocabulary 200 000, mean length 8, 10-token queries from the same
law), built ONCE by the driver into a temporary directory together with its token ids.  A SETTING is a filter size (m rows drawn
uniformly) and runs in a FRESH process (this script calls itself with --child, one `timeout`-bounded child per setting) on a LIVE
retriever; the settings alternate over --rounds passes, and the driver stops at the first child that fails.  In a child, for every nq
of --nq at k = --k, --calls calls each after 3 warm-up calls, p50 of a host clock around the call, per CALL, not per query:

  subset      search_columns(queries, k, subset=ids, stats="subset"), and where its time goes, the medians of the retriever's own
              clocks (last_subset_ms): pack (ids -> bitmap), stage (upload, length sum, df count, counts back), host (numpy's idf and
              avgdl), search (idf up, the scatter that scores from tf, select, sort, tail)
  corpus      search_columns(queries, k, subset=ids) on the same handle: whole-corpus statistics, one device call
  rebuild     the former route: gather the subset's token ids, bm25_index_arrays over them (rebuild_index), vf_bm25_create
              (rebuild_create), one search of the same queries and the handle's release (rebuild_search); --rebuild-calls calls

Every subset result is compared with the rebuilt index's (ids mapped back, score bits) before anything is timed.  Needs a GPU."""
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
    from veritasfi_amd import _ffi
    from veritasfi_amd import bm25 as B
    n, m, k = args.n, args.m_one, args.k_one
    off, toks = np.load(os.path.join(args.index_dir, "doc_offsets.npy")), np.load(os.path.join(args.index_dir, "doc_tokens.npy"))
    r = vf.BM25Retriever(args.index_dir, stemmer=None, load_corpus=False, live=True)
    assert r.num_docs == n
    rng = np.random.default_rng(args.seed + m)
    ids = np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    qrng = np.random.default_rng(args.seed)
    queries = [((qrng.zipf(1.25, size=args.query_len) - 1) % args.vocab).astype(np.int32) for _ in range(max(args.nqs))]
    lib = _ffi.lib()

    def rebuild(qs, kk, clock=None):
        t0 = time.perf_counter()
        lens = off[ids + 1] - off[ids]
        soff = np.zeros(m + 1, np.int64)
        np.cumsum(lens, out=soff[1:])
        stoks = toks[np.repeat(off[ids] - soff[:-1], lens) + np.arange(int(soff[-1]))]
        indptr, indices, data = B.bm25_index_arrays(soff, stoks, args.vocab, r._k1, r._b)
        t1 = time.perf_counter()
        h = _ffi.vp()
        _ffi.check(lib.vf_bm25_create(indptr.ctypes.data_as(_ffi.p_i64), int(indptr.size - 1), indices.ctypes.data_as(_ffi.p_i32),
                                      data.ctypes.data_as(_ffi.p_f32), int(data.size), m, 0, _ffi.ctypes.byref(h), None), "vf_bm25_create")
        t2 = time.perf_counter()
        qoff = np.zeros(len(qs) + 1, np.int64)
        np.cumsum([q.size for q in qs], out=qoff[1:])
        terms = np.ascontiguousarray(np.concatenate(qs), np.int32)
        out_ids, out_sc = np.empty((len(qs), kk), np.int64), np.empty((len(qs), kk), np.float32)
        _ffi.check(lib.vf_bm25_search(h, qoff.ctypes.data_as(_ffi.p_i64), terms.ctypes.data_as(_ffi.p_i32), len(qs), kk,
                                      out_ids.ctypes.data_as(_ffi.p_i64), out_sc.ctypes.data_as(_ffi.p_f32)), "vf_bm25_search")
        lib.vf_bm25_create(None, 0, None, None, 0, 0, 0, _ffi.ctypes.byref(h), None)
        if clock is not None:
            clock.append((1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (time.perf_counter() - t2)))
        return ids[out_ids], out_sc

    for nq in args.nqs:
        qs = queries[:nq]
        kk = min(k, m)
        got_ids, got_sc = r.search_columns(qs, k, subset=ids, stats="subset")
        want_ids, want_sc = rebuild(qs, kk)
        assert np.array_equal(got_ids[:, :kk], want_ids), "stats='subset' differs from the index rebuilt over the subset"
        assert np.array_equal(got_sc[:, :kk].view(np.uint32), want_sc.view(np.uint32))
        split = []

        def subset_call():
            r.search_columns(qs, k, subset=ids, stats="subset")
            split.append(dict(r.last_subset_ms))

        t_subset = p50(subset_call, args.calls)
        parts = {key: round(statistics.median(s[key] for s in split[3:]), 4) for key in ("pack", "stage", "host", "search")}
        t_corpus = p50(lambda: r.search_columns(qs, k, subset=ids), args.calls)
        clock = []
        t_rebuild = p50(lambda: rebuild(qs, kk, clock), args.rebuild_calls, warm=1)
        rb = [round(statistics.median(c[i] for c in clock[1:]), 3) for i in range(3)]
        print(json.dumps({"m": m, "n": n, "nq": nq, "k": k, "subset_p50_ms": t_subset, "pack_ms": parts["pack"], "stage_ms": parts["stage"],
                          "host_ms": parts["host"], "search_ms": parts["search"], "corpus_p50_ms": t_corpus, "rebuild_p50_ms": t_rebuild,
                          "rebuild_index_ms": rb[0], "rebuild_create_ms": rb[1], "rebuild_search_ms": rb[2]}), flush=True)
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
    ap.add_argument("--rebuild-calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_bm25_substats.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
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

    say("# " + " ".join(["tools/bench_bm25_substats.py"] + sys.argv[1:]))
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        rng = np.random.default_rng(0)
        lens = rng.poisson(args.doc_len, size=args.n)
        off = np.zeros(args.n + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        toks = (rng.zipf(1.25, size=int(off[-1])) - 1) % args.vocab
        B.build_bm25_index_from_ids(off, toks, args.vocab, d)
        np.save(os.path.join(d, "doc_offsets.npy"), off)
        np.save(os.path.join(d, "doc_tokens.npy"), toks.astype(np.int64))
        say(f"# index: n_docs={args.n} vocab={args.vocab} tokens={toks.size} built in {time.perf_counter() - t0:.1f} s")
        del toks

        def run(m):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--m-one", str(m),
                   "--n", str(args.n), "--vocab", str(args.vocab), "--query-len", str(args.query_len), "--nq", args.nq, "--k-one", str(args.k),
                   "--calls", str(args.calls), "--rebuild-calls", str(args.rebuild_calls), "--seed", str(args.seed), "--index-dir", d]
            proc = subprocess.run(cmd, capture_output=True, text=True)
            if proc.returncode != 0:
                say(f"# m={m}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}")
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
                recs = run(m)
                if recs is None:
                    return 1
                for rec in recs:
                    got.setdefault((m, rec["nq"]), []).append(rec)
    say("# medians over the rounds, per call: subset = pack + stage + host idf + search | corpus mode, same handle | the rebuilt index = build + create + search")
    for (m, nq), v in sorted(got.items()):
        med = {key: statistics.median(rec[key] for rec in v) for key in v[0] if key.endswith("_ms")}
        say(f"# m={m:7d} nq={nq:3d} k={args.k}  subset {med['subset_p50_ms']:8.4f} ms (pack {med['pack_ms']:7.4f} + stage {med['stage_ms']:7.4f} + host {med['host_ms']:7.4f} "
            f"+ search {med['search_ms']:7.4f}) | corpus {med['corpus_p50_ms']:8.4f} ms = {med['subset_p50_ms'] / med['corpus_p50_ms']:5.2f} x of it | rebuild "
            f"{med['rebuild_p50_ms']:10.3f} ms (index {med['rebuild_index_ms']:9.3f} + create {med['rebuild_create_ms']:8.3f} + search {med['rebuild_search_ms']:8.3f}) "
            f"= {med['rebuild_p50_ms'] / med['subset_p50_ms']:8.1f} x")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
