#!/usr/bin/env python3
"""What evaluating an operator `where` on the device buys a request (EnsembleRetriever.rows_where / prepare_where / invoke(where=) with
Chroma's operator grammar: veritasfi_amd/where.py, vf_index_search_device with VF_SEARCH_WHERE), beside the only route there was before
it: the plain dict, which for a range must LIST every value that lies in it.

    python tools/bench_where.py                         # every filter, written to profiles/r24_where.log as well
    python tools/bench_where.py --filters A,B50         # a part of it

tools/bench_bm25_prepared.py's method: one box; a SETTING is a filter and runs in a FRESH process (this script calls itself with --child,
one `timeout`-bounded child per setting); the settings alternate over --rounds passes, and the driver stops at the first child that
fails.  A child builds an EnsembleRetriever over n chunks of d = 32 with the dense leg (faiss_k = 5) and the live BM25 leg (bm25_k = 12)
on and the title leg off; the metadata is `company` (1000 tenants, str), `date_published` (about 2500 distinct ISO dates) and
`page_number` (int).  Filters: A `{"company": {"$eq": c}}` (about n / 1000 rows); B10 / B50 / B90 `{"date_published": {"$lte": D}}` at about
10 / 50 / 90 % of the rows; C the `$and` of A and B50.  "parent" is the plain dict of the same meaning (B: every passing date listed), run
through the code the parent commit has.  p50 of a host clock around the call, after 3 warm-up calls:

  rows_where      parent | numpy (compile + WhereProgram.evaluate_numpy + flatnonzero) | device
  prepare_where   parent | device        (--prepare-calls calls, the object closed after each)
  invoke          parent | device        (where = the dict, per request, one query)
  device split    the C call (three launches and its one wait) | bitmap download | ids copy + download | RowMask

Every route's rows are compared before anything is timed.  Needs a GPU."""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILTERS = ("A", "B10", "B50", "B90", "C")
DAYS = 2500


def p50(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return round(statistics.median(t), 4)


class _Store:
    def __init__(self, metas, embs):
        self.metas, self.embs = metas, embs

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


def _day(i):
    return datetime.date.fromordinal(datetime.date(2018, 1, 1).toordinal() + int(i)).isoformat()


def child(args):
    import numpy as np
    import torch
    import veritasfi_amd as vf
    from veritasfi_amd import _ffi
    from veritasfi_amd import where as W
    from veritasfi_amd.ensemble import EnsembleRetriever
    n, d, name = args.n, 32, args.filter
    rng = np.random.default_rng(args.seed)
    embs = rng.standard_normal((n, d)).astype(np.float32)
    tenant, day, page = rng.integers(0, 1000, size=n).tolist(), rng.integers(0, DAYS, size=n).tolist(), rng.integers(1, 301, size=n).tolist()
    dates = [_day(i) for i in range(DAYS)]
    metas = [{"doc_id": f"d{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": "t", "company": f"tenant{tenant[i]:04d}",
              "date_published": dates[day[i]], "page_number": page[i]} for i in range(n)]
    ts = _Store([None], None)
    ts.get = lambda ids=None, include=(): {"documents": ["t"], "embeddings": np.ones((1, d), np.float32)}
    query = " ".join(f"t{int(c)}" for c in (np.random.default_rng(args.seed).zipf(1.25, size=args.query_len) - 1) % args.vocab)
    c = "tenant0007"
    cut = {"B10": DAYS // 10, "B50": DAYS // 2, "B90": DAYS * 9 // 10, "C": DAYS // 2}.get(name)
    if name == "A":
        where, parent = {"company": {"$eq": c}}, {"company": c}
    elif name == "C":
        where = {"$and": [{"company": {"$eq": c}}, {"date_published": {"$lte": dates[cut]}}]}
        parent = {"company": c, "date_published": dates[:cut + 1]}
    else:
        where, parent = {"date_published": {"$lte": dates[cut]}}, {"date_published": dates[:cut + 1]}
    with vf.BM25Retriever(args.index_dir, stemmer=None, load_corpus=False, live=True) as bm:
        er = EnsembleRetriever("unused", _Store(metas, embs), ts, 5, _Emb(d), bm25_k=12, faiss_ts_k=0, bm25_retriever=bm)
        ix = er.faiss_retriever.index
        fields = W.fields_of(where)

        def numpy_route():
            cols = {f: er._where_column(f) for f in fields}
            return np.flatnonzero(W.compile_where(where, cols, n=n).evaluate_numpy(cols, n)).astype(np.int64)

        t0 = time.perf_counter()
        cols = {f: er._where_column(f) for f in fields}
        t_columns = 1e3 * (time.perf_counter() - t0)
        rows = er.rows_where(where)
        assert np.array_equal(rows, er.rows_where(parent)) and np.array_equal(rows, numpy_route()), "the routes disagree"
        assert er.invoke(query, [], where=where) == er.invoke(query, [], where=parent)

        def prepare(w):
            er.prepare_where(w).close()

        rec = {"filter": name, "n": n, "passing": int(rows.size), "listed_values": len(parent.get("date_published", [])) if name != "A" else 1,
               "columns_once_ms": round(t_columns, 2),
               "rows_where_parent_p50_ms": p50(lambda: er.rows_where(parent), args.calls), "rows_where_numpy_p50_ms": p50(numpy_route, args.calls),
               "rows_where_device_p50_ms": p50(lambda: er.rows_where(where), args.calls),
               "prepare_parent_p50_ms": p50(lambda: prepare(parent), args.prepare_calls, warm=1), "prepare_device_p50_ms": p50(lambda: prepare(where), args.prepare_calls, warm=1),
               "invoke_parent_p50_ms": p50(lambda: er.invoke(query, [], where=parent), args.calls), "invoke_device_p50_ms": p50(lambda: er.invoke(query, [], where=where), args.calls),
               "invoke_unfiltered_p50_ms": p50(lambda: er.invoke(query, []), args.calls)}
        # the device route's parts, by the host clock around each (the columns are on the device already)
        program = W.compile_where(where, cols, n=n)
        dev = torch.device(f"cuda:{ix.device_id}")
        ptrs = [(cols[f]._device[ix.device_id][0].data_ptr(), None if cols[f]._device[ix.device_id][1] is None else cols[f]._device[ix.device_id][1].data_ptr())
                for f in program.fields]
        words = torch.empty(2 * ((n + 63) // 64), dtype=torch.int32, device=dev)
        ids = torch.empty(n, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        state = {}

        def call():
            rc, state["m"] = _ffi.eval_where_device(_ffi.lib(), ix._h, n, ptrs, program.leaves, program.ops, program.set_values, words.data_ptr(), ids.data_ptr(), n, stream)
            assert rc == 0

        def bitmap_down():
            state["words"] = words.cpu().numpy()

        def ids_down():
            state["ids"] = ids[:state["m"]].clone().cpu().numpy()

        rec.update({"compile_p50_ms": p50(lambda: W.compile_where(where, cols, n=n), args.calls), "call_p50_ms": p50(call, args.calls),
                    "bitmap_download_p50_ms": p50(bitmap_down, args.calls), "ids_download_p50_ms": p50(ids_down, args.calls),
                    "row_mask_p50_ms": p50(lambda: W.RowMask.from_words(state["words"].view(np.uint32), n, state["m"]), args.calls)})
        assert np.array_equal(state["ids"], rows + ix.id_offset)
        print(json.dumps(rec), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--doc-len", type=float, default=8.0)
    ap.add_argument("--query-len", type=int, default=10)
    ap.add_argument("--filters", default=",".join(FILTERS))
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--prepare-calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_where.log"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--filter", default="", help=argparse.SUPPRESS)
    ap.add_argument("--index-dir", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
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

    say("# " + " ".join(["tools/bench_where.py"] + sys.argv[1:]))
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
                  "--calls", str(args.calls), "--prepare-calls", str(args.prepare_calls)]
        settings = args.filters.split(",")
        got = {}
        for rnd in range(args.rounds):
            for name in (settings if rnd % 2 == 0 else settings[::-1]):    # the settings alternate: no setting always follows the same one
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--filter", name] + common
                proc = subprocess.run(cmd, capture_output=True, text=True)
                if proc.returncode != 0:
                    say(f"# {name}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}")
                    return 1
                for line in proc.stdout.splitlines():
                    if line.startswith("{"):
                        say(line)
                        got.setdefault(name, []).append(json.loads(line))
        say("# medians over the rounds, ms per call: parent | numpy | device")
        for name in settings:
            v = got[name]
            med = {key: statistics.median(rec[key] for rec in v) for key in v[0] if key.endswith("_ms")}
            say(f"# {name:3s} passing {v[0]['passing']:7d} listed {v[0]['listed_values']:5d}  rows_where {med['rows_where_parent_p50_ms']:8.3f} | {med['rows_where_numpy_p50_ms']:7.3f} | "
                f"{med['rows_where_device_p50_ms']:7.3f}   prepare_where {med['prepare_parent_p50_ms']:8.3f} | - | {med['prepare_device_p50_ms']:7.3f}   invoke {med['invoke_parent_p50_ms']:8.3f} | - | "
                f"{med['invoke_device_p50_ms']:7.3f}   (unfiltered {med['invoke_unfiltered_p50_ms']:6.3f})")
        say("# the device route's parts, ms: compile | the C call (3 launches + its wait) | bitmap download | ids copy + download | RowMask   (columns, once per field and corpus)")
        for name in settings:
            v = got[name]
            med = {key: statistics.median(rec[key] for rec in v) for key in v[0] if key.endswith("_ms")}
            say(f"# {name:3s} {med['compile_p50_ms']:6.3f} | {med['call_p50_ms']:6.3f} | {med['bitmap_download_p50_ms']:6.3f} | {med['ids_download_p50_ms']:6.3f} | {med['row_mask_p50_ms']:6.3f}   "
                f"({med['columns_once_ms']:8.1f})")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
