#!/usr/bin/env python3
"""What an update of a live BM25 index costs (BM25Retriever(live=True): vf_bm25_create with VF_BM25_LIVE), against the only other
route to the same state -- bm25_index_arrays over all the documents plus vf_bm25_create -- and whether a handle grown by adds
searches like one built at once.

    python tools/bench_bm25_live.py                      # every measurement, written to profiles/r15_bm25_live.log as well
    python tools/bench_bm25_live.py --only update        # update costs only;  --only search: the search comparison only

The driver builds the index directories once (Zipf tokens, Poisson lengths, from a seed) in a temporary directory; every measurement
then runs in a FRESH process (this script calls itself with --child, one `timeout`-bounded child per setting and pass), the settings
alternate, and the driver stops at the first child that fails.  A call's time is a host clock around it: an update returns after a
device synchronise.

  add / remove / update   --calls updates of a live handle over --n documents: --m documents added, --m scattered documents removed, or
             both in one pass; p50 / min / max per call, and the p50 of its parts (stage: upload, row map, count, scan, counts back to
             the host; host: numpy's log over the vocabulary, the mean length; commit: the rewrite).  Beside it, in the same process:
             a plain device-to-device copy of the posting arrays (12 B per posting: the floor of any rewrite), and -- first pass only --
             the rebuild route, once.
  search     64 queries of tools/bench_bm25.py's shape, k = 100: a handle grown from --search-n0 documents by adds of --search-m against
             one built at once; --rounds windows each, alternating; p50 per batch of --reps."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def prepare(args, tmp, say):
    from veritasfi_amd import bm25 as B
    rng = np.random.default_rng(args.seed)
    t0 = time.perf_counter()
    n = args.n + (args.calls + 2) * args.m
    lens = rng.poisson(args.doc_len, size=n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    toks = ((rng.zipf(1.25, size=int(off[-1])) - 1) % args.vocab).astype(np.int32)
    np.save(os.path.join(tmp, "off.npy"), off)
    np.save(os.path.join(tmp, "toks.npy"), toks)
    for name, docs in (("full", args.n), ("part", args.search_n0)):
        B.build_bm25_index_from_ids(off[:docs + 1], toks[:off[docs]], args.vocab, os.path.join(tmp, name))
    say(f"# index directories: {args.n} and {args.search_n0} documents, vocab {args.vocab}, mean length {args.doc_len}, "
        f"{int(off[args.n])} tokens, built in {time.perf_counter() - t0:.1f} s")


def child_update(args, tmp):
    import torch
    import veritasfi_amd as vf
    from veritasfi_amd import _ffi
    from veritasfi_amd import bm25 as B
    off, toks = np.load(os.path.join(tmp, "off.npy")), np.load(os.path.join(tmp, "toks.npy"), mmap_mode="r")
    rng = np.random.default_rng(args.seed + 1)
    t0 = time.perf_counter()
    r = vf.BM25Retriever(os.path.join(tmp, "full"), stemmer=None, load_corpus=False, live=True)
    rec = {"setting": args.setting, "n": args.n, "m": args.m, "vocab": r.info()["vocab"], "nnz": r.info()["nnz"],
           "open_live_s": round(time.perf_counter() - t0, 2)}
    t, parts = [], []
    for i in range(args.calls + 2):
        lo, hi = args.n + i * args.m, args.n + (i + 1) * args.m
        add_off, add_tok = off[lo:hi + 1] - off[lo], np.asarray(toks[off[lo]:off[hi]], np.int64)
        gone = rng.choice(r.num_docs, size=args.m, replace=False)
        a = time.perf_counter()
        if args.setting == "add":
            r.add_token_ids(add_off, add_tok)
        elif args.setting == "remove":
            r.remove(gone)
        else:
            r.add_token_ids(add_off, add_tok, remove_ids=gone)
        t.append(1e3 * (time.perf_counter() - a))
        parts.append(dict(r.last_update_ms))
    t, parts = t[2:], parts[2:]                                     # the first calls load the kernels' code
    rec.update({"calls": len(t), "p50_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)})
    rec.update({f"{k}_p50_ms": round(statistics.median(p[k] for p in parts), 3) for k in ("stage", "host", "commit")})
    V, n = r.info()["vocab"], r.num_docs
    df = r._df.astype(np.float64)
    a = time.perf_counter()
    for _ in range(10):
        np.log(1.0 + (n - df + 0.5) / (df + 0.5))
    rec["numpy_log_over_vocab_ms"] = round(1e2 * (time.perf_counter() - a), 3)
    nnz = r.info()["nnz"]
    r.search_columns([np.array([0, 5, 40], np.int32)], 100)          # the handle still serves
    src, dst = torch.empty(3 * nnz, dtype=torch.int32, device="cuda"), torch.empty(3 * nnz, dtype=torch.int32, device="cuda")
    src.zero_()
    c = []
    for _ in range(12):
        torch.cuda.synchronize()
        a = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        c.append(1e3 * (time.perf_counter() - a))
    rec["d2d_copy_12B_per_posting_p50_ms"] = round(statistics.median(c[2:]), 3)
    del src, dst
    r.close()
    if args.rebuild:                                                 # the parent commit's route to the same state, once
        a = time.perf_counter()
        indptr, indices, data = B.bm25_index_arrays(off[:args.n + args.m + 1], np.asarray(toks[:off[args.n + args.m]]), V)
        b = time.perf_counter()
        h, slots = _ffi.vp(), _ffi.c_i32()
        _ffi.check(_ffi.lib().vf_bm25_create(indptr.ctypes.data_as(_ffi.p_i64), V, indices.ctypes.data_as(_ffi.p_i32), data.ctypes.data_as(_ffi.p_f32),
                                             int(data.size), args.n + args.m, 0, _ffi.ctypes.byref(h), _ffi.ctypes.byref(slots)), "vf_bm25_create")
        rec["rebuild_index_arrays_s"], rec["rebuild_create_s"] = round(b - a, 2), round(time.perf_counter() - b, 2)
        _ffi.lib().vf_bm25_create(None, 0, None, None, 0, 0, 0, _ffi.ctypes.byref(h), None)
    print(json.dumps(rec), flush=True)


def child_search(args, tmp):
    import veritasfi_amd as vf
    off, toks = np.load(os.path.join(tmp, "off.npy")), np.load(os.path.join(tmp, "toks.npy"), mmap_mode="r")
    if args.setting == "search_grown":
        r = vf.BM25Retriever(os.path.join(tmp, "part"), stemmer=None, load_corpus=False, live=True)
        for lo in range(args.search_n0, args.n, args.search_m):
            hi = min(args.n, lo + args.search_m)
            r.add_token_ids(off[lo:hi + 1] - off[lo], np.asarray(toks[off[lo]:off[hi]], np.int64))
    else:
        r = vf.BM25Retriever(os.path.join(tmp, "full"), stemmer=None, load_corpus=False, live=True)
    assert r.num_docs == args.n
    rng = np.random.default_rng(args.seed + 2)
    queries = [((rng.zipf(1.25, size=10) - 1) % args.vocab).astype(np.int32) for _ in range(64)]
    ids, _ = r.search_columns(queries, 100)
    t = []
    for _ in range(args.reps):
        a = time.perf_counter()
        ids, _ = r.search_columns(queries, 100)
        t.append(1e3 * (time.perf_counter() - a))
    print(json.dumps({"setting": args.setting, "n": args.n, "nnz": r.info()["nnz"], "nq": 64, "k": 100, "p50_ms_per_batch": round(statistics.median(t), 3),
                      "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "checksum_ids": int(ids.sum())}), flush=True)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000, help="documents in the index before the updates")
    ap.add_argument("--vocab", type=int, default=200_000)
    ap.add_argument("--doc-len", type=float, default=150.0)
    ap.add_argument("--m", type=int, default=100, help="documents added and / or removed per update")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--search-n0", type=int, default=900_000)
    ap.add_argument("--search-m", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--timeout", type=int, default=400, help="seconds a child may take")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--only", choices=["update", "search"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_bm25_live.log"))
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    ap.add_argument("--setting", default="", help=argparse.SUPPRESS)
    ap.add_argument("--rebuild", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        (child_search if args.setting.startswith("search") else child_update)(args, args.child)
        return 0
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(args.out, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    with tempfile.TemporaryDirectory() as tmp:
        def run(setting, rebuild=False):
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", tmp, "--setting", setting]
            for name in ("n", "vocab", "doc_len", "m", "calls", "search_n0", "search_m", "reps", "seed"):
                cmd += ["--" + name.replace("_", "-"), str(getattr(args, name))]
            proc = subprocess.run(cmd + (["--rebuild"] if rebuild else []), capture_output=True, text=True)
            if proc.returncode != 0:
                say(f"# {setting}: child ended with status {proc.returncode}; stopping\n{proc.stderr[-2000:]}")
                return None
            rec = None
            for line in proc.stdout.splitlines():
                if line.startswith("{"):
                    say(line)
                    rec = json.loads(line)
            return rec

        say("# " + " ".join(sys.argv))
        prepare(args, tmp, say)
        if args.only in (None, "update"):
            recs = {}
            for p in range(args.passes):
                for setting in (("add", "remove", "update") if p % 2 == 0 else ("update", "remove", "add")):
                    rec = run(setting, rebuild=p == 0)
                    if rec is None:
                        return 1
                    recs.setdefault(setting, []).append(rec)
            for setting, rs in recs.items():
                v = [r["p50_ms"] for r in rs]
                first = rs[0]
                say(f"# {setting:6s} n={args.n} m={args.m}: p50 per call {min(v):.3f} .. {max(v):.3f} ms over {len(v)} processes "
                    f"(stage {first['stage_p50_ms']} + host {first['host_p50_ms']} + commit {first['commit_p50_ms']} ms; numpy log over the vocabulary "
                    f"{first['numpy_log_over_vocab_ms']} ms); device-to-device copy of the postings {first['d2d_copy_12B_per_posting_p50_ms']} ms; "
                    f"rebuild route {first['rebuild_index_arrays_s']} s of bm25_index_arrays + {first['rebuild_create_s']} s of vf_bm25_create")
        if args.only in (None, "search"):
            t = {"search_grown": [], "search_built": []}
            for rnd in range(args.rounds):
                for setting in (("search_grown", "search_built") if rnd % 2 == 0 else ("search_built", "search_grown")):
                    rec = run(setting)
                    if rec is None:
                        return 1
                    t[setting].append(rec)
            for setting, rs in t.items():
                v = [r["p50_ms_per_batch"] for r in rs]
                say(f"# {setting:13s} n={args.n} nq=64 k=100: median {statistics.median(v):.3f} ms/batch (min {min(v):.3f} max {max(v):.3f}), "
                    f"ids checksum {rs[-1]['checksum_ids']}")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
