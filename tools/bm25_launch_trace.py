#!/usr/bin/env python3
"""The kernels one call of every kind of vf_bm25_search launches, for comparing two builds of the library (a host-path refactor must
leave the ordered list of launches as it was).  A tool, not a test.

    rocprofv3 --kernel-trace --output-format csv -d OUT_A -- python tools/bm25_launch_trace.py     # VF_LIB_PATH=<build A>
    rocprofv3 --kernel-trace --output-format csv -d OUT_B -- python tools/bm25_launch_trace.py     # VF_LIB_PATH=<build B>
    python tools/bm25_launch_trace.py --compare OUT_A OUT_B [--log profiles/<name>.log]

The run (no argument) opens ONE live retriever over an index of the shape tests/test_gpu_bm25_call_sequences.py uses (its own tokens:
70 001 documents, 50 columns, 3-token queries, 2000 rows allowed) and makes each call once: unfiltered, filtered, the subset-statistics stage and search, a prepare,
arm, search and release in both modes, the filtered and the unfiltered call at k = 4097, and an update.  Trace it alone, without
counters.  --compare reads the *_kernel_trace.csv under each directory, orders the dispatches, and holds the two lists of (kernel
name, grid, workgroup size) to each other; it prints the first difference, or the number of launches that agree."""
import argparse
import csv
import glob
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import numpy as np
    import veritasfi_amd as vf
    from veritasfi_amd import bm25 as B
    n, vocab, k, deep_k = 70001, 50, 200, 4097
    rng = np.random.default_rng(21)
    lens = rng.poisson(4, size=n)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    toks = (rng.zipf(1.25, size=int(off[-1])) - 1) % vocab
    by_count = np.argsort(np.bincount(toks, minlength=vocab), kind="stable").astype(np.int32)
    queries = [by_count[:3], by_count[-3:], by_count[[0, 25, 49]], by_count[[10, 20, 30]], by_count[[5, 15, 45]]]
    rows = np.sort(np.random.default_rng(2000).choice(n, 2000, replace=False))
    with tempfile.TemporaryDirectory() as d:
        B.build_bm25_index_from_ids(off, toks, vocab, d)
        with vf.BM25Retriever(d, stemmer=None, load_corpus=False, live=True) as r:
            r.search_columns(queries[:1], k)
            r.search_columns(queries[:3], k, subset=rows)
            r.search_columns(queries, k, subset=rows)
            r.search_columns(queries[:3], k, subset=rows, stats="subset")
            for stats in ("corpus", "subset"):
                with r.prepare_subset(rows, stats) as s:
                    r.search_columns(queries[:3], k, subset=s)
            r.search_columns(queries[:2], deep_k, subset=rows)
            r.search_columns(queries[:2], deep_k)
            r.add_token_ids([0, 3], np.array([0, 7, 49]), remove_ids=[5, 40000, 70000])
            r.search_columns(queries[:3], k, subset=rows[rows < r.num_docs])
    print(f"bm25_launch_trace: every kind of call made once on {os.environ.get('VF_LIB_PATH', 'the tree-built library')}")
    return 0


def launches(directory):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(paths) == 1, f"{directory}: expected one *kernel_trace.csv, found {paths}"
    with open(paths[0], newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    return [(r["Kernel_Name"], tuple(int(r[f"Grid_Size_{a}"]) for a in "XYZ"), tuple(int(r[f"Workgroup_Size_{a}"]) for a in "XYZ")) for r in rows]


def compare(a_dir, b_dir, log):
    a, b = launches(a_dir), launches(b_dir)
    lines = [f"# tools/bm25_launch_trace.py --compare: {len(a)} launches under {a_dir}, {len(b)} under {b_dir}"]
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    if first is None:
        names = sorted({x[0] for x in a})
        lines.append(f"identical: the same {len(a)} (kernel name, grid, workgroup size) in the same order; {len(names)} distinct kernels")
        lines += [f"#   {sum(1 for x in a if x[0] == name):5d} x {name}" for name in names]
    else:
        lines.append(f"DIFFERENT at launch {first}: {a[first] if first < len(a) else None} against {b[first] if first < len(b) else None}")
    print("\n".join(lines))
    if log:
        with open(log, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if first is None else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("DIR_A", "DIR_B"))
    ap.add_argument("--log", default="", help="append the comparison's outcome to this file")
    args = ap.parse_args()
    sys.exit(compare(args.compare[0], args.compare[1], args.log) if args.compare else run())
