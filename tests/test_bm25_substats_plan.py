"""The counts of a BM25 search scored by the subset's own statistics (veritasfi_amd/csrc/vf_bm25_substats.h), EXECUTED on the CPU: a
host-compiled driver (tests/substats_driver.py, UBSan) runs the stage of a VF_BM25_SUBSTATS request the way the entry point and the
kernels do -- the batch's distinct columns, the length sum per bitmap block and thread, the df count over the launch's grid -- and
numpy says what it must return: df_s[c] = the postings of column c whose row is allowed, the sum of the allowed rows' lengths, and
np.unique's inverse as the map from q_terms position to distinct column.  No GPU.

A 12-row index under every one of its 4096 filters; then 32 768 + 40 rows (two bitmap blocks, a column of more postings than one
workgroup takes) under rows 31 / 32 / 33 and 32767 / 32768, one block alone, every other row and all rows."""
import numpy as np
import pytest

import substats_driver as drv
from veritasfi_amd import bm25 as B


def _zipf(n_docs, vocab, mean_len, seed):
    rng = np.random.default_rng(seed)
    lens = rng.poisson(mean_len, size=n_docs)
    lens[5::7] = 0                                           # empty documents among them
    off = np.zeros(n_docs + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, (rng.zipf(1.25, size=int(off[-1])) - 1) % vocab


def _numpy_counts(indptr, indices, dl, q_terms, rows):
    mask = np.zeros(dl.size, bool)
    mask[rows] = True
    df = [int(mask[indices[indptr[c]:indptr[c + 1]]].sum()) for c in q_terms]
    return int(mask.sum()), int(dl[mask].sum()), df


def _run(tmp, exe, n, vocab, off, toks, q_terms, filters):
    indptr, indices, _, tf = B.bm25_index_arrays(off, toks, vocab, return_tf=True)
    dl = np.diff(off)
    assert np.array_equal(np.bincount(indices, weights=tf, minlength=n).astype(np.int64), dl)
    out = drv.run(exe, drv.write_input(tmp / f"in_{n}.txt", n, indptr, indices, dl, q_terms, filters))
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "runtime error" not in out.stderr, (out.stdout[-3000:], out.stderr[-3000:])
    assert "substats: 0 failure(s)" in out.stdout
    distinct, pos2d, got = drv.parse(out.stdout)
    want_distinct, want_pos = np.unique(q_terms, return_inverse=True)
    assert distinct == want_distinct.tolist() and pos2d == want_pos.tolist()
    assert len(got) == len(filters)
    for rows, g in zip(filters, got):
        assert g == _numpy_counts(indptr, indices, dl, q_terms, np.asarray(rows, np.int64)), rows
    return indptr


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("bm25_substats_plan"))


def test_every_filter_of_a_12_row_index_counts_what_numpy_counts(exe, tmp_path):
    n, vocab = 12, 8
    off, toks = _zipf(n, vocab, 3, seed=3)
    assert (np.diff(off) == 0).any(), "an empty document among the twelve"
    q_terms = np.array([3, 0, 3, 0, 5, 7, 1], np.int32)      # a repeat within a query's run, a column two queries share
    filters = [[r for r in range(n) if (f >> r) & 1] for f in range(1 << n)]
    assert len(filters) == 4096
    _run(tmp_path, exe, n, vocab, off, toks, q_terms, filters)


def test_word_and_block_boundaries_count_what_numpy_counts(exe, tmp_path):
    n, vocab = 32768 + 40, 64
    off, toks = _zipf(n, vocab, 4, seed=5)
    q_terms = np.array([0, 63, 0, 17, 1, 62], np.int32)
    filters = [[31], [32], [33], [31, 32, 33], [32767], [32768], [32767, 32768], [n - 1], list(range(32768, n)), list(range(0, n, 2)),
               list(range(n)), []]
    indptr = _run(tmp_path, exe, n, vocab, off, toks, q_terms, filters)
    assert indptr[1] - indptr[0] > drv_postings_per_workgroup(), "column 0 takes more than one workgroup of the df launch"


def drv_postings_per_workgroup() -> int:
    return 256 * 8      # kBm25SubThreads * kBm25SubPostingsPerThread
