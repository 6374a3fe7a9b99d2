"""A prepared filter's df for every column (veritasfi_amd/csrc/vf_bm25_prepared.h), EXECUTED on the CPU: a host-compiled driver
(tests/bm25_prepared_driver.py, UBSan) replays the launch of k_bm25_sub_df_all chunk by chunk and thread by thread -- the flags and
their prefix, the columns a chunk intersects, the owned and the straddling split -- and numpy says what it must return:
df_s[c] = mask[indices[indptr[c]:indptr[c + 1]]].sum() for every column c, every posting flagged exactly once.  No GPU.

A 12-row index under every one of its 4096 filters at chunk sizes 1, 2, 3, 5 and 2048; then 32 768 + 40 rows over 4096 columns (empty
columns, one-posting columns, a column of eight default chunks) at chunk sizes 7 and 2048 under word and block boundaries."""
import numpy as np
import pytest

import bm25_prepared_driver as drv
from veritasfi_amd import bm25 as B


def _zipf(n_docs, vocab, mean_len, seed):      # tests/test_bm25_substats_plan.py's generator
    rng = np.random.default_rng(seed)
    lens = rng.poisson(mean_len, size=n_docs)
    lens[5::7] = 0                                           # empty documents among them
    off = np.zeros(n_docs + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, (rng.zipf(1.25, size=int(off[-1])) - 1) % vocab


def _numpy_df(indptr, indices, n, rows):
    mask = np.zeros(n, bool)
    mask[rows] = True
    return int(mask.sum()), [int(mask[indices[indptr[c]:indptr[c + 1]]].sum()) for c in range(indptr.size - 1)]


def _run(tmp, exe, n, indptr, indices, chunks, filters):
    out = drv.run(exe, drv.write_input(tmp / f"in_{n}.txt", n, indptr, indices, chunks, filters))
    print(out.stdout[-2000:])
    assert out.returncode == 0 and "runtime error" not in out.stderr, (out.stdout[-3000:], out.stderr[-3000:])
    assert "prepared: 0 failure(s)" in out.stdout
    got = drv.parse(out.stdout)
    assert len(got) == len(filters) * len(chunks)
    for i, rows in enumerate(filters):
        want = _numpy_df(indptr, indices, n, np.asarray(rows, np.int64))
        for C in chunks:
            assert got[(C, i)] == want, (C, rows)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("bm25_prepared_plan"))


def test_every_filter_of_a_12_row_index_counts_every_column_as_numpy_does(exe, tmp_path):
    n, vocab = 12, 16
    off, toks = _zipf(n, vocab, 3, seed=3)
    indptr, indices, _ = B.bm25_index_arrays(off, toks, vocab)
    per = np.diff(indptr)
    assert indices.size == 31 and int((per == 0).sum()) == 1 and int((per == 1).sum()) == 6, per   # what the chunk sizes below cut through
    filters = [[r for r in range(n) if (f >> r) & 1] for f in range(1 << n)]
    assert len(filters) == 4096
    _run(tmp_path, exe, n, indptr, indices, [1, 2, 3, 5, 2048], filters)


def test_word_block_and_chunk_boundaries_count_every_column_as_numpy_does(exe, tmp_path):
    n, vocab = 32768 + 40, 4096
    off, toks = _zipf(n, vocab, 4, seed=5)
    indptr, indices, _ = B.bm25_index_arrays(off, toks, vocab)
    per = np.diff(indptr)
    assert int((per == 0).sum()) == 50 and int((per == 1).sum()) == 196 and int(per.max()) == 16336, (int((per == 0).sum()), int((per == 1).sum()), int(per.max()))
    assert (int(per.max()) + 2047) // 2048 == 8, "the longest column takes eight default chunks"
    filters = [[31], [32], [33], [31, 32, 33], [32767], [32768], [32767, 32768], [n - 1], list(range(32768, n)), list(range(0, n, 2)),
               list(range(n)), []]
    _run(tmp_path, exe, n, indptr, indices, [7, 2048], filters)
