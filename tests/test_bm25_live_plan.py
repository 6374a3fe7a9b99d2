"""The index arithmetic of a live BM25 update (veritasfi_amd/csrc/vf_bm25_live.h), EXECUTED on the CPU: a host-compiled driver
(tests/bm25_live_plan_driver.py, ASan + UBSan) runs the kernels' scheme chunk by chunk.  No GPU.

12 documents over 6 columns: column 0 holds every document, columns 3 and 4 one posting each, column 5 none.  Every subset of removed
rows that leaves a document, combined with adding 0, 1 or 3 documents (one of which brings a new column), at chunk sizes 1, 4 and
larger than nnz.  The driver holds the scheme to its own invariants; here each result is compared with ``bm25_index_arrays`` on the
edited token lists: indptr, indices, tf, and the score BITS (the driver's scores are a scalar float64 loop over the recipe, with idf
from a table numpy's log filled)."""
import struct

import numpy as np
import pytest

import bm25_live_plan_driver as drv
from veritasfi_amd import bm25 as B

N0, V0, K1, Bb = 12, 6, 1.5, 0.75
DOCS = [[0] + ([1] if i % 2 else []) + ([2, 2] if i % 3 == 0 else []) + ([3] if i == 4 else []) + ([4, 0] if i == 9 else []) for i in range(N0)]
ADDS = [[], [[6, 0]], [[0, 1, 1], [6, 0], [5, 2, 2, 2]]]
TABLE_N = 20   # idf[N][df] for N, df < 20


def _csc(docs, vocab):
    off = np.concatenate([[0], np.cumsum([len(t) for t in docs])]).astype(np.int64)
    toks = np.asarray([t for d in docs for t in d], np.int64)
    return B.bm25_index_arrays(off, toks, vocab, K1, Bb, return_tf=True)


def _vl(f, a):
    a = np.asarray(a, np.int64).ravel()
    f.write(struct.pack("<q", a.size))
    f.write(a.tobytes())


@pytest.fixture(scope="module")
def outcome(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bm25_live_plan")
    exe = drv.build(tmp)
    inp, out = str(tmp / "in.bin"), str(tmp / "out.bin")
    indptr, indices, _, tf = _csc(DOCS, V0)
    assert np.diff(indptr).tolist() == [12, 6, 4, 1, 1, 0]
    with open(inp, "wb") as f:
        _vl(f, [N0, V0, TABLE_N, len(ADDS)])
        _vl(f, indptr), _vl(f, indices), _vl(f, tf), _vl(f, [len(d) for d in DOCS])
        for add in ADDS:
            Vn = max([V0] + [t + 1 for d in add for t in d])
            if add:
                dptr, drows, _, dtf = _csc(add, Vn)
            else:
                dptr, drows, dtf = np.zeros(Vn + 1, np.int64), [], []
            _vl(f, [len(add), Vn]), _vl(f, dptr), _vl(f, drows), _vl(f, dtf), _vl(f, [len(d) for d in add])
        N, df = np.meshgrid(np.arange(TABLE_N, dtype=np.float64), np.arange(TABLE_N, dtype=np.float64), indexing="ij")
        f.write(np.ascontiguousarray(np.log(1.0 + (N - df + 0.5) / (df + 0.5))).tobytes())   # bm25_index_arrays' expression
        f.write(np.asarray([K1, Bb], np.float64).tobytes())
    run = drv.run(exe, inp, out)
    return run, np.fromfile(out, dtype=np.int32)


def test_the_scheme_holds_its_own_invariants_at_every_chunk_size(outcome):
    run, _ = outcome
    print(run.stdout[-3000:])
    assert run.returncode == 0 and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, (run.stdout[-3000:], run.stderr[-3000:])
    assert " 0 failure(s)" in run.stdout
    assert f"{(2 ** N0 - 1) * len(ADDS) * 3} cases" in run.stdout


def test_every_result_equals_bm25_index_arrays_on_the_edited_token_lists(outcome):
    _, words = outcome
    pos, seen = 0, 0
    while pos < words.size:
        mask, di, Vn, nnz = (int(x) for x in words[pos:pos + 4])
        pos += 4
        newptr, indices, tf, bits = (words[pos:pos + Vn + 1], words[pos + Vn + 1:pos + Vn + 1 + nnz],
                                     words[pos + Vn + 1 + nnz:pos + Vn + 1 + 2 * nnz], words[pos + Vn + 1 + 2 * nnz:pos + Vn + 1 + 3 * nnz])
        pos += Vn + 1 + 3 * nnz
        docs = [d for i, d in enumerate(DOCS) if not mask >> i & 1] + ADDS[di]
        want_ptr, want_idx, want_data, want_tf = _csc(docs, Vn)
        assert np.array_equal(newptr, want_ptr) and np.array_equal(indices, want_idx) and np.array_equal(tf, want_tf), (mask, di)
        assert np.array_equal(bits.view(np.uint32), want_data.view(np.uint32)), (mask, di)
        seen += 1
    assert seen == (2 ** N0 - 1) * len(ADDS)
