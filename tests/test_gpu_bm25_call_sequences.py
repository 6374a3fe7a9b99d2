"""The ORDER of calls on one BM25 handle (csrc/vf_sparse.hip's host path: which buffers a call makes, keeps, regrows and drops).  The
per-mode tests open a retriever and use one mode; here one live retriever goes through a fixed sequence of every kind of call, and
every step's ids and score BITS must equal the same call on a freshly opened retriever over the same documents.

Index: 70 001 documents (three bitmap blocks of 32 768 rows: the smallest size where a filtered tail counts more than one block and
k = 4097 is legal), 50 columns, 3-token queries.  The filter allows 2000 rows drawn with a fixed seed: at k = 200 the query of the
three rarest columns touches fewer than k of them and ends in the zero-score tail, at k = 4097 every filtered result ends in padding.

  1  unfiltered, nq = 1                         8  filtered at k = 4097 (the deep-k scratch with a filter)
  2  filtered, nq = 3 (the slots regrow)        9  unfiltered at k = 4097
  3  filtered, nq = 5 (they regrow while       10  an update: 3 rows leave, 1 arrives (n changes: all per-n scratch is dropped)
     the filter's buffers exist)               11  filtered, nq = 3 again
  4  subset statistics, stage + search         12  the old prepared objects are refused as stale
  5  ... the search after ANOTHER bitmap       13  a new prepared subset searches
     was staged (it must upload its own)
  6  prepared, corpus statistics
  7  prepared, subset statistics"""
import numpy as np
import pytest

import veritasfi_amd as vf
from veritasfi_amd import _ffi
from veritasfi_amd import bm25 as B
from test_bm25_prepared_plan import _zipf

pytestmark = pytest.mark.gpu

N, VOCAB, K, DEEP_K, ALLOWED = 70001, 50, 200, 4097, 2000
GONE, ARRIVES = [5, 40000, 70000], np.array([0, 7, 49], np.int64)
U32P = _ffi.ctypes.POINTER(_ffi.ctypes.c_uint32)
F64P = _ffi.ctypes.POINTER(_ffi.ctypes.c_double)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The index directory before the update and the one a rebuild gives after it, the queries, and the two filters."""
    off, toks = _zipf(N, VOCAB, 4, seed=21)
    before, after = str(tmp_path_factory.mktemp("bm25_sequence_before")), str(tmp_path_factory.mktemp("bm25_sequence_after"))
    B.build_bm25_index_from_ids(off, toks, VOCAB, before)
    keep = np.setdiff1d(np.arange(N), GONE)
    docs = [toks[off[r]:off[r + 1]] for r in keep] + [ARRIVES]
    off2 = np.zeros(len(docs) + 1, np.int64)
    np.cumsum([d.size for d in docs], out=off2[1:])
    B.build_bm25_index_from_ids(off2, np.concatenate(docs), VOCAB, after)
    by_count = np.argsort(np.bincount(toks, minlength=VOCAB), kind="stable").astype(np.int32)   # rarest column first
    rare, common = by_count[:3], by_count[-3:]
    queries = [rare, common, by_count[[0, 25, 49]], np.array([rare[0], rare[0], common[2]], np.int32), by_count[[10, 20, 30]]]
    rng = np.random.default_rng(2000)
    return {"before": before, "after": after, "queries": queries, "rows": np.sort(rng.choice(N, ALLOWED, replace=False)),
            "other_rows": np.sort(rng.choice(N, 300, replace=False)), "rows_after": np.sort(rng.choice(N - 2, ALLOWED, replace=False))}


def _open(d):
    return vf.BM25Retriever(d, stemmer=None, load_corpus=False, live=True)


def _search_after_another_stage(r, rows, other_rows, queries, k):
    """Stage ``rows`` (their counts), stage ``other_rows`` (its bitmap is now the one the device holds), then the search of ``rows``."""
    _, offsets, terms = r._columns_args(queries)
    nq = len(queries)
    ids, scores = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
    with r._update_mu, r._mu:
        words, _ = B.filter_words(rows, r.num_docs)
        sq = _ffi.Bm25SubstatsQuery(offsets.ctypes.data_as(_ffi.p_i64), words.ctypes.data_as(U32P), r.num_docs)
        df = r._substats_stage(sq, terms, nq)
        other, _ = B.filter_words(other_rows, r.num_docs)
        r._substats_stage(_ffi.Bm25SubstatsQuery(offsets.ctypes.data_as(_ffi.p_i64), other.ctypes.data_as(U32P), r.num_docs), terms, nq)
        idf, sq.avgdl = r._subset_idf_avgdl(int(sq.m), df, sq.total_len)
        sq.idf, sq.k1, sq.b, sq.phase = idf.ctypes.data_as(F64P), r._k1, r._b, _ffi.VF_BM25_SUBSTATS_SEARCH
        _ffi.check(r._search(sq, terms, nq | _ffi.VF_BM25_FILTER | _ffi.VF_BM25_SUBSTATS, k, ids, scores), "vf_bm25_search")
    return ids, scores


def _prepared(r, rows, stats, queries, k, keep=None):
    """A search through a filter prepared for it; ``keep``: a list the filter is left open in (else it is closed)."""
    s = r.prepare_subset(rows, stats)
    try:
        return r.search_columns(queries, k, subset=s)
    finally:
        keep.append(s) if keep is not None else s.close()


def test_every_kind_of_call_in_sequence_on_one_handle_equals_a_fresh_handle_bit_for_bit(world):
    q, rows = world["queries"], world["rows"]
    kept = []   # the sequence's prepared filters stay open: they must go stale with the update
    steps = [
        ("1 unfiltered nq=1", "before", lambda r, own: r.search_columns(q[:1], K)),
        ("2 filtered nq=3", "before", lambda r, own: r.search_columns(q[:3], K, subset=rows)),
        ("3 filtered nq=5", "before", lambda r, own: r.search_columns(q, K, subset=rows)),
        ("4 subset statistics", "before", lambda r, own: r.search_columns(q[:3], K, subset=rows, stats="subset")),
        ("5 subset statistics after another stage", "before",
         lambda r, own: _search_after_another_stage(r, rows, world["other_rows"], q[:3], K) if own else r.search_columns(q[:3], K, subset=rows, stats="subset")),
        ("6 prepared corpus", "before", lambda r, own: _prepared(r, rows, "corpus", q[:3], K, kept if own else None)),
        ("7 prepared subset", "before", lambda r, own: _prepared(r, rows, "subset", q[:3], K, kept if own else None)),
        ("8 filtered k=4097", "before", lambda r, own: r.search_columns(q[:2], DEEP_K, subset=rows)),
        ("9 unfiltered k=4097", "before", lambda r, own: r.search_columns(q[:2], DEEP_K)),
        ("11 filtered nq=3 after the update", "after", lambda r, own: r.search_columns(q[:3], K, subset=world["rows_after"])),
        ("13 prepared subset after the update", "after", lambda r, own: _prepared(r, world["rows_after"], "subset", q[:3], K)),
    ]
    got = {}
    with _open(world["before"]) as one:
        for name, which, call in steps:
            if which == "after" and one.num_docs == N:
                # 10: n changes, so the slots, the filter's buffers and the deep-k scratch all go
                assert one.add_token_ids([0, ARRIVES.size], ARRIVES, remove_ids=GONE) == N - 3 and one.num_docs == N - 2
                # 12: rows have moved
                assert len(kept) == 2 and all(s.stale for s in kept)
                for s in kept:
                    with pytest.raises(ValueError, match="stale"):
                        one.search_columns(q[:1], K, subset=s)
            got[name] = call(one, True)
        assert one.info()["prepared"] == 0
    for name, which, call in steps:   # the same call on a retriever that has seen nothing else
        with _open(world[which]) as fresh:
            want = call(fresh, False)
        print(name, "padding" if (want[0] < 0).any() else "", "zero-score tail" if ((want[0] >= 0) & (want[1] == 0)).any() else "")
        assert same(got[name], want), name
    # the shapes are what the docstring says: a zero-score tail at k = 200, padding at k = 4097 under the filter and none without it
    ids, scores = got["2 filtered nq=3"]
    assert (ids[0] >= 0).all() and scores[0, 0] > 0 and scores[0, -1] == 0
    assert (got["8 filtered k=4097"][0][:, ALLOWED - 1] >= 0).all() and (got["8 filtered k=4097"][0][:, ALLOWED:] == -1).all()
    assert (got["9 unfiltered k=4097"][0] >= 0).all()
