"""The host side of the subset search, without a GPU: the two C entry points answer bad arguments with codes (no HIP call is reached
with a null handle or null buffers), the Python layer turns lists and masks into the strictly ascending id array the library takes,
and ``EnsembleRetriever.rows_where`` equals a brute-force scan of the metadata."""
import numpy as np
import pytest


def test_entry_points_return_codes_for_null_arguments():
    from veritasfi_amd import _ffi
    L = _ffi.lib()
    q = np.zeros((1, 8), np.float32)
    ids = np.zeros(1, np.int64)
    out_i, out_s = np.zeros((1, 1), np.int64), np.zeros((1, 1), np.float32)
    rc = _ffi.search_subset(L, None, q.ctypes.data, 1, 1, ids.ctypes.data, 1, out_i.ctypes.data, out_s.ctypes.data)
    assert rc == -1 and "null handle" in _ffi.last_error()
    rc = _ffi.search_subset_device(L, None, q.ctypes.data, 1, 1, ids.ctypes.data, 1, out_i.ctypes.data, out_s.ctypes.data, None)
    assert rc == -1 and "null handle" in _ffi.last_error()
    # the remaining argument checks come before the handle is touched: a handle that is not one must not matter
    fake = 0x1000
    assert L.vf_index_search(fake, None, 1 | _ffi.VF_SEARCH_SUBSET, 1, out_i.ctypes.data, out_s.ctypes.data) == -1 and "null vf_subset_query" in _ffi.last_error()
    assert L.vf_index_search_device(fake, None, 1 | _ffi.VF_SEARCH_SUBSET, 1, out_i.ctypes.data, out_s.ctypes.data, None) == -1 and "null vf_subset_query" in _ffi.last_error()
    host = lambda *a: _ffi.search_subset(L, *a)                    # noqa: E731
    device = lambda *a: _ffi.search_subset_device(L, *a)           # noqa: E731
    for fn, tail in ((host, ()), (device, (None,))):
        assert fn(fake, None, 1, 1, ids.ctypes.data, 1, out_i.ctypes.data, out_s.ctypes.data, *tail) == -1 and "null buffer" in _ffi.last_error()
        assert fn(fake, q.ctypes.data, 1, 1, ids.ctypes.data, 1, None, out_s.ctypes.data, *tail) == -1 and "null buffer" in _ffi.last_error()
        assert fn(fake, q.ctypes.data, 1, 1, ids.ctypes.data, 1, out_i.ctypes.data, None, *tail) == -1 and "null buffer" in _ffi.last_error()
        assert fn(fake, q.ctypes.data, 1, 1, None, 1, out_i.ctypes.data, out_s.ctypes.data, *tail) == -1 and "null id list" in _ffi.last_error()
        assert fn(fake, q.ctypes.data, -1, 1, ids.ctypes.data, 1, out_i.ctypes.data, out_s.ctypes.data, *tail) == -1 and "negative" in _ffi.last_error()
        assert fn(fake, q.ctypes.data, 1, 1, ids.ctypes.data, -1, out_i.ctypes.data, out_s.ctypes.data, *tail) == -1 and "negative" in _ffi.last_error()


def test_stats_struct_keeps_its_size_and_names_subset_rows():
    import ctypes
    from veritasfi_amd import _ffi
    assert ctypes.sizeof(_ffi.SearchStats) == 16 * 8
    assert _ffi.SearchStats.subset_rows.offset == 13 * 8
    assert "subset_rows" in _ffi.SearchStats().as_dict()


def test_subset_ids_sorts_and_makes_distinct():
    from veritasfi_amd.index import subset_ids
    asc = np.array([3, 5, 9], dtype=np.int64)
    out = subset_ids(asc, 10)
    assert out.dtype == np.int64 and out.flags.c_contiguous and np.array_equal(out, asc)
    assert np.array_equal(subset_ids([9, 3, 5, 3, 9], 10), asc)
    assert np.array_equal(subset_ids((5, 3, 9), 10), asc)
    assert np.array_equal(subset_ids(np.array([9, 5, 3], dtype=np.int32), 10), asc)
    assert np.array_equal(subset_ids(np.array([103, 105, 109], dtype=np.uint64), 10, id_offset=100), asc + 100)
    assert subset_ids([], 10).size == 0 and subset_ids(np.empty(0, np.float64), 10).dtype == np.int64
    assert np.array_equal(subset_ids(np.arange(10), 10), np.arange(10))
    big = np.arange(0, 2_000_000, 2)
    assert subset_ids(big, 2_000_000) is not None and np.array_equal(subset_ids(big[::-1], 2_000_000), big)


def test_subset_ids_takes_masks():
    from veritasfi_amd.index import subset_ids
    mask = np.zeros(10, bool)
    mask[[0, 4, 9]] = True
    assert np.array_equal(subset_ids(mask, 10), [0, 4, 9])
    assert np.array_equal(subset_ids(mask, 10, id_offset=1000), [1000, 1004, 1009])
    assert np.array_equal(subset_ids(mask.tolist(), 10), [0, 4, 9])
    assert subset_ids(np.zeros(10, bool), 10).size == 0
    with pytest.raises(ValueError, match="one entry per row"):
        subset_ids(np.ones(9, bool), 10)


def test_subset_ids_refuses_what_is_not_a_list_of_rows():
    from veritasfi_amd.index import subset_ids
    with pytest.raises(ValueError, match=r"ids\[2\] = 10 is outside the index's ids \[0, 10\)"):
        subset_ids([1, 2, 10, 11], 10)
    with pytest.raises(ValueError, match=r"ids\[0\] = 99 is outside the index's ids \[100, 110\)"):
        subset_ids([99, 105], 10, id_offset=100)
    with pytest.raises(ValueError, match=r"ids\[1\] = -1"):
        subset_ids([3, -1], 10)
    with pytest.raises(TypeError, match="integers or a boolean mask"):
        subset_ids([1.0, 2.0], 10)
    with pytest.raises(ValueError, match="one-dimensional"):
        subset_ids(np.zeros((2, 2), np.int64), 10)
    with pytest.raises(ValueError, match="does not fit int64"):
        subset_ids(np.array([2 ** 63], dtype=np.uint64), 10)


class _Store:
    def __init__(self, metas, d=4):
        self.metas, self.d = metas, d

    def get(self, ids=None, include=()):
        n = len(self.metas)
        return {"documents": [f"t{i}" for i in range(n)], "metadatas": self.metas, "embeddings": np.ones((n, self.d), np.float32).tolist()}


class _NoRetriever:
    def __init__(self, embeddings, fn):
        self.n = len(embeddings)


def _brute(metas, where):
    rows = []
    for r, md in enumerate(metas):
        ok = True
        for field, want in where.items():
            values = list(want) if isinstance(want, (list, tuple, set, frozenset)) else [want]
            v = md.get(field, None)
            ok = ok and not isinstance(v, (list, dict)) and v in values
        if ok:
            rows.append(r)
    return np.asarray(rows, dtype=np.int64)


def test_rows_where_equals_a_brute_force_scan():
    from veritasfi_amd.ensemble import EnsembleRetriever
    rng = np.random.default_rng(7)
    metas = []
    for i in range(500):
        md = {"doc_id": f"d{i}", "issuer": ["zeekr", "lotus", "nio"][int(rng.integers(3))], "year": int(rng.integers(2019, 2026)),
              "is_table": bool(rng.integers(2))}
        if i % 11 == 0:
            del md["year"]               # a chunk without the field
        if i % 13 == 0:
            md["issuer"] = ["zeekr", "lotus"]   # an unhashable value
        metas.append(md)
    ts = _Store([None, None])
    er = EnsembleRetriever("unused", _Store(metas), ts, 3, None, bm25_k=0, retriever_cls=_NoRetriever)
    wheres = ({"issuer": "zeekr"}, {"year": 2024}, {"year": [2024, 2025]}, {"issuer": ("lotus", "nio"), "year": {2020, 2021}, "is_table": True},
              {"is_table": False}, {"year": None}, {"year": [None, 2019]}, {"issuer": "byd"}, {"no_such_field": 1}, {"no_such_field": None}, {})
    for where in wheres:
        got = er.rows_where(where)
        assert got.dtype == np.int64 and np.array_equal(got, _brute(metas, where)), where
        assert np.array_equal(er.rows_where(where), got)      # served from the dictionaries the first call built
    assert set(er._field_rows) == {"issuer", "year", "is_table", "no_such_field"}
    with pytest.raises(TypeError):
        er.rows_where(["zeekr"])
