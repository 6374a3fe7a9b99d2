"""The host side of the dense search with a row list per query (VF_SEARCH_SUBSETS), without a GPU: the two C entry points answer bad
arguments with codes before the handle is touched, the stats struct keeps its 128 bytes and gains ``subset_tiles`` where a reserved
word was, and ``subsets_plan`` -- the pure routing function behind ``DenseIndex.search(subsets=)`` -- sends each entry where it belongs."""
import ctypes

import numpy as np
import pytest


def test_entry_points_return_codes_before_the_handle_is_touched():
    from veritasfi_amd import _ffi
    L = _ffi.lib()
    q = np.zeros((1, 8), np.float32)
    ids = np.zeros(1, np.int64)
    out_i, out_s = np.zeros((1, 1), np.int64), np.zeros((1, 1), np.float32)
    host = lambda h, *a: _ffi.search_subsets(L, h, *a)                    # noqa: E731
    device = lambda h, *a: _ffi.search_subsets_device(L, h, *a, None)     # noqa: E731
    fake = 0x1000   # a handle that is not one must not matter: every check below comes before it is read
    for fn in (host, device):
        args = (q.ctypes.data, 1, 1, [ids.ctypes.data], [1], [0], out_i.ctypes.data, out_s.ctypes.data)
        assert fn(None, *args) == -1 and "null handle" in _ffi.last_error()
        assert fn(fake, None, 1, 1, [ids.ctypes.data], [1], [0], out_i.ctypes.data, out_s.ctypes.data) == -1 and "null buffer" in _ffi.last_error()
        assert fn(fake, q.ctypes.data, 1, 1, [ids.ctypes.data], [1], [0], None, out_s.ctypes.data) == -1 and "null buffer" in _ffi.last_error()
        assert fn(fake, q.ctypes.data, 1, 1, [ids.ctypes.data], [1], [0], out_i.ctypes.data, None) == -1 and "null buffer" in _ffi.last_error()
        assert fn(fake, q.ctypes.data, 1, -1, [ids.ctypes.data], [1], [0], out_i.ctypes.data, out_s.ctypes.data) == -1 and "negative" in _ffi.last_error()
    both = _ffi.VF_SEARCH_SUBSET | _ffi.VF_SEARCH_SUBSETS
    assert L.vf_index_search(fake, None, 1 | _ffi.VF_SEARCH_SUBSETS, 1, out_i.ctypes.data, out_s.ctypes.data) == -1 and "null vf_subsets_query" in _ffi.last_error()
    assert L.vf_index_search_device(fake, None, 1 | _ffi.VF_SEARCH_SUBSETS, 1, out_i.ctypes.data, out_s.ctypes.data, None) == -1 and "null vf_subsets_query" in _ffi.last_error()
    sq, keep = _ffi._subsets_query(q.ctypes.data, [ids.ctypes.data], [1], [0])
    assert L.vf_index_search(fake, ctypes.addressof(sq), 1 | both, 1, out_i.ctypes.data, out_s.ctypes.data) == -1 and "together" in _ffi.last_error()
    assert L.vf_index_search_device(fake, ctypes.addressof(sq), 1 | both, 1, out_i.ctypes.data, out_s.ctypes.data, None) == -1 and "together" in _ffi.last_error()
    # a null list table, and a negative list count
    null_tab = _ffi.SubsetsQuery(q.ctypes.data, None, None, 1, None)
    assert L.vf_index_search(fake, ctypes.addressof(null_tab), 1 | _ffi.VF_SEARCH_SUBSETS, 1, out_i.ctypes.data, out_s.ctypes.data) == -1 and "null list table" in _ffi.last_error()
    sq.n_lists = -1
    assert L.vf_index_search(fake, ctypes.addressof(sq), 1 | _ffi.VF_SEARCH_SUBSETS, 1, out_i.ctypes.data, out_s.ctypes.data) == -1 and "negative" in _ffi.last_error()
    assert L.vf_version() == 100
    del keep


def test_stats_struct_keeps_its_size_and_gains_subset_tiles():
    from veritasfi_amd import _ffi
    assert ctypes.sizeof(_ffi.SearchStats) == 128
    assert _ffi.SearchStats.subset_rows.offset == 104
    assert _ffi.SearchStats.subset_tiles.offset == 112
    d = _ffi.SearchStats().as_dict()
    assert "subset_tiles" in d and "subset_rows" in d and "reserved" not in d
    assert ctypes.sizeof(_ffi.SubsetsQuery) == 40 and _ffi.SubsetsQuery.list_of.offset == 32 and _ffi.SubsetsQuery.n_lists.offset == 24


def _row_subset(ids, device_id):
    from veritasfi_amd.index import RowSubset
    rs = RowSubset.__new__(RowSubset)          # no device: the plan reads ids and device_id alone
    rs.ids, rs.device_id, rs.tensor = np.asarray(ids, np.int64), device_id, None
    return rs


def test_subsets_plan_routes_a_mixed_list():
    from veritasfi_amd.index import SUBSETS_MAX_IDS, subsets_plan
    n = 40000
    short = np.array([9, 3, 5, 3], np.int64)                    # unsorted, repeating: made ascending and distinct
    mask = np.zeros(n, bool)
    mask[[1, 7, 30000]] = True
    long = np.arange(0, 2 * (SUBSETS_MAX_IDS + 1), 2)           # 16 385 ids: one too many for the list-per-query call
    edge = np.arange(SUBSETS_MAX_IDS)                           # 16 384: still inside
    twin = short.copy()                                         # equal content, another object: its own list
    subsets = [short, None, long, mask, short, edge, None, long, twin]
    plan = subsets_plan(subsets, len(subsets), n)
    assert plan["plain"] == [1, 6]
    assert len(plan["long"]) == 1 and plan["long"][0]["queries"] == [2, 7] and np.array_equal(plan["long"][0]["subset"], long)
    m = plan["multi"]
    assert m["form"] == "host" and m["queries"] == [0, 3, 4, 5, 8] and m["list_of"] == [0, 1, 0, 2, 3] and m["first_query"] == [0, 3, 5, 8]
    assert [x.tolist() for x in m["lists"][:2]] == [[3, 5, 9], [1, 7, 30000]] and np.array_equal(m["lists"][2], edge) and m["lists"][3].tolist() == [3, 5, 9]
    assert all(x.dtype == np.int64 and x.flags.c_contiguous for x in m["lists"])
    # id_offset: masks and ranges follow it
    off = subsets_plan([mask, None], 2, n, id_offset=1000)
    assert off["multi"]["lists"][0].tolist() == [1001, 1007, 31000]
    # the device form: every short entry is a RowSubset on the index's device
    a, b, far, big = _row_subset([1, 2, 3], 0), _row_subset([], 0), _row_subset([4], 1), _row_subset(np.arange(SUBSETS_MAX_IDS + 5), 0)
    dev = subsets_plan([a, b, None, a, big], 5, n, device_id=0)
    assert dev["multi"]["form"] == "device" and dev["multi"]["lists"] == [a, b] and dev["multi"]["list_of"] == [0, 1, 0] and dev["multi"]["queries"] == [0, 1, 3]
    assert dev["plain"] == [2] and dev["long"][0]["subset"] is big and dev["long"][0]["queries"] == [4]
    # one array among them, a RowSubset of another device, or no device at all: the host form, from the RowSubsets' host copies
    for entries, device_id in (([a, short], 0), ([a, far], 0), ([a, b], None)):
        host = subsets_plan(entries, 2, n, device_id=device_id)["multi"]
        assert host["form"] == "host" and all(isinstance(x, np.ndarray) for x in host["lists"])
    assert subsets_plan([a, short], 2, n, device_id=0)["multi"]["lists"][0] is a.ids
    # nothing to do in a mode leaves it out
    assert subsets_plan([None, None], 2, n) == {"plain": [0, 1], "long": [], "multi": None}
    assert subsets_plan([], 0, n) == {"plain": [], "long": [], "multi": None}


def test_subsets_plan_refusals():
    from veritasfi_amd.index import subsets_plan
    with pytest.raises(ValueError, match=r"3 entries for 2 queries"):
        subsets_plan([None, None, None], 2, 10)
    with pytest.raises(ValueError, match="cannot be given together"):
        subsets_plan([None, None], 2, 10, subset=[1, 2])
    with pytest.raises(TypeError, match="integers or a boolean mask"):
        subsets_plan([[1.5, 2.5], None], 2, 10)
    with pytest.raises(TypeError):
        subsets_plan(["rows"], 1, 10)
    with pytest.raises(ValueError, match=r"outside the index's ids \[0, 10\)"):
        subsets_plan([None, [3, 10]], 2, 10)
    with pytest.raises(ValueError, match="one entry per row"):
        subsets_plan([np.ones(9, bool)], 1, 10)


def test_library_messages_name_the_callers_entry():
    from veritasfi_amd.index import _name_subsets
    msg = "vf_index_search (VF_SEARCH_SUBSETS): lists[1]: ids[4] = 7 is a duplicate of ids[3] (the list must be strictly ascending)"
    assert _name_subsets(msg, [0, 5]) == msg.replace("lists[1]", "subsets[5]")
    assert _name_subsets("lists[9] holds", [0, 5]) == "lists[9] holds"


def test_the_retrievers_declare_and_pass_the_per_query_form():
    from veritasfi_amd.faiss_retriever import FaissRetriever

    class Ix:
        def search(self, q, k, subset=None, subsets=None):
            self.seen = (q.shape, k, subset, subsets)
            return "ids", "scores"

    class E:
        def embed_query(self, t):
            return [1.0, 0.0]

    assert FaissRetriever.per_query_subsets is True
    r = FaissRetriever.from_index(Ix(), E())
    subs = [None, [1, 2]]
    assert r.invoke(["a", "b"], 3, subsets=subs) == ("ids", "scores") and r.index.seen[0] == (2, 2) and r.index.seen[3] is subs and r.index.seen[2] is None
