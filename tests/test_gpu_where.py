"""A metadata filter evaluated on the GPU (vf_index_search_device with VF_SEARCH_WHERE: k_where_eval, k_where_scan, k_where_ids of
csrc/vf_where.hip; ``DenseIndex.eval_where``; the ensemble's operator ``where``).  Everything is exact: the bitmap words (tail bits
included), m and the ids equal BOTH ``WhereProgram.evaluate_numpy`` and ``where.matches``.

Direct C calls on indexes of d = 8 and id_offset 1000 at n = 1, 63, 64, 65, 1023, 1024, 1025, 2049 (tiles of 1024 and of 64 rows: several
tiles, the prefix) and 70 001 (default tile): all / none / alternating rows, a single passing row at 0, n - 1 and each side of every word
and tile boundary, intervals on int, number and str columns with and without a validity bitmap, set leaves of 1, 2 and 1000 values with
absent members, NOT, a chain 32 deep, 16 columns.  Output buffers are pre-filled, so a word or an id slot the kernels should not have
written shows.  Then the refusals (outputs untouched, the handle still searches), ``DenseIndex.eval_where`` and the real ensemble."""
import zlib

import numpy as np
import pytest

import veritasfi_amd as vf
from veritasfi_amd import _ffi
from veritasfi_amd import where as W
from veritasfi_amd.index import RowSubset

pytestmark = pytest.mark.gpu

ID0 = 1000
FILL_WORD, FILL_ID = 0x5A5A5A5A, -7
COMPANIES = ["acme", "Acme", "zeekr", "lotus", "é-corp", "中石化", "", "b"]


def _metadata(n):
    rng = np.random.default_rng(n)
    serial = rng.integers(0, 2000, size=n).tolist()
    drop = rng.random((4, n))
    out = []
    for r in range(n):
        md = {"i": r, "par": r & 1, "serial": serial[r], "weight": (r * 37 % 101) / 7.0 - 3.0, "date": f"20{18 + r % 8:02d}-{1 + r % 12:02d}-{1 + r % 28:02d}"}
        if drop[0, r] >= 0.1:
            md["page"] = 1 + (r * 7) % 60
        if drop[1, r] >= 0.15:
            md["ratio"] = [0.5, -0.0, 0.0, 3, -7, 2.25, -1e-300, 1e300, float("inf"), (r % 17) / 4.0 - 2][r % 10]
        if drop[2, r] >= 0.05:
            md["company"] = COMPANIES[(r // 3) % len(COMPANIES)]
        if drop[3, r] >= 0.3:
            md["flag"] = r % 5 < 2
        for j in range(16):
            md[f"c{j}"] = (r * (j + 3) + (r >> j)) % 7
        out.append(md)
    return out


def _by_hand(fields, leaves, code, sets, depth, n):
    arr = np.zeros(len(leaves), W.LEAF_DTYPE)
    for i, leaf in enumerate(leaves):
        arr[i] = leaf
    return W.WhereProgram(fields, arr, code, np.asarray(sets, np.int64), depth, n)


def _programs(n, columns, few=False):
    """[(name, WhereProgram, the filter `matches` is asked)]"""
    wide = {"$or": [{f"c{j}": {"$gte": 5}, f"c{j + 1}": {"$ne": 0}} for j in range(0, 16, 2)]}
    chain = {"serial": {"$lt": 40}}
    for j in range(31):
        chain = {("$or", "$and")[j & 1]: [{"serial": {"$gte": 60 * j, "$lt": 60 * j + 25 + j}}, chain]}
    wheres = [
        ("all", {"i": {"$gte": 0}}), ("none", {"i": {"$lt": 0}}), ("alternating", {"par": 1}),
        ("int, validity", {"page": {"$gte": 10, "$lte": 40}}), ("set of 1000", {"serial": {"$in": list(range(0, 4000, 4))}}),
        ("16 columns", wide),
    ]
    if not few:
        wheres += [
            ("depth 32", chain),
            ("int, no validity", {"serial": {"$gt": 500.5, "$lt": 1500}}), ("number, validity", {"ratio": {"$gt": -0.0, "$lte": 3}}),
            ("number, no validity", {"weight": {"$gte": -1.25, "$lt": 7.5}}), ("str, validity", {"company": {"$gt": "Acme", "$lte": "lotus"}}),
            ("str, no validity", {"date": {"$lte": "2021-06-15"}}), ("not", {"page": {"$ne": 8}}), ("not in", {"company": {"$nin": ["acme", "b", "nobody", "", "zz", None]}}),
            ("missing", {"flag": {"$eq": None}}), ("bool", {"flag": True, "par": 0}), ("four intervals", {"page": {"$in": [1, 8, 15, 99]}}),
            ("none or missing", {"ratio": {"$in": [None, 2.25, 1e300, 9.75, float("inf"), -7, 12]}}),
            ("nested", {"$and": [{"$or": [{"company": "zeekr"}, {"date": {"$gt": "2023"}}]}, {"$or": [{"page": {"$lt": 30}}, {"flag": {"$ne": True}}]}]}),
        ]
    out = [(name, W.compile_where(w, columns, n=n), w) for name, w in wheres]
    deep = dict((name, p) for name, p, _ in out)
    assert few or deep["depth 32"].depth == 32
    assert len(deep["16 columns"].fields) == 16 and deep["set of 1000"].set_values.size == 1000 and deep["int, validity"].n == n
    if not few:   # set leaves of 1 and 2 values (compile_where turns such lists into intervals): by hand, against the $in they mean
        out.append(("set of 1", _by_hand(["serial"], [(W.LEAF_SET, 0, 0, 1)], [0], [7], 1, n), {"serial": {"$in": [7]}}))
        out.append(("set of 2", _by_hand(["page", "serial"], [(W.LEAF_SET, 0, 1, 2), (W.LEAF_SET, 1, 0, 1)], [0, 1, -2], [3, 8, 1000], 2, n),
                    {"$or": [{"page": {"$in": [8, 1000]}}, {"serial": {"$in": [3]}}]}))
    return out


class _Columns(dict):
    """field -> WhereColumn, built on first use"""

    def __init__(self, metas):
        super().__init__()
        self.metas = metas

    def __missing__(self, field):
        self[field] = W.build_column([md.get(field) for md in self.metas], field)
        return self[field]


class World:
    def __init__(self, n):
        import torch
        self.n, self.torch = n, torch
        self.dev = torch.device("cuda:0")
        rows = np.random.default_rng(n + 1).standard_normal((n, 8)).astype(np.float32)
        self.rows = rows
        self.ix = vf.DenseIndex(rows, device_id=0, id_offset=ID0)
        self.metas = _metadata(n)
        self.columns = _Columns(self.metas)
        self.device_columns = {}
        self.words = torch.empty(2 * ((n + 63) // 64), dtype=torch.int32, device=self.dev)
        self.ids = torch.empty(n, dtype=torch.int64, device=self.dev)

    def call(self, program, tile_rows=0, n=None, flags=0, host_form=False, bitmap=True, ids=True, ids_cap=None):
        """(rc, m, words uint32, ids int64) of one C call over pre-filled output buffers"""
        self.words.fill_(FILL_WORD)
        self.ids.fill_(FILL_ID)
        for f in program.fields:
            if f not in self.device_columns:
                c = self.columns[f]
                self.device_columns[f] = (self.torch.from_numpy(c.keys).to(self.dev),
                                          None if c.valid is None else self.torch.from_numpy(c.valid_words().view(np.int32)).to(self.dev))
        ptrs = [(self.device_columns[f][0].data_ptr(), None if self.device_columns[f][1] is None else self.device_columns[f][1].data_ptr())
                for f in program.fields]
        code = [c if c >= 0 else {-1: W.OP_AND, -2: W.OP_OR, -3: W.OP_NOT}[c] for c in program.code]
        rc, m = _ffi.eval_where_device(_ffi.lib(), self.ix._h, self.n if n is None else n, ptrs, program.leaves, np.asarray(code, np.uint8), program.set_values,
                                       self.words.data_ptr() if bitmap else None, self.ids.data_ptr() if ids else None,
                                       self.n if ids_cap is None else ids_cap, self.torch.cuda.current_stream(self.dev).cuda_stream, tile_rows, flags, host_form)
        return rc, m, self.words.cpu().numpy().view(np.uint32), self.ids.cpu().numpy()

    def untouched(self, words, ids):
        return bool((words == FILL_WORD).all() and (ids == FILL_ID).all())

    def close(self):
        self.ix.close()


def _want_words(mask):
    n = mask.shape[0]
    words = np.zeros(2 * ((n + 63) // 64), np.uint32)
    packed = np.packbits(mask, bitorder="little")
    words.view(np.uint8)[:packed.size] = packed
    return words


def _hold(w, name, program, mask, tile_rows):
    rc, m, words, ids = w.call(program, tile_rows)
    assert rc == 0, (name, w.n, tile_rows, _ffi.last_error())
    rows = np.flatnonzero(mask)
    assert m == rows.size, (name, w.n, tile_rows, m, rows.size)
    assert np.array_equal(words, _want_words(mask)), (name, w.n, tile_rows)
    assert np.array_equal(ids[:m], rows + ID0) and (ids[m:] == FILL_ID).all(), (name, w.n, tile_rows)


def _boundary_rows(n, every):
    rows = {0, n - 1}
    step = 32 if every else 1024
    for b in range(step, n, step):
        rows |= {b - 1, b}
    if not every:   # the first and the last word boundaries too
        for b in (32, 64, 96, (n - 1) // 32 * 32, (n - 1) // 64 * 64):
            rows |= {b - 1, b}
    return sorted(r for r in rows if 0 <= r < n)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049, 70001])
def test_the_call_equals_numpy_and_matches(n):
    w = World(n)
    try:
        big = n > 4096
        tiles = (0,) if big else (0, 64)
        for name, program, where in _programs(n, w.columns, few=big):
            assert program.fits_device, name
            mask = program.evaluate_numpy(w.columns)
            ask = W.matcher(where)
            assert np.array_equal(mask, np.fromiter((ask(md) for md in w.metas), np.bool_, n)), (name, n)
            for tile_rows in tiles:
                _hold(w, name, program, mask, tile_rows)
        for r in _boundary_rows(n, every=not big):
            where = {"i": r}
            program = W.compile_where(where, w.columns, n=n)
            mask = program.evaluate_numpy(w.columns)
            ask = W.matcher({"i": {"$eq": r}})
            near = range(max(0, r - 70), min(n, r + 70)) if big else range(n)
            assert int(mask.sum()) == 1 and bool(mask[r]) and [q for q in near if ask(w.metas[q])] == [r]
            for tile_rows in tiles:
                _hold(w, f"row {r}", program, mask, tile_rows)
        for tile_rows in (128, 960):   # every tile size takes the same path; two more, once
            name, program, _ = _programs(n, w.columns, few=True)[3]
            _hold(w, name, program, program.evaluate_numpy(w.columns), tile_rows)
    finally:
        w.close()


def _ranked(w, k=5):
    q = np.random.default_rng(5).standard_normal((3, 8)).astype(np.float32)
    ids, scores = w.ix.search(q, k)
    return ids.tobytes() + scores.tobytes()


def test_refusals_write_nothing_and_leave_the_handle_searching():
    w = World(300)
    try:
        before = _ranked(w)
        good = W.compile_where({"page": {"$gte": 10}}, w.columns, n=w.n)
        assert w.call(good)[0] == 0

        def refused(rc_want, needle, program=good, **kw):
            rc, m, words, ids = w.call(program, **kw)
            assert rc == rc_want and needle in _ffi.last_error(), (rc, _ffi.last_error())
            assert m == -1 and w.untouched(words, ids), needle
            assert _ranked(w) == before

        refused(-1, "vf_index_search_device", host_form=True)                      # the flag on the host form: the message names the device form
        refused(-1, "together", flags=_ffi.VF_SEARCH_SUBSET)
        refused(-1, "together", flags=_ffi.VF_SEARCH_SUBSETS)
        refused(-1, "count bits", flags=3)
        refused(-1, "n = 299 but the index holds 300", n=299)
        refused(-1, "null d_bitmap", bitmap=False)
        refused(-1, "ids_cap = 299", ids_cap=299)
        refused(-1, "tile_rows = 100", tile_rows=100)
        refused(-1, "tile_rows = 2048", tile_rows=2048)
        # programs the checker refuses, each naming the position
        refused(-1, "leaves 2 values", _by_hand(["page"], [(W.LEAF_INTERVAL, 0, 1, 5)], [0, 0], [], 2, w.n))
        refused(-1, "ops[1] pops more", _by_hand(["page"], [(W.LEAF_INTERVAL, 0, 1, 5)], [0, -1], [], 1, w.n))
        refused(-1, "leaves[0]", _by_hand(["page"], [(W.LEAF_INTERVAL, 1, 1, 5)], [0], [], 1, w.n))
        refused(-1, "set_values[2]", _by_hand(["page"], [(W.LEAF_SET, 0, 0, 3)], [0], [1, 5, 5], 1, w.n))
        refused(-1, "leaves[0]: its run", _by_hand(["page"], [(W.LEAF_SET, 0, 2, 2)], [0], [1, 5, 7], 1, w.n))
        # over the limits: VF_EUNSUPPORTED
        refused(-4, "65 leaves", _by_hand(["page"], [(W.LEAF_INTERVAL, 0, j, j) for j in range(65)], [0], [], 1, w.n))
        refused(-4, "past the limit of 32", _by_hand(["page"], [(W.LEAF_INTERVAL, 0, 1, 5)], [0] * 33 + [-1] * 32, [], 33, w.n))
        refused(-4, "129 ops", _by_hand(["page"], [(W.LEAF_INTERVAL, 0, 1, 5)], [0] + [-3] * 128, [], 1, w.n))
        refused(-4, "17 columns", _by_hand(["page"] * 17, [(W.LEAF_INTERVAL, 0, 1, 5)], [0], [], 1, w.n))
        refused(-4, "65537 set values", _by_hand(["page"], [(W.LEAF_SET, 0, 0, 65537)], [0], list(range(65537)), 1, w.n))
        # the columns are stale after an append: n is off by one
        assert w.ix.add(w.rows[:1]) == ID0 + 300 and w.ix.n == 301
        rc, m, words, ids = w.call(good)
        assert rc == -1 and "n = 300 but the index holds 301" in _ffi.last_error() and "stale" in _ffi.last_error() and w.untouched(words, ids)
        assert w.ix.search(w.rows[:1], 2)[0][0].tolist() == [ID0, ID0 + 300]
    finally:
        w.close()


def test_a_group_handle_is_refused():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    rows = np.random.default_rng(0).standard_normal((300, 8)).astype(np.float32)
    cols = {"i": W.build_column(list(range(300)), "i")}
    program = W.compile_where({"i": {"$lt": 7}}, cols)
    with vf.DenseIndex(rows, device_ids=[0, 1]) as ix:
        keys = torch.from_numpy(cols["i"].keys).to("cuda:0")
        words = torch.full((10,), FILL_WORD, dtype=torch.int32, device="cuda:0")
        rc, m = _ffi.eval_where_device(_ffi.lib(), ix._h, 300, [(keys.data_ptr(), None)], program.leaves, program.ops, program.set_values, words.data_ptr(),
                                       None, 0, None)
        assert rc == -4 and "group handle" in _ffi.last_error() and m == -1 and bool((words == FILL_WORD).all())
        with pytest.raises(ValueError, match="numpy route"):
            ix.eval_where(program, cols)


def test_eval_where_of_the_index():
    n = 3000
    rows = np.random.default_rng(7).standard_normal((n, 8)).astype(np.float32)
    metas = _metadata(n)
    where = {"$or": [{"page": {"$gte": 10, "$lte": 40}, "company": {"$ne": "lotus"}}, {"serial": {"$in": list(range(0, 300, 3))}}]}
    fields = W.fields_of(where)

    def columns(mds):
        return {f: W.build_column([md.get(f) for md in mds], f) for f in fields}

    q = np.random.default_rng(8).standard_normal((4, 8)).astype(np.float32)
    with vf.DenseIndex(rows, device_id=0, id_offset=ID0) as ix:
        cols = columns(metas)
        program = W.compile_where(where, cols, n=n)
        subset, mask = ix.eval_where(program, cols)
        keep = np.asarray([r for r, md in enumerate(metas) if W.matches(md, where)], np.int64)
        assert 100 < keep.size < n - 100
        assert isinstance(subset, RowSubset) and subset.ids.tolist() == (keep + ID0).tolist() and subset.tensor.is_cuda and len(subset) == keep.size
        assert subset.tensor.cpu().numpy().tolist() == subset.ids.tolist()
        assert isinstance(mask, W.RowMask) and list(mask) == keep.tolist() and len(mask) == keep.size and -1 not in mask and n not in mask
        got, want = ix.search(q, 20, subset=subset), ix.search(q, 20, subset=keep + ID0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        # a second evaluation reuses the scratch and the columns' device copies; the first RowSubset keeps its own ids
        scratch, held = ix._where_ids.data_ptr(), {f: c._device[0][0].data_ptr() for f, c in cols.items()}
        other = W.compile_where({"page": {"$lt": 5}}, cols, n=n)
        subset2, mask2 = ix.eval_where(other, cols)
        assert ix._where_ids.data_ptr() == scratch and {f: c._device[0][0].data_ptr() for f, c in cols.items()} == held
        assert list(mask2) == [r for r, md in enumerate(metas) if md.get("page") is not None and md["page"] < 5]
        assert subset.tensor.cpu().numpy().tolist() == (keep + ID0).tolist()
        over = W.compile_where({"$or": [{"serial": j} for j in range(70)]}, cols, n=n)
        assert not over.fits_device
        with pytest.raises(ValueError, match="numpy route"):
            ix.eval_where(over, cols)
        # after a removal the columns are stale: refused; rebuilt columns work
        gone = [5, 6, 7, 2999]
        assert ix.remove(np.asarray(gone) + ID0) == 4
        with pytest.raises(RuntimeError, match="stale"):
            ix.eval_where(program, cols)
        left = [md for r, md in enumerate(metas) if r not in gone]
        cols = columns(left)
        subset3, mask3 = ix.eval_where(W.compile_where(where, cols, n=len(left)), cols)
        keep3 = [r for r, md in enumerate(left) if W.matches(md, where)]
        assert list(mask3) == keep3 and subset3.ids.tolist() == [r + ID0 for r in keep3]
        got, want = ix.search(q, 20, subset=subset3), ix.search(q, 20, subset=np.asarray(keep3) + ID0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


class _Emb:
    def __init__(self, d):
        self.d = d

    def embed_query(self, text):
        return np.random.default_rng(zlib.crc32(text.encode())).standard_normal(self.d).astype(np.float32).tolist()


def test_the_real_ensemble_under_a_range_filter(tmp_path, monkeypatch):
    from test_ensemble_where import Store
    from veritasfi_amd import bm25 as B
    from veritasfi_amd.ensemble import EnsembleRetriever
    from veritasfi_amd.index import DenseIndex
    rng = np.random.default_rng(2)
    vocab = [f"word{i}" for i in range(60)] + ["revenue", "margin", "guidance", "dividend"]
    n, d = 500, 32
    emb = _Emb(d)
    texts = [" ".join(rng.choice(vocab, size=int(rng.integers(3, 15)))) + f" uniq{i}" for i in range(n)]
    metas = [{"doc_id": f"d{i}", "prev_chunk_id": "", "next_chunk_id": "", "title_summary": f"title {i // 60}", "page_number": 1 + (i * 7) % 23,
              "date_published": f"20{20 + (i * 3) % 5:02d}-{1 + (i * 11) % 12:02d}-{1 + (i * 5) % 28:02d}",
              **({"bundle_id": f"b{i // 6}"} if i % 6 < 2 else {})} for i in range(n)]
    vecs = [emb.embed_query(t) for t in texts]
    ts = Store([f"title {t}" for t in range(9)], [None] * 9, rng.standard_normal((9, d)).tolist())
    queries = ["revenue guidance word3", "dividend dividend margin", "uniq312 word7", "word7 word8 word9 word10"]
    day = "2022-06-15"
    where = {"date_published": {"$lte": day}, "page_number": {"$gte": 3}}
    keep = [i for i, md in enumerate(metas) if md["date_published"] <= day and md["page_number"] >= 3]
    assert 100 < len(keep) < 400 and keep == [i for i, md in enumerate(metas) if W.matches(md, where)]
    listed = {"date_published": sorted({md["date_published"] for md in metas if md["date_published"] <= day}),
              "page_number": sorted({md["page_number"] for md in metas if md["page_number"] >= 3})}      # the plain dict that lists every passing value
    B.build_bm25_index(texts, str(tmp_path / "full"), doc_ids=[m["doc_id"] for m in metas], stemmer=None)
    B.build_bm25_index([texts[i] for i in keep], str(tmp_path / "small"), doc_ids=[metas[i]["doc_id"] for i in keep], stemmer=None)
    calls = []
    inner = DenseIndex.eval_where
    monkeypatch.setattr(DenseIndex, "eval_where", lambda self, *a, **kw: (calls.append(1), inner(self, *a, **kw))[1])
    with vf.BM25Retriever(str(tmp_path / "full"), stemmer=None, live=True) as bm, vf.BM25Retriever(str(tmp_path / "small"), stemmer=None) as bm_small:
        kw = dict(bm25_k=12, prefetch_documents=True)
        er = EnsembleRetriever("unused", Store(texts, metas, vecs), ts, 5, emb, bm25_retriever=bm, where_statistics="subset", **kw)
        small = EnsembleRetriever("unused", Store([texts[i] for i in keep], [metas[i] for i in keep], [vecs[i] for i in keep]), ts, 5, emb,
                                  bm25_retriever=bm_small, **kw)
        assert er.rows_where(where).tolist() == keep and len(calls) == 1, "the device evaluated the filter"
        want = [small.invoke(q, []) for q in queries]
        got = [er.invoke(q, [], where=where) for q in queries]
        assert len(calls) == 1 + len(queries)
        assert got == want, "the store of the passing chunks alone"
        assert any(c["retriever"] == "BM25" for out in got for c in out) and any(c["retriever"] == "FAISS" for out in got for c in out)
        assert all(c["metadata"]["date_published"] <= day and c["metadata"]["page_number"] >= 3 for out in got for c in out)
        assert any(not W.matches(c["metadata"], where) for q in queries for c in er.invoke(q, [])), "the unfiltered call reaches hidden chunks"
        assert [er.invoke(q, [], where=listed) for q in queries] == got, "the parent's only route: every passing value listed"
        assert er.invoke_batch(queries, [[] for _ in queries], wheres=[dict(where) for _ in queries]) == got
        assert len(calls) == 2 + len(queries), "a batch of equal filters is evaluated once"
        with er.prepare_where(where) as pw:
            assert isinstance(pw.dense, RowSubset) and isinstance(pw.bm25, B.BM25Subset) and isinstance(pw.allow, W.RowMask)
            assert pw.dense.ids.tolist() == keep and len(calls) == 3 + len(queries)
            assert [er.invoke(q, [], where=pw) for q in queries] == got
            assert er.invoke_batch(queries, [[] for _ in queries], wheres=[pw, dict(where), pw, None]) == got[:3] + [er.invoke(queries[3], [])]
        # under whole-corpus statistics (the default) the three forms still agree with one another
        plain = EnsembleRetriever("unused", Store(texts, metas, vecs), ts, 5, emb, bm25_retriever=bm, **kw)
        base = [plain.invoke(q, [], where=where) for q in queries]
        assert base == [plain.invoke(q, [], where=listed) for q in queries]
        assert plain.invoke_batch(queries, [[] for _ in queries], wheres=[where] * len(queries)) == base
