"""A row list PER QUERY of a dense batch (``DenseIndex.search(queries, k, subsets=[...])`` -> ``vf_index_search`` / ``_device`` with
``VF_SEARCH_SUBSETS``; k_subset_check_m, k_scan_subset_m, the ranking kernels, k_subset_ids_m) on the GPU.

The rule under test: row i is, ids and score BITS, what ``search(queries[i:i+1], k, subset=subsets[i])`` returns -- the plain search for
None.  So every expected value is that one-list call for the query alone, and the CPU oracle over ``values[list_i]`` with ids mapped
back (``tests/test_gpu_subset_search.py::_want``).  Shapes are the smallest at which each thing can break: 64 positions per workgroup
(lists of 63, 64, 65), tiles of 4 queries (five queries of one list are two tiles), size classes of 256 / 2048 / 8192 / 16 384 rows
(lists of 257 and 3000), passes of 256 queries (300), lists of at most 16 384 ids (16 385 is refused by the library and routed by Python).

The first test runs 11 queries, not 9: seven lists, one of them used five times, need 5 + 6."""
import numpy as np
import pytest

from test_gpu_subset_search import KINDS, FLT_MAX, _bits, _encode, _make, _pick, _same, _values, _want, _Embedder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()
    return m


@pytest.fixture(scope="module")
def pool():
    """One block of N(0, 1) values every test cuts its rows and queries from (generated once)."""
    return np.random.default_rng(2323).standard_normal((20_400, 1040), dtype=np.float32)


def _tiles(list_of, pass_queries=256):
    """Per pass, the sum over its lists of ceil(queries of that list / 4)."""
    total = 0
    for p0 in range(0, len(list_of), pass_queries):
        part = list(list_of[p0:p0 + pass_queries])
        total += sum(-(-part.count(j) // 4) for j in set(part))
    return total


def _alone(ix, q, k, subsets):
    """The rule's right-hand side: each query alone under its own list."""
    got = [ix.search(q[i:i + 1], k, subset=s) if s is not None else ix.search(q[i:i + 1], k) for i, s in enumerate(subsets)]
    return np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])


def _oracle_rows(oracle, vals, q, k, sels, id_offset=0):
    got = [_want(oracle, vals, s, q[i:i + 1], k, id_offset=id_offset) if s is not None else oracle.search(vals, q[i:i + 1], k) for i, s in enumerate(sels)]
    ids = np.concatenate([g[0] for g in got])
    if id_offset:
        for i, s in enumerate(sels):
            if s is None:
                ids[i] = np.where(ids[i] >= 0, ids[i] + id_offset, -1)
    return ids, np.concatenate([g[1] for g in got])


def _check(ix, oracle, vals, q, k, sels, id_offset=0, what=None):
    """sels: per query an ascending int64 array of ROWS, or None; the call is made with ids (rows + id_offset)."""
    as_ids = {id(s): s + id_offset for s in sels if s is not None}     # one object per list: queries of one list share it
    subsets = [None if s is None else as_ids[id(s)] for s in sels]
    got = ix.search(q, k, subsets=subsets)
    st = ix.stats()
    assert _same(got, _alone(ix, q, k, subsets)), what
    assert _same(got, _oracle_rows(oracle, vals, q, k, sels, id_offset)), what
    for i, s in enumerate(sels):
        if s is not None and s.size < k:      # each query pads from its own min(m_i, k)
            assert (got[0][i, s.size:] == -1).all() and (got[1][i, s.size:] == -FLT_MAX).all() and (got[0][i, :s.size] >= 0).all(), (what, i)
    return got, st


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [100, 768, 1040])
@pytest.mark.parametrize("kind", KINDS)
def test_rule(vf, oracle, pool, kind, d):
    """d = 100: rows that are not 16-byte aligned and a tail block; 1040: two K-slices.  Lists of 1, 63, 64, 65, 257 and 3000 (= n) rows
    and an empty one, interleaved A B A C A A A D E F G: the five queries of A are two tiles."""
    n, k = 3000, 20
    rows = _encode(vf, kind, pool[:n, :d])
    vals = _values(kind, rows)
    rng = np.random.default_rng(d)
    lists = {m: _pick(rng, n, m, ends=(m == 65)) for m in (1, 63, 64, 65, 257)}
    lists[3000], lists[0] = np.arange(n, dtype=np.int64), np.empty(0, np.int64)
    order = [64, 257, 64, 1, 64, 64, 64, 63, 3000, 0, 65]
    sels = [lists[m] for m in order]
    q = pool[20_000:20_000 + len(order), :d].copy()
    with _make(vf, kind, rows) as ix:
        got, st = _check(ix, oracle, vals, q, k, sels, what=(kind, d))
        assert st["path"] == 4 and st["n_queries"] == len(order), st
        assert st["subset_tiles"] == _tiles(order) == 8 and st["subset_rows"] == sum(order), st
        assert (got[0][9] == -1).all() and (got[1][9] == -FLT_MAX).all()          # the empty list


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2048, 5000])
def test_k_and_classes(vf, oracle, pool, k):
    """Lists of 40 and 3000 rows in one batch: two size classes; at k = 2048 the short one is ranked by the sort of its whole row and the
    long one by the select; k = 5000 is beyond every list."""
    n, d = 3200, 100
    rows = pool[:n, :d].astype(np.float16)
    rng = np.random.default_rng(40)
    a, b = _pick(rng, n, 40, ends=True), _pick(rng, n, 3000, ends=True)
    q = pool[20_000:20_003, :d].copy()
    with vf.DenseIndex(rows) as ix:
        got, st = _check(ix, oracle, rows, q, k, [a, b, a], what=k)
        assert st["path"] == 4 and st["subset_tiles"] == 2 and st["subset_rows"] == 3080
        assert (got[0][0, 40:] == -1).all() and (got[0][1, :min(k, 3000)] >= 0).all() and (got[0][1, 3000:] == -1).all()


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def _raw_m(ix, q, k, lists, list_of, device):
    """The C entry points themselves (the Python layer would sort the lists and route the long ones): (rc, message, out ids, out scores)."""
    import torch
    from veritasfi_amd import _ffi
    L = _ffi.lib()
    lists = [np.ascontiguousarray(x, dtype=np.int64) for x in lists]
    if not device:
        out_i = np.full((len(q), k), 7, np.int64)
        out_s = np.full((len(q), k), 7, np.float32)
        rc = _ffi.search_subsets(L, ix._h, q.ctypes.data, len(q), k, [x.ctypes.data for x in lists], [x.size for x in lists], list_of,
                                 out_i.ctypes.data, out_s.ctypes.data)
        return rc, _ffi.last_error(), out_i, out_s
    dq = torch.from_numpy(q).cuda()
    dl = [torch.from_numpy(x).cuda() for x in lists]
    out_i = torch.full((len(q), k), 7, dtype=torch.int64, device="cuda")
    out_s = torch.full((len(q), k), 7, dtype=torch.float32, device="cuda")
    rc = _ffi.search_subsets_device(L, ix._h, dq.data_ptr(), len(q), k, [x.data_ptr() for x in dl], [x.size for x in lists], list_of,
                                    out_i.data_ptr(), out_s.data_ptr(), None)
    msg = _ffi.last_error()
    torch.cuda.synchronize()
    return rc, msg, out_i.cpu().numpy(), out_s.cpu().numpy()


@pytest.fixture(scope="module")
def wide(vf, pool):
    n, d = 20_000, 100
    rows = pool[:n, :d].astype(np.float16)
    ix = vf.DenseIndex(rows)
    yield ix, rows, pool[20_000:20_012, :d].copy()
    ix.close()


@pytest.mark.parametrize("device", [False, True])
def test_bounds(wide, oracle, device):
    """16 383 and 16 384 ids are served by the library; 16 385 is rc = -4 naming the list, with nothing written."""
    ix, rows, q = wide
    rng = np.random.default_rng(16384)
    l3, l4, l5 = (_pick(rng, len(rows), m, ends=True) for m in (16_383, 16_384, 16_385))
    plain = ix.search(q[:3], 10)
    rc, msg, out_i, out_s = _raw_m(ix, q[:3], 10, [l3, l4], [1, 0, 1], device)
    assert rc == 0, msg
    assert ix.stats()["path"] == 4 and ix.stats()["subset_rows"] == 2 * 16_384 + 16_383 and ix.stats()["subset_tiles"] == 2
    assert _same((out_i, out_s), _oracle_rows(oracle, rows, q[:3], 10, [l4, l3, l4]))
    rc, msg, out_i, out_s = _raw_m(ix, q[:3], 10, [l3, l5, l4], [0, 1, 2], device)
    assert rc == -4 and "lists[1]" in msg and "16385" in msg, (rc, msg)
    assert (out_i == 7).all() and (out_s == 7).all(), "a refused call writes nothing"
    rc, msg, out_i, _ = _raw_m(ix, q[:3], 10, [l3, l5, l4], [0, 0, 2], device)
    assert rc == 0, "a list no query names is not looked at: " + msg
    if not device:      # the Python call routes the long list to the one-list call and returns the rule's answer
        got = ix.search(q[:4], 10, subsets=[l5, l4, None, l5])
        assert _same(got, _alone(ix, q[:4], 10, [l5, l4, None, l5]))
        assert _same(got, _oracle_rows(oracle, rows, q[:4], 10, [l5, l4, None, l5]))
    assert _same(ix.search(q[:3], 10), plain), "the plain search after the refusal"


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,n_lists", [(70, 70), (300, 40)])
def test_batch_size(wide, oracle, pool, nq, n_lists):
    """70 lists in one pass; 300 queries are two passes (256 + 44), each with its own permutation and tiles."""
    ix, rows, _ = wide
    rng = np.random.default_rng(nq)
    lists = [_pick(rng, len(rows), int(rng.integers(1, 300))) for _ in range(n_lists)]
    list_of = [j % n_lists for j in range(nq)] if nq == n_lists else rng.integers(0, n_lists, nq).tolist()
    q = pool[:nq, 300:400].copy()
    got, st = _check(ix, oracle, rows, q, 12, [lists[j] for j in list_of], what=nq)
    assert st["path"] == 4 and st["n_queries"] == nq and st["subset_tiles"] == _tiles(list_of) and st["subset_rows"] == sum(lists[j].size for j in list_of)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_forms(vf, oracle, pool):
    n, d = 3000, 100
    rows = pool[:n + 200, :d].astype(np.float16)
    q = pool[20_000:20_006, :d].copy()
    rng = np.random.default_rng(55)
    a, b, c = _pick(rng, n, 70, ends=True), _pick(rng, 2500, 300), _pick(rng, 2000, 5)   # a alone reaches past row 2500
    with vf.DenseIndex(rows[:n]) as ix:
        ra, rb, rc_ = ix.row_subset(a), ix.row_subset(b), ix.row_subset(c)
        host = ix.search(q, 9, subsets=[a, b, a, c, b, a])
        assert ix.stats()["path"] == 4
        dev = ix.search(q, 9, subsets=[ra, rb, ra, rc_, rb, ra])                  # every entry a RowSubset on the device: the device form
        assert ix.stats()["path"] == 4 and ix.stats()["subset_tiles"] == 3
        mix = ix.search(q, 9, subsets=[ra, b, ra, rc_, b, ra])                    # one array among them: the host form, from the host copies
        assert _same(host, dev) and _same(host, mix)
        assert _same(host, _oracle_rows(oracle, rows[:n], q, 9, [a, b, a, c, b, a]))
        with pytest.raises(ValueError, match="cannot be given together"):
            ix.search(q, 9, subset=a, subsets=[a] * 6)
        with pytest.raises(ValueError, match="5 entries for 6 queries"):
            ix.search(q, 9, subsets=[a] * 5)
        ix.remove(np.arange(2500, 3000))                                          # ra reaches past the new end: stale
        for subsets in ([rc_, rb, ra, ra, rb, rb], [c, b, ra, ra, b, b]):         # device form, host form
            with pytest.raises(RuntimeError, match=r"subsets\[2\]: ids\[\d+\] = \d+ is outside"):
                ix.search(q, 9, subsets=subsets)
        assert _same(ix.search(q, 9, subsets=[rc_, b, c, rc_, b, c]), _oracle_rows(oracle, rows[:2500], q, 9, [c, b, c, c, b, c])), "the refusals changed nothing"


@pytest.mark.parametrize("device", [False, True])
def test_refusals(vf, oracle, pool, device):
    n, d = 2500, 100
    rows = pool[:n, :d].astype(np.float16)
    q = pool[20_000:20_003, :d].copy()
    good = [10, 20, 2509]
    with vf.DenseIndex(rows, id_offset=10) as ix:
        before = ix.search(q, 5)
        for ids, where, word in (([30, 20, 40], 1, "not ascending"), ([20, 30, 30, 40], 2, "duplicate"), ([-1, 20], 0, "outside"),
                                 ([20, 2510], 1, "outside"), ([9, 20], 0, "outside")):
            rc, msg, out_i, out_s = _raw_m(ix, q, 5, [good, ids, good], [0, 1, 2], device)
            assert rc == -1 and f"lists[1]: ids[{where}]" in msg and word in msg, (ids, rc, msg)
            assert (out_i == 7).all() and (out_s == 7).all(), "a refused call writes nothing"
        rc, msg, out_i, out_s = _raw_m(ix, q, 5, [good, [40, 30], [50, 50]], [0, 2, 1], device)
        assert rc == -1 and "lists[1]: ids[1]" in msg, "the lowest list, then the lowest position: " + msg
        for list_of, query in (([0, 3, 1], 1), ([0, 1, -1], 2)):
            rc, msg, out_i, out_s = _raw_m(ix, q, 5, [good, good, good], list_of, device)
            assert rc == -1 and f"list_of[{query}]" in msg and f"query {query}" in msg, (rc, msg)
            assert (out_i == 7).all()
        rc, msg, out_i, out_s = _raw_m(ix, q, 5, [good, [30, 20]], [0, 0, 0], device)
        assert rc == 0, "a bad list no query names is not read: " + msg
        want = _want(oracle, rows, np.array([0, 10, 2499]), q, 5, id_offset=10)
        assert _same((out_i, out_s), want)
        assert _same(ix.search(q, 5), before)


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_ties_and_negative_zero(vf, oracle, pool):
    from rank_cases import negative_zero_case
    n, d = 2000, 768
    x = pool[:n, :d].copy()
    x[1200] = x[40]      # a copy inside list A and outside list B
    x[900] = x[40]       # a copy outside both
    rows = x.astype(np.float16)
    q = np.repeat(rows[40:41].astype(np.float32), 3, axis=0)
    a, b = np.array([3, 40, 41, 1200, 1999], dtype=np.int64), np.array([3, 40, 41, 1999], dtype=np.int64)
    with vf.DenseIndex(rows) as ix:
        (ids, sc), _ = _check(ix, oracle, rows, q, 5, [a, b, a])
    assert ids[0, :2].tolist() == [40, 1200] and _bits(sc[0, 0]) == _bits(sc[0, 1]) and 900 not in ids
    assert ids[1, 0] == 40 and 1200 not in ids[1] and ids[1, 4] == -1
    zrows, zq, _ = negative_zero_case(n=40, d=32)
    a, b = np.array([0, 1, 2, 3, 17, 39], dtype=np.int64), np.array([0, 2, 39], dtype=np.int64)
    with vf.DenseIndex(zrows) as ix:
        (ids, sc), _ = _check(ix, oracle, zrows, np.repeat(zq, 2, axis=0), 6, [a, b])
    assert ids[0].tolist() == [1, 0, 2, 3, 17, 39] and ids[1].tolist() == [0, 2, 39, -1, -1, -1]
    assert (_bits(sc[0, 1:]) == 0).all() and (_bits(sc[1, :3]) == 0).all(), "a zero score is reported as +0.0"


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_handle_state(vf, oracle, pool):
    import torch
    from veritasfi_amd import _ffi
    n, d = 2000, 100
    rows = pool[:n + 300, :d].astype(np.float16)
    q = pool[20_000:20_005, :d].copy()
    rng = np.random.default_rng(7)
    with vf.DenseIndex(rows[:n], id_offset=1000) as ix:
        a, b = _pick(rng, n, 90, ends=True), _pick(rng, n, 7)
        _check(ix, oracle, rows[:n], q, 8, [a, b, None, a, b], id_offset=1000, what="id_offset")
        ix.add(rows[n:])                                                          # a live index: old rows and new ones in one list
        c = np.array([5, 1999, 2000, 2100, 2299], dtype=np.int64)
        want, _ = _check(ix, oracle, rows, q, 8, [c, a, c, b, c], id_offset=1000, what="after add")
        # a search pending in a slot is not disturbed by a multi call between its begin and end, in either form
        dq = torch.from_numpy(q).cuda()
        ids, sc = ix.search_begin(1, dq, 10)
        ci, ai, bi = c + 1000, a + 1000, b + 1000
        assert _same(ix.search(q, 8, subsets=[ci, ai, ci, bi, ci]), want)
        rc_, ra, rb = ix.row_subset(ci), ix.row_subset(ai), ix.row_subset(bi)
        assert _same(ix.search(q, 8, subsets=[rc_, ra, rc_, rb, rc_]), want)
        ix.search_end(1)
        torch.cuda.synchronize()
        plain = oracle.search(rows, q, 10)
        assert _same((ids.cpu().numpy(), sc.cpu().numpy()), (np.where(plain[0] >= 0, plain[0] + 1000, -1), plain[1]))
    with vf.DenseIndex(rows[:n], device_ids=[0, 0]) as grp:
        with pytest.raises(ValueError, match="sharded"):
            grp.search(q, 4, subsets=[a] * 5)
        for device in (False, True):
            rc, msg, out_i, _ = _raw_m(grp, q, 4, [a], [0] * 5, device)
            assert rc == -4 and "group handle" in msg and (out_i == 7).all(), (rc, msg)
        assert _ffi.lib().vf_version() == 100


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_fuzz(vf, oracle):
    """100 seeded cases over the four row types: n <= 20 000, nq <= 12, up to 6 lists per batch, m <= 16 384, k in {1, 7, 100, 2048}; a
    quarter of the entries are None and a list may be empty.  Four indexes, twenty-five batches each."""
    rng = np.random.default_rng(2323)
    cases = 0
    for kind, d, n in (("f16", 64, 20_000), ("f32", 36, 17_000), ("e4m3", 48, 9000), ("int8", 33, 16_384)):
        x = rng.standard_normal((n + 12, d), dtype=np.float32)
        rows = _encode(vf, kind, x[:n])
        vals = _values(kind, rows)
        with _make(vf, kind, rows, id_offset=int(rng.integers(0, 1000))) as ix:
            for _ in range(25):
                nq, n_lists = int(rng.integers(1, 13)), int(rng.integers(1, 7))
                k = int(rng.choice([1, 7, 100, 2048]))
                lens = [int(rng.choice([rng.integers(0, 70), rng.integers(0, 300), rng.integers(0, 2100), rng.integers(0, min(n, 16_384) + 1)])) for _ in range(n_lists)]
                lists = [_pick(rng, n, m) for m in lens]
                sels = [None if rng.random() < 0.25 else lists[int(rng.integers(n_lists))] for _ in range(nq)]
                _check(ix, oracle, vals, x[n:n + nq], k, sels, id_offset=ix.id_offset, what=(kind, nq, lens, k))
                cases += 1
    assert cases == 100


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_faiss_retriever_subsets(vf, oracle, pool):
    n, d = 2000, 100
    emb = pool[:n, :d].copy()
    qtab = pool[20_000:20_010, :d]
    r = vf.FaissRetriever(emb, _Embedder(qtab))
    assert r.per_query_subsets is True
    a, b = np.array([1, 500, 501, 1999], dtype=np.int64), np.arange(300, 900, dtype=np.int64)
    got = r.invoke(["0", "3", "9", "4"], 5, subsets=[a, None, b, a])
    assert _same(got, _oracle_rows(oracle, emb, qtab[[0, 3, 9, 4]], 5, [a, None, b, a]))
    for i, (s, sub) in enumerate(zip("0394", (a, None, b, a))):
        one = r.invoke([s], 5, subset=sub)
        assert _same((got[0][i:i + 1], got[1][i:i + 1]), one), i
    r.index.close()


@pytest.mark.parametrize("expand", [False, True])
def test_ensemble_invoke_batch_on_the_gpu(vf, expand):
    """``invoke_batch`` with this package's FaissRetriever as the dense legs and three tenants equals the per-request ``invoke``; the dense
    leg of the batch is ONE list-per-query call (path 4)."""
    import test_ensemble_where as W
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, order, scores, queries = W._world(5)
    ts = W.Store(titles, [None] * len(titles), t_emb.tolist())
    er = EnsembleRetriever("unused", W.Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=W.Bm25(order, scores),
                           faiss_ts_k=2, bm25_k=5, enable_expand=expand, similarity_from_rows=False)
    try:
        tenants = [{"company": c} for c in W.COMPANIES]
        inputs, hyde = [q for q, _ in queries], [h for _, h in queries]
        with er.prepare_where(tenants[2]) as pw:
            for wheres in ([dict(tenants[i % 3]) for i in range(6)], [dict(tenants[0]), pw, None, {"company": "nobody"}, pw, dict(tenants[1])]):
                want = [er.invoke(q, h, where=w) for q, h, w in zip(inputs, hyde, wheres)]
                assert sum(len(o) for o in want) > 0
                got = er.invoke_batch(inputs, hyde, wheres)
                assert got == want
                st = er.faiss_retriever.index.stats()
                assert st["path"] == 4 and st["subset_tiles"] >= 3, st
    finally:
        er.faiss_retriever.index.close()
        er.title_summary_faiss_retriever.index.close()
