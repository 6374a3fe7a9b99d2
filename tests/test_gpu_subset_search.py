"""Searching a chosen subset of rows (``DenseIndex.search(subset=...)`` -> ``vf_index_search`` / ``_device`` with ``VF_SEARCH_SUBSET``; k_scan_subset) on the GPU.

The rule under test: the result is what an index over the listed rows alone would return, ids mapped back.  So every expected value
is the CPU oracle's on ``values[sel]`` with ids mapped through ``sel`` (+ ``id_offset``), and ids and score BITS must be equal.
Shapes are the smallest at which each thing can break: the kernel scores a row with a pair of lanes, 2 rows per pair, 64 rows per
workgroup, 4 queries per pass over the rows and 1024 elements of a query in LDS at a time; ranking takes 16 384 positions per part and a
merge takes as many parts as 16 384 keys hold."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
KINDS = ("f32", "f16", "e4m3", "int8")
# one value either side of: a block of 16, the 32 pairs of a wave, the 64 rows of a workgroup, 256
MS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257)
NQS = (1, 4, 5, 33, 64, 65)


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()
    return m


@pytest.fixture(scope="module")
def pool():
    """One block of N(0, 1) values every test cuts its rows and queries from (generated once)."""
    return np.random.default_rng(1616).standard_normal((20_100, 2560), dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _encode(vf, kind, x):
    import torch
    if kind == "f32":
        return np.ascontiguousarray(x, dtype=np.float32)
    if kind == "f16":
        return x.astype(np.float16)
    if kind == "e4m3":
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return vf.quantize_int8(x)


def _values(kind, rows):
    from oracle import ref_numpy
    if kind == "e4m3":
        return ref_numpy.decode_e4m3(rows).astype(np.float16)
    if kind == "int8":
        return rows.astype(np.float32)
    return rows


def _make(vf, kind, rows, **kw):
    return vf.DenseIndex.from_e4m3(rows, **kw) if kind == "e4m3" else vf.DenseIndex(rows, **kw)


def _want(oracle, values, sel, q, k, id_offset=0):
    """The oracle over the listed rows alone, ids mapped back through the list."""
    sel = np.asarray(sel, dtype=np.int64)
    if sel.size == 0:
        return np.full((len(q), k), -1, np.int64), np.full((len(q), k), -FLT_MAX, np.float32)
    ids, sc = oracle.search(values[sel], q, k)
    return np.where(ids >= 0, sel[np.maximum(ids, 0)] + id_offset, -1), sc


def _pick(rng, n, m, ends=False):
    sel = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    if ends and m >= 2:
        sel[0], sel[-1] = 0, n - 1
    return sel


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1538, 20_000])
@pytest.mark.parametrize("d", [100, 768, 2560])
@pytest.mark.parametrize("kind", KINDS)
def test_dtypes_and_widths(vf, oracle, pool, kind, d, n):
    """n = 1538: the small path's index (it keeps a cache of normalised rows, which the subset scan does not read); n = 20 000: a
    fused-path index, no cache.  d = 100: rows that are not 16-byte aligned and a tail block; 2560: three K-slices."""
    rows = _encode(vf, kind, pool[:n, :d])
    vals = _values(kind, rows)
    q = pool[20_000:20_065, :d].copy()
    rng = np.random.default_rng(n + d)
    k = 20
    with _make(vf, kind, rows) as ix:
        for m in MS:
            sel = _pick(rng, n, m, ends=(m == 33))
            want = _want(oracle, vals, sel, q, k)
            for nq in NQS:
                got = ix.search(q[:nq], k, subset=sel)
                st = ix.stats()
                assert _same(got, (want[0][:nq], want[1][:nq])), (kind, d, n, m, nq)
                assert st["path"] == 3 and st["subset_rows"] == m and st["n_queries"] == nq, st


def test_k_slices_at_4096_e4m3(vf, oracle):
    d, n = 4096, 600
    x = np.random.default_rng(4096).standard_normal((n + 64, d), dtype=np.float32)
    rows = _encode(vf, "e4m3", x[:n])
    sel = _pick(np.random.default_rng(1), n, 130, ends=True)
    with _make(vf, "e4m3", rows) as ix:
        got = ix.search(x[n:], 50, subset=sel)
    assert _same(got, _want(oracle, _values("e4m3", rows), sel, x[n:], 50))


def test_more_queries_than_one_pass(vf, oracle, pool):
    """257 queries: two passes (256 + 1) over the list."""
    n, d = 3000, 100
    rows = pool[:n, :d].astype(np.float16)
    q = pool[:257, 200:200 + d].copy()
    sel = _pick(np.random.default_rng(257), n, 70, ends=True)
    with vf.DenseIndex(rows) as ix:
        assert _same(ix.search(q, 9, subset=sel), _want(oracle, rows, sel, q, 9))


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_edges(vf, oracle, pool):
    n, d = 3000, 768
    rows = pool[:n, :d].astype(np.float16)
    q = pool[20_000:20_005, :d].copy()
    with vf.DenseIndex(rows, id_offset=1000) as ix:
        sel = np.array([0, 1, 77, 1500, n - 1], dtype=np.int64)
        got = ix.search(q, 8, subset=sel + 1000)                          # rows 0 and n - 1, an id offset, k > m pads
        assert _same(got, _want(oracle, rows, sel, q, 8, id_offset=1000))
        assert (got[0][:, 5:] == -1).all() and (got[1][:, 5:] == -FLT_MAX).all()
        mask = np.zeros(n, bool)
        mask[sel] = True
        assert _same(ix.search(q, 8, subset=mask), got)                   # the mask names rows, the list ids
        assert _same(ix.search(q, 8, subset=(sel + 1000)[::-1].tolist() + [1077]), got)   # unsorted, repeating: sorted on the host
        ids, sc = ix.search(q, 6, subset=np.empty(0, np.int64))           # nothing listed
        assert (ids == -1).all() and (sc == -FLT_MAX).all()
        assert ix.stats()["path"] == 3 and ix.stats()["subset_rows"] == 0
        plain = ix.search(q, 8)
        st_plain = ix.stats()
        allrows = ix.search(q, 8, subset=np.arange(1000, 1000 + n))       # every row listed: the ordinary search
        assert _same(allrows, plain) and ix.stats()["path"] == st_plain["path"] != 3
        big = ix.search(q[:1], 5000, subset=sel + 1000)                   # any k while the list is short
        assert big[0].shape == (1, 5000) and (big[0][0, 5:] == -1).all() and np.array_equal(big[0][0, :5], got[0][0, :5])


def test_ties_and_negative_zero(vf, oracle, pool):
    from rank_cases import negative_zero_case
    n, d = 2000, 768
    x = pool[:n, :d].copy()
    x[1200] = x[40]      # a copy inside the subset: ranks after the original, same bits
    x[900] = x[40]       # a copy outside the subset: never appears
    rows = x.astype(np.float16)
    q = rows[40:41].astype(np.float32)
    sel = np.array([3, 40, 41, 1200, 1999], dtype=np.int64)
    with vf.DenseIndex(rows) as ix:
        ids, sc = ix.search(q, 5, subset=sel)
    assert ids[0, 0] == 40 and ids[0, 1] == 1200 and _bits(sc[0, 0]) == _bits(sc[0, 1]) and 900 not in ids
    assert _same((ids, sc), _want(oracle, rows, sel, q, 5))
    zrows, zq, _ = negative_zero_case(n=40, d=32)
    sel = np.array([0, 1, 2, 3, 17, 39], dtype=np.int64)
    with vf.DenseIndex(zrows) as ix:
        ids, sc = ix.search(zq, 6, subset=sel)
    assert ids[0].tolist() == [1, 0, 2, 3, 17, 39]
    assert (_bits(sc[0, 1:]) == 0).all(), "a zero score is reported as +0.0"
    assert _same((ids, sc), _want(oracle, zrows, sel, zq, 6))


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(vf, pool):
    n, d = 150_000, 100
    rows = np.random.default_rng(150).standard_normal((n, d), dtype=np.float32).astype(np.float16)
    q = pool[20_000:20_002, :d].copy()
    ix = vf.DenseIndex(rows)
    yield ix, rows, q
    ix.close()


@pytest.mark.parametrize("m", [16_384, 16_385, 147_457])
def test_chunks_and_merges(big, oracle, m):
    """16 384: one part, no merge; 16 385: two parts, one merge; 147 457 at k = 2048: ten parts through an 8-slot buffer, two merges."""
    ix, rows, q = big
    sel = _pick(np.random.default_rng(m), len(rows), m, ends=True)
    got = ix.search(q, 2048, subset=sel)
    assert _same(got, _want(oracle, rows, sel, q, 2048)), m
    assert ix.stats()["path"] == 3 and ix.stats()["subset_rows"] == m


def test_k_limit_and_super_chunks(big, oracle):
    ix, rows, q = big
    sel = _pick(np.random.default_rng(8192), len(rows), 40_000)
    got = ix.search(q[:1], 8192, subset=sel)
    assert _same(got, _want(oracle, rows, sel, q[:1], 8192))
    with pytest.raises(RuntimeError, match="rc=-4"):
        ix.search(q[:1], 8193, subset=sel)
    want = _want(oracle, rows, sel, q, 100)
    assert _same(ix.search(q, 100, subset=sel), want)
    ix.set_option("subset_super_rows", 16_384)        # three launches of the scan instead of one
    try:
        assert _same(ix.search(q, 100, subset=sel), want)
    finally:
        ix.set_option("subset_super_rows", 0)
    assert _same(ix.search(q, 100), oracle.search(rows, q, 100)), "the ordinary search after the refusal"


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_live_index(vf, oracle, pool):
    n, d = 2000, 100
    rows = pool[:n + 300, :d].astype(np.float16)
    q = pool[20_000:20_003, :d].copy()
    with vf.DenseIndex(rows[:n]) as ix:
        ix.add(rows[n:])
        sel = np.array([5, 1999, 2000, 2100, 2299], dtype=np.int64)      # old rows and new ones
        assert _same(ix.search(q, 4, subset=sel), _want(oracle, rows, sel, q, 4))
        rs = ix.row_subset(sel)
        ix.remove(np.arange(100, 500))
        cur = np.delete(rows, np.arange(100, 500), 0)
        with pytest.raises(RuntimeError, match=r"ids\[1\] = 1999 is outside"):
            ix.search(q, 4, subset=rs)                                    # a stale subset that reaches past the new end
        sel = np.array([5, 100, 1899], dtype=np.int64)
        assert _same(ix.search(q, 4, subset=sel), _want(oracle, cur, sel, q, 4))


def _raw(vf, ix, q, k, ids, device):
    """The C entry points themselves (the Python layer would sort the list first): returns (rc, message, out ids)."""
    import torch
    from veritasfi_amd import _ffi
    L = _ffi.lib()
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    if not device:
        out_i = np.full((len(q), k), 7, np.int64)
        out_s = np.zeros((len(q), k), np.float32)
        rc = _ffi.search_subset(L, ix._h, q.ctypes.data, len(q), k, ids.ctypes.data, ids.size, out_i.ctypes.data, out_s.ctypes.data)
        return rc, _ffi.last_error(), out_i
    dq, di = torch.from_numpy(q).cuda(), torch.from_numpy(ids).cuda()
    out_i = torch.full((len(q), k), 7, dtype=torch.int64, device="cuda")
    out_s = torch.zeros((len(q), k), dtype=torch.float32, device="cuda")
    rc = _ffi.search_subset_device(L, ix._h, dq.data_ptr(), len(q), k, di.data_ptr(), ids.size, out_i.data_ptr(), out_s.data_ptr(), None)
    msg = _ffi.last_error()
    torch.cuda.synchronize()
    return rc, msg, out_i.cpu().numpy()


@pytest.mark.parametrize("device", [False, True])
def test_refusals(vf, oracle, pool, device):
    n, d = 2500, 100
    rows = pool[:n, :d].astype(np.float16)
    q = pool[20_000:20_002, :d].copy()
    with vf.DenseIndex(rows, id_offset=10) as ix:
        before = ix.search(q, 5)
        for ids, where, word in (([30, 20, 40], 1, "not ascending"), ([20, 30, 30, 40], 2, "duplicate"), ([-1, 20], 0, "outside"),
                                 ([20, 2510], 1, "outside"), ([9, 20], 0, "outside")):
            rc, msg, out = _raw(vf, ix, q, 5, ids, device)
            assert rc == -1 and f"ids[{where}]" in msg and word in msg, (ids, rc, msg)
            assert (out == 7).all(), "a refused call writes nothing"
        rc, msg, out = _raw(vf, ix, q, 5, [10, 20, 2509], device)
        assert rc == 0, msg
        assert np.array_equal(out, _want(oracle, rows, np.array([0, 10, 2499]), q, 5, id_offset=10)[0])
        assert _same(ix.search(q, 5), before)
    with pytest.raises(ValueError, match=r"ids\[1\] = 2500 is outside"):
        vf.index.subset_ids([3, 2500], 2500)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_row_subset_and_pending_slot(vf, oracle, pool):
    import torch
    n, d = 20_000, 768
    rows = pool[:n, :d].astype(np.float16)
    q = pool[20_000:20_008, :d].copy()
    sel = _pick(np.random.default_rng(5), n, 1234, ends=True)
    with vf.DenseIndex(rows) as ix:
        want = ix.search(q, 10, subset=sel)
        assert _same(want, _want(oracle, rows, sel, q, 10))
        rs = ix.row_subset(sel[::-1])
        assert len(rs) == 1234
        for _ in range(10):
            assert _same(ix.search(q, 10, subset=rs), want)
        # a search pending in a slot is not disturbed by a subset search between its begin and end
        dq = torch.from_numpy(q).cuda()
        ids, sc = ix.search_begin(1, dq, 10)
        assert _same(ix.search(q, 10, subset=rs), want)
        assert _same(ix.search(q, 10, subset=sel), want)
        ix.search_end(1)
        torch.cuda.synchronize()
        assert _same((ids.cpu().numpy(), sc.cpu().numpy()), oracle.search(rows, q, 10))


def test_group(vf, oracle, pool):
    n, d = 3001, 100
    rows = pool[:n, :d].astype(np.float16)
    q = pool[20_000:20_004, :d].copy()
    half = (n + 1) // 2       # rows of the first shard
    with vf.DenseIndex(rows, device_ids=[0, 0]) as grp, vf.DenseIndex(rows) as one:
        for name, sel in (("both shards", _pick(np.random.default_rng(2), n, 300, ends=True)),
                          ("the second shard only", np.arange(half + 3, half + 90, 2)),
                          ("the boundary", np.array([half - 2, half - 1, half, half + 1])),
                          ("the first shard whole", np.arange(half))):
            sel = np.asarray(sel, dtype=np.int64)
            got = grp.search(q, 12, subset=sel)
            assert _same(got, one.search(q, 12, subset=sel)), name
            assert _same(got, _want(oracle, rows, sel, q, 12)), name
            assert grp.stats()["path"] == 3 and grp.stats()["subset_rows"] == sel.size
        with pytest.raises(ValueError, match="sharded"):
            grp.row_subset([1, 2])
        from veritasfi_amd import _ffi
        rc = _ffi.search_subset_device(_ffi.lib(), grp._h, 8, 1, 1, 8, 1, 8, 8, None)
        assert rc == -4 and "host-buffer form" in _ffi.last_error()


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_fuzz(vf, oracle):
    """200 seeded cases over n <= 40 000, dtype, d, m, nq <= 8 and k: eight indexes, twenty-five searches each."""
    rng = np.random.default_rng(2026)
    cases = 0
    for kind, d, n in (("f16", 64, 40_000), ("f32", 100, 17_000), ("e4m3", 256, 20_000), ("int8", 48, 33_000),
                       ("f16", 1, 300), ("f32", 17, 16_384), ("e4m3", 33, 5000), ("int8", 200, 16_385)):
        x = rng.standard_normal((n + 8, d), dtype=np.float32)
        rows = _encode(vf, kind, x[:n])
        vals = _values(kind, rows)
        with _make(vf, kind, rows, id_offset=int(rng.integers(0, 1000))) as ix:
            for _ in range(25):
                m = int(rng.choice([rng.integers(0, 70), rng.integers(0, min(n, 2000)), rng.integers(0, n)]))
                nq = int(rng.integers(1, 9))
                k = int(rng.choice([1, 7, 100, 1000, 2048]))
                sel = _pick(rng, n, m)
                got = ix.search(x[n:n + nq], k, subset=sel + ix.id_offset)
                assert _same(got, _want(oracle, vals, sel, x[n:n + nq], k, id_offset=ix.id_offset)), (kind, d, n, m, nq, k)
                cases += 1
    assert cases == 200


# 7 ---------------------------------------------------------------------------------------------------------------------------------
class _Embedder:
    """Texts are row numbers: the embedding of "7" is row 7 of the table."""

    def __init__(self, table):
        self.table = table

    def embed_query(self, text):
        return self.table[int(text)].tolist()


def test_faiss_retriever_subset(vf, oracle, pool):
    n, d = 2000, 100
    emb = pool[:n, :d].copy()
    qtab = pool[20_000:20_010, :d]
    r = vf.FaissRetriever(emb, _Embedder(qtab))
    sel = np.array([1, 500, 501, 1999], dtype=np.int64)
    got = r.invoke(["0", "3", "9"], 3, subset=sel)
    assert _same(got, _want(oracle, emb, sel, qtab[[0, 3, 9]], 3))
    assert _same(r.invoke(["0", "3", "9"], 3), oracle.search(emb, qtab[[0, 3, 9]], 3))
    r.index.close()


@pytest.mark.parametrize("expand", [False, True])
def test_ensemble_where_on_the_gpu(vf, expand):
    """The rule of tests/test_ensemble_where.py with this package's FaissRetriever as the dense legs: ``invoke(where=w)`` over the full
    store equals ``invoke`` over the store of the passing chunks alone (canonical scores do not depend on what else the index holds)."""
    import test_ensemble_where as W
    from veritasfi_amd.ensemble import EnsembleRetriever
    docs, metas, base, titles, t_emb, emb, order, scores, queries = W._world(5)
    where = {"company": ["zeekr", "other"], "year": [2020, 2021, 2023]}
    keep = [i for i, md in enumerate(metas) if W._passes(md, where)]
    new_row = {r: j for j, r in enumerate(keep)}
    kept = [(new_row[r], s) for r, s in zip(order, scores) if r in new_row]
    ts = W.Store(titles, [None] * len(titles), t_emb.tolist())
    kw = dict(faiss_ts_k=2, bm25_k=5, enable_expand=expand, similarity_from_rows=False)
    full = EnsembleRetriever("unused", W.Store(docs, metas, base.tolist()), ts, 6, emb, bm25_retriever=W.Bm25(order, scores), **kw)
    small = EnsembleRetriever("unused", W.Store([docs[i] for i in keep], [metas[i] for i in keep], base[keep].tolist()), ts, 6, emb,
                              bm25_retriever=W.Bm25([r for r, _ in kept], [s for _, s in kept]), **kw)
    try:
        assert 0 < len(keep) < len(metas) and np.array_equal(full.rows_where(where), keep)
        emitted = 0
        for q, hyde in queries:
            got = full.invoke(q, hyde, where=where)
            assert got == small.invoke(q, hyde), q
            assert full.faiss_retriever.index.stats()["path"] == 3 and full.faiss_retriever.index.stats()["subset_rows"] == len(keep)
            emitted += len(got)
        assert emitted > 0
    finally:
        for er in (full, small):
            er.faiss_retriever.index.close()
            er.title_summary_faiss_retriever.index.close()
