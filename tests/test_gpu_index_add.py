"""Appending rows to a live index (``DenseIndex.add`` -> ``vf_index_create*`` with ``VF_INDEX_APPEND``; k_append_rows) on the GPU.

The rule under test: after every append the handle is what a fresh index over all the rows would be.  So every expected value is the
CPU oracle's on the concatenated rows (ids and score bits), and the search path, scan kernel and image use a search reports are those
of a fresh ``DenseIndex`` over the concatenation searched under the same options.  Shapes are the smallest at which each transition
shows: below / across / above the 16 384-row small-corpus limit, a row count that is not a whole number of 32-row tiles, the row-count
floor of the wide-row kernels, the int8 image's threshold (4M rows), a group of two shards."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
KINDS = ("f32", "f16", "e4m3", "int8")


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()
    return m


@pytest.fixture(scope="module")
def pool():
    """One block of N(0, 1) values every test cuts its rows from (generated once)."""
    return np.random.default_rng(1313).standard_normal((45_000, 1536), dtype=np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _encode(vf, kind, x):
    """fp32 values -> rows as an index of `kind` takes them."""
    import torch
    if kind == "f32":
        return np.ascontiguousarray(x, dtype=np.float32)
    if kind == "f16":
        return x.astype(np.float16)
    if kind == "e4m3":
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return vf.quantize_int8(x)


def _values(kind, rows):
    """The values the index scores: what the oracle is given (fp16 for fp16 / e4m3 rows -- exact --, fp32 otherwise)."""
    from oracle import ref_numpy
    if kind == "e4m3":
        return ref_numpy.decode_e4m3(rows).astype(np.float16)
    if kind == "int8":
        return rows.astype(np.float32)
    return rows


def _make(vf, kind, rows, **kw):
    return vf.DenseIndex.from_e4m3(rows, **kw) if kind == "e4m3" else vf.DenseIndex(rows, **kw)


def _check(vf, oracle, ix, kind, rows, q, k, opts=(), what=""):
    """ix (after its appends) against the oracle on `rows` (everything it holds) and against a fresh index over them under `opts`."""
    for name, value in opts:
        ix.set_option(name, value)
    got = ix.search(q, k)
    st = ix.stats()
    with _make(vf, kind, rows) as fresh:
        for name, value in opts:
            fresh.set_option(name, value)
        ref = fresh.search(q, k)
        st0 = fresh.stats()
    for key in ("path", "scan_kernel", "scan_image"):
        assert st[key] == st0[key], (what, key, st, st0)
    want = oracle.search(_values(kind, rows), q, k)
    assert _same(ref, want), (what, "the fresh index differs from the oracle")
    assert _same(got, want), (what, st)
    assert ix.n == len(rows)
    return st


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_small_path(vf, oracle, pool, kind):
    d, n0 = 100, 1000
    x = pool[:1538, :d].copy()
    x[1004] = 0.0                      # a zero row among the appended ones (second append, row 3)
    x[1008] = x[5]                     # ... and a copy of old row 5 (second append, row 7)
    rows = _encode(vf, kind, x)
    vals = np.asarray(_values(kind, rows), dtype=np.float32)
    q = pool[40_000:40_006, :d].copy()
    q[0] = vals[1000]                  # the first query is a copy of the one row of the first append
    q[1] = vals[5]
    q[2] = vals[1537]                  # ... and of the last row of the last append
    with _make(vf, kind, rows[:n0]) as ix:
        n = n0
        for m in (1, 37, 500):
            first = ix.add(rows[n:n + m])
            assert first == n and ix.n == n + m
            n += m
            for k in (10, n + 50):
                st = _check(vf, oracle, ix, kind, rows[:n], q, k, what=f"{kind} +{m} k={k}")
                assert st["path"] == 0
            ids, sc = ix.search(q, n + 50)
            assert (ids[:, n:] == -1).all() and (sc[:, n:] == -FLT_MAX).all()
            assert ids[0, 0] == 1000                                   # the planted row takes rank 1 under its new id
            if n > 1008:
                assert (sc[ids == 1004] == 0.0).all()                  # the zero row scores 0
                assert ids[1, 0] == 5 and ids[1, 1] == 1008 and _bits(sc[1, 0]) == _bits(sc[1, 1])   # the tie goes to the older id
            if n == 1538:
                assert ids[2, 0] == 1537
        pick = np.array([0, 5, 999, 1000, 1004, 1008, 1037, 1038, 1537, 5], dtype=np.int64)
        assert np.array_equal(_bits(ix.cosine_matrix_rows(pick)), _bits(oracle.cosine(vals[pick], vals[pick])))
        n_info = ctypes.c_int64(0)
        from veritasfi_amd import _ffi
        _ffi.check(_ffi.lib().vf_index_info(ix._h, ctypes.byref(n_info), None, None, None))
        assert n_info.value == 1538


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [("f16", 128), ("f32", 100)])
def test_crossing_the_small_corpus_limit(vf, oracle, pool, kind, d):
    """16 379 rows + 10: the handle was built without the fused scan's operands (the round-4 fault on force_path = 1); after the append
    it has them.  fp16 rows of 128 elements are scanned in place, fp32 rows of 100 through an owned, scaled copy."""
    n0, m = 16_379, 10
    rows = _encode(vf, kind, pool[:n0 + m, :d])
    vals = np.asarray(_values(kind, rows), dtype=np.float32)
    q = pool[40_000:40_005, :d].copy()
    q[0], q[1] = vals[n0 + m - 1], vals[0]
    with _make(vf, kind, rows[:n0]) as ix:
        st = _check(vf, oracle, ix, kind, rows[:n0], q, 10, what="before")
        assert st["path"] == 0
        assert ix.add(rows[n0:]) == n0
        for fp in (-1, 1, 2):
            st = _check(vf, oracle, ix, kind, rows, q, 10, opts=(("force_path", fp),), what=f"{kind} force_path={fp}")
            assert st["path"] == (1 if fp < 0 else fp)
        ids, _ = ix.search(q, 10)
        assert ids[0, 0] == n0 + m - 1 and ids[1, 0] == 0


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [("f16", 768), ("f32", 100), ("e4m3", 1024), ("int8", 768)])
def test_fused_path_each_dtype(vf, oracle, pool, kind, d):
    import torch
    n0 = 20_037                                                        # not a whole number of 32-row tiles
    steps = (100, 100, 100, 5000)
    n1 = n0 + sum(steps)
    rows = _encode(vf, kind, pool[:n1, :d])
    vals = np.asarray(_values(kind, rows), dtype=np.float32)
    opts = (("force_path", 1),) + ((("scan_image", 2),) if kind == "int8" else ())
    dev = torch.device("cuda", 0)
    if kind == "f16":                                                  # borrowed: the handle reads the tensor until its first append
        t = torch.from_numpy(rows[:n0]).to(dev)
        ix = vf.DenseIndex(t)
    else:
        ix = _make(vf, kind, rows[:n0])
    with ix:
        for name, value in opts:
            ix.set_option(name, value)
        n = n0
        for i, m in enumerate(steps):
            if i < 3:
                first = ix.add(rows[n:n + m])
            else:                                                      # the last one through the device entry point
                blk = torch.from_numpy(rows[n:n + m]).to(dev)
                first = ix.add(blk.view(torch.float8_e4m3fn) if kind == "e4m3" else blk)
                del blk
            assert first == n
            n += m
            if i == 0 and kind == "f16":
                t.zero_()                                              # the handle holds its own copy now: the tensor may change and go
                del t
                torch.cuda.empty_cache()
            if i == 0:
                q = pool[40_000:40_005, :d].copy()
                q[0], q[1], q[2] = vals[n0], vals[n - 1], vals[0]
                _check(vf, oracle, ix, kind, rows[:n], q, 100, opts=opts, what=f"{kind} after the first append")
        for nq, k in ((5, 100), (65, 100), (3, 2048)):
            q = pool[40_000:40_000 + nq, :d].copy()
            q[0], q[1], q[2] = vals[n0], vals[n1 - 1], vals[0]         # planted on the first and the last appended row and on old row 0
            st = _check(vf, oracle, ix, kind, rows, q, k, opts=opts, what=f"{kind} nq={nq} k={k}")
            assert st["path"] == 1
            if kind == "int8" and (nq, k) == (5, 100):
                assert st["scan_image"] == 1, st
            ids, _ = ix.search(q, k)
            assert ids[0, 0] == n0 and ids[1, 0] == n1 - 1 and ids[2, 0] == 0


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int8", "e4m3"])
def test_wide_rows_across_their_floor(vf, oracle, pool, kind):
    """Rows of 2560 elements take k_scan_ksplit8 / k_scan_ksplit8i from 32 768 rows: 32 700 + 100 crosses that count."""
    n0, m, d = 32_700, 100, 2560
    rng = np.random.default_rng(44)
    if kind == "int8":
        rows = rng.integers(-127, 128, size=(n0 + m, d), dtype=np.int8)
    else:
        rows = _encode(vf, kind, np.hstack([pool[:n0 + m, :1536], pool[8000:8000 + n0 + m, :1024]]))
    vals = _values(kind, rows)
    q = rng.standard_normal((4, d)).astype(np.float32)
    q[0], q[1] = vals[n0 + m - 1], vals[n0]
    with _make(vf, kind, rows[:n0]) as ix:
        ix.search(q, 100)
        assert ix.stats()["path"] == 2
        assert ix.add(rows[n0:]) == n0
        st = _check(vf, oracle, ix, kind, rows, q, 100, what=kind)
        assert st["path"] == 1 and st["scan_kernel"] == 7, st
        ids, _ = ix.search(q, 100)
        assert ids[0, 0] == n0 + m - 1 and ids[1, 0] == n0


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_fp16_image_appears_at_its_threshold_and_goes_with_a_row_it_cannot_hold(vf, oracle):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    n0, d = 3_999_900, 768
    host = np.empty((n0 + 201, d), np.float16)
    c = bench.make_shard(torch, 0, n0, d, dev, "f16")
    host[:n0] = c.cpu().numpy()
    new = bench.make_shard(torch, 90 * bench.GEN_CHUNK, 90 * bench.GEN_CHUNK + 200, d, dev, "f16")
    host[n0:n0 + 200] = new.cpu().numpy()
    bad = np.full(d, 0.003, np.float16)                               # quantises to code 0 beside the 1.0: residual ~ 0.083 > 1 / 64
    bad[0] = 1.0
    host[n0 + 200] = bad
    q = np.random.default_rng(55).standard_normal((64, d)).astype(np.float32)
    q[0], q[1] = host[n0 + 199], host[n0 + 3]                          # two of the first four planted on appended rows
    with vf.DenseIndex(c) as ix:
        ix.search(q, 100)
        assert ix.stats()["scan_image"] == 0                           # below the threshold: no image
        assert ix.add(new) == n0
        del c, new
        torch.cuda.empty_cache()
        got = ix.search(q, 100)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_image"] == 1, st
        ix.set_option("scan_image", 0)
        assert _same(got, ix.search(q, 100)) and ix.stats()["scan_image"] == 0
        ix.set_option("scan_image", 1)
        want = oracle.search(host[:n0 + 200], q[:4], 100)
        assert np.array_equal(got[0][:4], want[0]) and np.array_equal(_bits(got[1][:4]), _bits(want[1]))
        assert got[0][0, 0] == n0 + 199 and got[0][1, 0] == n0 + 3
        assert ix.add(bad[None, :]) == n0 + 200
        q[1] = bad                                                     # ... now on the row no image can hold
        got = ix.search(q, 100)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_image"] == 0, st           # a fresh build would have refused the image
        assert got[0][1, 0] == n0 + 200
        ix.set_option("scan_image", 0)
        assert _same(got, ix.search(q, 100))
        want = oracle.search(host, q[:4], 100)
        assert np.array_equal(got[0][:4], want[0]) and np.array_equal(_bits(got[1][:4]), _bits(want[1]))


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_group_appends_to_its_last_shard(vf, oracle, pool):
    n0, m, d = 40_000, 300, 768
    rows = _encode(vf, "f16", pool[:n0 + m, :d])
    q = pool[44_000:44_006, :d].copy()
    q[0] = rows[n0 + m - 1].astype(np.float32)
    with vf.DenseIndex(rows[:n0], device_ids=[0, 0]) as ix:
        assert ix.add(rows[n0:]) == n0 and ix.n == n0 + m
        assert ix.shard_devices() == [0, 0]
        for k in (100, 2048):
            got = ix.search(q, k)
            assert _same(got, oracle.search(rows, q, k)), k
        assert got[0][0, 0] == n0 + m - 1
        new_ids = np.arange(n0, n0 + m)
        hit = ix.search(rows[n0:].astype(np.float32), 1)[0][:, 0]
        assert np.array_equal(hit, new_ids)                            # ids 40 000 .. 40 299, one contiguous range
        pick = np.array([0, 19_999, 20_000, n0 - 1, n0, n0 + m - 1], dtype=np.int64)
        v = rows[pick].astype(np.float32)
        assert np.array_equal(_bits(ix.cosine_matrix_rows(pick)), _bits(oracle.cosine(v, v)))


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_append_is_refused_while_a_search_is_pending(vf, oracle, pool):
    import torch
    n0, m, d = 20_037, 64, 768
    rows = _encode(vf, "f16", pool[:n0 + m, :d])
    q = pool[44_000:44_008, :d].copy()
    tq = torch.from_numpy(q).to("cuda:0")
    with vf.DenseIndex(rows[:n0]) as ix:
        ids, sc = ix.search_begin(0, tq, 100)
        with pytest.raises(RuntimeError, match="search pending"):
            ix.add(rows[n0:])
        assert ix.n == n0
        ix.search_end(0)
        torch.cuda.synchronize()
        assert _same((ids.cpu().numpy(), sc.cpu().numpy()), oracle.search(rows[:n0], q, 100))
        assert ix.add(rows[n0:]) == n0
        assert _same(ix.search(q, 100), oracle.search(rows, q, 100))


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_reserve_keeps_appends_from_allocating(vf, oracle, pool):
    import torch
    n0, d = 20_037, 768
    rows = _encode(vf, "f16", pool[:n0 + 40 * 500, :d])
    q = pool[44_000:44_016, :d].copy()
    with vf.DenseIndex(rows[:n0]) as ix:
        ix.reserve(60_000)
        ix.reserve(10)                                                 # at or below n: nothing
        ix.search(q, 100)                                              # the warm-up: the slot's buffers exist from here on
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        n = n0
        for _ in range(40):
            ix.add(rows[n:n + 500])
            n += 500
        torch.cuda.synchronize()
        fall = free0 - torch.cuda.mem_get_info()[0]
        print(f"free memory fell by {fall} bytes over forty appends; one copy of the rows was {n0 * d * 2} bytes at the start")
        assert fall < n0 * d * 2, fall                                 # less than one copy of the row array, even at its smallest
        assert n == len(rows) and _same(ix.search(q, 100), oracle.search(rows, q, 100))


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_index_as_it_was(vf, oracle, pool):
    import torch
    from veritasfi_amd import _ffi
    n0, d = 3000, 100
    rows = _encode(vf, "f16", pool[:n0 + 10, :d])
    q = pool[44_000:44_004, :d].copy()
    L = _ffi.lib()
    with vf.DenseIndex(rows[:n0]) as ix:
        with pytest.raises(TypeError):
            ix.add(rows[n0:].astype(np.float32))                       # never cast across widths
        with pytest.raises(TypeError):
            ix.add(vf.quantize_int8(rows[n0:]))
        with pytest.raises(ValueError):
            ix.add(rows[n0:, :64])
        h = _ffi.vp(ix._h.value)
        f32 = np.zeros((2, d), np.float32)
        rc = L.vf_index_create(ctypes.byref(h), f32.ctypes.data, 2, d, _ffi.VF_INDEX_APPEND | _ffi.VF_DTYPE_F32, 0, 0)
        assert rc == -1 and "dtype" in _ffi.last_error() and h.value == ix._h.value
        rc = L.vf_index_create(ctypes.byref(h), rows.ctypes.data, 2, d + 1, _ffi.VF_INDEX_APPEND | _ffi.VF_DTYPE_F16, 0, 0)
        assert rc == -1 and h.value == ix._h.value
        rc = L.vf_index_create(ctypes.byref(h), rows.ctypes.data, 2, d, _ffi.VF_INDEX_APPEND | _ffi.VF_DTYPE_F16, 1, 0)
        assert rc == -1 and "device" in _ffi.last_error() and h.value == ix._h.value
        if torch.cuda.device_count() >= 2:                             # rows that live on another device
            with pytest.raises(RuntimeError, match="device"):
                ix.add(torch.from_numpy(rows[n0:]).to("cuda:1"))
        with pytest.raises(RuntimeError, match=r"rc=-4"):
            ix.reserve(2 ** 32)
        assert ix.add(rows[n0:n0]) == n0 and ix.n == n0                # no rows: nothing happens
        assert _same(ix.search(q, 10), oracle.search(rows[:n0], q, 10))
        assert ix.add(rows[n0:]) == n0
        assert _same(ix.search(q, 10), oracle.search(rows, q, 10))


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_seeded_random_sequences(vf, oracle, pool):
    seed = 20_261_019
    rng = np.random.default_rng(seed)
    for draw in range(24):
        kind = KINDS[int(rng.integers(4))]
        d = int(rng.choice([64, 100, 768, 1024, 1536]))
        big = bool(rng.integers(2))
        n0 = int(rng.integers(16_390, 20_000)) if big else int(rng.integers(200, 16_000))
        cap = 3000 if d >= 768 else 4000
        steps = [int(rng.integers(1, cap + 1)) for _ in range(int(rng.integers(2, 7)))]
        if not big and draw % 3 == 0:
            steps[-1] = max(steps[-1], 16_385 - n0 - sum(steps[:-1]))  # some small starts end above the limit
            steps[-1] = min(steps[-1], 44_000 - n0 - sum(steps[:-1]))
        n1 = n0 + sum(steps)
        nq, k = int(rng.integers(1, 71)), int(rng.integers(1, 257))
        fp = int(rng.choice([-1, 1, 2])) if n1 > 16_384 else int(rng.choice([-1, 0, 2]))
        reserve = bool(rng.integers(2))
        what = f"seed={seed} draw={draw}: {kind} d={d} n0={n0} steps={steps} nq={nq} k={k} force_path={fp} reserve={reserve}"
        rows = _encode(vf, kind, pool[:n1, :d])
        q = pool[44_000:44_000 + nq, :d].copy()
        q[0] = np.asarray(_values(kind, rows[n1 - 1:n1]), dtype=np.float32)[0]
        with _make(vf, kind, rows[:n0]) as ix:
            if reserve:
                ix.reserve(n0 + sum(steps) // 2)
            n = n0
            for m in steps:
                assert ix.add(rows[n:n + m]) == n, what
                n += m
            ix.set_option("force_path", fp)
            got = ix.search(q, k)
            st = ix.stats()
            want = oracle.search(_values(kind, rows), q, k)
            assert st["path"] == (fp if fp >= 0 else (1 if n1 > 16_384 else 0)), (what, st)
            assert _same(got, want), (what, st)
