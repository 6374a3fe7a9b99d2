"""Removing rows from a live index (``DenseIndex.remove`` -> ``vf_index_create`` with ``VF_INDEX_REMOVE``; k_compact_rows) on the GPU.

The rule under test: after every removal the handle is what a fresh index over the remaining rows, in their order, would be.  So every
expected value is the CPU oracle's on ``np.delete(rows, removed, 0)`` (ids and score bits), and the search path, scan kernel and image
use a search reports are those of a fresh ``DenseIndex`` over the same rows searched under the same options.  The index under test gets
its options ONCE, before its first removal: what it holds afterwards is the removal's doing.  Shapes are the smallest at which each
transition shows: below / across / above the 16 384-row small-corpus limit, row sizes that take the 16-byte and the narrower copy, many
chunks and one, the row-count floor of the wide-row kernels, the int8 image's threshold (4M rows), a group of two shards."""
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
    return np.random.default_rng(1414).standard_normal((45_000, 1536), dtype=np.float32)


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


def _with(ix, opts):
    for name, value in opts:
        ix.set_option(name, value)
    return ix


def _check(vf, oracle, ix, kind, rows, q, k, opts=(), what=""):
    """ix (after its removals; its options are already set) against the oracle on `rows` (everything it still holds) and against a fresh
    index over them under `opts`."""
    got = ix.search(q, k)
    st = ix.stats()
    with _make(vf, kind, rows) as fresh:
        ref = _with(fresh, opts).search(q, k)
        st0 = fresh.stats()
    for key in ("path", "scan_kernel", "scan_image"):
        assert st[key] == st0[key], (what, key, st, st0)
    want = oracle.search(_values(kind, rows), q, k)
    assert _same(ref, want), (what, "the fresh index differs from the oracle")
    assert _same(got, want), (what, st)
    assert ix.n == len(rows)
    n_info = ctypes.c_int64(0)
    from veritasfi_amd import _ffi
    _ffi.check(_ffi.lib().vf_index_info(ix._h, ctypes.byref(n_info), None, None, None))
    assert n_info.value == len(rows)
    return st


def _remove(ix, cur, gone):
    """Remove `gone` (current ids) from the index and from the host copy; returns the new host copy."""
    gone = np.asarray(gone, dtype=np.int64)
    distinct = np.unique(gone)
    n = ix.n
    assert ix.remove(gone) == distinct.size and ix.n == n - distinct.size
    return np.delete(cur, distinct, 0)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_small_path(vf, oracle, pool, kind):
    d = 100
    x = pool[:1538, :d].copy()
    x[1008] = x[5]                     # a copy of row 5: once row 5 is gone the copy answers, under the id the shift gives it
    cur = _encode(vf, kind, x)
    q = pool[40_000:40_006, :d].copy()
    q[0] = np.asarray(_values(kind, cur), dtype=np.float32)[5]
    with _make(vf, kind, cur) as ix:
        ids, sc = ix.search(q, 2)
        assert ids[0, 0] == 5 and ids[0, 1] == 1008 and _bits(sc[0, 0]) == _bits(sc[0, 1])
        steps = (("row 5", [5]), ("row 0", [0]), ("the last row", [1535]), ("a middle run", np.arange(500, 600)),
                 ("a list with duplicates", [10, 10, 20, 1000, 20, 1431]))
        for i, (name, gone) in enumerate(steps):
            cur = _remove(ix, cur, gone)
            n = len(cur)
            for k in (10, n + 50):
                st = _check(vf, oracle, ix, kind, cur, q, k, what=f"{kind} - {name} k={k}")
                assert st["path"] == 0
            ids, sc = ix.search(q, n + 50)
            assert (ids[:, n:] == -1).all() and (sc[:, n:] == -FLT_MAX).all() and (ids[:, :n] >= 0).all()
            assert ids[0, 0] == (1007, 1006, 1006, 906, 904)[i]   # the copy, under its id of the moment
        pick = np.array([0, 4, 5, 498, 499, 500, n - 1, 4], dtype=np.int64)
        vals = np.asarray(_values(kind, cur), dtype=np.float32)
        assert np.array_equal(_bits(ix.cosine_matrix_rows(pick)), _bits(oracle.cosine(vals[pick], vals[pick])))


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [100, 768])
def test_crossing_the_small_corpus_limit_downward(vf, oracle, pool, kind, d):
    """16 484 rows - 200 leaves 16 284: the scan copy goes and the cache of normalised rows is built, as a fresh build has it.
    16 484 - 50 stays above the limit and keeps the fused scan's operands."""
    n0 = 16_484
    rows = _encode(vf, kind, pool[:n0, :d])
    q = pool[40_000:40_005, :d].copy()
    q[0], q[1] = np.asarray(_values(kind, rows[n0 - 1:]), dtype=np.float32)[0], np.asarray(_values(kind, rows[1:2]), dtype=np.float32)[0]
    for count, path in ((200, 0), (50, 1)):
        gone = np.unique(np.concatenate([[0], np.linspace(3, n0 - 2, count - 1).astype(np.int64)]))
        assert gone.size == count
        with _make(vf, kind, rows) as ix:
            ix.search(q, 10)
            assert ix.stats()["path"] == 1
            cur = _remove(ix, rows, gone)
            st = _check(vf, oracle, ix, kind, cur, q, 10, what=f"{kind} d={d} -{count}")
            assert st["path"] == path, st
            ids, _ = ix.search(q, 10)
            assert ids[0, 0] == n0 - 1 - count and ids[1, 0] == 0      # the last row and old row 1 under their new ids
            ix.set_option("force_path", 2)
            st = _check(vf, oracle, ix, kind, cur, q, 10, opts=(("force_path", 2),), what=f"{kind} d={d} -{count} force_path=2")
            assert st["path"] == 2, st


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk_rows", [1000, 0])
@pytest.mark.parametrize("kind,d", [(k, d) for d in (100, 768) for k in KINDS] + [("e4m3", 101), ("int8", 101)])
def test_fused_path(vf, oracle, pool, kind, d, chunk_rows):
    """40 000 rows; rows of 400 / 200 / 100 / 101 bytes (d = 100, 101) and of 3072 / 1536 / 768 (d = 768) through the mover, in 40
    chunks of 1000 destination rows and in one."""
    n0 = 40_000
    cur = _encode(vf, kind, pool[:n0, :d])
    opts = (("force_path", 1),) + ((("scan_image", 2),) if kind == "int8" else ())
    rng = np.random.default_rng(33)
    steps = (("row 0 alone", [0]),                                                     # a shift of one row through everything
             ("the last row alone", [n0 - 2]),                                         # nothing moves
             ("37 rows and a run across a chunk boundary", np.concatenate([[100], np.arange(1090, 1121), rng.choice(np.arange(2000, 39_000), 5, replace=False)])),
             ("1000 scattered rows", rng.choice(39_961, 1000, replace=False)))
    with _with(_make(vf, kind, cur), opts + (("compact_chunk_rows", chunk_rows),)) as ix:
        for name, gone in steps:
            cur = _remove(ix, cur, gone)
            n = len(cur)
            vals = np.asarray(_values(kind, cur), dtype=np.float32)
            q = pool[40_000:40_005, :d].copy()
            q[0], q[1], q[2] = vals[0], vals[n - 1], vals[n // 2]
            st = _check(vf, oracle, ix, kind, cur, q, 100, opts=opts, what=f"{kind} d={d} chunk_rows={chunk_rows} - {name}")
            assert st["path"] == 1, st
            if kind == "int8" and d == 768:
                assert st["scan_image"] == 1, st
            ids, _ = ix.search(q, 100)
            assert ids[0, 0] == 0 and ids[1, 0] == n - 1 and ids[2, 0] == n // 2
        assert len(cur) == n0 - 1 - 1 - 37 - 1000 and len(cur) % 32 != 0
        q = pool[40_000:40_065, :d].copy()
        _check(vf, oracle, ix, kind, cur, q, 100, opts=opts, what=f"{kind} d={d} 65 queries")
        _check(vf, oracle, ix, kind, cur, q[:3], 2048, opts=opts, what=f"{kind} d={d} k=2048")


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_wide_rows_across_their_floor(vf, oracle):
    """int8 rows of 2560 elements take k_scan_ksplit8i from 32 768 rows: 32 868 - 200 falls below that count."""
    n0, d = 32_868, 2560
    rng = np.random.default_rng(44)
    rows = rng.integers(-127, 128, size=(n0, d), dtype=np.int8)
    gone = np.unique(np.concatenate([[0, n0 - 1], rng.choice(np.arange(2, n0 - 2), 198, replace=False)]))
    q = rng.standard_normal((4, d)).astype(np.float32)
    q[0], q[1] = rows[n0 - 2], rows[1]
    with _make(vf, "int8", rows) as ix:
        ix.search(q, 100)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_kernel"] == 7, st
        cur = _remove(ix, rows, gone)
        st = _check(vf, oracle, ix, "int8", cur, q, 100, what="int8 2560")
        assert st["path"] == 2, st
        ids, _ = ix.search(q, 100)
        assert ids[0, 0] == n0 - 201 and ids[1, 0] == 0


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_fp16_image_is_rebuilt_above_its_threshold_and_goes_below_it(vf, oracle):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    n0, d = 4_000_100, 768
    c = bench.make_shard(torch, 0, n0, d, dev, "f16")
    host = c.cpu().numpy()
    rng = np.random.default_rng(55)
    q = rng.standard_normal((64, d)).astype(np.float32)
    keep = np.ones(n0, dtype=bool)
    with vf.DenseIndex(c) as ix:
        ix.search(q, 100)
        assert ix.stats()["scan_image"] == 1
        gone = np.unique(np.concatenate([[0, n0 - 1], rng.choice(np.arange(1, n0 - 1), 48, replace=False)]))
        assert ix.remove(gone) == 50 and ix.n == n0 - 50
        assert torch.equal(c[:1000], torch.from_numpy(host[:1000]).to(dev))    # the borrowed tensor was not written
        del c
        torch.cuda.empty_cache()
        keep[gone] = False
        cur = host[keep]
        q[0], q[1] = cur[0], cur[-1]                                   # old row 1 and the old second-to-last row
        got = ix.search(q, 100)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_image"] == 1, st           # still above the threshold: an image of the rows that remain
        want = oracle.search(cur, q[:4], 100)
        assert np.array_equal(got[0][:4], want[0]) and np.array_equal(_bits(got[1][:4]), _bits(want[1]))
        assert got[0][0, 0] == 0 and got[0][1, 0] == n0 - 51
        ix.set_option("scan_image", 0)
        assert _same(got, ix.search(q, 100)) and ix.stats()["scan_image"] == 0
        ix.set_option("scan_image", 1)
        left = np.flatnonzero(keep)
        gone2 = rng.choice(left.size, 200, replace=False)
        assert ix.remove(gone2) == 200 and ix.n == n0 - 250
        keep[left[gone2]] = False
        cur = host[keep]
        q[0], q[1] = cur[0], cur[-1]
        got = ix.search(q, 100)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_image"] == 0, st           # below 4M rows a fresh build keeps no image
        want = oracle.search(cur, q[:4], 100)
        assert np.array_equal(got[0][:4], want[0]) and np.array_equal(_bits(got[1][:4]), _bits(want[1]))
        assert got[0][0, 0] == 0 and got[0][1, 0] == len(cur) - 1


def test_fp16_image_appears_when_the_row_it_could_not_hold_leaves(vf, oracle):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    n0, d, at = 4_000_001, 768, 1_234_567
    c = bench.make_shard(torch, 0, n0, d, dev, "f16")
    bad = np.full(d, 0.003, np.float16)                               # quantises to code 0 beside the 1.0: residual ~ 0.083 > 1 / 64
    bad[0] = 1.0
    c[at] = torch.from_numpy(bad).to(dev)
    host = c.cpu().numpy()
    q = np.random.default_rng(56).standard_normal((64, d)).astype(np.float32)
    q[0], q[1] = bad, host[at + 1]
    with vf.DenseIndex(c) as ix:
        got = ix.search(q, 100)
        assert ix.stats()["scan_image"] == 0 and got[0][0, 0] == at     # a fresh build refuses the image over that row
        assert ix.remove([at]) == 1
        del c
        torch.cuda.empty_cache()
        cur = np.delete(host, at, 0)
        got = ix.search(q, 100)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_image"] == 1, st           # ... and builds one without it
        assert got[0][1, 0] == at
        want = oracle.search(cur, q[:4], 100)
        assert np.array_equal(got[0][:4], want[0]) and np.array_equal(_bits(got[1][:4]), _bits(want[1]))
        ix.set_option("scan_image", 0)
        assert _same(got, ix.search(q, 100)) and ix.stats()["scan_image"] == 0


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_group_removes_in_every_shard(vf, oracle, pool):
    n0, d = 40_000, 768
    rows = _encode(vf, "f16", pool[:n0, :d])
    q = pool[44_000:44_006, :d].copy()
    gone = np.array([0, 5, 19_999, 20_000, 20_001, 39_999, 31_000, 5], dtype=np.int64)
    with vf.DenseIndex(rows, device_ids=[0, 0]) as ix:
        with pytest.raises(RuntimeError, match=r"rc=-4"):
            ix.remove(np.arange(20_000, 40_000))                       # would empty the second shard
        with pytest.raises(RuntimeError, match=r"rc=-4"):
            ix.remove(np.concatenate([[39_999], np.arange(0, 20_000)]))   # ... the first: nothing goes, not even the id of the other shard
        assert ix.n == n0 and _same(ix.search(q, 100), oracle.search(rows, q, 100))
        cur = _remove(ix, rows, gone)
        assert ix.n == n0 - 7 and ix.shard_devices() == [0, 0]
        q[0], q[1] = cur[19_996], cur[19_997]                          # the last row of the first shard, the first of the second
        for k in (100, 2048):
            got = ix.search(q, k)
            assert _same(got, oracle.search(cur, q, k)), k
        assert got[0][0, 0] == 19_996 and got[0][1, 0] == 19_997
        sel = np.unique(np.concatenate([np.arange(0, len(cur), 7), [19_995, 19_996, 19_997, 19_998, len(cur) - 1]]))
        hit = ix.search(cur[sel].astype(np.float32), 1)[0][:, 0]
        assert np.array_equal(hit, sel)                                # ids 0 .. n - 1, one contiguous range: each row finds itself
        pick = np.array([0, 19_996, 19_997, len(cur) - 1, 3, 30_000], dtype=np.int64)
        v = cur[pick].astype(np.float32)
        assert np.array_equal(_bits(ix.cosine_matrix_rows(pick)), _bits(oracle.cosine(v, v)))
        first = ix.add(rows[:3])                                       # appends still go behind the last id
        assert first == n0 - 7 and _same(ix.search(q, 100), oracle.search(np.concatenate([cur, rows[:3]]), q, 100))


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_removal_is_refused_while_a_search_is_pending(vf, oracle, pool):
    import torch
    n0, d = 20_037, 768
    rows = _encode(vf, "f16", pool[:n0, :d])
    q = pool[44_000:44_008, :d].copy()
    tq = torch.from_numpy(q).to("cuda:0")
    with vf.DenseIndex(rows) as ix:
        ids, sc = ix.search_begin(0, tq, 100)
        with pytest.raises(RuntimeError, match="search pending"):
            ix.remove([3])
        assert ix.n == n0
        ix.search_end(0)
        torch.cuda.synchronize()
        assert _same((ids.cpu().numpy(), sc.cpu().numpy()), oracle.search(rows, q, 100))
        cur = _remove(ix, rows, [3])
        assert _same(ix.search(q, 100), oracle.search(cur, q, 100))


def test_errors_leave_the_index_as_it_was(vf, oracle, pool):
    from veritasfi_amd import _ffi
    n0, d = 3000, 100
    rows = _encode(vf, "f16", pool[:n0, :d])
    q = pool[44_000:44_004, :d].copy()
    L = _ffi.lib()
    with vf.DenseIndex(rows, id_offset=1000) as ix:
        for bad in ([999], [4000], [1000, -1], [1500, 2 ** 40]):
            with pytest.raises(ValueError, match=r"ids\[\d\]"):
                ix.remove(bad)
        h = _ffi.vp(ix._h.value)

        def call(ids, n_ids, d_, dev=0, dtype=_ffi.VF_INDEX_REMOVE):
            arr = None if ids is None else np.asarray(ids, dtype=np.int64)
            rc = L.vf_index_create(ctypes.byref(h), None if arr is None else arr.ctypes.data, n_ids, d_, dtype, dev, 0)
            assert h.value == ix._h.value
            return rc, _ffi.last_error()

        rc, msg = call([1000, 1001, 4000], 3, d)                       # strict: a stale id removes nothing and names its position
        assert rc == -1 and "ids[2] = 4000" in msg, (rc, msg)
        rc, msg = call([999], 1, d)
        assert rc == -1 and "ids[0] = 999" in msg, (rc, msg)
        rc, msg = call([0], 1, d)                                      # ids are global: id_offset .. id_offset + n - 1
        assert rc == -1 and "ids[0] = 0" in msg, (rc, msg)
        assert call([1000], 1, d + 1)[0] == -1 and call([1000], 1, d, dev=1)[0] == -1
        assert call(None, 1, d)[0] == -1 and call([1000], -1, d)[0] == -1
        assert call(None, 0, d)[0] == 0 and ix.remove([]) == 0         # no ids: nothing happens
        h2 = _ffi.vp(ix._h.value)                                      # with any other bit the value is a dtype nobody knows: a create call, refused
        one = np.array([1000], dtype=np.int64)
        rc = L.vf_index_create(ctypes.byref(h2), one.ctypes.data, 1, d, _ffi.VF_INDEX_REMOVE | _ffi.VF_DTYPE_F16, 0, 0)
        assert rc == -1 and "unknown dtype" in _ffi.last_error()
        assert ix.n == n0 and _same(ix.search(q, 10), _shift(oracle.search(rows, q, 10), 1000))
        assert ix.remove([1000 + 7, 1000 + 2999]) == 2
        assert _same(ix.search(q, 10), _shift(oracle.search(np.delete(rows, [7, 2999], 0), q, 10), 1000))


def _shift(res, off):
    ids, sc = res
    return np.where(ids >= 0, ids + off, ids), sc


def test_a_plain_index_may_become_empty_and_grow_again(vf, oracle, pool):
    d = 100
    for kind, n0 in (("f16", 300), ("int8", 16_500)):
        rows = _encode(vf, kind, pool[:n0, :d])
        q = pool[44_000:44_004, :d].copy()
        with _make(vf, kind, rows) as ix:
            assert ix.remove(np.arange(n0)[::-1]) == n0 and ix.n == 0
            ids, sc = ix.search(q, 5)
            assert (ids == -1).all() and (sc == -FLT_MAX).all()
            assert ix.add(rows[:0]) == 0 and ix.add(rows[10:200]) == 0 and ix.n == 190
            _check(vf, oracle, ix, kind, rows[10:200], q, 10, what=f"{kind}: emptied, then 190 rows")
            cur = _remove(ix, rows[10:200], [0, 189])
            _check(vf, oracle, ix, kind, cur, q, 10, what=f"{kind}: ... minus two")


# 8 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0,d", [(20_037, 768), (3000, 100)])
def test_a_borrowed_tensor_is_never_written(vf, oracle, pool, n0, d):
    import torch
    rows = _encode(vf, "f16", pool[:n0, :d])
    q = pool[44_000:44_004, :d].copy()
    t = torch.from_numpy(rows).to("cuda:0")
    with vf.DenseIndex(t) as ix:
        cur = _remove(ix, rows, [0, 17, n0 // 2])
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint16), rows.view(np.uint16))
        t.zero_()                                                      # the handle holds its own copy now: the tensor may change and go
        del t
        torch.cuda.empty_cache()
        _check(vf, oracle, ix, "f16", cur, q, 10, what="after the tensor has gone")


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_seeded_random_sequences(vf, oracle, pool):
    seed = 20_261_020
    rng = np.random.default_rng(seed)
    for draw in range(20):
        kind = KINDS[int(rng.integers(4))]
        d = int(rng.choice([64, 100, 101, 768, 1024]))
        n0 = int(rng.integers(16_390, 19_000)) if draw % 2 else int(rng.integers(14_000, 16_380))
        chunk_rows = int(rng.choice([0, 0, 97, 333, 5000]))
        what = f"seed={seed} draw={draw}: {kind} d={d} n0={n0} chunk_rows={chunk_rows}"
        src = _encode(vf, kind, pool[:30_000, :d])
        cur, nxt = src[:n0], n0
        with _with(_make(vf, kind, cur), (("compact_chunk_rows", chunk_rows),)) as ix:
            if rng.integers(2):
                ix.reserve(n0 + 2000)
            for step in range(int(rng.integers(3, 7))):
                n = len(cur)
                if rng.integers(3) == 0:                               # an append: up to 3000 rows
                    m = int(rng.integers(1, 3001))
                    assert ix.add(src[nxt:nxt + m]) == n, what
                    cur, nxt = np.concatenate([cur, src[nxt:nxt + m]]), nxt + m
                    what += f" +{m}"
                    continue
                shape = int(rng.integers(4))                           # scattered / a run / the tail / across the limit
                if shape == 0:
                    gone = rng.choice(n, int(rng.integers(1, 400)), replace=True)
                elif shape == 1:
                    a = int(rng.integers(0, n - 1500))
                    gone = np.arange(a, a + int(rng.integers(1, 1500)))
                elif shape == 2:
                    gone = np.arange(n - int(rng.integers(1, 300)), n)
                else:
                    m = max(1, n - int(rng.integers(16_000, 16_385))) if n > 16_384 else int(rng.integers(1, 50))
                    gone = rng.choice(n, m, replace=False)
                cur = _remove(ix, cur, gone)
                what += f" -{np.unique(gone).size}(shape {shape})"
            n1 = len(cur)
            nq, k = int(rng.integers(1, 71)), int(rng.integers(1, 257))
            fp = int(rng.choice([-1, 1, 2])) if n1 > 16_384 else int(rng.choice([-1, 0, 2]))
            what += f" nq={nq} k={k} force_path={fp}"
            q = pool[44_000:44_000 + nq, :d].copy()
            q[0] = np.asarray(_values(kind, cur[n1 - 1:n1]), dtype=np.float32)[0]
            ix.set_option("force_path", fp)
            got = ix.search(q, k)
            st = ix.stats()
            want = oracle.search(_values(kind, cur), q, k)
            assert st["path"] == (fp if fp >= 0 else (1 if n1 > 16_384 else 0)), (what, st)
            assert _same(got, want), (what, st)
            assert got[0][0, 0] == n1 - 1, what
