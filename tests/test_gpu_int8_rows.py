"""int8 corpora (VF_DTYPE_INT8): rows of two's-complement int8 held one byte per element, scored as the canonical cosine of the integer
values.  Every expected value is the CPU oracle's (oracle/vf_oracle.c through the `oracle` fixture) on `codes.astype(np.float32)`: ids
and score BITS equal, on every path -- small, the conversion route (k_scan's int8 form, scan_kernel 1), the int8-MFMA route on the
index's own bytes (k_scan2r, scan_kernel 5, scan_image 1), the wide pass (k_scan_wide's int8 form, 3), chunked exact -- and through
every container.  A reference is computed once per corpus and sliced (the ranking is a total order: the best k of the best 2048 are the
result for k)."""
import ctypes

import numpy as np
import pytest

from conftest import assert_ranked

pytestmark = pytest.mark.gpu

STAT_KEYS = ("path", "scan_kernel", "scan_image", "candidates", "max_candidates", "uncertified", "overflowed", "exact_reruns")
N = 20_037                                                   # not a whole number of 32-row tiles
FLT_MAX = np.finfo(np.float32).max


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()  # raises if the HIP library is missing: no fallback
    n = _ffi.c_i32(0)
    _ffi.check(_ffi.lib().vf_device_count(n), "vf_device_count")
    assert n.value >= 1, "no GPU visible"
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(want, got, what=""):
    (wi, ws), (gi, gs) = want, got
    assert wi.shape == gi.shape and ws.shape == gs.shape, (what, wi.shape, gi.shape)
    bad = np.nonzero((wi != gi).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:8].tolist()} (first: got {gi[bad[0]][:8]}, want {wi[bad[0]][:8]})"
    assert np.array_equal(_bits(ws), _bits(gs)), f"{what}: score bits differ, max |diff| = {float(np.max(np.abs(ws - gs)))}"
    for q in range(gi.shape[0]):
        assert_ranked(gi[q], gs[q])


def _cut(full, nq, k, q0=0):
    return np.ascontiguousarray(full[0][q0:q0 + nq, :k]), np.ascontiguousarray(full[1][q0:q0 + nq, :k])


def _stats(tag, st):
    print(f"{tag}:", {x: st[x] for x in STAT_KEYS})


def _codes(vf, n, d, seed):
    """quantize_int8 of seeded N(0, 1) rows (what an int8 corpus of embeddings looks like)."""
    return vf.quantize_int8(np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32))


_cases = {}


def _case(vf, oracle, d, n=N, nq=65):
    """Corpus + queries + the oracle's top 2048, built once per (n, d).  Queries 0 / 1 / 2 are noisy copies of row 0, row n - 1 and the
    last row of the last whole 32-row tile; query `nq` (kept apart: `qtie`) has 40 identical rows at its ranks 81 .. 120."""
    key = (n, d, nq)
    if key in _cases:
        return _cases[key]
    codes = _codes(vf, n, d, 1000 + d)
    rng = np.random.default_rng(2000 + d)
    q = rng.standard_normal((nq + 1, d)).astype(np.float32)
    planted = [0, n - 1, n // 32 * 32 - 1]
    for i, r in enumerate(planted):
        q[i] = codes[r].astype(np.float32) + 8.0 * rng.standard_normal(d).astype(np.float32)
    # the tie query: its 81st best row, copied over 39 rows that rank below its 200 best (and are no planted row)
    c32 = codes.astype(np.float32)
    s = (c32 @ q[nq]) / np.maximum(np.linalg.norm(c32, axis=1), 1e-30)
    order = np.argsort(-s, kind="stable")
    low = [int(r) for r in order[200:] if int(r) not in planted]
    dst = np.array(low)[np.linspace(0, len(low) - 1, 39).astype(np.int64)]
    codes[dst] = codes[next(int(r) for r in order[80:] if int(r) not in planted)]
    full = oracle.search(codes.astype(np.float32), q, 2048)
    assert [int(x) for x in full[0][:3, 0]] == planted
    tie_ids, tie_sc = full[0][nq], full[1][nq]
    run = np.nonzero(_bits(tie_sc) == _bits(tie_sc)[99])[0]  # 40 ties across the 100th place, lower ids first
    assert run.size == 40 and run[0] <= 90 and run[-1] >= 109 and np.all(np.diff(tie_ids[run]) > 0), run
    _cases[key] = {"codes": codes, "q": q[:nq], "qtie": q[nq:nq + 1], "full": (full[0][:nq], full[1][:nq]),
                   "full_tie": (full[0][nq:], full[1][nq:]), "planted": planted}
    return _cases[key]


# ---- 1: the small path ----------------------------------------------------------------------------------------------------------------
def test_int8_small_corpus_every_code_value_zero_rows_duplicates_and_padding(vf, oracle):
    n, d = 1000, 100
    rng = np.random.default_rng(1)
    codes = rng.integers(-128, 128, size=(n, d), dtype=np.int8)
    codes[3, :4] = [-128, 127, -128, 127]
    codes[10] = 0; codes[500] = 0                            # zero rows score 0
    codes[20] = codes[7]; codes[999] = codes[7]              # duplicates: ties go to the lower id
    q = rng.standard_normal((5, d)).astype(np.float32)
    q[0] = codes[7]
    c32 = codes.astype(np.float32)
    full = oracle.search(c32, q, n)
    with vf.DenseIndex(codes) as ix:
        ids, sc = ix.search(q, 1)
        assert ix.stats()["path"] == 0
        _same(_cut(full, 5, 1), (ids, sc), "k=1")
        assert ids[0, 0] == 7
        ids, sc = ix.search(q, 1500)                         # more than the corpus holds: -1 / -FLT_MAX pad the tail
        _same(full, (ids[:, :n], sc[:, :n]), "k=1500")
        assert (ids[:, n:] == -1).all() and (sc[:, n:] == -FLT_MAX).all()
        zero_at = [int(np.nonzero(ids[0] == r)[0][0]) for r in (10, 500)]
        assert sc[0, zero_at[0]] == 0.0 and sc[0, zero_at[1]] == 0.0
        pick = np.array([3, 7, 20, 10, 999, 0, 998], np.int64)
        got = ix.cosine_matrix_rows(pick)
        assert np.array_equal(_bits(got), _bits(oracle.cosine(c32[pick], c32[pick])))


# ---- 2: the conversion route: k_scan's int8 form, every width class, both batch limits --------------------------------------------------
@pytest.mark.parametrize("d", [100, 768, 1024, 1536])
def test_int8_conversion_route_bit_equal_to_the_oracle(vf, oracle, d):
    c = _case(vf, oracle, d)
    with vf.DenseIndex(c["codes"]) as ix:
        ix.set_option("scan_image", 0)
        for k in (1, 100, 2048):
            for nq in (1, 64, 65):
                ids, sc = ix.search(c["q"][:nq], k)
                st = ix.stats()
                _stats(f"d={d} nq={nq} k={k}", st)
                assert st["path"] == 1 and st["scan_kernel"] == 1 and st["scan_image"] == 0 and st["exact_reruns"] == 0, st
                _same(_cut(c["full"], nq, k), (ids, sc), f"d={d} nq={nq} k={k}")
                assert [int(x) for x in ids[:3, 0]] == c["planted"][:min(nq, 3)]
        for k in (100, 1):                                   # 40 identical rows across the 100th place (exact with or without a repair)
            ids, sc = ix.search(c["qtie"], k)
            st = ix.stats()
            _stats(f"d={d} ties k={k}", st)
            assert st["path"] == 1 and st["scan_kernel"] == 1, st
            _same(_cut(c["full_tie"], 1, k), (ids, sc), f"d={d} ties k={k}")


# ---- 3: the int8-MFMA route: k_scan2r on the index's own bytes ---------------------------------------------------------------------------
@pytest.mark.parametrize("image_mfma", [0, 1, 2])
def test_int8_mfma_route_bit_equal_to_the_oracle(vf, oracle, image_mfma):
    c = _case(vf, oracle, 768)
    d = 768
    dom = np.random.default_rng(77).standard_normal((1, d)).astype(np.float32)
    dom[0, 123] = 40.0 * np.abs(dom).max()                   # one element 40 x the rest: the query's own int8 plane is coarse there
    want_dom = oracle.search(c["codes"].astype(np.float32), dom, 128)
    with vf.DenseIndex(c["codes"]) as ix:
        ix.set_option("scan_image", 2)
        ix.set_option("image_mfma", image_mfma)
        for k in (1, 128):
            for nq in (1, 64):
                ids, sc = ix.search(c["q"][:nq], k)
                st = ix.stats()
                _stats(f"image_mfma={image_mfma} nq={nq} k={k}", st)
                assert st["path"] == 1 and st["scan_kernel"] == 5 and st["scan_image"] == 1 and st["overflowed"] == 0, st
                _same(_cut(c["full"], nq, k), (ids, sc), f"image_mfma={image_mfma} nq={nq} k={k}")
        ids, sc = ix.search(c["qtie"], 100)
        _stats(f"image_mfma={image_mfma} ties", ix.stats())
        _same(_cut(c["full_tie"], 1, 100), (ids, sc), "ties")
        for k in (1, 128):
            ids, sc = ix.search(dom, k)
            _stats(f"image_mfma={image_mfma} dominant element k={k}", ix.stats())
            _same(_cut(want_dom, 1, k), (ids, sc), f"dominant element k={k}")
        ids, sc = ix.search(c["q"][:3], 129)                 # beyond the route's k: the conversion route answers
        st = ix.stats()
        assert st["scan_kernel"] == 1 and st["scan_image"] == 0, st
        _same(_cut(c["full"], 3, 129), (ids, sc), "k=129")


def test_int8_both_routes_in_turn_on_slot_0_of_one_handle(vf, oracle):
    import torch
    c = _case(vf, oracle, 768)
    q = torch.from_numpy(c["q"][:64]).cuda()
    with vf.DenseIndex(c["codes"]) as ix:
        for scan_image, kernel in ((0, 1), (2, 5), (0, 1), (1, 1)):   # (1 = auto at this size: the conversion route)
            ix.set_option("scan_image", scan_image)
            ids, sc = ix.search_begin(0, q, 100)
            ix.search_end(0)
            torch.cuda.synchronize()
            st = ix.stats()
            assert st["scan_kernel"] == kernel and st["scan_image"] == (1 if kernel == 5 else 0), (scan_image, st)
            _same(_cut(c["full"], 64, 100), (ids.cpu().numpy(), sc.cpu().numpy()), f"scan_image={scan_image}")


# ---- 4: the wide pass -------------------------------------------------------------------------------------------------------------------
def test_int8_wide_pass_of_130_queries(vf, oracle):
    c = _case(vf, oracle, 768)
    q = np.random.default_rng(9).standard_normal((130, 768)).astype(np.float32)
    q[:3] = c["q"][:3]
    want = oracle.search(c["codes"].astype(np.float32), q, 100)
    for scan_image in (1, 2):                                # (a wide batch never takes the int8-MFMA route)
        with vf.DenseIndex(c["codes"]) as ix:
            ix.set_option("scan_image", scan_image)
            ids, sc = ix.search(q, 100)
            st = ix.stats()
            _stats(f"wide scan_image={scan_image}", st)
            assert st["path"] == 1 and st["scan_kernel"] == 3 and st["wide_queries"] == 130 and st["overflowed"] == 0, st
            _same(want, (ids, sc), "wide")


# ---- 5: chunked exact -------------------------------------------------------------------------------------------------------------------
def test_int8_chunked_exact_path_and_rows_of_2560_elements(vf, oracle):
    c = _case(vf, oracle, 768)
    with vf.DenseIndex(c["codes"]) as ix:
        ix.set_option("force_path", 2)
        ids, sc = ix.search(c["q"][:5], 100)
        assert ix.stats()["path"] == 2
        _same(_cut(c["full"], 5, 100), (ids, sc), "force_path=2")
    n, d = 17_000, 2560                                      # no fused kernel converts int8 rows of this width: path 2, as documented
    codes = _codes(vf, n, d, 31)
    q = np.random.default_rng(32).standard_normal((3, d)).astype(np.float32)
    q[0] = codes[n - 1]
    want = oracle.search(codes.astype(np.float32), q, 100)
    with vf.DenseIndex(codes) as ix:
        for wide_rows in (1, 2):
            ix.set_option("wide_rows", wide_rows)
            ids, sc = ix.search(q, 100)
            assert ix.stats()["path"] == 2
            _same(want, (ids, sc), f"d=2560 wide_rows={wide_rows}")
        assert ids[0, 0] == n - 1
        ix.set_option("force_path", 1)
        with pytest.raises(Exception, match="not possible"):
            ix.search(q, 100)


# ---- 6: containers ----------------------------------------------------------------------------------------------------------------------
def test_int8_index_from_a_file_sharded_grouped_and_from_a_device_tensor(vf, oracle, tmp_path):
    import torch
    from veritasfi_amd import _ffi, corpus_file
    n, d = 40_011, 768                                       # halves of 20 005 / 20 006 rows: the shards run the fused path too
    c = _case(vf, oracle, d, n=n, nq=64)
    codes, q, want = c["codes"], c["q"], _cut(c["full"], 64, 100)
    with vf.DenseIndex(codes) as ix:
        single = ix.search(q, 100)
        assert ix.stats()["path"] == 1
        dt = _ffi.c_i32(-1)
        _ffi.check(_ffi.lib().vf_index_info(ix._h, None, None, ctypes.byref(dt), None), "vf_index_info")
        assert dt.value == _ffi.VF_DTYPE_INT8 == 3
    _same(want, single, "single")
    p = str(tmp_path / "c.vfc")
    corpus_file.write(p, codes)
    assert corpus_file.info(p)["dtype"] == 3
    with vf.DenseIndex.from_file(p) as ix:
        _same(single, ix.search(q, 100), "from_file")
    with vf.DenseIndex.from_file(p, rank=1, world=2) as ix:  # a rank's shard: rows 20 005 .., ids = file rows
        ids, sc = ix.search(q[:4], 10)
        lo, hi = vf.shard_bounds(n, 2, 1)
        assert ix.n == hi - lo and hi == n
        w = oracle.search(codes[lo:].astype(np.float32), q[:4], 10, id_offset=lo)
        _same(w, (ids, sc), "from_file rank 1 of 2")
    with vf.DenseIndex.from_file(p, device_ids=[0, 0]) as ix:
        _same(single, ix.search(q, 100), "from_file sharded")
    with vf.DenseIndex(codes, device_ids=[0, 0]) as ix:
        assert ix.shard_devices() == [0, 0]
        _same(single, ix.search(q, 100), "device_ids=[0, 0]")
        ix.set_option("scan_image", 2)                       # forwarded to the shards: the int8-MFMA route on each
        _same(single, ix.search(q, 100), "device_ids=[0, 0] scan_image=2")
    h = 17_003
    with vf.DenseIndex.group([vf.DenseIndex(codes[:h]), vf.DenseIndex(torch.from_numpy(codes[h:]), id_offset=h)]) as ix:
        _same(single, ix.search(q, 100), "group")
        pick = np.array([0, h - 1, h, n - 1], np.int64)
        assert np.array_equal(_bits(ix.cosine_matrix_rows(pick)), _bits(oracle.cosine(codes[pick].astype(np.float32), codes[pick].astype(np.float32))))
    t = torch.from_numpy(codes).cuda()
    ix = vf.DenseIndex(t)
    try:
        assert ix._keepalive is None                         # int8 rows are copied: the index holds no reference to the tensor
        t.fill_(0)                                           # ... so scribbling over it and freeing it changes nothing
        del t
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        _same(single, ix.search(q, 100), "CUDA tensor, deleted")
    finally:
        ix.close()


def test_faiss_retriever_with_corpus_dtype_int8(vf, oracle):
    rng = np.random.default_rng(17)
    emb = rng.standard_normal((N, 768)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)        # unit rows, as an embedder returns them

    class Emb:
        def embed_queries(self, texts):
            return [(emb[int(t)] + 0.05 * emb[(int(t) * 7 + 1) % len(emb)]).tolist() for t in texts]

    fr = vf.FaissRetriever(emb, Emb(), corpus_dtype="int8")
    try:
        assert fr.rows_as_given is False
        texts = [str(i) for i in (0, 1, 5, 4_321, N - 1)]
        I, D = fr.invoke(texts, 100)
        _stats("FaissRetriever(corpus_dtype='int8')", fr.index.stats())
        assert [int(i) for i in I[:, 0]] == [0, 1, 5, 4_321, N - 1]
        qv = np.asarray(Emb().embed_queries(texts), np.float32)
        _same(oracle.search(vf.quantize_int8(emb).astype(np.float32), qv, 100), (I, D), "invoke")
    finally:
        fr.index.close()
    with pytest.raises(ValueError, match="non-finite"):
        vf.FaissRetriever(np.array([[1.0, np.inf], [0.0, 1.0]], np.float32), Emb(), corpus_dtype="int8")


# ---- 7: memory: one byte per element and nothing wider --------------------------------------------------------------------------------
def test_int8_index_of_a_million_rows_holds_no_two_byte_copy(vf):
    import torch
    n, d = 1_000_000, 768
    g = torch.Generator(device="cuda").manual_seed(5)
    t = torch.randint(-128, 128, (n, d), generator=g, device="cuda", dtype=torch.int8)
    probe = t[123_456].float().cpu().numpy()[None, :]
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    ix = vf.DenseIndex(t)
    try:
        free1, _ = torch.cuda.mem_get_info()
        drop, bound = free0 - free1, n * (d + 16) + (64 << 20)
        print(f"free device memory fell by {drop / 2**20:.1f} MiB for {n} x {d} int8 rows (bound {bound / 2**20:.1f} MiB; fp16 rows alone: {n * d * 2 / 2**20:.1f})")
        assert drop <= bound, (drop, bound)
        del t
        torch.cuda.empty_cache()
        ids, sc = ix.search(probe, 10)
        st = ix.stats()
        _stats("1M x 768", st)
        assert st["path"] == 1 and ids[0, 0] == 123_456 and abs(float(sc[0, 0]) - 1.0) < 1e-6
        free1, _ = torch.cuda.mem_get_info()
        ix.set_option("scan_image", 2)                       # the int8-MFMA route adds two floats per row, no copy of the rows
        free2, _ = torch.cuda.mem_get_info()
        ids2, sc2 = ix.search(probe, 10)
        assert ix.stats()["scan_kernel"] == 5 and np.array_equal(ids, ids2) and np.array_equal(_bits(sc), _bits(sc2))
        assert free1 - free2 <= 2 * (n + 64) * 4 + (4 << 20), (free1, free2)
    finally:
        ix.close()


# ---- 8: errors ------------------------------------------------------------------------------------------------------------------------
def test_int8_bad_dtypes_raise(vf):
    from veritasfi_amd import _ffi
    rows = np.zeros((64, 16), np.int8)
    h = _ffi.vp()
    with pytest.raises(RuntimeError, match="unknown dtype"):
        _ffi.check(_ffi.lib().vf_index_create(ctypes.byref(h), rows.ctypes.data, 64, 16, 4, 0, 0), "vf_index_create")
    assert not h.value
    dev = (_ffi.c_i32 * 1)(0)
    with pytest.raises(RuntimeError, match="unknown dtype"):
        _ffi.check(_ffi.lib().vf_index_create_sharded(ctypes.byref(h), rows.ctypes.data, 64, 16, 4, dev, 1), "vf_index_create_sharded")
    with pytest.raises(TypeError, match="int8"):
        vf.DenseIndex.from_int8(rows.view(np.uint8))
    with vf.DenseIndex.from_int8(rows) as ix:                # (an all-zero corpus: every score 0, ids ascending)
        ids, sc = ix.search(np.ones((1, 16), np.float32), 3)
        assert ids.tolist() == [[0, 1, 2]] and not sc.any()
