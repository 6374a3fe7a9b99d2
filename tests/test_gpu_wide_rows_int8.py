"""int8 rows of 2560 to 4096 padded elements on the fused path (k_scan_ksplit8i: k_scan_ksplit8 with the int8 conversion,
vf_search_stats.scan_kernel == 7; option "wide_rows"), and k_scan_wide's int8 form on the same rows for batches of 65 or more queries.

Every expected value is the CPU oracle's (oracle/vf_oracle.c through the `oracle` fixture) on `codes.astype(np.float32)`: ids and score
BITS equal.  The kernel only feeds the approximate scan -- the canonical re-score, the certificate and the exact repair are the ones
every other width uses -- so a wrong scan shows as a wrong id, as repairs that ordinary data does not need (test 4 holds the kernel to
the fp16 kernel's record on the same values), or as an overflow.  int8 rows of these widths are served from 32 768 rows upward at every
setting (test 2), so every corpus here has at least that many rows; `wide` = 0 pins the 32-query passes where a test is not about the
query-count boundary."""
import numpy as np
import pytest

from conftest import assert_ranked

pytestmark = pytest.mark.gpu

STAT_KEYS = ("path", "scan_kernel", "candidates", "max_candidates", "uncertified", "overflowed", "exact_reruns", "wide_launches")
FLOOR = 32_768                                               # kWideRowsMinRowsI8


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


def _cut(full, nq, k):
    return np.ascontiguousarray(full[0][:nq, :k]), np.ascontiguousarray(full[1][:nq, :k])


def _codes(vf, n, d, seed):
    """quantize_int8 of seeded N(0, 1) rows (what an int8 corpus of embeddings looks like)."""
    return vf.quantize_int8(np.random.default_rng(seed).standard_normal((n, d), dtype=np.float32))


def _queries(seed, nq, d):
    return np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)


def _stats(tag, st):
    print(f"{tag}:", {x: st[x] for x in STAT_KEYS})


def _want(oracle, codes, q, k):
    return oracle.search(codes.astype(np.float32), q, k)


# ---- 1: every shape of the kernel (segments per wave 5 / 6 / 6 with a padded copy / 8 with an absent segment / 8) ------------------
@pytest.mark.parametrize("d", [2560, 2688, 3000, 3968, 4096])
def test_int8_wide_rows_on_the_fused_path_bit_equal_to_the_oracle(vf, oracle, d):
    n, nqs, ks = 32_805, (1, 3, 32), (1, 100, 2048)
    codes = _codes(vf, n, d, 100 + d)
    q = _queries(200 + d, max(nqs), d)
    full = _want(oracle, codes, q, max(ks))               # (ranked by a total order: the best k of it are the result for k)
    with vf.DenseIndex(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        for k in ks:
            for nq in nqs:
                ids, sc = ix.search(q[:nq], k)
                st = ix.stats()
                _stats(f"d={d} nq={nq} k={k}", st)
                assert st["path"] == 1 and st["scan_kernel"] == 7 and st["overflowed"] == 0, st
                _same(_cut(full, nq, k), (ids, sc), f"d={d} nq={nq} k={k}")
        ix.set_option("wide_rows", 0)                       # the kernel switched off: path 2, the same bits
        for k, nq in ((100, 3), (2048, 32), (1, 1)):
            ids, sc = ix.search(q[:nq], k)
            assert ix.stats()["path"] == 2
            _same(_cut(full, nq, k), (ids, sc), f"wide_rows=0 d={d} nq={nq} k={k}")
        ix.set_option("force_path", 1)                      # forcing the fused path with the kernel switched off is refused
        with pytest.raises(Exception, match="not possible"):
            ix.search(q[:2], 10)
        ix.set_option("force_path", -1)


# ---- 2: the floor of 32 768 rows, at every setting ---------------------------------------------------------------------------------
def test_int8_wide_rows_are_served_from_32768_rows_at_every_setting(vf, oracle):
    d, k = 2560, 100
    codes = _codes(vf, FLOOR, d, 11)
    q = _queries(12, 3, d)
    with vf.DenseIndex(codes) as ix:                        # exactly the floor under auto: the fused path
        ids, sc = ix.search(q, k)
        st = ix.stats()
        _stats("32 768 x 2560, wide_rows = 1", st)
        assert st["path"] == 1 and st["scan_kernel"] == 7, st
        _same(_want(oracle, codes, q, k), (ids, sc), "32 768 rows")
    want = _want(oracle, codes[:FLOOR - 1], q, k)
    with vf.DenseIndex(codes[:FLOOR - 1]) as ix:            # one row fewer: path 2 whatever is asked for
        ix.set_option("wide_rows", 2)
        ids, sc = ix.search(q, k)
        st = ix.stats()
        _stats("32 767 x 2560, wide_rows = 2", st)
        assert st["path"] == 2, st
        _same(want, (ids, sc), "32 767 rows")
        ix.set_option("force_path", 1)
        with pytest.raises(Exception, match="not possible"):
            ix.search(q, k)


# ---- 3: batch routing: one pass, two passes, the wide pass -------------------------------------------------------------------------
def test_int8_rows_padded_to_2688_take_two_passes_of_the_new_kernel_at_40_queries(vf, oracle):
    """The stats hold no pass count.  What shows the second pass: a pass of the kernel holds 32 queries, no wide pass ran
    (wide_launches == 0, scan_kernel == 7), and queries 32 .. 39 come back right without an exact re-run."""
    codes = _codes(vf, 32_800, 2688, 77)                    # dp % 256 != 0: no wide pass
    q = _queries(78, 40, 2688)
    with vf.DenseIndex(codes) as ix:
        ix.set_option("wide_rows", 2)
        ids, sc = ix.search(q, 100)
        st = ix.stats()
    _stats("2688, 40 queries", st)
    assert st["path"] == 1 and st["scan_kernel"] == 7 and st["wide_launches"] == 0 and st["wide_queries"] == 0, st
    assert st["overflowed"] == 0 and st["exact_reruns"] == 0, st      # (queries 32 .. 39 were scanned, not repaired)
    _same(_want(oracle, codes, q, 100), (ids, sc), "2688, 40 queries")


@pytest.mark.parametrize("d", [2560, 4096])
def test_int8_wide_rows_query_count_boundary_and_the_wide_pass(vf, oracle, d):
    n, ks = 32_790, (100, 1000)
    codes = _codes(vf, n, d, 300 + d)
    q = _queries(400 + d, 130, d)
    full = _want(oracle, codes, q, max(ks))
    with vf.DenseIndex(codes) as ix:                        # every option at its default: auto `wide`, auto `wide_rows`
        if d == 2560:
            ids, sc = ix.search(q[:64], 100)                # 64 queries: two passes of k_scan_ksplit8i
            st = ix.stats()
            _stats(f"d={d} nq=64", st)
            assert st["path"] == 1 and st["scan_kernel"] == 7 and st["wide_launches"] == 0 and st["overflowed"] == 0, st
            _same(_cut(full, 64, 100), (ids, sc), f"d={d} nq=64")
        for k in ks:
            for nq in (65, 130):                            # from 65: k_scan_wide's int8 form, new ground at these widths
                ids, sc = ix.search(q[:nq], k)
                st = ix.stats()
                _stats(f"d={d} nq={nq} k={k}", st)
                assert st["path"] == 1 and st["scan_kernel"] == 3 and st["wide_queries"] == nq and st["overflowed"] == 0, st
                _same(_cut(full, nq, k), (ids, sc), f"d={d} nq={nq} k={k}")


# ---- 4: the scan is right, not merely repaired --------------------------------------------------------------------------------------
# chosen on the GPU, seeds tried from 1 upward: with seed 1 the fp16 control (k_scan_ksplit on the same values) showed, at 2560 and at 4096,
# path 1, scan_kernel 6, exact_reruns 0, overflowed 0, uncertified 0 -- and the int8 index path 1, scan_kernel 7 and the same three zeros, with
# ids and score bits equal to the control's.  So the first seed serves both widths.
SEED_NO_REPAIR = {2560: 1, 4096: 1}


@pytest.mark.parametrize("d", [2560, 4096])
def test_int8_scan_needs_no_repair_where_the_fp16_scan_of_the_same_values_needs_none(vf, oracle, d):
    n, nq, k = 40_000, 32, 100
    codes = _codes(vf, n, d, SEED_NO_REPAIR[d])
    rows16 = codes.astype(np.float16)                       # every int8 value is an fp16 value: the same rows exactly
    q = _queries(SEED_NO_REPAIR[d] + 1000, nq, d)
    want = _want(oracle, codes, q, k)
    with vf.DenseIndex(rows16) as ix:                       # the control: if it fails, the data is at fault, not the new kernel
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        ids, sc = ix.search(q, k)
        st16 = ix.stats()
    _stats(f"d={d} fp16 control", st16)
    assert st16["path"] == 1 and st16["scan_kernel"] == 6, st16
    assert st16["exact_reruns"] == 0 and st16["overflowed"] == 0, st16
    _same(want, (ids, sc), "fp16 control")
    with vf.DenseIndex(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        ids, sc = ix.search(q, k)
        st = ix.stats()
    _stats(f"d={d} int8", st)
    assert st["path"] == 1 and st["scan_kernel"] == 7, st
    assert st["exact_reruns"] == 0 and st["overflowed"] == 0, st
    _same(want, (ids, sc), "int8")


# ---- 5: shapes that bite (the geometry is k_scan_ksplit8's: tests/test_wide_rows_fp8_geometry.py walks it) and hostile data ---------
@pytest.mark.parametrize("n,d,opts", [(32_771, 2688, {"waves": 8192, "sample_rows": 64}),   # ranges of 16 rows, shorter than their sample part
                                      (32_768, 4096, {}),                                   # exactly the floor, every LDS image segment in use
                                      (33_003, 3000, {"waves": 1024})])                     # n no multiple of 32, a padded width
def test_int8_shapes_that_bite(vf, oracle, n, d, opts):
    codes = _codes(vf, n, d, n)
    q = _queries(n + 1, 7, d)
    want = _want(oracle, codes, q, 50)
    with vf.DenseIndex(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        for name, val in opts.items():
            ix.set_option(name, val)
        ids, sc = ix.search(q, 50)
        st = ix.stats()
    _stats(f"n={n} d={d} {opts}", st)
    assert st["path"] == 1 and st["scan_kernel"] == 7, st
    _same(want, (ids, sc), f"n={n} d={d}")


def _hostile_case(oracle):
    n, d, k = 32_803, 2560, 40
    rng = np.random.default_rng(4242)
    codes = rng.integers(-128, 128, size=(n, d), dtype=np.int8)   # every byte value, -128 included
    codes[100:120] = codes[9_000]                           # duplicates, adjacent and far apart
    codes[25_000:25_040] = codes[9_000]
    codes[77] = 0                                           # all-zero row: scores 0
    codes[500] = 127
    codes[501] = -127
    codes[502] = -128
    codes[503, ::2], codes[503, 1::2] = 127, -128
    codes[600] = 0; codes[600, 17] = 1                      # zero but for one +1 / -1
    codes[601] = 0; codes[601, 17] = -1
    codes[:, d - 1] = codes[:, d - 2]                       # the last two elements are equal in every row ...
    codes[12_345, d - 2:] = (-50, 50)                       # ... but this one
    q = _queries(4243, 8, d)
    q[0] = codes[9_000]                                     # the duplicated row: 61 exact ties at the top
    q[1] = 0.0
    q[1, d - 2:] = (-1.0, 1.0)                              # orthogonal to every row but 12 345
    q[2] = 1.0                                              # the +127 row exactly
    q[3] = -1.0                                             # the -127 and the -128 row: cosine 1 twice
    q[4] = 0.0
    q[4, 17] = 1.0                                          # row 600 exactly, row 601 its opposite
    q[5] = codes[503]
    want = _want(oracle, codes, q, k)
    assert want[0][1, 0] == 12_345 and want[0][2, 0] == 500 and set(want[0][3, :2].tolist()) == {501, 502} and want[0][4, 0] == 600
    assert want[0][5, 0] == 503
    assert np.array_equal(want[0][0, :21], np.concatenate([np.arange(100, 120), [9_000]]))   # ties ranked by id
    return codes, q, want, k


def test_int8_hostile_rows(vf, oracle):
    """Every byte value (codes drawn from [-128, 127], -128 included), duplicate rows (ties go to the lower id), an all-zero row, rows of
    +127, of -127 and of -128 everywhere, rows that are zero but for one +-1, and a query orthogonal to everything but one row."""
    codes, q, want, k = _hostile_case(oracle)
    with vf.DenseIndex(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        ids, sc = ix.search(q, k)
        st = ix.stats()
        _stats("hostile rows, k_scan_ksplit8i", st)
        assert st["path"] == 1 and st["scan_kernel"] == 7, st
        _same(want, (ids, sc), "hostile rows")
        q72 = np.concatenate([q] * 9)                       # the same through the wide pass
        ix.set_option("wide", 1)
        ids, sc = ix.search(q72, k)
        st = ix.stats()
        _stats("hostile rows, k_scan_wide", st)
        assert st["path"] == 1 and st["scan_kernel"] == 3, st
        _same((np.concatenate([want[0]] * 9), np.concatenate([want[1]] * 9)), (ids, sc), "hostile rows, wide pass")


# ---- 6: the handle kinds ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sharded_case(vf, oracle):
    codes = _codes(vf, 3 * FLOOR + 5, 2560, 55)             # thirds of 32 769 / 32 770 rows: every shard at or above the floor
    q = _queries(56, 29, 2560)
    return codes, q, _want(oracle, codes, q, 100)


@pytest.mark.parametrize("shards", [2, 3])
def test_int8_sharded_handles_on_one_device(vf, sharded_case, shards):
    codes, q, want = sharded_case
    with vf.DenseIndex(codes, device_ids=[0] * shards) as ix:
        ix.set_option("wide", 0)
        ids, sc = ix.search(q, 100)
        st = ix.stats()
        _stats(f"{shards} shards", st)
        assert st["path"] == 1 and st["scan_kernel"] == 7 and st["overflowed"] == 0, st
        _same(want, (ids, sc), f"{shards} shards")


def test_int8_begin_end_over_all_slots_file_index_and_device_rows(vf, oracle, tmp_path):
    import torch
    from veritasfi_amd import corpus_file
    codes = _codes(vf, 33_000, 3072, 70)
    q = _queries(71, 48, 3072)
    k = 20
    want = _want(oracle, codes, q, k)
    path = str(tmp_path / "wide_i8.vfc")
    corpus_file.write(path, codes)
    assert corpus_file.info(path)["dtype"] == 3
    rows_dev = torch.from_numpy(codes).cuda()
    assert rows_dev.dtype == torch.int8
    for name, ix in (("host codes", vf.DenseIndex(codes)), (".vfc file of dtype 3", vf.DenseIndex.from_file(path)),
                     ("torch.int8 device tensor", vf.DenseIndex(rows_dev))):
        with ix:
            ix.set_option("wide", 0)
            nslots = ix.slots
            assert nslots >= 2
            parts = np.array_split(np.arange(q.shape[0]), nslots)
            qd = [torch.from_numpy(q[p]).cuda() for p in parts]
            for rep in range(2):                            # every slot in flight at once, twice (buffers reused)
                outs = [ix.search_begin(s, qd[s], k) for s in range(nslots)]
                for s in range(nslots):
                    ix.search_end(s)
                    st = ix.stats()
                    assert st["path"] == 1 and st["scan_kernel"] == 7, (name, st)
                torch.cuda.synchronize()
                for s, p in enumerate(parts):
                    _same((want[0][p], want[1][p]), (outs[s][0].cpu().numpy(), outs[s][1].cpu().numpy()), f"{name}, slot {s}")


# ---- 7: the same case forty times ---------------------------------------------------------------------------------------------------
def test_int8_forty_repeats_are_bit_equal(vf, oracle):
    codes = _codes(vf, 34_000, 4096, 90)
    q = _queries(91, 32, 4096)
    want = _want(oracle, codes, q, 100)
    with vf.DenseIndex(codes) as ix:
        ix.set_option("wide", 0)
        first = None
        for rep in range(40):
            ids, sc = ix.search(q, 100)
            st = ix.stats()
            assert st["path"] == 1 and st["scan_kernel"] == 7, st
            if first is None:
                _same(want, (ids, sc), "repeat 0")
                first = (ids.copy(), _bits(sc).copy())
            else:
                assert np.array_equal(ids, first[0]) and np.array_equal(_bits(sc), first[1]), f"run {rep} differs from run 0"


# ---- 8: the Python surface ----------------------------------------------------------------------------------------------------------
def test_faiss_retriever_with_corpus_dtype_int8_on_2560_wide_embeddings(vf, oracle):
    n = 32_800
    rng = np.random.default_rng(17)
    emb = rng.standard_normal((n, 2560), dtype=np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)       # unit rows, as an embedder returns them
    emb[::5] *= 37.0                                        # ... and rows that are not

    class Emb:
        def embed_queries(self, texts):
            return [(emb[int(t)] + 0.05 * emb[(int(t) * 7 + 1) % len(emb)]).tolist() for t in texts]

    fr = vf.FaissRetriever(emb, Emb(), corpus_dtype="int8")
    try:
        texts = [str(i) for i in (0, 1, 5, 4_321, n - 1)]
        I, D = fr.invoke(texts, 100)
        st = fr.index.stats()
        _stats("FaissRetriever(corpus_dtype='int8')", st)
        assert st["path"] == 1 and st["scan_kernel"] == 7, st
        assert [int(i) for i in I[:, 0]] == [0, 1, 5, 4_321, n - 1]
        qv = np.asarray(Emb().embed_queries(texts), np.float32)
        _same(_want(oracle, vf.quantize_int8(emb), qv, 100), (I, D), "FaissRetriever.invoke")
    finally:
        fr.index.close()
