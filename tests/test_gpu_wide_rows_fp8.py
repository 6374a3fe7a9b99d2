"""e4m3 rows of 2560 to 4096 padded elements on the fused path (k_scan_ksplit8, vf_search_stats.scan_kernel == 7; option "wide_rows"),
and the wide pass (k_scan_wide / k_scan_wide8) on the same rows for batches of 33 or more queries.

The rows are e4m3 codes cast from N(0, 1) with torch; the CPU oracle (oracle/vf_oracle.c through the `oracle` fixture) runs on the
exactly decoded rows (every e4m3 value is an fp16 value): ids and score BITS equal.  The kernel only feeds the approximate scan -- the
canonical re-score, the certificate and the exact repair are the ones every other width uses -- so a wrong scan shows as a wrong id, as
repairs that ordinary data does not need (test 3 holds the kernel to the fp16 kernel's record on the same values), or as an overflow.
`wide_rows = 2` serves the small corpora used here; `wide` = 0 / 2 pins the side of the query-count boundary, so that no test depends
on the two measured dispatch constants."""
import numpy as np
import pytest

from conftest import assert_ranked

pytestmark = pytest.mark.gpu

STAT_KEYS = ("path", "scan_kernel", "candidates", "max_candidates", "uncertified", "overflowed", "exact_reruns")


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
    bad = np.nonzero((wi != gi).any(axis=1))[0]
    assert bad.size == 0, f"{what}: ids differ for queries {bad[:8].tolist()} (first: got {gi[bad[0]][:8]}, want {wi[bad[0]][:8]})"
    assert np.array_equal(_bits(ws), _bits(gs)), f"{what}: score bits differ, max |diff| = {float(np.max(np.abs(ws - gs)))}"
    for q in range(gi.shape[0]):
        assert_ranked(gi[q], gs[q])


def _e4m3_codes(n, d, seed):
    """tests/test_gpu_retrieval.py's: N(0, 1) / 2 cast with torch, some rows at the top of the range, some in the subnormals."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, d), generator=g) * 0.5
    x[::97] *= 40.0
    x[5::89] *= 2.0 ** -8
    return x.to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()


def _decoded(codes):
    from oracle import ref_numpy as R
    rows16 = R.decode_e4m3(codes).astype(np.float16)
    assert np.array_equal(rows16.astype(np.float32), R.decode_e4m3(codes))   # exact
    return rows16


def _queries(seed, nq, d):
    return np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)


def _stats(tag, st):
    print(f"{tag}:", {x: st[x] for x in STAT_KEYS})


# ---- 1: every shape of the kernel (segments per wave 5 / 6 / 6 with a padded copy / 8 with an absent segment / 8) ------------------
@pytest.mark.parametrize("d", [2560, 2688, 3000, 3968, 4096])
def test_fp8_wide_rows_on_the_fused_path_bit_equal_to_the_oracle(vf, oracle, d):
    n, nqs, ks = 20_000, (1, 3, 32), (1, 100, 2048)
    codes = _e4m3_codes(n, d, 100 + d)
    q = _queries(200 + d, max(nqs), d)
    full = oracle.search(_decoded(codes), q, max(ks))     # (ranked by a total order: the best k of it are the result for k)
    want = {k: (np.ascontiguousarray(full[0][:, :k]), np.ascontiguousarray(full[1][:, :k])) for k in ks}
    with vf.DenseIndex.from_e4m3(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        for k in ks:
            for nq in nqs:
                ids, sc = ix.search(q[:nq], k)
                st = ix.stats()
                _stats(f"d={d} nq={nq} k={k}", st)
                assert st["path"] == 1 and st["scan_kernel"] == 7 and st["overflowed"] == 0, st
                _same((want[k][0][:nq], want[k][1][:nq]), (ids, sc), f"d={d} nq={nq} k={k}")
        ix.set_option("wide_rows", 0)                       # the kernel switched off: path 2, the same bits
        for k, nq in ((100, 3), (2048, 32), (1, 1)):
            ids, sc = ix.search(q[:nq], k)
            assert ix.stats()["path"] == 2
            _same((want[k][0][:nq], want[k][1][:nq]), (ids, sc), f"wide_rows=0 d={d} nq={nq} k={k}")
        with pytest.raises(Exception):                      # forcing the fused path with the kernel switched off is refused
            ix.set_option("force_path", 1)
            ix.search(q[:2], 10)
        ix.set_option("force_path", -1)


# ---- 2: 33 or more queries: the wide pass, on both matrix instructions; a padding it does not serve ---------------------------------
@pytest.mark.parametrize("wide_mfma,kernel", [(1, 4), (0, 3)], ids=["k_scan_wide8", "k_scan_wide"])
@pytest.mark.parametrize("d", [2560, 4096])
def test_fp8_wide_rows_on_the_wide_pass(vf, oracle, d, wide_mfma, kernel):
    n, nqs, ks = 20_000, (33, 130), (100, 1000)
    codes = _e4m3_codes(n, d, 300 + d)
    q = _queries(400 + d, max(nqs), d)
    full = oracle.search(_decoded(codes), q, max(ks))
    with vf.DenseIndex.from_e4m3(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 2)
        ix.set_option("wide_mfma", wide_mfma)
        for k in ks:
            for nq in nqs:
                ids, sc = ix.search(q[:nq], k)
                st = ix.stats()
                _stats(f"d={d} wide_mfma={wide_mfma} nq={nq} k={k}", st)
                assert st["path"] == 1 and st["scan_kernel"] == kernel and st["overflowed"] == 0, st
                _same((np.ascontiguousarray(full[0][:nq, :k]), np.ascontiguousarray(full[1][:nq, :k])), (ids, sc), f"d={d} nq={nq} k={k}")


def test_fp8_rows_padded_to_2688_take_two_passes_of_the_new_kernel_at_40_queries(vf, oracle):
    codes = _e4m3_codes(20_000, 2688, 77)                   # dp % 256 != 0: no wide pass
    q = _queries(78, 40, 2688)
    with vf.DenseIndex.from_e4m3(codes) as ix:
        ix.set_option("wide_rows", 2)
        ids, sc = ix.search(q, 100)
        st = ix.stats()
    assert st["path"] == 1 and st["scan_kernel"] == 7 and st["overflowed"] == 0, st
    _same(oracle.search(_decoded(codes), q, 100), (ids, sc), "2688, 40 queries")


# ---- 3: the scan is right, not merely repaired --------------------------------------------------------------------------------------
SEED_NO_REPAIR = {2560: 1, 4096: 1}   # chosen on the GPU: the fp16 control (k_scan_ksplit on the same values) needs no repair on these rows


@pytest.mark.parametrize("d", [2560, 4096])
def test_fp8_scan_needs_no_repair_where_the_fp16_scan_of_the_same_values_needs_none(vf, oracle, d):
    n, nq, k = 40_000, 32, 100
    codes = _e4m3_codes(n, d, SEED_NO_REPAIR[d])
    rows16 = _decoded(codes)
    q = _queries(SEED_NO_REPAIR[d] + 1000, nq, d)
    want = oracle.search(rows16, q, k)
    with vf.DenseIndex(rows16) as ix:                       # the control: if it fails, the data is at fault, not the new kernel
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        ids, sc = ix.search(q, k)
        st16 = ix.stats()
    _stats(f"d={d} fp16 control", st16)
    assert st16["path"] == 1 and st16["scan_kernel"] == 6, st16
    assert st16["exact_reruns"] == 0 and st16["overflowed"] == 0, st16
    _same(want, (ids, sc), "fp16 control")
    with vf.DenseIndex.from_e4m3(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        ids, sc = ix.search(q, k)
        st = ix.stats()
    _stats(f"d={d} e4m3", st)
    assert st["path"] == 1 and st["scan_kernel"] == 7, st
    assert st["exact_reruns"] == 0 and st["overflowed"] == 0, st
    _same(want, (ids, sc), "e4m3")


# ---- 4: shapes that bite (run only after tests/test_wide_rows_fp8_geometry.py passes) and hostile data ------------------------------
@pytest.mark.parametrize("n,d,opts", [(21_845, 2688, {"waves": 8192, "sample_rows": 64}),   # ranges shorter than their sample part
                                      (16_385, 4096, {}),                                   # one row past the small-corpus limit
                                      (20_011, 3000, {"waves": 1024})])                     # n no multiple of 32, a padded width
def test_fp8_shapes_that_bite(vf, oracle, n, d, opts):
    codes = _e4m3_codes(n, d, n)
    q = _queries(n + 1, 7, d)
    want = oracle.search(_decoded(codes), q, 50)
    with vf.DenseIndex.from_e4m3(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        for name, val in opts.items():
            ix.set_option(name, val)
        ids, sc = ix.search(q, 50)
        st = ix.stats()
    _stats(f"n={n} d={d} {opts}", st)
    assert st["path"] == 1 and st["scan_kernel"] == 7, st
    _same(want, (ids, sc), f"n={n} d={d}")


def test_fp8_hostile_rows(vf, oracle):
    """Duplicate rows (ties go to the lower id), an all-zero row, rows of the largest code (+-448 everywhere), rows of the smallest
    subnormal (2^-9), and a query orthogonal to everything but one row."""
    n, d, k = 20_003, 2560, 40
    codes = _e4m3_codes(n, d, 4242)
    codes[:, d - 1] = 0                                     # the last element belongs to row 12 345 alone
    codes[12_345, d - 1] = 0x38                             # 1.0
    codes[100:120] = codes[9_000]                           # duplicates, far apart and adjacent
    codes[15_000:15_040] = codes[9_000]
    codes[77] = 0                                           # all-zero row
    codes[500] = 0x7E                                       # +448 everywhere
    codes[501] = 0xFE                                       # -448 everywhere
    codes[502, ::2], codes[502, 1::2] = 0x7E, 0xFE
    codes[600] = 0x01                                       # the smallest subnormal, 2^-9, everywhere
    codes[601] = 0x81
    rows16 = _decoded(codes)
    q = _queries(4243, 8, d)
    q[0] = rows16[9_000].astype(np.float32)                 # the duplicated row: 61 exact ties at the top
    q[1] = 0.0
    q[1, d - 1] = 1.0                                       # orthogonal to every row but 12 345
    q[2] = 1.0                                              # the +448 row exactly, the 2^-9 row exactly (cosine 1 twice: a tie)
    q[3] = -1.0
    q[4] = rows16[502].astype(np.float32)
    want = oracle.search(rows16, q, k)
    assert want[0][1, 0] == 12_345 and set(want[0][2, :2].tolist()) == {500, 600}
    assert np.array_equal(want[0][0, :21], np.concatenate([np.arange(100, 120), [9_000]]))   # ties ranked by id
    with vf.DenseIndex.from_e4m3(codes) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        ids, sc = ix.search(q, k)
        st = ix.stats()
        _stats("hostile rows, k_scan_ksplit8", st)
        assert st["path"] == 1 and st["scan_kernel"] == 7, st
        _same(want, (ids, sc), "hostile rows")
        q40 = np.concatenate([q] * 5)                       # the same through both wide kernels
        ix.set_option("wide", 2)
        for wide_mfma, kernel in ((1, 4), (0, 3)):
            ix.set_option("wide_mfma", wide_mfma)
            ids, sc = ix.search(q40, k)
            st = ix.stats()
            _stats(f"hostile rows, wide_mfma={wide_mfma}", st)
            assert st["path"] == 1 and st["scan_kernel"] == kernel, st
            _same((np.concatenate([want[0]] * 5), np.concatenate([want[1]] * 5)), (ids, sc), f"hostile rows, wide_mfma={wide_mfma}")


# ---- 5: the handle kinds ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sharded_case(oracle):
    codes = _e4m3_codes(70_001, 2560, 55)
    q = _queries(56, 29, 2560)
    return codes, q, oracle.search(_decoded(codes), q, 100)


@pytest.mark.parametrize("shards", [2, 3])
def test_fp8_sharded_handles_on_one_device(vf, sharded_case, shards):
    codes, q, want = sharded_case
    with vf.DenseIndex.from_e4m3(codes, device_ids=[0] * shards) as ix:
        ix.set_option("wide_rows", 2)
        ix.set_option("wide", 0)
        ids, sc = ix.search(q, 100)
        st = ix.stats()
        assert st["path"] == 1 and st["scan_kernel"] == 7 and st["overflowed"] == 0, st
        _same(want, (ids, sc), f"{shards} shards")


def test_fp8_begin_end_over_all_slots_file_index_and_borrowed_rows(vf, oracle, tmp_path):
    import torch
    from veritasfi_amd import corpus_file
    codes = _e4m3_codes(40_000, 3072, 70)
    q = _queries(71, 48, 3072)
    k = 20
    want = oracle.search(_decoded(codes), q, k)
    path = str(tmp_path / "wide8.vfc")
    corpus_file.write(path, codes, e4m3=True)
    assert corpus_file.info(path)["dtype"] == 2
    rows_dev = torch.from_numpy(codes).cuda().view(torch.float8_e4m3fn)
    for name, ix in (("host codes", vf.DenseIndex.from_e4m3(codes)), (".vfc file of dtype 2", vf.DenseIndex.from_file(path)),
                     ("borrowed float8_e4m3fn device tensor", vf.DenseIndex(rows_dev))):
        with ix:
            ix.set_option("wide_rows", 2)
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


# ---- 6: the same case forty times ---------------------------------------------------------------------------------------------------
def test_fp8_forty_repeats_are_bit_equal(vf, oracle):
    codes = _e4m3_codes(50_000, 4096, 90)
    q = _queries(91, 32, 4096)
    want = oracle.search(_decoded(codes), q, 100)
    with vf.DenseIndex.from_e4m3(codes) as ix:
        ix.set_option("wide_rows", 2)
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


# ---- 7: the Python surface ----------------------------------------------------------------------------------------------------------
def test_faiss_retriever_with_corpus_dtype_fp8_on_2560_wide_embeddings(vf, oracle, monkeypatch):
    rng = np.random.default_rng(17)
    emb = rng.standard_normal((20_000, 2560)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)       # unit rows, as an embedder returns them: elements around 2^-6
    emb[::5] *= 37.0                                        # ... and rows that are not
    stored = {}
    real = vf.DenseIndex.from_e4m3.__func__

    def spy(cls, codes, *a, **kw):                          # the codes the retriever hands to its index: what it actually stored
        stored["codes"] = np.array(codes, copy=True)
        return real(cls, codes, *a, **kw)

    monkeypatch.setattr(vf.DenseIndex, "from_e4m3", classmethod(spy))

    class Emb:
        def embed_queries(self, texts):
            return [(emb[int(t)] + 0.05 * emb[(int(t) * 7 + 1) % len(emb)]).tolist() for t in texts]

    fr = vf.FaissRetriever(emb, Emb(), corpus_dtype="fp8")
    try:
        fr.index.set_option("wide_rows", 2)                 # 20 000 rows: below the auto threshold
        texts = [str(i) for i in (0, 1, 5, 4_321, 19_999)]
        I, D = fr.invoke(texts, 100)
        st = fr.index.stats()
        _stats("FaissRetriever(corpus_dtype='fp8')", st)
        assert st["path"] == 1 and st["scan_kernel"] == 7, st
        assert [int(i) for i in I[:, 0]] == [0, 1, 5, 4_321, 19_999]
        codes = stored["codes"]
        assert codes.shape == emb.shape and codes.dtype == np.uint8
        assert (np.abs(_decoded(codes).astype(np.float32)).max(axis=1) >= 224.0).all()   # every row uses the top binade: nothing flushed
        qv = np.asarray(Emb().embed_queries(texts), np.float32)
        _same(oracle.search(_decoded(codes), qv, 100), (I, D), "FaissRetriever.invoke")
    finally:
        fr.index.close()


# ---- one size that matters ----------------------------------------------------------------------------------------------------------
def test_fp8_one_million_rows_of_2560_whole_corpus_oracle_check(vf, oracle):
    import torch
    n, d, nq, k = 1_000_000, 2560, 64, 100
    g = torch.Generator().manual_seed(2560)
    codes = np.empty((n, d), np.uint8)
    for lo in range(0, n, 50_000):                          # (in blocks: the fp32 draw of the whole corpus would be 10 GB)
        codes[lo:lo + 50_000] = torch.randn((50_000, d), generator=g).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    q = _queries(2561, nq, d)
    with vf.DenseIndex.from_e4m3(codes) as ix:
        ix.set_option("wide", 2)
        ids, sc = ix.search(q, k)                           # 64 queries on the wide pass
        st = ix.stats()
        ix.set_option("wide", 0)
        ids32, sc32 = ix.search(q[:32], k)                  # 32 queries: k_scan_ksplit8
        st32 = ix.stats()
    _stats("1M x 2560 e4m3, 64 queries", st)
    _stats("1M x 2560 e4m3, 32 queries", st32)
    assert st["path"] == 1 and st["scan_kernel"] in (3, 4) and st["overflowed"] == 0 and st["exact_reruns"] == 0, st
    assert st32["path"] == 1 and st32["scan_kernel"] == 7 and st32["overflowed"] == 0 and st32["exact_reruns"] == 0, st32
    rows16 = np.empty((n, d), np.float16)
    for lo in range(0, n, 50_000):
        rows16[lo:lo + 50_000] = _decoded(codes[lo:lo + 50_000])
    want = oracle.search(rows16, q, k)
    _same(want, (ids, sc), "1M x 2560, 64 queries")
    _same((want[0][:32], want[1][:32]), (ids32, sc32), "1M x 2560, 32 queries")
