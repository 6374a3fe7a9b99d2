"""The int8 scan image (option scan_image) on the GPU: fp16 / fp32 rows of 768 elements in shards of 4M rows and more
are scanned through a per-row-scaled int8 copy (rows of 1024 keep the fp16 scan), and k_final's band re-score keeps ids and score bits those of the canonical
arithmetic -- the oracle's, and the fp16 scan's (scan_image = 0) on the same index."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4_000_000   # the image's smallest shard (kImageMinRows)


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _shard(n, d, seed=0):
    """N(0, 1) fp16 rows generated where they live (bench.make_shard's generator, shifted by `seed` chunks)."""
    import torch
    import bench
    lo = seed * bench.GEN_CHUNK
    return bench.make_shard(torch, lo, lo + n, d, torch.device("cuda", 0), "f16")


@pytest.fixture(scope="module")
def c768():
    return _shard(N, 768)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def _search_both(ix, q, k):
    """(image result, its stats), (fp16-path result, its stats) on one index; the image is dropped and rebuilt."""
    ix.set_option("scan_image", 1)
    got = ix.search(q, k)
    st = ix.stats()
    ix.set_option("scan_image", 0)
    ref = ix.search(q, k)
    st0 = ix.stats()
    ix.set_option("scan_image", 1)
    return got, st, ref, st0


@pytest.mark.parametrize("nq,k", [(64, 100), (1, 1), (128, 100), (64, 1), (7, 128), (7, 256)])
def test_image_768_matches_oracle_and_fp16_path(vf, oracle, c768, nq, k):
    q = np.random.default_rng(7002 + nq + k).standard_normal((nq, 768)).astype(np.float32)
    with vf.DenseIndex(c768) as ix:
        got, st, ref, st0 = _search_both(ix, q, k)
        image = nq <= 64 and k <= 128
        if image:
            assert st["path"] == 1 and st["scan_image"] == 1 and st["scan_kernel"] == 5, st
        elif nq > 64:                                            # 128 queries of fp16 rows: one wide pass, never the image
            assert st["scan_image"] == 0 and st["wide_launches"] == 1, st
        else:                                                    # k above the image's limit: the rows as stored
            assert st["scan_image"] == 0 and st["scan_kernel"] == 5, st
        assert st["exact_reruns"] == 0 and st["overflowed"] == 0, st
        assert st0["scan_image"] == 0 and st0["exact_reruns"] == 0, st0
        assert _same(got, ref)
        if (nq, k) == (64, 100):
            assert _same(got, oracle.search(c768.cpu().numpy(), q, k))
        # the same index again after the image was dropped and rebuilt: bit for bit
        assert _same(ix.search(q, k), ref) and ix.stats()["scan_image"] == (1 if image else 0)


def test_rows_of_1024_keep_the_fp16_scan(vf):
    """1024-wide rows: the 2 eps band of a top-100 over 4M rows overflows k_final's survivor area for most queries (measured with an
    image: 40 of 64 queries re-run exactly), so no image is built for them."""
    c = _shard(N, 1024, seed=3)
    q = np.random.default_rng(7102).standard_normal((64, 1024)).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        ix.set_option("scan_image", 2)
        ix.search(q, 100)
        st = ix.stats()
        assert st["scan_image"] == 0 and st["scan_kernel"] == 5 and st["exact_reruns"] == 0, st


def test_fp32_rows_take_the_image(vf, c768):
    c = c768.float() * 3.0
    q = np.random.default_rng(7202).standard_normal((16, 768)).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        got, st, ref, _ = _search_both(ix, q, 100)
        assert st["scan_image"] == 1 and st["exact_reruns"] == 0, st
        assert _same(got, ref)


def test_clustered_corpus_fails_the_certificate_and_is_repaired(vf, oracle):
    """Rows that are one direction plus a little noise: every score lies within the eps band of the k-th best, the band does not fit
    k_final's survivor area, the certificate fails and the exact path answers -- with the oracle's ids and score bits."""
    import torch
    d = 768
    g = torch.Generator(device="cuda")
    g.manual_seed(7301)
    base = torch.randn(d, generator=g, device="cuda")
    c = torch.empty((N, d), dtype=torch.float16, device="cuda")
    for r0 in range(0, N, 500_000):
        c[r0:r0 + 500_000] = (base + 0.02 * torch.randn((500_000, d), generator=g, device="cuda")).half()
    q = (base.cpu().numpy() + 0.5 * np.random.default_rng(7302).standard_normal((4, d))).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        i, s = ix.search(q, 100)
        st = ix.stats()
        assert st["scan_image"] == 1 and st["exact_reruns"] > 0, st
        assert _same((i, s), oracle.search(c.cpu().numpy(), q, 100))


def test_sharded_group_and_corpus_file(vf, c768, tmp_path):
    from veritasfi_amd import corpus_file
    c1 = _shard(N, 768, seed=40)
    q = np.random.default_rng(7402).standard_normal((64, 768)).astype(np.float32)
    with vf.DenseIndex(c768) as a, vf.DenseIndex(c1, id_offset=N) as b:
        a.set_option("scan_image", 0)
        b.set_option("scan_image", 0)
        ref = [a.search(q, 100), b.search(q, 100)]
    with vf.DenseIndex.group([vf.DenseIndex(c768), vf.DenseIndex(c1, id_offset=N)]) as ix:   # two 4M-row shards, one device
        got = ix.search(q, 100)
        assert ix.stats()["scan_image"] == 1, ix.stats()
        ix.set_option("scan_image", 0)
        assert _same(ix.search(q, 100), got)
    ids = np.concatenate([ref[0][0], ref[1][0]], axis=1)
    sc = np.concatenate([ref[0][1], ref[1][1]], axis=1)
    order = np.lexsort((ids, -sc.astype(np.float64)), axis=1)[:, :100]
    assert np.array_equal(np.take_along_axis(ids, order, 1), got[0])
    p = str(tmp_path / "img.vfc")
    corpus_file.write(p, c768.cpu().numpy())
    with vf.DenseIndex.from_file(p) as ix:
        i, s = ix.search(q, 100)
        assert ix.stats()["scan_image"] == 1 and ix.stats()["exact_reruns"] == 0
        assert _same((i, s), ref[0])


def test_option_values_and_smaller_shards(vf):
    c = _shard(2_500_000, 768, seed=80)                      # a 4-GPU rank's shard of the headline corpus: no image
    q = np.random.default_rng(7502).standard_normal((64, 768)).astype(np.float32)
    with vf.DenseIndex(c) as ix:
        with pytest.raises(Exception):
            ix.set_option("scan_image", 3)
        ix.set_option("scan_image", 2)                          # forced: still only for shards of 4M rows and more
        ix.search(q, 100)
        st = ix.stats()
        assert st["scan_image"] == 0 and st["scan_kernel"] == 5, st
