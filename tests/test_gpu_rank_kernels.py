"""The kernels that ORDER results -- k_merge_topk (counting and bitonic branches, both entry points), k_fuse_rank, k_topk_rows /
k_sort_rows and the chunked exact path -- on synthetic inputs placed at their switches, limits and tie structures
(tests/rank_cases.py), against plain references.  Every comparison is exact: ids equal, score BITS equal."""
import numpy as np
import pytest
import torch

import rank_cases as RC
import veritasfi_amd as vf
from oracle import ref_numpy
from veritasfi_amd import _ffi

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_same(got_i, got_s, want_i, want_s, what):
    got_i, got_s = np.asarray(got_i), np.asarray(got_s)
    bad = np.nonzero(got_i != want_i)
    assert bad[0].size == 0, f"{what}: {bad[0].size} ids differ, first at {tuple(int(b[0]) for b in bad)}: " \
                             f"got {got_i[bad][:4].tolist()}, want {want_i[bad][:4].tolist()}"
    bad = np.nonzero(_bits(got_s) != _bits(want_s))
    assert bad[0].size == 0, f"{what}: {bad[0].size} score bit patterns differ, first at {tuple(int(b[0]) for b in bad)}: " \
                             f"got {got_s[bad][:4].tolist()}, want {want_s[bad][:4].tolist()}"


def _merge_both(ids, scores, k):
    """The same parts through vf_merge_topk_device ([G, nq, k] tensors) and vf_merge_topk_packed_device (one blob per part)."""
    nparts, nq, _ = ids.shape
    ti, ts = torch.from_numpy(ids).to(DEV), torch.from_numpy(scores).to(DEV)
    mi, ms = vf.merge_topk_device(ti, ts, k)
    blobs = []
    for g in range(nparts):
        blob, vi, vs = vf.packed_result_buffer(nq, k, ti.device)
        assert blob.numel() == vf.packed_part_bytes(nq, k) and blob.numel() % 16 == 0
        vi.copy_(ti[g])
        vs.copy_(ts[g])
        blobs.append(blob)
    pi, ps = vf.merge_topk_packed_device(torch.cat(blobs), nparts, nq, k)
    torch.cuda.synchronize()
    return (mi.cpu().numpy(), ms.cpu().numpy()), (pi.cpu().numpy(), ps.cpu().numpy())


# ---- k_merge_topk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.MERGE_KINDS)
@pytest.mark.parametrize("nparts,k,nq", RC.MERGE_SHAPES)
def test_merge_synthetic_parts_both_entry_points(nparts, k, nq, kind):
    ids, scores = RC.merge_case(nparts, k, nq, kind, seed=1)
    want_i, want_s = RC.merge_reference(ids, scores, k)
    for name, (got_i, got_s) in zip(("tensors", "packed"), _merge_both(ids, scores, k)):
        _assert_same(got_i, got_s, want_i, want_s, f"{name} nparts={nparts} k={k} nq={nq} {kind}")
        if kind == "extremes":
            # a REAL entry whose score is the padding score keeps its id and precedes all padding (query 0 holds one and pads)
            real_low = np.nonzero((want_s[0] == -RC.FLT_MAX) & (want_i[0] >= 0))[0]
            assert real_low.size > 0
            assert np.all(got_i[0][real_low] >= RC.ID_BASE) and np.all(got_s[0][real_low] == -RC.FLT_MAX)
            pad = np.nonzero(got_i[0] == -1)[0]
            assert pad.size == 0 or real_low.max() < pad.min()
            assert np.all(got_i[0][:int((want_i[0] >= 0).sum())] >= RC.ID_BASE)
        if kind == "ties":
            # each output score is its source entry's bits: a -0.0 stays -0.0, a +0.0 stays +0.0
            for q in range(nq):
                src = {int(i): int(b) for i, b in zip(ids[:, q].reshape(-1), _bits(scores[:, q]).reshape(-1)) if i >= 0}
                live = got_i[q] >= 0
                assert [src[int(i)] for i in got_i[q][live]] == _bits(got_s[q][live]).tolist()


def test_merge_refuses_more_than_16384_keys_and_writes_nothing():
    nparts, k, nq = 17, 964, 2                       # m = 16388
    ids, scores = RC.merge_case(nparts, k, nq, "distinct", seed=1)
    ti, ts = torch.from_numpy(ids).to(DEV), torch.from_numpy(scores).to(DEV)
    with pytest.raises(RuntimeError, match=r"nparts \* k > 16384"):
        vf.merge_topk_device(ti, ts, k)
    out_i = torch.full((nq, k), 0x5A5A5A5A5A, dtype=torch.int64, device=DEV)
    out_s = torch.full((nq, k), 1234.5, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(ti.device).cuda_stream
    with pytest.raises(RuntimeError, match=r"nparts \* k > 16384"):
        _ffi.check(_ffi.lib().vf_merge_topk_device(ti.data_ptr(), ts.data_ptr(), nparts, nq, k, out_i.data_ptr(), out_s.data_ptr(),
                                                   0, stream), "vf_merge_topk_device")
    blob = torch.zeros(nparts * vf.packed_part_bytes(nq, k), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=r"nparts \* k > 16384"):
        vf.merge_topk_packed_device(blob, nparts, nq, k, out_i, out_s)
    torch.cuda.synchronize()
    assert bool((out_i == 0x5A5A5A5A5A).all()) and bool((out_s == 1234.5).all())
    # one part fewer (m = 15424, below the limit; m = 16384 itself is in the table of shapes) merges
    want_i, want_s = RC.merge_reference(ids[:16], scores[:16], k)
    for got_i, got_s in _merge_both(ids[:16], scores[:16], k):
        _assert_same(got_i, got_s, want_i, want_s, "16 parts of 964")


@pytest.mark.parametrize("nparts,k,nq", [(3, 7, 0), (3, 0, 5)])
def test_merge_of_nothing_returns_empty_results(nparts, k, nq):
    ti = torch.zeros((nparts, nq, k), dtype=torch.int64, device=DEV)
    ts = torch.zeros((nparts, nq, k), dtype=torch.float32, device=DEV)
    mi, ms = vf.merge_topk_device(ti, ts, k)
    assert tuple(mi.shape) == tuple(ms.shape) == (nq, k)
    blobs = [vf.packed_result_buffer(nq, k, ti.device)[0] for _ in range(nparts)]
    pi, ps = vf.merge_topk_packed_device(torch.cat(blobs), nparts, nq, k)
    assert tuple(pi.shape) == tuple(ps.shape) == (nq, k)


# ---- k_fuse_rank -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", RC.FUSE_KINDS)
@pytest.mark.parametrize("n", RC.FUSE_SIZES)
def test_fuse_rank_sizes_and_score_structures(n, kind):
    a, b = RC.fuse_case(n, kind, seed=2)
    scores, order = vf.fuse_rank(a, b)
    assert scores.shape == (n,) and order.shape == (n,) and order.dtype == np.int64
    assert np.array_equal(_bits(scores), _bits(RC.fuse_sums(a, b)))
    with np.errstate(over="ignore"):
        want = ref_numpy.fuse_and_rank(a, b)
    bad = np.nonzero(order != want)[0]
    assert bad.size == 0, f"n={n} {kind}: order differs at {bad[:4].tolist()}: got {order[bad][:4].tolist()}, want {want[bad][:4].tolist()}"


def test_fuse_rank_refuses_4097():
    a, b = RC.fuse_case(4097, "random", seed=2)
    with pytest.raises(RuntimeError, match=r"n must be in \[0, 4096\]"):
        vf.fuse_rank(a, b)


# ---- k_topk_rows / k_sort_rows: the small path on deep tie groups ----------------------------------------------------------------
def _search_all(oracle, ix, rows, queries, ks, path, what):
    for k in ks:
        ids, scores = ix.search(queries, k)
        assert ix.stats()["path"] == path, (what, k, ix.stats())
        want_i, want_s = oracle.search(rows, queries, k)
        _assert_same(ids, scores, want_i, want_s, f"{what} k={k}")


@pytest.mark.parametrize("n,groups,ks", [
    # tie groups of 4096 rows, the k-th place inside a group at 2048, 4097 and 6000.  At n = 16384 only k <= 2048 takes the radix
    # select (k_topk_rows needs n * 8 + Pk * 8 + 1088 bytes of LDS <= 160 KiB); there it descends into the row-number digits.
    # Every larger k here runs k_sort_rows, 16390 pads
    (16384, 4, (1, 2048, 4097, 6000, 8192, 8193, 16384, 16390)),
    # n = 10000 (P = 16384): every k selects; 5000 / 5001 give Pk = 8192, the last size with Pk * 2 <= P, in 146 KiB of LDS
    (10000, 3, (257, 3334, 5000, 5001)),
    (1, 1, (1, 5)), (2, 2, (1, 5)), (3, 2, (1, 5)),
])
def test_small_path_select_and_sort_inside_tie_groups(oracle, n, groups, ks):
    rows, vec = RC.tied_corpus(n, groups, 32, seed=3)
    queries = RC.tied_queries(vec, seed=3)
    with vf.DenseIndex(rows) as ix:
        _search_all(oracle, ix, rows, queries, ks, 0, f"tied n={n} groups={groups}")


# ---- the chunked exact path (force_path = 2): chunks of 16384 rows, k_sort_rows per chunk, a running two-part merge -----------
@pytest.mark.parametrize("n", [16385, 32768, 32769])      # a last chunk of ONE row; exact multiples; both
def test_chunked_path_chunk_boundaries_and_largest_k(oracle, n):
    rng = np.random.default_rng(n)
    rows = rng.standard_normal((n, 32)).astype(np.float32)
    queries = rng.standard_normal((3, 32)).astype(np.float32)
    with vf.DenseIndex(rows) as ix:
        ix.set_option("force_path", 2)
        _search_all(oracle, ix, rows, queries, (1, 1024, 1025, 8192), 2, f"chunked n={n}")


def test_chunked_path_tie_groups_across_chunk_boundaries(oracle):
    rows, vec = RC.tied_corpus(32769, 4, 32, seed=4)
    queries = RC.tied_queries(vec, seed=4)
    with vf.DenseIndex(rows) as ix:
        ix.set_option("force_path", 2)
        _search_all(oracle, ix, rows, queries, (100, 8192), 2, "chunked tied n=32769")


def test_chunked_path_refuses_k_8193_and_stays_usable(oracle):
    rng = np.random.default_rng(5)
    rows = rng.standard_normal((16385, 32)).astype(np.float32)
    queries = rng.standard_normal((3, 32)).astype(np.float32)
    with vf.DenseIndex(rows) as ix:
        ix.set_option("force_path", 2)
        with pytest.raises(RuntimeError, match=r"k <= 8192 when n > 16384"):
            ix.search(queries, 8193)
        _search_all(oracle, ix, rows, queries, (10,), 2, "after the refusal")


@pytest.mark.parametrize("n,path", [(4, 0), (16386, 2), (16386, -1)])
def test_a_negative_zero_dot_product_is_reported_as_plus_zero(oracle, n, path):
    """Rows 0 and 3 score -0.0 in the canonical arithmetic, row 2 and the rest +0.0: one tie set ranked by id, every score
    reported as +0.0, on the small path, through the chunked path's merge and on the route the library
    chooses itself for 16386 rows (path -1: not forced).  The test pins the RESULT.  Whether the device's dot product is a raw
    -0.0 before the ranking key folds it depends on the kernels keeping fp32 subnormals, which nothing here observes: with
    subnormals flushed the products are +0.0 to begin with and the same result comes out."""
    rows, query, want = RC.negative_zero_case(n)
    with vf.DenseIndex(rows) as ix:
        if path >= 0:
            ix.set_option("force_path", path)
        for k in (3, 16) if n > 4 else (3, 4, 6):
            ids, scores = ix.search(query, k)
            assert path < 0 or ix.stats()["path"] == path
            want_i, want_s = oracle.search(rows, query, k)
            _assert_same(ids, scores, want_i, want_s, f"negative zero n={n} path={path} k={k}")
            kk = min(k, n)
            assert np.array_equal(ids[0, :kk], want[:kk]) and not _bits(scores[0, 1:kk]).any()
