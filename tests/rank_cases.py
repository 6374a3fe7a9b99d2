"""Synthetic inputs and plain NumPy references for the kernels that ORDER results: k_merge_topk, k_fuse_rank,
k_sort_rows / k_topk_rows and the chunked exact path's running merge.  NumPy only; nothing here touches a GPU or the C oracle.

Every operation is exact (a ranking plus copies of the source bits), so the references are compared bit for bit.  Equal floats
are ties (-0.0 == +0.0) and ties go to the lower id / index.  NaN is outside these kernels' contract and is never generated.
"""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
ID_BASE = 5 << 32                         # ids above 2^32: a kernel that narrows an id to 32 bits fails every case
MERGE_KINDS = ("distinct", "ties", "short", "empty", "extremes")
FUSE_KINDS = ("random", "all_equal", "two_valued", "zeros", "inf")


def canonical_order(ids, scores):
    """Positions in rank order: score descending (equal floats tie, signed zeros included), lower id first."""
    return np.lexsort((ids, -scores))


def _scores(rng, kind, n):
    if kind == "ties":
        return rng.choice(np.array([-1.0, -0.0, 0.0, 0.5], np.float32), size=n)
    s = rng.standard_normal(n).astype(np.float32)
    if kind == "extremes":
        pick = rng.integers(0, 12, size=n)
        for code, v in ((0, np.inf), (1, -np.inf), (2, -FLT_MAX), (3, FLT_MAX)):
            s[pick == code] = v
    return s


def _sizes(rng, kind, nparts, k, q):
    """Real entries drawn for each part of one query, before the part keeps its best k."""
    if kind == "empty":
        return np.zeros(nparts, np.int64)
    if kind == "short" or (kind == "extremes" and q == 0):
        # fewer than k in every part and in total; "short" also leaves a middle part with nothing
        total = int(rng.integers(0, k)) if kind == "short" else (1 if k == 1 else int(rng.integers(1, k)))
        live = np.ones(nparts, bool)
        if kind == "short" and nparts >= 3:
            live[nparts // 2] = False
        sizes = np.zeros(nparts, np.int64)
        sizes[live] = rng.multinomial(total, np.full(int(live.sum()), 1.0 / live.sum()))
        return sizes
    options = np.array([0, 1, k // 2, k - 1, k, k + 1, k + k // 3 + 2, 2 * k], np.int64)
    return rng.choice(options, size=nparts)


def merge_case(nparts, k, nq, kind, seed):
    """(ids[G, nq, k] int64, scores[G, nq, k] float32) that satisfy k_merge_topk's precondition: parts hold ascending id
    ranges, each part is ranked (score descending, lower id first), unused slots are -1 / -FLT_MAX at the tail of a part.

    One pool of (id, score) per query is cut by id range into nparts pieces whose sizes are drawn separately (0 and sizes
    above k included); each piece keeps its best k.  `kind`: distinct (normal scores), ties (scores from {-1, -0.0, +0.0, 0.5}),
    short (every part and the total below k, a middle part empty), empty (nothing real), extremes (+inf, -inf, +-FLT_MAX among
    ordinary scores; query 0 stays below k entries and holds a real entry whose score is -FLT_MAX, the padding score)."""
    assert kind in MERGE_KINDS, kind
    rng = np.random.default_rng([seed, nparts, k, nq, MERGE_KINDS.index(kind)])
    ids = np.full((nparts, nq, k), -1, np.int64)
    scores = np.full((nparts, nq, k), -FLT_MAX, np.float32)
    for q in range(nq):
        sizes = _sizes(rng, kind, nparts, k, q)
        total = int(sizes.sum())
        if total == 0:
            continue
        pool_ids = np.sort(rng.choice(4 * total + 16, size=total, replace=False)).astype(np.int64) + ID_BASE
        pool_sc = _scores(rng, kind, total)
        if kind == "extremes" and q == 0:
            planted = np.array([-FLT_MAX, -np.inf, np.inf, FLT_MAX], np.float32)[:total]
            pool_sc[rng.choice(total, size=planted.size, replace=False)] = planted
        cut = np.concatenate([[0], np.cumsum(sizes)])
        for g in range(nparts):
            pi, ps = pool_ids[cut[g]:cut[g + 1]], pool_sc[cut[g]:cut[g + 1]]
            o = canonical_order(pi, ps)[:k]
            ids[g, q, :o.size] = pi[o]
            scores[g, q, :o.size] = ps[o]
    return ids, scores


def merge_reference(ids, scores, k):
    """The k best real entries of all parts per query: score descending, lower id first, padded with -1 / -FLT_MAX.
    Scores are copies of the source entries (a -0.0 stays -0.0)."""
    nparts, nq, kk = ids.shape
    assert kk == k and scores.shape == ids.shape
    out_ids = np.full((nq, k), -1, np.int64)
    out_sc = np.full((nq, k), -FLT_MAX, np.float32)
    for q in range(nq):
        i, s = ids[:, q, :].reshape(-1), scores[:, q, :].reshape(-1)
        real = i >= 0
        i, s = i[real], s[real]
        o = canonical_order(i, s)[:k]
        out_ids[q, :o.size] = i[o]
        out_sc[q, :o.size] = s[o]
    return out_ids, out_sc


def fuse_case(n, kind, seed):
    """(a, b) float32 [n] for vf_fuse_rank.  `kind`: random; all_equal (every a + b the same); two_valued; zeros (x + -x = +0.0
    and -0.0 + -0.0 = -0.0, interleaved); inf (FLT_MAX + FLT_MAX, inf + 1, -inf + 1 among ordinary sums; never inf + -inf)."""
    assert kind in FUSE_KINDS, kind
    rng = np.random.default_rng([seed, n, FUSE_KINDS.index(kind)])
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    i = np.arange(n)
    if kind in ("all_equal", "two_valued"):
        a = (rng.integers(-8, 9, size=n) / 4.0).astype(np.float32)            # quarters: target - a is exact
        target = np.float32(1.5) if kind == "all_equal" else rng.choice(np.array([1.5, -2.25], np.float32), size=n)
        b = (target - a).astype(np.float32)
    elif kind == "zeros":
        b = np.where(i % 2 == 0, -a, np.float32(-0.0)).astype(np.float32)
        a = np.where(i % 2 == 0, a, np.float32(-0.0)).astype(np.float32)
    elif kind == "inf":
        a = np.select([i % 4 == 0, i % 4 == 1, i % 4 == 2], [FLT_MAX, np.float32(np.inf), np.float32(-np.inf)], a).astype(np.float32)
        b = np.select([i % 4 == 0, i % 4 == 1, i % 4 == 2], [FLT_MAX, np.float32(1), np.float32(1)], b).astype(np.float32)
    return a, b


def fuse_sums(a, b):
    """np.float32 a + b (an overflow to inf is the intended value of the `inf` kind)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float32) + np.asarray(b, np.float32)


def tied_corpus(n, groups, d, seed):
    """(rows [n, d] fp32, vectors [groups, d] fp32): row i is the unit vector vectors[i % groups].  Equal rows score bit-equal
    against any query, so every group is one tie set of about n / groups rows whose members interleave in id order."""
    rng = np.random.default_rng([seed, n, groups, d])
    v = rng.standard_normal((groups, d))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    return np.ascontiguousarray(v[np.arange(n) % groups]), v


def tied_queries(vectors, seed):
    """Three queries for a tied corpus: two random ones and one that EQUALS a group vector (its group scores highest)."""
    rng = np.random.default_rng([seed, 77])
    q = rng.standard_normal((3, vectors.shape[1])).astype(np.float32)
    q[1] = vectors[len(vectors) // 2]
    return q


def negative_zero_case(n=4, d=32):
    """(rows [n, d] fp32, query [1, d] fp32, want_ids [n]) whose canonical dot product is -0.0 for rows 0 and 3: the query is
    large where those rows are subnormal and the reverse, and every product is negative and rounds to zero, so all sixteen
    partial sums are -0.0.  Row 1 scores 1 / sqrt(2); row 2 and rows from 4 on are all zeros and score +0.0.  -0.0 ties with
    +0.0, so the zero-scoring rows rank by id, and a search reports each of them as +0.0."""
    assert n >= 4 and d % 2 == 0
    tiny = np.float32(2.0 ** -147)        # times the 1 / sqrt(d / 2) of the normalisation: the smallest subnormal or nearly
    h = d // 2
    query = np.empty((1, d), np.float32)
    query[0, :h], query[0, h:] = 1.0, tiny
    rows = np.zeros((n, d), np.float32)
    rows[0, :h], rows[0, h:] = -tiny, -1.0
    rows[1] = 1.0
    rows[3] = rows[0]
    want = np.concatenate([[1, 0], np.arange(2, n)]).astype(np.int64)
    return rows, query, want


# the merge shapes of tests/test_gpu_rank_kernels.py (nparts, k, nq); the host test holds the two references to each other on them
MERGE_SHAPES = (
    (1, 1, 1),          # smallest
    (3, 7, 5),          # nq * k * 12 = 420: the packed stride is padded to 432
    (2, 1024, 2),       # m = 2048, last counting case; a thread owns two keys
    (8, 256, 2),        # m = 2048 with many parts
    (3, 683, 1),        # m = 2049, first bitonic case, P = 4096
    (2, 1025, 2),       # m = 2050, k > 1024 output loop
    (5, 100, 64),       # the sharded retriever's shape
    (2, 8192, 1),       # m = 16384, the chunked path's largest merge
    (16, 1024, 1),      # m = 16384 with many parts
    (1, 16384, 1),      # one part, largest k
)
FUSE_SIZES = (0, 1, 2, 3, 1023, 1024, 1025, 2048, 4095, 4096)


def check_merge_precondition(ids, scores):
    """Assert what k_merge_topk is promised: padding only at a part's tail, parts canonically ranked, id ranges ascending."""
    nparts, nq, k = ids.shape
    for q in range(nq):
        last_max = -1
        for g in range(nparts):
            i, s = ids[g, q], scores[g, q]
            real = i >= 0
            cnt = int(real.sum())
            assert real[:cnt].all() and not real[cnt:].any(), (q, g, "padding inside a part")
            assert np.all(i[cnt:] == -1) and np.all(s[cnt:] == -FLT_MAX), (q, g, "padding values")
            if cnt == 0:
                continue
            assert np.all(i[:cnt] >= ID_BASE)
            hi, lo = s[:cnt - 1], s[1:cnt]
            assert np.all((hi > lo) | ((hi == lo) & (i[:cnt - 1] < i[1:cnt]))), (q, g, "part not canonically ranked")
            assert i[:cnt].min() > last_max, (q, g, "id ranges not ascending")
            last_max = int(i[:cnt].max())
