"""vf_index_set_option through a live handle: the option table's rows (tests/option_table_driver.py holds the expectation,
tests/test_options.py walks the table itself on the CPU) on a plain index of 2 000 x 64 fp16 rows and on a group of two shards of
20 000 x 64 each, both on device 0 (20 000 rows per shard: a shard of 10 000 would sit on the small dense path and report no scan
kernel at all).

One refused value per option raises with the table's message, on the group from the shard the value was forwarded to; every accepted
edge value is taken; an option the group forwards shows in its shards' next search (scan_kernel against the host driver's prediction,
tests/scan_route_driver.py); aux_cus is fixed once the first search has created the slot's streams but may be set to what it is; and
after all of it the ids are still the NumPy oracle's (oracle/ref_numpy.py; the test checks that oracle's own top-k has no near tie, so
its fp32 BLAS order is the only order)."""
import numpy as np
import pytest

import option_table_driver as opt
import scan_route_driver as drv

pytestmark = pytest.mark.gpu

D, K, NQ = 64, 10, 8
FROZEN = "aux_cus is fixed once the first search has created the scan streams: set it before searching"


@pytest.fixture(scope="module")
def vf():
    import veritasfi_amd as m
    from veritasfi_amd import _ffi
    _ffi.lib()  # raises if the HIP library is missing: no fallback
    n = _ffi.c_i32(0)
    _ffi.check(_ffi.lib().vf_device_count(n), "vf_device_count")
    assert n.value >= 1, "no GPU visible"
    return m


@pytest.fixture(scope="module")
def rows():
    return opt.rows(experiments=opt.library_is_test_build())


@pytest.fixture(scope="module")
def data():
    """Corpus (40 000 x 64 fp16; the plain index holds its first 2 000 rows), queries, the NumPy oracle's ids for both."""
    from oracle import ref_numpy
    rng = np.random.default_rng(12)
    c = rng.standard_normal((40_000, D), dtype=np.float32).astype(np.float16)
    q = rng.standard_normal((NQ, D), dtype=np.float32)
    want = {}
    for n in (2_000, 40_000):
        ids, sc = ref_numpy.faiss_flat_ip_search(c[:n], q, K + 1)
        assert np.min(sc[:, :-1] - sc[:, 1:]) > 1e-5   # no near tie down to the first row left out: the ids do not hang on the arithmetic
        want[n] = ids[:, :K]
    return c, q, want


def _refusals_and_edges(ix, rows):
    for name, dflt, ok, bad, msg in rows:
        if bad:
            with pytest.raises(RuntimeError) as e:
                ix.set_option(name, bad[0])
            assert str(e.value).endswith(": " + msg), (name, bad[0], str(e.value))
        for v in ok + [dflt]:   # (back to the default: the searches below run on the library's own settings)
            ix.set_option(name, v)
    with pytest.raises(RuntimeError) as e:
        ix.set_option("no_such_option", 1)
    assert str(e.value).endswith(": " + opt.UNKNOWN_MESSAGE % "no_such_option")


def _aux_cus_is_fixed(ix, applied):
    """after a search: another value is refused, the one in force is accepted"""
    with pytest.raises(RuntimeError) as e:
        ix.set_option("aux_cus", 16)
    assert str(e.value).endswith(": " + FROZEN)
    ix.set_option("aux_cus", applied)


def test_plain_index(vf, rows, data):
    c, q, want = data
    with vf.DenseIndex(c[:2_000]) as ix:
        _refusals_and_edges(ix, rows)
        ix.set_option("aux_cus", 0)
        ids, _ = ix.search(q, K)
        assert ix.stats()["path"] == 0 and np.array_equal(ids, want[2_000])
        _aux_cus_is_fixed(ix, 0)
        ix.set_option("force_path", 2)
        ids, _ = ix.search(q, K)
        assert ix.stats()["path"] == 2 and np.array_equal(ids, want[2_000])
        ix.set_option("force_path", -1)
        ids, _ = ix.search(q, K)
        assert ix.stats()["path"] == 0 and np.array_equal(ids, want[2_000])


def test_group_forwards_to_its_shards(vf, rows, data, tmp_path):
    import torch
    c, q, want = data
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    shards = [vf.DenseIndex(c[:20_000], device_id=0), vf.DenseIndex(c[20_000:], device_id=0, id_offset=20_000)]
    with vf.DenseIndex.group(shards) as ix:
        assert ix.shard_devices() == [0, 0]
        _refusals_and_edges(ix, rows)
        ix.set_option("aux_cus", 0)
        got = {}
        for wide in (0, NQ):   # never a wide pass / wide passes from NQ queries: rows of 64 elements know k_scan and k_scan_wide only
            ix.set_option("wide", wide)
            ids, _ = ix.search(q, K)
            got[wide] = ix.stats()
            assert np.array_equal(ids, want[40_000]), f"wide = {wide}"
        exe = drv.build(tmp_path)
        pred = drv.evaluate(exe, [dict(dtype="f16", n=20_000, d=D, nq=NQ, k=K, n_cu=n_cu, aux_cus=0, aux_applied=0, wide=w) for w in (0, NQ)])
        print([(g["path"], g["scan_kernel"], g["aux_cus"]) for g in got.values()], [p["scan_kernel"] for p in pred])
        assert pred[0]["scan_kernel"] != pred[1]["scan_kernel"]   # the option makes a difference to see
        for g, p in zip(got.values(), pred):
            assert (g["path"], g["scan_kernel"], g["aux_cus"]) == (1, p["scan_kernel"], 0)
        _aux_cus_is_fixed(ix, 0)
        ix.set_option("force_path", 2)
        ids, _ = ix.search(q, K)
        assert ix.stats()["path"] == 2 and np.array_equal(ids, want[40_000])
        ix.set_option("force_path", -1)
        ix.set_option("wide", 1)
        ids, _ = ix.search(q, K)
        assert ix.stats()["path"] == 1 and ix.stats()["wide_launches"] == 0 and np.array_equal(ids, want[40_000])
