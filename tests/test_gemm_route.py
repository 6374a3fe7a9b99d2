"""Which kernel serves a matrix product (veritasfi_amd/csrc/vf_gemm_route.h), decided on the CPU: a host-compiled driver
(tests/gemm_route_driver.py, UBSan) routes a table of pinned products and walks the shape / knob grid against what the kernels rely on.
No GPU.

The table was derived by reading gemm() as it stood before its arithmetic moved into the header; tests/test_gpu_encoder.py's
test_gemm_splitk_tail_*, test_gemm9_whole_product_split_* and stream-K tests pin the cuts and their counters on the card.  Unless a row
says otherwise: 256 CUs, a 64 MiB workspace, every knob at its default.  Epilogue codes: 0 bias, 1 GELU, 2 bias + residual, 3 fp32
residual, 11 quick-GELU.  A route is (kernel, grid, slices, tail tiles, full tiles, stagger ticks); what a kernel has none of is 0."""
import pytest

import gemm_route_driver as drv


def _r(kernel, grid, slices=0, tail=0, full=0, ticks=0):
    return dict(kernel=drv.KERNELS[kernel], grid=grid, slices=slices, tail=tail, full=full, ticks=ticks)


def _p(M, N, K, epi, **kw):
    return dict(M=M, N=N, K=K, epi=epi, **kw)


# (the product, its route)
TABLE = [
    (_p(51200, 768, 768, 2), _r("gemm9", 256, ticks=2000)),
    (_p(51200, 2304, 768, 0), _r("gemm9", 256, ticks=2000)),
    (_p(51200, 3072, 768, 1), _r("gemm9", 256, ticks=2000)),
    (_p(51200, 3072, 768, 11), _r("gemm9", 256, ticks=2000)),
    (_p(51200, 768, 3072, 2), _r("8p", 688, 2, 88, 512)),
    (_p(51200, 1024, 4096, 2), _r("8p", 832, 2, 32, 768)),
    (_p(25600, 768, 3072, 2), _r("8p", 352, 2, 44, 256)),
    (_p(25600, 768, 3072, 2, splitk_tail=0), _r("gemm9", 256, ticks=7400)),
    (_p(6656, 3072, 3072, 1), _r("8p", 368, 2, 56, 256)),
    (_p(38400, 768, 3072, 2), _r("gemm9", 256, ticks=7400)),
    (_p(25600, 1024, 4096, 2), _r("gemm9", 256, ticks=9800)),
    (_p(12800, 768, 3072, 2), _r("gemm9", 150)),
    (_p(6656, 2304, 768, 0), _r("gemm9", 234)),
    (_p(32768, 256, 768, 0), _r("gemm9", 128)),
    (_p(32512, 256, 768, 0), _r("tn128", 508)),
    (_p(6656, 768, 768, 2), _r("tn128", 312)),
    (_p(6528, 768, 768, 0), _r("tn128", 306)),
    (_p(6656, 768, 3072, 2), _r("gemm9-split", 240, 3)),
    (_p(6656, 768, 3072, 11), _r("tn128", 312)),
    (_p(4096, 768, 3072, 1), _r("gemm9-split", 192, 4)),
    (_p(6656, 1024, 4096, 2), _r("gemm9-split", 208, 2)),
    (_p(6656, 1024, 4096, 2, gemm9_split=0), _r("8p", 208, 2, 104, 0)),
    (_p(6656, 1024, 4096, 2, ws=0), _r("tn128", 416)),
    (_p(6656, 768, 3072, 2, kind=10), _r("gemm9", 78)),
    (_p(25600, 768, 768, 0, kind=7, splitk_tail=2), _r("8p", 448, 4, 44, 256)),
    (_p(3328, 1024, 1024, 0, kind=7, splitk_tail=2), _r("8p", 224, 4, 52, 0)),
    (_p(12288, 1024, 96, 0), _r("dma16", 384)),
    (_p(8192, 2560, 2560, 3), _r("8p", 320)),
    (_p(4096, 2560, 2560, 3), _r("tn128", 640)),
    (_p(51200, 768, 3072, 2, n_cu=304), _r("gemm9", 304, ticks=7400)),
]

# The small decisions beside gemm(), at the boundaries their comments name (read off the code as it stood in vf_transformer.hip).
SMALL = [
    # the gated front half takes the 8-phase kernel from 384 tiles of 256 x 256 over its 2 F columns, whole tiles, K >= 128
    (dict(fn="gated", M=24576, F=512, K=2560), dict(ok=1)),      # 96 x 4 = 384 tiles
    (dict(fn="gated", M=24320, F=512, K=2560), dict(ok=0)),      # 95 x 4 = 380
    (dict(fn="gated", M=24704, F=512, K=2560), dict(ok=0)),      # M % 256
    (dict(fn="gated", M=24576, F=192, K=2560), dict(ok=0)),      # 2 F % 256
    (dict(fn="gated", M=24576, F=512, K=128), dict(ok=1)),
    (dict(fn="gated", M=24576, F=512, K=64), dict(ok=0)),
    (dict(fn="gated", M=24576, F=512, K=2592), dict(ok=0)),      # K % 64
    # the skinny kernel's slice count: K >= 2048, at most 64 column tiles, slices of whole 256-element steps, at most 256 workgroups
    (dict(fn="skinny", N=768, K=3072), dict(slices=4)),
    (dict(fn="skinny", N=768, K=2048), dict(slices=4)),
    (dict(fn="skinny", N=768, K=1792), dict(slices=1)),
    (dict(fn="skinny", N=1024, K=4096), dict(slices=4)),
    (dict(fn="skinny", N=1040, K=4096), dict(slices=1)),          # 65 column tiles
    (dict(fn="skinny", N=512, K=4096), dict(slices=8)),
    (dict(fn="skinny", N=768, K=3072, can_split=0), dict(slices=1)),
    # k_gemm_splitk's split count: whole K-steps, at least two per split, at most 512 workgroups, at most 8
    (dict(fn="splits", tiles=12, K=3072), dict(splits=8)),
    (dict(fn="splits", tiles=16, K=4096), dict(splits=8)),
    (dict(fn="splits", tiles=12, K=768), dict(splits=6)),
    (dict(fn="splits", tiles=100, K=3072), dict(splits=4)),
    (dict(fn="splits", tiles=600, K=3072), dict(splits=1)),
    (dict(fn="splits", tiles=12, K=128), dict(splits=1)),
    # the encoder forward's product class: 0 general, 1 skinny, 2 split-K (the FFN-down product of a single short sequence)
    (dict(fn="enc", M=64, H=768, F=3072), dict(cls=1)),
    (dict(fn="enc", M=64, H=768, F=3072, ffn_down=1), dict(cls=1)),
    (dict(fn="enc", M=1, H=1024, F=4096, ffn_down=1), dict(cls=1)),
    (dict(fn="enc", M=65, H=768, F=3072), dict(cls=0)),
    (dict(fn="enc", M=65, H=768, F=3072, ffn_down=1), dict(cls=0)),                    # 65 rows pad to 128 > 64
    (dict(fn="enc", M=64, H=768, F=3072, ffn_down=1, allow_skinny=0), dict(cls=2)),
    (dict(fn="enc", M=64, H=768, F=3072, ffn_down=0, allow_skinny=0), dict(cls=0)),    # the K = hidden products are never split
    (dict(fn="enc", M=64, H=384, F=2048, ffn_down=1), dict(cls=2)),                    # H % 256: not skinny
    (dict(fn="enc", M=64, H=384, F=1984, ffn_down=1), dict(cls=0)),                    # F < 2048
    (dict(fn="enc", M=64, H=384, F=2048, ffn_down=1, allow_splitk=0), dict(cls=0)),
    (dict(fn="enc", M=64, H=352, F=2048, ffn_down=1), dict(cls=0)),                    # H % 64
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("gemm_route"))


def _compare(driver, table):
    got = drv.evaluate(driver, [case for case, _ in table])
    wrong = []
    for (case, want), g in zip(table, got):
        print(case, g)
        if g != want:
            wrong.append((case, g, want))
    assert not wrong, "differs (case, got, expected): %r" % wrong


def test_pinned_routes(driver):
    _compare(driver, TABLE)


def test_small_decisions_at_their_boundaries(driver):
    _compare(driver, SMALL)


def test_every_route_of_the_grid_holds_what_the_kernels_rely_on(driver):
    run = drv.sweep(driver)
    print(run.stdout[-3000:], run.stderr[-3000:])
    assert run.returncode == 0 and " 0 failure(s)" in run.stdout and "runtime error" not in run.stderr
    assert " 46448640 products checked" in run.stdout   # the whole grid was walked
