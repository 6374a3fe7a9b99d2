"""Which kernels serve a search (veritasfi_amd/csrc/vf_route.h), decided on the CPU: a host-compiled driver (tests/scan_route_driver.py,
UBSan) routes a table of pinned searches and walks the option grid against the route's invariants.  No GPU.

The table was derived by reading the routing code as it stood before it moved into the header; the GPU suite's `scan_kernel`,
`scan_image`, `wide_launches`, `aux_cus` and `scans_overlap` assertions pin the same behaviour on the card.  Unless a row says otherwise:
256 CUs, CU masking available, every option at its default, k = 100, the scan copy present iff n > 16 384, no image.
`sample` / `scan_kernel` are the vf_search_stats.scan_kernel codes: 1 k_scan, 2 k_scan2, 3 k_scan_wide, 4 k_scan_wide8, 5 k_scan2r,
6 k_scan_ksplit, 7 k_scan_ksplit8 / k_scan_ksplit8i.  Row forms: 0 fp16, 1 e4m3, 2 int8 converted, 3 / 4 the int8 instruction with one / two
query planes."""
import pytest

import scan_route_driver as drv

M = 1_000_000
F16_17K = dict(dtype="f16", n=17000, d=768, nq=64)
F16_1250K = dict(dtype="f16", n=1_250_000, d=768, nq=64)
E4M3_1M = dict(dtype="e4m3", n=M, d=768)
I8_IMG = dict(dtype="int8", n=M, d=768, nq=64, has_image=1)
F16_17K_WIDE = dict(dtype="f16", n=17000, d=2560)
E4M3_32K_WIDE = dict(dtype="e4m3", n=32768, d=2560)

# (name, the search, what its route must show)
TABLE = [
    ("small corpus", dict(dtype="f16", n=16384, d=768, nq=1), dict(path=0, scan_kernel=0)),
    ("k at the fused limit", dict(dtype="f16", n=17000, d=768, nq=1, k=2048), dict(path=1)),
    ("k past the fused limit", dict(dtype="f16", n=17000, d=768, nq=1, k=2049), dict(path=2, scan_kernel=0)),
    ("forced fused, 1000 rows", dict(dtype="f16", n=1000, d=768, force_path=1), dict(path=-1)),
    ("forced fused, no scan copy", dict(dtype="f16", n=5000, d=768, has_scan=0, force_path=1), dict(path=-1)),
    ("17000 x 768", F16_17K, dict(path=1, aux_cus=32, tile=64, sample=5, scan_kernel=2)),
    ("17000 x 768, aux_cus 0", dict(F16_17K, aux_cus=0), dict(path=1, aux_cus=0, sample=1, scan_kernel=2)),
    ("17000 x 768, scan_impl 1", dict(F16_17K, scan_impl=1), dict(aux_cus=32, sample=1, scan_kernel=1)),
    ("1.25M x 768", F16_1250K, dict(sample=5, scan_kernel=5)),
    ("1.25M x 768, overlap_scans 0", dict(F16_1250K, overlap_scans=0), dict(scan_kernel=2)),
    ("1.25M x 768, steal 1", dict(F16_1250K, steal=1), dict(aux_cus=32, scan_kernel=1)),
    ("1M x 1024, 64 queries", dict(dtype="f16", n=M, d=1024, nq=64), dict(tile=64, sample=5, scan_kernel=1)),
    ("1M x 1024, 32 queries", dict(dtype="f16", n=M, d=1024, nq=32), dict(tile=32, sample=5, scan_kernel=2)),
    ("2M x 1024", dict(dtype="f16", n=2 * M, d=1024, nq=64), dict(scan_kernel=5)),
    ("2M x 640", dict(dtype="f16", n=2 * M, d=640, nq=64), dict(aux_cus=32, sample=1, scan_kernel=2)),
    ("200000 x 2432", dict(dtype="f16", n=200000, d=2432, nq=64), dict(per_pass=32, passes=2, scan_kernel=1)),
    ("e4m3 1M x 768", dict(E4M3_1M, nq=64), dict(sample=1, scan_kernel=1)),
    ("e4m3 1.25M x 768", dict(E4M3_1M, n=1_250_000, nq=64), dict(sample=5, scan_kernel=5)),
    ("e4m3 1.25M x 768, scan_impl 3", dict(E4M3_1M, n=1_250_000, nq=64, scan_impl=3), dict(scan_kernel=2)),
    ("1M x 768, 65 queries", dict(dtype="f16", n=M, d=768, nq=65), dict(wide=1, scan_kernel=3)),
    ("1M x 768, 65 queries, wide 0", dict(dtype="f16", n=M, d=768, nq=65, wide=0), dict(wide=0, scan_kernel=2)),
    ("e4m3 1M x 768, 128 queries", dict(E4M3_1M, nq=128), dict(wide=0, scan_kernel=1)),
    ("e4m3 1M x 768, 129 queries", dict(E4M3_1M, nq=129), dict(wide=1, scan_kernel=4)),
    ("e4m3 1M x 768, 129 queries, wide_mfma 0", dict(E4M3_1M, nq=129, wide_mfma=0), dict(wide=1, scan_kernel=3)),
    ("int8 1M x 768, no image", dict(dtype="int8", n=M, d=768, nq=64), dict(sample=1, scan_kernel=1, scan_image=0)),
    ("int8 1M x 768, image", I8_IMG, dict(scan_image=1, planes=1, sample=5, scan_kernel=5, sample_rows=3, main_rows=3)),
    ("int8 image, image_mfma 0", dict(I8_IMG, image_mfma=0), dict(scan_image=1, planes=0, scan_kernel=5, sample_rows=2, main_rows=2)),
    ("int8 image, image_mfma 2", dict(I8_IMG, image_mfma=2), dict(scan_image=1, planes=2, scan_kernel=5, sample_rows=4, main_rows=4)),
    ("int8 image, k 129", dict(I8_IMG, k=129), dict(scan_image=0, scan_kernel=1)),
    ("int8 image, scan_impl 1", dict(I8_IMG, scan_impl=1), dict(scan_image=0, scan_kernel=1)),
    ("int8 image, 130 queries", dict(I8_IMG, nq=130), dict(wide=1, scan_kernel=3, scan_image=0)),
    ("4M x 768 with image, k 100", dict(dtype="f16", n=4 * M, d=768, nq=64, has_image=1, k=100), dict(scan_kernel=5, scan_image=1)),
    ("4M x 768 with image, k 200", dict(dtype="f16", n=4 * M, d=768, nq=64, has_image=1, k=200), dict(scan_kernel=5, scan_image=0)),
    ("200000 x 2560, 32 queries", dict(dtype="f16", n=200000, d=2560, nq=32), dict(tile=32, sample=6, scan_kernel=6)),
    ("200000 x 2560, 33 queries", dict(dtype="f16", n=200000, d=2560, nq=33), dict(wide=1, scan_kernel=3)),
    ("17000 x 2560", F16_17K_WIDE, dict(path=2)),
    ("17000 x 2560, wide_rows 2", dict(F16_17K_WIDE, wide_rows=2), dict(path=1, scan_kernel=6)),
    ("17000 x 2560, force_path 1", dict(F16_17K_WIDE, force_path=1), dict(path=1, scan_kernel=6)),
    ("17000 x 2560, wide_rows 0, force_path 1", dict(F16_17K_WIDE, wide_rows=0, force_path=1), dict(path=-1)),
    ("200000 x 4097", dict(dtype="f16", n=200000, d=4097), dict(path=2)),
    ("200000 x 4097, force_path 1", dict(dtype="f16", n=200000, d=4097, force_path=1), dict(path=-1)),
    ("e4m3 32768 x 2560, 64 queries", dict(E4M3_32K_WIDE, nq=64), dict(per_pass=32, passes=2, scan_kernel=7, main_rows=1)),
    ("e4m3 32768 x 2560, 65 queries", dict(E4M3_32K_WIDE, nq=65), dict(wide=1, scan_kernel=3)),
    ("e4m3 32768 x 2560, 65 queries, wide_mfma 1", dict(E4M3_32K_WIDE, nq=65, wide_mfma=1), dict(wide=1, scan_kernel=4)),
    ("e4m3 32768 x 2688, 65 queries", dict(E4M3_32K_WIDE, d=2688, nq=65), dict(wide=0, scan_kernel=7)),
    ("e4m3 32767 x 2560", dict(E4M3_32K_WIDE, n=32767, nq=1), dict(path=2)),
    ("int8 32768 x 2560", dict(dtype="int8", n=32768, d=2560, nq=32), dict(scan_kernel=7, main_rows=2)),
    ("int8 17000 x 2560, wide_rows 2", dict(dtype="int8", n=17000, d=2560, wide_rows=2), dict(path=2)),
    ("int8 17000 x 2560, force_path 1", dict(dtype="int8", n=17000, d=2560, force_path=1), dict(path=-1)),
]

# What a pass is launched with beside its kernels -- refresh_every, clear_sample, scan_bytes of the search's FIRST pass -- derived by hand
# from the expressions as they stood in vf_api.hip's begin_impl (narrow passes) and wide_pass before they moved into the header.
#   narrow refresh_every = min(256, max(4, max(1, option) * nb / 64)) rounded down to a power of two
#   wide   refresh_every = the largest power of two <= min(256, max(1, option))
#   narrow clear_sample  = n / total_waves < samp            wide clear_sample = n / rgroups < samp * 8
#   scan_bytes = (n - sampled rows) x bytes per row: d x (1 or 2) + 4, the int8 image dp + 8;
#     sampled = total_waves x min(samp, n / total_waves), wide: rgroups x min(samp * 8, n / rgroups)
F16_1M_WIDE = dict(dtype="f16", n=M, d=768, nq=65)          # one wide pass: 65 queries pad to one tile of 256, 256 CUs / 1 tile = 256 row groups,
                                                            # one query tile samples 32 x 8 = 256 rows per group
F16_WAVES = dict(dtype="f16", d=768, nq=1, waves=320, sample_rows=64)   # waves = 320: 40 workgroups of 8 waves; 64 sample rows per wave
TABLE += [
    ("refresh 128, 64 queries", dict(F16_17K, refresh_every=128), dict(wide=0, refresh_every=128)),        # 128 * 64 / 64 = 128
    ("refresh 128, 33 queries", dict(F16_17K, nq=33, refresh_every=128), dict(wide=0, refresh_every=64)),  # 128 * 33 / 64 = 66 -> 64
    ("refresh 128, 1 query", dict(F16_17K, nq=1, refresh_every=128), dict(refresh_every=4)),               # 128 * 1 / 64 = 2 -> the floor of 4
    ("refresh 1, 64 queries", dict(F16_17K, refresh_every=1), dict(refresh_every=4)),                      # 1 -> the floor of 4
    ("refresh 256, 64 queries", dict(F16_17K, refresh_every=256), dict(refresh_every=256)),                # 256 * 64 / 64 = 256, the ceiling
    ("wide, refresh 128", dict(F16_1M_WIDE, refresh_every=128), dict(wide=1, refresh_every=128)),
    ("wide, refresh 100", dict(F16_1M_WIDE, refresh_every=100), dict(wide=1, refresh_every=64)),           # largest power of two <= 100
    ("wide, refresh 1", dict(F16_1M_WIDE, refresh_every=1), dict(wide=1, refresh_every=1)),                # no floor on a wide pass
    # 320 waves: 20480 / 320 = 64 rows per wave, not fewer than the 64 sampled; one row less and 20479 / 320 = 63 < 64
    ("clear_sample, narrow, at the boundary", dict(F16_WAVES, n=20480), dict(path=1, total_waves=320, samp=64, clear_sample=0)),
    ("clear_sample, narrow, below it", dict(F16_WAVES, n=20479), dict(path=1, total_waves=320, samp=64, clear_sample=1)),
    # 256 row groups sampling 256 rows each: 65536 / 256 = 256 is enough, 65535 / 256 = 255 is not
    ("clear_sample, wide, at the boundary", dict(F16_1M_WIDE, n=65536), dict(wide=1, clear_sample=0)),
    ("clear_sample, wide, below it", dict(F16_1M_WIDE, n=65535), dict(wide=1, clear_sample=1)),
    # fp16 17000 x 768: 224 scan CUs but 17000 / 512 = 33 workgroups = 264 waves sampling 8 rows each (64 per wave are there):
    # (17000 - 264 * 8) * (768 * 2 + 4) = 14888 * 1540
    ("scan_bytes, fp16", F16_17K, dict(grid=33, total_waves=264, samp=8, scan_bytes=22_927_520)),
    # e4m3 1M x 768: 224 workgroups = 1792 waves x 8 sample rows: (1000000 - 14336) * (768 + 4) = 985664 * 772
    ("scan_bytes, e4m3", dict(E4M3_1M, nq=64), dict(grid=224, total_waves=1792, samp=8, scan_bytes=760_932_608)),
    # the int8 image of 1M x 768: the same grid and sample, dp + 8 = 776 bytes per row: 985664 * 776
    ("scan_bytes, image", I8_IMG, dict(scan_image=1, grid=224, total_waves=1792, samp=8, scan_bytes=764_875_264)),
    # wide, fp16 1M x 768: 256 row groups x 256 sample rows: (1000000 - 65536) * 1540 = 934464 * 1540
    ("scan_bytes, wide", F16_1M_WIDE, dict(wide=1, scan_bytes=1_439_074_560)),
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return drv.build(tmp_path_factory.mktemp("scan_route"))


def test_pinned_routes(driver):
    got = drv.evaluate(driver, [case for _, case, _ in TABLE])
    wrong = []
    for (name, case, want), g in zip(TABLE, got):
        print(name, g)
        bad = {key: (g[key], v) for key, v in want.items() if g[key] != v}
        if bad:
            wrong.append((name, bad))
    assert not wrong, "route differs (got, expected): %r" % wrong


def test_every_route_of_the_option_grid_holds_the_invariants(driver):
    run = drv.sweep(driver)
    print(run.stdout[-3000:], run.stderr[-3000:])
    assert run.returncode == 0 and " 0 failure(s)" in run.stdout and "runtime error" not in run.stderr
