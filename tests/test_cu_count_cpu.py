"""No GPU: the tile assignment of every persistent kernel, copied into tests/cu_model.py, partitions its tile set for every planning CU count
1..320, and every case of tests/test_cu_count_gpu.py meets its conditions.

(1) For each count and a sweep of tile counts — 0 to 3 rounds of the grid and a little more, every tile count for the small counts (so every
    remainder class occurs), the rounds' edges for the large ones — each tile is taken exactly once and no index reaches `tiles`; the slice
    counts 1, 2, 3, 4, 8 for the XCD-sliced kernels. An envelope that divides by a count-derived number rejects the count first.
(2) Every GPU case: the model's conditions at the case's own count (cu_cases.gate), the exact-data gate and the two-order fp32 evaluation of
    tests/exact_ref.py, as tests/test_exact_cpu.py does for its lists. Prints, per case, tiles, grid and the maximum tiles per workgroup.
(3) Mutants of the model — slot and eslot swapped in the remainder round, per_xcd not rounded down to the slices, a grid larger than the tile
    count, the XCD remap without its remainder term, a stale stream count in rf — fail the same partition check, so the check is not vacuous.
"""
import numpy as np
import pytest

import cu_cases as CC
import cu_model as M
import exact_ref as E
import test_exact_cpu as XC
import test_exact_gpu as G

ALL_COUNTS = range(1, 321)
SLICES = (1, 2, 3, 4, 8)


def assert_partition(tiles_seen, tiles, what):
    """every tile of range(tiles) exactly once, none outside"""
    t = np.asarray(tiles_seen, np.int64)
    assert t.size == tiles, "%s: %d visits of %d tiles" % (what, t.size, tiles)
    if tiles:
        assert t.min() >= 0 and t.max() < tiles, "%s: tile index %d .. %d outside [0, %d)" % (what, t.min(), t.max(), tiles)
        assert np.array_equal(np.bincount(t, minlength=tiles), np.ones(tiles, np.int64)), "%s: a tile is taken twice or never" % what


def tile_counts(unit, small):
    """tile counts for a grid of `unit` workgroups (or waves): 0 to 3 rounds. small: every count up to 3 rounds + 2; else the rounds' edges."""
    if small:
        return range(1, 3 * unit + 3)
    edges = {1, 2, 7, 8, 9, unit // 2, unit - 1, unit, unit + 1, unit + 7, 2 * unit - 1, 2 * unit, 2 * unit + 3, 3 * unit - 5, 3 * unit, 3 * unit + 1}
    return sorted(t for t in edges if t >= 1)


# ----------------------------------------------------------------------------- (1) partitions

# persistent grids of min(num_cus * per_cu, tiles) workgroups: (kernel, source of per_cu, per_cu, goes through mbn_xcd_remap)
STRIDED = [
    ("pw_gemm fp32 64x64 / 128x128 / 128x64", "mbn_f32_pw.hip:522-530", (4, 2, 2), True),
    ("pw_gemm_xb tile 11, pw_gemm_x tiles 6 / 7", "mbn_f32_pw_x6.hip:494-501, 532-539", tuple(M.x6_per_cu(t)[2] for t in (11, 6, 7)), True),
    ("fused stem fp32 / bf16, alpha 1 / 0.5", "mbn_f32_stem.hip:573-575, 608", (2, 4, 3, 5), False),
    ("dwpw, dwpw2, dwpw2_x6, bf16 dwpw / dwpw2, ring, wide, big", "mbn_f32_dwpw.hip:222, mbn_f32_dwpw2.hip:597, mbn_f32_dwpw2_x6.hip:266, mbn_bf16_pw_ring.hip:250, mbn_bf16_pw_wide.hip:331", (1,), True),
    ("bf16 stream", "mbn_bf16_pw_stream.hip:417", (2,), True),
]


def test_x6_per_cu_is_what_the_sources_say():
    assert [M.x6_per_cu(t) for t in (11, 6, 7)] == [(128, 128, 2), (128, 128, 2), (128, 64, 3)]
    assert [M.pw_gemm_plan(4096, 64, 256, 256, M.PW_GEMM_F32_TILES[t])["per_cu"] for t in (3, 5, 2, 1)] == [4, 2, 2, 2]


@pytest.mark.parametrize("kernel", STRIDED, ids=lambda k: k[0])
def test_strided_grids_partition_their_tiles(kernel):
    name, _, per_cus, remap = kernel
    for per_cu in set(per_cus):
        for cus in ALL_COUNTS:
            for nwg in tile_counts(cus * per_cu, cus <= 24):
                grid = M.persistent_grid(cus, per_cu, nwg)
                assert 1 <= grid <= nwg
                wg, lid, per = M.strided(nwg, grid, remap)
                assert_partition(lid, nwg, "%s cus %d tiles %d" % (name, cus, nwg))
                assert per.sum() == nwg and per.max() - per.min() <= 1 and np.array_equal(np.bincount(wg, minlength=grid), per)


def p_xn_only(cus, pw_xn, k, cfg):
    """the XCD-group orderings (forced, or from a filter of 4 MB and more) depend on mt, nt and the grid alone: one tile shape, every count up
    to 48 and every eighth beyond; they exist only where the grid is a multiple of 8"""
    return (pw_xn or k >= 1024) and (cfg != (64, 64, 32, 32) or (cus > 48 and cus % 8 != 0))


def test_pw_gemm_launch_and_xcd_groups_partition():
    """launch_cfg for every fp32 tile shape, with and without a second k-tile, and the xn = 2 / 4 groups with vb_end (forced through pw_xn and
    through filter sizes of 4 and 16 MB)."""
    seen_xn = set()
    for cfg in sorted(set(M.PW_GEMM_F32_TILES.values())):
        for cus in ALL_COUNTS:
            for (k, n, pw_xn) in ((8, 3 * cfg[1] + 5, 0), (64, 2 * cfg[1], 0), (64, 5 * cfg[1], 2), (64, 5 * cfg[1], 4), (1024, 1024, 0), (2048, 2048, 0)):
                nt = M.cdiv(n, cfg[1])
                unit = cus * M.pw_gemm_plan(1 << 20, k, n, cus, cfg, pw_xn=pw_xn)["per_cu"]
                if p_xn_only(cus, pw_xn, k, cfg):
                    continue
                for nwg in (tile_counts(unit, True) if cus <= 6 and n <= 1024 else tile_counts(unit, False)):
                    mt = M.cdiv(nwg, nt)
                    p = M.pw_gemm_plan(mt * cfg[0] - 3, k, n, cus, cfg, pw_xn=pw_xn)
                    assert 1 <= p["grid"] <= p["nwg"]
                    if p["nbuf"] == 1:
                        assert p["grid"] == p["nwg"]
                    assert p["xn"] == 1 or p["grid"] % 8 == 0
                    seen_xn.add(p["xn"])
                    wg, mi, ni, per = M.pw_gemm_visits(p)
                    assert mi.max() < p["mt"] and ni.max() < p["nt"] and mi.min() >= 0 and ni.min() >= 0
                    assert_partition(mi * p["nt"] + ni, p["nwg"], "pw_gemm %s cus %d %s mt %d xn %d" % (cfg, cus, (k, n), mt, p["xn"]))
    assert seen_xn == {1, 2, 4}


@pytest.mark.parametrize("nw", [8, 12], ids=["8_waves", "12_waves_k512"])
def test_pw3_dwpw3_partition_per_slice(nw):
    """pw3 (8 waves; 12 at K = 512) and dwpw3 (8 waves): the launcher's per_xcd clamp, then r0, r1, per_round, full, rem, slot, eslot, tile_at."""
    for nh in SLICES:
        for cus in ALL_COUNTS:
            if cus < 8 * nh:
                assert M.pw3_grid(100, nh, cus) is None, "the envelope must reject count %d before per_xcd %% %d" % (cus, nh)
                continue
            per_round = (cus // 8 // nh) * nw
            for tiles in tile_counts(8 * per_round, cus <= 16):
                grid = M.pw3_grid(tiles, nh, cus)
                assert grid >= 8 * nh and grid % (8 * nh) == 0 and grid <= cus
                sl, tile, ntile, _ = M.pw3_visits(tiles, nh, grid, nw)
                assert sl.max() < nh
                for s in range(nh):
                    assert_partition(tile[sl == s], tiles, "pw3 nw %d nh %d cus %d tiles %d slice %d" % (nw, nh, cus, tiles, s))


def test_rf_partition_per_half():
    for nh in SLICES:
        for cus in ALL_COUNTS:
            if cus < 8 * nh:
                assert M.rf_plan(100, nh, cus) is None, "the envelope must reject count %d before gq = cus / 8 / %d" % (cus, nh)
                continue
            for mt in tile_counts(8 * (cus // 8 // nh), cus <= 40):
                p = M.rf_plan(mt, nh, cus)
                assert p["gq"] >= 1 and p["grid"] <= cus
                half, tile, nt = M.rf_visits(mt, nh, p["gq"], p["grid"])
                for h in range(nh):
                    assert_partition(tile[half == h], mt, "rf nh %d cus %d mt %d half %d" % (nh, cus, mt, h))


def test_resident_blocks_tail_poolfc_conv1_partition():
    for cus in ALL_COUNTS:
        for batch in tile_counts(cus, cus <= 24):
            n, per, grid = M.res_visits(batch, cus)
            assert 1 <= grid <= cus
            assert_partition(n, batch, "res cus %d batch %d" % (cus, batch))
            imgs, per, grid = M.tail_visits(batch, cus)
            assert 1 <= grid <= cus
            assert_partition(imgs, batch, "tail cus %d batch %d" % (cus, batch))
        for nblk in tile_counts(cus * 32, False):
            blk, wgs = M.conv1_mfma_visits(nblk, cus)
            assert 1 <= wgs <= cus * 8
            assert_partition(blk, nblk, "conv1 cus %d blocks %d" % (cus, nblk))
        for channels, classes in ((64, 10), (256, 40), (512, 1000), (1024, 1000), (1024, 1001), (1024, 15)):
            p = M.poolfc_plan(channels, classes, cus)
            ks, lo, hi = M.poolfc_visits(p, classes)
            assert p["nns"] >= 1 and np.all(lo < hi) and hi.max() == classes and p["npc"] % 16 == 0
            cells = np.concatenate([k * classes + np.arange(a, b) for k, a, b in zip(ks, lo, hi)])
            assert_partition(cells, p["nks"] * classes, "pool + FC cus %d %d -> %d" % (cus, channels, classes))


def test_depthwise_row_segments_cover_the_rows():
    for cus in ALL_COUNTS:
        for rows in (1, 2, 3, 7, 14, 28, 56, 112):
            for stride in (1, 2):
                for lanes in (1, 49, 1792, 100000, 10 ** 7):
                    for resident in (False, True):
                        sr, ns = M.dw_march_segments(lanes, rows, stride, resident, cus)
                        assert sr >= 1 and ns >= 1 and sr * ns >= rows > sr * (ns - 1), (cus, rows, stride, lanes, sr, ns)
            for batch, ch in ((1, 64), (4, 64), (64, 256)):
                for seg in (M.dw_lds_bf16_segments(batch, rows, rows, ch, cus), M.dw_lds_f32_segments(batch, rows, rows, 1, ch, False, 0, cus)):
                    if seg is None:                  # the bf16 form takes maps up to 62 pixels wide
                        assert rows > 61
                        continue
                    sr, ns = seg
                    assert sr >= 1 and ns >= 1 and sr * ns >= rows > sr * (ns - 1), (cus, rows, batch, ch, sr, ns)


# ----------------------------------------------------------------------------- (3) mutants

def _caught(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_partition_check_catches_the_mutants():
    # slot where the kernel has eslot in the remainder round: needs more than one workgroup per slice and XCD (16 CUs and up)
    def swapped():
        for cus in (16, 24, 72):
            for tiles in tile_counts(8 * (cus // 8) * 8, True):
                grid = M.pw3_grid(tiles, 1, cus)
                sl, tile, _, _ = M.pw3_visits(tiles, 1, grid, 8, mutant="swap")
                assert_partition(tile, tiles, "swap")
    # per_xcd not rounded down to the slices: 72 CUs, 2 / 4 / 8 slices
    def not_rounded():
        for nh in (2, 4, 8):
            tiles = 5000
            grid = (72 // 8) * 8
            sl, tile, _, _ = M.pw3_visits(tiles, nh, grid, 8)
            for s in range(nh):
                assert_partition(tile[sl == s], tiles, "per_xcd % nh != 0")
    # a grid that is not clamped to the tiles: workgroups past the last tile must take nothing (the kernels return: blockIdx >= nwg)
    def unclamped():
        wg, lid, per = M.strided(5, 12)
        assert per.sum() == 5 and np.all(per[5:] == 0)
        assert_partition(np.arange(12), 5, "every workgroup takes blockIdx")
    # the remap without its remainder term
    def remap_without_remainder():
        for nwg in range(1, 40):
            vb = np.arange(nwg)
            assert_partition((vb & 7) * (nwg >> 3) + (vb >> 3), nwg, "remap")
    # rf: gq not shrunk to the streams that have a tile is still a partition, but gq taken from the device's count while the grid comes from the planning count is not
    def rf_stale_gq():
        mt, nh = 37, 1
        p = M.rf_plan(mt, nh, 8)
        half, tile, nt = M.rf_visits(mt, nh, 256 // 8, p["grid"])
        assert_partition(tile, mt, "rf")
    for name, fn in (("slot / eslot swapped", swapped), ("per_xcd not rounded", not_rounded), ("unclamped grid", unclamped),
                     ("remap without remainder", remap_without_remainder), ("rf stale gq", rf_stale_gq)):
        assert _caught(fn), "mutant (%s) passes the partition check" % name
    # ... and the true model passes the very same calls
    for cus in (16, 24, 72):
        for tiles in tile_counts(8 * (cus // 8) * 8, True):
            assert_partition(M.pw3_visits(tiles, 1, M.pw3_grid(tiles, 1, cus), 8)[1], tiles, "true")


# ----------------------------------------------------------------------------- (2) the GPU cases

@pytest.mark.parametrize("case", CC.EXACT_CASES, ids=CC.case_id)
def test_gpu_case_meets_its_conditions(case):
    print("%s: %s" % (CC.case_id(case), CC.gate(case)))
    if case.kind in ("pw_f32", "pw_bf16"):
        # forced routes: inside the forced kernel's envelope at the case's count (the GPU test repeats this per count), as test_exact_cpu.py does
        assert G.pw_route_eligible(case.knobs, case.shape, case.count), case
    XC._gate(list(CC.layers(case)), CC.case_id(case))
    if case.kind == "pw_f32" and case.knobs.get("pw_emul"):
        l = CC.layers(case)[0]
        for a in (l.x, l.w):
            assert np.array_equal(E.bf16_rne(a), a), "pw_emul's split is exact for operands of at most 8 significant bits"


@pytest.mark.parametrize("case", CC.I8, ids=lambda c: "i8-%dx%d-%s-cus%d" % (c.shape[0], c.shape[1], "f32" if c.shape[2] else "u8", c.count))
def test_gpu_int8_case_meets_its_conditions(pkg, case):
    import test_int8_gpu as I8
    m, k, n, f32 = CC.i8_shape(pkg, case, I8)
    p = pkg.i8_pw_plan(m, k, n, case.count, True, f32)
    I8._assert_multipass(pkg, p, m)
    assert m <= 70000
    print("i8 %d -> %d m=%d at count %d: %s" % (k, n, m, case.count, I8._plan_str(p, pkg)))


def test_case_lists_cover_the_routes():
    routes = {(c.kind, c.route) for c in CC.ALL_CASES}
    for want in [("pw_f32", r) for r in ("gemm1", "gemm3", "gemm5", "gemm-nbuf1", "gemm-xn2", "pw3", "splitk", "x6-11", "x6-6", "x6-7")] + \
                [("block_f32", r) for r in ("dwpw-128", "dwpw-256", "dwpw2-128", "dwpw2-256", "dwpw3", "x6-128")] + \
                [("pw_bf16", r) for r in ("stream", "stream16", "ring", "wide", "big", "rf")] + \
                [("block_bf16", r) for r in ("dwpw-128", "dwpw2-128", "dwpw2-256", "dwpw2-h32")] + \
                [("dw_f32", "march"), ("dw_f32", "lds"), ("dw_bf16", "march"), ("dw_bf16", "lds"), ("stem_f32", "stem"), ("stem_bf16", "stem"),
                 ("res", "res"), ("tail", "tail"), ("i8", "persistent")]:
        assert want in routes, want
    assert {c.shape[1] for c in CC.PW_F32 if c.route == "pw3"} == {64, 128, 256, 512}
    assert {(c.shape[4], c.route) for c in CC.BLOCK_F32 if c.route.startswith("dwpw")} >= {(s, "dwpw%s-%d" % (v, w)) for s in (1, 2) for v in ("", "2") for w in (128, 256)}
    rows = lambda c: c.shape[0] * (c.shape[1] // c.shape[4]) ** 2 if c.kind.startswith("block") else c.shape[0]
    assert max(rows(c) for c in CC.PW_F32 + CC.PW_BF16 + CC.BLOCK_F32 + CC.BLOCK_BF16) <= 70000
    for c in CC.ALL_CASES:
        assert c.count in CC.COUNTS
        # a shipped-library run plans the same launch, or the case is a lab one
        assert c.lab or c.kind == "i8" or CC.plan(c, c.count, lab=False)["route"] == c.route, c
