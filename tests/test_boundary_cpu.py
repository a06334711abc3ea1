"""Score a segmentation at its boundaries, the host side (no GPU): tests/boundary_ref.py against scipy's erosion and against two maps whose depths
are derived by hand; mbn_boundary_d, mbn_boundary_metrics, mbn_boundary_envelope and mbn_boundary_tile; the trimap table under
mbn_confusion_metrics. Every comparison of counts and depths is exact."""
import ctypes as C

import numpy as np
import pytest

import boundary_ref as BR
import confusion_ref as CR


def _blocky(rng, rows, cols, classes, block=5, void=0.03):
    m = np.kron(rng.integers(0, classes, ((rows + block - 1) // block, (cols + block - 1) // block)), np.ones((block, block), np.int64))[:rows, :cols]
    m = m.astype(np.int32)
    m[rng.random((rows, cols)) < void] = 255
    return m


@pytest.mark.parametrize("d", [1, 2, 5])
def test_reference_band_is_scipy_erosion(d):
    """the official boundary IoU: mask minus d erosions of it with a 3 x 3 element, the frame eroding too (edge = 1), per value"""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(d)
    for rows, cols in ((23, 31), (7, 40), (3, 3)):
        m = _blocky(rng, rows, cols, 4)
        band = BR.depth(m, d, 1) <= d
        for value in np.unique(m):
            mask = m == value
            eroded = ndimage.binary_erosion(mask, structure=np.ones((3, 3)), iterations=d, border_value=0)
            assert np.array_equal(mask & ~eroded, mask & band), (rows, cols, int(value))


def test_hand_derived_depths_without_the_frame():
    """edge = 0, d = 3: one pixel of another value in the corner (5, 6). A 0-pixel's depth is max (5 - r, 6 - c), capped at 4; the corner pixel
    itself has a differing neighbour at distance 1. The frame counts for nothing: the far corner stays at the cap."""
    m = np.zeros((6, 7), np.int32)
    m[5, 6] = 1
    want = np.array([[4, 4, 4, 4, 4, 4, 4],
                     [4, 4, 4, 4, 4, 4, 4],
                     [4, 4, 4, 3, 3, 3, 3],
                     [4, 4, 4, 3, 2, 2, 2],
                     [4, 4, 4, 3, 2, 1, 1],
                     [4, 4, 4, 3, 2, 1, 1]], np.uint8)
    assert np.array_equal(BR.depth(m, 3, 0), want)
    assert not (BR.depth(np.zeros((6, 7), np.int32), 3, 0) <= 3).any(), "a constant map has no band without the frame"


def test_hand_derived_depths_with_the_frame():
    """edge = 1, d = 2: classes 1 | 2 split between columns 4 and 5, a void pixel (255) at (4, 6). The depth is the least of the distance to the
    frame min (r + 1, 6 - r, c + 1, 7 - c), the distance across the split (5 - c left of it, c - 4 right of it) and, for the class-2 pixels, the
    Chebyshev distance to the void pixel; capped at 3. The void pixel is a contour for its neighbours and has depth 1 itself."""
    m = np.ones((6, 7), np.int32)
    m[:, 5:] = 2
    m[4, 6] = 255
    want = np.array([[1, 1, 1, 1, 1, 1, 1],
                     [1, 2, 2, 2, 1, 1, 1],
                     [1, 2, 3, 2, 1, 1, 1],
                     [1, 2, 3, 2, 1, 1, 1],
                     [1, 2, 2, 2, 1, 1, 1],
                     [1, 1, 1, 1, 1, 1, 1]], np.uint8)
    assert np.array_equal(BR.depth(m, 2, 1), want)
    assert np.array_equal(BR.depth(m.astype(np.uint8), 2, 1), want), "a uint8 map of the same values"


def test_half_width(pkg):
    assert pkg.boundary_d(375, 500, 0.02) == 12 and pkg.boundary_d(500, 375, 0.02) == 12, "12.5 rounds to even, not to 13"
    assert pkg.boundary_d(224, 224, 0.02) == 6
    assert pkg.boundary_d(1, 1, 0.02) == 1 and pkg.boundary_d(20, 20, 0.001) == 1, "at least 1"
    assert pkg.boundary_d(3, 4, 0.5) == 2 and pkg.boundary_d(3, 4, 0.3) == 2 and pkg.boundary_d(3, 4, 0.7) == 4, "2.5, 1.5 and 3.5: ties to even"
    assert pkg.boundary_d(64, 1, 1.0) == pkg.BOUNDARY_MAX_D and pkg.boundary_d(39, 52, 1.0) == pkg.EUNSUPPORTED, "64 and 65"
    assert pkg.boundary_d(3000, 4000, 0.02) == pkg.EUNSUPPORTED
    for rows, cols, ratio in [(0, 5, 0.02), (5, 0, 0.02), (-1, 5, 0.02), (5, 5, 0.0), (5, 5, -0.1), (5, 5, 1.5), (5, 5, float("nan")), (5, 5, float("inf"))]:
        assert pkg.boundary_d(rows, cols, ratio) == pkg.EINVAL, (rows, cols, ratio)
    assert pkg.boundary_d(0, 5, 2.0) == pkg.EINVAL
    rng = np.random.default_rng(0)
    for _ in range(200):
        rows, cols, ratio = int(rng.integers(1, 1500)), int(rng.integers(1, 1500)), float(rng.choice([0.005, 0.01, 0.02, 0.03]))
        assert pkg.boundary_d(rows, cols, ratio) == BR.half_width(rows, cols, ratio), (rows, cols, ratio)


def _compare(pkg, biou, classes):
    m, iou = pkg.boundary_metrics(biou, classes)
    want = BR.metrics(biou, classes)
    assert np.array_equal(iou, want["iou"], equal_nan=True)          # single divisions of exact integers: bit-equal
    assert (m.truth_band_pixels, m.pred_band_pixels, m.classes_present) == (want["truth_band_pixels"], want["pred_band_pixels"], want["classes_present"])
    assert abs(m.boundary_miou - want["boundary_miou"]) <= classes * 2.0 ** -52 * abs(want["boundary_miou"])     # a sequential sum of `classes` terms
    return m, iou


@pytest.mark.parametrize("classes", [1, 3, 21, 150, 1000])
def test_metrics_against_the_reference(pkg, classes):
    rng = np.random.default_rng(classes)
    both = rng.integers(0, 1 << 20, classes)
    biou = np.stack([both + rng.integers(0, 1 << 20, classes), both + rng.integers(0, 1 << 20, classes), both], axis=1).astype(np.uint64)
    _compare(pkg, biou, classes)
    absent = rng.random(classes) < 0.5
    biou[absent] = 0
    m, iou = _compare(pkg, biou, classes)
    assert np.isnan(iou[absent]).all() and m.classes_present == int((~absent & (biou[:, :2].sum(axis=1) > 0)).sum())
    m, iou = _compare(pkg, np.zeros((classes, 3), np.uint64), classes)
    assert m.boundary_miou == 0.0 and m.classes_present == 0 and np.isnan(iou).all()


def test_metrics_known_answer_and_arguments(pkg):
    m, iou = pkg.boundary_metrics(np.array([[10, 8, 6], [0, 0, 0], [4, 0, 0], [0, 5, 0]], np.uint64), 4)
    assert iou[0] == 6 / 12 and np.isnan(iou[1]) and iou[2] == 0.0 and iou[3] == 0.0
    assert (m.classes_present, m.truth_band_pixels, m.pred_band_pixels, m.boundary_miou) == (3, 14.0, 13.0, (6 / 12) / 3)
    lib = pkg.host_lib()
    n, out = (C.c_uint64 * 6)(), pkg.BoundaryMetrics()
    assert lib.mbn_boundary_metrics(None, 2, C.byref(out), None) == pkg.EINVAL and lib.mbn_boundary_metrics(n, 2, None, None) == pkg.EINVAL
    assert lib.mbn_boundary_metrics(n, 0, C.byref(out), None) == pkg.EINVAL
    assert lib.mbn_boundary_metrics(n, pkg.CONFUSION_MAX_CLASSES + 1, C.byref(out), None) == pkg.EUNSUPPORTED
    assert lib.mbn_boundary_metrics(n, 2, C.byref(out), None) == pkg.OK                   # iou may be NULL


def test_envelope_statuses(pkg):
    env = pkg.boundary_envelope
    assert env(1, 21, 1, 1, 1, 1, 0) == pkg.OK and env(4, pkg.CONFUSION_MAX_CLASSES, 65535, 16384, 32767, pkg.BOUNDARY_MAX_D, 1) == pkg.OK
    for bad in [(0, 21, 1, 5, 5, 1, 1), (2, 21, 1, 5, 5, 1, 1), (8, 21, 1, 5, 5, 1, 1), (1, 0, 1, 5, 5, 1, 1), (1, 21, 0, 5, 5, 1, 1), (1, 21, 1, 0, 5, 1, 1),
                (1, 21, 1, 5, -3, 1, 1), (1, 21, 1, 5, 5, 0, 1), (1, 21, 1, 5, 5, -1, 1), (1, 21, 1, 5, 5, 1, 2), (1, 21, 1, 5, 5, 1, -1)]:
        assert env(*bad) == pkg.EINVAL, bad
    for limit in [(1, 21, 1, 5, 5, pkg.BOUNDARY_MAX_D + 1, 1), (1, pkg.CONFUSION_MAX_CLASSES + 1, 1, 5, 5, 1, 1), (1, 21, 1, 16384, 32768, 1, 1),
                  (1, 21, 65536, 5, 5, 1, 1)]:
        assert env(*limit) == pkg.EUNSUPPORTED, limit
    assert env(1, 21, 1, 5, 5, pkg.BOUNDARY_MAX_D + 1, 2) == pkg.EINVAL, "a caller error goes before a limit"


def test_tile_lds_is_monotone_and_fits_a_cu(pkg):
    tiles = [pkg.boundary_tile(d) for d in range(1, pkg.BOUNDARY_MAX_D + 1)]
    lds = [t[2] for t in tiles]
    assert all(a < b for a, b in zip(lds, lds[1:])), "monotone in d"
    assert lds[-1] <= 160 * 1024
    assert all(tc == 64 for _, tc, _ in tiles)
    rows = [t[0] for t in tiles]
    assert rows == sorted(rows) and len(set(rows)) == 2, "two half-width classes, one switch point"
    assert rows[15] != rows[16], "d = 16 and d = 17 are in different classes"
    lib = pkg.host_lib()
    assert lib.mbn_boundary_tile(0, None, None, None) == pkg.EINVAL and lib.mbn_boundary_tile(pkg.BOUNDARY_MAX_D + 1, None, None, None) == pkg.EUNSUPPORTED
    assert lib.mbn_boundary_tile(12, None, None, None) == pkg.OK


@pytest.mark.parametrize("edge", [0, 1])
def test_trimap_under_confusion_metrics(pkg, edge):
    """the trimap table is the confusion matrix of the pixels within d of a contour of the truth: mbn_confusion_metrics needs nothing new"""
    classes, d = 5, 2
    rng = np.random.default_rng(edge)
    truth = _blocky(rng, 37, 53, classes).astype(np.uint8)
    labels = np.roll(truth.astype(np.int32), 1, axis=1)
    labels[rng.random(labels.shape) < 0.05] = -1
    trimap, biou = BR.score(labels, truth, classes, d, edge)
    band = BR.depth(truth, d, edge) <= d
    assert 0 < int(band.sum()) < band.size and int(trimap.sum()) == int(band.sum())
    assert np.array_equal(trimap, CR.confusion(labels[band], truth[band], classes))
    m, iou = pkg.confusion_metrics(trimap, classes)
    want = CR.metrics(CR.confusion(labels[band], truth[band], classes), classes)
    assert m.pixels == float(band.sum()) and m.pixel_accuracy == want["pixel_accuracy"] and np.array_equal(iou, want["iou"], equal_nan=True)
    assert int(biou[:, 0].sum()) == int((band & (truth < classes)).sum()) and (biou[:, 2] <= biou[:, 0]).all() and (biou[:, 2] <= biou[:, 1]).all()


def test_symbols_exported(pkg):
    names = pkg.declared_symbols()
    host, lib = pkg.host_lib(), pkg.load()
    for n in ("mbn_boundary_d", "mbn_boundary_envelope", "mbn_boundary_tile", "mbn_boundary_metrics"):
        assert n in names and hasattr(host, n) and hasattr(lib, n), n
    for n in ("mbn_boundary_d_items", "mbn_boundary_depth", "mbn_boundary_depth_ragged", "mbn_boundary_score_i32", "mbn_boundary_score_ragged_i32",
              "mbn_net_segment_boundary_score", "mbn_net_segment_boundary_depth"):
        assert n in names and hasattr(lib, n) and not hasattr(host, n), n
    for cls, name in ((pkg.Context, "boundary_depth"), (pkg.Context, "boundary_depth_ragged"), (pkg.Context, "boundary_score"),
                      (pkg.Context, "boundary_score_ragged"), (pkg.Context, "boundary_d_items"), (pkg.Net, "segment_boundary_score"),
                      (pkg.Net, "segment_boundary_depth")):
        assert callable(getattr(cls, name))
