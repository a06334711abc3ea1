"""Score a segmentation by surface distance, the host side (no GPU): tests/surface_ref.py against scipy's exact Euclidean distance transform and
against cases derived by hand; mbn_surface_metrics against the reference's metrics; every refusal of mbn_surface_metrics and mbn_surface_envelope.
Every comparison of counts and distances is exact."""
import ctypes as C
import math

import numpy as np
import pytest

import surface_ref as SR

H = SR.HEAD


def _blocky(rng, rows, cols, classes, block=6, void=0.03):
    m = np.kron(rng.integers(0, classes, ((rows + block - 1) // block, (cols + block - 1) // block)), np.ones((block, block), np.int64))[:rows, :cols]
    m = m.astype(np.int32)
    m[rng.random((rows, cols)) < void] = 255
    return m


@pytest.mark.parametrize("edge", [0, 1])
def test_reference_is_scipy_edt(edge):
    """d2 of a query = the squared exact Euclidean distance transform of the COMPLEMENT of the class's contour in the other map, read at the query.
    distance_transform_edt returns float64 roots of integers below 2^13: squared and rounded they are those integers again"""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(edge)
    classes = 4
    for kind, rows, cols in (("blocky", 40, 60), ("blocky", 17, 23), ("random", 12, 31), ("random", 40, 60), ("blocky", 1, 50), ("blocky", 9, 1)):
        if kind == "blocky":
            labels, truth = _blocky(rng, rows, cols, classes), _blocky(rng, rows, cols, classes)
        else:
            labels, truth = rng.integers(0, classes, (rows, cols)).astype(np.int32), rng.integers(0, classes + 1, (rows, cols)).astype(np.int32)
        got = SR.dist2_map(labels, truth, classes, edge)
        want = np.full((rows, cols), SR.NOT_QUERY, np.uint32)
        surf = np.zeros((classes, 2, H + 8), np.uint64)
        for k, (src, oth) in enumerate(((labels, truth), (truth, labels))):
            cs, co = SR.contour(src, edge), SR.contour(oth, edge)
            for c in range(classes):
                q = cs & (src == c)
                g = co & (oth == c)
                surf[c, k, 0] = int(q.sum())
                if not g.any():
                    surf[c, k, 1] = int(q.sum())
                    if k == 0:
                        want[q] = SR.UNMATCHED
                    continue
                d2 = np.rint(ndimage.distance_transform_edt(~g) ** 2).astype(np.int64)
                if k == 0:
                    want[q] = d2[q]
                if q.any():
                    surf[c, k, 2] = int(d2[q].max())
                    surf[c, k, 3] = sum(math.isqrt(int(v) << 16) for v in d2[q])
                    for v in d2[q]:
                        surf[c, k, H + min(SR.ceil_root(v), 7)] += np.uint64(1)
        assert np.array_equal(got, want), (kind, rows, cols)
        assert np.array_equal(SR.score(labels, truth, classes, 8, edge), surf), (kind, rows, cols)


def _one(rows, cols, at, value=1, fill=0):
    m = np.full((rows, cols), fill, np.int32)
    m[at] = value
    return m


def test_a_single_pixel_against_a_single_pixel():
    """class 1 is ONE pixel in each map, (2, 3) in the labels and (5, 7) in the truth, edge = 0: a lone pixel of its value is its own contour. One
    query a direction, d2 = 3^2 + 4^2 = 25, d = 5 exactly: bin 5, sum256 = 1280, max_d2 = 25. Class 0 fills the rest: its contour is the ring of
    eight pixels around the 1, so a class-0 query has a match and nothing is unmatched"""
    labels, truth = _one(9, 11, (2, 3)), _one(9, 11, (5, 7))
    s = SR.score(labels, truth, 2, 8, 0)
    for k in range(2):
        assert list(s[1, k, :4]) == [1, 0, 25, 1280] and s[1, k, H + 5] == 1 and s[1, k, H:].sum() == 1
        assert list(s[0, k, :2]) == [8, 0]
    d = SR.dist2_map(labels, truth, 2, 0)
    assert d[2, 3] == 25 and (d != SR.NOT_QUERY).sum() == 9
    # the ring around (2, 3) against the ring around (5, 7): the nearest pair is (3, 4) -> (4, 6): 1 + 4
    assert d[3, 4] == 5 and d[1, 2] == (4 - 1) ** 2 + (6 - 2) ** 2


def test_squares_land_in_their_bin_and_one_more_in_the_next():
    """a query at (0, 0) and its only match at (0, t): d2 = t^2 -> bin t. The match at (1, t): d2 = t^2 + 1 -> ceil (sqrt) = t + 1. The class is 1,
    one pixel a map, in a sea of void (255): void forms no class, so these are the only queries. The last bin takes everything from bins - 1 on"""
    for t in (1, 2, 3, 7, 30):
        labels = _one(3, 40, (0, 0), fill=255)
        s = SR.score(labels, _one(3, 40, (0, t), fill=255), 2, 64, 0)
        assert s[1, 0, H + t] == 1 and s[1, 0, H:].sum() == 1 and s[1, 0, 2] == t * t and s[1, 0, 3] == 256 * t and s[0].sum() == 0
        s = SR.score(labels, _one(3, 40, (1, t), fill=255), 2, 64, 0)
        assert s[1, 0, H + t + 1] == 1 and s[1, 0, H:].sum() == 1 and s[1, 0, 2] == t * t + 1
        assert s[1, 0, 3] == math.isqrt((t * t + 1) << 16) and 256 * t < s[1, 0, 3] < 256 * (t + 1)
    # bins = 8: d = 7 exactly is the first distance of the overflow bin (>= bins - 1), d2 = 37 (ceil 7) and d = 30 land there too; d2 = 36 does not
    labels = _one(3, 40, (0, 0), fill=255)
    for at, where in (((0, 7), 7), ((1, 6), 7), ((0, 30), 7), ((0, 6), 6)):
        s = SR.score(labels, _one(3, 40, at, fill=255), 2, 8, 0)
        assert s[1, 0, H + where] == 1 and s[1, 0, H:].sum() == 1, at
    s = SR.score(labels, _one(3, 40, (0, 30), fill=255), 2, 2, 0)
    assert s[1, 0, H + 1] == 1 and s[1, 0, 2] == 900, "two bins: d = 0 and the rest"
    s = SR.score(labels, labels, 2, 2, 0)
    assert s[1, 0, H] == 1 and s[1, 1, H] == 1 and s[1, 0, 2] == 0 and s[1, 0, 3] == 0, "a query ON the other contour: d2 = 0"


def test_a_class_on_one_side_only_is_unmatched():
    """the labels hold a 2 x 2 block of class 2 the truth does not have: four queries of direction 0, all unmatched, none of direction 1. They
    reach no bin, no max and no sum; in dist2 they are 0xFFFFFFFE"""
    labels, truth = np.zeros((6, 6), np.int32), np.zeros((6, 6), np.int32)
    labels[2:4, 2:4] = 2
    s = SR.score(labels, truth, 3, 4, 0)
    assert list(s[2, 0]) == [4, 4, 0, 0, 0, 0, 0, 0] and s[2, 1].sum() == 0
    # class 0 of the labels: the 12 pixels around the block. The truth is constant and edge = 0: no contour of 0 there: unmatched as well
    assert list(s[0, 0, :2]) == [12, 12] and s[0, 1].sum() == 0
    d = SR.dist2_map(labels, truth, 3, 0)
    assert (d[2:4, 2:4] == SR.UNMATCHED).all() and (d == SR.UNMATCHED).sum() == 16 and (d == SR.NOT_QUERY).sum() == 20
    m = SR.metrics(s, 3, 4, 1, 95.0)
    assert m["classes_present"] == 2 and m["classes_measurable"] == 0 and m["unmatched"] == 16 and m["n"] == 16
    assert m["nsd_c"][2] == 0.0 and np.isnan(m["nsd_c"][1]) and np.isnan(m["hd_c"]).all()


def test_edge_on_a_constant_map():
    """a constant 4 x 5 map: without the frame no pixel is contour; with it the 14 frame pixels are, in both maps, each ON the other side's
    contour: d2 = 0 everywhere"""
    m = np.full((4, 5), 1, np.int32)
    assert SR.score(m, m, 2, 4, 0).sum() == 0 and (SR.dist2_map(m, m, 2, 0) == SR.NOT_QUERY).all()
    s = SR.score(m, m, 2, 4, 1)
    assert list(s[1, 0]) == [14, 0, 0, 0, 14, 0, 0, 0] and list(s[1, 1]) == list(s[1, 0])
    d = SR.dist2_map(m, m, 2, 1)
    assert (d[1:3, 1:4] == SR.NOT_QUERY).all() and (d == 0).sum() == 14
    one = np.full((1, 1), 1, np.int32)
    assert SR.score(one, one, 2, 4, 0).sum() == 0 and SR.score(one, one, 2, 4, 1)[1, 0, 0] == 1


def test_void_and_abstained_neighbours():
    """classes = 2. The truth is all 1 but for a void pixel (255) at (2, 2); the labels all 1 but for an abstained pixel (-1) at (2, 5); edge = 0.
    Each makes its eight neighbours contour pixels of class 1 and forms no class itself. A labels query at (r, c) around (2, 5) finds the nearest of
    the ring around (2, 2): the query (2, 4) has (2, 3) beside it (d2 = 1), the query (2, 6) has (1, 3), (2, 3), (3, 3) at dc = 3: d2 = 9"""
    truth, labels = np.ones((5, 8), np.int32), np.ones((5, 8), np.int32)
    truth[2, 2] = 255
    labels[2, 5] = -1
    s = SR.score(labels, truth, 2, 8, 0)
    assert list(s[1, 0, :2]) == [8, 0] and list(s[1, 1, :2]) == [8, 0] and s[0].sum() == 0
    d = SR.dist2_map(labels, truth, 2, 0)
    assert d[2, 5] == SR.NOT_QUERY and d[2, 4] == 1 and d[2, 6] == 9 and d[1, 4] == 1 and d[1, 6] == 9
    assert s[1, 0, 2] == 9 and s[1, 1, 2] == 9
    # a value of 2 = classes is out of range like 255: the same table
    truth[2, 2] = 2
    assert np.array_equal(SR.score(labels, truth, 2, 8, 0), s)


# ------------------------------------------------------------------------------------------------------------------ the host library

def _lib_metrics(pkg, surf, classes, bins, tolerance, percentile):
    return pkg.surface_metrics(surf, classes, bins, tolerance, percentile)


def _close(got, want, classes):
    return got == want or abs(got - want) <= classes * 2.0 ** -52 * abs(want)


@pytest.mark.parametrize("classes,bins,tolerance,percentile", [(1, 2, 0, 95.0), (3, 8, 2, 95.0), (5, 16, 3, 50.0), (21, 64, 2, 100.0),
                                                               (21, 4, 1, 99.5), (1000, 16, 2, 95.0)])
def test_metrics_against_the_reference(pkg, classes, bins, tolerance, percentile):
    rng = np.random.default_rng(classes + bins)
    top = min(classes, 12)
    pairs = []
    for _ in range(3):
        truth = _blocky(rng, 30, 44, top)
        labels = np.roll(truth, (1, 2), axis=(0, 1))
        labels[rng.random(labels.shape) < 0.05] = rng.integers(0, top)
        pairs.append((labels, truth))
    only = np.zeros((8, 8), np.int32)                            # a class on one side only: present, not measurable
    if classes > 1:
        only[3:5, 3:5] = classes - 1
    pairs.append((only, np.zeros((8, 8), np.int32)))
    surf = SR.score_maps(pairs, classes, bins, 1)
    want = SR.metrics(surf, classes, bins, tolerance, percentile)
    m, hd, hdp, assd, nsd = _lib_metrics(pkg, surf, classes, bins, tolerance, percentile)
    for key in ("classes_present", "classes_measurable", "saturated"):
        assert getattr(m, key) == want[key], key
    assert m.n == want["n"] and m.unmatched == want["unmatched"] and m.reserved == 0
    # beyond the 12 values of the blocky pairs the last class lies in the labels of the fourth pair only
    assert want["classes_measurable"] > 0 and (classes <= 12 or want["classes_present"] > want["classes_measurable"])
    for key in ("hd", "hdp", "assd", "nsd"):
        assert _close(getattr(m, key), want[key], classes), (key, getattr(m, key), want[key])
    for got, key in ((hd, "hd_c"), (hdp, "hdp_c"), (assd, "assd_c"), (nsd, "nsd_c")):
        assert np.array_equal(np.isnan(got), np.isnan(want[key])), key
        ok = ~np.isnan(got)
        assert all(_close(g, w, classes) for g, w in zip(got[ok], want[key][ok])), key
    if bins == 4:
        assert want["saturated"] > 0, "four bins: the percentile of some class lies in the overflow bin"


def test_metrics_by_hand(pkg):
    """one class, bins = 4. Direction 0: 10 queries, 2 unmatched, 8 matched in bins [4, 2, 1, 1], max_d2 = 10, sum256 = 2000. Direction 1: 4
    queries, all matched in bin 1, max_d2 = 1, sum256 = 1024. hd = sqrt (10). 95 %: ceil (7.6) = 8 of 8 -> the overflow bin (3), saturated; 50 %:
    need 4 -> bin 0, direction 1 need 2 -> bin 1: hdp = 1. assd = 3024 / 256 / 12. nsd at tolerance 1: (6 + 4) / 14"""
    surf = np.array([[[10, 2, 10, 2000, 4, 2, 1, 1], [4, 0, 1, 1024, 0, 4, 0, 0]]], np.uint64)
    m, hd, hdp, assd, nsd = pkg.surface_metrics(surf, 1, 4, 1, 95.0)
    assert hd[0] == math.sqrt(10.0) and hdp[0] == 3.0 and m.saturated == 1 and assd[0] == 3024 / 256.0 / 12.0 and nsd[0] == 10.0 / 14.0
    assert (m.classes_present, m.classes_measurable, m.n, m.unmatched) == (1, 1, 14.0, 2.0) and m.hd == hd[0] and m.nsd == nsd[0]
    m, hd, hdp, assd, nsd = pkg.surface_metrics(surf, 1, 4, 0, 50.0)
    assert hdp[0] == 1.0 and m.saturated == 0 and nsd[0] == 4.0 / 14.0
    want = SR.metrics(surf, 1, 4, 0, 50.0)
    assert want["hdp"] == 1.0 and want["nsd"] == 4.0 / 14.0 and want["assd"] == assd[0]
    # per-class arrays may be NULL; an empty table has no class
    lib = pkg.host_lib()
    mm = pkg.SurfaceMetrics()
    zero = np.zeros(2 * 8, np.uint64)
    assert lib.mbn_surface_metrics(zero.ctypes.data_as(C.POINTER(C.c_uint64)), 1, 4, 1, 95.0, C.byref(mm), None, None, None, None) == pkg.OK
    assert (mm.classes_present, mm.classes_measurable, mm.hd, mm.hdp, mm.assd, mm.nsd, mm.n) == (0, 0, 0.0, 0.0, 0.0, 0.0, 0.0)


def test_metrics_refusals(pkg):
    lib = pkg.host_lib()
    surf = np.zeros(2 * 2 * (H + 4), np.uint64)
    p = surf.ctypes.data_as(C.POINTER(C.c_uint64))
    m = pkg.SurfaceMetrics()

    def call(s=p, classes=2, bins=4, tol=1, pct=95.0, mm=C.byref(m)):
        return lib.mbn_surface_metrics(s, classes, bins, tol, pct, mm, None, None, None, None)

    assert call() == pkg.OK
    EI, EU = pkg.EINVAL, pkg.EUNSUPPORTED
    assert call(s=None) == EI and call(mm=None) == EI and call(classes=0) == EI and call(classes=-3) == EI and call(bins=1) == EI and call(bins=0) == EI
    assert call(tol=-1) == EI and call(tol=3) == EI and call(tol=2) == pkg.OK, "tolerance in [0, bins - 2]"
    assert call(pct=0.0) == EI and call(pct=-5.0) == EI and call(pct=100.5) == EI and call(pct=float("nan")) == EI and call(pct=100.0) == pkg.OK
    assert call(classes=pkg.CONFUSION_MAX_CLASSES + 1) == EU and call(bins=pkg.SURFACE_MAX_BINS + 1, tol=0) == EU
    assert call(classes=pkg.CONFUSION_MAX_CLASSES + 1, tol=-1) == EI, "a caller error goes before a limit"


def test_envelope_refusals(pkg):
    env = pkg.surface_envelope
    EI, EU = pkg.EINVAL, pkg.EUNSUPPORTED
    assert env(1, 21, 64, 1, 1, 1, 0) == pkg.OK and env(4, pkg.CONFUSION_MAX_CLASSES, pkg.SURFACE_MAX_BINS, 65535, 16384, 32767, 1) == pkg.OK
    for args in ((2, 21, 64, 1, 5, 5, 1), (0, 21, 64, 1, 5, 5, 1), (8, 21, 64, 1, 5, 5, 1), (1, 0, 64, 1, 5, 5, 1), (1, -1, 64, 1, 5, 5, 1),
                 (1, 21, 1, 1, 5, 5, 1), (1, 21, 0, 1, 5, 5, 1), (1, 21, 64, 0, 5, 5, 1), (1, 21, 64, 1, 0, 5, 1), (1, 21, 64, 1, 5, -2, 1),
                 (1, 21, 64, 1, 5, 5, 2), (1, 21, 64, 1, 5, 5, -1)):
        assert env(*args) == EI, args
    for args in ((1, pkg.CONFUSION_MAX_CLASSES + 1, 64, 1, 5, 5, 1), (1, 21, pkg.SURFACE_MAX_BINS + 1, 1, 5, 5, 1), (1, 21, 64, 1, 32768, 5, 1),
                 (1, 21, 64, 1, 5, 32768, 1), (1, 21, 64, 1, 16384, 32767 + 1, 1), (1, 21, 64, 1, 32767, 32767, 1), (1, 21, 64, 1, 16385, 32767, 1),
                 (1, 21, 64, 65536, 5, 5, 1)):
        assert env(*args) == EU, args
    assert env(1, 21, 64, 1, 32767, 16384, 1) == pkg.OK, "32767 x 16384 is just below 2^29"
    assert env(1, 21, 64, 65536, 5, 5, 3) == EI, "a caller error goes before a limit"
    assert pkg.surface_tile() == (256, 64)
    sb = pkg.surface_scratch_bytes
    assert sb(1, 1, 1) == 256 and sb(2, 1000, 21) == (8000 + 8 * 42 + 255) // 256 * 256 and sb(32, 6000000, 1000) % 256 == 0
    assert sb(0, 10, 1) == 0 and sb(1, 0, 1) == 0 and sb(1, 10, 0) == 0 and sb(65536, 10, 1) == 0 and sb(1, (1 << 34) + 1, 1) == 0
    assert sb(1, 10, pkg.CONFUSION_MAX_CLASSES + 1) == 0 and sb(65535, 1 << 34, pkg.CONFUSION_MAX_CLASSES) >= 8 << 34
