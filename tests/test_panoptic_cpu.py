"""Score a segmentation by its regions, the host side (no GPU): the pair-histogram reference of tests/panoptic_ref.py against a brute-force double
loop and against the device's bit-majority route in numpy, hand-derived cases with their derivations, and the pure host functions of
libmbn_host.so (mbn_panoptic_metrics, _envelope, _scratch_bytes).

The first three tests are a self-check of the reference alone: they run no code of the library and would pass without it. panoptic_vote is a numpy
re-statement of the device's route, not the device code: it shows that the route finds every match, the GPU tests show that the kernels follow
it. The tests of the host functions below them are the ones that need the library."""
import ctypes as C
import math

import numpy as np
import pytest

import panoptic_ref as P

I32_MAX = np.iinfo(np.int32).max


def _scene(rows, cols, seed):
    rng = np.random.default_rng(seed)
    # a few segments of a few classes, some pixels of no segment on either side; ids in any order, so the numbering is exercised too
    truth = P.segments(rng.integers(-1, 4, (rows, cols)), rng.integers(0, 3, 4))
    pred = P.segments(rng.integers(-1, 5, (rows, cols)), rng.integers(0, 3, 5))
    return pred, truth


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 7), (5, 1), (3, 4), (6, 7)])
def test_reference_against_brute_force(rows, cols):
    for seed in range(40):
        pred, truth = _scene(rows, cols, 1000 * rows + 10 * cols + seed)
        a = P.panoptic(pred[0], pred[1], truth[0], truth[1], 3)
        assert P.same(a, P.panoptic_brute(pred[0], pred[1], truth[0], truth[1], 3)), seed
        assert P.same(a, P.panoptic_vote(pred[0], pred[1], truth[0], truth[1], 3)), seed
        # classes = 2: the segments of class 2 are matched and written like any other and add nothing to pq
        b = P.panoptic(pred[0], pred[1], truth[0], truth[1], 2)
        assert np.array_equal(b.pq, a.pq[:2]) and all(np.array_equal(x, y) for x, y in zip(a[1:5], b[1:5]))


def test_the_vote_route_finds_every_match():
    """the device's route against the pair histogram on block scenes with noise, shifts, void truth and abstained predictions; all four outcomes occur"""
    seen = np.zeros(4, np.int64)
    for seed in range(24):
        rows, cols = 37 + seed, 51 + 2 * seed
        t = P.block_scene(rows, cols, 5, seed, side=6, drop=0.1 if seed % 3 == 0 else 0.0, drop_blocks=0.2, class_seed=seed)
        p = P.block_scene(rows, cols, 5, seed + 100, side=6, shift=seed % 4, noise=(0.0, 0.05, 0.3)[seed % 3], drop=0.05 * (seed % 2), class_seed=seed)
        a = P.panoptic(p[0], p[1], t[0], t[1], 5)
        assert P.same(a, P.panoptic_vote(p[0], p[1], t[0], t[1], 5)), seed
        seen += [int(a.pq[:, 0].sum()), int(a.pq[:, 1].sum()), int(a.pq[:, 2].sum()), int((a.match_pred == -2).sum())]
    assert (seen > 100).all(), seen


def hand_cases():
    """(name, comp_pred, pred records, comp_truth, truth records, classes, expected pq rows as (tp, fp, fn, S numerator / denominator pairs),
    match_pred, match_truth, inter, void). Every map is one row; a segment's record is (label, area). S of a class = sum of floor (i * 2^32 / u)."""
    def rec(*pairs):
        return P.records([p[0] for p in pairs], [p[1] for p in pairs])

    def S(*fracs):
        return sum((i << 32) // u for i, u in fracs)

    m = lambda *v: np.array(v, np.int32)
    cases = []
    # perfect: both sides are segment 0 (class 0, 3 pixels) and segment 1 (class 1, 2 pixels). inter = area on both sides, union = area: IoU 1.
    cases.append(("perfect", m(0, 0, 0, 1, 1), rec((0, 3), (1, 2)), m(0, 0, 0, 1, 1), rec((0, 3), (1, 2)), 2,
                  [(1, 0, 0, S((3, 3))), (1, 0, 0, S((2, 2)))], m(0, 1), m(0, 1), m(3, 2), m(0, 0)))
    # IoU exactly 1/2: truth g = 4 pixels, p covers 2 of them. inter 2, union = 2 - 0 + 4 - 2 = 4, 2 * 2 = 4 is not > 4: p is a false positive, g a
    # false negative
    cases.append(("iou one half", m(0, 0, -1, -1), rec((0, 2)), m(0, 0, 0, 0), rec((0, 4)), 1,
                  [(0, 1, 1, 0)], m(-1), m(-1), m(0), m(0)))
    # one pixel more: inter 3, union = 3 + 4 - 3 = 4, 6 > 4: a match at IoU 3/4
    cases.append(("iou three quarters", m(0, 0, 0, -1), rec((0, 3)), m(0, 0, 0, 0), rec((0, 4)), 1,
                  [(1, 0, 0, S((3, 4)))], m(0), m(0), m(3), m(0)))
    # void tie: p (class 0) has 4 pixels, 2 over void truth and 2 over g (class 1, so no match). 2 * void = 4 is not > 4: a false positive of
    # class 0; g is a false negative of class 1
    cases.append(("void tie", m(0, 0, 0, 0), rec((0, 4)), m(-1, -1, 0, 0), rec((1, 2)), 2,
                  [(0, 1, 0, 0), (0, 0, 1, 0)], m(-1), m(-1), m(0), m(2)))
    # one void pixel more: p has 5 pixels, 3 over void. 2 * 3 = 6 > 5: excused, it counts nowhere; g is still a false negative
    cases.append(("void majority", m(0, 0, 0, 0, 0), rec((0, 5)), m(-1, -1, -1, 0, 0), rec((1, 2)), 2,
                  [(0, 0, 0, 0), (0, 0, 1, 0)], m(-2), m(-1), m(0), m(3)))
    # the majority truth segment has another class: p (class 0) lies exactly on g (class 1): a false positive of 0 and a false negative of 1
    cases.append(("another class", m(0, 0, 0), rec((0, 3)), m(0, 0, 0), rec((1, 3)), 2,
                  [(0, 1, 0, 0), (0, 0, 1, 0)], m(-1), m(-1), m(0), m(0)))
    # one truth segment of 10 pixels split 7 | 3: p0 has inter 7, union 7 + 10 - 7 = 10, 14 > 10: a match; p1 has inter 3, union 10: a false positive
    cases.append(("split 7 3", m(0, 0, 0, 0, 0, 0, 0, 1, 1, 1), rec((0, 7), (0, 3)), m(*[0] * 10), rec((0, 10)), 1,
                  [(1, 1, 0, S((7, 10)))], m(0, -1), m(0), m(7, 0), m(0, 0)))
    # split 5 | 5: both have inter 5, union 10, 10 is not > 10: two false positives and a false negative
    cases.append(("split 5 5", m(0, 0, 0, 0, 0, 1, 1, 1, 1, 1), rec((0, 5), (0, 5)), m(*[0] * 10), rec((0, 10)), 1,
                  [(0, 2, 1, 0)], m(-1, -1), m(-1), m(0, 0), m(0, 0)))
    # two truth segments (6 and 4 pixels) fused into one p of 10: with g0 inter 6, union 10 + 6 - 6 = 10, 12 > 10: a match; g1 is a false negative
    cases.append(("fused 6 4", m(*[0] * 10), rec((0, 10)), m(0, 0, 0, 0, 0, 0, 1, 1, 1, 1), rec((0, 6), (0, 4)), 1,
                  [(1, 0, 1, S((6, 10)))], m(0), m(0, -1), m(6), m(0)))
    # fused 5 | 5: no majority: a false positive and two false negatives
    cases.append(("fused 5 5", m(*[0] * 10), rec((0, 10)), m(0, 0, 0, 0, 0, 1, 1, 1, 1, 1), rec((0, 5), (0, 5)), 1,
                  [(0, 1, 2, 0)], m(-1), m(-1, -1), m(0), m(0)))
    return cases


def test_hand_derived_cases():
    for name, cp, pred, ct, truth, classes, pq, mp, mt, inter, void in hand_cases():
        for form in (P.panoptic, P.panoptic_brute, P.panoptic_vote):
            got = form(cp, pred, ct, truth, classes)
            assert got.pq.tolist() == [list(r) for r in pq], name
            assert np.array_equal(got.match_pred, mp) and np.array_equal(got.match_truth, mt), name
            assert np.array_equal(got.inter, inter) and np.array_equal(got.void, void), name


# -------------------------------------------------------------------------------------------------------------------- the host functions

def _metrics_equal(pkg, pq, classes):
    m, pq_c, sq_c, rq_c = pkg.panoptic_metrics(pq, classes)
    want, wp, ws, wr = P.metrics(pq)
    got = (m.pq, m.sq, m.rq, m.tp, m.fp, m.fn, m.classes_present)
    assert got == want, (got, want)                             # bit for bit: == on floats
    for a, b in ((pq_c, wp), (sq_c, ws), (rq_c, wr)):
        assert a.tobytes() == b.tobytes() or (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))
    return m, pq_c, sq_c, rq_c


def test_metrics(pkg):
    rng = np.random.default_rng(3)
    # a table by hand: class 0 two matches of IoU 3/4 and 1/2 + 2^-32, a false positive; class 1 absent; class 2 only a false negative
    pq = np.array([[2, 1, 0, (3 << 30) + (1 << 31) + 1], [0, 0, 0, 0], [0, 0, 1, 0]], np.uint64)
    m, pq_c, sq_c, rq_c = _metrics_equal(pkg, pq, 3)
    iou = math.ldexp(float((3 << 30) + (1 << 31) + 1), -32)
    assert pq_c[0] == 2.0 * iou / 5.0 and rq_c[0] == 4.0 / 5.0 and sq_c[0] == iou / 2.0
    assert math.isnan(pq_c[1]) and math.isnan(sq_c[1]) and math.isnan(rq_c[1]), "an absent class"
    assert pq_c[2] == 0.0 and rq_c[2] == 0.0 and sq_c[2] == 0.0, "a present class without a match"
    assert m.classes_present == 2 and (m.tp, m.fp, m.fn) == (2.0, 1.0, 1.0)
    assert m.pq == (pq_c[0] + pq_c[2]) / 2.0 and m.sq == (sq_c[0] + sq_c[2]) / 2.0 and m.rq == (rq_c[0] + rq_c[2]) / 2.0
    # none present
    m, pq_c, _, _ = _metrics_equal(pkg, np.zeros((4, 4), np.uint64), 4)
    assert (m.pq, m.sq, m.rq, m.tp, m.fp, m.fn, m.classes_present) == (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0) and np.isnan(pq_c).all()
    # random tables, large counts and sums included
    for classes in (1, 2, 21, 150):
        for _ in range(10):
            pq = rng.integers(0, 1 << 20, (classes, 4)).astype(np.uint64)
            pq[:, 3] = (pq[:, 0] * rng.integers(1 << 31, 1 << 32, classes).astype(np.uint64))
            pq[rng.random(classes) < 0.3] = 0
            _metrics_equal(pkg, pq, classes)
    # NULL per-class outputs, and the refusals
    lib = pkg.host_lib()
    pq = np.ones((2, 4), np.uint64)
    m = pkg.PanopticMetrics()
    p = pq.ctypes.data_as(C.POINTER(C.c_uint64))
    assert lib.mbn_panoptic_metrics(p, 2, C.byref(m), None, None, None) == pkg.OK and m.classes_present == 2
    assert lib.mbn_panoptic_metrics(None, 2, C.byref(m), None, None, None) == pkg.EINVAL
    assert lib.mbn_panoptic_metrics(p, 2, None, None, None, None) == pkg.EINVAL
    assert lib.mbn_panoptic_metrics(p, 0, C.byref(m), None, None, None) == pkg.EINVAL
    assert lib.mbn_panoptic_metrics(p, -1, C.byref(m), None, None, None) == pkg.EINVAL
    assert lib.mbn_panoptic_metrics(p, 4097, C.byref(m), None, None, None) == pkg.EUNSUPPORTED
    with pytest.raises(ValueError):
        pkg.panoptic_metrics(pq, 3)


def test_envelope_and_scratch(pkg):
    env = pkg.panoptic_envelope
    assert env(1, 1, 1, 1, 1, 1) == pkg.OK and env(65535, 375, 500, 4096, 1 << 24, 1 << 24) == pkg.OK
    for bad in ((0, 4, 4, 2, 1, 1), (1, 0, 4, 2, 1, 1), (1, 4, -1, 2, 1, 1), (1, 4, 4, 0, 1, 1), (1, 4, 4, 2, 0, 1), (1, 4, 4, 2, 1, 0),
                (-1, 4, 4, 2, 1, 1), (1, 4, 4, 2, -5, 1)):
        assert env(*bad) == pkg.EINVAL, bad
    # both sides of every limit
    assert env(1, 1, (1 << 29) - 1, 2, 1, 1) == pkg.OK and env(1, 1, 1 << 29, 2, 1, 1) == pkg.EUNSUPPORTED
    assert env(1, 1 << 14, 1 << 15, 2, 1, 1) == pkg.EUNSUPPORTED and env(1, I32_MAX, I32_MAX, 2, 1, 1) == pkg.EUNSUPPORTED
    assert env(65535, 4, 4, 2, 1, 1) == pkg.OK and env(65536, 4, 4, 2, 1, 1) == pkg.EUNSUPPORTED
    assert env(1, 4, 4, 4096, 1, 1) == pkg.OK and env(1, 4, 4, 4097, 1, 1) == pkg.EUNSUPPORTED
    assert env(1, 4, 4, 2, pkg.COMPONENTS_MAX_REGIONS, 1) == pkg.OK and env(1, 4, 4, 2, pkg.COMPONENTS_MAX_REGIONS + 1, 1) == pkg.EUNSUPPORTED
    assert env(1, 4, 4, 2, 1, pkg.COMPONENTS_MAX_REGIONS) == pkg.OK and env(1, 4, 4, 2, 1, pkg.COMPONENTS_MAX_REGIONS + 1) == pkg.EUNSUPPORTED
    assert env(65536, 4, 4, 2, 0, 1) == pkg.EINVAL, "a caller error goes before a limit"
    sb = pkg.panoptic_scratch_bytes
    assert sb(1, 1) == 256 and sb(1, 2) == 256 and sb(1, 3) == 512, "116 bytes per slot, rounded up to 256"
    assert sb(32, 32 * 4096) == 116 * 32 * 4096 and sb(32, 32 * 4096) % 256 == 0
    assert sb(65535, 1 << 32) == 116 << 32 and sb(65535, (1 << 32) + 1) == 0 and sb(65536, 10) == 0
    assert sb(0, 10) == 0 and sb(1, 0) == 0 and sb(-1, -1) == 0 and sb(I32_MAX, 1 << 62) == 0
    assert sb(1, 1000) == sb(65535, 1000), "a function of the slots only"


def test_the_library_exports_the_calls(pkg):
    host = pkg.host_lib()
    for n in ("mbn_panoptic_envelope", "mbn_panoptic_scratch_bytes", "mbn_panoptic_metrics"):
        assert hasattr(host, n), n
    for n in ("mbn_panoptic_create", "mbn_panoptic_destroy", "mbn_panoptic_i32", "mbn_panoptic_ragged_i32", "mbn_net_segment_panoptic",
              "mbn_net_set_panoptic_regions", "mbn_widen_u8_i32", "mbn_ragged_readout_span"):
        assert n in pkg.declared_symbols(), n
    for cls, name in ((pkg.Context, "panoptic"), (pkg.Context, "panoptic_ragged"), (pkg.Net, "segment_panoptic"), (pkg.Panoptic, "close")):
        assert callable(getattr(cls, name))
