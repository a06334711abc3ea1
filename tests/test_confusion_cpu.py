"""Score a segmentation, the host side (no GPU): mbn_confusion_metrics against the hand-derived known answer and against tests/confusion_ref.py on
random and edge matrices, mbn_confusion_form's single switch point and every status of mbn_confusion_envelope."""
import ctypes as C

import numpy as np
import pytest

import confusion_ref as CR

RATIOS = ("pixels", "valid", "void_pixels", "abstained", "pixel_accuracy")
MEANS = ("mean_accuracy", "miou", "fw_iou")


def _compare(pkg, counts, classes):
    m, iou = pkg.confusion_metrics(counts, classes)
    want = CR.metrics(counts, classes)
    for k in RATIOS:                                            # integers and single divisions of exact integers: bit-equal
        assert getattr(m, k) == want[k], (k, getattr(m, k), want[k])
    assert m.classes_present == want["classes_present"]
    assert np.array_equal(iou, want["iou"], equal_nan=True)
    for k in MEANS:                                             # a sequential double sum of `classes` terms in [0, 1]
        assert abs(getattr(m, k) - want[k]) <= classes * 2.0 ** -52 * abs(want[k]), (k, getattr(m, k), want[k])
    return m, iou


def test_known_answer(pkg):
    counts = np.array([[5, 1, 2], [3, 4, 0], [7, 1, 1]], np.uint64)
    m, iou = pkg.confusion_metrics(counts, 2)
    assert (m.pixels, m.valid, m.void_pixels, m.abstained) == (24.0, 15.0, 9.0, 2.0)
    assert m.classes_present == 2
    assert m.pixel_accuracy == 9 / 15
    assert list(iou) == [5 / 11, 4 / 8]
    assert m.miou == (5 / 11 + 1 / 2) / 2
    assert m.mean_accuracy == (5 / 8 + 4 / 7) / 2
    assert m.fw_iou == (8 / 15) * (5 / 11) + (7 / 15) * (1 / 2)
    _compare(pkg, counts, 2)


@pytest.mark.parametrize("classes", [1, 2, 3, 21, 150, 1000])
def test_metrics_against_the_reference(pkg, classes):
    rng = np.random.default_rng(classes)
    s = classes + 1
    dense = rng.integers(0, 1 << 20, (s, s)).astype(np.uint64)
    _compare(pkg, dense, classes)
    sparse = dense * (rng.random((s, s)) < 0.05)                 # absent classes, classes with only misses
    _compare(pkg, sparse.astype(np.uint64), classes)
    bits = 52 - int(np.ceil(np.log2(s * s)))                     # the largest cells whose total stays below 2^53, where doubles are exact
    _compare(pkg, rng.integers(0, 1 << bits, (s, s)).astype(np.uint64), classes)


def test_metrics_edge_matrices(pkg):
    m, iou = _compare(pkg, np.zeros((4, 4), np.uint64), 3)       # nothing scored
    assert (m.pixels, m.valid, m.pixel_accuracy, m.mean_accuracy, m.miou, m.fw_iou, m.classes_present) == (0, 0, 0, 0, 0, 0, 0)
    assert np.isnan(iou).all()
    only_void = np.zeros((4, 4), np.uint64)
    only_void[3] = [5, 6, 7, 8]
    m, iou = _compare(pkg, only_void, 3)                         # the void row is in no class's fp: nothing is present
    assert (m.pixels, m.valid, m.void_pixels, m.classes_present, m.miou) == (26, 0, 26, 0, 0) and np.isnan(iou).all()
    only_fp = np.zeros((4, 4), np.uint64)
    only_fp[0, 0], only_fp[0, 2] = 10, 3                         # class 2 is never true but predicted: present with iou 0, outside mean_accuracy
    m, iou = _compare(pkg, only_fp, 3)
    assert m.classes_present == 2 and iou[0] == 10 / 13 and np.isnan(iou[1]) and iou[2] == 0.0
    assert m.miou == (10 / 13 + 0.0) / 2 and m.mean_accuracy == 10 / 13 and m.pixel_accuracy == 10 / 13
    one = np.array([[7, 2], [4, 1]], np.uint64)                  # classes = 1
    m, iou = _compare(pkg, one, 1)
    assert (m.valid, m.void_pixels, m.abstained, m.classes_present) == (9, 5, 2, 1) and iou[0] == 7 / 9 and m.miou == 7 / 9 and m.fw_iou == 7 / 9
    abstain = np.zeros((3, 3), np.uint64)
    abstain[0, 2], abstain[1, 2] = 4, 6                          # everything abstained: present (fn > 0) with iou 0
    m, iou = _compare(pkg, abstain, 2)
    assert m.classes_present == 2 and list(iou) == [0.0, 0.0] and m.abstained == 10 and m.pixel_accuracy == 0


def test_metrics_arguments(pkg):
    lib = pkg.host_lib()
    n = (C.c_uint64 * 9)()
    m = pkg.SegMetrics()
    assert lib.mbn_confusion_metrics(None, 2, C.byref(m), None) == pkg.EINVAL
    assert lib.mbn_confusion_metrics(n, 2, None, None) == pkg.EINVAL
    assert lib.mbn_confusion_metrics(n, 0, C.byref(m), None) == pkg.EINVAL
    assert lib.mbn_confusion_metrics(n, 4097, C.byref(m), None) == pkg.EUNSUPPORTED
    assert lib.mbn_confusion_metrics(n, 2, C.byref(m), None) == pkg.OK        # iou may be NULL


def test_form_is_monotone_with_one_switch_point(pkg):
    forms = [pkg.confusion_form(c) for c in range(1, pkg.CONFUSION_MAX_CLASSES + 2)]
    assert set(forms) == {pkg.CONFUSION_FORM_LDS, pkg.CONFUSION_FORM_GLOBAL}
    assert sum(1 for a, b in zip(forms, forms[1:]) if a != b) == 1 and forms == sorted(forms)
    assert all(f == pkg.CONFUSION_FORM_LDS for f in forms[:21]) and pkg.confusion_form(1000) == pkg.CONFUSION_FORM_GLOBAL
    t = forms.index(pkg.CONFUSION_FORM_GLOBAL)                   # the switch point T: classes = T is the last LDS count
    assert (t + 1) ** 2 * 4 <= 160 * 1024, "the LDS table of the last LDS class count fits a CU"


def test_envelope_statuses(pkg):
    env = pkg.confusion_envelope
    assert env(21, 1, 1) == pkg.OK and env(1, 4, 1) == pkg.OK and env(4096, 4, 1 << 34) == pkg.OK
    for bad in [(0, 1, 10), (-1, 1, 10), (21, 1, 0), (21, 1, -5), (21, 0, 10), (21, 2, 10), (21, 8, 10), (21, 3, 10)]:
        assert env(*bad) == pkg.EINVAL, bad
    assert env(4097, 1, 10) == pkg.EUNSUPPORTED and env(21, 4, (1 << 34) + 1) == pkg.EUNSUPPORTED
    assert env(4097, 2, 10) == pkg.EINVAL and env(0, 1, (1 << 34) + 1) == pkg.EINVAL      # a caller error goes before a limit
