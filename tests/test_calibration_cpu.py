"""Calibration score without a GPU: the numpy form (tests/calibration_ref.py) against a per-pixel loop and hand-worked rows; its three identities
against the confusion matrix; mbn_calibration_metrics and mbn_calibration_threshold through the library against numpy, with empty bins, an empty
table and a target no edge reaches; the power-of-two threshold equivalence; every status of mbn_calibration_envelope."""
import ctypes as C
import math

import numpy as np
import pytest

import calibration_ref as R
import confusion_ref


def _loop_table(labels, prob, truth, classes, bins):
    """the header's rules, one pixel at a time in Python"""
    table = [[0] * 4 for _ in range(bins + 1)]
    for l, x, t in zip(labels.tolist(), prob, truth.tolist()):
        if not 0 <= t < classes:
            table[bins][0] += 1
            continue
        p = np.float32(0) if (math.isnan(x) or x < 0) else np.float32(1) if x > 1 else np.float32(x)
        b = min(bins - 1, int(np.float32(p * np.float32(bins))))
        if not 0 <= l < classes:
            table[b][3] += 1
            continue
        table[b][0] += 1
        table[b][1] += int(l == t)
        table[b][2] += int(np.float32(p * np.float32(1 << 24)))
    return np.array(table, np.uint64)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
@pytest.mark.parametrize("bins", [1, 10, 15, 16, 1024])
def test_reference_against_a_loop(bins, dtype):
    labels, prob, truth = R.case(500, 21, dtype, seed=bins)
    got = R.calibration_table(labels, prob, truth, 21, bins)
    assert np.array_equal(got, _loop_table(labels, prob, truth, 21, bins))
    assert got[:, 0].sum() + got[:, 3].sum() == 500 and (got[bins, 1:] == 0).all()


def test_rows_by_hand():
    classes, bins = 3, 4
    #                  void   abstained  NaN    -0.5   2.0    exactly 1
    labels = np.array([1,     255,       2,     0,     1,     2], np.int32)
    truth = np.array([255,    1,         2,     1,     1,     2], np.uint8)
    prob = np.array([np.nan,  0.6,       np.nan, -0.5, 2.0,   1.0], np.float32)
    want = np.zeros((bins + 1, 4), np.uint64)
    want[4, 0] = 1                                  # void: nothing else, whatever its prob
    want[2, 3] = 1                                  # abstained at 0.6: bin trunc(2.4) = 2; no q
    want[0, 0] += 1; want[0, 1] += 1                # NaN -> p = 0: bin 0, correct, q = 0
    want[0, 0] += 1                                 # -0.5 -> p = 0: bin 0, wrong, q = 0
    want[3, 0] += 1; want[3, 1] += 1; want[3, 2] += 1 << 24      # 2.0 -> p = 1: the last bin, q = 2^24
    want[3, 0] += 1; want[3, 1] += 1; want[3, 2] += 1 << 24      # exactly 1.0: bin bins - 1, not bins
    got = R.calibration_table(labels, prob, truth, classes, bins)
    assert np.array_equal(got, want)
    # the bytes under a void pixel and an abstained pixel's probability beyond its bin do not matter
    labels2, prob2 = labels.copy(), prob.copy()
    labels2[0], prob2[0] = -7, 0.3
    assert np.array_equal(R.calibration_table(labels2, prob2, truth, classes, bins), want)


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_identities_against_the_confusion_matrix(dtype):
    classes, bins = 21, 15
    labels, prob, truth = R.case(3 * 37 * 41, classes, dtype, seed=5)
    table = R.calibration_table(labels, prob, truth, classes, bins)
    counts = confusion_ref.confusion(labels, truth, classes)
    assert table[:bins, 1].sum() == np.trace(counts[:classes, :classes])
    assert table[:bins, 3].sum() == counts[:classes, classes].sum()
    assert table[bins, 0] == counts[classes].sum()
    assert table[:, 0].sum() + table[:, 3].sum() == labels.size


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def _tables(bins, seed):
    rng = np.random.default_rng(seed)
    full = np.zeros((bins + 1, 4), np.uint64)
    full[:bins, 0] = rng.integers(1, 1 << 20, bins)
    full[:bins, 1] = (full[:bins, 0] * rng.random(bins)).astype(np.uint64)
    full[:bins, 2] = (full[:bins, 0] * (rng.random(bins) * (1 << 24))).astype(np.uint64)
    full[:bins, 3] = rng.integers(0, 1 << 10, bins)
    full[bins, 0] = 777
    sparse = full.copy()
    sparse[:bins:2, :3] = 0                                  # empty bins: NaN in the diagram
    empty = np.zeros_like(full)                              # N = 0
    abstained_only = empty.copy()
    abstained_only[:bins, 3] = 5
    abstained_only[bins, 0] = 9
    return full, sparse, empty, abstained_only


@pytest.mark.parametrize("bins", [1, 2, 15, 16, 1024])
def test_metrics_against_numpy(pkg, bins):
    for table in _tables(bins, bins):
        m, acc, conf, cov, sel = pkg.calibration_metrics(table, bins)
        want = R.metrics(table, bins)
        for name in ("pixels", "answered", "abstained", "void_pixels", "accuracy", "mean_confidence", "ece", "mce", "aurc"):
            assert getattr(m, name) == want[name], name
        assert _same(acc, want["bin_accuracy"]) and _same(conf, want["bin_confidence"])
        assert _same(cov, want["coverage"]) and _same(sel, want["selective_accuracy"])
        assert np.isnan(acc[table[:bins, 0] == 0]).all() and not np.isnan(acc[table[:bins, 0] > 0]).any()
        assert (np.diff(cov) <= 0).all() and 0 <= m.ece <= m.mce <= 1
    m, acc, conf, cov, sel = pkg.calibration_metrics(_tables(bins, 1)[2], bins)          # N = 0
    assert m.answered == 0 and m.accuracy == 0 and m.mean_confidence == 0 and m.ece == 0 and m.mce == 0 and m.aurc == 0
    assert np.isnan(acc).all() and np.isnan(sel).all() and (cov == 0).all()


def test_metrics_by_hand(pkg):
    one = 1 << 24
    table = np.array([[10, 2, 1 * one, 5],          # accuracy 0.2, confidence 0.1
                      [0, 0, 0, 1],                 # empty
                      [30, 27, 24 * one, 0],        # accuracy 0.9, confidence 0.8
                      [4, 0, 0, 0]], np.uint64)     # 4 void
    m, acc, conf, cov, sel = pkg.calibration_metrics(table, 3)
    assert (m.pixels, m.answered, m.abstained, m.void_pixels) == (50.0, 40.0, 6.0, 4.0)
    assert m.accuracy == 29.0 / 40.0 and m.mean_confidence == 25.0 / 40.0
    assert acc[0] == 0.2 and conf[0] == 0.1 and np.isnan(acc[1]) and np.isnan(conf[1]) and acc[2] == 0.9 and conf[2] == 0.8
    assert m.ece == (10.0 / 40.0) * abs(0.2 - 0.1) + (30.0 / 40.0) * abs(0.9 - 0.8) and m.mce == max(abs(0.2 - 0.1), abs(0.9 - 0.8))
    assert list(cov) == [40.0 / 46.0, 30.0 / 46.0, 30.0 / 46.0] and list(sel) == [29.0 / 40.0, 0.9, 0.9]
    assert m.aurc == (1 - 29.0 / 40.0) * (40.0 / 46.0 - 30.0 / 46.0) + (1 - 0.9) * (30.0 / 46.0 - 30.0 / 46.0) + (1 - 0.9) * (30.0 / 46.0)
    assert pkg.calibration_threshold(table, 3, 0.7) == (0.0, 40.0 / 46.0, 29.0 / 40.0)
    assert pkg.calibration_threshold(table, 3, 0.8) == (float(np.float32(1) / np.float32(3)), 30.0 / 46.0, 0.9)
    assert pkg.calibration_threshold(table, 3, 0.95) is None                          # no edge reaches it


@pytest.mark.parametrize("bins", [1, 15, 16, 1024])
def test_threshold_against_numpy(pkg, bins):
    for table in _tables(bins, bins + 1):
        for target in (0.0, 0.3, 0.5, 0.9, 1.0):
            got, want = pkg.calibration_threshold(table, bins, target), R.threshold(table, bins, target)
            assert (got is None) == (want is None), (bins, target)
            if got is not None:
                assert got == (float(want[0]), want[1], want[2])
    assert pkg.calibration_threshold(_tables(bins, 1)[2], bins, 0.0) is None           # an empty table has no edge


def test_metrics_and_threshold_statuses(pkg):
    lib = pkg.host_lib()
    table = _tables(4, 1)[0]
    p = table.ctypes.data_as(C.POINTER(C.c_uint64))
    m, out = pkg.Calibration(), (C.c_double * 4)()
    assert lib.mbn_calibration_metrics(p, 4, C.byref(m), None, None, None, None) == pkg.OK
    assert lib.mbn_calibration_metrics(p, 4, C.byref(m), out, out, out, out) == pkg.OK
    assert lib.mbn_calibration_metrics(None, 4, C.byref(m), None, None, None, None) == pkg.EINVAL
    assert lib.mbn_calibration_metrics(p, 4, None, None, None, None, None) == pkg.EINVAL
    assert lib.mbn_calibration_metrics(p, 0, C.byref(m), None, None, None, None) == pkg.EINVAL
    assert lib.mbn_calibration_metrics(p, pkg.CALIBRATION_MAX_BINS + 1, C.byref(m), None, None, None, None) == pkg.EUNSUPPORTED
    f, d = C.c_float(-1.0), C.c_double(-1.0)
    assert lib.mbn_calibration_threshold(p, 4, 0.0, None, None, None) == pkg.OK
    assert lib.mbn_calibration_threshold(None, 4, 0.5, C.byref(f), None, None) == pkg.EINVAL
    assert lib.mbn_calibration_threshold(p, 0, 0.5, C.byref(f), None, None) == pkg.EINVAL
    assert lib.mbn_calibration_threshold(p, pkg.CALIBRATION_MAX_BINS + 1, 0.5, C.byref(f), None, None) == pkg.EUNSUPPORTED
    for bad in (-0.1, 1.1, float("nan")):
        assert lib.mbn_calibration_threshold(p, 4, bad, C.byref(f), C.byref(d), C.byref(d)) == pkg.EINVAL
    table[:4, 1] = 0                                                                  # nothing is ever right
    assert lib.mbn_calibration_threshold(p, 4, 0.5, C.byref(f), C.byref(d), C.byref(d)) == pkg.ENOTFOUND
    assert f.value == -1.0 and d.value == -1.0, "nothing is written on a refusal"


@pytest.mark.parametrize("bins", [2, 16, 256, 1024])
def test_power_of_two_edges_are_the_read_outs_threshold(bins):
    """bin >= j is exactly the complement of the read-outs' strict prob < (float) j / bins, on random values and on every edge with its neighbours"""
    rng = np.random.default_rng(bins)
    edges = (np.arange(bins + 1, dtype=np.float32) / np.float32(bins)).astype(np.float32)
    near = np.concatenate([edges, np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(2))])
    p = np.concatenate([rng.random(200000).astype(np.float32), near[(near >= 0) & (near <= 1)]]).astype(np.float32)
    b = R.bin_of(p, bins)
    js = range(bins) if bins <= 16 else list(range(0, bins, 37)) + [1, bins - 1]
    for j in js:
        min_prob = np.float32(j) / np.float32(bins)
        kept_by_the_read_out = ~(p < min_prob)
        assert np.array_equal(b >= j, kept_by_the_read_out), j
    # and in one pass for every edge: the bin of p is the number of edges j >= 1 with j / bins <= p, capped at bins - 1
    assert np.array_equal(b, np.minimum(np.searchsorted(edges[1:], p, side="right"), bins - 1))


def test_envelope(pkg):
    OK, EINVAL, EUNS = pkg.OK, pkg.EINVAL, pkg.EUNSUPPORTED
    env = pkg.calibration_envelope
    assert env(21, 1, 15, 1000) == OK and env(1, 4, 1, 1) == OK and env(4096, 1, 1024, 1 << 34) == OK
    assert env(0, 1, 15, 1000) == EINVAL and env(21, 2, 15, 1000) == EINVAL and env(21, 1, 15, 0) == EINVAL and env(21, 1, 0, 1000) == EINVAL
    assert env(pkg.CONFUSION_MAX_CLASSES + 1, 1, 15, 1000) == EUNS and env(21, 1, pkg.CALIBRATION_MAX_BINS + 1, 1000) == EUNS
    assert env(21, 1, 15, (1 << 34) + 1) == EUNS
    assert env(pkg.CONFUSION_MAX_CLASSES + 1, 1, 0, 1000) == EINVAL and env(21, 3, 2000, 1000) == EINVAL      # an EINVAL goes in front
    assert pkg.CALIBRATION_MAX_BINS == 1024 and (pkg.CALIBRATION_MAX_BINS + 1) * 32 == 32800
