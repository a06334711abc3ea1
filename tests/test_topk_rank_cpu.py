"""Rank score without a GPU: mbn_topk_metrics against a hand-derived table and against the numpy form (tests/dense_topk_ref.py) on random, empty
and void-only tables; the numpy rank table on a hand-made case; every status of mbn_topk_rank_envelope and the form switch."""
import ctypes as C

import numpy as np
import pytest

import dense_topk_ref as T


def test_metrics_by_hand(pkg):
    # classes 3, k = 2: rows = truth, columns = rank 0, rank 1, missed; the last row is void
    ranks = np.array([[6, 2, 2],       # class 0: 10 pixels, top-1 0.6, top-2 0.8
                      [0, 0, 0],       # class 1: absent
                      [1, 3, 0],       # class 2: 4 pixels, top-1 0.25, top-2 1.0
                      [0, 0, 9]], np.uint64)
    acc, mean, valid = pkg.topk_metrics(ranks, 3, 2)
    assert valid == 14.0
    assert acc[0] == 7.0 / 14.0 and acc[1] == 12.0 / 14.0
    assert mean[0] == (0.6 + 0.25) / 2 and mean[1] == (0.8 + 1.0) / 2


@pytest.mark.parametrize("classes,k", [(1, 1), (21, 5), (150, 8), (1000, 8)])
def test_metrics_against_numpy(pkg, classes, k):
    rng = np.random.default_rng(classes + k)
    tables = [rng.integers(0, 1 << 20, (classes + 1, k + 1)).astype(np.uint64),
              np.zeros((classes + 1, k + 1), np.uint64)]                                   # empty
    void_only = np.zeros((classes + 1, k + 1), np.uint64)
    void_only[classes, k] = 12345
    sparse = tables[0].copy()
    sparse[::2] = 0                                                                        # absent classes
    for ranks in tables + [void_only, sparse]:
        acc, mean, valid = pkg.topk_metrics(ranks, classes, k)
        want_acc, want_mean, want_valid = T.metrics(ranks, classes, k)
        assert valid == want_valid
        assert np.array_equal(acc, want_acc) and np.array_equal(mean, want_mean)
        assert (np.diff(acc) >= 0).all() and (acc <= 1).all()
    acc, mean, valid = pkg.topk_metrics(void_only, classes, k)
    assert valid == 0 and (acc == 0).all() and (mean == 0).all()


def test_metrics_statuses(pkg):
    lib = pkg.host_lib()
    ranks = np.zeros((4, 3), np.uint64)
    p = ranks.ctypes.data_as(C.POINTER(C.c_uint64))
    out = (C.c_double * 8)()
    assert lib.mbn_topk_metrics(p, 3, 2, out, out, None) == pkg.OK                         # valid may be NULL
    assert lib.mbn_topk_metrics(p, 3, 2, None, None, None) == pkg.OK
    assert lib.mbn_topk_metrics(None, 3, 2, out, out, None) == pkg.EINVAL
    assert lib.mbn_topk_metrics(p, 0, 2, out, out, None) == pkg.EINVAL
    assert lib.mbn_topk_metrics(p, 3, 0, out, out, None) == pkg.EINVAL
    assert lib.mbn_topk_metrics(p, 3, 9, out, out, None) == pkg.EINVAL
    assert lib.mbn_topk_metrics(p, pkg.CONFUSION_MAX_CLASSES + 1, 2, out, out, None) == pkg.EUNSUPPORTED


def test_rank_table_by_hand():
    planes = np.array([[0, 1, 2, 255, -1, 2],
                       [1, 0, 0, 1, 1, -1]], np.int32)
    truth = np.array([0, 0, 1, 1, 255, 2], np.uint8)
    got = T.rank_table(planes, truth, 3)
    want = np.zeros((4, 3), np.uint64)
    want[0, 0] = 1      # pixel 0: hit at rank 0
    want[0, 1] = 1      # pixel 1: hit at rank 1
    want[1, 2] = 1      # pixel 2: in neither plane
    want[1, 1] = 1      # pixel 3: plane 0 holds the ignore label, plane 1 hits
    want[3, 2] = 1      # pixel 4: void
    want[2, 0] = 1      # pixel 5
    assert np.array_equal(got, want) and got.sum() == truth.size
    # a void truth whose value equals a label (-1 as int32) still goes to column k
    got = T.rank_table(np.array([[-1]], np.int32), np.array([-1], np.int32), 3)
    assert got[3, 1] == 1 and got.sum() == 1


def test_envelope_and_form(pkg):
    OK, EINVAL, EUNS = pkg.OK, pkg.EINVAL, pkg.EUNSUPPORTED
    env = pkg.topk_rank_envelope
    assert env(21, 1, 1000, 5, 1000) == OK and env(21, 4, 1, 1, 1) == OK
    assert env(21, 1, 1000, 0, 1000) == EINVAL and env(21, 1, 1000, 9, 1000) == EINVAL
    assert env(21, 1, 1000, 5, 999) == EINVAL                                              # the planes overlap
    assert env(0, 1, 1000, 5, 1000) == EINVAL and env(21, 2, 1000, 5, 1000) == EINVAL and env(21, 1, 0, 5, 1000) == EINVAL
    assert env(pkg.CONFUSION_MAX_CLASSES + 1, 1, 1000, 5, 1000) == EUNS
    assert env(21, 1, (1 << 34) + 1, 1, (1 << 34) + 1) == EUNS
    assert env(21, 1, 1000, 8, 1 << 37) == OK and env(21, 1, 1000, 8, (1 << 37) + 1) == EUNS
    assert env(pkg.CONFUSION_MAX_CLASSES + 1, 1, 1000, 9, 1000) == EINVAL                  # an EINVAL goes in front
    # one switch point per k: (classes + 1) * (k + 1) * 4 bytes against 48 KB
    for k in range(1, 9):
        last = 49152 // (4 * (k + 1)) - 1
        assert pkg.topk_rank_form(last, k) == pkg.CONFUSION_FORM_LDS and pkg.topk_rank_form(last + 1, k) == pkg.CONFUSION_FORM_GLOBAL
        assert pkg.topk_rank_form(1, k) == pkg.CONFUSION_FORM_LDS
        assert pkg.topk_rank_form(4096, k) == (pkg.CONFUSION_FORM_LDS if k == 1 else pkg.CONFUSION_FORM_GLOBAL)      # k = 1: 32 776 bytes fit
    assert pkg.topk_rank_form(1364, 8) == pkg.CONFUSION_FORM_LDS and pkg.topk_rank_form(1365, 8) == pkg.CONFUSION_FORM_GLOBAL
