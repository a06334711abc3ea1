"""Segment with confidence, without a GPU: tests/dense_prob_ref.py (the normative arithmetic of mbn_resample_softmax_f32 and its window form)
against dense_any_ref / dense_window_ref (labels and scores bit for bit), against torch's float64 softmax of its own bilinear interpolate, on
the special values, and on the inputs and thresholds of the GPU threshold test (no pixel close enough to a threshold to go either way); the
host-side argument check of min_prob; the symbols where they belong."""
import numpy as np
import pytest

import dense_any_ref
import dense_prob_ref as P
import dense_window_ref
from test_dense_cpu import logits_for


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", [(2, 5, 7, 21, 37, 61), (1, 3, 5, 130, 100, 23), (3, 1, 1, 5, 9, 4), (1, 7, 7, 65, 30, 28)])
def test_ref_labels_and_scores_are_the_argmax_reference(shape):
    n, h, w, classes, H, W = shape
    x = logits_for((n, h, w, classes, 0), seed=sum(shape))
    lab, sc, prob = P.resample_softmax(x, H, W)
    want_lab, want_sc = dense_any_ref.resample_argmax(x, H, W)
    assert lab.dtype == np.int32 and sc.dtype == np.float32 and prob.dtype == np.float64 and prob.shape == (n, H, W)
    assert np.array_equal(lab, want_lab) and np.array_equal(_bits(sc), _bits(want_sc))
    assert (prob > 0).all() and (prob <= 1).all()


@pytest.mark.parametrize("rect,H,W", [((0, 0, 224, 160), 37, 61), ((64, 32, 96, 96), 39, 41), ((9, 11, 180, 120), 67, 50)])
def test_ref_window_labels_and_scores_are_the_argmax_reference(rect, H, W):
    x = logits_for((2, 5, 7, 21, 0), seed=H)
    lab, sc, prob = P.resample_softmax_window(x, 160, 224, rect, H, W)
    want_lab, want_sc = dense_window_ref.resample_argmax_window(x, 160, 224, rect, H, W)
    assert np.array_equal(lab, want_lab) and np.array_equal(_bits(sc), _bits(want_sc))
    if rect == (0, 0, 224, 160):                       # the full window is the plain rule, the probabilities included
        assert np.array_equal(prob, P.resample_softmax(x, H, W)[2])


def test_ref_prob_vs_torch_float64():
    """torch forms its interpolation weights in another way, so its interpolants differ from the reference's fp32 v in the last bits: 1e-5"""
    import torch
    n, h, w, classes, H, W = 2, 5, 7, 21, 37, 61
    x = logits_for((n, h, w, classes, 0), seed=5)
    lab, _, prob = P.resample_softmax(x, H, W)
    t = torch.from_numpy(x).permute(0, 3, 1, 2).double()
    sm = torch.softmax(torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=False), dim=1).numpy()
    at_label = np.take_along_axis(sm, lab[:, None].astype(np.int64), axis=1)[:, 0]
    assert np.abs(at_label - prob).max() <= 1e-5
    # and where torch's own winner is the reference's, which is everywhere but at near-ties, its maximum is that value
    same = sm.argmax(axis=1) == lab
    assert same.mean() > 0.99 and np.abs(sm.max(axis=1) - prob)[same].max() <= 1e-5


def test_ref_special_values():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    lab, sc, prob = P.from_interpolants(np.full((3, 4, 21), nan, np.float32))                # all NaN: nothing wins
    assert (lab == 0).all() and (sc == -inf).all() and (prob == 0).all()
    lab, sc, prob = P.from_interpolants(np.full((2, 5), -inf, np.float32))                   # all -inf: nothing wins either
    assert (lab == 0).all() and (sc == -inf).all() and (prob == 0).all()
    v = np.array([0.0, 1.0, inf, 2.0], np.float32)                                           # a +inf winner: label 2, prob 0
    lab, sc, prob = P.from_interpolants(v)
    assert lab == 2 and sc == inf and prob == 0
    v = np.array([1.0, nan, 3.0, nan, 3.0, -inf], np.float32)                                # NaNs add nothing, -inf adds exp(-inf) = 0, a tie: the lowest
    lab, sc, prob = P.from_interpolants(v)
    assert lab == 2 and sc == 3 and prob == 1.0 / (np.exp(-2.0) + 2.0)
    # a NaN where the winner was: the runner-up wins and the NaN is no term of its sum
    x = logits_for((1, 3, 3, 21, 0), seed=13)
    x[0, 1, 1, int(x[0, 1, 1].argmax())] = nan
    lab, sc, prob = P.resample_softmax(x, 13, 17)
    want_lab, want_sc = dense_any_ref.resample_argmax(x, 13, 17)
    assert np.array_equal(lab, want_lab) and np.array_equal(_bits(sc), _bits(want_sc))
    v = dense_any_ref.resample(x, 13, 17)
    assert np.isnan(v).any() and np.isfinite(prob).all() and (prob > 0).all()
    manual = 1.0 / np.nansum(np.exp(v.astype(np.float64) - sc.astype(np.float64)[..., None]), axis=-1)
    assert np.allclose(prob, manual, rtol=1e-15, atol=0)
    # an all -inf coarse pixel: at its centre nothing wins
    x = logits_for((1, 3, 3, 21, 0), seed=17)
    x[0, 1, 1, :] = -inf
    lab, sc, prob = P.resample_softmax(x, 13, 13)
    assert lab[0, 6, 6] == 0 and sc[0, 6, 6] == -inf and prob[0, 6, 6] == 0 and (prob[sc > -inf] > 0).all()
    one = P.resample_softmax(logits_for((1, 2, 2, 1, 0), seed=1), 11, 9)[2]                  # one class: exactly 1
    assert (one == 1.0).all()


def test_ref_threshold():
    lab = np.array([3, 4, 5, 6], np.int32)
    prob = np.array([0.5, 0.49999, 0.0, 1.0])
    assert list(P.threshold(lab, prob, 0.5, 255)) == [3, 255, 255, 6]                        # strict
    assert list(P.threshold(lab, prob, 0.0, 255)) == [3, 4, 5, 6]                            # 0 never replaces, a prob of 0 included
    assert list(P.threshold(lab, prob, 1.0, -1)) == [-1, -1, -1, 6]
    assert P.bound(1000) == 1200 * 2.0 ** -24


@pytest.mark.parametrize("case", P.THRESHOLD_CASES)
def test_threshold_cases_leave_no_pixel_near_the_threshold(case):
    """What lets the GPU test compare thresholded label maps exactly: a kernel inside the bound decides every pixel of these inputs as the
    reference does. Both sides of every threshold are populated, so the comparison says something."""
    n, h, w, classes, H, W, seed, sigma, min_prob = case
    lab, _, prob = P.resample_softmax(P.threshold_input(case), H, W)
    assert int(P.excluded(prob, min_prob, classes).sum()) == 0
    under = prob < min_prob
    assert under.any() and not under.all(), under.mean()
    assert (P.threshold(lab, prob, min_prob, -1) == -1).sum() == under.sum()


def test_min_prob_check(pkg):
    chk = lambda have, p: pkg.softmax_readout_check(have, p)
    for have in (True, False):
        for bad in (float("nan"), -0.1, 1.5, float("inf"), -float("inf")):
            assert chk(have, bad) == pkg.EINVAL, (have, bad)
        for good in (1e-30, 0.5, 1.0):
            assert chk(have, good) == pkg.OK, (have, good)
    assert chk(True, 0.0) == pkg.OK and chk(True, -0.0) == pkg.OK
    assert chk(False, 0.0) == pkg.EINVAL                 # neither a map nor a threshold: that is the argmax call


DEVICE = ("mbn_resample_softmax_f32", "mbn_resample_softmax_window_f32", "mbn_resample_softmax_ragged_f32", "mbn_net_segment_prob_to",
          "mbn_net_segment_prob_fit", "mbn_net_segment_prob_images_fit")


def test_symbols_where_they_belong(pkg):
    lib, host = pkg.load(), pkg.host_lib()
    for name in DEVICE + ("mbn_softmax_readout_check",):
        assert hasattr(lib, name), name
    assert hasattr(host, "mbn_softmax_readout_check")
    for name in DEVICE:                                  # device code / the net runner: not in the host library
        assert not hasattr(host, name), name
    assert set(DEVICE) <= set(pkg.declared_symbols())
    for cls, name in ((pkg.Context, "resample_softmax"), (pkg.Context, "resample_softmax_window"), (pkg.RaggedReadout, "run_softmax"),
                      (pkg.Net, "segment_prob_to"), (pkg.Net, "segment_prob_fit"), (pkg.Net, "segment_prob_images_fit")):
        assert callable(getattr(cls, name))
