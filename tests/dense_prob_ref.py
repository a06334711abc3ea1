"""The dense head's read-out with confidence: the normative arithmetic of mbn_resample_softmax_f32 / _window_f32 (include/mbn.h, "Segment with
confidence") on top of dense_any_ref / dense_window_ref. The interpolated logits v are theirs, in numpy float32, bit for bit; best and label
follow their argmax rule; prob is the FLOAT64 evaluation of 1 / sum_c e(v_c), e(v) = exp(v - best) for a v that is not NaN and 0 for a NaN,
and 0 where best is not finite. The kernel's fp32 prob is held to bound(classes) relative to it."""
import numpy as np

import dense_any_ref
import dense_window_ref


def bound(classes):
    """the relative error a kernel's prob may have wherever the reference's is nonzero (include/mbn.h derives it)"""
    return (classes + 200) * 2.0 ** -24


def from_interpolants(v):
    """v: float32 [..., classes] -> (labels int32, score float32, prob float64) [...]. Classes ascending, class c taken iff v > best (strict),
    best = -inf and label = 0 to start with: the first of equal maxima wins, a NaN never wins."""
    v = np.asarray(v, np.float32)
    nan = np.isnan(v)
    cand = np.where(nan, np.float32(-np.inf), v)
    label = cand.argmax(axis=-1).astype(np.int32)                  # the first of equal maxima; 0 when every candidate is -inf
    best = np.take_along_axis(cand, label[..., None].astype(np.int64), axis=-1)[..., 0]
    finite = np.isfinite(best)
    with np.errstate(invalid="ignore", over="ignore"):
        d = v.astype(np.float64) - np.where(finite, best, np.float32(0)).astype(np.float64)[..., None]
        e = np.where(nan, 0.0, np.exp(d))                          # exp(-inf) = 0; d <= 0 wherever best is finite
        s = e.sum(axis=-1)
        prob = np.where(finite, 1.0 / np.where(finite, s, 1.0), 0.0)
    return label, best, prob


def resample_softmax(x, H, W):
    """(labels int32, score float32, prob float64) [n][H][W] of x float32 [n][h][w][classes] resampled to H x W"""
    return from_interpolants(dense_any_ref.resample(x, H, W))


def resample_softmax_window(x, in_rows, in_cols, rect, H, W):
    """the same for the window rect = (x, y, iw, ih) of the in_rows x in_cols input"""
    return from_interpolants(dense_window_ref.resample_window(x, in_rows, in_cols, rect, H, W))


def threshold(labels, prob, min_prob, ignore):
    """the stored labels: ignore wherever prob < min_prob (strict)"""
    return np.where(np.asarray(prob) < min_prob, np.int32(ignore), labels).astype(np.int32)


def excluded(prob, min_prob, classes):
    """the pixels whose thresholded label a kernel inside bound(classes) may get either way: |prob - min_prob| <= bound * prob"""
    prob = np.asarray(prob, np.float64)
    return np.abs(prob - min_prob) <= bound(classes) * prob


# The inputs and thresholds of the GPU threshold test (test_dense_prob_gpu.py); test_dense_prob_cpu.py checks that none of their pixels is
# `excluded`, so the GPU test may compare the thresholded maps exactly. (n, h, w, classes, H, W, seed, sigma, min_prob)
THRESHOLD_CASES = [(2, 5, 7, 21, 37, 61, 101, 3.0, 0.5),
                   (2, 5, 7, 21, 37, 61, 101, 3.0, 0.9),
                   (1, 3, 5, 64, 100, 23, 102, 2.0, 0.25),
                   (1, 2, 2, 130, 11, 9, 103, 1.0, 0.05)]


def threshold_input(case):
    n, h, w, classes, H, W, seed, sigma, _ = case
    return (sigma * np.random.default_rng(seed).standard_normal((n, h, w, classes))).astype(np.float32)
