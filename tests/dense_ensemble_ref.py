"""The ensemble read-out in numpy float32: the normative arithmetic of mbn_resample_ensemble_f32 (include/mbn.h, "Segment with test-time
augmentation"), bit for bit, on top of dense_window_ref. A view is (x, y, iw, ih, mirror): the rectangle of the network input that holds the whole
image and whether the network saw it mirrored. For view k the interpolants at output (oy, ox) are dense_window_ref.resample_window's for that
rectangle, the columns read at W - 1 - ox when the view is mirrored; the views are summed in order, one float32 addition each, the sum is
multiplied by float32(1) / float32(K) once, and the argmax (dense_window_ref's rule) and the float64 softmax (dense_prob_ref.from_interpolants)
see that mean."""
import numpy as np

import dense_prob_ref
import dense_window_ref


def view_tuple(v):
    """(x, y, iw, ih, mirror) of a tuple or of anything with those attributes (the package's View)"""
    if hasattr(v, "iw"):
        return int(v.x), int(v.y), int(v.iw), int(v.ih), int(v.mirror)
    x, y, iw, ih, mirror = (int(t) for t in v)
    return x, y, iw, ih, mirror


def interpolants(x, in_rows, in_cols, view, H, W):
    """x: float32 [n][h][w][classes] of ONE view -> its interpolated logits [n][H][W][classes] in the source's own orientation"""
    rx, ry, iw, ih, mirror = view_tuple(view)
    v = dense_window_ref.resample_window(x, in_rows, in_cols, (rx, ry, iw, ih), H, W)
    return v[:, :, ::-1] if mirror else v          # output ox reads the window's column W - 1 - ox


def mean(x, in_rows, in_cols, views, H, W):
    """x: float32 [K][n][h][w][classes], view-major -> t float32 [n][H][W][classes]: the sum in view order, then one product by 1 / K"""
    x = np.ascontiguousarray(x, np.float32)
    K = len(views)
    assert x.shape[0] == K and 1 <= K <= 8
    with np.errstate(invalid="ignore", over="ignore"):          # inf - inf is a NaN by the definition too
        s = interpolants(x[0], in_rows, in_cols, views[0], H, W)
        for k in range(1, K):
            s = s + interpolants(x[k], in_rows, in_cols, views[k], H, W)
        return s * (np.float32(1.0) / np.float32(K))


def ensemble(x, in_rows, in_cols, views, H, W):
    """(labels int32, score float32, prob float64) [n][H][W]: dense_prob_ref.from_interpolants on the mean (its labels and scores are
    dense_window_ref.resample_argmax_window's rule: classes ascending, strict compare, a NaN never wins, label 0 and -inf when nothing wins)"""
    return dense_prob_ref.from_interpolants(mean(x, in_rows, in_cols, views, H, W))


def fit_view(in_rows, in_cols, out_rows, out_cols, scale, mirror):
    """mbn_fit_view written out: (x, y, iw, ih, mirror), or None where it answers MBN_EINVAL. Python's round is rint (half to even)."""
    if not (0.0 < scale <= 1.0) or mirror not in (0, 1) or min(in_rows, in_cols, out_rows, out_cols) <= 0:
        return None
    scale = float(np.float32(scale))
    sc, sr = int(round(out_cols * scale)), int(round(out_rows * scale))
    if sr < 1 or sc < 1:
        return None
    # mbn_fit_pad(in_rows, in_cols, sr, sc): doubles, the quotient before the product
    iw, ih, x, y = sc, sr, 0, 0
    if in_cols / in_rows != sc / sr:
        if in_cols / in_rows > sc / sr:
            ih = int(round(in_rows / in_cols * sc))
        else:
            iw = int(round(in_cols / in_rows * sr))
    if iw < 1 or ih < 1 or iw > sc or ih > sr:
        return None
    if iw != sc:
        x = int(round((sc - iw) * 0.5))
    elif ih != sr:
        y = int(round((sr - ih) * 0.5))
    return x + (out_cols - sc) // 2, y + (out_rows - sr) // 2, iw, ih, mirror


# The inputs and thresholds of the GPU threshold test (test_dense_ensemble_gpu.py); test_dense_ensemble_cpu.py checks that `excluded` leaves out at
# most 1 % of their pixels and that each threshold cuts through its map (the mean of three views is flatter than one view).
# (n, h, w, classes, views, H, W, seed, sigma, min_prob); the maps cover a 32 h x 32 w input
def _views3(h, w):
    R, Cc = 32 * h, 32 * w
    return [(0, 0, Cc, R, 0), (Cc // 8, R // 8, 3 * Cc // 4, 3 * R // 4, 0), (Cc // 4, R // 4, Cc // 2, R // 2, 1)]


THRESHOLD_CASES = [(2, 5, 7, 21, _views3(5, 7), 37, 61, 201, 3.0, 0.25),
                   (2, 5, 7, 21, _views3(5, 7), 37, 61, 201, 3.0, 0.4),
                   (1, 2, 3, 64, _views3(2, 3)[:2], 45, 70, 202, 2.0, 0.1)]


def threshold_input(case):
    n, h, w, classes, views, H, W, seed, sigma, _ = case
    return (sigma * np.random.default_rng(seed).standard_normal((len(views), n, h, w, classes))).astype(np.float32)
