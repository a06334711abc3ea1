"""The dense head's read-out of a WINDOW of the network's input in numpy float32: the normative arithmetic of mbn_resample_argmax_window_f32
(include/mbn.h, "Segment through the letterbox"), bit for bit, on top of dense_any_ref. Only the index / weight rule differs from dense_any_ref:
the coarse map has n samples along an axis and covers R input pixels, the window [b, b + l) of them is resampled to N outputs. Every product and
every sum is one float32 numpy operation; a weight is the float64 quotient (num % den) / den rounded once to float32; 64-bit integers throughout."""
import numpy as np

import dense_any_ref

_CHUNK = 64          # classes per pass, as dense_any_ref


def axis_window(n_out, n_in, R, b, l):
    """(i0, i1, w0, w1) of every output coordinate: output o of n_out sits at input coordinate b + (o + 1/2) l / n_out of the R pixels that the
    n_in coarse samples cover. No clamp at the window's edge; i0 <= n_in - 1 follows from b + l <= R."""
    assert b >= 0 and l >= 1 and b + l <= R
    o = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * o + 1) * np.int64(l) * n_in + 2 * np.int64(b) * n_in * n_out - np.int64(n_out) * R, 0)
    den = 2 * np.int64(n_out) * R
    i0 = num // den
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = ((num % den).astype(np.float64) / np.float64(den)).astype(np.float32)
    w0 = np.float32(1.0) - w1
    return i0, i1, w0, w1


def resample_window(x, in_rows, in_cols, rect, H, W):
    """x: float32 [n][h][w][classes] -> the interpolated logits [n][H][W][classes] of the window rect = (x, y, iw, ih) of the in_rows x in_cols
    input: horizontal first, then vertical (dense_any_ref.resample's operations on the window's indices and weights)."""
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, c = x.shape
    rx, ry, iw, ih = (int(v) for v in rect)
    y0, y1, wy0, wy1 = axis_window(H, h, in_rows, ry, ih)
    x0, x1, wx0, wx1 = axis_window(W, w, in_cols, rx, iw)
    with np.errstate(invalid="ignore"):          # 0 * inf is a NaN by the definition too
        t = x[:, :, x0, :] * wx0[None, None, :, None] + x[:, :, x1, :] * wx1[None, None, :, None]
        return t[:, y0] * wy0[None, :, None, None] + t[:, y1] * wy1[None, :, None, None]


def resample_argmax_window(x, in_rows, in_cols, rect, H, W):
    """(labels int32, score float32) [n][H][W] under dense_any_ref.resample_argmax's rule: best = -inf, label = 0; classes ascending, class c
    taken iff v > best (strict); a NaN never wins."""
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, classes = x.shape
    best = np.full((n, H, W), -np.inf, np.float32)
    label = np.zeros((n, H, W), np.int32)
    for c0 in range(0, classes, _CHUNK):
        v = resample_window(x[..., c0:c0 + _CHUNK], in_rows, in_cols, rect, H, W)
        v = np.where(np.isnan(v), np.float32(-np.inf), v)
        idx = v.argmax(axis=-1)                    # the first of equal maxima
        m = np.take_along_axis(v, idx[..., None], axis=-1)[..., 0]
        take = m > best
        best = np.where(take, m, best)
        label = np.where(take, (c0 + idx).astype(np.int32), label)
    return label, best


tolerance = dense_any_ref.tolerance      # the same operations per output, so the same bound against a float64 evaluation
