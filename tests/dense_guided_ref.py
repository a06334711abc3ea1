"""The guided read-out in numpy float32: the normative arithmetic of mbn_resample_guided_f32 (include/mbn.h, "Segment along the image's edges"), bit
for bit, on dense_any_ref.axis / dense_window_ref.axis_window. Every product, sum and (correctly rounded) quotient is one float32 numpy operation."""
import numpy as np

import dense_any_ref
import dense_window_ref


def reduce_mean(canvas, S):
    """uint8 [n][R][C][3] -> uint8 [n][R / S][C / S][3]: per channel the rounded mean of every S x S block, (sum + S * S / 2) // (S * S)."""
    n, R, C, _ = canvas.shape
    s = canvas.reshape(n, R // S, S, C // S, S, 3).astype(np.int64).sum(axis=(2, 4))
    return ((s + S * S // 2) // (S * S)).astype(np.uint8)


def weights(guide_lo, guide_hi, lut, in_rows=0, in_cols=0, rect=None, dtype=np.float32):
    """-> (iy [2][H], ix [2][W], b [2][2] of dtype [n][H][W]): neighbour (j, k) of output (oy, ox) is (iy[j][oy], ix[k][ox]), b[j][k] its weight
    (dtype float64: the same operations in float64 on the float32 w1 and table, what tolerance() is stated against)."""
    (h, w), (H, W) = guide_lo.shape[1:3], guide_hi.shape[1:3]
    if rect is None:
        y0, y1, _, wy1 = dense_any_ref.axis(H, h)
        x0, x1, _, wx1 = dense_any_ref.axis(W, w)
    else:
        y0, y1, _, wy1 = dense_window_ref.axis_window(H, h, in_rows, int(rect[1]), int(rect[3]))
        x0, x1, _, wx1 = dense_window_ref.axis_window(W, w, in_cols, int(rect[0]), int(rect[2]))
    wy1, wx1 = wy1.astype(dtype), wx1.astype(dtype)
    iy, ix, wy, wx = (y0, y1), (x0, x1), (dtype(1.0) - wy1, wy1), (dtype(1.0) - wx1, wx1)
    hi, lut = guide_hi.astype(np.int64), np.asarray(lut, np.float32).astype(dtype)
    d = lambda j, k: np.abs(hi - guide_lo[:, iy[j]][:, :, ix[k]].astype(np.int64)).sum(axis=-1)               # [n][H][W], 0..765
    a = [[(wy[j][None, :, None] * wx[k][None, None, :]) * lut[d(j, k)] for k in range(2)] for j in range(2)]
    A = ((a[0][0] + a[0][1]) + a[1][0]) + a[1][1]
    return iy, ix, [[a[j][k] / A for k in range(2)] for j in range(2)]


def interpolants(x, guide_lo, guide_hi, lut, in_rows=0, in_cols=0, rect=None, dtype=np.float32):
    """x: float32 [n][h][w][classes] -> v [n][H][W][classes] in dtype."""
    iy, ix, b = weights(guide_lo, guide_hi, lut, in_rows, in_cols, rect, dtype)
    x = np.ascontiguousarray(x, np.float32).astype(dtype)
    g = lambda j, k: x[:, iy[j]][:, :, ix[k]]                                                              # [n][H][W][classes]
    with np.errstate(invalid="ignore"):          # 0 * inf is a NaN by the definition too
        return (b[0][0][..., None] * g(0, 0) + b[0][1][..., None] * g(0, 1)) + (b[1][0][..., None] * g(1, 0) + b[1][1][..., None] * g(1, 1))


def tolerance(x):
    """Bound on |v - the float64 evaluation of the same formula| (dtype=np.float64: the float32 w1 and table are its data), in
    units of u = 2^-24 max|x|, every rounding a relative error of at most 2^-24. A weight b_jk: w0 = 1.0f - w1 rounds once per axis (2), wy * wx
    (1) and the product with g (1) make 4 for a_jk; A sums four such terms (4) with three additions (3): 7; the quotient (1): 12. A term b * x
    then takes its product (1) and two of the three sums (2): 15 per term, and the exact weights are positive and sum to 1, so the terms'
    magnitudes sum to at most max|x|: 15 u. The second-order terms and the float64 side are below one unit at this scale: 16."""
    return 16.0 * 2.0 ** -24 * float(np.abs(x[np.isfinite(x)]).max())
