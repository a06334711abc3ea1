"""The dense head's read-out at any output size in numpy float32: the normative arithmetic of mbn_resample_argmax_f32 (include/mbn.h, "Dense head
at the source resolution"), bit for bit. Every product and every sum is one float32 numpy operation, so each rounds on its own (numpy never
contracts into an FMA); a weight is the float64 quotient (num % den) / den rounded once to float32. The argmax rule is dense_ref's."""
import numpy as np

_CHUNK = 64          # classes per pass: bounds the (n, H, W, chunk) intermediates


def axis(n_out, n_in):
    """(i0, i1, w0, w1) of every output coordinate of an axis with n_in coarse samples resampled to n_out (half-pixel centres)."""
    o = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * o + 1) * n_in - n_out, 0)
    den = 2 * n_out
    i0 = num // den
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = ((num % den).astype(np.float64) / np.float64(den)).astype(np.float32)
    w0 = np.float32(1.0) - w1
    return i0, i1, w0, w1


def resample(x, H, W):
    """x: float32 [n][h][w][classes] -> the interpolated logits [n][H][W][classes]: horizontal first, then vertical."""
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, c = x.shape
    y0, y1, wy0, wy1 = axis(H, h)
    x0, x1, wx0, wx1 = axis(W, w)
    with np.errstate(invalid="ignore"):          # 0 * inf is a NaN by the definition too
        t = x[:, :, x0, :] * wx0[None, None, :, None] + x[:, :, x1, :] * wx1[None, None, :, None]      # rows y: t0 = t[y0], t1 = t[y1]
        return t[:, y0] * wy0[None, :, None, None] + t[:, y1] * wy1[None, :, None, None]


def resample_argmax(x, H, W):
    """(labels int32, score float32) [n][H][W]: best = -inf, label = 0; classes ascending, class c taken iff v > best (strict): the lowest
    index wins a tie, a NaN never wins, an all-NaN / all -inf pixel is label 0 with score -inf (dense_ref.upsample_argmax's rule)."""
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, classes = x.shape
    best = np.full((n, H, W), -np.inf, np.float32)
    label = np.zeros((n, H, W), np.int32)
    for c0 in range(0, classes, _CHUNK):
        v = resample(x[..., c0:c0 + _CHUNK], H, W)
        v = np.where(np.isnan(v), np.float32(-np.inf), v)
        idx = v.argmax(axis=-1)                    # the first of equal maxima
        m = np.take_along_axis(v, idx[..., None], axis=-1)[..., 0]
        take = m > best
        best = np.where(take, m, best)
        label = np.where(take, (c0 + idx).astype(np.int32), label)
    return label, best


def tolerance(x):
    """Bound on |score - torch's interpolate on float64 inputs|, with each rounding at most 2^-24 max|x|: per stage two products and one sum
    plus at most 1.5 from the two rounded weights make 4.5, the two stages 9; the float64 side adds nothing at this scale; rounded up to 10."""
    return 10.0 * 2.0 ** -24 * float(np.abs(x[np.isfinite(x)]).max())
