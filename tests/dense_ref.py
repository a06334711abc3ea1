"""The dense head's read-out in numpy float32: the normative arithmetic of mbn_upsample_argmax_f32 (include/mbn.h, "Dense head read-out"),
bit for bit. Every product and every sum is one float32 numpy operation, so each rounds on its own (numpy never contracts into an FMA);
the weights are exact dyadic fractions."""
import numpy as np

_CHUNK = 64          # classes per pass: bounds the (n, H, W, chunk) intermediates


def axis(n_out, n_in, S):
    """(i0, i1, w0, w1) of every output coordinate of an axis with n_in coarse samples upsampled by S (half-pixel centres)."""
    o = np.arange(n_out, dtype=np.int64)
    num = np.maximum(2 * o + 1 - S, 0)
    i0 = num // (2 * S)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = (num % (2 * S)).astype(np.float32) / np.float32(2 * S)
    w0 = np.float32(1.0) - w1
    return i0, i1, w0, w1


def upsample(x, S):
    """x: float32 [n][h][w][classes] -> the interpolated logits [n][h*S][w*S][classes]: horizontal first, then vertical."""
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, c = x.shape
    y0, y1, wy0, wy1 = axis(h * S, h, S)
    x0, x1, wx0, wx1 = axis(w * S, w, S)
    with np.errstate(invalid="ignore"):          # 0 * inf is a NaN by the definition too
        t = x[:, :, x0, :] * wx0[None, None, :, None] + x[:, :, x1, :] * wx1[None, None, :, None]      # rows y: t0 = t[y0], t1 = t[y1]
        return t[:, y0] * wy0[None, :, None, None] + t[:, y1] * wy1[None, :, None, None]


def upsample_argmax(x, S):
    """(labels int32, score float32) [n][h*S][w*S]: best = -inf, label = 0; classes ascending, class c taken iff v > best (strict): the
    lowest index wins a tie, a NaN never wins, an all-NaN / all -inf pixel is label 0 with score -inf."""
    x = np.ascontiguousarray(x, np.float32)
    n, h, w, classes = x.shape
    best = np.full((n, h * S, w * S), -np.inf, np.float32)
    label = np.zeros((n, h * S, w * S), np.int32)
    for c0 in range(0, classes, _CHUNK):
        v = upsample(x[..., c0:c0 + _CHUNK], S)
        v = np.where(np.isnan(v), np.float32(-np.inf), v)
        idx = v.argmax(axis=-1)                    # the first of equal maxima
        m = np.take_along_axis(v, idx[..., None], axis=-1)[..., 0]
        take = m > best
        best = np.where(take, m, best)
        label = np.where(take, (c0 + idx).astype(np.int32), label)
    return label, best


def tolerance(x):
    """Bound on |dense_ref score - another correct float32 evaluation's| (torch): each evaluation makes at most four roundings of
    magnitudes <= max|x| on the path to a result (half an ulp of a value below max|x| is at most 2^-24 max|x|), and there are two."""
    return 8.0 * 2.0 ** -24 * float(np.abs(x[np.isfinite(x)]).max())
