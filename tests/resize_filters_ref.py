"""Numpy statement of the resize front-end's arithmetic for every filter (include/mbn.h, "resize front-end"): Pillow's 8-bit resize with a float32
box under NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX and HAMMING. Independent of tests/resize_ref.py (the bilinear statement the older tests share)
and of the C host. Byte for byte what PIL.Image.resize((ow, oh), filter, box=box) returns; tests/golden/resize_pillow_filters.npz pins that
without Pillow."""
import math

import numpy as np

PRECISION_BITS = 22
NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 0, 1, 2, 3, 4, 5      # PIL.Image.Resampling's own numbers
NAMES = {NEAREST: "nearest", LANCZOS: "lanczos", BILINEAR: "bilinear", BICUBIC: "bicubic", BOX: "box", HAMMING: "hamming"}
FILTERS = (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING)
CONVOLUTIONS = (LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING)
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0


_F = {BOX: _box, HAMMING: _hamming, BICUBIC: _bicubic, LANCZOS: _lanczos}


def _scale(b0, b1, out_size):
    b0, b1 = np.float32(b0), np.float32(b1)
    return float(np.float32(b1 - b0)) / out_size           # the subtraction in float32, the division in double


def ksize(filt, in_size, b0, b1, out_size):
    if filt == NEAREST:
        return 1
    return int(math.ceil(SUPPORT[filt] * max(_scale(b0, b1, out_size), 1.0))) * 2 + 1


def taps(filt, in_size, b0, b1, out_size):
    """(first [out_size], count [out_size], weights [out_size][ksize], zero padded), all int32. NEAREST: the index, 1 and 2^22."""
    if filt == NEAREST:
        idx = nearest_index(in_size, b0, b1, out_size)
        return idx, np.ones(out_size, np.int32), np.full((out_size, 1), 1 << PRECISION_BITS, np.int32)
    scale = _scale(b0, b1, out_size)
    fs = max(scale, 1.0)
    support = SUPPORT[filt] * fs
    ks = int(math.ceil(support)) * 2 + 1
    first = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    weights = np.zeros((out_size, ks), np.int32)
    for i in range(out_size):
        center = float(np.float32(b0)) + (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)             # int() truncates toward zero, like the C cast
        hi = min(int(center + support + 0.5), in_size)
        n = hi - lo
        if filt == BILINEAR:                                 # the division it has always had
            w = [max(0.0, 1.0 - abs((t + lo - center + 0.5) / fs)) for t in range(n)]
        else:                                                # Pillow's form: a multiply by the reciprocal
            w = [_F[filt]((t + lo - center + 0.5) * (1.0 / fs)) for t in range(n)]
        s = 0.0
        for v in w:
            s += v
        if s != 0.0:
            w = [v / s for v in w]
        first[i], count[i] = lo, n
        for t, v in enumerate(w):
            weights[i, t] = int(v * 4194304.0 + 0.5) if v >= 0 else int(v * 4194304.0 - 0.5)
    return first, count, weights


def nearest_index(in_size, b0, b1, out_size, closed_form=False):
    """Pillow's scaled-affine path: xo accumulated. closed_form=True is the OTHER reading, b0 + a * (i + 0.5), which the tests show to differ."""
    a = _scale(b0, b1, out_size)
    b0 = float(np.float32(b0))
    idx = np.zeros(out_size, np.int32)
    xo = b0 + a * 0.5
    for i in range(out_size):
        v = b0 + a * (i + 0.5) if closed_form else xo
        idx[i] = min(max(int(v), 0), in_size - 1)
        xo += a
    return idx


def _pass(src, first, count, weights):
    """One pass along axis 1 of src [rows][n][ch] uint8 -> [rows][out][ch] uint8."""
    rows, _, ch = src.shape
    out = np.empty((rows, len(first), ch), np.uint8)
    s = src.astype(np.int64)
    for i in range(len(first)):
        lo, n = int(first[i]), int(count[i])
        acc = (s[:, lo:lo + n, :] * weights[i, :n].astype(np.int64)[None, :, None]).sum(axis=1) + (1 << (PRECISION_BITS - 1))
        out[:, i, :] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(filt, img, out_rows, out_cols, box=None, closed_form=False):
    """img uint8 [H][W][3] (or [N][H][W][3]); box = (left, upper, right, lower) float32, None = the whole image."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 4:
        return np.stack([resize(filt, x, out_rows, out_cols, box, closed_form) for x in img])
    h, w, _ = img.shape
    if box is None:
        box = (0.0, 0.0, float(w), float(h))
    if filt == NEAREST:
        ix = nearest_index(w, box[0], box[2], out_cols, closed_form)
        iy = nearest_index(h, box[1], box[3], out_rows, closed_form)
        return np.ascontiguousarray(img[iy][:, ix])
    fx, cx, wx = taps(filt, w, box[0], box[2], out_cols)
    fy, cy, wy = taps(filt, h, box[1], box[3], out_rows)
    tmp = _pass(img, fx, cx, wx)                                                  # horizontal first, rounded to uint8
    return np.ascontiguousarray(_pass(tmp.transpose(1, 0, 2), fy, cy, wy).transpose(1, 0, 2))
