"""Numpy statement of the resize front-end's arithmetic (include/mbn.h, "resize front-end"): Pillow's 8-bit bilinear resize with a float32 box,
two passes with a uint8 intermediate, 22-bit fixed-point weights. Shared by the CPU and GPU tests: byte for byte what
PIL.Image.resize((ow, oh), Image.BILINEAR, box=box) returns (tests/golden/resize_pillow.npz pins that without Pillow)."""
import math

import numpy as np

PRECISION_BITS = 22
FIT_STRETCH, FIT_CROP = 0, 1


def ksize(in_size, b0, b1, out_size):
    b0, b1 = np.float32(b0), np.float32(b1)
    scale = float(np.float32(b1 - b0)) / out_size          # the subtraction in float32, the division in double
    return int(math.ceil(max(scale, 1.0))) * 2 + 1


def taps(in_size, b0, b1, out_size):
    """(first [out_size], count [out_size], weights [out_size][ksize], zero padded), all int32."""
    b0, b1 = np.float32(b0), np.float32(b1)
    scale = float(np.float32(b1 - b0)) / out_size
    fs = max(scale, 1.0)
    support = fs
    ks = int(math.ceil(support)) * 2 + 1
    first = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    weights = np.zeros((out_size, ks), np.int32)
    for i in range(out_size):
        center = float(b0) + (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)             # int() truncates toward zero, like the C cast
        hi = min(int(center + support + 0.5), in_size)
        n = hi - lo
        w = [max(0.0, 1.0 - abs((t + lo - center + 0.5) / fs)) for t in range(n)]
        s = 0.0
        for v in w:
            s += v
        if s != 0.0:
            w = [v / s for v in w]
        first[i], count[i] = lo, n
        for t, v in enumerate(w):
            weights[i, t] = int(v * float(1 << PRECISION_BITS) + 0.5)
    return first, count, weights


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


def resize(img, out_rows, out_cols, box=None):
    """img uint8 [H][W][3] (or [N][H][W][3]); box = (left, upper, right, lower) float32, None = the whole image."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 4:
        return np.stack([resize(x, out_rows, out_cols, box) for x in img])
    h, w, _ = img.shape
    if box is None:
        box = (0.0, 0.0, float(w), float(h))
    fx, cx, wx = taps(w, box[0], box[2], out_cols)
    fy, cy, wy = taps(h, box[1], box[3], out_rows)
    tmp = _pass(img, fx, cx, wx)                                                  # horizontal first, rounded to uint8
    return np.ascontiguousarray(_pass(tmp.transpose(1, 0, 2), fy, cy, wy).transpose(1, 0, 2))


def fit_box(in_rows, in_cols, out_rows, out_cols, fit=FIT_CROP, crop_fraction=1.0):
    """(left, upper, right, lower) as float32: the whole image (STRETCH) or the centred box with the output's aspect ratio (CROP)."""
    W, H = float(in_cols), float(in_rows)
    if fit == FIT_STRETCH:
        return np.array([0.0, 0.0, W, H], np.float32)
    bw = min(W, H * out_cols / out_rows) * float(np.float32(crop_fraction))                # the C interface takes a float32
    bh = bw * out_rows / out_cols
    left, upper = (W - bw) / 2, (H - bh) / 2
    b = np.array([left, upper, left + bw, upper + bh], np.float64).astype(np.float32)
    return np.array([max(b[0], 0), max(b[1], 0), min(b[2], np.float32(W)), min(b[3], np.float32(H))], np.float32)
