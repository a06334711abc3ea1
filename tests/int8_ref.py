"""numpy statement of the int8 inference mode (include/mbn.h, "int8 inference mode"), shared by tests/test_int8_cpu.py and
tests/test_int8_gpu.py. Everything here is exact integer arithmetic or single float32 operations in the order the header fixes, so the
device results must equal it bit for bit (conv1 excepted: its fp32 sum is compared against float64 within one step)."""
import numpy as np

L_CONV, L_DW, L_PW, L_POOL, L_FC = 1, 2, 3, 4, 5
DEFAULT_SCALE = np.float32(6.0) / np.float32(255.0)
NORM_SCALE, NORM_BIAS = np.float32(1.0) / np.float32(127.5), np.float32(-1.0)


def quantize_channels(w):
    """w float32 [C][T] (one row per output channel) -> (int8 [C][T], s_w float64 [C])"""
    w = np.asarray(w, np.float32)
    absmax = np.abs(w).max(axis=1).astype(np.float32)
    nz = absmax > 0
    inv = np.where(nz, np.float32(127.0) / np.where(nz, absmax, np.float32(1)), np.float32(0)).astype(np.float32)
    q = np.clip(np.rint((w * inv[:, None]).astype(np.float32)), -127, 127).astype(np.int8)
    q[~nz] = 0
    s_w = np.where(nz, absmax.astype(np.float64) / 127.0, 1.0)
    return q, s_w


def quantize(plan, blob, scales=None):
    """Per layer: dict(kind, w8 (blob element order, None for conv1 / pool), mult, bias (float32), in_scale, out_scale)."""
    blob = np.asarray(blob, np.float32)
    out = []
    s_prev = np.float32(1.0)
    for i in range(plan.n_layers):
        l = plan.layer[i]
        d = dict(kind=l.kind, w8=None, mult=None, bias=None, in_scale=s_prev)
        if l.kind == L_POOL:
            d["out_scale"] = s_prev
            out.append(d)
            continue
        fc = l.kind == L_FC
        s_out = np.float32(0.0) if fc else (np.float32(scales[i]) if scales is not None else DEFAULT_SCALE)
        d["out_scale"] = s_out
        C = l.out_ch
        w = blob[l.w_offset:l.w_offset + l.w_count]
        if l.kind == L_CONV:
            s_w = np.ones(C)
            s_in = 1.0
        elif l.kind == L_DW:
            q, s_w = quantize_channels(w.reshape(9, C).T)
            d["w8"] = np.ascontiguousarray(q.T).reshape(-1)
            s_in = float(s_prev)
        else:
            q, s_w = quantize_channels(w.reshape(C, l.in_ch))
            d["w8"] = q.reshape(-1)
            s_in = float(s_prev)
        bn_scale = blob[l.scale_offset:l.scale_offset + C].astype(np.float64) if l.scale_offset >= 0 else np.ones(C)
        bn_shift = blob[l.shift_offset:l.shift_offset + C].astype(np.float64) if l.shift_offset >= 0 else np.zeros(C)
        so = 1.0 if fc else float(s_out)
        d["mult"] = (s_w * s_in * bn_scale / so).astype(np.float32)
        d["bias"] = (bn_shift / so).astype(np.float32)
        out.append(d)
        s_prev = s_out
    return out


def requant_f32(acc, mult, bias):
    """y = (float)acc * mult + bias, two float32 roundings (no FMA); acc int64 holding an int32 value, channel last"""
    return (acc.astype(np.float32) * np.asarray(mult, np.float32)).astype(np.float32) + np.asarray(bias, np.float32)


def to_u8(y):
    return np.clip(np.rint(y), 0, 255).astype(np.uint8)


def same_pad(n, o, stride):
    t = (o - 1) * stride + 3 - n
    return t // 2 if t > 0 else 0


def dw_acc(x, w8, stride, pad_top, pad_left, ho, wo):
    """x uint8 [N][H][W][C], w8 int8 [3][3][C] -> exact int64 sums [N][ho][wo][C]"""
    n, h, w, c = x.shape
    xp = np.zeros((n, max(h, (ho - 1) * stride + 3) + pad_top + 3, max(w, (wo - 1) * stride + 3) + pad_left + 3, c), np.int64)
    xp[:, pad_top:pad_top + h, pad_left:pad_left + w] = x
    wk = np.asarray(w8, np.int64).reshape(3, 3, c)
    acc = np.zeros((n, ho, wo, c), np.int64)
    for ky in range(3):
        for kx in range(3):
            acc += xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride] * wk[ky, kx]
    return acc


def dw(x, w8, mult, bias, stride, pad_top=None, pad_left=None, ho=None, wo=None):
    h, w = x.shape[1:3]
    ho = ho if ho is not None else (h + stride - 1) // stride
    wo = wo if wo is not None else (w + stride - 1) // stride
    pt = same_pad(h, ho, stride) if pad_top is None else pad_top
    pl = same_pad(w, wo, stride) if pad_left is None else pad_left
    return to_u8(requant_f32(dw_acc(x, w8, stride, pt, pl, ho, wo), mult, bias))


def pw_acc(x, w8):
    """x uint8 [M][K], w8 int8 [N][K] -> exact sums [M][N] (float64 matmul: every partial sum < 2^53)"""
    return (np.asarray(x, np.float64) @ np.asarray(w8, np.float64).T).astype(np.int64)


def pw(x, w8, mult, bias, out_f32=False):
    y = requant_f32(pw_acc(x, w8), mult, bias)
    return y if out_f32 else to_u8(y)


def pw_blocks(x, w8, mult, bias, out_f32=False, block=8192):
    """pw() over row blocks of a tall x: yields (first row, rows' outputs); the float64 product of a block only is in memory"""
    w = np.asarray(w8, np.float64).T.copy()
    for i in range(0, len(x), block):
        y = requant_f32((np.asarray(x[i:i + block], np.float64) @ w).astype(np.int64), mult, bias)
        yield i, (y if out_f32 else to_u8(y))


def pool(x):
    """x uint8 [N][H][W][C] -> uint8 [N][C]"""
    n, h, w, c = x.shape
    s = x.reshape(n, h * w, c).astype(np.int64).sum(axis=1)
    inv = np.float32(1.0) / np.float32(h * w)
    return to_u8((s.astype(np.float32) * inv).astype(np.float32))


def conv1_y(img, w, mult, bias, stride=2, pad_top=None, pad_left=None):
    """img float [N][H][W][cin] (already normalised), w fp32 [3][3][cin][C] -> float64 y = acc * mult + bias [N][ho][wo][C]"""
    return conv1_acc(img, w, stride, pad_top, pad_left) * np.asarray(mult, np.float64) + np.asarray(bias, np.float64)


def conv1_acc(img, w, stride=2, pad_top=None, pad_left=None):
    """float64 sums of the 3x3 convolution; the output map is ceil(H / stride) x ceil(W / stride) whatever the pads (None: TF-SAME)"""
    n, h, wd, cin = img.shape
    C = w.shape[-1]
    ho, wo = (h + stride - 1) // stride, (wd + stride - 1) // stride
    pt = same_pad(h, ho, stride) if pad_top is None else pad_top
    pl = same_pad(wd, wo, stride) if pad_left is None else pad_left
    xp = np.zeros((n, h + 4, wd + 4, cin), np.float64)
    xp[:, pt:pt + h, pl:pl + wd] = img
    acc = np.zeros((n, ho, wo, C), np.float64)
    wk = np.asarray(w, np.float64).reshape(3, 3, cin, C)
    for ky in range(3):
        for kx in range(3):
            patch = xp[:, ky:ky + (ho - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
            acc += patch @ wk[ky, kx]
    return acc


# conv1 on a grid on which its fp32 sum is exact in any order: image values k / 2^7 in [-1, 1], taps k / 2^6 with |w| <= 2. A term is a multiple
# of 2^-13 of at most 2^14 units and the 27 of a sum stay below 27 * 2^14 < 2^24 units: every partial sum, fused or not, is an integer number of
# units that fp32 holds exactly (tests/test_int8_cpu.py proves it on the inputs built here).
CONV1_IMG_BITS, CONV1_TAP_BITS = 7, 6


CONV1_CHANNELS = (8, 16, 24, 32, 48)                            # every NG of i8_conv_k, and blockIdx.y > 0
CONV1_MAPS = ((64, 64), (63, 37), (5, 3))                       # a square map, an odd non-square one, one smaller than a workgroup
CONV1_PADS = ((None, None), (0, 1), (1, 0))                     # TF-SAME, and explicit pads with pad_top != pad_left


def conv1_exact_inputs(rng, n, h, w, c):
    """(image fp32 [n][h][w][3], taps fp32 [3][3][3][c], mult, bias) on that grid; mult / bias spread y over both clamps and the interior:
    the sums have a standard deviation near 3.5 (27 terms of variance 1/3 * 4/3), y = 36 acc + 128 leaves [0, 255] for |acc| > 3.5"""
    img = (rng.integers(-(1 << CONV1_IMG_BITS), (1 << CONV1_IMG_BITS) + 1, (n, h, w, 3)) / float(1 << CONV1_IMG_BITS)).astype(np.float32)
    taps = (rng.integers(-(2 << CONV1_TAP_BITS), (2 << CONV1_TAP_BITS) + 1, (3, 3, 3, c)) / float(1 << CONV1_TAP_BITS)).astype(np.float32)
    mult = rng.uniform(24, 48, c).astype(np.float32)
    bias = rng.uniform(100, 156, c).astype(np.float32)
    return img, taps, mult, bias


def conv1_grid_units(img, taps, stride=1, pad_top=None, pad_left=None):
    """max over the outputs of sum |term| in units of 2^-(CONV1_IMG_BITS + CONV1_TAP_BITS): below 2^24, every order of the sum is exact"""
    unit = float(1 << (CONV1_IMG_BITS + CONV1_TAP_BITS))
    for a, bits in ((img, CONV1_IMG_BITS), (taps, CONV1_TAP_BITS)):
        k = np.asarray(a, np.float64) * (1 << bits)
        assert np.array_equal(k, np.rint(k)), "off the grid"
    return float(conv1_acc(np.abs(img), np.abs(taps), stride, pad_top, pad_left).max() * unit)


def conv1_exact(img, taps, mult, bias, stride=2, pad_top=None, pad_left=None):
    """uint8 conv1 of grid inputs: the exact sum (fp32 holds it), then the header's two float32 roundings, rint, clamp"""
    acc = conv1_acc(img, taps, stride, pad_top, pad_left)
    a32 = acc.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), acc)
    return to_u8((a32 * np.asarray(mult, np.float32)).astype(np.float32) + np.asarray(bias, np.float32))


def assert_conv1_one_step(got, y, what=""):
    """The rule for a conv1 whose fp32 sum is not exact: within one step of rint(clip(y)) of the float64 y, and different only where y is
    within 2^-10 of a half-integer"""
    got = np.asarray(got).astype(np.int64)
    want = np.clip(np.rint(y), 0, 255).astype(np.int64)
    diff = got != want
    assert np.abs(got - want).max() <= 1, what
    yc = np.clip(y, 0, 255)
    assert np.all(np.abs(yc[diff] - (np.floor(yc[diff]) + 0.5)) < 2.0 ** -10), "%s: mismatch away from a half-integer" % what
    assert diff.mean() < 1e-3, what


def layer_from_prev(l, q, prev):
    """Layer l (plan descriptor) from the previous layer's device output `prev` (uint8 NHWC, or [N][C] after the pool)."""
    if l.kind == L_DW:
        return dw(prev, q["w8"], q["mult"], q["bias"], l.stride, l.pad_top, l.pad_left, l.out_rows, l.out_cols)
    if l.kind == L_PW:
        n = prev.shape[0]
        return pw(prev.reshape(-1, l.in_ch), q["w8"].reshape(l.out_ch, l.in_ch), q["mult"], q["bias"]).reshape(
            n, l.out_rows, l.out_cols, l.out_ch)
    if l.kind == L_POOL:
        return pool(prev).reshape(prev.shape[0], 1, 1, l.out_ch)
    if l.kind == L_FC:
        return pw(prev.reshape(prev.shape[0], l.in_ch), q["w8"].reshape(l.out_ch, l.in_ch), q["mult"], q["bias"], out_f32=True)
    raise ValueError(l.kind)
