"""Exactly representable test data for the bf16 (and fp32) kernels, and a float64 reference of every layer operation.

The inputs built here make every product and every partial sum of a layer, in ANY order, exact in fp32: operands sit on
power-of-two grids and the sum of the absolute products of one output stays below 2^24 grid units. The folded-BN scale is
a power of two per channel and the shift a multiple of 2^-7, so fma(acc, scale, shift) is exact as well. A correct kernel's
output is then bf16_rne(clip(exact, 0, 6)) bit for bit, whatever its summation order, and a test compares with array_equal.

Contract (the oracle's): activations NHWC, depthwise filter [3][3][C] fp32, pointwise filter [Cout][Cin] (bf16 values),
conv1 filter [3][3][3][Cout] fp32, scale / shift fp32 per output channel (either may be NULL: 1 / 0), act 0 (none), 1 (ReLU) or
2 (ReLU6), every layer output rounded to bf16 (round to nearest even) in bf16 mode. All arithmetic here is float64 numpy.

Test infrastructure only (like int8_ref.py); not a conftest.
"""
from __future__ import annotations

import numpy as np

ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
ACTS = (ACT_NONE, ACT_RELU, ACT_RELU6)
PARAMS = ("both", "scale", "shift", "none")          # which of scale / shift a call gives; the other is NULL
COMBOS = [(a, p) for p in PARAMS for a in ACTS]      # the 12 epilogue combinations, the forms with a scale first
Z_SHARES = dict(neg=0.10, mid=0.20, high=0.02)       # the least shares of z < 0, 0 < z < 6, z > 6 an epilogue case must have
LIMIT = 2.0 ** 24              # fp32 holds every integer below it


# ----------------------------------------------------------------------------- bf16 on bits

def f32_bits(y):
    """float64 values that are exact in fp32 -> their fp32 bit patterns (uint32); anything inexact is a bug in the caller."""
    y = np.ascontiguousarray(y, np.float64)
    f = y.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), y), "value not representable in fp32"
    return f.view(np.uint32)


def bf16_rne_bits(y):
    """bf16 bit patterns (uint16) of y, round to nearest, ties to even, done on the fp32 bits."""
    u = f32_bits(y).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def bf16_rne(y):
    return bf16_value(bf16_rne_bits(y))


def bf16_truncate(y):
    """mutant: round toward zero"""
    return bf16_value((f32_bits(y) >> 16).astype(np.uint16))


def bf16_ties_away(y):
    """mutant: round to nearest, ties away from zero"""
    u = f32_bits(y).astype(np.uint64)
    return bf16_value(((u + 0x8000) >> 16).astype(np.uint16))


def relu6(y):
    return np.clip(y, 0.0, 6.0)


def coverage(y, act=ACT_RELU6, z=None):
    """Shares of a tensor that is about to be rounded to bf16 (y: exact values after the activation). z: the values before the activation;
    with them the shares below 0, strictly inside (0, 6) and above 6 — the regions in which no activation, ReLU and ReLU6 differ."""
    u = f32_bits(y)
    low, odd = u & 0xFFFF, (u >> 16) & 1
    tie = low == 0x8000
    cov = dict(n=int(y.size), act=act, inside=float(np.mean((y > 0) & (y < 6))), at0=float(np.mean(y == 0)), at6=float(np.mean(y == 6)),
               changed=float(np.mean(low != 0)), ties_up=int(np.sum(tie & (odd == 1))), ties_down=int(np.sum(tie & (odd == 0))))
    if z is not None:
        cov.update(neg=float(np.mean(z < 0)), mid=float(np.mean((z > 0) & (z < 6))), high=float(np.mean(z > 6)))
    return cov


def lsb_grid(a):
    """The operand grid of an array: the largest power of two that divides every element (1 for all zeros)."""
    q = np.abs(np.asarray(a, np.float64)).ravel() * 2.0 ** 40
    q = q[q != 0]
    if q.size == 0:
        return 1.0
    qi = q.astype(np.int64)
    assert np.array_equal(qi.astype(np.float64), q), "operand finer than 2^-40 or beyond 2^22"
    return float(np.min(qi & -qi)) * 2.0 ** -40


# ----------------------------------------------------------------------------- generators (all seeded by the caller's rng)

def gen_act(rng, shape, step=1.0 / 8, fine=False):
    """Activations in [0, 6]: a wider integer range clipped, so exact 0 and exact 6 occur. fine: multiples of 2^-7 rounded to bf16
    (the bare pointwise and depthwise kernels); otherwise multiples of `step` (1/8: 6 significant bits, exact in bf16)."""
    if fine:
        return bf16_rne(np.clip(rng.integers(-160, 930, shape), 0, 768) * 2.0 ** -7)
    hi = int(round(6 / step))
    return np.clip(rng.integers(-hi // 5, hi + hi // 6 + 1, shape), 0, hi) * step


def gen_image(rng, shape, steps=8):
    """Network input on a 1/8 grid in [-1, 1] (the image is fp32 in every mode, so a finer grid, 1/steps, stays exact as well)."""
    return rng.integers(-steps, steps + 1, shape) / float(steps)


def gen_dw_filter(rng, c, first=True, live=7):
    """fp32 integers differing per channel: {-2, -1, 1, 2} on all nine taps for a first layer; later in a chain {-1, 0, 1} with `live` non-zero
    taps per channel, at positions that differ from channel to channel (every tap is live in some channel)."""
    if first:
        return rng.choice([-2.0, -1.0, 1.0, 2.0], (3, 3, c))
    w = rng.choice([-1.0, 1.0], (9, c))
    keep = np.argsort(rng.random((9, c)), axis=0) < live
    return (w * keep).reshape(3, 3, c)


def gen_pw_filter(rng, cout, cin, density=1.0):
    """bf16 integers in {-2..2}; columns 0 and cin - 1 asymmetric over the output channels. density < 1: only that share of each row is non-zero,
    at positions that differ from row to row (all k are still covered across the channels)."""
    w = rng.integers(-2, 3, (cout, cin)).astype(np.float64)
    if density < 1.0:
        w[rng.random((cout, cin)) >= density] = 0.0
    w[:, 0] = np.arange(cout) % 3
    w[:, cin - 1] = (np.arange(cout) + 1) % 3 - 1
    return w


def gen_conv1_filter(rng, cout, density=1.0):
    w = rng.choice([-2.0, -1.0, 1.0, 2.0], (3, 3, 3, cout))
    if density < 1.0:
        w[rng.random(w.shape) >= density] = 0.0
    return w


def spread_exponent(acc, target=2.0):
    """e0 with std(acc) * 2^-e0 nearest `target`: the accumulator's spread, pooled over the channels"""
    c = acc.shape[-1]
    sd = max(float(np.sqrt(np.mean(np.var(acc.reshape(-1, c), axis=0)))), 2.0 ** -20)
    return int(np.round(np.log2(sd / target)))


def gen_scale_shift(rng, acc, lo, hi, target=2.0, spread=1, unit_scale=False):
    """Per-channel scale 2^-e[c], e[c] = e0 + {-spread..spread}, e0 from the accumulator's per-channel standard deviation so that acc * scale
    has one near `target`; shift: an odd multiple of 2^-7 that puts the channel's mean at a value drawn from [lo, hi] (a channel whose filter sums
    far from zero would otherwise sit wholly at one clamp). Adjacent channels differ in both. unit_scale: the same draws, but the scale is 1
    for every channel (a call with scale NULL) and the shift is the one that goes with that."""
    c = acc.shape[-1]
    a2 = acc.reshape(-1, c)
    e0 = spread_exponent(acc, target)
    e = e0 + rng.integers(-spread, spread + 1, c)
    e[1::2] = np.where(e[1::2] == e[0::2][:e[1::2].size], e[1::2] - 1, e[1::2])          # a channel pair never shares its scale
    scale = np.ones(c) if unit_scale else 2.0 ** -e.astype(np.float64)
    mu = lo + (hi - lo) * (rng.permutation(c) + rng.random(c)) / c            # stratified: a handful of channels still spans [lo, hi]
    shift = 2.0 * np.round((mu - a2.mean(axis=0) * scale) * 64.0) + 1.0      # odd: the 2^-7 bit reaches every element
    shift[1::2] = np.where(shift[1::2] == shift[0::2][:shift[1::2].size], shift[1::2] + 2, shift[1::2])
    return scale, shift * 2.0 ** -7


# ----------------------------------------------------------------------------- accumulators (float64), with the sum of absolute terms

def same_pad(size, out, k, stride):
    return max((out - 1) * stride + k - size, 0) // 2


def _windows(x, stride, pad_top, pad_left, out_rows, out_cols, dilation):
    n, h, w, c = x.shape
    hh = max(pad_top + h, (out_rows - 1) * stride + 2 * dilation + 1)
    ww = max(pad_left + w, (out_cols - 1) * stride + 2 * dilation + 1)
    xp = np.zeros((n, hh, ww, c), np.float64)
    xp[:, pad_top:pad_top + h, pad_left:pad_left + w] = x
    for i in range(3):
        for j in range(3):
            yield i, j, xp[:, i * dilation:i * dilation + (out_rows - 1) * stride + 1:stride, j * dilation:j * dilation + (out_cols - 1) * stride + 1:stride]


def dw_geom(h, w, stride, pad_top=-1, pad_left=-1, out_rows=0, out_cols=0, dilation=1):
    oh, ow = out_rows or -(-h // stride), out_cols or -(-w // stride)
    k = 2 * dilation + 1
    return oh, ow, (pad_top if pad_top >= 0 else same_pad(h, oh, k, stride)), (pad_left if pad_left >= 0 else same_pad(w, ow, k, stride))


def dw_acc(x, wd, stride=1, pad_top=-1, pad_left=-1, out_rows=0, out_cols=0, dilation=1, order=1, dtype=np.float64):
    """3x3 depthwise sums [N][oh][ow][C] and the sums of the absolute terms. order = -1 adds the taps last to first; dtype float32 evaluates in fp32."""
    oh, ow, pt, pl = dw_geom(x.shape[1], x.shape[2], stride, pad_top, pad_left, out_rows, out_cols, dilation)
    taps = list(_windows(np.asarray(x, np.float64), stride, pt, pl, oh, ow, dilation))[::order]
    acc = np.zeros((x.shape[0], oh, ow, x.shape[3]), dtype)
    mag = np.zeros(acc.shape, np.float64)
    for i, j, win in taps:
        t = win.astype(dtype) * wd[i, j].astype(dtype)
        acc = acc + t
        mag += np.abs(t)
    return acc, mag


def conv1_acc(x, w1, order=1, dtype=np.float64):
    """3x3x3 stride-2 convolution [N][H/2][W/2][Cout] with SAME padding (even sides: nothing on top / left, one row / column at the far side)."""
    n, h, w, _ = x.shape
    oh, ow = -(-h // 2), -(-w // 2)
    pt, pl = same_pad(h, oh, 3, 2), same_pad(w, ow, 3, 2)
    acc = np.zeros((n, oh, ow, w1.shape[3]), dtype)
    mag = np.zeros(acc.shape, np.float64)
    for i, j, win in list(_windows(np.asarray(x, np.float64), 2, pt, pl, oh, ow, 1))[::order]:
        for ch in range(3)[::order]:
            t = win[..., ch:ch + 1].astype(dtype) * w1[i, j, ch].astype(dtype)
            acc = acc + t
            mag += np.abs(t)
    return acc, mag


def pw_acc(x, wp):
    """x [..., Cin] @ wp[Cout][Cin]^T and the sums of the absolute terms."""
    x, wp = np.asarray(x, np.float64), np.asarray(wp, np.float64)
    return x @ wp.T, np.abs(x) @ np.abs(wp).T


def pw_acc_f32(x2d, wp, order=1):
    """The same sum evaluated in fp32, one k at a time, first to last (order 1) or last to first (-1)."""
    x2d, wp = x2d.astype(np.float32), wp.astype(np.float32)
    acc = np.zeros((x2d.shape[0], wp.shape[0]), np.float32)
    for k in range(x2d.shape[1])[::order]:
        acc += x2d[:, k:k + 1] * wp[None, :, k]
    return acc


def bn_act(acc, scale, shift, act):
    y = acc * (1.0 if scale is None else scale) + (0.0 if shift is None else shift)
    if act not in ACTS:
        raise ValueError(act)
    return relu6(y) if act == ACT_RELU6 else np.maximum(y, 0.0) if act == ACT_RELU else y


def pool_mean(x):
    """whole-map average [N][C]; exact when rows * cols is a power of two"""
    return x.reshape(x.shape[0], -1, x.shape[3]).sum(axis=1) / float(x.shape[1] * x.shape[2])


# ----------------------------------------------------------------------------- layers, chains, the gate

class Layer:
    """One evaluated layer: inputs, parameters, the exact result y (after the activation) and `out` = what the next layer reads."""

    def __init__(self, kind, x, w, scale, shift, act, acc, mag, rounded, geom=None, epilogue_case=False):
        self.kind, self.x, self.w, self.scale, self.shift, self.act, self.acc, self.mag, self.rounded = kind, x, w, scale, shift, act, acc, mag, rounded
        self.geom = geom or {}
        self.epilogue_case = epilogue_case        # a case of the epilogue matrix: check_gate asks for Z_SHARES of z
        self.z = bn_act(acc, scale, shift, ACT_NONE)
        self.y = bn_act(acc, scale, shift, act)
        self.out = bf16_rne(self.y) if rounded else self.y

    def figures(self):
        """The gate's figures of this layer: the operand grid, max sum|terms| in grid units, the epilogue's magnitude in units of its grid,
        and the coverage of the output tensor (its rounding shares count only where it is rounded: `rounded`)."""
        grid = lsb_grid(self.x) * lsb_grid(self.w)
        sc = np.ones(self.acc.shape[-1]) if self.scale is None else self.scale
        sh = np.zeros(self.acc.shape[-1]) if self.shift is None else self.shift
        unit = np.minimum(grid * sc, lsb_grid(sh) if np.any(sh) else np.inf)
        epi = np.max((self.mag.reshape(-1, self.acc.shape[-1]).max(axis=0) * sc + np.abs(sh)) / unit)
        return dict(kind=self.kind, grid=grid, terms=float(self.mag.max() / grid), epilogue=float(epi),
                    rounded=self.rounded, coverage=coverage(self.y, self.act, self.z))


def make_layer(rng, kind, x, w, act=ACT_RELU6, rounded=True, shift_range=None, scale=True, target=2.0, spread=1, params=None, **geom):
    """params None: scale and shift given (scale False: the FC form), as every case before the epilogue matrix. params in PARAMS: a case of that
    matrix. "both" makes the same draws as None. With scale NULL ("shift", "none") the raw accumulator would lie far outside [0, 6]: the input is
    shrunk by the power of two that brings the accumulator's standard deviation s into [1.5, 3) x `target` (the operands stay bf16 values,
    sum|terms| in grid units does not change), and the shift centres the channels as it does behind a scale. That interval, [3, 6) at the default
    target: no per-channel scale spreads the channels here, and a channel centred on 0 (conv1: a zero-mean image) has P(z > 6) = 1 - Phi(6 / s),
    2.3 % at s = 3, and P(0 < z < 6) = Phi(6 / s) - 1 / 2, 34 % at s = 6. With shift NULL ("scale", "none") nothing centres a channel: z is what
    the filter gives. x and w do not depend on act or params beyond that power of two, so one upload serves a whole matrix."""
    if params is not None and (params not in PARAMS or not scale):
        raise ValueError(params)
    if kind == "dw":
        acc, mag = dw_acc(x, w, **geom)
        rng_sh = shift_range or (-1, 4)
    elif kind == "pw":
        acc, mag = pw_acc(x, w)
        rng_sh = shift_range or (-2, 6)
    elif kind == "conv1":
        acc, mag = conv1_acc(x, w)
        rng_sh = shift_range or (-1, 4)
    else:
        raise ValueError(kind)
    if params in ("shift", "none"):
        down = 2.0 ** -spread_exponent(acc, 1.5 * target * 2.0 ** 0.5)              # nearest to 1.5 sqrt(2) t in log2: s * down in [1.5 t, 3 t)
        x, acc, mag = x * down, acc * down, mag * down
    sc, sh = gen_scale_shift(rng, acc, *rng_sh, target=target, spread=spread, unit_scale=params in ("shift", "none"))
    if not scale:                                        # the FC form: integer bias, nothing to centre
        sh = rng.integers(rng_sh[0], rng_sh[1] + 1, acc.shape[-1]).astype(np.float64)
    if not scale or params in ("shift", "none"):
        sc = None
    if params in ("scale", "none"):
        sh = None
    return Layer(kind, x, w, sc, sh, act, acc, mag, rounded, geom, epilogue_case=params is not None)


def pool_layer(x, rounded=True):
    """whole-map average as a layer: the sum over the pixels, scale 1 / pixels (a power of two in every exact case), no activation"""
    n, h, w, c = x.shape
    flat = np.asarray(x, np.float64).reshape(n, h * w, c)
    return Layer("pool", x, np.ones(1), np.full(c, 1.0 / (h * w)), None, ACT_NONE, flat.sum(axis=1), np.abs(flat).sum(axis=1), rounded)


def gate(layers):
    return [l.figures() for l in layers]


def check_gate(layers, what=""):
    """The conditions every generated case must meet (conditions on the inputs, not measurements). Returns the figures."""
    figs = gate(layers)
    for i, (l, f) in enumerate(zip(layers, figs)):
        tag = "%s layer %d (%s)" % (what, i, l.kind)
        assert f["terms"] < LIMIT, "%s: sum|terms| = 2^%.1f grid units" % (tag, np.log2(f["terms"]))
        assert f["epilogue"] < LIMIT, "%s: |acc * scale| + |shift| = 2^%.1f units" % (tag, np.log2(f["epilogue"]))
        cov = f["coverage"]
        if l.rounded:                # an fp32 output is stored as it is: nothing to round
            ties = 16 if cov["n"] >= 4096 else 2
            assert cov["changed"] >= 0.20, "%s: %s" % (tag, cov)
            assert cov["ties_up"] >= ties and cov["ties_down"] >= ties, "%s: %s" % (tag, cov)
        if l.act == ACT_RELU6 and not (l.epilogue_case and (l.scale is None or l.shift is None)):
            # rounded or not (the fp32 epilogues clamp too); the clamp shares mean nothing without a clamp, and they are what a per-channel scale
            # and a centring shift give: an epilogue case with one of them NULL has Z_SHARES alone
            assert cov["inside"] >= 0.40 and cov["at0"] >= 0.10 and cov["at6"] >= 0.02, "%s: %s" % (tag, cov)
        if l.epilogue_case:          # every act: elements below 0, inside (0, 6) and above 6 tell none / ReLU / ReLU6 apart
            assert l.act in ACTS
            assert all(cov[k] >= v for k, v in Z_SHARES.items()), "%s: %s" % (tag, cov)
    return figs


def fp32_orders_agree(l, work=4.0e8, rows=2048):
    """acc * scale + shift of layer l evaluated in fp32 in two opposite summation orders equals the float64 value bit for bit. Every
    element of every layer, except a pointwise layer of more than `work` products: there the first and last rows and `rows` seeded ones
    spread over the matrix (the one-k-at-a-time fp32 sum is slow in numpy; the sum|terms| bound is the proof for all of them)."""
    if l.kind == "pw":
        x2 = l.x.reshape(-1, l.x.shape[-1])
        m = x2.shape[0]
        sel = np.arange(m)
        if float(m) * x2.shape[1] * l.w.shape[0] > work:
            sel = np.unique(np.concatenate([np.arange(256), np.arange(m - 256, m), np.random.default_rng(m).integers(0, m, rows)]))
        accs = [pw_acc_f32(x2[sel], l.w, o) for o in (1, -1)]
        want = l.acc.reshape(-1, l.acc.shape[-1])[sel]
    elif l.kind == "dw":
        accs = [dw_acc(l.x, l.w, order=o, dtype=np.float32, **l.geom)[0] for o in (1, -1)]
        want = l.acc
    elif l.kind == "pool":
        flat = l.x.reshape(l.x.shape[0], -1, l.x.shape[3]).astype(np.float32)
        accs = []
        for o in (1, -1):
            a = np.zeros(l.acc.shape, np.float32)
            for px in range(flat.shape[1])[::o]:
                a += flat[:, px]
            accs.append(a)
        want = l.acc
    else:
        accs = [conv1_acc(l.x, l.w, order=o, dtype=np.float32)[0] for o in (1, -1)]
        want = l.acc
    sc = np.float32(1) if l.scale is None else l.scale.astype(np.float32)
    sh = np.float32(0) if l.shift is None else l.shift.astype(np.float32)
    y64 = want * (1.0 if l.scale is None else l.scale) + (0.0 if l.shift is None else l.shift)
    for a in accs:
        assert a.dtype == np.float32
        y32 = a * sc + sh                     # two roundings where the kernels' fma has one: both exact here
        if not (np.array_equal(a.astype(np.float64), want) and np.array_equal(y32.astype(np.float64), y64)):
            return False
    return True


# ----------------------------------------------------------------------------- cases (what the GPU tests run; the CPU tests gate them)

def pw_case(m, k, n, act=ACT_RELU6, rounded=True, fc=False, seed=0, params=None):
    """One pointwise layer. fc: the FC form (scale NULL, shift given, act 0, fp32 out: nothing is rounded). params: see make_layer."""
    rng = np.random.default_rng([1, m, k, n, seed])
    x = gen_act(rng, (m, k), fine=True)
    w = gen_pw_filter(rng, n, k)
    if fc:
        return [make_layer(rng, "pw", x, w, act=ACT_NONE, rounded=False, scale=False, shift_range=(-50, 50))]
    return [make_layer(rng, "pw", x, w, act=act, rounded=rounded, params=params)]


def dw_case(n, h, c, stride, w=None, rounded=True, seed=0, act=ACT_RELU6, params=None, target=2.0, **geom):
    """(the seed of a case is the last thing to change when it misses a share of the gate: the conditions stay)"""
    rng = np.random.default_rng([2, n, h, c, stride, seed] + sorted(geom.values()))
    x = gen_act(rng, (n, h, w or h, c), fine=True)
    return [make_layer(rng, "dw", x, gen_dw_filter(rng, c), act=act, rounded=rounded, params=params, target=target, stride=stride, **geom)]


def pool_case(n, h, c, seed=0):
    rng = np.random.default_rng([3, n, h, c, seed])
    return gen_act(rng, (n, h, h, c), fine=True)


def block_case(n, h, w, cin, cout, stride, rounded=True, seed=0, first=True, x=None, density=1.0, live=7, spread=1, **geom):
    """depthwise + pointwise pair; both outputs rounded to bf16 unless rounded is False (the fp32 kernels)."""
    rng = np.random.default_rng([4, n, h, w, cin, cout, stride, seed] + sorted(geom.values()))
    if x is None:
        x = gen_act(rng, (n, h, w, cin), step=1.0 / 16)
    d = make_layer(rng, "dw", x, gen_dw_filter(rng, cin, first, live), rounded=rounded, stride=stride, spread=spread, **geom)
    p = make_layer(rng, "pw", d.out, gen_pw_filter(rng, cout, cin, density), rounded=rounded, spread=spread)
    return [d, p]


def chain_case(n, h, w, chans, strides, seed=0, images=None, first_density=1.0, density=0.25, live=7, spread=1, pool=False):
    """A run of blocks: chans = [c0, c1, ...] (block i: c[i] -> c[i + 1]), strides per block; later blocks take depthwise taps in {-1, 0, 1}
    and a pointwise filter about 25 % dense. images: build that many distinct images and tile them up to n."""
    rng = np.random.default_rng([5, n, h, w, seed] + list(chans) + list(strides))
    x = gen_act(rng, (images or n, h, w, chans[0]), step=1.0 / 16)
    layers = []
    for i, s in enumerate(strides):
        geom = dict(pad_top=0, pad_left=0, out_rows=x.shape[1] // 2, out_cols=x.shape[2] // 2) if s == 2 else dict(pad_top=1, pad_left=1)
        layers += block_case(x.shape[0], x.shape[1], x.shape[2], chans[i], chans[i + 1], s, seed=seed + 17 * i, first=(i == 0), x=x,
                             density=first_density if i == 0 else density, live=live, spread=spread, **geom)
        x = layers[-1].out
    if pool:
        layers.append(pool_layer(x))
    return layers


def stem_case(n, rows, cols, c1, c3, density=1.0, seed=0, rounded=True):
    """conv1 3x3x3 stride 2 -> depthwise stride 1 -> pointwise, every output rounded to bf16 (the bf16 fused stem), or none (rounded False: the fp32 one)."""
    rng = np.random.default_rng([6, n, rows, cols, c1, c3, seed])
    img = gen_image(rng, (n, rows, cols, 3))
    a = make_layer(rng, "conv1", img, gen_conv1_filter(rng, c1, density), rounded=rounded)
    d = make_layer(rng, "dw", a.out, gen_dw_filter(rng, c1, first=False), rounded=rounded, stride=1, pad_top=1, pad_left=1)
    p = make_layer(rng, "pw", d.out, gen_pw_filter(rng, c3, c1), rounded=rounded)
    return [a, d, p]


def conv1_case(n, rows, cols, cout, seed=0, act=ACT_RELU6, params=None, rounded=False):
    """params given (the epilogue matrix): the image on a 1/256 grid. With shift NULL no 2^-7 bit reaches the output, and sums of a 1/8-grid image
    times an integer filter have too few significant bits for a bf16 rounding to change any."""
    rng = np.random.default_rng([7, n, rows, cols, cout, seed])
    img = gen_image(rng, (n, rows, cols, 3), 8 if params is None else 256)
    return [make_layer(rng, "conv1", img, gen_conv1_filter(rng, cout), act=act, rounded=rounded, params=params)]


def inflate(wd, d):
    """3x3 filter at dilation d as the (2d+1)^2 filter with zeros between the taps (what an undilated reference takes)."""
    f = np.zeros((2 * d + 1, 2 * d + 1, wd.shape[2]), wd.dtype)
    f[::d, ::d] = wd
    return f
