"""Segment through the letterbox on the host (no GPU): the window rule of mbn_resample_argmax_window_f32 (tests/dense_window_ref.py, the
reference of the GPU tests). The three facts the kernel rests on: the full window is dense_any_ref's rule bit for bit, a window on the grid of a
full resample is a crop of it bit for bit, and the tile bounds carry over with n / N replaced by l n / (N R). The reference against torch's
grid_sample on float64 inputs at the sample points b + (o + 1/2) l / N, on the weight rule's chosen coordinates; the envelope, the plan and the
ragged window check through libmbn_host.so; the new symbols where they belong."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dense_any_ref
import dense_window_ref
from test_dense_cpu import logits_for


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_axis(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got[:2], want[:2])) and \
        all(g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w)) for g, w in zip(got[2:], want[2:]))


# ------------------------------------------------------------------------------------------------------------------ the three facts

def test_fact_1_full_window_is_the_existing_rule():
    """b = 0, l = R: num and den are R times dense_any_ref's, the same rational from exact float64 operands. 3000 random (n, S, N)."""
    rng = np.random.default_rng(1)
    for _ in range(3000):
        n = int(rng.integers(1, 65))
        R = n * int(rng.integers(1, 65))                   # R / n an integer here; the next test's R need not be
        if rng.integers(0, 4) == 0:
            R = int(rng.integers(n, 16385))
        N = int(rng.integers(4 * n, min(16384, 40 * n) + 1))
        assert _same_axis(dense_window_ref.axis_window(N, n, R, 0, R), dense_any_ref.axis(N, n)), (n, R, N)
    x = logits_for((2, 5, 7, 21, 0), seed=3)
    lab, sc = dense_window_ref.resample_argmax_window(x, 160, 224, (0, 0, 224, 160), 37, 61)
    want_lab, want_sc = dense_any_ref.resample_argmax(x, 37, 61)
    assert np.array_equal(lab, want_lab) and np.array_equal(_bits(sc), _bits(want_sc))


# (n, S, l, N, b): R = n * S; M = R * N / l and off = b * N / l are integers
CROP_CASES = [(2, 32, 32, 48, 16), (7, 32, 168, 336, 28), (7, 32, 112, 300, 56), (5, 8, 20, 60, 10), (14, 16, 168, 336, 28)]


@pytest.mark.parametrize("case", CROP_CASES)
def test_fact_2_window_on_the_grid_is_a_crop(case):
    n, S, l, N, b = case
    R = n * S
    assert (R * N) % l == 0 and (b * N) % l == 0
    M, off = R * N // l, b * N // l
    full = dense_any_ref.axis(M, n)
    assert _same_axis(dense_window_ref.axis_window(N, n, R, b, l), tuple(a[off:off + N] for a in full)), case
    # and the read-out of both axes at once
    x = logits_for((1, n, n, 21, 0), seed=n + S)
    lab, sc = dense_window_ref.resample_argmax_window(x, R, R, (b, b, l, l), N, N)
    want_lab, want_sc = dense_any_ref.resample_argmax(x, M, M)
    assert np.array_equal(lab[0], want_lab[0, off:off + N, off:off + N])
    assert np.array_equal(_bits(sc[0]), _bits(want_sc[0, off:off + N, off:off + N]))


def _random_geometry(rng):
    """(n, R, b, l, N) inside the envelope: N R >= 4 l n, sides at most 16384"""
    while True:
        n = int(rng.integers(1, 40))
        R = int(rng.integers(n, min(40 * n, 16384) + 1))
        l = int(rng.integers(1, R + 1))
        b = int(rng.integers(0, R - l + 1))
        lo = -(-4 * l * n // R)                             # the smallest N with N R >= 4 l n
        lo = max(lo, 1)
        if lo > 16384:
            continue
        N = lo if rng.integers(0, 3) == 0 else int(rng.integers(lo, min(16384, 8 * lo + 40) + 1))
        return n, R, b, l, N


def test_fact_3_tile_bounds_carry_over():
    """Under N R >= 4 l n any 32 aligned outputs touch at most min(n, floor(31 l n / (N R)) + 3) coarse samples (at most 10) and four aligned
    outputs have i0 in {ya, ya + 1}: what the kernel's LDS footprint and its three-row reduce rest on."""
    rng = np.random.default_rng(2)
    worst = 0
    for _ in range(4000):
        n, R, b, l, N = _random_geometry(rng)
        i0, i1, _, _ = dense_window_ref.axis_window(N, n, R, b, l)
        assert i0.min() >= 0 and i1.max() <= n - 1 and i0.max() <= n - 1
        bound = min(n, 31 * l * n // (N * R) + 3)
        assert bound <= 10
        starts = np.arange(0, N, 32)
        ends = np.minimum(starts + 32, N) - 1
        foot = np.maximum.reduceat(i1, starts) - i0[starts] + 1
        assert (i1[ends] == np.maximum.reduceat(i1, starts)).all()          # monotone
        assert (foot <= bound).all(), (n, R, b, l, N)
        worst = max(worst, int(foot.max()))
        s4 = np.arange(0, N, 4)
        assert (np.maximum.reduceat(i0, s4) - i0[s4] <= 1).all(), (n, R, b, l, N)
    assert worst <= 10


# -------------------------------------------------------------------------------------------------------------------------- torch

# (h, w, stride, H, W, classes): the map of a (h * stride) x (w * stride) input, the source H x W letterboxed into it
TORCH_SHAPES = [(7, 7, 32, 375, 500, 21), (7, 7, 32, 500, 375, 21), (2, 3, 32, 33, 100, 21), (4, 4, 8, 40, 17, 65), (7, 10, 32, 300, 300, 21),
                (14, 14, 16, 96, 640, 33)]


def torch_compare_window(x, R, Cc, rect, H, W, labels, score, what=""):
    """labels / score [n][H][W] against torch.nn.functional.grid_sample(x.double(), bilinear, padding_mode="border", align_corners=False) at the
    sample points b + (o + 1/2) l / N of the input, which do not go through the integer rule. The yardstick of
    test_dense_any_cpu.torch_compare: scores within dense_any_ref.tolerance(x), labels equal wherever torch's top-two margin exceeds twice that,
    at most 1 % of the pixels that close."""
    import torch
    n, h, w, classes = x.shape
    rx, ry, iw, ih = rect
    t = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2).double()
    py = ry + (torch.arange(H, dtype=torch.float64) + 0.5) * ih / H           # input coordinates, pixel edges at integers
    px = rx + (torch.arange(W, dtype=torch.float64) + 0.5) * iw / W
    gy, gx = 2.0 * py / R - 1.0, 2.0 * px / Cc - 1.0                          # align_corners=False: -1 .. 1 spans the R (C) input pixels
    grid = torch.stack([gx[None, :].expand(H, W), gy[:, None].expand(H, W)], dim=-1)[None].expand(n, H, W, 2)
    up = torch.nn.functional.grid_sample(t, grid, mode="bilinear", padding_mode="border", align_corners=False)
    top = torch.topk(up, min(2, classes), dim=1)
    t_score, t_label = top.values[:, 0].numpy(), top.indices[:, 0].numpy()
    margin = (top.values[:, 0] - top.values[:, 1]).numpy() if classes > 1 else np.full(t_score.shape, np.inf)
    tol = dense_any_ref.tolerance(x)
    err = float(np.abs(score.astype(np.float64) - t_score).max())
    decided = margin > 2 * tol
    excluded = 1.0 - float(decided.mean())
    mismatches = int((labels[decided] != t_label[decided]).sum())
    print("%s %s window %s -> %dx%d: max score diff %.3e = %.2f of the bound %.3e, excluded %.4f %%, label mismatches %d"
          % (what, x.shape, rect, H, W, err, err / tol, tol, 100 * excluded, mismatches))
    assert err <= tol, (what, err, tol)
    assert excluded <= 0.01, (what, excluded)
    assert mismatches == 0, (what, mismatches)
    return err, tol, excluded, mismatches


@pytest.mark.parametrize("shape", TORCH_SHAPES)
def test_ref_vs_torch_grid_sample_float64(pkg, shape):
    h, w, stride, H, W, classes = shape
    R, Cc = h * stride, w * stride
    rect = pkg.fit_pad(H, W, R, Cc)
    assert pkg.resample_window_envelope(1, h, w, classes, R, Cc, rect, H, W) == pkg.OK
    x = logits_for((1, h, w, classes, 0))
    labels, score = dense_window_ref.resample_argmax_window(x, R, Cc, rect, H, W)
    assert labels.shape == score.shape == (1, H, W) and labels.dtype == np.int32 and score.dtype == np.float32
    torch_compare_window(x, R, Cc, tuple(rect), H, W, labels, score, "dense_window_ref")


# ----------------------------------------------------------------------------------------------------------------- the weight rule

def test_weight_rule_at_chosen_coordinates():
    f32, f64 = np.float32, np.float64
    # n = 7 over R = 224 (stride 32), worked by hand. b = 0, l = 168 -> N = 336: o = 0 has num = max(1176 - 75264, 0) = 0, clamped
    i0, i1, w0, w1 = dense_window_ref.axis_window(336, 7, 224, 0, 168)
    assert (i0[0], i1[0], w1[0], w0[0]) == (0, 1, 0.0, 1.0)
    # b = 56, l = 112 -> N = 300: o = 0 sits at input 56 + 56 / 300 = 56.18667, map coordinate 1.25583: i0 = 1 at the first output.
    # num = 784 + 235200 - 67200 = 168784, den = 134400, remainder 34384
    i0, i1, w0, w1 = dense_window_ref.axis_window(300, 7, 224, 56, 112)
    assert (i0[0], i1[0]) == (1, 2) and w1[0] == f32(f64(34384) / f64(134400)) and w0[0] == f32(1.0) - w1[0]
    # b = 56, l = 168 -> N = 336, b + l = R: the last output sits at 223.75, map coordinate 6.4922: i1 clamps to the last sample.
    # num = 671 * 1176 + 263424 - 75264 = 977256, den = 150528, i0 = 6, remainder 74088
    i0, i1, w0, w1 = dense_window_ref.axis_window(336, 7, 224, 56, 168)
    assert (i0[335], i1[335]) == (6, 6) and w1[335] == f32(f64(74088) / f64(150528))
    # b = 28, l = 168 -> N = 336, b + l = 196 < R: the last output sits at 195.75, map coordinate 5.6172: no clamp, i1 = 6 lies OUTSIDE the
    # window's own samples and still takes its weight. num = 789096 + 131712 - 75264 = 845544, i0 = 5, remainder 92904
    i0, i1, w0, w1 = dense_window_ref.axis_window(336, 7, 224, 28, 168)
    assert (i0[335], i1[335]) == (5, 6) and w1[335] == f32(f64(92904) / f64(150528)) and w1[335] > 0.5
    # ... and its first output, at 28.25, map coordinate 0.3828, interpolates with sample 0, whose centre (16) lies in front of the window
    assert (i0[0], i1[0]) == (0, 1) and w1[0] == f32(f64(2 * 28 * 7 * 336 + 1176 - 75264) / f64(150528))
    # a 1-pixel window to many outputs: every output within one input pixel
    i0, i1, w0, w1 = dense_window_ref.axis_window(40, 5, 160, 77, 1)
    assert (i0 == 1).all() and (i1 == 2).all() and (np.diff(w1) > 0).all()
    assert w1.dtype == np.float32 and w0.dtype == np.float32 and i0.dtype == np.int64


# ----------------------------------------------------------------------------------------------------------------------- envelope

def _env(pkg, *a):
    return pkg.resample_window_envelope(*a)


def test_window_envelope_accepts(pkg):
    # (batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols)
    for a in [(1, 7, 7, 21, 224, 224, (28, 0, 168, 224), 500, 375), (32, 28, 28, 1000, 224, 224, (0, 28, 224, 168), 375, 500),
              (1, 1, 1, 1, 1, 1, (0, 0, 1, 1), 4, 4), (65535, 2, 3, 21, 64, 96, (0, 0, 96, 64), 8, 12),
              (1, 5, 7, 21, 160, 224, (100, 3, 1, 1), 1, 1),                 # a window of one pixel: any output size has the ratio
              (1, 7, 10, 21, 223, 321, (5, 6, 300, 200), 300, 300),          # R / n not an integer
              (1, 512, 512, 21, 16384, 16384, (0, 0, 16384, 16384), 16384, 16384)]:
        assert _env(pkg, *a) == pkg.OK, a


def test_window_envelope_bad_arguments(pkg):
    E = pkg.EINVAL
    ok = [1, 5, 7, 21, 160, 224, (8, 4, 100, 90), 200, 300]
    assert _env(pkg, *ok) == pkg.OK
    for i in (0, 1, 2, 3, 4, 5, 7, 8):                      # every size: zero and negative
        for v in (0, -1):
            a = list(ok)
            a[i] = v
            assert _env(pkg, *a) == E, a
    for rect in [(-1, 4, 100, 90), (8, -1, 100, 90), (8, 4, 0, 90), (8, 4, 100, 0), (8, 4, -3, 90)]:
        assert _env(pkg, 1, 5, 7, 21, 160, 224, rect, 200, 300) == E, rect
    assert _env(pkg, 1, 5, 7, 21, 160, 224, None, 200, 300) == E
    # the far edges: flush is inside, one past is not
    assert _env(pkg, 1, 5, 7, 21, 160, 224, (124, 70, 100, 90), 200, 300) == pkg.OK
    assert _env(pkg, 1, 5, 7, 21, 160, 224, (125, 70, 100, 90), 200, 300) == E
    assert _env(pkg, 1, 5, 7, 21, 160, 224, (124, 71, 100, 90), 200, 300) == E
    assert _env(pkg, 1, 5, 7, 21, 160, 224, (2 ** 31 - 1, 0, 2 ** 31 - 1, 90), 200, 300) == E     # x + iw does not wrap
    # the input no smaller than the map
    assert _env(pkg, 1, 5, 7, 21, 5, 7, (0, 0, 1, 1), 4, 4) == pkg.OK
    assert _env(pkg, 1, 5, 7, 21, 4, 7, (0, 0, 1, 1), 4, 4) == E
    assert _env(pkg, 1, 5, 7, 21, 5, 6, (0, 0, 1, 1), 4, 4) == E


def test_window_envelope_limits(pkg):
    U = pkg.EUNSUPPORTED
    # the ratio N R >= 4 l n: equal, and one output less, on each axis. rows: 5 samples over 160, ih = 80 -> N * 160 >= 1600: N = 10
    assert _env(pkg, 1, 5, 7, 21, 160, 224, (0, 0, 112, 80), 10, 14) == pkg.OK
    assert _env(pkg, 1, 5, 7, 21, 160, 224, (0, 0, 112, 80), 9, 14) == U
    assert _env(pkg, 1, 5, 7, 21, 160, 224, (0, 0, 112, 80), 10, 13) == U
    # an equality that only the 64-bit products see: R = 16384, n = 4096, l = 16384 -> N >= 16384
    assert _env(pkg, 1, 4096, 1, 2, 16384, 4, (0, 0, 4, 16384), 16384, 4) == pkg.OK
    assert _env(pkg, 1, 4096, 1, 2, 16384, 4, (0, 0, 4, 16384), 16383, 4) == U
    # the sides: outputs and inputs at most 16384
    assert _env(pkg, 1, 1, 1, 21, 16384, 16384, (0, 0, 16384, 16384), 16384, 16384) == pkg.OK
    assert _env(pkg, 1, 1, 1, 21, 16384, 16384, (0, 0, 1, 1), 16385, 4) == U
    assert _env(pkg, 1, 1, 1, 21, 16384, 16384, (0, 0, 1, 1), 4, 16385) == U
    assert _env(pkg, 1, 1, 1, 21, 16385, 16384, (0, 0, 1, 1), 4, 4) == U
    assert _env(pkg, 1, 1, 1, 21, 16384, 16385, (0, 0, 1, 1), 4, 4) == U
    # an image's logits below 2^31 bytes; the batch is grid.y
    assert _env(pkg, 1, 1, 1, 2 ** 29 - 1, 32, 32, (0, 0, 32, 32), 4, 4) == pkg.OK
    assert _env(pkg, 1, 1, 1, 2 ** 29, 32, 32, (0, 0, 32, 32), 4, 4) == U
    assert _env(pkg, 65535, 2, 2, 21, 64, 64, (3, 3, 40, 40), 11, 9) == pkg.OK
    assert _env(pkg, 65536, 2, 2, 21, 64, 64, (3, 3, 40, 40), 11, 9) == U


def _fields(l):
    return (l.fy, l.fx, l.ch, l.lds_bytes, l.tiles, l.span)


def test_window_plan(pkg):
    """The full window gives mbn_resample_plan's answer field for field; a letterbox window's larger ratio shrinks the footprint."""
    rng = np.random.default_rng(5)
    cases = [(28, 28, 224, 224), (5, 7, 20, 28), (14, 20, 56, 80), (14, 14, 375, 500), (1, 1, 70, 45), (7, 7, 30, 28)]
    for _ in range(200):
        h, w = int(rng.integers(1, 30)), int(rng.integers(1, 30))
        cases.append((h, w, int(rng.integers(4 * h, 40 * h)), int(rng.integers(4 * w, 40 * w))))
    for h, w, H, W in cases:
        for s in (1, 8, 32):
            R, Cc = h * s + (s > 1) * 3, w * s                               # R / n not always an integer
            assert _fields(pkg.resample_window_plan(h, w, R, Cc, (0, 0, Cc, R), H, W)) == _fields(pkg.resample_plan(h, w, H, W)), (h, w, H, W, s)
    # the minimum ratio inside a window: 5 x 7 samples' worth of input to 20 x 28 outputs, footprint min(n, 31 / 4 + 3 = 10)
    l = pkg.resample_window_plan(10, 14, 320, 448, (224, 160, 224, 160), 20, 28)
    assert (l.fy, l.fx, l.ch, l.lds_bytes, l.tiles, l.span) == (10, 10, 64, 100 * 68 * 4, 1, 560)
    # 375 x 500 through the letterbox of 224 x 224: rows 168 of 224 -> 31 * 168 * 28 / (375 * 224) = 1 -> 4; the stretch has 31 * 28 / 375 = 2 -> 5
    rect = pkg.fit_pad(375, 500, 224, 224)
    assert tuple(rect) == (0, 28, 224, 168)
    l = pkg.resample_window_plan(28, 28, 224, 224, rect, 375, 500)
    assert (l.fy, l.fx, l.ch, l.tiles) == (4, 4, 128, 12 * 16) and (pkg.resample_plan(28, 28, 375, 500).fy, pkg.resample_plan(28, 28, 375, 500).fx) == (5, 4)
    # it widens, as mbn_resample_plan does
    pkg.host_lib().mbn_resample_window_plan(28, 28, 224, 224, (C.c_int32 * 4)(0, 0, 224, 224), 112, 112, C.byref(l))
    assert (l.fy, l.fx, l.ch, l.tiles, l.span) == (10, 10, 64, 12 * 16, 375 * 500)


def test_ragged_window_check(pkg):
    h, w, classes, R, Cc = 5, 7, 21, 160, 224
    full = (0, 0, Cc, R)
    ok = [(0, 37, 61, full), (5000, 40, 56, (56, 0, 112, 160)), (2257 + 10, 20, 28, (32, 16, 160, 128))]
    rc, l = pkg.resample_ragged_window_check(h, w, classes, R, Cc, ok)
    assert rc == pkg.OK and l.span == 5000 + 40 * 56 and l.tiles == 4 and (l.fy, l.fx) == (5, 7)
    two = lambda a, b: pkg.resample_ragged_window_check(h, w, classes, R, Cc, [a, b])[0]
    assert two((0, 37, 61, full), (2257, 20, 28, full)) == pkg.OK                           # touching is not overlapping
    assert two((2256, 20, 28, full), (0, 37, 61, full)) == pkg.EINVAL                       # one element shared, any order
    assert two((0, 37, 61, full), (0, 37, 61, full)) == pkg.EINVAL
    assert two((-1, 37, 61, full), (9000, 37, 61, full)) == pkg.EINVAL
    assert two((0, 37, 61, full), (5000, 0, 61, full)) == pkg.EINVAL
    assert two((0, 37, 61, full), (5000, 37, 61, (0, 0, Cc + 1, R))) == pkg.EINVAL          # a rectangle past the input
    assert two((0, 37, 61, full), (5000, 37, 61, (1, 0, Cc, R))) == pkg.EINVAL
    assert two((0, 37, 61, full), (5000, 19, 28, full)) == pkg.EUNSUPPORTED                 # under ratio 4 for the full window ...
    assert two((0, 37, 61, full), (5000, 19, 28, (0, 0, Cc, 152))) == pkg.OK                # ... inside it for a shorter one: 19 * 160 = 4 * 152 * 5
    assert two((0, 37, 61, full), (5000, 19, 28, (0, 0, Cc, 153))) == pkg.EUNSUPPORTED
    assert two((0, 37, 61, full), (5000, 20, 16385, full)) == pkg.EUNSUPPORTED
    # a refused batch leaves the launch record as it was
    rec = pkg.ResampleLaunch()
    rec.fy, rec.fx, rec.ch, rec.lds_bytes, rec.tiles, rec.span = 91, 92, 93, 94, 95, 96
    for items in ([(0, 37, 61, full), (2256, 20, 28, full)], [(0, 37, 61, full), (5000, 19, 28, full)], [(0, 37, 61, full), (5000, 37, 61, (0, 0, 0, R))]):
        rc, _ = pkg.resample_ragged_window_check(h, w, classes, R, Cc, items, launch=rec)
        assert rc != pkg.OK and _fields(rec) == (91, 92, 93, 94, 95, 96)
    rc, _ = pkg.resample_ragged_window_check(h, w, classes, R, Cc, ok, launch=rec)
    assert rc == pkg.OK and _fields(rec) == _fields(l)


# ------------------------------------------------------------------------------------------- the whole map is the full window

def _edge_geometry(rng):
    """(batch, rows, cols, classes, H, W): inside the envelope of mbn_resample_argmax_f32 unless `edge` pushes one argument onto or over a limit"""
    rows, cols = int(rng.integers(1, 48)), int(rng.integers(1, 48))
    H, W = int(rng.integers(4 * rows, 12 * rows + 1)), int(rng.integers(4 * cols, 12 * cols + 1))
    batch, classes = int(rng.integers(1, 65)), int(rng.integers(1, 1001))
    edge = int(rng.integers(0, 40))                          # 20 and above: none
    zero = int(rng.integers(-1, 1))                          # 0 or -1
    if edge == 0: rows = zero
    elif edge == 1: cols = zero
    elif edge == 2: H = zero
    elif edge == 3: W = zero
    elif edge == 4: classes = zero
    elif edge == 5: batch = zero
    elif edge == 6: H = 16385
    elif edge == 7: W = 16385
    elif edge == 8: H = W = 16384
    elif edge == 9: H = 4 * rows - 1                         # the ratio just under 4
    elif edge == 10: W = 4 * cols - 1
    elif edge == 11: H, W = 4 * rows, 4 * cols               # and exactly 4
    elif edge == 12: batch = 65536
    elif edge == 13: batch = 65535
    elif edge == 14: classes = -(-2 ** 29 // (rows * cols))  # the first class count at which an image's logits reach 2^31 bytes
    elif edge == 15: classes = -(-2 ** 29 // (rows * cols)) - 1
    elif edge == 16: rows, H = 16385, 16384                  # a map no output can be four times of
    elif edge == 17: rows, H = 4096, 16384
    elif edge == 18: rows, H = 4097, 16384
    elif edge == 19: cols, W, rows, H = 4096, 16384, 4096, 16384
    return batch, rows, cols, classes, H, W


def _multiple(rng, rows, cols):
    """1, or m >= 2 with m * rows and m * cols at most 16384 where there is one"""
    top = 16384 // max(rows, cols, 1)
    return int(rng.integers(2, top + 1)) if top >= 2 and rng.integers(0, 4) else 1


def test_whole_map_is_the_full_window(pkg):
    """What lets host/mbn_envelope.c keep ONE geometry: the plain envelope, plan and ragged check are the window ones given the rectangle
    (0, 0, in_cols, in_rows), for in = (rows, cols) and for a multiple of it: the same status for every argument, refusals included, and where both
    accept the same mbn_resample_launch_t field for field. A fixed-seed sweep that sits on the limits (sides 0, -1, 16384 and 16385, ratio 4 and
    just under it, batch 65535 and 65536, class counts on both sides of the byte limit) and must see all three statuses."""
    host = pkg.host_lib()
    rng = np.random.default_rng(11)
    rect4, seen = C.c_int32 * 4, set()
    for _ in range(3000):
        batch, rows, cols, classes, H, W = _edge_geometry(rng)
        want = host.mbn_resample_argmax_envelope(batch, rows, cols, classes, H, W)
        seen.add(want)
        for m in {1, _multiple(rng, rows, cols)}:
            full = rect4(0, 0, m * cols, m * rows)
            got = host.mbn_resample_window_envelope(batch, rows, cols, classes, m * rows, m * cols, full, H, W)
            assert got == want, (batch, rows, cols, classes, H, W, m, got, want)
            if want == pkg.OK:
                a, b = pkg.ResampleLaunch(), pkg.ResampleLaunch()
                host.mbn_resample_plan(rows, cols, H, W, C.byref(a))
                host.mbn_resample_window_plan(rows, cols, m * rows, m * cols, full, H, W, C.byref(b))
                assert _fields(a) == _fields(b), (rows, cols, H, W, m)
    assert seen == {pkg.OK, pkg.EINVAL, pkg.EUNSUPPORTED}, seen
    # ragged: item lists that differ only in carrying the full rectangle
    seen = set()
    for _ in range(1500):
        _, rows, cols, classes, _, _ = _edge_geometry(rng)
        m = _multiple(rng, rows, cols)
        plain, window, at = [], [], 0
        for _ in range(int(rng.integers(1, 6))):
            _, _, _, _, H, W = _edge_geometry(rng)
            if rng.integers(0, 3):                           # mostly an output of THIS map
                H, W = int(rng.integers(4 * max(rows, 1), 12 * max(rows, 1) + 1)), int(rng.integers(4 * max(cols, 1), 12 * max(cols, 1) + 1))
            at += int(rng.integers(-1, 50)) if rng.integers(0, 8) else -int(rng.integers(0, 3))     # touching, a gap, or now and then an overlap
            plain.append((at, H, W))
            window.append((at, H, W, (0, 0, m * cols, m * rows)))
            at += max(H, 0) * max(W, 0)
        a, b = pkg.ResampleLaunch(), pkg.ResampleLaunch()
        a.tiles = b.tiles = -5                               # a refused batch leaves the record alone
        pa, wa = pkg.label_items(plain), pkg.label_window_items(window)
        sort = (C.c_int64 * (2 * len(plain)))()
        want = host.mbn_resample_ragged_check(rows, cols, classes, pa, len(plain), sort, C.byref(a))
        got = host.mbn_resample_ragged_window_check(rows, cols, classes, m * rows, m * cols, wa, len(window), sort, C.byref(b))
        seen.add(want)
        assert got == want and _fields(a) == _fields(b), (rows, cols, classes, m, plain, got, want)
        assert (a.tiles == -5) == (want != pkg.OK)
    assert seen == {pkg.OK, pkg.EINVAL, pkg.EUNSUPPORTED}, seen


# ------------------------------------------------------------------------------------------------------------------------ symbols

DEVICE = ("mbn_resample_argmax_window_f32", "mbn_ragged_readout_set_window", "mbn_net_segment_fit", "mbn_net_segment_images_fit")
PREDICATES = ("mbn_resample_window_envelope", "mbn_resample_window_plan", "mbn_resample_ragged_window_check")


def test_symbols_where_they_belong(pkg):
    lib, host = pkg.load(), pkg.host_lib()
    for name in DEVICE + PREDICATES:
        assert hasattr(lib, name), name
    for name in PREDICATES:
        assert hasattr(host, name), name
    for name in DEVICE:                                  # device code / the net runner: not in the host library
        assert not hasattr(host, name), name
    assert set(DEVICE) <= set(pkg.declared_symbols())
    for cls, name in ((pkg.Context, "resample_argmax_window"), (pkg.RaggedReadout, "set_window"), (pkg.Net, "segment_fit"),
                      (pkg.Net, "segment_images_fit")):
        assert callable(getattr(cls, name))


def test_label_window_item_struct_matches_header(pkg, tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "mbn.h"
#define O(f) offsetof(mbn_label_window_item, f)
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(mbn_label_window_item), O(dst_offset), O(rows), O(cols), O(x), O(y), O(iw), O(ih),
 sizeof(mbn_label_item));return 0;}'''
    (tmp_path / "t.c").write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-I", os.path.join(pkg.REPO_ROOT, "include"), "-o", exe, str(tmp_path / "t.c")])
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    L = pkg.LabelWindowItem
    assert vals == [32, 0, 8, 12, 16, 20, 24, 28, 16]
    assert vals[:8] == [C.sizeof(L)] + [getattr(L, f).offset for f in ("dst_offset", "rows", "cols", "x", "y", "iw", "ih")]
    assert C.sizeof(pkg.LabelItem) == 16
