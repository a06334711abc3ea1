"""Segment through the letterbox on the GPU. mbn_resample_argmax_window_f32 alone: labels and score bits equal to tests/dense_window_ref.py (the
normative arithmetic) on the smallest shapes that reach each way of going wrong, bit-equal to mbn_resample_argmax_f32 for the full window and to
a crop of it for a window on its grid, adversarial values inside and just outside the rectangle, argument errors, nothing written outside the
maps. The ragged window set: every image bit-equal to the reference, gaps untouched, a plain set and a window set alternating on one handle, a
refused set leaves the previous one valid. The net runner: segment_fit and segment_images_fit against the reference applied to forward_dense's
own logits over the letterboxed staging buffer. The C host's --fit pad --segment-source.

Planning CU counts: the kernel is one workgroup per output tile and not persistent; nothing in it or in its launch depends on the number of
compute units, so there is no planning-CU sweep here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_any_ref
import dense_window_ref
from test_dense_any_gpu import LAB_FILL, SC_FILL, TAIL, _logits, _ragged_layout
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _device(ctx, x, R, Cc, rect, H, W, offset=0, with_score=True):
    """mbn_resample_argmax_window_f32 on x [n][h][w][classes] (uploaded `offset` bytes into its allocation): (labels, score bits or None). The
    output buffers carry a sentinel pattern and TAIL more elements, which must come back unchanged."""
    n, h, w, classes = x.shape
    d_x = ctx.to_device(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
    npix = n * H * W
    d_lab = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32))
    d_sc = ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32)) if with_score else None
    ctx.resample_argmax_window(d_lab.ptr, d_sc.ptr if with_score else None, d_x.ptr + offset, n, h, w, classes, R, Cc, rect, H, W)
    ctx.sync()
    lab = d_lab.download((npix + TAIL,), np.int32)
    sc = d_sc.download((npix + TAIL,), np.uint32) if with_score else None
    for b in (d_x, d_lab, d_sc):
        if b is not None:
            b.free()
    assert (lab[npix:] == LAB_FILL).all(), "labels written past the last image"
    if sc is not None:
        assert (sc[npix:].view(np.float32) == SC_FILL).all(), "scores written past the last image"
        sc = sc[:npix].reshape(n, H, W)
    return lab[:npix].reshape(n, H, W), sc


def _check(ctx, x, R, Cc, rect, H, W, what, **kw):
    want_lab, want_sc = dense_window_ref.resample_argmax_window(x, R, Cc, rect, H, W)
    lab, sc = _device(ctx, x, R, Cc, rect, H, W, **kw)
    bad = int((lab != want_lab).sum())
    assert bad == 0, "%s: %d of %d labels differ from dense_window_ref" % (what, bad, lab.size)
    if sc is not None:
        bad = int((sc != _bits(want_sc)).sum())
        assert bad == 0, "%s: %d of %d score bit patterns differ from dense_window_ref" % (what, bad, sc.size)
    return want_lab, want_sc


# ----------------------------------------------------------------------------------------------------------------------- geometry

def _geometry(h, w):
    """name -> (rect = (x, y, iw, ih), H, W) for an h x w map of a 32 h x 32 w input"""
    R, Cc = 32 * h, 32 * w
    return {"smaller than a tile": ((Cc // 4 + 3, R // 4 + 1, 20, 17), 9, 13),
            "x = y = 0": ((0, 0, Cc - 21, R - 13), 45, 70),
            "flush with the far edge": ((21, 13, Cc - 21, R - 13), 45, 70),
            "minimum ratio": ((0, 0, Cc, R), 4 * h, 4 * w),                  # N R = 4 l n on both axes
            "one pixel wide": ((Cc // 2 + 5, 3, 1, R - 7), 37, 70),
            "rows % 4, cols % 32": ((7, 5, Cc - 20, R - 9), 37, 61)}


@pytest.mark.parametrize("classes", [21, 64])                  # 21: dword loads, a padded last group; 64: 16-byte loads
@pytest.mark.parametrize("name", list(_geometry(2, 3)))
@pytest.mark.parametrize("hw", [(2, 3), (5, 7)])
def test_kernel_geometry(pkg, ctx, hw, name, classes):
    h, w = hw
    rect, H, W = _geometry(h, w)[name]
    R, Cc = 32 * h, 32 * w
    assert pkg.resample_window_envelope(2, h, w, classes, R, Cc, rect, H, W) == pkg.OK
    if name == "minimum ratio":
        assert H * R == 4 * rect[3] * h and W * Cc == 4 * rect[2] * w
    _check(ctx, _logits(2, h, w, classes, seed=h * 1000 + w * 100 + H + W), R, Cc, rect, H, W, "%s %s classes %d" % (hw, name, classes))


@pytest.mark.parametrize("classes", [21, 64])
def test_kernel_minimum_ratio_footprint_10(pkg, ctx, classes):
    """Output 20 x 28 of the 5 x 7 samples' worth of input inside a 10 x 14 map: the ratio is exactly 4 and a tile stages 10 x 10 vectors."""
    h, w, R, Cc, rect, H, W = 10, 14, 320, 448, (224, 160, 224, 160), 20, 28
    assert H * R == 4 * rect[3] * h and W * Cc == 4 * rect[2] * w
    l = pkg.resample_window_plan(h, w, R, Cc, rect, H, W)
    assert (l.fy, l.fx, l.ch) == (10, 10, 64)
    _check(ctx, _logits(2, h, w, classes, seed=classes), R, Cc, rect, H, W, "footprint 10, classes %d" % classes)


def _waves_crossing(i0_rows, H):
    """per wave (eight output rows of a tile: two groups of four) whether one of its row groups crosses a coarse row"""
    out = []
    for y in range(0, H, 8):
        groups = [i0_rows[g:min(g + 4, H)] for g in (y, y + 4) if g < H]
        out.append(any(g.max() != g.min() for g in groups))
    return out


def test_kernel_waves_that_cross_a_coarse_row_and_waves_that_do_not(pkg, ctx):
    h, w, R, Cc, classes = 5, 7, 160, 224, 21
    # the full window at factor 8: i0 steps at o = 4 (mod 8), on a group's edge: no wave takes the loop with the third interpolant
    rect, H, W = (0, 0, Cc, R), 40, 56
    i0 = dense_window_ref.axis_window(H, h, R, rect[1], rect[3])[0]
    assert not any(_waves_crossing(i0, H))
    _check(ctx, _logits(1, h, w, classes, seed=5), R, Cc, rect, H, W, "no wave crosses")
    # a window at an odd ratio: some waves cross and some do not, in the same launch
    rect, H, W = (9, 11, 180, 120), 67, 50
    i0 = dense_window_ref.axis_window(H, h, R, rect[1], rect[3])[0]
    cr = _waves_crossing(i0, H)
    assert any(cr) and not all(cr), cr
    _check(ctx, _logits(1, h, w, classes, seed=6), R, Cc, rect, H, W, "some waves cross")


@pytest.mark.parametrize("R", [160, 163])                      # R / n an integer or not
def test_kernel_full_window_equals_the_plain_kernel(pkg, ctx, R):
    n, h, w, classes, H, W = 2, 5, 7, 21, 37, 61
    Cc = 224 if R == 160 else 229
    x = _logits(n, h, w, classes, seed=R)
    d_x = ctx.to_device(x)                              # both kernels on the same device buffer
    npix = n * H * W
    outs = [ctx.to_device(np.full(npix, LAB_FILL, np.int32)) for _ in range(2)] + [ctx.to_device(np.full(npix, SC_FILL, np.float32)) for _ in range(2)]
    ctx.resample_argmax(outs[0].ptr, outs[2].ptr, d_x.ptr, n, h, w, classes, H, W)
    ctx.resample_argmax_window(outs[1].ptr, outs[3].ptr, d_x.ptr, n, h, w, classes, R, Cc, (0, 0, Cc, R), H, W)
    ctx.sync()
    got = [b.download((npix,), np.uint32) for b in outs]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[3])
    want_lab, want_sc = dense_any_ref.resample_argmax(x, H, W)
    assert np.array_equal(got[1].view(np.int32).reshape(want_lab.shape), want_lab) and np.array_equal(got[3], _bits(want_sc).ravel())
    for b in [d_x] + outs:
        b.free()


@pytest.mark.parametrize("case", [(2, 32, 32, 48, 16), (7, 32, 168, 336, 28)])       # (n, S, l, N, b)
def test_kernel_window_on_the_grid_is_a_crop_of_the_plain_kernel(pkg, ctx, case):
    n, S, l, N, b = case
    R = n * S
    M, off = R * N // l, b * N // l
    assert M * l == R * N and off * l == b * N
    classes = 21
    x = _logits(1, n, n, classes, seed=n + N)
    d_x = ctx.to_device(x)
    d_full = [ctx.to_device(np.full(M * M, LAB_FILL, np.int32)), ctx.to_device(np.full(M * M, SC_FILL, np.float32))]
    d_win = [ctx.to_device(np.full(N * N, LAB_FILL, np.int32)), ctx.to_device(np.full(N * N, SC_FILL, np.float32))]
    ctx.resample_argmax(d_full[0].ptr, d_full[1].ptr, d_x.ptr, 1, n, n, classes, M, M)
    ctx.resample_argmax_window(d_win[0].ptr, d_win[1].ptr, d_x.ptr, 1, n, n, classes, R, R, (b, b, l, l), N, N)      # both axes
    ctx.sync()
    full = [d.download((M, M), np.uint32) for d in d_full]
    win = [d.download((N, N), np.uint32) for d in d_win]
    for f, g in zip(full, win):
        assert np.array_equal(f[off:off + N, off:off + N], g)
    for d in [d_x] + d_full + d_win:
        d.free()


# ------------------------------------------------------------------------------------------------------------------ classes, inputs

@pytest.mark.parametrize("classes", [1, 65, 1001])             # one class; an odd count over a 16-byte chunk; 7 chunks of 128 + 105
def test_kernel_class_counts(pkg, ctx, classes):
    n, h, w, R, Cc, rect, H, W = 2, 2, 2, 64, 64, (5, 9, 40, 30), 11, 9
    x = _logits(n, h, w, classes, seed=classes)
    x[0, 0, 0, classes - 1] += 100.0                   # a winner in the last class ...
    if classes > 128:
        x[1, h - 1, w - 1, 128] += 100.0               # ... and in the first class of a later chunk
    lab, _ = _check(ctx, x, R, Cc, rect, H, W, "classes %d" % classes)
    assert lab[0, 0, 0] == classes - 1 and (classes <= 128 or lab[1, -1, -1] == 128)


def test_kernel_class_counts_short_chunk(pkg, ctx):
    """130 classes at a footprint over 38 vectors: the 64-class chunk, two full and 2"""
    h, w, R, Cc, rect, H, W, classes = 14, 14, 224, 224, (32, 16, 112, 112), 28, 28, 130
    assert pkg.resample_window_plan(h, w, R, Cc, rect, H, W).ch == 64
    x = _logits(1, h, w, classes, seed=131)
    x[0, 0, 1, classes - 1] += 1000.0                  # output (0, 0) sits at input (18, 34): map coordinate (0.625, 1.625), weight 0.14 on (0, 1)
    x[0, 7, 8, 64] += 1000.0                           # the last one at (126, 142): (7.375, 8.375), weight 0.39 on (7, 8)
    lab, _ = _check(ctx, x, R, Cc, rect, H, W, "short chunk, classes %d" % classes)
    assert lab[0, 0, 0] == classes - 1 and lab[0, -1, -1] == 64


@pytest.mark.parametrize("classes", [21, 64])
def test_kernel_logits_at_a_4_byte_offset(pkg, ctx, classes):
    _check(ctx, _logits(3, 2, 3, classes, seed=9), 64, 96, (10, 7, 60, 50), 11, 17, "offset 4, classes %d" % classes, offset=4)


def test_kernel_score_null(pkg, ctx):
    _check(ctx, _logits(2, 3, 2, 21, seed=11), 96, 64, (3, 20, 50, 60), 13, 9, "score NULL", with_score=False)


def test_kernel_adversarial_values(pkg, ctx):
    """The rectangle (64, 32, 96, 96) of a 160 x 224 input covers the coarse samples of rows 1..3 and columns 2..4 of the 5 x 7 map; its border
    outputs interpolate with rows 0 / 4 and columns 1 / 5 outside it (no clamp at the window's edge)."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    h, w, R, Cc, rect, H, W = 5, 7, 160, 224, (64, 32, 96, 96), 39, 41
    y0, y1, _, wy1 = dense_window_ref.axis_window(H, h, R, rect[1], rect[3])
    x0, x1, _, wx1 = dense_window_ref.axis_window(W, w, Cc, rect[0], rect[2])
    assert y0[0] == 0 and wy1[0] < 1 and y1[-1] == 4 and wy1[-1] > 0 and x0[0] == 1 and wx1[0] < 1 and x1[-1] == 5 and wx1[-1] > 0
    x = np.zeros((2, h, w, 200), np.float32)           # equal maxima in different chunks: the lowest index wins
    x[..., 5] = x[..., 70] = x[..., 131] = 2.0
    lab, sc = _check(ctx, x, R, Cc, rect, H, W, "equal maxima")
    assert (lab == 5).all()
    lab, sc = _check(ctx, np.full((1, h, w, 21), 1.5, np.float32), R, Cc, rect, H, W, "constant map")
    assert (lab == 0).all()
    x = _logits(1, h, w, 65, seed=13)                  # NaNs inside the rectangle, where the winner was, and just outside it
    x[0, 2, 3, int(x[0, 2, 3].argmax())] = nan
    x[0, 0, 3, 64] = nan                               # row 0: outside, read by the first output rows
    x[0, 2, 5, int(x[0, 2, 5].argmax())] = nan         # column 5: outside, read by the last output columns
    _, want_sc = _check(ctx, x, R, Cc, rect, H, W, "NaN inside and outside")
    x2 = x.copy()
    x2[0, 2, 5, :] = _logits(1, 1, 1, 65, seed=14)[0, 0, 0]
    assert not np.array_equal(dense_window_ref.resample_argmax_window(x2, R, Cc, rect, H, W)[1][0, :, -1], want_sc[0, :, -1]), "outside samples count"
    x = _logits(1, h, w, 21, seed=15)                  # +inf just outside: inf and (where its weight is zero) NaN interpolants on the border
    x[0, 4, 1, 3] = inf
    x[0, 0, 5, 7] = -inf
    _check(ctx, x, R, Cc, rect, H, W, "inf outside")
    lab, sc = _check(ctx, np.full((1, h, w, 21), nan, np.float32), R, Cc, rect, H, W, "all NaN")
    assert (lab == 0).all() and (sc == -inf).all()
    x = _logits(2, h, w, 21, seed=17)                  # an all -inf pixel inside and one outside
    x[1, 2, 3, :] = -inf
    x[0, 0, 1, :] = -inf
    lab, sc = _check(ctx, x, R, Cc, rect, H, W, "all -inf pixels")
    assert (sc[1] == -inf).any() and (lab[1][sc[1] == -inf] == 0).all()
    x = np.random.default_rng(19).integers(-8, 9, (2, h, w, 65)).astype(np.float32)      # integer-valued logits: ties everywhere
    _check(ctx, x, R, Cc, rect, H, W, "integer-valued logits")


def test_kernel_argument_errors(pkg, ctx):
    x = ctx.to_device(np.zeros(2 * 2 * 21, np.float32))
    fill = np.full(16 * 16, LAB_FILL, np.int32)
    lab, sc = ctx.to_device(fill), ctx.to_device(fill.astype(np.float32))
    rect_t = lambda *v: (C.c_int32 * 4)(*v)
    call = lambda l, s, p, n, h, w, c, R, Cc, rect, H, W: ctx.lib.mbn_resample_argmax_window_f32(ctx.h, l, s, p, n, h, w, c, R, Cc, rect, H, W, None)
    full = rect_t(0, 0, 64, 64)
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, full, 7, 16) == pkg.EUNSUPPORTED           # under 4 x the samples of the window
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, full, 16, 7) == pkg.EUNSUPPORTED
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, rect_t(0, 0, 64, 57), 7, 16) == pkg.EUNSUPPORTED       # 7 * 64 = 4 * 56 * 2: one row too many
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 16385, 64, full, 16, 16) == pkg.EUNSUPPORTED
    assert call(None, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, full, 16, 16) == pkg.EINVAL
    assert call(lab.ptr, sc.ptr, None, 1, 2, 2, 21, 64, 64, full, 16, 16) == pkg.EINVAL
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, None, 16, 16) == pkg.EINVAL
    for bad in [(0, 2, 2, 21, 64, 64, 16, 16), (1, 0, 2, 21, 64, 64, 16, 16), (1, 2, 0, 21, 64, 64, 16, 16), (1, 2, 2, 0, 64, 64, 16, 16),
                (1, 2, 2, 21, 0, 64, 16, 16), (1, 2, 2, 21, 64, -1, 16, 16), (1, 2, 2, 21, 64, 64, 0, 16), (1, 2, 2, 21, 64, 64, 16, -1),
                (1, 2, 2, 21, 1, 64, 16, 16)]:                                                             # the last: an input smaller than the map
        assert call(lab.ptr, sc.ptr, x.ptr, *bad[:6], rect_t(0, 0, 1, 1), *bad[6:]) == pkg.EINVAL, bad
    for r in [(-1, 0, 64, 64), (0, -1, 64, 64), (0, 0, 0, 64), (0, 0, 64, 0), (1, 0, 64, 64), (0, 1, 64, 64)]:
        assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, rect_t(*r), 16, 16) == pkg.EINVAL, r
    assert call(lab.ptr, sc.ptr, x.ptr + 2, 1, 2, 2, 20, 64, 64, full, 16, 16) == pkg.EINVAL             # off 4 bytes
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, full, 16, 17) == pkg.EINVAL                 # 16 x 17 labels into a 16 x 16 buffer: the span check
    ctx.sync()
    assert np.array_equal(lab.download(fill.shape, np.int32), fill), "nothing may have been launched"
    assert np.array_equal(sc.download(fill.shape, np.float32), fill.astype(np.float32))
    assert call(lab.ptr, None, x.ptr, 1, 2, 2, 21, 64, 64, rect_t(0, 0, 64, 56), 7, 16) == pkg.OK       # the ratio exactly, score NULL
    ctx.sync()
    got = lab.download(fill.shape, np.int32)
    assert (got[:7 * 16] == 0).all() and (got[7 * 16:] == LAB_FILL).all()
    for b in (x, lab, sc):
        b.free()


# ------------------------------------------------------------------------------------------------------------------------- ragged

H5, W7, R5, C7 = 5, 7, 160, 224
FULL = (0, 0, C7, R5)
# (rows, cols, rect): a full window; the minimum ratio (20 x 28 of the whole input); a letterbox-like rectangle; two identical items
RAGGED = [(37, 61, FULL), (20, 28, FULL), (40, 56, (56, 0, 112, 160)), (100, 30, (9, 11, 180, 120)), (40, 56, (56, 0, 112, 160))]


def _ragged_run(ctx, rd, x, total):
    d_x = ctx.to_device(x)
    d_lab, d_sc = ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, SC_FILL, np.float32))
    rd.run(d_lab.ptr, d_sc.ptr, d_x.ptr)
    ctx.sync()
    lab, sc = d_lab.download((total,), np.int32), d_sc.download((total,), np.float32)
    for b in (d_x, d_lab, d_sc):
        b.free()
    return lab, sc


def _ragged_compare(want, offs, lab, sc):
    """want[i] = (labels, score) [H][W] of image i from a reference"""
    touched = np.zeros(lab.size, bool)
    for i, ((wl, ws), off) in enumerate(zip(want, offs)):
        H, W = wl.shape
        assert np.array_equal(lab[off:off + H * W].reshape(H, W), wl), "item %d labels" % i
        assert np.array_equal(_bits(sc[off:off + H * W]).reshape(H, W), _bits(ws)), "item %d scores" % i
        touched[off:off + H * W] = True
    assert (lab[~touched] == LAB_FILL).all() and (sc[~touched] == SC_FILL).all(), "written between or behind the maps"


def _want_window(x, items):
    out = []
    for i, (H, W, rect) in enumerate(items):
        l, s = dense_window_ref.resample_argmax_window(x[i:i + 1], R5, C7, rect, H, W)
        out.append((l[0], s[0]))
    return out


def _want_plain(x, sizes):
    out = []
    for i, (H, W) in enumerate(sizes):
        l, s = dense_any_ref.resample_argmax(x[i:i + 1], H, W)
        out.append((l[0], s[0]))
    return out


def test_ragged_window(pkg, ctx):
    classes = 21
    x = _logits(5, H5, W7, classes, seed=78)
    sizes = [(H, W) for H, W, _ in RAGGED]
    rd = pkg.RaggedReadout(ctx, 5)
    offs, total = _ragged_layout(sizes, order=(3, 0, 4, 2, 1))
    items = [(o, H, W, rect) for o, (H, W, rect) in zip(offs, RAGGED)]
    rd.set_window(H5, W7, classes, R5, C7, items)
    lab, sc = _ragged_run(ctx, rd, x, total)
    want = _want_window(x, RAGGED)
    _ragged_compare(want, offs, lab, sc)
    # refused window sets: overlapping maps, an item under the ratio, a rectangle past the input, beyond max_batch: the set before stays valid
    lib = ctx.lib
    wset = lambda its: lib.mbn_ragged_readout_set_window(rd.h, H5, W7, classes, R5, C7, pkg.label_window_items(its), len(its), None)
    assert wset([(0, 37, 61, FULL), (37 * 61 - 1, 20, 28, FULL)]) == pkg.EINVAL
    assert wset([(0, 37, 61, FULL), (5000, 19, 28, FULL)]) == pkg.EUNSUPPORTED
    assert wset([(0, 37, 61, FULL), (5000, 37, 61, (1, 0, C7, R5))]) == pkg.EINVAL
    assert wset(items + [(90000, 20, 28, FULL)]) == pkg.EINVAL
    lab2, sc2 = _ragged_run(ctx, rd, x, total)
    assert np.array_equal(lab2, lab) and np.array_equal(_bits(sc2), _bits(sc))
    # a plain set after the window set on the same handle: the plain kernel's bits ...
    psizes = [(37, 61), (20, 28)]
    poffs, ptotal = _ragged_layout(psizes, order=(1, 0), gap=9, first=0)
    rd.set(H5, W7, classes, [(o, H, W) for o, (H, W) in zip(poffs, psizes)])
    plab, psc = _ragged_run(ctx, rd, x[:2], ptotal)
    _ragged_compare(_want_plain(x, psizes), poffs, plab, psc)
    # ... a refused window set leaves that plain set in place ...
    assert wset([(0, 37, 61, FULL), (5000, 19, 28, FULL)]) == pkg.EUNSUPPORTED
    plab2, psc2 = _ragged_run(ctx, rd, x[:2], ptotal)
    assert np.array_equal(plab2, plab) and np.array_equal(_bits(psc2), _bits(psc))
    # ... and the reverse: a window set after the plain one, with other rectangles for the same two sizes
    witems = [(37, 61, (100, 40, 90, 77)), (20, 28, (0, 0, 111, 160))]
    rd.set_window(H5, W7, classes, R5, C7, [(o, H, W, rect) for o, (H, W, rect) in zip(poffs, witems)])
    wlab, wsc = _ragged_run(ctx, rd, x[:2], ptotal)
    _ragged_compare(_want_window(x, witems), poffs, wlab, wsc)
    assert not np.array_equal(_bits(wsc), _bits(psc))
    rd.close()


# ------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS, BATCH = 0.5, 21, 64, 96, 3
SOURCES = [(75, 130), (64, 96), (120, 100)]


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _i32(v):
    return (C.c_int32 * len(v))(*v)


@pytest.mark.parametrize("dtype,os_", [("f32", 8), ("f32", 16), ("bf16", 8), ("i8", 32)])
def test_net_segment_fit(pkg, ctx, tmp_path, dtype, os_):
    n = BATCH
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, os_)
    h, w = ROWS // os_, COLS // os_
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    dt = {"f32": pkg.DT_F32, "bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype]
    if dt != pkg.DT_F32:
        net.set_dtype(dt)
    lib = ctx.lib
    rng = np.random.default_rng(31)
    d_dense = ctx.alloc(n * h * w * CLASSES * 4)
    bufs = [d_dense]

    def outputs(total):
        pair = ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, SC_FILL, np.float32))
        bufs.extend(pair)
        return pair

    # ---- uniform sources: (75, 130) letterboxed; (64, 96), whose aspect is the canvas's, goes through the window path as the full window
    first = True
    for sh, sw in SOURCES[:2]:
        src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
        d_src = ctx.to_device(src)
        bufs.append(d_src)
        npix = n * sh * sw
        d_lab, d_sc = outputs(npix + TAIL)
        if first:
            assert lib.mbn_net_segment_fit(net.h, d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr, d_sc.ptr) == pkg.EINVAL      # no uint8 images yet
            net.set_input_u8(True)
            assert lib.mbn_net_segment_fit(net.h, d_src.ptr, n, sh, sw, pkg.FIT_CROP, d_lab.ptr, d_sc.ptr) == pkg.EUNSUPPORTED
            assert lib.mbn_net_segment_fit(net.h, d_src.ptr, n, sh, sw, 7, d_lab.ptr, d_sc.ptr) == pkg.EINVAL
            assert lib.mbn_net_segment_fit(net.h, d_src.ptr, n + 1, sh, sw, pkg.FIT_PAD, d_lab.ptr, d_sc.ptr) == pkg.EINVAL
            # a 6 x 9 source has the canvas's aspect: the full window, 6 outputs of at least 2 coarse rows: under the ratio at every stride here
            assert lib.mbn_net_segment_fit(net.h, d_src.ptr, n, 6, 9, pkg.FIT_PAD, d_lab.ptr, d_sc.ptr) == pkg.EUNSUPPORTED
            ctx.sync()
            assert (d_lab.download((npix + TAIL,), np.int32) == LAB_FILL).all() and (d_sc.download((npix + TAIL,), np.float32) == SC_FILL).all()
            first = False
        rect = tuple(pkg.fit_pad(sh, sw, ROWS, COLS))
        assert (rect == (0, 0, COLS, ROWS)) == ((sh, sw) == (ROWS, COLS))
        staging = net.resize_input(d_src.ptr, n, sh, sw, fit=pkg.FIT_PAD)
        net.forward_dense(staging, d_dense.ptr, n)
        ctx.sync()
        dense = d_dense.download((n, h, w, CLASSES), np.float32)
        assert np.isfinite(dense).all() and dense.std() > 0
        net.segment_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr, d_sc.ptr)
        ctx.sync()
        want_lab, want_sc = dense_window_ref.resample_argmax_window(dense, ROWS, COLS, rect, sh, sw)
        lab, sc = d_lab.download((npix + TAIL,), np.int32), d_sc.download((npix + TAIL,), np.float32)
        assert np.array_equal(lab[:npix].reshape(n, sh, sw), want_lab), "%s os %d %dx%d: %d labels differ" % (dtype, os_, sh, sw,
                                                                                                          int((lab[:npix] != want_lab.ravel()).sum()))
        assert np.array_equal(_bits(sc[:npix]), _bits(want_sc).ravel())
        assert (lab[npix:] == LAB_FILL).all() and (sc[npix:] == SC_FILL).all()
        assert want_sc.std() > 0 and (dtype == "i8" or len(np.unique(want_lab)) > 1)       # (the 2 x 3 map of the int8 net has one label on noise)
        # FIT_STRETCH: segment_to's bits
        d_lab2, d_sc2 = outputs(npix)
        d_lab3, d_sc3 = outputs(npix)
        net.segment_fit(d_src.ptr, n, sh, sw, pkg.FIT_STRETCH, d_lab2.ptr, d_sc2.ptr)
        staging = net.resize_input(d_src.ptr, n, sh, sw, fit=pkg.FIT_STRETCH)
        net.segment_to(staging, n, sh, sw, d_lab3.ptr, d_sc3.ptr)
        ctx.sync()
        assert np.array_equal(d_lab2.download((npix,), np.int32), d_lab3.download((npix,), np.int32))
        assert np.array_equal(d_sc2.download((npix,), np.uint32), d_sc3.download((npix,), np.uint32))
        if (sh, sw) == (ROWS, COLS):                    # the canvas's own size: the letterbox is the stretch and the full window the plain rule
            assert np.array_equal(d_lab2.download((npix,), np.int32), lab[:npix]) and np.array_equal(d_sc2.download((npix,), np.uint32), _bits(sc[:npix]))
    # ---- segment_images_fit: three sources of their own sizes, each through its own rectangle
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in SOURCES]
    src_offs, at = [], 0
    for img in images:
        src_offs.append(at)
        at += img.size
    d_src = ctx.to_device(np.concatenate([img.ravel() for img in images]))
    bufs.append(d_src)
    rows, cols = [s[0] for s in SOURCES], [s[1] for s in SOURCES]
    dst, total = _ragged_layout(SOURCES, order=(2, 0, 1), gap=7)
    d_rlab, d_rsc = outputs(total)
    args = lambda r, c, fit: (net.h, d_src.ptr, _i64(src_offs), _i32(r), _i32(c), n, fit, d_rlab.ptr, _i64(dst), d_rsc.ptr)
    assert lib.mbn_net_segment_images_fit(*args(rows, cols, pkg.FIT_CROP)) == pkg.EUNSUPPORTED
    assert lib.mbn_net_segment_images_fit(*args(rows, cols, 7)) == pkg.EINVAL
    assert lib.mbn_net_segment_images_fit(*args([6] + rows[1:], [9] + cols[1:], pkg.FIT_PAD)) == pkg.EUNSUPPORTED      # an item under the ratio
    ctx.sync()
    assert (d_rlab.download((total,), np.int32) == LAB_FILL).all() and (d_rsc.download((total,), np.float32) == SC_FILL).all(), "a refused call may not write"
    staging = net.resize_inputs(d_src.ptr, src_offs, rows, cols, fit=pkg.FIT_PAD)
    net.forward_dense(staging, d_dense.ptr, n)
    ctx.sync()
    dense = d_dense.download((n, h, w, CLASSES), np.float32)
    net.segment_images_fit(d_src.ptr, src_offs, rows, cols, pkg.FIT_PAD, d_rlab.ptr, dst, d_rsc.ptr)
    ctx.sync()
    lab, sc = d_rlab.download((total,), np.int32), d_rsc.download((total,), np.float32)
    want = []
    for i, (sh, sw) in enumerate(SOURCES):
        l, s = dense_window_ref.resample_argmax_window(dense[i:i + 1], ROWS, COLS, tuple(pkg.fit_pad(sh, sw, ROWS, COLS)), sh, sw)
        want.append((l[0], s[0]))
    _ragged_compare(want, dst, lab, sc)
    # FIT_STRETCH: segment_images' bits
    d_a, d_as = outputs(total)
    d_b, d_bs = outputs(total)
    net.segment_images_fit(d_src.ptr, src_offs, rows, cols, pkg.FIT_STRETCH, d_a.ptr, dst, d_as.ptr)
    net.segment_images(d_src.ptr, src_offs, rows, cols, d_b.ptr, dst, d_bs.ptr)
    ctx.sync()
    assert np.array_equal(d_a.download((total,), np.int32), d_b.download((total,), np.int32))
    assert np.array_equal(d_as.download((total,), np.uint32), d_bs.download((total,), np.uint32))
    assert not np.array_equal(d_as.download((total,), np.uint32), _bits(sc))              # the two fits are different read-outs
    net.destroy()
    for b in bufs:
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def test_c_host_segment_source_pad(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    seed, alpha, os_, sh, sw = 3, 0.5, 16, 75, 130
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, out = str(tmp_path / "a.ppm"), str(tmp_path / "out.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", str(seed), "--alpha", str(alpha), "--res", "%dx%d" % (ROWS, COLS), "--output-stride", str(os_), "--ppm", ppm]
    r = subprocess.run(common + ["--segment-source", out], capture_output=True, text=True, timeout=300)      # the default fit is the crop
    assert r.returncode == 2 and not os.path.exists(out), r.stdout + r.stderr
    r = subprocess.run(common + ["--fit", "pad", "--segment-source", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    assert m, raw[:32]
    classes = 1000                                      # the host's synthetic weights
    assert tuple(int(g) for g in m.groups()) == (sw, sh, classes - 1)
    got = np.frombuffer(raw[m.end():], ">u2").astype(np.int32).reshape(sh, sw)
    # the same through the mirror
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(ROWS, COLS), lib=pkg.load(), output_stride=os_)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 1)
    net.set_input_u8(True)
    d_src, d_lab = ctx.to_device(src), ctx.alloc(sh * sw * 4)
    net.segment_fit(d_src.ptr, 1, sh, sw, pkg.FIT_PAD, d_lab.ptr)
    ctx.sync()
    want = d_lab.download((sh, sw), np.int32)
    assert np.array_equal(got, want), "%d of %d pixels differ from Net.segment_fit" % (int((got != want).sum()), want.size)
    assert len(np.unique(want)) > 1
    net.destroy()
    d_src.free()
    d_lab.free()
    hw.free()
