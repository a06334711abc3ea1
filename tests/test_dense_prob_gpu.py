"""Segment with confidence on the GPU. mbn_resample_softmax_f32 / _window_f32 / _ragged_f32: labels and score bits equal to the reference
(tests/dense_prob_ref.py) and to the argmax calls on the same device buffer, prob within bound(classes) = (classes + 200) * 2^-24 of the float64
reference and exactly 0 where that is 0, on the shapes of test_dense_any_gpu.py / test_dense_window_gpu.py; the ramps that break a naive online
rescale, logits around +80 and -80, special values; the threshold, exact against the kernel's own prob and, on the pairs test_dense_prob_cpu.py
clears, against the reference; argument errors with nothing written. The net runner's segment_prob_to / _fit / _images_fit against the
reference applied to forward_dense's own logits and against the argmax paths' labels. The C host's --segment-confidence and --min-confidence.

Every comparison prints its largest prob error in units of 2^-24 before it asserts (pytest -s shows them)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_prob_ref as P
from test_dense_any_gpu import GEOMETRY, LAB_FILL, SC_FILL, TAIL, _logits, _ragged_layout
from test_dilation_gpu import _weights_os
from test_rect_gpu import _images

pytestmark = pytest.mark.gpu

PR_FILL = -5.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(ctx, x, H, W, window=None, offset=0, with_score=True, with_prob=True, min_prob=0.0, ignore=0, argmax=False):
    """mbn_resample_softmax_f32 (window = (R, C, rect): _window_f32; argmax: the argmax call of the same form) on x [n][h][w][classes], uploaded
    `offset` bytes into its allocation: (labels, score or None, prob or None). The output buffers carry a sentinel pattern and TAIL more
    elements, which must come back unchanged."""
    n, h, w, classes = x.shape
    d_x = ctx.to_device(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
    npix = n * H * W
    d_lab = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32))
    d_sc = ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32)) if with_score else None
    d_pr = ctx.to_device(np.full(npix + TAIL, PR_FILL, np.float32)) if with_prob and not argmax else None
    sc_ptr, pr_ptr = d_sc.ptr if d_sc else None, d_pr.ptr if d_pr else None
    if argmax and window:
        ctx.resample_argmax_window(d_lab.ptr, sc_ptr, d_x.ptr + offset, n, h, w, classes, window[0], window[1], window[2], H, W)
    elif argmax:
        ctx.resample_argmax(d_lab.ptr, sc_ptr, d_x.ptr + offset, n, h, w, classes, H, W)
    elif window:
        ctx.resample_softmax_window(d_lab.ptr, pr_ptr, sc_ptr, d_x.ptr + offset, n, h, w, classes, window[0], window[1], window[2], H, W, min_prob, ignore)
    else:
        ctx.resample_softmax(d_lab.ptr, pr_ptr, sc_ptr, d_x.ptr + offset, n, h, w, classes, H, W, min_prob, ignore)
    ctx.sync()
    lab = d_lab.download((npix + TAIL,), np.int32)
    sc = d_sc.download((npix + TAIL,), np.float32) if d_sc else None
    pr = d_pr.download((npix + TAIL,), np.float32) if d_pr else None
    for b in (d_x, d_lab, d_sc, d_pr):
        if b is not None:
            b.free()
    assert (lab[npix:] == LAB_FILL).all(), "labels written past the last image"
    assert sc is None or (sc[npix:] == SC_FILL).all(), "scores written past the last image"
    assert pr is None or (pr[npix:] == PR_FILL).all(), "probabilities written past the last image"
    shape = (n, H, W)
    return lab[:npix].reshape(shape), None if sc is None else sc[:npix].reshape(shape), None if pr is None else pr[:npix].reshape(shape)


def _prob_check(pr, want, classes, what):
    """pr (fp32, the kernel's) against want (float64, the reference's): exactly 0 where want is 0, within bound(classes) relative elsewhere"""
    assert pr.dtype == np.float32 and pr.shape == want.shape
    zero = want == 0
    nz = ~zero
    err = float((np.abs(pr[nz].astype(np.float64) - want[nz]) / want[nz]).max()) if nz.any() else 0.0
    print("%s: max prob error %.2f x 2^-24 (bound %d), %d pixels, %d with prob 0" % (what, err * 2.0 ** 24, classes + 200, want.size, int(zero.sum())))
    assert not zero.any() or (pr[zero] == 0).all(), "%s: a nonzero prob where best is not finite" % what
    assert err <= P.bound(classes), "%s: prob error %.1f x 2^-24 above the bound %d x 2^-24" % (what, err * 2.0 ** 24, classes + 200)
    assert (pr >= 0).all() and (pr <= 1).all()


def _check(ctx, x, H, W, what, window=None, **kw):
    if window:
        want_lab, want_sc, want_pr = P.resample_softmax_window(x, window[0], window[1], window[2], H, W)
    else:
        want_lab, want_sc, want_pr = P.resample_softmax(x, H, W)
    lab, sc, pr = _run(ctx, x, H, W, window=window, **kw)
    bad = int((lab != want_lab).sum())
    assert bad == 0, "%s: %d of %d labels differ from the reference" % (what, bad, lab.size)
    if sc is not None:
        bad = int((_bits(sc) != _bits(want_sc)).sum())
        assert bad == 0, "%s: %d of %d score bit patterns differ from the reference" % (what, bad, sc.size)
    if pr is not None:
        _prob_check(pr, want_pr, x.shape[3], what)
    return want_lab, want_sc, want_pr, pr


# ------------------------------------------------------------------------------------------------------------- against the reference

@pytest.mark.parametrize("n,classes", [(1, 21), (3, 64)])       # 21: dword loads, a padded last group; 64: 16-byte loads
@pytest.mark.parametrize("geo", GEOMETRY)
def test_kernel_geometry(pkg, ctx, geo, n, classes):
    h, w, H, W = geo
    _check(ctx, _logits(n, h, w, classes, seed=h * 1000 + w * 100 + H + W), H, W, "%s n %d classes %d" % (geo, n, classes))


@pytest.mark.parametrize("classes", [1, 2, 21, 64, 65, 1001])  # one class; chunk of 128: under, a full 16-byte chunk, an odd count, 7 chunks + 105
def test_kernel_class_counts(pkg, ctx, classes):
    n, h, w, H, W = 2, 2, 2, 11, 9
    x = _logits(n, h, w, classes, seed=classes)
    x[0, 0, 0, classes - 1] += 100.0                   # a winner in the last class ...
    if classes > 128:
        x[1, h - 1, w - 1, 128] += 100.0               # ... and in the first class of a later chunk
    lab, _, _, pr = _check(ctx, x, H, W, "classes %d" % classes)
    assert lab[0, 0, 0] == classes - 1 and (classes <= 128 or lab[1, -1, -1] == 128)
    if classes == 1:
        assert (pr == 1.0).all()


@pytest.mark.parametrize("classes", [64, 65, 130])             # the 64-class chunk (more than 38 staged vectors): one full, one + 1, two + 2
def test_kernel_class_counts_short_chunk(pkg, ctx, classes):
    assert pkg.resample_plan(7, 7, 30, 28).ch == 64
    x = _logits(1, 7, 7, classes, seed=classes + 1)
    x[0, 0, 0, classes - 1] += 100.0
    if classes > 64:
        x[0, 6, 6, 64] += 100.0
    lab, _, _, _ = _check(ctx, x, 30, 28, "short chunk, classes %d" % classes)
    assert lab[0, 0, 0] == classes - 1 and (classes <= 64 or lab[0, -1, -1] == 64)


@pytest.mark.parametrize("step", [0.25, 20.0, -0.25, -20.0])
def test_kernel_ramp(pkg, ctx, step):
    """x[..., c] = c * step: ascending, every class is a new maximum, which is what a rescale per maximum cannot afford; at 0.25 some 64 classes
    lie within the margin of the reference, at 20 every group of four moves it. Descending: the first class is the reference of all."""
    n, h, w, classes, H, W = 2, 2, 2, 1001, 11, 9
    c = np.arange(classes, dtype=np.float32)
    x = np.broadcast_to((c if step > 0 else c[::-1]) * np.float32(abs(step)), (n, h, w, classes)).astype(np.float32)
    lab, _, want_pr, _ = _check(ctx, x, H, W, "ramp %g" % step)
    assert (lab == (classes - 1 if step > 0 else 0)).all()
    assert abs(step) > 1 or want_pr.max() < 0.25       # the shallow ramp's sum has many terms that count
    # the same with noise on it, so that new maxima come in no regular order
    x = (x + np.random.default_rng(7).standard_normal(x.shape).astype(np.float32)).astype(np.float32)
    _check(ctx, x, H, W, "noisy ramp %g" % step)


@pytest.mark.parametrize("centre", [80.0, -80.0])
def test_kernel_sign_of_the_maximum(pkg, ctx, centre):
    """exp(80) overflows fp32 and exp(-80) * 1001 is far below 1: without a real max-subtraction neither gives a probability"""
    x = (_logits(2, 3, 2, 1001, seed=23) + np.float32(centre)).astype(np.float32)
    _, _, want_pr, _ = _check(ctx, x, 13, 9, "logits around %g" % centre)
    assert 0 < want_pr.min() and want_pr.max() < 1
    x = (_logits(1, 5, 7, 21, seed=24) + np.float32(centre)).astype(np.float32)
    _check(ctx, x, 37, 61, "logits around %g, 21 classes" % centre)


def test_kernel_special_values(pkg, ctx):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    lab, sc, pr, got = _check(ctx, np.full((1, 2, 2, 21), nan, np.float32), 9, 11, "all NaN")
    assert (lab == 0).all() and (sc == -inf).all() and (got == 0).all()
    x = _logits(2, 3, 3, 21, seed=17)                  # an all -inf pixel: -inf and NaN interpolants around it; at 3 -> 13 output 6 is its centre
    x[1, 1, 1, :] = -inf
    lab, sc, pr, got = _check(ctx, x, 13, 13, "all -inf pixel")
    assert lab[1, 6, 6] == 0 and sc[1, 6, 6] == -inf and got[1, 6, 6] == 0 and (got[0] > 0).all()
    x = _logits(1, 3, 3, 65, seed=18)                  # a +inf winner: prob 0 where it wins (everywhere its weight is not zero), NaN where it is
    x[0, 1, 1, 40] = inf
    lab, sc, pr, got = _check(ctx, x, 13, 17, "+inf winner")
    assert (sc == inf).any() and (got[sc == inf] == 0).all() and (lab[sc == inf] == 40).all() and (got[sc < inf] > 0).all()
    x = _logits(1, 3, 3, 65, seed=13)                  # a NaN where the winner was: the runner-up wins, the NaN is no term of the sum
    x[0, 1, 1, int(x[0, 1, 1].argmax())] = nan
    x[0, 0, 2, 64] = nan
    _check(ctx, x, 13, 17, "NaN in the winning position")
    x = np.zeros((2, 2, 3, 200), np.float32)           # equal maxima in different chunks (of 128 and of 64): the lowest index wins
    x[..., 5] = x[..., 70] = x[..., 131] = 2.0
    lab, sc, pr, got = _check(ctx, x, 11, 17, "equal maxima")
    assert (lab == 5).all() and np.allclose(pr, 1.0 / (3 + 197 * np.exp(-2.0)), rtol=1e-6)
    x = np.zeros((1, 7, 7, 200), np.float32)
    x[..., 5] = x[..., 70] = x[..., 131] = 2.0
    lab, _, _, _ = _check(ctx, x, 30, 28, "equal maxima, short chunk")
    assert (lab == 5).all()
    _check(ctx, _logits(2, 3, 2, 21, seed=11), 13, 9, "score NULL", with_score=False)


# --------------------------------------------------------------------------------------------------------- bit equality with argmax

def _equal_to_argmax(ctx, x, H, W, what, window=None, offset=0):
    """both kernels on the same device buffer: labels and score bits"""
    n, h, w, classes = x.shape
    d_x = ctx.to_device(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
    npix = n * H * W
    labs = [ctx.to_device(np.full(npix, LAB_FILL, np.int32)) for _ in range(2)]
    scs = [ctx.to_device(np.full(npix, SC_FILL, np.float32)) for _ in range(2)]
    d_pr = ctx.to_device(np.full(npix, PR_FILL, np.float32))
    p = d_x.ptr + offset
    if window:
        R, Cc, rect = window
        ctx.resample_argmax_window(labs[0].ptr, scs[0].ptr, p, n, h, w, classes, R, Cc, rect, H, W)
        ctx.resample_softmax_window(labs[1].ptr, d_pr.ptr, scs[1].ptr, p, n, h, w, classes, R, Cc, rect, H, W)
    else:
        ctx.resample_argmax(labs[0].ptr, scs[0].ptr, p, n, h, w, classes, H, W)
        ctx.resample_softmax(labs[1].ptr, d_pr.ptr, scs[1].ptr, p, n, h, w, classes, H, W)
    ctx.sync()
    got_l = [b.download((npix,), np.int32) for b in labs]
    got_s = [b.download((npix,), np.uint32) for b in scs]
    pr = d_pr.download((npix,), np.float32)
    for b in [d_x, d_pr] + labs + scs:
        b.free()
    assert np.array_equal(got_l[0], got_l[1]), "%s: %d labels differ from the argmax kernel's" % (what, int((got_l[0] != got_l[1]).sum()))
    assert np.array_equal(got_s[0], got_s[1]), "%s: score bits differ from the argmax kernel's" % what
    assert (pr > 0).all() and (pr <= 1).all()


@pytest.mark.parametrize("classes", [21, 64, 1000])            # dword loads; 16-byte loads; 16-byte loads over eight chunks
@pytest.mark.parametrize("offset", [0, 4])                     # at a 4-byte offset every class count takes the dword path
def test_kernel_equals_argmax(pkg, ctx, classes, offset):
    _equal_to_argmax(ctx, _logits(3, 5, 7, classes, seed=classes + offset), 37, 61, "classes %d offset %d" % (classes, offset), offset=offset)
    _equal_to_argmax(ctx, _logits(1, 7, 7, classes, seed=classes + offset + 1), 30, 28, "short chunk, classes %d offset %d" % (classes, offset),
                     offset=offset)


WINDOWS = [((0, 0, 224, 160), 37, 61),                 # the full window
           ((64, 32, 96, 96), 39, 41),                 # reads samples outside the rectangle
           ((9, 11, 180, 120), 67, 50)]                # an odd ratio: some waves cross a coarse row and some do not


@pytest.mark.parametrize("classes", [21, 64])
@pytest.mark.parametrize("win", WINDOWS)
def test_kernel_window(pkg, ctx, win, classes):
    rect, H, W = win
    x = _logits(2, 5, 7, classes, seed=H + classes)
    window = (160, 224, rect)
    _equal_to_argmax(ctx, x, H, W, "window %s classes %d" % (rect, classes), window=window)
    _, _, _, pr = _check(ctx, x, H, W, "window %s classes %d" % (rect, classes), window=window)
    if rect == (0, 0, 224, 160):                       # the full window is the plain rule: the plain kernel's prob bits
        assert np.array_equal(_bits(pr), _bits(_run(ctx, x, H, W)[2]))


H5, W7, R5, C7 = 5, 7, 160, 224
FULL = (0, 0, C7, R5)
RAGGED_PLAIN = [(37, 61), (40, 56), (20, 28), (100, 30), (37, 61)]
RAGGED_WINDOW = [(37, 61, FULL), (20, 28, FULL), (40, 56, (56, 0, 112, 160)), (100, 30, (9, 11, 180, 120)), (40, 56, (56, 0, 112, 160))]


def _ragged_run(ctx, rd, d_x, total, min_prob=0.0, ignore=0):
    outs = ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, SC_FILL, np.float32)), \
        ctx.to_device(np.full(total, PR_FILL, np.float32))
    rd.run_softmax(outs[0].ptr, outs[2].ptr, outs[1].ptr, d_x.ptr, min_prob, ignore)
    ctx.sync()
    got = outs[0].download((total,), np.int32), outs[1].download((total,), np.float32), outs[2].download((total,), np.float32)
    for b in outs:
        b.free()
    return got


def _ragged_compare(ctx, x, items, offs, got, window):
    """every image equal to the uniform softmax call on it alone (itself checked against the reference), gaps untouched"""
    lab, sc, pr = got
    touched = np.zeros(lab.size, bool)
    for i, (it, off) in enumerate(zip(items, offs)):
        H, W = it[0], it[1]
        win = (R5, C7, it[2]) if window else None
        _check(ctx, x[i:i + 1], H, W, "ragged item %d alone" % i, window=win)
        one = _run(ctx, x[i:i + 1], H, W, window=win)
        for name, a, b in zip(("labels", "scores", "probabilities"), (lab, sc, pr), one):
            assert np.array_equal(_bits(a[off:off + H * W]), _bits(b.ravel())), "item %d %s" % (i, name)
        touched[off:off + H * W] = True
    assert (lab[~touched] == LAB_FILL).all() and (sc[~touched] == SC_FILL).all() and (pr[~touched] == PR_FILL).all(), "written between or behind the maps"


def test_ragged_after_either_set_and_a_replay_after_a_later_set(pkg, ctx):
    classes = 21
    x = _logits(5, H5, W7, classes, seed=79)
    d_x = ctx.to_device(x)
    rd = pkg.RaggedReadout(ctx, 5)
    lib = ctx.lib
    # a plain set: the plain kernel
    offs, total = _ragged_layout(RAGGED_PLAIN, order=(3, 0, 4, 2, 1))
    rd.set(H5, W7, classes, [(o, H, W) for o, (H, W) in zip(offs, RAGGED_PLAIN)])
    got = _ragged_run(ctx, rd, d_x, total)
    _ragged_compare(ctx, x, RAGGED_PLAIN, offs, got, window=False)
    # the same launch captured as one kernel node and replayed: the same bits
    g = C.c_void_p()
    cap = ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, SC_FILL, np.float32)), ctx.to_device(np.full(total, PR_FILL, np.float32))
    assert lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = lib.mbn_resample_softmax_ragged_f32(rd.h, cap[0].ptr, cap[2].ptr, cap[1].ptr, d_x.ptr, 0.0, 0, None)
    assert lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert (cap[0].download((total,), np.int32) == LAB_FILL).all(), "the captured call ran"
    assert lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    for a, b in zip(cap, got):
        assert np.array_equal(_bits(a.download((total,), b.dtype)), _bits(b))
    # a window set on the same handle: the window kernel
    woffs, wtotal = _ragged_layout([(H, W) for H, W, _ in RAGGED_WINDOW], order=(1, 4, 0, 3, 2), gap=6)
    rd.set_window(H5, W7, classes, R5, C7, [(o, H, W, rect) for o, (H, W, rect) in zip(woffs, RAGGED_WINDOW)])
    wgot = _ragged_run(ctx, rd, d_x, wtotal)
    _ragged_compare(ctx, x, RAGGED_WINDOW, woffs, wgot, window=True)
    # the launch captured under the plain set, replayed after the window set, writes nothing
    for b, fill in zip(cap, (LAB_FILL, SC_FILL, PR_FILL)):
        b.upload(np.full(total, fill, np.int32 if fill == LAB_FILL else np.float32))
    assert lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert (cap[0].download((total,), np.int32) == LAB_FILL).all() and (cap[1].download((total,), np.float32) == SC_FILL).all() \
        and (cap[2].download((total,), np.float32) == PR_FILL).all(), "a replay after a later set wrote"
    assert lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    # threshold and NULL prob through the ragged launch: the plain call's thresholded labels
    lab_t = _ragged_run(ctx, rd, d_x, wtotal, min_prob=0.4, ignore=-3)
    assert np.array_equal(lab_t[0], np.where((wgot[2] < np.float32(0.4)) & (wgot[0] != LAB_FILL), -3, wgot[0])) and np.array_equal(_bits(lab_t[2]), _bits(wgot[2]))
    assert (lab_t[0] == -3).any() and (lab_t[0] >= 0).any()
    d_lab = ctx.to_device(np.full(wtotal, LAB_FILL, np.int32))
    rd.run_softmax(d_lab.ptr, None, None, d_x.ptr, 0.4, -3)
    ctx.sync()
    assert np.array_equal(d_lab.download((wtotal,), np.int32), lab_t[0])
    # argument errors of the launch: nothing is written
    d_lab.upload(np.full(wtotal, LAB_FILL, np.int32))
    d_pr = ctx.to_device(np.full(wtotal, PR_FILL, np.float32))
    call = lambda l, p, s, q, m: lib.mbn_resample_softmax_ragged_f32(rd.h, l, p, s, q, m, 0, None)
    assert call(d_lab.ptr, None, None, d_x.ptr, 0.0) == pkg.EINVAL
    assert call(d_lab.ptr, d_pr.ptr, None, d_x.ptr, 1.5) == pkg.EINVAL
    assert call(d_lab.ptr, d_pr.ptr, None, d_x.ptr, float("nan")) == pkg.EINVAL
    assert call(None, d_pr.ptr, None, d_x.ptr, 0.0) == pkg.EINVAL
    assert call(d_lab.ptr, d_pr.ptr + 2, None, d_x.ptr, 0.0) == pkg.EINVAL
    small = ctx.to_device(np.zeros(8, np.float32))
    assert call(d_lab.ptr, small.ptr, None, d_x.ptr, 0.0) == pkg.EINVAL      # an 8-element tracked prob buffer: the span check
    fresh = pkg.RaggedReadout(ctx, 2)
    assert lib.mbn_resample_softmax_ragged_f32(fresh.h, d_lab.ptr, d_pr.ptr, None, d_x.ptr, 0.0, 0, None) == pkg.EINVAL      # no set yet
    ctx.sync()
    assert (d_lab.download((wtotal,), np.int32) == LAB_FILL).all() and (d_pr.download((wtotal,), np.float32) == PR_FILL).all()
    fresh.close()
    rd.close()
    for b in (d_x, d_lab, d_pr, small) + cap:
        b.free()


# ------------------------------------------------------------------------------------------------------------------------ threshold

@pytest.mark.parametrize("case", P.THRESHOLD_CASES)
def test_kernel_threshold(pkg, ctx, case):
    n, h, w, classes, H, W, seed, sigma, min_prob = case
    x = P.threshold_input(case)
    ignore = -9
    lab0, sc0, pr0 = _run(ctx, x, H, W)                                                      # min_prob = 0
    lab_a, sc_a, _ = _run(ctx, x, H, W, argmax=True)
    assert np.array_equal(lab0, lab_a) and np.array_equal(_bits(sc0), _bits(sc_a)), "min_prob = 0 is the argmax call's labels"
    lab, sc, pr = _run(ctx, x, H, W, min_prob=min_prob, ignore=ignore)
    assert np.array_equal(_bits(pr), _bits(pr0)) and np.array_equal(_bits(sc), _bits(sc0)), "prob and score are written unchanged"
    assert np.array_equal(lab, np.where(pr < np.float32(min_prob), ignore, lab_a)), "ignore_label exactly where the stored prob < min_prob"
    want_lab, _, want_pr = P.resample_softmax(x, H, W)                                       # the pairs the CPU test clears: the reference's map
    assert np.array_equal(lab, P.threshold(want_lab, want_pr, min_prob, ignore))
    assert (lab == ignore).any() and (lab != ignore).any()
    lab_n, _, _ = _run(ctx, x, H, W, with_score=False, with_prob=False, min_prob=min_prob, ignore=ignore)      # thresholded labels alone
    assert np.array_equal(lab_n, lab)
    lab_1, _, _ = _run(ctx, x, H, W, min_prob=1.0, ignore=2 ** 31 - 1)                       # every pixel below 1 goes; any int32 is a label
    assert np.array_equal(lab_1, np.where(pr < np.float32(1.0), 2 ** 31 - 1, lab_a))


def test_kernel_threshold_window(pkg, ctx):
    x = P.threshold_input(P.THRESHOLD_CASES[0])
    window = (R5, C7, (64, 32, 96, 96))
    lab_a, _, _ = _run(ctx, x, 39, 41, window=window, argmax=True)
    lab, _, pr = _run(ctx, x, 39, 41, window=window, min_prob=0.5, ignore=255)
    assert np.array_equal(lab, np.where(pr < np.float32(0.5), 255, lab_a)) and (lab == 255).any() and (lab != 255).any()
    lab_n, _, _ = _run(ctx, x, 39, 41, window=window, with_prob=False, min_prob=0.5, ignore=255)
    assert np.array_equal(lab_n, lab)


def test_kernel_argument_errors(pkg, ctx):
    x = ctx.to_device(np.zeros(2 * 2 * 21, np.float32))
    fill = np.full(16 * 16, LAB_FILL, np.int32)
    lab, sc, pr = ctx.to_device(fill), ctx.to_device(fill.astype(np.float32)), ctx.to_device(fill.astype(np.float32))
    lib = ctx.lib
    soft = lambda l, p, s, q, *a, m=0.0: lib.mbn_resample_softmax_f32(ctx.h, l, p, s, q, *a, m, 0, None)
    arg = lambda l, s, q, *a: lib.mbn_resample_argmax_f32(ctx.h, l, s, q, *a, None)
    ok = (1, 2, 2, 21, 16, 16)
    # its own arguments
    assert soft(lab.ptr, None, sc.ptr, x.ptr, *ok) == pkg.EINVAL                            # neither a map nor a threshold
    for bad in (float("nan"), -0.1, 1.5):
        assert soft(lab.ptr, pr.ptr, sc.ptr, x.ptr, *ok, m=bad) == pkg.EINVAL, bad
        assert soft(lab.ptr, None, sc.ptr, x.ptr, *ok, m=bad) == pkg.EINVAL, bad
    assert soft(lab.ptr, pr.ptr + 2, sc.ptr, x.ptr, *ok) == pkg.EINVAL                       # prob off 4 bytes
    assert soft(None, pr.ptr, sc.ptr, x.ptr, *ok) == pkg.EINVAL
    assert soft(lab.ptr, pr.ptr, sc.ptr, None, *ok) == pkg.EINVAL
    # the envelope and the spans: the argmax call's status on the same shape
    shapes = [(1, 2, 2, 21, 7, 16), (1, 2, 2, 21, 16, 7), (1, 2, 2, 21, 16385, 16), (0, 2, 2, 21, 16, 16), (1, 0, 2, 21, 16, 16), (1, 2, 2, 0, 16, 16),
              (1, 2, 2, 21, 16, -1), (65536, 2, 2, 21, 16, 16), (1, 2, 2, 21, 16, 17)]
    for s in shapes:
        want = arg(lab.ptr, sc.ptr, x.ptr, *s)
        assert want != pkg.OK and soft(lab.ptr, pr.ptr, sc.ptr, x.ptr, *s) == want, s
        assert soft(lab.ptr, None, sc.ptr, x.ptr, *s, m=0.5) == want, s
    assert arg(lab.ptr, sc.ptr, x.ptr + 2, 1, 2, 2, 20, 16, 16) == soft(lab.ptr, pr.ptr, sc.ptr, x.ptr + 2, 1, 2, 2, 20, 16, 16) == pkg.EINVAL
    small = ctx.to_device(np.zeros(8, np.float32))
    assert soft(lab.ptr, small.ptr, sc.ptr, x.ptr, *ok) == pkg.EINVAL                        # the span check of prob
    # the window call
    rect_t = lambda *v: (C.c_int32 * 4)(*v)
    wsoft = lambda l, p, s, q, n, h, w, c, R, Cc, rect, H, W, m=0.0: lib.mbn_resample_softmax_window_f32(ctx.h, l, p, s, q, n, h, w, c, R, Cc, rect, H, W, m, 0, None)
    warg = lambda l, s, q, n, h, w, c, R, Cc, rect, H, W: lib.mbn_resample_argmax_window_f32(ctx.h, l, s, q, n, h, w, c, R, Cc, rect, H, W, None)
    full = rect_t(0, 0, 64, 64)
    assert wsoft(lab.ptr, None, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, full, 16, 16) == pkg.EINVAL
    assert wsoft(lab.ptr, pr.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, full, 16, 16, 1.5) == pkg.EINVAL
    assert wsoft(lab.ptr, pr.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64, 64, None, 16, 16) == pkg.EINVAL
    for a in [(1, 2, 2, 21, 64, 64, full, 7, 16), (1, 2, 2, 21, 64, 64, rect_t(0, 0, 64, 57), 7, 16), (1, 2, 2, 21, 16385, 64, full, 16, 16),
              (1, 2, 2, 21, 64, 64, rect_t(1, 0, 64, 64), 16, 16), (1, 2, 2, 21, 1, 64, rect_t(0, 0, 1, 1), 16, 16), (1, 2, 2, 21, 64, 64, full, 16, 17)]:
        want = warg(lab.ptr, sc.ptr, x.ptr, *a)
        assert want != pkg.OK and wsoft(lab.ptr, pr.ptr, sc.ptr, x.ptr, *a) == want, a[:6]
    ctx.sync()
    for b in (lab, sc, pr):
        assert np.array_equal(b.download(fill.shape, np.int32 if b is lab else np.float32), fill), "nothing may have been launched"
    assert soft(lab.ptr, pr.ptr, None, x.ptr, *ok) == pkg.OK                                 # score NULL; all-zero logits: label 0, prob 1 / 21
    assert wsoft(sc.ptr, None, None, x.ptr, 1, 2, 2, 21, 64, 64, rect_t(0, 0, 64, 56), 7, 16, 0.5) == pkg.OK      # the ratio exactly, labels alone
    ctx.sync()
    assert (lab.download(fill.shape, np.int32) == 0).all() and (pr.download(fill.shape, np.float32) == np.float32(1 / 21.0)).all()
    got = sc.download(fill.shape, np.int32)
    assert (got[:7 * 16] == 0).all() and (got[7 * 16:] == fill.astype(np.float32).view(np.int32)[7 * 16:]).all()
    for b in (x, lab, sc, pr, small):
        b.free()


# ------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS, BATCH = 0.25, 21, 64, 64, 3
SOURCES = [(75, 130), (64, 64), (120, 100)]


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _i32(v):
    return (C.c_int32 * len(v))(*v)


@pytest.mark.parametrize("dtype,os_", [("f32", 32), ("f32", 16), ("f32", 8), ("bf16", 32), ("bf16", 16), ("bf16", 8), ("i8", 32)])
def test_net_segment_prob(pkg, ctx, tmp_path, dtype, os_):
    n = BATCH
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, os_)
    h, w = ROWS // os_, COLS // os_
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    dt = {"f32": pkg.DT_F32, "bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype]
    if dt != pkg.DT_F32:
        net.set_dtype(dt)
    lib = ctx.lib
    tag = "%s os %d" % (dtype, os_)
    d_dense = ctx.alloc(n * h * w * CLASSES * 4)
    bufs = [d_dense]

    def outputs(total):
        trio = ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, PR_FILL, np.float32)), \
            ctx.to_device(np.full(total, LAB_FILL, np.int32))
        bufs.extend(trio)
        return trio

    def dense_of(images_ptr):
        net.forward_dense(images_ptr, d_dense.ptr, n)
        ctx.sync()
        dense = d_dense.download((n, h, w, CLASSES), np.float32)
        assert np.isfinite(dense).all() and dense.std() > 0
        return dense

    def compare(what, lab, pr, want, lab_argmax):
        want_lab, _, want_pr = want
        assert np.array_equal(lab, want_lab.ravel()), "%s %s: %d labels differ from the reference" % (tag, what, int((lab != want_lab.ravel()).sum()))
        _prob_check(pr.reshape(want_pr.shape), want_pr, CLASSES, "%s %s" % (tag, what))
        assert np.array_equal(lab, lab_argmax), "%s %s: labels differ from the argmax path's" % (tag, what)

    # ---- segment_prob_to: float images of the plan's size, to 75 x 130 and to the input size itself
    H, W = SOURCES[0]
    d_in = ctx.to_device(_images(n, ROWS, COLS, 21))
    bufs.append(d_in)
    npix = n * H * W
    d_lab, d_pr, d_arg = outputs(npix + TAIL)
    assert lib.mbn_net_segment_prob_to(net.h, d_in.ptr, n, 4 * h - 1, W, d_lab.ptr, d_pr.ptr, 0.0, 0) == pkg.EUNSUPPORTED
    assert lib.mbn_net_segment_prob_to(net.h, d_in.ptr, n, H, W, d_lab.ptr, d_pr.ptr, 1.5, 0) == pkg.EINVAL
    assert lib.mbn_net_segment_prob_to(net.h, d_in.ptr, n, H, W, d_lab.ptr, None, 0.0, 0) == pkg.EINVAL
    assert lib.mbn_net_segment_prob_to(net.h, d_in.ptr, n + 1, H, W, d_lab.ptr, d_pr.ptr, 0.0, 0) == pkg.EINVAL
    ctx.sync()
    assert (d_lab.download((npix + TAIL,), np.int32) == LAB_FILL).all() and (d_pr.download((npix + TAIL,), np.float32) == PR_FILL).all()
    dense = dense_of(d_in.ptr)
    net.segment_prob_to(d_in.ptr, n, H, W, d_lab.ptr, d_pr.ptr)                              # the net is usable after the refusals
    net.segment_to(d_in.ptr, n, H, W, d_arg.ptr)
    ctx.sync()
    lab, pr, arg = d_lab.download((npix + TAIL,), np.int32), d_pr.download((npix + TAIL,), np.float32), d_arg.download((npix + TAIL,), np.int32)
    assert (lab[npix:] == LAB_FILL).all() and (pr[npix:] == PR_FILL).all()
    compare("segment_prob_to", lab[:npix], pr[:npix], P.resample_softmax(dense, H, W), arg[:npix])
    npix = n * ROWS * COLS
    d_lab, d_pr, d_arg = outputs(npix)
    net.segment_prob_to(d_in.ptr, n, ROWS, COLS, d_lab.ptr, d_pr.ptr)
    net.segment(d_in.ptr, n, d_arg.ptr)                                                      # the integer-factor kernel
    ctx.sync()
    compare("segment_prob_to at the input size", d_lab.download((npix,), np.int32), d_pr.download((npix,), np.float32),
            P.resample_softmax(dense, ROWS, COLS), d_arg.download((npix,), np.int32))
    # ---- segment_prob_fit: uniform uint8 sources, stretch and pad
    rng = np.random.default_rng(31)
    sh, sw = SOURCES[0]
    d_src = ctx.to_device(rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8))
    bufs.append(d_src)
    npix = n * sh * sw
    d_lab, d_pr, d_arg = outputs(npix + TAIL)
    assert lib.mbn_net_segment_prob_fit(net.h, d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr, d_pr.ptr, 0.0, 0) == pkg.EINVAL      # no uint8 images yet
    net.set_input_u8(True)
    assert lib.mbn_net_segment_prob_fit(net.h, d_src.ptr, n, sh, sw, pkg.FIT_CROP, d_lab.ptr, d_pr.ptr, 0.0, 0) == pkg.EUNSUPPORTED
    assert lib.mbn_net_segment_prob_fit(net.h, d_src.ptr, n, sh, sw, 7, d_lab.ptr, d_pr.ptr, 0.0, 0) == pkg.EINVAL
    assert lib.mbn_net_segment_prob_fit(net.h, d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr, d_pr.ptr, float("nan"), 0) == pkg.EINVAL
    assert lib.mbn_net_segment_prob_fit(net.h, d_src.ptr, n, 4 * h - 1, 4 * w - 1, pkg.FIT_PAD, d_lab.ptr, d_pr.ptr, 0.0, 0) == pkg.EUNSUPPORTED
    ctx.sync()
    assert (d_lab.download((npix + TAIL,), np.int32) == LAB_FILL).all() and (d_pr.download((npix + TAIL,), np.float32) == PR_FILL).all()
    for fit in (pkg.FIT_STRETCH, pkg.FIT_PAD):
        dense = dense_of(net.resize_input(d_src.ptr, n, sh, sw, fit=fit))
        net.segment_prob_fit(d_src.ptr, n, sh, sw, fit, d_lab.ptr, d_pr.ptr)
        net.segment_fit(d_src.ptr, n, sh, sw, fit, d_arg.ptr)
        ctx.sync()
        lab, pr, arg = d_lab.download((npix + TAIL,), np.int32), d_pr.download((npix + TAIL,), np.float32), d_arg.download((npix + TAIL,), np.int32)
        assert (lab[npix:] == LAB_FILL).all() and (pr[npix:] == PR_FILL).all()
        want = P.resample_softmax(dense, sh, sw) if fit == pkg.FIT_STRETCH else \
            P.resample_softmax_window(dense, ROWS, COLS, tuple(pkg.fit_pad(sh, sw, ROWS, COLS)), sh, sw)
        compare("segment_prob_fit %d" % fit, lab[:npix], pr[:npix], want, arg[:npix])
    # the threshold through the net: exactly the pixels whose stored prob is below it
    cut = float(np.median(pr[:npix]))
    net.segment_prob_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr, None, cut, 255)
    ctx.sync()
    lab_t = d_lab.download((npix,), np.int32)
    assert np.array_equal(lab_t, np.where(pr[:npix] < np.float32(cut), 255, lab[:npix])) and (lab_t == 255).any() and (lab_t != 255).any()
    # ---- segment_prob_images_fit: three sources of their own sizes
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in SOURCES]
    src_offs, at = [], 0
    for img in images:
        src_offs.append(at)
        at += img.size
    d_srcs = ctx.to_device(np.concatenate([img.ravel() for img in images]))
    bufs.append(d_srcs)
    rows, cols = [s[0] for s in SOURCES], [s[1] for s in SOURCES]
    dst, total = _ragged_layout(SOURCES, order=(2, 0, 1), gap=7)
    d_rlab, d_rpr, d_rarg = outputs(total)
    args = lambda r, c, fit, m=0.0: (net.h, d_srcs.ptr, _i64(src_offs), _i32(r), _i32(c), n, fit, d_rlab.ptr, _i64(dst), d_rpr.ptr, m, 0)
    assert lib.mbn_net_segment_prob_images_fit(*args(rows, cols, pkg.FIT_CROP)) == pkg.EUNSUPPORTED
    assert lib.mbn_net_segment_prob_images_fit(*args(rows, cols, 7)) == pkg.EINVAL
    assert lib.mbn_net_segment_prob_images_fit(*args(rows, cols, pkg.FIT_PAD, -0.1)) == pkg.EINVAL
    assert lib.mbn_net_segment_prob_images_fit(*args([4 * h - 1] + rows[1:], [4 * w - 1] + cols[1:], pkg.FIT_PAD)) == pkg.EUNSUPPORTED
    ctx.sync()
    assert (d_rlab.download((total,), np.int32) == LAB_FILL).all() and (d_rpr.download((total,), np.float32) == PR_FILL).all(), "a refused call may not write"
    for fit in (pkg.FIT_STRETCH, pkg.FIT_PAD):
        dense = dense_of(net.resize_inputs(d_srcs.ptr, src_offs, rows, cols, fit=fit))
        net.segment_prob_images_fit(d_srcs.ptr, src_offs, rows, cols, fit, d_rlab.ptr, dst, d_rpr.ptr)
        net.segment_images_fit(d_srcs.ptr, src_offs, rows, cols, fit, d_rarg.ptr, dst)
        ctx.sync()
        lab, pr, arg = d_rlab.download((total,), np.int32), d_rpr.download((total,), np.float32), d_rarg.download((total,), np.int32)
        touched = np.zeros(total, bool)
        for i, ((ih, iw), off) in enumerate(zip(SOURCES, dst)):
            want = P.resample_softmax(dense[i:i + 1], ih, iw) if fit == pkg.FIT_STRETCH else \
                P.resample_softmax_window(dense[i:i + 1], ROWS, COLS, tuple(pkg.fit_pad(ih, iw, ROWS, COLS)), ih, iw)
            sl = slice(off, off + ih * iw)
            compare("segment_prob_images_fit %d image %d" % (fit, i), lab[sl], pr[sl], want, arg[sl])
            touched[sl] = True
        assert (lab[~touched] == LAB_FILL).all() and (pr[~touched] == PR_FILL).all(), "written between or behind the maps"
    net.destroy()
    for b in bufs:
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def _pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    assert m, raw[:32]
    width, height, maxval = (int(g) for g in m.groups())
    return np.frombuffer(raw[m.end():], ">u2" if maxval > 255 else np.uint8).astype(np.int32).reshape(height, width), maxval


@pytest.mark.parametrize("fit", ["stretch", "pad"])
def test_c_host_segment_confidence(pkg, ctx, tmp_path, fit):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    seed, alpha, os_, sh, sw, rows, cols = 3, 0.5, 16, 75, 130, 64, 96
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, out, conf = str(tmp_path / "a.ppm"), str(tmp_path / "out.pgm"), str(tmp_path / "conf.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", str(seed), "--alpha", str(alpha), "--res", "%dx%d" % (rows, cols), "--output-stride", str(os_), "--ppm", ppm]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
    # bad combinations: usage status 2 and nothing written
    for extra in (["--segment-confidence", conf],                                                                  # the default fit is the crop
                  ["--fit", fit, "--segment-source", out, "--min-confidence", "0.5"],                              # no --ignore-label
                  ["--fit", fit, "--segment-source", out, "--ignore-label", "255"],                                # no --min-confidence
                  ["--fit", fit, "--segment-confidence", conf, "--min-confidence", "0.5", "--ignore-label", "255"],    # no label map to apply it to
                  ["--fit", fit, "--segment-source", out, "--min-confidence", "1.5", "--ignore-label", "255"],
                  ["--fit", fit, "--segment-source", out, "--min-confidence", "0.5", "--ignore-label", "-1"]):
        r = run(extra)
        assert r.returncode == 2 and not os.path.exists(out) and not os.path.exists(conf), (extra, r.stdout + r.stderr)
    # the same through the mirror
    classes = 1000                                      # the host's synthetic weights
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(rows, cols), lib=pkg.load(), output_stride=os_)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 1)
    net.set_input_u8(True)
    d_src, d_lab, d_pr = ctx.to_device(src), ctx.alloc(sh * sw * 4), ctx.alloc(sh * sw * 4)
    net.segment_prob_fit(d_src.ptr, 1, sh, sw, pkg.FIT_STRETCH if fit == "stretch" else pkg.FIT_PAD, d_lab.ptr, d_pr.ptr)
    ctx.sync()
    want_lab, want_pr = d_lab.download((sh, sw), np.int32), d_pr.download((sh, sw), np.float32)
    net.destroy()
    for b in (d_src, d_lab, d_pr):
        b.free()
    hw.free()
    assert len(np.unique(want_lab)) > 1 and want_pr.std() > 0
    want_bytes = np.floor(want_pr.astype(np.float64) * 255.0 + 0.5).astype(np.int32)
    # --segment-confidence beside --segment-source, and alone
    r = run(["--fit", fit, "--segment-source", out, "--segment-confidence", conf])
    assert r.returncode == 0, r.stdout + r.stderr
    got, maxval = _pgm(conf)
    assert maxval == 255 and got.shape == (sh, sw) and np.array_equal(got, want_bytes), "%d confidence bytes differ" % int((got != want_bytes).sum())
    labels, maxval = _pgm(out)
    assert maxval == classes - 1 and np.array_equal(labels, want_lab)
    os.remove(conf)
    r = run(["--fit", fit, "--segment-confidence", conf])
    assert r.returncode == 0 and np.array_equal(_pgm(conf)[0], want_bytes), r.stdout + r.stderr
    # --min-confidence: 0 (nothing is replaced), 0.5, and the median of the map so that both sides are populated
    for cut in (0.0, 0.5, float(np.median(want_pr))):
        r = run(["--fit", fit, "--segment-source", out, "--min-confidence", "%.9g" % cut, "--ignore-label", "255"])
        assert r.returncode == 0, r.stdout + r.stderr
        got, maxval = _pgm(out)
        under = want_pr < np.float32(cut)
        assert maxval == classes - 1 and np.array_equal(got, np.where(under, 255, want_lab)), (cut, int(under.sum()))
    assert under.any() and not under.all()
    r = run(["--fit", fit, "--segment-source", out, "--min-confidence", "0.5", "--ignore-label", "2000"])      # a label beyond the classes widens maxval
    assert r.returncode == 0 and _pgm(out)[1] == 2000, r.stdout + r.stderr
