"""Segment with test-time augmentation on the GPU. mbn_resample_ensemble_f32 alone: labels and score bits equal to tests/dense_ensemble_ref.py
(the normative arithmetic) on the smallest shapes that reach each way of going wrong: every view count's kernel, mirrored and plain views with
rectangles of their own, both staging paths, the largest staging, the order of the sum, adversarial values in one view only, the softmax form
within dense_prob_ref's bound, argument errors, nothing written outside the maps. The view resizer against Pillow's recorded canvases
(tests/golden/resize_pillow_views.npz). The net runner: segment_views_fit against the reference applied to forward_dense of resize_views' own
staging. The C host's --tta-scales / --tta-flip.

Planning CU counts: the kernel is one workgroup per output tile and not persistent; nothing in it or in its launch depends on the number of
compute units, so there is no planning-CU sweep here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_ensemble_ref as E
import dense_prob_ref as P
import dense_window_ref
import resize_filters_ref as R
from test_dense_any_gpu import LAB_FILL, SC_FILL, TAIL, _logits
from test_dense_ensemble_cpu import fixture, order_input, view_canvas_ref
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

PR_FILL = -3.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _views_logits(K, n, h, w, classes, seed):
    return np.stack([_logits(n, h, w, classes, seed=seed + 17 * k) for k in range(K)])


def _run(ctx, x, R_, Cc, views, H, W, offset=0, with_score=True, with_prob=False, min_prob=0.0, ignore=0):
    """mbn_resample_ensemble_f32 on x [K][n][h][w][classes] (uploaded `offset` bytes into its allocation): (labels, score or None, prob or None).
    The output buffers carry a sentinel pattern and TAIL more elements, which must come back unchanged."""
    K, n, h, w, classes = x.shape
    assert K == len(views)
    d_x = ctx.to_device(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
    npix = n * H * W
    d_lab = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32))
    d_sc = ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32)) if with_score else None
    d_pr = ctx.to_device(np.full(npix + TAIL, PR_FILL, np.float32)) if with_prob else None
    ctx.resample_ensemble(d_lab.ptr, d_pr.ptr if d_pr else None, d_sc.ptr if d_sc else None, d_x.ptr + offset, n, h, w, classes, R_, Cc, views, H, W,
                          min_prob, ignore)
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


def _check(ctx, x, R_, Cc, views, H, W, what, **kw):
    want_lab, want_sc, want_pr = E.ensemble(x, R_, Cc, views, H, W)
    lab, sc, pr = _run(ctx, x, R_, Cc, views, H, W, **kw)
    bad = int((lab != want_lab).sum())
    assert bad == 0, "%s: %d of %d labels differ from dense_ensemble_ref" % (what, bad, lab.size)
    if sc is not None:
        bad = int((_bits(sc) != _bits(want_sc)).sum())
        assert bad == 0, "%s: %d of %d score bit patterns differ from dense_ensemble_ref" % (what, bad, sc.size)
    if pr is not None:
        _prob_check(pr, want_pr, x.shape[4], what)
    return want_lab, want_sc, want_pr


# ----------------------------------------------------------------------------------------------------------------------- geometry

def _view_sets(h, w):
    """name -> views (x, y, iw, ih, mirror) of a 32 h x 32 w input; the rectangles of a set are distinct, so the per-view footprints differ"""
    R_, Cc = 32 * h, 32 * w
    full = (0, 0, Cc, R_)
    three = [full + (0,), (Cc // 8, R_ // 8, 3 * Cc // 4, 3 * R_ // 4, 0), (Cc // 4, R_ // 4, Cc // 2, R_ // 2, 1)]
    mixed = three + [(7, 5, Cc - 20, R_ - 9, 1), (Cc // 2 + 5, 3, 1, R_ - 7, 0), (0, 0, Cc - 21, R_ - 13, 1), (21, 13, Cc - 21, R_ - 13, 0),
                     (Cc // 4 + 3, R_ // 4 + 1, 20, 17, 1)]
    return {"K1 full": [full + (0,)], "K2 full + mirrored": [full + (0,), full + (1,)], "K3": three, "K8 mixed": mixed}


OUTPUTS = ["37x61", "45x70", "minimum ratio"]


@pytest.mark.parametrize("classes", [21, 64])                  # 21: dword loads, a padded last group; 64: 16-byte loads
@pytest.mark.parametrize("out", OUTPUTS)
@pytest.mark.parametrize("name", list(_view_sets(2, 3)))
@pytest.mark.parametrize("hw", [(2, 3), (5, 7)])
def test_kernel_geometry(pkg, ctx, hw, name, out, classes):
    h, w = hw
    views = _view_sets(h, w)[name]
    H, W = {"37x61": (37, 61), "45x70": (45, 70), "minimum ratio": (4 * h, 4 * w)}[out]
    R_, Cc = 32 * h, 32 * w
    assert pkg.resample_ensemble_envelope(2, h, w, classes, R_, Cc, views, H, W) == pkg.OK
    x = _views_logits(len(views), 2, h, w, classes, seed=h * 1000 + w * 100 + H + W)
    _check(ctx, x, R_, Cc, views, H, W, "%s %s %s classes %d" % (hw, name, out, classes), with_prob=classes == 21)


@pytest.mark.parametrize("K", [4, 5, 6, 7])                    # the view counts the sets above leave out: every K has kernels of its own
def test_kernel_every_view_count(pkg, ctx, K):
    h, w, classes, H, W = 5, 7, 21, 37, 61
    views = _view_sets(h, w)["K8 mixed"][:K]
    _check(ctx, _views_logits(K, 1, h, w, classes, seed=K), 32 * h, 32 * w, views, H, W, "K = %d" % K, with_prob=True)
    _check(ctx, _views_logits(K, 1, h, w, 64, seed=K + 50), 32 * h, 32 * w, views, H, W, "K = %d, 16-byte loads" % K)


@pytest.mark.parametrize("classes", [21, 64])
def test_kernel_largest_staging(pkg, ctx, classes):
    """Eight views of 160 x 224-pixel rectangles (5 x 7 samples' worth) of a 10 x 14 map to 20 x 28: the ratio is exactly 4 in every view and the
    launch stages 8 x 10 x 10 vectors of 16 classes, 64 000 bytes."""
    h, w, R_, Cc, H, W = 10, 14, 320, 448, 20, 28
    views = [(32 * (k % 4) * 2, 32 * (k // 4) * 5, 224, 160, k & 1) for k in range(8)]
    l = pkg.resample_ensemble_plan(h, w, R_, Cc, views, H, W)
    assert (l.fy, l.fx, l.ch) == (10, 10, 16) and l.lds_bytes == 64000
    _check(ctx, _views_logits(8, 2, h, w, classes, seed=classes), R_, Cc, views, H, W, "largest staging, classes %d" % classes, with_prob=True)


@pytest.mark.parametrize("classes", [1, 65, 1001])             # one class; an odd count over a 16-byte chunk; many chunks and a short last one
def test_kernel_class_counts(pkg, ctx, classes):
    h, w = 2, 3
    views = _view_sets(h, w)["K3"]
    _check(ctx, _views_logits(3, 1, h, w, classes, seed=classes), 64, 96, views, 37, 61, "classes %d" % classes, with_prob=True)


@pytest.mark.parametrize("classes", [21, 64])
def test_kernel_logits_at_a_4_byte_offset(pkg, ctx, classes):
    views = _view_sets(2, 3)["K3"]
    _check(ctx, _views_logits(3, 2, 2, 3, classes, seed=9), 64, 96, views, 11, 17, "offset 4, classes %d" % classes, offset=4)


def test_kernel_score_null(pkg, ctx):
    views = _view_sets(2, 3)["K2 full + mirrored"]
    _check(ctx, _views_logits(2, 2, 2, 3, 21, seed=11), 64, 96, views, 13, 17, "score NULL", with_score=False)
    _check(ctx, _views_logits(2, 2, 2, 3, 21, seed=12), 64, 96, views, 13, 17, "score NULL, softmax", with_score=False, with_prob=True)


# --------------------------------------------------------------------------------------------------------------- device identities

@pytest.mark.parametrize("copies", [1, 2, 4])
def test_kernel_copies_of_one_view_equal_the_window_kernel(pkg, ctx, copies):
    """on the same device buffer: K = 1 is the window read-out, and 2 or 4 copies of the view over the same logits are too (exact sums)"""
    n, h, w, classes, R_, Cc, rect, H, W = 2, 5, 7, 21, 160, 224, (9, 11, 180, 120), 67, 50
    x = _logits(n, h, w, classes, seed=copies)
    d_x = ctx.to_device(np.concatenate([x.ravel()] * copies))
    npix = n * H * W
    outs = [ctx.to_device(np.full(npix, LAB_FILL, np.int32)) for _ in range(2)] + [ctx.to_device(np.full(npix, SC_FILL, np.float32)) for _ in range(2)]
    ctx.resample_argmax_window(outs[0].ptr, outs[2].ptr, d_x.ptr, n, h, w, classes, R_, Cc, rect, H, W)
    ctx.resample_ensemble(outs[1].ptr, None, outs[3].ptr, d_x.ptr, n, h, w, classes, R_, Cc, [rect + (0,)] * copies, H, W)
    ctx.sync()
    got = [b.download((npix,), np.uint32) for b in outs]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[3])
    want_lab, want_sc = dense_window_ref.resample_argmax_window(x, R_, Cc, rect, H, W)
    assert np.array_equal(got[1].view(np.int32).reshape(want_lab.shape), want_lab) and np.array_equal(got[3], _bits(want_sc).ravel())
    for b in [d_x] + outs:
        b.free()


def test_kernel_sums_in_view_order(pkg, ctx):
    x = order_input()
    views = [(0, 0, 96, 64, 0)] * 3
    _, sc, _ = _check(ctx, x, 64, 96, views, 9, 13, "1e8, -1e8, 1")
    assert (sc == np.float32(1.0) / np.float32(3.0)).all()
    _, sc, _ = _check(ctx, np.ascontiguousarray(x[[0, 2, 1]]), 64, 96, views, 9, 13, "1e8, 1, -1e8")
    assert (sc == 0).all()


def test_kernel_adversarial_values(pkg, ctx):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    h, w, R_, Cc, H, W = 5, 7, 160, 224, 39, 41
    views = _view_sets(h, w)["K3"]
    x = _views_logits(3, 1, h, w, 65, seed=13)                  # a NaN in one view only, where the mean's winner was
    lab0, _, _ = E.ensemble(x, R_, Cc, views, H, W)
    x[1, 0, 2, 3, int(lab0[0, H // 2, W // 2])] = nan
    want_lab, want_sc, want_pr = _check(ctx, x, R_, Cc, views, H, W, "NaN in one view", with_prob=True)
    assert (want_lab != lab0).any() and np.isfinite(want_sc).all(), "a NaN sum never wins"
    x = _views_logits(3, 1, h, w, 21, seed=15)                  # +inf and -inf in one view only
    x[0, 0, 1, 2, 3] = inf
    x[2, 0, 3, 4, 7] = -inf
    _, want_sc, want_pr = _check(ctx, x, R_, Cc, views, H, W, "inf in one view", with_prob=True)
    assert (want_sc == inf).any() and (want_pr[want_sc == inf] == 0).all()
    x = _views_logits(2, 1, h, w, 21, seed=16)                  # +inf in one view and -inf in another on the same class: a NaN sum
    x[0, :, :, :, 3] = inf
    x[1, :, :, :, 3] = -inf
    want_lab, want_sc, _ = _check(ctx, x, R_, Cc, views[:2], H, W, "+inf and -inf", with_prob=True)
    assert (want_lab != 3).all() and np.isfinite(want_sc).all()
    x = np.full((2, 1, h, w, 21), nan, np.float32)              # nothing wins anywhere
    want_lab, want_sc, want_pr = _check(ctx, x, R_, Cc, views[:2], H, W, "all NaN", with_prob=True)
    assert (want_lab == 0).all() and (want_sc == -inf).all() and (want_pr == 0).all()
    x = np.zeros((3, 2, h, w, 200), np.float32)                 # equal maxima in different chunks: the lowest index wins
    x[..., 5] = x[..., 70] = x[..., 131] = 2.0
    want_lab, _, _ = _check(ctx, x, R_, Cc, views, H, W, "equal maxima")
    assert (want_lab == 5).all()
    x = np.random.default_rng(19).integers(-8, 9, (3, 2, h, w, 65)).astype(np.float32)      # integer-valued logits: ties everywhere
    _check(ctx, x, R_, Cc, views, H, W, "integer-valued logits", with_prob=True)


# ------------------------------------------------------------------------------------------------------------------------ softmax

@pytest.mark.parametrize("case", E.THRESHOLD_CASES)
def test_kernel_threshold(pkg, ctx, case):
    n, h, w, classes, views, H, W, seed, sigma, min_prob = case
    x = E.threshold_input(case)
    R_, Cc, ignore = 32 * h, 32 * w, -9
    lab_a, sc_a, _ = _run(ctx, x, R_, Cc, views, H, W)                                        # the argmax form
    lab0, sc0, pr0 = _run(ctx, x, R_, Cc, views, H, W, with_prob=True)                        # min_prob = 0
    assert np.array_equal(lab0, lab_a) and np.array_equal(_bits(sc0), _bits(sc_a)), "labels and score bits are the argmax form's"
    lab, sc, pr = _run(ctx, x, R_, Cc, views, H, W, with_prob=True, min_prob=min_prob, ignore=ignore)
    assert np.array_equal(_bits(pr), _bits(pr0)) and np.array_equal(_bits(sc), _bits(sc0)), "prob and score are written unchanged"
    assert np.array_equal(lab, np.where(pr < np.float32(min_prob), ignore, lab_a)), "ignore_label exactly where the stored prob < min_prob"
    want_lab, _, want_pr = E.ensemble(x, R_, Cc, views, H, W)
    _prob_check(pr, want_pr, classes, "threshold case")
    out = P.excluded(want_pr, min_prob, classes)
    assert out.mean() <= 0.01
    assert np.array_equal(lab[~out], P.threshold(want_lab, want_pr, min_prob, ignore)[~out])
    assert (lab == ignore).any() and (lab != ignore).any()
    lab_n, _, _ = _run(ctx, x, R_, Cc, views, H, W, with_score=False, with_prob=False, min_prob=min_prob, ignore=ignore)     # prob = NULL, min_prob > 0
    assert np.array_equal(lab_n, lab)


# ------------------------------------------------------------------------------------------------------------------------- errors

def test_kernel_argument_errors(pkg, ctx):
    x = ctx.to_device(np.zeros(3 * 2 * 2 * 21, np.float32))
    fill = np.full(16 * 16, LAB_FILL, np.int32)
    lab, sc, pr = ctx.to_device(fill), ctx.to_device(fill.astype(np.float32)), ctx.to_device(fill.astype(np.float32))
    full = (0, 0, 64, 64, 0)

    def call(l, p, s, logits, n, h, w, c, R_, Cc, views, H, W, min_prob=0.0, n_views=None):
        arr = None if views is None else pkg.views(views)
        return ctx.lib.mbn_resample_ensemble_f32(ctx.h, l, p, s, logits, n, h, w, c, R_, Cc, arr, len(views) if n_views is None else n_views, H, W,
                                                 min_prob, 0, None)

    ok = (1, 2, 2, 21, 64, 64)
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, [full] * 3, 7, 16) == pkg.EUNSUPPORTED                # under 4 x the samples
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, [full, (0, 0, 64, 57, 0)], 7, 16) == pkg.EUNSUPPORTED
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, [(0, 0, 64, 56, 0), (0, 0, 64, 57, 1)], 7, 16) == pkg.EUNSUPPORTED      # one bad view refuses the set
    assert call(None, None, sc.ptr, x.ptr, *ok, [full], 16, 16) == pkg.EINVAL
    assert call(lab.ptr, None, sc.ptr, None, *ok, [full], 16, 16) == pkg.EINVAL
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, None, 16, 16, n_views=1) == pkg.EINVAL
    for n_views in (0, 9, -1):
        assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, [full] * 9, 16, 16, n_views=n_views) == pkg.EINVAL
    for bad in [(0, 2, 2, 21, 64, 64, 16, 16), (1, 0, 2, 21, 64, 64, 16, 16), (1, 2, 0, 21, 64, 64, 16, 16), (1, 2, 2, 0, 64, 64, 16, 16),
                (1, 2, 2, 21, 0, 64, 16, 16), (1, 2, 2, 21, 64, -1, 16, 16), (1, 2, 2, 21, 64, 64, 0, 16), (1, 2, 2, 21, 64, 64, 16, -1)]:
        assert call(lab.ptr, None, sc.ptr, x.ptr, *bad[:6], [(0, 0, 1, 1, 0)], *bad[6:]) == pkg.EINVAL, bad
    for v in [(-1, 0, 64, 64, 0), (0, -1, 64, 64, 0), (0, 0, 0, 64, 0), (0, 0, 64, 0, 0), (1, 0, 64, 64, 0), (0, 1, 64, 64, 0), (0, 0, 64, 64, 2),
              (0, 0, 64, 64, -1)]:
        assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, [full, v], 16, 16) == pkg.EINVAL, v
    arr = pkg.views([full])
    arr[0].reserved[1] = 5
    assert ctx.lib.mbn_resample_ensemble_f32(ctx.h, lab.ptr, None, sc.ptr, x.ptr, *ok, arr, 1, 16, 16, 0.0, 0, None) == pkg.EINVAL
    assert call(lab.ptr, None, sc.ptr, x.ptr + 2, 1, 2, 2, 20, 64, 64, [full], 16, 16) == pkg.EINVAL      # off 4 bytes
    assert call(lab.ptr, pr.ptr + 2, sc.ptr, x.ptr, *ok, [full], 16, 16) == pkg.EINVAL
    for min_prob in (-0.5, 1.5, float("nan")):
        assert call(lab.ptr, pr.ptr, sc.ptr, x.ptr, *ok, [full], 16, 16, min_prob=min_prob) == pkg.EINVAL
        assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, [full], 16, 16, min_prob=min_prob) == pkg.EINVAL
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, [full], 16, 17) == pkg.EINVAL                          # 16 x 17 labels into a 16 x 16 buffer
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, [full] * 4, 16, 16) == pkg.EINVAL                      # four views' logits in a buffer of three
    ctx.sync()
    for b, dt in ((lab, np.int32), (sc, np.float32), (pr, np.float32)):
        assert np.array_equal(b.download(fill.shape, dt), fill.astype(dt)), "nothing may have been launched"
    assert call(lab.ptr, None, None, x.ptr, *ok, [(0, 0, 64, 56, 0), (0, 0, 64, 56, 1), full], 8, 16) == pkg.OK      # the ratio exactly, score NULL
    ctx.sync()
    got = lab.download(fill.shape, np.int32)
    assert (got[:8 * 16] == 0).all() and (got[8 * 16:] == LAB_FILL).all()
    for b in (x, lab, sc, pr):
        b.free()


# ------------------------------------------------------------------------------------------------------------------ the view resizer

GUARD, SENTINEL = 16, 0xAB


def _resize_view(pkg, ctx, f, imgs, oh, ow, view, fill):
    n, H, W, _ = imgs.shape
    nb = n * oh * ow * 3
    d_in = ctx.to_device(imgs)
    d_out = ctx.to_device(np.full(GUARD + nb + GUARD, SENTINEL, np.uint8))
    r = pkg.Resizer(ctx, H, W, oh, ow, filter=f, pad=fill, view=view)
    r.run(d_out.ptr + GUARD, d_in.ptr, n)
    ctx.sync()
    raw = d_out.download((GUARD + nb + GUARD,), np.uint8)
    r.close()
    d_in.free()
    d_out.free()
    assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + nb:] == SENTINEL).all(), "bytes around `out` were written"
    return raw[GUARD:GUARD + nb].reshape(n, oh, ow, 3)


@pytest.mark.parametrize("index", range(18))
def test_view_resizer_equals_pillow(pkg, ctx, index):
    cases, fill = fixture()
    assert SENTINEL not in fill
    name, img, (oh, ow), view, scale, canvases = cases[index]
    batch = np.stack([img, img[::-1].copy(), 255 - img])           # batch 3: the image, upside down, its complement
    for f in R.FILTERS:
        got = _resize_view(pkg, ctx, f, batch, oh, ow, view, fill)
        bad = int((got[0] != canvases[f]).sum())
        assert bad == 0, "%s under %s: %d of %d bytes differ from Pillow's" % (name, R.NAMES[f], bad, got[0].size)
        for i in (1, 2):
            assert np.array_equal(got[i], view_canvas_ref(f, batch[i], oh, ow, view, fill)), "%s under %s: image %d of the batch" % (name, R.NAMES[f], i)


def test_view_resizer_wide_inner_image_and_the_letterbox(pkg, ctx):
    """an inner image of three column tiles with a short last one, mirrored: the tiles land at the mirrored places; and mirror = 0 with fit_pad's
    rectangle is Resizer(pad=...)'s bytes"""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (2, 90, 300, 3), dtype=np.uint8)
    fill = (9, 200, 30)
    for f in R.FILTERS:
        for view in [(13, 6, 150, 45, 1), (0, 0, 177, 64, 1), (13, 6, 150, 45, 0)]:
            got = _resize_view(pkg, ctx, f, img, 64, 177, view, fill)
            for i in range(2):
                assert np.array_equal(got[i], view_canvas_ref(f, img[i], 64, 177, view, fill)), (R.NAMES[f], view, i)
        H, W, oh, ow = 45, 60, 64, 96
        v = pkg.fit_view(H, W, oh, ow)
        src = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
        got = _resize_view(pkg, ctx, f, src, oh, ow, v, fill)
        d_in, d_out = ctx.to_device(src), ctx.alloc(3 * oh * ow * 3)
        r = pkg.Resizer(ctx, H, W, oh, ow, filter=f, pad=fill)
        r.run(d_out.ptr, d_in.ptr, 3)
        ctx.sync()
        assert np.array_equal(got, d_out.download((3, oh, ow, 3), np.uint8)), R.NAMES[f]
        r.close()
        d_in.free()
        d_out.free()


def test_view_resizer_refusals(pkg, ctx):
    lib, h = ctx.lib, C.c_void_p()
    fill = (C.c_uint8 * 3)(1, 2, 3)
    mk = lambda view, f=R.BILINEAR, H=45, fl=fill: lib.mbn_resizer_create_view(ctx.h, f, H, 60, 64, 96, None if view is None else pkg.views([view]), fl,
                                                                               C.byref(h))
    for bad in [(-1, 0, 10, 10, 0), (0, -1, 10, 10, 0), (0, 0, 0, 10, 0), (0, 0, 10, 0, 0), (90, 0, 10, 10, 0), (0, 60, 10, 10, 0), (0, 0, 10, 10, 2)]:
        assert mk(bad) == pkg.EINVAL and not h.value, bad
    arr = pkg.views([(0, 0, 10, 10, 0)])
    arr[0].reserved[0] = 1
    assert lib.mbn_resizer_create_view(ctx.h, R.BILINEAR, 45, 60, 64, 96, arr, fill, C.byref(h)) == pkg.EINVAL
    assert mk(None) == pkg.EINVAL and mk((0, 0, 10, 10, 0), fl=None) == pkg.EINVAL and mk((0, 0, 10, 10, 0), f=9) == pkg.EINVAL
    assert mk((0, 0, 10, 10, 0), H=8000) == pkg.EUNSUPPORTED and not h.value          # the envelope of (8000, 60) -> (10, 10)


# ------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS, BATCH = 0.5, 21, 64, 96, 2
SCALES = [1.0, 1.0, 0.75, 0.75, 0.5, 0.5]
MIRRORS = [0, 1, 0, 1, 0, 1]


def _staged(pkg, ctx, p, shape):
    got = np.empty(shape, np.uint8)
    assert ctx.lib.mbn_download(ctx.h, got.ctypes.data, p, got.nbytes) == pkg.OK
    return got


def _f32(v):
    return (C.c_float * len(v))(*v)


def _i32(v):
    return (C.c_int32 * len(v))(*v)


@pytest.mark.parametrize("dtype,os_", [("f32", 8), ("f32", 16), ("bf16", 8), ("i8", 32)])
def test_net_segment_views_fit(pkg, ctx, tmp_path, dtype, os_):
    n, K = BATCH, len(SCALES)
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, os_)
    h, w = ROWS // os_, COLS // os_
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n * K)
    dt = {"f32": pkg.DT_F32, "bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype]
    if dt != pkg.DT_F32:
        net.set_dtype(dt)
    lib = ctx.lib
    rng = np.random.default_rng(31)
    d_dense = ctx.alloc(n * K * h * w * CLASSES * 4)
    bufs = [d_dense]

    def outputs(total):
        trio = (ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, PR_FILL, np.float32)),
                ctx.to_device(np.full(total, SC_FILL, np.float32)))
        bufs.extend(trio)
        return trio

    first = True
    for sh, sw in [(75, 130), (64, 96)]:
        src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
        d_src = ctx.to_device(src)
        bufs.append(d_src)
        npix = n * sh * sw
        d_lab, d_pr, d_sc = outputs(npix + TAIL)
        call = lambda batch, rows, cols, scales, mirrors: lib.mbn_net_segment_views_fit(net.h, d_src.ptr, batch, rows, cols, _f32(scales), _i32(mirrors),
                                                                                       len(scales), d_lab.ptr, d_pr.ptr, d_sc.ptr, 0.0, 0)
        if first:
            assert call(n, sh, sw, SCALES, MIRRORS) == pkg.EINVAL                            # no uint8 images yet
            net.set_input_u8(True)
            assert call(n + 1, sh, sw, SCALES, MIRRORS) == pkg.EINVAL                        # batch * K above max_batch
            assert call(n, sh, sw, [1.0, 0.0], [0, 0]) == pkg.EINVAL and call(n, sh, sw, [1.5], [0]) == pkg.EINVAL
            assert call(n, sh, sw, [1.0, 0.5], [0, 2]) == pkg.EINVAL
            assert call(n, sh, sw, [1.0] * 9, [0] * 9) == pkg.EINVAL
            # a 6 x 9 source has the canvas's aspect: the full window, 6 outputs of at least 2 coarse rows: under the ratio at every stride here
            assert call(n, 6, 9, [1.0, 0.5], [0, 0]) == pkg.EUNSUPPORTED
            ctx.sync()
            assert (d_lab.download((npix + TAIL,), np.int32) == LAB_FILL).all() and (d_sc.download((npix + TAIL,), np.float32) == SC_FILL).all()
            assert (d_pr.download((npix + TAIL,), np.float32) == PR_FILL).all(), "a refused call may not write"
            first = False
        views = [pkg.fit_view(sh, sw, ROWS, COLS, s, m) for s, m in zip(SCALES, MIRRORS)]
        staging = net.resize_views(d_src.ptr, n, sh, sw, SCALES, MIRRORS)
        ctx.sync()
        d_stage = _staged(pkg, ctx, staging, (K, n, ROWS, COLS, 3))
        for k in (0, 3):                                     # the staging is view-major: view k's canvases at images k * n ..
            for i in range(n):
                assert np.array_equal(d_stage[k, i], view_canvas_ref(R.BILINEAR, src[i], ROWS, COLS, E.view_tuple(views[k]), (0, 0, 0))), (k, i)
        net.forward_dense(staging, d_dense.ptr, n * K)
        ctx.sync()
        dense = d_dense.download((K, n, h, w, CLASSES), np.float32)
        assert np.isfinite(dense).all() and dense.std() > 0
        net.segment_views_fit(d_src.ptr, n, sh, sw, SCALES, MIRRORS, d_lab.ptr, d_pr.ptr, d_sc.ptr)
        ctx.sync()
        want_lab, want_sc, want_pr = E.ensemble(dense, ROWS, COLS, views, sh, sw)
        lab, sc, pr = (d_lab.download((npix + TAIL,), np.int32), d_sc.download((npix + TAIL,), np.float32), d_pr.download((npix + TAIL,), np.float32))
        assert np.array_equal(lab[:npix].reshape(n, sh, sw), want_lab), "%s os %d %dx%d: %d labels differ" % (dtype, os_, sh, sw,
                                                                                                          int((lab[:npix] != want_lab.ravel()).sum()))
        assert np.array_equal(_bits(sc[:npix]), _bits(want_sc).ravel())
        _prob_check(pr[:npix].reshape(n, sh, sw), want_pr, CLASSES, "%s os %d %dx%d" % (dtype, os_, sh, sw))
        assert (lab[npix:] == LAB_FILL).all() and (sc[npix:] == SC_FILL).all() and (pr[npix:] == PR_FILL).all()
        assert want_sc.std() > 0
        # one view at scale 1, unmirrored: segment_fit's labels and score bits
        d_lab2, _, d_sc2 = outputs(npix)
        d_lab3, _, d_sc3 = outputs(npix)
        net.segment_views_fit(d_src.ptr, n, sh, sw, [1.0], [0], d_lab2.ptr, None, d_sc2.ptr)
        net.segment_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab3.ptr, d_sc3.ptr)
        ctx.sync()
        assert np.array_equal(d_lab2.download((npix,), np.int32), d_lab3.download((npix,), np.int32))
        assert np.array_equal(d_sc2.download((npix,), np.uint32), d_sc3.download((npix,), np.uint32))
    # another filter and another colour build new view resizers: the staging follows
    net.set_resize_filter(R.BICUBIC)
    net.set_pad_color(10, 20, 30)
    staging = net.resize_views(d_src.ptr, n, 64, 96, [0.5], [1])
    ctx.sync()
    one = _staged(pkg, ctx, staging, (n, ROWS, COLS, 3))
    v = E.view_tuple(pkg.fit_view(64, 96, ROWS, COLS, 0.5, 1))
    assert np.array_equal(one[1], view_canvas_ref(R.BICUBIC, src[1], ROWS, COLS, v, (10, 20, 30)))
    net.destroy()
    for b in bufs:
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def test_c_host_tta(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    seed, alpha, os_, sh, sw = 3, 0.5, 16, 75, 130
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, out = str(tmp_path / "a.ppm"), str(tmp_path / "out.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", str(seed), "--alpha", str(alpha), "--res", "%dx%d" % (ROWS, COLS), "--output-stride", str(os_), "--ppm", ppm]
    tta = ["--tta-scales", "1,0.5", "--tta-flip"]
    for args in (["--segment-source", out] + tta,                                              # the default fit is the crop
                 ["--fit", "stretch", "--segment-source", out] + tta,
                 ["--fit", "pad"] + tta,                                                       # no --segment-source
                 ["--fit", "pad", "--segment-source", out, "--tta-flip"],                      # no scales
                 ["--fit", "pad", "--segment-source", out, "--tta-scales", "1,0.9,0.8,0.7,0.6", "--tta-flip"],      # ten views
                 ["--fit", "pad", "--segment-source", out, "--tta-scales", "1,1.5"],
                 ["--fit", "pad", "--segment-source", out, "--tta-scales", "1,,0.5"]):
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and not os.path.exists(out), (args, r.stdout + r.stderr)
    r = subprocess.run(common + ["--fit", "pad", "--segment-source", out] + tta, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    assert m, raw[:32]
    classes = 1000                                      # the host's synthetic weights
    assert tuple(int(g) for g in m.groups()) == (sw, sh, classes - 1)
    got = np.frombuffer(raw[m.end():], ">u2").astype(np.int32).reshape(sh, sw)
    # the same through the mirror: the views are (1, plain), (1, mirrored), (0.5, plain), (0.5, mirrored)
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(ROWS, COLS), lib=pkg.load(), output_stride=os_)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 4)
    net.set_input_u8(True)
    d_src, d_lab = ctx.to_device(src), ctx.alloc(sh * sw * 4)
    net.segment_views_fit(d_src.ptr, 1, sh, sw, [1.0, 1.0, 0.5, 0.5], [0, 1, 0, 1], d_lab.ptr)
    ctx.sync()
    want = d_lab.download((sh, sw), np.int32)
    assert np.array_equal(got, want), "%d of %d pixels differ from Net.segment_views_fit" % (int((got != want).sum()), want.size)
    assert len(np.unique(want)) > 1
    # --min-confidence / --ignore-label and --segment-confidence keep working
    conf = str(tmp_path / "conf.pgm")
    r = subprocess.run(common + ["--fit", "pad", "--segment-source", out, "--segment-confidence", conf, "--min-confidence", "0.5", "--ignore-label", "7"]
                       + tta, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(conf), r.stdout + r.stderr
    d_pr = ctx.alloc(sh * sw * 4)
    net.segment_views_fit(d_src.ptr, 1, sh, sw, [1.0, 1.0, 0.5, 0.5], [0, 1, 0, 1], d_lab.ptr, d_pr.ptr, None, 0.5, 7)
    ctx.sync()
    raw = open(out, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    assert np.array_equal(np.frombuffer(raw[m.end():], ">u2").astype(np.int32).reshape(sh, sw), d_lab.download((sh, sw), np.int32))
    raw = open(conf, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n255\n", raw)
    prob = d_pr.download((sh, sw), np.float32)
    assert np.array_equal(np.frombuffer(raw[m.end():], np.uint8).reshape(sh, sw), np.floor(prob.astype(np.float64) * 255.0 + 0.5).astype(np.uint8))
    net.destroy()
    for b in (d_src, d_lab, d_pr):
        b.free()
    hw.free()
