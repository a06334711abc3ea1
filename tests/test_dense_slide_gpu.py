"""Segment by sliding window on the GPU. mbn_resample_slide_f32 alone: labels and score bits equal to tests/dense_slide_ref.py (the normative
arithmetic) on the smallest shapes that reach each way of going wrong: every coverage count 1, 2, 3, 4, 6, 9 in one map, the minimum ratio (largest
footprints, smallest chunk), cells wider than a workgroup's 32 outputs with ragged edges, a hand-made irregular plan, both staging paths, the order
of the sum, adversarial values in one tile only, the softmax form within dense_prob_ref's bound, argument errors, nothing written outside the
maps, one capture. The net runner: resize_tiles against numpy slices / resize_filters_ref, segment_slide against the reference applied to
forward_dense of that same staging, and the consumers of its label maps. The C host's --slide.

Planning CU counts: the kernel is one workgroup per piece of the output and not persistent; nothing in it or in its launch depends on the number
of compute units, so there is no planning-CU sweep here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_any_ref
import dense_prob_ref as P
import dense_slide_ref as S
import resize_filters_ref as R
from test_dense_any_gpu import LAB_FILL, SC_FILL, TAIL, _logits
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

PR_FILL = -3.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _tiles_logits(n, T, h, w, classes, seed):
    return np.stack([_logits(n, h, w, classes, seed=seed + 17 * t) for t in range(T)], axis=1)


def _run(ctx, x, plan, H, W, offset=0, with_score=True, with_prob=False, min_prob=0.0, ignore=0):
    """mbn_resample_slide_f32 on x [n][tiles][h][w][classes] (uploaded `offset` bytes into its allocation): (labels, score or None, prob or None).
    The output buffers carry a sentinel pattern and TAIL more elements, which must come back unchanged."""
    n, T, h, w, classes = x.shape
    d_x = ctx.to_device(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
    npix = n * H * W
    d_lab = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32))
    d_sc = ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32)) if with_score else None
    d_pr = ctx.to_device(np.full(npix + TAIL, PR_FILL, np.float32)) if with_prob else None
    ctx.resample_slide(d_lab.ptr, d_pr.ptr if d_pr else None, d_sc.ptr if d_sc else None, d_x.ptr + offset, n, h, w, classes, plan, H, W, min_prob, ignore)
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


def _check(ctx, x, plan, H, W, what, **kw):
    want_lab, want_sc, want_pr = S.slide(x, plan, H, W)
    lab, sc, pr = _run(ctx, x, plan, H, W, **kw)
    assert (lab != LAB_FILL).all(), "%s: %d pixels were not written" % (what, int((lab == LAB_FILL).sum()))
    bad = int((lab != want_lab).sum())
    assert bad == 0, "%s: %d of %d labels differ from dense_slide_ref" % (what, bad, lab.size)
    if sc is not None:
        bad = int((_bits(sc) != _bits(want_sc)).sum())
        assert bad == 0, "%s: %d of %d score bit patterns differ from dense_slide_ref" % (what, bad, sc.size)
    if pr is not None:
        _prob_check(pr, want_pr, x.shape[4], what)
    return want_lab, want_sc, want_pr


# ----------------------------------------------------------------------------------------------------------------------- geometry

@pytest.mark.parametrize("classes", [21, 64])                  # 21: dword loads, a padded last group; 64: 16-byte loads
@pytest.mark.parametrize("name", list(S.GEOMETRY))
def test_kernel_geometry(pkg, ctx, name, classes):
    h, w, plan, H, W = S.geometry_plan(name)
    assert pkg.resample_slide_envelope(2, h, w, classes, plan, H, W) == pkg.OK
    assert set(np.unique(S.count_map(plan, H, W)).tolist()) == S.COUNTS, "the placement no longer reaches every coverage count"
    x = _tiles_logits(2, len(plan[2]) * len(plan[3]), h, w, classes, seed=h * 1000 + w * 100 + H + W)
    _check(ctx, x, plan, H, W, "%s classes %d" % (name, classes), with_prob=classes == 21)
    _check(ctx, x, pkg.slide_plan(H, W, plan[0], plan[1], *S.GEOMETRY[name][2]), H, W, "%s by mbn_slide_plan" % name)


def test_kernel_hand_made_irregular_plan(pkg, ctx):
    """not from the helper: uneven steps, tiles that only touch (columns 15 | 16), three over rows 6..11 and columns 30..31 and 33..35"""
    plan = (10, 16, [0, 2, 6, 10, 16, 20], [0, 16, 20, 30, 33])
    H, W, h, w = 30, 49, 2, 4
    assert pkg.resample_slide_envelope(2, h, w, 21, plan, H, W) == pkg.OK
    assert set(np.unique(S.count_map(plan, H, W)).tolist()) == {1, 2, 3, 4, 6, 9}
    _check(ctx, _tiles_logits(2, 30, h, w, 21, seed=5), plan, H, W, "irregular plan", with_prob=True)
    _check(ctx, _tiles_logits(2, 30, h, w, 64, seed=6), plan, H, W, "irregular plan, 16-byte loads")


@pytest.mark.parametrize("classes", [21, 64])
def test_kernel_largest_staging(pkg, ctx, classes):
    """10 x 10 maps at the minimum ratio, nine tiles over the middle: the launch stages 9 x 10 x 10 vectors of 8 classes, 43 200 bytes"""
    plan, H, W = (40, 40, [0, 14, 28, 42], [0, 14, 28, 42]), 82, 82
    l = pkg.resample_slide_plan(10, 10, plan, H, W)
    assert (l.fy, l.fx, l.ch) == (10, 10, 8) and l.lds_bytes == 43200
    _check(ctx, _tiles_logits(1, 16, 10, 10, classes, seed=classes), plan, H, W, "largest staging, classes %d" % classes, with_prob=True)


@pytest.mark.parametrize("classes", [1, 3, 1001])              # one class; fewer than a group; many chunks and a short last one
def test_kernel_class_counts(pkg, ctx, classes):
    h, w, plan, H, W = S.geometry_plan("A")
    _check(ctx, _tiles_logits(1, 16, h, w, classes, seed=classes), plan, H, W, "classes %d" % classes, with_prob=True)


@pytest.mark.parametrize("classes", [21, 64])
def test_kernel_logits_at_a_4_byte_offset(pkg, ctx, classes):
    h, w, plan, H, W = S.geometry_plan("B")
    _check(ctx, _tiles_logits(2, 16, h, w, classes, seed=9), plan, H, W, "offset 4, classes %d" % classes, offset=4)


def test_kernel_score_null(pkg, ctx):
    h, w, plan, H, W = S.geometry_plan("B")
    _check(ctx, _tiles_logits(2, 16, h, w, 21, seed=11), plan, H, W, "score NULL", with_score=False)
    _check(ctx, _tiles_logits(2, 16, h, w, 21, seed=12), plan, H, W, "score NULL, softmax", with_score=False, with_prob=True)


# --------------------------------------------------------------------------------------------------------------- device identities

@pytest.mark.parametrize("touching", [False, True])
def test_kernel_count_1_equals_the_plain_kernel_on_the_device(pkg, ctx, touching):
    """one tile (ny = nx = 1), and two tiles that only touch (stride = tile): per tile the bits of mbn_resample_argmax_f32 to the tile's size"""
    n, h, w, classes, th, tw = 2, 5, 7, 21, 67, 50
    nx = 2 if touching else 1
    plan = pkg.slide_plan(th, nx * tw, th, tw, th, tw)
    assert plan.xs == [0, tw][:nx] and plan.ys == [0]
    H, W = th, nx * tw
    x = _tiles_logits(n, nx, h, w, classes, seed=3 + nx)
    d_x = ctx.to_device(x)
    d_t = ctx.to_device(np.ascontiguousarray(x.transpose(1, 0, 2, 3, 4)))                  # tile-major: each tile's batch on its own
    slide = [ctx.to_device(np.full(n * H * W, LAB_FILL, np.int32)), ctx.to_device(np.full(n * H * W, SC_FILL, np.float32))]
    plain = [ctx.to_device(np.full(nx * n * th * tw, LAB_FILL, np.int32)), ctx.to_device(np.full(nx * n * th * tw, SC_FILL, np.float32))]
    ctx.resample_slide(slide[0].ptr, None, slide[1].ptr, d_x.ptr, n, h, w, classes, plan, H, W)
    ctx.resample_argmax(plain[0].ptr, plain[1].ptr, d_t.ptr, nx * n, h, w, classes, th, tw)
    ctx.sync()
    got = [b.download((n, H, W), np.uint32) for b in slide]
    want = [b.download((nx, n, th, tw), np.uint32) for b in plain]
    for t in range(nx):
        assert np.array_equal(got[0][:, :, t * tw:(t + 1) * tw], want[0][t]) and np.array_equal(got[1][:, :, t * tw:(t + 1) * tw], want[1][t]), t
    want_lab, want_sc = dense_any_ref.resample_argmax(x[:, 0], th, tw)
    assert np.array_equal(got[0][:, :, :tw].view(np.int32), want_lab) and np.array_equal(got[1][:, :, :tw], _bits(want_sc))
    for b in [d_x, d_t] + slide + plain:
        b.free()


def test_kernel_sums_in_tile_order(pkg, ctx):
    x = S.order_input()
    plan = (8, 12, [0], [0, 4, 8])                              # columns 8..11 lie under all three tiles
    _, sc, _ = _check(ctx, x, plan, 8, 20, "1e8, -1e8, 1")
    assert (sc[0, :, 8:12] == np.float32(1.0) / np.float32(3.0)).all()
    _, sc, _ = _check(ctx, np.ascontiguousarray(x[:, [0, 2, 1]]), plan, 8, 20, "1e8, 1, -1e8")
    assert (sc[0, :, 8:12] == 0).all()
    xt = np.ascontiguousarray(x.transpose(0, 1, 3, 2, 4))      # the same down the rows: ascending iy
    _, sc, _ = _check(ctx, xt, (12, 8, [0, 4, 8], [0]), 20, 8, "1e8, -1e8, 1 down the rows")
    assert (sc[0, 8:12] == np.float32(1.0) / np.float32(3.0)).all()
    # iy before ix: tiles (0, 0), (0, 1), (1, 0) hold 1e8, -1e8, 1 and (1, 1) holds 0: ((1e8 - 1e8) + 1) + 0 = 1 over the four-tile cell
    x4 = np.zeros((1, 4, 2, 3, 4), np.float32)
    x4[0, 0, ..., 1], x4[0, 1, ..., 1], x4[0, 2, ..., 1] = 1e8, -1e8, 1.0
    _, sc, _ = _check(ctx, x4, (8, 12, [0, 4], [0, 6]), 12, 18, "iy before ix")
    assert (sc[0, 4:8, 6:12] == np.float32(0.25)).all()
    _, sc, _ = _check(ctx, np.ascontiguousarray(x4[:, [0, 2, 1, 3]]), (8, 12, [0, 4], [0, 6]), 12, 18, "ix before iy would give this")
    assert (sc[0, 4:8, 6:12] == 0).all()


def test_kernel_adversarial_values(pkg, ctx):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    h, w, plan, H, W = S.geometry_plan("A")
    T = 16
    x = _tiles_logits(1, T, h, w, 65, seed=13)                  # a NaN in one tile only, where the mean's winner was under nine tiles
    lab0, _, _ = S.slide(x, plan, H, W)
    assert S.count_map(plan, H, W)[50, 75] == 9
    x[0, 5, :, :, int(lab0[0, 50, 75])] = nan
    want_lab, want_sc, _ = _check(ctx, x, plan, H, W, "NaN in one tile", with_prob=True)
    assert (want_lab != lab0).any() and np.isfinite(want_sc).all(), "a NaN sum never wins"
    x = _tiles_logits(1, T, h, w, 21, seed=15)                  # +inf and -inf in one tile each
    x[0, 0, 1, 2, 3] = inf
    x[0, 10, 0, 1, 7] = -inf
    _, want_sc, want_pr = _check(ctx, x, plan, H, W, "inf in one tile", with_prob=True)
    assert (want_sc == inf).any() and (want_pr[want_sc == inf] == 0).all()
    x = _tiles_logits(1, T, h, w, 21, seed=16)                  # +inf in one tile and -inf in its neighbour on the same class: a NaN sum between
    x[0, 5, :, :, 3] = inf
    x[0, 6, :, :, 3] = -inf
    want_lab, want_sc, _ = _check(ctx, x, plan, H, W, "+inf and -inf", with_prob=True)
    assert (want_lab == 3).any() and (want_lab != 3).any()
    x = np.full((1, T, h, w, 21), nan, np.float32)              # nothing wins anywhere
    want_lab, want_sc, want_pr = _check(ctx, x, plan, H, W, "all NaN", with_prob=True)
    assert (want_lab == 0).all() and (want_sc == -inf).all() and (want_pr == 0).all()
    x = np.zeros((2, T, h, w, 200), np.float32)                 # equal maxima in different chunks: the lowest index wins
    x[..., 5] = x[..., 70] = x[..., 131] = 2.0
    want_lab, _, _ = _check(ctx, x, plan, H, W, "equal maxima")
    assert (want_lab == 5).all()
    x = np.random.default_rng(19).integers(-8, 9, (2, T, h, w, 65)).astype(np.float32)      # integer-valued logits: ties everywhere
    _check(ctx, x, plan, H, W, "integer-valued logits", with_prob=True)


# ------------------------------------------------------------------------------------------------------------------------ softmax

@pytest.mark.parametrize("case", S.THRESHOLD_CASES)
def test_kernel_threshold(pkg, ctx, case):
    n, name, classes, seed, sigma, min_prob = case
    h, w, plan, H, W = S.geometry_plan(name)
    x = S.threshold_input(case)
    ignore = -9
    lab_a, sc_a, _ = _run(ctx, x, plan, H, W)                                                  # the argmax form
    lab0, sc0, pr0 = _run(ctx, x, plan, H, W, with_prob=True)                                  # min_prob = 0
    assert np.array_equal(lab0, lab_a) and np.array_equal(_bits(sc0), _bits(sc_a)), "labels and score bits are the argmax form's"
    lab, sc, pr = _run(ctx, x, plan, H, W, with_prob=True, min_prob=min_prob, ignore=ignore)
    assert np.array_equal(_bits(pr), _bits(pr0)) and np.array_equal(_bits(sc), _bits(sc0)), "prob and score are written unchanged"
    assert np.array_equal(lab, np.where(pr < np.float32(min_prob), ignore, lab_a)), "ignore_label exactly where the stored prob < min_prob"
    want_lab, _, want_pr = S.slide(x, plan, H, W)
    _prob_check(pr, want_pr, classes, "threshold case")
    out = P.excluded(want_pr, min_prob, classes)
    assert out.mean() <= 0.01
    assert np.array_equal(lab[~out], P.threshold(want_lab, want_pr, min_prob, ignore)[~out])
    assert (lab == ignore).any() and (lab != ignore).any()
    lab_n, _, _ = _run(ctx, x, plan, H, W, with_score=False, with_prob=False, min_prob=min_prob, ignore=ignore)      # prob = NULL, min_prob > 0
    assert np.array_equal(lab_n, lab)


# ------------------------------------------------------------------------------------------------------------------------- errors

def test_kernel_argument_errors(pkg, ctx):
    ok_plan = (8, 12, [0, 4, 8], [0, 6])                        # 3 x 2 tiles of 2 x 3 maps over 16 x 18
    x = ctx.to_device(np.zeros(6 * 2 * 3 * 21, np.float32))
    fill = np.full(16 * 18, LAB_FILL, np.int32)
    lab, sc, pr = ctx.to_device(fill), ctx.to_device(fill.astype(np.float32)), ctx.to_device(fill.astype(np.float32))

    def call(l, p, s, logits, n, h, w, c, plan, H, W, min_prob=0.0):
        return ctx.lib.mbn_resample_slide_f32(ctx.h, l, p, s, logits, n, h, w, c, None if plan is None else C.byref(pkg.slide(plan)), H, W, min_prob,
                                              0, None)

    ok = (1, 2, 3, 21)
    assert call(None, None, sc.ptr, x.ptr, *ok, ok_plan, 16, 18) == pkg.EINVAL
    assert call(lab.ptr, None, sc.ptr, None, *ok, ok_plan, 16, 18) == pkg.EINVAL
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, None, 16, 18) == pkg.EINVAL
    for bad in [(0, 2, 3, 21, 16, 18), (1, 0, 3, 21, 16, 18), (1, 2, 0, 21, 16, 18), (1, 2, 3, 0, 16, 18), (1, 2, 3, 21, 0, 18), (1, 2, 3, 21, 16, -1)]:
        assert call(lab.ptr, None, sc.ptr, x.ptr, *bad[:4], ok_plan, *bad[4:]) == pkg.EINVAL, bad
    # not flush, not from 0, not ascending, a gap (on y for 17 rows, on x), no tiles, no tile
    for plan, H, W in [((8, 12, [0, 4, 9], [0, 6]), 16, 18), ((8, 12, [1, 4, 8], [0, 6]), 16, 18), ((8, 12, [0, 4, 4, 8], [0, 6]), 16, 18),
                       ((8, 12, [0, 9], [0, 6]), 17, 18), ((8, 12, [0, 4, 8], [0, 13]), 16, 25), ((8, 12, [], [0, 6]), 16, 18),
                       ((0, 12, [0, 4, 8], [0, 6]), 16, 18)]:
        assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, plan, H, W) == pkg.EINVAL, plan
    s = pkg.slide(ok_plan)
    s.x[9] = 3
    assert ctx.lib.mbn_resample_slide_f32(ctx.h, lab.ptr, None, sc.ptr, x.ptr, *ok, C.byref(s), 16, 18, 0.0, 0, None) == pkg.EINVAL      # an unused entry
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, (8, 12, [0, 2, 4, 6, 8], [0, 6]), 16, 18) == pkg.EUNSUPPORTED      # four tiles over rows 6, 7
    assert call(lab.ptr, None, sc.ptr, x.ptr, 1, 3, 3, 14, ok_plan, 16, 18) == pkg.EUNSUPPORTED                      # tile_rows < 4 x rows
    assert call(lab.ptr, None, sc.ptr, x.ptr, 1, 2, 4, 15, ok_plan, 16, 18) == pkg.EUNSUPPORTED                      # tile_cols < 4 x cols
    assert call(lab.ptr, None, sc.ptr, x.ptr + 2, 1, 2, 3, 20, ok_plan, 16, 18) == pkg.EINVAL                        # off 4 bytes
    assert call(lab.ptr, pr.ptr + 2, sc.ptr, x.ptr, *ok, ok_plan, 16, 18) == pkg.EINVAL
    for min_prob in (-0.5, 1.5, float("nan")):
        assert call(lab.ptr, pr.ptr, sc.ptr, x.ptr, *ok, ok_plan, 16, 18, min_prob=min_prob) == pkg.EINVAL
        assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, ok_plan, 16, 18, min_prob=min_prob) == pkg.EINVAL
    assert call(lab.ptr, None, sc.ptr, x.ptr, *ok, (8, 12, [0, 4, 8], [0, 6, 7]), 16, 19) == pkg.EINVAL              # 16 x 19 labels, nine tiles' logits
    assert call(lab.ptr, None, sc.ptr, x.ptr, 2, 2, 3, 21, ok_plan, 16, 18) == pkg.EINVAL                            # two images' maps
    ctx.sync()
    for b, dt in ((lab, np.int32), (sc, np.float32), (pr, np.float32)):
        assert np.array_equal(b.download(fill.shape, dt), fill.astype(dt)), "nothing may have been launched"
    assert call(lab.ptr, None, None, x.ptr, *ok, ok_plan, 16, 18) == pkg.OK                                          # the ratio exactly, score NULL
    ctx.sync()
    assert (lab.download(fill.shape, np.int32) == 0).all()
    for b in (x, lab, sc, pr):
        b.free()


def test_kernel_captured_as_one_launch(pkg, ctx):
    """no allocation and no blocking call: legal between mbn_graph_begin and mbn_graph_end; the capture runs nothing, the replay writes the bytes
    of the plain call"""
    h, w, plan, H, W = S.geometry_plan("A")
    n, classes = 2, 21
    x = _tiles_logits(n, 16, h, w, classes, seed=77)
    want = _run(ctx, x, plan, H, W, with_prob=True)
    d_x = ctx.to_device(x)
    npix = n * H * W
    cap = [ctx.to_device(np.full(npix, LAB_FILL, np.int32)), ctx.to_device(np.full(npix, SC_FILL, np.float32)), ctx.to_device(np.full(npix, PR_FILL, np.float32))]
    lib, g = ctx.lib, C.c_void_p()
    assert lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = lib.mbn_resample_slide_f32(ctx.h, cap[0].ptr, cap[2].ptr, cap[1].ptr, d_x.ptr, n, h, w, classes, C.byref(pkg.slide(plan)), H, W, 0.0, 0, None)
    assert lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert (cap[0].download((npix,), np.int32) == LAB_FILL).all(), "the captured call ran"
    assert lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    for a, b, dt in zip(cap, (want[0], want[1], want[2]), (np.int32, np.float32, np.float32)):
        assert np.array_equal(_bits(a.download((n, H, W), dt)), _bits(b))
    lib.mbn_graph_destroy(ctx.h, g)
    for b in [d_x] + cap:
        b.free()


# ------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS, BATCH = 0.5, 21, 64, 96, 2


def _staged(pkg, ctx, p, shape):
    got = np.empty(shape, np.uint8)
    assert ctx.lib.mbn_download(ctx.h, got.ctypes.data, p, got.nbytes) == pkg.OK
    return got


@pytest.mark.parametrize("dtype,os_", [("f32", 8), ("f32", 16), ("bf16", 8), ("i8", 32)])
def test_net_segment_slide(pkg, ctx, tmp_path, dtype, os_):
    n = BATCH
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, os_)
    h, w = ROWS // os_, COLS // os_
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 4 * n)
    dt = {"f32": pkg.DT_F32, "bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype]
    if dt != pkg.DT_F32:
        net.set_dtype(dt)
    lib = ctx.lib
    rng = np.random.default_rng(31)
    d_dense = ctx.alloc(4 * n * h * w * CLASSES * 4)
    bufs = [d_dense]

    def outputs(total):
        trio = (ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, PR_FILL, np.float32)),
                ctx.to_device(np.full(total, SC_FILL, np.float32)))
        bufs.extend(trio)
        return trio

    first = True
    # 75 x 130: the tile is the plan's input, a byte copy; 64 x 96: a 40 x 60 tile that the ragged resizer upscales
    for (sh, sw), tile, stride in [((75, 130), (ROWS, COLS), (43, 64)), ((64, 96), (40, 60), (27, 40))]:
        src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
        d_src = ctx.to_device(src)
        bufs.append(d_src)
        npix = n * sh * sw
        d_lab, d_pr, d_sc = outputs(npix + TAIL)
        call = lambda batch, rows, cols, t, s, min_prob=0.0: lib.mbn_net_segment_slide(net.h, d_src.ptr, batch, rows, cols, t[0], t[1], s[0], s[1],
                                                                                       d_lab.ptr, d_pr.ptr, d_sc.ptr, min_prob, 0)
        if first:
            assert call(n, sh, sw, tile, stride) == pkg.EINVAL                               # no uint8 images yet
            net.set_input_u8(True)
            assert call(n + 1, sh, sw, tile, stride) == pkg.EINVAL                           # batch * tiles above max_batch
            assert call(n, sh, sw, tile, (65, 64)) == pkg.EINVAL                             # stride > tile
            assert call(n, sh, sw, (0, COLS), stride) == pkg.EINVAL and call(0, sh, sw, tile, stride) == pkg.EINVAL
            assert call(n, sh, sw, (76, COLS), (76, 64)) == pkg.EUNSUPPORTED                 # a tile larger than the source
            assert call(n, sh, sw, tile, (31, 64)) == pkg.EUNSUPPORTED                       # a stride under half a tile
            assert call(1, 4 * h - 1, 4 * w, (4 * h - 1, 4 * w), (4 * h - 1, 4 * w)) == pkg.EUNSUPPORTED      # one tile under 4 x the map
            assert call(n, sh, sw, tile, stride, min_prob=1.5) == pkg.EINVAL
            ctx.sync()
            assert (d_lab.download((npix + TAIL,), np.int32) == LAB_FILL).all() and (d_sc.download((npix + TAIL,), np.float32) == SC_FILL).all()
            assert (d_pr.download((npix + TAIL,), np.float32) == PR_FILL).all(), "a refused call may not write"
            first = False
        plan = pkg.slide_plan(sh, sw, tile[0], tile[1], stride[0], stride[1])
        T = plan.ny * plan.nx
        assert T == 4 and set(np.unique(S.count_map(plan, sh, sw)).tolist()) == {1, 2, 4}
        staging = net.resize_tiles(d_src.ptr, n, sh, sw, plan)
        ctx.sync()
        d_stage = _staged(pkg, ctx, staging, (n, T, ROWS, COLS, 3))
        for b in range(n):
            for iy, y in enumerate(plan.ys):
                for ix, x0 in enumerate(plan.xs):
                    if tile == (ROWS, COLS):
                        want = src[b, y:y + ROWS, x0:x0 + COLS]
                    else:
                        want = R.resize(R.BILINEAR, src[b], ROWS, COLS, (float(x0), float(y), float(x0 + tile[1]), float(y + tile[0])))
                    assert np.array_equal(d_stage[b, iy * plan.nx + ix], want), (b, iy, ix)
        net.forward_dense(staging, d_dense.ptr, n * T)
        ctx.sync()
        dense = d_dense.download((n, T, h, w, CLASSES), np.float32)
        assert np.isfinite(dense).all() and dense.std() > 0
        net.segment_slide(d_src.ptr, n, sh, sw, tile, stride, d_lab.ptr, d_pr.ptr, d_sc.ptr)
        ctx.sync()
        want_lab, want_sc, want_pr = S.slide(dense, plan, sh, sw)
        lab, sc, pr = (d_lab.download((npix + TAIL,), np.int32), d_sc.download((npix + TAIL,), np.float32), d_pr.download((npix + TAIL,), np.float32))
        assert np.array_equal(lab[:npix].reshape(n, sh, sw), want_lab), "%s os %d %dx%d: %d labels differ" % (dtype, os_, sh, sw,
                                                                                                          int((lab[:npix] != want_lab.ravel()).sum()))
        assert np.array_equal(_bits(sc[:npix]), _bits(want_sc).ravel())
        _prob_check(pr[:npix].reshape(n, sh, sw), want_pr, CLASSES, "%s os %d %dx%d" % (dtype, os_, sh, sw))
        assert (lab[npix:] == LAB_FILL).all() and (sc[npix:] == SC_FILL).all() and (pr[npix:] == PR_FILL).all()
        assert want_sc.std() > 0
        # the consumers serve a slide call as any uniform source-size call: the confusion of the downloaded labels
        truth = rng.integers(0, CLASSES + 2, (n, sh, sw)).astype(np.uint8)
        d_truth, d_counts = ctx.to_device(truth), ctx.to_device(np.zeros((CLASSES + 1) ** 2, np.uint64))
        bufs.extend([d_truth, d_counts])
        net.segment_score(d_lab.ptr, d_truth.ptr, 1, d_counts.ptr)
        ctx.sync()
        want_counts = np.zeros((CLASSES + 1, CLASSES + 1), np.uint64)
        np.add.at(want_counts, (np.minimum(truth, CLASSES).ravel().astype(np.int64), want_lab.ravel().astype(np.int64)), 1)
        assert np.array_equal(d_counts.download((CLASSES + 1, CLASSES + 1), np.uint64), want_counts)
    # one tile over a source of exactly the input size: segment_to's labels and score bits
    npix = n * ROWS * COLS
    d_lab2, _, d_sc2 = outputs(npix)
    d_lab3, _, d_sc3 = outputs(npix)
    net.segment_slide(d_src.ptr, n, ROWS, COLS, (ROWS, COLS), (ROWS, COLS), d_lab2.ptr, None, d_sc2.ptr)
    net.segment_to(d_src.ptr, n, ROWS, COLS, d_lab3.ptr, d_sc3.ptr)
    ctx.sync()
    assert np.array_equal(d_lab2.download((npix,), np.int32), d_lab3.download((npix,), np.int32))
    assert np.array_equal(d_sc2.download((npix,), np.uint32), d_sc3.download((npix,), np.uint32))
    # the ragged path's refusal is passed on, and the net stays usable
    net.set_resize_filter(R.LANCZOS)
    p = C.c_void_p()
    assert lib.mbn_net_resize_tiles(net.h, d_src.ptr, n, ROWS, COLS, C.byref(pkg.slide_plan(ROWS, COLS, 40, 60, 27, 40)), C.byref(p)) == pkg.EUNSUPPORTED
    net.set_resize_filter(R.BICUBIC)
    staging = net.resize_tiles(d_src.ptr, n, ROWS, COLS, pkg.slide_plan(ROWS, COLS, 40, 60, 27, 40))
    ctx.sync()
    one = _staged(pkg, ctx, staging, (n, 4, ROWS, COLS, 3))
    assert np.array_equal(one[1, 3], R.resize(R.BICUBIC, src[1], ROWS, COLS, (36.0, 24.0, 96.0, 64.0)))
    net.destroy()
    for b in bufs:
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def _pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    assert m, raw[:32]
    w, h, maxval = (int(g) for g in m.groups())
    return np.frombuffer(raw[m.end():], ">u2" if maxval > 255 else np.uint8).astype(np.int32).reshape(h, w), maxval


def test_c_host_slide(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    seed, alpha, os_, sh, sw = 3, 0.5, 16, 75, 130
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, out = str(tmp_path / "a.ppm"), str(tmp_path / "out.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", str(seed), "--alpha", str(alpha), "--res", "%dx%d" % (ROWS, COLS), "--output-stride", str(os_), "--ppm", ppm]
    for args in (["--slide", "64x96"],                                                         # no --segment-source
                 ["--segment-source", out, "--fit", "pad", "--slide", "64x96"],
                 ["--segment-source", out, "--fit", "crop", "--slide", "64x96"],
                 ["--segment-source", out, "--slide", "64x96", "--tta-flip"],
                 ["--segment-source", out, "--fit", "pad", "--slide", "64x96", "--tta-scales", "1,0.5"],
                 ["--segment-source", out, "--slide-stride", "43x64"],                         # a stride without a tile
                 ["--segment-source", out, "--slide", "64x"], ["--segment-source", out, "--slide", "0x96"],
                 ["--segment-source", out, "--slide", "64x96", "--slide-stride", "65x64"],     # gaps
                 ["--segment-source", out, "--slide", "64x96", "--slide-stride", "31x64"],     # under half a tile
                 ["--segment-source", out, "--slide", "76x96"]):                               # a tile larger than the image
        r = subprocess.run(common + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and not os.path.exists(out), (args, r.stdout + r.stderr)
    r = subprocess.run(common + ["--segment-source", out, "--slide", "64x96"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tiles of 64 x 96 at a stride of 43 x 64" in r.stdout                               # the default stride: (2 * tile + 2) / 3
    classes = 1000                                      # the host's synthetic weights
    got, maxval = _pgm(out)
    assert got.shape == (sh, sw) and maxval == classes - 1
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(ROWS, COLS), lib=pkg.load(), output_stride=os_)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 4)
    net.set_input_u8(True)
    d_src, d_lab, d_pr = ctx.to_device(src), ctx.alloc(sh * sw * 4), ctx.alloc(sh * sw * 4)
    net.segment_slide(d_src.ptr, 1, sh, sw, (64, 96), (43, 64), d_lab.ptr)
    ctx.sync()
    want = d_lab.download((sh, sw), np.int32)
    assert np.array_equal(got, want), "%d of %d pixels differ from Net.segment_slide" % (int((got != want).sum()), want.size)
    assert len(np.unique(want)) > 1
    # an explicit stride, --fit stretch given, and the confidence options keep working
    conf = str(tmp_path / "conf.pgm")
    r = subprocess.run(common + ["--fit", "stretch", "--segment-source", out, "--slide", "40x60", "--slide-stride", "20x35", "--segment-confidence", conf,
                                 "--min-confidence", "0.5", "--ignore-label", "7"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(conf), r.stdout + r.stderr
    net2 = pkg.Net(ctx, hw.plan, hw.blob.copy(), 12)
    net2.set_input_u8(True)
    net2.segment_slide(d_src.ptr, 1, sh, sw, (40, 60), (20, 35), d_lab.ptr, d_pr.ptr, None, 0.5, 7)
    ctx.sync()
    assert np.array_equal(_pgm(out)[0], d_lab.download((sh, sw), np.int32))
    prob = d_pr.download((sh, sw), np.float32)
    assert np.array_equal(_pgm(conf)[0], np.floor(prob.astype(np.float64) * 255.0 + 0.5).astype(np.int32))
    net.destroy()
    net2.destroy()
    for b in (d_src, d_lab, d_pr):
        b.free()
    hw.free()
