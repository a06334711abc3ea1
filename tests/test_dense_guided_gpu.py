"""The guided read-out on the GPU against tests/dense_guided_ref.py: labels and score bits equal, prob inside the bound of include/mbn.h; the block
mean; an edge followed; a flat guide; refusals; the net runner against the context-level chain. The table is always mbn_guided_lut's own."""
import numpy as np
import pytest

import dense_any_ref
import dense_guided_ref as ref
import dense_prob_ref
from test_dense_any_gpu import LAB_FILL, SC_FILL, TAIL
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu


_bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def _reduce(ctx, canvas, S):
    n, R, C, _ = canvas.shape
    d_c, d_lo = ctx.to_device(canvas), ctx.to_device(np.full(n * (R // S) * (C // S) * 3 + TAIL, 0xA5, np.uint8))
    ctx.guide_reduce(d_lo.ptr, d_c.ptr, n, R, C, S)
    ctx.sync()
    lo = d_lo.download((n * (R // S) * (C // S) * 3 + TAIL,), np.uint8)
    d_c.free(), d_lo.free()
    assert (lo[-TAIL:] == 0xA5).all(), "guide_lo written past the last image"
    return lo[:-TAIL].reshape(n, R // S, C // S, 3)


def _device(pkg, ctx, x, lo, hi, sigma, rect=None, R=0, Cc=0, prob=True, score=True):
    n, h, w, classes = x.shape                   # -> (labels, score bits or None, prob or None) [n][H][W]; the sentinels behind them must stay
    (H, W), npix = hi.shape[1:3], x.shape[0] * hi.shape[1] * hi.shape[2]
    bufs = [ctx.to_device(a) for a in (x, lo, hi, pkg.guided_lut(sigma))]
    d_lab = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32))
    d_sc, d_pr = (ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32)) if on else None for on in (score, prob))
    ctx.resample_guided(d_lab.ptr, d_pr.ptr if prob else None, d_sc.ptr if score else None, *(b.ptr for b in bufs), n, h, w, classes, H, W, R, Cc, rect)
    ctx.sync()
    out = [d_lab.download((npix + TAIL,), np.int32)] + [b.download((npix + TAIL,), np.float32) if b else None for b in (d_sc, d_pr)]
    [b.free() for b in bufs + [d_lab, d_sc, d_pr] if b is not None]
    assert (out[0][npix:] == LAB_FILL).all() and all(o is None or (o[npix:] == SC_FILL).all() for o in out[1:]), "written past the last image"
    lab, sc, pr = (None if o is None else o[:npix].reshape(n, H, W) for o in out)
    return lab, None if sc is None else _bits(sc), pr


def _check(pkg, ctx, x, lo, hi, sigma, what, rect=None, R=0, Cc=0, forms=((True, True), (False, True), (True, False), (False, False))):
    v = ref.interpolants(x, lo, hi, pkg.guided_lut(sigma), R, Cc, rect)
    want_lab, want_sc, want_pr = dense_prob_ref.from_interpolants(v)
    for prob, score in forms:
        lab, sc, pr = _device(pkg, ctx, x, lo, hi, sigma, rect, R, Cc, prob, score)
        name = "%s prob %d score %d" % (what, prob, score)
        assert np.array_equal(lab, want_lab), "%s: %d of %d labels differ from dense_guided_ref" % (name, int((lab != want_lab).sum()), lab.size)
        if score:
            assert np.array_equal(sc, _bits(want_sc)), "%s: %d score bit patterns differ" % (name, int((sc != _bits(want_sc)).sum()))
        if prob:
            assert (np.abs(pr - want_pr) <= dense_prob_ref.bound(x.shape[-1]) * want_pr).all(), name
    return want_lab, want_sc


def _inputs(h, w, H, W, classes, n=2, S=8):
    rng = np.random.default_rng(h * 1000 + W + classes)
    x = rng.standard_normal((n, h, w, classes)).astype(np.float32)
    canvas = rng.integers(0, 256, (n, h * S, w * S, 3), dtype=np.uint8)
    hi = np.clip(canvas[:, (np.arange(H) * h * S) // H][:, :, (np.arange(W) * w * S) // W].astype(np.int64) + rng.integers(-40, 41, (n, H, W, 3)), 0, 255)
    return x, canvas, hi.astype(np.uint8)


@pytest.mark.parametrize("sigma", [2.0, 24.0, 1000.0])
@pytest.mark.parametrize("classes", [1, 5, 8, 130])            # 5: dword loads, a padded group; 8: 16-byte loads; 130: crosses the chunk at 64 and 128
@pytest.mark.parametrize("shape", [(2, 3, 9, 13), (3, 5, 33, 70), (7, 7, 40, 28)])
def test_reference_parity(pkg, ctx, shape, classes, sigma):
    x, canvas, hi = _inputs(*shape, classes)
    lo = _reduce(ctx, canvas, 8)
    assert np.array_equal(lo, ref.reduce_mean(canvas, 8))
    _check(pkg, ctx, x, lo, hi, sigma, "%s classes %d sigma %g" % (shape, classes, sigma))


def test_nan_inf_and_an_all_nan_pixel(pkg, ctx):
    x, canvas, hi = _inputs(3, 5, 33, 70, 5)
    x[0, 1, 2, 3], x[0, 2, 1, 0], x[1, 0, 4, 2] = np.nan, np.inf, -np.inf
    x[1, 0, 0, :] = np.nan                                     # every output that touches coarse (0, 0) of image 1 is NaN in every class
    lab, sc = _check(pkg, ctx, x, ref.reduce_mean(canvas, 8), hi, 24.0, "special values")
    assert lab[1, 0, 0] == 0 and sc[1, 0, 0] == -np.inf and (sc == np.inf).any()


@pytest.mark.parametrize("classes", [5, 8])
def test_window_of_a_letterbox(pkg, ctx, classes):
    R, Cc, H, W, n = 64, 96, 375, 500, 2
    rect = tuple(pkg.fit_pad(H, W, R, Cc))
    rng = np.random.default_rng(classes)
    x = rng.standard_normal((n, 2, 3, classes)).astype(np.float32)
    lo = ref.reduce_mean(rng.integers(0, 256, (n, R, Cc, 3), dtype=np.uint8), 32)
    hi = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    _check(pkg, ctx, x, lo, hi, 24.0, "letterbox %s" % (rect,), rect, R, Cc, forms=((True, True),))
    whole = _device(pkg, ctx, x, lo, hi, 24.0, (0, 0, Cc, R), R, Cc)
    plain = _device(pkg, ctx, x, lo, hi, 24.0)
    assert all(np.array_equal(a, b) for a, b in zip(whole[:2], plain[:2])) and np.array_equal(_bits(whole[2]), _bits(plain[2])), "whole window != NULL rect"


@pytest.mark.parametrize("S", [1, 8, 32])
def test_guide_reduce(pkg, ctx, S):
    canvas = np.random.default_rng(S).integers(0, 256, (2, 64, 96, 3), dtype=np.uint8)
    assert np.array_equal(_reduce(ctx, canvas, S), ref.reduce_mean(canvas, S))


def test_it_follows_the_edge(pkg, ctx):
    """A colour edge at x = 50 inside a coarse cell (stride 32: cells end at 32, 64): the bilinear read-out puts the boundary at 64."""
    hi = np.empty((1, 64, 128, 3), np.uint8)
    hi[:, :, :50], hi[:, :, 50:] = (200, 30, 30), (30, 30, 200)
    x = np.empty((1, 2, 4, 2), np.float32)
    x[:, :, :2], x[:, :, 2:] = (4, -4), (-4, 4)
    lab, _, _ = _device(pkg, ctx, x, _reduce(ctx, hi, 32), hi, 24.0, prob=False)
    assert np.array_equal(lab[0], np.broadcast_to(np.arange(128) >= 50, (64, 128)).astype(np.int32))
    d_x, d_lab = ctx.to_device(x), ctx.alloc(64 * 128 * 4)
    ctx.resample_argmax(d_lab.ptr, None, d_x.ptr, 1, 2, 4, 2, 64, 128)
    ctx.sync()
    assert np.array_equal(d_lab.download((64, 128), np.int32), np.broadcast_to(np.arange(128) >= 64, (64, 128)).astype(np.int32))
    d_x.free(), d_lab.free()


def test_a_flat_guide_is_the_bilinear_read_out(pkg, ctx):
    n, h, w, classes, H, W = 2, 3, 5, 8, 33, 70
    x = np.random.default_rng(11).standard_normal((n, h, w, classes)).astype(np.float32)
    top, tol = np.sort(dense_any_ref.resample(x, H, W), axis=-1), ref.tolerance(x)
    assert (top[..., -1] - top[..., -2]).min() > 2 * tol, "the logits of this test must keep the top two classes apart (another seed)"
    lo, hi = np.full((n, h, w, 3), 77, np.uint8), np.full((n, H, W, 3), 77, np.uint8)
    lab, sc, _ = _device(pkg, ctx, x, lo, hi, 24.0, prob=False)
    want_lab, want_sc = dense_any_ref.resample_argmax(x, H, W)
    assert np.array_equal(lab, want_lab) and float(np.abs(sc.view(np.float32).astype(np.float64) - want_sc).max()) <= tol


def test_refusals_launch_nothing(pkg, ctx):
    n, h, w, classes, H, W = 1, 3, 5, 4, 33, 70
    d_x, d_lo, d_hi = ctx.alloc(n * h * w * classes * 4), ctx.alloc(n * h * w * 3), ctx.alloc(n * H * W * 3)
    d_lut = ctx.to_device(np.concatenate([pkg.guided_lut(24.0), np.ones(1, np.float32)]))
    d_lab, d_sc = ctx.to_device(np.full(n * H * W, LAB_FILL, np.int32)), ctx.to_device(np.full(n * H * W, SC_FILL, np.float32))
    def call(lo=d_lo.ptr, hi=d_hi.ptr, lut=d_lut.ptr, classes=classes, H=H):
        return ctx.lib.mbn_resample_guided_f32(ctx.h, d_lab.ptr, None, d_sc.ptr, d_x.ptr, lo, hi, lut, n, h, w, classes, 0, 0, None, H, W, 0.0, 0, None)
    assert call(H=4 * h - 1) == pkg.EUNSUPPORTED
    assert call(lo=None) == pkg.EINVAL and call(hi=None) == pkg.EINVAL and call(lut=None) == pkg.EINVAL
    assert call(lut=d_lut.ptr + 2) == pkg.EINVAL and call(classes=0) == pkg.EINVAL
    assert ctx.lib.mbn_guide_reduce_u8(ctx.h, d_lab.ptr, d_hi.ptr, 1, 64, 96, 5, None) == pkg.EINVAL       # a stride that does not divide
    ctx.sync()
    assert (d_lab.download((n * H * W,), np.int32) == LAB_FILL).all() and (d_sc.download((n * H * W,), np.float32) == SC_FILL).all()
    [b.free() for b in (d_x, d_lo, d_hi, d_lut, d_lab, d_sc)]


@pytest.mark.parametrize("dtype,cus", [("f32", 0), ("f32", 1), ("f32", 3), ("bf16", 0)])
def test_net_segment_guided_fit(pkg, ctx, tmp_path, dtype, cus):
    CLASSES, ROWS, COLS, STRIDE, SIGMA, n, sh, sw, h, w = 11, 64, 96, 32, 24.0, 2, 75, 130, 2, 3
    hw = _weights_os(pkg, tmp_path, 0.25, ROWS, COLS, CLASSES, STRIDE)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_dtype(pkg.DT_BF16 if dtype == "bf16" else pkg.DT_F32)
    net.set_input_u8(True)
    npix, d_src = n * sh * sw, ctx.to_device(np.random.default_rng(5).integers(0, 256, (n, sh, sw, 3), dtype=np.uint8))
    d_dense, d_lo, d_lut = ctx.alloc(n * h * w * CLASSES * 4), ctx.alloc(n * h * w * 3), ctx.to_device(pkg.guided_lut(SIGMA))
    outs = [ctx.to_device(np.full(npix + TAIL, f, t)) for _ in range(2) for f, t in ((LAB_FILL, np.int32), (SC_FILL, np.float32), (SC_FILL, np.float32))]
    try:
        assert ctx.lib.mbn_set_planning_cus(ctx.h, cus) == pkg.OK
        lib, a = ctx.lib, (net.h, d_src.ptr, n, sh, sw)
        assert lib.mbn_net_segment_guided_fit(*a, pkg.FIT_CROP, SIGMA, outs[0].ptr, None, None, 0.0, 0) == pkg.EUNSUPPORTED       # then sigma = 0
        assert lib.mbn_net_segment_guided_fit(*a, pkg.FIT_PAD, 0.0, outs[0].ptr, None, None, 0.0, 0) == pkg.EINVAL
        for fit in (pkg.FIT_STRETCH, pkg.FIT_PAD):
            net.segment_guided_fit(d_src.ptr, n, sh, sw, fit, SIGMA, outs[0].ptr, outs[2].ptr, outs[1].ptr)
            staging = net.resize_input(d_src.ptr, n, sh, sw, fit=fit)
            ctx.guide_reduce(d_lo.ptr, staging, n, ROWS, COLS, STRIDE)
            net.forward_dense(staging, d_dense.ptr, n)
            ctx.resample_guided(outs[3].ptr, outs[5].ptr, outs[4].ptr, d_dense.ptr, d_lo.ptr, d_src.ptr, d_lut.ptr, n, h, w, CLASSES, sh, sw, ROWS, COLS,
                                tuple(pkg.fit_pad(sh, sw, ROWS, COLS)) if fit == pkg.FIT_PAD else None)
            ctx.sync()
            got, want = ([b.download((npix + TAIL,), np.uint32) for b in outs[i:i + 3]] for i in (0, 3))
            assert all(np.array_equal(g, v) for g, v in zip(got, want)), "%s fit %d at %d planning CUs differs from the chain" % (dtype, fit, cus)
            assert (got[0][npix:].view(np.int32) == LAB_FILL).all() and got[1][:npix].view(np.float32).std() > 0
    finally:
        assert ctx.lib.mbn_set_planning_cus(ctx.h, 0) == pkg.OK
        net.destroy()
        [b.free() for b in [d_src, d_dense, d_lo, d_lut] + outs]
        hw.free()
