"""Non-square inputs (rows x cols, multiples of 32) on the GPU: the network against the oracle per layer, the fused runner against one
launch per layer bit for bit, the fused blocks, the stem, the bf16 resident run and tail, int8, the pool, classify, streams and the C host.

The oracle's net_forward and pool are square-only, so the reference here chains its per-layer functions from the device plan's
descriptors and computes the pool as a mean over the plane."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import int8_ref as ref

pytestmark = pytest.mark.gpu

TOL_DW = 1e-5
TOL_PW = 1e-4
TOL_NET = 1e-3
TOL_BF16 = 1e-2
TOL_BF16_NET = 2e-2


def assert_close(got, want, rtol, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), what
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    assert err <= rtol * scale + 1e-7, "%s: max abs err %.3e vs scale %.3e (rel %.3e > %.1e)" % (what, err, scale, err / scale, rtol)


def _weights(pkg, tmp_path, alpha, rows, cols, classes, seed=3):
    path = str(tmp_path / ("w_%g_%dx%d_%d.h5" % (alpha, rows, cols, classes)))
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    return pkg.HostWeights(path, res=(rows, cols), lib=pkg.load())


def _images(n, rows, cols, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, rows, cols, 3)).astype(np.float32)


def _bf16_dev(pkg, ctx, x):
    return ctx.to_device(pkg.f32_to_bf16_bits(x))


def _bf16_get(pkg, buf, shape):
    return pkg.bf16_bits_to_f32(buf.download(shape, np.uint16))


def _oracle_layer(orc, plan, blob, i, x, bf16=False):
    """Layer i+1 of the (device) plan applied to x by the oracle's per-layer functions; the pool is a mean over the plane."""
    l = plan.layer[i]
    w = blob[l.w_offset:l.w_offset + max(l.w_count, 0)]
    sc = blob[l.scale_offset:l.scale_offset + l.out_ch] if l.scale_offset >= 0 else None
    sh = blob[l.shift_offset:l.shift_offset + l.out_ch] if l.shift_offset >= 0 else None
    n = x.shape[0]
    if l.kind == orc.L_CONV:
        y = orc.f32_conv(x, w.reshape(3, 3, 3, l.out_ch), sc, sh, l.stride, orc.ACT_RELU6, pad_top=l.pad_top, pad_left=l.pad_left)
    elif l.kind == orc.L_DW:
        y = orc.f32_depthwise(x, w.reshape(3, 3, l.out_ch), sc, sh, l.stride, orc.ACT_RELU6, out_rows=l.out_rows, out_cols=l.out_cols,
                              pad_top=l.pad_top, pad_left=l.pad_left)
    elif l.kind == orc.L_PW:
        wm = w.reshape(l.out_ch, l.in_ch)
        y = orc.f32_pointwise(x, orc.bf16_round(wm) if bf16 else wm, sc, sh, orc.ACT_RELU6).reshape(n, l.out_rows, l.out_cols, l.out_ch)
    elif l.kind == orc.L_POOL:
        assert x.shape[1:3] == (l.in_rows, l.in_cols)
        y = x.astype(np.float64).mean(axis=(1, 2)).astype(np.float32).reshape(n, 1, 1, l.out_ch)
    else:
        wm = w.reshape(l.out_ch, l.in_ch)
        return orc.f32_pointwise(x.reshape(n, -1), orc.bf16_round(wm) if bf16 else wm, None, sh, orc.ACT_NONE).reshape(n, 1, 1, l.out_ch)
    return orc.bf16_round(y) if bf16 else y


# ------------------------------------------------------------------------------------------------------------ fp32 network

@pytest.mark.parametrize("alpha,rows,cols,n", [(1.0, 224, 320, 2), (0.5, 96, 160, 3), (0.25, 64, 128, 4), (1.0, 128, 96, 6)])
def test_net_per_layer_vs_oracle(pkg, orc, ctx, tmp_path, alpha, rows, cols, n):
    classes = 50
    hw = _weights(pkg, tmp_path, alpha, rows, cols, classes)
    plan = hw.plan
    assert plan.res == 0 and (plan.layer[0].in_rows, plan.layer[0].in_cols) == (rows, cols)
    net = pkg.Net(ctx, plan, hw.blob.copy(), n)
    net.keep_activations(True)
    imgs = _images(n, rows, cols, 1)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * classes * 4)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    logits = d_out.download((n, 1, 1, classes), np.float32)
    prev = imgs
    for i in range(plan.n_layers):
        l = plan.layer[i]
        got = logits if i == plan.n_layers - 1 else net.layer_output(i + 1, n).reshape(n, l.out_rows, l.out_cols, l.out_ch)
        want = _oracle_layer(orc, plan, hw.blob, i, prev)
        assert_close(got, want, TOL_NET, "%gx%dx%d layer %d" % (alpha, rows, cols, i + 1))
        prev = got
    net.destroy()
    hw.free()


@pytest.mark.parametrize("n", [7, 24])
@pytest.mark.parametrize("rows,cols", [(224, 320), (320, 224)])
def test_net_fused_equals_unfused(pkg, ctx, tmp_path, rows, cols, n):
    """The default runner (fused stem, fused blocks) and one launch per layer give the same bits on a non-square 1.0 network; so does
    the uint8 front-end. At batch 24 the launches group as the square network's."""
    hw = _weights(pkg, tmp_path, 1.0, rows, cols, 1000)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    sq = _weights(pkg, tmp_path, 1.0, 224, 224, 1000)
    sqnet = pkg.Net(ctx, pkg.plan_build(1.0, 224, 1000), sq.blob.copy(), n)
    spans = [c for _, c in net.launches(n)]
    if n == 24:
        assert spans == [c for _, c in sqnet.launches(n)]
        assert spans[:5] == [3, 2, 2, 2, 2]
    assert spans[0] == 3
    sqnet.destroy()
    u8 = np.random.default_rng(99).integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)
    d_u, d_f = ctx.to_device(u8), ctx.alloc(u8.size * 4)
    assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, d_f.ptr, d_u.ptr, u8.size, 1 / 127.5, -1.0, None) == 0
    d_a, d_b, d_c = ctx.alloc(n * 4000), ctx.alloc(n * 4000), ctx.alloc(n * 4000)
    net.forward(d_f.ptr, d_a.ptr, n)
    net.set_fuse_stem(False)
    net.set_fuse_blocks(0)
    assert len(net.launches(n)) == 29
    net.forward(d_f.ptr, d_b.ptr, n)
    net.set_fuse_stem(True)
    net.set_fuse_blocks(0xFFFFFFFE)
    net.set_input_u8(True)
    net.forward(d_u.ptr, d_c.ptr, n)
    ctx.sync()
    a, b, c = (d.download((n, 1000), np.float32) for d in (d_a, d_b, d_c))
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
    assert np.array_equal(a, b) and np.array_equal(a, c)
    net.destroy()
    hw.free()
    sq.free()


# ------------------------------------------------------------------------------------------------------------ fused blocks

_MAPS = [((112, 160), 64, 128), ((56, 80), 128, 256), ((28, 40), 256, 256), ((14, 20), 512, 512)]
BLOCK_SHAPES = [(2, h, w, cin, cout, s) for (hh, ww), cin, cout in _MAPS for h, w in ((hh, ww), (ww, hh)) for s in (1, 2)] + \
               [(1, 7, 10, 128, 128, 1), (3, 10, 8, 128, 128, 1), (1, 14, 20, 64, 128, 2)]      # ragged pixel counts (m % 32 != 0)


def _block_case(rng, n, h, w, cin, cout, stride):
    x = rng.uniform(0, 4, (n, h, w, cin)).astype(np.float32)
    wd = rng.normal(0, 0.5, (3, 3, cin)).astype(np.float32)
    wp = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    s2, s3 = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b2, b3 = rng.normal(0, 0.1, cin).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    oh, ow = (h + stride - 1) // stride, (w + stride - 1) // stride
    pt = max((oh - 1) * stride + 3 - h, 0) // 2
    pl = max((ow - 1) * stride + 3 - w, 0) // 2
    return x, wd, wp, s2, b2, s3, b3, oh, ow, pt, pl


@pytest.mark.parametrize("shape", BLOCK_SHAPES)
def test_f32_dwpw_fused_non_square(pkg, orc, ctx, shape):
    n, h, w, cin, cout, stride = shape
    rng = np.random.default_rng(h * 7 + w + cin + stride)
    x, wd, wp, s2, b2, s3, b3, oh, ow, pt, pl = _block_case(rng, n, h, w, cin, cout, stride)
    mid = orc.f32_depthwise(x, wd, s2, b2, stride, 2, out_rows=oh, out_cols=ow, pad_top=pt, pad_left=pl)
    want = orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(n, oh, ow, cout)
    d = [ctx.to_device(a) for a in (x, wd, s2, b2, wp, s3, b3)]
    d_f, d_m, d_u = ctx.alloc(want.nbytes), ctx.alloc(mid.nbytes), ctx.alloc(want.nbytes)
    rc = ctx.lib.mbn_dwpw_fused(ctx.h, d_f.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr,
                                n, h, w, oh, ow, cin, cout, stride, pt, pl, None)
    if ow % 2:                       # an odd output row (20 x 14 -> 10 x 7) is outside the envelope: the runner issues two launches
        assert rc == pkg.EUNSUPPORTED, rc
        return
    assert rc == 0, rc
    ctx.depthwise(d_m.ptr, d[0].ptr, d[1].ptr, oh, ow, 3, stride, cin,
                  pkg.make_ext(batch=n, act=2, pad_top=pt, pad_left=pl, in_rows=h, in_cols=w, scale=d[2].ptr, shift=d[3].ptr))
    try:   # the pointwise layer on pw_gemm: the summation order of the fused blocks
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 1) == 0
        ctx.pointwise(d_u.ptr, d_m.ptr, d[4].ptr, n * oh * ow, 1, cin, cout, pkg.make_ext(batch=1, act=2, scale=d[5].ptr, shift=d[6].ptr))
    finally:
        ctx.lib.mbn_tune_set(b"pw_splitk", 0)
    ctx.sync()
    fused, sep = d_f.download(want.shape, np.float32), d_u.download(want.shape, np.float32)
    assert_close(fused, want, TOL_PW, "fp32 block %s vs oracle" % (shape,))
    assert np.array_equal(fused, sep), "fp32 block %s differs from depthwise + pointwise by %g" % (shape, np.abs(fused - sep).max())
    for b in d + [d_f, d_m, d_u]:
        b.free()


@pytest.mark.parametrize("shape", BLOCK_SHAPES)
def test_bf16_dwpw_fused_non_square(pkg, orc, ctx, shape):
    n, h, w, cin, cout, stride = shape
    rng = np.random.default_rng(h * 13 + w + cin + stride)
    x, wd, wp, s2, b2, s3, b3, oh, ow, pt, pl = _block_case(rng, n, h, w, cin, cout, stride)
    x, wp = orc.bf16_round(x), orc.bf16_round(wp)
    mid = orc.bf16_round(orc.f32_depthwise(x, wd, s2, b2, stride, 2, out_rows=oh, out_cols=ow, pad_top=pt, pad_left=pl))
    want = orc.bf16_round(orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(n, oh, ow, cout))
    d_x, d_wp = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, wp)
    d = [ctx.to_device(a) for a in (wd, s2, b2, s3, b3)]
    d_f, d_m, d_u = ctx.alloc(want.size * 2), ctx.alloc(mid.size * 2), ctx.alloc(want.size * 2)
    rc = ctx.lib.mbn_dwpw_fused_bf16(ctx.h, d_f.ptr, d_x.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d_wp.ptr, d[3].ptr, d[4].ptr,
                                     n, h, w, oh, ow, cin, cout, stride, pt, pl, None)
    if ow % 2:
        assert rc == pkg.EUNSUPPORTED, rc
        return
    assert rc == 0, rc
    ctx.depthwise(d_m.ptr, d_x.ptr, d[0].ptr, oh, ow, 3, stride, cin,
                  pkg.make_ext(batch=n, dtype=pkg.DT_BF16, act=2, pad_top=pt, pad_left=pl, in_rows=h, in_cols=w, scale=d[1].ptr, shift=d[2].ptr))
    ctx.pointwise(d_u.ptr, d_m.ptr, d_wp.ptr, n * oh * ow, 1, cin, cout, pkg.make_ext(batch=1, dtype=pkg.DT_BF16, act=2, scale=d[3].ptr, shift=d[4].ptr))
    ctx.sync()
    fused, sep = _bf16_get(pkg, d_f, want.shape), _bf16_get(pkg, d_u, want.shape)
    assert_close(fused, want, TOL_BF16, "bf16 block %s vs oracle" % (shape,))
    assert_close(fused, sep, TOL_BF16, "bf16 block %s vs separate launches" % (shape,))
    for b in d + [d_x, d_wp, d_f, d_m, d_u]:
        b.free()


# ------------------------------------------------------------------------------------------------------------ stem

def _stem_call(ctx, hw, d_out, d_img, n, rows, cols, flags, wp_ptr=None):
    L = hw.plan.layer
    blob = hw._dev

    def at(off):
        return blob.ptr + off * 4
    return ctx.lib.mbn_stem_fused_hw(ctx.h, d_out.ptr, d_img.ptr, at(L[0].w_offset), at(L[0].scale_offset), at(L[0].shift_offset),
                                     at(L[1].w_offset), at(L[1].scale_offset), at(L[1].shift_offset),
                                     wp_ptr if wp_ptr is not None else at(L[2].w_offset), at(L[2].scale_offset), at(L[2].shift_offset),
                                     n, rows, cols, L[0].out_ch, L[2].out_ch, flags, None)


@pytest.mark.parametrize("form", ["f32", "u8", "bf16", "emul6"])
@pytest.mark.parametrize("alpha,rows,cols,n", [(1.0, 224, 320, 2), (1.0, 96, 64, 3), (0.5, 160, 128, 2), (0.5, 64, 160, 3)])
def test_stem_hw_equals_three_layers_and_oracle(pkg, orc, ctx, tmp_path, form, alpha, rows, cols, n):
    hw = _weights(pkg, tmp_path, alpha, rows, cols, 20)
    hw._dev = ctx.to_device(hw.blob)
    c3 = hw.plan.layer[2].out_ch
    oh, ow = rows // 2, cols // 2
    bf = form == "bf16"
    rng = np.random.default_rng(rows * 3 + cols)
    u8 = rng.integers(0, 256, (n, rows, cols, 3), dtype=np.uint8)
    if form == "u8":                                   # the separate layers read the image normalised by the library's own pass
        d_img, d_f32 = ctx.to_device(u8), ctx.alloc(u8.size * 4)
        assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, d_f32.ptr, d_img.ptr, u8.size, 1 / 127.5, -1.0, None) == 0
        ctx.sync()
        imgs = d_f32.download(u8.shape, np.float32)
    else:
        imgs = _images(n, rows, cols, 4)
        d_img = d_f32 = ctx.to_device(imgs)
    es = 2 if bf else 4
    d_a, d_b = ctx.alloc(n * oh * ow * c3 * es), ctx.alloc(n * oh * ow * c3 * es)
    net = pkg.Net(ctx, hw.plan, hw._dev.ptr, n)
    if bf:
        net.set_dtype(pkg.DT_BF16)
    if form == "emul6":
        assert ctx.lib.mbn_tune_set(b"pw_emul", 6) == 0
    try:
        wp_ptr = None
        if bf:
            wp = hw.blob[hw.plan.layer[2].w_offset:hw.plan.layer[2].w_offset + hw.plan.layer[2].w_count]
            d_wp = _bf16_dev(pkg, ctx, wp)
            wp_ptr = d_wp.ptr
        flags = (1 if form == "u8" else 0) | (2 if bf else 0)
        assert _stem_call(ctx, hw, d_a, d_img, n, rows, cols, flags, wp_ptr) == 0
        net.set_fuse_stem(False)
        net.forward(d_f32.ptr, d_b.ptr, n, 3)                  # conv1, dw2, pw3 as separate launches
        ctx.sync()
        if bf:
            fused, sep = _bf16_get(pkg, d_a, (n, oh, ow, c3)), _bf16_get(pkg, d_b, (n, oh, ow, c3))
        else:
            fused, sep = d_a.download((n, oh, ow, c3), np.float32), d_b.download((n, oh, ow, c3), np.float32)
        x = imgs
        for i in range(3):
            x = _oracle_layer(orc, hw.plan, hw.blob, i, x, bf)
        if bf:
            assert_close(fused, x, 2 * TOL_BF16, "bf16 stem vs oracle")
            assert_close(fused, sep, 2 * TOL_BF16, "bf16 stem vs separate launches")
        else:
            assert_close(fused, x, TOL_PW, "stem vs oracle")
            if form != "emul6":           # split products: the stem's and the separate GEMM's forms are compared in their own tests
                assert np.array_equal(fused, sep), "stem differs from three layers by %g" % np.abs(fused - sep).max()
        # through the runner: the fused stem at rows x cols, the same bits as the direct call
        net.set_fuse_stem(True)
        assert net.fused_layers(3) == 3
        net.forward(d_f32.ptr, d_b.ptr, n, 3)
        ctx.sync()
        assert np.array_equal(d_a.download((n * oh * ow * c3 * es,), np.uint8), d_b.download((n * oh * ow * c3 * es,), np.uint8))
    finally:
        ctx.lib.mbn_tune_set(b"pw_emul", 0)
    net.destroy()
    hw.free()


@pytest.mark.parametrize("flags", [0, 1, 2])
@pytest.mark.parametrize("alpha,res", [(1.0, 224), (0.5, 160), (1.0, 64)])
def test_stem_hw_square_equals_stem_ex(pkg, ctx, tmp_path, flags, alpha, res):
    hw = _weights(pkg, tmp_path, alpha, res, res, 20)
    hw._dev = ctx.to_device(hw.blob)
    L = hw.plan.layer
    c3, n, oh = L[2].out_ch, 3, res // 2
    u8 = np.random.default_rng(res).integers(0, 256, (n, res, res, 3), dtype=np.uint8)
    d_img = ctx.to_device(u8 if flags & 1 else (u8.astype(np.float32) / np.float32(127.5) - np.float32(1)).astype(np.float32))
    wp_ptr = _bf16_dev(pkg, ctx, hw.blob[L[2].w_offset:L[2].w_offset + L[2].w_count]).ptr if flags & 2 else None
    nb = n * oh * oh * c3 * (2 if flags & 2 else 4)
    d_a, d_b = ctx.alloc(nb), ctx.alloc(nb)
    assert _stem_call(ctx, hw, d_a, d_img, n, res, res, flags, wp_ptr) == 0

    def at(off):
        return hw._dev.ptr + off * 4
    rc = ctx.lib.mbn_stem_fused_ex(ctx.h, d_b.ptr, d_img.ptr, at(L[0].w_offset), at(L[0].scale_offset), at(L[0].shift_offset),
                                   at(L[1].w_offset), at(L[1].scale_offset), at(L[1].shift_offset), wp_ptr or at(L[2].w_offset),
                                   at(L[2].scale_offset), at(L[2].shift_offset), n, res, L[0].out_ch, c3, flags, None)
    assert rc == 0
    ctx.sync()
    assert np.array_equal(d_a.download((nb,), np.uint8), d_b.download((nb,), np.uint8))
    # sides that are not multiples of 32 are refused
    assert _stem_call(ctx, hw, d_a, d_img, 1, 64, 48, flags, wp_ptr) == pkg.EUNSUPPORTED
    hw.free()


# ------------------------------------------------------------------------------------------------------------ bf16

def test_bf16_net_224x320_vs_oracle_chain(pkg, orc, ctx, tmp_path):
    n, classes, rows, cols = 16, 64, 224, 320
    hw = _weights(pkg, tmp_path, 1.0, rows, cols, classes)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_dtype(pkg.DT_BF16)
    imgs = _images(n, rows, cols, 5)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * classes * 4)
    assert [c for _, c in net.launches(n)][0] == 3
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    got = d_out.download((n, 1, 1, classes), np.float32)
    x = imgs
    for i in range(hw.plan.n_layers):
        x = _oracle_layer(orc, hw.plan, hw.blob, i, x, True)
    assert_close(got, x, TOL_BF16_NET, "bf16 1.0x224x320 logits vs the oracle's bf16 chain")
    net.destroy()
    hw.free()


@pytest.mark.parametrize("rows,cols", [(160, 128), (128, 160)])
def test_bf16_resident_run_and_tail_non_square(pkg, ctx, tmp_path, rows, cols):
    n, classes = 24, 100
    hw = _weights(pkg, tmp_path, 0.5, rows, cols, classes)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_dtype(pkg.DT_BF16)
    launches = net.launches(n)
    spans = [c for _, c in launches]
    assert (14, 10) in launches, launches            # the five 256 -> 256 blocks on the 10 x 8 map, resident in LDS
    assert (24, 5) in launches, launches             # the last two blocks + pool on the 10 x 8 input
    assert spans[0] == 3
    imgs = _images(n, rows, cols, 8)
    d_in, d_a, d_b = ctx.to_device(imgs), ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    net.forward(d_in.ptr, d_a.ptr, n)
    net.set_fuse_resident(False)
    assert (14, 10) not in net.launches(n) and (24, 5) not in net.launches(n)
    net.forward(d_in.ptr, d_b.ptr, n)
    ctx.sync()
    a, b = d_a.download((n, classes), np.float32), d_b.download((n, classes), np.float32)
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
    assert_close(a, b, TOL_BF16_NET, "bf16 resident run + tail vs separate blocks")
    net.destroy()
    hw.free()


# ------------------------------------------------------------------------------------------------------------ int8

@pytest.mark.parametrize("alpha,rows,cols", [(1.0, 224, 320), (0.5, 160, 96)])
def test_int8_every_layer_bit_exact(pkg, ctx, tmp_path, alpha, rows, cols):
    classes, n = 40, 3
    hw = _weights(pkg, tmp_path, alpha, rows, cols, classes, seed=7)
    plan = hw.plan
    net = pkg.Net(ctx, plan, hw.blob.copy(), 8)
    d_cal = ctx.to_device(_images(8, rows, cols, 99))
    net.calibrate_i8(d_cal.ptr, 8)
    assert net.get_act_scales_i8()[0] != np.float32(6 / 255.0)
    imgs = _images(n, rows, cols, 3)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * classes * 4)
    net.set_dtype(pkg.DT_I8)
    net.keep_activations(True)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    got = d_out.download((n, classes), np.float32)
    scales = net.get_act_scales_i8()
    q = ref.quantize(plan, hw.blob, scales)
    l0 = plan.layer[0]
    conv = net.layer_output(1, n).astype(np.int64)
    assert conv.shape == (n, rows // 2, cols // 2, l0.out_ch)
    y = ref.conv1_y(imgs.astype(np.float64), hw.blob[l0.w_offset:l0.w_offset + l0.w_count].reshape(3, 3, 3, -1), q[0]["mult"], q[0]["bias"])
    want = np.clip(np.rint(y), 0, 255).astype(np.int64)
    assert np.abs(conv - want).max() <= 1 and (conv != want).mean() < 1e-3
    ref.assert_conv1_one_step(conv, y, "layer 1")          # and the mismatches only at half-integers of y
    prev = net.layer_output(1, n)
    for i in range(2, plan.n_layers + 1):
        l = plan.layer[i - 1]
        want = ref.layer_from_prev(l, q[i - 1], prev)
        dev = net.layer_output(i, n) if i < plan.n_layers else got
        assert np.array_equal(dev.reshape(want.shape).view(np.uint8 if dev.dtype == np.uint8 else np.uint32),
                              want.view(np.uint8 if want.dtype == np.uint8 else np.uint32)), "layer %d" % i
        prev = dev.reshape(want.shape) if l.kind != ref.L_POOL else dev.reshape(n, 1, 1, l.out_ch)
    assert np.isfinite(got).all() and got.std() > 0
    net.destroy()
    hw.free()


# ------------------------------------------------------------------------------------------------------------ pool

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows,cols,ch", [(7, 10, 1024), (10, 7, 512), (5, 4, 256), (7, 7, 64)])
def test_pool_non_square_is_the_sequential_sum(pkg, ctx, dtype, rows, cols, ch):
    n = 3
    rng = np.random.default_rng(rows * 10 + cols)
    x = rng.uniform(0, 6, (n, rows, cols, ch)).astype(np.float32)
    bf = dtype == "bf16"
    if bf:
        x = pkg.bf16_bits_to_f32(pkg.f32_to_bf16_bits(x))
    acc = np.zeros((n, ch), np.float32)
    for y in range(rows):                    # the kernel's order: rows outer, columns inner, left to right, fp32
        for xx in range(cols):
            acc = (acc + x[:, y, xx, :]).astype(np.float32)
    want = (acc / np.float32(rows * cols)).astype(np.float32)
    d_x = _bf16_dev(pkg, ctx, x) if bf else ctx.to_device(x)
    d_o = ctx.alloc(n * ch * 4)
    ctx.pool(d_o.ptr, d_x.ptr, rows, cols, max(rows, cols), ch,
             pkg.make_ext(batch=n, dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=pkg.ACT_NONE))
    ctx.sync()
    if bf:
        got = d_o.download((n, ch), np.uint16)
        assert np.array_equal(got, pkg.f32_to_bf16_bits(want))
    else:
        got = d_o.download((n, ch), np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()


def test_pool_fc_one_launch_on_a_224x320_net(pkg, ctx, tmp_path):
    n, classes = 2, 1000
    hw = _weights(pkg, tmp_path, 1.0, 224, 320, classes)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    imgs = _images(n, 224, 320, 6)
    d_in, d_a, d_b = ctx.to_device(imgs), ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    net.forward(d_in.ptr, d_a.ptr, n)
    net.set_fuse_tail(True)
    assert net.launches(n)[-1] == (28, 2)
    net.forward(d_in.ptr, d_b.ptr, n)
    ctx.sync()
    a, b = d_a.download((n, classes), np.float32), d_b.download((n, classes), np.float32)
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
    assert_close(b, a, 1e-5, "pool + FC as one launch vs two")
    net.destroy()
    hw.free()


# ------------------------------------------------------------------------------------------------------------ classify, streams, C host

def test_classify_and_streams_non_square(pkg, ctx, tmp_path):
    n, classes, k = 24, 1000, 5
    hw = _weights(pkg, tmp_path, 1.0, 224, 320, classes)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    imgs = _images(n, 224, 320, 12)
    d_in, d_a, d_b = ctx.to_device(imgs), ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    d_idx, d_prob = ctx.alloc(n * k * 4), ctx.alloc(n * k * 4)
    net.forward(d_in.ptr, d_a.ptr, n)
    net.classify(d_in.ptr, n, k, d_idx.ptr, d_prob.ptr)
    net.set_streams(2)
    net.forward(d_in.ptr, d_b.ptr, n)
    ctx.sync()
    a, b = d_a.download((n, classes), np.float32), d_b.download((n, classes), np.float32)
    assert np.array_equal(a, b), "two streams differ from one"
    idx = d_idx.download((n, k), np.int32)
    assert np.array_equal(idx[:, 0], a.argmax(axis=1))
    order = np.argsort(-a, axis=1, kind="stable")[:, :k]
    assert np.array_equal(np.sort(idx, axis=1), np.sort(order, axis=1))
    net.destroy()
    hw.free()


def test_c_host_non_square_ppm(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    rows, cols, seed = 224, 320, 5
    img = np.random.default_rng(21).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    ppm = str(tmp_path / "frame.ppm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), img.ctypes.data, cols, rows) == 0     # 320 wide, 224 high
    r = subprocess.run([exe, "--synthetic", str(seed), "--res", "%dx%d" % (rows, cols), "--ppm", ppm], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "warning" not in r.stderr, r.stderr
    m = re.search(r"present at location (\d+) and it's value is ([0-9]+\.[0-9]+)", r.stdout)
    assert m, r.stdout
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=1.0, classes=1000, seed=seed, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(rows, cols), lib=pkg.load())
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 1)
    net.set_input_u8(True)
    d_in, d_out = ctx.to_device(img.reshape(1, rows, cols, 3)), ctx.alloc(4000)
    net.forward(d_in.ptr, d_out.ptr, 1)
    ctx.sync()
    logits = d_out.download((1000,), np.float32)
    assert int(m.group(1)) == int(logits.argmax()) + 1
    net.destroy()
    hw.free()
