"""output_stride 16 / 8 on the GPU: mbn_depthwise with ext.dilation against the oracle and, bit for bit, against the same call made
with a zero-inflated (2D+1) x (2D+1) filter on the generic kernel; the output-stride networks per layer against the oracle chain; the
launch grouping (no fused launch covers a dilated layer) and its bits; layer-27 features; classify; the int8 refusal; the C host.

The oracle has no dilation: a rate-D 3x3 filter is its (2D+1)^2 filter with zeros between the taps (pinned against torch in
test_dilation_cpu.py). Inputs of the depthwise cases are uniform in [-1, 1], so the fmaf(x, 0, acc) the inflated route inserts are exact
and the two device routes must agree in every bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_dilation_cpu import inflate
from test_rect_gpu import TOL_BF16, TOL_BF16_NET, TOL_DW, TOL_NET, _bf16_dev, _images, _oracle_layer, assert_close

pytestmark = pytest.mark.gpu


def _same_pad(inp, out, k, stride):
    return max((out - 1) * stride + k - inp, 0) // 2


def _dw_inputs(orc, n, h, w, c, bf, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (n, h, w, c)).astype(np.float32)
    f = rng.uniform(-1, 1, (3, 3, c)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, c).astype(np.float32)
    sh = rng.normal(0, 0.1, c).astype(np.float32)
    return (orc.bf16_round(x) if bf else x), f, sc, sh


def _dw_both_routes(pkg, orc, ctx, n, h, w, c, d, bf=False, stride=1, pads=None, seed=0):
    """(a) ext.dilation = d with a 3x3 filter, (b) the parent-commit way: filtersize 2d+1, zero-inflated filter, explicit pads, no
    dilation (the generic kernel). Returns (a, b, oracle) as float32 arrays plus the raw device bits of (a) and (b)."""
    x, f, sc, sh = _dw_inputs(orc, n, h, w, c, bf, seed + 31 * h + w + c + d)
    oh, ow = -(-h // stride), -(-w // stride)
    k = 2 * d + 1
    pt, pl = pads if pads is not None else (_same_pad(h, oh, k, stride), _same_pad(w, ow, k, stride))
    fi = inflate(f, d)
    want = orc.f32_depthwise(x, fi, sc, sh, stride, orc.ACT_RELU6, out_rows=oh, out_cols=ow, pad_top=pt, pad_left=pl)
    dt, es, raw = (pkg.DT_BF16, 2, np.uint16) if bf else (pkg.DT_F32, 4, np.uint32)
    d_x = _bf16_dev(pkg, ctx, x) if bf else ctx.to_device(x)
    d_f, d_fi, d_sc, d_sh = (ctx.to_device(a) for a in (f, fi, sc, sh))
    d_a, d_b = ctx.alloc(want.size * es), ctx.alloc(want.size * es)
    common = dict(batch=n, dtype=dt, act=pkg.ACT_RELU6, in_rows=h, in_cols=w, scale=d_sc.ptr, shift=d_sh.ptr)
    ea = pkg.make_ext(dilation=d, **(dict(pad_top=pt, pad_left=pl) if pads is not None else {}), **common)   # pads -1: SAME of the window 2d+1
    ctx.depthwise(d_a.ptr, d_x.ptr, d_f.ptr, oh, ow, 3, stride, c, ea)
    ctx.depthwise(d_b.ptr, d_x.ptr, d_fi.ptr, oh, ow, k, stride, c, pkg.make_ext(pad_top=pt, pad_left=pl, **common))
    ctx.sync()
    ra, rb = d_a.download(want.shape, raw), d_b.download(want.shape, raw)
    for b in (d_x, d_f, d_fi, d_sc, d_sh, d_a, d_b):
        b.free()
    val = pkg.bf16_bits_to_f32 if bf else (lambda r: r.view(np.float32))
    return val(ra), val(rb), want, ra, rb


# (batch, rows, cols, C, D)
F32_CASES = [(1, 14, 14, 64, 2),        # one image: segmented marches
             (3, 5, 7, 4, 2),           # minimum channels, odd cols, ragged phases
             (2, 3, 3, 8, 4),           # map smaller than the dilation: eight taps fall entirely in padding
             (2, 9, 6, 36, 4),          # cw not a power of two
             (6, 28, 28, 512, 2),       # several slabs
             (2, 7, 7, 1024, 4),
             (2, 10, 9, 6, 2)]          # channels % 4 != 0: the generic path
BF16_CASES = F32_CASES[:-1] + [(2, 6, 5, 8, 2), (2, 6, 5, 12, 4)]


@pytest.mark.parametrize("case", F32_CASES)
def test_depthwise_dilated_f32(pkg, orc, ctx, case):
    n, h, w, c, d = case
    a, b, want, ra, rb = _dw_both_routes(pkg, orc, ctx, n, h, w, c, d)
    assert float(np.abs(want).max()) > 0
    assert_close(a, want, TOL_DW, "fp32 dilated depthwise %s vs the oracle's inflated filter" % (case,))
    assert np.array_equal(ra, rb), "fp32 %s: ext.dilation differs from the inflated filter by %g" % (case, np.abs(a - b).max())


@pytest.mark.parametrize("case", BF16_CASES)
def test_depthwise_dilated_bf16(pkg, orc, ctx, case):
    n, h, w, c, d = case
    a, b, want, ra, rb = _dw_both_routes(pkg, orc, ctx, n, h, w, c, d, bf=True)
    assert_close(a, orc.bf16_round(want), TOL_BF16, "bf16 dilated depthwise %s vs the oracle's inflated filter" % (case,))
    assert np.array_equal(ra, rb), "bf16 %s: ext.dilation differs from the inflated filter by %g" % (case, np.abs(a - b).max())


def test_depthwise_dilated_explicit_pads(pkg, orc, ctx):
    a, b, want, ra, rb = _dw_both_routes(pkg, orc, ctx, 2, 8, 9, 16, 2, pads=(0, 1))
    assert_close(a, want, TOL_DW, "pad_top 0, pad_left 1, D 2")
    assert np.array_equal(ra, rb)


def test_depthwise_dilated_stride_2_takes_the_generic_kernel(pkg, orc, ctx):
    a, b, want, ra, rb = _dw_both_routes(pkg, orc, ctx, 2, 10, 12, 8, 2, stride=2)
    assert want.shape == (2, 5, 6, 8)
    assert_close(a, want, TOL_DW, "stride 2, D 2 vs the oracle's inflated 5x5 at stride 2")
    assert np.array_equal(ra, rb)


def test_depthwise_dilation_1_is_dilation_0_and_negative_is_einval(pkg, orc, ctx):
    n, h, w, c = 2, 9, 9, 16
    x, f, sc, sh = _dw_inputs(orc, n, h, w, c, False, 5)
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    outs = []
    for dil in (0, 1):
        d_o = ctx.alloc(x.nbytes)
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, h, w, 3, 1, c, pkg.make_ext(batch=n, act=2, scale=d_sc.ptr, shift=d_sh.ptr, dilation=dil))
        ctx.sync()
        outs.append(d_o.download(x.shape, np.uint32))
    assert np.array_equal(outs[0], outs[1])
    want = orc.f32_depthwise(x, f, sc, sh, 1, orc.ACT_RELU6)
    assert_close(outs[0].view(np.float32), want, TOL_DW, "undilated")
    ext = pkg.make_ext(batch=n, act=2, scale=d_sc.ptr, shift=d_sh.ptr, dilation=-1)
    assert ctx.lib.mbn_depthwise(ctx.h, d_o.ptr, d_x.ptr, d_f.ptr, h, w, 3, 1, c, C.byref(ext)) == pkg.EINVAL


@pytest.mark.parametrize("mode", ["i8", "literal"])
def test_depthwise_dilation_unsupported_in_integer_modes(pkg, ctx, mode):
    n, h, w, c = 1, 8, 8, 8
    fill = np.full(n * h * w * c, 0xAB, np.uint8)
    d_o, d_x = ctx.to_device(fill), ctx.to_device(np.ones(n * h * w * c, np.uint8))
    d_f, d_m = ctx.to_device(np.ones(9 * c, np.int32)), ctx.to_device(np.ones(c, np.float32))
    if mode == "i8":
        ext = pkg.make_ext(batch=n, dtype=pkg.DT_I8, act=2, scale=d_m.ptr, shift=d_m.ptr, dilation=2)
    else:
        ext = pkg.make_ext(batch=n, dtype=pkg.DT_U8, dilation=2)
    assert ctx.lib.mbn_depthwise(ctx.h, d_o.ptr, d_x.ptr, d_f.ptr, h, w, 3, 1, c, C.byref(ext)) == pkg.EUNSUPPORTED
    ctx.sync()
    assert np.array_equal(d_o.download(fill.shape, np.uint8), fill), "nothing may have been launched"
    ext.dilation = 1                       # the same call undilated runs
    assert ctx.lib.mbn_depthwise(ctx.h, d_o.ptr, d_x.ptr, d_f.ptr, h, w, 3, 1, c, C.byref(ext)) == pkg.OK
    ctx.sync()


# ------------------------------------------------------------------------------------------------------------ networks

def _weights_os(pkg, tmp_path, alpha, rows, cols, classes, os_, seed=3):
    path = str(tmp_path / ("w_%g_%d.h5" % (alpha, classes)))
    if not os.path.exists(path):
        pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    return pkg.HostWeights(path, res=(rows, cols), lib=pkg.load(), output_stride=os_)


def _oracle_layer_os(orc, plan, blob, i, x, bf16=False):
    """_oracle_layer of test_rect_gpu.py, with the inflated filter for a dilated depthwise layer."""
    l = plan.layer[i]
    if l.kind != orc.L_DW or l.dilation <= 1:
        return _oracle_layer(orc, plan, blob, i, x, bf16)
    w = inflate(blob[l.w_offset:l.w_offset + l.w_count].reshape(3, 3, l.out_ch), l.dilation)
    y = orc.f32_depthwise(x, w, blob[l.scale_offset:l.scale_offset + l.out_ch], blob[l.shift_offset:l.shift_offset + l.out_ch], l.stride,
                          orc.ACT_RELU6, out_rows=l.out_rows, out_cols=l.out_cols, pad_top=l.pad_top, pad_left=l.pad_left)
    return orc.bf16_round(y) if bf16 else y


NET_CONFIGS = [(0.25, 64, 64, 16, 3), (0.25, 64, 64, 8, 3),          # os 8: D = 4 on an 8 x 8 map
               (1.0, 96, 128, 8, 2), (0.5, 96, 160, 16, 5)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("alpha,rows,cols,os_,n", NET_CONFIGS)
def test_net_os_per_layer_vs_oracle(pkg, orc, ctx, tmp_path, alpha, rows, cols, os_, n, dtype):
    classes, bf = 50, dtype == "bf16"
    hw = _weights_os(pkg, tmp_path, alpha, rows, cols, classes, os_)
    plan = hw.plan
    dilated = [i + 1 for i in range(plan.n_layers) if plan.layer[i].dilation > 1]
    assert dilated and (plan.layer[26].out_rows, plan.layer[26].out_cols) == (rows // os_, cols // os_)
    net = pkg.Net(ctx, plan, hw.blob.copy(), n)
    if bf:
        net.set_dtype(pkg.DT_BF16)
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
        want = _oracle_layer_os(orc, plan, hw.blob, i, prev, bf)
        assert_close(got, want, TOL_BF16_NET if bf else TOL_NET, "%s %gx%dx%d os %d layer %d" % (dtype, alpha, rows, cols, os_, i + 1))
        prev = got
    net.destroy()
    hw.free()


def _no_fused_launch_covers_a_dilated_layer(plan, launches):
    assert sum(c for _, c in launches) == plan.n_layers
    for first, count in launches:
        if count > 1:
            assert all(plan.layer[k - 1].dilation <= 1 for k in range(first, first + count)), (first, count)


def test_launch_grouping_f32_os8(pkg, ctx, tmp_path):
    n, classes = 6, 100
    hw = _weights_os(pkg, tmp_path, 1.0, 128, 128, classes, 8)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_fuse_blocks(0xFFFFFFFE)
    launches = net.launches(n)
    _no_fused_launch_covers_a_dilated_layer(hw.plan, launches)
    assert launches[0] == (1, 3) and (12, 2) in launches, launches       # the stem; layer 12 (now stride 1, undilated) still fuses
    for k in (14, 24, 26):
        assert (k, 1) in launches and (k + 1, 1) in launches, launches
    d_in, d_a, d_b = ctx.to_device(_images(n, 128, 128, 2)), ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    net.forward(d_in.ptr, d_a.ptr, n)
    net.set_fuse_stem(False)
    net.set_fuse_blocks(0)
    assert len(net.launches(n)) == 29
    net.forward(d_in.ptr, d_b.ptr, n)
    ctx.sync()
    a, b = d_a.download((n, classes), np.float32), d_b.download((n, classes), np.float32)
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
    assert np.array_equal(a, b)
    net.destroy()
    hw.free()


@pytest.mark.parametrize("os_", [16, 8])
def test_launch_grouping_bf16_resident_run_and_tail(pkg, ctx, tmp_path, os_):
    n, classes = 24, 100
    hw = _weights_os(pkg, tmp_path, 0.5, 160, 160, classes, os_)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_dtype(pkg.DT_BF16)
    net.set_fuse_blocks(0xFFFFFFFE)
    launches = net.launches(n)
    _no_fused_launch_covers_a_dilated_layer(hw.plan, launches)
    assert launches[0] == (1, 3) and (24, 5) not in launches, launches
    # os 16: layers 14-23 are the undilated 10 x 10 blocks they always were (still one resident run); os 8 dilates them
    assert ((14, 10) in launches) == (os_ == 16), launches
    d_in, d_a, d_b = ctx.to_device(_images(n, 160, 160, 8)), ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    net.forward(d_in.ptr, d_a.ptr, n)
    net.set_fuse_stem(False)
    net.set_fuse_blocks(0)
    assert len(net.launches(n)) == 29
    net.forward(d_in.ptr, d_b.ptr, n)
    ctx.sync()
    a, b = d_a.download((n, classes), np.float32), d_b.download((n, classes), np.float32)
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
    assert_close(a, b, TOL_BF16_NET, "bf16 os %d: grouped launches vs 29 single launches" % os_)
    net.destroy()
    hw.free()


def test_feature_output_layer_27_at_stride_16(pkg, ctx, tmp_path):
    n, rows, cols = 5, 96, 160
    hw = _weights_os(pkg, tmp_path, 0.5, rows, cols, 50, 16)
    l27 = hw.plan.layer[26]
    assert (l27.out_rows, l27.out_cols, l27.out_ch) == (rows // 16, cols // 16, 512)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    d_in, d_logits = ctx.to_device(_images(n, rows, cols, 4)), ctx.alloc(n * 50 * 4)
    shape = (n, l27.out_rows, l27.out_cols, l27.out_ch)
    d_feat = ctx.alloc(int(np.prod(shape)) * 4)
    net.keep_activations(True)
    net.forward(d_in.ptr, d_logits.ptr, n)
    ctx.sync()
    kept = net.layer_output(27, n)
    net.keep_activations(False)
    net.forward(d_in.ptr, d_feat.ptr, n, last_layer=27)
    ctx.sync()
    feat = d_feat.download(shape, np.float32)
    assert feat.std() > 0 and np.array_equal(feat, kept)
    net.destroy()
    hw.free()


def test_classify_and_int8_refusal_on_an_os16_net(pkg, ctx, tmp_path):
    n, classes, k, res = 6, 100, 5, 64
    hw = _weights_os(pkg, tmp_path, 1.0, res, res, classes, 16)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    d_in, d_a, d_b = ctx.to_device(_images(n, res, res, 12)), ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    d_idx, d_prob = ctx.alloc(n * k * 4), ctx.alloc(n * k * 4)
    net.forward(d_in.ptr, d_a.ptr, n)
    net.classify(d_in.ptr, n, k, d_idx.ptr, d_prob.ptr)
    ctx.sync()
    a = d_a.download((n, classes), np.float32)
    idx, prob = d_idx.download((n, k), np.int32), d_prob.download((n, k), np.float32)
    e = np.exp(a.astype(np.float64) - a.max(axis=1, keepdims=True))
    sm = e / e.sum(axis=1, keepdims=True)
    order = np.argsort(-a, axis=1, kind="stable")[:, :k]
    assert np.array_equal(idx, order)
    assert np.abs(prob - np.take_along_axis(sm, order, axis=1)).max() < 1e-5
    with pytest.raises(pkg.MbnError) as err:
        net.set_dtype(pkg.DT_I8)
    assert err.value.code == pkg.EUNSUPPORTED
    net.forward(d_in.ptr, d_b.ptr, n)                  # still an fp32 net
    ctx.sync()
    assert np.array_equal(a, d_b.download((n, classes), np.float32))
    net.destroy()
    hw.free()


def test_c_host_output_stride(pkg, ctx):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    r = subprocess.run([exe, "--synthetic", "3", "--alpha", "0.25", "--res", "96", "--batch", "3", "--output-stride", "16"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"present at location (\d+) and it's value is ([0-9]+\.[0-9]+)", r.stdout), r.stdout
    bad = subprocess.run([exe, "--synthetic", "3", "--alpha", "0.25", "--res", "96", "--output-stride", "4"], capture_output=True, text=True,
                         timeout=300)
    assert bad.returncode != 0
