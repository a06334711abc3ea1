"""The dense head on the GPU. mbn_upsample_argmax_f32 alone: labels and score bits equal to tests/dense_ref.py (the normative arithmetic)
on the smallest shapes that reach each way of going wrong, adversarial values, torch, argument errors. The net runner: forward_dense bit
for bit against forward(last_layer = 27) + Context.pointwise, against the oracle in fp32, segment against dense_ref on forward_dense's
output, the 1 x 1 map, scratch reuse. The C host's --segment."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_ref
from test_dense_cpu import logits_for, torch_compare
from test_dilation_gpu import _oracle_layer_os, _weights_os
from test_rect_gpu import TOL_NET, _images, assert_close

pytestmark = pytest.mark.gpu


def _device(pkg, ctx, x, S, offset=0, with_score=True):
    """mbn_upsample_argmax_f32 on x [n][h][w][classes] (uploaded `offset` bytes into its allocation): (labels, score bits or None)"""
    n, h, w, classes = x.shape
    raw = np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()])
    d_x = ctx.to_device(raw)
    npix = n * h * S * w * S
    d_lab = ctx.to_device(np.full(npix, -7, np.int32))
    d_sc = ctx.to_device(np.full(npix, 123.0, np.float32)) if with_score else None
    ctx.upsample_argmax(d_lab.ptr, d_sc.ptr if with_score else None, d_x.ptr + offset, n, h, w, classes, S)
    ctx.sync()
    lab = d_lab.download((n, h * S, w * S), np.int32)
    sc = d_sc.download((n, h * S, w * S), np.uint32) if with_score else None
    for b in (d_x, d_lab, d_sc):
        if b is not None:
            b.free()
    return lab, sc


def _check(pkg, ctx, x, S, what, **kw):
    want_lab, want_sc = dense_ref.upsample_argmax(x, S)
    lab, sc = _device(pkg, ctx, x, S, **kw)
    bad = int((lab != want_lab).sum())
    assert bad == 0, "%s: %d of %d labels differ from dense_ref" % (what, bad, lab.size)
    if sc is not None:
        bad = int((sc != want_sc.view(np.uint32)).sum())
        assert bad == 0, "%s: %d of %d score bit patterns differ from dense_ref" % (what, bad, sc.size)
    return want_lab, want_sc


MAPS = [(1, 1), (1, 3), (3, 1), (2, 2), (5, 7)]       # 1 x 1: every weight clamped; 5 x 7 at S = 8: 2 x 2 workgroups, part-empty tiles
FACTORS = [8, 16, 32]


@pytest.mark.parametrize("n,classes", [(1, 21), (3, 64)])       # 21: dword loads, a padded last group; 64: 16-byte loads
@pytest.mark.parametrize("S", FACTORS)
@pytest.mark.parametrize("hw", MAPS)
def test_kernel_maps(pkg, ctx, hw, S, n, classes):
    x = logits_for((n, hw[0], hw[1], classes, S), seed=hw[0] * 100 + hw[1] * 10 + S)
    _check(pkg, ctx, x, S, "map %s S %d n %d classes %d" % (hw, S, n, classes))


@pytest.mark.parametrize("S", FACTORS)
@pytest.mark.parametrize("classes", [1, 2, 21, 64, 65, 1001])  # one class; chunk of 128: under, a full 16-byte chunk, an odd count, 7 chunks + 105
def test_kernel_class_counts(pkg, ctx, classes, S):
    n, h, w = 2, 2, 2
    x = logits_for((n, h, w, classes, S), seed=classes + S)
    x[0, 0, 0, classes - 1] += 100.0                   # a winner in the last class ...
    if classes > 128:
        x[1, h - 1, w - 1, 128] += 100.0               # ... and in the first class of a later chunk
    lab, _ = _check(pkg, ctx, x, S, "classes %d S %d" % (classes, S))
    assert lab[0, 0, 0] == classes - 1 and (classes <= 128 or lab[1, -1, -1] == 128)


def test_kernel_1000_classes(pkg, ctx):
    _check(pkg, ctx, logits_for((1, 2, 3, 1000, 8), seed=5), 8, "1000 classes")          # 16-byte loads over eight chunks, the last one short


@pytest.mark.parametrize("classes", [21, 64])
def test_kernel_logits_at_a_4_byte_offset(pkg, ctx, classes):
    _check(pkg, ctx, logits_for((3, 2, 3, classes, 16), seed=9), 16, "offset 4, classes %d" % classes, offset=4)


def test_kernel_score_null(pkg, ctx):
    _check(pkg, ctx, logits_for((2, 3, 2, 21, 8), seed=11), 8, "score NULL", with_score=False)


def test_kernel_adversarial_values(pkg, ctx):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.zeros((2, 2, 3, 200), np.float32)           # two equal maxima, in two chunks: the lowest index wins
    x[..., 5] = x[..., 131] = 2.0
    lab, sc = _check(pkg, ctx, x, 8, "equal maxima")
    assert (lab == 5).all() and (sc == 2.0).all()
    lab, sc = _check(pkg, ctx, np.full((1, 3, 3, 21), 1.5, np.float32), 16, "constant map")
    assert (lab == 0).all() and (sc == 1.5).all()
    x = logits_for((1, 3, 3, 65, 8), seed=13)          # a NaN where the winner was: the runner-up's pixel values decide
    x[0, 1, 1, int(x[0, 1, 1].argmax())] = nan
    x[0, 0, 2, 64] = nan
    _check(pkg, ctx, x, 8, "NaN in the winning position")
    lab, sc = _check(pkg, ctx, np.full((1, 2, 2, 21), nan, np.float32), 32, "all NaN")
    assert (lab == 0).all() and (sc == -inf).all()
    x = logits_for((2, 3, 3, 21, 16), seed=17)         # an all -inf pixel: -inf and NaN interpolants around it, label 0 / score -inf at its centre
    x[1, 1, 1, :] = -inf
    lab, sc = _check(pkg, ctx, x, 16, "all -inf pixel")
    assert lab[1, 24, 24] == 0 and sc[1, 24, 24] == -inf
    x = np.random.default_rng(19).integers(-8, 9, (2, 5, 7, 65)).astype(np.float32)      # integers: every interpolant is exact
    _check(pkg, ctx, x, 32, "integer-valued logits")


def test_kernel_vs_torch(pkg, ctx):
    x = logits_for((2, 5, 7, 21, 8))
    lab, sc = _device(pkg, ctx, x, 8)
    torch_compare(x, 8, lab, sc.view(np.float32), "device")


def test_kernel_argument_errors(pkg, ctx):
    x = ctx.to_device(np.zeros(2 * 2 * 21, np.float32))
    fill = np.full(16 * 16, -7, np.int32)
    lab, sc = ctx.to_device(fill), ctx.to_device(fill.astype(np.float32))
    call = lambda *a: ctx.lib.mbn_upsample_argmax_f32(ctx.h, *a, None)
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 4) == pkg.EUNSUPPORTED
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 64) == pkg.EUNSUPPORTED
    assert call(None, sc.ptr, x.ptr, 1, 2, 2, 21, 8) == pkg.EINVAL
    assert call(lab.ptr, sc.ptr, None, 1, 2, 2, 21, 8) == pkg.EINVAL
    for bad in [(0, 2, 2, 21), (1, 0, 2, 21), (1, 2, 0, 21), (1, 2, 2, 0), (-1, 2, 2, 21)]:
        assert call(lab.ptr, sc.ptr, x.ptr, *bad, 8) == pkg.EINVAL, bad
    assert call(lab.ptr, sc.ptr, x.ptr + 2, 1, 2, 2, 20, 8) == pkg.EINVAL                  # off 4 bytes
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 16) == pkg.EINVAL                     # 32 x 32 labels into a 16 x 16 buffer: the span check
    ctx.sync()
    assert np.array_equal(lab.download(fill.shape, np.int32), fill), "nothing may have been launched"
    assert call(lab.ptr, None, x.ptr, 1, 2, 2, 21, 8) == pkg.OK
    ctx.sync()
    assert (lab.download(fill.shape, np.int32) == 0).all()
    for b in (x, lab, sc):
        b.free()


# ------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS, BATCH = 0.5, 30, 64, 96, 3
_oracle_dense = {}


def _oracle(orc, hw, imgs, os_):
    """the oracle's layer-27 output times the FC, [n][h][w][classes]; once per output stride"""
    if os_ not in _oracle_dense:
        plan, prev = hw.plan, imgs
        for i in range(plan.n_layers - 2):
            prev = _oracle_layer_os(orc, plan, hw.blob, i, prev)
        fc = plan.layer[plan.n_layers - 1]
        wm = hw.blob[fc.w_offset:fc.w_offset + fc.w_count].reshape(fc.out_ch, fc.in_ch)
        sh = hw.blob[fc.shift_offset:fc.shift_offset + fc.out_ch]
        n, h, w, _ = prev.shape
        _oracle_dense[os_] = orc.f32_pointwise(prev, wm, None, sh, orc.ACT_NONE).reshape(n, h, w, fc.out_ch).copy()
    return _oracle_dense[os_]


def _fc_operands(pkg, ctx, net, hw, dtype):
    """device (filter, scale, shift, io_flags, buffers to free) of the FC as the runner passes them in the net's current mode"""
    plan = hw.plan
    fc = plan.layer[plan.n_layers - 1]
    blob = net._dev_blob.ptr
    at = lambda off: None if off < 0 else blob + 4 * off
    if dtype == "f32":
        return at(fc.w_offset), at(fc.scale_offset), at(fc.shift_offset), 0, []
    if dtype == "bf16":
        d_w = ctx.to_device(pkg.f32_to_bf16_bits(hw.blob[fc.w_offset:fc.w_offset + fc.w_count]))
        return d_w.ptr, at(fc.scale_offset), at(fc.shift_offset), pkg.IO_OUT_F32, [d_w]
    p, i8blob = pkg.quantize_i8(plan, hw.blob, net.get_act_scales_i8())
    d_q = ctx.to_device(i8blob)
    q = p.layer[plan.n_layers - 1]
    return d_q.ptr + q.w_offset, d_q.ptr + q.mult_offset, d_q.ptr + q.bias_offset, pkg.IO_OUT_F32, [d_q]


@pytest.mark.parametrize("dtype,os_", [("f32", 8), ("f32", 16), ("f32", 32), ("bf16", 8), ("bf16", 16), ("bf16", 32), ("i8", 32)])
def test_net_dense_and_segment(pkg, orc, ctx, tmp_path, dtype, os_):
    n = BATCH
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, os_)
    plan = hw.plan
    l27, fc = plan.layer[plan.n_layers - 3], plan.layer[plan.n_layers - 1]
    h, w = l27.out_rows, l27.out_cols
    assert (h, w) == (ROWS // os_, COLS // os_) and l27.index == 27 and fc.out_ch == CLASSES
    net = pkg.Net(ctx, plan, hw.blob.copy(), n)
    dt = {"f32": pkg.DT_F32, "bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype]
    if dt != pkg.DT_F32:
        net.set_dtype(dt)
    es = {"f32": 4, "bf16": 2, "i8": 1}[dtype]
    imgs = _images(n, ROWS, COLS, 21)
    d_in = ctx.to_device(imgs)
    count = n * h * w * CLASSES
    d_feat, d_comp, d_dense = ctx.alloc(n * h * w * l27.out_ch * es), ctx.alloc(count * 4), ctx.alloc(count * 4)
    # forward_dense == forward(last_layer = 27) followed by the FC as a pointwise call over the map, bit for bit
    net.forward(d_in.ptr, d_feat.ptr, n, last_layer=27)
    filt, scale, shift, io, bufs = _fc_operands(pkg, ctx, net, hw, dtype)
    ctx.pointwise(d_comp.ptr, d_feat.ptr, filt, h, w, fc.in_ch, fc.out_ch,
                  pkg.make_ext(batch=n, dtype=dt, act=pkg.ACT_NONE, scale=scale, shift=shift, io_flags=io))
    net.forward_dense(d_in.ptr, d_dense.ptr, n)
    ctx.sync()
    comp, dense = d_comp.download((n, h, w, CLASSES), np.uint32), d_dense.download((n, h, w, CLASSES), np.uint32)
    assert np.array_equal(dense, comp), "%s os %d: forward_dense differs from forward(27) + pointwise" % (dtype, os_)
    dense = dense.view(np.float32)
    assert np.isfinite(dense).all() and dense.std() > 0
    if dtype == "f32":
        assert_close(dense, _oracle(orc, hw, imgs, os_), TOL_NET, "fp32 os %d dense logits vs the oracle's layer 27 x FC" % os_)
    # segment == dense_ref on forward_dense's output, exactly; a second call reuses the scratch and gives the same bytes
    npix = n * ROWS * COLS
    want_lab, want_sc = dense_ref.upsample_argmax(dense, os_)
    d_lab, d_sc, d_lab2 = ctx.alloc(npix * 4), ctx.alloc(npix * 4), ctx.to_device(np.full(npix, -7, np.int32))
    net.segment(d_in.ptr, n, d_lab.ptr, d_sc.ptr)
    ctx.sync()
    lab, sc = d_lab.download((n, ROWS, COLS), np.int32), d_sc.download((n, ROWS, COLS), np.uint32)
    assert np.array_equal(lab, want_lab), "%s os %d: %d labels differ" % (dtype, os_, int((lab != want_lab).sum()))
    assert np.array_equal(sc, want_sc.view(np.uint32))
    assert len(np.unique(lab)) > 1
    net.segment(d_in.ptr, n, d_lab2.ptr, None)
    ctx.sync()
    assert np.array_equal(d_lab2.download((n, ROWS, COLS), np.int32), lab)
    net.destroy()
    for b in [d_in, d_feat, d_comp, d_dense, d_lab, d_sc, d_lab2] + bufs:
        b.free()
    hw.free()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "i8"])
def test_net_1x1_map_is_the_classifier(pkg, ctx, tmp_path, dtype):
    """A 32 x 32 input at output stride 32: the map is 1 x 1, the pool of one pixel divides by 1, so the dense logits are forward's
    logits bit for bit and the label map is constant argmax(logits)."""
    hw = _weights_os(pkg, tmp_path, ALPHA, 32, 32, CLASSES, 32)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 1)
    if dtype != "f32":
        net.set_dtype({"bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype])
    net.set_fuse_resident(False)           # bf16: the resident tail (layers 24-28 in one launch) exists in the full forward only and sums in another order
    d_in = ctx.to_device(_images(1, 32, 32, 23))
    d_a, d_b, d_lab, d_sc = ctx.alloc(CLASSES * 4), ctx.alloc(CLASSES * 4), ctx.alloc(32 * 32 * 4), ctx.alloc(32 * 32 * 4)
    net.forward(d_in.ptr, d_a.ptr, 1)
    net.forward_dense(d_in.ptr, d_b.ptr, 1)
    net.segment(d_in.ptr, 1, d_lab.ptr, d_sc.ptr)
    ctx.sync()
    a, b = d_a.download((CLASSES,), np.uint32), d_b.download((CLASSES,), np.uint32)
    assert np.array_equal(a, b) and a.view(np.float32).std() > 0
    lab, sc = d_lab.download((32, 32), np.int32), d_sc.download((32, 32), np.float32)
    want_lab, want_sc = dense_ref.upsample_argmax(a.view(np.float32).reshape(1, 1, 1, CLASSES), 32)
    assert (lab == int(a.view(np.float32).argmax())).all()
    assert np.array_equal(lab, want_lab[0]) and np.array_equal(sc.view(np.uint32), want_sc[0].view(np.uint32))
    net.destroy()
    for buf in (d_in, d_a, d_b, d_lab, d_sc):
        buf.free()
    hw.free()


def test_net_segment_refusals(pkg, ctx, tmp_path):
    hw = _weights_os(pkg, tmp_path, ALPHA, 32, 32, CLASSES, 32)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 2)
    d_in, d_lab = ctx.to_device(_images(2, 32, 32, 1)), ctx.alloc(2 * 32 * 32 * 4)
    lib = ctx.lib
    assert lib.mbn_net_segment(net.h, d_in.ptr, 3, d_lab.ptr, None) == pkg.EINVAL          # beyond max_batch
    assert lib.mbn_net_segment(net.h, d_in.ptr, 0, d_lab.ptr, None) == pkg.EINVAL
    assert lib.mbn_net_segment(net.h, None, 2, d_lab.ptr, None) == pkg.EINVAL
    assert lib.mbn_net_segment(net.h, d_in.ptr, 2, None, None) == pkg.EINVAL
    assert lib.mbn_net_forward_dense(net.h, d_in.ptr, None, 2) == pkg.EINVAL
    assert lib.mbn_net_segment(net.h, d_in.ptr, 2, d_lab.ptr, None) == pkg.OK              # the net is still usable
    ctx.sync()
    net.destroy()
    d_in.free()
    d_lab.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def test_c_host_segment(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    out = str(tmp_path / "out.pgm")
    r = subprocess.run([exe, "--synthetic", "3", "--alpha", "0.25", "--res", "96", "--batch", "2", "--output-stride", "16", "--segment", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(out, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    assert m, raw[:32]
    width, height, maxval = (int(g) for g in m.groups())
    classes = 1000                                      # the host's synthetic weights
    assert (width, height, maxval) == (96, 96, classes - 1)
    body = raw[m.end():]
    assert len(body) == 96 * 96 * 2                     # maxval > 255: two bytes per pixel, big-endian
    lab = np.frombuffer(body, ">u2").astype(np.int64)
    assert lab.max() < classes
    line = re.search(r"^segment: 96x96 label map -> .*; most frequent labels:((?: \d+ \(\d+\))+)$", r.stdout, re.M)
    assert line, r.stdout
    printed = [(int(a), int(b)) for a, b in re.findall(r"(\d+) \((\d+)\)", line.group(1))]
    counts = np.bincount(lab, minlength=classes)
    order = sorted(np.nonzero(counts)[0], key=lambda c: (-counts[c], c))[:5]
    assert printed == [(int(c), int(counts[c])) for c in order]
    assert sum(b for _, b in printed) <= 96 * 96
    # without the option the program prints what it always did
    r0 = subprocess.run([exe, "--synthetic", "3", "--alpha", "0.25", "--res", "96", "--batch", "2", "--output-stride", "16"],
                        capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and "segment" not in r0.stdout
    keep = lambda s: [l for l in s.splitlines() if not l.startswith("Kernel Execution time") and not l.startswith("segment:")]
    assert keep(r0.stdout) == keep(r.stdout)
