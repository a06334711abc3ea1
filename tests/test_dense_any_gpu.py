"""The dense head at any output size on the GPU. mbn_resample_argmax_f32 alone: labels and score bits equal to tests/dense_any_ref.py (the
normative arithmetic) on the smallest shapes that reach each way of going wrong, bit-equal to mbn_upsample_argmax_f32 at integer factors,
adversarial values, argument errors, nothing written outside the maps. The ragged form: every image bit-equal to the uniform call on it alone,
gaps untouched, a refused set leaves the previous one valid. The net runner: segment_to and segment_images against the reference applied to
forward_dense's own logits. The C host's --segment-source."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_any_ref
from test_dense_cpu import logits_for
from test_dilation_gpu import _weights_os
from test_rect_gpu import _images

pytestmark = pytest.mark.gpu

TAIL = 64            # sentinel elements behind the last image of every output buffer
LAB_FILL, SC_FILL = -7, 123.0


def _logits(n, h, w, classes, seed):
    return logits_for((n, h, w, classes, 0), seed=seed)


def _device(ctx, x, H, W, offset=0, with_score=True):
    """mbn_resample_argmax_f32 on x [n][h][w][classes] (uploaded `offset` bytes into its allocation): (labels, score bits or None). The
    output buffers carry a sentinel pattern and TAIL more elements, which must come back unchanged."""
    n, h, w, classes = x.shape
    d_x = ctx.to_device(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
    npix = n * H * W
    d_lab = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32))
    d_sc = ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32)) if with_score else None
    ctx.resample_argmax(d_lab.ptr, d_sc.ptr if with_score else None, d_x.ptr + offset, n, h, w, classes, H, W)
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


def _check(ctx, x, H, W, what, **kw):
    want_lab, want_sc = dense_any_ref.resample_argmax(x, H, W)
    lab, sc = _device(ctx, x, H, W, **kw)
    bad = int((lab != want_lab).sum())
    assert bad == 0, "%s: %d of %d labels differ from dense_any_ref" % (what, bad, lab.size)
    if sc is not None:
        bad = int((sc != want_sc.view(np.uint32)).sum())
        assert bad == 0, "%s: %d of %d score bit patterns differ from dense_any_ref" % (what, bad, sc.size)
    return want_lab, want_sc


# (h, w, H, W)
GEOMETRY = [(1, 1, 9, 4),        # smaller than a tile, one vector
            (1, 1, 70, 45),      # several tiles over one vector
            (5, 7, 37, 61),      # non-integer, unequal ratios; H no multiple of 4 or 32
            (5, 7, 20, 28),      # the minimum ratio exactly
            (3, 5, 100, 23),     # ratio 33 on one axis, 4.6 on the other
            (9, 4, 65, 33),      # one row and one column past a tile edge
            (7, 7, 30, 28)]      # ratios just above 4: 49 staged vectors, the 64-class chunk


@pytest.mark.parametrize("n,classes", [(1, 21), (3, 64)])       # 21: dword loads, a padded last group; 64: 16-byte loads
@pytest.mark.parametrize("geo", GEOMETRY)
def test_kernel_geometry(pkg, ctx, geo, n, classes):
    h, w, H, W = geo
    _check(ctx, _logits(n, h, w, classes, seed=h * 1000 + w * 100 + H + W), H, W, "%s n %d classes %d" % (geo, n, classes))


@pytest.mark.parametrize("S", [8, 16, 32])
@pytest.mark.parametrize("hw", [(2, 3), (5, 7)])
def test_kernel_integer_factors_equal_the_factor_kernel(pkg, ctx, hw, S):
    h, w = hw
    n, classes = 2, 21
    x = _logits(n, h, w, classes, seed=h + w + S)
    want_lab, want_sc = _check(ctx, x, h * S, w * S, "%s x %d" % (hw, S))
    d_x = ctx.to_device(x)                              # both kernels on the same device buffer
    npix = n * h * S * w * S
    outs = [ctx.to_device(np.full(npix, LAB_FILL, np.int32)) for _ in range(2)] + [ctx.to_device(np.full(npix, SC_FILL, np.float32)) for _ in range(2)]
    ctx.upsample_argmax(outs[0].ptr, outs[2].ptr, d_x.ptr, n, h, w, classes, S)
    ctx.resample_argmax(outs[1].ptr, outs[3].ptr, d_x.ptr, n, h, w, classes, h * S, w * S)
    ctx.sync()
    got = [b.download((npix,), np.uint32) for b in outs]
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[2], got[3])
    assert np.array_equal(got[1].view(np.int32).reshape(want_lab.shape), want_lab)
    for b in [d_x] + outs:
        b.free()


@pytest.mark.parametrize("classes", [1, 2, 21, 64, 65, 1001])  # one class; chunk of 128: under, a full 16-byte chunk, an odd count, 7 chunks + 105
def test_kernel_class_counts(pkg, ctx, classes):
    n, h, w, H, W = 2, 2, 2, 11, 9
    x = _logits(n, h, w, classes, seed=classes)
    x[0, 0, 0, classes - 1] += 100.0                   # a winner in the last class ...
    if classes > 128:
        x[1, h - 1, w - 1, 128] += 100.0               # ... and in the first class of a later chunk
    lab, _ = _check(ctx, x, H, W, "classes %d" % classes)
    assert lab[0, 0, 0] == classes - 1 and (classes <= 128 or lab[1, -1, -1] == 128)


@pytest.mark.parametrize("classes", [64, 65, 130])             # the 64-class chunk (more than 38 staged vectors): one full, one + 1, two + 2
def test_kernel_class_counts_short_chunk(pkg, ctx, classes):
    assert pkg.resample_plan(7, 7, 30, 28).ch == 64
    x = _logits(1, 7, 7, classes, seed=classes + 1)
    x[0, 0, 0, classes - 1] += 100.0
    if classes > 64:
        x[0, 6, 6, 64] += 100.0
    lab, _ = _check(ctx, x, 30, 28, "short chunk, classes %d" % classes)
    assert lab[0, 0, 0] == classes - 1 and (classes <= 64 or lab[0, -1, -1] == 64)


@pytest.mark.parametrize("classes", [21, 64])
def test_kernel_logits_at_a_4_byte_offset(pkg, ctx, classes):
    _check(ctx, _logits(3, 2, 3, classes, seed=9), 11, 17, "offset 4, classes %d" % classes, offset=4)


def test_kernel_score_null(pkg, ctx):
    _check(ctx, _logits(2, 3, 2, 21, seed=11), 13, 9, "score NULL", with_score=False)


def test_kernel_adversarial_values(pkg, ctx):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.zeros((2, 2, 3, 200), np.float32)           # equal maxima in different chunks (of 128 and of 64): the lowest index wins
    x[..., 5] = x[..., 70] = x[..., 131] = 2.0
    lab, sc = _check(ctx, x, 11, 17, "equal maxima")
    assert (lab == 5).all()
    x = np.zeros((1, 7, 7, 200), np.float32)
    x[..., 5] = x[..., 70] = x[..., 131] = 2.0
    lab, sc = _check(ctx, x, 30, 28, "equal maxima, short chunk")
    assert (lab == 5).all()
    lab, sc = _check(ctx, np.full((1, 3, 3, 21), 1.5, np.float32), 13, 14, "constant map")
    assert (lab == 0).all()
    x = _logits(1, 3, 3, 65, seed=13)                  # a NaN where the winner was: the runner-up's pixel values decide
    x[0, 1, 1, int(x[0, 1, 1].argmax())] = nan
    x[0, 0, 2, 64] = nan
    _check(ctx, x, 13, 17, "NaN in the winning position")
    lab, sc = _check(ctx, np.full((1, 2, 2, 21), nan, np.float32), 9, 11, "all NaN")
    assert (lab == 0).all() and (sc == -inf).all()
    x = _logits(2, 3, 3, 21, seed=17)                  # an all -inf pixel: -inf and NaN interpolants around it; at 3 -> 13 output 6 is its centre
    x[1, 1, 1, :] = -inf
    lab, sc = _check(ctx, x, 13, 13, "all -inf pixel")
    assert lab[1, 6, 6] == 0 and sc[1, 6, 6] == -inf
    x = np.random.default_rng(19).integers(-8, 9, (2, 5, 7, 65)).astype(np.float32)      # integer-valued logits: against the reference only
    _check(ctx, x, 37, 61, "integer-valued logits")


def test_kernel_argument_errors(pkg, ctx):
    x = ctx.to_device(np.zeros(2 * 2 * 21, np.float32))
    fill = np.full(16 * 16, LAB_FILL, np.int32)
    lab, sc = ctx.to_device(fill), ctx.to_device(fill.astype(np.float32))
    call = lambda *a: ctx.lib.mbn_resample_argmax_f32(ctx.h, *a, None)
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 7, 16) == pkg.EUNSUPPORTED          # under 4 x the map
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 16, 7) == pkg.EUNSUPPORTED
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 16385, 16) == pkg.EUNSUPPORTED
    assert call(None, sc.ptr, x.ptr, 1, 2, 2, 21, 16, 16) == pkg.EINVAL
    assert call(lab.ptr, sc.ptr, None, 1, 2, 2, 21, 16, 16) == pkg.EINVAL
    for bad in [(0, 2, 2, 21, 16, 16), (1, 0, 2, 21, 16, 16), (1, 2, 0, 21, 16, 16), (1, 2, 2, 0, 16, 16), (1, 2, 2, 21, 0, 16), (1, 2, 2, 21, 16, -1)]:
        assert call(lab.ptr, sc.ptr, x.ptr, *bad) == pkg.EINVAL, bad
    assert call(lab.ptr, sc.ptr, x.ptr + 2, 1, 2, 2, 20, 16, 16) == pkg.EINVAL           # off 4 bytes
    assert call(lab.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, 16, 17) == pkg.EINVAL               # 16 x 17 labels into a 16 x 16 buffer: the span check
    ctx.sync()
    assert np.array_equal(lab.download(fill.shape, np.int32), fill), "nothing may have been launched"
    assert call(lab.ptr, None, x.ptr, 1, 2, 2, 21, 16, 16) == pkg.OK
    ctx.sync()
    assert (lab.download(fill.shape, np.int32) == 0).all()
    for b in (x, lab, sc):
        b.free()


# ------------------------------------------------------------------------------------------------------------------------- ragged

RAGGED_SIZES = [(37, 61), (40, 56), (20, 28), (100, 30), (37, 61)]       # 40 x 56: the integer factor 8; 20 x 28: the minimum ratio


def _ragged_layout(sizes, order, gap=5, first=3):
    """element offsets of the items when they lie in `order` with `gap` sentinel elements between them; (offsets, total elements)"""
    offs, at = [0] * len(sizes), first
    for i in order:
        offs[i] = at
        at += sizes[i][0] * sizes[i][1] + gap
    return offs, at + TAIL


def _ragged_run(ctx, rd, x, sizes, offs, total):
    d_x = ctx.to_device(x)
    d_lab, d_sc = ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, SC_FILL, np.float32))
    rd.run(d_lab.ptr, d_sc.ptr, d_x.ptr)
    ctx.sync()
    lab, sc = d_lab.download((total,), np.int32), d_sc.download((total,), np.float32)
    for b in (d_x, d_lab, d_sc):
        b.free()
    return lab, sc


def _ragged_compare(ctx, x, sizes, offs, lab, sc):
    touched = np.zeros(lab.size, bool)
    for i, ((H, W), off) in enumerate(zip(sizes, offs)):
        one_lab, one_sc = _check(ctx, x[i:i + 1], H, W, "ragged item %d alone" % i)      # the uniform call on that image alone, itself == the reference
        assert np.array_equal(lab[off:off + H * W].reshape(H, W), one_lab[0]), "item %d labels" % i
        assert np.array_equal(sc[off:off + H * W].view(np.uint32).reshape(H, W), one_sc[0].view(np.uint32)), "item %d scores" % i
        touched[off:off + H * W] = True
    assert (lab[~touched] == LAB_FILL).all() and (sc[~touched] == SC_FILL).all(), "written between or behind the maps"


def test_ragged(pkg, ctx):
    h, w, classes = 5, 7, 21
    x = _logits(5, h, w, classes, seed=77)
    rd = pkg.RaggedReadout(ctx, 5)
    offs, total = _ragged_layout(RAGGED_SIZES, order=(3, 0, 4, 2, 1))
    items = [(o, H, W) for o, (H, W) in zip(offs, RAGGED_SIZES)]
    rd.set(h, w, classes, items)
    lab, sc = _ragged_run(ctx, rd, x, RAGGED_SIZES, offs, total)
    _ragged_compare(ctx, x, RAGGED_SIZES, offs, lab, sc)
    # refused sets: overlapping maps, an item under ratio 4; the descriptors of the set before stay valid
    lib = ctx.lib
    overlap = pkg.label_items([(0, 37, 61), (37 * 61 - 1, 20, 28)])
    assert lib.mbn_ragged_readout_set(rd.h, h, w, classes, overlap, 2, None) == pkg.EINVAL
    small = pkg.label_items([(0, 37, 61), (5000, 19, 28)])
    assert lib.mbn_ragged_readout_set(rd.h, h, w, classes, small, 2, None) == pkg.EUNSUPPORTED
    assert lib.mbn_ragged_readout_set(rd.h, h, w, classes, pkg.label_items(items + [(90000, 20, 28)]), 6, None) == pkg.EINVAL      # beyond max_batch
    lab2, sc2 = _ragged_run(ctx, rd, x, RAGGED_SIZES, offs, total)
    assert np.array_equal(lab2, lab) and np.array_equal(sc2.view(np.uint32), sc.view(np.uint32))
    # a second set with a smaller batch on the same handle, other sizes in another order
    sizes = [(20, 28), (37, 61)]
    offs, total = _ragged_layout(sizes, order=(1, 0), gap=9, first=0)
    rd.set(h, w, classes, [(o, H, W) for o, (H, W) in zip(offs, sizes)])
    lab, sc = _ragged_run(ctx, rd, x[:2], sizes, offs, total)
    _ragged_compare(ctx, x[:2], sizes, offs, lab, sc)
    # argument errors of the launch
    d = ctx.to_device(np.zeros(8, np.float32))
    assert lib.mbn_resample_argmax_ragged_f32(rd.h, None, None, d.ptr, None) == pkg.EINVAL
    assert lib.mbn_resample_argmax_ragged_f32(rd.h, d.ptr, None, d.ptr, None) == pkg.EINVAL      # an 8-element tracked buffer: the span check
    fresh = pkg.RaggedReadout(ctx, 2)
    assert lib.mbn_resample_argmax_ragged_f32(fresh.h, d.ptr, None, d.ptr, None) == pkg.EINVAL   # no set yet
    ctx.sync()
    d.free()
    fresh.close()
    rd.close()


# ------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS, BATCH = 0.5, 21, 64, 96, 3
SOURCES = [(75, 130), (64, 96), (120, 100)]


@pytest.mark.parametrize("dtype,os_", [("f32", 8), ("f32", 16), ("bf16", 8), ("bf16", 16), ("i8", 32)])
def test_net_segment_to_and_images(pkg, ctx, tmp_path, dtype, os_):
    n = BATCH
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, os_)
    plan = hw.plan
    h, w = ROWS // os_, COLS // os_
    net = pkg.Net(ctx, plan, hw.blob.copy(), n)
    dt = {"f32": pkg.DT_F32, "bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype]
    if dt != pkg.DT_F32:
        net.set_dtype(dt)
    lib = ctx.lib
    # ---- segment_to: the reference applied to the download of forward_dense's own logits
    H, W = 75, 130
    d_in = ctx.to_device(_images(n, ROWS, COLS, 21))
    d_dense = ctx.alloc(n * h * w * CLASSES * 4)
    npix = n * H * W
    d_lab, d_sc = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32)), ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32))
    net.forward_dense(d_in.ptr, d_dense.ptr, n)
    # refusals first: an output under 4 x the map, then the call that works on the same net
    assert lib.mbn_net_segment_to(net.h, d_in.ptr, n, 4 * h - 1, W, d_lab.ptr, d_sc.ptr) == pkg.EUNSUPPORTED
    assert lib.mbn_net_segment_to(net.h, d_in.ptr, n, H, 4 * w - 1, d_lab.ptr, d_sc.ptr) == pkg.EUNSUPPORTED
    assert lib.mbn_net_segment_to(net.h, d_in.ptr, n + 1, H, W, d_lab.ptr, d_sc.ptr) == pkg.EINVAL
    net.segment_to(d_in.ptr, n, H, W, d_lab.ptr, d_sc.ptr)
    ctx.sync()
    dense = d_dense.download((n, h, w, CLASSES), np.float32)
    assert np.isfinite(dense).all() and dense.std() > 0
    want_lab, want_sc = dense_any_ref.resample_argmax(dense, H, W)
    lab, sc = d_lab.download((npix + TAIL,), np.int32), d_sc.download((npix + TAIL,), np.float32)
    assert np.array_equal(lab[:npix].reshape(n, H, W), want_lab), "%s os %d: %d labels differ" % (dtype, os_, int((lab[:npix] != want_lab.ravel()).sum()))
    assert np.array_equal(sc[:npix].view(np.uint32), want_sc.view(np.uint32).ravel())
    assert (lab[npix:] == LAB_FILL).all() and (sc[npix:] == SC_FILL).all()
    assert len(np.unique(want_lab)) > 1
    # ---- segment_images: three sources of their own sizes; the reference per image on forward_dense of resize_inputs' staging buffer
    rng = np.random.default_rng(31)
    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in SOURCES]
    src_offs, at = [], 0
    for img in images:
        src_offs.append(at)
        at += img.size
    d_src = ctx.to_device(np.concatenate([img.ravel() for img in images]))
    rows, cols = [s[0] for s in SOURCES], [s[1] for s in SOURCES]
    dst, total = _ragged_layout(SOURCES, order=(2, 0, 1), gap=7)
    d_rlab, d_rsc = ctx.to_device(np.full(total, LAB_FILL, np.int32)), ctx.to_device(np.full(total, SC_FILL, np.float32))
    assert lib.mbn_net_segment_images(net.h, d_src.ptr, (C.c_int64 * n)(*src_offs), (C.c_int32 * n)(*rows), (C.c_int32 * n)(*cols), n, d_rlab.ptr,
                                      (C.c_int64 * n)(*dst), d_rsc.ptr) == pkg.EINVAL           # the net does not take uint8 images yet
    net.set_input_u8(True)
    bad_rows = [4 * h - 1] + rows[1:]                                                            # an item under 4 x the map
    assert lib.mbn_net_segment_images(net.h, d_src.ptr, (C.c_int64 * n)(*src_offs), (C.c_int32 * n)(*bad_rows), (C.c_int32 * n)(*cols), n, d_rlab.ptr,
                                      (C.c_int64 * n)(*dst), d_rsc.ptr) == pkg.EUNSUPPORTED
    ctx.sync()
    assert (d_rlab.download((total,), np.int32) == LAB_FILL).all(), "a refused call may not write"
    staging = net.resize_inputs(d_src.ptr, src_offs, rows, cols, fit=pkg.FIT_STRETCH)
    net.forward_dense(staging, d_dense.ptr, n)
    ctx.sync()
    dense = d_dense.download((n, h, w, CLASSES), np.float32)
    net.segment_images(d_src.ptr, src_offs, rows, cols, d_rlab.ptr, dst, d_rsc.ptr)
    ctx.sync()
    lab, sc = d_rlab.download((total,), np.int32), d_rsc.download((total,), np.float32)
    touched = np.zeros(total, bool)
    for i, ((sh, sw), off) in enumerate(zip(SOURCES, dst)):
        want_lab, want_sc = dense_any_ref.resample_argmax(dense[i:i + 1], sh, sw)
        assert np.array_equal(lab[off:off + sh * sw], want_lab.ravel()), "%s os %d image %d labels" % (dtype, os_, i)
        assert np.array_equal(sc[off:off + sh * sw].view(np.uint32), want_sc.view(np.uint32).ravel()), "%s os %d image %d scores" % (dtype, os_, i)
        touched[off:off + sh * sw] = True
    assert (lab[~touched] == LAB_FILL).all() and (sc[~touched] == SC_FILL).all()
    net.destroy()
    for b in (d_in, d_dense, d_lab, d_sc, d_src, d_rlab, d_rsc):
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def test_c_host_segment_source(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    seed, alpha, os_, sh, sw = 3, 0.5, 16, 75, 130
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, out = str(tmp_path / "a.ppm"), str(tmp_path / "out.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", str(seed), "--alpha", str(alpha), "--res", "%dx%d" % (ROWS, COLS), "--output-stride", str(os_), "--ppm", ppm]
    r = subprocess.run(common + ["--segment-source", out], capture_output=True, text=True, timeout=300)      # the default fit is the crop
    assert r.returncode == 2 and not os.path.exists(out), r.stdout + r.stderr
    r = subprocess.run(common + ["--fit", "stretch", "--segment-source", out], capture_output=True, text=True, timeout=300)
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
    staging = net.resize_input(d_src.ptr, 1, sh, sw, fit=pkg.FIT_STRETCH)
    net.segment_to(staging, 1, sh, sw, d_lab.ptr)
    ctx.sync()
    want = d_lab.download((sh, sw), np.int32)
    assert np.array_equal(got, want), "%d of %d pixels differ from Net.segment_to" % (int((got != want).sum()), want.size)
    assert len(np.unique(want)) > 1
    net.destroy()
    d_src.free()
    d_lab.free()
    hw.free()
