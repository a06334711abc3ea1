"""The resize front-end's filters on the GPU: the table kernels (mbn_resizer_create_filter: one kernel on five filters' tables, NEAREST's gather)
against Pillow's recorded bytes (tests/golden/resize_pillow_filters.npz) for every filter and geometry, also at batch 3 and through pointers one byte
off alignment with a guard band around `out`; the ragged kernels (NEAREST, BOX, BILINEAR, BICUBIC) in one launch of five differently sized images
against the table kernel's bytes; the device's own taps as int32 against the host's; the net runner's filter and the C host's --filter. Every
comparison is exact equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resize_filters_ref as R
from test_resize_filters_cpu import N_CASES, cases

pytestmark = pytest.mark.gpu

RAGGED_FILTERS = (R.NEAREST, R.BOX, R.BILINEAR, R.BICUBIC)
GUARD = 16


def _table(pkg, ctx, f, img, oh, ow, box, in_off=0, out_off=0):
    """mbn_resize_u8 under filter f on img [n][H][W][3]: `in` at byte in_off of its buffer, `out` at out_off + GUARD of a buffer of 0xAB with GUARD
    more bytes behind: (the output, the bytes around it)"""
    n, H, W, _ = img.shape
    nb = n * oh * ow * 3
    d_in = ctx.to_device(np.concatenate([np.zeros(in_off, np.uint8), img.ravel()]))
    d_out = ctx.to_device(np.full(GUARD + out_off + nb + GUARD, 0xAB, np.uint8))
    r = pkg.Resizer(ctx, H, W, oh, ow, box, filter=f)
    r.run(d_out.ptr + GUARD + out_off, d_in.ptr + in_off, n)
    ctx.sync()
    raw = d_out.download((GUARD + out_off + nb + GUARD,), np.uint8)
    r.close()
    d_in.free()
    d_out.free()
    lo = GUARD + out_off
    return raw[lo:lo + nb].reshape(n, oh, ow, 3), np.concatenate([raw[:lo], raw[lo + nb:]])


@pytest.mark.parametrize("index", range(N_CASES))
def test_table_kernel_equals_pillow(pkg, ctx, index):
    name, f, img, box, want = cases()[index]
    oh, ow = want.shape[:2]
    got, guard = _table(pkg, ctx, f, img[None], oh, ow, box)
    bad = int((got[0] != want).sum())
    assert bad == 0, "%s under %s: %d of %d bytes differ from Pillow's" % (name, R.NAMES[f], bad, want.size)
    assert (guard == 0xAB).all(), "bytes around `out` were written"
    # batch 3 (the image, its mirror, its complement), `in` and `out` one byte off alignment
    batch = np.stack([img, img[:, ::-1], 255 - img])
    got, guard = _table(pkg, ctx, f, batch, oh, ow, box, in_off=1, out_off=1)
    assert (guard == 0xAB).all(), "%s under %s: bytes around an unaligned `out` were written" % (name, R.NAMES[f])
    assert np.array_equal(got[0], want), "%s under %s: an unaligned call differs" % (name, R.NAMES[f])
    for i in (1, 2):
        assert np.array_equal(got[i], R.resize(f, batch[i], oh, ow, box)), "%s under %s: image %d of the batch" % (name, R.NAMES[f], i)


@pytest.mark.parametrize("f", R.FILTERS, ids=[R.NAMES[f] for f in R.FILTERS])
def test_table_kernel_every_alignment(pkg, ctx, f):
    """an output row of 24 * 3 = 72 bytes and one of 33 * 3 = 99: head, dwords and tail of NEAREST's stores at every offset of `out` and `in`"""
    for name in ("inexact_box", "up"):
        _, _, img, box, want = [c for c in cases() if c[0] == name and c[1] == f][0]
        for off in (1, 2, 3):
            got, guard = _table(pkg, ctx, f, img[None], want.shape[0], want.shape[1], box, in_off=4 - off, out_off=off)
            assert (guard == 0xAB).all() and np.array_equal(got[0], want), (name, R.NAMES[f], off)


def test_create_refusals(pkg, ctx):
    lib, h = ctx.lib, C.c_void_p()
    mk = lambda f, *a: lib.mbn_resizer_create_filter(ctx.h, f, *a, C.byref(h))
    assert mk(6, 37, 53, None, 32, 32) == pkg.EINVAL and mk(-1, 37, 53, None, 32, 32) == pkg.EINVAL and not h.value
    assert mk(R.LANCZOS, 353, 40, None, 32, 32) == pkg.EUNSUPPORTED and mk(R.BICUBIC, 529, 40, None, 32, 32) == pkg.EUNSUPPORTED
    assert mk(R.BOX, 3200, 3200, None, 64, 64) == pkg.EUNSUPPORTED and not h.value           # a one-row tile does not fit: the plan's answer
    assert mk(R.NEAREST, 8193, 64, None, 32, 32) == pkg.EUNSUPPORTED
    assert mk(R.NEAREST, 37, 53, (C.c_float * 4)(0.0, 0.0, 54.0, 37.0), 32, 32) == pkg.EINVAL
    rag = lambda f, *a: lib.mbn_ragged_resizer_create_filter(ctx.h, f, *a, C.byref(h))
    assert rag(R.HAMMING, 4, 32, 32) == pkg.EUNSUPPORTED and rag(R.LANCZOS, 4, 32, 32) == pkg.EUNSUPPORTED and not h.value
    assert rag(6, 4, 32, 32) == pkg.EINVAL and rag(R.BICUBIC, 0, 32, 32) == pkg.EINVAL
    d = ctx.alloc(4 * 32 * 69)
    for f in (R.HAMMING, R.LANCZOS):
        assert lib.mbn_resize_taps_device_filter(ctx.h, f, 37, 0.0, 37.0, 32, d.ptr, d.ptr, d.ptr) == pkg.EUNSUPPORTED
    assert lib.mbn_resize_taps_device_filter(ctx.h, 9, 37, 0.0, 37.0, 32, d.ptr, d.ptr, d.ptr) == pkg.EINVAL
    assert lib.mbn_resize_taps_device_filter(ctx.h, R.BICUBIC, 529, 0.0, 529.0, 32, d.ptr, d.ptr, d.ptr) == pkg.EUNSUPPORTED
    d.free()


def _five(f):
    """five differently sized fixture sources with their boxes: the float box, the upscale, two tiles on both axes, the identity's source and the
    steepest one the filter has in the fixture (NEAREST: a 1222-wide row)"""
    steep = {R.NEAREST: "nearest_1222", R.BOX: "steep_box", R.BILINEAR: "steep_33x", R.BICUBIC: "steep_bicubic_67"}[f]
    by_name = {c[0]: c for c in cases() if c[1] == f}
    return [(by_name[n][2], tuple(float(v) for v in by_name[n][3])) for n in ("inexact_box", "up", "two_tiles", "identity", steep)]


@pytest.mark.parametrize("f", RAGGED_FILTERS, ids=[R.NAMES[f] for f in RAGGED_FILTERS])
def test_ragged_kernel_equals_table_kernel(pkg, ctx, f):
    """one launch of five images into 35 x 70 (two column tiles, two row tiles) from byte 1 of the source, `out` one byte off alignment"""
    oh, ow = 35, 70
    items = _five(f)
    offs, cur = [], 1
    for img, _ in items:
        offs.append(cur)
        cur += img.size + 1                                  # the gaps move the alignment from image to image
    src = np.zeros(cur, np.uint8)
    for (img, _), off in zip(items, offs):
        src[off:off + img.size] = img.ravel()
    n, nb = len(items), len(items) * oh * ow * 3
    d_src, d_out = ctx.to_device(src), ctx.to_device(np.full(GUARD + 1 + nb + GUARD, 0xAB, np.uint8))
    r = pkg.RaggedResizer(ctx, n, oh, ow, filter=f)
    r.set([(off, img.shape[0], img.shape[1], box) for (img, box), off in zip(items, offs)])
    r.run(d_out.ptr + GUARD + 1, d_src.ptr)
    ctx.sync()
    raw = d_out.download((GUARD + 1 + nb + GUARD,), np.uint8)
    r.close()
    d_src.free()
    d_out.free()
    got = raw[GUARD + 1:GUARD + 1 + nb].reshape(n, oh, ow, 3)
    assert (raw[:GUARD + 1] == 0xAB).all() and (raw[GUARD + 1 + nb:] == 0xAB).all(), "bytes around `out` were written"
    for i, (img, box) in enumerate(items):
        table, _ = _table(pkg, ctx, f, img[None], oh, ow, box)
        bad = int((got[i] != table[0]).sum())
        assert bad == 0, "%s image %d (%dx%d): %d bytes differ from the table kernel's" % (R.NAMES[f], i, img.shape[0], img.shape[1], bad)
        assert np.array_equal(table[0], R.resize(f, img, oh, ow, box)), "%s image %d: the table kernel differs from the reference" % (R.NAMES[f], i)


# (in_size, b0, b1, out_size)
AXES = [(53, 0.1, 52.7, 24), (7, 0, 7, 33), (150, 0, 150, 70), (12, 0, 12, 12), (396, 0, 396, 24), (1584, 0, 1584, 24), (504, 0, 504, 188),
        (1222, 0, 1222, 65), (8192, 0, 8192, 4096)]


@pytest.mark.parametrize("f", RAGGED_FILTERS, ids=[R.NAMES[f] for f in RAGGED_FILTERS])
def test_device_taps_equal_host(pkg, ctx, f):
    for in_size, b0, b1, out_size in AXES:
        b0, b1 = float(np.float32(b0)), float(np.float32(b1))
        if R.ksize(f, in_size, b0, b1, out_size) > 67:
            continue
        first, count, weights = pkg.resize_taps_device(ctx, in_size, b0, b1, out_size, filter=f)
        hf, hc, hw = pkg.resize_taps(in_size, b0, b1, out_size, filter=f)
        assert weights.dtype == np.int32 and weights.shape == hw.shape
        assert np.array_equal(first, hf) and np.array_equal(count, hc), (R.NAMES[f], in_size, out_size)
        bad = int((weights != hw).sum())
        assert bad == 0, "%s %d -> %d: %d of %d weights differ from the host's" % (R.NAMES[f], in_size, out_size, bad, hw.size)
        if out_size <= 200:
            rf, rc, rw = R.taps(f, in_size, b0, b1, out_size)
            assert np.array_equal(first, rf) and np.array_equal(count, rc) and np.array_equal(weights, rw), (R.NAMES[f], in_size, out_size)


def _net(pkg, ctx, tmp_path, batch, classes=40):
    path = str(tmp_path / ("w%d.h5" % classes))
    pkg.synthetic_h5(path, alpha=0.25, classes=classes, seed=7, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(64, 96), lib=pkg.load())
    return hw, pkg.Net(ctx, hw.plan, hw.blob.copy(), batch)


def _staged(pkg, ctx, p, n):
    got = np.empty((n, 64, 96, 3), np.uint8)
    assert ctx.lib.mbn_download(ctx.h, got.ctypes.data, p, got.nbytes) == pkg.OK
    return got


def test_net_resize_filter(pkg, ctx, tmp_path):
    import resize_ref
    n, classes, H, W = 2, 40, 75, 100
    hw, net = _net(pkg, ctx, tmp_path, n)
    net.set_input_u8(True)
    src = np.random.default_rng(41).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    box = pkg.fit_box(H, W, 64, 96, pkg.FIT_CROP, 1.0)
    d_src, d_a, d_b = ctx.to_device(src), ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    idx_a, prob = ctx.alloc(n * 4), ctx.alloc(n * 4)
    # no setter call: today's bilinear bytes
    assert net.resize_filter() == pkg.FILTER_BILINEAR
    p = net.resize_input(d_src.ptr, n, H, W, pkg.FIT_CROP, 1.0)
    ctx.sync()
    assert np.array_equal(_staged(pkg, ctx, p, n), resize_ref.resize(src, 64, 96, box)), "the default filter is not the bilinear one"
    for f in (R.BICUBIC, R.NEAREST, R.LANCZOS):               # the cached resizer is rebuilt when the filter changes, the geometry unchanged
        net.set_resize_filter(f)
        assert net.resize_filter() == f
        want_u8 = R.resize(f, src, 64, 96, box)
        p = net.resize_input(d_src.ptr, n, H, W, pkg.FIT_CROP, 1.0)
        net.forward(p, d_a.ptr, n)
        ctx.sync()
        assert np.array_equal(_staged(pkg, ctx, p, n), want_u8), "%s: the staged images differ from the reference" % R.NAMES[f]
        d_ref = ctx.to_device(want_u8)
        net.forward(d_ref.ptr, d_b.ptr, n)
        ctx.sync()
        a, b = d_a.download((n, classes), np.uint32), d_b.download((n, classes), np.uint32)
        assert np.array_equal(a, b), "%s: logits differ from a forward on the reference's bytes" % R.NAMES[f]
        assert np.isfinite(a.view(np.float32)).all() and a.view(np.float32).std() > 0
        d_ref.free()
    # images of different sizes: the ragged path under the net's filter; HAMMING / LANCZOS are refused and the net stays usable
    images = [src[0], src[1, :50, :80].copy()]
    offs = [0, images[0].size]
    d_two = ctx.to_device(np.concatenate([im.ravel() for im in images]))
    rows, cols = [im.shape[0] for im in images], [im.shape[1] for im in images]
    want = lambda f: np.stack([R.resize(f, im, 64, 96, pkg.fit_box(im.shape[0], im.shape[1], 64, 96, pkg.FIT_CROP, 1.0)) for im in images])
    net.set_resize_filter(R.BICUBIC)
    p = net.resize_inputs(d_two.ptr, offs, rows, cols, pkg.FIT_CROP, 1.0)
    ctx.sync()
    assert np.array_equal(_staged(pkg, ctx, p, 2), want(R.BICUBIC))
    for f in (R.LANCZOS, R.HAMMING):
        net.set_resize_filter(f)
        with pytest.raises(pkg.MbnError) as e:
            net.resize_inputs(d_two.ptr, offs, rows, cols, pkg.FIT_CROP, 1.0)
        assert e.value.code == pkg.EUNSUPPORTED
    net.set_resize_filter(R.NEAREST)
    p = net.resize_inputs(d_two.ptr, offs, rows, cols, pkg.FIT_CROP, 1.0)
    ctx.sync()
    assert np.array_equal(_staged(pkg, ctx, p, 2), want(R.NEAREST))
    assert ctx.lib.mbn_net_set_resize_filter(net.h, 6) == pkg.EINVAL and ctx.lib.mbn_net_set_resize_filter(None, 2) == pkg.EINVAL
    assert net.resize_filter() == R.NEAREST
    net.destroy()
    hw.free()
    for b in (d_src, d_a, d_b, idx_a, prob, d_two):
        b.free()


def test_net_classify_under_bicubic(pkg, ctx, tmp_path):
    """mbn_net_set_resize_filter(BICUBIC) then classify: the classes and probabilities of a classify on the reference's bytes, bit for bit"""
    n, H, W = 2, 75, 100
    hw, net = _net(pkg, ctx, tmp_path, n)
    net.set_input_u8(True)
    net.set_resize_filter(pkg.FILTER_BICUBIC)
    _, _, img, _, _ = [c for c in cases() if c[0] == "two_tiles"][0]
    src = np.stack([img[:H, :W], img[5:5 + H, 50:50 + W]])
    box = pkg.fit_box(H, W, 64, 96, pkg.FIT_CROP, 0.875)
    d_src, d_ref = ctx.to_device(src), ctx.to_device(R.resize(R.BICUBIC, src, 64, 96, box))
    out = []
    for images in (net.resize_input(d_src.ptr, n, H, W, pkg.FIT_CROP, 0.875), d_ref.ptr):
        d_idx, d_prob = ctx.alloc(n * 5 * 4), ctx.alloc(n * 5 * 4)
        assert ctx.lib.mbn_net_classify(net.h, C.c_void_p(images), n, 5, d_idx.ptr, d_prob.ptr) == pkg.OK, ctx.last_error()
        ctx.sync()
        out.append((d_idx.download((n, 5), np.int32), d_prob.download((n, 5), np.uint32)))
        d_idx.free()
        d_prob.free()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    net.destroy()
    hw.free()
    d_src.free()
    d_ref.free()


def test_c_host_filter(pkg, ctx, tmp_path):
    """mobilenet --ppm F --filter bicubic prints the top-5 of the image the reference resizes with bicubic; the usage errors are status 2"""
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    _, _, img, _, _ = [c for c in cases() if c[0] == "two_tiles"][0]
    src = np.ascontiguousarray(img[:75, :100])
    small = {f: R.resize(f, src, 64, 96, pkg.fit_box(75, 100, 64, 96, pkg.FIT_CROP, 1.0)) for f in (R.BICUBIC, R.BILINEAR)}
    assert not np.array_equal(small[R.BICUBIC], small[R.BILINEAR])
    odd, fit = str(tmp_path / "odd.ppm"), str(tmp_path / "fit.ppm")
    assert pkg.load().mbn_write_ppm(odd.encode(), src.ctypes.data, 100, 75) == 0
    assert pkg.load().mbn_write_ppm(fit.encode(), small[R.BICUBIC].ctypes.data, 96, 64) == 0
    common = [exe, "--synthetic", "7", "--alpha", "0.25", "--res", "64x96"]
    lines = []
    for extra in (["--ppm", odd, "--filter", "bicubic"], ["--ppm", fit]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "warning" not in r.stderr, r.stderr
        lines.append(re.search(r"^top-5:.*$", r.stdout, re.M).group(0))
    assert lines[0] == lines[1], lines
    # the Python path on the same image and the C host's weights (seed 7, 1000 classes): the same top-1
    hw, net = _net(pkg, ctx, tmp_path, 1, classes=1000)
    net.set_input_u8(True)
    net.set_resize_filter(pkg.FILTER_BICUBIC)
    d_src, d_idx, d_prob = ctx.to_device(src), ctx.alloc(4), ctx.alloc(4)
    p = net.resize_input(d_src.ptr, 1, 75, 100, pkg.FIT_CROP, 1.0)
    assert ctx.lib.mbn_net_classify(net.h, C.c_void_p(p), 1, 1, d_idx.ptr, d_prob.ptr) == pkg.OK, ctx.last_error()
    ctx.sync()
    assert int(d_idx.download((1,), np.int32)[0]) + 1 == int(re.search(r"^top-5: (\d+) ", lines[0], re.M).group(1))
    net.destroy()
    hw.free()
    for b in (d_src, d_idx, d_prob):
        b.free()
    r = subprocess.run(common + ["--ppm", odd, "--filter", "cubic"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage" in r.stderr
    for name in ("hamming", "lanczos"):
        r = subprocess.run(common + ["--batch", "2", "--ppm", odd, "--ppm", fit, "--filter", name], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and name in r.stderr and "sin" in r.stderr, r.stderr
