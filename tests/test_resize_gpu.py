"""The resize front-end on the GPU: mbn_resize_u8's bytes equal tests/resize_ref.py (which tests/test_resize_cpu.py pins to Pillow byte for byte) on
the smallest geometries that reach each way of going wrong; interior pointers, the mbn_alloc bounds rule, the handle's lifetime; the net runner's
resize_input in fp32, bf16 and int8 bit for bit against a forward on resize_ref's bytes; the C host's --ppm with an image of another size."""
import os
import re
import subprocess

import numpy as np
import pytest

import resize_ref

pytestmark = pytest.mark.gpu


def _image(shape, seed, extreme):
    """random bytes, or only 0 and 255: the worst case for the rounding and the clamp"""
    rng = np.random.default_rng(seed)
    if extreme:
        return (rng.integers(0, 2, shape) * 255).astype(np.uint8)
    return rng.integers(0, 256, shape, dtype=np.uint8)


def _run(pkg, ctx, img, oh, ow, box=None, in_off=0, out_off=0, fill=0xAB, slack=0):
    """mbn_resize_u8 on img [n][H][W][3], `in` at byte in_off of its buffer, `out` at out_off of a buffer pre-filled with `fill`: the whole out buffer"""
    n, H, W, _ = img.shape
    d_in = ctx.to_device(np.concatenate([np.zeros(in_off, np.uint8), img.ravel()]))
    d_out = ctx.to_device(np.full(out_off + n * oh * ow * 3 + slack, fill, np.uint8))
    r = pkg.Resizer(ctx, H, W, oh, ow, box)
    r.run(d_out.ptr + out_off, d_in.ptr + in_off, n)
    ctx.sync()
    raw = d_out.download((out_off + n * oh * ow * 3 + slack,), np.uint8)
    r.close()
    d_in.free()
    d_out.free()
    return raw


def _crop_box(pkg):
    return pkg.fit_box(375, 500, 224, 224, pkg.FIT_CROP, 0.875)


# (H, W, oh, ow, box, batch)
CASES = [
    (37, 53, 32, 32, None, 1),
    (20, 30, 64, 96, None, 1),                               # upscale; one-tap borders
    (1000, 17, 32, 32, None, 1),                             # 65 vertical taps with a horizontal upscale: the LDS window at its largest
    (33, 47, 32, 64, (3.5, 2.25, 40.0, 30.75), 1),           # fractional box
    (31, 29, 224, 224, (1, 2, 28, 30), 1),
    (64, 64, 64, 64, None, 1),                               # identity: a byte copy
    (64, 96, 32, 96, None, 1),                               # vertical pass only
    (64, 96, 64, 32, None, 1),                               # horizontal pass only
    (375, 500, 224, 224, "crop", 3),                         # batch stride
    (8, 4096, 4, 4096, None, 1),                             # the widest row; column tiling
    (1, 1, 5, 7, None, 1),
]


@pytest.mark.parametrize("index", range(len(CASES)))
def test_kernel_equals_ref(pkg, ctx, index):
    H, W, oh, ow, box, n = CASES[index]
    if box == "crop":
        box = _crop_box(pkg)
        assert box.tolist() == [85.9375, 23.4375, 414.0625, 351.5625]
    img = _image((n, H, W, 3), 100 + index, extreme=index % 3 == 2)
    want = resize_ref.resize(img, oh, ow, box)
    got = _run(pkg, ctx, img, oh, ow, box, slack=64)
    bad = int((got[:want.size] != want.ravel()).sum())
    assert bad == 0, "%dx%d -> %dx%d: %d of %d bytes differ from resize_ref" % (H, W, oh, ow, bad, want.size)
    assert (got[want.size:] == 0xAB).all(), "bytes behind `out` were written"
    if (H, W) == (oh, ow) and box is None:
        assert np.array_equal(got[:want.size], img.ravel())


def test_kernel_33x_downscale_both_axes(pkg, ctx):
    """67 taps on both axes (the envelope's edge) and two column tiles: the largest weights + staged rows + window the tile rule has to fit"""
    assert pkg.resize_ksize(2112, 0, 2112, 64) == 67 and pkg.resize_ksize(1056, 0, 1056, 32) == 67
    img = _image((1, 1056, 2112, 3), 7, extreme=False)
    want = resize_ref.resize(img, 32, 64)
    got = _run(pkg, ctx, img, 32, 64)
    assert np.array_equal(got, want.ravel())


def test_interior_pointers(pkg, ctx):
    img = _image((1, 37, 53, 3), 100, extreme=False)
    want = resize_ref.resize(img, 32, 32).ravel()
    aligned = _run(pkg, ctx, img, 32, 32)
    assert np.array_equal(aligned, want)
    for in_off in (1, 2, 3):
        got = _run(pkg, ctx, img, 32, 32, in_off=in_off, out_off=1, slack=7)
        assert got[0] == 0xAB and (got[1 + want.size:] == 0xAB).all(), "in + %d: a byte outside `out` was written" % in_off
        assert np.array_equal(got[1:1 + want.size], aligned), "in + %d: bytes differ from the aligned call" % in_off


def test_bounds_and_argument_errors(pkg, ctx):
    lib = ctx.lib
    img = _image((2, 37, 53, 3), 3, extreme=False)
    d_in, d_out = ctx.to_device(img), ctx.to_device(np.full(2 * 32 * 32 * 3, 0xAB, np.uint8))
    r = pkg.Resizer(ctx, 37, 53, 32, 32)
    call = lambda out, inp, n: lib.mbn_resize_u8(r.h, out, inp, n, None)
    assert call(d_out.ptr + 1, d_in.ptr, 2) == pkg.EINVAL            # `out` one byte short
    assert "resize_u8 out" in ctx.last_error()
    assert call(d_out.ptr, d_in.ptr + 1, 2) == pkg.EINVAL            # `in` one byte short
    assert "resize_u8 in" in ctx.last_error()
    assert call(None, d_in.ptr, 1) == pkg.EINVAL and call(d_out.ptr, None, 1) == pkg.EINVAL
    assert call(d_out.ptr, d_in.ptr, 0) == pkg.EINVAL and call(d_out.ptr, d_in.ptr, -1) == pkg.EINVAL
    assert lib.mbn_resize_u8(None, d_out.ptr, d_in.ptr, 1, None) == pkg.EINVAL
    assert call(d_out.ptr, d_in.ptr, 65536) == pkg.EUNSUPPORTED
    ctx.sync()
    assert (d_out.download((2 * 32 * 32 * 3,), np.uint8) == 0xAB).all(), "a refused call wrote to `out`"
    assert call(d_out.ptr + 32 * 32 * 3, d_in.ptr + 37 * 53 * 3, 1) == pkg.OK          # the second halves: exactly enough room
    ctx.sync()
    got = d_out.download((2, 32, 32, 3), np.uint8)
    assert (got[0] == 0xAB).all() and np.array_equal(got[1], resize_ref.resize(img[1], 32, 32))
    r.close()
    import ctypes as C
    h = C.c_void_p()
    mk = lambda *a: lib.mbn_resizer_create(ctx.h, *a, C.byref(h))
    assert mk(1057, 40, None, 32, 32) == pkg.EUNSUPPORTED and mk(40, 1057, None, 32, 32) == pkg.EUNSUPPORTED and not h.value
    assert mk(8193, 64, None, 4096, 64) == pkg.EUNSUPPORTED and mk(64, 64, None, 64, 4097) == pkg.EUNSUPPORTED
    assert mk(0, 64, None, 32, 32) == pkg.EINVAL and mk(64, 64, None, 32, 0) == pkg.EINVAL
    assert mk(37, 53, (C.c_float * 4)(0.0, 0.0, 54.0, 37.0), 32, 32) == pkg.EINVAL
    assert mk(37, 53, (C.c_float * 4)(5.0, 0.0, 5.0, 37.0), 32, 32) == pkg.EINVAL
    assert mk(37, 53, (C.c_float * 4)(0.0, float("nan"), 53.0, 37.0), 32, 32) == pkg.EINVAL
    assert lib.mbn_resizer_create(ctx.h, 37, 53, None, 32, 32, None) == pkg.EINVAL
    assert lib.mbn_resizer_destroy(None) == pkg.OK
    d_in.free()
    d_out.free()


def test_handle_lifetime(pkg, ctx):
    r = pkg.Resizer(ctx, 33, 47, 32, 64, (3.5, 2.25, 40.0, 30.75))
    a, b = _image((1, 33, 47, 3), 1, extreme=False), _image((3, 33, 47, 3), 2, extreme=True)
    d_a, d_b, d_out = ctx.to_device(a), ctx.to_device(b), ctx.alloc(3 * 32 * 64 * 3)
    r.run(d_out.ptr, d_a.ptr, 1)
    ctx.sync()
    assert np.array_equal(d_out.download((1, 32, 64, 3), np.uint8), resize_ref.resize(a, 32, 64, (3.5, 2.25, 40.0, 30.75)))
    r.run(d_out.ptr, d_b.ptr, 3)
    ctx.sync()
    assert np.array_equal(d_out.download((3, 32, 64, 3), np.uint8), resize_ref.resize(b, 32, 64, (3.5, 2.25, 40.0, 30.75)))
    r.close()
    r.close()                                     # idempotent on the Python side
    for buf in (d_a, d_b, d_out):
        buf.free()
    other = pkg.Context(0)                        # a context shut down with a handle alive: the handle goes with it
    live = pkg.Resizer(other, 20, 30, 64, 96)
    d_in, d_o = other.to_device(a[:, :20, :30].copy()), other.alloc(64 * 96 * 3)
    live.run(d_o.ptr, d_in.ptr, 1)
    assert other.lib.mbn_shutdown(other.h) == pkg.OK
    other.h = None
    live.h = None


def test_capture_in_a_graph(pkg, ctx):
    """the hot call makes no blocking call: it is legal between mbn_graph_begin and mbn_graph_end"""
    import ctypes as C
    img = _image((2, 37, 53, 3), 11, extreme=False)
    d_in, d_out = ctx.to_device(img), ctx.to_device(np.zeros(2 * 32 * 32 * 3, np.uint8))
    r = pkg.Resizer(ctx, 37, 53, 32, 32)
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_resize_u8(r.h, d_out.ptr, d_in.ptr, 2, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert not d_out.download((2 * 32 * 32 * 3,), np.uint8).any(), "the captured call ran"
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(d_out.download((2, 32, 32, 3), np.uint8), resize_ref.resize(img, 32, 32))
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    d_in.free()
    d_out.free()


def _net(pkg, ctx, tmp_path, batch):
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=0.25, classes=40, seed=7, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(64, 96), lib=pkg.load())
    return hw, pkg.Net(ctx, hw.plan, hw.blob.copy(), batch)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "i8"])
def test_net_resize_input(pkg, ctx, tmp_path, dtype):
    n, classes = 2, 40
    hw, net = _net(pkg, ctx, tmp_path, n)
    net.set_dtype({"f32": pkg.DT_F32, "bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype])
    net.set_input_u8(True)
    d_a, d_b = ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    staging = []
    for (H, W), seed in (((75, 100), 1), ((50, 80), 2)):     # the second source rebuilds the resizer
        src = _image((n, H, W, 3), seed, extreme=False)
        box = pkg.fit_box(H, W, 64, 96, pkg.FIT_CROP, 1.0)
        want_u8 = resize_ref.resize(src, 64, 96, box)
        d_src = ctx.to_device(src)
        p = net.resize_input(d_src.ptr, n, H, W, pkg.FIT_CROP, 1.0)
        staging.append(p)
        net.forward(p, d_a.ptr, n)
        ctx.sync()
        got_u8 = np.empty((n, 64, 96, 3), np.uint8)
        assert ctx.lib.mbn_download(ctx.h, got_u8.ctypes.data, p, got_u8.nbytes) == pkg.OK
        assert np.array_equal(got_u8, want_u8), "%s %dx%d: the staged images differ from resize_ref" % (dtype, H, W)
        d_ref = ctx.to_device(want_u8)
        net.forward(d_ref.ptr, d_b.ptr, n)
        ctx.sync()
        a, b = d_a.download((n, classes), np.uint32), d_b.download((n, classes), np.uint32)
        assert np.array_equal(a, b), "%s %dx%d: logits differ from a forward on resize_ref's bytes" % (dtype, H, W)
        assert np.isfinite(a.view(np.float32)).all() and a.view(np.float32).std() > 0
        d_src.free()
        d_ref.free()
    assert staging[0] == staging[1], "the staging buffer was reallocated"
    assert ctx.lib.mbn_net_resize_input(net.h, None, n, 75, 100, pkg.FIT_CROP, 1.0, None) == pkg.EINVAL
    with pytest.raises(pkg.MbnError):
        net.resize_input(d_a.ptr, n + 1, 75, 100)             # beyond max_batch
    with pytest.raises(pkg.MbnError):
        net.resize_input(d_a.ptr, n, 75, 100, pkg.FIT_CROP, 0.0)
    net.destroy()
    hw.free()
    d_a.free()
    d_b.free()


def test_net_resize_input_stretch(pkg, ctx, tmp_path):
    hw, net = _net(pkg, ctx, tmp_path, 1)
    src = _image((1, 40, 200, 3), 5, extreme=True)
    d_src = ctx.to_device(src)
    p = net.resize_input(d_src.ptr, 1, 40, 200, pkg.FIT_STRETCH, 0.5)       # the fraction is ignored
    ctx.sync()
    got = np.empty((1, 64, 96, 3), np.uint8)
    assert ctx.lib.mbn_download(ctx.h, got.ctypes.data, p, got.nbytes) == pkg.OK
    assert np.array_equal(got, resize_ref.resize(src, 64, 96))
    net.destroy()
    hw.free()
    d_src.free()


def test_c_host_ppm_of_another_size(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    src = _image((75, 100, 3), 31, extreme=False)
    small = resize_ref.resize(src, 64, 96, pkg.fit_box(75, 100, 64, 96, pkg.FIT_CROP, 1.0))
    odd, fit = str(tmp_path / "odd.ppm"), str(tmp_path / "fit.ppm")
    assert pkg.load().mbn_write_ppm(odd.encode(), src.ctypes.data, 100, 75) == 0
    assert pkg.load().mbn_write_ppm(fit.encode(), small.ctypes.data, 96, 64) == 0
    lines = []
    for ppm in (odd, fit):
        r = subprocess.run([exe, "--synthetic", "7", "--alpha", "0.25", "--res", "64x96", "--ppm", ppm], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "using a synthetic one" not in r.stderr and "warning" not in r.stderr, r.stderr
        m = re.search(r"^top-5:.*$", r.stdout, re.M)
        assert m, r.stdout
        lines.append(m.group(0))
    assert lines[0] == lines[1], lines
