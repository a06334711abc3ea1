"""The ragged resize on the GPU: one launch of mbn_resize_ragged_u8 over images of different sizes, byte for byte tests/resize_ref.py per image (and
Pillow's recorded bytes, and the table kernel's); the device's own tap tables as int32 against the host's and the reference's; refusals, the mbn_alloc
bounds rule, guard bytes, re-set, lifetime, graph capture; the net runner's resize_inputs in fp32, bf16 and int8; the C host with several --ppm.
Every comparison is exact equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resize_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _image(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _crop(pkg, h, w, oh, ow, f=0.875):
    return tuple(float(v) for v in pkg.fit_box(h, w, oh, ow, pkg.FIT_CROP, f))


def _layout(images, first=0, gaps=(0,), order=None):
    """byte offsets for `images` laid out in `order` (default: as given) from byte `first`, gaps[k % len] bytes behind the k-th placed; (offsets, size)"""
    offs, cur = [0] * len(images), first
    for k, i in enumerate(order if order is not None else range(len(images))):
        offs[i] = cur
        cur += images[i].size + gaps[k % len(gaps)]
    return offs, max(o + img.size for o, img in zip(offs, images))          # the source ends with the last image's last byte


def _source(images, offs, size):
    buf = np.zeros(size, np.uint8)
    for img, off in zip(images, offs):
        buf[off:off + img.size] = img.ravel()
    return buf


def _run(pkg, ctx, images, boxes, offs, size, oh, ow, max_batch=None):
    """one ragged launch of `images` (image i at byte offs[i] of a source of `size` bytes): [n][oh][ow][3]"""
    n = len(images)
    d_src, d_out = ctx.to_device(_source(images, offs, size)), ctx.to_device(np.full(n * oh * ow * 3, 0xAB, np.uint8))
    r = pkg.RaggedResizer(ctx, max_batch or n, oh, ow)
    r.set([(off, img.shape[0], img.shape[1], box) for img, box, off in zip(images, boxes, offs)])
    r.run(d_out.ptr, d_src.ptr)
    ctx.sync()
    got = d_out.download((n, oh, ow, 3), np.uint8)
    r.close()
    d_src.free()
    d_out.free()
    return got


def _assert_each_equals_ref(got, images, boxes, oh, ow):
    for i, (img, box) in enumerate(zip(images, boxes)):
        want = resize_ref.resize(img, oh, ow, box)
        bad = int((got[i] != want).sum())
        assert bad == 0, "image %d (%dx%d -> %dx%d): %d of %d bytes differ from resize_ref" % (i, img.shape[0], img.shape[1], oh, ow, bad, want.size)


# (in_size, b0, b1, out_size)
AXES = [(53, 0, 53, 32), (30, 0, 30, 96), (1, 0, 1, 7), (64, 0, 64, 64),
        (1290, 0, 1290, 40),                       # ksize 67
        (2300, 0, 2300, 72),                       # ksize 65
        (47, 2.25, 30.75, 64),                     # a fractional box
        (41, 0.1, 40.7, 20), (53, 0.3, 52.9, 32),  # the inexact box of the golden file, both axes
        (500, 85.9375, 414.0625, 224)]             # 500 wide, crop 0.875 -> 224


@pytest.mark.parametrize("axis", AXES)
def test_device_taps_equal_host_and_ref(pkg, ctx, axis):
    in_size, b0, b1, out_size = axis
    b0, b1 = float(np.float32(b0)), float(np.float32(b1))
    first, count, weights = pkg.resize_taps_device(ctx, in_size, b0, b1, out_size)
    for name, (f, c, w) in (("host", pkg.resize_taps(in_size, b0, b1, out_size)), ("resize_ref", resize_ref.taps(in_size, b0, b1, out_size))):
        assert weights.dtype == np.int32 and weights.shape == w.shape, name
        assert np.array_equal(first, f) and np.array_equal(count, c), name
        bad = int((weights != w).sum())
        assert bad == 0, "%s: %d of %d weights differ (largest difference %d)" % (name, bad, w.size, int(np.abs(weights.astype(np.int64) - w).max()))
    if axis == AXES[4]:
        assert weights.shape[1] == 67
    if axis == AXES[5]:
        assert weights.shape[1] == 65


def test_device_taps_refusals(pkg, ctx):
    lib = ctx.lib
    d = ctx.alloc(4 * 32 * 69)
    call = lambda *a: lib.mbn_resize_taps_device(ctx.h, *a)
    assert call(1057, 0.0, 1057.0, 32, d.ptr, d.ptr, d.ptr) == pkg.EUNSUPPORTED          # 69 taps
    assert call(37, 5.0, 5.0, 32, d.ptr, d.ptr, d.ptr) == pkg.EINVAL
    assert call(37, 0.0, 37.0, 32, None, d.ptr, d.ptr) == pkg.EINVAL
    assert call(37, 0.0, 37.0, 32, d.ptr, d.ptr, d.ptr + 4 * 32 * 69 - 4 * 32 * 5 + 4) == pkg.EINVAL      # the weights one int32 short
    assert lib.mbn_resize_taps_device(None, 37, 0.0, 37.0, 32, d.ptr, d.ptr, d.ptr) == pkg.EINVAL
    d.free()


def _mixed_batch(pkg):
    """out 40 x 72: two tiles in x (64 + 8), two in y for the mild scales, flatter tiles for the steep ones"""
    oh, ow = 40, 72
    shapes = [(37, 53), (20, 30), (1, 1), (40, 72), (1290, 17), (9, 2300), (33, 47), (375, 500)]
    images = [_image(s + (3,), 200 + i) for i, s in enumerate(shapes)]
    boxes = [None, None, None, None, None, None, (3.5, 2.25, 40.0, 30.75), _crop(pkg, 375, 500, oh, ow)]
    # laid out back to front from byte 1, with gaps that move the alignment: the offsets fall, one is odd, one is 2 mod 4
    offs, size = _layout(images, first=1, gaps=(0, 3, 1, 2), order=range(len(images) - 1, -1, -1))
    images.append(images[0])                        # 37 x 53 again: another box, the SAME source bytes
    boxes.append((1.5, 0.0, 50.25, 36.5))
    offs.append(offs[0])
    return oh, ow, images, boxes, offs, size


def test_mixed_batch_equals_ref_per_image(pkg, ctx):
    oh, ow, images, boxes, offs, size = _mixed_batch(pkg)
    assert any(o % 2 == 1 for o in offs) and any(o % 4 == 2 for o in offs) and offs[:8] != sorted(offs[:8]) and offs[8] == offs[0]
    assert pkg.resize_ksize(1290, 0, 1290, oh) == 67 and pkg.resize_ksize(2300, 0, 2300, ow) == 65
    got = _run(pkg, ctx, images, boxes, offs, size, oh, ow)
    _assert_each_equals_ref(got, images, boxes, oh, ow)
    assert np.array_equal(got[3], images[3]), "the identity is a byte copy"


def test_one_partial_tile_on_the_32_column_path(pkg, ctx):
    """out 5 x 7. 310 rows -> 5 is a 62x downscale, 125 taps: outside the envelope, so that batch is refused as a whole; 165 rows -> 5 (67 taps) is
    the steepest image this output takes"""
    oh, ow = 5, 7
    r = pkg.RaggedResizer(ctx, 3, oh, ow)
    with pytest.raises(pkg.MbnError) as e:
        r.set([(0, 1, 1, None), (3, 64, 64, None), (3 + 64 * 64 * 3, 310, 9, None)])
    assert e.value.code == pkg.EUNSUPPORTED
    r.close()
    images = [_image(s + (3,), 300 + i) for i, s in enumerate([(1, 1), (64, 64), (165, 9)])]
    boxes = [None] * 3
    offs, size = _layout(images, first=2, gaps=(1,))
    assert pkg.resize_ksize(165, 0, 165, oh) == 67
    _assert_each_equals_ref(_run(pkg, ctx, images, boxes, offs, size, oh, ow), images, boxes, oh, ow)


def test_224_batch(pkg, ctx):
    oh = ow = 224
    images = [_image(s + (3,), 400 + i) for i, s in enumerate([(31, 29), (375, 500), (480, 640), (224, 224)])]
    boxes = [(1, 2, 28, 30), _crop(pkg, 375, 500, oh, ow), None, None]
    assert list(boxes[1]) == [85.9375, 23.4375, 414.0625, 351.5625]
    offs, size = _layout(images, first=3, gaps=(2, 0, 1))
    got = _run(pkg, ctx, images, boxes, offs, size, oh, ow, max_batch=7)
    _assert_each_equals_ref(got, images, boxes, oh, ow)
    assert np.array_equal(got[3], images[3])


def test_pillows_bytes(pkg, ctx):
    """each golden case as a ragged batch of one, against the bytes Pillow itself produced"""
    z = np.load(os.path.join(HERE, "golden", "resize_pillow.npz"))
    assert len(z["names"]) == 10
    for name in (str(n) for n in z["names"]):
        img, box, want = z[name + "_in"], z[name + "_box"], z[name + "_out"]
        got = _run(pkg, ctx, [img], [tuple(float(v) for v in box)], [0], img.size, want.shape[0], want.shape[1])
        bad = int((got[0] != want).sum())
        assert bad == 0, "%s: %d of %d bytes differ from Pillow's" % (name, bad, want.size)


def test_same_bytes_as_the_table_kernel(pkg, ctx):
    n, H, W, oh, ow = 3, 375, 500, 224, 224
    img = _image((n, H, W, 3), 5)
    box = _crop(pkg, H, W, oh, ow)
    d_in, d_a = ctx.to_device(img), ctx.alloc(n * oh * ow * 3)
    rz = pkg.Resizer(ctx, H, W, oh, ow, box)
    rz.run(d_a.ptr, d_in.ptr, n)
    ctx.sync()
    table = d_a.download((n, oh, ow, 3), np.uint8)
    rz.close()
    d_in.free()
    d_a.free()
    ragged = _run(pkg, ctx, list(img), [box] * n, [i * H * W * 3 for i in range(n)], img.size, oh, ow)
    assert np.array_equal(ragged, table)


def test_refusals_and_bounds(pkg, ctx):
    lib = ctx.lib
    oh = ow = 32
    a, b = _image((37, 53, 3), 1), _image((20, 30, 3), 2)
    offs, size = _layout([a, b], first=5, gaps=(3,))
    d_src = ctx.to_device(_source([a, b], offs, size))                     # exactly as long as the last image's last byte
    out_bytes = 2 * oh * ow * 3
    d_out = ctx.to_device(np.full(8 + out_bytes + 8, 0xAB, np.uint8))
    good = [(offs[0], 37, 53, None), (offs[1], 20, 30, None)]
    r = pkg.RaggedResizer(ctx, 3, oh, ow)
    launch = lambda out, src: lib.mbn_resize_ragged_u8(r.h, out, src, None)
    assert launch(d_out.ptr, d_src.ptr) == pkg.EINVAL                      # no batch yet
    # 69 taps in the middle of a batch: refused as a whole, and the handle is left without a batch
    r.set(good)
    with pytest.raises(pkg.MbnError) as e:
        r.set([good[0], (0, 1057, 2, None), good[1]])
    assert e.value.code == pkg.EUNSUPPORTED and pkg.resize_ksize(1057, 0, 1057, 32) == 69
    assert launch(d_out.ptr + 8, d_src.ptr) == pkg.EINVAL
    for bad in ((0, 37, 53, (0.0, float("nan"), 53.0, 37.0)), (0, 37, 53, (5.0, 0.0, 5.0, 37.0)), (-1, 37, 53, None), (0, 0, 53, (0.0, 0.0, 53.0, 1.0)),
                (0, 37, 53, (0.0, 0.0, 54.0, 37.0))):
        with pytest.raises(pkg.MbnError) as e:
            r.set([good[0], bad])
        assert e.value.code == pkg.EINVAL, bad
    with pytest.raises(pkg.MbnError) as e:
        r.set([(0, 8193, 2, None)])
    assert e.value.code == pkg.EUNSUPPORTED
    with pytest.raises(pkg.MbnError) as e:
        r.set(good + good)                                                 # max_batch + 1
    assert e.value.code == pkg.EINVAL
    items = pkg.resize_items(good)
    assert lib.mbn_ragged_resizer_set(r.h, items, 0, None) == pkg.EINVAL and lib.mbn_ragged_resizer_set(r.h, None, 2, None) == pkg.EINVAL
    assert lib.mbn_ragged_resizer_set(None, items, 2, None) == pkg.EINVAL
    assert launch(d_out.ptr + 8, d_src.ptr) == pkg.EINVAL
    # the mbn_alloc bounds rule, then NULL pointers
    r.set(good)
    assert launch(d_out.ptr + 8, d_src.ptr + 1) == pkg.EINVAL              # src one byte short of the largest offset + size
    assert "resize_ragged_u8 src" in ctx.last_error()
    assert launch(d_out.ptr + 8 + 8 + 1, d_src.ptr) == pkg.EINVAL          # out one byte short
    assert "resize_ragged_u8 out" in ctx.last_error()
    assert launch(None, d_src.ptr) == pkg.EINVAL and launch(d_out.ptr, None) == pkg.EINVAL
    assert lib.mbn_resize_ragged_u8(None, d_out.ptr, d_src.ptr, None) == pkg.EINVAL
    ctx.sync()
    assert (d_out.download((8 + out_bytes + 8,), np.uint8) == 0xAB).all(), "a refused call wrote to `out`"
    # a good launch at an interior pointer: the guard bytes on both sides stay
    assert launch(d_out.ptr + 8, d_src.ptr) == pkg.OK
    ctx.sync()
    raw = d_out.download((8 + out_bytes + 8,), np.uint8)
    assert (raw[:8] == 0xAB).all() and (raw[8 + out_bytes:] == 0xAB).all(), "a byte outside `out` was written"
    got = raw[8:8 + out_bytes].reshape(2, oh, ow, 3)
    assert np.array_equal(got[0], resize_ref.resize(a, oh, ow)) and np.array_equal(got[1], resize_ref.resize(b, oh, ow))
    r.close()
    h = C.c_void_p()
    mk = lambda *args: lib.mbn_ragged_resizer_create(ctx.h, *args, C.byref(h))
    assert mk(0, 32, 32) == pkg.EINVAL and mk(4, 0, 32) == pkg.EINVAL and mk(4, 32, 4097) == pkg.EUNSUPPORTED and mk(65536, 32, 32) == pkg.EUNSUPPORTED
    assert not h.value and lib.mbn_ragged_resizer_create(ctx.h, 4, 32, 32, None) == pkg.EINVAL
    assert lib.mbn_ragged_resizer_destroy(None) == pkg.OK
    d_src.free()
    d_out.free()


def test_set_again_and_lifetime(pkg, ctx):
    oh, ow = 32, 64
    a, b, c = _image((33, 47, 3), 1), _image((50, 20, 3), 2), _image((7, 90, 3), 3)
    offs, size = _layout([a, b, c], first=0, gaps=(1,))
    d_src, d_out = ctx.to_device(_source([a, b, c], offs, size)), ctx.alloc(3 * oh * ow * 3)
    box = (3.5, 2.25, 40.0, 30.75)
    r = pkg.RaggedResizer(ctx, 3, oh, ow)
    r.set([(offs[0], 33, 47, box)])
    r.run(d_out.ptr, d_src.ptr)
    r.set([(offs[2], 7, 90, None), (offs[1], 50, 20, None), (offs[0], 33, 47, None)])      # waits for the launch above, then overwrites the descriptors
    r.run(d_out.ptr, d_src.ptr)
    ctx.sync()
    got = d_out.download((3, oh, ow, 3), np.uint8)
    for i, img in enumerate((c, b, a)):
        assert np.array_equal(got[i], resize_ref.resize(img, oh, ow)), i
    r.set([(offs[0], 33, 47, box)])
    r.run(d_out.ptr, d_src.ptr)
    ctx.sync()
    assert np.array_equal(d_out.download((1, oh, ow, 3), np.uint8)[0], resize_ref.resize(a, oh, ow, box))
    r.close()
    r.close()                                     # idempotent on the Python side
    d_src.free()
    d_out.free()
    other = pkg.Context(0)                        # a context shut down with a handle alive: the handle goes with it
    live = pkg.RaggedResizer(other, 2, 64, 96)
    d_in, d_o = other.to_device(a), other.alloc(64 * 96 * 3)
    live.set([(0, 33, 47, None)])
    live.run(d_o.ptr, d_in.ptr)
    assert other.lib.mbn_shutdown(other.h) == pkg.OK
    other.h = None
    live.h = None


def test_capture_in_a_graph(pkg, ctx):
    """the launch makes no blocking call: legal between mbn_graph_begin and mbn_graph_end, one kernel node; replayed after another set it does nothing"""
    oh = ow = 32
    a, b = _image((37, 53, 3), 11), _image((64, 40, 3), 12)
    offs, size = _layout([a, b], first=1, gaps=(0,))
    d_src, d_out = ctx.to_device(_source([a, b], offs, size)), ctx.to_device(np.zeros(2 * oh * ow * 3, np.uint8))
    r = pkg.RaggedResizer(ctx, 2, oh, ow)
    items = [(offs[0], 37, 53, None), (offs[1], 64, 40, None)]
    r.set(items)
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_resize_ragged_u8(r.h, d_out.ptr, d_src.ptr, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert not d_out.download((2 * oh * ow * 3,), np.uint8).any(), "the captured call ran"
    want = np.stack([resize_ref.resize(a, oh, ow), resize_ref.resize(b, oh, ow)])
    for _ in range(2):
        assert ctx.lib.mbn_memset(ctx.h, d_out.ptr, 0, 2 * oh * ow * 3) == pkg.OK
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        ctx.sync()
        assert np.array_equal(d_out.download((2, oh, ow, 3), np.uint8), want)
    r.set(items[:1])                              # the captured launch belonged to the set before this one
    assert ctx.lib.mbn_memset(ctx.h, d_out.ptr, 0, 2 * oh * ow * 3) == pkg.OK
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert not d_out.download((2 * oh * ow * 3,), np.uint8).any(), "a replay after another set wrote"
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    d_src.free()
    d_out.free()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "i8"])
def test_net_resize_inputs(pkg, ctx, tmp_path, dtype):
    n, classes = 3, 40
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=0.25, classes=classes, seed=7, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(64, 96), lib=pkg.load())
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_dtype({"f32": pkg.DT_F32, "bf16": pkg.DT_BF16, "i8": pkg.DT_I8}[dtype])
    net.set_input_u8(True)
    images = [_image(s + (3,), 20 + i) for i, s in enumerate([(75, 100), (50, 80), (130, 64)])]
    offs, size = _layout(images, first=1, gaps=(2,), order=(2, 0, 1))
    d_src = ctx.to_device(_source(images, offs, size))
    d_a, d_b = ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)
    staging = []
    for fit, frac in ((pkg.FIT_CROP, 0.875), (pkg.FIT_STRETCH, 0.5)):           # the fraction is ignored by STRETCH
        want_u8 = np.stack([resize_ref.resize(img, 64, 96, resize_ref.fit_box(img.shape[0], img.shape[1], 64, 96, fit, 1.0 if fit == pkg.FIT_STRETCH else frac))
                            for img in images])
        p = net.resize_inputs(d_src.ptr, offs, [i.shape[0] for i in images], [i.shape[1] for i in images], fit, frac)
        staging.append(p)
        net.forward(p, d_a.ptr, n)
        ctx.sync()
        got_u8 = np.empty((n, 64, 96, 3), np.uint8)
        assert ctx.lib.mbn_download(ctx.h, got_u8.ctypes.data, p, got_u8.nbytes) == pkg.OK
        assert np.array_equal(got_u8, want_u8), "%s: the staged images differ from resize_ref" % dtype
        d_ref = ctx.to_device(want_u8)
        net.forward(d_ref.ptr, d_b.ptr, n)
        ctx.sync()
        a, b = d_a.download((n, classes), np.uint32), d_b.download((n, classes), np.uint32)
        assert np.array_equal(a, b), "%s: logits differ from a forward on resize_ref's bytes" % dtype
        assert np.isfinite(a.view(np.float32)).all() and a.view(np.float32).std() > 0
        d_ref.free()
    assert staging[0] == staging[1], "the staging buffer was reallocated"
    assert net.resize_input(d_src.ptr + offs[0], 1, 75, 100) == staging[0], "resize_input and resize_inputs share the staging buffer"
    i64, i32 = (C.c_int64 * 1)(0), (C.c_int32 * 1)(75)
    assert ctx.lib.mbn_net_resize_inputs(net.h, None, i64, i32, i32, 1, pkg.FIT_CROP, 1.0, None) == pkg.EINVAL
    with pytest.raises(pkg.MbnError):
        net.resize_inputs(d_src.ptr, [0] * (n + 1), [75] * (n + 1), [100] * (n + 1))           # beyond max_batch
    with pytest.raises(pkg.MbnError):
        net.resize_inputs(d_src.ptr, [0], [75], [100], pkg.FIT_CROP, 0.0)
    net.destroy()
    hw.free()
    for buf in (d_src, d_a, d_b):
        buf.free()


def test_c_host_several_ppm(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    files = []
    for i, (h, w) in enumerate([(75, 100), (50, 80), (130, 64)]):
        src = _image((h, w, 3), 40 + i)
        files.append(str(tmp_path / ("img%d.ppm" % i)))
        assert pkg.load().mbn_write_ppm(files[-1].encode(), src.ctypes.data, w, h) == 0
    common = [exe, "--synthetic", "1", "--alpha", "0.25", "--res", "64x96"]
    single = []
    for f in files:
        r = subprocess.run(common + ["--ppm", f], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "top-1 of image" not in r.stdout
        single.append(int(re.search(r"^top-5: (\d+) ", r.stdout, re.M).group(1)))
    args = common + ["--batch", "3"]
    for f in files:
        args += ["--ppm", f]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "warning" not in r.stderr, r.stderr
    tops = re.findall(r"^top-1 of image (\d+) \((.*)\): (\d+) \(", r.stdout, re.M)
    assert [(int(i), f) for i, f, _ in tops] == list(enumerate(files)), r.stdout
    assert [int(c) for _, _, c in tops] == single, (tops, single)
    r = subprocess.run(common + ["--batch", "2"] + args[-6:], capture_output=True, text=True, timeout=300)      # more files than the batch holds
    assert r.returncode == 2 and "--batch 3" in r.stderr
