"""The letterbox fit (MBN_FIT_PAD) on the GPU. The uniform handle (mbn_resizer_create_pad) against Pillow's recorded canvases
(tests/golden/resize_pillow_pad.npz: ImageOps.pad under all six filters) with a sentinel in `out` and guard bytes around it, at batch 3 and through
pointers one byte off alignment; the ragged handle (mbn_ragged_resizer_create_pad) in one launch of differently shaped images against the per-image
reference and the uniform handle, set again, set with another batch size and replayed from a graph after another set; the net runner's FIT_PAD and pad
colour; the C host's --fit pad. Every comparison is exact equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resize_filters_ref as R
from test_resize_pad_cpu import RAGGED_FILTERS, canvas_ref, fixture, rule

pytestmark = pytest.mark.gpu

GUARD = 16
SENTINEL = 0xAB
N_CASES = 11


def _uniform(pkg, ctx, f, imgs, oh, ow, fill, in_off=0, out_off=0):
    """mbn_resize_u8 of a pad handle on imgs [n][H][W][3]: `in` at byte in_off of its buffer, `out` at GUARD + out_off of a buffer of SENTINEL with
    GUARD more bytes behind: (the canvases, the bytes around them)"""
    n, H, W, _ = imgs.shape
    nb = n * oh * ow * 3
    d_in = ctx.to_device(np.concatenate([np.zeros(in_off, np.uint8), imgs.ravel()]))
    d_out = ctx.to_device(np.full(GUARD + out_off + nb + GUARD, SENTINEL, np.uint8))
    r = pkg.Resizer(ctx, H, W, oh, ow, filter=f, pad=fill)
    r.run(d_out.ptr + GUARD + out_off, d_in.ptr + in_off, n)
    ctx.sync()
    raw = d_out.download((GUARD + out_off + nb + GUARD,), np.uint8)
    r.close()
    d_in.free()
    d_out.free()
    lo = GUARD + out_off
    return raw[lo:lo + nb].reshape(n, oh, ow, 3), np.concatenate([raw[:lo], raw[lo + nb:]])


@pytest.mark.parametrize("index", range(N_CASES))
def test_uniform_equals_pillow(pkg, ctx, index):
    cases, fill = fixture()
    assert len(cases) == N_CASES and SENTINEL not in fill
    name, img, (oh, ow), rect, canvases, black = cases[index]
    batch = np.stack([img, img[:, ::-1], 255 - img])
    for f in R.FILTERS:
        got, guard = _uniform(pkg, ctx, f, img[None], oh, ow, fill)
        bad = int((got[0] != canvases[f]).sum())
        assert bad == 0, "%s under %s: %d of %d bytes differ from Pillow's" % (name, R.NAMES[f], bad, got[0].size)
        assert (guard == SENTINEL).all(), "%s under %s: bytes around `out` were written" % (name, R.NAMES[f])
        # batch 3 (the image, its mirror, its complement), `in` and `out` one byte off alignment
        got, guard = _uniform(pkg, ctx, f, batch, oh, ow, fill, in_off=1, out_off=1)
        assert (guard == SENTINEL).all(), "%s under %s: bytes around an unaligned `out` were written" % (name, R.NAMES[f])
        assert np.array_equal(got[0], canvases[f]), "%s under %s: an unaligned call differs" % (name, R.NAMES[f])
        for i in (1, 2):
            assert np.array_equal(got[i], canvas_ref(f, batch[i], oh, ow, fill)), "%s under %s: image %d of the batch" % (name, R.NAMES[f], i)
    got, _ = _uniform(pkg, ctx, R.BILINEAR, img[None], oh, ow, (0, 0, 0))
    assert np.array_equal(got[0], black), "%s: the default colour's canvas" % name


def test_uniform_same_aspect_equals_the_stretch_resizer(pkg, ctx):
    cases, fill = fixture()
    _, img, (oh, ow), rect, _, _ = [c for c in cases if c[0] == "128x192_to_64x96"][0]
    assert rect == (0, 0, ow, oh)
    for f in R.FILTERS:
        pad, _ = _uniform(pkg, ctx, f, img[None], oh, ow, fill)
        d_in, d_out = ctx.to_device(img), ctx.alloc(oh * ow * 3)
        r = pkg.Resizer(ctx, img.shape[0], img.shape[1], oh, ow, filter=f)
        r.run(d_out.ptr, d_in.ptr, 1)
        ctx.sync()
        assert np.array_equal(pad[0], d_out.download((oh, ow, 3), np.uint8)), R.NAMES[f]
        r.close()
        d_in.free()
        d_out.free()


def test_uniform_refusals_bounds_and_capture(pkg, ctx):
    lib, h = ctx.lib, C.c_void_p()
    fill = (C.c_uint8 * 3)(1, 2, 3)
    mk = lambda f, *a: lib.mbn_resizer_create_pad(ctx.h, f, *a, C.byref(h))
    assert mk(R.BILINEAR, 37, 53, 32, 32, None) == pkg.EINVAL and mk(6, 37, 53, 32, 32, fill) == pkg.EINVAL and not h.value
    assert mk(R.BILINEAR, 8192, 1, 32, 32, fill) == pkg.EINVAL                       # an empty inner side: Pillow raises
    assert mk(R.BILINEAR, 0, 53, 32, 32, fill) == pkg.EINVAL and mk(R.BILINEAR, 37, 53, 0, 32, fill) == pkg.EINVAL
    assert mk(R.BILINEAR, 1060, 1060, 32, 32, fill) == pkg.EUNSUPPORTED              # the envelope of (H, W) -> (ih, iw): 69 taps
    assert mk(R.BILINEAR, 37, 53, 4097, 64, fill) == pkg.EUNSUPPORTED and not h.value
    assert lib.mbn_resizer_create_pad(None, R.BILINEAR, 37, 53, 32, 32, fill, C.byref(h)) == pkg.EINVAL
    # the mbn_alloc bounds rule is the canvas's, and a captured call, border included, runs on every replay
    img = np.random.default_rng(7).integers(0, 256, (2, 97, 31, 3), dtype=np.uint8)
    oh, ow, nb = 64, 96, 2 * 64 * 96 * 3
    d_in, d_out = ctx.to_device(img), ctx.to_device(np.zeros(nb, np.uint8))
    r = pkg.Resizer(ctx, 97, 31, oh, ow, pad=(9, 8, 7))
    assert lib.mbn_resize_u8(r.h, d_out.ptr + 1, d_in.ptr, 2, None) == pkg.EINVAL and "resize_u8 out" in ctx.last_error()
    assert lib.mbn_resize_u8(r.h, d_out.ptr, d_in.ptr + 1, 2, None) == pkg.EINVAL and "resize_u8 in" in ctx.last_error()
    g = C.c_void_p()
    assert lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = lib.mbn_resize_u8(r.h, d_out.ptr, d_in.ptr, 2, None)
    assert lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert not d_out.download((nb,), np.uint8).any(), "the captured call ran, or a refused one wrote"
    want = np.stack([canvas_ref(R.BILINEAR, im, oh, ow, (9, 8, 7)) for im in img])
    for _ in range(2):
        assert lib.mbn_memset(ctx.h, d_out.ptr, 0, nb) == pkg.OK
        assert lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        ctx.sync()
        assert np.array_equal(d_out.download((2, oh, ow, 3), np.uint8), want)
    assert lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    d_in.free()
    d_out.free()


# ---- the ragged handle. Canvas 64 x 96 (two column tiles, two row tiles). In this order: borders left / right (x = 38), top / bottom with two column
# tiles, the canvas's own size (the identity), its aspect ratio, a one-pixel-wide inner image (iw = 1, x = round(47.5) = 48), a one-row inner image
# (ih = 1: the plan's toh = 1 under every filter), flatter tiles (1056 rows -> 64: 67 taps under bicubic), an odd border (x = round(24.5) = 24)
OH, OW = 64, 96
SHAPES = [(97, 31), (31, 97), (64, 96), (128, 192), (100, 2), (2, 200), (1056, 96), (50, 37)]
_RAGGED = {}


def _ragged_inputs():
    """the batch's images, laid out from byte 1 with gaps that move the alignment, and the reference canvases per filter: made once"""
    if not _RAGGED:
        fill = fixture()[1]
        images = [np.random.default_rng(500 + i).integers(0, 256, s + (3,), dtype=np.uint8) for i, s in enumerate(SHAPES)]
        offs, cur = [], 1
        for k, img in enumerate(images):
            offs.append(cur)
            cur += img.size + (0, 3, 1, 2)[k % 4]
        src = np.zeros(cur, np.uint8)
        for img, off in zip(images, offs):
            src[off:off + img.size] = img.ravel()
        _RAGGED.update(images=images, offs=offs, src=src, fill=fill,
                       want={f: np.stack([canvas_ref(f, img, OH, OW, fill) for img in images]) for f in RAGGED_FILTERS})
    return _RAGGED


def _launch(pkg, ctx, r, d_src, n, order):
    """set the images `order` and launch once into a buffer of SENTINEL, `out` one byte off alignment: (the canvases, the bytes around them)"""
    z = _ragged_inputs()
    nb = n * OH * OW * 3
    d_out = ctx.to_device(np.full(GUARD + 1 + nb + GUARD, SENTINEL, np.uint8))
    r.set([(z["offs"][i], SHAPES[i][0], SHAPES[i][1], None) for i in order])
    r.run(d_out.ptr + GUARD + 1, d_src.ptr)
    ctx.sync()
    raw = d_out.download((GUARD + 1 + nb + GUARD,), np.uint8)
    d_out.free()
    return raw[GUARD + 1:GUARD + 1 + nb].reshape(n, OH, OW, 3), np.concatenate([raw[:GUARD + 1], raw[GUARD + 1 + nb:]])


@pytest.mark.parametrize("f", RAGGED_FILTERS, ids=[R.NAMES[f] for f in RAGGED_FILTERS])
def test_ragged_mixed_batch(pkg, ctx, f):
    z = _ragged_inputs()
    n = len(SHAPES)
    rects = [rule(h, w, OH, OW) for h, w in SHAPES]
    assert rects[0] == (38, 0, 20, 64) and rects[1] == (0, 16, 96, 31) and rects[2] == rects[3] == (0, 0, 96, 64)
    assert rects[4] == (48, 0, 1, 64) and rects[5] == (0, 32, 96, 1) and rects[7] == (24, 0, 47, 64)
    desc, _, _, _ = pkg.resize_pad_ragged_plan([(o, h, w, None) for o, (h, w) in zip(z["offs"], SHAPES)], OH, OW, filter=f)
    assert desc[5].img.toh == 1 and any(o % 2 == 1 for o in z["offs"]) and any(o % 4 == 2 for o in z["offs"])
    d_src = ctx.to_device(z["src"])
    r = pkg.RaggedResizer(ctx, n, OH, OW, filter=f, pad=z["fill"])
    got, guard = _launch(pkg, ctx, r, d_src, n, range(n))
    assert (guard == SENTINEL).all(), "bytes around `out` were written"
    for i in range(n):
        bad = int((got[i] != z["want"][f][i]).sum())
        assert bad == 0, "%s image %d (%dx%d): %d of %d bytes differ from the reference canvas" % (R.NAMES[f], i, SHAPES[i][0], SHAPES[i][1], bad, got[i].size)
        one, _ = _uniform(pkg, ctx, f, z["images"][i][None], OH, OW, z["fill"])
        assert np.array_equal(got[i], one[0]), "%s image %d: the uniform pad handle differs" % (R.NAMES[f], i)
    assert np.array_equal(got[2], z["images"][2]), "the identity is a byte copy"
    # a second set on the same handle, in another order; then a set of another batch size
    order = [5, 0, 7, 6, 1, 4, 3, 2]
    got, guard = _launch(pkg, ctx, r, d_src, n, order)
    assert (guard == SENTINEL).all() and np.array_equal(got, z["want"][f][order]), "%s: the second set" % R.NAMES[f]
    got, guard = _launch(pkg, ctx, r, d_src, 3, [6, 4, 1])
    assert (guard == SENTINEL).all() and np.array_equal(got, z["want"][f][[6, 4, 1]]), "%s: a set of three" % R.NAMES[f]
    r.close()
    d_src.free()


@pytest.mark.parametrize("f", (R.NEAREST, R.BILINEAR), ids=["nearest", "bilinear"])
def test_ragged_capture_in_a_graph(pkg, ctx, f):
    """one kernel node, border included; replayed after another set it does nothing"""
    z = _ragged_inputs()
    pick = [0, 1, 5]
    nb = len(pick) * OH * OW * 3
    d_src, d_out = ctx.to_device(z["src"]), ctx.to_device(np.zeros(nb, np.uint8))
    r = pkg.RaggedResizer(ctx, 4, OH, OW, filter=f, pad=z["fill"])
    items = [(z["offs"][i], SHAPES[i][0], SHAPES[i][1], None) for i in pick]
    r.set(items)
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_resize_ragged_u8(r.h, d_out.ptr, d_src.ptr, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert not d_out.download((nb,), np.uint8).any(), "the captured call ran"
    for _ in range(2):
        assert ctx.lib.mbn_memset(ctx.h, d_out.ptr, 0, nb) == pkg.OK
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        ctx.sync()
        assert np.array_equal(d_out.download((len(pick), OH, OW, 3), np.uint8), z["want"][f][pick])
    r.set(items[:2])                              # the captured launch belonged to the set before this one
    assert ctx.lib.mbn_memset(ctx.h, d_out.ptr, 0, nb) == pkg.OK
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert not d_out.download((nb,), np.uint8).any(), "a replay after another set wrote"
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    d_src.free()
    d_out.free()


def test_ragged_refusals(pkg, ctx):
    lib, h = ctx.lib, C.c_void_p()
    fill = (C.c_uint8 * 3)(1, 2, 3)
    mk = lambda f, *a: lib.mbn_ragged_resizer_create_pad(ctx.h, f, *a, C.byref(h))
    assert mk(R.HAMMING, 4, 32, 32, fill) == pkg.EUNSUPPORTED and mk(R.LANCZOS, 4, 32, 32, fill) == pkg.EUNSUPPORTED and not h.value
    assert mk(R.BILINEAR, 4, 32, 32, None) == pkg.EINVAL and mk(6, 4, 32, 32, fill) == pkg.EINVAL and mk(R.BILINEAR, 0, 32, 32, fill) == pkg.EINVAL
    assert mk(R.BILINEAR, 4, 32, 4097, fill) == pkg.EUNSUPPORTED and not h.value
    a = np.random.default_rng(3).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    d_src, d_out = ctx.to_device(a), ctx.to_device(np.full(2 * 32 * 32 * 3, SENTINEL, np.uint8))
    r = pkg.RaggedResizer(ctx, 2, 32, 32, pad=(1, 2, 3))
    launch = lambda: lib.mbn_resize_ragged_u8(r.h, d_out.ptr, d_src.ptr, None)
    assert launch() == pkg.EINVAL                                                    # no batch yet
    r.set([(0, 37, 53, None), (0, 37, 53, (0.0, 0.0, 53.0, 37.0))])
    for bad in ((1.0, 0.0, 53.0, 37.0), (0.0, 0.0, 53.0, 36.5), (0.0, 2.25, 40.0, 30.75)):      # a partial box: a pad of a box is not built
        with pytest.raises(pkg.MbnError) as e:
            r.set([(0, 37, 53, None), (0, 37, 53, bad)])
        assert e.value.code == pkg.EINVAL, bad
        assert launch() == pkg.EINVAL, "a failed set leaves the handle without a batch"
    with pytest.raises(pkg.MbnError) as e:
        r.set([(0, 8192, 1, None)])                                                  # an empty inner side
    assert e.value.code == pkg.EINVAL
    with pytest.raises(pkg.MbnError) as e:
        r.set([(0, 1060, 1060, None)])                                               # 69 taps
    assert e.value.code == pkg.EUNSUPPORTED
    ctx.sync()
    assert (d_out.download((2 * 32 * 32 * 3,), np.uint8) == SENTINEL).all(), "a refused call wrote to `out`"
    r.set([(0, 37, 53, None)])
    assert launch() == pkg.OK
    ctx.sync()
    raw = d_out.download((2, 32, 32, 3), np.uint8)
    assert np.array_equal(raw[0], canvas_ref(R.BILINEAR, a, 32, 32, (1, 2, 3))) and (raw[1] == SENTINEL).all()
    r.close()
    d_src.free()
    d_out.free()


def _net(pkg, ctx, tmp_path, batch, classes=40):
    path = str(tmp_path / ("w%d.h5" % classes))
    pkg.synthetic_h5(path, alpha=0.25, classes=classes, seed=7, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(64, 96), lib=pkg.load())
    return hw, pkg.Net(ctx, hw.plan, hw.blob.copy(), batch)


def _staged(pkg, ctx, p, n):
    got = np.empty((n, 64, 96, 3), np.uint8)
    assert ctx.lib.mbn_download(ctx.h, got.ctypes.data, p, got.nbytes) == pkg.OK
    return got


def test_net_fit_pad(pkg, ctx, tmp_path):
    n, classes = 3, 40
    hw, net = _net(pkg, ctx, tmp_path, n)
    net.set_input_u8(True)
    assert net.pad_color() == (0, 0, 0)
    images = [np.random.default_rng(20 + i).integers(0, 256, s + (3,), dtype=np.uint8) for i, s in enumerate([(75, 100), (50, 80), (130, 64)])]
    offs = [1, 1 + images[0].size + 2, 1 + images[0].size + 2 + images[1].size + 1]
    src = np.zeros(offs[2] + images[2].size, np.uint8)
    for img, off in zip(images, offs):
        src[off:off + img.size] = img.ravel()
    uniform = np.stack([images[0], images[0][::-1]])
    d_src, d_uni = ctx.to_device(src), ctx.to_device(uniform)
    d_a, d_b = ctx.alloc(n * classes * 4), ctx.alloc(n * classes * 4)

    def check(p, want_u8, what):
        k = len(want_u8)
        net.forward(p, d_a.ptr, k)
        ctx.sync()
        assert np.array_equal(_staged(pkg, ctx, p, k), want_u8), "%s: the staged canvases differ from the reference" % what
        d_ref = ctx.to_device(want_u8)
        net.forward(d_ref.ptr, d_b.ptr, k)
        ctx.sync()
        a, b = d_a.download((k, classes), np.uint32), d_b.download((k, classes), np.uint32)
        assert np.array_equal(a, b), "%s: logits differ from a forward on the reference canvases" % what
        assert np.isfinite(a.view(np.float32)).all() and a.view(np.float32).std() > 0
        d_ref.free()

    rows, cols = [i.shape[0] for i in images], [i.shape[1] for i in images]
    for colour in ((0, 0, 0), (128, 7, 255), (1, 2, 3)):                 # the colour takes effect on the next call, on both paths
        if colour != (0, 0, 0):
            net.set_pad_color(*colour)
            assert net.pad_color() == colour
        p = net.resize_inputs(d_src.ptr, offs, rows, cols, pkg.FIT_PAD, 0.25)            # the fraction is ignored
        check(p, np.stack([canvas_ref(R.BILINEAR, img, 64, 96, colour) for img in images]), "resize_inputs %r" % (colour,))
        p = net.resize_input(d_uni.ptr, 2, 75, 100, pkg.FIT_PAD, 0.0)
        check(p, np.stack([canvas_ref(R.BILINEAR, img, 64, 96, colour) for img in uniform]), "resize_input %r" % (colour,))
    # the other fits and the filter still rebuild the kept resizers
    net.set_resize_filter(pkg.FILTER_BICUBIC)
    p = net.resize_inputs(d_src.ptr, offs, rows, cols, pkg.FIT_PAD)
    check(p, np.stack([canvas_ref(R.BICUBIC, img, 64, 96, (1, 2, 3)) for img in images]), "bicubic")
    p = net.resize_inputs(d_src.ptr, offs, rows, cols, pkg.FIT_STRETCH)
    ctx.sync()
    assert np.array_equal(_staged(pkg, ctx, p, n), np.stack([R.resize(R.BICUBIC, img, 64, 96) for img in images]))
    p = net.resize_input(d_uni.ptr, 2, 75, 100, pkg.FIT_STRETCH)
    ctx.sync()
    assert np.array_equal(_staged(pkg, ctx, p, 2), R.resize(R.BICUBIC, uniform, 64, 96))
    assert ctx.lib.mbn_net_set_pad_color(net.h, 256, 0, 0) == pkg.EINVAL and ctx.lib.mbn_net_set_pad_color(net.h, 0, -1, 0) == pkg.EINVAL
    assert ctx.lib.mbn_net_set_pad_color(None, 0, 0, 0) == pkg.EINVAL and net.pad_color() == (1, 2, 3)
    with pytest.raises(pkg.MbnError):
        net.resize_input(d_uni.ptr, 1, 75, 100, 3)                       # no such fit
    net.destroy()
    hw.free()
    for b in (d_src, d_uni, d_a, d_b):
        b.free()


def test_c_host_fit_pad(pkg, ctx, tmp_path):
    """mobilenet --ppm F --fit pad --pad-color 128,128,128 prints the top-5 of the reference canvas; --segment adds the rectangle; several --ppm take the
    ragged letterbox; a bad colour is usage status 2"""
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    grey = (128, 128, 128)
    srcs = [np.random.default_rng(60 + i).integers(0, 256, s + (3,), dtype=np.uint8) for i, s in enumerate([(75, 60), (40, 100)])]
    odd, fit = [], []
    for i, src in enumerate(srcs):
        odd.append(str(tmp_path / ("odd%d.ppm" % i)))
        fit.append(str(tmp_path / ("fit%d.ppm" % i)))
        canvas = canvas_ref(R.BILINEAR, src, 64, 96, grey)
        assert pkg.load().mbn_write_ppm(odd[-1].encode(), src.ctypes.data, src.shape[1], src.shape[0]) == 0
        assert pkg.load().mbn_write_ppm(fit[-1].encode(), canvas.ctypes.data, 96, 64) == 0
    common = [exe, "--synthetic", "7", "--alpha", "0.25", "--res", "64x96"]
    pad = ["--fit", "pad", "--pad-color", "128,128,128"]
    out = {}
    for key, extra in (("pad", ["--ppm", odd[0], "--segment", str(tmp_path / "labels.pgm")] + pad), ("ref0", ["--ppm", fit[0]]), ("ref1", ["--ppm", fit[1]]),
                       ("two", ["--batch", "2", "--ppm", odd[0], "--ppm", odd[1]] + pad)):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "warning" not in r.stderr, r.stderr
        out[key] = r.stdout
    top5 = lambda s: re.search(r"^top-5:.*$", s, re.M).group(0)
    assert top5(out["pad"]) == top5(out["ref0"]), (top5(out["pad"]), top5(out["ref0"]))
    assert "(pad)" in out["pad"] and rule(75, 60, 64, 96) == (22, 0, 51, 64)
    assert re.search(r"^segment: image 0 is the 51 x 64 rectangle at \(22, 0\)", out["pad"], re.M), out["pad"]
    tops = [int(c) for c in re.findall(r"^top-1 of image \d+ \(.*\): (\d+) \(", out["two"], re.M)]
    assert tops == [int(re.search(r"^top-5: (\d+) ", out[k], re.M).group(1)) for k in ("ref0", "ref1")], out["two"]
    for bad in ("128,128", "128,128,256", "1,2,3,4", "red", "1,2,x"):
        r = subprocess.run(common + ["--ppm", odd[0], "--fit", "pad", "--pad-color", bad], capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "usage" in r.stderr, bad
    r = subprocess.run(common + ["--ppm", odd[0], "--fit", "letterbox"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "usage" in r.stderr
