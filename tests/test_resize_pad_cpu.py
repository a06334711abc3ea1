"""The letterbox fit (MBN_FIT_PAD) without a GPU: mbn_fit_pad against the rectangles Pillow itself pasted into (tests/golden/resize_pillow_pad.npz)
and against a restatement of the rule with Python's round; the rule + tests/resize_filters_ref.py against Pillow's canvases; the new plans
(mbn_resize_pad_table_plan_filter, mbn_resize_pad_ragged_plan_filter, _batch_filter) field for field against the existing plans of
(H, W) -> (ih, iw), and their tile windows against resize_ref's tables; the structs that must not move. Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import resize_filters_ref as R
import resize_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FILL_ROWS = 32
RAGGED_FILTERS = (R.NEAREST, R.BOX, R.BILINEAR, R.BICUBIC)
_FIXTURE = {}


def fixture():
    """tests/golden/resize_pillow_pad.npz, read once: [(name, source, (oh, ow), rect (x, y, iw, ih), {filter: canvas}, black canvas)], the fill"""
    if not _FIXTURE:
        z = np.load(os.path.join(HERE, "golden", "resize_pillow_pad.npz"))
        _FIXTURE["fill"] = tuple(int(v) for v in z["fill"])
        _FIXTURE["cases"] = [(n, z[n + "_in"], tuple(int(v) for v in z[n + "_canvas"]), tuple(int(v) for v in z[n + "_rect"]),
                              {f: z[n + "_" + R.NAMES[f]] for f in R.FILTERS}, z[n + "_black"]) for n in (str(s) for s in z["names"])]
    return _FIXTURE["cases"], _FIXTURE["fill"]


def rule(H, W, oh, ow):
    """PIL.ImageOps.contain + pad, centering (0.5, 0.5), restated with Python's own round: (x, y, iw, ih), or None where Pillow raises"""
    im_ratio, dest_ratio = W / H, ow / oh
    iw, ih = ow, oh
    if im_ratio != dest_ratio:
        if im_ratio > dest_ratio:
            ih = round(H / W * ow)
        else:
            iw = round(W / H * oh)
    if iw < 1 or ih < 1:
        return None
    if (iw, ih) == (ow, oh):
        return 0, 0, iw, ih
    if iw != ow:
        return round((ow - iw) * 0.5), 0, iw, ih
    return 0, round((oh - ih) * 0.5), iw, ih


def canvas_ref(f, img, oh, ow, fill):
    """the normative statement: a canvas of `fill`, the whole image resized into rule()'s rectangle"""
    x, y, iw, ih = rule(img.shape[0], img.shape[1], oh, ow)
    out = np.empty((oh, ow, 3), np.uint8)
    out[:] = np.array(fill, np.uint8)
    out[y:y + ih, x:x + iw] = R.resize(f, img, ih, iw)
    return out


def test_fixture_is_the_issues_eleven_cases():
    cases, fill = fixture()
    assert fill == (128, 7, 255)
    assert [(c[1].shape[0], c[1].shape[1]) + c[2] for c in cases] == [
        (45, 60, 28, 28), (60, 45, 28, 28), (37, 50, 32, 48), (50, 37, 32, 48), (31, 97, 64, 96), (97, 31, 64, 96), (64, 96, 64, 96), (128, 192, 64, 96),
        (33, 100, 32, 32), (100, 3, 32, 32), (7, 5, 32, 64)]
    by = {c[0]: c[3] for c in cases}
    assert by["33x100_to_32x32"] == (0, 10, 32, 11) and by["97x31_to_64x96"] == (38, 0, 20, 64) and by["100x3_to_32x32"] == (16, 0, 1, 32)


def test_fit_pad_gives_pillows_rectangles(pkg):
    for name, img, (oh, ow), rect, _, _ in fixture()[0]:
        assert pkg.fit_pad(img.shape[0], img.shape[1], oh, ow) == rect == rule(img.shape[0], img.shape[1], oh, ow), name


@pytest.mark.parametrize("f", R.FILTERS, ids=[R.NAMES[f] for f in R.FILTERS])
def test_rule_and_reference_resize_give_pillows_canvases(f):
    cases, fill = fixture()
    for name, img, (oh, ow), _, canvases, black in cases:
        assert np.array_equal(canvas_ref(f, img, oh, ow, fill), canvases[f]), name
        if f == R.BILINEAR:
            assert np.array_equal(canvas_ref(f, img, oh, ow, (0, 0, 0)), black), name


def test_fit_pad_random_sweep(pkg):
    rng = np.random.default_rng(20261020)
    lib = pkg.host_lib()
    rect = (C.c_int32 * 4)()
    n_ok = n_bad = n_half = 0
    for k in range(4000):
        src, dst = (64, 700, 8192)[k % 3], (48, 300, 4096)[k % 3]
        H, W, oh, ow = [int(rng.integers(1, src + 1)) for _ in range(2)] + [int(rng.integers(1, dst + 1)) for _ in range(2)]
        want = rule(H, W, oh, ow)
        rc = lib.mbn_fit_pad(H, W, oh, ow, rect)
        if want is None:
            assert rc == pkg.EINVAL, (H, W, oh, ow)
            n_bad += 1
            continue
        assert rc == pkg.OK and tuple(rect[:]) == want, (H, W, oh, ow, tuple(rect[:]), want)
        x, y, iw, ih = want
        assert 0 <= x and x + iw <= ow and 0 <= y and y + ih <= oh and (x == 0 or y == 0)
        n_half += (ow - iw) % 2 + (oh - ih) % 2
        n_ok += 1
    assert n_ok > 3000 and n_bad > 0 and n_half > 500          # odd borders, where half to even decides, are common in the sweep


def test_fit_pad_refusals_and_fit_box(pkg):
    lib = pkg.host_lib()
    rect = (C.c_int32 * 4)()
    assert lib.mbn_fit_pad(100, 3, 32, 32, rect) == pkg.OK and tuple(rect[:]) == (16, 0, 1, 32)
    assert lib.mbn_fit_pad(8192, 1, 32, 32, rect) == pkg.EINVAL and lib.mbn_fit_pad(1, 8192, 32, 32, rect) == pkg.EINVAL      # Pillow raises
    for bad in ((0, 5, 32, 32), (5, 0, 32, 32), (5, 5, 0, 32), (5, 5, 32, 0), (-1, 5, 32, 32)):
        assert lib.mbn_fit_pad(*bad, rect) == pkg.EINVAL, bad
    assert lib.mbn_fit_pad(5, 5, 32, 32, None) == pkg.EINVAL
    with pytest.raises(pkg.MbnError):
        pkg.fit_pad(8192, 1, 32, 32)
    # the box of the fit is the whole image, whatever the fraction; every other answer of mbn_fit_box stays
    assert pkg.FIT_PAD == 2
    for frac in (1.0, 0.5, 0.0):
        assert list(pkg.fit_box(375, 500, 224, 224, pkg.FIT_PAD, frac)) == [0.0, 0.0, 500.0, 375.0]
    assert list(pkg.fit_box(375, 500, 224, 224, pkg.FIT_STRETCH, 1.0)) == [0.0, 0.0, 500.0, 375.0]
    assert list(pkg.fit_box(480, 640, 224, 224, pkg.FIT_CROP, 1.0)) == [80.0, 0.0, 560.0, 480.0]
    box = (C.c_float * 4)()
    assert lib.mbn_fit_box(375, 500, 224, 224, 7, 1.0, box) == pkg.EINVAL and lib.mbn_fit_box(375, 500, 224, 224, 3, 1.0, box) == pkg.EINVAL
    assert lib.mbn_fit_box(375, 500, 224, 224, pkg.FIT_PAD, 1.0, None) == pkg.EINVAL


def _border(rect, oh, ow):
    x, y, iw, ih = rect
    rows = oh if iw < ow else oh - ih
    return rows, -(-rows // FILL_ROWS)


def _fields(s):
    return [getattr(s, n) if not isinstance(getattr(s, n), C.Array) else list(getattr(s, n)) for n, _ in s._fields_]


# the fixture's geometries, then steeper and larger ones: 67 taps down a one-column inner image (beyond bicubic's envelope), flatter tiles (1056 rows -> 64
# has toh 31 under bilinear and 24 under bicubic), a one-row inner image (toh = 1 under every filter), a 32-column inner image in a wide canvas
GEOMETRIES = [(c[1].shape[0], c[1].shape[1]) + c[2] for c in fixture()[0]] + [
    (1290, 17, 40, 72), (375, 500, 224, 224), (500, 375, 224, 224), (480, 640, 224, 224), (1056, 96, 64, 96), (2, 200, 64, 96), (100, 2, 64, 96),
    (300, 100, 96, 200), (1, 1, 5, 7)]


@pytest.mark.parametrize("f", R.FILTERS, ids=[R.NAMES[f] for f in R.FILTERS])
def test_table_plan_is_the_plan_of_the_inner_image(pkg, f):
    for H, W, oh, ow in GEOMETRIES:
        rect = rule(H, W, oh, ow)
        x, y, iw, ih = rect
        want = pkg.host_lib().mbn_resize_table_plan_filter(f, H, W, None, ih, iw, C.byref(pkg.ResizePlan()))
        if want != pkg.OK:
            with pytest.raises(pkg.MbnError) as e:
                pkg.resize_pad_table_plan(H, W, oh, ow, filter=f)
            assert e.value.code == want
            continue
        p = pkg.resize_pad_table_plan(H, W, oh, ow, filter=f)
        assert _fields(p.plan) == _fields(pkg.resize_table_plan(H, W, ih, iw, filter=f)), (H, W, oh, ow)
        assert (p.x, p.y, p.iw, p.ih) == rect and (p.fill_rows, p.fill_wgs) == _border(rect, oh, ow)
        assert p.plan.tow == (32 if iw <= 32 else 64)
    lib, p = pkg.host_lib(), pkg.ResizePadPlan()
    assert lib.mbn_resize_pad_table_plan_filter(f, 8192, 1, 32, 32, C.byref(p)) == pkg.EINVAL              # an empty inner side
    assert lib.mbn_resize_pad_table_plan_filter(f, 37, 53, 32, 32, None) == pkg.EINVAL
    assert lib.mbn_resize_pad_table_plan_filter(6, 37, 53, 32, 32, C.byref(p)) == pkg.EINVAL
    assert lib.mbn_resize_pad_table_plan_filter(f, 37, 53, 4097, 64, C.byref(p)) == pkg.EUNSUPPORTED         # the canvas
    assert lib.mbn_resize_pad_table_plan_filter(f, 8193, 8193, 64, 64, C.byref(p)) == pkg.EUNSUPPORTED       # the envelope of (H, W) -> (ih, iw)


def test_border_rows_cover_the_canvas_outside_the_rectangle():
    """the row map of MBN_RESIZE_FILL_ROW, restated: with the rectangle's rows x columns, the border rows' runs tile the canvas exactly once"""
    for H, W, oh, ow in GEOMETRIES:
        x, y, iw, ih = rule(H, W, oh, ow)
        rows, _ = _border((x, y, iw, ih), oh, ow)
        hits = np.zeros((oh, ow), np.int32)
        hits[y:y + ih, x:x + iw] += 1
        for k in range(rows):
            r = k if iw < ow or k < y else k + ih
            if r < y or r >= y + ih:
                hits[r, :] += 1
            else:
                hits[r, :x] += 1
                hits[r, x + iw:] += 1
        assert (hits == 1).all(), (H, W, oh, ow)


@pytest.mark.parametrize("f", RAGGED_FILTERS, ids=[R.NAMES[f] for f in RAGGED_FILTERS])
def test_ragged_plan_is_the_plan_of_each_inner_image(pkg, f):
    for oh, ow in ((64, 96), (40, 72), (32, 32), (224, 224)):
        geos = [g for g in GEOMETRIES if g[2:] == (oh, ow)] + [(97, 31, oh, ow), (31, 97, oh, ow), (oh, ow, oh, ow), (100, 3, oh, ow)]
        status = [pkg.host_lib().mbn_resize_ragged_plan_filter(f, pkg.resize_items([(0, H, W, None)]), rule(H, W, oh, ow)[3], rule(H, W, oh, ow)[2],
                                                               C.byref(pkg.ResizeDesc())) for H, W, _, _ in geos]
        for (H, W, _, _), rc in zip(geos, status):               # an image outside the envelope of (H, W) -> (ih, iw) is refused with that status
            assert pkg.host_lib().mbn_resize_pad_ragged_plan_filter(f, pkg.resize_items([(0, H, W, None)]), oh, ow, C.byref(pkg.ResizePadDesc())) == rc
        geos = [g for g, rc in zip(geos, status) if rc == pkg.OK]
        items = [(7 * i, H, W, None) for i, (H, W, _, _) in enumerate(geos)]
        desc, wgs, lds, span = pkg.resize_pad_ragged_plan(items, oh, ow, filter=f)
        wg0 = 0
        for d, (off, H, W, _) in zip(desc, items):
            rect = rule(H, W, oh, ow)
            x, y, iw, ih = rect
            plain, _, plain_lds, _ = pkg.resize_ragged_plan([(off, H, W, None)], ih, iw, filter=f)
            want = _fields(plain[0])
            assert plain[0].wg0 == 0
            got = _fields(d.img)
            assert got[:8] + got[9:] == want[:8] + want[9:], (H, W, oh, ow)           # every field but wg0 (index 8), which is the pad launch's
            assert d.img.wg0 == wg0
            tow = 32 if iw <= 32 else 64
            assert (d.x, d.y, d.iw, d.ih) == rect and (d.tow, d.tiles_x) == (tow, -(-iw // tow))
            assert (d.fill_rows, d.fill_wgs) == _border(rect, oh, ow)
            wg0 += d.tiles_x * d.img.tiles_y + d.fill_wgs
            assert d.img.lds_bytes == plain_lds <= 60 * 1024
            if f == R.BILINEAR:                                                       # the tile windows: resize_ref's tables, as for the plain plan
                for in_size, out_size, tile in ((W, iw, tow), (H, ih, d.img.toh)):
                    first, count, _ = resize_ref.taps(in_size, 0.0, float(in_size), out_size)
                    for o in range(0, out_size, tile):
                        last = min(o + tile, out_size) - 1
                        assert pkg.resize_window(in_size, 0.0, float(in_size), out_size, o, last) == (int(first[o]), int(first[last] + count[last]))
        assert wgs == wg0 and lds == max(d.img.lds_bytes for d in desc)
        assert span == max(off + H * W * 3 for off, H, W, _ in items)
        if (oh, ow) == (64, 96):
            toh = {(d.img.rows, d.img.cols): d.img.toh for d in desc}
            assert toh[(2, 200)] == 1 and toh[(64, 96)] == 32
            if f in (R.BILINEAR, R.BICUBIC):
                assert toh[(1056, 96)] == {R.BILINEAR: 31, R.BICUBIC: 24}[f]


def test_ragged_plan_refusals(pkg):
    lib, d = pkg.host_lib(), pkg.ResizePadDesc()
    plan = lambda f, off, rows, cols, box, oh=32, ow=32: lib.mbn_resize_pad_ragged_plan_filter(f, pkg.resize_items([(off, rows, cols, box)]), oh, ow, C.byref(d))
    assert plan(R.BILINEAR, 0, 37, 53, None) == pkg.OK and (d.x, d.y, d.iw, d.ih) == (0, 5, 32, 22)
    assert plan(R.BILINEAR, 0, 37, 53, (0.0, 0.0, 53.0, 37.0)) == pkg.OK
    for box in ((1.0, 0.0, 53.0, 37.0), (0.0, 0.0, 52.5, 37.0), (0.0, 0.0, 53.0, 36.0), (0.0, float("nan"), 53.0, 37.0)):      # a pad of a box is not built
        assert plan(R.BILINEAR, 0, 37, 53, box) == pkg.EINVAL, box
    assert plan(R.BILINEAR, -1, 37, 53, None) == pkg.EINVAL and plan(R.BILINEAR, 0, 8192, 1, None) == pkg.EINVAL
    assert plan(R.HAMMING, 0, 37, 53, None) == pkg.EUNSUPPORTED and plan(R.LANCZOS, 0, 37, 53, None) == pkg.EUNSUPPORTED
    assert plan(6, 0, 37, 53, None) == pkg.EINVAL
    assert plan(R.BILINEAR, 0, 1060, 1060, None) == pkg.EUNSUPPORTED and plan(R.BILINEAR, 0, 1056, 1056, None) == pkg.OK      # 33.1x: 69 taps; 33x: 67
    assert plan(R.BILINEAR, 0, 37, 53, None, 4097, 64) == pkg.EUNSUPPORTED
    with pytest.raises(pkg.MbnError) as e:
        pkg.resize_pad_ragged_plan([(0, 37, 53, None), (0, 37, 53, (1.0, 0.0, 53.0, 37.0))], 32, 32)
    assert e.value.code == pkg.EINVAL


def test_structs_keep_their_layout(pkg):
    assert C.sizeof(pkg.ResizeDesc) == 64 and C.sizeof(pkg.ResizeItem) == 32 and C.sizeof(pkg.ResizePlan) == 40
    assert C.sizeof(pkg.ResizePadDesc) == 96 and pkg.ResizePadDesc.img.offset == 0 and pkg.ResizePadDesc.x.offset == 64
    assert C.sizeof(pkg.ResizePadPlan) == 64 and pkg.ResizePadPlan.x.offset == 40
    assert [n for n, _ in pkg.ResizeDesc._fields_] == ["src_offset", "rows", "cols", "box", "kx", "ky", "toh", "tiles_y", "wg0", "seg_stride", "tmp_off",
                                                       "lds_bytes"]
    # the existing plans answer as before for an output that is a letterbox's inner size
    d, _, _, _ = pkg.resize_ragged_plan([(0, 375, 500, None)], 168, 224)
    assert (d[0].kx, d[0].ky, d[0].toh, d[0].tiles_y) == (7, 7, 32, 6)


def test_symbols_declared(pkg):
    names = pkg.declared_symbols()
    for s in ("mbn_fit_pad", "mbn_resizer_create_pad", "mbn_ragged_resizer_create_pad", "mbn_net_set_pad_color", "mbn_net_get_pad_color"):
        assert s in names, s
    host = pkg.host_lib()
    for s in ("mbn_fit_pad", "mbn_resize_pad_table_plan_filter", "mbn_resize_pad_ragged_plan_filter", "mbn_resize_pad_ragged_plan_batch_filter"):
        assert hasattr(host, s), s
