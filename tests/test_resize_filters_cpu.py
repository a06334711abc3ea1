"""The resize front-end's filters without a GPU: tests/resize_filters_ref.py (the numpy statement of include/mbn.h, "resize front-end", for all six of
Pillow's filters) against Pillow's own bytes (tests/golden/resize_pillow_filters.npz, and live where Pillow is installed), and the host side of
libmbn_host.so (the _filter entry points: tables, NEAREST's index, windows, envelope, plans) against that reference as int32, exactly. Every
comparison is exact; nothing here has a tolerance."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import resize_filters_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "resize_pillow_filters.npz")
_cache = {}


def fixture_module():
    if "module" not in _cache:
        spec = importlib.util.spec_from_file_location("make_resize_filter_fixtures", os.path.join(HERE, "golden", "make_resize_filter_fixtures.py"))
        _cache["module"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_cache["module"])
    return _cache["module"]


def cases():
    """[(case, filter, image, box, Pillow's bytes)], loaded once"""
    if "cases" not in _cache:
        z = np.load(FIXTURE)
        _cache["cases"] = [(str(n), int(f), z[str(n) + "_in"], z[str(n) + "_rect"], z[str(n) + "_" + R.NAMES[int(f)]])
                           for n in z["names"] for f in z[str(n) + "_filters"]]
    return _cache["cases"]


N_CASES = 6 * 6 + 6 + 2      # six geometries under every filter, the steepest factor of each filter (bicubic twice), NEAREST's two


def test_fixture_is_small_and_complete():
    assert os.path.getsize(FIXTURE) < 200 * 1024
    z = np.load(FIXTURE)
    fx = fixture_module()
    assert [str(n) for n in z["names"]] == [c[0] for c in fx.CASES] and str(z["pillow_version"])
    assert len(cases()) == N_CASES
    for i, (name, h, w, oh, ow, box, values, filters) in enumerate(fx.CASES):        # the inputs are the generator's, the outputs Pillow's
        assert np.array_equal(z[name + "_in"], fx.image(i, h, w, values)), name
        assert np.array_equal(z[name + "_rect"], fx.box_f32(h, w, box)) and z[name + "_rect"].dtype == np.float32, name
        assert z[name + "_filters"].tolist() == list(filters)
        for f in filters:
            assert z[name + "_" + R.NAMES[f]].shape == (oh, ow, 3), name
    for f in R.FILTERS:                                     # the six geometries the issue names, under every filter
        for name in ("inexact_box", "up", "identity", "two_tiles", "white", "black"):
            assert name + "_" + R.NAMES[f] in z.files
        assert np.array_equal(z["identity_" + R.NAMES[f]], z["identity_in"]), "identity weights under %s" % R.NAMES[f]
    assert z["two_tiles_bicubic"].shape == (35, 70, 3)      # more than 32 rows, more than 64 columns


@pytest.mark.parametrize("index", range(N_CASES))
def test_ref_equals_recorded_pillow(index):
    name, f, img, box, want = cases()[index]
    got = R.resize(f, img, want.shape[0], want.shape[1], box)
    bad = int((got != want).sum())
    assert bad == 0, "%s under %s: %d of %d bytes differ from Pillow's" % (name, R.NAMES[f], bad, want.size)


def test_nearest_accumulates():
    """the two sources encode their column, and the closed form b0 + a * (i + 0.5) would take other columns: the cases tell the two readings apart"""
    for name, differing in (("nearest_504", 4), ("nearest_1222", 6)):
        _, f, img, box, want = [c for c in cases() if c[0] == name][0]
        assert f == R.NEAREST
        column = want[0, :, 0].astype(np.int32) + 256 * want[0, :, 1].astype(np.int32)
        acc = R.nearest_index(img.shape[1], box[0], box[2], want.shape[1])
        closed = R.nearest_index(img.shape[1], box[0], box[2], want.shape[1], closed_form=True)
        assert np.array_equal(column, acc), name
        assert int((closed != acc).sum()) == differing, name
        assert not np.array_equal(R.resize(f, img, want.shape[0], want.shape[1], box, closed_form=True), want), name


def _random_geometry(rng):
    """sides 1..80 and a box whose edges have no exact float32 form"""
    H, W, oh, ow = (int(v) for v in rng.integers(1, 81, 4))
    left, right = np.float32(rng.uniform(0, W * 0.4)), np.float32(W - rng.uniform(0, W * 0.4))
    upper, lower = np.float32(rng.uniform(0, H * 0.4)), np.float32(H - rng.uniform(0, H * 0.4))
    return H, W, oh, ow, np.array([left, upper, right, lower], np.float32)


def test_ref_equals_live_pillow():
    pytest.importorskip("PIL")
    fx = fixture_module()
    for name, f, img, box, want in cases():
        assert np.array_equal(fx.pillow_resize(f, img, want.shape[0], want.shape[1], box), want), "%s: the fixture is not this Pillow's output" % name
    rng = np.random.default_rng(2025)
    for k in range(12):
        H, W, oh, ow, box = _random_geometry(rng)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if k % 3 else (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
        for f in R.FILTERS:
            bad = int((R.resize(f, img, oh, ow, box) != fx.pillow_resize(f, img, oh, ow, box)).sum())
            assert bad == 0, "%s %dx%d -> %dx%d box %s: %d bytes differ from Pillow" % (R.NAMES[f], H, W, oh, ow, box.tolist(), bad)


# (in_size, b0, b1, out_size): the older tests' axes, then a steep one per filter family and NEAREST's two
AXES = [(37, 0, 37, 32), (20, 0, 20, 64), (47, 3.5, 40.0, 64), (53, 0.1, 50.3, 32), (64, 0, 64, 64), (1, 0, 1, 5), (80, 0, 80, 1), (5, 1.25, 1.5, 7),
        (150, 0, 150, 70), (264, 0, 264, 24), (396, 0, 396, 24), (504, 0, 504, 188), (1222, 0, 1222, 65)]


@pytest.mark.parametrize("f", R.FILTERS, ids=[R.NAMES[f] for f in R.FILTERS])
def test_host_taps_equal_ref(pkg, f):
    for axis in AXES:
        if R.ksize(f, *axis) > 4096:
            continue
        first, count, weights = pkg.resize_taps(*axis, filter=f)
        rf, rc, rw = R.taps(f, *axis)
        assert weights.dtype == np.int32 and weights.shape == rw.shape, axis
        assert np.array_equal(first, rf) and np.array_equal(count, rc) and np.array_equal(weights, rw), axis
        assert pkg.resize_ksize(*axis, filter=f) == rw.shape[1] == R.ksize(f, *axis)
        assert (count >= 1).all() and (first >= 0).all() and (first + count <= axis[0]).all()
        assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()         # what the kernel's window rests on
        if f == R.NEAREST:
            assert np.array_equal(pkg.resize_nearest_index(*axis), R.nearest_index(*axis)) and np.array_equal(first, R.nearest_index(*axis))


def test_host_taps_negative_weights_and_sums(pkg):
    """what the two passes must not assume: a weight below zero, rounded away from zero, and rows of weights that do not sum to 2^22"""
    for f in (R.BICUBIC, R.LANCZOS, R.HAMMING):
        _, _, w = pkg.resize_taps(53, 0.1, 50.3, 32, filter=f)
        assert np.array_equal(w, R.taps(f, 53, 0.1, 50.3, 32)[2])
        assert (w.sum(axis=1) != 1 << 22).any(), R.NAMES[f]
        if f != R.HAMMING:
            assert (w < 0).any(), R.NAMES[f]
    _, _, w = pkg.resize_taps(9, 0, 9, 40, filter=R.BICUBIC)              # an upscale: the lobes are negative
    assert w.min() < -100000 and w.max() > 1 << 22
    for f in R.FILTERS:                                                    # identity weights under every filter
        first, count, w = pkg.resize_taps(12, 0, 12, 12, filter=f)
        dense = np.zeros((12, 12), np.int64)
        for i in range(12):
            dense[i, first[i]:first[i] + count[i]] = w[i, :count[i]]
        assert np.array_equal(dense, np.eye(12, dtype=np.int64) << 22), R.NAMES[f]


def test_bilinear_filter_calls_equal_the_old_functions(pkg):
    """every existing function is the MBN_FILTER_BILINEAR call of its _filter sibling: same status, same fields, over the older tests' geometries"""
    import resize_ref
    import test_resize_cpu
    import test_resize_gpu
    import test_resize_ragged_cpu
    lib, B = pkg.host_lib(), pkg.FILTER_BILINEAR
    i32p = C.POINTER(C.c_int32)
    for axis in test_resize_cpu.AXES + [(1056, 0, 1056, 32), (1057, 0, 1057, 32), (37, -0.5, 10.0, 32), (37, 5.0, 5.0, 32), (0, 0.0, 1.0, 32)]:
        ks = lib.mbn_resize_ksize(*axis)
        assert lib.mbn_resize_ksize_filter(B, *axis) == ks
        if ks < 0:
            continue
        n = axis[3]
        old = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, ks), np.int32)]
        new = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, ks), np.int32)]
        assert lib.mbn_resize_taps(*axis, *[a.ctypes.data_as(i32p) for a in old]) == lib.mbn_resize_taps_filter(B, *axis, *[a.ctypes.data_as(i32p) for a in new])
        assert all(np.array_equal(a, b) for a, b in zip(old, new)), axis
        rf, rc, rw = resize_ref.taps(*axis)
        assert np.array_equal(new[0], rf) and np.array_equal(new[1], rc) and np.array_equal(new[2], rw), axis
        lo, hi, lo2, hi2 = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        for o0, o1 in ((0, n - 1), (n // 2, n - 1), (0, 0)):
            assert lib.mbn_resize_window(*axis, o0, o1, C.byref(lo), C.byref(hi)) == lib.mbn_resize_window_filter(B, *axis, o0, o1, C.byref(lo2), C.byref(hi2))
            assert (lo.value, hi.value) == (lo2.value, hi2.value)
    crop = lambda H, W, f: tuple(float(v) for v in pkg.fit_box(H, W, 224, 224, pkg.FIT_CROP, f))
    geoms = [(H, W, oh, ow, crop(H, W, 0.875) if box == "crop" else box) for H, W, oh, ow, box, _ in test_resize_gpu.CASES]
    geoms += [(1056, 2112, 32, 64, None), (1057, 40, 32, 32, None), (8193, 64, 4096, 64, None), (37, 53, 32, 32, (0.0, 0.0, 54.0, 37.0))]
    geoms += [(rows, cols, oh, ow, box) for oh, ow, images in test_resize_ragged_cpu.BATCHES for rows, cols, box in images]
    plan_fields, desc_fields = [n for n, _ in pkg.ResizePlan._fields_], [n for n, _ in pkg.ResizeDesc._fields_ if n != "box"]
    for H, W, oh, ow, box in geoms:
        b = pkg._box4(box)
        assert lib.mbn_resize_envelope(H, W, b, oh, ow) == lib.mbn_resize_envelope_filter(B, H, W, b, oh, ow)
        p, q = pkg.ResizePlan(), pkg.ResizePlan()
        rc = lib.mbn_resize_table_plan(H, W, b, oh, ow, C.byref(p))
        assert rc == lib.mbn_resize_table_plan_filter(B, H, W, b, oh, ow, C.byref(q)), (H, W, oh, ow)
        if rc == pkg.OK:
            assert [getattr(p, n) for n in plan_fields] == [getattr(q, n) for n in plan_fields], (H, W, oh, ow)
        item = pkg.resize_items([(7, H, W, box if box is not None else None)])
        d, e = pkg.ResizeDesc(), pkg.ResizeDesc()
        rc = lib.mbn_resize_ragged_plan(item, oh, ow, C.byref(d))
        assert rc == lib.mbn_resize_ragged_plan_filter(B, item, oh, ow, C.byref(e)), (H, W, oh, ow)
        if rc == pkg.OK:
            assert [getattr(d, n) for n in desc_fields] == [getattr(e, n) for n in desc_fields] and list(d.box) == list(e.box), (H, W, oh, ow)
    for oh, ow, images in test_resize_ragged_cpu.BATCHES:
        items = pkg.resize_items([(13 * i, r, c, b) for i, (r, c, b) in enumerate(images)])
        out = []
        for fn, head in ((lib.mbn_resize_ragged_plan_batch, ()), (lib.mbn_resize_ragged_plan_batch_filter, (B,))):
            desc = (pkg.ResizeDesc * len(items))()
            wgs, lds, span = C.c_int32(), C.c_int32(), C.c_int64()
            rc = fn(*head, items, len(items), oh, ow, desc, C.byref(wgs), C.byref(lds), C.byref(span))
            out.append((rc, wgs.value, lds.value, span.value, bytes(desc)))
        assert out[0] == out[1] and out[0][0] == pkg.OK, (oh, ow)


@pytest.mark.parametrize("f", [R.BICUBIC, R.LANCZOS, R.BOX, R.HAMMING, R.NEAREST], ids=["bicubic", "lanczos", "box", "hamming", "nearest"])
def test_planned_windows_equal_ref_tables(pkg, f):
    """every planned window is (first[o], first[last] + count[last]) of the reference's tables, for tiles of 1, 5, 32 and 64 outputs"""
    rng = np.random.default_rng(7 + f)
    axes = [a for a in AXES if R.ksize(f, *a) <= 67]
    for k in range(60):
        out_size = int(rng.integers(1, 80))
        scale = float(rng.choice([rng.uniform(0.05, 1.0), rng.uniform(1.0, 4.0), rng.uniform(4.0, 10.9)]))
        in_size = max(1, min(8192, int(round(out_size * scale / rng.uniform(0.6, 1.0)))))
        extent = min(in_size, out_size * scale)
        b0 = np.float32(rng.uniform(0, in_size - extent)) if k % 4 else np.float32(0)
        b1 = np.float32(min(float(b0) + extent, in_size))
        if b1 > b0:
            axes.append((in_size, float(b0), float(b1), out_size))
    checked = 0
    for in_size, b0, b1, out_size in axes:
        first, count, _ = R.taps(f, in_size, b0, b1, out_size)
        for tile in (1, 5, 32, 64):
            for o in range(0, out_size, tile):
                last = min(o + tile, out_size) - 1
                assert pkg.resize_window(in_size, b0, b1, out_size, o, last, filter=f) == (int(first[o]), int(first[last] + count[last])), \
                    (R.NAMES[f], in_size, b0, b1, out_size, o, last)
                checked += 1
    assert checked > 1000


def test_plans_hold_the_reference_windows(pkg):
    """a planned tile has room for its window under the wide filters: the LDS image of mbn_envelope.h from the reference's tables"""
    for f, (H, W, oh, ow) in [(R.BICUBIC, (375, 500, 224, 224)), (R.LANCZOS, (375, 500, 224, 224)), (R.BICUBIC, (384, 150, 24, 70)),
                              (R.LANCZOS, (770, 704, 70, 64)), (R.BOX, (3136, 3136, 64, 64)), (R.HAMMING, (1056, 2112, 32, 64))]:
        for ragged in (False, True):
            if ragged and f in (R.LANCZOS, R.HAMMING):
                continue
            if ragged:
                d = pkg.resize_ragged_plan([(0, H, W, None)], oh, ow, filter=f)[0][0]
                p = dict(kx=d.kx, ky=d.ky, toh=d.toh, tow=32 if ow <= 32 else 64, seg_stride=d.seg_stride, tmp_off=d.tmp_off, lds_bytes=d.lds_bytes)
            else:
                q = pkg.resize_table_plan(H, W, oh, ow, filter=f)
                p = {n: getattr(q, n) for n, _ in pkg.ResizePlan._fields_}
            (fx, cx, wx), (fy, cy, wy) = R.taps(f, W, 0, W, ow), R.taps(f, H, 0, H, oh)
            window = lambda fi, c, t: max(int(fi[min(o + t, len(fi)) - 1] + c[min(o + t, len(fi)) - 1] - fi[o]) for o in range(0, len(fi), t))
            assert (p["kx"], p["ky"]) == (wx.shape[1], wy.shape[1])
            tables = 4 * (p["tow"] * p["kx"] + ((p["toh"] * p["ky"] + p["tow"] + 2 * p["toh"]) if ragged else 0))
            assert p["seg_stride"] == ((window(fx, cx, p["tow"]) + p["kx"]) * 3 + 6) & ~3
            assert p["tmp_off"] == (((tables + 15) & ~15) + 4 * p["seg_stride"] + 15) & ~15
            assert p["lds_bytes"] == p["tmp_off"] + window(fy, cy, p["toh"]) * p["tow"] * 3 <= 61440, (R.NAMES[f], H, W)
    p = pkg.resize_table_plan(375, 500, 224, 224, filter=R.NEAREST)
    assert (p.kx, p.ky, p.tow, p.toh, p.tiles_x, p.tiles_y, p.lds_bytes) == (1, 1, 64, 32, 4, 7, 0)
    d = pkg.resize_ragged_plan([(0, 375, 500, None)], 224, 224, filter=R.NEAREST)[0][0]
    assert (d.kx, d.ky, d.toh, d.tiles_y, d.lds_bytes) == (1, 1, 32, 7, 4 * (64 + 32))


def test_largest_factor_per_filter(pkg):
    """include/mbn.h states the largest downscale each filter takes; one step inside the limit and one step outside it. ksize <= 67 ends lanczos
    at 11x, bicubic at 16.5x and bilinear / hamming at 33x; box has 67 taps at 66x and is ended earlier by the staged rows of a one-row tile"""
    lib = pkg.host_lib()
    env = lambda f, H, W, oh, ow: lib.mbn_resize_envelope_filter(f, H, W, None, oh, ow)
    plan = lambda f, H, W, oh, ow: lib.mbn_resize_table_plan_filter(f, H, W, None, oh, ow, C.byref(pkg.ResizePlan()))
    OK, UNS = pkg.OK, pkg.EUNSUPPORTED
    for f, inside, outside in [(R.LANCZOS, 352, 353), (R.BICUBIC, 528, 529), (R.BILINEAR, 1056, 1057), (R.HAMMING, 1056, 1057), (R.BOX, 2112, 2113)]:
        assert pkg.resize_ksize(inside, 0, inside, 32, filter=f) == 67 and pkg.resize_ksize(outside, 0, outside, 32, filter=f) == 69
        for rc, side in ((OK, inside), (UNS, outside)):                # rows alone, columns alone (32 of them), both
            assert env(f, side, 40, 32, 32) == rc and env(f, 40, side, 32, 32) == rc, (R.NAMES[f], side)
            assert plan(f, side, 40, 32, 32) == rc and plan(f, 40, side, 32, 32) == rc and plan(f, side, side, 32, 32) == rc, (R.NAMES[f], side)
    for f, side in [(R.LANCZOS, 704), (R.BICUBIC, 1056), (R.BILINEAR, 2112), (R.HAMMING, 2112)]:       # and on two column tiles of 64
        assert plan(f, side // 2, side, 32, 64) == OK and plan(f, side // 2, side + 1, 32, 64) == UNS, R.NAMES[f]
    # box with more than 32 output columns: the envelope takes 66x, the plan refuses what a one-row tile cannot stage
    assert env(R.BOX, 40, 4224, 32, 64) == OK and env(R.BOX, 4224, 4224, 64, 64) == OK
    assert plan(R.BOX, 40, 3712, 32, 64) == OK and plan(R.BOX, 40, 3776, 32, 64) == UNS             # columns alone: 58x, not 59x
    assert plan(R.BOX, 3136, 3136, 64, 64) == OK and plan(R.BOX, 3200, 3200, 64, 64) == UNS         # both axes: 49x, not 50x
    assert plan(R.BOX, 4224, 40, 64, 64) == OK                                                      # rows alone: 66x
    d = pkg.ResizeDesc()
    rag = lambda f, H, W, oh, ow: lib.mbn_resize_ragged_plan_filter(f, pkg.resize_items([(0, H, W, None)]), oh, ow, C.byref(d))
    assert rag(R.BICUBIC, 528, 1056, 32, 64) == OK and rag(R.BICUBIC, 529, 1056, 32, 64) == UNS
    assert rag(R.BOX, 40, 3712, 32, 64) == OK and rag(R.BOX, 40, 3776, 32, 64) == UNS
    assert rag(R.BOX, 3136, 3136, 64, 64) == OK and rag(R.BOX, 3200, 3200, 64, 64) == UNS
    assert env(R.NEAREST, 8192, 8192, 1, 1) == OK and plan(R.NEAREST, 8192, 8192, 1, 1) == OK     # NEAREST: any factor
    assert env(R.NEAREST, 8193, 64, 32, 32) == UNS and env(R.NEAREST, 64, 64, 4097, 32) == UNS


def test_status_codes(pkg):
    lib = pkg.host_lib()
    i32 = (C.c_int32 * 64)()
    p, d, lo, hi = pkg.ResizePlan(), pkg.ResizeDesc(), C.c_int32(), C.c_int32()
    item = pkg.resize_items([(0, 37, 53, None)])
    for bad in (-1, 6, 99):                                                # an unknown filter
        assert lib.mbn_resize_ksize_filter(bad, 37, 0.0, 37.0, 32) == pkg.EINVAL
        assert lib.mbn_resize_taps_filter(bad, 4, 0.0, 4.0, 2, i32, i32, i32) == pkg.EINVAL
        assert lib.mbn_resize_envelope_filter(bad, 37, 53, None, 32, 32) == pkg.EINVAL
        assert lib.mbn_resize_table_plan_filter(bad, 37, 53, None, 32, 32, C.byref(p)) == pkg.EINVAL
        assert lib.mbn_resize_window_filter(bad, 37, 0.0, 37.0, 32, 0, 31, C.byref(lo), C.byref(hi)) == pkg.EINVAL
        assert lib.mbn_resize_ragged_plan_filter(bad, item, 32, 32, C.byref(d)) == pkg.EINVAL
    for f in (R.HAMMING, R.LANCZOS):                                       # no device form of their weights: the ragged path refuses them
        assert lib.mbn_resize_ragged_plan_filter(f, item, 32, 32, C.byref(d)) == pkg.EUNSUPPORTED
        with pytest.raises(pkg.MbnError) as e:
            pkg.resize_ragged_plan([(0, 37, 53, None)], 32, 32, filter=f)
        assert e.value.code == pkg.EUNSUPPORTED
        assert lib.mbn_resize_table_plan_filter(f, 37, 53, None, 32, 32, C.byref(p)) == pkg.OK
    for f in (R.NEAREST, R.BOX, R.BILINEAR, R.BICUBIC):
        assert lib.mbn_resize_ragged_plan_filter(f, item, 32, 32, C.byref(d)) == pkg.OK
        assert lib.mbn_resize_ragged_plan_filter(f, pkg.resize_items([(-1, 37, 53, None)]), 32, 32, C.byref(d)) == pkg.EINVAL
    nan = float("nan")
    for f in R.FILTERS:                                                    # a box is refused under every filter alike
        for b0, b1 in [(-0.5, 10.0), (0.0, 37.5), (5.0, 5.0), (nan, 10.0)]:
            assert lib.mbn_resize_ksize_filter(f, 37, b0, b1, 32) == pkg.EINVAL
        assert lib.mbn_resize_taps_filter(f, 4, 0.0, 4.0, 2, None, i32, i32) == pkg.EINVAL
    assert lib.mbn_resize_nearest_index(37, 0.0, 37.0, 32, None) == pkg.EINVAL
    assert lib.mbn_resize_nearest_index(37, 5.0, 5.0, 32, i32) == pkg.EINVAL and lib.mbn_resize_nearest_index(0, 0.0, 1.0, 32, i32) == pkg.EINVAL
    assert (pkg.FILTER_NEAREST, pkg.FILTER_LANCZOS, pkg.FILTER_BILINEAR, pkg.FILTER_BICUBIC, pkg.FILTER_BOX, pkg.FILTER_HAMMING) == (0, 1, 2, 3, 4, 5)


def test_symbols_declared(pkg):
    names = pkg.declared_symbols()
    for s in ("mbn_resize_ksize_filter", "mbn_resize_taps_filter", "mbn_resize_nearest_index", "mbn_resizer_create_filter",
              "mbn_ragged_resizer_create_filter", "mbn_resize_taps_device_filter", "mbn_net_set_resize_filter", "mbn_net_get_resize_filter"):
        assert s in names, s
    host = pkg.host_lib()
    for s in ("mbn_resize_ksize_filter", "mbn_resize_taps_filter", "mbn_resize_nearest_index", "mbn_resize_envelope_filter", "mbn_resize_window_filter",
              "mbn_resize_table_plan_filter", "mbn_resize_ragged_plan_filter", "mbn_resize_ragged_plan_batch_filter"):
        assert hasattr(host, s), s
    header = open(pkg.HEADER).read()
    for name, value in (("NEAREST", 0), ("LANCZOS", 1), ("BILINEAR", 2), ("BICUBIC", 3), ("BOX", 4), ("HAMMING", 5)):
        import re
        assert re.search(r"#define MBN_FILTER_%s\s+%d\b" % (name, value), header), name
