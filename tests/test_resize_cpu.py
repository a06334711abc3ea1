"""The resize front-end without a GPU: tests/resize_ref.py (the numpy statement of include/mbn.h, "resize front-end") against Pillow's own bytes —
recorded in tests/golden/resize_pillow.npz, and live where Pillow is installed — and the host tables of libmbn_host.so (mbn_resize_taps,
mbn_resize_ksize, mbn_fit_box, the envelope) against resize_ref, as int32, exactly."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import resize_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "resize_pillow.npz")


def _fixture_module():
    spec = importlib.util.spec_from_file_location("make_resize_fixtures", os.path.join(HERE, "golden", "make_resize_fixtures.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _cases():
    z = np.load(FIXTURE)
    return [(str(n), z[str(n) + "_in"], z[str(n) + "_box"], z[str(n) + "_out"]) for n in z["names"]]


def test_fixture_is_small_and_complete():
    assert os.path.getsize(FIXTURE) < 100 * 1024
    z = np.load(FIXTURE)
    fx = _fixture_module()
    assert [str(n) for n in z["names"]] == [c[0] for c in fx.CASES]
    assert str(z["pillow_version"])
    for i, (name, h, w, oh, ow, box, values) in enumerate(fx.CASES):        # the inputs are the generator's, the outputs Pillow's
        assert np.array_equal(z[name + "_in"], fx.image(i, h, w, values)), name
        assert np.array_equal(z[name + "_box"], fx.box_f32(h, w, box)) and z[name + "_box"].dtype == np.float32, name
        assert z[name + "_out"].shape == (oh, ow, 3) and oh <= 64 and ow <= 96, name


@pytest.mark.parametrize("index", range(10))
def test_ref_equals_recorded_pillow(index):
    name, img, box, want = _cases()[index]
    got = resize_ref.resize(img, want.shape[0], want.shape[1], box)
    bad = int((got != want).sum())
    assert bad == 0, "%s: %d of %d bytes differ from Pillow's" % (name, bad, want.size)


def test_ref_identity_axis_is_a_copy():
    name, img, box, want = [c for c in _cases() if c[0] == "identity"][0]
    assert np.array_equal(want, img)
    f, c, w = resize_ref.taps(24, 0, 24, 24)
    assert (w[:, 0] == 1 << 22).all() and (w[:, 1:] == 0).all() and np.array_equal(f, np.arange(24))


def _random_geometry(rng):
    """sides 1..80 and a box whose edges have no exact float32 form"""
    H, W, oh, ow = (int(v) for v in rng.integers(1, 81, 4))
    left, right = np.float32(rng.uniform(0, W * 0.4)), np.float32(W - rng.uniform(0, W * 0.4))
    upper, lower = np.float32(rng.uniform(0, H * 0.4)), np.float32(H - rng.uniform(0, H * 0.4))
    return H, W, oh, ow, np.array([left, upper, right, lower], np.float32)


def test_ref_equals_live_pillow():
    pytest.importorskip("PIL")
    fx = _fixture_module()
    for name, img, box, want in _cases():
        assert np.array_equal(fx.pillow_resize(img, want.shape[0], want.shape[1], box), want), "%s: the fixture is not this Pillow's output" % name
    rng = np.random.default_rng(2024)
    for k in range(20):
        H, W, oh, ow, box = _random_geometry(rng)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8) if k % 3 else (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)
        want = fx.pillow_resize(img, oh, ow, box)
        got = resize_ref.resize(img, oh, ow, box)
        bad = int((got != want).sum())
        assert bad == 0, "%dx%d -> %dx%d box %s: %d bytes differ from Pillow" % (H, W, oh, ow, box.tolist(), bad)


AXES = [(37, 0, 37, 32), (20, 0, 20, 64), (1000, 0, 1000, 32), (47, 3.5, 40.0, 64), (53, 0.1, 50.3, 32), (64, 0, 64, 64), (1, 0, 1, 5),
        (80, 0, 80, 1), (5, 1.25, 1.5, 7)]


@pytest.mark.parametrize("axis", AXES)
def test_host_taps_equal_ref(pkg, axis):
    first, count, weights = pkg.resize_taps(*axis)
    f, c, w = resize_ref.taps(*axis)
    assert weights.dtype == np.int32 and weights.shape == w.shape
    assert np.array_equal(first, f) and np.array_equal(count, c) and np.array_equal(weights, w)
    assert pkg.resize_ksize(*axis) == w.shape[1] == resize_ref.ksize(*axis)
    assert (count >= 1).all() and (first >= 0).all() and (first + count <= axis[0]).all()
    assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()         # what the kernel's window rests on


def test_host_taps_special_values(pkg):
    assert pkg.resize_ksize(1000, 0, 1000, 32) == 65
    _, _, w = pkg.resize_taps(64, 0, 64, 64)
    assert (w[:, 0] == 1 << 22).all() and (w[:, 1:] == 0).all()
    lib = pkg.host_lib()
    buf = (C.c_int32 * 16)()
    assert lib.mbn_resize_taps(4, 0.0, 4.0, 2, None, buf, buf) == pkg.EINVAL


def test_fit_box(pkg):
    assert pkg.fit_box(480, 640, 224, 224, pkg.FIT_CROP, 1.0).tolist() == [80.0, 0.0, 560.0, 480.0]
    assert pkg.fit_box(375, 500, 224, 224, pkg.FIT_CROP, 0.875).tolist() == [85.9375, 23.4375, 414.0625, 351.5625]
    assert pkg.fit_box(375, 500, 224, 224, pkg.FIT_STRETCH, 0.3).tolist() == [0.0, 0.0, 500.0, 375.0]
    for args in [(375, 500, 224, 224, 1, 0.875), (480, 640, 224, 224, 1, 1.0), (75, 100, 64, 96, 1, 1.0), (50, 80, 64, 96, 1, 0.9),
                 (1, 7, 3, 5, 1, 0.33), (100, 30, 64, 96, 0, 1.0)]:
        got, want = pkg.fit_box(*args), resize_ref.fit_box(*args)
        assert got.dtype == np.float32 and np.array_equal(got, want), args
        assert 0 <= got[0] < got[2] <= args[1] and 0 <= got[1] < got[3] <= args[0]
    lib = pkg.host_lib()
    box = (C.c_float * 4)()
    for f in (0.0, -0.5, 1.5, float("nan")):
        assert lib.mbn_fit_box(375, 500, 224, 224, pkg.FIT_CROP, f, box) == pkg.EINVAL
    assert lib.mbn_fit_box(375, 500, 224, 224, 7, 1.0, box) == pkg.EINVAL
    assert lib.mbn_fit_box(0, 500, 224, 224, pkg.FIT_CROP, 1.0, box) == pkg.EINVAL
    assert lib.mbn_fit_box(375, 500, 224, 224, pkg.FIT_CROP, 1.0, None) == pkg.EINVAL


def test_boxes_refused(pkg):
    lib = pkg.host_lib()
    nan = float("nan")
    for b0, b1 in [(-0.5, 10.0), (0.0, 37.5), (5.0, 5.0), (6.0, 5.0), (nan, 10.0), (0.0, nan)]:
        assert lib.mbn_resize_ksize(37, b0, b1, 32) == pkg.EINVAL, (b0, b1)
        with pytest.raises(pkg.MbnError):
            pkg.resize_taps(37, b0, b1, 32)
    assert lib.mbn_resize_ksize(0, 0.0, 1.0, 32) == pkg.EINVAL and lib.mbn_resize_ksize(37, 0.0, 37.0, 0) == pkg.EINVAL
    bad = (C.c_float * 4)(0.0, 0.0, 54.0, 37.0)                                       # right edge beyond a 53-wide image
    assert lib.mbn_resize_envelope(37, 53, bad, 32, 32) == pkg.EINVAL
    assert lib.mbn_resize_envelope(37, 53, None, 0, 32) == pkg.EINVAL


def test_envelope_edges(pkg):
    lib = pkg.host_lib()
    assert pkg.resize_ksize(1056, 0, 1056, 32) == 67 and pkg.resize_ksize(1057, 0, 1057, 32) == 69
    assert lib.mbn_resize_envelope(1056, 40, None, 32, 32) == pkg.OK                 # 67 taps: the last geometry inside
    assert lib.mbn_resize_envelope(1057, 40, None, 32, 32) == pkg.EUNSUPPORTED       # 69
    assert lib.mbn_resize_envelope(40, 1056, None, 32, 32) == pkg.OK
    assert lib.mbn_resize_envelope(40, 1057, None, 32, 32) == pkg.EUNSUPPORTED
    assert lib.mbn_resize_envelope(8192, 8192, None, 4096, 4096) == pkg.OK
    assert lib.mbn_resize_envelope(8193, 64, None, 4096, 64) == pkg.EUNSUPPORTED
    assert lib.mbn_resize_envelope(64, 8193, None, 64, 4096) == pkg.EUNSUPPORTED
    assert lib.mbn_resize_envelope(64, 64, None, 4097, 64) == pkg.EUNSUPPORTED
    assert lib.mbn_resize_envelope(64, 64, None, 64, 4097) == pkg.EUNSUPPORTED
    assert lib.mbn_resize_envelope(1, 1, None, 4096, 4096) == pkg.OK                  # any upscale


def _table_plan_rule(H, W, oh, ow, box):
    """The tile rule of mbn_resizer_create as it stood when the plan lived beside the kernel, from resize_ref's tables: a tile's window is
    first[last] + count[last] - first[o], and a rule's window the largest over the tiles."""
    b = box if box is not None else (0.0, 0.0, float(W), float(H))
    (fx, cx, wx), (fy, cy, wy) = resize_ref.taps(W, b[0], b[2], ow), resize_ref.taps(H, b[1], b[3], oh)
    window = lambda f, c, t: max(int(f[min(o + t, len(f)) - 1] + c[min(o + t, len(f)) - 1] - f[o]) for o in range(0, len(f), t))
    kx, ky = wx.shape[1], wy.shape[1]
    tow = 32 if ow <= 32 else 64
    stage_off = (tow * kx * 4 + 15) & ~15
    seg_stride = ((window(fx, cx, tow) + kx) * 3 + 6) & ~3
    tmp_off = (stage_off + 4 * seg_stride + 15) & ~15
    toh = min(oh, 32)
    while toh > 1 and tmp_off + window(fy, cy, toh) * tow * 3 > 61440:
        toh -= 1
    return dict(kx=kx, ky=ky, tow=tow, toh=toh, tiles_x=-(-ow // tow), tiles_y=-(-oh // toh), seg_stride=seg_stride, stage_off=stage_off,
                tmp_off=tmp_off, lds_bytes=tmp_off + window(fy, cy, toh) * tow * 3)


def test_table_plan_did_not_move(pkg):
    """mbn_resize_table_plan (plain C, two exact lo / hi per tile) gives, field for field, the tile mbn_resizer_build used to size from whole tap
    tables: on every geometry of test_resize_gpu.CASES, the 33x downscale of both axes, every image of test_resize_ragged_cpu.BATCHES (the golden
    fixtures are among them) and four anchors written out. No geometry inside mbn_resize_envelope has an output row that does not fit: the
    largest one-row tile is the 33x downscale of both axes below, 55984 of 61440 bytes (64 x 67 weights, four staged rows of 64 x 33 + 2 x 67
    pixels, a window of 67 rows), and a fractional box moves a window by a pixel or two. So MBN_EUNSUPPORTED is pinned here only as the
    envelope's answer."""
    import test_resize_gpu
    import test_resize_ragged_cpu
    crop = lambda H, W, f: tuple(float(v) for v in pkg.fit_box(H, W, 224, 224, pkg.FIT_CROP, f))
    geoms = [(H, W, oh, ow, crop(H, W, 0.875) if box == "crop" else box) for H, W, oh, ow, box, _ in test_resize_gpu.CASES]
    geoms += [(1056, 2112, 32, 64, None), (1080, 1920, 224, 224, crop(1080, 1920, 1.0))]
    geoms += [(rows, cols, oh, ow, box) for oh, ow, images in test_resize_ragged_cpu.BATCHES for rows, cols, box in images]
    fields = [n for n, _ in pkg.ResizePlan._fields_]
    plans = {}
    for H, W, oh, ow, box in geoms:
        p = pkg.resize_table_plan(H, W, oh, ow, box)
        plans[(H, W, oh, ow)] = got = {n: getattr(p, n) for n in fields}
        assert got == _table_plan_rule(H, W, oh, ow, box), (H, W, oh, ow, box)
        assert got["lds_bytes"] <= 61440
    assert crop(375, 500, 0.875) == (85.9375, 23.4375, 414.0625, 351.5625) and crop(1080, 1920, 1.0) == (420.0, 0.0, 1500.0, 1080.0)
    anchors = {(375, 500, 224, 224): dict(kx=5, ky=5, toh=32, seg_stride=304, tmp_off=2496, lds_bytes=11904, tiles_x=4, tiles_y=7),
               (1000, 17, 32, 32): dict(kx=3, ky=65, toh=19, seg_stride=64, tmp_off=640, lds_bytes=59104),
               (1056, 2112, 32, 64): dict(kx=67, ky=67, toh=1, seg_stride=6540, tmp_off=43312, lds_bytes=55984),
               (1080, 1920, 224, 224): dict(kx=11, ky=11, toh=32, seg_stride=980, tmp_off=6736, lds_bytes=37456)}
    for g, want in anchors.items():
        assert {n: plans[g][n] for n in want} == want, g
    window_rows = lambda g: (plans[g]["lds_bytes"] - plans[g]["tmp_off"]) // (plans[g]["tow"] * 3)
    assert window_rows((375, 500, 224, 224)) == 49 and window_rows((1000, 17, 32, 32)) == 609
    lib, p = pkg.host_lib(), pkg.ResizePlan()
    assert lib.mbn_resize_table_plan(1057, 40, None, 32, 32, C.byref(p)) == pkg.EUNSUPPORTED           # 69 taps: the envelope's answer
    assert lib.mbn_resize_table_plan(37, 53, (C.c_float * 4)(0.0, 0.0, 54.0, 37.0), 32, 32, C.byref(p)) == pkg.EINVAL
    assert lib.mbn_resize_table_plan(37, 53, None, 32, 32, None) == pkg.EINVAL


def test_symbols_declared(pkg):
    names = pkg.declared_symbols()
    for s in ("mbn_resize_ksize", "mbn_resize_taps", "mbn_fit_box", "mbn_resizer_create", "mbn_resize_u8", "mbn_resizer_destroy", "mbn_net_resize_input"):
        assert s in names, s
    host = pkg.host_lib()
    for s in ("mbn_resize_ksize", "mbn_resize_taps", "mbn_fit_box", "mbn_resize_envelope", "mbn_resize_table_plan"):
        assert hasattr(host, s), s
