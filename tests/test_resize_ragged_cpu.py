"""The ragged resize without a GPU: what the host plans per image (libmbn_host.so: mbn_resize_window, mbn_resize_ragged_plan, _plan_batch) against the
tables of tests/resize_ref.py. The kernel derives every tile's source window from two evaluations of lo / hi; the planner sizes LDS from the same two,
so they are pinned here, exactly, against (first[o], first[last] + count[last]) of the reference tables."""
import ctypes as C
import os

import numpy as np
import pytest

import resize_ref

HERE = os.path.dirname(os.path.abspath(__file__))
LDS = 60 * 1024
WAVES = 4


def _crop(h, w, oh, ow, f=0.875):
    return tuple(float(v) for v in resize_ref.fit_box(h, w, oh, ow, resize_ref.FIT_CROP, f))


def _golden():
    z = np.load(os.path.join(HERE, "golden", "resize_pillow.npz"))
    return [(str(n), z[str(n) + "_in"], z[str(n) + "_box"], z[str(n) + "_out"]) for n in z["names"]]


# (out_rows, out_cols, [(rows, cols, box)]): every batch of tests/test_resize_ragged_gpu.py, then the golden cases and the envelope's corners
BATCHES = [
    (40, 72, [(37, 53, None), (20, 30, None), (1, 1, None), (40, 72, None), (1290, 17, None), (9, 2300, None), (33, 47, (3.5, 2.25, 40.0, 30.75)),
              (375, 500, _crop(375, 500, 40, 72)), (37, 53, (1.5, 0.0, 50.25, 36.5))]),
    (5, 7, [(1, 1, None), (64, 64, None), (165, 9, None)]),          # 165 rows -> 5: 67 taps, the steepest 5 rows take (310 -> 5 is refused below)
    (224, 224, [(31, 29, (1, 2, 28, 30)), (375, 500, _crop(375, 500, 224, 224)), (480, 640, None), (224, 224, None)]),
    (32, 64, [(1056, 2112, None), (1000, 17, None), (8, 2048, None)]),
    (4096, 4096, [(1, 1, None), (8192, 8192, None)]),
    (1, 1, [(33, 33, None), (1, 1, None)]),
    (33, 65, [(1056, 2080, None), (7, 300, (0.5, 0.25, 299.75, 6.5))]),
]
BATCHES += [(out.shape[0], out.shape[1], [(img.shape[0], img.shape[1], tuple(float(v) for v in box))]) for _, img, box, out in _golden()]


def _whole(rows, cols, box):
    return box if box is not None else (0.0, 0.0, float(cols), float(rows))


def _check_axis_windows(pkg, in_size, b0, b1, out_size, tile):
    """every tile of `tile` outputs: the planner's window is the tables'; returns the widest"""
    first, count, _ = resize_ref.taps(in_size, b0, b1, out_size)
    most = 0
    for o in range(0, out_size, tile):
        last = min(o + tile, out_size) - 1
        want = (int(first[o]), int(first[last] + count[last]))
        assert pkg.resize_window(in_size, b0, b1, out_size, o, last) == want, (in_size, b0, b1, out_size, o, last)
        most = max(most, want[1] - want[0])
    return most, first, count


@pytest.mark.parametrize("index", range(len(BATCHES)))
def test_plan_equals_reference_tables(pkg, index):
    oh, ow, images = BATCHES[index]
    items = [(13 * i, r, c, b) for i, (r, c, b) in enumerate(images)]
    desc, wgs, lds, span = pkg.resize_ragged_plan(items, oh, ow)
    tow = 32 if ow <= 32 else 64
    tiles_x = -(-ow // tow)
    wg0 = 0
    for d, (off, rows, cols, box) in zip(desc, items):
        b = _whole(rows, cols, box)
        assert (d.src_offset, d.rows, d.cols, list(d.box)) == (off, rows, cols, [float(np.float32(v)) for v in b])
        assert d.kx == resize_ref.ksize(cols, b[0], b[2], ow) and d.ky == resize_ref.ksize(rows, b[1], b[3], oh)
        assert 1 <= d.toh <= min(32, oh)
        assert d.tiles_y == -(-oh // d.toh) and (d.tiles_y - 1) * d.toh < oh <= d.tiles_y * d.toh      # the tiles cover the output exactly
        assert d.wg0 == wg0
        wg0 += tiles_x * d.tiles_y
        most_x, _, _ = _check_axis_windows(pkg, cols, b[0], b[2], ow, tow)
        most_y, fy, cy = _check_axis_windows(pkg, rows, b[1], b[3], oh, d.toh)
        # the LDS image: int32 tables, four staged rows (segment + kx pixels of slack + 3, on 4 bytes), the window
        assert d.seg_stride % 4 == 0 and d.seg_stride >= (most_x + d.kx) * 3 + 3
        tables = 4 * (tow * d.kx + d.toh * d.ky + tow + 2 * d.toh)
        assert d.tmp_off % 16 == 0 and d.tmp_off >= tables + WAVES * d.seg_stride
        assert d.lds_bytes == d.tmp_off + most_y * tow * 3 and d.lds_bytes <= LDS
        if d.toh < min(32, oh):                                                         # the tallest tile that fits: one row more does not
            t = d.toh + 1
            taller = max(int(fy[min(o + t, oh) - 1] + cy[min(o + t, oh) - 1] - fy[o]) for o in range(0, oh, t))
            tables = 4 * (tow * d.kx + t * d.ky + tow + 2 * t)
            assert ((tables + 15) & ~15) + WAVES * d.seg_stride + taller * tow * 3 > LDS
    assert wgs == wg0 and lds == max(d.lds_bytes for d in desc)
    assert span == max(off + rows * cols * 3 for off, rows, cols, _ in items)


def test_random_windows_equal_reference_tables(pkg):
    """about 2000 axes with scale <= 33 and boxes without an exact float32 form: the window of every tile of 1, 5 and 32 outputs"""
    rng = np.random.default_rng(20261019)
    checked = 0
    for k in range(2000):
        out_size = int(rng.integers(1, 41))
        scale = float(rng.choice([rng.uniform(0.05, 1.0), rng.uniform(1.0, 4.0), rng.uniform(4.0, 33.0)], p=[0.3, 0.5, 0.2]))
        in_size = max(1, min(8192, int(round(out_size * scale / rng.uniform(0.6, 1.0)))))
        extent = min(in_size, out_size * scale)
        b0 = np.float32(rng.uniform(0, in_size - extent)) if k % 4 else np.float32(0)
        b1 = np.float32(min(float(b0) + extent, in_size))
        if not b1 > b0 or float(np.float32(b1 - b0)) / out_size > 33.0:
            continue
        first, count, _ = resize_ref.taps(in_size, b0, b1, out_size)
        for tile in (1, 5, 32):
            for o in range(0, out_size, tile):
                last = min(o + tile, out_size) - 1
                assert pkg.resize_window(in_size, float(b0), float(b1), out_size, o, last) == (int(first[o]), int(first[last] + count[last])), \
                    (in_size, float(b0), float(b1), out_size, o, last)
                checked += 1
    assert checked > 20000


def test_refusals(pkg):
    lib = pkg.host_lib()
    d = pkg.ResizeDesc()
    plan = lambda off, rows, cols, box, oh=32, ow=32: lib.mbn_resize_ragged_plan(pkg.resize_items([(off, rows, cols, box)]), oh, ow, C.byref(d))
    nan = float("nan")
    assert plan(0, 1056, 40, None) == pkg.OK and d.ky == 67
    assert plan(0, 1060, 40, None) == pkg.EUNSUPPORTED                           # a 33.1x downscale: 69 taps
    assert plan(0, 40, 1060, None) == pkg.EUNSUPPORTED
    assert plan(0, 310, 9, None, 5, 7) == pkg.EUNSUPPORTED and plan(0, 165, 9, None, 5, 7) == pkg.OK      # 62x: 125 taps; 33x: 67
    assert plan(0, 8193, 64, None, 4096, 64) == pkg.EUNSUPPORTED                 # a source side of 8193
    assert plan(0, 64, 8193, None, 64, 4096) == pkg.EUNSUPPORTED
    assert plan(0, 64, 64, None, 4097, 64) == pkg.EUNSUPPORTED
    assert plan(0, 37, 53, (0.0, nan, 53.0, 37.0)) == pkg.EINVAL                 # a NaN box
    assert plan(0, 37, 53, (5.0, 0.0, 5.0, 37.0)) == pkg.EINVAL                  # b1 <= b0
    assert plan(0, 37, 53, (6.0, 0.0, 5.0, 37.0)) == pkg.EINVAL
    assert plan(0, 37, 53, (0.0, 0.0, 54.0, 37.0)) == pkg.EINVAL                 # beyond the image
    assert plan(0, 0, 53, (0.0, 0.0, 53.0, 1.0)) == pkg.EINVAL and plan(0, 37, 53, None, 0, 32) == pkg.EINVAL
    assert plan(-1, 37, 53, None) == pkg.EINVAL                                  # a negative offset
    assert lib.mbn_resize_ragged_plan(None, 32, 32, C.byref(d)) == pkg.EINVAL
    # a batch answers with its first refused item, wherever it stands
    good, steep = (0, 37, 53, None), (0, 1060, 40, None)
    with pytest.raises(pkg.MbnError) as e:
        pkg.resize_ragged_plan([good, steep, good], 32, 32)
    assert e.value.code == pkg.EUNSUPPORTED
    with pytest.raises(pkg.MbnError) as e:
        pkg.resize_ragged_plan([good, good, (0, 37, 53, (0.0, nan, 53.0, 37.0))], 32, 32)
    assert e.value.code == pkg.EINVAL
    lo, hi = C.c_int32(), C.c_int32()
    assert lib.mbn_resize_window(37, 0.0, 37.0, 32, 0, 32, C.byref(lo), C.byref(hi)) == pkg.EINVAL      # an index outside the axis
    assert lib.mbn_resize_window(37, 0.0, 37.0, 32, 5, 4, C.byref(lo), C.byref(hi)) == pkg.EINVAL
    assert lib.mbn_resize_window(37, 5.0, 5.0, 32, 0, 0, C.byref(lo), C.byref(hi)) == pkg.EINVAL


def test_symbols_declared(pkg):
    names = pkg.declared_symbols()
    for s in ("mbn_ragged_resizer_create", "mbn_ragged_resizer_set", "mbn_resize_ragged_u8", "mbn_ragged_resizer_destroy", "mbn_resize_taps_device",
              "mbn_net_resize_inputs"):
        assert s in names, s
    host = pkg.host_lib()
    for s in ("mbn_resize_window", "mbn_resize_ragged_plan", "mbn_resize_ragged_plan_batch"):
        assert hasattr(host, s), s
    assert C.sizeof(pkg.ResizeItem) == 32 and C.sizeof(pkg.ResizeDesc) == 64
