"""The source-size segment paths of ONE net, one after the other: what they share on a net is the staging buffer, the one ragged resizer, the
ragged read-out set and the score record. Every step must give the bits of the same single call on a fresh net, a refused call in between must
write nothing and leave the record of the previous successful call, and the next step must still match its fresh net.

test_net_segment_fit / _views_fit / _slide (test_dense_window_gpu.py, test_dense_ensemble_gpu.py, test_dense_slide_gpu.py) pin each path on a net
of its own against the numpy references; this file takes their configuration and source sizes and pins the order of the calls."""
import ctypes as C

import numpy as np
import pytest

import resize_filters_ref as R
from test_dense_any_gpu import LAB_FILL, SC_FILL, TAIL, _ragged_layout
from test_dilation_gpu import _weights_os

ALPHA, CLASSES, ROWS, COLS, BATCH, MAX_BATCH, OS = 0.5, 21, 64, 96, 2, 8, 8
SH, SW = 75, 130                                    # the uniform source: letterboxed (its aspect is not the canvas's), 4 tiles under the slide below
SOURCES = [(SH, SW), (ROWS, COLS)]                  # the ragged sources of test_net_segment_fit: one letterboxed, one of the canvas's own size
TILE, STRIDE = (ROWS, COLS), (43, 64)
COLOR = (200, 30, 90)


def _i64(v):
    return (C.c_int64 * len(v))(*v)


def _i32(v):
    return (C.c_int32 * len(v))(*v)


@pytest.mark.gpu
def test_paths_share_one_net(pkg, ctx, tmp_path):
    n = BATCH
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, OS)
    lib = ctx.lib
    rng = np.random.default_rng(77)
    bufs = []

    def dev(a):
        bufs.append(ctx.to_device(a))
        return bufs[-1]

    def new_net(color):
        net = pkg.Net(ctx, hw.plan, hw.blob.copy(), MAX_BATCH)
        net.set_input_u8(True)
        if color:
            net.set_pad_color(*color)
        return net

    def drop(net):
        net.destroy()
        net._dev_blob.free()

    images = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in SOURCES]
    src_offs = [0, images[0].size]
    d_rag = dev(np.concatenate([img.ravel() for img in images]))
    d_uni = dev(rng.integers(0, 256, (n, SH, SW, 3), dtype=np.uint8))
    d_canvas = dev(rng.integers(0, 256, (n, ROWS, COLS, 3), dtype=np.uint8))
    rrows, rcols = [s[0] for s in SOURCES], [s[1] for s in SOURCES]
    dst, rag_total = _ragged_layout(SOURCES, order=(1, 0), gap=7)
    total = n * SH * SW + TAIL
    assert rag_total <= total
    rag_span = [(dst[i], SOURCES[i][0] * SOURCES[i][1]) for i in range(n)]
    uni_span = [(0, n * SH * SW)]
    truth = rng.integers(0, CLASSES + 2, total).astype(np.uint8)
    d_truth, d_counts, d_n = dev(truth), dev(np.zeros((CLASSES + 1) ** 2, np.uint64)), dev(np.zeros(2 * n, np.int32))

    def images_fit(fit):
        return lambda net, lab, sc: lib.mbn_net_segment_images_fit(net.h, d_rag.ptr, _i64(src_offs), _i32(rrows), _i32(rcols), n, fit, lab.ptr,
                                                                   _i64(dst), sc.ptr)

    def slide(stride):
        return lambda net, lab, sc: lib.mbn_net_segment_slide(net.h, d_uni.ptr, n, SH, SW, TILE[0], TILE[1], stride[0], stride[1], lab.ptr, None,
                                                              sc.ptr, 0.0, 0)

    def views(net, lab, sc):
        return lib.mbn_net_segment_views_fit(net.h, d_uni.ptr, n, SH, SW, (C.c_float * 2)(1.0, 0.5), _i32([0, 1]), 2, lab.ptr, None, sc.ptr, 0.0, 0)

    def fit(kind):
        return lambda net, lab, sc: lib.mbn_net_segment_fit(net.h, d_uni.ptr, n, SH, SW, kind, lab.ptr, sc.ptr)

    def to(net, lab, sc):
        return lib.mbn_net_segment_to(net.h, d_canvas.ptr, n, SH, SW, lab.ptr, sc.ptr)

    def outputs():
        return dev(np.full(total, LAB_FILL, np.int32)), dev(np.full(total, SC_FILL, np.float32))

    def written(span):
        m = np.zeros(total, bool)
        for at, count in span:
            m[at:at + count] = True
        return m

    A = new_net(None)
    prev = {}                                       # the previous successful call on A: its label buffer, its labels and its span
    d_rlab, d_rsc = outputs()                       # what the refused calls are given

    def step(what, call, span, color):
        """`call` on A and on a fresh net: the same labels and score bits, nothing past the span; returns (labels, score bits, the fresh net)"""
        got = []
        fresh = new_net(color)
        for net in (A, fresh):
            d_lab, d_sc = outputs()
            assert call(net, d_lab, d_sc) == pkg.OK, (what, ctx.last_error())
            ctx.sync()
            lab, sc = d_lab.download((total,), np.int32), d_sc.download((total,), np.uint32)
            m = written(span)
            assert (lab[~m] == LAB_FILL).all() and (sc[~m].view(np.float32) == SC_FILL).all(), "%s writes past its span" % what
            assert ((lab[m] >= 0) & (lab[m] < CLASSES)).all(), what
            got.append((d_lab, lab, sc))
        assert np.array_equal(got[0][1], got[1][1]), "%s: %d labels differ from the fresh net's" % (what, int((got[0][1] != got[1][1]).sum()))
        assert np.array_equal(got[0][2], got[1][2]), "%s: score bits differ from the fresh net's" % what
        prev.update(d_lab=got[0][0], lab=got[0][1], mask=written(span), what=what)
        return got[0][1], got[0][2], fresh

    def refuse(what, call, status):
        """a refused call writes nothing, and segment_score still counts the maps of the previous successful call"""
        assert call(A, d_rlab, d_rsc) == status, what
        ctx.sync()
        assert (d_rlab.download((total,), np.int32) == LAB_FILL).all() and (d_rsc.download((total,), np.float32) == SC_FILL).all(), \
            "%s: a refused call may not write" % what
        d_counts.upload(np.zeros((CLASSES + 1) ** 2, np.uint64))
        A.segment_score(prev["d_lab"].ptr, d_truth.ptr, 1, d_counts.ptr)
        ctx.sync()
        want = np.zeros((CLASSES + 1, CLASSES + 1), np.uint64)
        m = prev["mask"]
        np.add.at(want, (np.minimum(truth[m], CLASSES).astype(np.int64), prev["lab"][m].astype(np.int64)), 1)
        assert np.array_equal(d_counts.download((CLASSES + 1, CLASSES + 1), np.uint64), want), "%s after %s" % (what, prev["what"])

    def lanczos(net, lab, sc):
        net.set_resize_filter(R.LANCZOS)
        rc = images_fit(pkg.FIT_PAD)(net, lab, sc)
        net.set_resize_filter(R.BILINEAR)
        return rc

    def refusals():
        refuse("a slide with a stride above the tile", slide((65, 64)), pkg.EINVAL)
        refuse("segment_images_fit under LANCZOS", lanczos, pkg.EUNSUPPORTED)
        refuse("segment_fit(CROP)", fit(pkg.FIT_CROP), pkg.EUNSUPPORTED)

    steps = [("1 images_fit(PAD)", images_fit(pkg.FIT_PAD), rag_span, None),
             ("2 slide", slide(STRIDE), uni_span, None),
             ("3 images_fit(PAD) again", images_fit(pkg.FIT_PAD), rag_span, None),
             ("4 images_fit(PAD) in another colour", images_fit(pkg.FIT_PAD), rag_span, COLOR),
             ("5 images_fit(STRETCH)", images_fit(pkg.FIT_STRETCH), rag_span, COLOR),
             ("6 views_fit", views, uni_span, COLOR),
             ("7 fit(PAD)", fit(pkg.FIT_PAD), uni_span, COLOR),
             ("8 segment_to", to, uni_span, COLOR)]
    results, fresh = [], None
    for what, call, span, color in steps:
        if color and A.pad_color() != color:
            A.set_pad_color(*color)
        if fresh:
            drop(fresh)
        lab, sc, fresh = step(what, call, span, color)
        results.append((lab, sc))
        refusals()
    assert np.array_equal(results[0][0], results[2][0]) and np.array_equal(results[0][1], results[2][1]), "steps 1 and 3 are the same call"
    assert not np.array_equal(results[3][1], results[0][1]), "step 4 pads in another colour"
    assert not np.array_equal(results[4][1], results[3][1]), "the two fits are different read-outs"
    # the regions of the last maps: the same count on both nets
    for k, net in enumerate((A, fresh)):
        net.segment_regions(prev["d_lab"].ptr, d_n.ptr + 4 * n * k)
    ctx.sync()
    counts = d_n.download((2, n), np.int32)
    assert (counts[0] > 0).all() and np.array_equal(counts[0], counts[1])
    drop(A)
    drop(fresh)
    for b in bufs:
        b.free()
    hw.free()
