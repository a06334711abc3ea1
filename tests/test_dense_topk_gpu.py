"""Segment with runners-up on the GPU. mbn_resample_topk_f32 / _ragged_f32 against the reference (tests/dense_topk_ref.py): labels and score bits
equal in every case, prob within tolerance = (classes + 200 + 2 |val_j - best|) 2^-24 relative + 2^-125 and exactly 0 where the rule says 0; the
bit equalities with the softmax and argmax read-outs; the threshold on plane 0; the ragged form; every status. The net runner's segment_topk_fit /
_images_fit / _score against segment_prob_fit, segment_score and each other.

Every comparison prints its largest prob error in units of its tolerance before it asserts (pytest -s shows them)."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import dense_topk_ref as T
from test_dense_any_gpu import LAB_FILL, SC_FILL, TAIL, _logits, _ragged_layout
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

PR_FILL = -5.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _run(ctx, x, H, W, k, window=None, offset=0, with_score=True, with_prob=True, min_prob=0.0, ignore=0):
    """mbn_resample_topk_f32 on x [n][h][w][classes], uploaded `offset` bytes into its allocation; window = (in_rows, in_cols, rect) or None.
    (labels, score or None, prob or None), each [k][n][H][W]. The outputs carry a sentinel pattern and TAIL more elements behind the last plane."""
    n, h, w, classes = x.shape
    d_x = ctx.to_device(np.concatenate([np.zeros(offset // 4, np.float32), x.ravel()]))
    npix = k * n * H * W
    d_lab = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32))
    d_sc = ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32)) if with_score else None
    d_pr = ctx.to_device(np.full(npix + TAIL, PR_FILL, np.float32)) if with_prob else None
    R, Cc, rect = window if window else (0, 0, None)
    ctx.resample_topk(d_lab.ptr, d_pr.ptr if d_pr else None, d_sc.ptr if d_sc else None, d_x.ptr + offset, n, h, w, classes, H, W, k, rect=rect,
                      in_rows=R, in_cols=Cc, min_prob=min_prob, ignore_label=ignore)
    ctx.sync()
    lab = d_lab.download((npix + TAIL,), np.int32)
    sc = d_sc.download((npix + TAIL,), np.float32) if d_sc else None
    pr = d_pr.download((npix + TAIL,), np.float32) if d_pr else None
    for b in (d_x, d_lab, d_sc, d_pr):
        if b is not None:
            b.free()
    assert (lab[npix:] == LAB_FILL).all(), "labels written past the last plane"
    assert sc is None or (sc[npix:] == SC_FILL).all(), "scores written past the last plane"
    assert pr is None or (pr[npix:] == PR_FILL).all(), "probabilities written past the last plane"
    shape = (k, n, H, W)
    return lab[:npix].reshape(shape), None if sc is None else sc[:npix].reshape(shape), None if pr is None else pr[:npix].reshape(shape)


def _compare(got, want, classes, what):
    """got = (labels, score, prob) of the kernel (score / prob may be None), want = the reference's, at least as many planes"""
    lab, sc, pr = got
    k = lab.shape[0]
    want_lab, want_sc, want_pr = (a[:k] for a in want)      # the prefix property (tests/test_dense_topk_cpu.py checks the reference's own)
    bad = int((lab != want_lab).sum())
    assert bad == 0, "%s: %d of %d labels differ from the reference" % (what, bad, lab.size)
    if sc is not None:
        bad = int((_bits(sc) != _bits(want_sc)).sum())
        assert bad == 0, "%s: %d of %d score bit patterns differ from the reference" % (what, bad, sc.size)
    if pr is not None:
        tol = T.tolerance(classes, want_sc, want_pr)
        err = np.abs(pr.astype(np.float64) - want_pr)
        zero = tol == 0
        worst = float((err[~zero] / tol[~zero]).max()) if (~zero).any() else 0.0
        print("%s: max prob error %.3f of its tolerance, %d values, %d that must be 0" % (what, worst, pr.size, int(zero.sum())))
        assert (pr[zero] == 0).all(), "%s: a nonzero prob where best is not finite or the slot is unfilled" % what
        assert worst <= 1.0, "%s: prob error %.3f of the tolerance" % (what, worst)
        assert (pr >= 0).all() and (pr <= 1).all()


def _check(ctx, x, H, W, k, what, want=None, **kw):
    want = want or T.resample_topk(x, H, W, k, window=kw.get("window"))
    got = _run(ctx, x, H, W, k, **kw)
    _compare(got, want, x.shape[3], what)
    return got, want


# ------------------------------------------------------------------------------------------------------------- against the reference

X7 = functools.lru_cache(None)(lambda: _logits(2, 3, 3, 7, seed=41))


@functools.lru_cache(None)
def _want7():
    return T.resample_topk(X7(), 13, 17, 7)


@pytest.mark.parametrize("k", [1, 2, 5, 7])
def test_dword_path(pkg, ctx, k):
    """7 classes: dword loads and a NaN padding class, which must not enter even at k = classes"""
    (lab, sc, pr), _ = _check(ctx, X7(), 13, 17, k, "3x3x7 -> 13x17 k %d" % k, want=_want7())
    assert (lab >= 0).all() and (lab < 7).all() and np.isfinite(sc).all()
    assert np.allclose(pr.sum(axis=0), 1.0, atol=1e-5) if k == 7 else (pr.sum(axis=0) < 1).all()


@functools.lru_cache(None)
def _chunk_case(classes):
    x = _logits(1, 5, 4, classes, seed=classes)
    return x, T.resample_topk(x, 45, 37, 8)


@pytest.mark.parametrize("k", [5, 8])
@pytest.mark.parametrize("classes", [1000, 1001])
def test_slots_fill_across_chunks(pkg, ctx, classes, k):
    x, want = _chunk_case(classes)
    got, _ = _check(ctx, x, 45, 37, k, "5x4x%d -> 45x37 k %d" % (classes, k), want=want)
    assert len({int(v) // 128 for v in want[0][:k, 0, 20, 20]}) > 1, "the slots of a pixel come from different chunks"
    if classes == 1000:                                     # an interior pointer 4 bytes off 16: the dword path gives the bytes of the 16-byte path
        off = _run(ctx, x, 45, 37, k, offset=4)
        for a, b in zip(got, off):
            assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("H,W", [(32, 32), (33, 35)])
def test_ratio_4(pkg, ctx, H, W):
    """8 x 8 -> 32 x 32: the 10 x 10 footprint and the 64-class chunk; 33 x 35: partial second tiles"""
    assert pkg.resample_plan(8, 8, H, W).ch == 64
    x = _logits(2, 8, 8, 130, seed=H + W)
    _check(ctx, x, H, W, 5, "8x8x130 -> %dx%d" % (H, W))


def test_values(pkg, ctx):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    n, h, w, classes, H, W, k = 2, 3, 3, 133, 13, 17, 8
    (lab, sc, pr), _ = _check(ctx, np.full((n, h, w, classes), 0.5, np.float32), H, W, k, "constant")
    assert all((lab[j] == j).all() for j in range(k))                                        # equal values: ascending class order
    x = np.zeros((n, h, w, classes), np.float32)
    x[..., [5, 70, 131]] = 2.0                                                               # two values, the high one in two chunks
    (lab, sc, pr), _ = _check(ctx, x, H, W, k, "two-valued")
    assert [int(lab[j, 0, 0, 0]) for j in range(k)] == [5, 70, 131, 0, 1, 2, 3, 4]
    c = np.arange(1001, dtype=np.float32)
    for name, ramp in (("ascending", c), ("descending", c[::-1])):                           # ascending: every class is inserted at rank 0
        x = np.broadcast_to(ramp * np.float32(0.25), (1, 2, 2, 1001)).astype(np.float32)
        (lab, sc, pr), _ = _check(ctx, x, 11, 9, k, "%s ramp" % name)
        want = 1000 - np.arange(k) if name == "ascending" else np.arange(k)
        assert all((lab[j] == want[j]).all() for j in range(k))
    x = _logits(n, h, w, classes, seed=5)
    rng = np.random.default_rng(6)
    for v, share in ((nan, 0.03), (inf, 0.002), (-inf, 0.03)):                                # few +inf: most pixels keep a finite best
        x[rng.random(x.shape) < share] = v
    (lab, sc, pr), _ = _check(ctx, x, H, W, k, "sprinkled NaN and inf")
    assert np.isposinf(sc[0]).any() and (pr[:, np.isposinf(sc[0])] == 0).all() and (pr[0][np.isfinite(sc[0])] > 0).all()
    assert np.isfinite(sc[0]).sum() > sc[0].size // 8
    x = np.full((n, h, w, classes), nan, np.float32)                                         # fewer real classes than k
    x[..., [3, 129, 60]] = _logits(n, h, w, 3, seed=7)
    (lab, sc, pr), _ = _check(ctx, x, H, W, k, "three real classes")
    assert (lab[:3] >= 0).all() and (lab[3:] == -1).all() and (sc[3:] == -inf).all() and (pr[3:] == 0).all() and (pr[:3] > 0).all()
    (lab, sc, pr), _ = _check(ctx, np.full((n, h, w, classes), nan, np.float32), H, W, k, "every class NaN")
    assert (lab[0] == 0).all() and (lab[1:] == -1).all() and (sc == -inf).all() and (pr == 0).all()


# ------------------------------------------------------------------------------------------------------------------- bit equalities

def test_equalities(pkg, ctx):
    n, h, w, classes, H, W = 2, 5, 7, 64, 37, 61
    x = _logits(n, h, w, classes, seed=9)
    d_x = ctx.to_device(x)
    npix = n * H * W
    outs = [ctx.to_device(np.full(npix, LAB_FILL, np.int32)) for _ in range(3)]
    ctx.resample_softmax(outs[0].ptr, outs[2].ptr, outs[1].ptr, d_x.ptr, n, h, w, classes, H, W)
    ctx.sync()
    soft = [b.download((npix,), np.uint32) for b in outs]
    ctx.resample_argmax(outs[0].ptr, outs[1].ptr, d_x.ptr, n, h, w, classes, H, W)
    ctx.sync()
    arg = [b.download((npix,), np.uint32) for b in outs[:2]]
    for b in outs + [d_x]:
        b.free()
    one = _run(ctx, x, H, W, 1)
    for name, a, b in zip(("labels", "score", "prob"), one, soft):
        assert np.array_equal(_bits(a).ravel(), b), "k = 1 %s differ from mbn_resample_softmax_f32" % name
    eight = _run(ctx, x, H, W, 8)
    logit = _run(ctx, x, H, W, 8, with_prob=False)
    assert logit[2] is None
    for name, a, b in zip(("labels", "score"), logit, arg):
        assert np.array_equal(_bits(a[0]).ravel(), b), "the logit form's plane 0 %s differ from mbn_resample_argmax_f32" % name
        assert np.array_equal(_bits(a), _bits(eight[0 if name == "labels" else 1])), "the logit form's %s differ from the prob form's" % name
    full = _run(ctx, x, H, W, 8, window=(160, 224, (0, 0, 224, 160)))
    three = _run(ctx, x, H, W, 3)
    for name, a, b, c in zip(("labels", "score", "prob"), eight, full, three):
        assert np.array_equal(_bits(a), _bits(b)), "a full-input rect %s differ from rect = NULL" % name
        assert np.array_equal(_bits(a[:3]), _bits(c)), "the planes of k = 3 differ from the first three of k = 8 (%s)" % name
    window = (160, 224, (56, 0, 112, 160))                  # a true window against the reference, and its plane 0 against the window softmax call
    got, _ = _check(ctx, x, 40, 56, 5, "window", window=window)
    d_x = ctx.to_device(x)
    m = n * 40 * 56
    outs = [ctx.to_device(np.full(m, LAB_FILL, np.int32)) for _ in range(3)]
    ctx.resample_softmax_window(outs[0].ptr, outs[2].ptr, outs[1].ptr, d_x.ptr, n, h, w, classes, 160, 224, window[2], 40, 56)
    ctx.sync()
    for name, a, b in zip(("labels", "score", "prob"), got, outs):
        assert np.array_equal(_bits(a[0]).ravel(), b.download((m,), np.uint32)), "plane 0 %s differ from mbn_resample_softmax_window_f32" % name
    for b in outs + [d_x]:
        b.free()


def test_threshold(pkg, ctx):
    """only plane-0 labels change, on the stored prob, strict"""
    x = (3.0 * np.random.default_rng(101).standard_normal((2, 5, 7, 21))).astype(np.float32)
    H, W, k, ignore = 37, 61, 5, -9
    lab0, sc0, pr0 = _run(ctx, x, H, W, k)
    cut = float(np.median(pr0[0]))                                                           # a stored value: the compare is strict at it
    lab, sc, pr = _run(ctx, x, H, W, k, min_prob=cut, ignore=ignore)
    assert np.array_equal(_bits(pr), _bits(pr0)) and np.array_equal(_bits(sc), _bits(sc0)), "prob and score are written unchanged"
    assert np.array_equal(lab[1:], lab0[1:]), "the planes >= 1 are written unchanged"
    assert np.array_equal(lab[0], np.where(pr0[0] < np.float32(cut), ignore, lab0[0]))
    assert (lab[0] == ignore).any() and (lab[0][pr0[0] == np.float32(cut)] != ignore).all()
    lab_n, _, _ = _run(ctx, x, H, W, k, with_score=False, with_prob=False, min_prob=cut, ignore=ignore)      # thresholded labels alone
    assert np.array_equal(lab_n, lab)


# ---------------------------------------------------------------------------------------------------------------------------- ragged

H5, W7, R5, C7 = 5, 7, 160, 224
RAGGED_PLAIN = [(37, 61), (100, 30), (20, 28)]              # one under 32 wide
RAGGED_WINDOW = [(37, 61, (0, 0, C7, R5)), (100, 30, (9, 11, 180, 120)), (40, 56, (56, 0, 112, 160))]
FILLS = (LAB_FILL, SC_FILL, PR_FILL)


def _ragged_outputs(ctx, elements):
    return [ctx.to_device(np.full(elements, f, np.int32 if f == LAB_FILL else np.float32)) for f in FILLS]


def _ragged_compare(ctx, x, items, offs, got, k, stride, window):
    """every plane of every image equal to the uniform call on it alone (itself checked against the reference); the sentinel elsewhere"""
    touched = np.zeros(got[0].size, bool)
    for i, (it, off) in enumerate(zip(items, offs)):
        H, W = it[0], it[1]
        one, _ = _check(ctx, x[i:i + 1], H, W, k, "ragged item %d alone" % i, window=(R5, C7, it[2]) if window else None)
        for j in range(k):
            at = j * stride + off
            for name, a, b in zip(("labels", "scores", "probabilities"), got, one):
                assert np.array_equal(_bits(a[at:at + H * W]), _bits(b[j].ravel())), "item %d rank %d %s" % (i, j, name)
            touched[at:at + H * W] = True
    for a, f in zip(got, FILLS):
        assert (a[~touched] == f).all(), "written between the maps, between the planes or behind them"


def test_ragged(pkg, ctx):
    classes, k = 21, 5
    x = _logits(3, H5, W7, classes, seed=79)
    d_x = ctx.to_device(x)
    rd = pkg.RaggedReadout(ctx, 3)
    lib = ctx.lib
    offs, total = _ragged_layout(RAGGED_PLAIN, order=(2, 0, 1))                              # out of order, with gaps; `total` includes the tail
    stride = total + 11                                                                      # ... and a gap between the planes
    elements = (k - 1) * stride + total
    rd.set(H5, W7, classes, [(o, H, W) for o, (H, W) in zip(offs, RAGGED_PLAIN)])
    outs = _ragged_outputs(ctx, elements)
    rd.resample_topk(outs[0].ptr, outs[2].ptr, outs[1].ptr, d_x.ptr, k, stride)
    ctx.sync()
    got = [b.download((elements,), np.int32 if b is outs[0] else np.float32) for b in outs]
    _ragged_compare(ctx, x, RAGGED_PLAIN, offs, got, k, stride, window=False)
    # the same launch captured as one kernel node and replayed: the same bits
    cap = _ragged_outputs(ctx, elements)
    g = C.c_void_p()
    assert lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = lib.mbn_resample_topk_ragged_f32(rd.h, cap[0].ptr, cap[2].ptr, cap[1].ptr, d_x.ptr, k, stride, 0.0, 0, None)
    assert lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert (cap[0].download((elements,), np.int32) == LAB_FILL).all(), "the captured call ran"
    assert lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    for a, b in zip(cap, got):
        assert np.array_equal(_bits(a.download((elements,), b.dtype)), _bits(b))
    # a window set on the same handle
    woffs, wtotal = _ragged_layout([(H, W) for H, W, _ in RAGGED_WINDOW], order=(1, 2, 0), gap=6)
    wstride = wtotal
    welements = (k - 1) * wstride + wtotal
    rd.set_window(H5, W7, classes, R5, C7, [(o, H, W, rect) for o, (H, W, rect) in zip(woffs, RAGGED_WINDOW)])
    wouts = _ragged_outputs(ctx, welements)
    rd.resample_topk(wouts[0].ptr, wouts[2].ptr, wouts[1].ptr, d_x.ptr, k, wstride)
    ctx.sync()
    wgot = [b.download((welements,), np.int32 if b is wouts[0] else np.float32) for b in wouts]
    _ragged_compare(ctx, x, RAGGED_WINDOW, woffs, wgot, k, wstride, window=True)
    # the launch captured under the plain set, replayed after the window set, writes nothing
    for b, f in zip(cap, FILLS):
        b.upload(np.full(elements, f, np.int32 if f == LAB_FILL else np.float32))
    assert lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    for b, f in zip(cap, FILLS):
        assert (b.download((elements,), np.int32 if f == LAB_FILL else np.float32) == f).all(), "a replay after a later set wrote"
    assert lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    # the statuses of the ragged launch: nothing is written
    for b, f in zip(wouts, FILLS):
        b.upload(np.full(welements, f, np.int32 if f == LAB_FILL else np.float32))
    call = lambda l, p, s, q, kk, st, m=0.0: lib.mbn_resample_topk_ragged_f32(rd.h, l, p, s, q, kk, st, m, 0, None)
    lab, sc, pr = (b.ptr for b in wouts)
    span = rd.ctx.lib.mbn_ragged_readout_span(rd.h)
    assert call(lab, pr, sc, d_x.ptr, 0, wstride) == pkg.EINVAL and call(lab, pr, sc, d_x.ptr, 9, wstride) == pkg.EINVAL
    assert call(lab, pr, sc, d_x.ptr, k, span - 1) == pkg.EINVAL                             # the planes would overlap
    assert call(lab, pr, sc, d_x.ptr, k, span) == pkg.OK
    assert call(lab, pr, sc, d_x.ptr, k, wstride, 1.5) == pkg.EINVAL and call(lab, pr, sc, d_x.ptr, k, wstride, float("nan")) == pkg.EINVAL
    assert call(None, pr, sc, d_x.ptr, k, wstride) == pkg.EINVAL and call(lab, pr + 2, sc, d_x.ptr, k, wstride) == pkg.EINVAL
    assert call(lab, pr, sc, d_x.ptr, k, wstride + TAIL) == pkg.EINVAL                       # the last plane would end past the tracked buffers
    assert call(lab, pr, sc, d_x.ptr, 8, (1 << 37) + 1) == pkg.EUNSUPPORTED
    fresh = pkg.RaggedReadout(ctx, 2)
    assert lib.mbn_resample_topk_ragged_f32(fresh.h, lab, pr, sc, d_x.ptr, k, wstride, 0.0, 0, None) == pkg.EINVAL      # no set yet
    fresh.close()
    rd.close()
    for b in [d_x] + outs + cap + wouts:
        b.free()


# -------------------------------------------------------------------------------------------------------------------------- statuses

def test_statuses(pkg, ctx):
    x = ctx.to_device(np.zeros(2 * 2 * 21, np.float32))
    k = 3
    fill = np.full(k * 16 * 16, LAB_FILL, np.int32)
    lab, sc, pr = ctx.to_device(fill), ctx.to_device(fill.astype(np.float32)), ctx.to_device(fill.astype(np.float32))
    lib = ctx.lib
    rect_t = lambda *v: (C.c_int32 * 4)(*v)

    def topk(l, p, s, q, n=1, h=2, w=2, c=21, R=0, Cc=0, rect=None, H=16, W=16, kk=k, m=0.0):
        return lib.mbn_resample_topk_f32(ctx.h, l, p, s, q, n, h, w, c, R, Cc, rect, H, W, kk, m, 0, None)

    for kk in (0, -1, 9, 22):
        assert topk(lab.ptr, pr.ptr, sc.ptr, x.ptr, kk=kk) == pkg.EINVAL, kk                 # outside 1..8, above the classes
    assert topk(lab.ptr, pr.ptr, sc.ptr, x.ptr, c=2) == pkg.EINVAL                            # k = 3 > classes = 2
    for bad in (float("nan"), -0.1, 1.5):
        assert topk(lab.ptr, pr.ptr, sc.ptr, x.ptr, m=bad) == pkg.EINVAL and topk(lab.ptr, None, sc.ptr, x.ptr, m=bad) == pkg.EINVAL
    assert topk(None, pr.ptr, sc.ptr, x.ptr) == pkg.EINVAL and topk(lab.ptr, pr.ptr, sc.ptr, None) == pkg.EINVAL
    assert topk(lab.ptr, pr.ptr + 2, sc.ptr, x.ptr) == pkg.EINVAL and topk(lab.ptr, pr.ptr, sc.ptr + 2, x.ptr) == pkg.EINVAL
    # the envelope of the same form: the softmax call's status on the same shape
    for s in [dict(H=7), dict(W=7), dict(H=16385), dict(n=0), dict(h=0), dict(c=0), dict(W=-1), dict(n=65536)]:
        a = dict(n=1, h=2, w=2, c=21, H=16, W=16)
        a.update(s)
        want = lib.mbn_resample_softmax_f32(ctx.h, lab.ptr, pr.ptr, sc.ptr, x.ptr, a["n"], a["h"], a["w"], a["c"], a["H"], a["W"], 0.0, 0, None)
        assert want != pkg.OK and topk(lab.ptr, pr.ptr, sc.ptr, x.ptr, **s) == want, s
    full = rect_t(0, 0, 64, 64)
    for s in [dict(H=7), dict(rect=rect_t(1, 0, 64, 64)), dict(R=16385), dict(R=1, rect=rect_t(0, 0, 1, 1))]:
        a = dict(R=64, Cc=64, rect=full, H=16, W=16)
        a.update(s)
        want = lib.mbn_resample_softmax_window_f32(ctx.h, lab.ptr, pr.ptr, sc.ptr, x.ptr, 1, 2, 2, 21, a["R"], a["Cc"], a["rect"], a["H"], a["W"], 0.0, 0, None)
        assert want != pkg.OK and topk(lab.ptr, pr.ptr, sc.ptr, x.ptr, **a) == want, s
    # undersized tracked buffers: each output spans k planes; the logits one map
    two = ctx.to_device(np.zeros(2 * 16 * 16, np.float32))                                   # two planes where three are written
    assert topk(two.ptr, pr.ptr, sc.ptr, x.ptr) == pkg.EINVAL and topk(lab.ptr, two.ptr, sc.ptr, x.ptr) == pkg.EINVAL
    assert topk(lab.ptr, pr.ptr, two.ptr, x.ptr) == pkg.EINVAL and topk(lab.ptr, pr.ptr, sc.ptr, x.ptr, n=2, H=8) == pkg.EINVAL
    ctx.sync()
    for b in (lab, sc, pr):
        assert np.array_equal(b.download(fill.shape, np.int32 if b is lab else np.float32), fill), "nothing may have been launched"
    assert topk(two.ptr, pr.ptr, sc.ptr, x.ptr, kk=2) == pkg.OK                              # ... and two planes fit the smaller buffer
    # the logit form: no prob map, no threshold; score NULL too. All-zero logits: labels 0, 1, 2
    assert topk(lab.ptr, None, None, x.ptr) == pkg.OK
    ctx.sync()
    got = lab.download((k, 16, 16), np.int32)
    assert all((got[j] == j).all() for j in range(k))
    for b in (x, lab, sc, pr, two):
        b.free()


# --------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS, BATCH = 0.25, 21, 64, 64, 3
SOURCE = (75, 130)


def test_net_segment_topk(pkg, ctx, tmp_path):
    n, k = BATCH, 5
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, 32)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    lib = ctx.lib
    rng = np.random.default_rng(31)
    sh, sw = SOURCE
    npix = n * sh * sw
    src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    truth = rng.integers(0, CLASSES + 2, npix).astype(np.uint8)
    truth[truth >= CLASSES] = 255
    d_src, d_truth = ctx.to_device(src), ctx.to_device(truth)
    d_lab, d_pr, d_sc = ctx.to_device(np.full(k * npix + TAIL, LAB_FILL, np.int32)), ctx.alloc(k * npix * 4), ctx.alloc(k * npix * 4)
    d_plab, d_ppr = ctx.alloc(npix * 4), ctx.alloc(npix * 4)
    cells, rcells = (CLASSES + 1) ** 2, (CLASSES + 1) * (k + 1)
    d_counts, d_ranks = ctx.alloc(cells * 8), ctx.alloc(rcells * 8)
    topk_fit = lambda fit, kk=k, m=0.0: lib.mbn_net_segment_topk_fit(net.h, d_src.ptr, n, sh, sw, fit, kk, d_lab.ptr, d_pr.ptr, d_sc.ptr, m, 0)
    assert topk_fit(pkg.FIT_PAD) == pkg.EINVAL                                               # no uint8 images yet
    net.set_input_u8(True)
    assert topk_fit(pkg.FIT_CROP) == pkg.EUNSUPPORTED and topk_fit(7) == pkg.EINVAL
    assert topk_fit(pkg.FIT_PAD, kk=0) == pkg.EINVAL and topk_fit(pkg.FIT_PAD, kk=9) == pkg.EINVAL and topk_fit(pkg.FIT_PAD, m=1.5) == pkg.EINVAL
    assert lib.mbn_net_segment_topk_score(net.h, d_lab.ptr, d_truth.ptr, 1, d_ranks.ptr) == pkg.EINVAL      # no segment call yet
    ctx.sync()
    assert (d_lab.download((k * npix + TAIL,), np.int32) == LAB_FILL).all()

    def counts_after(score, buf, size):
        assert lib.mbn_memset(ctx.h, buf.ptr, 0, size * 8) == pkg.OK
        score()
        ctx.sync()
        return buf.download((size,), np.uint64)

    for fit in (pkg.FIT_STRETCH, pkg.FIT_PAD):
        net.segment_prob_fit(d_src.ptr, n, sh, sw, fit, d_plab.ptr, d_ppr.ptr)
        want_counts = counts_after(lambda: net.segment_score(d_plab.ptr, d_truth.ptr, 1, d_counts.ptr), d_counts, cells)
        assert lib.mbn_net_segment_topk_score(net.h, d_plab.ptr, d_truth.ptr, 1, d_ranks.ptr) == pkg.EINVAL  # the last call was not a top-k call
        ctx.sync()
        plab, ppr = d_plab.download((npix,), np.uint32), d_ppr.download((npix,), np.uint32)
        net.segment_topk_fit(d_src.ptr, n, sh, sw, fit, k, d_lab.ptr, d_pr.ptr, d_sc.ptr)
        counts = counts_after(lambda: net.segment_score(d_lab.ptr, d_truth.ptr, 1, d_counts.ptr), d_counts, cells)
        ranks = counts_after(lambda: net.segment_topk_score(d_lab.ptr, d_truth.ptr, 1, d_ranks.ptr), d_ranks, rcells)
        lab, pr = d_lab.download((k * npix + TAIL,), np.uint32), d_pr.download((k * npix,), np.uint32)
        assert (lab[k * npix:].view(np.int32) == LAB_FILL).all()
        assert np.array_equal(lab[:npix], plab) and np.array_equal(pr[:npix], ppr), "fit %d: plane 0 differs from segment_prob_fit" % fit
        assert np.array_equal(counts, want_counts), "fit %d: segment_score after the top-k call" % fit
        ranks = ranks.reshape(CLASSES + 1, k + 1)
        assert np.array_equal(ranks[:, 0], counts.reshape(CLASSES + 1, CLASSES + 1).diagonal() * (np.arange(CLASSES + 1) < CLASSES))
        assert np.array_equal(ranks, T.rank_table(lab[:k * npix].view(np.int32).reshape(k, npix), truth, CLASSES)) and ranks.sum() == npix
        # the images form on equal-size images: the uniform form's bytes
        d_ilab, d_ipr = ctx.to_device(np.full(k * npix, LAB_FILL, np.int32)), ctx.alloc(k * npix * 4)
        one = sh * sw
        net.segment_topk_images_fit(d_src.ptr, [i * one * 3 for i in range(n)], [sh] * n, [sw] * n, fit, k, npix, d_ilab.ptr,
                                    [i * one for i in range(n)], d_ipr.ptr, None)
        iranks = counts_after(lambda: net.segment_topk_score(d_ilab.ptr, d_truth.ptr, 1, d_ranks.ptr), d_ranks, rcells)
        assert np.array_equal(d_ilab.download((k * npix,), np.uint32), lab[:k * npix]) and np.array_equal(d_ipr.download((k * npix,), np.uint32), pr)
        assert np.array_equal(iranks.reshape(CLASSES + 1, k + 1), ranks)
        d_ilab.free()
        d_ipr.free()
    # a refused image call (the planes overlap) leaves the record of the call before
    args = (net.h, d_src.ptr, (C.c_int64 * n)(*[i * sh * sw * 3 for i in range(n)]), (C.c_int32 * n)(*[sh] * n), (C.c_int32 * n)(*[sw] * n), n,
            pkg.FIT_PAD, k, npix - 1, d_lab.ptr, (C.c_int64 * n)(*[i * sh * sw for i in range(n)]), d_pr.ptr, None, 0.0, 0)
    assert lib.mbn_net_segment_topk_images_fit(*args) == pkg.EINVAL
    net.destroy()
    for b in (d_src, d_truth, d_lab, d_pr, d_sc, d_plab, d_ppr, d_counts, d_ranks):
        b.free()


# ------------------------------------------------------------------------------------------------------------------------ the C host

def _pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    assert m, raw[:32]
    width, height, maxval = (int(g) for g in m.groups())
    return np.frombuffer(raw[m.end():], ">u2" if maxval > 255 else np.uint8).astype(np.int32).reshape(height, width), maxval


def test_c_host_segment_topk(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    seed, alpha, os_, sh, sw, rows, cols, k, classes = 3, 0.5, 16, 75, 130, 64, 96, 3, 1000
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, out, conf, tr = (str(tmp_path / f) for f in ("a.ppm", "out.pgm", "conf.pgm", "truth.pgm"))
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", str(seed), "--alpha", str(alpha), "--res", "%dx%d" % (rows, cols), "--output-stride", str(os_), "--ppm", ppm, "--fit", "pad"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
    for extra in (["--segment-topk", "3"], ["--segment-source", out, "--segment-topk", "0"], ["--segment-source", out, "--segment-topk", "9"],
                  ["--segment-source", out, "--segment-topk", "3", "--regions"]):
        r = run(extra)
        assert r.returncode == 2 and not os.path.exists(out), (extra, r.stdout + r.stderr)
    # the same through the mirror
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(rows, cols), lib=pkg.load(), output_stride=os_)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 1)
    net.set_input_u8(True)
    d_src, d_lab, d_pr = ctx.to_device(src), ctx.alloc(k * sh * sw * 4), ctx.alloc(k * sh * sw * 4)
    net.segment_topk_fit(d_src.ptr, 1, sh, sw, pkg.FIT_PAD, k, d_lab.ptr, d_pr.ptr)
    ctx.sync()
    want_lab, want_pr = d_lab.download((k, sh, sw), np.int32), d_pr.download((k, sh, sw), np.float32)
    net.destroy()
    for b in (d_src, d_lab, d_pr):
        b.free()
    hw.free()
    truth = want_lab[0].copy()                              # top-1 right on the left half, top-2 right on the right half, a void column
    truth[:, sw // 2:] = want_lab[1][:, sw // 2:]
    truth[:, 0] = 65535
    with open(tr, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (sw, sh) + truth.astype(">u2").tobytes())
    r = run(["--segment-source", out, "--segment-topk", str(k), "--segment-confidence", conf, "--truth", tr])
    assert r.returncode == 0, r.stdout + r.stderr
    for j in range(k):
        name = lambda p: p if j == 0 else p.replace(".pgm", ".rank%d.pgm" % j)
        got, maxval = _pgm(name(out))
        assert maxval == (classes - 1 if j == 0 else classes) and np.array_equal(got, want_lab[j]), "rank %d labels" % j
        got, maxval = _pgm(name(conf))
        assert maxval == 255 and np.array_equal(got, np.floor(want_pr[j].astype(np.float64) * 255.0 + 0.5).astype(np.int32)), "rank %d confidence" % j
    line = [l for l in r.stdout.splitlines() if l.startswith("topk: ")]
    assert len(line) == 1, r.stdout
    f = dict(p.split("=") for p in line[0].split()[1:])
    ranks = T.rank_table(want_lab.reshape(k, -1), truth.ravel(), classes)
    acc, mean, valid = pkg.topk_metrics(ranks, classes, k)
    assert int(f["k"]) == k and float(f["valid"]) == valid == sh * (sw - 1)
    for j in range(k):
        assert float(f["top%d_acc" % (j + 1)]) == acc[j] and float(f["top%d_mean_acc" % (j + 1)]) == mean[j]
    assert 0 < acc[0] < acc[1] == 1.0
