"""Rank score on the GPU. mbn_topk_rank_i32 / _ragged_i32 against the numpy form (tests/dense_topk_ref.py): the same table, byte for byte, for both
forms of the kernel, both truth types with void values, interior pointers, accumulating calls, every planning CU count and a graph replay;
column 0 against the diagonal of mbn_confusion_i32 on plane 0; the ragged form against the per-item uniform calls; every status."""
import ctypes as C

import numpy as np
import pytest

import dense_topk_ref as T

pytestmark = pytest.mark.gpu


def _case(count, classes, k, dtype, seed, stride=None):
    """k label planes in which the truth turns up at every rank and not at all, with ignore labels (255 in plane 0) and unfilled slots (-1)"""
    rng = np.random.default_rng(seed)
    stride = stride or count
    truth = rng.integers(0, classes, count)
    planes = rng.integers(0, classes, (k, stride)).astype(np.int32)
    rank = rng.integers(0, k + 2, count)                    # k: in no plane (unless by chance), k + 1: void
    for j in range(k):
        planes[j, :count][rank == j] = truth[rank == j]
    planes[0, :count][rng.random(count) < 0.05] = 255       # the ignore label of a thresholded plane 0
    if k > 1:
        planes[k - 1, :count][rng.random(count) < 0.1] = -1
    truth = truth.astype(dtype)
    void = rank == k + 1
    truth[void] = 255 if dtype == np.uint8 else rng.choice(np.array([255, -1, classes, 2 ** 31 - 1]), int(void.sum())).astype(dtype)
    return planes, truth


def _device(ctx, planes, truth, classes, count, stride, lab_off=0, tr_off=0, calls=1):
    k = planes.shape[0]
    d_lab = ctx.to_device(np.concatenate([np.zeros(lab_off, np.int32), planes.ravel()]))
    d_tr = ctx.to_device(np.concatenate([np.zeros(tr_off, truth.dtype), truth]))
    d_ranks = ctx.to_device(np.zeros((classes + 1) * (k + 1), np.uint64))
    for _ in range(calls):
        ctx.topk_rank(d_ranks.ptr, d_lab.ptr + 4 * lab_off, k, stride, d_tr.ptr + truth.itemsize * tr_off, truth.itemsize, classes, count)
    ctx.sync()
    got = d_ranks.download((classes + 1, k + 1), np.uint64)
    for b in (d_lab, d_tr, d_ranks):
        b.free()
    return got


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
@pytest.mark.parametrize("k", [1, 5, 8])
@pytest.mark.parametrize("count", [1, 1000, 3 * 37 * 41])
def test_against_numpy(pkg, ctx, count, k, dtype):
    classes = 21
    planes, truth = _case(count, classes, k, dtype, seed=count + k)
    want = T.rank_table(planes, truth, classes)
    got = _device(ctx, planes, truth, classes, count, count)
    assert np.array_equal(got, want) and got.sum() == count
    if count > 1:
        assert (want[:classes].sum(axis=0) > 0).all() and want[classes, k] > 0, "every column and the void row are exercised"
    # column 0 is the diagonal of the confusion matrix of plane 0
    d_lab, d_tr = ctx.to_device(planes[0]), ctx.to_device(truth)
    d_counts = ctx.to_device(np.zeros((classes + 1) ** 2, np.uint64))
    ctx.confusion(d_counts.ptr, d_lab.ptr, d_tr.ptr, truth.itemsize, classes, count)
    ctx.sync()
    diag = d_counts.download((classes + 1, classes + 1), np.uint64).diagonal()
    assert np.array_equal(got[:classes, 0], diag[:classes]) and got[classes, 0] == 0
    for b in (d_lab, d_tr, d_counts):
        b.free()


@pytest.mark.parametrize("k", [1, 8])
def test_both_sides_of_the_form_switch(pkg, ctx, k):
    last = 49152 // (4 * (k + 1)) - 1                       # the largest table that a workgroup counts in LDS
    last = min(last, pkg.CONFUSION_MAX_CLASSES - 1)         # (k = 1: every class count of the envelope fits)
    count = 5000
    for classes in (last, last + 1):
        assert pkg.topk_rank_form(classes, k) == (pkg.CONFUSION_FORM_LDS if classes == last or k == 1 else pkg.CONFUSION_FORM_GLOBAL)
        planes, truth = _case(count, classes, k, np.int32, seed=classes)
        assert np.array_equal(_device(ctx, planes, truth, classes, count, count), T.rank_table(planes, truth, classes))
    planes, truth = _case(count, 4096, 8, np.int32, seed=3)  # the global form at the envelope's last class count
    assert np.array_equal(_device(ctx, planes, truth, 4096, count, count), T.rank_table(planes, truth, 4096))


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_interior_pointers_strides_and_accumulation(pkg, ctx, dtype):
    classes, k, count = 21, 5, 1000
    planes, truth = _case(count, classes, k, dtype, seed=7, stride=count + 13)              # a gap between the planes
    want = T.rank_table(planes[:, :count], truth, classes)
    for lab_off, tr_off in [(0, 0), (1, 1), (3, 2), (2, 3)]:
        assert np.array_equal(_device(ctx, planes, truth, classes, count, count + 13, lab_off, tr_off), want), (lab_off, tr_off)
    assert np.array_equal(_device(ctx, planes, truth, classes, count, count + 13, calls=2), 2 * want), "two calls accumulate"


def test_planning_cus_and_replay_give_the_same_bytes(pkg, ctx):
    classes, k, count = 21, 5, 3 * 37 * 41
    planes, truth = _case(count, classes, k, np.uint8, seed=11)
    want = T.rank_table(planes, truth, classes)
    try:
        for cus in (1, 3, 0):
            ctx.set_planning_cus(cus)
            assert np.array_equal(_device(ctx, planes, truth, classes, count, count), want), "planning CU count %d" % cus
    finally:
        ctx.set_planning_cus(0)
    d_lab, d_tr = ctx.to_device(planes), ctx.to_device(truth)
    d_ranks = ctx.to_device(np.zeros((classes + 1) * (k + 1), np.uint64))
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_topk_rank_i32(ctx.h, d_ranks.ptr, d_lab.ptr, k, count, d_tr.ptr, 1, classes, count, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    for _ in range(2):
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(d_ranks.download((classes + 1, k + 1), np.uint64), 2 * want)
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    for b in (d_lab, d_tr, d_ranks):
        b.free()


@pytest.mark.parametrize("window", [False, True])
def test_ragged_equals_the_uniform_calls(pkg, ctx, window):
    classes, k = 21, 5
    sizes = [(37, 41), (20, 28), (100, 30)]
    offs, at = [0] * 3, 3
    for i in (2, 0, 1):                                     # out of order, with gaps
        offs[i] = at
        at += sizes[i][0] * sizes[i][1] + 5
    span = max(o + r * c for o, (r, c) in zip(offs, sizes))
    stride = span + 9
    rng = np.random.default_rng(13)
    planes = rng.integers(0, classes, (k, stride)).astype(np.int32)
    truth = rng.integers(0, classes + 3, span).astype(np.uint8)
    hit = rng.random(span) < 0.4
    planes[1, :span][hit] = truth[hit]
    rd = pkg.RaggedReadout(ctx, 3)
    if window:
        rd.set_window(5, 7, classes, 160, 224, [(o, r, c, (0, 0, 224, 160)) for o, (r, c) in zip(offs, sizes)])
    else:
        rd.set(5, 7, classes, [(o, r, c) for o, (r, c) in zip(offs, sizes)])
    d_lab, d_tr = ctx.to_device(planes), ctx.to_device(truth)
    d_ranks = ctx.to_device(np.zeros((classes + 1) * (k + 1), np.uint64))
    ctx.topk_rank_ragged(rd, d_ranks.ptr, d_lab.ptr, k, stride, d_tr.ptr, 1, classes)
    ctx.sync()
    got = d_ranks.download((classes + 1, k + 1), np.uint64)
    want = np.zeros_like(got)
    for o, (r, c) in zip(offs, sizes):                      # the per-item uniform calls, which test_against_numpy holds to the numpy form
        d_one =ctx.to_device(np.zeros((classes + 1) * (k + 1), np.uint64))
        ctx.topk_rank(d_one.ptr, d_lab.ptr + 4 * o, k, stride, d_tr.ptr + o, 1, classes, r * c)
        ctx.sync()
        want += d_one.download((classes + 1, k + 1), np.uint64)
        d_one.free()
    assert np.array_equal(got, want) and got.sum() == sum(r * c for r, c in sizes)
    inside = np.zeros(span, bool)
    for o, (r, c) in zip(offs, sizes):
        inside[o:o + r * c] = True
    assert np.array_equal(got, T.rank_table(planes[:, :span][:, inside], truth[inside], classes))
    # the statuses of the ragged call
    call = lambda rk, lb, kk, st, tr, tb=1, cl=classes: ctx.lib.mbn_topk_rank_ragged_i32(rd.h, rk, lb, kk, st, tr, tb, cl, None)
    assert call(d_ranks.ptr, d_lab.ptr, k, span - 1, d_tr.ptr) == pkg.EINVAL and call(d_ranks.ptr, d_lab.ptr, 0, stride, d_tr.ptr) == pkg.EINVAL
    assert call(d_ranks.ptr, d_lab.ptr, k, stride + 64, d_tr.ptr) == pkg.EINVAL              # the planes end past the tracked labels
    fresh = pkg.RaggedReadout(ctx, 2)
    assert ctx.lib.mbn_topk_rank_ragged_i32(fresh.h, d_ranks.ptr, d_lab.ptr, k, stride, d_tr.ptr, 1, classes, None) == pkg.EINVAL
    fresh.close()
    rd.close()
    for b in (d_lab, d_tr, d_ranks):
        b.free()


def test_statuses(pkg, ctx):
    classes, k, count = 21, 3, 100
    d_lab, d_tr = ctx.to_device(np.zeros(k * count, np.int32)), ctx.to_device(np.zeros(count, np.int32))
    d_ranks = ctx.to_device(np.zeros((classes + 1) * (k + 1), np.uint64))
    call = lambda rk, lb, tr, kk=k, st=count, tb=4, cl=classes, n=count: ctx.lib.mbn_topk_rank_i32(ctx.h, rk, lb, kk, st, tr, tb, cl, n, None)
    assert call(None, d_lab.ptr, d_tr.ptr) == pkg.EINVAL and call(d_ranks.ptr, None, d_tr.ptr) == pkg.EINVAL
    assert call(d_ranks.ptr, d_lab.ptr, None) == pkg.EINVAL
    assert call(d_ranks.ptr + 4, d_lab.ptr, d_tr.ptr) == pkg.EINVAL and call(d_ranks.ptr, d_lab.ptr + 2, d_tr.ptr) == pkg.EINVAL
    assert call(d_ranks.ptr, d_lab.ptr, d_tr.ptr + 2) == pkg.EINVAL and call(d_ranks.ptr, d_lab.ptr, d_tr.ptr + 2, tb=1, n=50) == pkg.OK
    for bad in (dict(kk=0), dict(kk=9), dict(st=count - 1), dict(tb=2), dict(cl=0), dict(n=0)):
        assert call(d_ranks.ptr, d_lab.ptr, d_tr.ptr, **bad) == pkg.EINVAL, bad
    assert call(d_ranks.ptr, d_lab.ptr, d_tr.ptr, cl=pkg.CONFUSION_MAX_CLASSES + 1) == pkg.EUNSUPPORTED
    # undersized tracked buffers: the ranks table, the label planes, the truth
    assert call(d_ranks.ptr, d_lab.ptr, d_tr.ptr, cl=classes + 1) == pkg.EINVAL
    assert call(d_ranks.ptr, d_lab.ptr, d_tr.ptr, st=count + 1) == pkg.EINVAL and call(d_ranks.ptr, d_lab.ptr, d_tr.ptr, kk=2, st=count + 1) == pkg.OK
    assert call(d_ranks.ptr, d_lab.ptr, d_lab.ptr, kk=1, st=count + 1, n=count + 1) == pkg.OK
    assert call(d_ranks.ptr, d_lab.ptr, d_tr.ptr, kk=1, st=count + 1, n=count + 1) == pkg.EINVAL
    ctx.sync()
    for b in (d_lab, d_tr, d_ranks):
        b.free()
