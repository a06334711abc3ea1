"""Calibration score on the GPU. mbn_calibration_f32 / _ragged_f32 against the numpy form (tests/calibration_ref.py): the same table, byte for byte,
for both truth types with void values, NaN and out-of-range probabilities, interior pointers, accumulating calls, every planning CU count and a graph
replay; the identities against mbn_confusion_i32; the one-leader and the leftover path of the wave aggregation; the ragged form against the per-item
uniform calls; the curve's edges against the thresholded read-out itself; the net's call; every status."""
import ctypes as C

import numpy as np
import pytest

import calibration_ref as R
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

CLASSES = 21
BIG = 3 * 37 * 41           # 4 551 pixels: five chunks, the last one partial
BIG_SEED = 1                # a seed of R.case at which every bin of 10, 15 and 16 has an answered pixel (asserted below)


def _table_buf(ctx, bins):
    return ctx.to_device(np.zeros((bins + 1) * 4, np.uint64))


def _device(ctx, labels, prob, truth, classes, bins, offs=(0, 0, 0), calls=1):
    count = labels.size
    lo, po, to = offs
    d_lab = ctx.to_device(np.concatenate([np.full(lo, -9, np.int32), labels]))
    d_pr = ctx.to_device(np.concatenate([np.full(po, np.nan, np.float32), prob]))
    d_tr = ctx.to_device(np.concatenate([np.zeros(to, truth.dtype), truth]))
    d_cal = _table_buf(ctx, bins)
    for _ in range(calls):
        ctx.calibration(d_cal.ptr, d_lab.ptr + 4 * lo, d_pr.ptr + 4 * po, d_tr.ptr + truth.itemsize * to, truth.itemsize, classes, bins, count)
    ctx.sync()
    got = d_cal.download((bins + 1, 4), np.uint64)
    for b in (d_lab, d_pr, d_tr, d_cal):
        b.free()
    return got


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
@pytest.mark.parametrize("bins", [1, 10, 15, 16, 1024])
@pytest.mark.parametrize("count", [1, 1000, BIG])
def test_against_numpy(pkg, ctx, count, bins, dtype):
    labels, prob, truth = R.case(count, CLASSES, dtype, seed=BIG_SEED if count == BIG else count + bins)
    want = R.calibration_table(labels, prob, truth, CLASSES, bins)
    got = _device(ctx, labels, prob, truth, CLASSES, bins)
    assert np.array_equal(got, want)
    assert got[:, 0].sum() + got[:, 3].sum() == count
    if count == BIG:
        assert want[bins, 0] > 0 and want[:bins, 3].sum() > 0 and (want[:bins, 1] < want[:bins, 0]).any(), "void, abstained and wrong pixels"
        if bins <= 16:
            assert (want[:bins, 0] > 0).all(), "every answered bin is exercised"


@pytest.mark.parametrize("classes", [1000, 4096])
def test_many_classes(pkg, ctx, classes):
    labels, prob, truth = R.case(BIG, classes, np.int32, seed=classes)
    want = R.calibration_table(labels, prob, truth, classes, 15)
    assert np.array_equal(_device(ctx, labels, prob, truth, classes, 15), want) and want[15, 0] > 0 and want[:15, 1].sum() > 0


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_identities_against_the_confusion_call(pkg, ctx, dtype):
    bins = 15
    labels, prob, truth = R.case(BIG, CLASSES, dtype, seed=5)
    got = _device(ctx, labels, prob, truth, CLASSES, bins)
    d_lab, d_tr = ctx.to_device(labels), ctx.to_device(truth)
    d_counts = ctx.to_device(np.zeros((CLASSES + 1) ** 2, np.uint64))
    ctx.confusion(d_counts.ptr, d_lab.ptr, d_tr.ptr, truth.itemsize, CLASSES, BIG)
    ctx.sync()
    counts = d_counts.download((CLASSES + 1, CLASSES + 1), np.uint64)
    assert got[:bins, 1].sum() == np.trace(counts[:CLASSES, :CLASSES]) > 0
    assert got[:bins, 3].sum() == counts[:CLASSES, CLASSES].sum() > 0
    assert got[bins, 0] == counts[CLASSES].sum() > 0 and (got[bins, 1:] == 0).all()
    for b in (d_lab, d_tr, d_counts):
        b.free()


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_interior_pointers_and_accumulation(pkg, ctx, dtype):
    bins = 15
    labels, prob, truth = R.case(1000, CLASSES, dtype, seed=7)
    want = R.calibration_table(labels, prob, truth, CLASSES, bins)
    for offs in [(0, 0, 0), (1, 1, 1), (3, 2, 1), (2, 3, 3)]:
        assert np.array_equal(_device(ctx, labels, prob, truth, CLASSES, bins, offs), want), offs
    assert np.array_equal(_device(ctx, labels, prob, truth, CLASSES, bins, calls=2), 2 * want), "two calls accumulate"


def test_planning_cus_and_replay_give_the_same_bytes(pkg, ctx):
    bins = 16
    labels, prob, truth = R.case(BIG, CLASSES, np.uint8, seed=11)
    want = R.calibration_table(labels, prob, truth, CLASSES, bins)
    try:
        for cus in (1, 3, 0):
            ctx.set_planning_cus(cus)
            assert np.array_equal(_device(ctx, labels, prob, truth, CLASSES, bins), want), "planning CU count %d" % cus
    finally:
        ctx.set_planning_cus(0)
    d_lab, d_pr, d_tr, d_cal = ctx.to_device(labels), ctx.to_device(prob), ctx.to_device(truth), _table_buf(ctx, bins)
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_calibration_f32(ctx.h, d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, CLASSES, bins, BIG, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    for _ in range(2):
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(d_cal.download((bins + 1, 4), np.uint64), 2 * want)
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    for b in (d_lab, d_pr, d_tr, d_cal):
        b.free()


@pytest.mark.parametrize("kind", ["answered", "abstained", "void"])
def test_constant_map_one_leader(pkg, ctx, kind):
    """every pixel has the same bin, label and truth: one leader per wave adds for all of its lanes"""
    count, bins = BIG, 15
    labels = np.full(count, 255 if kind == "abstained" else 7, np.int32)
    truth = np.full(count, 255 if kind == "void" else 7, np.uint8)
    prob = np.full(count, 0.97, np.float32)
    want = R.calibration_table(labels, prob, truth, CLASSES, bins)
    assert np.count_nonzero(want) == {"answered": 3, "abstained": 1, "void": 1}[kind]
    if kind == "answered":
        assert want[14, 0] == want[14, 1] == count and want[14, 2] == count * int(np.float32(0.97) * np.float32(1 << 24))
    assert np.array_equal(_device(ctx, labels, prob, truth, CLASSES, bins), want)


def test_every_lane_its_own_bin(pkg, ctx):
    """bins = 1024 and prob a ramp: the 64 lanes of a wave hold 64 different bins, so all but the leaders' add on their own"""
    count, bins = 4 * 1024 + 77, 1024
    prob = ((np.arange(count) % 1024 + 0.5) / 1024).astype(np.float32)
    assert np.array_equal(R.bin_of(prob[:1024], bins), np.arange(1024))
    rng = np.random.default_rng(3)
    truth = rng.integers(0, CLASSES, count).astype(np.int32)
    labels = np.where(rng.random(count) < 0.7, truth, 255).astype(np.int32)
    labels[::3] = (truth[::3] + 1) % CLASSES
    want = R.calibration_table(labels, prob, truth, CLASSES, bins)
    assert (want[:bins, 0] + want[:bins, 3] >= 4).all()
    assert np.array_equal(_device(ctx, labels, prob, truth, CLASSES, bins), want)


@pytest.mark.parametrize("window", [False, True])
def test_ragged_equals_the_uniform_calls(pkg, ctx, window):
    bins = 15
    sizes = [(37, 41), (20, 28), (100, 30)]
    offs, at = [0] * 3, 3
    for i in (2, 0, 1):                                     # out of order, with gaps
        offs[i] = at
        at += sizes[i][0] * sizes[i][1] + 5
    span = max(o + r * c for o, (r, c) in zip(offs, sizes))
    items = [(o, r, c) for o, (r, c) in zip(offs, sizes)]
    labels, prob, truth = R.case(span, CLASSES, np.uint8, seed=13)
    inside = np.zeros(span, bool)
    for o, r, c in items:
        inside[o:o + r * c] = True
    labels[~inside], prob[~inside], truth[~inside] = 3, np.nan, 3      # the gaps: valid-looking garbage that must not be counted
    prob[np.flatnonzero(~inside)[::2]] = 0.5
    rd = pkg.RaggedReadout(ctx, 3)
    if window:
        rd.set_window(5, 7, CLASSES, 160, 224, [(o, r, c, (0, 0, 224, 160)) for o, r, c in items])
    else:
        rd.set(5, 7, CLASSES, items)
    d_lab, d_pr, d_tr, d_cal = ctx.to_device(labels), ctx.to_device(prob), ctx.to_device(truth), _table_buf(ctx, bins)
    ctx.calibration_ragged(rd, d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, CLASSES, bins)
    ctx.sync()
    got = d_cal.download((bins + 1, 4), np.uint64)
    each = np.zeros_like(got)
    for o, r, c in items:                                   # the per-item uniform calls, which test_against_numpy holds to the numpy form
        d_one = _table_buf(ctx, bins)
        ctx.calibration(d_one.ptr, d_lab.ptr + 4 * o, d_pr.ptr + 4 * o, d_tr.ptr + o, 1, CLASSES, bins, r * c)
        ctx.sync()
        each += d_one.download((bins + 1, 4), np.uint64)
        d_one.free()
    want = R.calibration_table_ragged(labels, prob, truth, CLASSES, bins, items)
    assert got[:, 0].sum() + got[:, 3].sum() == sum(r * c for r, c in sizes), "the gaps were counted, or pixels lost"
    assert np.array_equal(got, each) and np.array_equal(got, want)
    # a captured launch belongs to its set: replayed after a later set it adds nothing
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_calibration_ragged_f32(rd.h, d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, CLASSES, bins, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(d_cal.download((bins + 1, 4), np.uint64), 2 * want), "a replay under its own set adds"
    rd.set(1, 1, CLASSES, [(0, 4, 4)])
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(d_cal.download((bins + 1, 4), np.uint64), 2 * want), "a replay after a later set adds nothing"
    ctx.calibration_ragged(rd, d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, CLASSES, bins)          # the new set is what a new launch scores
    ctx.sync()
    assert np.array_equal(d_cal.download((bins + 1, 4), np.uint64), 2 * want + R.calibration_table(labels[:16], prob[:16], truth[:16], CLASSES, bins))
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    # the statuses of the ragged call
    call = lambda cal, lb, pr, tr, tb=1, cl=CLASSES, nb=bins: ctx.lib.mbn_calibration_ragged_f32(rd.h, cal, lb, pr, tr, tb, cl, nb, None)
    assert call(None, d_lab.ptr, d_pr.ptr, d_tr.ptr) == pkg.EINVAL and call(d_cal.ptr, d_lab.ptr, None, d_tr.ptr) == pkg.EINVAL
    assert call(d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, nb=0) == pkg.EINVAL and call(d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, nb=16) == pkg.EINVAL
    fresh = pkg.RaggedReadout(ctx, 2)
    assert ctx.lib.mbn_calibration_ragged_f32(fresh.h, d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, CLASSES, bins, None) == pkg.EINVAL
    fresh.close()
    rd.close()
    for b in (d_lab, d_pr, d_tr, d_cal):
        b.free()


def test_edges_are_what_the_thresholded_read_out_keeps(pkg, ctx):
    """mbn_resample_softmax_f32 at min_prob = 0 gives the table; at min_prob = j / 16 the confusion matrix of its labels has the diagonal and the
    answered pixels of the bins >= j: edge j of the curve is what that threshold produces"""
    batch, rows, cols, out_rows, out_cols, bins = 2, 7, 7, 60, 80, 16
    rng = np.random.default_rng(17)
    logits = (rng.standard_normal((batch, rows, cols, CLASSES)) * 1.5).astype(np.float32)
    npix = batch * out_rows * out_cols
    truth = rng.integers(0, CLASSES + 2, npix).astype(np.uint8)
    truth[truth >= CLASSES] = 255
    d_logits, d_tr = ctx.to_device(logits), ctx.to_device(truth)
    d_lab, d_pr, d_cal = ctx.alloc(npix * 4), ctx.alloc(npix * 4), _table_buf(ctx, bins)
    d_counts = ctx.to_device(np.zeros((CLASSES + 1) ** 2, np.uint64))
    ctx.resample_softmax(d_lab.ptr, d_pr.ptr, None, d_logits.ptr, batch, rows, cols, CLASSES, out_rows, out_cols, 0.0, 0)
    ctx.calibration(d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, CLASSES, bins, npix)
    ctx.sync()
    table = d_cal.download((bins + 1, 4), np.uint64)
    lab0, pr0 = d_lab.download((npix,), np.int32), d_pr.download((npix,), np.float32)
    assert np.array_equal(table, R.calibration_table(lab0, pr0, truth, CLASSES, bins))
    # the truth agrees with the winner on a third of the pixels, so the diagonal is worth comparing
    agree = rng.random(npix) < 0.33
    truth[agree & (truth != 255)] = lab0[agree & (truth != 255)].astype(np.uint8)
    assert ctx.lib.mbn_upload(ctx.h, d_tr.ptr, truth.ctypes.data, npix) == pkg.OK
    assert ctx.lib.mbn_memset(ctx.h, d_cal.ptr, 0, (bins + 1) * 32) == pkg.OK
    ctx.calibration(d_cal.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, CLASSES, bins, npix)
    ctx.sync()
    table = d_cal.download((bins + 1, 4), np.uint64)
    assert table[:bins, 3].sum() == 0 and table[:bins, 1].sum() > npix // 4 and np.count_nonzero(table[:bins, 0]) >= 8
    for j in (0, 5, 11, 15):
        ctx.resample_softmax(d_lab.ptr, d_pr.ptr, None, d_logits.ptr, batch, rows, cols, CLASSES, out_rows, out_cols, j / 16, 255)
        assert ctx.lib.mbn_memset(ctx.h, d_counts.ptr, 0, (CLASSES + 1) ** 2 * 8) == pkg.OK
        ctx.confusion(d_counts.ptr, d_lab.ptr, d_tr.ptr, 1, CLASSES, npix)
        ctx.sync()
        counts = d_counts.download((CLASSES + 1, CLASSES + 1), np.uint64)
        valid, abstained = counts[:CLASSES].sum(), counts[:CLASSES, CLASSES].sum()
        assert np.trace(counts[:CLASSES, :CLASSES]) == table[j:bins, 1].sum(), j
        assert valid - abstained == table[j:bins, 0].sum(), j
    for b in (d_logits, d_tr, d_lab, d_pr, d_cal, d_counts):
        b.free()


def test_net_segment_calibration(pkg, ctx, tmp_path):
    n, bins = 3, 16
    hw = _weights_os(pkg, tmp_path, 0.25, 64, 64, CLASSES, 32)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_input_u8(True)
    rng = np.random.default_rng(31)
    sh, sw = 75, 130
    npix = n * sh * sw
    src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    truth = rng.integers(0, CLASSES + 2, npix).astype(np.uint8)
    truth[truth >= CLASSES] = 255
    d_src, d_tr = ctx.to_device(src), ctx.to_device(truth)
    d_lab, d_pr, d_cal, d_want = ctx.alloc(npix * 4), ctx.alloc(npix * 4), _table_buf(ctx, bins), _table_buf(ctx, bins)
    lib = ctx.lib
    assert lib.mbn_net_segment_calibration(net.h, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, bins, d_cal.ptr) == pkg.EINVAL      # no segment call yet
    ctx.sync()
    assert not d_cal.download(((bins + 1) * 4,), np.uint64).any()
    # a uniform call: one span; with a threshold, so that there are abstained pixels
    net.segment_prob_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr, d_pr.ptr, 0.06, 255)
    net.segment_calibration(d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, bins, d_cal.ptr)
    ctx.calibration(d_want.ptr, d_lab.ptr, d_pr.ptr, d_tr.ptr, 1, CLASSES, bins, npix)
    ctx.sync()
    got, want = d_cal.download((bins + 1, 4), np.uint64), d_want.download((bins + 1, 4), np.uint64)
    lab, pr = d_lab.download((npix,), np.int32), d_pr.download((npix,), np.float32)
    assert np.array_equal(got, want) and np.array_equal(got, R.calibration_table(lab, pr, truth, CLASSES, bins))
    assert got[:, 0].sum() + got[:, 3].sum() == npix and got[bins, 0] > 0
    # an image call: the net's own ragged set, maps out of order with a gap; the direct calls are one uniform call per map
    one = sh * sw
    dst = [2 * one + 7, 0, one + 3]
    d_rlab, d_rpr = ctx.to_device(np.full(3 * one + 7, 3, np.int32)), ctx.to_device(np.full(3 * one + 7, np.nan, np.float32))
    rtruth = rng.integers(0, CLASSES + 2, 3 * one + 7).astype(np.uint8)
    d_rtr = ctx.to_device(rtruth)
    net.segment_prob_images_fit(d_src.ptr, [i * one * 3 for i in range(n)], [sh] * n, [sw] * n, pkg.FIT_PAD, d_rlab.ptr, dst, d_rpr.ptr)
    for buf in (d_cal, d_want):
        assert lib.mbn_memset(ctx.h, buf.ptr, 0, (bins + 1) * 32) == pkg.OK
    net.segment_calibration(d_rlab.ptr, d_rpr.ptr, d_rtr.ptr, 1, bins, d_cal.ptr)
    for o in dst:
        ctx.calibration(d_want.ptr, d_rlab.ptr + 4 * o, d_rpr.ptr + 4 * o, d_rtr.ptr + o, 1, CLASSES, bins, one)
    ctx.sync()
    got, want = d_cal.download((bins + 1, 4), np.uint64), d_want.download((bins + 1, 4), np.uint64)
    assert np.array_equal(got, want) and got[:, 0].sum() + got[:, 3].sum() == npix
    rlab, rpr = d_rlab.download((3 * one + 7,), np.int32), d_rpr.download((3 * one + 7,), np.float32)
    assert np.array_equal(got, R.calibration_table_ragged(rlab, rpr, rtruth, CLASSES, bins, [(o, sh, sw) for o in dst]))
    net.destroy()
    for b in (d_src, d_tr, d_lab, d_pr, d_cal, d_want, d_rlab, d_rpr, d_rtr):
        b.free()
    hw.free()


def test_statuses(pkg, ctx):
    bins, count = 15, 100
    d_lab, d_pr, d_tr = ctx.to_device(np.zeros(count, np.int32)), ctx.to_device(np.full(count, 0.5, np.float32)), ctx.to_device(np.zeros(count, np.int32))
    d_cal = _table_buf(ctx, bins)
    call = lambda cal, lb, pr, tr, tb=4, cl=CLASSES, nb=bins, n=count: ctx.lib.mbn_calibration_f32(ctx.h, cal, lb, pr, tr, tb, cl, nb, n, None)
    L, P, T, K = d_lab.ptr, d_pr.ptr, d_tr.ptr, d_cal.ptr
    assert call(None, L, P, T) == pkg.EINVAL and call(K, None, P, T) == pkg.EINVAL and call(K, L, None, T) == pkg.EINVAL and call(K, L, P, None) == pkg.EINVAL
    assert ctx.lib.mbn_calibration_f32(None, K, L, P, T, 4, CLASSES, bins, count, None) == pkg.EINVAL
    assert call(K + 4, L, P, T) == pkg.EINVAL and call(K, L + 2, P, T) == pkg.EINVAL and call(K, L, P + 2, T) == pkg.EINVAL
    assert call(K, L, P, T + 2) == pkg.EINVAL
    for bad in (dict(tb=2), dict(cl=0), dict(n=0), dict(nb=0), dict(nb=-1)):
        assert call(K, L, P, T, **bad) == pkg.EINVAL, bad
    assert call(K, L, P, T, cl=pkg.CONFUSION_MAX_CLASSES + 1) == pkg.EUNSUPPORTED
    assert call(K, L, P, T, nb=pkg.CALIBRATION_MAX_BINS + 1) == pkg.EUNSUPPORTED
    assert call(K, L, P, T, n=(1 << 34) + 1) == pkg.EUNSUPPORTED
    assert call(K + 4, L, P, T, nb=pkg.CALIBRATION_MAX_BINS + 1) == pkg.EINVAL                    # an EINVAL goes in front
    # undersized tracked buffers: the table, the labels, the probabilities, the truth
    assert call(K, L, P, T, nb=bins + 1) == pkg.EINVAL
    assert call(K, L + 4, P, T) == pkg.EINVAL and call(K, L, P + 4, T) == pkg.EINVAL and call(K, L, P, T + 4) == pkg.EINVAL
    ctx.sync()
    assert not d_cal.download(((bins + 1) * 4,), np.uint64).any(), "nothing is written on a refusal"
    assert call(K, L, P, T + 2, tb=1, n=50) == pkg.OK                                             # a uint8 truth on any byte
    ctx.sync()
    got = d_cal.download((bins + 1, 4), np.uint64)
    assert got[7, 0] == 50 and got[7, 1] == 50 and got[7, 2] == 50 << 23 and got.sum() == 100 + (50 << 23)
    for b in (d_lab, d_pr, d_tr, d_cal):
        b.free()
