"""Score a segmentation on the GPU: mbn_confusion_i32 / mbn_confusion_ragged_i32 against tests/confusion_ref.py. The arithmetic is integer, so
every comparison is exact; the counts buffers carry a sentinel tail that must come back unchanged. The shapes are the smallest that reach each way
of going wrong: every count up to 300 (head, body and tail of every length), every alignment of labels and truth against each other, both forms on
both sides of the switch point, one workgroup and many, wave-uniform and wave-straddling inputs, the 64-bit carry, planning CU counts (at 1 CU the
LDS table is flushed in the middle of the run), graph replay, ragged sets of both kinds, label bytes across 2^32, the net runner and the C host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import confusion_ref as CR
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

TAIL = 8
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


def _switch(pkg):
    """T: the last class count of the LDS form"""
    return next(c for c in range(1, pkg.CONFUSION_MAX_CLASSES + 1) if pkg.confusion_form(c + 1) == pkg.CONFUSION_FORM_GLOBAL)


def _counts_buf(ctx, classes, slots=1, preset=None):
    cells = (classes + 1) ** 2
    host = np.zeros(slots * cells + TAIL, np.uint64)
    if preset is not None:
        host[:cells] = preset.ravel()
    host[slots * cells:] = SENTINEL
    return ctx.to_device(host)


def _read_counts(buf, classes, slots=1):
    cells = (classes + 1) ** 2
    got = buf.download((slots * cells + TAIL,), np.uint64)
    assert (got[slots * cells:] == SENTINEL).all(), "counts written past the last cell"
    got = got[:slots * cells]
    return got.reshape(classes + 1, classes + 1) if slots == 1 else got.reshape(slots, classes + 1, classes + 1)


def _score(ctx, labels, truth, classes, preset=None, calls=1):
    """mbn_confusion_i32 on freshly uploaded labels / truth, `calls` times into one counts buffer"""
    tb = truth.dtype.itemsize
    d_lab, d_tr, d_n = ctx.to_device(labels), ctx.to_device(truth), _counts_buf(ctx, classes, preset=preset)
    for _ in range(calls):
        ctx.confusion(d_n.ptr, d_lab.ptr, d_tr.ptr, tb, classes, labels.size)
    ctx.sync()
    got = _read_counts(d_n, classes)
    for b in (d_lab, d_tr, d_n):
        b.free()
    return got


def _special_labels(rng, classes, count):
    lab = rng.integers(0, classes, count).astype(np.int32)
    pick = rng.random(count) < 0.1
    lab[pick] = rng.choice(np.array([-1, classes, 255, I32_MAX, I32_MIN], np.int64), int(pick.sum())).astype(np.int32)
    return lab


def _special_truth(rng, classes, count, dtype):
    if dtype == np.uint8:
        tr = rng.integers(0, min(classes, 256), count).astype(np.uint8)
        tr[rng.random(count) < 0.1] = 255
        return tr
    tr = rng.integers(0, classes, count).astype(np.int32)
    pick = rng.random(count) < 0.1
    tr[pick] = rng.choice(np.array([-1, -7, classes, 255, I32_MAX, I32_MIN, 1 << 20], np.int64), int(pick.sum())).astype(np.int32)
    return tr


# ------------------------------------------------------------------------------------------------------------ small counts, alignment

@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_every_count_up_to_300(pkg, ctx, dtype):
    classes, cells = 3, 16
    rng = np.random.default_rng(1)
    lab, tr = _special_labels(rng, classes, 300), _special_truth(rng, classes, 300, dtype)
    d_lab, d_tr, d_n = ctx.to_device(lab), ctx.to_device(tr), _counts_buf(ctx, classes, slots=300)
    for count in range(1, 301):
        ctx.confusion(d_n.ptr + (count - 1) * cells * 8, d_lab.ptr, d_tr.ptr, tr.dtype.itemsize, classes, count)
    ctx.sync()
    got = _read_counts(d_n, classes, slots=300)
    for count in range(1, 301):
        want = CR.confusion(lab[:count], tr[:count], classes)
        assert np.array_equal(got[count - 1], want), "count %d" % count
        assert int(got[count - 1].sum()) == count
    for b in (d_lab, d_tr, d_n):
        b.free()


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_every_alignment_of_labels_against_truth(pkg, ctx, dtype):
    """labels at element offsets 0..3 of a 16-byte boundary x truth at byte offsets 0..3 (uint8) or element offsets 0..3 (int32): interior pointers,
    with other in-range data on both sides that must not be counted"""
    classes, cells, counts = 3, 16, [1, 3, 4, 5, 63, 64, 65, 257]
    rng = np.random.default_rng(2)
    lab, tr = _special_labels(rng, classes, 300), _special_truth(rng, classes, 300, dtype)
    es = tr.dtype.itemsize
    cases = [(lo, to, n) for lo in range(4) for to in range(4) for n in counts]
    d_lab, d_tr, d_n = ctx.to_device(lab), ctx.to_device(tr), _counts_buf(ctx, classes, slots=len(cases))
    assert d_lab.ptr % 16 == 0 and d_tr.ptr % 16 == 0
    for k, (lo, to, n) in enumerate(cases):
        ctx.confusion(d_n.ptr + k * cells * 8, d_lab.ptr + 4 * lo, d_tr.ptr + es * to, es, classes, n)
    ctx.sync()
    got = _read_counts(d_n, classes, slots=len(cases))
    for k, (lo, to, n) in enumerate(cases):
        assert np.array_equal(got[k], CR.confusion(lab[lo:lo + n], tr[to:to + n], classes)), "labels +%d, truth +%d, count %d" % (lo, to, n)
    for b in (d_lab, d_tr, d_n):
        b.free()


# -------------------------------------------------------------------------------------------------------------- class counts, inputs

def _inputs(classes, count, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(count, dtype=np.int64)
    u8_classes = min(classes, 256)
    yield "random, uint8 truth", _special_labels(rng, classes, count), _special_truth(rng, classes, count, np.uint8)
    yield "random, int32 truth", _special_labels(rng, classes, count), _special_truth(rng, classes, count, np.int32)
    yield "constant", np.full(count, classes - 1, np.int32), np.full(count, u8_classes - 1, np.uint8)
    yield "constant, abstained against void", np.full(count, -1, np.int32), np.full(count, I32_MAX, np.int32)
    for period in (63, 64, 65):                                 # waves straddle a change of the pair
        yield "stripes of %d" % period, ((i // period) % classes).astype(np.int32), (((i + 1) // period) % u8_classes).astype(np.uint8)


@pytest.mark.parametrize("count", [4097, 1000003])
@pytest.mark.parametrize("which", ["1", "2", "21", "T", "T+1", "1000", "4096"])
def test_class_counts_and_inputs(pkg, ctx, which, count):
    t = _switch(pkg)
    classes = {"T": t, "T+1": t + 1}.get(which) or int(which)
    assert pkg.confusion_form(classes) == (pkg.CONFUSION_FORM_LDS if classes <= t else pkg.CONFUSION_FORM_GLOBAL)
    for name, lab, tr in _inputs(classes, count, seed=classes + count):
        got = _score(ctx, lab, tr, classes)
        assert int(got.sum()) == count, "%s: the cells sum to %d" % (name, int(got.sum()))
        want = CR.confusion(lab, tr, classes)
        assert np.array_equal(got, want), "%s: %d cells differ" % (name, int((got != want).sum()))


# --------------------------------------------------------------------------------------------------------------------- accumulation

@pytest.mark.parametrize("form", ["lds", "global"])
def test_accumulation_and_the_64_bit_carry(pkg, ctx, form):
    classes = 3 if form == "lds" else _switch(pkg) + 1
    rng = np.random.default_rng(3)
    count = 5000
    lab, tr = _special_labels(rng, classes, count), _special_truth(rng, classes, count, np.uint8)
    lab[:1000], tr[:1000] = 1, 2                                # a wave-uniform stretch among the random pixels
    one = CR.confusion(lab, tr, classes)
    assert np.array_equal(_score(ctx, lab, tr, classes, calls=2), 2 * one), "two calls add"
    assert np.array_equal(_score(ctx, lab, tr, classes), _score(ctx, lab, tr, classes)), "the same call twice"
    preset = np.where(one > 0, np.uint64(0xFFFFFFF0), np.uint64(7)).astype(np.uint64)
    hit = one >= 16
    assert hit.any()
    got = _score(ctx, lab, tr, classes, preset=preset)
    assert np.array_equal(got, preset + one)
    assert (got[hit] >= np.uint64(1 << 32)).all(), "the adds carry into the high word"


def test_planning_cus_give_the_same_counts(pkg, ctx):
    """1, 2 and 3 planning CUs against the device's own. 3 000 009 pixels are 733 chunks of 4096: at one CU the T-class table has one workgroup,
    which counts them all and so flushes its table in the middle of the run, when the epoch of 512 chunks is reached"""
    t = _switch(pkg)
    count = 1000003 * 3
    try:
        for classes in (21, t, t + 1):
            rng = np.random.default_rng(classes)
            lab, tr = _special_labels(rng, classes, count), _special_truth(rng, classes, count, np.int32)
            lab[5000:400000], tr[5000:400000] = 0, 0
            want = CR.confusion(lab, tr, classes)
            for cus in (1, 2, 3, 0):
                assert ctx.lib.mbn_set_planning_cus(ctx.h, cus) == pkg.OK
                assert np.array_equal(_score(ctx, lab, tr, classes), want), "classes %d at %d planning CUs" % (classes, cus)
    finally:
        assert ctx.lib.mbn_set_planning_cus(ctx.h, 0) == pkg.OK


def test_graph_capture_and_replay(pkg, ctx):
    classes, count = 21, 70001
    rng = np.random.default_rng(4)
    lab, tr = _special_labels(rng, classes, count), _special_truth(rng, classes, count, np.uint8)
    d_lab, d_tr, d_n = ctx.to_device(lab), ctx.to_device(tr), _counts_buf(ctx, classes)
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_confusion_i32(ctx.h, d_n.ptr, d_lab.ptr, d_tr.ptr, 1, classes, count, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert not _read_counts(d_n, classes).any(), "the captured call ran"
    want = CR.confusion(lab, tr, classes)
    for k in (1, 2):
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        ctx.sync()
        assert np.array_equal(_read_counts(d_n, classes), k * want), "replay %d" % k
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    for b in (d_lab, d_tr, d_n):
        b.free()


# --------------------------------------------------------------------------------------------------------------------------- ragged

PLAIN_ITEMS = [(900, 37, 61), (0, 5, 7), (40, 4, 200), (3200, 100, 203), (23600, 4, 4)]           # any order, gaps between the maps
WINDOW_ITEMS = [(17, 1, 1, (3, 5, 1, 1)), (30, 1, 300, (0, 7, 64, 1)), (400, 37, 61, (0, 0, 64, 64)), (5000, 9, 1, (9, 0, 1, 64))]


def _ragged_case(classes, items, dtype, seed):
    span = max(off + r * c for off, r, c in items)
    rng = np.random.default_rng(seed)
    return _special_labels(rng, classes, span + 5), _special_truth(rng, classes, span + 5, dtype)      # the gaps hold in-range garbage


@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
@pytest.mark.parametrize("kind", ["plain", "window"])
@pytest.mark.parametrize("form", ["lds", "global"])
def test_ragged(pkg, ctx, form, kind, dtype):
    classes = 5 if form == "lds" else _switch(pkg) + 1
    r = pkg.RaggedReadout(ctx, 8)
    if kind == "plain":
        items = PLAIN_ITEMS
        r.set(1, 1, 5, items)                                   # the set's own class count is not the call's
    else:
        items = [it[:3] for it in WINDOW_ITEMS]
        r.set_window(1, 1, 5, 64, 64, WINDOW_ITEMS)
    lab, tr = _ragged_case(classes, items, dtype, seed=len(items))
    es = tr.dtype.itemsize
    d_lab, d_tr, d_n, d_each = ctx.to_device(lab), ctx.to_device(tr), _counts_buf(ctx, classes), _counts_buf(ctx, classes)
    ctx.confusion_ragged(r, d_n.ptr, d_lab.ptr, d_tr.ptr, es, classes)
    for off, rows, cols in items:                               # the same maps one uniform call each
        ctx.confusion(d_each.ptr, d_lab.ptr + 4 * off, d_tr.ptr + es * off, es, classes, rows * cols)
    ctx.sync()
    got, each = _read_counts(d_n, classes), _read_counts(d_each, classes)
    want = CR.confusion_ragged(lab, tr, classes, items)
    assert int(got.sum()) == sum(rows * cols for _, rows, cols in items), "the gaps were counted, or pixels lost"
    assert np.array_equal(got, want) and np.array_equal(each, want)
    # a captured launch belongs to its set: replayed after a later set, of either kind, it adds nothing
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_confusion_ragged_i32(r.h, d_n.ptr, d_lab.ptr, d_tr.ptr, es, classes, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(_read_counts(d_n, classes), 2 * want), "a replay under its own set adds"
    r.set(1, 1, 5, [(0, 4, 4)])
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(_read_counts(d_n, classes), 2 * want), "a replay after a later set adds nothing"
    ctx.confusion_ragged(r, d_n.ptr, d_lab.ptr, d_tr.ptr, es, classes)          # the new set is what a new launch scores
    ctx.sync()
    assert np.array_equal(_read_counts(d_n, classes), 2 * want + CR.confusion(lab[:16], tr[:16], classes))
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    for b in (d_lab, d_tr, d_n, d_each):
        b.free()


# --------------------------------------------------------------------------------------------------------------------- 32-bit limits

def test_label_bytes_across_4g(pkg, ctx):
    """2^30 + 4099 pixels: the labels' byte offsets cross 2^32. The buffers are cleared on the device (labels 0x01010101: abstained, truth 1) and
    small patterned patches are uploaded at both ends, so the expected counts are the patches' plus one large cell. Both forms."""
    count, patch = (1 << 30) + 4099, 1500
    bufs = []
    for nbytes in (4 * count, count):
        p = C.c_void_p()
        rc = ctx.lib.mbn_alloc(ctx.h, nbytes, C.byref(p))
        if rc == pkg.ENOMEM:
            for q in bufs:
                ctx.lib.mbn_free(ctx.h, q)
            pytest.skip("not enough device memory for %d bytes" % nbytes)
        assert rc == pkg.OK
        bufs.append(p)
    d_lab, d_tr = bufs[0].value, bufs[1].value
    assert ctx.lib.mbn_memset(ctx.h, d_lab, 1, 4 * count) == pkg.OK and ctx.lib.mbn_memset(ctx.h, d_tr, 1, count) == pkg.OK
    rng = np.random.default_rng(5)
    t = _switch(pkg)
    lab_p = [_special_labels(rng, 3, patch) for _ in range(2)]
    tr_p = [_special_truth(rng, 3, patch, np.uint8) for _ in range(2)]
    for k, at in enumerate((3, count - patch)):                # the far patch ends at the last pixel
        assert ctx.lib.mbn_upload(ctx.h, d_lab + 4 * at, lab_p[k].ctypes.data, 4 * patch) == pkg.OK
        assert ctx.lib.mbn_upload(ctx.h, d_tr + at, tr_p[k].ctypes.data, patch) == pkg.OK
    for classes in (3, t + 1):
        want = CR.confusion(np.concatenate(lab_p), np.concatenate(tr_p), classes)
        want[1, classes] += np.uint64(count - 2 * patch)
        d_n = _counts_buf(ctx, classes)
        ctx.confusion(d_n.ptr, d_lab, d_tr, 1, classes, count)
        ctx.sync()
        got = _read_counts(d_n, classes)
        assert int(got.sum()) == count
        assert np.array_equal(got, want), "classes %d: %d cells differ" % (classes, int((got != want).sum()))
        d_n.free()
    for q in bufs:
        ctx.lib.mbn_free(ctx.h, q)


# ------------------------------------------------------------------------------------------------------------------ argument errors

def test_argument_errors(pkg, ctx):
    classes, count = 3, 100
    lab, tr = ctx.to_device(np.zeros(count, np.int32)), ctx.to_device(np.zeros(count, np.int32))
    d_n = _counts_buf(ctx, classes)
    small = ctx.to_device(np.full(15, SENTINEL, np.uint64))      # one cell short of 4 x 4
    lib = ctx.lib

    def call(n, l, t, tb=1, c=classes, cnt=count):
        return lib.mbn_confusion_i32(ctx.h, n, l, t, tb, c, cnt, None)

    assert call(None, lab.ptr, tr.ptr) == pkg.EINVAL and call(d_n.ptr, None, tr.ptr) == pkg.EINVAL and call(d_n.ptr, lab.ptr, None) == pkg.EINVAL
    assert lib.mbn_confusion_i32(None, d_n.ptr, lab.ptr, tr.ptr, 1, classes, count, None) == pkg.EINVAL
    assert call(d_n.ptr + 4, lab.ptr, tr.ptr) == pkg.EINVAL                      # counts off 8 bytes
    assert call(d_n.ptr, lab.ptr + 2, tr.ptr) == pkg.EINVAL                      # labels off 4
    assert call(d_n.ptr, lab.ptr, tr.ptr + 2, tb=4, cnt=50) == pkg.EINVAL        # an int32 truth off 4
    assert call(d_n.ptr, lab.ptr, tr.ptr + 3, tb=1, cnt=50) == pkg.OK            # a uint8 truth may be anywhere
    for c in (0, -1):
        assert call(d_n.ptr, lab.ptr, tr.ptr, c=c) == pkg.EINVAL
    for cnt in (0, -1):
        assert call(d_n.ptr, lab.ptr, tr.ptr, cnt=cnt) == pkg.EINVAL
    for tb in (0, 2, 3, 8, -1):
        assert call(d_n.ptr, lab.ptr, tr.ptr, tb=tb) == pkg.EINVAL
    assert call(small.ptr, lab.ptr, tr.ptr) == pkg.EINVAL and "confusion counts" in ctx.last_error()
    assert call(d_n.ptr, lab.ptr, tr.ptr, cnt=count + 1) == pkg.EINVAL and "confusion labels" in ctx.last_error()
    assert call(d_n.ptr, lab.ptr + 4, tr.ptr, tb=4) == pkg.EINVAL                # an interior pointer: one element short
    assert call(d_n.ptr, lab.ptr, tr.ptr + 4 * count - 50, tb=1) == pkg.EINVAL and "confusion truth" in ctx.last_error()
    assert call(d_n.ptr, lab.ptr, tr.ptr, c=pkg.CONFUSION_MAX_CLASSES + 1) == pkg.EUNSUPPORTED
    assert call(d_n.ptr, lab.ptr, tr.ptr, cnt=(1 << 34) + 1) == pkg.EUNSUPPORTED
    r = pkg.RaggedReadout(ctx, 4)
    assert lib.mbn_confusion_ragged_i32(r.h, d_n.ptr, lab.ptr, tr.ptr, 1, classes, None) == pkg.EINVAL          # no set
    assert lib.mbn_confusion_ragged_i32(None, d_n.ptr, lab.ptr, tr.ptr, 1, classes, None) == pkg.EINVAL
    r.set(1, 1, 5, [(2, 4, 5), (60, 5, 8)])
    assert lib.mbn_confusion_ragged_i32(r.h, d_n.ptr, lab.ptr, tr.ptr, 2, classes, None) == pkg.EINVAL
    assert lib.mbn_confusion_ragged_i32(r.h, d_n.ptr, None, tr.ptr, 1, classes, None) == pkg.EINVAL
    assert lib.mbn_confusion_ragged_i32(r.h, d_n.ptr, lab.ptr, tr.ptr, 1, 4097, None) == pkg.EUNSUPPORTED
    assert lib.mbn_confusion_ragged_i32(r.h, d_n.ptr, lab.ptr + 4, tr.ptr, 1, classes, None) == pkg.EINVAL       # the set reaches element 100
    r.set(1, 1, 5, [(2, 4, 5), (61, 5, 8)])
    assert lib.mbn_confusion_ragged_i32(r.h, d_n.ptr, lab.ptr, tr.ptr, 4, classes, None) == pkg.EINVAL           # ... and now 101
    ctx.sync()
    got = _read_counts(d_n, classes)
    assert int(got.sum()) == 50 and got[0, 0] == 50, "only the one accepted call may have been launched"
    assert (small.download((15,), np.uint64) == SENTINEL).all()
    r.close()
    for b in (lab, tr, d_n, small):
        b.free()


# ------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS = 0.5, 21, 64, 96


def test_net_segment_score(pkg, ctx, tmp_path):
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, 16)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 8)
    net.set_input_u8(True)
    rng = np.random.default_rng(6)
    n, sh, sw = 2, 75, 130
    src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    npix = n * sh * sw
    truth = _special_truth(rng, CLASSES, npix + 64, np.uint8)
    d_src, d_lab, d_pr, d_tr = ctx.to_device(src), ctx.alloc(4 * (npix + 64)), ctx.alloc(4 * (npix + 64)), ctx.to_device(truth)
    d_n = _counts_buf(ctx, CLASSES)
    assert ctx.lib.mbn_net_segment_score(net.h, d_lab.ptr, d_tr.ptr, 1, d_n.ptr) == pkg.EINVAL, "before any segment call"
    total = np.zeros((CLASSES + 1, CLASSES + 1), np.uint64)

    def check(what, items=None):
        nonlocal total
        net.segment_score(d_lab.ptr, d_tr.ptr, 1, d_n.ptr)
        ctx.sync()
        lab = d_lab.download((npix + 64,), np.int32)
        total = total + (CR.confusion(lab[:npix], truth[:npix], CLASSES) if items is None else CR.confusion_ragged(lab, truth, CLASSES, items))
        assert np.array_equal(_read_counts(d_n, CLASSES), total), what
        return lab

    net.segment_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr)
    lab = check("segment_fit")
    assert len(np.unique(lab[:npix])) > 1
    # a refused call leaves the record in place: the same span is scored again
    assert ctx.lib.mbn_net_segment_fit(net.h, d_src.ptr, n, sh, sw, pkg.FIT_CROP, d_lab.ptr, None) == pkg.EUNSUPPORTED
    check("after a refused call")
    # image calls score the net's own ragged set; with a threshold the abstained column fills
    rows, cols = [sh, 40], [sw, 50]
    offs, dst = [0, sh * sw * 3], [sh * sw + 11, 3]
    ctx.lib.mbn_memset(ctx.h, d_lab.ptr, 0xFF, 4 * (npix + 64))
    net.segment_prob_images_fit(d_src.ptr, offs, rows, cols, pkg.FIT_PAD, d_lab.ptr, dst, d_pr.ptr)
    ctx.sync()
    prob = d_pr.download((npix + 64,), np.float32)
    min_prob = float(np.median(np.concatenate([prob[dst[i]:dst[i] + rows[i] * cols[i]] for i in range(2)])))      # about half of the pixels abstain
    net.segment_prob_images_fit(d_src.ptr, offs, rows, cols, pkg.FIT_PAD, d_lab.ptr, dst, d_pr.ptr, min_prob=min_prob, ignore_label=255)
    before = total.copy()
    lab = check("segment_prob_images_fit", items=[(dst[i], rows[i], cols[i]) for i in range(2)])
    added = total - before
    assert int(added.sum()) == sh * sw + 40 * 50 and 0 < int(added[:, CLASSES].sum()) < int(added.sum()), "some pixels abstain, not all"
    net.segment_views_fit(d_src.ptr, n, sh, sw, [1.0, 0.75], [0, 1], d_lab.ptr)
    check("segment_views_fit")
    m, iou = pkg.confusion_metrics(total, CLASSES)
    want = CR.metrics(total, CLASSES)
    assert m.pixels == float(total.sum()) and m.pixel_accuracy == want["pixel_accuracy"] and np.array_equal(iou, want["iou"], equal_nan=True)
    net.destroy()
    for b in (d_src, d_lab, d_pr, d_tr, d_n):
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def _pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    w, h, maxval = (int(g) for g in m.groups())
    return np.frombuffer(raw[m.end():], ">u2" if maxval > 255 else np.uint8).astype(np.int32).reshape(h, w)


def _score_line(out):
    m = re.search(r"^score: (.*)$", out, re.M)
    assert m, out
    return {k: float(v) for k, v in (f.split("=") for f in m.group(1).split())}


def test_c_host_truth(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    sh, sw, classes = 75, 130, 1000                             # the host's synthetic weights have 1000 classes
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, plain, tta = str(tmp_path / "a.ppm"), str(tmp_path / "plain.pgm"), str(tmp_path / "tta.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", "3", "--alpha", "0.5", "--res", "%dx%d" % (ROWS, COLS), "--output-stride", "16", "--ppm", ppm, "--fit", "pad"]
    r = subprocess.run(common + ["--segment-source", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "score:" not in r.stdout, r.stdout + r.stderr
    r = subprocess.run(common + ["--segment-source", str(tmp_path / "again.pgm"), "--truth", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    s = _score_line(r.stdout)
    assert s["pixel_acc"] == 1 and s["miou"] == 1 and s["mean_acc"] == 1 and s["fw_iou"] == 1
    assert s["pixels"] == sh * sw and s["valid"] == sh * sw and s["void"] == 0 and s["abstained"] == 0
    # test-time augmentation against the plain run's map: what the reference computes from the two files
    r = subprocess.run(common + ["--segment-source", tta, "--tta-scales", "1,0.5", "--tta-flip", "--truth", plain], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    s = _score_line(r.stdout)
    want = CR.metrics(CR.confusion(_pgm(tta), _pgm(plain), classes), classes)
    for key, field in (("pixels", "pixels"), ("valid", "valid"), ("void", "void_pixels"), ("abstained", "abstained"),
                       ("classes_present", "classes_present"), ("pixel_acc", "pixel_accuracy")):
        assert s[key] == want[field], (key, s[key], want[field])
    for key, field in (("mean_acc", "mean_accuracy"), ("miou", "miou"), ("fw_iou", "fw_iou")):
        assert abs(s[key] - want[field]) <= classes * 2.0 ** -52 * abs(want[field]), (key, s[key], want[field])
    assert 0 < s["pixel_acc"] <= 1
    # --min-confidence / --ignore-label: the abstained column fills
    r = subprocess.run(common + ["--segment-source", tta, "--min-confidence", "0.5", "--ignore-label", "65535", "--truth", plain], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    s = _score_line(r.stdout)
    assert s["abstained"] == int((_pgm(tta) == 65535).sum()) and s["pixels"] == sh * sw
    # a truth of another size, a truth without --segment-source, more truths than images
    wrong = str(tmp_path / "wrong.pgm")
    with open(wrong, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (sw, sh - 1) + bytes(sw * (sh - 1)))
    r = subprocess.run(common + ["--segment-source", tta, "--truth", wrong], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "score:" not in r.stdout, r.stdout + r.stderr
    r = subprocess.run(common + ["--truth", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stdout + r.stderr
    r = subprocess.run(common + ["--segment-source", tta, "--truth", plain, "--truth", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2, r.stdout + r.stderr
