"""Score a segmentation by its regions on the GPU: mbn_panoptic_i32 / mbn_panoptic_ragged_i32 against the pair histogram of tests/panoptic_ref.py.
Everything the device writes is an integer, so every comparison is exact and in full: pq_u64, scored, and the four per-segment outputs. Every
output carries a sentinel tail (and, per image, sentinel entries from n on; in the ragged form the maps lie between gaps of in-range garbage) that
must come back unchanged. The shapes are the smallest that reach each way of going wrong: 1 x 1, one row on both sides of a wave, sizes on both
sides of the pixel kernels' unit of work (PANOPTIC_CHUNK pixels), batches with a different image per slot. Then the net runner in both forms and
the C host.

Truth numbers up to bit 17 are reached (400 x 400 single-pixel truth segments). Higher bits run the same loop over the bits of n_truth - 1 and
are not tested: bit 23 would need maps of 8 M pixels.

The only floating-point comparisons are those of mbn_panoptic_metrics: bit for bit against the Python formulas on the same pq_u64, and within
tp * 2^-32 of the IoU sum of the reference, which is formed exactly for that (fractions.Fraction): each floor loses less than 2^-32, and that is
the whole error."""
import ctypes as C
import math
import os
from fractions import Fraction
import re
import subprocess

import numpy as np
import pytest

import components_ref as R
import panoptic_ref as P
from test_dilation_gpu import _weights_os
from test_panoptic_cpu import hand_cases

pytestmark = pytest.mark.gpu

TAIL = 16
SENT = np.int32(0x5A5A5A5A)
SENT64 = np.uint64(0x5A5A5A5A5A5A5A5A)
OUTPUTS = ("match_pred", "match_truth", "inter", "void")
POINTERS = ("pq", "scored") + OUTPUTS + ("comp_pred", "pred", "n_pred", "comp_truth", "truth", "n_truth")


@pytest.fixture(scope="module")
def pan(pkg, ctx):
    h = pkg.Panoptic(ctx, 8, 1 << 16)
    yield h
    h.close()


def _table(images, k, cap):
    """records [batch][cap][8]: each image's first min(n, cap) records, sentinels behind them"""
    t = np.full((len(images), cap, 8), SENT, np.int32)
    for i, im in enumerate(images):
        n = min(len(im[k]), cap)
        t[i, :n] = im[k][:n]
    return t


def _expected(images, classes, max_pred, max_truth, pq0):
    """pq, scored and the four per-segment tables as one call must leave them, from the reference"""
    batch = len(images)
    pq = pq0.copy()
    scored = np.zeros(batch, np.int32)
    tables = {"match_pred": np.full((batch, max_pred), SENT, np.int32), "match_truth": np.full((batch, max_truth), SENT, np.int32),
              "inter": np.full((batch, max_pred), SENT, np.int32), "void": np.full((batch, max_pred), SENT, np.int32)}
    iou = np.zeros(classes, np.float64)
    for i, (cp, pred, ct, truth) in enumerate(images):
        if len(pred) > max_pred or len(truth) > max_truth:
            continue                                            # not scored: nothing added, nothing written
        scored[i] = 1
        r = P.panoptic(cp, pred, ct, truth, classes)
        pq += r.pq
        iou += r.iou
        tables["match_pred"][i, :len(pred)] = r.match_pred
        tables["match_truth"][i, :len(truth)] = r.match_truth
        tables["inter"][i, :len(pred)] = r.inter
        tables["void"][i, :len(pred)] = r.void
    return pq, scored, tables, iou


class Call:
    """the device buffers of one mbn_panoptic_i32: every pointer at its element offset (offs) from a 16-byte aligned buffer"""

    def __init__(self, ctx, images, classes, max_pred, max_truth, pq0=None, outputs=OUTPUTS, offs=None):
        self.ctx, self.images, self.classes, self.max_pred, self.max_truth = ctx, images, classes, max_pred, max_truth
        self.batch = len(images)
        self.shape = images[0][0].shape
        self.count = self.batch * images[0][0].size
        self.outputs = outputs
        self.offs = dict.fromkeys(POINTERS, 0)
        self.offs.update(offs or {})
        self.pq0 = np.zeros((classes, 4), np.uint64) if pq0 is None else pq0
        o = self.offs
        host = {"comp_pred": np.concatenate([im[0].ravel() for im in images]).astype(np.int32),
                "comp_truth": np.concatenate([im[2].ravel() for im in images]).astype(np.int32),
                "pred": _table(images, 1, max_pred).ravel(), "truth": _table(images, 3, max_truth).ravel(),
                "n_pred": np.array([len(im[1]) for im in images], np.int32), "n_truth": np.array([len(im[3]) for im in images], np.int32)}
        self.fresh = {"pq": self._padded(self.pq0.ravel(), o["pq"], SENT64), "scored": np.full(self.batch + TAIL + 4, SENT, np.int32)}
        for name in OUTPUTS:
            self.fresh[name] = np.full(self.batch * (max_truth if name == "match_truth" else max_pred) + TAIL + 4, SENT, np.int32)
        self.d = {name: ctx.to_device(self._padded(a, o[name], SENT)) for name, a in host.items()}
        self.d.update({name: ctx.to_device(a) for name, a in self.fresh.items()})
        assert all(b.ptr % 16 == 0 for b in self.d.values())

    @staticmethod
    def _padded(a, off, fill):
        out = np.full(a.size + TAIL + 4, fill, a.dtype)
        out[off:off + a.size] = a
        return out

    def ptr(self, name):
        if name in OUTPUTS and name not in self.outputs:
            return None
        return self.d[name].ptr + self.offs[name] * (8 if name == "pq" else 4)

    def args(self):
        p = self.ptr
        return (p("pq"), p("scored"), p("match_pred"), p("match_truth"), p("inter"), p("void"), p("comp_pred"), p("pred"), p("n_pred"), self.max_pred,
                p("comp_truth"), p("truth"), p("n_truth"), self.max_truth, self.batch, self.shape[0], self.shape[1], self.classes, None)

    def reset(self):
        for name, a in self.fresh.items():
            self.d[name].upload(a)

    def got(self):
        self.ctx.sync()
        return {name: self.d[name].download(a.shape, a.dtype) for name, a in self.fresh.items()}

    def check(self, got, what, times=1):
        """every output in full after `times` calls on fresh outputs"""
        pq, scored, tables, iou = _expected(self.images, self.classes, self.max_pred, self.max_truth, self.pq0)
        pq = self.pq0 + (pq - self.pq0) * np.uint64(times)
        want = self._padded(pq.ravel(), self.offs["pq"], SENT64)
        assert np.array_equal(got["pq"], want), "%s: pq\n%s\nexpected\n%s" % (what, got["pq"], want)
        assert np.array_equal(got["scored"], self._padded(scored, self.offs["scored"], SENT)[:got["scored"].size]), what + ": scored"
        for name in OUTPUTS:
            if name not in self.outputs:
                assert (got[name] == SENT).all(), "%s: %s is NULL and was written" % (what, name)
                continue
            want = np.full(got[name].size, SENT, np.int32)
            want[self.offs[name]:self.offs[name] + tables[name].size] = tables[name].ravel()
            bad = np.flatnonzero(got[name] != want)
            assert bad.size == 0, "%s: %s differs in %d entries, first at %d: %d, expected %d" % (what, name, bad.size, bad[0], got[name][bad[0]],
                                                                                                 want[bad[0]])
        return pq, iou

    def free(self):
        for b in self.d.values():
            b.free()


def _run(pkg, ctx, pan, images, classes, max_pred=None, max_truth=None, what="", **kw):
    """one mbn_panoptic_i32 on freshly uploaded buffers, compared with the reference in full. Returns (pq, the reference's float IoU sums)"""
    if max_pred is None:
        max_pred = max(len(im[1]) for im in images) + 1
    if max_truth is None:
        max_truth = max(len(im[3]) for im in images) + 2
    c = Call(ctx, images, classes, max_pred, max_truth, **kw)
    rc = ctx.lib.mbn_panoptic_i32(pan.h, *c.args())
    assert rc == pkg.OK, "%s: %d %s" % (what, rc, ctx.last_error())
    out = c.check(c.got(), what)
    c.free()
    return out


def _scene(rows, cols, classes, seed, side=5, shift=1, noise=0.05, drop=0.05, void_blocks=0.15):
    t = P.block_scene(rows, cols, classes, seed, side=side, drop=drop, drop_blocks=void_blocks, class_seed=seed)
    p = P.block_scene(rows, cols, classes, seed + 1, side=side, shift=shift, noise=noise, drop=drop, class_seed=seed)
    return (p[0], p[1], t[0], t[1])


# ------------------------------------------------------------------------------------------------------------------------- the shapes

@pytest.mark.parametrize("batch", [1, 3])
def test_smallest_shapes(pkg, ctx, pan, batch):
    unit = pkg.PANOPTIC_CHUNK
    assert unit == 1024
    shapes = [(1, 1), (1, 2), (1, 63), (1, 64), (1, 65), (1, unit - 1), (1, unit), (1, unit + 1), (3, 341), (32, 32), (25, 41), (2, unit), (2 * unit + 1, 1),
              (37, 59)]
    seen = np.zeros(3, np.int64)
    for rows, cols in shapes:
        images = [_scene(rows, cols, 4, seed=rows * 1000 + cols + 7 * i, side=3 + i, shift=i) for i in range(batch)]   # a different image per slot
        pq, _ = _run(pkg, ctx, pan, images, 4, what="%d x %d x %d" % (batch, rows, cols))
        seen += pq[:, :3].sum(0).astype(np.int64)
    assert (seen > 0).all(), "true positives, false positives and false negatives all occurred: %s" % seen


# ------------------------------------------------------------------------------------------------------------------------ the patterns

def _constant(rows, cols, label):
    return P.stuff(np.full((rows, cols), label, np.int32), 8)


def test_patterns(pkg, ctx, pan):
    rows, cols, classes = 45, 83, 6
    n = rows * cols
    one, other = _constant(rows, cols, 2), _constant(rows, cols, 3)
    pq, _ = _run(pkg, ctx, pan, [one + one], classes, what="constant against constant")
    assert pq[2].tolist() == [1, 0, 0, 1 << 32] and pq.sum() == 1 + (1 << 32)
    pq, _ = _run(pkg, ctx, pan, [one + other], classes, what="constant against another constant")
    assert pq[2].tolist() == [0, 1, 0, 0] and pq[3].tolist() == [0, 0, 1, 0]
    truth = P.block_scene(rows, cols, classes, 3, side=9, class_seed=5)
    for shift in (0, 1, 2):
        pred = P.block_scene(rows, cols, classes, 3, side=9, shift=shift, class_seed=5)
        pq, _ = _run(pkg, ctx, pan, [pred + truth], classes, what="blocks shifted by %d" % shift)
        if shift == 0:
            assert pq[:, 0].sum() == len(truth[1]) and pq[:, 1:3].sum() == 0 and pq[:, 3].sum() == len(truth[1]) << 32, "every block matches itself"
        else:
            assert pq[:, 0].sum() > 0 and pq[:, 1].sum() > 0, "the whole blocks still match, the slivers at the frame do not"
    noisy = P.block_scene(rows, cols, classes, 4, side=9, noise=0.3, class_seed=5)
    pq, _ = _run(pkg, ctx, pan, [noisy + truth], classes, what="30 % noise")
    assert pq[:, 1].sum() > 1000, "most segments are single pixels without a majority worth a match"
    pq, _ = _run(pkg, ctx, pan, [truth + noisy], classes, what="30 % noise in the truth")
    assert pq[:, 2].sum() > 1000
    void = (np.full((rows, cols), -1, np.int32), np.zeros((0, 8), np.int32))
    pq, _ = _run(pkg, ctx, pan, [noisy + void], classes, what="all-void truth")
    assert pq.sum() == 0, "every predicted segment is excused"
    pq, _ = _run(pkg, ctx, pan, [void + truth], classes, what="all-abstained prediction")
    assert pq[:, 2].sum() == len(truth[1]) and pq[:, [0, 1, 3]].sum() == 0
    # every pixel a segment of its own on both sides: a wave of the pixel kernels holds 64 predicted segments, four times what it aggregates
    rng = np.random.default_rng(9)
    ids = rng.permutation(n).reshape(rows, cols)
    single = P.segments(ids, rng.integers(0, classes, n))
    pq, _ = _run(pkg, ctx, pan, [single + single], classes, what="single pixels against themselves")
    assert pq[:, 0].sum() == n and pq[:, 3].sum() == n << 32
    pq, _ = _run(pkg, ctx, pan, [single + truth, truth + single, noisy + single], classes, what="single pixels against blocks, both ways")
    # whole-class segments, and a class count below some labels: those segments add nothing
    L, T = R.blocks(rows, cols, classes, seed=11, side=7), R.blocks(rows, cols, classes, seed=11, side=7)
    T[:, 40:] = R.blocks(rows, cols, classes, seed=12, side=7)[:, 40:]
    T[:6] = 255
    _run(pkg, ctx, pan, [P.stuff(L, classes) + P.stuff(T, classes)], classes, what="stuff segments")
    pq, _ = _run(pkg, ctx, pan, [P.stuff(L, classes) + P.stuff(T, classes)], 3, what="labels beyond the class count")
    assert pq.shape == (3, 4)


def test_class_counts_at_the_lds_limit(pkg, ctx, pan):
    """one class, and both sides of the class count up to which a workgroup of the deciding kernels counts in LDS; the labels spread over all classes"""
    limit = pkg.PANOPTIC_LDS_CLASSES
    for classes in (1, 2, limit - 1, limit, limit + 1, 4096):
        images = [_scene(40, 67, classes, seed=classes + i, side=3 + i) for i in range(2)]
        pq, _ = _run(pkg, ctx, pan, images, classes, what="%d classes" % classes)
        assert pq[:, 0].sum() > 0 and pq[:, 1].sum() > 0 and pq[:, 2].sum() > 0
        assert classes < 3 or (np.flatnonzero(pq[:, :3].sum(1))[-1] > classes * 3 // 4), "the top classes are reached"


def test_truth_numbers_with_bit_17(pkg, ctx):
    """400 x 400 single-pixel truth segments (numbers up to 159 999: bit 17 is set from 131 072 on) against 2 x 1 dominoes: a domino meets two truth
    segments with inter 1 each, union = 2 + 1 - 1 = 2, and 2 is not > 2: no match. The last two rows are predicted pixel by pixel and match truth
    numbers that have bit 17 set."""
    side, classes = 400, 3
    n = side * side
    rng = np.random.default_rng(17)
    truth = P.segments(np.arange(n).reshape(side, side), rng.integers(0, classes, n))
    ids = np.arange(n).reshape(side, side)
    ids[:side - 2] = ids[:side - 2] // 2 * 2                       # dominoes, but for the last two rows
    pred = P.segments(ids, truth[1][:, 0])                         # a domino has the class of its first pixel
    assert len(truth[1]) == n and len(pred[1]) == n // 2 + side
    h = pkg.Panoptic(ctx, 1, n)
    pq, _ = _run(pkg, ctx, h, [pred + truth], classes, max_pred=n, max_truth=n, what="bit 17")
    h.close()
    assert pq[:, 0].sum() == 2 * side and pq[:, 1].sum() == (n - 2 * side) // 2 and pq[:, 2].sum() == n - 2 * side and pq[:, 3].sum() == (2 * side) << 32


def test_hand_derived_cases(pkg, ctx, pan):
    for name, cp, pred, ct, truth, classes, pq_want, mp, mt, inter, void in hand_cases():
        pq, _ = _run(pkg, ctx, pan, [(cp[None], pred, ct[None], truth)], classes, what=name)
        assert pq.tolist() == [list(r) for r in pq_want], name


# ---------------------------------------------------------------------------------------------- overflow, accumulation, NULL, alignment

def _three(rows=33, cols=47, classes=5):
    return [_scene(rows, cols, classes, seed=50, side=4), _scene(rows, cols, classes, seed=51, side=11, noise=0.0), _scene(rows, cols, classes, seed=52, side=6)]


def test_table_overflow(pkg, ctx, pan):
    images = _three()
    n_pred, n_truth = [len(im[1]) for im in images], [len(im[3]) for im in images]
    assert n_pred[0] > n_pred[2] > n_pred[1] and n_truth[0] > n_truth[2] > n_truth[1]
    pq0 = np.arange(20, dtype=np.uint64).reshape(5, 4) + np.uint64(1 << 40)
    for mp, mt, scored in ((n_pred[0], n_truth[0], 3), (n_pred[0] - 1, n_truth[0], 2), (n_pred[0], n_truth[0] - 1, 2), (n_pred[2], n_truth[0], 2),
                           (n_pred[2] - 1, n_truth[0], 1), (n_pred[0], n_truth[2] - 1, 1), (n_pred[1] - 1, n_truth[0], 0), (1, 1, 0)):
        c = Call(ctx, images, 5, mp, mt, pq0=pq0)
        assert ctx.lib.mbn_panoptic_i32(pan.h, *c.args()) == pkg.OK
        got = c.got()
        c.check(got, "max_pred %d, max_truth %d" % (mp, mt))
        assert int(got["scored"][:3].sum()) == scored
        if scored == 0:
            assert np.array_equal(got["pq"][:20].reshape(5, 4), pq0), "nothing is added"
        c.free()


def test_two_calls_accumulate_and_null_outputs(pkg, ctx, pan):
    images = _three()
    c = Call(ctx, images, 5, 600, 500)
    for times in (1, 2, 3):
        assert ctx.lib.mbn_panoptic_i32(pan.h, *c.args()) == pkg.OK
        c.check(c.got(), "call %d" % times, times=times)
    c.free()
    for outputs in ((), ("match_pred",), ("match_truth",), ("inter",), ("void",), ("match_truth", "void")):
        _run(pkg, ctx, pan, images, 5, outputs=outputs, what="outputs %s" % (outputs,))


def test_every_alignment(pkg, ctx, pan):
    images = _three(rows=9, cols=21)
    for k in range(4):
        offs = {name: (i + k) % 4 for i, name in enumerate(POINTERS)}                # elements: 4 bytes, for pq 8
        _run(pkg, ctx, pan, images, 5, offs=offs, what="offsets %s" % offs)
    for name in POINTERS:
        for off in (1, 2, 3):
            _run(pkg, ctx, pan, images[:1], 5, offs={name: off}, what="%s + %d" % (name, off))


# ------------------------------------------------------------------------------------------------------------------ planning CUs, graph

def test_planning_cus_give_the_same_bytes(pkg, ctx, pan):
    images = [_scene(70, 131, 21, seed=60, side=9), _scene(70, 131, 21, seed=61, side=4, noise=0.3), _scene(70, 131, 21, seed=62, side=25, shift=3)]
    pq0 = np.full((21, 4), 5, np.uint64)
    try:
        results = []
        for cus in (1, 3, 0):
            assert ctx.lib.mbn_set_planning_cus(ctx.h, cus) == pkg.OK
            c = Call(ctx, images, 21, 3000, 2000, pq0=pq0)
            assert ctx.lib.mbn_panoptic_i32(pan.h, *c.args()) == pkg.OK
            results.append(c.got())
            c.check(results[-1], "%d planning CUs" % cus)
            c.free()
        for other in results[1:]:
            assert all(results[0][k].tobytes() == other[k].tobytes() for k in results[0]), "identical bytes in every output"
    finally:
        assert ctx.lib.mbn_set_planning_cus(ctx.h, 0) == pkg.OK


def test_graph_capture_and_replay(pkg, ctx, pan):
    images = _three()
    c = Call(ctx, images, 5, 600, 500)
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_panoptic_i32(pan.h, *c.args())
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    got = c.got()
    assert (got["scored"] == SENT).all() and np.array_equal(got["pq"], c.fresh["pq"]), "the captured call did not run"
    for times in (1, 2):
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        c.check(c.got(), "replay %d" % times, times=times)
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    c.free()


# ----------------------------------------------------------------------------------------------------------------------------- ragged

@pytest.mark.parametrize("kind", ["plain", "window"])
def test_ragged(pkg, ctx, pan, kind):
    unit = pkg.PANOPTIC_CHUNK
    sizes = [(33, 65), (4 if kind == "plain" else 1,) * 2, (5, 3 * 64 + 8), (unit // 8 + 1, 8), (32, 32)]
    order, off, items = [3, 0, 4, 1, 2], 7, [None] * 5            # any order in memory, gaps between the maps
    for i in order:
        items[i] = (off, sizes[i][0], sizes[i][1])
        off += sizes[i][0] * sizes[i][1] + 13 + i
    span, classes, max_pred, max_truth = off, 4, 700, 300
    rng = np.random.default_rng(71)
    cp, ct = rng.integers(-1, 5, span + TAIL).astype(np.int32), rng.integers(-1, 5, span + TAIL).astype(np.int32)   # the gaps hold in-range garbage
    images = []
    for i, (o, rows, cols) in enumerate(items):
        images.append(_scene(rows, cols, classes, seed=80 + i, side=3 + i % 3, shift=i % 2))
        cp[o:o + rows * cols], ct[o:o + rows * cols] = images[-1][0].ravel(), images[-1][2].ravel()
        assert len(images[-1][1]) <= max_pred and len(images[-1][3]) <= max_truth
    pq_want, scored_want, tables, _ = _expected(images, classes, max_pred, max_truth, np.zeros((classes, 4), np.uint64))
    r = pkg.RaggedReadout(ctx, 8)
    if kind == "plain":
        r.set(1, 1, 5, items)                                   # the set's own class count is not the call's
    else:
        r.set_window(1, 1, 5, 64, 64, [it + ((3, 5, 1, 1),) for it in items])
    d_in = [ctx.to_device(a) for a in (cp, _table(images, 1, max_pred), np.array([len(im[1]) for im in images], np.int32), ct,
                                       _table(images, 3, max_truth), np.array([len(im[3]) for im in images], np.int32))]
    fresh = [np.full(classes * 4 + TAIL, 0, np.uint64), np.full(5 + TAIL, SENT, np.int32), np.full(5 * max_pred + TAIL, SENT, np.int32),
             np.full(5 * max_truth + TAIL, SENT, np.int32), np.full(5 * max_pred + TAIL, SENT, np.int32), np.full(5 * max_pred + TAIL, SENT, np.int32)]
    fresh[0][classes * 4:] = SENT64
    d_out = [ctx.to_device(a) for a in fresh]

    def call():
        return ctx.lib.mbn_panoptic_ragged_i32(pan.h, r.h, *[b.ptr for b in d_out], d_in[0].ptr, d_in[1].ptr, d_in[2].ptr, max_pred, d_in[3].ptr,
                                               d_in[4].ptr, d_in[5].ptr, max_truth, classes, None)

    def outputs():
        ctx.sync()
        return [b.download(a.shape, a.dtype) for b, a in zip(d_out, fresh)]

    def reset():
        for b, a in zip(d_out, fresh):
            b.upload(a)

    def expect(got, times, what):
        assert np.array_equal(got[0][:classes * 4].reshape(classes, 4), pq_want * np.uint64(times)) and (got[0][classes * 4:] == SENT64).all(), what
        assert np.array_equal(got[1][:5], scored_want) and (got[1][5:] == SENT).all(), what
        for a, name in zip(got[2:], OUTPUTS):
            assert np.array_equal(a[:tables[name].size], tables[name].ravel()) and (a[tables[name].size:] == SENT).all(), what + ": " + name

    assert call() == pkg.OK, ctx.last_error()
    expect(outputs(), 1, "ragged")
    assert pq_want[:, 0].sum() > 0 and pq_want[:, 1].sum() > 0 and pq_want[:, 2].sum() > 0
    # each map alone through the uniform call gives its share
    total = np.zeros((classes, 4), np.uint64)
    for im in images:
        total += _run(pkg, ctx, pan, [im], classes, what="a map alone")[0]
    assert np.array_equal(total, pq_want)
    # a captured launch belongs to its set: replayed under it, it adds again; after a later set it does nothing
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = call()
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    reset()
    for times in (1, 2):
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        expect(outputs(), times, "replay %d" % times)
    reset()
    r.set(1, 1, 5, [(0, 4, 4)])
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    assert all(np.array_equal(a, b) for a, b in zip(outputs(), fresh)), "a replay after a later set writes nothing"
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    for b in d_in + d_out:
        b.free()


# ------------------------------------------------------------------------------------------------------- end to end, and the metrics

def test_components_on_both_sides_and_metrics(pkg, ctx, pan):
    """labels and truth through mbn_components_i32, their outputs straight into mbn_panoptic_i32: nothing leaves the device in between"""
    batch, rows, cols, classes, max_regions = 3, 61, 97, 5, 1500
    truth = np.stack([R.blocks(rows, cols, classes, seed=90 + i, side=9) for i in range(batch)])
    labels = truth.copy()
    rng = np.random.default_rng(91)
    labels[:, :, 3:] = truth[:, :, :-3]                          # shifted
    noise = rng.random(labels.shape) < 0.03
    labels[noise] = rng.integers(0, classes, int(noise.sum()))
    labels[rng.random(labels.shape) < 0.02] = 255                # abstained
    truth[:, :8, :30] = 255                                      # void
    comps = pkg.Components(ctx, batch, batch * rows * cols)
    sides = []
    for maps in (labels, truth):
        d = (ctx.to_device(maps.astype(np.int32)), ctx.alloc(4 * maps.size), ctx.alloc(32 * batch * max_regions), ctx.alloc(4 * batch))
        ctx.components(comps, d[0].ptr, batch, rows, cols, classes, d[3].ptr, comp=d[1].ptr, regions=d[2].ptr, connectivity=8, min_area=2,
                       max_regions=max_regions)
        sides.append(d)
    pq0 = np.zeros(classes * 4 + TAIL, np.uint64)
    pq0[classes * 4:] = SENT64
    d_pq, d_scored = ctx.to_device(pq0), ctx.to_device(np.full(batch, SENT, np.int32))
    ctx.panoptic(pan, d_pq.ptr, d_scored.ptr, sides[0][1].ptr, sides[0][2].ptr, sides[0][3].ptr, max_regions, sides[1][1].ptr, sides[1][2].ptr,
                 sides[1][3].ptr, max_regions, batch, rows, cols, classes)
    ctx.sync()
    want, exact = np.zeros((classes, 4), np.uint64), [Fraction(0)] * classes
    for i in range(batch):
        p, t = R.components(labels[i], classes, 8, 2, 0), R.components(truth[i], classes, 8, 2, 0)
        assert len(p[1]) <= max_regions and len(t[1]) <= max_regions
        r = P.panoptic(p[0], p[1], t[0], t[1], classes)
        want += r.pq
        exact = [a + b for a, b in zip(exact, r.exact)]
    got = d_pq.download((classes * 4 + TAIL,), np.uint64)
    assert np.array_equal(got[:classes * 4].reshape(classes, 4), want) and (got[classes * 4:] == SENT64).all()
    assert d_scored.download((batch,), np.int32).tolist() == [1] * batch
    assert want[:, 0].sum() > 10 and want[:, 1].sum() > 10 and want[:, 2].sum() > 0
    # the metrics: the Python formulas on the same table bit for bit; the IoU sum of the reference within tp * 2^-32
    m, pq_c, sq_c, rq_c = pkg.panoptic_metrics(want, classes)
    ref, ref_pq, ref_sq, ref_rq = P.metrics(want)
    assert (m.pq, m.sq, m.rq, m.tp, m.fp, m.fn, m.classes_present) == ref
    assert np.array_equal(pq_c, ref_pq) and np.array_equal(sq_c, ref_sq) and np.array_equal(rq_c, ref_rq) and m.classes_present == classes
    for c in range(classes):
        tp = int(want[c, 0])
        # what the metrics divide: ldexp ((double) S, -32), exact in a double while S < 2^53; sq_c is that over tp, one division
        s = math.ldexp(float(want[c, 3]), -32)
        assert Fraction(s) == Fraction(int(want[c, 3]), 1 << 32) and sq_c[c] == (s / tp if tp else 0.0)
        assert 0 <= exact[c] - Fraction(s) <= Fraction(tp, 1 << 32), "class %d: S * 2^-32 = %r against the exact sum %r" % (c, s, float(exact[c]))
    comps.close()
    for b in sides[0] + sides[1] + (d_pq, d_scored):
        b.free()


# -------------------------------------------------------------------------------------------------------------------- argument errors

def test_argument_errors(pkg, ctx):
    lib = ctx.lib
    images = _three(rows=6, cols=10, classes=3)[:2]
    h = pkg.Panoptic(ctx, 2, 2 * 40)
    c = Call(ctx, images, 3, 40, 30)
    base = dict(zip(("pq", "scored") + OUTPUTS + ("comp_pred", "pred", "n_pred", "max_pred", "comp_truth", "truth", "n_truth", "max_truth", "batch", "rows",
                                                "cols", "classes", "stream"), c.args()))

    def call(hh=h.h, **kw):
        a = dict(base)
        a.update(kw)
        return lib.mbn_panoptic_i32(hh, *a.values())

    assert call(hh=None) == pkg.EINVAL
    for name in ("pq", "scored", "comp_pred", "pred", "n_pred", "comp_truth", "truth", "n_truth"):
        assert call(**{name: None}) == pkg.EINVAL, name + " NULL"
    for name in POINTERS:
        for off in (1, 2, 3) + ((4,) if name == "pq" else ()):
            assert call(**{name: base[name] + off}) == pkg.EINVAL, "%s off its alignment by %d" % (name, off)
    for name in ("batch", "rows", "cols", "classes", "max_pred", "max_truth"):
        assert call(**{name: 0}) == pkg.EINVAL and call(**{name: -1}) == pkg.EINVAL, name
    assert call(batch=3, rows=1, cols=1) == pkg.EINVAL, "a batch beyond the handle"
    assert call(max_pred=41) == pkg.EINVAL and call(max_truth=41) == pkg.EINVAL, "more slots than the handle holds"
    assert call(batch=1, max_pred=80, max_truth=80, rows=1, cols=1) == pkg.EINVAL and "panoptic" in ctx.last_error(), "inside the handle, the tables are short"
    assert call(rows=1 << 14, cols=1 << 15, batch=1) == pkg.EUNSUPPORTED and call(classes=4097) == pkg.EUNSUPPORTED
    assert call(max_pred=(1 << 24) + 1) == pkg.EUNSUPPORTED and call(max_truth=(1 << 24) + 1) == pkg.EUNSUPPORTED and call(batch=65536) == pkg.EUNSUPPORTED
    assert call(batch=65536, rows=0) == pkg.EINVAL, "a caller error goes before a limit"

    def untouched(what):
        got = c.got()
        assert all(np.array_equal(got[k], c.fresh[k]) for k in got), what

    untouched("a refused uniform call wrote")
    # the bounds rule of mbn_alloc: an interior pointer leaves the call one element short. The call on the exact buffer is accepted and runs;
    # the refused one behind it must leave every output, that buffer included, as the accepted one left it
    for name in POINTERS:
        step = 8 if name == "pq" else 4
        size = c.d[name].nbytes // step - TAIL - 4
        exact = ctx.to_device(np.zeros(size, np.uint64 if name == "pq" else np.int32))
        assert call(**{name: exact.ptr}) == pkg.OK, name
        before, kept = c.got(), exact.download((size,), np.uint64 if name == "pq" else np.int32)
        assert call(**{name: exact.ptr + step}) == pkg.EINVAL and ("panoptic " + name) in ctx.last_error(), name
        after = c.got()
        assert all(np.array_equal(after[k], before[k]) for k in after), name + ": the refused call wrote"
        assert np.array_equal(exact.download((size,), np.uint64 if name == "pq" else np.int32), kept), name + ": the refused call wrote"
        exact.free()
        c.reset()
    r = pkg.RaggedReadout(ctx, 4)

    def ragged(hh=h.h, rr=r.h, **kw):
        a = dict(base)
        a.update(kw)
        for k in ("batch", "rows", "cols"):
            del a[k]
        return lib.mbn_panoptic_ragged_i32(hh, rr, *a.values())

    assert ragged() == pkg.EINVAL, "a handle without a set"
    assert ragged(rr=None) == pkg.EINVAL and ragged(hh=None) == pkg.EINVAL
    r.set(1, 1, 5, [(2, 4, 5), (60, 5, 8)])
    assert ragged(pq=None) == pkg.EINVAL and ragged(n_truth=None) == pkg.EINVAL and ragged(classes=0) == pkg.EINVAL and ragged(max_pred=0) == pkg.EINVAL
    assert ragged(comp_pred=base["comp_pred"] + 4 * 41) == pkg.EINVAL and "panoptic comp_pred" in ctx.last_error()   # the set reaches element 100 of 140
    assert ragged(max_truth=41) == pkg.EINVAL
    r.set(1, 1, 5, [(0, 4, 5), (20, 4, 5), (40, 4, 5)])
    assert ragged() == pkg.EINVAL, "a set of more maps than the handle holds"
    created = C.c_void_p()
    assert lib.mbn_panoptic_create(ctx.h, 0, 10, C.byref(created)) == pkg.EINVAL and lib.mbn_panoptic_create(ctx.h, 1, 0, C.byref(created)) == pkg.EINVAL
    assert lib.mbn_panoptic_create(None, 1, 10, C.byref(created)) == pkg.EINVAL and lib.mbn_panoptic_create(ctx.h, 1, 10, None) == pkg.EINVAL
    assert lib.mbn_panoptic_create(ctx.h, 65536, 10, C.byref(created)) == pkg.EUNSUPPORTED
    assert lib.mbn_panoptic_create(ctx.h, 1, (1 << 32) + 1, C.byref(created)) == pkg.EUNSUPPORTED and not created.value
    assert lib.mbn_panoptic_destroy(None) == pkg.OK
    untouched("a refused ragged call wrote")
    r.close()
    h.close()
    c.free()


# -------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS = 0.5, 21, 64, 96


def _net_truth(lab, items, rng):
    """a truth for the net's maps: the labels themselves, shifted by two columns, with some blocks of other classes and a void band"""
    truth = np.full(lab.size, 255, np.int32)
    for off, rows, cols in items:
        L = lab[off:off + rows * cols].reshape(rows, cols)
        T = np.roll(L, 2, axis=1)
        T[rows // 2:rows // 2 + 9, 5:40] = rng.integers(0, CLASSES)
        T[:4] = 255
        truth[off:off + rows * cols] = T.ravel()
    return truth


def _net_want(lab, truth, items, conn, min_area, max_regions):
    pq, scored = np.zeros((CLASSES, 4), np.uint64), []
    for off, rows, cols in items:
        p = R.components(lab[off:off + rows * cols].reshape(rows, cols), CLASSES, conn, min_area, 0)
        t = R.components(truth[off:off + rows * cols].reshape(rows, cols), CLASSES, conn, min_area, 0)
        scored.append(int(len(p[1]) <= max_regions and len(t[1]) <= max_regions))
        if scored[-1]:
            pq += P.panoptic(p[0], p[1], t[0], t[1], CLASSES).pq
    return pq, scored


def test_net_segment_panoptic(pkg, ctx, tmp_path):
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, 16)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 8)
    net.set_input_u8(True)
    rng = np.random.default_rng(6)
    n, sh, sw = 2, 75, 130
    src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    npix = n * sh * sw
    d_src, d_lab = ctx.to_device(src), ctx.alloc(4 * (npix + 64))
    d_t8, d_t32 = ctx.alloc(npix + 64), ctx.alloc(4 * (npix + 64))
    d_pq, d_scored = ctx.alloc(8 * (CLASSES * 4 + TAIL)), ctx.alloc(4 * (n + TAIL))
    assert ctx.lib.mbn_net_segment_panoptic(net.h, d_lab.ptr, d_t8.ptr, 1, 4, 1, d_pq.ptr, d_scored.ptr) == pkg.EINVAL, "before any segment call"

    def check(what, items, conn, min_area, max_regions):
        ctx.sync()
        lab = d_lab.download((npix + 64,), np.int32)
        truth = _net_truth(lab, items, np.random.default_rng(8))
        want, scored = _net_want(lab, truth, items, conn, min_area, max_regions)
        d_t8.upload(truth.astype(np.uint8))
        d_t32.upload(truth)
        for ptr, nbytes in ((d_t8.ptr, 1), (d_t32.ptr, 4)):
            pq0 = np.full(CLASSES * 4 + TAIL, SENT64, np.uint64)
            pq0[:CLASSES * 4] = 3
            d_pq.upload(pq0)
            d_scored.upload(np.full(n + TAIL, SENT, np.int32))
            net.segment_panoptic(d_lab.ptr, ptr, nbytes, d_pq.ptr, d_scored.ptr, connectivity=conn, min_area=min_area)
            ctx.sync()
            got, got_scored = d_pq.download((CLASSES * 4 + TAIL,), np.uint64), d_scored.download((n + TAIL,), np.int32)
            assert np.array_equal(got[:CLASSES * 4].reshape(CLASSES, 4), want + np.uint64(3)) and (got[CLASSES * 4:] == SENT64).all(), what
            assert got_scored[:len(items)].tolist() == scored and (got_scored[len(items):] == SENT).all(), what
            assert np.array_equal(d_lab.download((npix + 64,), np.int32), lab), what + ": the labels are only read"
        return want, scored

    uniform = [(i * sh * sw, sh, sw) for i in range(n)]
    net.segment_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr)
    want, scored = check("segment_fit", uniform, 4, 1, pkg.NET_PANOPTIC_REGIONS)
    assert scored == [1, 1] and want[:, 0].sum() > 0
    check("segment_fit, cleaned", uniform, 8, 10, pkg.NET_PANOPTIC_REGIONS)
    # a table too small for the regions of the maps: not scored, and that is reported
    net.set_panoptic_regions(1)
    want, scored = check("one region a side", uniform, 4, 1, 1)
    assert scored == [0, 0] and want.sum() == 0
    net.set_panoptic_regions(pkg.NET_PANOPTIC_REGIONS)
    # an image call: the net's own ragged set, truth at the labels' offsets; the gaps of a uint8 truth are widened into private scratch only
    rows, cols = [sh, 40], [sw, 50]
    offs, dst = [0, sh * sw * 3], [sh * sw + 11, 3]
    ctx.lib.mbn_memset(ctx.h, d_lab.ptr, 0xFF, 4 * (npix + 64))
    net.segment_images_fit(d_src.ptr, offs, rows, cols, pkg.FIT_PAD, d_lab.ptr, dst)
    want, scored = check("segment_images_fit", [(dst[i], rows[i], cols[i]) for i in range(2)], 8, 2, pkg.NET_PANOPTIC_REGIONS)
    assert scored == [1, 1] and want[:, 0].sum() > 0
    assert ctx.lib.mbn_net_set_panoptic_regions(net.h, 0) == pkg.EINVAL and ctx.lib.mbn_net_set_panoptic_regions(net.h, (1 << 24) + 1) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_net_segment_panoptic(net.h, d_lab.ptr, d_t8.ptr, 2, 4, 1, d_pq.ptr, d_scored.ptr) == pkg.EINVAL
    assert ctx.lib.mbn_net_segment_panoptic(net.h, d_lab.ptr, d_t32.ptr + 2, 4, 4, 1, d_pq.ptr, d_scored.ptr) == pkg.EINVAL
    assert ctx.lib.mbn_net_segment_panoptic(net.h, d_lab.ptr, d_t8.ptr, 1, 4, 1, None, d_scored.ptr) == pkg.EINVAL
    net.destroy()
    for b in (d_src, d_lab, d_t8, d_t32, d_pq, d_scored):
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def _pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    w, h, maxval = (int(g) for g in m.groups())
    return np.frombuffer(raw[m.end():], ">u2" if maxval > 255 else np.uint8).astype(np.int32).reshape(h, w)


def _write_pgm(path, a, maxval):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n%d\n" % (a.shape[1], a.shape[0], maxval))
        f.write(a.astype(">u2" if maxval > 255 else np.uint8).tobytes())


def test_c_host_panoptic(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    sh, sw, classes = 75, 130, 1000                             # the host's synthetic weights have 1000 classes
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, plain, out, truth_path = str(tmp_path / "a.ppm"), str(tmp_path / "plain.pgm"), str(tmp_path / "out.pgm"), str(tmp_path / "truth.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", "3", "--alpha", "0.5", "--res", "%dx%d" % (ROWS, COLS), "--output-stride", "16", "--ppm", ppm, "--fit", "pad"]
    r = subprocess.run(common + ["--segment-source", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "panoptic:" not in r.stdout, r.stdout + r.stderr
    L = _pgm(plain)
    # the truth: the map itself shifted by two columns, a void band (the class count: outside the classes) on top; two bytes per pixel
    T = np.roll(L, 2, axis=1)
    T[:4] = classes
    _write_pgm(truth_path, T, 65535)
    for conn, min_area, extra in ((4, 1, []), (8, 6, ["--connectivity", "8", "--min-area", "6"])):
        r = subprocess.run(common + ["--segment-source", out, "--truth", truth_path, "--panoptic"] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        p, t = R.components(L, classes, conn, min_area, 0), R.components(T, classes, conn, min_area, 0)
        assert len(p[1]) <= pkg.NET_PANOPTIC_REGIONS and len(t[1]) <= pkg.NET_PANOPTIC_REGIONS
        want = P.panoptic(p[0], p[1], t[0], t[1], classes).pq
        (head, pq_c, sq_c, rq_c) = P.metrics(want)
        line = re.search(r"^panoptic: (connectivity=.*)$", r.stdout, re.M).group(1)
        s = {k: v for k, v in (f.split("=") for f in line.split())}
        assert (int(s["connectivity"]), int(s["min_area"]), s["scored"], int(s["classes_present"])) == (conn, min_area, "1/1", head[6])
        assert (float(s["tp"]), float(s["fp"]), float(s["fn"])) == head[3:6] and (float(s["pq"]), float(s["sq"]), float(s["rq"])) == head[0:3]
        rows = [m.groups() for m in re.finditer(r"^panoptic_class: class (\d+) tp (\d+) fp (\d+) fn (\d+) pq (\S+) sq (\S+) rq (\S+)$", r.stdout, re.M)]
        present = [c for c in range(classes) if want[c, :3].sum() > 0]
        assert [int(g[0]) for g in rows] == present and head[3] > 0
        for g in rows:
            c = int(g[0])
            assert [int(v) for v in g[1:4]] == want[c, :3].tolist() and (float(g[4]), float(g[5]), float(g[6])) == (pq_c[c], sq_c[c], rq_c[c])
        assert np.array_equal(_pgm(out), L), "the written map is the plain one"
    for bad in (["--segment-source", out, "--panoptic"], ["--truth", truth_path, "--panoptic"],
                ["--segment-source", out, "--truth", truth_path, "--panoptic", "--connectivity", "6"],
                ["--segment-source", out, "--truth", truth_path, "--panoptic", "--min-area", "0"],
                ["--segment-source", out, "--truth", truth_path, "--panoptic", "--max-regions", "7"]):
        r = subprocess.run(common + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "panoptic:" not in r.stdout, (bad, r.stdout + r.stderr)
