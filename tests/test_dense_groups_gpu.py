"""The group read-out on the GPU against tests/dense_groups_ref.py: EVERY label equal (test_dense_groups_cpu.py holds the inputs to a gap between
the two largest groups), prob and score inside the bounds of include/mbn.h; the threshold; the identity grouping against the softmax call; refusals;
the net runner against the context-level chain, its record and what follows it."""
import ctypes as C

import numpy as np
import pytest

import confusion_ref
import dense_groups_ref as ref
import dense_prob_ref
from test_dense_any_gpu import LAB_FILL, SC_FILL, TAIL
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu


def _device(pkg, ctx, x, group_of, groups, H, W, win=None, prob=True, score=True, min_prob=0.0, ignore=0):
    n, h, w, classes = x.shape                   # -> (labels, prob or None, score or None) [n][H][W]; the sentinels behind them must stay
    npix, cg, d_x = n * H * W, pkg.ClassGroups(ctx, group_of, groups), ctx.to_device(x)
    d_lab = ctx.to_device(np.full(npix + TAIL, LAB_FILL, np.int32))
    d_pr, d_sc = (ctx.to_device(np.full(npix + TAIL, SC_FILL, np.float32)) if on else None for on in (prob, score))
    ctx.resample_groups(cg, d_lab.ptr, d_pr.ptr if prob else None, d_sc.ptr if score else None, d_x.ptr, n, h, w, classes, H, W,
                        *(win or (0, 0, None)), min_prob, ignore)
    ctx.sync()
    out = [d_lab.download((npix + TAIL,), np.int32)] + [b.download((npix + TAIL,), np.float32) if b else None for b in (d_pr, d_sc)]
    cg.close()
    [b.free() for b in (d_x, d_lab, d_pr, d_sc) if b is not None]
    assert (out[0][npix:] == LAB_FILL).all() and all(o is None or (o[npix:] == SC_FILL).all() for o in out[1:]), "written past the last image"
    return [None if o is None else o[:npix].reshape(n, H, W) for o in out]


@pytest.mark.parametrize("name", ref.CASES)
def test_reference_parity(pkg, ctx, name):
    x, group_of, groups, sizes, win = ref.case(name)
    prob_bound, score_bound = ref.bounds(x.shape[-1], groups)
    for H, W in sizes:
        want_lab, want_pr, want_sc, m, _ = ref.from_interpolants(ref.interpolants(x, H, W, *(win or ())), group_of, groups)
        lab, pr, sc = _device(pkg, ctx, x, group_of, groups, H, W, win)
        what, finite = "%s to %dx%d" % (name, H, W), np.isfinite(m)
        assert np.array_equal(lab, want_lab), "%s: %d of %d labels differ" % (what, int((lab != want_lab).sum()), lab.size)
        err = np.abs(pr - want_pr) / np.where(want_pr > 0, want_pr, 1.0)
        print("%s: prob error %.3g of %.3g allowed" % (what, err.max(), prob_bound))
        assert (err <= prob_bound).all() and (pr[~finite] == 0).all(), what
        with np.errstate(invalid="ignore"):
            err = np.where(finite, np.abs(sc - want_sc) - np.abs(m) * 2.0 ** -24, np.where(sc == want_sc, 0.0, np.inf))
        print("%s: score error %.3g of %.3g allowed" % (what, err.max(), score_bound))
        assert (err <= score_bound).all(), what
        assert np.array_equal(_device(pkg, ctx, x, group_of, groups, H, W, win, prob=False, score=False)[0], want_lab), what + ", labels alone"
    if name == "one group":
        assert not lab.any()
    if name == "special":
        assert (~finite).any() and (lab[~finite] == 0).all() and (sc == np.inf).any() and (sc == -np.inf).any()
    if name == "window":                          # the window that covers the whole input is the NULL rectangle
        whole, plain = (_device(pkg, ctx, x, group_of, groups, H, W, w) for w in ((64, 96, (0, 0, 96, 64)), None))
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(whole, plain))


@pytest.mark.parametrize("with_prob", [True, False])
@pytest.mark.parametrize("name", ["padding", "dropped", "special"])
def test_threshold(pkg, ctx, name, with_prob):
    x, group_of, groups, ((H, W), *_), win = ref.case(name)
    want_lab, want_pr = ref.from_interpolants(ref.interpolants(x, H, W), group_of, groups)[:2]
    plain = _device(pkg, ctx, x, group_of, groups, H, W)
    lab, pr, sc = _device(pkg, ctx, x, group_of, groups, H, W, prob=with_prob, min_prob=ref.MIN_PROB, ignore=255)
    assert np.array_equal(lab, np.where(plain[1] < np.float32(ref.MIN_PROB), 255, plain[0])), "not the strict compare on the stored prob"
    assert np.array_equal(lab, dense_prob_ref.threshold(want_lab, want_pr, ref.MIN_PROB, 255)) and (lab == 255).any() and (lab != 255).any()
    assert np.array_equal(sc.view(np.uint32), plain[2].view(np.uint32)) and (pr is None or np.array_equal(pr.view(np.uint32), plain[1].view(np.uint32)))


def test_identity_grouping_is_the_softmax_call(pkg, ctx):
    x, group_of, groups, ((H, W),), _ = ref.case("identity")
    n, h, w, classes = x.shape
    lab, pr, sc = _device(pkg, ctx, x, group_of, groups, H, W)
    d_x, d_lab, d_pr, d_sc = ctx.to_device(x), ctx.alloc(lab.nbytes), ctx.alloc(lab.nbytes), ctx.alloc(lab.nbytes)
    ctx.resample_softmax(d_lab.ptr, d_pr.ptr, d_sc.ptr, d_x.ptr, n, h, w, classes, H, W)
    ctx.sync()
    s_lab, s_pr, s_sc = d_lab.download(lab.shape, np.int32), d_pr.download(lab.shape, np.float32), d_sc.download(lab.shape, np.float32)
    [b.free() for b in (d_x, d_lab, d_pr, d_sc)]
    assert np.array_equal(lab, s_lab)
    assert (np.abs(pr.astype(np.float64) - s_pr) <= (ref.bounds(classes, groups)[0] + dense_prob_ref.bound(classes)) * 1.001 * s_pr).all()
    assert (np.abs(sc.astype(np.float64) - s_sc) <= ref.bounds(classes, groups)[1] + np.abs(s_sc) * 2.0 ** -23).all(), "a group of one: its logit"


def test_refusals_launch_nothing(pkg, ctx):
    n, h, w, classes, H, W = 1, 3, 5, 4, 33, 70
    cg, other = pkg.ClassGroups(ctx, [0, 1, 1, -1], 2), pkg.ClassGroups(ctx, [0, 1, 1], 2)
    d_x = ctx.alloc(n * h * w * classes * 4)
    d_lab, d_sc = ctx.to_device(np.full(n * H * W, LAB_FILL, np.int32)), ctx.to_device(np.full(n * H * W, SC_FILL, np.float32))
    def call(g=cg.h, lab=d_lab.ptr, x=d_x.ptr, classes=classes, H=H, min_prob=0.0, rect=None):
        return ctx.lib.mbn_resample_groups_f32(ctx.h, g, lab, None, d_sc.ptr, x, n, h, w, classes, 64, 96, rect, H, W, min_prob, 0, None)
    assert call(H=4 * h - 1) == pkg.EUNSUPPORTED
    assert call(g=None) == pkg.EINVAL and call(g=other.h) == pkg.EINVAL and call(classes=3) == pkg.EINVAL, "the handle's class count"
    assert call(lab=None) == pkg.EINVAL and call(x=None) == pkg.EINVAL and call(lab=d_lab.ptr + 2) == pkg.EINVAL
    assert call(min_prob=1.5) == pkg.EINVAL and call(min_prob=float("nan")) == pkg.EINVAL
    assert call(rect=(C.c_int32 * 4)(0, 4, 97, 55)) == pkg.EINVAL
    made = C.c_void_p()
    bad = np.array([0, 2, 1], np.int32)
    assert ctx.lib.mbn_class_groups_create(ctx.h, 3, 2, bad.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(made)) == pkg.EINVAL and not made.value
    ctx.sync()
    assert (d_lab.download((n * H * W,), np.int32) == LAB_FILL).all() and (d_sc.download((n * H * W,), np.float32) == SC_FILL).all()
    cg.close(), other.close()
    [b.free() for b in (d_x, d_lab, d_sc)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_net_segment_groups_fit(pkg, ctx, tmp_path, dtype):
    CLASSES, GROUPS, SIDE, STRIDE, n, sh, sw, h, w = 11, 4, 64, 32, 2, 75, 130, 2, 2
    hw = _weights_os(pkg, tmp_path, 0.25, SIDE, SIDE, CLASSES, STRIDE)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_dtype(pkg.DT_BF16 if dtype == "bf16" else pkg.DT_F32)
    net.set_input_u8(True)
    cg, wrong = pkg.ClassGroups(ctx, np.arange(CLASSES) % 3 + 2 * (np.arange(CLASSES) > 8), GROUPS), pkg.ClassGroups(ctx, [0, 1], 2)
    rng = np.random.default_rng(5)
    truth = rng.integers(0, GROUPS, n * sh * sw, dtype=np.uint8)
    npix, d_src, d_truth = n * sh * sw, ctx.to_device(rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)), ctx.to_device(truth)
    d_dense, d_counts = ctx.alloc(n * h * w * CLASSES * 4), ctx.alloc((GROUPS + 1) ** 2 * 8)
    outs = [ctx.to_device(np.full(npix + TAIL, f, t)) for _ in range(2) for f, t in ((LAB_FILL, np.int32), (SC_FILL, np.float32), (SC_FILL, np.float32))]
    try:
        lib, a = ctx.lib, (d_src.ptr, n, sh, sw)
        assert lib.mbn_net_segment_groups_fit(net.h, cg.h, *a, pkg.FIT_CROP, outs[0].ptr, None, None, 0.0, 0) == pkg.EUNSUPPORTED
        assert lib.mbn_net_segment_groups_fit(net.h, wrong.h, *a, pkg.FIT_PAD, outs[0].ptr, None, None, 0.0, 0) == pkg.EINVAL
        assert lib.mbn_net_segment_groups_fit(net.h, cg.h, *a, pkg.FIT_PAD, outs[0].ptr, None, None, 2.0, 0) == pkg.EINVAL
        for fit in (pkg.FIT_STRETCH, pkg.FIT_PAD):
            net.segment_groups_fit(cg, d_src.ptr, n, sh, sw, fit, outs[0].ptr, outs[1].ptr, outs[2].ptr)
            d_counts.upload(np.zeros((GROUPS + 1) ** 2, np.uint64))
            net.segment_score(outs[0].ptr, d_truth.ptr, 1, d_counts.ptr)
            with pytest.raises(pkg.MbnError):
                net.segment_nll(d_truth.ptr, 1, [1.0], d_counts.ptr)
            staging = net.resize_input(d_src.ptr, n, sh, sw, fit=fit)
            net.forward_dense(staging, d_dense.ptr, n)
            ctx.resample_groups(cg, outs[3].ptr, outs[4].ptr, outs[5].ptr, d_dense.ptr, n, h, w, CLASSES, sh, sw, SIDE, SIDE,
                                tuple(pkg.fit_pad(sh, sw, SIDE, SIDE)) if fit == pkg.FIT_PAD else None)
            ctx.sync()
            got, want = ([b.download((npix + TAIL,), np.uint32) for b in outs[i:i + 3]] for i in (0, 3))
            assert all(np.array_equal(g, v) for g, v in zip(got, want)), "%s fit %d differs from the chain" % (dtype, fit)
            labels = got[0][:npix].view(np.int32)
            assert (got[0][npix:].view(np.int32) == LAB_FILL).all() and labels.min() >= 0 and labels.max() < GROUPS and np.unique(labels).size > 1
            counts = d_counts.download((GROUPS + 1, GROUPS + 1), np.uint64)
            assert np.array_equal(counts, confusion_ref.confusion(labels, truth, GROUPS)), "the confusion table is (groups + 1)^2 of group labels"
    finally:
        net.destroy()
        cg.close(), wrong.close()
        [b.free() for b in [d_src, d_truth, d_dense, d_counts] + outs]
        hw.free()
