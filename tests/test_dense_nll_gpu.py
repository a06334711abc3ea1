"""Score the probabilities on the GPU. mbn_resample_nll_f32 / _ragged_f32 against the reference (tests/dense_nll_ref.py): the maps within
bound_nll / bound_brier (exactly the cap and exactly -1 where the rule says so), the table byte for byte the integer table of the DOWNLOADED planes;
the identities with the argmax, softmax and confusion calls; the wave aggregation's paths; accumulation, planning CU counts and graph replay; the
ragged form; the temperature fit end to end; the net runner's segment_nll; every status.

Every comparison prints its largest errors in units of their bounds before it asserts (pytest -s shows them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dense_nll_ref as R
from test_dense_any_gpu import TAIL, _ragged_layout
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

FILL = 77.0             # the sentinel of both maps
WORST = {"nll": 0.0, "brier": 0.0}      # the largest errors seen in this run, in units of the bounds


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _f32(betas):
    return [float(np.float32(b)) for b in betas]


def _run(ctx, x, truth, H, W, betas, window=None, offset=0, with_nll=True, with_brier=True, table=None, calls=1):
    """mbn_resample_nll_f32 on x [n][h][w][classes] and truth [n][H][W] (uint8 or int32); every buffer is uploaded `offset` bytes (the table twice
    that) into its allocation. (table uint64 [temps][classes + 1][4], nll or None, brier or None), the maps [temps][n][H][W]. The maps carry a
    sentinel and TAIL more elements; `table` preloads the device table (default zeros)."""
    n, h, w, classes = x.shape
    temps = len(betas)
    npix = temps * n * H * W
    pad = offset // 4
    d_x = ctx.to_device(np.concatenate([np.zeros(pad, np.float32), x.ravel()]))
    tb = truth.dtype.itemsize
    t_off = offset if tb == 4 else (1 if offset else 0)                                       # a uint8 truth at any byte
    d_t = ctx.to_device(np.concatenate([np.zeros(t_off // tb, truth.dtype), truth.ravel()]))
    cells = temps * (classes + 1) * 4
    d_tab = ctx.to_device(np.concatenate([np.zeros(2 * pad // 2, np.uint64), np.zeros(cells, np.uint64) if table is None else table.ravel()]))
    tab_off = 8 * (2 * pad // 2)
    maps = [ctx.to_device(np.full(pad + npix + TAIL, FILL, np.float32)) if on else None for on in (with_nll, with_brier)]
    R_, C_, rect = window if window else (0, 0, None)
    for _ in range(calls):
        ctx.resample_nll(d_tab.ptr + tab_off, maps[0].ptr + offset if maps[0] else None, maps[1].ptr + offset if maps[1] else None, d_x.ptr + offset,
                         d_t.ptr + t_off, tb, n, h, w, classes, H, W, betas, rect=rect, in_rows=R_, in_cols=C_)
    ctx.sync()
    tab = d_tab.download((2 * pad // 2 + cells,), np.uint64)
    assert (tab[:2 * pad // 2] == 0).all(), "written in front of the table"
    out = []
    for m in maps:
        if m is None:
            out.append(None)
            continue
        a = m.download((pad + npix + TAIL,), np.float32)
        assert (a[:pad] == FILL).all() and (a[pad + npix:] == FILL).all(), "written outside the planes"
        out.append(a[pad:pad + npix].reshape(temps, n, H, W))
    for b in [d_x, d_t, d_tab] + maps:
        if b is not None:
            b.free()
    return tab[2 * pad // 2:].reshape(temps, classes + 1, 4), out[0], out[1]


def _compare_maps(nll, brier, d, classes, what):
    """the kernel's planes (either may be None) against the reference's details d"""
    valid = np.broadcast_to(d["valid"], d["nll"].shape)
    capped, plain = d["capped"] & valid, valid & ~d["capped"]
    if nll is not None:
        assert (nll[~valid] == -1).all(), "%s: a void pixel's nll is not -1" % what
        assert (nll[capped] == R.CAP).all(), "%s: a capped pixel's nll is not MBN_NLL_CAP" % what
        err = np.abs(nll.astype(np.float64) - d["nll"]) / R.bound_nll(classes, d["x_t"])
        worst = float(err[plain].max()) if plain.any() else 0.0
        WORST["nll"] = max(WORST["nll"], worst)
        print("%s: max nll error %.3f of its bound, largest nll %.4f, %d values, %d capped" % (what, worst, float(d["nll"].max()), nll.size, capped.sum()))
        assert worst <= 1.0, "%s: nll error %.3f of the bound" % (what, worst)
        assert (nll[valid] >= 0).all() and (nll[valid] <= R.CAP).all()
    if brier is not None:
        assert (brier[~valid] == -1).all(), "%s: a void pixel's brier is not -1" % what
        err = np.abs(brier.astype(np.float64) - d["brier"]) / R.bound_brier(classes)
        worst = float(err[valid].max()) if valid.any() else 0.0
        WORST["brier"] = max(WORST["brier"], worst)
        print("%s: max brier error %.3f of its bound" % (what, worst))
        assert worst <= 1.0, "%s: brier error %.3f of the bound" % (what, worst)
        assert (brier[valid] >= 0).all() and (brier[valid] <= 2).all()


def _check(ctx, x, truth, H, W, betas, what, **kw):
    v = R.interpolants(x, H, W, kw.get("window"))
    d = R.details(v, truth, betas)
    tab, nll, brier = _run(ctx, x, truth, H, W, betas, **kw)
    _compare_maps(nll, brier, d, x.shape[3], what)
    if nll is not None and brier is not None and kw.get("table") is None and kw.get("calls", 1) == 1:
        want = R.table(nll, brier, d["label"], truth, x.shape[3])
        assert np.array_equal(tab, want), "%s: the table is not the integer table of the downloaded planes" % what
    return tab, nll, brier, d


def _truth(shape, classes, seed, dtype=None):
    return R.truth_map(shape, classes, seed, dtype or (np.uint8 if classes < 255 else np.int32))


# ------------------------------------------------------------------------------------------------------------- against the reference

@pytest.mark.parametrize("classes", [1, 3, 21, 64, 130, 260])
def test_classes(pkg, ctx, classes):
    """(2, 5, 7) -> 37 x 61: 2 x 2 tiles, partial tiles, rows that cross a coarse row. 3 / 21: dword loads and NaN padding; 64: 16-byte loads;
    130: two chunks, dword; 260: three chunks, 16-byte"""
    x = R.logits(2, 5, 7, classes, seed=classes)
    truth = _truth((2, 37, 61), classes, classes + 1)
    tab, nll, brier, d = _check(ctx, x, truth, 37, 61, [0.5, 1.0, 2.0], "5x7x%d -> 37x61" % classes)
    if classes == 1:
        assert (nll[:, d["valid"]] == 0).all() and (brier[:, d["valid"]] == 0).all() and (tab[:, 0, 1:3] == 0).all()
    assert (tab[:, :, 0].sum(axis=1) == truth.size).all()


@pytest.mark.parametrize("temps", [1, 3, 4, 5, 8])
def test_temperatures(pkg, ctx, temps):
    """every capacity boundary (1 | 2..4 | 5..8), beta drawn from {1/16, 1/2, 1, 2, 16}"""
    betas = (R.BETAS[temps % 5:] + R.BETAS + R.BETAS)[:temps]
    x = R.logits(2, 5, 7, 21, seed=40 + temps)
    _check(ctx, x, _truth((2, 37, 61), 21, temps), 37, 61, betas, "temps %d betas %s" % (temps, betas))


def test_truth_and_shapes(pkg, ctx):
    x = R.logits(2, 5, 7, 21, seed=3)
    t32 = _truth((2, 37, 61), 21, 5, np.int32)
    assert (t32 == -1).any() and (t32 == 21).any()
    got32 = _check(ctx, x, t32, 37, 61, [1.0, 16.0], "int32 truth")
    t8 = np.where((t32 < 0) | (t32 >= 21), 255, t32).astype(np.uint8)
    got8 = _check(ctx, x, t8, 37, 61, [1.0, 16.0], "uint8 truth")
    for a, b in zip(got32[:3], got8[:3]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    # interior pointers on every buffer: 4 bytes off 16 (the logits take the dword path), the table 8 off, a uint8 truth 1 byte off
    for truth in (t8, t32):
        off = _check(ctx, x, truth, 37, 61, [1.0, 16.0], "interior pointers, %s truth" % truth.dtype, offset=4)
        for a, b in zip(off[:3], got8[:3]):
            assert np.array_equal(a.view(np.uint64 if a.dtype == np.uint64 else np.uint32), b.view(np.uint64 if b.dtype == np.uint64 else np.uint32))
    x64 = R.logits(2, 5, 7, 64, seed=4)
    t64 = _truth((2, 37, 61), 64, 6)
    a = _check(ctx, x64, t64, 37, 61, [2.0], "64 classes on 16 bytes")
    b = _check(ctx, x64, t64, 37, 61, [2.0], "64 classes 4 bytes off", offset=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(_bits(a[2]), _bits(b[2]))
    # smaller than a tile, two chunks
    _check(ctx, R.logits(1, 2, 2, 130, seed=103, sigma=1.0), _truth((1, 11, 9), 130, 7), 11, 9, [0.5, 2.0], "2x2x130 -> 11x9")
    # a rectangle of a 160 x 224 input
    window = (160, 224, (56, 0, 112, 160))
    both = _check(ctx, x, _truth((2, 40, 56), 21, 8), 40, 56, [1.0, 2.0, 0.5], "window", window=window)
    # each map NULL in turn: the other map and the table are unchanged
    only_n = _check(ctx, x, _truth((2, 40, 56), 21, 8), 40, 56, [1.0, 2.0, 0.5], "window, brier NULL", window=window, with_brier=False)
    only_b = _check(ctx, x, _truth((2, 40, 56), 21, 8), 40, 56, [1.0, 2.0, 0.5], "window, nll NULL", window=window, with_nll=False)
    neither = _run(ctx, x, _truth((2, 40, 56), 21, 8), 40, 56, [1.0, 2.0, 0.5], window=window, with_nll=False, with_brier=False)
    assert only_n[2] is None and only_b[1] is None
    assert np.array_equal(_bits(only_n[1]), _bits(both[1])) and np.array_equal(_bits(only_b[2]), _bits(both[2]))
    assert np.array_equal(only_n[0], both[0]) and np.array_equal(only_b[0], both[0]) and np.array_equal(neither[0], both[0])


def test_non_finite_logits(pkg, ctx):
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    n, h, w, classes, H, W = 2, 3, 3, 133, 13, 17
    truth = np.full((n, H, W), 7, np.uint8)
    betas = [0.5, 1.0, 16.0]
    x = R.logits(n, h, w, classes, seed=5)
    x[..., 7] = nan                                                                          # a NaN at the truth class, everywhere
    tab, nll, brier, d = _check(ctx, x, truth, H, W, betas, "NaN at the truth")
    assert d["capped"].all() and (nll == R.CAP).all() and (brier >= 1).all() and (tab[:, 7, 1] == truth.size * int(R.CAP * R.ONE_NLL)).all()
    x = R.logits(n, h, w, classes, seed=5)
    x[..., 9] = nan                                                                          # a NaN elsewhere: it adds nothing
    tab, nll, brier, d = _check(ctx, x, truth, H, W, betas, "NaN elsewhere")
    assert not d["capped"].any() and (nll < R.CAP).all()
    x = R.logits(n, h, w, classes, seed=5)
    x[0, 1, 1, 20] = inf                                                                     # a +inf winner around one coarse sample
    tab, nll, brier, d = _check(ctx, x, truth, H, W, betas, "+inf winner")
    hit = d["capped"][0]
    assert hit.any() and not hit.all() and (nll[0][hit] == R.CAP).all() and (brier[0][hit] == 1).all() and (d["label"][hit] == 20).all()
    x[0] = -inf                                                                              # an image where nothing wins
    tab, nll, brier, d = _check(ctx, x, truth, H, W, betas, "all -inf")
    assert (nll[:, 0] == R.CAP).all() and (brier[:, 0] == 1).all() and (d["label"][0] == 0).all() and (nll[:, 1] < R.CAP).all()
    x = R.logits(n, h, w, classes, seed=5)
    x[..., 7] = -inf                                                                         # -inf at the truth under a finite best
    tab, nll, brier, d = _check(ctx, x, truth, H, W, betas, "-inf at the truth")
    assert (nll == R.CAP).all() and (brier >= 1).all()


def test_large_nll_stays_in_the_log_domain(pkg, ctx):
    """an ascending ramp of 0.5 a class over 130 classes at beta = 16, truth class 0: p_t underflows, the NLL is about 1032, finite and in bound"""
    x = np.broadcast_to((np.arange(130) * 0.5).astype(np.float32), (1, 2, 2, 130)).copy()
    truth = np.zeros((1, 11, 9), np.uint8)
    tab, nll, brier, d = _check(ctx, x, truth, 11, 9, [16.0, 1.0], "ramp at beta 16")
    assert (np.abs(nll[0] - 1032.0) < 0.01).all() and (nll[0] < R.CAP).all() and (np.abs(nll[1] - 64.5 - np.log(1 / (1 - np.exp(-0.5)))) < 1e-3).all()
    assert np.exp(-float(nll[0].max())) == 0.0, "p_t underflows even in float64"
    assert (np.abs(brier[0] - 2.0) < 1e-3).all()


# ------------------------------------------------------------------------------------------------------------------------ identities

def test_identities(pkg, ctx):
    n, h, w, classes, H, W = 2, 5, 7, 64, 37, 61
    x = R.logits(n, h, w, classes, seed=9)
    truth = _truth((n, H, W), classes, 10)
    winner = R.from_interpolants(R.interpolants(x, H, W), truth, [1.0])[0]
    truth = np.where(np.random.default_rng(11).random(truth.shape) < 0.5, winner, truth).astype(np.uint8)      # half of the pixels: the truth is the winner
    npix = n * H * W
    betas8 = _f32([1 / 16, 0.3, 0.5, 0.9, 1.0, 2.0, 7.0, 16.0])
    tab8, nll8, brier8, d = _check(ctx, x, truth, H, W, betas8, "eight temperatures")
    # against the argmax call's labels through mbn_confusion_i32, and the softmax call's prob
    d_x, d_t = ctx.to_device(x), ctx.to_device(truth)
    d_lab, d_pr, d_cnt = ctx.alloc(npix * 4), ctx.alloc(npix * 4), ctx.to_device(np.zeros((classes + 1) ** 2, np.uint64))
    ctx.resample_argmax(d_lab.ptr, None, d_x.ptr, n, h, w, classes, H, W)
    ctx.confusion(d_cnt.ptr, d_lab.ptr, d_t.ptr, 1, classes, npix)
    ctx.resample_softmax(d_lab.ptr, d_pr.ptr, None, d_x.ptr, n, h, w, classes, H, W)
    ctx.sync()
    counts = d_cnt.download((classes + 1, classes + 1), np.uint64)
    lab, prob = d_lab.download((n, H, W), np.int32), d_pr.download((n, H, W), np.float32)
    for b in (d_x, d_t, d_lab, d_pr, d_cnt):
        b.free()
    assert np.array_equal(lab, d["label"])
    for j in range(8):
        assert tab8[j, :classes, 3].sum() == counts[:classes, :classes].diagonal().sum(), "column 3 is the trace of the confusion matrix"
        assert np.array_equal(tab8[j, :classes, 0], counts[:classes].sum(axis=1)) and tab8[j, classes, 0] == counts[classes].sum()
        assert (tab8[j, classes, 1:] == 0).all()
    right = d["valid"] & (truth == lab)
    p = np.exp(-nll8[4].astype(np.float64))[right]                                           # beta = 1
    tol = (classes + 200) * 2.0 ** -24 * prob[right] + R.bound_nll(classes, 0.0) * p          # both bounds (x_t = 0: the truth is the winner)
    assert right.sum() > 100 and (np.abs(p - prob[right]) <= tol).all(), "exp(-nll) against mbn_resample_softmax_f32's prob"
    # inv_temps = [1, 1]: two identical planes
    tab, nll, brier = _run(ctx, x, truth, H, W, [1.0, 1.0])
    assert np.array_equal(_bits(nll[0]), _bits(nll[1])) and np.array_equal(_bits(brier[0]), _bits(brier[1])) and np.array_equal(tab[0], tab[1])
    # beta_j alone (capacity 1), among four (capacity 4) and among eight (capacity 8): the same bits
    for j in (0, 3, 4, 7):
        t1, n1, b1 = _run(ctx, x, truth, H, W, betas8[j:j + 1])
        assert np.array_equal(_bits(n1[0]), _bits(nll8[j])) and np.array_equal(_bits(b1[0]), _bits(brier8[j])) and np.array_equal(t1[0], tab8[j]), j
    t4, n4, b4 = _run(ctx, x, truth, H, W, betas8[2:6])
    assert np.array_equal(_bits(n4), _bits(nll8[2:6])) and np.array_equal(_bits(b4), _bits(brier8[2:6])) and np.array_equal(t4, tab8[2:6])
    # the full-input rect equals rect = NULL
    tf, nf, bf = _run(ctx, x, truth, H, W, betas8, window=(160, 224, (0, 0, 224, 160)))
    assert np.array_equal(_bits(nf), _bits(nll8)) and np.array_equal(_bits(bf), _bits(brier8)) and np.array_equal(tf, tab8)


# ----------------------------------------------------------------------------------------------------------------------- aggregation

def test_aggregation_paths(pkg, ctx):
    n, h, w, classes, H, W = 1, 5, 7, 130, 70, 61
    x = R.logits(n, h, w, classes, seed=12)
    betas = [0.5, 1.0, 2.0, 4.0, 8.0]
    const = np.full((n, H, W), 3, np.uint8)                                                  # one leader a wave
    tab, _, _, _ = _check(ctx, x, const, H, W, betas, "constant truth")
    assert (tab[:, 3, 0] == H * W).all() and (np.delete(tab, 3, axis=1) == 0).all()
    spread = np.broadcast_to((np.arange(W) % classes).astype(np.uint8), (n, H, W)).copy()     # every lane of a wave its own class
    tab, _, _, _ = _check(ctx, x, spread, H, W, betas, "truth = column mod classes")
    assert (tab[:, :W, 0] == H).all()
    mixed = np.where(np.arange(W)[None, None, :] < 40, spread, 200).astype(np.uint8)          # leaders, leftovers and void in one wave
    _check(ctx, x, mixed, H, W, betas, "mixed truth")
    void = np.full((n, H, W), 255, np.uint8)
    tab, nll, brier, _ = _check(ctx, x, void, H, W, betas, "all void")
    assert (tab[:, classes, 0] == H * W).all() and tab.sum() == len(betas) * H * W and (nll == -1).all() and (brier == -1).all()


# ------------------------------------------------------------------------------------------------ accumulation and determinism

def test_accumulation_planning_cus_and_replay(pkg, ctx):
    n, h, w, classes, H, W = 2, 5, 7, 21, 37, 61
    x = R.logits(n, h, w, classes, seed=13)
    truth = _truth((n, H, W), classes, 14)
    betas = [0.5, 1.0, 2.0]
    tab, nll, brier, _ = _check(ctx, x, truth, H, W, betas, "once")
    twice, n2, b2 = _run(ctx, x, truth, H, W, betas, calls=2)
    assert np.array_equal(twice, 2 * tab) and np.array_equal(_bits(n2), _bits(nll))
    onto = np.arange(tab.size, dtype=np.uint64).reshape(tab.shape)
    assert np.array_equal(_run(ctx, x, truth, H, W, betas, table=onto)[0], tab + onto), "the call adds to the table"
    try:
        for cus in (1, 3, 0):
            ctx.set_planning_cus(cus)
            t, a, b = _run(ctx, x, truth, H, W, betas)
            assert np.array_equal(t, tab) and np.array_equal(_bits(a), _bits(nll)) and np.array_equal(_bits(b), _bits(brier)), "planning CU count %d" % cus
    finally:
        ctx.set_planning_cus(0)
    # ONE kernel node, replayed twice: the same map bytes, 2 x the table
    npix = len(betas) * n * H * W
    d_x, d_t = ctx.to_device(x), ctx.to_device(truth)
    d_tab, d_n, d_b = ctx.to_device(np.zeros(tab.size, np.uint64)), ctx.to_device(np.full(npix, FILL, np.float32)), ctx.to_device(np.full(npix, FILL, np.float32))
    arr = (C.c_float * 3)(*betas)
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_resample_nll_f32(ctx.h, d_tab.ptr, d_n.ptr, d_b.ptr, d_x.ptr, d_t.ptr, 1, n, h, w, classes, 0, 0, None, H, W, arr, 3, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert (d_tab.download((tab.size,), np.uint64) == 0).all(), "the captured call ran"
    arr[0] = 9.0                                                                             # the temperatures travelled in the kernel's arguments
    for _ in range(2):
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(d_tab.download(tab.shape, np.uint64), 2 * tab)
    assert np.array_equal(_bits(d_n.download(nll.shape, np.float32)), _bits(nll)) and np.array_equal(_bits(d_b.download(brier.shape, np.float32)), _bits(brier))
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    for b in (d_x, d_t, d_tab, d_n, d_b):
        b.free()


# ---------------------------------------------------------------------------------------------------------------------------- ragged

H5, W7, R5, C7 = 5, 7, 160, 224
RAGGED_PLAIN = [(37, 61), (100, 30), (20, 28)]
RAGGED_WINDOW = [(37, 61, (0, 0, C7, R5)), (100, 30, (9, 11, 180, 120)), (40, 56, (56, 0, 112, 160))]


def _ragged_run(ctx, rd, d_x, truth_flat, elements, stride, betas, classes):
    temps = len(betas)
    total = (temps - 1) * stride + elements
    d_t = ctx.to_device(truth_flat)
    d_tab = ctx.to_device(np.zeros(temps * (classes + 1) * 4, np.uint64))
    d_n, d_b = ctx.to_device(np.full(total, FILL, np.float32)), ctx.to_device(np.full(total, FILL, np.float32))
    ctx.resample_nll_ragged(rd, d_tab.ptr, d_n.ptr, d_b.ptr, stride, d_x.ptr, d_t.ptr, truth_flat.dtype.itemsize, betas)
    ctx.sync()
    out = d_tab.download((temps, classes + 1, 4), np.uint64), d_n.download((total,), np.float32), d_b.download((total,), np.float32)
    return out, (d_t, d_tab, d_n, d_b)


def _ragged_compare(ctx, x, items, offs, truth_flat, got, stride, betas, window):
    """maps bit for bit and the table equal to the per-item uniform calls (themselves checked against the reference); the sentinel elsewhere"""
    tab, nll, brier = got
    classes = x.shape[3]
    touched = np.zeros(nll.size, bool)
    want_tab = np.zeros_like(tab)
    for i, (it, off) in enumerate(zip(items, offs)):
        H, W = it[0], it[1]
        truth = truth_flat[off:off + H * W].reshape(1, H, W)
        t1, n1, b1, _ = _check(ctx, x[i:i + 1], truth, H, W, betas, "ragged item %d alone" % i, window=(R5, C7, it[2]) if window else None)
        want_tab += t1
        for j in range(len(betas)):
            at = j * stride + off
            assert np.array_equal(_bits(nll[at:at + H * W]), _bits(n1[j].ravel())) and np.array_equal(_bits(brier[at:at + H * W]), _bits(b1[j].ravel())), (i, j)
            touched[at:at + H * W] = True
    assert np.array_equal(tab, want_tab), "the ragged table is not the sum of the items' tables"
    assert (nll[~touched] == FILL).all() and (brier[~touched] == FILL).all(), "written between the maps, between the planes or behind them"


def test_ragged(pkg, ctx):
    classes, betas = 21, [0.5, 1.0, 4.0]
    x = R.logits(3, H5, W7, classes, seed=79)
    d_x = ctx.to_device(x)
    rd = pkg.RaggedReadout(ctx, 3)
    lib = ctx.lib
    offs, elements = _ragged_layout(RAGGED_PLAIN, order=(2, 0, 1))                           # out of order, with gaps; `elements` includes the tail
    stride = elements + 11
    truth = np.full(elements, 200, np.uint8)                                                 # the garbage in the gaps: void values, never counted
    for i, ((H, W), off) in enumerate(zip(RAGGED_PLAIN, offs)):
        truth[off:off + H * W] = _truth((H * W,), classes, 80 + i)
    rd.set(H5, W7, classes, [(o, H, W) for o, (H, W) in zip(offs, RAGGED_PLAIN)])
    got, bufs = _ragged_run(ctx, rd, d_x, truth, elements, stride, betas, classes)
    _ragged_compare(ctx, x, RAGGED_PLAIN, offs, truth, got, stride, betas, window=False)
    assert got[0][:, :, 0].sum() == len(betas) * sum(H * W for H, W in RAGGED_PLAIN), "the gaps are uncounted"
    # the generation rule: a captured launch replayed under its own set adds, after a later set it adds nothing and writes nothing
    d_t, d_tab, d_n, d_b = bufs
    arr = (C.c_float * 3)(*betas)
    g = C.c_void_p()
    assert lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = lib.mbn_resample_nll_ragged_f32(rd.h, d_tab.ptr, d_n.ptr, d_b.ptr, stride, d_x.ptr, d_t.ptr, 1, arr, 3, None)
    assert lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    assert lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(d_tab.download(got[0].shape, np.uint64), 2 * got[0]), "a replay under its own set adds"
    # a window set on the same handle
    woffs, welements = _ragged_layout([(H, W) for H, W, _ in RAGGED_WINDOW], order=(1, 2, 0), gap=6)
    wtruth = np.full(welements, -3, np.int32)
    for i, ((H, W, _), off) in enumerate(zip(RAGGED_WINDOW, woffs)):
        wtruth[off:off + H * W] = _truth((H * W,), classes, 90 + i, np.int32)
    rd.set_window(H5, W7, classes, R5, C7, [(o, H, W, rect) for o, (H, W, rect) in zip(woffs, RAGGED_WINDOW)])
    wgot, wbufs = _ragged_run(ctx, rd, d_x, wtruth, welements, welements, betas, classes)
    _ragged_compare(ctx, x, RAGGED_WINDOW, woffs, wtruth, wgot, welements, betas, window=True)
    d_n.upload(np.full(got[1].size, FILL, np.float32))
    assert lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(d_tab.download(got[0].shape, np.uint64), 2 * got[0]), "a replay after a later set adds nothing"
    assert (d_n.download((got[1].size,), np.float32) == FILL).all(), "a replay after a later set wrote"
    assert lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    # the statuses of the ragged call: nothing is written
    w_t, w_tab, w_n, w_b = wbufs
    w_tab.upload(np.zeros(wgot[0].size, np.uint64))
    w_n.upload(np.full(wgot[1].size, FILL, np.float32))
    span = lib.mbn_ragged_readout_span(rd.h)
    f = lambda *v: (C.c_float * len(v))(*v)

    def call(tab=w_tab.ptr, nm=w_n.ptr, bm=w_b.ptr, st=welements, q=d_x.ptr, t=w_t.ptr, tb=4, b=f(*betas), temps=3, r=rd.h):
        return lib.mbn_resample_nll_ragged_f32(r, tab, nm, bm, st, q, t, tb, b, temps, None)

    assert call(st=span - 1) == pkg.EINVAL and call(temps=0) == pkg.EINVAL and call(temps=9, b=f(*([1.0] * 9))) == pkg.EINVAL
    assert call(tab=None) == pkg.EINVAL and call(q=None) == pkg.EINVAL and call(t=None) == pkg.EINVAL and call(b=None) == pkg.EINVAL
    assert call(tab=w_tab.ptr + 4) == pkg.EINVAL and call(nm=w_n.ptr + 2) == pkg.EINVAL and call(bm=w_b.ptr + 2) == pkg.EINVAL
    assert call(t=w_t.ptr + 2) == pkg.EINVAL and call(tb=2) == pkg.EINVAL
    assert call(b=f(0.5, float("nan"), 1.0)) == pkg.EINVAL and call(b=f(0.5, 17.0, 1.0)) == pkg.EINVAL
    assert call(st=welements + TAIL) == pkg.EINVAL                                           # the last plane would end past the tracked maps
    assert call(st=(1 << 39)) == pkg.EUNSUPPORTED
    fresh = pkg.RaggedReadout(ctx, 2)
    assert call(r=fresh.h) == pkg.EINVAL and call(r=None) == pkg.EINVAL                      # no set yet, no handle
    fresh.close()
    ctx.sync()
    assert (w_tab.download((wgot[0].size,), np.uint64) == 0).all() and (w_n.download((wgot[1].size,), np.float32) == FILL).all()
    assert call(st=span) == pkg.OK and call(nm=None, bm=None) == pkg.OK
    ctx.sync()
    rd.close()
    for b in (d_x,) + bufs + wbufs:
        b.free()


# ------------------------------------------------------------------------------------------------------------------- the temperature fit

def test_temperature_fit_end_to_end(pkg, ctx):
    """the truth was sampled from softmax(z), the kernel sees 2 z: the device table's minimum is at beta = 0.5 (tests/test_dense_nll_cpu.py checks
    that the reference's is, with 0.036 nats to the next plane)"""
    x, truth = R.fit_case()
    classes = R.FIT_SHAPE[3]
    tab, nll, brier, d = _check(ctx, x, truth, R.FIT_OUT[0], R.FIT_OUT[1], R.FIT_GRID, "fit case")
    b, beta, edge = pkg.nll_best(tab, classes, R.FIT_GRID)
    means = [pkg.nll_metrics(tab, classes, len(R.FIT_GRID), j)[0].nll for j in range(len(R.FIT_GRID))]
    print("fit case: device NLL per beta", dict(zip(R.FIT_GRID, np.round(means, 4))), "refined beta %.4f" % beta)
    assert (b, edge) == (R.FIT_BEST, 0) and 0.35 < beta < 0.7
    want = d["nll"].reshape(len(R.FIT_GRID), -1).mean(axis=1)
    assert np.abs(np.array(means) - want).max() < 2.0 ** -16 + float(R.bound_nll(classes, d["x_t"]).max())


# --------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS, BATCH = 0.25, 21, 64, 64, 3
SOURCE = (75, 130)


def test_net_segment_nll(pkg, ctx, tmp_path):
    n, betas = BATCH, [0.5, 1.0, 2.0]
    temps = len(betas)
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, 32)
    h, w = ROWS // 32, COLS // 32
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    lib = ctx.lib
    rng = np.random.default_rng(31)
    sh, sw = SOURCE
    npix = n * sh * sw
    src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    truth = _truth((npix,), CLASSES, 32)
    d_src, d_truth = ctx.to_device(src), ctx.to_device(truth)
    d_lab, d_pr = ctx.alloc(npix * 4), ctx.alloc(npix * 4)
    d_dense = ctx.alloc(n * h * w * CLASSES * 4)
    cells = temps * (CLASSES + 1) * 4
    seed = np.arange(cells, dtype=np.uint64)
    d_tab, d_want = ctx.to_device(seed), ctx.alloc(cells * 8)
    d_n, d_b, d_wn, d_wb = (ctx.alloc(temps * npix * 4) for _ in range(4))
    arr = (C.c_float * temps)(*betas)
    nll_call = lambda t=d_truth.ptr, tb=1, k=temps, tab=d_tab.ptr: lib.mbn_net_segment_nll(net.h, t, tb, arr, k, tab, d_n.ptr, d_b.ptr, npix)
    assert nll_call() == pkg.EINVAL                                                          # before any segment call
    net.set_input_u8(True)

    def same(what, m=npix):
        ctx.sync()
        assert np.array_equal(d_tab.download((cells,), np.uint64), d_want.download((cells,), np.uint64)), "%s: table" % what
        assert d_want.download((temps, CLASSES + 1, 4), np.uint64)[:, :, 0].sum() == temps * m
        for a, b in ((d_n, d_wn), (d_b, d_wb)):
            assert np.array_equal(a.download((temps * m,), np.uint32), b.download((temps * m,), np.uint32)), "%s: maps" % what

    def clear():
        assert lib.mbn_memset(ctx.h, d_tab.ptr, 0, cells * 8) == pkg.OK and lib.mbn_memset(ctx.h, d_want.ptr, 0, cells * 8) == pkg.OK

    # after segment_prob_fit (pad): the direct call with the letterbox rectangle on forward_dense of the same staged images
    net.segment_prob_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr, d_pr.ptr)
    # a refused call leaves the table and the record as they were
    assert nll_call(tb=2) == pkg.EINVAL and nll_call(k=9) == pkg.EINVAL and nll_call(t=None) == pkg.EINVAL and nll_call(tab=d_tab.ptr + 4) == pkg.EINVAL
    ctx.sync()
    assert np.array_equal(d_tab.download((cells,), np.uint64), seed)
    clear()
    net.segment_nll(d_truth.ptr, 1, betas, d_tab.ptr, d_n.ptr, d_b.ptr)
    staged = net.resize_input(d_src.ptr, n, sh, sw, fit=pkg.FIT_PAD)
    net.forward_dense(staged, d_dense.ptr, n)
    rect = pkg.fit_pad(sh, sw, ROWS, COLS)
    ctx.resample_nll(d_want.ptr, d_wn.ptr, d_wb.ptr, d_dense.ptr, d_truth.ptr, 1, n, h, w, CLASSES, sh, sw, betas, rect=rect, in_rows=ROWS, in_cols=COLS)
    same("after segment_prob_fit (pad)")
    # after segment_prob_fit (stretch): the whole map
    net.segment_prob_fit(d_src.ptr, n, sh, sw, pkg.FIT_STRETCH, d_lab.ptr, d_pr.ptr)
    clear()
    net.segment_nll(d_truth.ptr, 1, betas, d_tab.ptr, d_n.ptr, d_b.ptr)
    staged = net.resize_input(d_src.ptr, n, sh, sw, fit=pkg.FIT_STRETCH)
    net.forward_dense(staged, d_dense.ptr, n)
    ctx.resample_nll(d_want.ptr, d_wn.ptr, d_wb.ptr, d_dense.ptr, d_truth.ptr, 1, n, h, w, CLASSES, sh, sw, betas)
    same("after segment_prob_fit (stretch)")
    # after segment_prob_images_fit: the net's own set; equal-size images give the uniform call's bytes
    one = sh * sw
    net.segment_prob_images_fit(d_src.ptr, [i * one * 3 for i in range(n)], [sh] * n, [sw] * n, pkg.FIT_PAD, d_lab.ptr, [i * one for i in range(n)], d_pr.ptr)
    clear()
    net.segment_nll(d_truth.ptr, 1, betas, d_tab.ptr, d_n.ptr, d_b.ptr, plane_stride=npix)
    staged = net.resize_input(d_src.ptr, n, sh, sw, fit=pkg.FIT_PAD)
    net.forward_dense(staged, d_dense.ptr, n)
    ctx.resample_nll(d_want.ptr, d_wn.ptr, d_wb.ptr, d_dense.ptr, d_truth.ptr, 1, n, h, w, CLASSES, sh, sw, betas, rect=rect, in_rows=ROWS, in_cols=COLS)
    same("after segment_prob_images_fit")
    assert lib.mbn_net_segment_nll(net.h, d_truth.ptr, 1, arr, temps, d_tab.ptr, d_n.ptr, d_b.ptr, one * n - 1) == pkg.EINVAL      # the planes would overlap
    # after segment (the factor path): the whole-map call at out = 32 x map on the network-size images
    m = n * ROWS * COLS
    imgs = ctx.to_device(rng.integers(0, 256, (n, ROWS, COLS, 3), dtype=np.uint8))
    net.segment(imgs.ptr, n, d_lab.ptr)
    clear()
    net.segment_nll(d_truth.ptr, 1, betas, d_tab.ptr, d_n.ptr, d_b.ptr)
    net.forward_dense(imgs.ptr, d_dense.ptr, n)
    ctx.resample_nll(d_want.ptr, d_wn.ptr, d_wb.ptr, d_dense.ptr, d_truth.ptr, 1, n, h, w, CLASSES, ROWS, COLS, betas)
    same("after segment", m)
    # several presentations of an image: another probability model
    net.segment_views_fit(d_src.ptr, 1, sh, sw, [1.0, 0.75], [0, 1], d_lab.ptr, d_pr.ptr)
    assert nll_call() == pkg.EUNSUPPORTED
    big = ctx.to_device(rng.integers(0, 256, (1, 100, 64, 3), dtype=np.uint8))           # two tiles of 64 x 64
    net.segment_slide(big.ptr, 1, 100, 64, (64, 64), (36, 36), d_lab.ptr, d_pr.ptr)
    assert nll_call() == pkg.EUNSUPPORTED
    net.destroy()
    for b in (d_src, d_truth, d_lab, d_pr, d_dense, d_tab, d_want, d_n, d_b, d_wn, d_wb, imgs, big):
        b.free()
    hw.free()


# ------------------------------------------------------------------------------------------------------------------------ the C host

def test_c_host_nll(pkg, ctx, tmp_path):
    """mobilenet --truth --nll --temperatures: the lines are the mirror's numbers (Net.segment_nll, nll_metrics, nll_best), digit for digit"""
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    seed, alpha, os_, sh, sw, rows, cols, classes = 3, 0.5, 16, 75, 130, 64, 96, 1000
    rng = np.random.default_rng(41)
    src = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    truth = rng.integers(0, 40, (sh, sw)).astype(np.int32)
    truth[:, 0] = 65535                                                                      # a void column
    ppm, out, tr = (str(tmp_path / f) for f in ("a.ppm", "out.pgm", "truth.pgm"))
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    with open(tr, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (sw, sh) + truth.astype(">u2").tobytes())
    common = [exe, "--synthetic", str(seed), "--alpha", str(alpha), "--res", "%dx%d" % (rows, cols), "--output-stride", str(os_), "--ppm", ppm, "--fit", "pad"]
    run = lambda extra: subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
    for extra in (["--segment-source", out, "--nll"], ["--segment-source", out, "--truth", tr, "--temperatures", "1,2"],
                  ["--segment-source", out, "--truth", tr, "--nll", "--temperatures", "1,1"],
                  ["--segment-source", out, "--truth", tr, "--nll", "--temperatures", "0.01"],
                  ["--segment-source", out, "--truth", tr, "--nll", "--temperatures", "1,2,"],
                  ["--segment-source", out, "--truth", tr, "--nll", "--segment-topk", "3"]):
        r = run(extra)
        assert r.returncode == 2 and not os.path.exists(out), (extra, r.stdout + r.stderr)
    r = run(["--segment-source", out, "--truth", tr, "--nll", "--temperatures", "1,0.5,2"])
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [dict(p.split("=") for p in l.split()[1:]) for l in r.stdout.splitlines() if l.startswith("nll: ")]
    best = [dict(p.split("=") for p in l.split()[1:]) for l in r.stdout.splitlines() if l.startswith("nll_best: ")]
    assert len(lines) == 3 and len(best) == 1, r.stdout
    # the mirror
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    hw = pkg.HostWeights(path, res=(rows, cols), lib=pkg.load(), output_stride=os_)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 1)
    net.set_input_u8(True)
    betas = [0.5, 1.0, 2.0]                                                                  # T = 2, 1, 0.5: the CLI's order
    d_src, d_lab, d_pr, d_t = ctx.to_device(src), ctx.alloc(sh * sw * 4), ctx.alloc(sh * sw * 4), ctx.to_device(truth)
    d_tab = ctx.to_device(np.zeros(3 * (classes + 1) * 4, np.uint64))
    net.segment_prob_fit(d_src.ptr, 1, sh, sw, pkg.FIT_PAD, d_lab.ptr, d_pr.ptr)
    net.segment_nll(d_t.ptr, 4, betas, d_tab.ptr)
    ctx.sync()
    tab = d_tab.download((3, classes + 1, 4), np.uint64)
    net.destroy()
    for b in (d_src, d_lab, d_pr, d_t, d_tab):
        b.free()
    hw.free()
    for j, f in enumerate(lines):
        m = pkg.nll_metrics(tab, classes, 3, j)[0]
        assert float(f["temperature"]) == 1 / betas[j] and float(f["scored"]) == m.scored == sh * (sw - 1) and float(f["void"]) == m.void_pixels == sh
        assert float(f["nll"]) == m.nll and float(f["brier"]) == m.brier and float(f["mean_class_nll"]) == m.mean_class_nll and float(f["accuracy"]) == m.accuracy
    b, beta, edge = pkg.nll_best(tab, classes, betas)
    assert float(best[0]["temperature"]) == 1 / betas[b] and int(best[0]["at_edge"]) == edge
    assert np.isclose(float(best[0]["refined_temperature"]), 1 / beta, rtol=1e-15)


# -------------------------------------------------------------------------------------------------------------------------- statuses

def test_statuses(pkg, ctx):
    temps, classes, H, W = 3, 21, 16, 16
    x = ctx.to_device(np.zeros(2 * 2 * classes, np.float32))
    fill = np.full(temps * H * W, FILL, np.float32)
    zeros = np.zeros(temps * (classes + 1) * 4, np.uint64)
    nm, bm, tab = ctx.to_device(fill), ctx.to_device(fill), ctx.to_device(zeros)
    t8, t32 = ctx.to_device(np.zeros(H * W, np.uint8)), ctx.to_device(np.zeros(H * W, np.int32))
    lib = ctx.lib
    f = lambda *v: (C.c_float * len(v))(*v)
    rect_t = lambda *v: (C.c_int32 * 4)(*v)
    good = f(0.5, 1.0, 2.0)

    def nll(tb_=tab.ptr, n_=nm.ptr, b_=bm.ptr, q=x.ptr, t=t8.ptr, tb=1, n=1, h=2, w=2, c=classes, R_=0, C_=0, rect=None, H_=H, W_=W, b=good, k=temps, cx=ctx.h):
        return lib.mbn_resample_nll_f32(cx, tb_, n_, b_, q, t, tb, n, h, w, c, R_, C_, rect, H_, W_, b, k, None)

    # the caller's errors
    assert nll(cx=None) == pkg.EINVAL and nll(tb_=None) == pkg.EINVAL and nll(q=None) == pkg.EINVAL and nll(t=None) == pkg.EINVAL and nll(b=None) == pkg.EINVAL
    assert nll(tb_=tab.ptr + 4) == pkg.EINVAL and nll(n_=nm.ptr + 2) == pkg.EINVAL and nll(b_=bm.ptr + 2) == pkg.EINVAL and nll(q=x.ptr + 2) == pkg.EINVAL
    assert nll(t=t32.ptr + 2, tb=4) == pkg.EINVAL and nll(tb=2) == pkg.EINVAL and nll(tb=0) == pkg.EINVAL
    assert nll(k=0) == pkg.EINVAL and nll(k=-1) == pkg.EINVAL and nll(k=9, b=f(*([1.0] * 9))) == pkg.EINVAL
    for bad in (float("nan"), float("inf"), -1.0, 0.0, 0.06, 16.5):
        assert nll(b=f(0.5, bad, 2.0)) == pkg.EINVAL, bad
    for s in (dict(n=0), dict(h=0), dict(c=0), dict(W_=-1), dict(R_=64, C_=64, rect=rect_t(1, 0, 64, 64)), dict(R_=64, C_=64, rect=rect_t(-1, 0, 64, 64))):
        assert nll(**s) == pkg.EINVAL, s
    # the limits; an EINVAL goes in front
    for s in (dict(H_=7), dict(W_=7), dict(H_=16385), dict(n=65536), dict(c=pkg.CONFUSION_MAX_CLASSES + 1), dict(R_=64, C_=64, rect=rect_t(0, 0, 64, 64), H_=7)):
        assert nll(**s) == pkg.EUNSUPPORTED, s
        assert nll(b=f(0.5, 17.0, 2.0), **s) == pkg.EINVAL and nll(tb_=tab.ptr + 4, **s) == pkg.EINVAL and nll(tb=3, **s) == pkg.EINVAL, s
    # undersized tracked buffers: the table, each map (temps planes), the truth, the logits
    small_tab, two = ctx.to_device(zeros[:-1]), ctx.to_device(fill[:2 * H * W])
    assert nll(tb_=small_tab.ptr) == pkg.EINVAL and nll(n_=two.ptr) == pkg.EINVAL and nll(b_=two.ptr) == pkg.EINVAL
    assert nll(n=2, H_=8) == pkg.EINVAL and nll(t=t8.ptr + 1) == pkg.EINVAL and nll(t=t32.ptr + 4, tb=4) == pkg.EINVAL
    ctx.sync()
    assert np.array_equal(tab.download(zeros.shape, np.uint64), zeros), "a refusal added to the table"
    for m in (nm, bm, two):
        assert (m.download((2 * H * W,), np.float32) == FILL).all(), "a refusal wrote a map"
    # ... and what fits: two planes in the smaller maps, an int32 truth, both maps NULL. All-zero logits: nll = ln 21 at every temperature
    assert nll(n_=two.ptr, b_=two.ptr, k=2) == pkg.OK and nll(t=t32.ptr, tb=4) == pkg.OK and nll(n_=None, b_=None) == pkg.OK
    ctx.sync()
    got = nm.download((temps, H, W), np.float32)
    assert np.abs(got - np.log(21.0)).max() < 1e-5
    t = tab.download((temps, classes + 1, 4), np.uint64)
    assert (t[:2, 0, 0] == 3 * H * W).all() and t[2, 0, 0] == 2 * H * W and (t[:, 0, 3] == t[:, 0, 0]).all()
    for b in (x, nm, bm, tab, t8, t32, small_tab, two):
        b.free()


def test_report_worst_errors():
    """the largest errors of this run in units of the bounds (profiles/LOG.md records them); runs last in the file"""
    print("NLL and Brier: largest error %.3f of bound_nll, %.3f of bound_brier" % (WORST["nll"], WORST["brier"]))
    assert WORST["nll"] <= 1.0 and WORST["brier"] <= 1.0
