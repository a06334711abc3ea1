"""Score the probabilities without a GPU: the reference (tests/dense_nll_ref.py) against independent formulations (torch.log_softmax / one_hot in
float64, scipy's logsumexp), its special cases, clamps and quantisation identities; mbn_nll_metrics, mbn_nll_best and mbn_resample_nll_envelope
through ctypes against numpy; and the temperature-fit case of the GPU test: its minimum is where that test will look."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import dense_nll_ref as R
import dense_prob_ref


def _cases():
    for case in dense_prob_ref.THRESHOLD_CASES[1:] + [(1, 2, 3, 1000, 9, 13, 104, 2.0, 0.0)]:
        n, h, w, classes, H, W, seed = case[:7]
        x = dense_prob_ref.threshold_input(case)
        yield x, R.interpolants(x, H, W), R.truth_map((n, H, W), classes, seed, np.int32)


def test_reference_against_torch_and_scipy():
    for x, v, truth in _cases():
        classes = v.shape[-1]
        d = R.details(v, truth, R.BETAS)
        valid = d["valid"]
        t = torch.from_numpy(np.where(valid, truth, 0).astype(np.int64))
        for j, beta in enumerate(np.asarray(R.BETAS, np.float32)):
            z = torch.from_numpy(v.astype(np.float64)) * float(beta)
            logp = torch.log_softmax(z, dim=-1)
            nll = -logp.gather(-1, t[..., None])[..., 0].numpy()
            brier = ((logp.exp() - torch.nn.functional.one_hot(t, classes).double()) ** 2).sum(-1).numpy()
            assert np.abs(d["nll"][j] - nll)[valid].max() < 1e-9 * max(1.0, nll[valid].max())
            assert np.abs(d["brier"][j] - brier)[valid].max() < 1e-12
            assert (d["nll"][j][~valid] == -1).all() and (d["brier"][j][~valid] == -1).all()
            try:
                from scipy.special import logsumexp
            except ImportError:
                continue
            zz = z.numpy()
            lse = logsumexp(zz, axis=-1) - np.take_along_axis(zz, t.numpy()[..., None], axis=-1)[..., 0]
            assert np.abs(d["nll"][j] - lse)[valid].max() < 1e-9 * max(1.0, lse[valid].max())
        lab, _ = dense_prob_ref.from_interpolants(v)[:2]
        assert np.array_equal(d["label"], lab)


def test_special_cases_and_clamps():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    v = np.zeros((6, 4), np.float32)
    v[0] = [1, 2, 3, 4]                       # plain
    v[1] = [1, nan, 3, 4]                     # a NaN at the truth (class 1)
    v[2] = [nan, 2, 3, 4]                     # a NaN elsewhere
    v[3] = [1, 2, inf, 4]                     # a +inf winner
    v[4] = [-inf, -inf, -inf, -inf]           # nothing wins
    v[5] = [1, -inf, 3, 4]                    # -inf at the truth under a finite best
    truth = np.array([1, 1, 1, 1, 1, 1])
    d = R.details(v, truth, [1.0, 2.0])
    e = np.exp(np.array([1.0, 2, 3, 4]) - 4)
    assert np.isclose(d["nll"][0, 0], np.log(e.sum()) + 2) and np.isclose(d["brier"][0, 0], ((e / e.sum() - [0, 1, 0, 0]) ** 2).sum())
    e3 = np.exp(np.array([1.0, 3, 4]) - 4)
    for i in (1, 5):
        assert d["nll"][0, i] == R.CAP and d["capped"][0, i] and np.isclose(d["brier"][0, i], 1 + (e3 ** 2).sum() / e3.sum() ** 2)
    e2 = np.exp(np.array([2.0, 3, 4]) - 4)
    assert np.isclose(d["nll"][0, 2], np.log(e2.sum()) + 2) and not d["capped"][0, 2]
    for i in (3, 4):
        assert d["nll"][0, i] == R.CAP and d["brier"][0, i] == 1.0 and d["capped"][1, i]
    assert list(d["label"]) == [3, 3, 3, 2, 0, 3]
    # the truth is the winner and alone: nll = brier = 0; one class: likewise
    one = R.details(np.array([[50.0, 0, 0, 0]], np.float32), np.array([0]), [16.0])
    assert one["nll"][0, 0] < 1e-300 and one["brier"][0, 0] < 1e-300
    one = R.details(np.array([[0.3]], np.float32), np.array([0]), [0.5])
    assert one["nll"][0, 0] == 0 and one["brier"][0, 0] == 0
    # the log domain: a ramp of 64.5 units at beta 16 is finite, about 1032, far from the cap; the cap needs a ramp beyond 2048 units
    ramp = (np.arange(130) * 0.5).astype(np.float32)[None]
    big = R.details(ramp, np.array([0]), [16.0])
    assert 1031.9 < big["nll"][0, 0] < 1032.1 and np.isclose(big["x_t"][0, 0], -1032.0)
    huge = R.details(np.array([[0.0, 4000.0]], np.float32), np.array([0]), [16.0])
    assert huge["nll"][0, 0] == R.CAP and not huge["capped"][0, 0], "the clamp, not a special case"
    # brier <= 2: all the mass on a wrong class
    assert np.isclose(R.details(np.array([[0.0, 90.0]], np.float32), np.array([0]), [1.0])["brier"][0, 0], 2.0)


def test_quantisation_identities():
    rng = np.random.default_rng(3)
    nll = np.concatenate([rng.random(500) * 40, [0.0, R.CAP, 1032.0003]]).astype(np.float32)
    brier = np.concatenate([rng.random(500) * 2, [0.0, 2.0, 1.0]]).astype(np.float32)
    for a, one, top in ((nll, R.ONE_NLL, 2 ** 31), (brier, R.ONE_BRIER, 2 ** 25)):
        prod32 = a * np.float32(one)                                                       # the kernel's fp32 product
        assert np.array_equal(prod32.astype(np.float64), a.astype(np.float64) * one), "the product is exact in fp32"
        assert (prod32.astype(np.float64) <= top).all() and top <= 2 ** 32 - 1
    classes = 5
    truth = rng.integers(-1, classes + 1, nll.size)
    label = rng.integers(0, classes, nll.size)
    tab = R.table(nll[None], brier[None], label, truth, classes)
    valid = (truth >= 0) & (truth < classes)
    assert tab[0, :, 0].sum() == nll.size and tab[0, classes, 0] == (~valid).sum() and (tab[0, classes, 1:] == 0).all()
    assert tab[0, :, 3].sum() == (label == truth)[valid].sum()
    assert tab[0, :, 1].sum() == int((nll[valid].astype(np.float64) * R.ONE_NLL).astype(np.uint64).astype(object).sum())
    # 2^33 pixels at the cap stay below 2^64
    assert 2 ** 33 * int(R.CAP * R.ONE_NLL) <= 2 ** 64


def _random_table(classes, temps, seed, empty=()):
    rng = np.random.default_rng(seed)
    tab = np.zeros((temps, classes + 1, 4), np.uint64)
    count = rng.integers(1, 1000, classes).astype(np.uint64)
    count[list(empty)] = 0
    for j in range(temps):
        tab[j, :classes, 0] = count
        tab[j, classes, 0] = 17
        tab[j, :classes, 1] = count * rng.integers(0, 40 * R.ONE_NLL, classes).astype(np.uint64)
        tab[j, :classes, 2] = count * rng.integers(0, 2 * R.ONE_BRIER, classes).astype(np.uint64)
        tab[j, :classes, 3] = (count * rng.random(classes)).astype(np.uint64)
    return tab


def test_metrics_against_numpy(pkg):
    for classes, temps, empty in ((1, 1, ()), (21, 3, (4, 20)), (300, 8, (0,))):
        tab = _random_table(classes, temps, classes, empty)
        for j in range(temps):
            m, cn, cb = pkg.nll_metrics(tab, classes, temps, j)
            want = R.metrics(tab, classes, temps, j)
            for f in ("pixels", "scored", "void_pixels", "nll", "brier", "accuracy", "mean_class_nll", "mean_class_brier", "classes_present"):
                assert getattr(m, f) == want[f], (classes, j, f)
            assert np.array_equal(cn, want["class_nll"], equal_nan=True) and np.array_equal(cb, want["class_brier"], equal_nan=True)
            assert np.isnan(cn[list(empty)]).all() and m.classes_present == classes - len(empty) and m.void_pixels == 17
    # an empty table: zeros, NaN per class
    m, cn, cb = pkg.nll_metrics(np.zeros((2, 4, 4), np.uint64), 3, 2, 1)
    assert (m.scored, m.nll, m.brier, m.accuracy, m.mean_class_nll, m.classes_present) == (0, 0, 0, 0, 0, 0) and np.isnan(cn).all() and np.isnan(cb).all()
    # NULL arrays, and the statuses
    lib = pkg.host_lib()
    tab = _random_table(3, 2, 1)
    p = tab.ctypes.data_as(C.POINTER(C.c_uint64))
    m = pkg.Nll()
    assert lib.mbn_nll_metrics(p, 3, 2, 0, C.byref(m), None, None) == pkg.OK and m.scored > 0
    for args in ((None, 3, 2, 0, C.byref(m)), (p, 0, 2, 0, C.byref(m)), (p, 3, 0, 0, C.byref(m)), (p, 3, 9, 0, C.byref(m)), (p, 3, 2, 2, C.byref(m)),
                 (p, 3, 2, -1, C.byref(m)), (p, 3, 2, 0, None), (p, 5000, 9, 0, C.byref(m))):
        assert lib.mbn_nll_metrics(*args, None, None) == pkg.EINVAL, args[1:4]
    assert lib.mbn_nll_metrics(p, pkg.CONFUSION_MAX_CLASSES + 1, 2, 0, C.byref(m), None, None) == pkg.EUNSUPPORTED


def _grid_table(classes, nlls, scored=1000):
    """a table whose plane j has the mean NLL nlls[j], all on class 0"""
    tab = np.zeros((len(nlls), classes + 1, 4), np.uint64)
    for j, v in enumerate(nlls):
        tab[j, 0, 0] = scored
        tab[j, 0, 1] = int(round(v * R.ONE_NLL)) * scored
    return tab


def test_best_against_numpy(pkg):
    grid = [0.25, 0.5, 1.0, 2.0, 4.0]
    for nlls in ([3, 2, 1.5, 2, 3], [1, 2, 3, 4, 5], [5, 4, 3, 2, 1], [2, 1, 1, 2, 3], [3, 3, 3, 3, 3], [3, 2.5, 1.0, 1.2, 4], [3, 1, 2, 0.5, 4]):
        tab = _grid_table(4, nlls)
        got = pkg.nll_best(tab, 4, grid)
        want = R.best(tab, 4, grid)
        assert got[0] == want[0] == int(np.argmin(nlls)) and got[2] == want[2] and np.isclose(got[1], want[1], rtol=1e-14), nlls
        if got[2]:
            assert got[1] == grid[got[0]], "no refinement at an edge"
    # a symmetric minimum on an even log grid stays put; a skewed one moves toward the lower neighbour, inside the neighbours
    assert np.isclose(pkg.nll_best(_grid_table(4, [3, 2, 1.5, 2, 3]), 4, grid)[1], 1.0)
    b, beta, edge = pkg.nll_best(_grid_table(4, [3, 1.6, 1.5, 2.5, 3]), 4, grid)
    assert (b, edge) == (2, 0) and 0.5 < beta < 1.0
    # the exact vertex of a parabola in ln beta on an UNEVEN grid
    ugrid = [0.3, 0.5, 1.1, 2.0]
    tab = _grid_table(2, [1 + (np.log(g) - np.log(0.8)) ** 2 for g in ugrid], scored=1)
    b, beta, edge = pkg.nll_best(tab, 2, ugrid)
    assert b in (1, 2) and edge == 0 and abs(beta - 0.8) < 2e-4                            # (the table rounds the NLLs to 2^-16)
    # a tie: the lowest index; one temperature: never an edge; a flat interior (a = 0): unrefined
    assert pkg.nll_best(_grid_table(4, [2, 1, 1, 2, 3]), 4, grid)[0] == 1
    assert pkg.nll_best(_grid_table(4, [2.0]), 4, [1.0]) == (0, 1.0, 0)
    assert pkg.nll_best(_grid_table(4, [3, 3, 3, 3, 3]), 4, grid) == (0, 0.25, 1)
    assert pkg.nll_best(_grid_table(4, [4, 3, 3, 3, 4]), 4, grid)[:1] == (1,)
    # nothing scored; the statuses
    assert pkg.nll_best(np.zeros((5, 5, 4), np.uint64), 4, grid) is None
    lib = pkg.host_lib()
    tab = _grid_table(4, [3, 2, 1.5, 2, 3])
    p, best = tab.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_int(-5)
    f = lambda *v: (C.c_float * len(v))(*v)
    assert lib.mbn_nll_best(p, 4, 5, f(*grid), C.byref(best), None, None) == pkg.OK and best.value == 2
    for g in (f(0.25, 0.5, 0.5, 2, 4), f(0.25, 0.5, 0.4, 2, 4), f(0, 0.5, 1, 2, 4), f(0.25, 0.5, float("nan"), 2, 4), f(0.25, 0.5, 1, 2, float("inf"))):
        assert lib.mbn_nll_best(p, 4, 5, g, C.byref(best), None, None) == pkg.EINVAL
    assert lib.mbn_nll_best(None, 4, 5, f(*grid), C.byref(best), None, None) == pkg.EINVAL
    assert lib.mbn_nll_best(p, 4, 5, None, C.byref(best), None, None) == pkg.EINVAL and lib.mbn_nll_best(p, 4, 5, f(*grid), None, None, None) == pkg.EINVAL
    assert lib.mbn_nll_best(p, 4, 0, f(*grid), C.byref(best), None, None) == pkg.EINVAL and lib.mbn_nll_best(p, 4, 9, f(*grid), C.byref(best), None, None) == pkg.EINVAL
    assert lib.mbn_nll_best(p, pkg.CONFUSION_MAX_CLASSES + 1, 5, f(*grid), C.byref(best), None, None) == pkg.EUNSUPPORTED
    assert lib.mbn_nll_best(np.zeros(100, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64)), 4, 5, f(*grid), C.byref(best), None, None) == pkg.ENOTFOUND
    assert best.value == 2, "nothing is written on a refusal"


def test_envelope(pkg):
    env = lambda n=1, h=2, w=2, c=21, R_=0, C_=0, rect=None, H=16, W=16, tb=1, temps=3: pkg.nll_envelope(n, h, w, c, R_, C_, rect, H, W, tb, temps)
    assert env() == pkg.OK and env(tb=4, temps=8) == pkg.OK and env(temps=1) == pkg.OK
    assert env(R_=64, C_=64, rect=(0, 0, 64, 64)) == pkg.OK
    for bad in (dict(tb=2), dict(tb=0), dict(temps=0), dict(temps=9), dict(n=0), dict(c=0), dict(H=-1), dict(R_=64, C_=64, rect=(1, 0, 64, 64))):
        assert env(**bad) == pkg.EINVAL, bad
    for lim in (dict(H=7), dict(H=16385), dict(n=65536), dict(c=pkg.CONFUSION_MAX_CLASSES + 1)):
        assert env(**lim) == pkg.EUNSUPPORTED, lim
    assert env(c=pkg.CONFUSION_MAX_CLASSES) == pkg.OK
    assert env(H=7, temps=9) == pkg.EINVAL and env(c=5000, tb=3) == pkg.EINVAL, "an EINVAL goes in front of an EUNSUPPORTED"
    # the shape part is the argmax / window call's
    for s in (dict(H=7), dict(W=7), dict(h=0), dict(n=65536)):
        a = dict(n=1, h=2, w=2, c=21, H=16, W=16)
        a.update(s)
        assert env(**s) == pkg.resample_argmax_envelope(a["n"], a["h"], a["w"], a["c"], a["H"], a["W"])
    lib = pkg.host_lib()
    assert lib.mbn_resample_nll_ragged_check(21, 100, 1, 3, 100) == pkg.OK and lib.mbn_resample_nll_ragged_check(21, 100, 1, 3, 99) == pkg.EINVAL
    assert lib.mbn_resample_nll_ragged_check(21, 100, 1, 8, (1 << 37) + 1) == pkg.EUNSUPPORTED
    assert lib.mbn_resample_nll_ragged_check(21, 100, 2, 3, 100) == pkg.EINVAL and lib.mbn_resample_nll_ragged_check(21, 100, 1, 9, 1 << 38) == pkg.EINVAL
    f = lambda *v: (C.c_float * len(v))(*v)
    assert lib.mbn_nll_temps_check(f(1 / 16, 16.0, 1.0), 3) == pkg.OK and lib.mbn_nll_temps_check(f(1.0, 1.0), 2) == pkg.OK
    for g in (f(0.06), f(16.5), f(float("nan")), f(float("inf")), f(-1.0), f(0.0)):
        assert lib.mbn_nll_temps_check(g, 1) == pkg.EINVAL
    assert lib.mbn_nll_temps_check(None, 1) == pkg.EINVAL and lib.mbn_nll_temps_check(f(1.0), 0) == pkg.EINVAL
    assert pkg.NLL_MAX_TEMPS == R.MAX_TEMPS == 8 and pkg.NLL_CAP == R.CAP and pkg.NLL_ONE == R.ONE_NLL and pkg.CALIBRATION_ONE == R.ONE_BRIER


@functools.lru_cache(None)
def _fit_reference():
    x, truth = R.fit_case()
    d = R.details(R.interpolants(x, *R.FIT_OUT), truth, R.FIT_GRID)
    return d, truth


def test_fit_case_has_its_minimum_where_the_gpu_test_looks(pkg):
    d, truth = _fit_reference()
    assert d["valid"].all() and not d["capped"].any()
    nll = d["nll"].reshape(len(R.FIT_GRID), -1).mean(axis=1)
    print("fit case: reference NLL per beta", dict(zip(R.FIT_GRID, np.round(nll, 4))))
    assert int(nll.argmin()) == R.FIT_BEST
    gap = float(np.sort(nll)[1] - nll.min())
    classes = R.FIT_SHAPE[3]
    worst = float(R.bound_nll(classes, d["x_t"]).max())
    assert gap > 0.01 and gap > 100 * worst, "the next plane is %g nats away, the tolerance %g" % (gap, worst)
    # and the host functions on the reference's own table answer what the GPU test will ask of the device's
    n32, b32 = R.quantise(d["nll"], d["brier"])
    tab = R.table(n32, b32, d["label"], truth, classes)
    b, beta, edge = pkg.nll_best(tab, classes, R.FIT_GRID)
    assert (b, edge) == (R.FIT_BEST, 0) and 0.35 < beta < 0.7
    m = pkg.nll_metrics(tab, classes, len(R.FIT_GRID), b)[0]
    assert abs(m.nll - nll[b]) < 1e-4 and m.scored == truth.size
