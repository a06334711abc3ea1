"""Score the probabilities: the normative arithmetic of mbn_resample_nll_f32 / _ragged_f32 and of mbn_nll_metrics / mbn_nll_best (include/mbn.h,
"Score the probabilities") in numpy, on top of dense_any_ref / dense_window_ref. The interpolated logits v are theirs, in float32, bit for bit;
best and label follow their argmax rule. Per inverse temperature beta (fp32) the scores are the FLOAT64 evaluation of

    x_c = beta (v_c - best);  e_c = exp(x_c), 0 for a NaN v_c;  S = sum e_c;  Q = sum e_c^2;  nll = log S - x_t;  brier = 1 - 2 e_t / S + Q / S^2

with the header's special cases and clamps. The kernel's fp32 maps are held to bound_nll / bound_brier; its table is integer and must equal
table(...) of the planes it stored, byte for byte."""
import numpy as np

import dense_any_ref
import dense_window_ref

MAX_TEMPS = 8
CAP = 32768.0
ONE_NLL = 1 << 16       # the fixed point of column 1
ONE_BRIER = 1 << 24     # the fixed point of column 2
BETAS = [1 / 16, 1 / 2, 1.0, 2.0, 16.0]


def bound_nll(classes, x_t):
    """the absolute error a kernel's nll may have outside the capped cases (include/mbn.h derives it); x_t = beta (v_t - best)"""
    return (classes + 200 + 4.0 * np.abs(x_t)) * 2.0 ** -24


def bound_brier(classes):
    """the absolute error a kernel's brier may have"""
    return 4.0 * (classes + 200) * 2.0 ** -24


def _argmax(v):
    nan = np.isnan(v)
    cand = np.where(nan, np.float32(-np.inf), v)
    label = cand.argmax(axis=-1).astype(np.int32)                  # the first of equal maxima; 0 when every candidate is -inf
    best = np.take_along_axis(cand, label[..., None].astype(np.int64), axis=-1)[..., 0]
    return label, best


def details(v, truth, inv_temps):
    """v float32 [..., classes], truth int [...] -> dict: label int32 [...], valid bool [...] (the truth is a class), and per temperature
    [temps, ...]: nll and brier float64 (-1 on void pixels), x_t float64 (0 where there is none), capped bool (nll is MBN_NLL_CAP by a special
    case, not by the formula)"""
    v = np.asarray(v, np.float32)
    classes = v.shape[-1]
    t = np.asarray(truth).astype(np.int64)
    assert t.shape == v.shape[:-1]
    valid = (t >= 0) & (t < classes)
    tc = np.where(valid, t, 0)
    label, best = _argmax(v)
    finite = np.isfinite(best)
    nan = np.isnan(v)
    v_t = np.take_along_axis(v, tc[..., None], axis=-1)[..., 0]
    have = finite & (v_t > -np.inf)                                # not for a NaN, not for -inf
    betas = np.asarray(inv_temps, np.float32)
    assert 1 <= betas.size <= MAX_TEMPS
    out = {k: [] for k in ("nll", "brier", "x_t", "capped")}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        d = v.astype(np.float64) - np.where(finite, best, np.float32(0)).astype(np.float64)[..., None]
        d_t = np.where(have, v_t.astype(np.float64) - best.astype(np.float64), 0.0)
        for beta in betas.astype(np.float64):
            e = np.where(nan, 0.0, np.exp(beta * d))
            S, Q = e.sum(axis=-1), (e * e).sum(axis=-1)
            S = np.where(finite, S, 1.0)
            x_t = beta * d_t
            nll = np.where(have, np.log(S) - x_t, CAP)
            brier = np.where(have, 1.0 - 2.0 * np.exp(x_t) / S + Q / (S * S), 1.0 + Q / (S * S))
            brier = np.where(finite, brier, 1.0)
            out["nll"].append(np.where(valid, np.clip(nll, 0.0, CAP), -1.0))
            out["brier"].append(np.where(valid, np.clip(brier, 0.0, 2.0), -1.0))
            out["x_t"].append(np.where(valid, x_t, 0.0))
            out["capped"].append(valid & ~have)
    out = {k: np.stack(a) for k, a in out.items()}
    out["label"], out["valid"] = label, valid
    return out


def from_interpolants(v, truth, inv_temps):
    """(label int32 [...], nll float64 [temps, ...], brier float64 [temps, ...]); -1 in both on void pixels"""
    d = details(v, truth, inv_temps)
    return d["label"], d["nll"], d["brier"]


def interpolants(x, H, W, window=None):
    """the fp32 v [n][H][W][classes] of x [n][h][w][classes]; window = (in_rows, in_cols, rect) or None for the whole map"""
    return dense_any_ref.resample(x, H, W) if window is None else dense_window_ref.resample_window(x, window[0], window[1], window[2], H, W)


def table(nll32, brier32, label, truth, classes):
    """uint64 [temps][classes + 1][4] from the STORED fp32 planes nll32, brier32 [temps, ...]: per truth row the pixels, trunc(nll * 2^16),
    trunc(brier * 2^24) (both products exact) and (label == truth); a void pixel adds 1 to [j][classes][0] alone"""
    nll32, brier32 = np.asarray(nll32, np.float32), np.asarray(brier32, np.float32)
    temps = nll32.shape[0]
    t = np.asarray(truth).astype(np.int64).ravel()
    lab = np.asarray(label).astype(np.int64).ravel()
    valid = (t >= 0) & (t < classes)
    row = np.where(valid, t, classes)
    out = np.zeros((temps, classes + 1, 4), np.uint64)
    for j in range(temps):
        qn = (nll32[j].ravel().astype(np.float64) * ONE_NLL).astype(np.uint64)[valid]
        qb = (brier32[j].ravel().astype(np.float64) * ONE_BRIER).astype(np.uint64)[valid]
        np.add.at(out[j, :, 0], row, np.uint64(1))
        np.add.at(out[j, :, 1], row[valid], qn)
        np.add.at(out[j, :, 2], row[valid], qb)
        np.add.at(out[j, :, 3], row[valid], (lab[valid] == t[valid]).astype(np.uint64))
    return out


def quantise(nll, brier):
    """the fp32 a kernel stores for float64 scores, for building a table without a kernel (tests of the host functions)"""
    return np.asarray(nll, np.float64).astype(np.float32), np.asarray(brier, np.float64).astype(np.float32)


def metrics(tab, classes, temps, j):
    """dict of the fields of mbn_nll and the two [classes] arrays of plane j. Every ratio is one float64 division of exact integers"""
    n = np.asarray(tab, np.uint64).reshape(temps, classes + 1, 4)[j].astype(np.float64)      # exact below 2^53
    rows = n[:classes]
    scored = float(rows[:, 0].sum())
    have = rows[:, 0] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        cn = np.where(have, rows[:, 1] / (rows[:, 0] * ONE_NLL), np.nan)
        cb = np.where(have, rows[:, 2] / (rows[:, 0] * ONE_BRIER), np.nan)
    mean = lambda a: float(sum(a[t] for t in np.nonzero(have)[0]) / int(have.sum())) if have.any() else 0.0     # ascending class order
    return dict(pixels=scored + float(n[classes, 0]), scored=scored, void_pixels=float(n[classes, 0]),
                nll=float(rows[:, 1].sum()) / (scored * ONE_NLL) if scored else 0.0,
                brier=float(rows[:, 2].sum()) / (scored * ONE_BRIER) if scored else 0.0,
                accuracy=float(rows[:, 3].sum()) / scored if scored else 0.0, mean_class_nll=mean(cn), mean_class_brier=mean(cb),
                classes_present=int(have.sum()), class_nll=cn, class_brier=cb)


def best(tab, classes, inv_temps):
    """(index, refined beta, at_edge) by mbn_nll_best's rule; None when nothing is scored"""
    betas = np.asarray(inv_temps, np.float32).astype(np.float64)
    temps = betas.size
    n = np.asarray(tab, np.uint64).reshape(temps, classes + 1, 4)
    if int(n[0, :classes, 0].sum()) == 0:
        return None
    sums = [int(n[j, :classes, 1].astype(object).sum()) for j in range(temps)]
    b = min(range(temps), key=lambda j: (sums[j], j))
    beta = float(betas[b])
    if 0 < b < temps - 1:
        x0, x1, x2 = (float(np.log(betas[i])) for i in (b - 1, b, b + 1))
        y0, y1, y2 = (float(sums[i]) for i in (b - 1, b, b + 1))
        s01, s12 = (y1 - y0) / (x1 - x0), (y2 - y1) / (x2 - x1)
        a = (s12 - s01) / (x2 - x0)
        if a > 0:
            beta = float(np.exp(min(max(0.5 * (x0 + x1) - s01 / (2 * a), x0), x2)))
    return b, beta, int(temps > 1 and b in (0, temps - 1))


# ---- the case generators of the GPU tests

def logits(n, h, w, classes, seed, sigma=3.0):
    return (sigma * np.random.default_rng(seed).standard_normal((n, h, w, classes))).astype(np.float32)


def truth_map(shape, classes, seed, dtype=np.uint8, void=0.1):
    """a random truth of `shape` with a share of void values: 255 (uint8), or -1 and `classes` (int32)"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, classes, shape).astype(dtype)
    bad = rng.random(shape) < void
    if dtype == np.uint8:
        assert classes <= 255
        t[bad] = 255
    else:
        t[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, classes).astype(dtype)
    return t


FIT_SHAPE, FIT_OUT, FIT_SEED = (2, 5, 7, 21), (60, 80), 7
FIT_GRID = [0.25, 0.35, 0.5, 0.7, 1.0, 1.4, 2.0, 4.0]
FIT_BEST = 2            # beta = 0.5: the kernel sees 2 z, the truth was drawn from softmax(z)


def fit_case():
    """(x = 2 z fp32, truth uint8 [n][H][W]): z = 1.5 N(0, 1), the truth of every output pixel sampled from softmax of the interpolated z"""
    rng = np.random.default_rng(FIT_SEED)
    z = (1.5 * rng.standard_normal(FIT_SHAPE)).astype(np.float32)
    v = dense_any_ref.resample(z, *FIT_OUT).astype(np.float64)
    p = np.exp(v - v.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    u = rng.random(p.shape[:-1])
    truth = np.minimum((p.cumsum(axis=-1) < u[..., None]).sum(axis=-1), FIT_SHAPE[3] - 1).astype(np.uint8)
    return (np.float32(2.0) * z).astype(np.float32), truth
