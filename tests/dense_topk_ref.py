"""Segment with runners-up: the normative arithmetic of mbn_resample_topk_f32 / _ragged_f32 and of the rank score mbn_topk_rank_i32 /
mbn_topk_metrics (include/mbn.h, "Segment with runners-up", "Rank score") in numpy, on top of dense_any_ref / dense_window_ref. The interpolated
logits v are theirs, in float32, bit for bit. The selection is the header's state machine, vectorised over the pixels: k slots (val, lab), every
val = -inf; the classes in ascending order; class c enters iff v_c > val[k - 1] (strict) and goes to the smallest j with v_c > val[j], the slots
from there moving down one. prob is the FLOAT64 evaluation of e(val_j) / sum_c e(v_c), e(v) = exp(v - best) and 0 for a NaN; 0 where best is
not finite or the slot is unfilled. The kernel's fp32 prob is held to tolerance(...)."""
import numpy as np

import dense_any_ref
import dense_window_ref

TOPK_MAX = 8


def select(v, k):
    """v: float32 [..., classes] -> (val float32 [k, ...], lab int32 [k, ...]) by the header's insertion rule, class by class"""
    v = np.asarray(v, np.float32)
    shape = v.shape[:-1]
    val = np.full((k,) + shape, -np.inf, np.float32)
    lab = np.full((k,) + shape, -1, np.int32)               # an unfilled slot: -1 wherever it ends up ...
    with np.errstate(invalid="ignore"):
        for c in range(v.shape[-1]):
            x = v[..., c]
            gt = x[None] > val                              # [k, ...]: a NaN is greater than nothing; the slots are sorted, so gt is a suffix
            if not gt[k - 1].any():
                continue
            for j in range(k - 1, 0, -1):                   # from the bottom up, every slot from the OLD content of the one above
                val[j] = np.where(gt[j - 1], val[j - 1], np.where(gt[j], x, val[j]))
                lab[j] = np.where(gt[j - 1], lab[j - 1], np.where(gt[j], np.int32(c), lab[j]))
            val[0] = np.where(gt[0], x, val[0])
            lab[0] = np.where(gt[0], np.int32(c), lab[0])
    lab[0] = np.where(val[0] > -np.inf, lab[0], np.int32(0))    # ... but 0 at rank 0: the argmax rule, label 0 when nothing wins
    return val, lab


def from_interpolants(v, k):
    """v: float32 [..., classes] -> (labels int32, score float32, prob float64), each [k, ...]"""
    v = np.asarray(v, np.float32)
    val, lab = select(v, k)
    best = val[0]
    finite = np.isfinite(best)
    nan = np.isnan(v)
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.where(finite, best, np.float32(0)).astype(np.float64)
        s = np.where(nan, 0.0, np.exp(v.astype(np.float64) - ref[..., None])).sum(axis=-1)
        filled = val > -np.inf
        num = np.where(filled, np.exp(np.where(filled, val, np.float32(0)).astype(np.float64) - ref[None]), 0.0)
        prob = np.where(finite[None] & filled, num / np.where(finite, s, 1.0)[None], 0.0)
    return lab, val, prob


def resample_topk(x, H, W, k, window=None):
    """(labels, score, prob) [k][n][H][W] of x float32 [n][h][w][classes]; window = (in_rows, in_cols, rect) or None for the whole map"""
    v = dense_any_ref.resample(x, H, W) if window is None else dense_window_ref.resample_window(x, window[0], window[1], window[2], H, W)
    return from_interpolants(v, k)


def tolerance(classes, score, prob):
    """what |kernel prob - prob| may be, per element of prob [k, ...] (include/mbn.h derives it):
    (classes + 200 + 2 |val_j - best|) 2^-24 relative and 2^-125 absolute; 0 where prob is 0 by the rule (best not finite, slot unfilled)"""
    score = np.asarray(score, np.float32)
    best = score[0]
    ok = np.isfinite(best)[None] & (score > -np.inf)
    with np.errstate(invalid="ignore"):
        gap = np.where(ok, np.abs(score.astype(np.float64) - best.astype(np.float64)[None]), 0.0)
    return np.where(ok, (classes + 200 + 2.0 * gap) * 2.0 ** -24 * np.asarray(prob, np.float64) + 2.0 ** -125, 0.0)


# ---- rank score

def rank_table(planes, truth, classes):
    """planes int32 [k][count], truth [count] (uint8 or int32) -> uint64 [classes + 1][k + 1]: row = truth (outside [0, classes): the void row
    `classes`), column = the smallest j with planes[j] == truth, else k; every void pixel goes to column k"""
    planes = np.asarray(planes, np.int32)
    k = planes.shape[0]
    t = np.asarray(truth).astype(np.int64).ravel()
    valid = (t >= 0) & (t < classes)
    row = np.where(valid, t, classes)
    hit = (planes.reshape(k, -1).astype(np.int64) == t[None]) & valid[None]
    col = np.where(hit.any(axis=0), hit.argmax(axis=0), k)
    out = np.zeros((classes + 1, k + 1), np.uint64)
    np.add.at(out, (row, col), np.uint64(1))
    return out


def metrics(ranks, classes, k):
    """(accuracy [k], mean_accuracy [k], valid) of a rank table, in float64: mbn_topk_metrics"""
    n = np.asarray(ranks, np.uint64).reshape(classes + 1, k + 1)[:classes].astype(np.float64)
    rows = n.sum(axis=1)
    valid = float(rows.sum())
    cum = np.cumsum(n[:, :k], axis=1)
    acc = cum.sum(axis=0) / valid if valid > 0 else np.zeros(k)
    have = rows > 0
    mean = np.zeros(k)
    if have.any():
        for j in range(k):
            s = 0.0
            for t in np.nonzero(have)[0]:                   # ascending class order, as the C function sums
                s += cum[t, j] / rows[t]
            mean[j] = s / int(have.sum())
    return acc, mean, valid
