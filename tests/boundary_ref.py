"""The normative arithmetic of "score a segmentation at its boundaries" (include/mbn.h) in numpy, by brute force: the depth of every pixel (its
Chebyshev distance to the nearest pixel of another value, the frame counting as one under edge = 1, capped at d + 1), the trimap and boundary-IoU
tables of a prediction against a truth, and the metrics of a biou table in float64. Everything but the final ratios is integer, so the device must
reproduce depth(), score() cell for cell."""
import numpy as np


def half_width(rows, cols, ratio):
    """mbn_boundary_d: int (round (ratio * diagonal)) of the official boundary IoU (Python's round: ties to even), at least 1"""
    return max(1, int(round(ratio * np.sqrt(float(rows) * rows + float(cols) * cols))))


def depth(m, d, edge):
    """uint8 [rows][cols]: min (D, d + 1). m is one 2-D map; values are compared as stored. The rings k = 1 .. d are tried in turn: a pixel whose
    depth is still open and that sees another value (or, under edge, the outside) at Chebyshev distance exactly k takes k. The loop ends early
    when no pixel is open any more, or when a ring lies wholly outside the map and the outside counts for nothing."""
    m = np.asarray(m)
    rows, cols = m.shape
    out = np.full((rows, cols), d + 1, np.int64)
    for k in range(1, d + 1):
        if not (out == d + 1).any() or (not edge and k >= max(rows, cols)):
            break
        hit = np.zeros((rows, cols), bool)
        for dr in range(-k, k + 1):
            for dc in (range(-k, k + 1) if abs(dr) == k else (-k, k)):           # the ring max (|dr|, |dc|) == k
                r0, r1 = max(0, -dr), min(rows, rows - dr)       # the pixels (r, c) whose neighbour (r + dr, c + dc) is inside
                c0, c1 = max(0, -dc), min(cols, cols - dc)
                outside = np.ones((rows, cols), bool)
                if r0 < r1 and c0 < c1:
                    outside[r0:r1, c0:c1] = False
                    hit[r0:r1, c0:c1] |= m[r0:r1, c0:c1] != m[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
                if edge:
                    hit |= outside
        out[(out == d + 1) & hit] = k
    return out.astype(np.uint8)


def clamp(v, classes):
    v = np.asarray(v).astype(np.int64)
    return np.where((v >= 0) & (v < classes), v, classes)


def score(labels, truth, classes, d, edge):
    """(trimap uint64 [classes + 1][classes + 1], biou uint64 [classes][3]) of one 2-D map pair"""
    labels, truth = np.asarray(labels), np.asarray(truth)
    tb = depth(truth, d, edge) <= d
    pb = depth(labels, d, edge) <= d
    t, p = clamp(truth, classes), clamp(labels, classes)
    s = classes + 1
    trimap = np.bincount((t * s + p)[tb], minlength=s * s).astype(np.uint64).reshape(s, s)
    tv = t < classes
    biou = np.zeros((classes, 3), np.uint64)
    biou[:, 0] = np.bincount(t[tb & tv], minlength=classes)[:classes]
    biou[:, 1] = np.bincount(p[pb & tv & (p < classes)], minlength=classes)[:classes]
    biou[:, 2] = np.bincount(t[tb & pb & tv & (t == p)], minlength=classes)[:classes]
    return trimap, biou


def score_maps(pairs, classes, d, edge):
    """the sums over (labels, truth) or (labels, truth, d) 2-D pairs: a batch or a ragged set"""
    trimap = np.zeros((classes + 1, classes + 1), np.uint64)
    biou = np.zeros((classes, 3), np.uint64)
    for pair in pairs:
        a, b = score(pair[0], pair[1], classes, pair[2] if len(pair) > 2 else d, edge)
        trimap += a
        biou += b
    return trimap, biou


def metrics(biou, classes):
    """dict of the fields of mbn_boundary_metrics_t and `iou` (float64 [classes], NaN for an absent class); the mean is summed in ascending class
    order, every ratio is one float64 division of exact integers"""
    n = np.asarray(biou, dtype=np.uint64).reshape(classes, 3).astype(np.float64)
    den = n[:, 0] + n[:, 1] - n[:, 2]
    present = den > 0
    iou = np.full(classes, np.nan)
    iou[present] = n[present, 2] / den[present]
    total = 0.0
    for c in range(classes):
        if present[c]:
            total += iou[c]
    return {"boundary_miou": total / int(present.sum()) if present.any() else 0.0, "truth_band_pixels": float(n[:, 0].sum()),
            "pred_band_pixels": float(n[:, 1].sum()), "classes_present": int(present.sum()), "iou": iou}
