"""The normative arithmetic of "score a segmentation" (include/mbn.h) in numpy: the confusion matrix of int32 labels against a uint8 or int32
truth, and the metrics of such a matrix in float64. Integer counting is exact, so the device must reproduce confusion() cell for cell."""
import numpy as np


def clamp(v, classes):
    """row of a truth value / column of a label: itself inside [0, classes), else `classes` (void / abstained), negative values included"""
    v = np.asarray(v).astype(np.int64).ravel()
    return np.where((v >= 0) & (v < classes), v, classes)


def confusion(labels, truth, classes):
    """uint64 [classes + 1][classes + 1]: row = truth, column = label; every pixel adds 1 to one cell"""
    labels, truth = np.asarray(labels), np.asarray(truth)
    assert labels.size == truth.size
    s = classes + 1
    return np.bincount(clamp(truth, classes) * s + clamp(labels, classes), minlength=s * s).astype(np.uint64).reshape(s, s)


def confusion_ragged(labels, truth, classes, items):
    """the same over the maps (dst_offset, rows, cols) of a ragged set; labels and truth share the element offsets"""
    n = np.zeros((classes + 1, classes + 1), np.uint64)
    for off, rows, cols in items:
        n += confusion(labels[off:off + rows * cols], truth[off:off + rows * cols], classes)
    return n


def metrics(counts, classes):
    """dict of the fields of mbn_seg_metrics and `iou` (float64 [classes], NaN for an absent class). Every ratio is one float64 division of exact
    integers; the means are summed in ascending class order."""
    n = np.asarray(counts, dtype=np.uint64).reshape(classes + 1, classes + 1).astype(np.float64)     # exact below 2^53
    rows = n[:classes].sum(axis=1)
    valid = float(rows.sum())
    void_pixels = float(n[classes].sum())
    tp = np.diag(n)[:classes]
    fn = rows - tp
    fp = n[:classes, :classes].sum(axis=0) - tp
    den = tp + fp + fn
    present = den > 0
    iou = np.full(classes, np.nan)
    iou[present] = tp[present] / den[present]
    have = rows > 0
    iou_sum = acc_sum = fw = 0.0
    for c in range(classes):
        if present[c]:
            iou_sum += iou[c]
            fw += (rows[c] / valid) * iou[c]
        if have[c]:
            acc_sum += tp[c] / rows[c]
    return {
        "pixels": valid + void_pixels, "valid": valid, "void_pixels": void_pixels, "abstained": float(n[:classes, classes].sum()),
        "pixel_accuracy": float(tp.sum()) / valid if valid > 0 else 0.0,
        "mean_accuracy": acc_sum / int(have.sum()) if have.any() else 0.0,
        "miou": iou_sum / int(present.sum()) if present.any() else 0.0,
        "fw_iou": fw, "classes_present": int(present.sum()), "iou": iou,
    }
