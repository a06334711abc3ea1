"""The normative arithmetic of the calibration score (include/mbn.h, "calibration score") in numpy: the reliability table of int32 labels and fp32
probabilities against a uint8 or int32 truth, and the metrics of such a table in float64. Once a pixel's bin and fixed-point probability are formed
everything is integer, so the device must reproduce calibration_table() cell for cell."""
import numpy as np

ONE = 1 << 24       # the fixed point of column 2


def clamp_prob(prob):
    """p: 0 for a NaN or x < 0, 1 for x > 1, else x (fp32)"""
    x = np.asarray(prob, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x) | (x < 0), np.float32(0), np.where(x > 1, np.float32(1), x)).astype(np.float32)


def bin_of(prob, bins):
    """min(bins - 1, trunc(p (*) bins)): ONE fp32 multiplication"""
    p = clamp_prob(prob)
    return np.minimum(bins - 1, (p * np.float32(bins)).astype(np.int64))


def fixed_of(prob):
    """q = trunc(p * 2^24): the product is exact in fp32"""
    return (clamp_prob(prob) * np.float32(ONE)).astype(np.int64)


def calibration_table(labels, prob, truth, classes, bins):
    """uint64 [bins + 1][4]: answered, answered correctly, the sum of q, abstained per bin; [bins][0] the void pixels. What lies under a void pixel
    (label, prob) and the q of an abstained pixel do not enter."""
    lab = np.asarray(labels).astype(np.int64).ravel()
    t = np.asarray(truth).astype(np.int64).ravel()
    assert lab.size == t.size == np.asarray(prob).size
    valid = (t >= 0) & (t < classes)
    answered = valid & (lab >= 0) & (lab < classes)
    abstained = valid & ~answered
    b, q = bin_of(prob, bins), fixed_of(prob)
    table = np.zeros((bins + 1, 4), np.uint64)
    table[:bins, 0] = np.bincount(b[answered], minlength=bins)
    table[:bins, 1] = np.bincount(b[answered & (lab == t)], minlength=bins)
    for i in range(bins):                                   # integer sums: no float weights
        table[i, 2] = int(q[answered & (b == i)].sum())
    table[:bins, 3] = np.bincount(b[abstained], minlength=bins)
    table[bins, 0] = int((~valid).sum())
    return table


def calibration_table_ragged(labels, prob, truth, classes, bins, items):
    """the same over the maps (dst_offset, rows, cols) of a ragged set; labels, prob and truth share the element offsets"""
    table = np.zeros((bins + 1, 4), np.uint64)
    for off, rows, cols in items:
        s = slice(off, off + rows * cols)
        table += calibration_table(labels[s], prob[s], truth[s], classes, bins)
    return table


def metrics(calib, bins):
    """dict of the fields of mbn_calibration and the four [bins] arrays. Every ratio is one float64 division of exact integers; ece and aurc are
    summed in ascending order."""
    n = np.asarray(calib, np.uint64).reshape(bins + 1, 4).astype(np.float64)                # exact below 2^53
    nb, right, conf, abst = n[:bins, 0], n[:bins, 1], n[:bins, 2], n[:bins, 3]
    N, abstained = float(nb.sum()), float(abst.sum())
    accuracy, confidence = np.full(bins, np.nan), np.full(bins, np.nan)
    ece = mce = 0.0
    for b in range(bins):
        if nb[b] > 0:
            accuracy[b] = right[b] / nb[b]
            confidence[b] = conf[b] / (nb[b] * float(ONE))
            gap = abs(accuracy[b] - confidence[b])
            ece += (nb[b] / N) * gap
            mce = max(mce, gap)
    kept = np.cumsum(nb[::-1])[::-1]
    kept_right = np.cumsum(right[::-1])[::-1]
    coverage = kept / (N + abstained) if N + abstained > 0 else np.zeros(bins)
    selective = np.full(bins, np.nan)
    selective[kept > 0] = kept_right[kept > 0] / kept[kept > 0]
    aurc = 0.0
    for j in range(bins):
        if kept[j] > 0:
            aurc += (1.0 - selective[j]) * (coverage[j] - (coverage[j + 1] if j + 1 < bins else 0.0))
    return {
        "pixels": N + abstained + float(n[bins, 0]), "answered": N, "abstained": abstained, "void_pixels": float(n[bins, 0]),
        "accuracy": float(right.sum()) / N if N > 0 else 0.0, "mean_confidence": float(conf.sum()) / (N * float(ONE)) if N > 0 else 0.0,
        "ece": ece, "mce": mce, "aurc": aurc,
        "bin_accuracy": accuracy, "bin_confidence": confidence, "coverage": coverage, "selective_accuracy": selective,
    }


def threshold(calib, bins, target):
    """(min_prob fp32, coverage, selective accuracy) of the smallest edge whose kept pixels reach `target`; None when no edge does"""
    m = metrics(calib, bins)
    for j in range(bins):
        if m["selective_accuracy"][j] >= target:            # a NaN (empty) is never >=
            return np.float32(j) / np.float32(bins), m["coverage"][j], m["selective_accuracy"][j]
    return None


def case(count, classes, dtype, seed):
    """The generator of the GPU tests: prob = u^0.25, the label equals the truth with probability prob; 5 % of the labels are 255, 5 % of the
    truth void (void pixels carry a NaN prob and a random label); the first five probabilities are 0, 1, NaN, -0.5, 2.0."""
    rng = np.random.default_rng(seed)
    prob = (rng.random(count) ** 0.25).astype(np.float32)
    truth = rng.integers(0, classes, count)
    other = (truth + 1 + rng.integers(0, max(classes - 1, 1), count)) % classes
    labels = np.where(rng.random(count) < prob, truth, other).astype(np.int32)
    labels[rng.random(count) < 0.05] = 255
    head = np.array([0.0, 1.0, np.nan, -0.5, 2.0], np.float32)[:count]
    prob[:head.size] = head
    void = rng.random(count) < 0.05
    void[:head.size] = False
    truth = truth.astype(dtype)
    truth[void] = 255 if dtype == np.uint8 else rng.choice(np.array([255, -1, classes, 2 ** 31 - 1]), int(void.sum())).astype(dtype)
    prob[void] = np.nan
    labels[void] = rng.integers(-3, classes + 3, int(void.sum()))
    return labels, prob, truth
