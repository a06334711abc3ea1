"""The numpy form of "score a segmentation by its regions" (include/mbn.h): panoptic quality of a predicted against a true segment map. Written as
the PAIR HISTOGRAM (np.unique of the (predicted, truth) pairs), so it shares nothing with the device's bit-majority route; `panoptic_brute` is a
plain double loop over the segments for tiny maps, and `panoptic_vote` is that device route in numpy (used by the CPU tests only, to check the
route itself against the histogram).

A segmentation of one image is (comp int32 [rows][cols], records int32 [n][8]): comp holds a segment number or -1, a record is an mbn_region
(label, area, first_row, first_col, min_row, min_col, max_row, max_col) of which only label and area matter here. `segments` builds both from an
arbitrary map of ids and a class per id, vectorised; `stuff` builds whole-class segments from a label map.

The result of every form is a Result: pq uint64 [classes][4] = tp, fp, fn, S with S = sum over the matches of floor (inter * 2^32 / union);
match_pred [n_pred] (the matched g, -1 false positive, -2 excused), match_truth [n_truth] (the matched p or -1), inter [n_pred] (of the match, else
0), void [n_pred]; iou float64 [classes], the float sum of inter / union over the matches of the class; exact [classes], the same sum as a
fractions.Fraction, without any rounding."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

Result = namedtuple("Result", "pq match_pred match_truth inter void iou exact")


def records(labels, areas, firsts=None, cols=1):
    """int32 [n][8] from a label and an area per segment; first pixel (a linear index) and box where known, else 0"""
    n = len(labels)
    rec = np.zeros((n, 8), np.int32)
    rec[:, 0], rec[:, 1] = labels, areas
    if firsts is not None:
        rec[:, 2], rec[:, 3] = np.asarray(firsts) // cols, np.asarray(firsts) % cols
    return rec


def segments(ids, label_of):
    """(comp, records) of a map of arbitrary ids (< 0: no segment): the segments are numbered 0 .. n - 1 in ascending order of their first pixel;
    label_of: id -> class, a callable on an array of ids or an array indexed by id. Vectorised."""
    ids = np.asarray(ids)
    flat = ids.ravel()
    inside = np.flatnonzero(flat >= 0)
    comp = np.full(flat.size, -1, np.int32)
    if inside.size == 0:
        return comp.reshape(ids.shape), np.zeros((0, 8), np.int32)
    uniq, first, inverse, counts = np.unique(flat[inside], return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")                    # by first pixel
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    comp[inside] = rank[inverse]
    labels = label_of(uniq[order]) if callable(label_of) else np.asarray(label_of)[uniq[order]]
    return comp.reshape(ids.shape), records(labels, counts[order], inside[first[order]], ids.shape[-1])


def stuff(L, classes):
    """whole-class segments of a label map: one segment per class present, values outside [0, classes) belong to none"""
    L = np.asarray(L, np.int64)
    return segments(np.where((L >= 0) & (L < classes), L, -1), lambda ids: ids)


def _clean(comp_pred, pred, comp_truth, truth):
    cp, ct = np.asarray(comp_pred, np.int64).ravel(), np.asarray(comp_truth, np.int64).ravel()
    pred, truth = np.asarray(pred, np.int64).reshape(-1, 8), np.asarray(truth, np.int64).reshape(-1, 8)
    cp = np.where((cp >= 0) & (cp < len(pred)), cp, -1)         # anything else: no predicted segment
    return cp, pred, ct, truth


def _classify(pairs, void, pred, truth, classes):
    """pairs: iterable of (p, g, inter) with g a listed truth segment and inter > 0. The match rule and the four outcomes, in Python integers"""
    n_pred, n_truth = len(pred), len(truth)
    pq = np.zeros((classes, 4), np.uint64)
    iou = np.zeros(classes, np.float64)
    exact = [Fraction(0)] * classes
    match_pred, match_truth = np.full(n_pred, -1, np.int32), np.full(n_truth, -1, np.int32)
    inter_out = np.zeros(n_pred, np.int32)
    for p, g, inter in pairs:
        p, g, inter = int(p), int(g), int(inter)
        union = int(pred[p, 1]) - int(void[p]) + int(truth[g, 1]) - inter
        if pred[p, 0] == truth[g, 0] and 2 * inter > union:
            assert match_pred[p] == -1 and match_truth[g] == -1, "at most one match on either side"
            match_pred[p], match_truth[g], inter_out[p] = g, p, inter
            c = int(pred[p, 0])
            if 0 <= c < classes:
                pq[c, 0] += np.uint64(1)
                pq[c, 3] += np.uint64((inter << 32) // union)
                iou[c] += inter / union
                exact[c] += Fraction(inter, union)
    for p in range(n_pred):
        if match_pred[p] >= 0:
            continue
        if 2 * int(void[p]) > int(pred[p, 1]):
            match_pred[p] = -2                                  # excused: counts nowhere
        elif 0 <= pred[p, 0] < classes:
            pq[int(pred[p, 0]), 1] += np.uint64(1)
    for g in range(n_truth):
        if match_truth[g] < 0 and 0 <= truth[g, 0] < classes:
            pq[int(truth[g, 0]), 2] += np.uint64(1)
    return Result(pq, match_pred, match_truth, inter_out, np.asarray(void, np.int32), iou, exact)


def panoptic(comp_pred, pred, comp_truth, truth, classes):
    """the pair histogram: one np.unique over the pixels of the predicted segments"""
    cp, pred, ct, truth = _clean(comp_pred, pred, comp_truth, truth)
    n_pred, n_truth = len(pred), len(truth)
    inside = cp >= 0
    # column 0: void truth; 1 .. n_truth: a listed truth segment; n_truth + 1: a truth number the table does not list
    col = np.where(ct < 0, 0, np.minimum(ct, n_truth) + 1)
    keys, counts = np.unique(cp[inside] * (n_truth + 2) + col[inside], return_counts=True)
    kp, kc = keys // (n_truth + 2), keys % (n_truth + 2)
    void = np.zeros(n_pred, np.int64)
    void[kp[kc == 0]] = counts[kc == 0]
    listed = (kc >= 1) & (kc <= n_truth)
    return _classify(zip(kp[listed], kc[listed] - 1, counts[listed]), void, pred, truth, classes)


def panoptic_brute(comp_pred, pred, comp_truth, truth, classes):
    """a double loop over the segments: for maps of a few pixels"""
    cp, pred, ct, truth = _clean(comp_pred, pred, comp_truth, truth)
    void = [int(((cp == p) & (ct < 0)).sum()) for p in range(len(pred))]
    pairs = []
    for p in range(len(pred)):
        for g in range(len(truth)):
            inter = int(((cp == p) & (ct == g)).sum())
            if inter:
                pairs.append((p, g, inter))
    return _classify(pairs, void, pred, truth, classes)


def panoptic_vote(comp_pred, pred, comp_truth, truth, classes):
    """the device's route: per predicted segment the majority of each bit of the truth numbers of its non-void pixels forms a candidate, a second
    pass counts the candidate's intersection exactly"""
    cp, pred, ct, truth = _clean(comp_pred, pred, comp_truth, truth)
    n_pred, n_truth = len(pred), len(truth)
    inside = cp >= 0
    live = inside & (ct >= 0)
    total = np.bincount(cp[live], minlength=n_pred)
    void = np.bincount(cp[inside & (ct < 0)], minlength=n_pred)
    cand = np.zeros(n_pred, np.int64)
    for b in range(max(n_truth - 1, 0).bit_length()):
        ones = np.bincount(cp[live & ((ct >> b) & 1 == 1)], minlength=n_pred)
        cand |= (2 * ones > total).astype(np.int64) << b
    hit = inside.copy()
    hit[inside] = ct[inside] == cand[cp[inside]]
    inter = np.bincount(cp[hit], minlength=n_pred)
    pairs = [(p, cand[p], inter[p]) for p in range(n_pred) if cand[p] < n_truth and inter[p] > 0]
    return _classify(pairs, void, pred, truth, classes)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))


def metrics(pq):
    """the formulas of mbn_panoptic_metrics in Python floats: (pq, sq, rq, tp, fp, fn, classes_present), pq_c, sq_c, rq_c"""
    import math
    pq_c, sq_c, rq_c = [], [], []
    for tp, fp, fn, S in np.asarray(pq, np.uint64).reshape(-1, 4).tolist():
        iou = math.ldexp(float(S), -32)
        if tp + fp + fn > 0:
            den = float(2 * tp + fp + fn)
            pq_c.append(2.0 * iou / den)
            rq_c.append(2.0 * float(tp) / den)
            sq_c.append(iou / float(tp) if tp else 0.0)
        else:
            pq_c.append(math.nan); rq_c.append(math.nan); sq_c.append(math.nan)
    present = [c for c in range(len(pq_c)) if not math.isnan(pq_c[c])]
    mean = lambda v: _sum([v[c] for c in present]) / float(len(present)) if present else 0.0
    tot = np.asarray(pq, np.uint64).reshape(-1, 4)[:, :3].astype(np.float64)
    return ((mean(pq_c), mean(sq_c), mean(rq_c), _sum(tot[:, 0]), _sum(tot[:, 1]), _sum(tot[:, 2]), len(present)),
            np.array(pq_c), np.array(sq_c), np.array(rq_c))


def _sum(values):
    s = 0.0
    for v in values:                                            # in ascending class order, one addition at a time, as the C code adds
        s += float(v)
    return s


# ------------------------------------------------------------------------------------------------------------------------------ maps

def block_ids(rows, cols, side, shift=0):
    """an id per side x side block, the blocks shifted right by `shift` columns"""
    r, c = np.mgrid[0:rows, 0:cols]
    return (r // side) * (cols // side + 3) + (c + side - shift % side) // side


def block_scene(rows, cols, classes, seed, side=8, shift=0, noise=0.0, drop=0.0, drop_blocks=0.0, class_seed=0):
    """(comp, records) of a map of blocks: each block one segment of a random class (the class depends on the block's id and class_seed only, so a
    shifted scene keeps its classes); `noise`: that share of the pixels become single-pixel segments of random classes; `drop`: that share of the
    pixels belong to no segment (void in a truth, abstained in a prediction); `drop_blocks`: that share of the blocks, whole, do not either"""
    rng = np.random.default_rng(seed)
    ids = block_ids(rows, cols, side, shift).astype(np.int64)
    n_blocks = int(ids.max()) + 1
    label_of = np.random.default_rng(class_seed).integers(0, classes, n_blocks + rows * cols)
    if noise:
        m = rng.random(ids.shape) < noise
        ids[m] = n_blocks + np.flatnonzero(m.ravel())
    if drop:
        ids[rng.random(ids.shape) < drop] = -1
    if drop_blocks:
        gone = rng.random(n_blocks) < drop_blocks
        ids[(ids >= 0) & (ids < n_blocks) & gone[np.minimum(ids, n_blocks - 1)]] = -1
    return segments(ids, label_of)
