"""The normative arithmetic of "score a segmentation by surface distance" (include/mbn.h) in numpy, by brute force: the contour of every class
of a map (boundary_ref.depth == 1), per class the |P| x |G| matrix of squared distances between the contour pixels of the two maps in int64 and
its row minima, math.isqrt for both roots, the table surf [classes][2][HEAD + bins], the per-pixel dist2 map of direction 0, and the metrics of a
table in float64. Nothing here walks rings or windows, so it shares nothing with the device's route; everything but the final ratios is integer,
so the device must reproduce score() and dist2_map() cell for cell."""
import math

import numpy as np

import boundary_ref as BR

HEAD = 4
UNMATCHED = 0xFFFFFFFE
NOT_QUERY = 0xFFFFFFFF


def contour(m, edge):
    """bool [rows][cols]: the pixels whose depth is 1"""
    return BR.depth(m, 1, edge) == 1


def _coords(mask):
    return np.argwhere(mask).astype(np.int64)


def nearest_d2(p, g):
    """int64 [len (p)]: for every row of p the smallest squared distance to a row of g (len (g) > 0), brute force in slabs"""
    out = np.empty(len(p), np.int64)
    step = max(1, (1 << 22) // max(1, len(g)))
    for i in range(0, len(p), step):
        d = p[i:i + step, None, :] - g[None, :, :]
        out[i:i + step] = (d * d).sum(axis=2).min(axis=1)
    return out


def ceil_root(d2):
    """the smallest integer t with t * t >= d2"""
    t = math.isqrt(int(d2))
    return t + (t * t < int(d2))


def _queries(labels, truth, classes, edge):
    """per class present on either side and direction (0: labels -> truth, 1: truth -> labels): (c, k, coords of the queries, d2 or None)"""
    labels, truth = np.asarray(labels), np.asarray(truth)
    maps = (labels.astype(np.int64), truth.astype(np.int64))
    cont = (contour(labels, edge), contour(truth, edge))
    values = set()
    for m, cm in zip(maps, cont):
        values |= set(int(v) for v in np.unique(m[cm]) if 0 <= v < classes)
    for c in sorted(values):
        pts = [_coords(cont[k] & (maps[k] == c)) for k in range(2)]
        for k in range(2):
            if len(pts[k]):
                yield c, k, pts[k], (nearest_d2(pts[k], pts[1 - k]) if len(pts[1 - k]) else None)


def score(labels, truth, classes, bins, edge):
    """uint64 [classes][2][HEAD + bins] of one 2-D map pair; max_d2 is the pair's own maximum"""
    surf = np.zeros((classes, 2, HEAD + bins), np.uint64)
    for c, k, pts, d2 in _queries(labels, truth, classes, edge):
        row = surf[c, k]
        row[0] = len(pts)
        if d2 is None:
            row[1] = len(pts)
            continue
        row[2] = int(d2.max())
        row[3] = sum(math.isqrt(int(v) << 16) for v in d2)
        for v in d2:
            row[HEAD + min(ceil_root(v), bins - 1)] += np.uint64(1)
    return surf


def add(total, one):
    """total += one, cell for cell; max_d2 by maximum"""
    far = np.maximum(total[:, :, 2], one[:, :, 2])
    total += one
    total[:, :, 2] = far
    return total


def score_maps(pairs, classes, bins, edge):
    """the table of a batch or a ragged set: (labels, truth) 2-D pairs"""
    total = np.zeros((classes, 2, HEAD + bins), np.uint64)
    for labels, truth in pairs:
        add(total, score(labels, truth, classes, bins, edge))
    return total


def dist2_map(labels, truth, classes, edge):
    """uint32 [rows][cols] of direction 0: d2 of a matched query, UNMATCHED, or NOT_QUERY"""
    out = np.full(np.asarray(labels).shape, NOT_QUERY, np.uint32)
    for c, k, pts, d2 in _queries(labels, truth, classes, edge):
        if k == 0:
            out[pts[:, 0], pts[:, 1]] = UNMATCHED if d2 is None else d2.astype(np.uint32)
    return out


def surface_map(dist2):
    """the 16-bit image mobilenet --surface-map writes of a dist2 map: 0 no query, 65535 unmatched, else 1 + min (ceil (sqrt (d2)), 65533)"""
    out = np.zeros(dist2.shape, np.int32)
    for (r, c), v in np.ndenumerate(dist2):
        if v == UNMATCHED:
            out[r, c] = 65535
        elif v != NOT_QUERY:
            out[r, c] = 1 + min(ceil_root(v), 65533)
    return out


def metrics(surf, classes, bins, tolerance, percentile):
    """dict of the fields of mbn_surface_metrics_t and the per-class float64 arrays hd, hdp, assd, nsd (NaN where undefined). Means are summed in
    ascending class order; every ratio is formed from exact integers in the order include/mbn.h gives"""
    s = np.asarray(surf, dtype=np.uint64).reshape(classes, 2, HEAD + bins)
    hd, hdp, assd, nsd = (np.full(classes, np.nan) for _ in range(4))
    present = measurable = saturated = 0
    sums = [0.0, 0.0, 0.0, 0.0]
    for c in range(classes):
        n = [int(s[c, k, 0]) for k in range(2)]
        matched = [n[k] - int(s[c, k, 1]) for k in range(2)]
        cum = [np.cumsum(s[c, k, HEAD:].astype(object)) for k in range(2)]
        if n[0] + n[1] > 0:
            nsd[c] = float(int(cum[0][tolerance]) + int(cum[1][tolerance])) / float(n[0] + n[1])
            present += 1
            sums[3] += nsd[c]
        if matched[0] > 0 and matched[1] > 0:
            hd[c] = math.sqrt(float(max(int(s[c, 0, 2]), int(s[c, 1, 2]))))
            t = 0
            for k in range(2):
                need = math.ceil(percentile / 100.0 * float(matched[k]))
                tk = next((i for i in range(bins - 1) if int(cum[k][i]) >= need), bins - 1)
                t = max(t, tk)
            saturated += t == bins - 1
            hdp[c] = float(t)
            assd[c] = (float(int(s[c, 0, 3])) + float(int(s[c, 1, 3]))) / 256.0 / float(matched[0] + matched[1])
            measurable += 1
            sums[0] += hd[c]; sums[1] += hdp[c]; sums[2] += assd[c]
    return {"hd": sums[0] / measurable if measurable else 0.0, "hdp": sums[1] / measurable if measurable else 0.0,
            "assd": sums[2] / measurable if measurable else 0.0, "nsd": sums[3] / present if present else 0.0,
            "n": float(int(s[:, :, 0].astype(object).sum())), "unmatched": float(int(s[:, :, 1].astype(object).sum())),
            "classes_present": present, "classes_measurable": measurable, "saturated": int(saturated),
            "hd_c": hd, "hdp_c": hdp, "assd_c": assd, "nsd_c": nsd}
