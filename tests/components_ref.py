"""The numpy form of "regions of a label map" (include/mbn.h): connected components of an int32 label map per class, numbered by first pixel, with
the min_area drop. Two independent forms: `components` labels each class's mask with scipy.ndimage.label and orders the regions explicitly;
`components_flood` is a breadth-first flood fill in plain Python. Both return (comp int32 [rows][cols], regions int32 [n][8], labels_out int32
[rows][cols]); a region's record is (label, area, first_row, first_col, min_row, min_col, max_row, max_col)."""
from collections import deque

import numpy as np

FIELDS = ("label", "area", "first_row", "first_col", "min_row", "min_col", "max_row", "max_col")


def _finish(L, found, min_area, ignore_label):
    """found: (first linear index, label, linear indices of the region's pixels). Orders by first pixel, drops, numbers the survivors."""
    rows, cols = L.shape
    comp = np.full(rows * cols, -1, np.int32)
    out = L.astype(np.int32).ravel().copy()
    regions = []
    for first, label, idx in sorted(found, key=lambda f: f[0]):
        if len(idx) < min_area:
            out[idx] = ignore_label
            continue
        comp[idx] = len(regions)
        r, c = idx // cols, idx % cols
        regions.append((label, len(idx), first // cols, first % cols, r.min(), c.min(), r.max(), c.max()))
    return comp.reshape(rows, cols), np.array(regions, np.int32).reshape(len(regions), 8), out.reshape(rows, cols)


def components(L, classes, connectivity=4, min_area=1, ignore_label=0):
    from scipy import ndimage
    L = np.asarray(L, np.int32)
    assert L.ndim == 2 and classes >= 1 and connectivity in (4, 8) and min_area >= 1
    structure = np.ones((3, 3), int) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    found = []
    for label in np.unique(L):
        if not 0 <= label < classes:
            continue                                            # abstained: no region, connects and separates nothing
        lab, n = ndimage.label(L == label, structure=structure)
        flat = lab.ravel()
        order = np.argsort(flat, kind="stable")
        bounds = np.searchsorted(flat[order], np.arange(1, n + 2))
        for k in range(n):
            idx = order[bounds[k]:bounds[k + 1]]                # ascending linear indices (the sort is stable)
            found.append((int(idx[0]), int(label), idx))
    return _finish(L, found, min_area, ignore_label)


def components_flood(L, classes, connectivity=4, min_area=1, ignore_label=0):
    L = np.asarray(L, np.int32)
    rows, cols = L.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    grid = L.tolist()
    seen = [[False] * cols for _ in range(rows)]
    found = []
    for r0 in range(rows):
        for c0 in range(cols):
            label = grid[r0][c0]
            if seen[r0][c0] or not 0 <= label < classes:
                continue
            seen[r0][c0] = True
            queue, idx = deque([(r0, c0)]), []
            while queue:
                r, c = queue.popleft()
                idx.append(r * cols + c)
                for dr, dc in steps:
                    rr, cc = r + dr, c + dc
                    if 0 <= rr < rows and 0 <= cc < cols and not seen[rr][cc] and grid[rr][cc] == label:
                        seen[rr][cc] = True
                        queue.append((rr, cc))
            found.append((r0 * cols + c0, label, np.array(sorted(idx), np.int64)))
    return _finish(L, found, min_area, ignore_label)


# ---- the patterns both test files use. Each returns an int32 map [rows][cols] --------------------------------------------------------------

def constant(rows, cols, label=1):
    return np.full((rows, cols), label, np.int32)


def checkerboard(rows, cols):
    r, c = np.mgrid[0:rows, 0:cols]
    return ((r + c) & 1).astype(np.int32)


def stripes(rows, cols, vertical):
    r, c = np.mgrid[0:rows, 0:cols]
    return ((c if vertical else r) & 1).astype(np.int32)


def spiral(rows, cols):
    """a one-pixel-wide path of class 1 that winds inward from (0, 0), a wall of class 0 between its turns: the longest chain the map admits"""
    L = np.zeros((rows, cols), np.int32)
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(r, c):
        return 0 <= r < rows and 0 <= c < cols and L[r, c] == 0

    r, c, d = 0, 0, 0
    L[0, 0] = 1
    while True:
        for turn in range(2):                                   # straight on, else one turn to the right
            dr, dc = steps[(d + turn) % 4]
            ahead = (r + 2 * dr, c + 2 * dc)
            if free(r + dr, c + dc) and not (0 <= ahead[0] < rows and 0 <= ahead[1] < cols and L[ahead] == 1):
                d = (d + turn) % 4
                break
        else:
            return L
        r, c = r + dr, c + dc
        L[r, c] = 1


def rings(rows, cols):
    r, c = np.mgrid[0:rows, 0:cols]
    d = np.minimum(np.minimum(r, rows - 1 - r), np.minimum(c, cols - 1 - c))
    return (d % 3).astype(np.int32)


def comb(rows, cols, spine_last_row):
    """teeth of class 1 every other column (or row) that join only through a spine in the last row (or column)"""
    L = stripes(rows, cols, vertical=spine_last_row)
    if spine_last_row:
        L[-1, :] = 1
    else:
        L[:, -1] = 1
    return L


def corner_touch(rows, cols, tr, tc, anti):
    """two pixels of class 1 on class 0 that touch only diagonally across the tile corner at (tr, tc)"""
    L = np.zeros((rows, cols), np.int32)
    if anti:
        L[tr - 1, tc], L[tr, tc - 1] = 1, 1
    else:
        L[tr - 1, tc - 1], L[tr, tc] = 1, 1
    return L


def random_map(rows, cols, classes, seed, abstain=False):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, classes, (rows, cols)).astype(np.int32)
    if abstain:
        pick = rng.random((rows, cols)) < 0.1
        vals = np.array([-1, classes, 255, np.iinfo(np.int32).max, np.iinfo(np.int32).min], np.int64)
        L[pick] = rng.choice(vals, int(pick.sum())).astype(np.int32)
    return L


def blocks(rows, cols, classes, seed, side=25):
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, classes, ((rows + side - 1) // side, (cols + side - 1) // side)).astype(np.int32)
    return np.repeat(np.repeat(coarse, side, 0), side, 1)[:rows, :cols].copy()


def patterns(rows, cols, tr, tc, seed=0):
    """(name, classes, map) of every pattern at one size; tr, tc = a tile corner inside the map where there is one"""
    yield "constant", 3, constant(rows, cols)
    yield "checkerboard", 2, checkerboard(rows, cols)
    yield "row stripes", 2, stripes(rows, cols, False)
    yield "column stripes", 2, stripes(rows, cols, True)
    yield "spiral", 2, spiral(rows, cols)
    yield "rings", 3, rings(rows, cols)
    yield "comb, spine in the last row", 2, comb(rows, cols, True)
    yield "comb, spine in the last column", 2, comb(rows, cols, False)
    if 0 < tr < rows and 0 < tc < cols:
        yield "corner, diagonal", 2, corner_touch(rows, cols, tr, tc, False)
        yield "corner, anti-diagonal", 2, corner_touch(rows, cols, tr, tc, True)
    for classes in (2, 3, 21):
        yield "random %d" % classes, classes, random_map(rows, cols, classes, seed + classes)
        yield "random %d, abstained" % classes, classes, random_map(rows, cols, classes, seed + 100 + classes, abstain=True)
    yield "blocks", 21, blocks(rows, cols, 21, seed + 7)
