"""The sliding-window read-out in numpy float32: the normative arithmetic of mbn_resample_slide_f32 (include/mbn.h, "Segment by sliding window"),
bit for bit, on top of dense_any_ref. A plan is (tile_rows, tile_cols, ys, xs): tile (iy, ix) covers output rows [ys[iy], ys[iy] + tile_rows) and
columns [xs[ix], xs[ix] + tile_cols). Per tile the interpolants are dense_any_ref.resample's of that tile's own map to tile_rows x tile_cols (each
tile an image of its own); over a pixel they are summed in tile order (ascending iy, then ix), one float32 addition each, the sum is multiplied
by float32(1) / float32(count) once, and the argmax and the float64 softmax (dense_prob_ref.from_interpolants) see that mean."""
import numpy as np

import dense_any_ref
import dense_prob_ref

MAX_AXIS = 16


def axis(size, tile, stride):
    """mbn_slide_axis written out: the positions of the tiles along an axis, regular steps and the last one flush with the far edge"""
    n = (-(-(size - tile) // stride) if size > tile else 0) + 1
    return [min(i * stride, size - tile) for i in range(n)]


def plan(H, W, tile_rows, tile_cols, stride_rows, stride_cols):
    return tile_rows, tile_cols, axis(H, tile_rows, stride_rows), axis(W, tile_cols, stride_cols)


def plan_tuple(p):
    """(tile_rows, tile_cols, ys, xs) of a tuple or of the package's Slide"""
    if hasattr(p, "ny"):
        return int(p.tile_rows), int(p.tile_cols), [int(v) for v in p.y[:p.ny]], [int(v) for v in p.x[:p.nx]]
    th, tw, ys, xs = p
    return int(th), int(tw), [int(v) for v in ys], [int(v) for v in xs]


def count_map(p, H, W):
    """int32 [H][W]: the tiles over each pixel"""
    th, tw, ys, xs = plan_tuple(p)
    cy, cx = np.zeros(H, np.int32), np.zeros(W, np.int32)
    for y in ys:
        cy[y:y + th] += 1
    for x in xs:
        cx[x:x + tw] += 1
    return cy[:, None] * cx[None, :]


def mean(x, p, H, W):
    """x: float32 [n][ny * nx][h][w][classes], image-major, tile t = iy * nx + ix -> t float32 [n][H][W][classes]"""
    x = np.ascontiguousarray(x, np.float32)
    th, tw, ys, xs = plan_tuple(p)
    n, T, h, w, c = x.shape
    assert T == len(ys) * len(xs)
    count = count_map(p, H, W)
    assert count.min() >= 1, "a pixel no tile covers"
    s = np.zeros((n, H, W, c), np.float32)
    seen = np.zeros((H, W), bool)
    with np.errstate(invalid="ignore", over="ignore"):          # inf - inf is a NaN by the definition too
        for iy, y in enumerate(ys):
            for ix, x0 in enumerate(xs):
                v = dense_any_ref.resample(x[:, iy * len(xs) + ix], th, tw)
                first = ~seen[y:y + th, x0:x0 + tw]
                part = s[:, y:y + th, x0:x0 + tw]
                s[:, y:y + th, x0:x0 + tw] = np.where(first[None, :, :, None], v, part + v)
                seen[y:y + th, x0:x0 + tw] = True
        return s * (np.float32(1.0) / count.astype(np.float32))[None, :, :, None]


def slide(x, p, H, W):
    """(labels int32, score float32, prob float64) [n][H][W]"""
    return dense_prob_ref.from_interpolants(mean(x, p, H, W))


# The geometry cases of the GPU test (map h x w, tile, stride, source); test_dense_slide_cpu.py checks what the last column says of each
GEOMETRY = {"A": ((2, 3), (40, 61), (20, 31), (85, 131)),       # positions [0, 20, 40, 45] x [0, 31, 62, 70]
            "B": ((2, 3), (8, 12), (4, 6), (17, 25)),           # the minimum ratio: largest footprints, smallest chunk
            "C": ((5, 7), (100, 150), (60, 90), (230, 333))}    # cells wider than 32: several output tiles a cell, ragged cell edges
COUNTS = {1, 2, 3, 4, 6, 9}

# The inputs and thresholds of the GPU threshold test: (n, geometry, classes, seed, sigma, min_prob). test_dense_slide_cpu.py checks that
# `excluded` leaves out at most 1 % of their pixels and that each threshold cuts through its map.
THRESHOLD_CASES = [(2, "A", 21, 301, 3.0, 0.25), (2, "A", 21, 301, 3.0, 0.4), (1, "B", 64, 302, 2.0, 0.1)]


def geometry_plan(name):
    (h, w), (th, tw), (sh, sw), (H, W) = GEOMETRY[name]
    return h, w, plan(H, W, th, tw, sh, sw), H, W


def threshold_input(case):
    n, name, classes, seed, sigma, _ = case
    h, w, p, H, W = geometry_plan(name)
    return (sigma * np.random.default_rng(seed).standard_normal((n, len(p[2]) * len(p[3]), h, w, classes))).astype(np.float32)


def order_input(h=2, w=3, classes=4):
    """three tiles over every pixel of a column band: 1e8, -1e8 and 1 in tile order give (1e8 - 1e8) + 1 = 1, any other order 0"""
    x = np.zeros((1, 3, h, w, classes), np.float32)
    x[0, 0, ..., 1], x[0, 1, ..., 1], x[0, 2, ..., 1] = 1e8, -1e8, 1.0
    return x
