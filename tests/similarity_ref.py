"""The nearest-neighbour search of include/mbn.h ("Nearest neighbours") in float64 numpy: scores, the total-order ranking and the header's two
bounds. CASES: the exact cases of tests/test_similarity_gpu.py, a pruned product of the issue's D, Q, G and k values."""
import numpy as np

U = 2.0 ** -24


def scores(q, g, q_scale=None, g_scale=None):
    """float64 scores [Q][G] of fp32 inputs; the scales are the fp32 values the device multiplies by."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = q.astype(np.float64) @ g.astype(np.float64).T
        if q_scale is not None:
            s = s * q_scale.astype(np.float64)[:, None]
        if g_scale is not None:
            s = s * g_scale.astype(np.float64)[None, :]
    return s


def rank(s, k):
    """(idx [Q][k] int32, score [Q][k]) under the total order: score descending, index ascending, a NaN never ranked, -inf last in index
    order; -1 / 0 in the slots past the ranked entries."""
    idx, sc = np.full((s.shape[0], k), -1, np.int32), np.zeros((s.shape[0], k), s.dtype)
    for q, row in enumerate(s):
        keep = np.flatnonzero(~np.isnan(row))
        best = keep[np.lexsort((keep, -row[keep]))][:k]
        idx[q, :best.size], sc[q, :best.size] = best, row[best]
    return idx, sc


def score_bound(q, g, q_scale=None, g_scale=None):
    """|score - score64| <= (D + 4) 2^-24 |q_scale g_scale| sum_d |q_d g_d|, per pair [Q][G]."""
    return (q.shape[1] + 4) * U * np.abs(scores(np.abs(q), np.abs(g), q_scale, g_scale))


def inv_norm_bound(D): return (D + 4) * U          # relative: |out - out64| <= (D + 4) 2^-24 out64


def inv_norm(x):
    n = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    return np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), 0.0)


# name: (D, Q, (a, b) with G = a * g_tile + b, k). D: one partial k-step, a k-tile plus a remainder, whole tiles; Q around one and two query tiles
# of both tile sizes (32 up to 32 queries, 64 beyond); G: single rows up to three chunks and a ragged panel
CASES = {
    "one pair": (4, 1, (0, 1), 1),
    "partial step": (4, 31, (0, 7), 5),
    "short, chunks": (4, 129, (3, 5), 8),
    "tile + rest": (36, 33, (0, 33), 8),
    "tile + rest, chunks": (36, 65, (3, 5), 1),
    "whole tiles": (128, 63, (1, -1), 5),
    "whole tiles, chunks": (128, 1, (3, 5), 8),
    "long rows": (1024, 31, (3, 5), 8),
    "long rows, two blocks": (1024, 33, (1, -1), 5),
    "long rows, tiles": (1024, 129, (0, 33), 1),
    "long rows, few": (1024, 65, (0, 7), 8),
}


def exact_case(name, g_tile):
    """Integer-valued inputs in [-8, 8] (every sum exact in fp32 at D <= 1024) with engineered ties: gallery rows 1, 4, 32, g_tile and 2 g_tile + 3
    repeat row 0 (the same lane, the other lane half, the next wave, the next chunks), and query 0 IS row 0, so they tie at the very top."""
    D, Q, (a, b), k = CASES[name]
    G = a * g_tile + b
    rng = np.random.default_rng(sum(map(ord, name)))
    q, g = (rng.integers(-8, 9, (n, D)).astype(np.float32) for n in (Q, G))
    g[0] = np.where(g[0] >= 0, 8, -8)
    ties = [j for j in (0, 1, 4, 32, g_tile, 2 * g_tile + 3) if j < G]
    g[ties] = g[0]
    q[0] = g[0]
    return q, g, k, ties
