"""The nearest-neighbour search on a bf16 gallery (include/mbn.h, "Nearest neighbours") in float64 numpy: the rounding a gallery is packed with,
the header's bound B(D), and CASES: the exact cases of tests/test_similarity_bf16_gpu.py. Scores, ranking and inverse norms are similarity_ref's."""
import numpy as np

from similarity_ref import U, inv_norm, inv_norm_bound, rank, scores  # noqa: F401  (the GPU test reads them from here)


def to_bf16(x):
    """fp32 -> bf16 bits (uint16): round to nearest even on the upper 16 bits, a NaN stays a NaN (0x7fc0), beyond the range: infinity."""
    x = np.ascontiguousarray(x, np.float32)
    b = x.view(np.uint32).astype(np.uint64)
    return np.where(np.isnan(x), 0x7fc0, (b + 0x7fff + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def widen(bits): return (bits.astype(np.uint32) << 16).view(np.float32)


def score_bound(q, g, q_scale=None, g_scale=None):
    """|score - score64| <= B(D) 2^-24 |q_scale g_scale| sum_d |q_d g~_d| with B(D) = (3 D + 26) (1 + 2^-6), per pair [Q][G]; g = the widened gallery."""
    return (3 * q.shape[1] + 26) * 1.015625 * U * np.abs(scores(np.abs(q), np.abs(g), q_scale, g_scale))


# name: (D, Q, (a, b) with G = a * g_tile + b, k, s): gallery values in {-1, 0, 1}, query values odd multiples of 2^-s in [1/2, 1) of either sign,
# so every partial sum of plane products is a multiple of 2^-s of magnitude at most D (1 + 2^-7) <= 2^(24 - s): exact in fp32 in any order
CASES = {
    "three planes": (8, 1, (0, 1), 1, 20),              # one partial k-tile through registers; h and m of every element and l of most non-zero
    "tile + rest": (72, 33, (0, 33), 8, 16),            # a k-tile and a remainder; two query blocks
    "one k-tile, chunks": (64, 31, (3, 5), 5, 16),      # DMA; three chunks and a ragged panel
    "ring wrap": (192, 65, (3, 5), 8, 16),              # three k-tiles through a two-slot ring; two query tiles
    "long rows": (1024, 33, (1, -1), 5, 13),
    "long rows, tiles": (1024, 129, (0, 33), 1, 13),
    "sparse wide": (1024, 64, (3, 5), 8, 20),           # 8 non-zeros per query, one in the first and one in the last k-tile: all three planes everywhere
}


def exact_case(name, g_tile):
    """(q fp32, gallery bits, k, ties): rows 1, 4, 32, g_tile and 2 g_tile + 3 repeat row 0 (all +-1); with several queries query 0 IS row 0: ties at the top."""
    D, Q, (a, b), k, s = CASES[name]
    G = a * g_tile + b
    rng = np.random.default_rng(sum(map(ord, name)))
    g = rng.integers(-1, 2, (G, D)).astype(np.float32)
    q = ((rng.integers(2 ** (s - 1), 2 ** s, (Q, D)) | 1) * rng.choice([-1.0, 1.0], (Q, D)) * 2.0 ** -s).astype(np.float32)
    if name == "sparse wide":
        keep = np.zeros((Q, D), bool)
        for row in keep:
            row[np.concatenate([rng.integers(0, 64, 1), rng.integers(D - 64, D, 1), rng.choice(np.arange(64, D - 64), 6, replace=False)])] = True
        q *= keep
    g[0] = np.where(g[0] >= 0, 1, -1)
    ties = [j for j in (0, 1, 4, 32, g_tile, 2 * g_tile + 3) if j < G]
    g[ties] = g[0]
    if Q > 1:
        q[0] = g[0]
    return q, to_bf16(g), k, ties
