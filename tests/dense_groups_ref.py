"""The dense head's read-out by class groups: the normative arithmetic of mbn_resample_groups_f32 (include/mbn.h, "Segment by class groups") on
top of dense_window_ref. The interpolated logits v are its float32 values, bit for bit (the whole map is the window that covers the whole input);
the group sums, prob and score are the FLOAT64 evaluation on them. The kernel's fp32 prob and score are held to bounds(); its labels must be equal
wherever the two largest group sums differ by `GAP`, which the inputs below do on every pixel (test_dense_groups_cpu.py asserts it)."""
import math

import numpy as np

import dense_window_ref

GAP = 1.0 + 2.0 ** -10


def layout(group_of, groups):
    """mbn_class_groups_layout in numpy: (slot_class, quad_group)"""
    group_of, slot_class, quad_group = np.asarray(group_of), [], []
    for g in range(groups):
        members = np.flatnonzero(group_of == g)
        if members.size:
            quads = (members.size + 3) // 4
            slot_class += list(members) + [-1] * (4 * quads - members.size)
            quad_group += [-1] * (quads - 1) + [g]
    return np.array(slot_class, np.int32), np.array(quad_group, np.int32)


def bounds(classes, groups):
    """(prob's relative bound, score's absolute bound without its |m| * 2^-24 term): include/mbn.h derives both"""
    L = math.log(classes * groups)
    A = classes + groups + 2.5 * (16 + 2 * L) + 3 + (2 + math.ceil(L / 16)) * (2.5 * (16 + L) + 3)
    return (2 * A + 1) * 2.0 ** -24, (1.01 * A + 4 * (16 + L) + 16) * 2.0 ** -24


def interpolants(x, H, W, in_rows=0, in_cols=0, rect=None):
    n, h, w, _ = x.shape
    return dense_window_ref.resample_window(x, in_rows, in_cols, rect, H, W) if rect else dense_window_ref.resample_window(x, h, w, (0, 0, w, h), H, W)


def from_interpolants(v, group_of, groups):
    """v float32 [..., classes] -> (labels int32, prob, score, m, gap) [...], float64: gap = the ratio of the two largest group sums (inf with one
    non-empty group and where m is not finite: the label there is the rule's, the lowest non-empty group)"""
    group_of = np.asarray(group_of)
    v = np.asarray(v, np.float32).astype(np.float64)
    kept = v[..., group_of >= 0]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.where(np.isnan(kept), -np.inf, kept).max(axis=-1)
        finite = np.isfinite(m)
        e = np.where(np.isnan(v), 0.0, np.exp(v - np.where(finite, m, 0.0)[..., None]))
        S = np.stack([e[..., group_of == g].sum(axis=-1) if (group_of == g).any() else np.full(m.shape, -1.0) for g in range(groups)], axis=-1)
        first = int(group_of[group_of >= 0].min())
        label = np.where(finite, S.argmax(axis=-1), first).astype(np.int32)            # the first of equal maxima: the lowest group
        top = np.sort(S, axis=-1)
        best = top[..., -1]
        prob = np.where(finite, best / S.clip(0).sum(axis=-1), 0.0)
        score = np.where(finite, m + np.log(best), m)
        second = top[..., -2] if groups > 1 else np.zeros(m.shape)
        gap = np.where(finite & (second > 0), best / second, np.inf)
    return label, prob, score, m, gap


# The inputs of the GPU tests, by name: (x float32 [n][h][w][classes], group_of, groups, [(H, W), ...], (in_rows, in_cols, rect) or None).
# SEEDS: found on the CPU so that every pixel keeps its two largest group sums GAP apart (a resampled field crosses every label boundary somewhere,
# so most seeds leave a few pixels closer than that)
SEEDS = {"padding": 1, "window": 2, "one group": 1, "straddle": 4, "straddle 64": 2, "identity": 2, "dropped": 2, "ramps": 2, "special": 2}
MIN_PROB = 0.5      # the threshold of the GPU tests: no pixel of these inputs has a prob within twice the bound of it


def case(name, seed=None):
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    normal = lambda n, h, w, c, s=8.0: (s * rng.standard_normal((n, h, w, c))).astype(np.float32)
    if name == "padding":              # groups of 1 / 3 / 1 classes: NaN pad slots, a partial tile, rows that cross
        return normal(2, 2, 3, 5), [0, 1, 1, 1, 2], 3, [(9, 13)], None
    if name == "window":               # the same through the letterbox rectangle of a 64 x 96 input
        return normal(2, 2, 3, 5), [0, 1, 1, 1, 2], 3, [(30, 52)], (64, 96, (0, 4, 96, 55))
    if name == "one group":
        return normal(2, 2, 3, 9), [0] * 9, 1, [(9, 13)], None
    if name == "straddle":             # two singles, one group of 131 members open across the chunk ends at 64 and 128, seven singles
        x = normal(1, 3, 3, 140, 2.0)
        group_of = np.array([0, 1] + [2] * 131 + list(range(3, 10)))
        x[..., group_of != 2] += 4.0   # a single at +4 weighs about as much as the 131 together
        return x, group_of, 10, [(37, 41), (12, 12)], None
    if name == "straddle 64":          # a 10 x 10 footprint: the launch whose chunk is 64 slots
        x = normal(1, 10, 10, 140, 2.0)
        group_of = np.array([0, 1] + [2] * 131 + list(range(3, 10)))
        x[..., group_of != 2] += 4.0
        return x, group_of, 10, [(40, 40)], None
    if name == "identity":
        return normal(2, 3, 5, 21), np.arange(21), 21, [(33, 70)], None
    if name == "dropped":              # the largest logits sit in classes that are left out; group 2 has no class
        group_of = np.array([0, -1, 1, 1, 3, -1, 3, 4, 4, 4, 0, -1])
        x = normal(2, 3, 5, 12)
        x[..., group_of < 0] += 20.0
        return x, group_of, 5, [(33, 70)], None
    if name == "ramps":                # up by 3 a class for 20 classes, then down: the reference moves several times while bsum is alive
        c = np.arange(40)
        ramp = np.where(c < 20, 3.0 * c, 54.0 - 3.0 * (c - 20)).astype(np.float32)
        return normal(2, 3, 5, 40, 4.0) + ramp, c // 10, 4, [(33, 70)], None
    if name == "special":              # NaN, +inf, -inf, and a vector of NaNs: pixels without a finite maximum
        x = normal(2, 3, 5, 5)
        x[0, 1, 2, 3], x[0, 2, 1, 0], x[1, 0, 4, 2] = np.nan, np.inf, -np.inf
        x[1, 0, 0, :] = np.nan
        return x, [0, 1, 1, 1, 2], 3, [(33, 70)], None
    raise KeyError(name)


CASES = ["padding", "window", "one group", "straddle", "straddle 64", "identity", "dropped", "ramps", "special"]
