"""Reference and case tables of the classifier read-out tests (test_readout_cpu.py gates them, test_readout_gpu.py runs them).

The reference is plain numpy float64: softmax64 (row maximum subtracted, exp in float64), topk_order (the total order value descending, index
ascending on the float32 values: exact, no tolerance; a NaN is never ranked; -1 pads), pool_fc64 (mean over the pixels, then the dot product).

The logit patterns are built per class count. Every FINITE row holds no -0.0 (an FC that adds +0.0 to it would hand back +0.0) and, apart from
the ties a pattern plants on purpose, pairwise distinct values — test_readout_cpu.py checks both.
"""
import math

import numpy as np

U = 2.0 ** -24                     # unit round-off of float32 (round to nearest): one add, one subtract, one divide
EXP_ERR = 2.0 ** -23               # expf: 1 ulp, the accuracy of the device's expf expansion on normal results

CLASS_COUNTS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 129, 255, 256, 257, 511, 513, 1000, 1001, 1023, 1024)   # every form
CLASS_COUNTS_BLOCK = CLASS_COUNTS + (1025, 4097)                                                            # block form and mbn_softmax_f32 only
KS = tuple(range(1, 9))
TAIL_KS = (1, 5, 8)
BATCH = 3                          # direct calls
CU_COUNTS = (3, 8, 20, 72)
CU_SHAPES = ((64, 10), (256, 40), (1024, 1000), (1024, 1001), (1024, 15))        # channels x classes, as tests/test_cu_count_cpu.py
MAPS = ((1, 1), (4, 4), (1, 17), (7, 7), (8, 16), (3, 43), (12, 12), (14, 14))   # 1, 16, 17, 49, 128, 129, 144, 196 taps
POOL_CHANNELS = (64, 192, 1024)
POOL_CLASSES = (1, 15, 16, 17, 1000, 1001, 2049)
POOL_GROUP, POOL_GROUPED_MAX = 16, 128


def sum_adds(classes):
    """Rounding adds on the longest path of the softmax sum: a lane adds its ceil(classes / 256) terms one after the other (the first, to 0, is
    exact), six levels of the xor tree, three adds over the four waves. The wave form sums in the same order."""
    return max(-(-classes // 256) - 1, 0) + 6 + 3


def prob_bound_worst_case(classes):
    """Bound on max_i |p_i - softmax64_i| / max_i softmax64_i of a row, and on |sum_i p_i - 1|, from the arithmetic alone: `classes` float32
    adds (in the kernels' tree), one expf and one divide.
    p_i = fl(e_i / S), e_i = expf(fl(l_i - mx)), S = the float32 sum of the e_j. With d_i = mx - l_i >= 0 and first-order in U:
      the subtraction is off by at most U d_i, which expf turns into a relative error U d_i of e_i, plus expf's own EXP_ERR;
      S is a sum of positive terms, so each of the sum_adds(classes) rounding adds on a path costs at most U relative, and the errors of its
      terms cost their weighted mean: EXP_ERR + U sum_j p_j d_j, where sum_j p_j d_j = entropy - ln(S) <= ln(classes);
      the divide rounds once more: U.
    So rel_i <= U (sum_adds + 1 + d_i + ln classes) + 2 EXP_ERR. Against the row maximum p_max = 1 / S the error of p_i is
    rel_i e^(-d_i) with d e^(-d) <= 1 / e; summed over the row it is sum_i p_i rel_i with sum_i p_i d_i <= ln(classes) again. Both are
    under U (sum_adds + 2 + 2 ln classes) + 2 EXP_ERR: 8.9e-7 for one class, 1.9e-6 for 1000, 2.8e-6 for 4097. A denormal result adds at
    most one denormal step (1.4e-45), far below this."""
    return U * (sum_adds(classes) + 2 + 2 * math.log(classes)) + 2 * EXP_ERR


# Every rounding at its worst and all of one sign is what prob_bound_worst_case adds up; the roundings of a row are neither. Measured on the
# MI355X against float64 (profiles/LOG.md, "Classifier read-out") the largest entry of the per-class-count table (direct calls: every class
# count, every form, every pattern) is 2.13e-7, at 1025 classes; the largest figure of all, 2.66e-7 (4.5 U), is not in that table: it is the
# one-launch tail on the FC logits of test_pool_fc_geometry (its "tail-probs" print, quoted in the paragraph under the table). No trend over
# the class count: the largest terms of a softmax sum are few. The asserted bound is held to at most four times the worst measured figure,
# and it is under the worst case at every class count (test_readout_cpu.py), so it never allows what the arithmetic cannot produce.
# 13 U = 7.7e-7; the 1e-5 max|want| of the older tests is 13 times wider. The constant below is copied by hand from that run.
PROB_BOUND_MEASURED_WORST = 2.66e-7
PROB_BOUND = 13 * U


def prob_bound(classes):
    """what the tests assert: see above"""
    return min(prob_bound_worst_case(classes), PROB_BOUND)


def softmax64(logits):
    x = np.asarray(logits, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - x.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)


def topk_order(logits32, k):
    """[rows][k] int32: the k first entries of each row in the total order (value descending, index ascending) on the float32 values as they
    are; a NaN is never ranked; -1 where the ranked entries run out."""
    x = np.asarray(logits32)
    assert x.dtype == np.float32 and x.ndim == 2
    out = np.full((x.shape[0], k), -1, np.int32)
    for r, row in enumerate(x):
        with np.errstate(invalid="ignore"):
            order = np.argsort(-row.astype(np.float64), kind="stable")      # stable: equal values keep index order; NaN sorts last
        order = order[:int((~np.isnan(row)).sum())][:k]
        out[r, :order.size] = order
    return out


def pool_fc64(x, w, bias=None):
    """x [batch][pix][ch], w [classes][ch], bias [classes] or None -> float64 [batch][classes]"""
    y = np.asarray(x, np.float64).mean(axis=1) @ np.asarray(w, np.float64).T
    return y if bias is None else y + np.asarray(bias, np.float64)


# ----------------------------------------------------------------------------- logit patterns

def base_row(rng, classes, quantum=None):
    """`classes` pairwise distinct values in (-9, 9), none of them 0: normal(0, 3) in shape; with `quantum` multiples of it (then a shift by a
    multiple of the quantum up to 2^24 quanta is exact)."""
    q = quantum or 2.0 ** -12
    lim = int(9 / q)
    v = np.unique(np.clip(np.rint(rng.normal(0, 3 / q, 4 * classes + 64)), -lim, lim).astype(np.int64))
    v = v[v != 0]
    if v.size < classes:                                   # very many classes: fill up with the unused multiples
        v = np.union1d(v, np.setdiff1d(np.arange(-lim, lim + 1), np.append(v, 0))[:classes - v.size])
    return (rng.permutation(v)[:classes] * q).astype(np.float32)


def tie_pairs(classes):
    """Index pairs on the seams of the one-wave form's map (class 64 i + lane -> wave i & 3, trip i >> 2): neighbours in a wave, the same lane
    of the next wave, the same lane of the next trip, the wave and trip boundaries, the two ends."""
    pairs = [(c, c + 1) for c in (0, 62, 63, 255, classes - 2)]
    pairs += [(c, c + 64) for c in (0, 63, 192, classes - 65)]
    pairs += [(c, c + 256) for c in (0, 255, classes - 257)]
    pairs += [(63, 64), (255, 256), (0, classes - 1)]
    seen, out = set(), []
    for a, b in pairs:
        if 0 <= a < b < classes and (a, b) not in seen:
            seen.add((a, b))
            out.append((a, b))
    return out


def tie_rows(classes, seed=0):
    """[(name, row)]: for every pair a row whose maximum sits at both, and one whose second place does (the maximum elsewhere); an all-equal
    row, a row of two values, an ascending and a descending ramp (the winners in one trip of adjacent lanes / spread over the last lanes)."""
    rng = np.random.default_rng(1000 + classes + seed)
    rows = []
    for a, b in tie_pairs(classes):
        r = base_row(rng, classes)
        r[a] = r[b] = 40.0
        rows.append(("max@%d=%d" % (a, b), r))
        if classes >= 3:
            r = base_row(rng, classes)
            r[a] = r[b] = 40.0
            m = next(i for i in (classes // 2, 0, 1, 2) if i not in (a, b))
            r[m] = 50.0
            rows.append(("second@%d=%d" % (a, b), r))
    rows.append(("all-equal", np.full(classes, 0.25, np.float32)))
    rows.append(("two-values", np.where(rng.integers(0, 2, classes) > 0, 1.5, -2.0).astype(np.float32)))
    ramp = (np.arange(classes, dtype=np.float32) - classes // 2) * np.float32(2.0 ** -6) + np.float32(2.0 ** -7)
    rows.append(("ramp-up", ramp))
    rows.append(("ramp-down", ramp[::-1].copy()))
    return rows


SHIFTS = (80.0, -80.0, 1.0e4, -1.0e4)
SHIFT_QUANTUM = 2.0 ** -8          # 1e4 + 9 < 2^14: float32 holds multiples of 2^-10 there, so every shifted value is exact


def magnitude_rows(classes, seed=0):
    """[(name, row, unshifted)]: `unshifted` is the row whose float64 softmax is the reference (the row itself unless a shift cancels)."""
    rng = np.random.default_rng(2000 + classes + seed)
    rows = []
    base = base_row(rng, classes, SHIFT_QUANTUM)
    for s in SHIFTS:
        rows.append(("shift%+g" % s, (base.astype(np.float64) + s).astype(np.float32), base))
    # at 3e38 a float32 step is 2^104: three levels that far apart, the top one shared by every third class
    top = np.float32(3e38)
    r = (np.float64(top) - 2.0 ** 104 * (np.arange(classes) % 3)).astype(np.float32)
    rows.append(("at-3e38", r, r))
    # spread over 104: expf underflows to 0 for most of the row, and nothing may turn NaN
    r = (base_row(rng, classes) - np.float32(130.0) * rng.permutation(classes).astype(np.float32) / max(classes - 1, 1)).astype(np.float32)
    rows.append(("spread130", r, r))
    # denormal logits: the differences are a few steps of 2^-149 and still decide the order
    r = (rng.permutation(classes) % 7 + 1).astype(np.float64) * 2.0 ** -149
    rows.append(("denormal", r.astype(np.float32), r.astype(np.float32)))
    # some entries -inf, not all: they rank last in index order with probability exactly 0
    r = base_row(rng, classes)
    if classes > 1:
        r[rng.permutation(classes)[:max(1, classes // 3)]] = -np.inf
    rows.append(("some-minus-inf", r, r))
    r = np.full(classes, -np.inf, np.float32)
    r[classes - 1] = 3.0
    if classes > 300:
        r[257] = 3.0
    rows.append(("mostly-minus-inf", r, r))
    return rows


def nonfinite_rows(classes, seed=0):
    """[(name, row)]: rows without a finite maximum, or with a NaN in them (include/mbn.h at mbn_softmax_f32 states what they give)."""
    rng = np.random.default_rng(3000 + classes + seed)
    rows = [("all-minus-inf", np.full(classes, -np.inf, np.float32)), ("all-nan", np.full(classes, np.nan, np.float32))]
    r = base_row(rng, classes)
    r[classes // 2] = np.nan
    rows.append(("one-nan", r))
    r = np.full(classes, np.nan, np.float32)
    r[::2] = -np.inf
    rows.append(("nan-and-minus-inf", r))
    r = base_row(rng, classes)
    r[classes - 1] = np.inf
    rows.append(("plus-inf", r))
    if classes > 1:
        r = np.full(classes, np.nan, np.float32)
        r[classes - 1] = 1.0
        rows.append(("nan-but-last", r))
    return rows


def random_rows(classes, rows, seed=0):
    """the data of the class-count cases: normal(0, 3), as the existing softmax tests use"""
    return np.random.default_rng(4000 + classes + seed).normal(0, 3, (rows, classes)).astype(np.float32)


def has_max(row):
    """the row has a finite maximum and no NaN: its probabilities are numbers"""
    return bool(np.isfinite(np.max(row))) if not np.isnan(row).any() else False


def finite_patterns(classes):
    """[(name, row, unshifted)] of items 2 and 3: every row has a finite maximum"""
    return [(n, r, r) for n, r in tie_rows(classes)] + magnitude_rows(classes)


def all_patterns(classes):
    """items 2, 3 and 4"""
    return finite_patterns(classes) + [(n, r, r) for n, r in nonfinite_rows(classes)]


def fc_for_rows(rows, channels=64):
    """An FC filter [classes][channels] whose column j is rows[j] and whose other columns are 0, and the images [len(rows)][channels] e_j
    (1 in channel j, a 1 x 1 map): pool + FC without a bias hands back rows[j] for image j bit for bit, as long as every row is finite (0 times
    a finite value is 0, and adding 0 changes nothing but a -0.0). A row that is not finite goes alone, in column 0, for every image of its call."""
    rows = np.asarray(rows, np.float32)
    n, classes = rows.shape
    assert n <= 64
    w = np.zeros((classes, channels), np.float32)
    w[:, :n] = rows.T
    x = np.zeros((n, channels), np.float32)
    x[np.arange(n), np.arange(n)] = 1.0
    return w, x


def pool_path(pix):
    return "unrolled49" if pix == 49 else "grouped" if pix <= POOL_GROUPED_MAX else "loop"
