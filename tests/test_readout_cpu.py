"""The reference and the case tables of the classifier read-out tests (tests/readout_ref.py), checked without a GPU: the reference against
torch in float64, and for every table of test_readout_gpu.py the conditions its comparisons rest on — planted ties are ties and nothing else is,
shifts are exact, the FC that reproduces chosen logits does so exactly, every pooling path and both sides of each boundary are in the maps, and no
row is left out of a comparison."""
import numpy as np
import pytest
import torch

import cu_model as M
import readout_ref as R


def test_reference_against_torch_on_tie_free_rows():
    for classes in (1, 2, 17, 1000, 4097):
        x = R.random_rows(classes, 4)
        assert all(np.unique(r).size == classes for r in x), "tie-free data wanted"
        want = torch.softmax(torch.from_numpy(x).double(), dim=1).numpy()
        assert np.abs(R.softmax64(x) - want).max() <= 4 * np.finfo(np.float64).eps
        for k in R.KS:
            kk = min(k, classes)
            idx = torch.topk(torch.from_numpy(x), kk, dim=1).indices.numpy()
            got = R.topk_order(x, k)
            assert np.array_equal(got[:, :kk], idx) and (got[:, kk:] == -1).all()
    x = np.random.default_rng(0).uniform(0, 6, (3, 10, 64)).astype(np.float32)
    w = np.random.default_rng(1).normal(0, 1, (5, 64)).astype(np.float32)
    b = np.arange(5, dtype=np.float32)
    want = torch.from_numpy(x).double().mean(1) @ torch.from_numpy(w).double().T + torch.from_numpy(b).double()
    assert np.abs(R.pool_fc64(x, w, b) - want.numpy()).max() <= 1e-13


def test_topk_order_contract():
    """value descending, index ascending; -inf last in index order; a NaN never; -1 pads (the contract of _topk_ref in test_parity_gpu.py)"""
    row = np.array([[1, 5, -np.inf, 5, np.nan, -np.inf, 0]], np.float32)
    assert R.topk_order(row, 8).tolist() == [[1, 3, 0, 6, 2, 5, -1, -1]]
    assert R.topk_order(np.full((1, 3), np.nan, np.float32), 2).tolist() == [[-1, -1]]
    assert R.topk_order(np.full((1, 3), -np.inf, np.float32), 2).tolist() == [[0, 1]]
    rng = np.random.default_rng(2)
    x = rng.integers(-3, 4, (5, 40)).astype(np.float32)
    for i, row in enumerate(x):
        want = sorted(range(40), key=lambda j: (-float(row[j]), j))[:8]
        assert R.topk_order(x, 8)[i].tolist() == want


@pytest.mark.parametrize("classes", R.CLASS_COUNTS_BLOCK)
def test_pattern_tables(classes):
    ties = R.tie_rows(classes)
    names = [n for n, _ in ties]
    for a, b in R.tie_pairs(classes):
        assert 0 <= a < b < classes
    for name, row in ties:
        assert row.dtype == np.float32 and row.shape == (classes,) and np.isfinite(row).all() and not (np.signbit(row) & (row == 0)).any()
        order = R.topk_order(row[None], 8)[0]
        vals = row[order[order >= 0]]
        if name.startswith(("max@", "second@")):
            a, b = [int(s) for s in name.split("@")[1].split("=")]
            first = 0 if name.startswith("max@") else 1
            assert order[first] == a and order[first + 1] == b and vals[first] == vals[first + 1], name        # gap 0 where a tie is planted ...
            assert np.unique(row).size == classes - 1, name                                                      # ... and nowhere else
            if first:
                assert vals[0] > vals[1]
    # the seams: neighbours, the next wave's lane, the next trip's lane, the wave and trip boundaries, the two ends — wherever the row is long enough
    for want, need in (("max@0=1", 2), ("max@0=64", 65), ("max@0=256", 257), ("max@63=64", 65), ("max@255=256", 257), ("max@0=%d" % (classes - 1), 2)):
        assert (want in names) == (classes >= need), want
    assert {"all-equal", "two-values", "ramp-up", "ramp-down"} <= set(names)
    two = dict(ties)["two-values"]
    assert np.unique(two).size == (2 if classes > 1 else 1) or classes < 8
    up = dict(ties)["ramp-up"]
    assert (np.diff(up) > 0).all() and R.topk_order(up[None], 1)[0, 0] == classes - 1 and R.topk_order(dict(ties)["ramp-down"][None], 1)[0, 0] == 0

    mags = R.magnitude_rows(classes)
    for name, row, ref in mags:
        assert row.dtype == np.float32 and not np.isnan(row).any() and R.has_max(row), name
        assert not (np.signbit(row) & (row == 0)).any(), name
        if name.startswith("shift"):
            s = float(name[5:])
            assert np.array_equal(row.astype(np.float64), ref.astype(np.float64) + s), "the shift is not exact: " + name
            assert np.array_equal(R.topk_order(row[None], 8), R.topk_order(ref[None], 8))
    d = {n: r for n, r, _ in mags}
    p = R.softmax64(d["spread130"])
    if classes >= 16:
        assert float(d["spread130"].max() - d["spread130"].min()) > 104 and (p < 2.0 ** -150).mean() > 0.1
    assert np.isfinite(d["at-3e38"]).all() and d["at-3e38"].max() == np.float32(3e38)
    assert (d["denormal"] > 0).all() and d["denormal"].max() < 2.0 ** -126
    if classes > 1:
        m = np.isinf(d["some-minus-inf"])
        assert 0 < m.sum() < classes and (R.softmax64(d["some-minus-inf"])[m] == 0).all()
        order = R.topk_order(d["mostly-minus-inf"][None], 8)[0]
        fin = int(np.isfinite(d["mostly-minus-inf"]).sum())
        assert np.isfinite(d["mostly-minus-inf"][order[:fin]]).all() and (np.diff(order[fin:][order[fin:] >= 0]) > 0).all()

    bad = R.nonfinite_rows(classes)
    assert {"all-minus-inf", "all-nan", "one-nan", "plus-inf"} <= {n for n, _ in bad}
    for name, row in bad:
        assert not R.has_max(row), name
        assert np.isnan(R.softmax64(row)).all(), name                 # what the contract says of such a row: every probability NaN
        order = R.topk_order(row[None], 8)[0]
        assert ((order == -1) | ((order >= 0) & (order < classes))).all()

    # share of rows left out of a comparison: none. Every row of every table is ranked exactly; every row with a maximum is compared with
    # softmax64, every other one with the all-NaN row the contract states.
    rows = R.all_patterns(classes)
    assert sum(R.has_max(r) for _, r, _ in rows) == len(ties) + len(mags) and len(rows) == len(ties) + len(mags) + len(bad)
    rnd = R.random_rows(classes, R.BATCH)
    assert all(R.has_max(r) for r in rnd)


@pytest.mark.parametrize("classes", R.CLASS_COUNTS)
@pytest.mark.parametrize("channels", [64, 256, 1024])
def test_fc_reproduces_the_logits_exactly(classes, channels):
    """logits = w[:, j] for image e_j: the products with 0 and the sums with 0 are exact in any order, in float32 as in float64"""
    rows = [r for _, r, _ in R.finite_patterns(classes) if np.isfinite(r).all()][:64]
    w, x = R.fc_for_rows(rows, channels)
    assert w.shape == (classes, channels) and x.shape == (len(rows), channels)
    got = R.pool_fc64(x[:, None, :], w)
    assert np.array_equal(got.astype(np.float32).view(np.uint32), np.asarray(rows, np.float32).view(np.uint32))
    for j in range(len(rows)):
        assert np.array_equal(w[:, j], rows[j]) and x[j, j] == 1 and x[j].sum() == 1
    assert not w[:, len(rows):].any()
    # a row that is not finite goes alone in column 0 and every other weight is 0: image e_0 meets no 0 * inf
    for _, r in R.nonfinite_rows(classes):
        w, x = R.fc_for_rows(r[None], channels)
        assert not w[:, 1:].any() and x.tolist() == [[1.0] + [0.0] * (channels - 1)]


def test_bounds_and_geometry_tables():
    # the bound grows with the sum's depth, stays far under the 1e-5 the existing tests allow, and is what the docstring derives
    assert R.sum_adds(1) == 9 and R.sum_adds(256) == 9 and R.sum_adds(257) == 10 and R.sum_adds(4097) == 25
    for c in R.CLASS_COUNTS_BLOCK:
        assert 2 * R.EXP_ERR + 11 * R.U <= R.prob_bound_worst_case(c) < 3.5e-6
        # the asserted bound: never over what the arithmetic allows, at most four times the worst error measured, far under the old 1e-5
        assert R.prob_bound(c) <= R.prob_bound_worst_case(c) and R.PROB_BOUND_MEASURED_WORST < R.prob_bound(c) <= 4 * R.PROB_BOUND_MEASURED_WORST
        assert R.prob_bound(c) < 1e-5 / 10
    assert set(R.CLASS_COUNTS) <= set(R.CLASS_COUNTS_BLOCK) and max(R.CLASS_COUNTS) == 1024 and max(R.CLASS_COUNTS_BLOCK) == 4097
    for need in (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024):
        assert need in R.CLASS_COUNTS
    # maps: all three summation paths, both sides of the group size and of POOL_GROUPED_MAX
    taps = [r * c for r, c in R.MAPS]
    assert taps == [1, 16, 17, 49, 128, 129, 144, 196]
    assert {R.pool_path(t) for t in taps} == {"unrolled49", "grouped", "loop"}
    assert R.POOL_GROUP in taps and R.POOL_GROUP + 1 in taps and R.POOL_GROUPED_MAX in taps and R.POOL_GROUPED_MAX + 1 in taps
    # planning counts: one class range at 3 CUs x 1024 channels, a short last range at 20 and 72 (the model of tests/cu_model.py)
    assert M.poolfc_plan(1024, 1000, 3)["nns"] == 1
    for cus in (20, 72):
        p = M.poolfc_plan(1024, 1000, cus)
        assert p["nns"] > 1 and 1000 - (p["nns"] - 1) * p["npc"] < p["npc"]
    for channels, classes in R.CU_SHAPES:
        assert classes <= 1024 and channels % 64 == 0
        plans = {cus: M.poolfc_plan(channels, classes, cus) for cus in R.CU_COUNTS + (256,)}
        assert all(1 <= p["nns"] <= 64 for p in plans.values())
    assert len({M.poolfc_plan(1024, 1000, cus)["nns"] for cus in R.CU_COUNTS + (256,)}) >= 3
