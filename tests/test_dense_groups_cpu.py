"""The group read-out on the host (no GPU): mbn_class_groups_layout against the numpy statement of tests/dense_groups_ref.py, every refusal of the
layout and of mbn_resample_groups_envelope, and the premise of the GPU tests: on every pixel of their inputs the two largest group sums differ by
a factor of at least 1 + 2^-10, far above the derived bound, so the GPU tests may require every label equal (and no prob sits at their threshold)."""
import numpy as np
import pytest

import dense_groups_ref as ref


@pytest.mark.parametrize("name", ref.CASES)
def test_layout_and_label_gap(pkg, name):
    x, group_of, groups, sizes, win = ref.case(name)
    rc, slot_class, quad_group = pkg.class_groups_layout(group_of, groups)
    want = ref.layout(group_of, groups)
    assert rc == pkg.OK and np.array_equal(slot_class, want[0]) and np.array_equal(quad_group, want[1])
    assert slot_class.size % 4 == 0 and slot_class.size <= len(group_of) + 3 * groups
    if win:
        assert tuple(pkg.fit_pad(*sizes[0], win[0], win[1])) == win[2], "the window case's rectangle is the letterbox of its source"
    prob_bound, _ = ref.bounds(x.shape[-1], groups)
    assert 4 * prob_bound < ref.GAP - 1
    for H, W in sizes:
        _, prob, _, _, gap = ref.from_interpolants(ref.interpolants(x, H, W, *(win or ())), group_of, groups)
        assert (np.abs(prob - ref.MIN_PROB) > 2 * prob_bound).all(), "%s: a prob too near the threshold of the GPU test (another seed)" % name
        assert gap.min() >= ref.GAP, "%s to %dx%d: two groups within 1 + 2^-10 on %d pixels (another seed)" % (name, H, W, int((gap < ref.GAP).sum()))


@pytest.mark.parametrize("group_of,groups,status", [([0, 1, 2], 2, "EINVAL"), ([0, -2, 1], 2, "EINVAL"), ([-1, -1], 2, "EINVAL"), ([], 1, "EINVAL"),
                                                    ([0, 0], 0, "EINVAL"), ([0, 0], -3, "EINVAL"), ([0, 4096], 4097, "EUNSUPPORTED"),
                                                    ([0, 4095], 4096, "OK")])
def test_layout_refusals(pkg, group_of, groups, status):
    assert pkg.class_groups_layout(group_of, groups)[0] == getattr(pkg, status)


@pytest.mark.parametrize("change,status", [({}, "OK"), ({"rect": None}, "OK"), ({"group_classes": 20}, "EINVAL"), ({"min_prob": 1.5}, "EINVAL"),
                                           ({"min_prob": -0.1}, "EINVAL"), ({"min_prob": float("nan")}, "EINVAL"), ({"batch": 0}, "EINVAL"),
                                           ({"classes": 0, "group_classes": 0}, "EINVAL"), ({"rect": (0, 4, 97, 55)}, "EINVAL"),
                                           ({"in_rows": 1}, "EINVAL"), ({"out_rows": 5}, "EUNSUPPORTED"), ({"rect": None, "out_cols": 11}, "EUNSUPPORTED"),
                                           ({"batch": 65536}, "EUNSUPPORTED"), ({"out_cols": 16385}, "EUNSUPPORTED"),
                                           ({"group_classes": 20, "out_rows": 5}, "EINVAL")])
def test_envelope_refusals(pkg, change, status):
    a = dict(batch=2, rows=2, cols=3, classes=21, group_classes=21, in_rows=64, in_cols=96, rect=(0, 4, 96, 55), out_rows=75, out_cols=130, min_prob=0.5)
    a.update(change)
    assert pkg.resample_groups_envelope(**a) == getattr(pkg, status)
    if a["group_classes"] == a["classes"] and 0 <= a["min_prob"] <= 1:              # otherwise the status of the softmax call of the same form
        plain = (a["batch"], a["rows"], a["cols"], a["classes"])
        want = pkg.resample_window_envelope(*plain, a["in_rows"], a["in_cols"], a["rect"], a["out_rows"], a["out_cols"]) if a["rect"] else \
            pkg.host_lib().mbn_resample_argmax_envelope(*plain, a["out_rows"], a["out_cols"])
        assert getattr(pkg, status) == want
