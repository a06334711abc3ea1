"""Segment with runners-up without a GPU: the numpy reference (tests/dense_topk_ref.py) against the argmax references it extends, against its own
prefix property and against torch.topk of the same interpolants; every status of mbn_resample_topk_envelope and of the ragged form's check."""
import numpy as np
import pytest
import torch

import dense_any_ref
import dense_prob_ref
import dense_topk_ref as T
import dense_window_ref


def _x(n, h, w, classes, seed):
    return np.random.default_rng(seed).standard_normal((n, h, w, classes)).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_rank_0_is_the_argmax_reference(k):
    x = _x(2, 3, 3, 21, 1)
    x[0, 1, 1, 4] = np.nan
    x[1, 0, 0, :] = -np.inf
    lab, sc, pr = T.resample_topk(x, 13, 17, k)
    want_lab, want_sc = dense_any_ref.resample_argmax(x, 13, 17)
    assert np.array_equal(lab[0], want_lab) and np.array_equal(_bits(sc[0]), _bits(want_sc))
    _, _, want_pr = dense_prob_ref.resample_softmax(x, 13, 17)
    assert np.array_equal(pr[0], want_pr)                   # the same float64 formula at rank 0
    window = (64, 64, (3, 8, 58, 48))
    lab, sc, _ = T.resample_topk(x, 13, 17, k, window=window)
    want_lab, want_sc = dense_window_ref.resample_argmax_window(x, 64, 64, window[2], 13, 17)
    assert np.array_equal(lab[0], want_lab) and np.array_equal(_bits(sc[0]), _bits(want_sc))


def test_prefix_property():
    x = _x(2, 3, 3, 7, 2)
    x[0, :, :, 2] = np.nan
    x[..., 5] = x[..., 1]                                   # equal values: ascending class order
    full = T.resample_topk(x, 13, 17, 7)
    for k in (1, 2, 5):
        part = T.resample_topk(x, 13, 17, k)
        for a, b in zip(part, full):
            assert np.array_equal(a, b[:k], equal_nan=True)
    lab = full[0]
    both = (lab == 1) | (lab == 5)
    first = both.argmax(axis=0)                             # wherever both are present, 1 comes directly in front of 5
    assert (np.take_along_axis(lab, first[None], axis=0)[0] == 1).all()


def test_against_torch_topk():
    """tie-free random logits: an independent selection over the same [H][W][classes] interpolants"""
    x = _x(2, 5, 4, 101, 3)
    v = dense_any_ref.resample(x, 45, 37)
    lab, sc, pr = T.from_interpolants(v, 8)
    tv, ti = torch.topk(torch.from_numpy(v), 8, dim=-1)
    assert np.array_equal(lab, np.moveaxis(ti.numpy(), -1, 0).astype(np.int32))
    assert np.array_equal(_bits(sc), _bits(np.moveaxis(tv.numpy(), -1, 0)))
    p = torch.softmax(torch.from_numpy(v).double(), dim=-1).numpy()
    want = np.moveaxis(np.take_along_axis(p, ti.numpy(), axis=-1), -1, 0)
    assert np.allclose(pr, want, rtol=1e-12, atol=0)


def test_unfilled_slots():
    x = np.full((1, 2, 2, 5), np.nan, np.float32)
    lab, sc, pr = T.resample_topk(x, 9, 11, 3)
    assert (lab[0] == 0).all() and (lab[1:] == -1).all() and (sc == -np.inf).all() and (pr == 0).all()
    x[..., 3] = 1.0
    x[..., 1] = np.inf
    lab, sc, pr = T.resample_topk(x, 9, 11, 3)
    top = sc[0] == np.inf                                   # (a zero weight times inf is a NaN: at the clamped borders class 3 is alone)
    assert top.any() and not top.all() and (lab[2] == -1).all()
    assert (lab[0][top] == 1).all() and (lab[1][top] == 3).all() and (pr[:, top] == 0).all()              # a +inf best: every prob is 0
    assert (lab[0][~top] == 3).all() and (lab[1][~top] == -1).all() and (pr[0][~top] == 1).all()
    assert (T.tolerance(5, sc, pr)[:, top] == 0).all() and (T.tolerance(5, sc, pr)[1:] == 0).all()


def test_envelope_statuses(pkg):
    OK, EINVAL, EUNS = pkg.OK, pkg.EINVAL, pkg.EUNSUPPORTED
    env = pkg.resample_topk_envelope
    assert pkg.TOPK_MAX == T.TOPK_MAX == 8
    for k in range(1, 9):
        assert env(2, 3, 3, 8, 0, 0, None, 13, 17, k) == OK
    assert env(2, 3, 3, 8, 0, 0, None, 13, 17, 0) == EINVAL
    assert env(2, 3, 3, 8, 0, 0, None, 13, 17, 9) == EINVAL
    assert env(2, 3, 3, 7, 0, 0, None, 13, 17, 8) == EINVAL              # k > classes
    assert env(2, 3, 3, 7, 0, 0, None, 13, 17, 7) == OK
    assert env(0, 3, 3, 8, 0, 0, None, 13, 17, 1) == EINVAL              # the argmax envelope's
    assert env(2, 3, 3, 8, 0, 0, None, 11, 17, 1) == EUNS                # below ratio 4
    assert env(2, 3, 3, 7, 0, 0, None, 11, 17, 8) == EINVAL              # an EINVAL goes in front of an EUNSUPPORTED
    assert env(65536, 3, 3, 8, 0, 0, None, 13, 17, 1) == EUNS
    rect = (3, 8, 58, 48)
    assert env(2, 3, 3, 8, 64, 64, rect, 13, 17, 5) == OK
    assert env(2, 3, 3, 8, 64, 64, (3, 8, 62, 48), 13, 17, 5) == EINVAL  # the window envelope's: past the input
    assert env(2, 3, 3, 8, 64, 64, (0, 0, 64, 64), 11, 17, 5) == EUNS
    assert env(2, 3, 3, 8, 2, 64, rect, 13, 17, 5) == EINVAL             # in_rows < rows
    # the planes: k * batch * out_rows * out_cols up to 2^40 elements
    assert pkg.TOPK_MAX_ELEMENTS == 1 << 40
    assert env(4096, 1, 1, 8, 0, 0, None, 16384, 16384, 1) == OK         # 2^40 exactly
    assert env(4096, 1, 1, 8, 0, 0, None, 16384, 16384, 2) == EUNS
    assert env(512, 1, 1, 8, 0, 0, None, 16384, 16384, 8) == OK
    assert env(513, 1, 1, 8, 0, 0, None, 16384, 16384, 8) == EUNS
    # same answers as the envelope of the same form at every k inside the classes
    for args in [(2, 3, 3, 8, 13, 17), (2, 3, 3, 8, 12, 12), (2, 5, 7, 8, 20, 28), (1, 1, 1, 8, 16385, 4)]:
        assert env(args[0], args[1], args[2], args[3], 0, 0, None, args[4], args[5], 3) == pkg.resample_argmax_envelope(*args)


def test_ragged_check_statuses(pkg):
    OK, EINVAL, EUNS = pkg.OK, pkg.EINVAL, pkg.EUNSUPPORTED
    chk = pkg.resample_topk_ragged_check
    assert chk(21, 1000, 5, 1000) == OK and chk(21, 1000, 5, 999) == EINVAL and chk(21, 1000, 5, 5000) == OK
    assert chk(21, 1000, 0, 1000) == EINVAL and chk(21, 1000, 9, 1000) == EINVAL and chk(4, 1000, 5, 1000) == EINVAL
    assert chk(21, 1000, 8, 1 << 37) == OK and chk(21, 1000, 8, (1 << 37) + 1) == EUNS
    assert chk(0, 1000, 1, 1000) == EINVAL and chk(21, 0, 1, 1000) == EINVAL
