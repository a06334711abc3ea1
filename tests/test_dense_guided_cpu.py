"""The guided read-out on the host (no GPU): mbn_guided_lut through libmbn_host.so against numpy, and the block mean of the reference
(tests/dense_guided_ref.py, what the GPU tests compare mbn_guide_reduce_u8 with) on a case worked by hand."""
import ctypes as C

import numpy as np
import pytest

import dense_guided_ref


@pytest.mark.parametrize("sigma", [2.0, 24.0, 1000.0])
def test_lut_against_numpy(pkg, sigma):
    lut = pkg.guided_lut(sigma)
    d = np.arange(766, dtype=np.float64)
    s = np.float64(np.float32(sigma))
    want = np.maximum(np.exp(-d * d / (2.0 * s * s)).astype(np.float32), np.float32(2.0 ** -60))
    assert np.abs(lut.view(np.int32) - want.view(np.int32)).max() <= 1, "more than 1 ulp from numpy (the two exp may differ in the last place)"
    assert lut[0] == 1.0
    assert (np.diff(lut) <= 0).all() and (lut >= np.float32(2.0 ** -60)).all(), "the table increases somewhere or goes under the floor"
    if sigma == 2.0:                              # the floor is reached: exp(-d^2 / 8) passes 2^-60 between d = 18 and d = 19
        assert lut[18] > np.float32(2.0 ** -60) and (lut[19:] == np.float32(2.0 ** -60)).all()
        assert (pkg.guided_lut(1e-30)[1:] == np.float32(2.0 ** -60)).all()


@pytest.mark.parametrize("sigma", [0.0, -1.0, float("nan"), float("inf"), float("-inf")])
def test_lut_refuses_a_sigma_that_is_not_finite_and_positive(pkg, sigma):
    lut = np.zeros(766, np.float32)
    assert pkg.host_lib().mbn_guided_lut(sigma, lut.ctypes.data_as(C.POINTER(C.c_float))) == pkg.EINVAL
    assert not lut.any(), "a refused call wrote the table"


def test_block_mean_worked_by_hand():
    """One 2 x 4 canvas, S = 2: two blocks. R: (1 + 2 + 3 + 4 + 2) / 4 = 3 and (255 * 4 + 2) / 4 = 255; G: (0 + 0 + 0 + 1 + 2) / 4 = 0 (0.25 rounds
    down) and (1 + 1 + 0 + 0 + 2) / 4 = 1 (0.5 rounds up); B: (10 + 11 + 12 + 12 + 2) / 4 = 11 (11.25) and (7 + 8 + 8 + 8 + 2) / 4 = 8 (7.75)."""
    canvas = np.array([[[[1, 0, 10], [2, 0, 11], [255, 1, 7], [255, 1, 8]],
                        [[3, 0, 12], [4, 1, 12], [255, 0, 8], [255, 0, 8]]]], np.uint8)
    want = np.array([[[[3, 0, 11], [255, 1, 8]]]], np.uint8)
    assert np.array_equal(dense_guided_ref.reduce_mean(canvas, 2), want)
    assert np.array_equal(dense_guided_ref.reduce_mean(canvas, 1), canvas)
