"""The dense head on the host (no GPU): the reference of the GPU tests (tests/dense_ref.py, the normative arithmetic of
mbn_upsample_argmax_f32) against torch's bilinear interpolate + argmax and on the argmax rule's corner cases; the envelope predicate
mbn_upsample_argmax_envelope through libmbn_host.so; the new symbols where they belong."""
import ctypes as C

import numpy as np
import pytest

import dense_ref

# (n, h, w, classes, S)
TORCH_SHAPES = [(2, 5, 7, 21, 8), (1, 3, 3, 1000, 16), (1, 2, 3, 65, 32), (1, 1, 1, 21, 8)]


def torch_compare(x, S, labels, score, what=""):
    """labels / score [n][H][W] against torch.nn.functional.interpolate(bilinear, align_corners=False).argmax on the CPU. Scores within
    dense_ref.tolerance(x); labels equal wherever torch's top-two margin exceeds twice that (closer than that the two roundings may order
    the classes differently), and at most 1 % of the pixels may be that close. Returns the figures."""
    import torch
    n, h, w, classes = x.shape
    t = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2)
    up = torch.nn.functional.interpolate(t, size=(h * S, w * S), mode="bilinear", align_corners=False)
    top = torch.topk(up, min(2, classes), dim=1)
    t_score, t_label = top.values[:, 0].numpy(), top.indices[:, 0].numpy()
    margin = (top.values[:, 0] - top.values[:, 1]).numpy() if classes > 1 else np.full(t_score.shape, np.inf, np.float32)
    tol = dense_ref.tolerance(x)
    err = float(np.abs(score.astype(np.float64) - t_score.astype(np.float64)).max())
    decided = margin > 2 * tol
    excluded = 1.0 - float(decided.mean())
    mismatches = int((labels[decided] != t_label[decided]).sum())
    print("%s %s: max score diff %.3e (bound %.3e), excluded %.4f %%, label mismatches %d" % (what, x.shape, err, tol, 100 * excluded, mismatches))
    assert err <= tol, (what, err, tol)
    assert excluded <= 0.01, (what, excluded)
    assert mismatches == 0, (what, mismatches)
    return err, tol, excluded, mismatches


def logits_for(shape, seed=0):
    n, h, w, classes, _ = shape
    return (3.0 * np.random.default_rng(seed).standard_normal((n, h, w, classes))).astype(np.float32)


@pytest.mark.parametrize("shape", TORCH_SHAPES)
def test_dense_ref_vs_torch(shape):
    x = logits_for(shape)
    labels, score = dense_ref.upsample_argmax(x, shape[4])
    assert labels.shape == score.shape == (shape[0], shape[1] * shape[4], shape[2] * shape[4])
    assert labels.dtype == np.int32 and score.dtype == np.float32
    torch_compare(x, shape[4], labels, score, "dense_ref")


def test_dense_ref_weights_are_the_formula():
    """Spot values of the index / weight rule: S = 8, 3 coarse samples."""
    i0, i1, w0, w1 = dense_ref.axis(24, 3, 8)
    assert list(i0[:5]) == [0] * 5 and list(w1[:4]) == [0.0] * 4 and w1[4] == np.float32(1 / 16)      # clamped border, first centre at 3.5
    assert (i0[12], i1[12], w1[12]) == (1, 2, np.float32(1 / 16))
    assert (i0[11], i1[11], w1[11]) == (0, 1, np.float32(15 / 16))
    assert (i0[23], i1[23], w1[23]) == (2, 2, np.float32(7 / 16))                                      # y1 clamps to the last sample
    assert np.array_equal(w0 + w1, np.ones(24, np.float32))


def test_dense_ref_argmax_rule():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    x = np.zeros((1, 1, 1, 70), np.float32)
    x[..., 5] = x[..., 66] = 2.0                        # equal maxima in two chunks: the lowest index
    lab, sc = dense_ref.upsample_argmax(x, 8)
    assert (lab == 5).all() and (sc == 2.0).all()
    x[..., 3] = nan                                     # a NaN never wins
    lab, sc = dense_ref.upsample_argmax(x, 8)
    assert (lab == 5).all() and (sc == 2.0).all()
    lab, sc = dense_ref.upsample_argmax(np.full((1, 1, 1, 70), -inf, np.float32), 8)
    assert (lab == 0).all() and (sc == -inf).all()
    lab, sc = dense_ref.upsample_argmax(np.full((1, 2, 2, 3), nan, np.float32), 16)
    assert (lab == 0).all() and (sc == -inf).all()
    x = np.zeros((1, 1, 2, 2), np.float32)             # a weight of zero still multiplies: 1 * 1 + -inf * 0 is a NaN and never wins
    x[0, 0, 0, 1] = 1.0
    x[0, 0, 1, 1] = -1e30
    lab, sc = dense_ref.upsample_argmax(x, 8)
    assert (lab[0, :, :4] == 1).all() and (sc[0, :, :4] == 1.0).all() and (lab[0, :, 4:] == 0).all()
    x[0, 0, 1, 1] = -inf
    lab, sc = dense_ref.upsample_argmax(x, 8)
    assert (lab == 0).all() and (sc == 0.0).all()


# ----------------------------------------------------------------------------------------------------------------------- envelope

def _env(pkg, *a):
    return pkg.host_lib().mbn_upsample_argmax_envelope(*a)


def test_envelope_accepts(pkg):
    for a in [(1, 1, 1, 1, 8), (32, 28, 28, 1000, 8), (32, 14, 14, 1000, 16), (256, 7, 7, 1000, 32), (3, 8, 12, 30, 8), (65535, 1, 1, 21, 32),
              (1, 128, 128, 21, 32)]:
        assert _env(pkg, *a) == pkg.OK, a


def test_envelope_limits(pkg):
    U = pkg.EUNSUPPORTED
    # an image's logits below 2^31 bytes: rows * cols * classes < 2^29 floats
    assert _env(pkg, 1, 1, 1, 2 ** 29 - 1, 8) == pkg.OK
    assert _env(pkg, 1, 1, 1, 2 ** 29, 8) == U
    assert _env(pkg, 5, 64, 64, 2 ** 17 - 1, 8) == pkg.OK         # the batch does not count: it goes through a 64-bit base
    assert _env(pkg, 5, 64, 64, 2 ** 17, 8) == U
    # an image's label map below 2^31 bytes: rows * cols * factor^2 < 2^29 pixels
    assert _env(pkg, 1, 2 ** 9, 2 ** 10 - 1, 2, 32) == pkg.OK     # 2^29 - 2^19 pixels
    assert _env(pkg, 1, 2 ** 9, 2 ** 10, 2, 32) == U              # 2^29
    assert _env(pkg, 1, 1, 2 ** 23 - 1, 1, 8) == pkg.OK
    assert _env(pkg, 1, 1, 2 ** 23, 1, 8) == U
    # the grid: the batch is grid.y
    assert _env(pkg, 65535, 2, 2, 21, 16) == pkg.OK
    assert _env(pkg, 65536, 2, 2, 21, 16) == U


def test_envelope_bad_arguments(pkg):
    for f in (0, 1, 2, 4, 7, 12, 24, 64, -8):
        assert _env(pkg, 1, 4, 4, 21, f) == pkg.EUNSUPPORTED, f
    for a in [(0, 4, 4, 21, 8), (1, 0, 4, 21, 8), (1, 4, 0, 21, 8), (1, 4, 4, 0, 8), (-1, 4, 4, 21, 8)]:
        assert _env(pkg, *a) == pkg.EUNSUPPORTED, a


def test_symbols_where_they_belong(pkg):
    lib, host = pkg.load(), pkg.host_lib()
    for name in ("mbn_upsample_argmax_f32", "mbn_upsample_argmax_envelope", "mbn_net_forward_dense", "mbn_net_segment"):
        assert hasattr(lib, name), name
    assert hasattr(host, "mbn_upsample_argmax_envelope")
    for name in ("mbn_upsample_argmax_f32", "mbn_net_forward_dense", "mbn_net_segment"):      # device code / the net runner: not in the host library
        assert not hasattr(host, name), name
    assert {"mbn_upsample_argmax_f32", "mbn_net_forward_dense", "mbn_net_segment"} <= set(pkg.declared_symbols())
    for cls, name in ((pkg.Context, "upsample_argmax"), (pkg.Net, "forward_dense"), (pkg.Net, "segment")):
        assert callable(getattr(cls, name))
