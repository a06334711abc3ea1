"""The dense head at any output size on the host (no GPU): the reference of the GPU tests (tests/dense_any_ref.py, the normative arithmetic of
mbn_resample_argmax_f32) against dense_ref at integer factors (bit for bit), against torch's bilinear interpolate on float64 inputs, and on the
weight rule's chosen coordinates; the envelope predicate and the ragged set's check through libmbn_host.so; the new symbols where they belong."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dense_any_ref
import dense_ref
from test_dense_cpu import logits_for


# ---------------------------------------------------------------------------------------------------------------- integer factors

@pytest.mark.parametrize("S", [8, 16, 32])
@pytest.mark.parametrize("shape", [(2, 5, 7, 21), (1, 3, 3, 65), (1, 2, 3, 33), (1, 1, 1, 21)])
def test_ref_equals_dense_ref_at_integer_factors(shape, S):
    n, h, w, classes = shape
    x = logits_for(shape + (S,), seed=h * 10 + w + S)
    for got, want in zip(dense_any_ref.axis(h * S, h), dense_ref.axis(h * S, h, S)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    up, want_up = dense_any_ref.resample(x, h * S, w * S), dense_ref.upsample(x, S)
    assert np.array_equal(up.view(np.uint32), want_up.view(np.uint32))
    lab, sc = dense_any_ref.resample_argmax(x, h * S, w * S)
    want_lab, want_sc = dense_ref.upsample_argmax(x, S)
    assert lab.dtype == np.int32 and sc.dtype == np.float32
    assert np.array_equal(lab, want_lab) and np.array_equal(sc.view(np.uint32), want_sc.view(np.uint32))


# -------------------------------------------------------------------------------------------------------------------------- torch

# (n, h, w, classes, H, W)
TORCH_SHAPES = [(2, 5, 7, 21, 37, 61), (1, 7, 7, 21, 30, 28), (1, 4, 6, 65, 16, 24), (1, 3, 5, 21, 100, 23), (1, 1, 1, 5, 9, 4),
                (1, 14, 20, 21, 375, 500)]


def torch_compare(x, H, W, labels, score, what=""):
    """labels / score [n][H][W] against torch.nn.functional.interpolate(x.double(), size=(H, W), bilinear, align_corners=False) on the CPU.
    Scores within dense_any_ref.tolerance(x) = 10 * 2^-24 * max|x|; labels equal wherever torch's top-two margin exceeds twice that; at most
    1 % of the pixels may be that close. Returns the figures."""
    import torch
    n, h, w, classes = x.shape
    t = torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2).double()
    up = torch.nn.functional.interpolate(t, size=(H, W), mode="bilinear", align_corners=False)
    top = torch.topk(up, min(2, classes), dim=1)
    t_score, t_label = top.values[:, 0].numpy(), top.indices[:, 0].numpy()
    margin = (top.values[:, 0] - top.values[:, 1]).numpy() if classes > 1 else np.full(t_score.shape, np.inf)
    tol = dense_any_ref.tolerance(x)
    err = float(np.abs(score.astype(np.float64) - t_score).max())
    decided = margin > 2 * tol
    excluded = 1.0 - float(decided.mean())
    mismatches = int((labels[decided] != t_label[decided]).sum())
    print("%s %s -> %dx%d: max score diff %.3e = %.2f of the bound %.3e, excluded %.4f %%, label mismatches %d"
          % (what, x.shape, H, W, err, err / tol, tol, 100 * excluded, mismatches))
    assert err <= tol, (what, err, tol)
    assert excluded <= 0.01, (what, excluded)
    assert mismatches == 0, (what, mismatches)
    return err, tol, excluded, mismatches


@pytest.mark.parametrize("shape", TORCH_SHAPES)
def test_ref_vs_torch_float64(shape):
    n, h, w, classes, H, W = shape
    x = logits_for((n, h, w, classes, 0))
    labels, score = dense_any_ref.resample_argmax(x, H, W)
    assert labels.shape == score.shape == (n, H, W)
    torch_compare(x, H, W, labels, score, "dense_any_ref")


# ----------------------------------------------------------------------------------------------------------------- the weight rule

def test_weight_rule_at_chosen_coordinates():
    # n = 5 -> N = 37: den = 74
    i0, i1, w0, w1 = dense_any_ref.axis(37, 5)
    assert (i0[0], i1[0], w1[0], w0[0]) == (0, 1, 0.0, 1.0)                       # o = 0: (1 * 5 - 37) clamps to 0
    assert (i0[3], w1[3]) == (0, 0.0) and (i0[4], w1[4]) == (0, np.float32(np.float64(8) / 74))      # the clamp ends between o = 3 and o = 4
    assert (i0[36], i1[36]) == (4, 4)                                             # o = N - 1: i1 clamps to the last sample
    assert w1[36] == np.float32(np.float64((73 * 5 - 37) % 74) / 74)
    assert (i0[18], i1[18], w1[18]) == (2, 3, 0.0)                                # the centre: num = 37 * 5 - 37 = 148 = 2 * 74, num % den == 0
    # a weight is the float64 quotient rounded once: for den = 74 the float32 division of the float32 operands gives the same here, but the
    # definition does not rest on that
    for o in range(37):
        num = max((2 * o + 1) * 5 - 37, 0)
        assert w1[o] == np.float32(np.float64(num % 74) / np.float64(74)) and w0[o] == np.float32(1.0) - w1[o]
    # n = 1: both indices are 0 everywhere; the weights still follow the rule (num = 2o + 1 - 9 past the clamp) and multiply the same sample
    i0, i1, w0, w1 = dense_any_ref.axis(9, 1)
    assert not i0.any() and not i1.any()
    assert list(w1) == [np.float32(np.float64(max(2 * o - 8, 0)) / 18) for o in range(9)] and w1[8] == np.float32(8 / 18)
    # the minimum ratio, 7 -> 28: a dyadic quarter grid, i0 steps every four outputs
    i0, i1, w0, w1 = dense_any_ref.axis(28, 7)
    assert list(i0[:8]) == [0, 0, 0, 0, 0, 0, 1, 1] and list(w1[:8]) == [0.0, 0.0, 0.125, 0.375, 0.625, 0.875, 0.125, 0.375]
    assert w1.dtype == np.float32 and w0.dtype == np.float32 and i1.max() == 6


def test_footprint_bound_holds():
    """What the kernel's LDS sizing rests on: along an axis a 32-output tile touches at most min(n, floor(31 n / N) + 3) coarse samples, and
    four consecutive outputs at most three (their i0 spans at most one step), for every N >= 4 n."""
    for n in (1, 2, 3, 5, 7, 9, 14, 28, 33):
        for N in sorted({4 * n, 4 * n + 1, 5 * n - 1, 8 * n, 8 * n + 3, 16 * n, 33 * n + 1, 100}):
            if N < 4 * n:
                continue
            i0, i1, _, _ = dense_any_ref.axis(N, n)
            bound = min(n, 31 * n // N + 3)
            for o in range(0, N, 32):
                assert i1[o:o + 32].max() - i0[o] + 1 <= bound, (n, N, o)
            for o in range(0, N, 4):
                assert i0[o:o + 4].max() - i0[o] <= 1, (n, N, o)


# ----------------------------------------------------------------------------------------------------------------------- envelope

def _env(pkg, *a):
    return pkg.resample_argmax_envelope(*a)


def test_envelope_accepts(pkg):
    for a in [(1, 1, 1, 1, 4, 4), (32, 28, 28, 1000, 375, 500), (32, 14, 14, 1000, 375, 500), (3, 5, 7, 21, 37, 61), (65535, 1, 1, 21, 9, 4),
              (1, 7, 7, 1000, 224, 224), (1, 512, 512, 21, 16384, 16384)]:
        assert _env(pkg, *a) == pkg.OK, a


def test_envelope_limits(pkg):
    U = pkg.EUNSUPPORTED
    # the ratio: exactly 4 and one below, on each axis
    assert _env(pkg, 1, 5, 7, 21, 20, 28) == pkg.OK
    assert _env(pkg, 1, 5, 7, 21, 19, 28) == U
    assert _env(pkg, 1, 5, 7, 21, 20, 27) == U
    assert _env(pkg, 1, 4096, 1, 2, 16384, 4) == pkg.OK
    assert _env(pkg, 1, 4097, 1, 2, 16384, 4) == U
    # the output side: 16384 / 16385
    assert _env(pkg, 1, 1, 1, 21, 16384, 16384) == pkg.OK
    assert _env(pkg, 1, 1, 1, 21, 16385, 4) == U
    assert _env(pkg, 1, 1, 1, 21, 4, 16385) == U
    # an image's logits below 2^31 bytes: rows * cols * classes < 2^29 floats; the batch does not count (a 64-bit base)
    assert _env(pkg, 1, 1, 1, 2 ** 29 - 1, 4, 4) == pkg.OK
    assert _env(pkg, 1, 1, 1, 2 ** 29, 4, 4) == U
    assert _env(pkg, 5, 64, 64, 2 ** 17 - 1, 256, 256) == pkg.OK
    assert _env(pkg, 5, 64, 64, 2 ** 17, 256, 256) == U
    # an image's output map below 2^31 bytes: the largest map the side limit allows, 16384^2 pixels = 2^30 bytes, is inside; beyond it
    # the side limit refuses first, so this limit has no reachable far side
    assert _env(pkg, 2, 1, 1, 1, 16384, 16384) == pkg.OK
    # the grid: the batch is grid.y
    assert _env(pkg, 65535, 2, 2, 21, 11, 9) == pkg.OK
    assert _env(pkg, 65536, 2, 2, 21, 11, 9) == U


def test_envelope_bad_arguments(pkg):
    for a in [(0, 4, 4, 21, 16, 16), (1, 0, 4, 21, 16, 16), (1, 4, 0, 21, 16, 16), (1, 4, 4, 0, 16, 16), (1, 4, 4, 21, 0, 16), (1, 4, 4, 21, 16, 0),
              (-1, 4, 4, 21, 16, 16), (1, 4, 4, 21, -16, 16)]:
        assert _env(pkg, *a) == pkg.EINVAL, a


def test_launch_plan(pkg):
    """LDS sized to the launch's footprint: 6 x 6 vectors at ratio 8 (chunk 128, 19 KB: eight workgroups a CU), 10 x 10 only at ratio 4 (chunk 64, 27 KB)."""
    l = pkg.resample_plan(28, 28, 224, 224)
    assert (l.fy, l.fx, l.ch, l.lds_bytes, l.tiles, l.span) == (6, 6, 128, 36 * 132 * 4, 49, 224 * 224)
    l = pkg.resample_plan(5, 7, 20, 28)
    assert (l.fy, l.fx, l.ch, l.lds_bytes, l.tiles) == (5, 7, 128, 35 * 132 * 4, 1)
    l = pkg.resample_plan(14, 20, 56, 80)
    assert (l.fy, l.fx, l.ch, l.lds_bytes, l.tiles) == (10, 10, 64, 100 * 68 * 4, 6)
    l = pkg.resample_plan(14, 14, 375, 500)
    assert (l.fy, l.fx, l.ch, l.tiles) == (4, 3, 128, 12 * 16)
    l = pkg.resample_plan(1, 1, 70, 45)
    assert (l.fy, l.fx, l.tiles) == (1, 1, 6)
    assert l.lds_bytes <= 64 * 1024


def test_ragged_check(pkg):
    ok = [(0, 37, 61), (5000, 40, 56), (2257 + 10, 20, 28)]
    rc, l = pkg.resample_ragged_check(5, 7, 21, ok)
    assert rc == pkg.OK and l.span == 5000 + 40 * 56 and l.tiles == 4 and (l.fy, l.fx) == (5, 7)
    assert pkg.resample_ragged_check(5, 7, 21, [(0, 37, 61), (2257, 20, 28)])[0] == pkg.OK               # touching is not overlapping
    assert pkg.resample_ragged_check(5, 7, 21, [(2256, 20, 28), (0, 37, 61)])[0] == pkg.EINVAL           # one element shared, any order
    assert pkg.resample_ragged_check(5, 7, 21, [(0, 37, 61), (0, 37, 61)])[0] == pkg.EINVAL
    assert pkg.resample_ragged_check(5, 7, 21, [(-1, 37, 61)])[0] == pkg.EINVAL
    assert pkg.resample_ragged_check(5, 7, 21, [(0, 37, 61), (5000, 0, 61)])[0] == pkg.EINVAL
    assert pkg.resample_ragged_check(5, 7, 21, [(0, 37, 61), (5000, 19, 28)])[0] == pkg.EUNSUPPORTED     # under ratio 4
    assert pkg.resample_ragged_check(5, 7, 21, [(0, 37, 61), (5000, 20, 16385)])[0] == pkg.EUNSUPPORTED


# ------------------------------------------------------------------------------------------------------------------------ symbols

DEVICE = ("mbn_resample_argmax_f32", "mbn_ragged_readout_create", "mbn_ragged_readout_set", "mbn_resample_argmax_ragged_f32",
          "mbn_ragged_readout_destroy", "mbn_net_segment_to", "mbn_net_segment_images")
PREDICATES = ("mbn_resample_argmax_envelope", "mbn_resample_plan", "mbn_resample_ragged_check")


def test_symbols_where_they_belong(pkg):
    lib, host = pkg.load(), pkg.host_lib()
    for name in DEVICE + PREDICATES:
        assert hasattr(lib, name), name
    for name in PREDICATES:
        assert hasattr(host, name), name
    for name in DEVICE:                                  # device code / the net runner: not in the host library
        assert not hasattr(host, name), name
    assert set(DEVICE) <= set(pkg.declared_symbols())
    for cls, name in ((pkg.Context, "resample_argmax"), (pkg.RaggedReadout, "set"), (pkg.RaggedReadout, "run"), (pkg.Net, "segment_to"),
                      (pkg.Net, "segment_images")):
        assert callable(getattr(cls, name))


def test_label_item_struct_matches_header(pkg, tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "mbn.h"
int main(void){printf("%zu %zu %zu %zu\n", sizeof(mbn_label_item), offsetof(mbn_label_item, dst_offset), offsetof(mbn_label_item, rows),
 offsetof(mbn_label_item, cols));return 0;}'''
    (tmp_path / "t.c").write_text(src)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-I", os.path.join(pkg.REPO_ROOT, "include"), "-o", exe, str(tmp_path / "t.c")])
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    L = pkg.LabelItem
    assert vals == [16, 0, 8, 12] == [C.sizeof(L), L.dst_offset.offset, L.rows.offset, L.cols.offset]
