"""CPU tests of the int8 inference mode's host quantizer (mbn_quantize_i8 through libmbn_host.so): its output equals the numpy
statement of include/mbn.h's arithmetic bit for bit, its blob layout, the plans it refuses, and the ctypes mirror of its structs."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import int8_ref as ref


@pytest.fixture(scope="module")
def weights(pkg):
    """fp32 blobs (BN folded) of synthetic networks at three widths, res 128, 24 classes"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for alpha in (1.0, 0.5, 0.25):
            path = os.path.join(d, "w%g.h5" % alpha)
            pkg.synthetic_h5(path, alpha=alpha, classes=24, seed=11)
            hw = pkg.HostWeights(path, res=128)
            out[alpha] = (hw.plan, hw.blob.copy())
            hw.free()
    return out


def _check_equal(pkg, plan, blob, scales):
    p, b = pkg.quantize_i8(plan, blob, scales)
    want = ref.quantize(plan, blob, scales)
    for i in range(plan.n_layers):
        l, q, r = plan.layer[i], p.layer[i], want[i]
        assert q.in_scale == np.float32(r["in_scale"]) and q.out_scale == np.float32(r["out_scale"]), i
        if l.kind == ref.L_POOL:
            assert (q.w_offset, q.mult_offset, q.bias_offset) == (-1, -1, -1)
            continue
        if l.kind == ref.L_CONV:
            assert q.w_offset == -1
        else:
            got = b[q.w_offset:q.w_offset + l.w_count].view(np.int8)
            assert np.array_equal(got, r["w8"]), "layer %d int8 filter" % (i + 1)
        mult = b[q.mult_offset:q.mult_offset + 4 * l.out_ch].view(np.float32)
        bias = b[q.bias_offset:q.bias_offset + 4 * l.out_ch].view(np.float32)
        assert np.array_equal(mult.view(np.uint32), r["mult"].view(np.uint32)), "layer %d mult" % (i + 1)
        assert np.array_equal(bias.view(np.uint32), r["bias"].view(np.uint32)), "layer %d bias" % (i + 1)
    return p, b


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.25])
def test_quantize_matches_numpy_default_scales(pkg, weights, alpha):
    plan, blob = weights[alpha]
    p, _ = _check_equal(pkg, plan, blob, None)
    assert p.layer[0].out_scale == np.float32(6.0) / np.float32(255.0)
    assert p.layer[plan.n_layers - 1].out_scale == 0.0


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.25])
def test_quantize_matches_numpy_calibrated_scales(pkg, weights, alpha):
    plan, blob = weights[alpha]
    rng = np.random.default_rng(int(alpha * 100))
    scales = (rng.uniform(0.5, 6.0, plan.n_layers) / 255.0).astype(np.float32)
    p, _ = _check_equal(pkg, plan, blob, scales)
    for i in range(1, plan.n_layers - 1):        # each layer reads the scale of the one before it; the pool passes it on
        assert p.layer[i].in_scale == p.layer[i - 1].out_scale


def test_quantize_all_zero_channels(pkg, weights):
    plan, blob = weights[0.5]
    blob = blob.copy()
    d, pwl, fc = plan.layer[3], plan.layer[4], plan.layer[plan.n_layers - 1]
    blob[d.w_offset:d.w_offset + d.w_count].reshape(9, d.out_ch)[:, 5] = 0       # depthwise channel 5
    blob[pwl.w_offset:pwl.w_offset + pwl.w_count].reshape(pwl.out_ch, pwl.in_ch)[7] = 0   # pointwise row 7
    blob[fc.w_offset:fc.w_offset + fc.w_count].reshape(fc.out_ch, fc.in_ch)[3] = 0        # FC row 3
    p, b = _check_equal(pkg, plan, blob, None)
    q = p.layer[4]
    mult = b[q.mult_offset:q.mult_offset + 4 * pwl.out_ch].view(np.float32)
    bn = blob[pwl.scale_offset + 7]
    sd = float(ref.DEFAULT_SCALE)
    assert mult[7] == np.float32(1.0 * sd * float(bn) / sd)          # s_w = 1
    w8 = b[q.w_offset:q.w_offset + pwl.w_count].view(np.int8).reshape(pwl.out_ch, pwl.in_ch)
    assert not w8[7].any() and w8[6].any()


def test_quantizer_rounds_half_to_even(pkg, weights):
    """Rows worked by hand, written into a pointwise filter of the fp32 blob: values that land exactly on .5 after the float32 scaling
    round to even in mbn_quantize_i8 (absmax 127: inv = 1; absmax 254: inv = 0.5), the extremes map to +-127, s_w = absmax / 127."""
    plan, blob = weights[0.5]
    blob = blob.copy()
    l = plan.layer[2]                            # pointwise 16 -> 32
    assert l.kind == ref.L_PW and l.in_ch == 16
    w = blob[l.w_offset:l.w_offset + l.w_count].reshape(l.out_ch, l.in_ch)
    w[0] = [127.0, 0.5, 1.5, 2.5, -2.5, -127.0, 126.5, -0.5, 3.5, -3.5, 0.0, 1.0, -1.0, 100.5, -100.5, 0.25]
    w[1] = [254.0, 1.0, 3.0, 5.0, -5.0, -254.0, 253.0, -1.0, 7.0, -7.0, 0.0, 2.0, -2.0, 201.0, -201.0, 0.4]
    p, b = pkg.quantize_i8(plan, blob)
    q = p.layer[2]
    w8 = b[q.w_offset:q.w_offset + l.w_count].view(np.int8).reshape(l.out_ch, l.in_ch)
    want = [127, 0, 2, 2, -2, -127, 126, 0, 4, -4, 0, 1, -1, 100, -100, 0]
    assert w8[0].tolist() == want and w8[1].tolist() == want
    mult = b[q.mult_offset:q.mult_offset + 4 * l.out_ch].view(np.float32)
    s_in = float(p.layer[1].out_scale)
    for r, absmax in ((0, 127.0), (1, 254.0)):
        bn = float(blob[l.scale_offset + r])
        assert mult[r] == np.float32(absmax / 127.0 * s_in * bn / float(ref.DEFAULT_SCALE))


@pytest.mark.parametrize("alpha", [1.0, 0.5, 0.25])
def test_blob_segments_aligned_disjoint_and_sized(pkg, weights, alpha):
    plan, blob = weights[alpha]
    p, b = pkg.quantize_i8(plan, blob)
    assert p.n_layers == plan.n_layers
    segs = []
    for i in range(plan.n_layers):
        l, q = plan.layer[i], p.layer[i]
        if q.w_offset >= 0:
            segs.append((q.w_offset, l.w_count))
        if q.mult_offset >= 0:
            segs += [(q.mult_offset, 4 * l.out_ch), (q.bias_offset, 4 * l.out_ch)]
    assert all(o % 256 == 0 for o, _ in segs)
    segs.sort()
    for (o0, n0), (o1, _) in zip(segs, segs[1:]):
        assert o0 + n0 <= o1
    last_o, last_n = segs[-1]
    assert p.blob_bytes == (last_o + last_n + 255) // 256 * 256 and len(b) == p.blob_bytes
    # filling the layout only (no blob) gives the same layout
    p2 = pkg.I8Params()
    assert pkg.host_lib().mbn_quantize_i8(C.byref(plan), None, None, C.byref(p2), None) == 0
    assert bytes(p2) == bytes(p)


def test_unsupported_and_invalid_requests(pkg, weights):
    lib = pkg.host_lib()
    p = pkg.I8Params()
    for alpha in (0.3, 0.6):                     # conv1 9 / 19 channels: not a multiple of 8
        plan = pkg.plan_build(alpha, 128, 24)
        assert lib.mbn_quantize_i8(C.byref(plan), None, None, C.byref(p), None) == pkg.EUNSUPPORTED
    plan, blob = weights[0.25]
    for a in (0.25, 0.5, 0.75, 1.0):             # the issue's minimum coverage
        for res in (128, 160, 192, 224):
            pl = pkg.plan_build(a, res, 1000)
            assert lib.mbn_quantize_i8(C.byref(pl), None, None, C.byref(p), None) == 0, (a, res)
    bad = pkg.Plan.from_buffer_copy(plan)
    bad.layer[plan.n_layers - 1].in_ch = 70000   # FC K above 65536: |acc| could pass 2^31
    assert lib.mbn_quantize_i8(C.byref(bad), None, None, C.byref(p), None) == pkg.EUNSUPPORTED
    bad = pkg.Plan.from_buffer_copy(plan)
    bad.layer[2].in_ch = 12                      # pointwise K not a multiple of 8
    assert lib.mbn_quantize_i8(C.byref(bad), None, None, C.byref(p), None) == pkg.EUNSUPPORTED
    bad = pkg.Plan.from_buffer_copy(plan)
    bad.layer[1].stride = 3
    assert lib.mbn_quantize_i8(C.byref(bad), None, None, C.byref(p), None) == pkg.EUNSUPPORTED
    scales = np.full(plan.n_layers, 6 / 255.0, np.float32)
    for v in (0.0, -1.0, np.inf, np.nan):
        s = scales.copy()
        s[5] = v
        assert lib.mbn_quantize_i8(C.byref(plan), None, s.ctypes.data, C.byref(p), None) == pkg.EINVAL
    s = scales.copy()
    s[plan.n_layers - 2] = 0.0                   # pool / FC entries are ignored
    s[plan.n_layers - 1] = -1.0
    assert lib.mbn_quantize_i8(C.byref(plan), None, s.ctypes.data, C.byref(p), None) == 0
    assert lib.mbn_quantize_i8(None, None, None, C.byref(p), None) == pkg.EINVAL
    assert lib.mbn_quantize_i8(C.byref(plan), None, None, None, None) == pkg.EINVAL
    buf = np.zeros(16, np.uint8)
    assert lib.mbn_quantize_i8(C.byref(plan), None, None, C.byref(p), buf.ctypes.data) == pkg.EINVAL   # a blob needs the fp32 source


def test_i8_structs_match_header(pkg):
    """ctypes mirror == C structs: sizeof / offsetof from a C program compiled against include/mbn.h."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "mbn.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(mbn_i8_layer), offsetof(mbn_i8_layer, mult_offset),
 offsetof(mbn_i8_layer, bias_offset), offsetof(mbn_i8_layer, in_scale), offsetof(mbn_i8_layer, out_scale), sizeof(mbn_i8_params),
 offsetof(mbn_i8_params, blob_bytes), offsetof(mbn_i8_params, layer), sizeof(mbn_layer_ext), (int)MBN_DT_I8);return 0;}'''
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(pkg.REPO_ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        vals = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    L, P = pkg.I8Layer, pkg.I8Params
    assert vals == [C.sizeof(L), L.mult_offset.offset, L.bias_offset.offset, L.in_scale.offset, L.out_scale.offset, C.sizeof(P),
                    P.blob_bytes.offset, P.layer.offset, C.sizeof(pkg.LayerExt), pkg.DT_I8]
