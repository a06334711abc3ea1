"""The epilogue of every stand-alone layer kernel, bit for bit: out = act(acc * (scale ? scale[c] : 1) + (shift ? shift[c] : 0)) with act none, ReLU
or ReLU6 and scale / shift each given or NULL: 12 combinations per kernel.

The data are those of tests/test_exact_gpu.py (exact_ref.py: every product, sum and fma exact in fp32 in any order), so a result is right or
wrong, without a tolerance. In every case at least 10 % of the values before the activation lie below 0, 20 % inside (0, 6) and 2 % above 6
(exact_ref.Z_SHARES; tests/test_exact_cpu.py passes every case of the lists below through that gate): a ReLU that clamps at 6, an activation
that is skipped or applied where none was asked, a parameter dropped or applied where NULL was passed, or a launcher that lets a ReLU6-only
kernel take another combination shows as a failed array_equal. With scale NULL the activations are shrunk by a power of two (make_layer).

One test per route (kernel and shape). It uploads the filter once, the activations twice (as they are, and shrunk for the scale-NULL forms),
each parameter vector once, and runs the 12 calls into one output with a 0xFF canary behind it, refilled before every call. All combinations
are run before the test fails, so its message names every combination that is wrong. Lab knobs skip on the shipped library.
"""
import ctypes

import numpy as np
import pytest

import exact_ref as E
from test_exact_gpu import Dev, Knobs, same_bits, want_bits, pw_route_eligible, _cus, ptr

pytestmark = pytest.mark.gpu

# ----------------------------------------------------------------------------- the routes (test_exact_cpu.py gates all 12 cases of each)

PW_SHAPE = (200, 128, 128)          # 64 x 64 tiles: three interior row tiles and a ragged one (8 rows), two column tiles
# fp32 pointwise (knobs, shape). A call of M = 200, K = 128 is inside split-K's few-tile regime, so pw_gemm needs pw_splitk = 1 (off); split-K forced
# (2: its own tile rule gives 16 x 16 here; 32: the 32 x 32 tile); pw_emul on each of its tiles; pw_tile = 9 forces the resident-filter GEMM (ReLU6 with
# both parameters only: the other 11 combinations must fall through to pw_gemm). (127, 36, 100): ragged N and K; (64, 6, 10): K % 4 != 0, pw_generic.
F32_PW_ROUTES = [({"pw_splitk": 1}, PW_SHAPE), ({}, (127, 36, 100)), ({}, (64, 6, 10)), ({"pw_splitk": 2}, PW_SHAPE), ({"pw_splitk": 32}, PW_SHAPE),
                 ({"pw_tile": 9, "pw_splitk": 1}, PW_SHAPE)] + [({"pw_emul": 6, "pw_splitk": 1, "pw_tile": t}, PW_SHAPE) for t in (11, 6, 7)]
# bf16 pointwise (shape, fp32 out). (130, 8, 24): pw_gemm<bf16, 64, 64> (N < 128), one column block per wave: not paired; (397, 256, 256) and (549, 64, 128):
# inside the streaming kernels' envelopes (16x16x32 form from K = 256, 32x32x16 form for M >= 512), which take ReLU6 with both parameters only:
# everything else falls to pw_gemm<bf16, 64, 128>'s channel-paired element path; (64, 6, 10): pw_generic<bf16>; (77, 72, 40) with MBN_IO_OUT_F32.
BF16_PW_ROUTES = [((130, 8, 24), False), ((397, 256, 256), False), ((549, 64, 128), False), ((64, 6, 10), False), ((77, 72, 40), True)]
# depthwise (batch, side, channels, stride, geometry), each in fp32 and bf16. fp32: the 4-channel column march at both strides, 12 channels (a slab of
# three lanes), the generic kernel (6 channels), the dilated march. bf16: the 8-channel march (8 and 64 channels), the 4-channel march (12 channels:
# C % 8 != 0), the generic kernel, the dilated march.
DW_ROUTES = [(2, 9, 8, 1, {}), (2, 14, 64, 2, {}), (2, 9, 12, 1, {}), (1, 10, 6, 1, {}), (2, 14, 64, 1, dict(dilation=2)), (2, 14, 64, 1, dict(dilation=4))]
DW_LDS_LAB = (1, 40, 32, 1, {})     # exp0 = 6: dw3x3_lds (fp32), by default only from 512 MB up
# conv1 3x3x3 stride 2 (batch, side, Cout), each in fp32 and in bf16 with MBN_IO_IN_F32. (2, 32, 32): conv1_mfma_f32 takes fp32 ReLU6 with both
# parameters, conv3x3s2c3_f32_nhwc everything else; (1, 33, 8): cols % 4 != 0, conv_f32_nhwc; (1, 32, 6): Cout % 4 != 0, conv_generic_f32_nhwc.
CONV_ROUTES = [(2, 32, 32), (1, 33, 8), (1, 32, 6)]


# Seeds other than 0: the cases whose seed-0 data miss a condition of the gate in one of the 12 combinations (a handful of channels with shift NULL
# sit where their filter sums put them; under ReLU6 a case with few elements inside (0, 6) has too few that a bf16 rounding changes). The conditions
# are exact_ref.check_gate's and stay; the seed is the first that meets them all, in fp32 and in bf16.
PW_SEED = {(130, 8, 24): 5}
DW_SEED = {(2, 9, 8, 1): 1, (2, 14, 64, 2): 1, (1, 10, 6, 1): 2, (1, 40, 32, 1): 1}
# Depthwise: the target spread of z is 1.5, not the generators' 2. An activation map is >= 0 with a mean near 2.7, so a channel is offset by its filter
# sum by more than its own spread; z reaches 6 through the offsets, and a wider spread only empties (0, 6), where the bf16 rounding is checked.
DW_TARGET = 1.5


def pw_matrix(shape, rounded):
    """{(act, params): layer} of one pointwise shape"""
    return {(a, p): E.pw_case(*shape, act=a, rounded=rounded, params=p, seed=PW_SEED.get(shape, 0))[0] for a, p in E.COMBOS}


def dw_matrix(case, rounded):
    n, h, c, stride, geom = case
    seed = DW_SEED.get((n, h, c, stride), 0) if not geom else 0
    return {(a, p): E.dw_case(n, h, c, stride, rounded=rounded, act=a, params=p, seed=seed, target=DW_TARGET, **geom)[0] for a, p in E.COMBOS}


def conv_matrix(case, rounded):
    n, h, cout = case
    return {(a, p): E.conv1_case(n, h, h, cout, act=a, params=p, rounded=rounded)[0] for a, p in E.COMBOS}


def shared_operands(layers):
    """What lets one upload serve a matrix: one filter; one input for the forms with a scale and the same input times a power of two for the
    forms without; one scale, one shift per form. Returns the power of two."""
    ref = layers[(E.ACT_RELU6, "both")]
    down = None
    for (a, p), l in layers.items():
        same = layers[(E.ACT_RELU6, p)]
        assert l.act == a and np.array_equal(l.w, ref.w) and np.array_equal(l.x, same.x)
        assert (l.scale is None) == (p in ("shift", "none")) and (l.shift is None) == (p in ("scale", "none"))
        assert l.scale is None or np.array_equal(l.scale, same.scale)
        assert l.shift is None or np.array_equal(l.shift, same.shift)
        if l.scale is None:
            k = l.x.ravel()[np.flatnonzero(ref.x)[0]] / ref.x.ravel()[np.flatnonzero(ref.x)[0]]
            assert np.array_equal(l.x, ref.x * k) and np.log2(k) == np.round(np.log2(k)) and down in (None, k)
            down = k
        else:
            assert np.array_equal(l.x, ref.x)
    return down


# ----------------------------------------------------------------------------- one matrix on one set of buffers

def _run_matrix(pkg, ctx, layers, call, in_bf16, what, knobs=None):
    """call(out, x, w, layer, scale, shift): one layer call on device pointers (scale / shift None: NULL). Compares all 12 results."""
    ref = layers[(E.ACT_RELU6, "both")]
    out_f32 = not ref.rounded
    count = ref.y.size
    failed = []
    with Dev(pkg, ctx) as dev, Knobs(ctx, knobs or {}):
        up = dev.bf16 if in_bf16 else dev.f32
        d_w = dev.bf16(ref.w) if (ref.kind == "pw" and in_bf16) else dev.f32(ref.w)
        d_o = dev.out(count, 4 if out_f32 else 2)
        d_x, d_par = {}, {}
        for (act, params), l in layers.items():
            shrunk = l.scale is None
            if shrunk not in d_x:
                d_x[shrunk] = up(l.x)
            if params not in d_par:
                d_par[params] = (dev.opt_f32(l.scale), dev.opt_f32(l.shift))
            d_sc, d_sh = d_par[params]
            assert ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, count * (4 if out_f32 else 2) + 64) == 0
            call(d_o.ptr, d_x[shrunk].ptr, d_w.ptr, l, ptr(d_sc), ptr(d_sh))
            try:
                same_bits(dev.fetch(d_o, count, np.uint32 if out_f32 else np.uint16), want_bits(pkg, l), "%s act %d %s" % (what, act, params))
            except AssertionError as e:
                failed.append("act %d params %s: %s" % (act, params, e))
    assert not failed, "%s %s: %d of %d combinations wrong:\n  %s" % (what, knobs or "", len(failed), len(layers), "\n  ".join(failed))


def _run_pw_matrix(pkg, ctx, shape, bf, out_f32=False, knobs=None):
    m, k, n = shape
    layers = pw_matrix(shape, rounded=bf and not out_f32)

    def call(out, x, w, l, sc, sh):
        ext = pkg.make_ext(dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=l.act, scale=sc, shift=sh, io_flags=pkg.IO_OUT_F32 if (bf and out_f32) else 0)
        ctx.pointwise(out, x, w, m, 1, k, n, ext)

    _run_matrix(pkg, ctx, layers, call, bf, "%s pointwise %s%s" % ("bf16" if bf else "fp32", shape, " fp32 out" if out_f32 else ""), knobs)


def _knob_id(knobs):
    return "-".join("%s%d" % kv for kv in sorted(knobs.items())) or "default"


@pytest.mark.parametrize("route", F32_PW_ROUTES, ids=lambda r: "%s-%s" % (_knob_id(r[0]), "x".join(map(str, r[1]))))
def test_f32_pointwise_epilogue(pkg, ctx, route):
    """mbn_pointwise in fp32: pw_gemm<float, 64, 64>'s general epilogue on interior and ragged tiles (its fast epilogue takes the interior tiles of the
    default combination only), pw_generic<float>, split-K at both tiles, the three pw_emul tiles, and the resident-filter GEMM's launcher, which must
    decline 11 of the 12."""
    knobs, shape = route
    assert pw_route_eligible({"pw_splitk": 2} if knobs.get("pw_splitk", 0) > 1 else knobs, shape, _cus(ctx)), route
    _run_pw_matrix(pkg, ctx, shape, False, knobs=knobs)


@pytest.mark.parametrize("route", BF16_PW_ROUTES, ids=lambda r: "%s%s" % ("x".join(map(str, r[0])), "-f32out" if r[1] else ""))
def test_bf16_pointwise_epilogue(pkg, ctx, route):
    """mbn_pointwise in bf16: pw_gemm<bf16>'s plain and channel-paired element paths, pw_generic<bf16>, the fp32 output of MBN_IO_OUT_F32 (nothing
    rounded), and the streaming kernels' launcher, which takes the default combination of the two shapes inside its envelope and must decline the
    other 11."""
    shape, out_f32 = route
    _run_pw_matrix(pkg, ctx, shape, True, out_f32)


def _run_dw_matrix(pkg, ctx, case, bf, knobs=None):
    n, h, c, stride, geom = case
    layers = dw_matrix(case, rounded=bf)
    oh, ow = layers[(E.ACT_RELU6, "both")].acc.shape[1:3]

    def call(out, x, w, l, sc, sh):
        ext = pkg.make_ext(batch=n, dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=l.act, in_rows=h, in_cols=h, scale=sc, shift=sh,
                           pad_top=geom.get("pad_top", -1), pad_left=geom.get("pad_left", -1), dilation=geom.get("dilation", 0))
        ctx.depthwise(out, x, w, oh, ow, 3, stride, c, ext)

    _run_matrix(pkg, ctx, layers, call, bf, "%s depthwise %s" % ("bf16" if bf else "fp32", case), knobs)


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", DW_ROUTES, ids=lambda c: "%dx%dx%d-s%d%s" % (c[0], c[1], c[2], c[3], "".join("-%s%d" % kv for kv in sorted(c[4].items()))))
def test_depthwise_epilogue(pkg, ctx, case, bf):
    """mbn_depthwise: act4 behind the 4-channel column march (fp32 and bf16), the 8-channel bf16 march and the dilated march, and dw_generic_nhwc's own epilogue."""
    _run_dw_matrix(pkg, ctx, case, bf)


def test_f32_depthwise_lds_staged_epilogue(pkg, ctx):
    """LAB (exp0 = 6): dw3x3_lds, which the default dispatch reaches only from 512 MB up; the same act4 call."""
    _run_dw_matrix(pkg, ctx, DW_LDS_LAB, False, {"exp0": 6})


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16-f32in"])
@pytest.mark.parametrize("case", CONV_ROUTES, ids=lambda c: "%dx%dx%d" % c)
def test_conv1_epilogue(pkg, ctx, case, bf):
    """mbn_convolute 3x3x3 stride 2: conv3x3s2c3_f32_nhwc (and the MFMA form's launcher, which takes only fp32 ReLU6 with both parameters), conv_f32_nhwc and
    conv_generic_f32_nhwc, with fp32 and with bf16 outputs."""
    n, h, cout = case
    layers = conv_matrix(case, rounded=bf)

    def call(out, x, w, l, sc, sh):
        ext = pkg.make_ext(batch=n, dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=l.act, cin=3, scale=sc, shift=sh, io_flags=pkg.IO_IN_F32 if bf else 0)
        ctx.convolute(out, x, None, None, w, h, h, 3, 2, cout, ext)

    _run_matrix(pkg, ctx, layers, call, False, "%s conv1 %s" % ("bf16" if bf else "fp32", case))


@pytest.mark.parametrize("act", [-1, 3])
def test_act_out_of_range_is_einval(pkg, ctx, act):
    """ext->act outside {0, 1, 2}: MBN_EINVAL from each of the three layer calls, nothing launched."""
    with Dev(pkg, ctx) as dev:
        d_x, d_w, d_p, d_o = dev.f32(np.zeros(8 * 8 * 4)), dev.f32(np.zeros(9 * 4 * 4)), dev.f32(np.zeros(4)), dev.out(8 * 8 * 4, 4)
        lib, ref = ctx.lib, ctypes.byref
        for dtype in (pkg.DT_F32, pkg.DT_BF16):
            ext = pkg.make_ext(dtype=dtype, act=act, in_rows=8, in_cols=8, cin=3, scale=d_p.ptr, shift=d_p.ptr, io_flags=pkg.IO_IN_F32 if dtype == pkg.DT_BF16 else 0)
            assert lib.mbn_pointwise(ctx.h, d_o.ptr, d_x.ptr, d_w.ptr, 8, 8, 4, 4, ref(ext)) == pkg.EINVAL
            assert lib.mbn_depthwise(ctx.h, d_o.ptr, d_x.ptr, d_w.ptr, 8, 8, 3, 1, 4, ref(ext)) == pkg.EINVAL
            assert lib.mbn_convolute(ctx.h, d_o.ptr, d_x.ptr, None, None, d_w.ptr, 8, 8, 3, 2, 4, ref(ext)) == pkg.EINVAL
        dev.fetch(d_o, 8 * 8 * 4, np.uint32)            # (the canary; the output itself is still 0xFF)
        assert np.all(d_o.download((8 * 8 * 4 * 4,), np.uint8) == 0xFF)
