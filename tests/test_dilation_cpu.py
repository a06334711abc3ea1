"""output_stride 16 / 8 on the host (no GPU): mbn_plan_build_os, the `dilation` fields of the two structs, mbn_weights_from_h5_os, the
int8 quantizer's refusal, and the pin of the reference the GPU tests use (the oracle's depthwise with a zero-inflated filter).

The rule (include/mbn.h): walk the 13 depthwise layers with current = 2, rate = 1; a layer of table stride s runs, when
current == output_stride, with stride 1 and dilation `rate` (then rate *= s), otherwise with stride s undilated (then current *= s)."""
import ctypes as C

import numpy as np
import pytest

DW_LAYERS = range(2, 27, 2)             # 1-based numbers of the 13 depthwise layers
TABLE_STRIDE = {2: 1, 4: 2, 6: 1, 8: 2, 10: 1, 12: 2, 14: 1, 16: 1, 18: 1, 20: 1, 22: 1, 24: 2, 26: 1}


def _os_plan(pkg, alpha, rows, cols, classes, os_):
    p = pkg.Plan()
    rc = pkg.host_lib().mbn_plan_build_os(alpha, rows, cols, classes, os_, C.byref(p))
    return rc, p


def _offsets(plan):
    return [(plan.layer[i].w_offset, plan.layer[i].w_count, plan.layer[i].scale_offset, plan.layer[i].shift_offset)
            for i in range(plan.n_layers)]


def _walk(rows, cols, os_):
    """{layer: (stride, dilation, pad, in, out)} of the depthwise layers by the normative rule, written out independently."""
    h, w = rows // 2, cols // 2
    current, rate, want = 2, 1, {}
    for L in DW_LAYERS:
        s = TABLE_STRIDE[L]
        if current == os_:
            stride, dil = 1, rate
            rate *= s
        else:
            stride, dil = s, 1
            current *= s
        oh, ow = -(-h // stride), -(-w // stride)
        pad = dil if stride == 1 else 0          # SAME: window 2 D + 1 at stride 1; 3 at stride 2 on an even map pads bottom / right only
        want[L] = (stride, dil, pad, (h, w), (oh, ow))
        h, w = oh, ow
    return want, (h, w)


def _check_plan(pkg, p, alpha, rows, cols, os_):
    want, final = _walk(rows, cols, os_)
    for L in DW_LAYERS:
        l = p.layer[L - 1]
        stride, dil, pad, (ih, iw), (oh, ow) = want[L]
        assert l.kind == pkg.L_DW
        assert (l.stride, l.dilation if l.dilation else 1) == (stride, dil), L
        assert l.dilation != 1, "undilated layers carry 0"
        assert (l.pad_top, l.pad_left) == (pad, pad), L
        assert (l.in_rows, l.in_cols, l.out_rows, l.out_cols) == (ih, iw, oh, ow), L
        pw = p.layer[L]
        assert pw.kind == pkg.L_PW and pw.dilation == 0 and (pw.in_rows, pw.in_cols, pw.out_rows, pw.out_cols) == (oh, ow, oh, ow)
    pool = p.layer[27]
    assert pool.kind == pkg.L_POOL and (pool.in_rows, pool.in_cols) == final == (rows // os_, cols // os_)
    assert (pool.out_rows, pool.out_cols) == (1, 1)
    acts = [rows * cols * 3] + [p.layer[i].out_rows * p.layer[i].out_cols * p.layer[i].out_ch for i in range(p.n_layers)]
    assert p.max_act_floats == max(acts)


@pytest.mark.parametrize("os_", [32, 16, 8])
def test_plan_os_table_1_0_x_224(pkg, os_):
    p = pkg.plan_build(1.0, 224, 1000, output_stride=os_)
    _check_plan(pkg, p, 1.0, 224, 224, os_)
    L = p.layer
    by = {i: (L[i - 1].stride, L[i - 1].dilation) for i in DW_LAYERS}
    if os_ == 32:
        assert all(d == 0 for _, d in by.values()) and [i for i in DW_LAYERS if by[i][0] == 2] == [4, 8, 12, 24]
        assert (L[26].out_rows, L[26].out_cols) == (7, 7)
    elif os_ == 16:
        assert by[12] == (2, 0) and by[24] == (1, 0) and by[26] == (1, 2)
        assert [i for i in DW_LAYERS if by[i][1]] == [26]
        assert (L[23].pad_top, L[25].pad_top, L[25].pad_left) == (1, 2, 2)
        assert (L[26].out_rows, L[26].out_cols) == (14, 14)
    else:
        assert by[12] == (1, 0) and by[24] == (1, 2) and by[26] == (1, 4)
        assert [i for i in DW_LAYERS if by[i][1] == 2] == [14, 16, 18, 20, 22, 24] and [i for i in DW_LAYERS if by[i][1] == 4] == [26]
        assert (L[11].pad_top, L[13].pad_top, L[23].pad_left, L[25].pad_top) == (1, 2, 2, 4)
        assert all((L[i].out_rows, L[i].out_cols) == (28, 28) for i in range(11, 27))
        assert p.max_act_floats == 112 * 112 * 64


@pytest.mark.parametrize("os_", [32, 16, 8])
def test_plan_os_non_square_half_width(pkg, os_):
    rc, p = _os_plan(pkg, 0.5, 96, 160, 10, os_)
    assert rc == pkg.OK and p.res == 0
    _check_plan(pkg, p, 0.5, 96, 160, os_)
    assert bytes(p) == bytes(pkg.plan_build(0.5, (96, 160), 10, output_stride=os_))


@pytest.mark.parametrize("alpha,rows,cols", [(1.0, 224, 224), (0.5, 96, 160), (0.25, 64, 64)])
def test_plan_os_32_is_plan_build_hw_byte_for_byte(pkg, alpha, rows, cols):
    hw = pkg.Plan()
    assert pkg.host_lib().mbn_plan_build_hw(alpha, rows, cols, 1000, C.byref(hw)) == pkg.OK
    for os_ in (32, 0):
        rc, p = _os_plan(pkg, alpha, rows, cols, 1000, os_)
        assert rc == pkg.OK
        assert C.string_at(C.addressof(p), C.sizeof(p)) == C.string_at(C.addressof(hw), C.sizeof(hw))
    q = pkg.plan_build(alpha, (rows, cols), 1000, output_stride=32)
    assert C.string_at(C.addressof(q), C.sizeof(q)) == C.string_at(C.addressof(hw), C.sizeof(hw))
    assert all(hw.layer[i].dilation == 0 for i in range(pkg.MAX_LAYERS))


@pytest.mark.parametrize("os_", [16, 8])
@pytest.mark.parametrize("alpha,rows,cols", [(1.0, 224, 224), (0.5, 96, 160)])
def test_plan_os_shares_the_blob_layout(pkg, alpha, rows, cols, os_):
    base = pkg.plan_build(alpha, (rows, cols), 1000)
    p = pkg.plan_build(alpha, (rows, cols), 1000, output_stride=os_)
    assert p.blob_floats == base.blob_floats and _offsets(p) == _offsets(base)
    assert [(p.layer[i].kind, p.layer[i].in_ch, p.layer[i].out_ch) for i in range(29)] == \
           [(base.layer[i].kind, base.layer[i].in_ch, base.layer[i].out_ch) for i in range(29)]


@pytest.mark.parametrize("os_", [4, 64, 1, 24, -8])
def test_plan_os_refuses_other_strides(pkg, os_):
    rc, _ = _os_plan(pkg, 1.0, 224, 224, 1000, os_)
    assert rc == pkg.EINVAL
    with pytest.raises(pkg.MbnError):
        pkg.plan_build(1.0, 224, 1000, output_stride=os_)


def test_struct_layout_keeps_every_offset(pkg):
    D, E = pkg.LayerDesc, pkg.LayerExt
    assert C.sizeof(D) == 80 and D.w_offset.offset == 48 and D.dilation.offset == 44 and D.pad_left.offset == 40
    assert E.dilation.offset == E.io_flags.offset + 4 and C.sizeof(E) == E.dilation.offset + 4
    assert pkg.make_ext(dilation=2).dilation == 2 and pkg.make_ext().dilation == 0


def test_weights_os_blob_equals_the_stride_32_load(pkg, tmp_path):
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=0.5, classes=30, seed=11)
    base = pkg.HostWeights(path, res=(96, 160))
    for os_ in (8, 16, 32):
        hw = pkg.HostWeights(path, res=(96, 160), output_stride=os_)
        assert np.array_equal(hw.blob.view(np.uint32), base.blob.view(np.uint32))
        assert bytes(hw.plan) == bytes(pkg.plan_build(0.5, (96, 160), 30, output_stride=os_))
        hw.free()
    w = pkg.Weights()
    assert pkg.host_lib().mbn_weights_from_h5_os(path.encode(), 0.0, 96, 160, 4, C.byref(w)) == pkg.EINVAL
    base.free()


def test_quantize_i8_refuses_a_dilated_plan(pkg):
    host = pkg.host_lib()
    q = pkg.I8Params()
    for os_, want in ((32, pkg.OK), (16, pkg.EUNSUPPORTED), (8, pkg.EUNSUPPORTED)):
        p = pkg.plan_build(1.0, 224, 1000, output_stride=os_)
        assert host.mbn_quantize_i8(C.byref(p), None, None, C.byref(q), None) == want


def inflate(w, d):
    """3x3xC filter -> (2d+1) x (2d+1) x C with the taps d apart and zeros between: the dilated filter as an ordinary one."""
    k = 2 * d + 1
    out = np.zeros((k, k, w.shape[2]), np.float32)
    out[::d, ::d, :] = w
    return out


@pytest.mark.parametrize("d", [2, 4])
def test_reference_pinned_inflated_filter_is_torch_dilation(orc, d):
    """The GPU tests' reference: the oracle's f32_depthwise with the zero-inflated filter and pad = D against torch's dilated grouped
    convolution in float64. fp32 sums of 9 products of values in [-1, 1]: 9 * 2^-24 * 9 < 1e-5 absolute."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(d)
    n, h, w, c = 2, 9, 7, 8
    x = rng.uniform(-1, 1, (n, h, w, c)).astype(np.float32)
    f = rng.uniform(-1, 1, (3, 3, c)).astype(np.float32)
    got = orc.f32_depthwise(x, inflate(f, d), None, None, 1, orc.ACT_NONE, out_rows=h, out_cols=w, pad_top=d, pad_left=d)
    xt = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(f.astype(np.float64)).permute(2, 0, 1).unsqueeze(1)
    want = torch.nn.functional.conv2d(xt, wt, padding=d, dilation=d, groups=c).permute(0, 2, 3, 1).numpy()
    assert got.shape == want.shape == (n, h, w, c)
    assert np.abs(got.astype(np.float64) - want).max() < 1e-5
