"""Non-square inputs on the host (no GPU): mbn_plan_build_hw, mbn_weights_from_h5_hw and the Python mirror's res=(rows, cols).

A rows x cols plan tracks each side on its own through the 29 layers; its blob layout is the square plan's; the square call is the
rows == cols case byte for byte."""
import ctypes as C

import pytest


def _plan_hw(pkg, alpha, rows, cols, classes=1000):
    p = pkg.Plan()
    rc = pkg.host_lib().mbn_plan_build_hw(alpha, rows, cols, classes, C.byref(p))
    return rc, p


def _sizes(plan):
    return [(plan.layer[i].out_rows, plan.layer[i].out_cols) for i in range(plan.n_layers)]


def _offsets(plan):
    return [(plan.layer[i].w_offset, plan.layer[i].w_count, plan.layer[i].scale_offset, plan.layer[i].shift_offset)
            for i in range(plan.n_layers)]


@pytest.mark.parametrize("rows,cols", [(224, 320), (320, 224)])
def test_plan_hw_layers_pads_and_sizes(pkg, rows, cols):
    rc, p = _plan_hw(pkg, 1.0, rows, cols)
    assert rc == pkg.OK
    assert p.n_layers == 29 and p.res == 0
    assert (p.layer[0].in_rows, p.layer[0].in_cols) == (rows, cols)
    # the maps halve at conv1 and at the four stride-2 depthwise layers: 224x320 -> 112x160 -> 56x80 -> 28x40 -> 14x20 -> 7x10
    maps = {(rows >> k, cols >> k) for k in range(1, 6)}
    seen = {(l.out_rows, l.out_cols) for l in p.layer[:27]}
    assert seen == maps
    assert (p.layer[26].out_rows, p.layer[26].out_cols) == (rows // 32, cols // 32)
    pool = p.layer[27]
    assert pool.kind == pkg.L_POOL and (pool.in_rows, pool.in_cols) == (rows // 32, cols // 32)
    for i in range(27):
        l = p.layer[i]
        if i + 1 < 27:
            assert (p.layer[i + 1].in_rows, p.layer[i + 1].in_cols) == (l.out_rows, l.out_cols)
        if l.kind in (pkg.L_CONV, pkg.L_DW):
            want = 0 if l.stride == 2 else 1
            assert (l.pad_top, l.pad_left) == (want, want), i
    assert p.max_act_floats == 112 * 160 * 64 == 1146880
    sq = pkg.plan_build(1.0, 224, 1000)
    assert p.blob_floats == sq.blob_floats
    assert _offsets(p) == _offsets(sq)


@pytest.mark.parametrize("alpha", [0.5, 0.25])
@pytest.mark.parametrize("rows,cols", [(224, 320), (320, 224), (160, 128), (96, 160)])
def test_plan_hw_other_widths_share_the_square_blob(pkg, alpha, rows, cols):
    rc, p = _plan_hw(pkg, alpha, rows, cols)
    assert rc == pkg.OK and p.res == 0
    sq = pkg.plan_build(alpha, 224, 1000)
    assert p.blob_floats == sq.blob_floats and _offsets(p) == _offsets(sq)
    assert (p.layer[26].out_rows, p.layer[26].out_cols) == (rows // 32, cols // 32)
    c1 = int(64 * alpha)
    assert p.max_act_floats == max(rows * cols * 3, (rows // 2) * (cols // 2) * c1)


@pytest.mark.parametrize("alpha,res", [(1.0, 224), (0.5, 160), (0.25, 128), (0.75, 192), (1.0, 32), (1.0, 4096)])
def test_plan_hw_square_is_byte_identical(pkg, alpha, res):
    rc, p = _plan_hw(pkg, alpha, res, res)
    assert rc == pkg.OK
    q = pkg.Plan()
    assert pkg.host_lib().mbn_plan_build(alpha, res, 1000, C.byref(q)) == pkg.OK
    assert bytes(p) == bytes(q)
    assert p.res == res


@pytest.mark.parametrize("rows,cols", [(224, 240), (240, 224), (48, 64), (16, 224), (224, 16), (0, 224), (224, 4128), (4128, 224),
                                       (224, -32), (100, 100)])
def test_plan_hw_refuses_what_the_square_call_refuses(pkg, rows, cols):
    rc, _ = _plan_hw(pkg, 1.0, rows, cols)
    q = pkg.Plan()
    lib = pkg.host_lib()
    want = min((lib.mbn_plan_build(1.0, s, 1000, C.byref(q)) for s in (rows, cols) if s % 32 or s < 32 or s > 4096),
               default=pkg.OK)
    # a side below 32 or above 4096 is EINVAL, a side that is not a multiple of 32 EUNSUPPORTED: the square codes
    bad = [s for s in (rows, cols) if s < 32 or s > 4096]
    assert rc == (pkg.EINVAL if bad else pkg.EUNSUPPORTED)
    assert rc == want


def test_weights_hw_blob_equals_the_square_load(pkg, tmp_path):
    import numpy as np
    path = str(tmp_path / "w.h5")
    pkg.synthetic_h5(path, alpha=0.5, classes=30, seed=11)
    sq = pkg.HostWeights(path, res=224)
    w = pkg.Weights()
    assert pkg.host_lib().mbn_weights_from_h5_hw(path.encode(), 0.0, 224, 320, C.byref(w)) == pkg.OK
    blob = np.ctypeslib.as_array(w.blob, shape=(w.plan.blob_floats,)).copy()
    assert w.plan.res == 0 and (w.plan.layer[0].in_rows, w.plan.layer[0].in_cols) == (224, 320)
    assert blob.shape == sq.blob.shape and np.array_equal(blob.view(np.uint32), sq.blob.view(np.uint32))
    pkg.host_lib().mbn_weights_free(C.byref(w))
    # the Python mirror: res = (rows, cols)
    hw = pkg.HostWeights(path, res=(320, 224))
    assert hw.plan.res == 0 and (hw.plan.layer[0].in_rows, hw.plan.layer[0].in_cols) == (320, 224)
    assert np.array_equal(hw.blob.view(np.uint32), sq.blob.view(np.uint32))
    sq2 = pkg.HostWeights(path, res=(160, 160))
    assert bytes(sq2.plan) == bytes(pkg.HostWeights(path, res=160).plan)
    hw.free()
    sq.free()
    sq2.free()


def test_python_plan_build_accepts_rows_cols(pkg):
    p = pkg.plan_build(1.0, (224, 320), 1000)
    assert p.res == 0 and (p.layer[0].in_rows, p.layer[0].in_cols) == (224, 320)
    assert _sizes(p)[0] == (112, 160)
    assert bytes(pkg.plan_build(0.5, (160, 160), 10)) == bytes(pkg.plan_build(0.5, 160, 10))
    assert pkg.input_hw(224) == (224, 224) and pkg.input_hw((224, 320)) == (224, 320)
    with pytest.raises(pkg.MbnError):
        pkg.plan_build(1.0, (224, 250), 1000)


def test_stem_envelope_hw(pkg):
    host = pkg.host_lib()
    ok, no = pkg.OK, pkg.EUNSUPPORTED
    for c1, c3 in ((32, 64), (16, 32)):
        assert host.mbn_stem_envelope_hw(1, 224, 320, c1, c3) == ok and host.mbn_stem_envelope_hw(3, 480, 640, c1, c3) == ok
        assert host.mbn_stem_envelope_hw(1, 224, 240, c1, c3) == no and host.mbn_stem_envelope_hw(1, 240, 224, c1, c3) == no
        for r in (32, 64, 224):
            assert host.mbn_stem_envelope_hw(2, r, r, c1, c3) == host.mbn_stem_envelope(2, r, c1, c3) == ok
    # 7 x 10 tiles per 224 x 320 image (112 x 160 map in 8 x 16 tiles): the 32-bit tile index bound
    assert host.mbn_stem_envelope_hw(2147483646 // 140, 224, 320, 32, 64) == ok
    assert host.mbn_stem_envelope_hw(2147483647 // 140 + 1, 224, 320, 32, 64) == no
