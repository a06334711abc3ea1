"""GPU parity: the HIP path, called through the C-ABI (libmbn.so), against the CPU oracle on the same seeded
inputs. LITERAL mode (uint8/int32, kernel.cl semantics): bit-exact. F32 mode: tolerances from SURVEY.md §8c,
written next to each test.

Run with `pytest -m gpu` on the MI355X box. No test here reads /root/reference.
"""
import ctypes as C
import os
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# fp32 tolerances: max |got - want| <= RTOL * max|want| + ATOL, per tensor.
TOL_DW = 1e-5      # 9-term sums (conv1: 27, pool: 49)
TOL_PW = 1e-4      # K <= 1024, MFMA summation order != serial order
TOL_NET = 1e-3     # end-to-end logits


def assert_close(got, want, rtol, what=""):
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), what
    scale = max(float(np.abs(want).max()), 1e-6)
    err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    assert err <= rtol * scale + 1e-7, "%s: max abs err %.3e vs scale %.3e (rel %.3e > %.1e)" % (
        what, err, scale, err / scale, rtol)


# =========================================================================== LITERAL (bit-exact)

QUIRK_SETS = [0x0, 0xF, 0x1, 0x2, 0x4, 0x5, 0xB]


@pytest.mark.parametrize("quirks", QUIRK_SETS)
@pytest.mark.parametrize("shape", [(8, 8, 5, 1), (12, 10, 7, 1), (7, 7, 16, 2), (14, 14, 9, 2), (28, 28, 32, 1)])
def test_literal_depthwise(pkg, orc, ctx, quirks, shape):
    rows, cols, ch, stride = shape
    rng = np.random.default_rng(rows * 1000 + ch + quirks)
    in_rows, in_cols = rows * stride, cols * stride
    x = rng.integers(0, 256, (ch, in_rows, in_cols), dtype=np.uint8)
    f = rng.integers(-3, 4, (ch, 3, 3), dtype=np.int32)
    want = orc.lit_depthwise(x, f, rows, cols, 3, stride, ch, quirks=quirks)
    d_x, d_f = ctx.to_device(x), ctx.to_device(f)
    d_o = ctx.alloc(ch * rows * cols)
    ext = pkg.make_ext(dtype=pkg.DT_U8, quirks=quirks)
    ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, 3, stride, ch, ext)
    ctx.sync()
    got = d_o.download((ch * rows * cols,), np.uint8)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("quirks", [0x0, 0x2, 0x4, 0x6])
@pytest.mark.parametrize("case", [(112, 32, 1, 3), (56, 24, 2, 3), (9, 7, 1, 127), (14, 16, 2, 128), (10, 5, 1, 300)])
def test_literal_3x3_rows_on_dot4_are_bit_exact(pkg, orc, ctx, quirks, case):
    """Round 3: without the carry quirk the filter rows of `depthwise` and `convolute` (kernel.cl:75-86, 16-50) run
    on v_dot4_i32_i8 — one unaligned dword per filter row, x ^ 0x80 as int8 plus 128 * sum(w). Bit for bit against the oracle and
    against the tap-by-tap kernels (tune lit_dot = 1): image borders (tap-by-tap rows), weights at the int8 limits (+-127/-128),
    weights outside int8 (the channel falls back), DW_PLANE0 / LITERAL_INDEX at stride 1 (dot) and 2 (dilated taps: fallback)."""
    rows, ch, stride, wmax = case
    rng = np.random.default_rng(rows * 31 + ch + quirks + wmax)
    in_rows = rows * stride
    x = rng.integers(0, 256, (ch, in_rows, in_rows), dtype=np.uint8)
    f = rng.integers(-wmax - 1 if wmax >= 127 else -wmax, wmax + 1, (ch, 3, 3), dtype=np.int32)
    if wmax == 127:
        f[0] = 127; f[1 % ch] = -128
    want = orc.lit_depthwise(x, f, rows, rows, 3, stride, ch, quirks=quirks)
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(ch * rows * rows)
    ext = pkg.make_ext(dtype=pkg.DT_U8, quirks=quirks)
    outs = []
    try:
        for mode in (0, 1):
            assert ctx.lib.mbn_tune_set(b"lit_dot", mode) == 0
            ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0, ch * rows * rows)
            ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, rows, 3, stride, ch, ext)
            ctx.sync()
            outs.append(d_o.download((ch * rows * rows,), np.uint8))
    finally:
        ctx.lib.mbn_tune_set(b"lit_dot", 0)
    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want)
    # first conv: three planes, stride 2
    oc = min(ch, 12)
    r, g, b = (rng.integers(0, 256, in_rows * in_rows, dtype=np.uint8) for _ in range(3))
    fc = rng.integers(-wmax - 1 if wmax >= 127 else -wmax, wmax + 1, (oc, 3, 3, 3), dtype=np.int32)
    qc = quirks & ~0x2                                           # DW_PLANE0 is a depthwise quirk
    wantc = orc.lit_convolute(r, g, b, fc, in_rows, in_rows, 3, 2, oc, quirks=qc)
    d = [ctx.to_device(a) for a in (r, g, b, fc)]
    d_oc = ctx.alloc(wantc.size)
    try:
        for mode in (0, 1):
            assert ctx.lib.mbn_tune_set(b"lit_dot", mode) == 0
            ctx.convolute(d_oc.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, in_rows, in_rows, 3, 2, oc, pkg.make_ext(dtype=pkg.DT_U8, quirks=qc))
            ctx.sync()
            assert np.array_equal(d_oc.download(wantc.shape, np.uint8), wantc), mode
    finally:
        ctx.lib.mbn_tune_set(b"lit_dot", 0)


def test_literal_depthwise_null_ext_is_kernel_cl(pkg, orc, ctx):
    """ext == NULL => the context default = MBN_QUIRKS_KERNEL_CL (what kernel.cl computes in bounds)."""
    rng = np.random.default_rng(5)
    x = rng.integers(0, 256, (6, 9, 9), dtype=np.uint8)
    f = rng.integers(-2, 3, (6, 3, 3), dtype=np.int32)
    want = orc.lit_depthwise(x, f, 9, 9, 3, 1, 6, quirks=orc.QUIRKS_KERNEL_CL)
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(6 * 81)
    ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, 9, 9, 3, 1, 6, None)
    ctx.sync()
    assert np.array_equal(d_o.download((6 * 81,), np.uint8), want)
    # and the context default can be switched to the intended geometry
    assert ctx.lib.mbn_set_literal_quirks(ctx.h, pkg.QUIRKS_NONE) == 0
    try:
        want0 = orc.lit_depthwise(x, f, 9, 9, 3, 1, 6, quirks=0)
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, 9, 9, 3, 1, 6, None)
        ctx.sync()
        assert np.array_equal(d_o.download((6 * 81,), np.uint8), want0)
    finally:
        ctx.lib.mbn_set_literal_quirks(ctx.h, pkg.QUIRKS_KERNEL_CL)


@pytest.mark.parametrize("quirks", [0x0, 0xF, 0x1, 0x4])
@pytest.mark.parametrize("shape", [(8, 8, 4), (16, 12, 8), (224, 224, 32)])
def test_literal_convolute(pkg, orc, ctx, quirks, shape):
    rows, cols, oc = shape
    rng = np.random.default_rng(rows + oc + quirks)
    r, g, b = (rng.integers(0, 256, rows * cols, dtype=np.uint8) for _ in range(3))
    f = rng.integers(-2, 3, (oc, 3, 3, 3), dtype=np.int32)
    want = orc.lit_convolute(r, g, b, f, rows, cols, 3, 2, oc, quirks=quirks)
    d = [ctx.to_device(a) for a in (r, g, b, f)]
    d_o = ctx.alloc(want.size)
    ext = pkg.make_ext(dtype=pkg.DT_U8, quirks=quirks)
    ctx.convolute(d_o.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, rows, cols, 3, 2, oc, ext)
    ctx.sync()
    assert np.array_equal(d_o.download(want.shape, np.uint8), want)


@pytest.mark.parametrize("quirks", [0x0, 0x1])
@pytest.mark.parametrize("shape", [(4, 4, 3, 5, 3), (14, 14, 32, 64, 32), (7, 7, 64, 48, 1), (1, 1, 128, 100, 128)])
def test_literal_pointwise(pkg, orc, ctx, quirks, shape):
    rows, cols, cin, oc, fs = shape     # fs = the `filtersize` argument = channels actually summed (B3 when 1)
    rng = np.random.default_rng(cin + oc + quirks)
    x = rng.integers(0, 256, (cin, rows, cols), dtype=np.uint8)
    f = rng.integers(-2, 3, (oc, fs), dtype=np.int32)
    want = orc.lit_pointwise(x, f, rows, cols, fs, oc, quirks=quirks)
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(oc * rows * cols)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, fs, oc, pkg.make_ext(dtype=pkg.DT_U8, quirks=quirks))
    ctx.sync()
    assert np.array_equal(d_o.download(want.shape, np.uint8), want)


@pytest.mark.parametrize("quirks", [0x0, 0x1, 0x8, 0x9, 0xF])
@pytest.mark.parametrize("shape", [(7, 7, 7, 1024), (7, 7, 7, 70), (5, 5, 3, 33)])
def test_literal_pool(pkg, orc, ctx, quirks, shape):
    rows, cols, fs, ch = shape
    rng = np.random.default_rng(ch + quirks)
    x = rng.integers(0, 256, (ch, rows, cols), dtype=np.uint8)
    want = orc.lit_pool(x, rows, cols, fs, ch, quirks=quirks)
    d_x, d_o = ctx.to_device(x), ctx.alloc(ch)
    ctx.pool(d_o.ptr, d_x.ptr, rows, cols, fs, ch, pkg.make_ext(dtype=pkg.DT_U8, quirks=quirks))
    ctx.sync()
    assert np.array_equal(d_o.download((ch,), np.uint8), want)


def _kat_cases():
    import json
    return json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_literal.json")))["cases"]


@pytest.mark.parametrize("case", _kat_cases(), ids=lambda c: c["name"])
def test_literal_device_kernels_against_hand_derived_kats(pkg, ctx, case):
    """Round 4: the hand-derived known-answer vectors (tests/golden/kat_literal.json: worked out from the text of kernel.cl:2-132, each with its
    derivation) run straight through the DEVICE LITERAL kernels by the C-ABI — no oracle in between. The oracle and csrc/mbn_literal.hip are two
    writings of one reading of kernel.cl; these 23 cases are the check of the device code that does not share that reading's code."""
    k, q = case["kernel"], case["quirks"]
    rows, cols, fs, oc = case["rows"], case["cols"], case["filtersize"], case["op_size"]
    ext = pkg.make_ext(dtype=pkg.DT_U8, quirks=q)
    want = np.array(case["expected"], np.uint8)
    if k == "depthwise":
        x, f = np.array(case["input"], np.uint8), np.array(case["filter"], np.int32)
        d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(max(want.size, 4))
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, fs, case["stride"], oc, ext)
    elif k == "pointwise":
        x, f = np.array(case["input"], np.uint8), np.array(case["filter"], np.int32)
        d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(max(want.size, 4))
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, fs, oc, ext)
    elif k == "pool":
        x = (np.concatenate([np.full(rows * cols, v, np.uint8) for v in case["input_fill"]]) if "input_fill" in case
             else np.array(case["input"], np.uint8))
        d_x, d_o = ctx.to_device(x), ctx.alloc(max(want.size, 4))
        ctx.pool(d_o.ptr, d_x.ptr, rows, cols, fs, oc, ext)
    else:
        r = np.array(case["input_r"], np.uint8)
        g = np.array(case["input_g"], np.uint8) if "input_g" in case else np.full(rows * cols, case["input_g_fill"], np.uint8)
        b = np.array(case["input_b"], np.uint8) if "input_b" in case else np.full(rows * cols, case["input_b_fill"], np.uint8)
        f = np.array(case["filter"], np.int32) if "filter" in case else np.full(oc * 27, case["filter_fill"], np.int32)
        d = [ctx.to_device(a) for a in (r, g, b, f)]
        d_o = ctx.alloc(max(want.size, 4))
        ctx.convolute(d_o.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, rows, cols, fs, case["stride"], oc, ext)
    ctx.sync()
    assert list(d_o.download((want.size,), np.uint8)) == case["expected"], case["why"]


def test_literal_truncation_and_wrap(pkg, orc, ctx):
    """int -> uchar store truncates mod 256 (kernel.cl:112) and int32 products wrap."""
    x = np.full((1, 2, 2), 200, np.uint8)
    f = np.array([[3], [2 ** 30], [-1]], np.int32)       # 600 -> 88 ; 200*2^30 wraps ; negative -> 0
    want = orc.lit_pointwise(x, f, 2, 2, 1, 3, quirks=0)
    assert want[0] == 600 % 256 and want[8] == 0
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(12)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, 2, 2, 1, 3, pkg.make_ext(dtype=pkg.DT_U8, quirks=0))
    ctx.sync()
    assert np.array_equal(d_o.download((12,), np.uint8), want)


def test_literal_batched(pkg, orc, ctx):
    """ext->batch > 1 in LITERAL mode = the same call per image."""
    rng = np.random.default_rng(11)
    n, ch, rows = 3, 8, 10
    x = rng.integers(0, 256, (n, ch, rows, rows), dtype=np.uint8)
    f = rng.integers(-2, 3, (ch, 3, 3), dtype=np.int32)
    want = np.stack([orc.lit_depthwise(x[i], f, rows, rows, 3, 1, ch, quirks=0xF) for i in range(n)])
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(want.size)
    ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, rows, 3, 1, ch, pkg.make_ext(batch=n, dtype=pkg.DT_U8, quirks=0xF))
    ctx.sync()
    assert np.array_equal(d_o.download(want.shape, np.uint8), want)


def test_literal_racy_ndrange_is_rejected(pkg, ctx):
    """The reference launches 224x224 work-items over a 112x112 output plane (MobileNet.c:291-292): a data race.
    The ABI refuses an emulated NDRange larger than the output plane instead of producing undefined bytes."""
    d = ctx.alloc(1 << 16)
    ext = pkg.make_ext(dtype=pkg.DT_U8, quirks=0xF, gsize=(16, 16))
    rc = ctx.lib.mbn_depthwise(ctx.h, d.ptr, d.ptr, d.ptr, 8, 8, 3, 1, 4, C.byref(ext))
    assert rc == pkg.EINVAL


# =========================================================================== F32 kernels

DW_SHAPES = [  # (batch, in_rows, channels, stride) — every distinct §2.1 depthwise geometry, scaled batch
    (2, 112, 32, 1), (2, 112, 64, 2), (2, 56, 128, 1), (2, 56, 128, 2), (2, 28, 256, 1), (2, 28, 256, 2),
    (3, 14, 512, 1), (3, 14, 512, 2), (3, 7, 1024, 1),
    (1, 9, 8, 1), (2, 11, 12, 2), (1, 5, 4, 2), (1, 3, 16, 1), (1, 20, 24, 1),        # odd sizes / ragged
]


@pytest.mark.parametrize("shape", DW_SHAPES)
@pytest.mark.parametrize("act", [0, 2])
def test_f32_depthwise(pkg, orc, ctx, shape, act):
    n, h, ch, stride = shape
    rng = np.random.default_rng(h * 7 + ch + stride)
    x = rng.uniform(-1, 1, (n, h, h, ch)).astype(np.float32)
    f = rng.normal(0, 0.5, (3, 3, ch)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, ch).astype(np.float32)
    sh = rng.normal(0, 0.1, ch).astype(np.float32)
    want = orc.f32_depthwise(x, f, sc, sh, stride, act)
    oh = want.shape[1]
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    d_o = ctx.alloc(want.nbytes)
    ext = pkg.make_ext(batch=n, act=act, in_rows=h, in_cols=h, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, oh, oh, 3, stride, ch, ext)
    ctx.sync()
    assert_close(d_o.download(want.shape, np.float32), want, TOL_DW, "dw %s" % (shape,))
    for b in (d_x, d_f, d_sc, d_sh, d_o):
        b.free()


@pytest.mark.parametrize("shape", [(160, 112, 32), (161, 56, 128)])
def test_f32_depthwise_streaming_sizes_take_the_lds_staged_kernel(pkg, orc, ctx, shape):
    """Stride-1 depthwise on maps >= 50 pixels wide whose input + output exceed 512 MB (layers 2 and 6 at the headline batch) run on
    dw3x3_lds (input rows through an LDS ring by LDS-DMA): against the oracle on the first and last images, no store past the output, and
    bit for bit equal to the register column march, which a call with the first 8 images alone takes (same fma order; an image's result
    does not depend on the batch)."""
    n, h, ch = shape
    rng = np.random.default_rng(n + h + ch)
    x = rng.uniform(-1, 1, (n, h, h, ch)).astype(np.float32)
    f = rng.normal(0, 0.5, (3, 3, ch)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, ch).astype(np.float32), rng.normal(0, 0.1, ch).astype(np.float32)
    sel = np.r_[0:3, n - 2:n]
    want = orc.f32_depthwise(x[sel], f, sc, sh, 1, 2)
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    d_o, d_p = ctx.alloc(x.nbytes + 64), ctx.alloc(8 * h * h * ch * 4)
    ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, x.nbytes + 64)
    ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, h, h, 3, 1, ch, pkg.make_ext(batch=n, act=2, in_rows=h, in_cols=h, scale=d_sc.ptr, shift=d_sh.ptr))
    ctx.sync()
    raw = d_o.download((x.size + 16,), np.float32)
    assert np.all(raw[x.size:].view(np.uint32) == 0xFFFFFFFF), "stores past the output"
    got = raw[:x.size].reshape(x.shape)
    assert_close(got[sel], want, TOL_DW, "dw streaming size %s" % (shape,))
    ctx.depthwise(d_p.ptr, d_x.ptr, d_f.ptr, h, h, 3, 1, ch, pkg.make_ext(batch=8, act=2, in_rows=h, in_cols=h, scale=d_sc.ptr, shift=d_sh.ptr))
    ctx.sync()
    assert np.array_equal(got[:8], d_p.download((8, h, h, ch), np.float32)), "LDS-staged kernel differs from the column march"
    for b in (d_x, d_f, d_sc, d_sh, d_o, d_p):
        b.free()


@pytest.mark.parametrize("shape", [(2, 112, 32, 1), (2, 112, 64, 2), (3, 56, 128, 1), (2, 56, 128, 2), (2, 28, 256, 1), (5, 14, 512, 1), (3, 14, 512, 2),
                                   (2, 7, 1024, 1), (1, 40, 32, 1), (2, 70, 64, 1), (1, 37, 96, 2), (1, 130, 32, 1), (1, 5, 32, 1), (2, 9, 64, 2)])
@pytest.mark.parametrize("knob", [6, 7, 16, 17])
def test_f32_depthwise_lds_staged_form(pkg, orc, ctx, shape, knob):
    """LAB: dw3x3_lds (north_star's 'LDS-staged 3x3 input halos': input rows of a column strip through a ring of LDS rows filled by
    buffer_load ... lds, nine ds_read_b128 per output pixel) against the oracle and bit for bit against the shipped register column march
    (same fma order); strips (widths above 62 / 31 output pixels), row segments, odd sizes, both strides, no store outside the output.
    knob: 6 = 32-channel slabs (64-pixel ring rows), 7 = 64-channel slabs (32-pixel ring rows; C % 64 != 0 falls back to the shipped
    kernel), + 10 = the long ring (look-ahead 6 / 3 output rows)."""
    _tune_lab(ctx, b"exp0", knob)
    n, h, ch, stride = shape
    rng = np.random.default_rng(h * 5 + ch + stride)
    x = rng.uniform(-1, 1, (n, h, h, ch)).astype(np.float32)
    f = rng.normal(0, 0.5, (3, 3, ch)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, ch).astype(np.float32), rng.normal(0, 0.1, ch).astype(np.float32)
    want = orc.f32_depthwise(x, f, sc, sh, stride, 2)
    oh = want.shape[1]
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    d_o, d_p = ctx.alloc(want.nbytes + 64), ctx.alloc(want.nbytes)
    ext = pkg.make_ext(batch=n, act=2, in_rows=h, in_cols=h, scale=d_sc.ptr, shift=d_sh.ptr)
    for nseg in (0, 1, 3):
        ctx.lib.mbn_tune_set(b"dw_nseg", nseg)
        ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, want.nbytes + 64)
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, oh, oh, 3, stride, ch, ext)
        ctx.sync()
        raw = d_o.download((want.size + 16,), np.float32)
        assert np.all(raw[want.size:].view(np.uint32) == 0xFFFFFFFF), "stores past the output"
        got = raw[:want.size].reshape(want.shape)
        assert_close(got, want, TOL_DW, "dw lds %s nseg %d" % (shape, nseg))
    ctx.lib.mbn_tune_set(b"dw_nseg", 0)
    ctx.lib.mbn_tune_set(b"exp0", 0)
    ctx.depthwise(d_p.ptr, d_x.ptr, d_f.ptr, oh, oh, 3, stride, ch, ext)
    ctx.sync()
    assert np.array_equal(got, d_p.download(want.shape, np.float32)), "LDS-staged form differs from the column march"
    for b in (d_x, d_f, d_sc, d_sh, d_o, d_p):
        b.free()


def test_f32_depthwise_explicit_padding_and_generic_path(pkg, orc, ctx):
    """pad_top/left = 1 with stride 2 (the reference's top/left convention, B6) and a channel count that is
    not a multiple of 4 (generic kernel)."""
    rng = np.random.default_rng(3)
    for ch in (8, 6):
        x = rng.uniform(-1, 1, (2, 12, 12, ch)).astype(np.float32)
        f = rng.normal(0, 0.5, (3, 3, ch)).astype(np.float32)
        want = orc.f32_depthwise(x, f, None, None, 2, 1, pad_top=1, pad_left=1)
        d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(want.nbytes)
        ext = pkg.make_ext(batch=2, act=1, pad_top=1, pad_left=1, in_rows=12, in_cols=12)
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, 6, 6, 3, 2, ch, ext)
        ctx.sync()
        assert_close(d_o.download(want.shape, np.float32), want, TOL_DW, "dw pad ch=%d" % ch)


PW_SHAPES = [  # (M, Cin, Cout): §2.1 pointwise GEMMs at small batch + ragged M / N / K
    (2 * 112 * 112, 32, 64), (2 * 56 * 56, 64, 128), (56 * 56, 128, 128), (2 * 28 * 28, 128, 256),
    (28 * 28, 256, 256), (2 * 14 * 14, 256, 512), (2 * 14 * 14, 512, 512), (3 * 49, 512, 1024),
    (3 * 49, 1024, 1024), (256 * 49, 1024, 1024),
    (5, 1024, 1000), (256, 1024, 1000),                 # FC (batch 5 / 256), Cout not a multiple of 32
    (49, 16, 32), (130, 8, 24), (1, 64, 64), (127, 36, 100), (300, 72, 40), (1000, 24, 8),   # ragged
    (64, 6, 10),                                        # K % 4 != 0 -> generic kernel
]


@pytest.mark.parametrize("shape", PW_SHAPES)
def test_f32_pointwise(pkg, orc, ctx, shape):
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin * 3 + cout)
    x = rng.uniform(-1, 1, (m, cin)).astype(np.float32)
    f = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = rng.normal(0, 0.1, cout).astype(np.float32)
    want = orc.f32_pointwise(x, f, sc, sh, 2)
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    d_o = ctx.alloc(want.nbytes)
    ext = pkg.make_ext(batch=1, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)   # rows*cols = M
    ctx.sync()
    assert_close(d_o.download(want.shape, np.float32), want, TOL_PW, "pw %s" % (shape,))
    for b in (d_x, d_f, d_sc, d_sh, d_o):
        b.free()


PW3_SHAPES = [  # (M, Cin, Cout) inside mbn_f32_pw3.hip's envelope: the short-K layers 5 / 7 / 9 / 11 / 13 at small batch, ragged M, several tiles per wave
    (2 * 56 * 56, 64, 128), (56 * 56 + 7, 128, 128), (2 * 28 * 28, 128, 256), (28 * 28, 256, 256), (2 * 14 * 14, 256, 512), (33, 64, 384),
    (40 * 56 * 56, 64, 128), (70 * 28 * 28, 128, 256), (90 * 14 * 14 + 5, 256, 128),
    (2 * 14 * 14, 512, 512), (3 * 49 + 1, 512, 1024), (130 * 14 * 14, 512, 64), (300 * 14 * 14, 512, 512),      # K = 512: 64-channel slices, 12 waves per workgroup
]


@pytest.mark.parametrize("shape", PW3_SHAPES)
def test_f32_pointwise_short_k_resident_filter(pkg, orc, ctx, shape):
    """Round 6: mbn_f32_pw3.hip (pw_tile = 9 forces it: filter slice resident in LDS, wave-private A staging, no barrier in the loop) against the
    oracle and BIT FOR BIT against pw_gemm (pw_tile = 10 keeps it off; pw_splitk = 1 keeps the few-tile calls on pw_gemm too): the same
    v_mfma_f32_32x32x2_f32 k pairs in the same order and the same epilogue arithmetic (kernel.cl:94-114 in the F32 mode)."""
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin * 5 + cout)
    x = rng.uniform(-1, 1, (m, cin)).astype(np.float32)
    f = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = rng.normal(0, 0.1, cout).astype(np.float32)
    want = orc.f32_pointwise(x, f, sc, sh, 2)
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    d_a, d_b = ctx.alloc(want.nbytes + 256), ctx.alloc(want.nbytes)
    ext = pkg.make_ext(batch=1, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    try:
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 1) == 0
        assert ctx.lib.mbn_tune_set(b"pw_tile", 9) == 0
        ctx.lib.mbn_memset(ctx.h, d_a.ptr, 0xFF, want.nbytes + 256)
        ctx.pointwise(d_a.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
        assert ctx.lib.mbn_tune_set(b"pw_tile", 10) == 0
        ctx.pointwise(d_b.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    finally:
        ctx.lib.mbn_tune_set(b"pw_tile", 0)
        ctx.lib.mbn_tune_set(b"pw_splitk", 0)
    ctx.sync()
    got, ref = d_a.download(want.shape, np.float32), d_b.download(want.shape, np.float32)
    assert_close(got, want, TOL_PW, "pw3 %s vs oracle" % (shape,))
    assert np.array_equal(got, ref), "pw3 differs from pw_gemm by %g" % np.abs(got - ref).max()
    tail = d_a.download((want.size + 64,), np.float32)[want.size:]
    assert np.isnan(tail).all(), "pw3 stored past the output"
    for b in (d_x, d_f, d_sc, d_sh, d_a, d_b):
        b.free()


def test_f32_pointwise_exact_integers(pkg, ctx):
    """Integer-valued operands: every product and partial sum is exact in fp32, so any k-order gives the same
    result — checks the MFMA operand/C-D lane maps bit-exactly with an ASYMMETRIC filter (cdna guide §3)."""
    rng = np.random.default_rng(0)
    m, cin, cout = 200, 96, 160
    x = rng.integers(-8, 9, (m, cin)).astype(np.float32)
    f = rng.integers(-8, 9, (cout, cin)).astype(np.float32)
    f[:, 0] += np.arange(cout)          # asymmetric
    want = x.astype(np.float64) @ f.astype(np.float64).T
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(m * cout * 4)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, pkg.make_ext(act=0))
    ctx.sync()
    got = d_o.download((m, cout), np.float32)
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("shape", [(2, 224, 32), (1, 160, 16), (2, 33, 8), (1, 64, 6), (3, 32, 32), (2, 96, 32), (1, 200, 32)])
def test_f32_conv1(pkg, orc, ctx, shape):
    """First layer (kernel.cl:2-60 in the mode the metric measures). Round 4: 32 output channels with an output width that is a multiple of 16
    (224, 32, 96 here) run conv1_mfma_f32 — v_mfma_f32_16x16x4_f32, the fused stem's arithmetic — every other shape the fmaf-chain kernels
    (200 -> 100 columns: the chain kernel at 32 channels); both within 1e-5 of the oracle's float64 sums."""
    n, h, cout = shape
    rng = np.random.default_rng(h + cout)
    x = rng.uniform(-1, 1, (n, h, h, 3)).astype(np.float32)
    f = rng.normal(0, 0.27, (3, 3, 3, cout)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = rng.normal(0, 0.1, cout).astype(np.float32)
    want = orc.f32_conv(x, f, sc, sh, 2, 2)
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    d_o = ctx.alloc(want.nbytes)
    ext = pkg.make_ext(batch=n, act=2, cin=3, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.convolute(d_o.ptr, d_x.ptr, None, None, d_f.ptr, h, h, 3, 2, cout, ext)
    ctx.sync()
    assert_close(d_o.download(want.shape, np.float32), want, TOL_DW, "conv1 %s" % (shape,))


@pytest.mark.parametrize("shape", [(3, 7, 1024), (2, 5, 512), (1, 7, 30)])
def test_f32_pool(pkg, orc, ctx, shape):
    n, h, ch = shape
    x = np.random.default_rng(ch).uniform(0, 6, (n, h, h, ch)).astype(np.float32)
    want = orc.f32_pool(x)
    d_x, d_o = ctx.to_device(x), ctx.alloc(want.nbytes)
    ctx.pool(d_o.ptr, d_x.ptr, h, h, h, ch, pkg.make_ext(batch=n, act=0))
    ctx.sync()
    assert_close(d_o.download(want.shape, np.float32), want, TOL_DW, "pool")


def test_f32_softmax_and_normalize(pkg, orc, ctx):
    rng = np.random.default_rng(1)
    logits = rng.normal(0, 3, (5, 1000)).astype(np.float32)
    logits[2, 17] = logits[2, 400] = 50.0            # tie -> lowest index wins, like the oracle's strict '>'
    want_p, want_a = orc.f32_softmax(logits)
    d_l, d_p, d_a = ctx.to_device(logits), ctx.alloc(logits.nbytes), ctx.alloc(5 * 4)
    assert ctx.lib.mbn_softmax_f32(ctx.h, d_p.ptr, d_a.ptr, d_l.ptr, 5, 1000, None) == 0
    ctx.sync()
    assert np.array_equal(d_a.download((5,), np.int32), want_a)
    assert_close(d_p.download((5, 1000), np.float32), want_p, 1e-5, "softmax")
    u8 = rng.integers(0, 256, 224 * 224 * 3 + 3, dtype=np.uint8)
    d_u, d_f = ctx.to_device(u8), ctx.alloc(u8.size * 4)
    assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, d_f.ptr, d_u.ptr, u8.size, 1 / 127.5, -1.0, None) == 0
    ctx.sync()
    want = np.float32(u8) * np.float32(1 / 127.5) + np.float32(-1)
    assert_close(d_f.download((u8.size,), np.float32), want, 1e-6, "normalize")


# =========================================================================== F32 <-> LITERAL tie

def test_f32_matches_literal_on_integer_inputs(pkg, orc, ctx):
    """Where the two modes coincide (identity BN, ReLU, top/left pad, values < 256, quirks off), the fp32 NHWC
    kernel reproduces the integer NCHW kernel exactly — ties the fp32 path back to kernel.cl's arithmetic."""
    rng = np.random.default_rng(9)
    ch, h = 8, 10
    x = rng.integers(0, 4, (ch, h, h), dtype=np.uint8)
    f = rng.integers(-1, 3, (ch, 3, 3), dtype=np.int32)
    lit = orc.lit_depthwise(x, f, h, h, 3, 1, ch, quirks=0).reshape(ch, h, h)
    xf = np.ascontiguousarray(x.transpose(1, 2, 0)[None].astype(np.float32))
    ff = np.ascontiguousarray(f.transpose(1, 2, 0).astype(np.float32))
    d_x, d_f, d_o = ctx.to_device(xf), ctx.to_device(ff), ctx.alloc(xf.nbytes)
    ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, h, h, 3, 1, ch, pkg.make_ext(act=1, pad_top=1, pad_left=1, in_rows=h, in_cols=h))
    ctx.sync()
    got = d_o.download((1, h, h, ch), np.float32)[0].transpose(2, 0, 1)
    assert got.max() < 256
    assert np.array_equal(got.astype(np.int64), lit.astype(np.int64))


# =========================================================================== whole network

def _make_net(pkg, ctx, tmp_path, alpha, res, classes, batch, seed=3):
    path = str(tmp_path / ("w_%g_%d.h5" % (alpha, res)))
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed, lib=pkg.load())
    hw = pkg.HostWeights(path, res=res, lib=pkg.load())
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), batch)
    return hw, net


@pytest.mark.parametrize("cfg", [(0.25, 64, 2), (0.5, 96, 1), (0.75, 96, 3), (1.0, 64, 4), (0.75, 64, 6)])
def test_net_per_layer_vs_oracle(pkg, orc, ctx, tmp_path, cfg):
    """BASELINE config 2 in miniature: every layer's output vs the CPU oracle, each GPU layer fed by the GPU's
    own previous layer (so per-layer error is what the tolerance bounds, not accumulated drift). 1..4 images take the
    split-K pointwise kernel on their few-tile layers (alpha 0.75: K = 192, 384, 768; alpha 1: K = 128 ... 1024), 6 images
    the tiled GEMM everywhere."""
    alpha, res, n = cfg
    hw, net = _make_net(pkg, ctx, tmp_path, alpha, res, 50, n)
    imgs = np.random.default_rng(0).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    net.keep_activations(True)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 50 * 4)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    oplan = orc.plan_build(alpha, res, 50)
    want_out, layers = orc.net_forward(oplan, hw.blob, imgs, keep_layers=True)
    for i in range(hw.plan.n_layers - 1):
        got = net.layer_output(i + 1, n)
        assert_close(got, layers[i], TOL_NET, "layer %d" % (i + 1))
    assert_close(d_out.download((n, 50), np.float32), want_out.reshape(n, 50), TOL_NET, "logits")
    net.destroy()


def test_net_full_size_batch1_first_layers(pkg, orc, ctx, tmp_path):
    """BASELINE configs 1-2: 1.0x224, batch 1, layers 1..5 and 1..13 against the oracle."""
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, 1)
    imgs = np.random.default_rng(1).uniform(-1, 1, (1, 224, 224, 3)).astype(np.float32)
    d_in = ctx.to_device(imgs)
    oplan = orc.plan_build(1.0, 224, 1000)
    for last in (5, 13):
        l = hw.plan.layer[last - 1]
        want, _ = orc.net_forward(oplan, hw.blob, imgs, last_layer=last, threads=orc.num_threads())
        d_out = ctx.alloc(want.nbytes)
        net.forward(d_in.ptr, d_out.ptr, 1, last)
        ctx.sync()
        assert_close(d_out.download(want.shape, np.float32), want, TOL_NET, "L1..%d" % last)
        d_out.free()
    net.destroy()


def test_net_full_size_properties(pkg, ctx, tmp_path):
    """1.0x224 at batch 16 (size-independent properties): (a) batch independence — image i's logits do not
    depend on its batch-mates or its slot; (b) determinism; (c) timed == untimed."""
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, 16)
    rng = np.random.default_rng(2)
    imgs = rng.uniform(-1, 1, (16, 224, 224, 3)).astype(np.float32)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(16 * 1000 * 4)
    net.forward(d_in.ptr, d_out.ptr, 16)
    ctx.sync()
    a = d_out.download((16, 1000), np.float32)
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    net.forward(d_in.ptr, d_out.ptr, 16)
    ctx.sync()
    assert np.array_equal(a, d_out.download((16, 1000), np.float32))
    perm = rng.permutation(16)
    d_in.upload(imgs[perm])
    net.forward(d_in.ptr, d_out.ptr, 16)
    ctx.sync()
    assert np.array_equal(a[perm], d_out.download((16, 1000), np.float32))
    d_in.upload(imgs[:7])
    net.forward(d_in.ptr, d_out.ptr, 7)
    ctx.sync()
    b = d_out.download((7, 1000), np.float32)
    assert np.array_equal(b, a[:7])                                # a smaller batch changes tiles, not sums
    d_in.upload(imgs[:3])                                          # 1..4 images: the split-K pointwise kernel, another
    net.forward(d_in.ptr, d_out.ptr, 3)                            # summation order — equal within the fp32 tolerance,
    ctx.sync()                                                     # and bit-equal among themselves
    c3 = d_out.download((3, 1000), np.float32)
    assert_close(c3, a[:3], TOL_NET, "3 images vs the same images in a batch of 16")
    d_in.upload(imgs[1:3])
    net.forward(d_in.ptr, d_out.ptr, 2)
    ctx.sync()
    assert np.array_equal(d_out.download((2, 1000), np.float32), c3[1:3])
    d_in.upload(imgs)
    ms = net.forward_timed(d_in.ptr, d_out.ptr, 16)
    ctx.sync()
    assert len(ms) == 29 and all(m > 0 for m in ms)
    assert np.array_equal(a, d_out.download((16, 1000), np.float32))
    net.destroy()


def test_net_batch_slice_equals_smaller_batch(pkg, ctx, tmp_path):
    """Sharding property used by the multi-GPU path: forward(images[a:b]) == forward(images)[a:b].
    Tile shapes differ between batch sizes (M changes), so pointwise rows may be summed by different
    workgroups — but each row's k-order is fixed by the kernel, so results are bit-identical: among calls of 5 images and
    more (pw_gemm everywhere) and among calls of 1..4 images (the split-K kernel picks its split by K alone)."""
    hw, net = _make_net(pkg, ctx, tmp_path, 0.5, 128, 100, 16)
    imgs = np.random.default_rng(4).uniform(-1, 1, (16, 128, 128, 3)).astype(np.float32)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(16 * 100 * 4)
    net.forward(d_in.ptr, d_out.ptr, 16)
    ctx.sync()
    full = d_out.download((16, 100), np.float32)
    for a, b in ((8, 16), (3, 8), (11, 16)):
        d_in.upload(imgs[a:b])
        net.forward(d_in.ptr, d_out.ptr, b - a)
        ctx.sync()
        assert np.array_equal(full[a:b], d_out.download((b - a, 100), np.float32)), (a, b)
    d_in.upload(imgs[:4])
    net.forward(d_in.ptr, d_out.ptr, 4)
    ctx.sync()
    four = d_out.download((4, 100), np.float32)
    assert_close(four, full[:4], TOL_NET, "1..4-image kernels vs the large-batch ones")
    for a, b in ((0, 1), (1, 3), (3, 4), (0, 3)):
        d_in.upload(imgs[a:b])
        net.forward(d_in.ptr, d_out.ptr, b - a)
        ctx.sync()
        assert np.array_equal(four[a:b], d_out.download((b - a, 100), np.float32)), (a, b)
    net.destroy()


# =========================================================================== the C host binary (./mobilenet)

def test_c_host_binary_literal_and_fp32(pkg, orc, tmp_path):
    """`mobilenet` is the counterpart of the reference's ./out: plain C over the C-ABI. --literal runs the 29 integer
    layers with the reference's loaders (weights_c.txt prefix re-read per layer, raw image bytes incl. PPM header) and
    prints the reference's two kinds of line; check the printed argmax against the oracle run on the same inputs."""
    import re
    import subprocess
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    rng = np.random.default_rng(12)
    wtxt = tmp_path / "weights_c.txt"
    w = rng.integers(-1, 2, 1024 * 1024)
    wtxt.write_text(" ".join("%d.0" % v for v in w))
    img = rng.integers(0, 256, (224, 224, 3), dtype=np.uint8)
    ppm = str(tmp_path / "Cat_Image0.ppm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), img.ctypes.data, 224, 224) == 0
    r = subprocess.run([exe, "--literal", "--weights", str(wtxt), "--image", ppm], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(re.findall(r"Kernel Execution time for Layer \d+: ", r.stdout)) == 28
    assert "Kernel Execution time for Fully Connected Layer" in r.stdout
    m = re.search(r"present at location (\d+) and it's value is ([0-9]+\.[0-9]+)", r.stdout)
    assert m, r.stdout
    # the same pipeline on the oracle: decode_image semantics = raw bytes from offset 0 (header included, B14)
    raw = np.frombuffer(open(ppm, "rb").read()[:224 * 224 * 3], np.uint8).reshape(-1, 3)
    planes = [np.ascontiguousarray(raw[:, k]) for k in range(3)]
    plan = orc.plan_build(1.0, 224, 1000)
    q = orc.QUIRKS_KERNEL_CL
    x = None
    for i in range(plan.n_layers):
        l = plan.layer[i]
        f = np.int32(w[:max(l.w_count, 1)])
        if l.kind == orc.L_CONV:
            x = orc.lit_convolute(*planes, f, 224, 224, 3, 2, l.out_ch, quirks=q)
        elif l.kind == orc.L_DW:
            x = orc.lit_depthwise(x, f, l.out_rows, l.out_cols, 3, l.stride, l.out_ch, quirks=q)
        elif l.kind in (orc.L_PW, orc.L_FC):
            x = orc.lit_pointwise(x, f, l.out_rows, l.out_cols, l.in_ch, l.out_ch, quirks=q)
        else:
            x = orc.lit_pool(x, l.in_rows, l.in_cols, 7, l.out_ch, quirks=q)
    _, loc, mx = orc.softmax_argmax_u8(x)
    assert int(m.group(1)) == loc and abs(float(m.group(2)) - mx) < 1e-5
    # fp32 mode with synthetic weights: runs, prints 29 layer lines and a class in range
    r = subprocess.run([exe, "--synthetic", "5", "--alpha", "0.25", "--res", "96", "--batch", "3"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"present at location (\d+) and it's value is ([0-9]+\.[0-9]+)", r.stdout)
    assert m and 1 <= int(m.group(1)) <= 1000 and 0 < float(m.group(2)) <= 1.0


# =========================================================================== bf16 mode (BASELINE config 5)
# Storage bf16, arithmetic fp32. One bf16 ulp is 2^-8 = 0.39 % relative; the GPU sums in fp32 (MFMA / fmaf order), the
# oracle in double, so a result near a rounding boundary may land on the neighbouring bf16 value.
TOL_BF16 = 1e-2        # per layer, relative to max|ref| (SURVEY §8c allows 2e-2)
TOL_BF16_NET = 2e-2    # bf16 logits after 28 layers of storage rounding, relative to max|ref| (observed 4.6-5.2e-3 at full size; 6e-2 until round 4)


def _bf16_dev(pkg, ctx, x):
    return ctx.to_device(pkg.f32_to_bf16_bits(x))


def _bf16_get(pkg, buf, shape):
    return pkg.bf16_bits_to_f32(buf.download(shape, np.uint16))


@pytest.mark.parametrize("shape", [(2, 112, 32, 1), (2, 56, 128, 2), (3, 14, 512, 1), (2, 7, 1024, 1), (1, 9, 8, 2), (1, 10, 6, 1)])
def test_bf16_depthwise(pkg, orc, ctx, shape):
    n, h, ch, stride = shape
    rng = np.random.default_rng(h + ch)
    x = orc.bf16_round(rng.uniform(-1, 1, (n, h, h, ch)))
    f = rng.normal(0, 0.5, (3, 3, ch)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, ch).astype(np.float32), rng.normal(0, 0.1, ch).astype(np.float32)
    want = orc.bf16_round(orc.f32_depthwise(x, f, sc, sh, stride, 2))
    oh = want.shape[1]
    d_x, d_f, d_sc, d_sh = _bf16_dev(pkg, ctx, x), ctx.to_device(f), ctx.to_device(sc), ctx.to_device(sh)
    d_o = ctx.alloc(want.size * 2)
    ext = pkg.make_ext(batch=n, dtype=pkg.DT_BF16, act=2, in_rows=h, in_cols=h, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, oh, oh, 3, stride, ch, ext)
    ctx.sync()
    assert_close(_bf16_get(pkg, d_o, want.shape), want, TOL_BF16, "bf16 dw %s" % (shape,))


@pytest.mark.parametrize("shape", [(9, 14, 512), (4, 14, 64), (5, 28, 256), (13, 7, 1024), (2, 56, 128), (3, 9, 64), (1, 62, 64), (7, 3, 128)])
def test_bf16_depthwise_lds_staged_form(pkg, orc, ctx, shape):
    """LAB (exp0=8 forces it): dw3x3_lds_bf16 — G images side by side in 64-pixel LDS ring rows filled by LDS-DMA, dw3x3_nhwc_bf16x8's arithmetic from
    ds_read_b128: against the oracle and bit for bit against the register kernel (exp0=1); images per workgroup 1 ... 6, batches that do not
    fill the last group, odd widths (even-rounded pixel slots), row segments, no store outside the output."""
    _tune_lab(ctx, b"exp0", 8)
    n, h, ch = shape
    rng = np.random.default_rng(n + h + ch)
    x = orc.bf16_round(rng.uniform(-1, 1, (n, h, h, ch)))
    f = rng.normal(0, 0.5, (3, 3, ch)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, ch).astype(np.float32), rng.normal(0, 0.1, ch).astype(np.float32)
    want = orc.bf16_round(orc.f32_depthwise(x, f, sc, sh, 1, 2))
    d_x, d_f, d_sc, d_sh = _bf16_dev(pkg, ctx, x), ctx.to_device(f), ctx.to_device(sc), ctx.to_device(sh)
    d_o, d_p = ctx.alloc(want.size * 2 + 64), ctx.alloc(want.size * 2)
    ext = pkg.make_ext(batch=n, dtype=pkg.DT_BF16, act=2, in_rows=h, in_cols=h, scale=d_sc.ptr, shift=d_sh.ptr)
    try:
        for nseg in (0, 1, 2, 3):
            ctx.lib.mbn_tune_set(b"dw_nseg", nseg)
            ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, want.size * 2 + 64)
            ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, h, h, 3, 1, ch, ext)
            ctx.sync()
            raw = d_o.download((want.size + 32,), np.uint16)
            assert np.all(raw[want.size:] == 0xFFFF), "stores past the output"
            got = _bf16_get(pkg, d_o, want.shape)
            assert_close(got, want, TOL_BF16, "bf16 dw lds %s nseg %d" % (shape, nseg))
        ctx.lib.mbn_tune_set(b"dw_nseg", 0)
        ctx.lib.mbn_tune_set(b"exp0", 1)
        ctx.depthwise(d_p.ptr, d_x.ptr, d_f.ptr, h, h, 3, 1, ch, ext)
        ctx.sync()
        assert np.array_equal(got, _bf16_get(pkg, d_p, want.shape)), "LDS-staged bf16 form differs from the register kernel"
    finally:
        ctx.lib.mbn_tune_set(b"dw_nseg", 0)
        ctx.lib.mbn_tune_set(b"exp0", 0)
        for b in (d_x, d_f, d_sc, d_sh, d_o, d_p):
            b.free()


@pytest.mark.parametrize("shape", [(2 * 56 * 56, 64, 128), (2 * 14 * 14, 512, 512), (3 * 49, 1024, 1024), (12544, 32, 64),
                                   (130, 8, 24), (77, 72, 40), (5, 1024, 1000), (64, 6, 10)])
def test_bf16_pointwise(pkg, orc, ctx, shape):
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin + cout)
    x = orc.bf16_round(rng.uniform(-1, 1, (m, cin)))
    f = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)))
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    ref = orc.f32_pointwise(x, f, sc, sh, 2)
    d_x, d_f, d_sc, d_sh = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, f), ctx.to_device(sc), ctx.to_device(sh)
    d_o = ctx.alloc(m * cout * 4)
    ext = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    assert_close(_bf16_get(pkg, d_o, (m, cout)), orc.bf16_round(ref), TOL_BF16, "bf16 pw %s" % (shape,))
    # fp32 output (the FC form): only the fp32 summation order differs from the oracle
    ext = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr, io_flags=pkg.IO_OUT_F32)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    assert_close(d_o.download((m, cout), np.float32), ref, TOL_PW, "bf16 pw f32-out %s" % (shape,))


def test_bf16_pointwise_exact_integers(pkg, ctx):
    """Small integers are exact in bf16 and their dot products exact in fp32: checks the bf16 MFMA operand maps
    bit-exactly with an asymmetric filter."""
    rng = np.random.default_rng(1)
    m, cin, cout = 200, 192, 160
    x = rng.integers(-4, 5, (m, cin)).astype(np.float32)
    f = rng.integers(-4, 5, (cout, cin)).astype(np.float32)
    f[:, 0] = np.arange(cout) % 7
    want = x.astype(np.float64) @ f.astype(np.float64).T
    d_x, d_f, d_o = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, f), ctx.alloc(m * cout * 4)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, pkg.make_ext(dtype=pkg.DT_BF16, act=0, io_flags=pkg.IO_OUT_F32))
    ctx.sync()
    assert np.array_equal(d_o.download((m, cout), np.float32).astype(np.float64), want)


def test_bf16_convert_roundtrip(pkg, orc, ctx):
    x = np.random.default_rng(2).normal(0, 3, 100003).astype(np.float32)
    d_x, d_b, d_y = ctx.to_device(x), ctx.alloc(x.size * 2), ctx.alloc(x.size * 4)
    assert ctx.lib.mbn_convert_f32_to_bf16(ctx.h, d_b.ptr, d_x.ptr, x.size, None) == 0
    assert ctx.lib.mbn_convert_bf16_to_f32(ctx.h, d_y.ptr, d_b.ptr, x.size, None) == 0
    ctx.sync()
    assert np.array_equal(d_y.download((x.size,), np.float32), orc.bf16_round(x))      # same RNE rounding as the oracle
    assert np.array_equal(d_b.download((x.size,), np.uint16), pkg.f32_to_bf16_bits(x))


def _oracle_layer(orc, plan, blob, i, x, bf16):
    """Layer i+1 of the plan applied to activation x by the oracle's per-layer functions."""
    l = plan.layer[i]
    w = blob[l.w_offset:l.w_offset + max(l.w_count, 0)]
    sc = blob[l.scale_offset:l.scale_offset + l.out_ch] if l.scale_offset >= 0 else None
    sh = blob[l.shift_offset:l.shift_offset + l.out_ch] if l.shift_offset >= 0 else None
    if l.kind == orc.L_CONV:
        y = orc.f32_conv(x, w.reshape(3, 3, 3, l.out_ch), sc, sh, l.stride, orc.ACT_RELU6)
    elif l.kind == orc.L_DW:
        y = orc.f32_depthwise(x, w.reshape(3, 3, l.out_ch), sc, sh, l.stride, orc.ACT_RELU6)
    elif l.kind == orc.L_PW:
        wm = w.reshape(l.out_ch, l.in_ch)
        y = orc.f32_pointwise(x, orc.bf16_round(wm) if bf16 else wm, sc, sh, orc.ACT_RELU6).reshape(
            x.shape[0], l.out_rows, l.out_cols, l.out_ch)
    elif l.kind == orc.L_POOL:
        y = orc.f32_pool(x).reshape(x.shape[0], 1, 1, l.out_ch)
    else:
        wm = w.reshape(l.out_ch, l.in_ch)
        y = orc.f32_pointwise(x.reshape(x.shape[0], -1), orc.bf16_round(wm) if bf16 else wm, None, sh, orc.ACT_NONE)
        return y.reshape(x.shape[0], 1, 1, l.out_ch)
    return orc.bf16_round(y) if bf16 else y


@pytest.mark.parametrize("cfg", [(0.5, 160, 2), (1.0, 224, 1)])
def test_bf16_net_per_layer(pkg, orc, ctx, tmp_path, cfg):
    """BASELINE config 5: MobileNet-V1 0.5x160 and 1.0x224 in bf16. Every layer is checked against the oracle applied to
    the GPU's OWN previous activation (true per-layer error, no accumulated drift); the logits are also compared with the
    oracle's all-bf16 forward, where rounding flips accumulate over 28 layers (bound stated below)."""
    alpha, res, n = cfg
    hw, net = _make_net(pkg, ctx, tmp_path, alpha, res, 64, n)
    net.set_dtype(pkg.DT_BF16)
    net.keep_activations(True)
    imgs = np.random.default_rng(5).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 64 * 4)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    logits = d_out.download((n, 1, 1, 64), np.float32)
    oplan = orc.plan_build(alpha, res, 64)
    prev = imgs
    for i in range(hw.plan.n_layers):
        got = logits if i == hw.plan.n_layers - 1 else net.layer_output(i + 1, n)
        w = hw.blob.copy()
        if oplan.layer[i].kind == orc.L_FC:
            l = oplan.layer[i]
            w[l.w_offset:l.w_offset + l.w_count] = orc.bf16_round(w[l.w_offset:l.w_offset + l.w_count])
            want = orc.f32_pointwise(prev.reshape(n, -1), w[l.w_offset:l.w_offset + l.w_count].reshape(l.out_ch, l.in_ch),
                                     None, w[l.shift_offset:l.shift_offset + l.out_ch], orc.ACT_NONE).reshape(n, 1, 1, -1)
            assert_close(got, want, TOL_PW, "bf16 net FC")
        else:
            want = _oracle_layer(orc, oplan, w, i, prev, True)
            assert_close(got, want, TOL_BF16, "bf16 net layer %d" % (i + 1))
        prev = got
    full, _ = orc.net_forward(oplan, hw.blob, imgs, bf16=True)
    assert_close(logits, full, TOL_BF16_NET, "bf16 logits vs all-oracle bf16 forward (accumulated rounding flips)")
    # and the fp32 net on the same weights agrees with bf16 to bf16 precision (sanity of the whole mode)
    net.set_dtype(pkg.DT_F32)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    f32 = d_out.download((n, 1, 1, 64), np.float32)
    assert float(np.abs(f32 - logits).max()) <= 0.1 * max(1e-6, float(np.abs(f32).max()))
    net.destroy()


@pytest.mark.parametrize("ns", [2, 3, 8])
def test_net_multi_stream_equals_single_stream(pkg, ctx, tmp_path, ns):
    """mbn_net_set_streams: sub-batches on forked/joined streams give bit-identical logits, also for a batch that does
    not divide evenly and for a following operation queued on the context's stream (join ordering). Sub-batches of fewer
    than 5 images are not forked (they would take the 1..4-image kernels): such a forward equals the single-stream one."""
    n = 5 * ns + 1
    hw, net = _make_net(pkg, ctx, tmp_path, 0.5, 96, 40, n)
    imgs = np.random.default_rng(6).uniform(-1, 1, (n, 96, 96, 3)).astype(np.float32)
    d_in, d_out, d_p, d_a = ctx.to_device(imgs), ctx.alloc(n * 40 * 4), ctx.alloc(n * 40 * 4), ctx.alloc(n * 4)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    want = d_out.download((n, 40), np.float32)
    net.forward(d_in.ptr, d_out.ptr, 2)
    ctx.sync()
    want2 = d_out.download((2, 40), np.float32)
    net.set_streams(ns)
    for _ in range(3):
        ctx.lib.mbn_memset(ctx.h, d_out.ptr, 0xFF, n * 40 * 4)        # queued on the context stream BEFORE the fork
        net.forward(d_in.ptr, d_out.ptr, n)
        assert ctx.lib.mbn_softmax_f32(ctx.h, d_p.ptr, d_a.ptr, d_out.ptr, n, 40, None) == 0    # after the join
        ctx.sync()
        assert np.array_equal(d_out.download((n, 40), np.float32), want)
        assert np.array_equal(d_a.download((n,), np.int32), want.argmax(1))
    net.forward(d_in.ptr, d_out.ptr, 2)                               # too few images to fork
    ctx.sync()
    assert np.array_equal(d_out.download((2, 40), np.float32), want2)
    assert_close(want2, want[:2], TOL_NET, "1..4-image kernels vs the large-batch ones")
    net.destroy()


def test_net_graph_replay_equals_eager(pkg, ctx, tmp_path):
    """mbn_net_set_graph: the captured hipGraph replays bit-identically, follows changed INPUT CONTENTS (same
    pointers), and is re-captured when the batch, a pointer or the kept-activations switch changes."""
    hw, net = _make_net(pkg, ctx, tmp_path, 0.25, 64, 30, 4)
    rng = np.random.default_rng(8)
    a, b = (rng.uniform(-1, 1, (4, 64, 64, 3)).astype(np.float32) for _ in range(2))
    d_in, d_out, d_out2 = ctx.to_device(a), ctx.alloc(4 * 30 * 4), ctx.alloc(4 * 30 * 4)
    net.forward(d_in.ptr, d_out.ptr, 4)
    ctx.sync()
    want_a = d_out.download((4, 30), np.float32)
    net.set_graph(True)
    for _ in range(3):                                   # capture, then two replays
        net.forward(d_in.ptr, d_out.ptr, 4)
        ctx.sync()
        assert np.array_equal(d_out.download((4, 30), np.float32), want_a)
    d_in.upload(b)                                       # new contents, same pointers -> replay must see them
    net.forward(d_in.ptr, d_out.ptr, 4)
    ctx.sync()
    got_b = d_out.download((4, 30), np.float32)
    assert not np.array_equal(got_b, want_a)
    net.forward(d_in.ptr, d_out2.ptr, 2)                 # other batch + other output pointer -> re-capture
    ctx.sync()
    assert np.array_equal(d_out2.download((2, 30), np.float32), got_b[:2])
    net.keep_activations(True)                           # kept buffers are allocated before the capture, never inside it
    net.forward(d_in.ptr, d_out.ptr, 4)
    ctx.sync()
    assert np.array_equal(d_out.download((4, 30), np.float32), got_b)
    assert net.layer_output(13, 4).shape[0] == 4
    net.keep_activations(False)
    net.set_graph(False)
    net.forward(d_in.ptr, d_out.ptr, 4)
    ctx.sync()
    assert np.array_equal(d_out.download((4, 30), np.float32), got_b)
    net.destroy()


@pytest.mark.parametrize("cfg", [(1.0, 224), (0.5, 160)])
def test_bf16_net_full_size_batch512_every_layer(pkg, orc, ctx, tmp_path, cfg):
    """BASELINE config 5 at its own size, layer by layer (bf16 had per-layer checks on small nets only): bf16 storage, batch
    512, 1000 classes, one launch per layer (kept activations switch the fusions off, so these are the batch-512 grids of the stand-alone bf16
    kernels: dw3x3_nhwc_bf16x8, pw_stream_bf16 in both MFMA shapes, pw_gemm<bf16>). Four images spread over the batch; every layer against the
    oracle applied to the GPU's OWN previous activation of those images (true per-layer error), logits against the all-oracle bf16 forward."""
    alpha, res = cfg
    n, pick = 512, [0, 170, 341, 511]
    hw, net = _make_net(pkg, ctx, tmp_path, alpha, res, 1000, n)
    net.set_dtype(pkg.DT_BF16)
    net.keep_activations(True)
    imgs = _headline_images(n, res, 77 + res)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 1000 * 4)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    logits = d_out.download((n, 1, 1, 1000), np.float32)[pick]
    oplan = orc.plan_build(alpha, res, 1000)
    prev = imgs[pick]
    for i in range(hw.plan.n_layers):
        got = logits if i == hw.plan.n_layers - 1 else net.layer_output(i + 1, n, images=pick)
        l = oplan.layer[i]
        if l.kind == orc.L_FC:
            w = orc.bf16_round(hw.blob[l.w_offset:l.w_offset + l.w_count]).reshape(l.out_ch, l.in_ch)
            want = orc.f32_pointwise(prev.reshape(len(pick), -1), w, None, hw.blob[l.shift_offset:l.shift_offset + l.out_ch], orc.ACT_NONE).reshape(len(pick), 1, 1, -1)
            assert_close(got, want, TOL_PW, "bf16 %gx%d batch-512 FC" % cfg)
        else:
            want = _oracle_layer(orc, oplan, hw.blob, i, prev, True)
            assert_close(got, want, TOL_BF16, "bf16 %gx%d batch-512 layer %d" % (alpha, res, i + 1))
        prev = got
    full, _ = orc.net_forward(oplan, hw.blob, imgs[pick], threads=orc.num_threads(), bf16=True)
    assert_close(logits.reshape(len(pick), 1000), np.asarray(full).reshape(len(pick), 1000), TOL_BF16_NET, "bf16 %gx%d batch-512 logits" % cfg)
    net.destroy()


def test_net_full_size_batch1_every_layer(pkg, orc, ctx, tmp_path):
    """BASELINE config 2 verbatim: full MobileNet-V1 1.0x224 fp32, batch 1, on one MI355X — per-layer numerics of all
    29 layers (and the softmax tail) against the CPU oracle, each GPU layer fed by the GPU's own previous layer."""
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, 1)
    imgs = np.random.default_rng(21).uniform(-1, 1, (1, 224, 224, 3)).astype(np.float32)
    net.keep_activations(True)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(4000)
    net.forward(d_in.ptr, d_out.ptr, 1)
    ctx.sync()
    logits = d_out.download((1, 1, 1, 1000), np.float32)
    oplan = orc.plan_build(1.0, 224, 1000)
    prev = imgs
    for i in range(29):
        got = logits if i == 28 else net.layer_output(i + 1, 1)
        want = _oracle_layer(orc, oplan, hw.blob, i, prev, False)
        tol = TOL_PW if oplan.layer[i].kind in (orc.L_PW, orc.L_FC) else TOL_DW
        assert_close(got, want, tol, "1.0x224 batch-1 layer %d" % (i + 1))
        prev = got
    full, _ = orc.net_forward(oplan, hw.blob, imgs, threads=orc.num_threads())
    assert_close(logits, full, TOL_NET, "1.0x224 batch-1 logits")
    d_p, d_a = ctx.alloc(4000), ctx.alloc(4)
    assert ctx.lib.mbn_softmax_f32(ctx.h, d_p.ptr, d_a.ptr, d_out.ptr, 1, 1000, None) == 0
    ctx.sync()
    p_want, a_want = orc.f32_softmax(full.reshape(1, 1000))
    assert d_a.download((1,), np.int32)[0] == a_want[0]
    assert_close(d_p.download((1, 1000), np.float32), p_want, 1e-3, "softmax of the logits")
    net.destroy()


@pytest.mark.parametrize("alpha,res,n", [(1.0, 224, 2), (1.0, 64, 3), (1.0, 96, 1), (0.5, 160, 2), (0.5, 64, 3), (0.5, 224, 1)])
def test_fused_stem_equals_three_layers_and_oracle(pkg, orc, ctx, tmp_path, alpha, res, n):
    """mbn_stem_fused (layers 1-3 in one kernel) vs the three separate layer calls (same fmaf/MFMA order -> expected
    bit-identical) and vs the oracle's layer-3 activation. Tiles at the image border exercise the zero halo. alpha = 1:
    32 -> 32 -> 64 channels; alpha = 0.5 (BASELINE config 5's 0.5x160): 16 -> 16 -> 32, the template's second instance."""
    hw, net = _make_net(pkg, ctx, tmp_path, alpha, res, 20, n)
    c3 = hw.plan.layer[2].out_ch
    assert c3 == int(64 * alpha)
    imgs = np.random.default_rng(res).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    h = res // 2
    d_in, d_a, d_b = ctx.to_device(imgs), ctx.alloc(n * h * h * c3 * 4), ctx.alloc(n * h * h * c3 * 4)
    assert net.fused_layers(3) == 3
    net.forward(d_in.ptr, d_a.ptr, n, 3)                 # fused
    net.set_fuse_stem(False)
    assert net.fused_layers(3) == 0
    net.forward(d_in.ptr, d_b.ptr, n, 3)                 # conv1, dw2, pw3 as separate launches
    ctx.sync()
    fused, unfused = d_a.download((n, h, h, c3), np.float32), d_b.download((n, h, h, c3), np.float32)
    assert np.array_equal(fused, unfused)
    want, _ = orc.net_forward(orc.plan_build(alpha, res, 20), hw.blob, imgs, last_layer=3, threads=orc.num_threads())
    assert_close(fused, want, TOL_PW, "fused stem vs oracle")
    # whole net with and without the fused stem
    d_l1, d_l2 = ctx.alloc(n * 20 * 4), ctx.alloc(n * 20 * 4)
    net.forward(d_in.ptr, d_l2.ptr, n)
    net.set_fuse_stem(True)
    net.forward(d_in.ptr, d_l1.ptr, n)
    ctx.sync()
    assert np.array_equal(d_l1.download((n, 20), np.float32), d_l2.download((n, 20), np.float32))
    net.destroy()


@pytest.mark.parametrize("form", [6, 9])
@pytest.mark.parametrize("alpha,res,n", [(1.0, 224, 2), (1.0, 96, 3), (0.5, 160, 2), (0.5, 64, 3)])
def test_fused_stem_pw_emul(pkg, orc, ctx, tmp_path, alpha, res, n, form):
    """The fused stem under the opt-in pw_emul = 6 | 9: its pointwise phase forms the products from the exact bf16 split of the
    depthwise output and of the filter (mbn_f32_stem.hip, X6). Against the oracle at the fp32 tolerance; at alpha = 1 (K = 32)
    bit-identical to conv1 + depthwise + mbn_pointwise under the same pw_emul (same split, same product order); at alpha = 0.5
    (K = 16, outside the split GEMM's envelope) the separate layers run the fp32 MFMA kernel: fp32 tolerance."""
    hw, net = _make_net(pkg, ctx, tmp_path, alpha, res, 20, n)
    c3 = hw.plan.layer[2].out_ch
    imgs = np.random.default_rng(res + form).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    h = res // 2
    d_in, d_a, d_b = ctx.to_device(imgs), ctx.alloc(n * h * h * c3 * 4), ctx.alloc(n * h * h * c3 * 4)
    net.forward(d_in.ptr, d_b.ptr, n, 3)
    ctx.sync()
    base = d_b.download((n, h, h, c3), np.float32)
    try:
        assert ctx.lib.mbn_tune_set(b"pw_emul", form) == 0
        net.forward(d_in.ptr, d_a.ptr, n, 3)                 # fused, split products
        net.set_fuse_stem(False)
        assert ctx.lib.mbn_tune_set(b"pw_tile", 7) == 0       # the split GEMM for the narrow layer 3 whatever the tile count
        net.forward(d_in.ptr, d_b.ptr, n, 3)                 # conv1, dw2, pw3 as separate launches
        ctx.sync()
    finally:
        ctx.lib.mbn_tune_set(b"pw_emul", 0)
        ctx.lib.mbn_tune_set(b"pw_tile", 0)
    fused, unfused = d_a.download((n, h, h, c3), np.float32), d_b.download((n, h, h, c3), np.float32)
    assert not np.array_equal(fused, base), "the split form was not on the path"
    want, _ = orc.net_forward(orc.plan_build(alpha, res, 20), hw.blob, imgs, last_layer=3, threads=orc.num_threads())
    assert_close(fused, want, TOL_PW, "fused stem (pw_emul %d) vs oracle" % form)
    if alpha == 1.0:
        assert np.array_equal(fused, unfused)
    else:
        assert_close(fused, unfused, TOL_PW, "fused stem (pw_emul) vs separate layers")
    net.destroy()


def test_fused_stem_unsupported_shapes_fall_back(pkg, ctx, tmp_path):
    """Widths other than alpha = 1 (32 -> 64) and alpha = 0.5 (16 -> 32): mbn_stem_fused answers MBN_EUNSUPPORTED and the
    runner issues the 3 calls (alpha = 0.25: conv1 has 8 channels)."""
    hw, net = _make_net(pkg, ctx, tmp_path, 0.25, 64, 10, 1)
    assert net.fused_layers(0) == 0
    d = ctx.alloc(1 << 20)
    rc = ctx.lib.mbn_stem_fused(ctx.h, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, 1, 64, 8, 16, None)
    assert rc == pkg.EUNSUPPORTED
    rc = ctx.lib.mbn_stem_fused(ctx.h, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, 1, 64, 16, 64, None)
    assert rc == pkg.EUNSUPPORTED
    net.destroy()
    hw, net = _make_net(pkg, ctx, tmp_path, 0.5, 64, 10, 1)
    assert net.fused_layers(0) == 3                        # alpha = 0.5 is inside the envelope since round 2
    net.destroy()


# =========================================================================== fused depthwise -> pointwise block (§8f-1)

DWPW_SHAPES = [  # (batch, in side, Cin, Cout, stride)
    (2, 112, 64, 128, 2), (2, 56, 128, 128, 1), (2, 56, 128, 256, 2), (2, 28, 256, 256, 1),    # L4-5, L6-7, L8-9, L10-11
    (1, 28, 256, 512, 2),                                  # L12-13: two 256-column tiles, depthwise recomputed
    (3, 14, 32, 128, 1), (1, 6, 64, 384, 1), (5, 12, 96, 128, 2), (1, 2, 32, 256, 1),          # ragged M, 3 n-tiles, tiny maps
    (2, 14, 512, 512, 1), (3, 28, 512, 1024, 2), (40, 14, 64, 256, 1),                         # L14-15, Cin 512 stride 2; many tiles per workgroup
    (70, 28, 128, 128, 1), (9, 28, 64, 384, 2), (33, 10, 256, 128, 1),      # r6 (wave-private form): several tiles per wave + a remainder round; 3 slices; ragged last tile
]


@pytest.mark.parametrize("variant", [0, 6, 5, 7, 8, 11, 12])
@pytest.mark.parametrize("shape", DWPW_SHAPES)
def test_f32_dwpw_fused(pkg, orc, ctx, shape, variant):
    """mbn_dwpw_fused vs mbn_depthwise + mbn_pointwise (same arithmetic order -> bit-identical) and vs the oracle.
    variant 6 / 5 (lab build): the unified kernel with 12 / 16 waves on 192- / 256-row tiles (128-column tiles only);
    7 / 8 (lab build, round 4): the x window requested two steps ahead into a second register set (7: stride 1 with 128-column tiles;
    8: also stride 2 with 128-column tiles and the taps read inside the step); 11 / 12 (lab build, round 6): the wave-private form
    (mbn_f32_dwpw3.hip) wherever eligible / nowhere."""
    n, h, cin, cout, stride = shape
    if variant:
        _tune_lab(ctx, b"dwpw_variant", variant)
    rng = np.random.default_rng(h * 11 + cin + cout + stride)
    x = rng.uniform(-1, 1, (n, h, h, cin)).astype(np.float32)
    wd = rng.normal(0, 0.5, (3, 3, cin)).astype(np.float32)
    wp = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    s2, s3 = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b2, b3 = rng.normal(0, 0.1, cin).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    oh = (h + stride - 1) // stride
    pad = max((oh - 1) * stride + 3 - h, 0) // 2                       # TF-SAME: 1 for stride 1, 0 for stride 2 (even h)
    mid = orc.f32_depthwise(x, wd, s2, b2, stride, 2, pad_top=pad, pad_left=pad)
    want = orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(n, oh, oh, cout)
    d = [ctx.to_device(a) for a in (x, wd, s2, b2, wp, s3, b3)]
    d_f, d_m, d_u = ctx.alloc(want.nbytes), ctx.alloc(mid.nbytes), ctx.alloc(want.nbytes)
    rc = ctx.lib.mbn_dwpw_fused(ctx.h, d_f.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr,
                                n, h, h, oh, oh, cin, cout, stride, pad, pad, None)
    assert rc == 0, rc
    ctx.depthwise(d_m.ptr, d[0].ptr, d[1].ptr, oh, oh, 3, stride, cin,
                  pkg.make_ext(batch=n, act=2, pad_top=pad, pad_left=pad, in_rows=h, in_cols=h, scale=d[2].ptr, shift=d[3].ptr))
    pw_ext = pkg.make_ext(batch=1, act=2, scale=d[5].ptr, shift=d[6].ptr)
    ctx.pointwise(d_u.ptr, d_m.ptr, d[4].ptr, n * oh * oh, 1, cin, cout, pw_ext)
    ctx.sync()
    fused, unfused = d_f.download(want.shape, np.float32), d_u.download(want.shape, np.float32)
    assert_close(fused, want, TOL_PW, "dwpw %s vs oracle" % (shape,))
    assert_close(fused, unfused, TOL_PW, "dwpw %s vs depthwise+pointwise" % (shape,))
    # bit-identical with the pointwise layer on pw_gemm (the kernel every call of 5 and more images takes; a few-tile call of
    # 1..4 images takes the split-K kernel, whose summation order is another one)
    try:
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 1) == 0
        ctx.pointwise(d_u.ptr, d_m.ptr, d[4].ptr, n * oh * oh, 1, cin, cout, pw_ext)
    finally:
        ctx.lib.mbn_tune_set(b"pw_splitk", 0)
    ctx.sync()
    unfused = d_u.download(want.shape, np.float32)
    ctx.lib.mbn_tune_set(b"dwpw_variant", 0)
    assert np.array_equal(fused, unfused), "fused block differs from depthwise+pointwise by %g" % np.abs(fused - unfused).max()
    for b in d + [d_f, d_m, d_u]:
        b.free()


DWPW_EMUL_SHAPES = DWPW_SHAPES[:4] + [(3, 14, 32, 128, 1), (5, 12, 96, 128, 2), (1, 2, 32, 256, 1), (2, 14, 512, 512, 1),
                                       (43, 28, 256, 256, 1), (170, 28, 128, 256, 2),        # enough tiles for the 256-column tile
                                       (3, 14, 640, 128, 1)]                                  # Cin > 512: falls back to the fp32 kernels


@pytest.mark.parametrize("form", [6, 9])
@pytest.mark.parametrize("shape", DWPW_EMUL_SHAPES)
def test_f32_dwpw_fused_emul(pkg, orc, ctx, shape, form):
    """mbn_dwpw_fused under the opt-in pw_emul = 6 | 9 (mbn_f32_dwpw2_x6.hip: depthwise output split into three bf16 planes on its
    way into LDS, pre-split channel-paired filter image, bf16 MFMAs): against the oracle at the fp32 tolerance and BIT-IDENTICAL
    to mbn_depthwise + mbn_pointwise under the same pw_emul (same depthwise fma order, same split, same product and chunk order
    as pw_gemm_xb). Both tile widths, both strides, ragged M, many tiles per workgroup; repeatable."""
    n, h, cin, cout, stride = shape
    rng = np.random.default_rng(h * 13 + cin + cout + stride + form)
    x = rng.uniform(-1, 1, (n, h, h, cin)).astype(np.float32)
    wd = rng.normal(0, 0.5, (3, 3, cin)).astype(np.float32)
    wp = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    s2, s3 = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b2, b3 = rng.normal(0, 0.1, cin).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    oh = (h + stride - 1) // stride
    pad = max((oh - 1) * stride + 3 - h, 0) // 2
    big = n * oh * oh > 20000
    sel = slice(0, 2) if big else slice(0, n)                           # the oracle on the first two images of the big cases
    mid = orc.f32_depthwise(x[sel], wd, s2, b2, stride, 2, pad_top=pad, pad_left=pad)
    want = orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(-1, oh, oh, cout)
    full = (n, oh, oh, cout)
    d = [ctx.to_device(a) for a in (x, wd, s2, b2, wp, s3, b3)]
    nbytes = int(np.prod(full)) * 4
    d_f, d_m, d_u = ctx.alloc(nbytes + 64), ctx.alloc(n * oh * oh * cin * 4), ctx.alloc(nbytes)
    try:
        assert ctx.lib.mbn_tune_set(b"pw_emul", form) == 0
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 1) == 0
        ctx.lib.mbn_memset(ctx.h, d_f.ptr, 0xFF, nbytes + 64)
        rc = ctx.lib.mbn_dwpw_fused(ctx.h, d_f.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr,
                                    n, h, h, oh, oh, cin, cout, stride, pad, pad, None)
        assert rc == 0, rc
        ctx.sync()
        raw = d_f.download((nbytes // 4 + 16,), np.float32)
        assert np.all(raw[nbytes // 4:].view(np.uint32) == 0xFFFFFFFF), "stores past the output"
        fused = raw[:nbytes // 4].reshape(full)
        assert_close(fused[sel], want, TOL_PW, "dwpw emul %s vs oracle" % (shape,))
        rc = ctx.lib.mbn_dwpw_fused(ctx.h, d_f.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr,
                                    n, h, h, oh, oh, cin, cout, stride, pad, pad, None)
        ctx.sync()
        assert np.array_equal(fused, d_f.download(full, np.float32)), "not repeatable"
        ctx.depthwise(d_m.ptr, d[0].ptr, d[1].ptr, oh, oh, 3, stride, cin,
                      pkg.make_ext(batch=n, act=2, pad_top=pad, pad_left=pad, in_rows=h, in_cols=h, scale=d[2].ptr, shift=d[3].ptr))
        if cin <= 512:
            assert ctx.lib.mbn_tune_set(b"pw_tile", 11) == 0          # the split GEMM whatever the tile count
        ctx.pointwise(d_u.ptr, d_m.ptr, d[4].ptr, n * oh * oh, 1, cin, cout, pkg.make_ext(batch=1, act=2, scale=d[5].ptr, shift=d[6].ptr))
        ctx.sync()
        unfused = d_u.download(full, np.float32)
        if cin <= 512:
            assert np.array_equal(fused, unfused), "fused emul block differs from depthwise + pointwise(emul) by %g" % np.abs(fused - unfused).max()
        else:
            assert_close(fused, unfused, TOL_PW, "fallback block")
    finally:
        for k in (b"pw_emul", b"pw_splitk", b"pw_tile"):
            ctx.lib.mbn_tune_set(k, 0)
        for b in d + [d_f, d_m, d_u]:
            b.free()


def test_f32_dwpw_fused_envelope(pkg, ctx):
    """Shapes outside the kernel's envelope answer MBN_EUNSUPPORTED (caller falls back to two launches); null -> EINVAL."""
    d = ctx.alloc(1 << 20)
    call = lambda *a: ctx.lib.mbn_dwpw_fused(ctx.h, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, *a, None)
    assert call(1, 14, 14, 7, 7, 64, 128, 2, 0, 0) == pkg.EUNSUPPORTED          # odd output width
    assert call(1, 8, 8, 8, 8, 48, 128, 1, 1, 1) == pkg.EUNSUPPORTED            # Cin not a multiple of 32
    assert call(1, 8, 8, 8, 8, 2048, 512, 1, 1, 1) == pkg.EUNSUPPORTED          # Cin beyond the LDS-resident filter
    assert call(1, 8, 8, 8, 8, 64, 64, 1, 1, 1) == pkg.EUNSUPPORTED             # Cout < 128
    assert call(1, 8, 8, 8, 8, 64, 128, 3, 1, 1) == pkg.EUNSUPPORTED            # stride 3
    assert ctx.lib.mbn_dwpw_fused(ctx.h, None, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, 1, 8, 8, 8, 8, 64, 128, 1, 1, 1, None) == pkg.EINVAL
    d.free()


def test_net_fused_blocks_equal_separate_layers(pkg, orc, ctx, tmp_path):
    """Net runner with depthwise->pointwise blocks fused (mbn_net_set_fuse_blocks) vs every layer its own launch:
    identical logits and identical partial outputs (last_layer inside/at the end of a fused block); the launch list
    mbn_net_launches reports matches the mask; the oracle bounds the result."""
    n, res = 5, 64
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, res, 20, n)
    imgs = np.random.default_rng(11).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    d_in = ctx.to_device(imgs)
    # default mask: stem + blocks 4, 6, 8, 10 — each only from the batch at which its launch has enough 128 x 128 tiles
    # (half the compute units; below that two shorter launches are faster: profiles/r02/i_small_batch.txt)
    assert net.launches(256)[:5] == [(1, 3), (4, 2), (6, 2), (8, 2), (10, 2)]
    assert (12, 1) in net.launches(256)
    assert net.launches(n) == [(1, 3)] + [(l, 1) for l in range(4, 30)]
    assert net.launches(64)[:4] == [(1, 3), (4, 2), (6, 2), (8, 1)]
    outs = {}
    for mask in (0xFFFFFFFE, 0):
        net.set_fuse_blocks(mask)
        la = net.launches(n)
        if mask:
            assert la == [(1, 3)] + [(l, 2) for l in range(4, 27, 2)] + [(28, 1), (29, 1)], la
        else:
            assert la == [(1, 3)] + [(l, 1) for l in range(4, 30)], la
        for last in (0, 5, 7, 13, 27):
            l = hw.plan.layer[(last or 29) - 1]
            d_out = ctx.alloc(n * l.out_rows * l.out_cols * l.out_ch * 4)
            net.forward(d_in.ptr, d_out.ptr, n, last)
            ctx.sync()
            outs[(mask, last)] = d_out.download((n, l.out_rows, l.out_cols, l.out_ch), np.float32)
            d_out.free()
    for last in (0, 5, 7, 13, 27):
        assert np.array_equal(outs[(0xFFFFFFFE, last)], outs[(0, last)]), last
    want, _ = orc.net_forward(orc.plan_build(1.0, res, 20), hw.blob, imgs, threads=orc.num_threads())
    assert_close(outs[(0xFFFFFFFE, 0)].reshape(n, 20), np.asarray(want).reshape(n, 20), TOL_NET, "fused-block net vs oracle")
    # kept activations force single-layer launches
    net.set_fuse_blocks(0xFFFFFFFE)
    net.keep_activations(True)
    assert net.launches(n) == [(l, 1) for l in range(1, 30)]
    net.destroy()


def _launches_run(ctx, net, plan, d_in, batch, last):
    """Number of launches one single-stream forward(batch, last) records in the profiling scope."""
    l = plan.layer[(last or plan.n_layers) - 1]
    d_out = ctx.alloc(batch * l.out_rows * l.out_cols * l.out_ch * 4)
    ctx.profile_begin(64)
    try:
        net.forward(d_in.ptr, d_out.ptr, batch, last)
    finally:
        ran = ctx.profile_end(64)
        d_out.free()
    return len(ran)


def test_net_launch_list_is_what_runs(pkg, ctx, tmp_path):
    """mbn_net_launches lists exactly the launches one forward issues (bench.py sizes its per-launch profile from it): the count a
    profiled single-stream forward records equals the list's length, in fp32 and bf16, under the default and an explicit mask, with
    kept activations, the stem unfused, pool + FC fused, the resident launches on and off, and last_layer values inside fused launches."""
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 64, 20, 64)
    d_in = ctx.to_device(np.random.default_rng(21).uniform(-1, 1, (64, 64, 64, 3)).astype(np.float32))
    cases = [("default mask", n, last) for n in (1, 5, 64) for last in (0, 3, 5, 13, 27)]
    cases += [("mask 0xFFFFFFFE", n, last) for n in (1, 5, 64) for last in (0, 3, 5, 13, 27)]
    cases += [("kept", 5, last) for last in (0, 5, 13)] + [("stem unfused", 5, last) for last in (0, 3, 5)] + [("pool + FC", 2, 0)]
    for what, n, last in cases:
        if what == "mask 0xFFFFFFFE":
            net.set_fuse_blocks(0xFFFFFFFE)
        net.keep_activations(what == "kept")
        net.set_fuse_stem(what != "stem unfused")
        net.set_fuse_tail(what == "pool + FC")
        if what == "pool + FC":
            assert net.launches(n)[-1] == (28, 2), net.launches(n)
        listed = net.launches(n, last)
        assert _launches_run(ctx, net, hw.plan, d_in, n, last) == len(listed), (what, n, last, listed)
    net.destroy()

    hw, net = _make_net(pkg, ctx, tmp_path, 0.5, 160, 20, 16)
    net.set_dtype(pkg.DT_BF16)
    d_in = ctx.to_device(np.random.default_rng(22).uniform(-1, 1, (16, 160, 160, 3)).astype(np.float32))
    for resident in (True, False):
        net.set_fuse_resident(resident)
        for n in (1, 16):
            if resident:
                assert (14, 10) in net.launches(n) and (24, 5) in net.launches(n), net.launches(n)
            for last in (0, 15, 18, 23, 26, 28):      # cut into the resident run (layers 14-23) and the resident tail (24-28)
                listed = net.launches(n, last)
                assert _launches_run(ctx, net, hw.plan, d_in, n, last) == len(listed), (resident, n, last, listed)
    net.destroy()


def test_net_misaligned_blob_segments_run_unfused(pkg, orc, ctx, tmp_path):
    """A caller's plan whose blob segments are not 16-byte aligned (one leading float in the device blob, every offset one float further):
    the fused kernels cannot take them, so the launch list holds single layers only, the forward issues exactly those, and the logits
    match the oracle. fp32 only: mbn_net_set_dtype(bf16) refuses misaligned pointwise segments."""
    n, res = 5, 64
    hw, aligned = _make_net(pkg, ctx, tmp_path, 1.0, res, 20, n)
    aligned.destroy()
    plan = pkg.Plan.from_buffer_copy(hw.plan)
    for i in range(plan.n_layers):
        l = plan.layer[i]
        for f in ("w_offset", "scale_offset", "shift_offset"):
            if getattr(l, f) >= 0:
                setattr(l, f, getattr(l, f) + 1)
    plan.blob_floats += 1
    net = pkg.Net(ctx, plan, np.concatenate([np.zeros(1, np.float32), hw.blob]), n)
    assert [c for _, c in net.launches(n)] == [1] * 29                   # the default would fuse the stem
    net.set_fuse_blocks(0xFFFFFFFE)
    assert [c for _, c in net.launches(n)] == [1] * 29                   # ... and this mask every block
    imgs = np.random.default_rng(23).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 20 * 4)
    assert _launches_run(ctx, net, plan, d_in, n, 0) == 29
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    want, _ = orc.net_forward(orc.plan_build(1.0, res, 20), hw.blob, imgs, threads=orc.num_threads())
    assert_close(d_out.download((n, 20), np.float32), np.asarray(want).reshape(n, 20), TOL_NET, "misaligned-segment net vs oracle")
    net.destroy()


@pytest.mark.parametrize("broken", ["pool_not_global", "d1_map", "p0_in_ch"])
def test_net_inconsistent_tail_plan_is_not_fused(pkg, ctx, tmp_path, broken):
    """mbn_tail_resident_bf16 takes only (rows, cols, 256, 512) and assumes the rest of layers 24-28: a plan that breaks one of those
    assumptions is not listed as the resident tail. The launch list only: no forward runs on a broken geometry."""
    hw, net = _make_net(pkg, ctx, tmp_path, 0.5, 160, 20, 16)
    net.set_dtype(pkg.DT_BF16)
    assert (24, 5) in net.launches(16)
    net.destroy()
    plan = pkg.Plan.from_buffer_copy(hw.plan)
    if broken == "pool_not_global":
        plan.layer[27].out_rows = plan.layer[27].out_cols = 2
    elif broken == "d1_map":
        plan.layer[25].in_rows = plan.layer[25].in_cols = 6
    else:
        plan.layer[24].in_ch = 512
    net = pkg.Net(ctx, plan, hw.blob.copy(), 16)
    net.set_dtype(pkg.DT_BF16)
    assert 5 not in [c for _, c in net.launches(16)], net.launches(16)
    net.destroy()


# =========================================================================== classifier tail (§8f-3)

def _topk_ref(logits, k):
    """Oracle-side top-k: softmax from the oracle, order = (value descending, index ascending) like its strict '>' scan."""
    n, c = logits.shape
    idx = np.full((n, k), -1, np.int32)
    for i in range(n):
        order = sorted(range(c), key=lambda j: (-float(logits[i, j]), j))[:k]
        idx[i, :len(order)] = order
    return idx


def test_softmax_topk_and_classifier_tail(pkg, orc, ctx):
    rng = np.random.default_rng(21)
    n, classes, k = 6, 1000, 5
    logits = rng.normal(0, 3, (n, classes)).astype(np.float32)
    logits[1, 7] = logits[1, 900] = logits[1, 3] = 40.0          # three-way tie for the maximum -> indices 3, 7, 900 in order
    logits[2, :] = 0.25                                            # all equal -> 0, 1, 2, 3, 4
    want_p, want_a = orc.f32_softmax(logits)
    want_i = _topk_ref(logits, k)
    d_l, d_p, d_i, d_v = ctx.to_device(logits), ctx.alloc(logits.nbytes), ctx.alloc(n * k * 4), ctx.alloc(n * k * 4)
    assert ctx.lib.mbn_softmax_topk_f32(ctx.h, d_p.ptr, d_i.ptr, d_v.ptr, d_l.ptr, n, classes, k, None) == 0
    ctx.sync()
    got_i, got_v = d_i.download((n, k), np.int32), d_v.download((n, k), np.float32)
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_i[:, 0], want_a)
    assert_close(d_p.download((n, classes), np.float32), want_p, 1e-5, "softmax")
    assert_close(got_v, np.take_along_axis(want_p, want_i.astype(np.int64), axis=1), 1e-5, "top-k probabilities")
    # fewer classes than k: padded with -1 / 0
    small = rng.normal(0, 1, (2, 3)).astype(np.float32)
    d_s = ctx.to_device(small)
    assert ctx.lib.mbn_softmax_topk_f32(ctx.h, None, d_i.ptr, d_v.ptr, d_s.ptr, 2, 3, 5, None) == 0
    ctx.sync()
    gi = d_i.download((n, k), np.int32)[:2]
    assert np.array_equal(gi.reshape(-1)[:10].reshape(2, 5)[:, 3:], -np.ones((2, 2), np.int32))
    assert ctx.lib.mbn_softmax_topk_f32(ctx.h, None, d_i.ptr, d_v.ptr, d_s.ptr, 2, 3, 9, None) == pkg.EINVAL
    # whole tail: pool -> FC(+bias) -> softmax/top-k against the oracle's three stages
    ch, h, classes2 = 1024, 7, 1000
    x = rng.uniform(0, 6, (n, h, h, ch)).astype(np.float32)
    w = rng.normal(0, (1.0 / ch) ** 0.5, (classes2, ch)).astype(np.float32)
    b = rng.normal(0, 0.5, classes2).astype(np.float32)
    pooled = orc.f32_pool(x)
    ref_logits = orc.f32_pointwise(pooled.reshape(n, ch), w, None, b, 0)
    ref_p, _ = orc.f32_softmax(ref_logits)
    d_x, d_w, d_b = ctx.to_device(x), ctx.to_device(w), ctx.to_device(b)
    d_lg, d_po = ctx.alloc(n * classes2 * 4), ctx.alloc(n * ch * 4)
    assert ctx.lib.mbn_classifier_tail(ctx.h, d_i.ptr, d_v.ptr, None, d_lg.ptr, d_po.ptr, d_x.ptr, d_w.ptr, d_b.ptr,
                                       n, h, h, ch, classes2, k, None) == 0
    ctx.sync()
    got_logits = d_lg.download((n, classes2), np.float32)
    assert_close(got_logits, ref_logits, TOL_PW, "tail logits")
    got_i = d_i.download((n, k), np.int32)
    assert np.array_equal(got_i, _topk_ref(got_logits, k))                     # order decided on the device's own logits
    assert_close(d_v.download((n, k), np.float32), np.take_along_axis(ref_p, got_i.astype(np.int64), axis=1), 1e-3, "tail top-k probs")


@pytest.mark.parametrize("shape", [(1, 7, 1024, 1000), (4, 7, 1024, 1000), (3, 5, 512, 1000), (2, 7, 256, 37), (4, 2, 64, 16), (1, 3, 1024, 1001)])
def test_pool_fc_one_launch(pkg, orc, ctx, shape):
    """mbn_pool_fc (pool + FC in one launch for 1...4 images: MobileNet.c:2601-2739 as one kernel): against the oracle's pool ->
    pointwise(bias, no ReLU); an image's logits do not depend on the batch it is in (bit for bit); repeatable on the same workspace
    (the counters return to zero); exact on small integers with an asymmetric filter (slice / class-range maps); envelope errors."""
    n, h, ch, classes = shape
    rng = np.random.default_rng(n + h + ch + classes)
    x = rng.uniform(0, 6, (n, h, h, ch)).astype(np.float32)
    w = rng.normal(0, (1.0 / ch) ** 0.5, (classes, ch)).astype(np.float32)
    b = rng.normal(0, 0.5, classes).astype(np.float32)
    ref = orc.f32_pointwise(orc.f32_pool(x).reshape(n, ch), w, None, b, 0)
    nb = ctx.lib.mbn_pool_fc_workspace_bytes(ch, classes)
    assert nb >= 512 + (ch // 64) * 4 * classes * 4
    d_x, d_w, d_b, d_o, d_ws = ctx.to_device(x), ctx.to_device(w), ctx.to_device(b), ctx.alloc(n * classes * 4 + 64), ctx.alloc(nb)
    ctx.lib.mbn_memset(ctx.h, d_ws.ptr, 0, nb)
    ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, n * classes * 4 + 64)

    def run(count, bias=d_b.ptr):
        assert ctx.lib.mbn_pool_fc(ctx.h, d_o.ptr, d_x.ptr, d_w.ptr, bias, count, h, h, ch, classes, d_ws.ptr, nb, None) == 0
        ctx.sync()
        return d_o.download((count, classes), np.float32)
    got = run(n)
    assert np.all(d_o.download((n * classes + 16,), np.uint32)[n * classes:] == 0xFFFFFFFF), "stores past the output"
    assert_close(got, ref, TOL_PW, "pool_fc %s vs oracle" % (shape,))
    assert np.array_equal(got, run(n)), "not repeatable on the same workspace"
    assert np.all(d_ws.download((128,), np.uint32) == 0), "arrival counters not back to zero"
    for k in range(1, n):
        assert np.array_equal(run(k), got[:k]), "logits depend on the batch (%d of %d)" % (k, n)
    # the WHOLE tail in one launch (round 4, mbn_classifier_tail_fused: + softmax + top-k by the last class range to finish): logits, probabilities
    # and winners bit for bit those of mbn_pool_fc + mbn_softmax_topk_f32, against the oracle's softmax, repeatable, counters back to zero
    if classes <= 1024:
        kk = min(5, classes)
        d_p, d_i, d_v = ctx.alloc(n * classes * 4), ctx.alloc(n * 8 * 4), ctx.alloc(n * 8 * 4)
        d_p2, d_i2, d_v2, d_o2 = ctx.alloc(n * classes * 4), ctx.alloc(n * 8 * 4), ctx.alloc(n * 8 * 4), ctx.alloc(n * classes * 4)
        assert ctx.lib.mbn_softmax_topk_f32(ctx.h, d_p.ptr, d_i.ptr, d_v.ptr, d_o.ptr, n, classes, kk, None) == 0
        for rep in range(2):
            assert ctx.lib.mbn_classifier_tail_fused(ctx.h, d_i2.ptr, d_v2.ptr, d_p2.ptr, d_o2.ptr, d_x.ptr, d_w.ptr, d_b.ptr, n, h, h, ch, classes, kk,
                                                     d_ws.ptr, nb, None) == 0
            ctx.sync()
            assert np.array_equal(d_o2.download((n, classes), np.float32), got), "one-launch tail: logits"
            assert np.array_equal(d_i2.download((n, kk), np.int32), d_i.download((n, kk), np.int32)), "one-launch tail: winners"
            assert np.array_equal(d_v2.download((n, kk), np.float32), d_v.download((n, kk), np.float32)), "one-launch tail: winners' probabilities"
            assert np.array_equal(d_p2.download((n, classes), np.float32), d_p.download((n, classes), np.float32)), "one-launch tail: distribution"
            assert np.all(d_ws.download((128,), np.uint32) == 0), "arrival counters not back to zero"
        e = np.exp(ref.astype(np.float64) - ref.max(1, keepdims=True))
        assert_close(d_p2.download((n, classes), np.float32), e / e.sum(1, keepdims=True), 1e-4, "one-launch tail vs float64 softmax")
        assert np.array_equal(d_i2.download((n, kk), np.int32)[:, 0], ref.argmax(1))
        assert ctx.lib.mbn_classifier_tail_fused(ctx.h, d_i2.ptr, d_v2.ptr, None, d_o2.ptr, d_x.ptr, d_w.ptr, None, 1, h, h, ch, classes, 1, d_ws.ptr, nb, None) == 0
        assert ctx.lib.mbn_classifier_tail_fused(ctx.h, d_i2.ptr, d_v2.ptr, None, d_o2.ptr, d_x.ptr, d_w.ptr, None, 5, h, h, ch, classes, 1, d_ws.ptr, nb, None) == pkg.EUNSUPPORTED
        assert ctx.lib.mbn_classifier_tail_fused(ctx.h, d_i2.ptr, d_v2.ptr, None, d_o2.ptr, d_x.ptr, d_w.ptr, None, 1, h, h, ch, classes, 9, d_ws.ptr, nb, None) == pkg.EINVAL
        ctx.sync()
        for bfr in (d_p, d_i, d_v, d_p2, d_i2, d_v2, d_o2):
            bfr.free()
    assert_close(run(n, None), ref - b, TOL_PW, "no bias")
    xi = rng.integers(0, 4, (n, h, h, ch)).astype(np.float32)
    xi[:, 1:] = xi[:, :1]                                        # every row equal: the pooled value is the exact integer mean over columns
    xi[:, :, 1:] = xi[:, :, :1]
    wi = rng.integers(-2, 3, (classes, ch)).astype(np.float32)
    wi[:, 0] = np.arange(classes) % 5
    wi[:, ch - 1] = np.arange(classes) % 3
    d_x.upload(xi); d_w.upload(wi)
    want = xi[:, 0, 0].astype(np.float64) @ wi.astype(np.float64).T
    assert np.array_equal(run(n, None).astype(np.float64), want)
    assert ctx.lib.mbn_pool_fc(ctx.h, d_o.ptr, d_x.ptr, d_w.ptr, None, 5, h, h, ch, classes, d_ws.ptr, nb, None) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_pool_fc(ctx.h, d_o.ptr, d_x.ptr, d_w.ptr, None, n, h, h, ch, classes, d_ws.ptr, nb - 4, None) == pkg.EINVAL
    assert ctx.lib.mbn_pool_fc_workspace_bytes(ch + 32, classes) == 0
    for bfr in (d_x, d_w, d_b, d_o, d_ws):
        bfr.free()


def test_net_tail_one_launch_matches_two(pkg, orc, ctx, tmp_path):
    """The net runner's pool + FC launch at 1...4 images (mbn_net_set_fuse_tail; off by default: measured slower) against the two launches: same launch list
    except the tail, logits within the fp32 tolerance of each other and of the oracle, and forward(4)[:k] == forward(k) either way."""
    n, res = 4, 224
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, res, 1000, n)
    imgs = _headline_images(n, res, 5)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 1000 * 4)
    outs = {}
    for fused in (True, False):
        net.set_fuse_tail(fused)
        la = net.launches(n)
        assert la[-1] == ((28, 2) if fused else (29, 1)), la
        for k in (n, 1, 3):
            net.forward(d_in.ptr, d_out.ptr, k)
            ctx.sync()
            outs[(fused, k)] = d_out.download((k, 1000), np.float32)
        for k in (1, 3):
            assert np.array_equal(outs[(fused, k)], outs[(fused, n)][:k]), (fused, k)
    assert_close(outs[(True, n)], outs[(False, n)], 1e-5, "one-launch tail vs two launches")
    want, _ = orc.net_forward(orc.plan_build(1.0, res, 1000), hw.blob, imgs, threads=orc.num_threads())
    assert_close(outs[(True, n)], np.asarray(want).reshape(n, 1000), TOL_NET, "one-launch tail vs oracle")
    net.destroy()


def test_net_classify_matches_forward(pkg, orc, ctx, tmp_path):
    n, res = 4, 64
    hw, net = _make_net(pkg, ctx, tmp_path, 0.5, res, 30, n)
    imgs = np.random.default_rng(2).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 30 * 4)
    d_i, d_v = ctx.alloc(n * 3 * 4), ctx.alloc(n * 3 * 4)
    net.forward(d_in.ptr, d_out.ptr, n)
    net.classify(d_in.ptr, n, 3, d_i.ptr, d_v.ptr)
    ctx.sync()
    logits = d_out.download((n, 30), np.float32)
    assert np.array_equal(d_i.download((n, 3), np.int32), _topk_ref(logits, 3))
    p, _ = orc.f32_softmax(logits)
    assert_close(d_v.download((n, 3), np.float32), np.take_along_axis(p, _topk_ref(logits, 3).astype(np.int64), axis=1), 1e-5, "classify")
    net.destroy()


# =========================================================================== uint8 front-end (§8f-2)

def test_u8_input_conv1_stem_and_net(pkg, orc, ctx, tmp_path):
    """MBN_IO_IN_U8: conv1 / the fused stem / the whole net fed with the raw uint8 HWC image == the same fed with
    mbn_normalize_u8_to_f32's output (bit-identical: same fmaf), and within tolerance of the oracle on x/127.5 - 1."""
    rng = np.random.default_rng(8)
    for (n, h, cout) in [(2, 64, 32), (1, 33, 8), (2, 20, 6)]:          # fast first-layer kernel, LDS-weights kernel, generic
        u8 = rng.integers(0, 256, (n, h, h, 3), dtype=np.uint8)
        xf = (u8.astype(np.float32) * np.float32(1 / 127.5) + np.float32(-1)).astype(np.float32)
        f = rng.normal(0, 0.3, (3, 3, 3, cout)).astype(np.float32)
        sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
        want = orc.f32_conv(xf, f, sc, sh, 2, 2)
        d_u, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (u8, f, sc, sh))
        d_n, d_a, d_b = ctx.alloc(xf.nbytes), ctx.alloc(want.nbytes), ctx.alloc(want.nbytes)
        assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, d_n.ptr, d_u.ptr, u8.size, 1 / 127.5, -1.0, None) == 0
        ctx.convolute(d_a.ptr, d_u.ptr, None, None, d_f.ptr, h, h, 3, 2, cout,
                      pkg.make_ext(batch=n, act=2, cin=3, scale=d_sc.ptr, shift=d_sh.ptr, io_flags=pkg.IO_IN_U8))
        ctx.convolute(d_b.ptr, d_n.ptr, None, None, d_f.ptr, h, h, 3, 2, cout,
                      pkg.make_ext(batch=n, act=2, cin=3, scale=d_sc.ptr, shift=d_sh.ptr))
        ctx.sync()
        got = d_a.download(want.shape, np.float32)
        assert np.array_equal(got, d_b.download(want.shape, np.float32)), (n, h, cout)
        assert_close(got, want, TOL_DW, "conv1 from uint8")
    # whole net (fused stem path and separate-layer path)
    n, res = 2, 64
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, res, 20, n)
    u8 = rng.integers(0, 256, (n, res, res, 3), dtype=np.uint8)
    d_u, d_n = ctx.to_device(u8), ctx.alloc(u8.size * 4)
    assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, d_n.ptr, d_u.ptr, u8.size, 1 / 127.5, -1.0, None) == 0
    d_o1, d_o2, d_o3 = ctx.alloc(n * 80), ctx.alloc(n * 80), ctx.alloc(n * 80)
    net.forward(d_n.ptr, d_o1.ptr, n)
    net.set_input_u8(True)
    assert net.fused_layers(0) == 3
    net.forward(d_u.ptr, d_o2.ptr, n)                     # mbn_stem_fused_u8
    net.set_fuse_stem(False)
    net.forward(d_u.ptr, d_o3.ptr, n)                     # mbn_convolute with MBN_IO_IN_U8
    ctx.sync()
    a, b, c = (d.download((n, 20), np.float32) for d in (d_o1, d_o2, d_o3))
    assert np.array_equal(a, b) and np.array_equal(a, c)
    net.destroy()


def test_f32_dwpw_fused_top_left_padding(pkg, orc, ctx):
    """Stride 2 with pad_top = pad_left = 1 — the reference's own top/left-only convention (kernel.cl:16-20, B6) — through
    the fused block: the buffer-load zero padding must follow the explicit pads, not TF-SAME."""
    rng = np.random.default_rng(77)
    n, h, cin, cout = 2, 12, 64, 128
    x = rng.uniform(-1, 1, (n, h, h, cin)).astype(np.float32)
    wd = rng.normal(0, 0.5, (3, 3, cin)).astype(np.float32)
    wp = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    s2, s3 = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b2, b3 = rng.normal(0, 0.1, cin).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    mid = orc.f32_depthwise(x, wd, s2, b2, 2, 2, out_rows=6, out_cols=6, pad_top=1, pad_left=1)
    want = orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(n, 6, 6, cout)
    d = [ctx.to_device(a) for a in (x, wd, s2, b2, wp, s3, b3)]
    d_f = ctx.alloc(want.nbytes)
    assert ctx.lib.mbn_dwpw_fused(ctx.h, d_f.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr,
                                  n, h, h, 6, 6, cin, cout, 2, 1, 1, None) == 0
    ctx.sync()
    assert_close(d_f.download(want.shape, np.float32), want, TOL_PW, "dwpw top/left padding")


# Asymmetric pads on tiles that span many images: 9 images of 6 x 10 pixels, (stride, pad_top, pad_left, out_rows, out_cols). The output sizes are
# given explicitly: 48 / 40 / 16 / 18 pixels per image, so a 128-row tile covers 2.7 - 8 images (in the full-rate window offsets the second
# reciprocal division, the image quotient q2, is then > 0 for most lanes) and the last tile is ragged (432, 360, 144, 162 pixels).
DWPW_ASYM_N, DWPW_ASYM_H, DWPW_ASYM_W = 9, 6, 10
DWPW_ASYM_GEOM = [(1, 1, 0, 6, 8), (1, 0, 1, 4, 10), (2, 1, 0, 4, 4), (2, 0, 1, 3, 6)]


def _dwpw_asym_taps(geom):
    """inside[oy][ox] = taps of output pixel (oy, ox) that lie inside the 6 x 10 image (of 9)."""
    stride, pt, pl, oh, ow = geom
    iy = np.arange(oh)[:, None] * stride - pt + np.arange(3)[None, :]                 # [oh][dy]
    ix = np.arange(ow)[:, None] * stride - pl + np.arange(3)[None, :]                 # [ow][dx]
    rin = ((iy >= 0) & (iy < DWPW_ASYM_H)).sum(1)
    cin = ((ix >= 0) & (ix < DWPW_ASYM_W)).sum(1)
    return rin[:, None] * cin[None, :]


def _dwpw_asym_check(geom):
    """What makes the case a test of the padding: no output pixel is all padding (the data decides every value), every pixel of the padded edge
    has taps outside the image (zeros that are not there change it), the far edge overruns the image too, and the tiles are as the table
    above says. (A pixel in the middle of the map has its nine taps inside: not every pixel can have one outside; those pixels are there too.)"""
    stride, pt, pl, oh, ow = geom
    inside = _dwpw_asym_taps(geom)
    assert inside.min() >= 1, geom
    outside = inside < 9
    assert (outside[0, :].all() if pt else outside[:, 0].all()), geom                # the padded edge: every pixel of it
    assert (outside[:, -1].all() if pl else outside[-1, :].all()), geom              # the far edge of the same axis: past the image
    assert (~outside).any(), geom
    m = DWPW_ASYM_N * oh * ow
    assert ow % 2 == 0 and oh * ow <= 64 and m > 128 and m % 128 != 0, geom          # >= 2 images per tile, >= 2 tiles, ragged


@pytest.mark.parametrize("chan", [(64, 128), (128, 128)])
@pytest.mark.parametrize("geom", DWPW_ASYM_GEOM)
def test_f32_dwpw_fused_asymmetric_pads_many_images(pkg, orc, ctx, geom, chan):
    """mbn_dwpw_fused with pad_top != pad_left on tiles that span several images (see DWPW_ASYM_GEOM): vs the oracle at TOL_PW and bit-identical
    with mbn_depthwise + mbn_pointwise (pw_gemm). 64 -> 128: the unified-wave kernel; 128 -> 128 at stride 1: the wave-private form."""
    _dwpw_asym_check(geom)
    stride, pt, pl, oh, ow = geom
    cin, cout = chan
    n, h, w = DWPW_ASYM_N, DWPW_ASYM_H, DWPW_ASYM_W
    rng = np.random.default_rng(1000 * stride + 100 * pt + 10 * pl + cin)
    x = rng.uniform(-1, 1, (n, h, w, cin)).astype(np.float32)
    wd = rng.normal(0, 0.5, (3, 3, cin)).astype(np.float32)
    wp = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    s2, s3 = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b2, b3 = rng.normal(0, 0.1, cin).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    mid = orc.f32_depthwise(x, wd, s2, b2, stride, 2, out_rows=oh, out_cols=ow, pad_top=pt, pad_left=pl)
    want = orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(n, oh, ow, cout)
    d = [ctx.to_device(a) for a in (x, wd, s2, b2, wp, s3, b3)]
    d_f, d_m, d_u = ctx.alloc(want.nbytes), ctx.alloc(mid.nbytes), ctx.alloc(want.nbytes)
    rc = ctx.lib.mbn_dwpw_fused(ctx.h, d_f.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, d[6].ptr,
                                n, h, w, oh, ow, cin, cout, stride, pt, pl, None)
    assert rc == 0, rc
    ctx.depthwise(d_m.ptr, d[0].ptr, d[1].ptr, oh, ow, 3, stride, cin,
                  pkg.make_ext(batch=n, act=2, pad_top=pt, pad_left=pl, in_rows=h, in_cols=w, scale=d[2].ptr, shift=d[3].ptr))
    try:
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 1) == 0
        ctx.pointwise(d_u.ptr, d_m.ptr, d[4].ptr, n * oh * ow, 1, cin, cout, pkg.make_ext(batch=1, act=2, scale=d[5].ptr, shift=d[6].ptr))
    finally:
        ctx.lib.mbn_tune_set(b"pw_splitk", 0)
    ctx.sync()
    fused, unfused = d_f.download(want.shape, np.float32), d_u.download(want.shape, np.float32)
    for b in d + [d_f, d_m, d_u]:
        b.free()
    assert_close(fused, want, TOL_PW, "dwpw %s %s vs oracle" % (geom, chan))
    assert np.array_equal(fused, unfused), "fused block %s %s differs from depthwise+pointwise by %g" % (geom, chan, np.abs(fused - unfused).max())


@pytest.mark.parametrize("chan", [(64, 128), (128, 128), (32, 64)])
@pytest.mark.parametrize("geom", DWPW_ASYM_GEOM)
def test_bf16_dwpw_fused_asymmetric_pads_many_images(pkg, orc, ctx, geom, chan):
    """mbn_dwpw_fused_bf16 on the same geometry; 32 -> 64 is the form in which four lanes cover a pixel pair (256-row tiles) and, on the general
    offsets, the one with lanes masked out. Against the oracle's bf16 emulation at the bf16 tests' tolerance."""
    _dwpw_asym_check(geom)
    stride, pt, pl, oh, ow = geom
    cin, cout = chan
    n, h, w = DWPW_ASYM_N, DWPW_ASYM_H, DWPW_ASYM_W
    rng = np.random.default_rng(2000 * stride + 100 * pt + 10 * pl + cin)
    x = orc.bf16_round(rng.uniform(0, 4, (n, h, w, cin)).astype(np.float32))
    wd = rng.normal(0, 0.5, (3, 3, cin)).astype(np.float32)
    wp = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32))
    s2, s3 = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b2, b3 = rng.normal(0, 0.1, cin).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    mid = orc.bf16_round(orc.f32_depthwise(x, wd, s2, b2, stride, 2, out_rows=oh, out_cols=ow, pad_top=pt, pad_left=pl))
    want = orc.bf16_round(orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(n, oh, ow, cout))
    d_x, d_wp = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, wp)
    d = [ctx.to_device(a) for a in (wd, s2, b2, s3, b3)]
    d_f = ctx.alloc(want.size * 2)
    rc = ctx.lib.mbn_dwpw_fused_bf16(ctx.h, d_f.ptr, d_x.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d_wp.ptr, d[3].ptr, d[4].ptr,
                                     n, h, w, oh, ow, cin, cout, stride, pt, pl, None)
    assert rc == 0, rc
    ctx.sync()
    fused = _bf16_get(pkg, d_f, want.shape)
    for b in d + [d_x, d_wp, d_f]:
        b.free()
    assert_close(fused, want, TOL_BF16, "bf16 fused block %s %s vs oracle" % (geom, chan))


@pytest.mark.parametrize("alpha", [1.0, 0.5])
def test_bf16_fused_stem_vs_oracle_and_separate_layers(pkg, orc, ctx, tmp_path, alpha):
    """bf16 mode of the fused stem (MBN_STEM_BF16): layer-3 activation vs the oracle's bf16 emulation of layers 1-3 (every
    layer output rounded to bf16, bf16 pointwise filter) and vs the three separate bf16 launches. Not bit-identical to the
    separate launches by construction — their pointwise runs on the bf16 MFMA, the stem's on the fp32 MFMA over the same
    bf16-representable operands, so the fp32 summation order differs — hence the bf16 tolerance on both comparisons."""
    n, res = 2, 64
    hw, net = _make_net(pkg, ctx, tmp_path, alpha, res, 20, n)
    c3 = hw.plan.layer[2].out_ch
    net.set_dtype(pkg.DT_BF16)
    imgs = np.random.default_rng(31).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    h = res // 2
    d_in, d_a, d_b = ctx.to_device(imgs), ctx.alloc(n * h * h * c3 * 2), ctx.alloc(n * h * h * c3 * 2)
    assert net.fused_layers(3) == 3
    net.forward(d_in.ptr, d_a.ptr, n, 3)
    net.set_fuse_stem(False)
    net.forward(d_in.ptr, d_b.ptr, n, 3)
    ctx.sync()
    fused, sep = _bf16_get(pkg, d_a, (n, h, h, c3)), _bf16_get(pkg, d_b, (n, h, h, c3))
    oplan = orc.plan_build(alpha, res, 20)
    x = imgs
    for i in range(3):
        x = _oracle_layer(orc, oplan, hw.blob, i, x, True)
    assert_close(fused, x, 2 * TOL_BF16, "bf16 fused stem vs oracle (3 layers of rounding)")
    assert_close(fused, sep, 2 * TOL_BF16, "bf16 fused stem vs separate bf16 launches")
    # whole net with the fused stem: logits vs the all-oracle bf16 forward, same bound as the unfused test
    net.set_fuse_stem(True)
    d_l = ctx.alloc(n * 20 * 4)
    net.forward(d_in.ptr, d_l.ptr, n)
    ctx.sync()
    full, _ = orc.net_forward(oplan, hw.blob, imgs, bf16=True)
    assert_close(d_l.download((n, 20), np.float32), np.asarray(full).reshape(n, 20), TOL_BF16_NET, "bf16 logits, fused stem")
    net.destroy()


@pytest.mark.parametrize("n", [7, 24])
def test_net_full_size_fused_equals_unfused(pkg, ctx, tmp_path, n):
    """BASELINE.json's full geometry (1.0x224, 1000 classes), batch 7 (ragged last row tile in every GEMM-shaped kernel) and 24: the default runner (fused stem + fused blocks
    4-11) and the one-launch-per-layer runner produce bit-identical logits; so does the uint8 front-end against the
    separate normalise pass. Size-independent property — no oracle run at this size."""
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, n)
    rng = np.random.default_rng(99)
    u8 = rng.integers(0, 256, (n, 224, 224, 3), dtype=np.uint8)
    d_u, d_f = ctx.to_device(u8), ctx.alloc(u8.size * 4)
    assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, d_f.ptr, d_u.ptr, u8.size, 1 / 127.5, -1.0, None) == 0
    d_a, d_b, d_c = ctx.alloc(n * 4000), ctx.alloc(n * 4000), ctx.alloc(n * 4000)
    assert [c for _, c in net.launches(n)][:5] == ([3, 2, 2, 2, 2] if n == 24 else [3, 2, 2, 1, 1])   # blocks 8, 10: from batch 11
    assert [c for _, c in net.launches(1)] == [3] + [1] * 26                                           # batch 1: only the stem
    net.forward(d_f.ptr, d_a.ptr, n)
    net.set_fuse_stem(False)
    net.set_fuse_blocks(0)
    assert len(net.launches(n)) == 29
    net.forward(d_f.ptr, d_b.ptr, n)
    net.set_fuse_stem(True)
    net.set_fuse_blocks(0xFFFFFFFE)                        # every block the kernel accepts (the 7x7 ones fall back)
    net.set_input_u8(True)
    net.forward(d_u.ptr, d_c.ptr, n)
    ctx.sync()
    a, b, c = (d.download((n, 1000), np.float32) for d in (d_a, d_b, d_c))
    assert np.isfinite(a).all() and float(np.abs(a).max()) > 0
    assert np.array_equal(a, b) and np.array_equal(a, c)
    net.destroy()


@pytest.mark.parametrize("shape", [(2, 112, 64, 128, 2), (2, 56, 128, 128, 1), (2, 56, 128, 256, 2), (2, 28, 256, 256, 1),
                                   (1, 28, 256, 512, 2), (3, 14, 64, 128, 1), (1, 6, 192, 384, 1), (2, 14, 512, 512, 1),
                                   (2, 40, 64, 64, 1), (3, 20, 64, 192, 2), (1, 14, 128, 320, 1), (5, 40, 64, 64, 1),    # round 5: Cout = 64 (mod 128) on a padded tile
                                   (2, 80, 32, 64, 2), (3, 24, 32, 128, 1), (1, 10, 32, 64, 1),                          # ... and Cin = 32: half a K chunk
                                   (105, 28, 32, 64, 1)])              # r6: Cin = 32 on the 256-row tile, stride 1, 322 tiles > one grid pass (the persistent-tile cursors)
def test_bf16_dwpw_fused(pkg, orc, ctx, shape):
    """mbn_dwpw_fused_bf16 vs the oracle's bf16 emulation of the pair (depthwise output rounded to bf16, bf16 pointwise
    filter, output rounded) and vs the two separate bf16 launches; bf16 tolerance (the pointwise summation order differs)."""
    _bf16_dwpw_fused_body(pkg, orc, ctx, shape)


@pytest.mark.parametrize("shape", [(3, 10, 10, 5), (600, 10, 10, 5), (2, 8, 8, 1), (5, 7, 9, 3), (1, 10, 10, 8), (4, 6, 6, 2), (3, 2, 16, 2), (2, 10, 9, 2), (2, 1, 1, 3),
                                   (2, 6, 16, 2)])
def test_bf16_blocks_resident(pkg, orc, ctx, shape):
    """Round 6: mbn_blocks_resident_bf16 (mbn_bf16_res.hip): a run of 256 -> 256 depthwise + pointwise blocks on a small map in one launch, the map
    resident in LDS — against the oracle's bf16 emulation of the chain (every layer output rounded to bf16) and against the same blocks issued one by
    one through mbn_dwpw_fused_bf16 (layers 14-23 of the 0.5x160 network: MobileNet.c:322-2599 pairs; kernel.cl:62-92 + 94-114). bf16 tolerance per
    block, compounding over the run; odd map sides, one image per several passes of the grid (600 images > one workgroup per CU), wide short maps (16 columns: eight
    column pairs, the quarter-row jobs of waves 4-7 on four of them), a single pixel, the widest bordered map that fits (8 x 18 = 144 pixels)."""
    n, h, w, nblk = shape
    c = 256
    rng = np.random.default_rng(n + 7 * h + 13 * w + nblk)
    x = orc.bf16_round(rng.uniform(0, 4, (n, h, w, c)).astype(np.float32))
    params, dev = [], []
    for _ in range(nblk):
        wd = rng.normal(0, 0.5, (3, 3, c)).astype(np.float32)
        wp = orc.bf16_round(rng.normal(0, (2.0 / c) ** 0.5, (c, c)).astype(np.float32))
        s2, s3 = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32)
        b2, b3 = rng.normal(0, 0.1, c).astype(np.float32), rng.normal(0, 0.1, c).astype(np.float32)
        params.append((wd, s2, b2, wp, s3, b3))
        dev.append([ctx.to_device(wd), ctx.to_device(s2), ctx.to_device(b2), _bf16_dev(pkg, ctx, wp), ctx.to_device(s3), ctx.to_device(b3)])
    nref = min(n, 3)                                  # the oracle chain on the first images (and the last one) only: it is the slow part
    sel = list(range(nref)) + ([n - 1] if n > nref else [])
    want = x[sel].copy()
    for wd, s2, b2, wp, s3, b3 in params:
        mid = orc.bf16_round(orc.f32_depthwise(want, wd, s2, b2, 1, 2, pad_top=1, pad_left=1))
        want = orc.bf16_round(orc.f32_pointwise(mid.reshape(-1, c), wp, s3, b3, 2).reshape(want.shape))
    d_x = _bf16_dev(pkg, ctx, x)
    d_o, d_p, d_q = ctx.alloc(x.size * 2 + 64), ctx.alloc(x.size * 2), ctx.alloc(x.size * 2)
    ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, x.size * 2 + 64)
    arr = (pkg.BlockParams * nblk)()
    for i, d in enumerate(dev):
        arr[i].wd, arr[i].s2, arr[i].b2, arr[i].wp_bf16, arr[i].s3, arr[i].b3 = (t.ptr for t in d)
    rc = ctx.lib.mbn_blocks_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, nblk, n, h, w, c, None)
    assert rc == 0, rc
    src, dst = d_x, d_p
    for d in dev:                                      # the same run, block by block
        rc = ctx.lib.mbn_dwpw_fused_bf16(ctx.h, dst.ptr, src.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[5].ptr, n, h, w, h, w, c, c, 1, 1, 1, None)
        if rc == pkg.EUNSUPPORTED:                     # odd widths are outside the block kernel's envelope: the oracle alone checks those
            src = None
            break
        assert rc == 0, rc
        src, dst = dst, (d_q if dst is d_p else d_p)
    ctx.sync()
    got = _bf16_get(pkg, d_o, (n, h, w, c))
    scale = max(float(np.abs(want).max()), 1e-3)
    err = float(np.abs(got[sel] - want).max()) / scale
    assert err <= TOL_BF16 * (1 + 0.5 * (nblk - 1)), "resident blocks %s vs oracle: %g" % (shape, err)
    if src is not None:
        ref = _bf16_get(pkg, src, (n, h, w, c))
        err2 = float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-3)
        assert err2 <= TOL_BF16 * (1 + 0.5 * (nblk - 1)), "resident blocks %s vs block-by-block: %g" % (shape, err2)
    tail = d_o.download((x.size + 32,), np.uint16)[x.size:]
    assert (tail == 0xFFFF).all(), "resident blocks stored past the output"
    # outside the envelope: MBN_EUNSUPPORTED, never a launch
    assert ctx.lib.mbn_blocks_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, nblk, n, 12, 12, c, None) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_blocks_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, nblk, n, h, w, 128, None) == pkg.EUNSUPPORTED


@pytest.mark.parametrize("shape", [(3, 10, 10), (600, 10, 10), (2, 8, 8), (5, 6, 10), (1, 2, 2), (4, 10, 4)])
def test_bf16_tail_resident(pkg, orc, ctx, shape):
    """Round 6: mbn_tail_resident_bf16 (mbn_bf16_tail.hip): depthwise stride 2 (256 ch) -> pointwise 256 -> 512 -> depthwise stride 1 -> pointwise 512 -> 512 ->
    global average pool in one launch, an image's maps resident in LDS (layers 24-28 of the 0.5x160 network: MobileNet.c:322-2599 pairs + the pool launch
    :2601-2679; kernel.cl:62-92, 94-114, 116-132) — against the oracle's bf16 emulation of the five layers (every layer output rounded to bf16) and against the
    same five layers issued one by one through mbn_depthwise / mbn_pointwise / mbn_pool. bf16 tolerance compounding over the four conv layers; ragged
    batches (600 images > one workgroup per CU), non-square and tiny maps; nothing stored past the output; outside the envelope MBN_EUNSUPPORTED."""
    n, h, w = shape
    c0, c1 = 256, 512
    h1, w1 = h // 2, w // 2
    rng = np.random.default_rng(n + 7 * h + 13 * w)
    x = orc.bf16_round(rng.uniform(0, 4, (n, h, w, c0)).astype(np.float32))
    P = []
    for ci in (c0, c1):
        wd = rng.normal(0, 0.5, (3, 3, ci)).astype(np.float32)
        wp = orc.bf16_round(rng.normal(0, (2.0 / ci) ** 0.5, (c1, ci)).astype(np.float32))
        s2, s3 = rng.uniform(0.5, 1.5, ci).astype(np.float32), rng.uniform(0.5, 1.5, c1).astype(np.float32)
        b2, b3 = rng.normal(0, 0.1, ci).astype(np.float32), rng.normal(0, 0.1, c1).astype(np.float32)
        P.append((wd, s2, b2, wp, s3, b3))
    dev = [[ctx.to_device(p[0]), ctx.to_device(p[1]), ctx.to_device(p[2]), _bf16_dev(pkg, ctx, p[3]), ctx.to_device(p[4]), ctx.to_device(p[5])] for p in P]
    sel = list(range(min(n, 3))) + ([n - 1] if n > 3 else [])
    t = x[sel]
    t = orc.bf16_round(orc.f32_depthwise(t, P[0][0], P[0][1], P[0][2], 2, 2, pad_top=0, pad_left=0))
    assert t.shape[1:3] == (h1, w1)
    t = orc.bf16_round(orc.f32_pointwise(t.reshape(-1, c0), P[0][3], P[0][4], P[0][5], 2).reshape(len(sel), h1, w1, c1))
    t = orc.bf16_round(orc.f32_depthwise(t, P[1][0], P[1][1], P[1][2], 1, 2, pad_top=1, pad_left=1))
    t = orc.bf16_round(orc.f32_pointwise(t.reshape(-1, c1), P[1][3], P[1][4], P[1][5], 2).reshape(len(sel), h1, w1, c1))
    if h1 == w1:
        want = orc.bf16_round(orc.f32_pool(t).reshape(len(sel), c1))
    else:                                              # the oracle's pool window is square (kernel.cl:116-132): the whole-map mean by hand, same left-to-right fp32 sum
        acc = np.zeros((len(sel), c1), np.float32)
        for px in t.reshape(len(sel), h1 * w1, c1).transpose(1, 0, 2):
            acc = (acc + px).astype(np.float32)
        want = orc.bf16_round((acc / np.float32(h1 * w1)).astype(np.float32))
    d_x = _bf16_dev(pkg, ctx, x)
    d_o = ctx.alloc(n * c1 * 2 + 64)
    ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, n * c1 * 2 + 64)
    arr = (pkg.BlockParams * 2)()
    for i, d in enumerate(dev):
        arr[i].wd, arr[i].s2, arr[i].b2, arr[i].wp_bf16, arr[i].s3, arr[i].b3 = (q.ptr for q in d)
    rc = ctx.lib.mbn_tail_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, n, h, w, c0, c1, None)
    assert rc == 0, rc
    ctx.sync()
    got = _bf16_get(pkg, d_o, (n, c1))
    scale = max(float(np.abs(want).max()), 1e-3)
    err = float(np.abs(got[sel] - want).max()) / scale
    assert err <= TOL_BF16 * 2.5, "resident tail %s vs oracle: %g" % (shape, err)
    tail = d_o.download((n * c1 + 32,), np.uint16)[n * c1:]
    assert (tail == 0xFFFF).all(), "resident tail stored past the output"
    # the same five layers one by one (square maps: mbn_pool's window is filtersize x filtersize)
    d_a, d_b = ctx.alloc(n * h * w * c1 * 2), ctx.alloc(n * h * w * c1 * 2)
    if h1 != w1:
        for d in dev:
            for q in d:
                q.free()
        for q in (d_x, d_o, d_a, d_b):
            q.free()
        return
    e = lambda d, **kw: pkg.make_ext(batch=n, dtype=pkg.DT_BF16, act=2, scale=d[0].ptr, shift=d[1].ptr, **kw)
    ctx.depthwise(d_a.ptr, d_x.ptr, dev[0][0].ptr, h1, w1, 3, 2, c0, e(dev[0][1:3], pad_top=0, pad_left=0, in_rows=h, in_cols=w))
    ctx.pointwise(d_b.ptr, d_a.ptr, dev[0][3].ptr, h1, w1, c0, c1, e(dev[0][4:6]))
    ctx.depthwise(d_a.ptr, d_b.ptr, dev[1][0].ptr, h1, w1, 3, 1, c1, e(dev[1][1:3], pad_top=1, pad_left=1, in_rows=h1, in_cols=w1))
    ctx.pointwise(d_b.ptr, d_a.ptr, dev[1][3].ptr, h1, w1, c1, c1, e(dev[1][4:6]))
    ctx.pool(d_a.ptr, d_b.ptr, h1, w1, h1, c1, pkg.make_ext(batch=n, dtype=pkg.DT_BF16, act=0))
    ctx.sync()
    ref = _bf16_get(pkg, d_a, (n, c1))
    err2 = float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-3)
    assert err2 <= TOL_BF16 * 2.5, "resident tail %s vs the five launches: %g" % (shape, err2)
    assert ctx.lib.mbn_tail_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, n, 12, 12, c0, c1, None) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_tail_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, n, 9, 10, c0, c1, None) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_tail_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, n, h, w, 128, 256, None) == pkg.EUNSUPPORTED
    for d in dev:
        for q in d:
            q.free()
    for q in (d_x, d_o, d_a, d_b):
        q.free()


@pytest.mark.parametrize("shape", [(2, 112, 64, 128, 2), (2, 56, 128, 128, 1), (2, 56, 128, 256, 2), (2, 28, 256, 256, 1), (3, 14, 64, 128, 1)])
def test_bf16_dwpw_fused_16x16x32_form(pkg, orc, ctx, shape):
    """LAB (misc = 32): the same block kernel with its pointwise products on v_mfma_f32_16x16x32_bf16 (round 4; measured equal to the shipped
    32x32x16 form, profiles/r04/c_bf16_mfma_shape_blocks.txt): same checks, the exact-integer part pins its lane maps and channel pairing."""
    _tune_lab(ctx, b"misc", 32)
    try:
        _bf16_dwpw_fused_body(pkg, orc, ctx, shape)
    finally:
        ctx.lib.mbn_tune_set(b"misc", 0)


def _bf16_dwpw_fused_body(pkg, orc, ctx, shape):
    n, h, cin, cout, stride = shape
    rng = np.random.default_rng(h * 13 + cin + cout + stride)
    x = orc.bf16_round(rng.uniform(0, 4, (n, h, h, cin)).astype(np.float32))
    wd = rng.normal(0, 0.5, (3, 3, cin)).astype(np.float32)
    wp = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32))
    s2, s3 = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b2, b3 = rng.normal(0, 0.1, cin).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    oh = (h + stride - 1) // stride
    pad = max((oh - 1) * stride + 3 - h, 0) // 2
    mid = orc.bf16_round(orc.f32_depthwise(x, wd, s2, b2, stride, 2, pad_top=pad, pad_left=pad))
    want = orc.bf16_round(orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(n, oh, oh, cout))
    d_x, d_wp = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, wp)
    d = [ctx.to_device(a) for a in (wd, s2, b2, s3, b3)]
    d_f, d_m, d_u = ctx.alloc(want.size * 2), ctx.alloc(mid.size * 2), ctx.alloc(want.size * 2)
    rc = ctx.lib.mbn_dwpw_fused_bf16(ctx.h, d_f.ptr, d_x.ptr, d[0].ptr, d[1].ptr, d[2].ptr, d_wp.ptr, d[3].ptr, d[4].ptr,
                                     n, h, h, oh, oh, cin, cout, stride, pad, pad, None)
    assert rc == 0, rc
    ctx.depthwise(d_m.ptr, d_x.ptr, d[0].ptr, oh, oh, 3, stride, cin,
                  pkg.make_ext(batch=n, dtype=pkg.DT_BF16, act=2, pad_top=pad, pad_left=pad, in_rows=h, in_cols=h, scale=d[1].ptr, shift=d[2].ptr))
    ctx.pointwise(d_u.ptr, d_m.ptr, d_wp.ptr, n * oh * oh, 1, cin, cout, pkg.make_ext(batch=1, dtype=pkg.DT_BF16, act=2, scale=d[3].ptr, shift=d[4].ptr))
    ctx.sync()
    fused, sep = _bf16_get(pkg, d_f, want.shape), _bf16_get(pkg, d_u, want.shape)
    assert_close(fused, want, TOL_BF16, "bf16 fused block %s vs oracle" % (shape,))
    assert_close(fused, sep, TOL_BF16, "bf16 fused block %s vs separate launches" % (shape,))
    # exact small integers: a centre-tap depthwise filter with
    # identity BN hands the window's centre pixel through, an asymmetric integer pointwise filter then makes every output an exact small
    # integer — any mix-up of the operand lane maps (k = 32 kg + 8 q), of the 16 x 16 C/D map or of the channel pairing across LDS blocks
    # j and j + 2 shows as a wrong integer
    xi = rng.integers(0, 4, (n, h, h, cin)).astype(np.float32)
    wdi = np.zeros((3, 3, cin), np.float32)
    wdi[1, 1, :] = 1.0
    wpi = rng.integers(-2, 3, (cout, cin)).astype(np.float32)
    wpi[:, 0] = np.arange(cout) % 5
    wpi[:, cin - 1] = np.arange(cout) % 3
    one2, zero2, one3, zero3 = (ctx.to_device(a) for a in (np.ones(cin, np.float32), np.zeros(cin, np.float32), np.ones(cout, np.float32), np.zeros(cout, np.float32)))
    d_xi, d_wdi, d_wpi = _bf16_dev(pkg, ctx, xi), ctx.to_device(wdi), _bf16_dev(pkg, ctx, wpi)
    rc = ctx.lib.mbn_dwpw_fused_bf16(ctx.h, d_f.ptr, d_xi.ptr, d_wdi.ptr, one2.ptr, zero2.ptr, d_wpi.ptr, one3.ptr, zero3.ptr,
                                     n, h, h, oh, oh, cin, cout, stride, pad, pad, None)
    assert rc == 0, rc
    ctx.sync()
    midi = orc.f32_depthwise(xi, wdi, np.ones(cin, np.float32), np.zeros(cin, np.float32), stride, 2, pad_top=pad, pad_left=pad)
    wanti = np.clip(midi.reshape(-1, cin).astype(np.float64) @ wpi.astype(np.float64).T, 0, 6).reshape(n, oh, oh, cout)
    assert np.array_equal(_bf16_get(pkg, d_f, want.shape).astype(np.float64), wanti), "bf16 fused block %s: exact integers" % (shape,)
    for b in (one2, zero2, one3, zero3, d_xi, d_wdi, d_wpi):
        b.free()


# =========================================================================== headline workloads

def _headline_images(n, res, seed):
    """Seeded U[-1,1) batch generated in slices (a 512 x 224 x 224 x 3 float64 temporary is avoided)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, res, res, 3), np.float32)
    for i in range(0, n, 64):
        out[i:i + 64] = rng.random((min(64, n - i), res, res, 3), dtype=np.float32) * 2.0 - 1.0
    return out


def _emul_modes(ctx, form, tile):
    assert ctx.lib.mbn_tune_set(b"pw_splitk", 1) == 0
    assert ctx.lib.mbn_tune_set(b"pw_emul", form) == 0
    assert ctx.lib.mbn_tune_set(b"pw_tile", tile) == 0


def _emul_reset(ctx):
    for k in (b"pw_splitk", b"pw_emul", b"pw_tile"):
        assert ctx.lib.mbn_tune_set(k, 0) == 0


@pytest.mark.parametrize("form", [6, 9])
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20])
def test_f32_pointwise_emul_split_is_exact(pkg, ctx, form, tile):
    """mbn_f32_pw_x6.hip (opt-in, tune pw_emul = 6 | 9): every fp32 operand is split into three bf16 values that carry all 24
    bits. Proof on the device, for every tile instantiation: with one operand a (signed) power of two per row, the output is a
    single product x * 2^e, which the kernel must return BIT FOR BIT for x with random full 24-bit significands — once with the
    activations random (A split: h, m and l all needed) and once with the filter random (B split). Replaces the arithmetic of
    kernel.cl:94-114 for the pointwise call sites MobileNet.c:1218-2576."""
    if tile not in (6, 7, 11) and not _lab(ctx):
        pytest.skip("tile %d of the split GEMM is compiled into the lab build only (the dispatch takes 11, 6 and 7)" % tile)
    m, k, n = 517, 96, 200                      # ragged in m and n for every tile shape
    rng = np.random.default_rng(form * 100 + tile)

    def full24(shape):
        bits = rng.integers(0, 1 << 23, shape, dtype=np.uint32) | (rng.integers(120, 134, shape, dtype=np.uint32) << 23)
        bits |= rng.integers(0, 2, shape, dtype=np.uint32) << 31
        return bits.view(np.float32)

    ext = pkg.make_ext(batch=1, act=0)
    d_o = ctx.alloc(m * n * 4)
    try:
        _emul_modes(ctx, form, tile)
        # activations random, filter one-hot powers of two
        x = full24((m, k))
        f = np.zeros((n, k), np.float32)
        kk = (np.arange(n) * 7) % k
        f[np.arange(n), kk] = (2.0 ** ((np.arange(n) % 5) - 2)) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
        d_x, d_f = ctx.to_device(x), ctx.to_device(f)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, k, n, ext)
        ctx.sync()
        want = x[:, kk] * f[np.arange(n), kk][None, :]
        assert np.array_equal(d_o.download((m, n), np.float32).view(np.uint32), want.view(np.uint32)), "A split loses bits"
        # filter random, activations one-hot powers of two
        x = np.zeros((m, k), np.float32)
        km = (np.arange(m) * 5) % k
        x[np.arange(m), km] = 2.0 ** (np.arange(m) % 3)
        f = full24((n, k))
        d_x.upload(x); d_f.upload(f)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, k, n, ext)
        ctx.sync()
        want = f[:, km].T * x[np.arange(m), km][:, None]
        assert np.array_equal(d_o.download((m, n), np.float32).view(np.uint32), want.view(np.uint32)), "B split loses bits"
    finally:
        _emul_reset(ctx)


@pytest.mark.parametrize("shape", [(4099, 512, 512), (1000, 96, 200), (777, 32, 64), (1500, 1024, 1000), (6272, 256, 256)])
def test_f32_pointwise_emul_accuracy(pkg, orc, ctx, shape):
    """pw_emul = 6 and 9 against (a) the oracle's pointwise + BN + ReLU6 at the fp32 pointwise tolerance, (b) a float64
    product of the same fp32 operands, in units of sum_k |a_k b_k| * 2^-24: the bound is the one the fp32 MFMA kernel itself
    is held to here (16 units; it measures 4-8) and the split forms may not be worse than 1.5x the fp32 kernel's own maximum
    on the same data (measured: equal or smaller, profiles/r02/m_pw_emul.txt). No stores past a ragged last tile; repeatable;
    a K outside the envelope (K % 32 != 0) falls through to the default kernel, bit for bit."""
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin + cout)
    x = np.clip(rng.normal(1.0, 1.5, (m, cin)), 0, 6).astype(np.float32)
    f = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    want = orc.f32_pointwise(x, f, sc, sh, 2)
    ref = x.astype(np.float64) @ f.astype(np.float64).T
    unit = (np.abs(x).astype(np.float64) @ np.abs(f).astype(np.float64).T) * 2.0 ** -24
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    d_o = ctx.alloc(want.nbytes + 64)
    ext_bn = pkg.make_ext(batch=1, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    ext_raw = pkg.make_ext(batch=1, act=0)
    worst = {}
    try:
        for form in (0, 6, 9):
            _emul_modes(ctx, form, 0 if form == 0 else (11 if cout >= 128 else 7))     # the two shipped kernels
            ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, want.nbytes + 64)
            ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext_bn)
            ctx.sync()
            raw = d_o.download((want.size + 16,), np.float32)
            assert np.all(raw[want.size:].view(np.uint32) == 0xFFFFFFFF), "stores past the ragged last tile (form %d)" % form
            got = raw[:want.size].reshape(want.shape)
            assert_close(got, want, TOL_PW, "pw_emul %d %s vs oracle" % (form, shape))
            ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext_bn)
            ctx.sync()
            assert np.array_equal(got, d_o.download(want.shape, np.float32)), "not repeatable"
            ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext_raw)
            ctx.sync()
            e = np.abs(d_o.download(want.shape, np.float32).astype(np.float64) - ref) / unit
            worst[form] = float(e.max())
            assert worst[form] <= 16.0, "form %d: %.2f units of the magnitude sum's fp32 rounding" % (form, worst[form])
        assert worst[6] <= 1.5 * worst[0] + 1.0 and worst[9] <= 1.5 * worst[0] + 1.0, worst
        # outside the envelope: K = 40 -> the default kernel answers, whatever pw_emul says
        xs = rng.uniform(0, 6, (m, 40)).astype(np.float32)
        fs = rng.normal(0, 0.2, (cout, 40)).astype(np.float32)
        d_xs, d_fs = ctx.to_device(xs), ctx.to_device(fs)
        outs = []
        for form in (0, 6):
            _emul_modes(ctx, form, 0)
            ctx.pointwise(d_o.ptr, d_xs.ptr, d_fs.ptr, m, 1, 40, cout, ext_bn)
            ctx.sync()
            outs.append(d_o.download(want.shape, np.float32))
        assert np.array_equal(outs[0], outs[1])
    finally:
        _emul_reset(ctx)


def test_f32_pointwise_emul_static_images(pkg, ctx):
    """pw_emul_static = 1: a filter's pre-split image is built once and reused — and rebuilt after the filter was rewritten through
    mbn_upload (the library sees its own writes). Results equal the per-call-split mode bit for bit, before and after the
    rewrite; a second context-owned filter at another pointer is unaffected."""
    m, k, n = 4099, 256, 256
    rng = np.random.default_rng(5)
    x = rng.uniform(0, 6, (m, k)).astype(np.float32)
    f1 = rng.normal(0, 0.1, (n, k)).astype(np.float32)
    f2 = rng.normal(0, 0.1, (n, k)).astype(np.float32)
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f1), ctx.alloc(m * n * 4)
    ext = pkg.make_ext(batch=1, act=0)

    def run():
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, k, n, ext)
        ctx.sync()
        return d_o.download((m, n), np.float32)
    try:
        _emul_modes(ctx, 6, 11)
        ref1 = run()                                            # per-call split
        assert ctx.lib.mbn_tune_set(b"pw_emul_static", 1) == 0
        assert np.array_equal(run(), ref1) and np.array_equal(run(), ref1)     # built, then reused
        d_f.upload(f2)                                           # mbn_upload: the image of this filter is stale from here
        got2 = run()
        assert ctx.lib.mbn_tune_set(b"pw_emul_static", 0) == 0
        ref2 = run()
        assert np.array_equal(got2, ref2) and not np.array_equal(ref2, ref1)
        want = x.astype(np.float64) @ f2.astype(np.float64).T
        assert_close(ref2, want.astype(np.float32), TOL_PW, "after the filter was rewritten")
    finally:
        ctx.lib.mbn_tune_set(b"pw_emul_static", 0)
        _emul_reset(ctx)


def test_headline_fp32_batch256_pw_emul(pkg, orc, ctx, tmp_path):
    """The opt-in split form on the headline configuration (1.0x224 fp32, batch 256, default runner): with pw_emul = 6 the
    stand-alone pointwise layers 13-27 run on mbn_f32_pw_x6.hip; logits of four images against the oracle at the SAME bound
    as the default path (TOL_NET), and against the default path's own logits."""
    n = 256
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, n)
    imgs = _headline_images(n, 224, 20261005)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 1000 * 4)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    base = d_out.download((n, 1000), np.float32)
    try:
        assert ctx.lib.mbn_tune_set(b"pw_emul", 6) == 0
        net.forward(d_in.ptr, d_out.ptr, n)
        ctx.sync()
        got = d_out.download((n, 1000), np.float32)
    finally:
        assert ctx.lib.mbn_tune_set(b"pw_emul", 0) == 0
    assert np.isfinite(got).all() and not np.array_equal(got, base), "the split kernel was not on the path"
    pick = [0, 85, 170, 255]
    oplan = orc.plan_build(1.0, 224, 1000)
    want, _ = orc.net_forward(oplan, hw.blob, imgs[pick], threads=orc.num_threads())
    want = np.asarray(want).reshape(len(pick), 1000)
    assert_close(got[pick], want, TOL_NET, "pw_emul 6, batch-256 logits of images %s" % pick)
    assert_close(got, base, 1e-4, "pw_emul 6 vs the fp32 MFMA path, all 256 images")
    assert (got.argmax(1) == base.argmax(1)).all()
    net.destroy()


def test_headline_fp32_batch256_vs_oracle(pkg, orc, ctx, tmp_path):
    """BASELINE.json configs[2] itself — MobileNet-V1 1.0x224 fp32, batch 256, the runner's DEFAULT configuration (fused
    stem, fused blocks, persistent GEMM tiles walking many tiles per workgroup) — checked for correctness, not just
    finiteness: logits of the first, two middle and the last image against the oracle run on those images alone
    (TOL_NET), and forward(256)[:24] == forward(24) bit for bit (tile and segment heuristics depend on the batch, the
    per-row arithmetic must not). Reference behaviour matched: the 29-layer sequence MobileNet.c:240-2763."""
    n = 256
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, n)
    imgs = _headline_images(n, 224, 20261004)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 1000 * 4)
    spans = [c for _, c in net.launches(n)]
    assert spans[0] == 3 and spans.count(2) >= 4, spans          # the fused kernels are on the path being checked
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    got = d_out.download((n, 1000), np.float32)
    assert np.isfinite(got).all()
    pick = [0, 85, 170, 255]
    oplan = orc.plan_build(1.0, 224, 1000)
    want, _ = orc.net_forward(oplan, hw.blob, imgs[pick], threads=orc.num_threads())
    assert_close(got[pick], np.asarray(want).reshape(len(pick), 1000), TOL_NET, "batch-256 logits of images %s" % pick)
    assert (got[pick].argmax(1) == np.asarray(want).reshape(len(pick), 1000).argmax(1)).all()
    d_small = ctx.alloc(24 * 1000 * 4)
    net.forward(d_in.ptr, d_small.ptr, 24)
    ctx.sync()
    assert np.array_equal(d_small.download((24, 1000), np.float32), got[:24])
    net.destroy()


@pytest.mark.parametrize("cfg", [(1.0, 224), (0.5, 160)])
def test_headline_bf16_batch512_vs_oracle(pkg, orc, ctx, tmp_path, cfg):
    """BASELINE.json configs[4]: bf16 storage, batch 512, at 1.0x224 and 0.5x160, default runner. Logits of four images
    spread over the batch against the oracle's bf16-emulating forward of those images alone (TOL_BF16_NET = 2e-2 of max|ref|; observed 4.6-5.2e-3: rounding
    flips accumulate over 28 layers, same bound as the small bf16 net tests), and batch-slot independence at full size:
    forward(512)[:16] == forward(16)."""
    alpha, res = cfg
    n = 512
    hw, net = _make_net(pkg, ctx, tmp_path, alpha, res, 1000, n)
    net.set_dtype(pkg.DT_BF16)
    imgs = _headline_images(n, res, 512 + res)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 1000 * 4)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    got = d_out.download((n, 1000), np.float32)
    assert np.isfinite(got).all()
    pick = [0, 170, 341, 511]
    oplan = orc.plan_build(alpha, res, 1000)
    want, _ = orc.net_forward(oplan, hw.blob, imgs[pick], threads=orc.num_threads(), bf16=True)
    assert_close(got[pick], np.asarray(want).reshape(len(pick), 1000), TOL_BF16_NET, "bf16 batch-512 logits %s" % (cfg,))
    d_small = ctx.alloc(16 * 1000 * 4)
    net.forward(d_in.ptr, d_small.ptr, 16)
    ctx.sync()
    assert np.array_equal(d_small.download((16, 1000), np.float32), got[:16])
    # round 6: at 0.5x160 the five 256 -> 256 blocks on the 10 x 10 map (layers 14-23) are ONE launch with the map resident in LDS (mbn_blocks_resident_bf16);
    # and layers 24-28 another (mbn_tail_resident_bf16); switched off they are launches per block / layer again, and the logits are the same bits (same arithmetic)
    spans = [c for _, c in net.launches(n)]
    if alpha == 0.5:
        assert 10 in spans and spans[-2:] == [5, 1], spans            # ... and layers 24-28 (two blocks + the pool) one resident launch, then the FC layer
        net.set_fuse_resident(False)
        assert max(c for _, c in net.launches(n)) <= 3
        net.forward(d_in.ptr, d_out.ptr, n)
        ctx.sync()
        assert np.array_equal(d_out.download((n, 1000), np.float32), got)
        net.set_fuse_resident(True)
    else:
        assert max(spans) <= 3, spans
    net.destroy()


def test_undersized_buffers_are_einval_not_faults(pkg, ctx):
    """The fault class on record from round 1 (gpurun_out/fault.log: the C host handed a 3*96*96*3-BYTE uint8 image to the
    fp32 first-layer kernel, which read 4x the buffer) is a caller error the ABI can see: every mbn_alloc buffer's size
    is known. An undersized input, output, filter or scale must come back as MBN_EINVAL with nothing launched."""
    n, res = 3, 96
    u8 = np.zeros((n, res, res, 3), np.uint8)
    d_img = ctx.to_device(u8)                                        # n*res*res*3 BYTES
    d_out = ctx.alloc(n * 48 * 48 * 8 * 4)
    d_w = ctx.to_device(np.zeros((3, 3, 3, 8), np.float32))
    ext = pkg.make_ext(batch=n, cin=3)
    rc = ctx.lib.mbn_convolute(ctx.h, d_out.ptr, d_img.ptr, None, None, d_w.ptr, res, res, 3, 2, 8, C.byref(ext))
    assert rc == pkg.EINVAL and b"convolute image" in ctx.lib.mbn_last_device_error(ctx.h)
    ext_u8 = pkg.make_ext(batch=n, cin=3, io_flags=pkg.IO_IN_U8)     # the same buffer IS right for the uint8 front-end
    assert ctx.lib.mbn_convolute(ctx.h, d_out.ptr, d_img.ptr, None, None, d_w.ptr, res, res, 3, 2, 8, C.byref(ext_u8)) == 0
    # output one image short; interior pointer whose remainder is too small; short filter; short scale
    x = ctx.to_device(np.zeros((2, 14, 14, 64), np.float32))
    w = ctx.to_device(np.zeros((128, 64), np.float32))
    o = ctx.alloc(1 * 14 * 14 * 128 * 4)
    e2 = pkg.make_ext(batch=2)
    assert ctx.lib.mbn_pointwise(ctx.h, o.ptr, x.ptr, w.ptr, 14, 14, 64, 128, C.byref(e2)) == pkg.EINVAL
    o2 = ctx.alloc(2 * 14 * 14 * 128 * 4)
    assert ctx.lib.mbn_pointwise(ctx.h, o2.ptr, x.ptr, w.ptr, 14, 14, 64, 128, C.byref(e2)) == 0
    assert ctx.lib.mbn_pointwise(ctx.h, o2.ptr + 4096, x.ptr, w.ptr, 14, 14, 64, 128, C.byref(e2)) == pkg.EINVAL
    assert ctx.lib.mbn_pointwise(ctx.h, o2.ptr, x.ptr, w.ptr, 14, 14, 64, 256, C.byref(e2)) == pkg.EINVAL   # filter 128x64, call says 256
    sc = ctx.to_device(np.ones(64, np.float32))
    e3 = pkg.make_ext(batch=2, scale=sc.ptr, shift=sc.ptr)
    assert ctx.lib.mbn_pointwise(ctx.h, o2.ptr, x.ptr, w.ptr, 14, 14, 64, 128, C.byref(e3)) == pkg.EINVAL   # 64 scales for 128 channels
    dwf = ctx.to_device(np.zeros((3, 3, 64), np.float32))
    assert ctx.lib.mbn_depthwise(ctx.h, o2.ptr, x.ptr, dwf.ptr, 14, 14, 3, 1, 64, C.byref(pkg.make_ext(batch=3))) == pkg.EINVAL
    assert ctx.lib.mbn_pool(ctx.h, o2.ptr, x.ptr, 14, 14, 14, 64, C.byref(pkg.make_ext(batch=4, act=0))) == pkg.EINVAL
    assert ctx.lib.mbn_upload(ctx.h, sc.ptr, u8.ctypes.data, 64 * 4 + 1) == pkg.EINVAL
    ctx.sync()                                                        # nothing faulted; the context is still usable
    # the whole-network runner inherits the guard through the layer calls: a logits buffer sized for half the batch
    plan = pkg.plan_build(0.25, 64, 10)
    blob = np.zeros(plan.blob_floats, np.float32)
    net = pkg.Net(ctx, plan, blob, 4)
    imgs = ctx.to_device(np.zeros((4, 64, 64, 3), np.float32))
    small = ctx.alloc(2 * 10 * 4)
    assert ctx.lib.mbn_net_forward(net.h, imgs.ptr, small.ptr, 4, 0) == pkg.EINVAL
    ok = ctx.alloc(4 * 10 * 4)
    assert ctx.lib.mbn_net_forward(net.h, imgs.ptr, ok.ptr, 4, 0) == 0
    ctx.sync()
    net.destroy()


def test_profile_scope_not_consumed_by_rejected_calls(pkg, ctx):
    """VERDICT r1 weak #13 / ADVICE: a call that returns MBN_EINVAL after validation must not take an event slot —
    mbn_profile_end then read a start event whose stop was never recorded."""
    x = ctx.to_device(np.zeros((1, 8, 8, 3), np.float32))
    w = ctx.to_device(np.zeros((3, 3, 3, 8), np.float32))
    o = ctx.alloc(4 * 4 * 8 * 4)
    ctx.profile_begin(4)
    lit = pkg.make_ext(dtype=pkg.DT_U8, quirks=0)
    assert ctx.lib.mbn_convolute(ctx.h, o.ptr, x.ptr, None, None, w.ptr, 8, 8, 3, 2, 8, C.byref(lit)) == pkg.EINVAL   # LITERAL needs g/b planes
    assert ctx.lib.mbn_convolute(ctx.h, o.ptr, x.ptr, None, None, w.ptr, 8, 8, 3, 2, 8, C.byref(pkg.make_ext(cin=3))) == 0
    ms = ctx.profile_end(4)
    assert len(ms) == 1 and ms[0] > 0


def test_step_markers(pkg, ctx):
    x = ctx.alloc(1 << 20)
    for _ in range(4):
        ctx.mark()
        assert ctx.lib.mbn_memset(ctx.h, x.ptr, 0, 1 << 20) == 0
    ctx.mark()
    ms = ctx.marks_read(16)
    assert len(ms) == 4 and all(m >= 0 for m in ms)
    assert ctx.marks_read(16) == []


def test_dist_single_gpu_path_and_c_host_gpus_mode(pkg, ctx, tmp_path):
    """Multi-GPU from C, exercised on the one GPU this box has: mbn_dist_init(1) hands out a context
    that behaves like mbn_init's, the broadcast is the identity for one rank, asking for more GPUs than exist is an error
    code, and `mobilenet --gpus 1` runs the sharded-host code path end to end (the 8-GPU run is the driver's)."""
    import re
    import subprocess
    lib = ctx.lib
    d = C.c_void_p()
    have = C.c_int()
    assert lib.mbn_device_count(C.byref(have)) == 0 and have.value >= 1
    assert lib.mbn_dist_init(have.value + 1, None, C.byref(d)) == pkg.ENODEVICE
    assert lib.mbn_dist_init(0, None, C.byref(d)) == pkg.EINVAL
    assert lib.mbn_dist_init(1, None, C.byref(d)) == 0
    n = C.c_int()
    assert lib.mbn_dist_size(d, C.byref(n)) == 0 and n.value == 1
    c0 = C.c_void_p()
    assert lib.mbn_dist_context(d, 0, C.byref(c0)) == 0 and lib.mbn_dist_context(d, 1, C.byref(c0)) == pkg.EINVAL
    assert lib.mbn_dist_context(d, 0, C.byref(c0)) == 0
    buf = C.c_void_p()
    assert lib.mbn_alloc(c0, 4096, C.byref(buf)) == 0
    x = np.arange(1024, dtype=np.float32)
    assert lib.mbn_upload(c0, buf, x.ctypes.data, 4096) == 0
    ptrs = (C.c_void_p * 1)(buf.value)
    assert lib.mbn_dist_broadcast(d, ptrs, 4096, 0) == 0
    assert lib.mbn_dist_broadcast(d, ptrs, 4096, 1) == pkg.EINVAL
    y = np.empty_like(x)
    assert lib.mbn_download(c0, y.ctypes.data, buf, 4096) == 0 and np.array_equal(x, y)
    assert lib.mbn_dist_sync(d) == 0 and lib.mbn_dist_shutdown(d) == 0
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    out = subprocess.run([exe, "--gpus", "1", "--batch", "5", "--synthetic", "3", "--alpha", "0.25", "--res", "96",
                          "--steps", "3", "--warmup", "1", "--verify"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    # per-shard checksum of the logits, and --verify: the shard replayed on GPU 0 is bit-identical (here the shard's GPU is GPU 0)
    ck = re.search(r"logits fnv1a ([0-9a-f]{16})", out.stdout)
    vf = re.search(r"verify: shard 0 \(GPU 0\) vs the same images on GPU 0: identical \(fnv1a ([0-9a-f]{16})\)", out.stdout)
    assert ck and vf and ck.group(1) == vf.group(1), out.stdout
    m = re.search(r"GPU 0: images \[0, 5\) 3 steps in ([0-9.]+) s; first image -> class (\d+)", out.stdout)
    assert m and 1 <= int(m.group(2)) <= 1000, out.stdout
    m = re.search(r"1 GPUs, batch 5 .* ([0-9.]+) images/sec", out.stdout)
    assert m and float(m.group(1)) > 0, out.stdout
    # --streams 2: each GPU's shard as two free-running sub-batch streams (12 images: sub-batches of 6, forked) -> same class
    runs = []
    for extra in ([], ["--streams", "2"]):
        out = subprocess.run([exe, "--gpus", "1", "--batch", "12", "--synthetic", "3", "--alpha", "0.25", "--res", "96",
                              "--steps", "3", "--warmup", "1"] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        runs.append(re.search(r"first image -> class (\d+)", out.stdout).group(1))
    assert runs[0] == runs[1]
    # asking the host for more GPUs than the box has fails cleanly
    out = subprocess.run([exe, "--gpus", str(have.value + 1), "--batch", "8", "--synthetic", "3", "--alpha", "0.25", "--res", "64"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and "mbn_dist_init" in out.stderr and "no HIP device" in out.stderr      # MBN_ENODEVICE, not a hang


def test_dist_rccl_path_rehearsed_on_one_gpu(pkg):
    """Round 4: the RCCL leg of the C multi-GPU path (csrc/mbn_dist.hip: dlopen of librccl, symbol binding, ncclCommInitAll, ONE grouped ncclBroadcast on
    the context's stream, sync, teardown) had never executed anywhere (one-GPU boxes). MBN_DIST_FORCE_RCCL=1 makes mbn_dist_init build the
    communicator for a single GPU as well, so everything except the xGMI transfer itself runs for real: `mobilenet --gpus 1 --verify` in a child process
    with that variable set must give the same logits checksum as without it, and say so in --verify."""
    import re
    import subprocess
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    args = [exe, "--gpus", "1", "--batch", "6", "--synthetic", "3", "--alpha", "0.25", "--res", "96", "--steps", "2", "--warmup", "1", "--verify"]
    sums = []
    for force in ("0", "1"):
        env = dict(os.environ, MBN_DIST_FORCE_RCCL=force, HSA_ENABLE_IPC_MODE_LEGACY="0")
        out = subprocess.run(args, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (force, out.stderr[-2000:], out.stdout[-500:])
        ck = re.search(r"logits fnv1a ([0-9a-f]{16})", out.stdout)
        assert ck and "identical" in out.stdout, out.stdout
        sums.append(ck.group(1))
    assert sums[0] == sums[1]


def test_bench_rccl_collectives_rehearsed_with_one_rank(pkg):
    """The torch.distributed leg of bench.py over the real "nccl" (= RCCL) backend had never run (one-GPU boxes): with MBN_DIST_FORCE_PG=1 a single rank
    joins a process group and runs the blob broadcast, the barriers and the MAX all-reduce through RCCL for real. The line must be the N = 1 line
    (cpu_baseline off here for time) with a passing parity check."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(MBN_DIST_FORCE_PG="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(pkg.REPO_ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--batch", "16", "--alpha", "0.5", "--res", "96",
           "--no-configs-alt", "--no-cpu-variants", "--no-unfused-stages", "--no-pw-emul-alt"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.splitlines()[-1])                         # the LAST stdout line is the record
    assert len(r.stdout.splitlines()[-1]) < 6000
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["parity_check"]["ok"]
    # one rank in a real RCCL group: the line proves it
    assert out["collective_world_size"] == 1 and out["backend"] == "nccl" and len(out["ranks"]) == 1 and out["ranks"][0][2].count(":") == 2


def test_bench_dump_outputs_repeat_run_for_run(pkg, tmp_path):
    """bench.py --dump-outputs DIR: after exactly --steps timed steps the logits the last one left on the device land in DIR/logits.npy
    (float32, [batch, 1000], finite), the line's ms_per_step covers those steps, and a second run with the same arguments (seeded images
    and weights) dumps the same logits bit for bit."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    dumps = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        cmd = [sys.executable, os.path.join(pkg.REPO_ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16", "--alpha", "0.5",
               "--res", "96", "--no-configs-alt", "--no-cpu-baseline", "--no-unfused-stages", "--no-pw-emul-alt", "--no-power",
               "--record", str(tmp_path / ("full%d.json" % i)), "--dump-outputs", str(d)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads(r.stdout.splitlines()[-1])
        assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
        full = json.load(open(tmp_path / ("full%d.json" % i)))         # unrounded: value = batch / the time one timed step took
        assert full["steps"] == 3 and abs(full["value"] * full["ms_per_step"] * 1e-3 - 16) < 1e-6
        assert sorted(os.listdir(d)) == ["logits.npy"]
        got = np.load(d / "logits.npy")
        assert got.dtype == np.float32 and got.shape == (16, 1000) and np.isfinite(got).all() and np.abs(got).max() > 0
        dumps.append(got)
    assert np.array_equal(dumps[0], dumps[1])


def _lab(ctx):
    return ctx.lib.mbn_lab_build() == 1


def _tune_lab(ctx, key, value):
    """mbn_tune_set of a lab knob: skips the test on the shipped library (MBN_EUNSUPPORTED there by design)."""
    rc = ctx.lib.mbn_tune_set(key, value)
    if rc == -8:
        pytest.skip("lab knob %s: this is the shipped libmbn.so (run with MBN_LAB=1 for the lab build)" % key.decode())
    assert rc == 0, rc


@pytest.mark.parametrize("shape", [(1000, 128, 256), (512, 64, 128), (3 * 3136, 64, 128), (2 * 784 + 5, 256, 256), (50176, 512, 512),
                                   (8 * 49 * 4, 1024, 1024), (640, 192, 384), (100352, 512, 512), (25088, 512, 1024), (70001, 320, 640)])
def test_bf16_pointwise_stream_kernel(pkg, orc, ctx, shape):
    """mbn_bf16_pw_stream.hip (three activation + two filter LDS slots per workgroup, two workgroups per CU, counted vmcnt waits,
    flattened (tile, k-tile) sequence, out-of-range dummy DMA past the end): the default bf16 pointwise kernel for K % 64 == 0,
    N % 128 == 0. Against the oracle's bf16 emulation, and with exact small integers through an asymmetric filter and identity
    BN (operand maps, channel pairing, every slot of both rings: K/64 = 1, 2, 3, 4, 5, 8, 16 k-tiles per tile; ragged last row
    tile; one to seven tiles per workgroup so the sequence crosses tile boundaries and ends on every slot phase). With the lab
    build also bit for bit against the tiled pw_gemm<bf16> (pw_ring = 1) and round 2's ring kernel (pw_ring = 2): all three add
    the same 64-wide k-groups of exact bf16 products in the same order."""
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin + cout)
    x = orc.bf16_round(rng.uniform(-1, 1, (m, cin)))
    f = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)))
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    d_x, d_f, d_sc, d_sh = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, f), ctx.to_device(sc), ctx.to_device(sh)
    d_o, d_p = ctx.alloc(m * cout * 2 + 64), ctx.alloc(m * cout * 2)
    ext = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, m * cout * 2 + 64)
    if _lab(ctx):
        assert ctx.lib.mbn_tune_set(b"pw_ring", 4) == 0      # the streaming kernel on every eligible shape, not only where the dispatch takes it
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    raw = d_o.download((m * cout + 32,), np.uint16)
    assert np.all(raw[m * cout:] == 0xFFFF), "stores past the output"
    got = _bf16_get(pkg, d_o, (m, cout))
    if m * cin * cout <= 2e9:
        ref = orc.bf16_round(orc.f32_pointwise(x, f, sc, sh, 2))
        assert_close(got, ref, TOL_BF16, "stream %s vs oracle" % (shape,))
    else:                                                    # headline-size shapes: the oracle on rows spread over the matrix
        rows = np.unique(np.concatenate([np.arange(0, 256), np.arange(m - 300, m), rng.integers(0, m, 2000)]))
        ref = orc.bf16_round(orc.f32_pointwise(x[rows], f, sc, sh, 2))
        assert_close(got[rows], ref, TOL_BF16, "stream %s vs oracle (sampled rows)" % (shape,))
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    assert np.array_equal(got, _bf16_get(pkg, d_o, (m, cout))), "not repeatable"
    if _lab(ctx):
        try:
            for mode in (1, 2):
                assert ctx.lib.mbn_tune_set(b"pw_ring", mode) == 0
                ctx.pointwise(d_p.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
                ctx.sync()
                other = _bf16_get(pkg, d_p, (m, cout))
                assert np.array_equal(got, other), "stream vs pw_ring=%d %s: max diff %g" % (mode, shape, np.abs(got - other).max())
        finally:
            ctx.lib.mbn_tune_set(b"pw_ring", 4)
    # exact integers with an asymmetric filter and identity BN: any slot / operand / channel-pair mix-up shows
    xi = rng.integers(-3, 4, (m, cin)).astype(np.float32)
    fi = rng.integers(-2, 3, (cout, cin)).astype(np.float32)
    fi[:, 0] = np.arange(cout) % 5
    one, zero = ctx.to_device(np.ones(cout, np.float32)), ctx.to_device(np.zeros(cout, np.float32))
    d_x.upload(pkg.f32_to_bf16_bits(xi)); d_f.upload(pkg.f32_to_bf16_bits(fi))
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=one.ptr, shift=zero.ptr))
    ctx.sync()
    goti = _bf16_get(pkg, d_o, (m, cout))
    for lo in (0, max(0, m - 4096)):                         # the first and the last rows (the tail of every workgroup's sequence)
        want = np.clip(xi[lo:lo + 4096].astype(np.float64) @ fi.astype(np.float64).T, 0, 6)
        assert np.array_equal(goti[lo:lo + 4096].astype(np.float64), orc.bf16_round(want.astype(np.float32)).astype(np.float64))
    ctx.lib.mbn_tune_set(b"pw_ring", 0)
    for b in (d_x, d_f, d_sc, d_sh, d_o, d_p, one, zero):
        b.free()


@pytest.mark.parametrize("shape", [(4 * 196, 256, 256), (8 * 196 + 57, 256, 512), (16 * 196, 512, 512), (50176, 512, 512), (25088, 512, 1024),
                                   (6 * 196 - 1, 1024, 1024), (100352, 512, 512), (100352, 256, 512), (25088, 1024, 1024), (31 * 196 + 100, 512, 256)])
def test_bf16_pointwise_wide_kernel(pkg, orc, ctx, shape):
    """mbn_bf16_pw_wide.hip (196 x 256 tiles, filter from its packed image straight into registers, activations through a 3-slot LDS
    ring, DPP-paired 4-byte stores), taken for pointwise calls that carry IO_FILT_PACKED with K in {256, 512, 1024} and N % 256 == 0.
    Against the oracle's bf16 emulation (sampled rows at the headline sizes), repeatable, no store past the output or into rows of
    the next tile (canary + ragged M), exact small integers through an asymmetric filter (packing order, operand maps, channel
    pairing by DPP, both filter register sets, every ring slot, 1 to 8 tiles per workgroup), and bit for bit equal to the same call
    WITHOUT the flag (pw_gemm<bf16> / the streaming kernel: same k-order of the sums)."""
    _tune_lab(ctx, b"pw_ring", 6)                              # lab build only: the kernel is not part of the shipped library
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin + cout)
    x = orc.bf16_round(rng.uniform(-1, 1, (m, cin)))
    f = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)))
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    d_x, d_sc, d_sh = _bf16_dev(pkg, ctx, x), ctx.to_device(sc), ctx.to_device(sh)
    d_f, flag = pkg.packed_filter_dev(ctx, f)
    assert flag == pkg.IO_FILT_PACKED
    d_o, d_p = ctx.alloc(m * cout * 2 + 64), ctx.alloc(m * cout * 2)
    ext = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr, io_flags=flag)
    ext0 = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, m * cout * 2 + 64)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    raw = d_o.download((m * cout + 32,), np.uint16)
    assert np.all(raw[m * cout:] == 0xFFFF), "stores past the output"
    got = _bf16_get(pkg, d_o, (m, cout))
    assert np.isfinite(got).all()
    rows = np.arange(m) if m * cin * cout <= 2e9 else np.unique(np.concatenate([np.arange(0, 420), np.arange(m - 420, m), rng.integers(0, m, 2000)]))
    ref = orc.bf16_round(orc.f32_pointwise(x[rows], f, sc, sh, 2))
    assert_close(got[rows], ref, TOL_BF16, "wide %s vs oracle" % (shape,))
    ctx.lib.mbn_tune_set(b"pw_ring", 1)                                      # pw_gemm<bf16>: the same 32x32x16 sums (the default path takes 16x16x32 from K = 512 up)
    ctx.pointwise(d_p.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext0)
    ctx.sync()
    ctx.lib.mbn_tune_set(b"pw_ring", 6)
    other = _bf16_get(pkg, d_p, (m, cout))
    assert np.array_equal(got, other), "wide vs unpacked path %s: max diff %g" % (shape, np.abs(got - other).max())
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    assert np.array_equal(got, _bf16_get(pkg, d_o, (m, cout))), "not repeatable"
    # exact integers with an asymmetric filter and identity BN
    xi = rng.integers(-3, 4, (m, cin)).astype(np.float32)
    fi = rng.integers(-2, 3, (cout, cin)).astype(np.float32)
    fi[:, 0] = np.arange(cout) % 5
    fi[:, cin - 1] = np.arange(cout) % 3
    one, zero = ctx.to_device(np.ones(cout, np.float32)), ctx.to_device(np.zeros(cout, np.float32))
    d_x.upload(pkg.f32_to_bf16_bits(xi))
    d_fi, _ = pkg.packed_filter_dev(ctx, fi)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_fi.ptr, m, 1, cin, cout, pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=one.ptr, shift=zero.ptr, io_flags=flag))
    ctx.sync()
    goti = _bf16_get(pkg, d_o, (m, cout))
    for lo in (0, max(0, m - 4096)):
        want = np.clip(xi[lo:lo + 4096].astype(np.float64) @ fi.astype(np.float64).T, 0, 6)
        assert np.array_equal(goti[lo:lo + 4096].astype(np.float64), orc.bf16_round(want.astype(np.float32)).astype(np.float64))
    ctx.lib.mbn_tune_set(b"pw_ring", 0)
    for b in (d_x, d_f, d_fi, d_sc, d_sh, d_o, d_p, one, zero):
        b.free()


@pytest.mark.parametrize("shape", [(49, 1024, 1024), (196, 512, 512), (5, 512, 1024), (3 * 196 + 1, 512, 512), (12544, 1024, 1024),
                                   (196, 256, 512), (2 * 3136 + 5, 256, 256), (25600 + 77, 256, 512), (400, 256, 128)])
def test_bf16_pointwise_k256_up_is_one_kernel_at_every_m(pkg, orc, ctx, shape):
    """bf16 pointwise layers with K >= 256 (1.0x224: layers 13 ... 27; 0.5x160: 15 ... 27; round 3: K >= 512) run on the streaming kernel's
    16x16x32 form at EVERY M — one image or 512 — so that an image's result does not depend on the batch: against the oracle, the first rows
    of a call bit for bit equal to a call with those rows alone (M = 1, 49, 196 included: fewer rows than one tile), and — on this SHIPPED
    path, not a lab knob — exact small integers through an asymmetric filter (operand lane maps k = 32 kg + 8 q, the 16 x 16 C/D map, channel
    pairing across LDS blocks j and j + 2, ragged M)."""
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin + cout)
    x = orc.bf16_round(rng.uniform(-1, 1, (m, cin)))
    f = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)))
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    d_x, d_f, d_sc, d_sh = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, f), ctx.to_device(sc), ctx.to_device(sh)
    d_o = ctx.alloc(m * cout * 2 + 64)
    ext = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, m * cout * 2 + 64)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    raw = d_o.download((m * cout + 32,), np.uint16)
    assert np.all(raw[m * cout:] == 0xFFFF), "stores past the output"
    got = _bf16_get(pkg, d_o, (m, cout))
    assert_close(got, orc.bf16_round(orc.f32_pointwise(x, f, sc, sh, 2)), TOL_BF16, "K >= 512 %s vs oracle" % (shape,))
    for k in sorted({1, min(m, 49), min(m, 196)}):
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, k, 1, cin, cout, ext)
        ctx.sync()
        assert np.array_equal(_bf16_get(pkg, d_o, (k, cout)), got[:k]), "rows depend on M (%d of %d)" % (k, m)
    xi = rng.integers(-3, 4, (m, cin)).astype(np.float32)
    fi = rng.integers(-2, 3, (cout, cin)).astype(np.float32)
    fi[:, 0] = np.arange(cout) % 5
    fi[:, cin - 1] = np.arange(cout) % 3
    one, zero = ctx.to_device(np.ones(cout, np.float32)), ctx.to_device(np.zeros(cout, np.float32))
    d_x.upload(pkg.f32_to_bf16_bits(xi)); d_f.upload(pkg.f32_to_bf16_bits(fi))
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=one.ptr, shift=zero.ptr))
    ctx.sync()
    goti = _bf16_get(pkg, d_o, (m, cout))
    for lo in (0, max(0, m - 4096)):
        want = np.clip(xi[lo:lo + 4096].astype(np.float64) @ fi.astype(np.float64).T, 0, 6)
        assert np.array_equal(goti[lo:lo + 4096].astype(np.float64), orc.bf16_round(want.astype(np.float32)).astype(np.float64)), "exact integers %s" % (shape,)
    one.free(); zero.free()
    for b in (d_x, d_f, d_sc, d_sh, d_o):
        b.free()


@pytest.mark.parametrize("shape", [(1000, 128, 256), (3 * 3136, 64, 128), (50176, 512, 512), (8 * 49 * 4, 1024, 1024), (70001, 320, 640)])
def test_bf16_pointwise_stream_kernel_on_16x16x32_mfma(pkg, orc, ctx, shape):
    """LAB (misc=16): the streaming GEMM's products on v_mfma_f32_16x16x32_bf16 (the shape the chip holds a higher clock under): against the
    oracle's bf16 emulation, exact small integers through an asymmetric filter (operand lane maps, C/D map of the 16 x 16 blocks, channel
    pairing across blocks j and j + 2, ragged M), no store past the output, repeatable. Not bit-identical to the 32x32x16 kernels (32 products
    are summed per instruction instead of 16): compared at the bf16 tolerance."""
    _tune_lab(ctx, b"misc", 16)
    ctx.lib.mbn_tune_set(b"pw_ring", 4)
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin + cout)
    x = orc.bf16_round(rng.uniform(-1, 1, (m, cin)))
    f = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)))
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    d_x, d_f, d_sc, d_sh = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, f), ctx.to_device(sc), ctx.to_device(sh)
    d_o = ctx.alloc(m * cout * 2 + 64)
    ext = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    try:
        ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, m * cout * 2 + 64)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
        ctx.sync()
        raw = d_o.download((m * cout + 32,), np.uint16)
        assert np.all(raw[m * cout:] == 0xFFFF), "stores past the output"
        got = _bf16_get(pkg, d_o, (m, cout))
        rows = np.arange(m) if m * cin * cout <= 2e9 else np.unique(np.concatenate([np.arange(0, 300), np.arange(m - 300, m), rng.integers(0, m, 1500)]))
        assert_close(got[rows], orc.bf16_round(orc.f32_pointwise(x[rows], f, sc, sh, 2)), TOL_BF16, "16x16x32 %s vs oracle" % (shape,))
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
        ctx.sync()
        assert np.array_equal(got, _bf16_get(pkg, d_o, (m, cout))), "not repeatable"
        xi = rng.integers(-3, 4, (m, cin)).astype(np.float32)
        fi = rng.integers(-2, 3, (cout, cin)).astype(np.float32)
        fi[:, 0] = np.arange(cout) % 5
        fi[:, cin - 1] = np.arange(cout) % 3
        one, zero = ctx.to_device(np.ones(cout, np.float32)), ctx.to_device(np.zeros(cout, np.float32))
        d_x.upload(pkg.f32_to_bf16_bits(xi)); d_f.upload(pkg.f32_to_bf16_bits(fi))
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=one.ptr, shift=zero.ptr))
        ctx.sync()
        goti = _bf16_get(pkg, d_o, (m, cout))
        for lo in (0, max(0, m - 4096)):
            want = np.clip(xi[lo:lo + 4096].astype(np.float64) @ fi.astype(np.float64).T, 0, 6)
            assert np.array_equal(goti[lo:lo + 4096].astype(np.float64), orc.bf16_round(want.astype(np.float32)).astype(np.float64))
        one.free(); zero.free()
    finally:
        ctx.lib.mbn_tune_set(b"misc", 0)
        ctx.lib.mbn_tune_set(b"pw_ring", 0)
        for b in (d_x, d_f, d_sc, d_sh, d_o):
            b.free()


@pytest.mark.parametrize("shape", [(100352, 512, 512), (25088 + 5, 512, 1024), (31, 512, 256), (32 * 8 * 16 * 3 + 1, 512, 512), (7 * 32 + 3, 512, 768),
                                   (2 * 196, 512, 512), (65536 + 33, 512, 256)])
def test_bf16_pointwise_register_filter_kernel(pkg, orc, ctx, shape):
    """mbn_bf16_pw_rf.hip (round 6): K = 512 with the wave's filter rows in registers for the whole launch and only the activations through a four-stage
    LDS ring (one LDS-DMA per pixel row, counted vmcnt, out-of-range dummy DMA past the end). Against the oracle's bf16 emulation (sampled rows on the big
    shapes: first and last tiles included), no store past the output (ragged last tile: rows past M are dropped by the buffer range), repeatable, exact
    small integers through an asymmetric filter (A / B lane maps k = 32 g + 8 q, the 16 x 16 C/D map, every channel slice: N / 256 = 1, 2, 3, 4), fewer tiles
    than pixel streams, tile counts that end on every stage of the ring — and bit for bit the M16 streaming kernel it replaces on these layers (same
    instruction, same k order; pw_ring = 8 selects it, 5 the streaming kernel). LAB build only: measured equal to slower, not in the shipped library."""
    _tune_lab(ctx, b"pw_ring", 8)          # lab build only (skips on the shipped library): the kernel is measured, not taken
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin + cout)
    x = orc.bf16_round(rng.uniform(-1, 1, (m, cin)))
    f = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)))
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    d_x, d_f, d_sc, d_sh = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, f), ctx.to_device(sc), ctx.to_device(sh)
    d_o = ctx.alloc(m * cout * 2 + 64)
    ext = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    try:
        ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, m * cout * 2 + 64)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
        ctx.sync()
        raw = d_o.download((m * cout + 32,), np.uint16)
        assert np.all(raw[m * cout:] == 0xFFFF), "stores past the output"
        got = _bf16_get(pkg, d_o, (m, cout))
        rows = np.arange(m) if m * cin * cout <= 2e9 else np.unique(np.concatenate([np.arange(0, 300), np.arange(m - 300, m), rng.integers(0, m, 1500)]))
        assert_close(got[rows], orc.bf16_round(orc.f32_pointwise(x[rows], f, sc, sh, 2)), TOL_BF16, "register filter %s vs oracle" % (shape,))
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
        ctx.sync()
        assert np.array_equal(got, _bf16_get(pkg, d_o, (m, cout))), "not repeatable"
        if _lab(ctx):
            assert ctx.lib.mbn_tune_set(b"pw_ring", 5) == 0      # the M16 streaming kernel these layers ran on before
            ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
            ctx.sync()
            ref = _bf16_get(pkg, d_o, (m, cout))
            assert np.array_equal(got, ref), "not the streaming kernel's bits: %d of %d differ" % (int(np.sum(got != ref)), got.size)
            assert ctx.lib.mbn_tune_set(b"pw_ring", 8) == 0
        xi = rng.integers(-3, 4, (m, cin)).astype(np.float32)
        fi = rng.integers(-2, 3, (cout, cin)).astype(np.float32)
        fi[:, 0] = np.arange(cout) % 5
        fi[:, cin - 1] = np.arange(cout) % 3
        one, zero = ctx.to_device(np.ones(cout, np.float32)), ctx.to_device(np.zeros(cout, np.float32))
        d_x.upload(pkg.f32_to_bf16_bits(xi)); d_f.upload(pkg.f32_to_bf16_bits(fi))
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=one.ptr, shift=zero.ptr))
        ctx.sync()
        goti = _bf16_get(pkg, d_o, (m, cout))
        for lo in (0, max(0, m - 4096)):
            want = np.clip(xi[lo:lo + 4096].astype(np.float64) @ fi.astype(np.float64).T, 0, 6)
            assert np.array_equal(goti[lo:lo + 4096].astype(np.float64), orc.bf16_round(want.astype(np.float32)).astype(np.float64)), "exact integers %s" % (shape,)
        one.free(); zero.free()
    finally:
        ctx.lib.mbn_tune_set(b"pw_ring", 0)
        for b in (d_x, d_f, d_sc, d_sh, d_o):
            b.free()


@pytest.mark.parametrize("shape", [(100352, 512, 512), (100352 + 77, 256, 512), (66000, 128, 256), (131072 + 300, 1024, 256), (40000, 512, 1024)])
def test_bf16_pointwise_big_tile_kernel(pkg, orc, ctx, shape):
    """The 256 x 256 form of mbn_bf16_pw_stream.hip (16 waves, two LDS slots per operand, one workgroup per CU) for whole rounds of the
    persistent grid, the remaining rows through pw_gemm<bf16> in a second launch: against the oracle's bf16 emulation on sampled rows
    (first and last rows of both launches included), no store past the output, bit for bit equal to the default path (same k-order of
    the sums in every kernel), repeatable, and exact small integers through an asymmetric filter (operand maps, channel pairing, both
    slots of both rings, every wave's 64 x 64 block)."""
    _tune_lab(ctx, b"pw_ring", 7)
    m, cin, cout = shape
    rng = np.random.default_rng(m + cin + cout)
    x = orc.bf16_round(rng.uniform(-1, 1, (m, cin)))
    f = orc.bf16_round(rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)))
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    d_x, d_f, d_sc, d_sh = _bf16_dev(pkg, ctx, x), _bf16_dev(pkg, ctx, f), ctx.to_device(sc), ctx.to_device(sh)
    d_o, d_p = ctx.alloc(m * cout * 2 + 64), ctx.alloc(m * cout * 2)
    ext = pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, m * cout * 2 + 64)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    raw = d_o.download((m * cout + 32,), np.uint16)
    assert np.all(raw[m * cout:] == 0xFFFF), "stores past the output"
    got = _bf16_get(pkg, d_o, (m, cout))
    assert np.isfinite(got).all()
    tiles = (m // 256) * (cout // 256)
    split = (tiles // 256 * 256) // (cout // 256) * 256            # first row of the second launch
    assert 0 < split <= m
    rows = np.unique(np.concatenate([np.arange(0, 300), np.arange(max(0, split - 300), min(m, split + 300)), np.arange(m - 300, m), rng.integers(0, m, 1500)]))
    ref = orc.bf16_round(orc.f32_pointwise(x[rows], f, sc, sh, 2))
    assert_close(got[rows], ref, TOL_BF16, "big tile %s vs oracle" % (shape,))
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    assert np.array_equal(got, _bf16_get(pkg, d_o, (m, cout))), "not repeatable"
    ctx.lib.mbn_tune_set(b"pw_ring", 1)                         # pw_gemm<bf16> (the default path takes the 16x16x32 form from K = 512 up: other bits)
    ctx.pointwise(d_p.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
    ctx.sync()
    other = _bf16_get(pkg, d_p, (m, cout))
    assert np.array_equal(got, other), "big tile vs pw_gemm %s: max diff %g" % (shape, np.abs(got - other).max())
    _tune_lab(ctx, b"pw_ring", 7)
    xi = rng.integers(-3, 4, (m, cin)).astype(np.float32)
    fi = rng.integers(-2, 3, (cout, cin)).astype(np.float32)
    fi[:, 0] = np.arange(cout) % 5
    fi[:, cin - 1] = np.arange(cout) % 3
    one, zero = ctx.to_device(np.ones(cout, np.float32)), ctx.to_device(np.zeros(cout, np.float32))
    d_x.upload(pkg.f32_to_bf16_bits(xi))
    d_f.upload(pkg.f32_to_bf16_bits(fi))
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, pkg.make_ext(dtype=pkg.DT_BF16, act=2, scale=one.ptr, shift=zero.ptr))
    ctx.sync()
    goti = _bf16_get(pkg, d_o, (m, cout))
    for lo in (0, max(0, split - 2048), max(0, m - 4096)):
        want = np.clip(xi[lo:lo + 4096].astype(np.float64) @ fi.astype(np.float64).T, 0, 6)
        assert np.array_equal(goti[lo:lo + 4096].astype(np.float64), orc.bf16_round(want.astype(np.float32)).astype(np.float64))
    ctx.lib.mbn_tune_set(b"pw_ring", 0)
    for b in (d_x, d_f, d_sc, d_sh, d_o, d_p, one, zero):
        b.free()


@pytest.mark.parametrize("shape", [(196, 512, 512, 1), (49, 1024, 1024, 1), (4 * 196, 256, 512, 4), (3 * 49 , 512, 1024, 3), (1, 1024, 1000, 1),
                                   (4, 1024, 1000, 4), (2 * 25, 128, 256, 2), (37, 192, 40, 1), (100, 320, 72, 1), (2 * 81, 384, 104, 2)])
def test_f32_pointwise_splitk_kernel(pkg, orc, ctx, shape):
    """mbn_f32_pw_splitk.hip (1..4 images, few tiles: one 16x16 tile per workgroup, K split over its 4/8/16 waves, partial
    tiles summed in LDS in fixed order): against the oracle, against pw_gemm (tune pw_splitk=1) within the fp32 tolerance,
    bit-exactly on integer operands with an asymmetric filter (operand / C-D lane maps, k permutation, ragged rows and
    columns, every S and CH instantiation: K = 128, 192, 256, 320, 384, 512, 1024), and repeatably (no atomics)."""
    m, cin, cout, batch = shape
    rng = np.random.default_rng(m + cin + cout)
    x = rng.uniform(-1, 1, (m, cin)).astype(np.float32)
    f = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, cout).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    want = orc.f32_pointwise(x, f, sc, sh, 2)
    d_x, d_f, d_sc, d_sh = (ctx.to_device(a) for a in (x, f, sc, sh))
    d_o, d_p = ctx.alloc(want.nbytes + 64), ctx.alloc(want.nbytes)
    ext = pkg.make_ext(batch=batch, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    try:
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 2) == 0          # wherever the shape is eligible
        ctx.lib.mbn_memset(ctx.h, d_o.ptr, 0xFF, want.nbytes + 64)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m // batch, 1, cin, cout, ext)
        ctx.sync()
        raw = d_o.download((want.size + 16,), np.float32)
        assert np.all(raw[want.size:].view(np.uint32) == 0xFFFFFFFF), "stores past the ragged last tile"
        got = raw[:want.size].reshape(want.shape)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m // batch, 1, cin, cout, ext)
        ctx.sync()
        assert np.array_equal(got, d_o.download(want.shape, np.float32)), "not repeatable"
        for tw in (16, 32):                                        # both workgroup tiles: same split, same k map -> same bits
            assert ctx.lib.mbn_tune_set(b"pw_splitk", tw) == 0
            ctx.pointwise(d_p.ptr, d_x.ptr, d_f.ptr, m // batch, 1, cin, cout, ext)
            ctx.sync()
            assert np.array_equal(got, d_p.download(want.shape, np.float32)), "tile %d differs" % tw
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 1) == 0          # never
        ctx.pointwise(d_p.ptr, d_x.ptr, d_f.ptr, m // batch, 1, cin, cout, ext)
        ctx.sync()
        tiled = d_p.download(want.shape, np.float32)
        assert_close(got, want, TOL_PW, "split-K %s vs oracle" % (shape,))
        assert_close(got, tiled, TOL_PW, "split-K %s vs pw_gemm" % (shape,))
        # default mode: a call of 1..4 images of a layer with few tiles takes this kernel by itself -> same bits
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 0) == 0
        ctx.pointwise(d_p.ptr, d_x.ptr, d_f.ptr, m // batch, 1, cin, cout, ext)
        ctx.sync()
        dflt = d_p.download(want.shape, np.float32)
        assert np.array_equal(dflt, got) or np.array_equal(dflt, tiled)
        if -(-4 * (m // batch) // 64) * -(-cout // 64) * 2 <= 256:
            assert np.array_equal(dflt, got), "default dispatch did not take the split-K kernel"
        # exact integers, identity BN, no activation (FC form: scale NULL, bias as shift)
        assert ctx.lib.mbn_tune_set(b"pw_splitk", 2) == 0
        xi = rng.integers(-8, 9, (m, cin)).astype(np.float32)
        fi = rng.integers(-8, 9, (cout, cin)).astype(np.float32)
        fi[:, 0] += np.arange(cout) % 11
        fi[:, cin - 1] -= np.arange(cout) % 7
        bias = rng.integers(-50, 51, cout).astype(np.float32)
        d_x.upload(xi); d_f.upload(fi); d_sh.upload(bias)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m // batch, 1, cin, cout, pkg.make_ext(batch=batch, act=0, shift=d_sh.ptr))
        ctx.sync()
        wi = xi.astype(np.float64) @ fi.astype(np.float64).T + bias
        assert np.array_equal(d_o.download(want.shape, np.float32).astype(np.float64), wi)
        for tw in (16, 32):
            assert ctx.lib.mbn_tune_set(b"pw_splitk", tw) == 0          # wherever eligible, with the 16x16 / 32x32 workgroup tile forced
            ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m // batch, 1, cin, cout, pkg.make_ext(batch=batch, act=0, shift=d_sh.ptr))
            ctx.sync()
            assert np.array_equal(d_o.download(want.shape, np.float32).astype(np.float64), wi), "tile %d" % tw
    finally:
        ctx.lib.mbn_tune_set(b"pw_splitk", 0)
    for b in (d_x, d_f, d_sc, d_sh, d_o, d_p):
        b.free()


def test_net_free_running_streams_interleaved_with_single_stream(pkg, ctx, tmp_path):
    """bench.py's default schedule: free-running two-stream forwards (consecutive steps overlap across the step boundary)
    with a single-stream forward in between (the steps whose kernels are timed one by one), same buffers throughout, a
    changed batch, and changed input CONTENTS between forwards. Every forward must equal the plain single-stream result:
    the runner re-inserts the fork whenever the call differs from the previous multi-stream one or a single-stream
    forward came in between (the ping-pong activation buffers are shared)."""
    n = 12
    hw, net = _make_net(pkg, ctx, tmp_path, 0.5, 96, 30, n)
    rng = np.random.default_rng(17)
    a, b = (rng.uniform(-1, 1, (n, 96, 96, 3)).astype(np.float32) for _ in range(2))
    d_in, d_out = ctx.to_device(a), ctx.alloc(n * 30 * 4)
    def ref(x, k):
        net.set_streams(1)
        d_in.upload(x)
        net.forward(d_in.ptr, d_out.ptr, k)
        ctx.sync()
        return d_out.download((k, 30), np.float32)
    wa, wb, wa5 = ref(a, n), ref(b, n), ref(a, 5)
    d_in.upload(a)
    for rep in range(3):
        net.set_streams(2, free_running=True)
        for _ in range(4):
            net.forward(d_in.ptr, d_out.ptr, n)              # back to back: overlap across the step boundary
        net.set_streams(1)
        net.forward(d_in.ptr, d_out.ptr, n)                  # single-stream step in between
        net.set_streams(2, free_running=True)
        net.forward(d_in.ptr, d_out.ptr, n)
        ctx.sync()
        assert np.array_equal(d_out.download((n, 30), np.float32), wa)
        net.forward(d_in.ptr, d_out.ptr, 5)                  # another batch: other sub-batch slices of the shared buffers
        net.forward(d_in.ptr, d_out.ptr, n)
        ctx.sync()
        assert np.array_equal(d_out.download((n, 30), np.float32), wa)
    net.forward(d_in.ptr, d_out.ptr, 5)
    ctx.sync()
    assert np.array_equal(d_out.download((5, 30), np.float32), wa5)
    d_in.upload(b)                                           # blocking upload: the documented precondition of free-running
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    assert np.array_equal(d_out.download((n, 30), np.float32), wb)
    net.destroy()


@pytest.mark.parametrize("shape", [(14, 14, 32, 64, 1), (7, 7, 1024, 1024, 2), (9, 5, 30, 13, 1), (1, 1, 1024, 1000, 3), (28, 28, 130, 20, 1), (56, 56, 64, 128, 1)])
def test_literal_pointwise_on_dot4_is_bit_exact(pkg, orc, ctx, shape):
    """the reference's integer pointwise (kernel.cl:94-114, quirks off) on the packed-int8 units — v_mfma_i32_32x32x32_i8 (round 5, the default
    where Cin and Cout >= 16) and v_dot4_i32_i8 (tune lit_dot=2; the default for the narrower shapes) — bit-exact against the oracle and against the scalar
    LITERAL kernel (lit_dot=1): random int8-range filters incl. the extremes -128 / 127, activations over the whole uint8 range (the x - 128 re-centring and its
    128 * sum(w) correction), Cin not a multiple of 4 / 32, Cout not a multiple of 8 / 32, planes not a multiple of 64, batch > 1; and a filter with ONE value
    outside int8, for which every form must fall back to the scalar loop on the device."""
    rows, cols, cin, oc, n = shape
    rng = np.random.default_rng(rows * 100 + cin + oc)
    x = rng.integers(0, 256, (n, cin, rows, cols), dtype=np.uint8)
    f = rng.integers(-128, 128, (oc, cin), dtype=np.int32)
    f[0, 0], f[-1, -1] = -128, 127
    d_x, d_f = ctx.to_device(x), ctx.to_device(f)
    d_o, d_s, d_d, d_m = (ctx.alloc(n * oc * rows * cols) for _ in range(4))
    ext = pkg.make_ext(batch=n, dtype=pkg.DT_U8, quirks=0)
    for trial in range(2):
        want = np.stack([orc.lit_pointwise(x[i], f, rows, cols, cin, oc, quirks=0) for i in range(n)])
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, cin, oc, ext)           # default: the matrix cores where they measured faster, else v_dot4
        try:
            assert ctx.lib.mbn_tune_set(b"lit_dot", 1) == 0
            ctx.pointwise(d_s.ptr, d_x.ptr, d_f.ptr, rows, cols, cin, oc, ext)
            assert ctx.lib.mbn_tune_set(b"lit_dot", 2) == 0
            ctx.pointwise(d_d.ptr, d_x.ptr, d_f.ptr, rows, cols, cin, oc, ext)
            assert ctx.lib.mbn_tune_set(b"lit_dot", 3) == 0                       # the matrix cores wherever eligible (Cin, Cout >= 16), whatever the size
            ctx.pointwise(d_m.ptr, d_x.ptr, d_f.ptr, rows, cols, cin, oc, ext)
        finally:
            ctx.lib.mbn_tune_set(b"lit_dot", 0)
        ctx.sync()
        got, scalar, dot4 = d_o.download(want.shape, np.uint8), d_s.download(want.shape, np.uint8), d_d.download(want.shape, np.uint8)
        assert np.array_equal(d_m.download(want.shape, np.uint8), want), "int8 MFMA form, trial %d" % trial
        assert np.array_equal(scalar, want)
        assert np.array_equal(dot4, want), "v_dot4, trial %d: %d of %d bytes differ" % (trial, int((dot4 != want).sum()), want.size)
        assert np.array_equal(got, want), "default (int8 MFMA where eligible), trial %d: %d of %d bytes differ" % (trial, int((got != want).sum()), want.size)
        f[oc // 2, cin // 2] = 300 if trial == 0 else f[oc // 2, cin // 2]       # second trial: one value outside int8 -> device fallback
        d_f.upload(f)
    # with the carry quirk the channels are a serial chain: the call must still be right (scalar kernel)
    wantc = orc.lit_pointwise(x[0], f, rows, cols, cin, oc, quirks=1)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, cin, oc, pkg.make_ext(dtype=pkg.DT_U8, quirks=1))
    ctx.sync()
    assert np.array_equal(d_o.download(wantc.shape, np.uint8), wantc)


def test_literal_pointwise_mfma_operand_map_with_one_hot_filters(pkg, orc, ctx):
    """The int8 MFMA form's operand maps, pinned without the oracle: a filter whose row oc is one-hot at input channel perm[oc] with weight s[oc] in {1, -1, 2}
    must move plane perm[oc] of the input into plane oc of the output (x, 0 after the ReLU for -1, (2 x) mod 256 after the truncating store of kernel.cl:112) —
    every (output channel, input channel, pixel) pairing of the 32 x 32 x 32 instruction is hit by a known answer. Cin = 96, Cout = 80 (padded to 96 rows),
    a 9 x 9 plane (pixels past the 64-pixel tile and a ragged last tile)."""
    rows, cols, cin, oc, n = 9, 9, 96, 80, 2
    assert ctx.lib.mbn_tune_set(b"lit_dot", 3) == 0                           # 3 = the matrix-core form wherever it is eligible, whatever the size
    rng = np.random.default_rng(2)
    x = rng.integers(0, 256, (n, cin, rows, cols), dtype=np.uint8)
    perm = rng.permutation(cin)[:oc]
    sgn = rng.choice(np.array([1, -1, 2], np.int32), oc)
    f = np.zeros((oc, cin), np.int32)
    f[np.arange(oc), perm] = sgn
    want = np.empty((n, oc, rows, cols), np.uint8)
    for o in range(oc):
        src = x[:, perm[o]].astype(np.int64) * int(sgn[o])
        want[:, o] = (np.maximum(src, 0) % 256).astype(np.uint8)
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(want.size)
    try:
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, cin, oc, pkg.make_ext(batch=n, dtype=pkg.DT_U8, quirks=0))
    finally:
        ctx.lib.mbn_tune_set(b"lit_dot", 0)
    ctx.sync()
    got = d_o.download(want.shape, np.uint8)
    assert np.array_equal(got, want), "%d of %d bytes differ" % (int((got != want).sum()), want.size)
    assert np.array_equal(np.stack([orc.lit_pointwise(x[i], f, rows, cols, cin, oc, quirks=0) for i in range(n)]).reshape(want.shape), want)     # the oracle says the same
    try:                                                                     # and so does the v_dot4 form
        assert ctx.lib.mbn_tune_set(b"lit_dot", 2) == 0
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, cin, oc, pkg.make_ext(batch=n, dtype=pkg.DT_U8, quirks=0))
    finally:
        ctx.lib.mbn_tune_set(b"lit_dot", 0)
    ctx.sync()
    assert np.array_equal(d_o.download(want.shape, np.uint8), want)


def test_literal_pointwise_mfma_random_ragged_shapes(pkg, orc, ctx):
    """The int8 MFMA form forced (lit_dot = 3) on 24 seeded random shapes — Cin 16..200 (padded to 32s), Cout 16..150 (padded to 32s), planes of 1..211 pixels (ragged 64-pixel
    tiles, single-pixel FC-like calls), batch 1..3, weights over the whole int8 range — bit-exact against the oracle; every third shape also with one weight outside int8
    (device fallback to the scalar loop)."""
    rng = np.random.default_rng(20261004)
    try:
        assert ctx.lib.mbn_tune_set(b"lit_dot", 3) == 0
        for case in range(24):
            cin, oc = int(rng.integers(16, 201)), int(rng.integers(16, 151))
            rows, cols, n = int(rng.integers(1, 15)), int(rng.integers(1, 16)), int(rng.integers(1, 4))
            x = rng.integers(0, 256, (n, cin, rows, cols), dtype=np.uint8)
            f = rng.integers(-128, 128, (oc, cin), dtype=np.int32)
            if case % 3 == 2:
                f[int(rng.integers(0, oc)), int(rng.integers(0, cin))] = int(rng.choice([128, -129, 4000, -70000]))
            want = np.stack([orc.lit_pointwise(x[i], f, rows, cols, cin, oc, quirks=0) for i in range(n)]).reshape(n, oc, rows, cols)
            d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(want.size)
            ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, rows, cols, cin, oc, pkg.make_ext(batch=n, dtype=pkg.DT_U8, quirks=0))
            ctx.sync()
            got = d_o.download(want.shape, np.uint8)
            assert np.array_equal(got, want), "case %d (cin %d, cout %d, %d x %d, batch %d): %d of %d bytes differ" % (
                case, cin, oc, rows, cols, n, int((got != want).sum()), want.size)
            for b in (d_x, d_f, d_o):
                b.free()
    finally:
        ctx.lib.mbn_tune_set(b"lit_dot", 0)


def test_net_graph_under_pw_emul(pkg, ctx, tmp_path):
    """mbn_net_set_graph with the opt-in pw_emul: the pre-split filter images are allocated on first use, which may not happen
    inside a capture — the runner makes one eager pass before it captures, and the graph key holds the pw_emul value. Replayed
    logits == eager logits bit for bit under pw_emul 6, and switching back to 0 re-captures the default kernels."""
    n = 64
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, n)
    imgs = _headline_images(n, 224, 77)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 1000 * 4)

    def fwd():
        net.forward(d_in.ptr, d_out.ptr, n)
        ctx.sync()
        return d_out.download((n, 1000), np.float32)
    base = fwd()
    try:
        assert ctx.lib.mbn_tune_set(b"pw_emul", 6) == 0
        net.set_graph(True)                                  # first forward under the graph: eager pass + capture + replay
        g1 = fwd()
        g2 = fwd()
        net.set_graph(False)
        eager = fwd()
        assert np.array_equal(g1, eager) and np.array_equal(g2, eager)
        assert not np.array_equal(eager, base), "the split kernels were not on the path"
        net.set_graph(True)
        fwd()
        assert ctx.lib.mbn_tune_set(b"pw_emul", 0) == 0
        assert np.array_equal(fwd(), base), "the graph was not re-captured after pw_emul changed"
    finally:
        ctx.lib.mbn_tune_set(b"pw_emul", 0)
        net.destroy()


def test_net_graph_pw_emul_static_follows_weight_upload(pkg, ctx, tmp_path):
    """hipGraph + pw_emul 6 + pw_emul_static 1, then new weights through mbn_upload. The eager pass before
    the capture marks every filter image 'built'; a capture that baked that in would replay GEMMs on the old images for ever
    (the graph key does not change with the weights). Inside a capture the split is now always recorded as a graph node:
    replayed logits after the upload == eager logits with the new weights, bit for bit, and differ from the old ones."""
    n = 64                                                      # layer 15 at 64 images: 392 tiles of 128 x 128, on the split GEMM
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, n)
    imgs = _headline_images(n, 224, 78)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 1000 * 4)

    def fwd():
        net.forward(d_in.ptr, d_out.ptr, n)
        ctx.sync()
        return d_out.download((n, 1000), np.float32)
    try:
        assert ctx.lib.mbn_tune_set(b"pw_emul", 6) == 0
        assert ctx.lib.mbn_tune_set(b"pw_emul_static", 1) == 0
        net.set_graph(True)
        old = fwd()
        assert np.array_equal(fwd(), old)
        blob2 = hw.blob.copy()
        for li in (6, 14):                                      # pointwise filters of layer 7 (inside fused block 6-7) and layer 15 (stand-alone)
            l = hw.plan.layer[li]
            blob2[l.w_offset:l.w_offset + l.w_count] *= np.float32(0.5)
        net._dev_blob.upload(blob2)                             # mbn_upload: same pointers, new contents
        replay = fwd()
        net.set_graph(False)
        eager = fwd()
        assert np.array_equal(replay, eager), "the graph replayed the pre-upload filter images"
        assert not np.array_equal(replay, old)
    finally:
        ctx.lib.mbn_tune_set(b"pw_emul", 0)
        ctx.lib.mbn_tune_set(b"pw_emul_static", 0)
        net.destroy()


def test_net_reset_fuse_blocks_and_stream_change_between_free_running_forwards(pkg, ctx, tmp_path):
    """(1) set(get()) makes the mask explicit, which switches the few-tile rule off — the launch list changes and
    mbn_net_reset_fuse_blocks brings the default rules back; (2) changing the stream count between two otherwise identical
    free-running forwards re-inserts the fork (the sub-batch slices move): logits stay bit-identical to the single-stream ones."""
    n = 24
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, n)
    imgs = _headline_images(n, 224, 79)
    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * 1000 * 4)
    default_launches = net.launches(4)
    net.set_fuse_blocks(net.get_fuse_blocks())
    assert net.launches(4) != default_launches                  # explicit mask: blocks fused even at 4 images
    net.reset_fuse_blocks()
    assert net.launches(4) == default_launches

    def fwd():
        net.forward(d_in.ptr, d_out.ptr, n)
        ctx.sync()
        return d_out.download((n, 1000), np.float32)
    base = fwd()
    for ns in (2, 4, 3, 2):
        net.set_streams(ns, free_running=True)
        assert np.array_equal(fwd(), base) and np.array_equal(fwd(), base), ns
    net.destroy()


def test_bench_multi_rank_branch_on_one_gpu(pkg):
    """bench.py's N > 1 branch (it referenced an undefined name) run for real: two ranks on gloo sharing
    this box's one GPU. The line must carry n_gpus = 2, the whole-job value, and a passing parity_check of rank 0's shard."""
    import json
    import subprocess
    import sys
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29617", os.path.join(pkg.REPO_ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo",
           "--device-override", "0", "--steps", "5", "--warmup", "1", "--batch", "16", "--alpha", "0.5", "--res", "96"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = r.stdout.splitlines()[-1]
    out = json.loads(line)
    assert len(line) < 6000
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 32 and out["value"] > 0
    assert out["parity_check"]["ok"] and out["parity_check"]["images"] == 8
    assert "cpu_baseline" not in out and "configs_alt" not in out
    assert out["profiled_steps"] == 5
    full = json.load(open(os.path.join(pkg.REPO_ROOT, out["full_record"])))
    assert full["event_overhead_us"]["empty_pair"] >= 0 and len(full["layers"]) > 5 and full["profiled_steps_where"].startswith("after")


def test_bench_self_launches_its_ranks(pkg):
    """`python bench.py --gpus 2` started the way the driver starts `--gpus 1` — no torch.distributed.run in
    front — must start its own ranks as a child process (before touching the GPU) and print rank 0's line, instead of exiting.
    Rehearsed with both ranks on this box's one card over gloo; without --device-override the same command is refused with the
    MBN_ENODEVICE text because the box has fewer than 2 GPUs (the reference has one device, MobileNet.c:155)."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(pkg.REPO_ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--device-override", "0",
           "--steps", "5", "--warmup", "1", "--batch", "16", "--alpha", "0.5", "--res", "96"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0] == r.stdout.splitlines()[-1]    # ONE line, rank 0's, and it is the LAST thing on stdout
    assert len(lines[0]) < 6000                                         # the 20 KB line did not fit the driver's stdout tail
    out = json.loads(r.stdout.splitlines()[-1])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 32 and out["value"] > 0 and out["parity_check"]["ok"]
    # the N > 1 line proves its ranks: one entry per rank, the group's own world size, the backend
    assert len(out["ranks"]) == 2 and [x[0] for x in out["ranks"]] == [0, 1] and out["collective_world_size"] == 2 and out["backend"] == "gloo"
    assert out["ranks"][0][2] == out["ranks"][1][2] and all(x[3] == 16 and x[4] > 0 for x in out["ranks"])      # --device-override: the same card, said so
    # round 6: each rank also reports what ITS card held while all ranks ran (package W, sclk MHz, clock inside the GEMM launches); None only where the box has no rocm-smi
    assert all(len(x) == 8 for x in out["ranks"]) and "package_w" in out["ranks_cols"]
    assert all((x[5] is None or x[5] > 0) and (x[7] is None or 0.5 < x[7] < 3.0) for x in out["ranks"])
    # flat per-stage triples [ms, frac_hbm, frac_mfma]; roofline holds scalars only (the driver's parser keeps scalars)
    assert len(out["stages_frac"]["pointwise"]) == 3 and all(not isinstance(v, (dict, list)) for v in out["roofline"].values())
    import torch
    if torch.cuda.device_count() < 2:
        r = subprocess.run([sys.executable, os.path.join(pkg.REPO_ROOT, "bench.py"), "--gpus", "2", "--steps", "2"], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 19 and "MBN_ENODEVICE" in r.stderr and not r.stdout.strip()


def test_held_clock_counters_and_pci_bus_id(pkg, ctx):
    """Round 5: mbn_device_pci_bus_id names the card a context holds; the product switch pw_clock makes every pw_gemm launch add the core
    cycles (s_memtime) and 100 MHz reference ticks (s_memrealtime) its first eight workgroups lived to device counters, mbn_pw_clock_read turns them into the clock
    the chip held. Off: nothing is recorded. The GEMM's result does not depend on the switch."""
    bus = ctx.pci_bus_id()
    assert bus.count(":") == 2 and "." in bus and len(bus) >= 10, bus
    m, k, n = 50176, 512, 512
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    f = rng.normal(0, (2.0 / k) ** 0.5, (n, k)).astype(np.float32)
    d_x, d_f, d_o = ctx.to_device(x), ctx.to_device(f), ctx.alloc(m * n * 4)
    d_sc, d_sh = ctx.to_device(np.ones(n, np.float32)), ctx.to_device(np.zeros(n, np.float32))
    ext = pkg.make_ext(act=2, scale=d_sc.ptr, shift=d_sh.ptr)
    ctx.pw_clock(reset=True)
    ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, k, n, ext)
    ctx.sync()
    base = d_o.download((m, n), np.float32)
    assert ctx.pw_clock(reset=True) == (0.0, 0)                      # switch off: nothing recorded
    try:
        assert ctx.lib.mbn_tune_set(b"pw_clock", 1) == 0
        for _ in range(6):
            ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, k, n, ext)
        ghz, launches = ctx.pw_clock(reset=False)
        assert launches == 6 and 0.8 < ghz < 2.6, (ghz, launches)    # MI355X: 2.4 GHz peak engine clock; held 2.1-2.4 under the fp32 MFMA stream
        assert ctx.pw_clock(reset=True)[1] == 6 and ctx.pw_clock(reset=True) == (0.0, 0)
    finally:
        ctx.lib.mbn_tune_set(b"pw_clock", 0)
    assert np.array_equal(d_o.download((m, n), np.float32), base)
    for b in (d_x, d_f, d_o, d_sc, d_sh):
        b.free()


def test_graft_entry_smoke_runs():
    """__graft_entry__.smoke() is what the driver runs on the GPU box before the bench: it must keep passing when dispatch
    rules change (it asserts which fused kernels are on its path)."""
    import importlib
    ge = importlib.import_module("__graft_entry__")
    ge.smoke()

