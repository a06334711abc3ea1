"""Interior pointers at every element alignment: mbn_pointwise, mbn_depthwise, mbn_convolute and mbn_pool in fp32 and bf16 with one
operand at a time (and all of them at once) 2, 4 or 8 bytes off its allocation's 256-byte alignment, against the oracle, bit for bit against
the fully aligned call where the launcher keeps the kernel, and with 0xFF guards on both sides of the output; the fused calls, pool + FC,
convert and normalize, which refuse such pointers with a named code; and the net runner writing into a misaligned caller buffer.

Every operand sits at base + 256 + off inside an mbn_alloc buffer of nbytes + 512 that was filled with 0xFF first, so an alignment
mistake stays inside the allocation: a load rounded down reads NaNs or a neighbouring element, a store rounded down lands in the guard in
front of the tensor. Each case's comment names the kernel the launcher's pointer conditions send it to (csrc/mbn_f32_pw.hip, mbn_f32_dw.hip,
mbn_f32_misc.hip); `same` marks the cases in which that is the aligned call's kernel (or one documented as bit-identical to it)."""
import ctypes as C

import numpy as np
import pytest

from test_rect_gpu import TOL_BF16, TOL_BF16_NET, TOL_DW, TOL_PW, _bf16_dev, _images, _weights, assert_close

pytestmark = pytest.mark.gpu

GUARD = 256


class Slot:
    """`nbytes` at base + 256 + off inside an mbn_alloc buffer of nbytes + 512, the whole buffer 0xFF before `data` goes in through the
    interior pointer. Every Slot is freed when its test ends (_free_slots)."""

    live = []

    def __init__(self, ctx, nbytes, off=0, data=None):
        assert 0 <= off < GUARD
        Slot.live.append(self)
        self.ctx, self.nbytes, self.off = ctx, int(nbytes), off
        self.buf = ctx.alloc(self.nbytes + 2 * GUARD)
        assert self.buf.ptr % GUARD == 0
        self.ptr = self.buf.ptr + GUARD + off
        assert ctx.lib.mbn_memset(ctx.h, self.buf.ptr, 0xFF, self.buf.nbytes) == 0
        ctx.sync()
        if data is not None:
            a = np.ascontiguousarray(data)
            assert a.nbytes == self.nbytes
            assert ctx.lib.mbn_upload(ctx.h, self.ptr, a.ctypes.data, a.nbytes) == 0

    def read(self, shape, dtype, what=""):
        """The tensor, after checking that no byte of the guards in front of it and behind it changed."""
        raw = self.buf.download((self.buf.nbytes,), np.uint8)
        lo = GUARD + self.off
        front, back = raw[:lo], raw[lo + self.nbytes:]
        assert (front == 0xFF).all(), "%s: %d guard bytes IN FRONT of the tensor were overwritten (first at %d before it)" % (
            what, int((front != 0xFF).sum()), lo - int(np.flatnonzero(front != 0xFF)[0]))
        assert (back == 0xFF).all(), "%s: %d guard bytes behind the tensor were overwritten (first at +%d)" % (
            what, int((back != 0xFF).sum()), int(np.flatnonzero(back != 0xFF)[0]))
        return raw[lo:lo + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self.buf.download((self.buf.nbytes,), np.uint8) == 0xFF).all())

    def free(self):
        self.buf.free()


@pytest.fixture(autouse=True)
def _free_slots():
    yield
    for s in Slot.live:
        s.free()
    del Slot.live[:]


class Spec:
    """One layer call: host inputs by operand name (already in their device format), the output's raw format, the oracle's result, the
    launch, and the offsets of the all-operands-misaligned case."""

    def __init__(self, inputs, out_shape, out_raw, want, tol, launch, all_offs, relu6=True, bf16_out=False):
        self.inputs, self.out_shape, self.out_raw, self.want, self.tol = inputs, out_shape, out_raw, want, tol
        self.launch, self.all_offs, self.relu6, self.bf16_out = launch, all_offs, relu6, bf16_out
        self.aligned = None


def _run(pkg, ctx, spec, offs, what):
    slots = {k: Slot(ctx, a.nbytes, offs.get(k, 0), a) for k, a in spec.inputs.items()}
    out = Slot(ctx, int(np.prod(spec.out_shape)) * np.dtype(spec.out_raw).itemsize, offs.get("out", 0))
    ptrs = {k: s.ptr for k, s in slots.items()}
    ptrs["out"] = out.ptr
    rc = spec.launch(ctx, ptrs)
    assert rc == pkg.OK, "%s: rc %d (%s)" % (what, rc, ctx.last_error())
    ctx.sync()
    raw = out.read(spec.out_shape, spec.out_raw, what)
    for s in list(slots.values()) + [out]:
        s.free()
    return raw


def _unclamped(want):
    """A clamp must not hide a shifted operand: at least a quarter of a ReLU6 case's reference outputs lie strictly inside (0, 6)."""
    inside = float(((want > 0) & (want < 6)).mean())
    assert inside >= 0.25, "only %.0f %% of the reference outputs are strictly inside (0, 6)" % (100 * inside)


def _check(pkg, ctx, spec, operand, off, same, what):
    offs = {} if operand == "none" else spec.all_offs if operand == "all" else {operand: off}
    if spec.relu6:
        _unclamped(spec.want)
    raw = _run(pkg, ctx, spec, offs, what)
    got = pkg.bf16_bits_to_f32(raw) if spec.bf16_out else raw.view(np.float32)
    assert_close(got, spec.want, spec.tol, what + " vs the oracle")
    if same:
        if spec.aligned is None:
            spec.aligned = _run(pkg, ctx, spec, {}, what + " (aligned call)")
        assert np.array_equal(raw, spec.aligned), "%s: %d of %d elements differ from the aligned call's bits" % (
            what, int((raw != spec.aligned).sum()), raw.size)


_SPECS = {}


def _spec(key, build):
    if key not in _SPECS:
        _SPECS[key] = build()
    return _SPECS[key]


def _cases(operand_offsets, extra=("all",)):
    return [(op, off) for op, offs in operand_offsets for off in offs] + [(e, 0) for e in extra]


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------------------ fp32 pointwise

def _cus(ctx):
    n = C.c_int()
    assert ctx.lib.mbn_device_cus(ctx.h, C.byref(n)) == 0
    return n.value


# name: (M, K, N, batch, scale given) and the kernel the ALIGNED call takes under the default knobs. A misaligned `in` or `filt` sends every
# shape to pw_generic (the launcher's `fast` comes first, so the in / filt conditions of the split-K, pw3 and pw_emul guards cannot be false
# when they are reached: no call takes them the other way); a misaligned
# `out`, `scale` or `shift` is checked by pw3 alone, which then falls through to pw_gemm — documented as the same bits.
PW_F32 = {
    "gemm": (56 * 56, 128, 128, 1, True),         # pw_gemm<float, 64, 64>: direct-to-LDS, pipelined k-loop, scale / shift staged in LDS, fast epilogue
    "splitk": (2 * 25, 128, 256, 2, True),        # pw_splitk_f32<4, ., 1>: 2 images, K >= 128, few tiles; ragged rows (50 = 3 x 16 + 2)
    "pw3": (None, 64, 128, 1, True),              # M = 128 x CUs + 7: the smallest M at which MBN_PW3_DEFAULT holds -> pw3_f32<64>; off 16 bytes: pw_gemm<float, 128, 128>
    "n1000": (256, 1024, 1000, 1, True),          # pw_gemm<float, 64, 64>, ragged column tile (1000 = 15 x 64 + 40): the general epilogue there
    "noscale": (300, 72, 40, 1, False),           # NULL scale, K % 32 != 0: pw_gemm<float, 64, 64, ., 2, false, false> (register staging), general epilogue
}
PW_F32_CASES = [(name,) + c for name, v in PW_F32.items()
                for c in _cases([(op, (4, 8)) for op in ("in", "filt", "out", "scale", "shift") if v[4] or op != "scale"])]


def _pw_spec(pkg, orc, ctx, name, m, k, n, batch, has_scale, bf, act=2, out_f32=False, seed=0):
    rng = np.random.default_rng(seed + m + 3 * k + n)
    x = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    f = rng.normal(0, (2.0 / k) ** 0.5, (n, k)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, n).astype(np.float32) if has_scale else None
    sh = rng.normal(0, 0.1, n).astype(np.float32)
    if bf:
        x, f = orc.bf16_round(x), orc.bf16_round(f)
    want = orc.f32_pointwise(x, f, sc, sh, act)
    bf_out = bf and not out_f32
    if bf_out:
        want = orc.bf16_round(want)
    inputs = {"in": pkg.f32_to_bf16_bits(x) if bf else x, "filt": pkg.f32_to_bf16_bits(f) if bf else f, "shift": sh}
    if has_scale:
        inputs["scale"] = sc
    es = 2 if bf else 4

    def launch(ctx, p):
        ext = pkg.make_ext(batch=batch, dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=act, scale=p.get("scale"), shift=p["shift"],
                           io_flags=pkg.IO_OUT_F32 if out_f32 else 0)
        return ctx.lib.mbn_pointwise(ctx.h, p["out"], p["in"], p["filt"], m // batch, 1, k, n, C.byref(ext))
    all_offs = {"in": es, "filt": es, "out": 2 if bf_out else 4, "scale": 4, "shift": 4}
    return Spec(inputs, (m, n), np.uint16 if bf_out else np.uint32, want, TOL_BF16 if bf else TOL_PW, launch, all_offs, relu6=act == 2,
                bf16_out=bf_out)


@pytest.mark.parametrize("case", PW_F32_CASES, ids=_ids)
def test_f32_pointwise_interior_pointers(pkg, orc, ctx, case):
    name, operand, off = case
    m, k, n, batch, has_scale = PW_F32[name]
    if m is None:
        m = 128 * _cus(ctx) + 7
    spec = _spec(("pwf", name), lambda: _pw_spec(pkg, orc, ctx, name, m, k, n, batch, has_scale, False))
    # in / filt / all: pw_generic<float>. out / scale / shift: the aligned call's kernel (pw3: pw_gemm, the same bits)
    same = operand in ("out", "scale", "shift")
    _check(pkg, ctx, spec, operand, off, same, "fp32 pointwise %s, %s + %d" % (name, operand, off))


# ------------------------------------------------------------------------------------------------------------ bf16 pointwise

# name: (M, K, N, act, out_f32, scale given). in / filt off 16 bytes: pw_generic<__bf16> for every shape.
PW_BF16 = {
    "k64n128": (250, 64, 128, 2, False, True),     # M < 512: the streaming kernel refuses (m < 4 BM) -> pw_gemm<__bf16, 64, 128, 32, 64>, one k-tile, channel-paired
                                                   # 4-byte stores and 8-byte scale / shift loads from global memory; nothing downstream looks at out / scale / shift
    "stream32": (517, 64, 128, 2, False, True),    # pw_stream_bf16<ShapeStd> on 32x32x16; out off 4 or scale / shift off 8 bytes: pw_gemm<__bf16, 64, 128, 32, 64>
    "stream16": (250, 512, 512, 2, False, True),   # K >= 256: pw_stream_bf16<ShapeStd, 0, true> on 16x16x32 at every M; same fall-back, onto pw_gemm<__bf16, 64, 128, 32, 64>
    "tile64": (250, 128, 96, 2, False, True),      # N < 128: pw_gemm<__bf16, 64, 64, 32, 32>, 2-byte stores, ragged column tile
    "oddn": (203, 64, 129, 2, False, True),        # odd N: pw_gemm<__bf16, 64, 128, 32, 64> on its element-wise epilogue; every second row starts on an odd element
    "f32out": (250, 128, 100, 0, True, False),     # MBN_IO_OUT_F32 (the FC form: bias, no scale, no activation): pw_gemm<__bf16, 64, 64, 32, 32> storing fp32
}
PW_BF16_CASES = [(name,) + c for name, v in PW_BF16.items()
                 for c in _cases([("out", (4, 8) if v[4] else (2, 4, 8)), ("in", (2, 8)), ("filt", (2, 8))] + ([("scale", (4, 8))] if v[5] else []) +
                                 [("shift", (4, 8))])]


@pytest.mark.parametrize("case", PW_BF16_CASES, ids=_ids)
def test_bf16_pointwise_interior_pointers(pkg, orc, ctx, case):
    name, operand, off = case
    m, k, n, act, out_f32, has_scale = PW_BF16[name]
    spec = _spec(("pwb", name), lambda: _pw_spec(pkg, orc, ctx, name, m, k, n, 1, has_scale, True, act=act, out_f32=out_f32, seed=11))
    if operand in ("in", "filt", "all"):
        same = False                                               # pw_generic<__bf16>
    elif name.startswith("stream"):                                # stream_common_ok: out % 4, scale % 8, shift % 8 — else pw_gemm, other bits
        same = off % (4 if operand == "out" else 8) == 0
    else:
        same = True                                                # pw_gemm checks nothing more: the same kernel, paired stores on an odd element included
    _check(pkg, ctx, spec, operand, off, same, "bf16 pointwise %s, %s + %d" % (name, operand, off))


# ------------------------------------------------------------------------------------------------------------ depthwise

# name: (batch, rows, cols, stride, dilation); fp32 with C = 8, bf16 with C = 16
DW_SHAPES = {"s1": (2, 9, 9, 1, 1), "s2": (2, 12, 11, 2, 1), "dil2": (2, 9, 9, 1, 2)}


def _dw_spec(pkg, orc, n, h, w, c, stride, dil, bf, seed=0):
    from test_dilation_cpu import inflate
    rng = np.random.default_rng(seed + 31 * h + w + c + stride + dil)
    x = rng.uniform(-1, 1, (n, h, w, c)).astype(np.float32)
    f = rng.normal(0, 0.5, (3, 3, c)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, c).astype(np.float32)
    sh = rng.normal(0, 0.1, c).astype(np.float32)
    if bf:
        x = orc.bf16_round(x)
    oh, ow = -(-h // stride), -(-w // stride)
    if dil > 1:       # the oracle has no dilation: the zero-inflated (2 D + 1)^2 filter, SAME padding D (test_dilation_cpu.py pins it)
        want = orc.f32_depthwise(x, inflate(f, dil), sc, sh, stride, 2, out_rows=oh, out_cols=ow, pad_top=dil, pad_left=dil)
    else:
        want = orc.f32_depthwise(x, f, sc, sh, stride, 2)
    assert want.shape == (n, oh, ow, c)
    if bf:
        want = orc.bf16_round(want)

    def launch(ctx, p):
        ext = pkg.make_ext(batch=n, dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=2, in_rows=h, in_cols=w, scale=p["scale"], shift=p["shift"],
                           dilation=dil)
        return ctx.lib.mbn_depthwise(ctx.h, p["out"], p["in"], p["filt"], oh, ow, 3, stride, c, C.byref(ext))
    es = 2 if bf else 4
    return Spec({"in": pkg.f32_to_bf16_bits(x) if bf else x, "filt": f, "scale": sc, "shift": sh}, want.shape, np.uint16 if bf else np.uint32, want,
                TOL_BF16 if bf else TOL_DW, launch, {"in": es, "out": es, "filt": 4, "scale": 4, "shift": 4}, bf16_out=bf)


@pytest.mark.parametrize("case", _cases([("in", (4, 8)), ("out", (4, 8)), ("filt", (4,)), ("scale", (4,)), ("shift", (4,))]), ids=_ids)
@pytest.mark.parametrize("name", list(DW_SHAPES))
def test_f32_depthwise_interior_pointers(pkg, orc, ctx, name, case):
    """Aligned: dw3x3_nhwc<S, 2, float> (s1, s2) / dw3x3_dil_nhwc<2, 2, float> (dil2). launch_dw's `fast` wants in, out, filt, scale and shift
    on 16 bytes in fp32: every case here runs dw_generic_nhwc<float>, so the oracle's tolerance alone applies."""
    operand, off = case
    n, h, w, stride, dil = DW_SHAPES[name]
    spec = _spec(("dwf", name), lambda: _dw_spec(pkg, orc, n, h, w, 8, stride, dil, False))
    _check(pkg, ctx, spec, operand, off, False, "fp32 depthwise %s, %s + %d" % (name, operand, off))


@pytest.mark.parametrize("case", _cases([("in", (2, 8)), ("out", (2, 8))]), ids=_ids)
@pytest.mark.parametrize("name", list(DW_SHAPES))
def test_bf16_depthwise_interior_pointers(pkg, orc, ctx, name, case):
    """Aligned, C = 16: dw3x3_nhwc_bf16x8<S, 2>, the 8-channel march (s1, s2) / dw3x3_dil_nhwc<2, 2, __bf16> (dil2). in or out + 2 (and `all`):
    off the 8-byte channel quad -> dw_generic_nhwc<__bf16>. in or out + 8: still `fast`, off the 16 bytes of the 8-channel march ->
    dw3x3_nhwc<S, 2, __bf16>, the 4-channel march; the dilated kernel marches channel quads anyway and is the aligned call's kernel."""
    operand, off = case
    n, h, w, stride, dil = DW_SHAPES[name]
    spec = _spec(("dwb", name), lambda: _dw_spec(pkg, orc, n, h, w, 16, stride, dil, True, seed=5))
    _check(pkg, ctx, spec, operand, off, name == "dil2" and off == 8, "bf16 depthwise %s, %s + %d" % (name, operand, off))


@pytest.mark.parametrize("shape", [(2, 9, 7, 12, 1), (2, 11, 9, 12, 2), (3, 7, 9, 20, 1), (2, 13, 10, 20, 2)], ids=_ids)
def test_bf16_depthwise_four_channel_march(pkg, orc, ctx, shape):
    """C % 8 == 4 with every pointer aligned: launch_dw's middle tier, dw3x3_nhwc<S, 2, __bf16> (4 channels per lane), which no other test
    reaches; both strides, odd map sides, C / 4 = 3 and 5 lanes per slab."""
    n, h, w, c, stride = shape
    spec = _spec(("dw4", shape), lambda: _dw_spec(pkg, orc, n, h, w, c, stride, 1, True, seed=9))
    _check(pkg, ctx, spec, "none", 0, False, "bf16 depthwise %s on the 4-channel march" % (shape,))


# ------------------------------------------------------------------------------------------------------------ convolute

CONV_MODES = ["f32", "bf16", "u8"]       # fp32; bf16 + MBN_IO_IN_F32; fp32 + MBN_IO_IN_U8


def _conv_spec(pkg, orc, mode, cout):
    n, res = 2, 32
    rng = np.random.default_rng(res + cout + len(mode))
    if mode == "u8":
        img = rng.integers(0, 256, (n, res, res, 3), dtype=np.uint8)
        x = (img.astype(np.float32) * np.float32(1 / 127.5) + np.float32(-1)).astype(np.float32)
    else:
        img = x = rng.uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    f = rng.normal(0, 0.27, (3, 3, 3, cout)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = rng.normal(0, 0.1, cout).astype(np.float32)
    want = orc.f32_conv(x, f, sc, sh, 2, 2)
    bf = mode == "bf16"
    if bf:
        want = orc.bf16_round(want)

    def launch(ctx, p):
        ext = pkg.make_ext(batch=n, dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=2, cin=3, scale=p["scale"], shift=p["shift"],
                           io_flags=pkg.IO_IN_F32 if bf else pkg.IO_IN_U8 if mode == "u8" else 0)
        return ctx.lib.mbn_convolute(ctx.h, p["out"], p["in"], None, None, p["filt"], res, res, 3, 2, cout, C.byref(ext))
    return Spec({"in": img, "filt": f, "scale": sc, "shift": sh}, want.shape, np.uint16 if bf else np.uint32, want, TOL_BF16 if bf else TOL_DW, launch,
                {"in": 1 if mode == "u8" else 4, "out": 2 if bf else 4, "filt": 4, "scale": 4, "shift": 4}, bf16_out=bf)


def _conv_cases(mode):
    ops = [(op, (4, 8)) for op in ("filt", "scale", "shift")]
    ops.append(("out", (2, 4, 8) if mode == "bf16" else (4, 8)))
    ops.append(("in", (1, 2, 4) if mode == "u8" else (4, 8)))
    return [(mode,) + c for c in _cases(ops)]


@pytest.mark.parametrize("case", [c for m in CONV_MODES for c in _conv_cases(m)], ids=_ids)
@pytest.mark.parametrize("cout", [32, 8])
def test_convolute_interior_pointers(pkg, orc, ctx, cout, case):
    """32 x 32 images, stride 2. Aligned: fp32 with 32 channels conv1_mfma_f32 (16 output columns per row), every other aligned call
    conv3x3s2c3_f32_nhwc<T>. out (fp32: off 16, bf16: off 8 bytes), filt, scale or shift off 16 bytes: `fast` is false ->
    conv_generic_f32_nhwc<T>. The image off 16 bytes (uint8: off 4): `first_layer` is false -> conv_f32_nhwc<T>, which reads it per element.
    The same kernel as the aligned call, hence the same bits: a bf16 output 8 bytes off, a uint8 image 4 bytes off."""
    mode, operand, off = case
    spec = _spec(("conv", mode, cout), lambda: _conv_spec(pkg, orc, mode, cout))
    same = (mode == "bf16" and operand == "out" and off == 8) or (mode == "u8" and operand == "in" and off == 4)
    _check(pkg, ctx, spec, operand, off, same, "convolute %s, %d channels, %s + %d" % (mode, cout, operand, off))


# ------------------------------------------------------------------------------------------------------------ pool

@pytest.mark.parametrize("case", [("f32",) + c for c in _cases([("in", (4, 8)), ("out", (4, 8))])] +
                         [("bf16",) + c for c in _cases([("in", (2, 8)), ("out", (2, 8))])], ids=_ids)
def test_pool_interior_pointers(pkg, orc, ctx, case):
    """mbn_launch_f32_pool has no pointer condition: pool_f32_nhwc<T> reads and writes per element — the aligned call's kernel, the same bits."""
    dtype, operand, off = case
    bf = dtype == "bf16"

    def build():
        n, h, ch = 2, 7, 64
        x = np.random.default_rng(ch + bf).uniform(0, 6, (n, h, h, ch)).astype(np.float32)
        if bf:
            x = orc.bf16_round(x)
        want = orc.f32_pool(x)
        if bf:
            want = orc.bf16_round(want)

        def launch(ctx, p):
            ext = pkg.make_ext(batch=n, dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=pkg.ACT_NONE)
            return ctx.lib.mbn_pool(ctx.h, p["out"], p["in"], h, h, h, ch, C.byref(ext))
        es = 2 if bf else 4
        return Spec({"in": pkg.f32_to_bf16_bits(x) if bf else x}, want.shape, np.uint16 if bf else np.uint32, want, TOL_BF16 if bf else TOL_DW, launch,
                    {"in": es, "out": es}, relu6=False, bf16_out=bf)
    _check(pkg, ctx, _spec(("pool", dtype), build), operand, off, True, "pool %s, %s + %d" % (dtype, operand, off))


# ------------------------------------------------------------------------------------------------------------ refusals

def _zeros(ctx, nbytes, off=0):
    s = Slot(ctx, nbytes, off)
    assert ctx.lib.mbn_memset(ctx.h, s.ptr, 0, nbytes) == 0
    ctx.sync()
    return s


def _block_args(ctx, cin, cout, bf):
    """wd, s2, b2, wp, s3, b3 of a fused block, zero-filled and aligned"""
    return [_zeros(ctx, nb) for nb in (36 * cin, 4 * cin, 4 * cin, (2 if bf else 4) * cin * cout, 4 * cout, 4 * cout)]


@pytest.mark.parametrize("bf", [False, True], ids=["mbn_dwpw_fused", "mbn_dwpw_fused_bf16"])
@pytest.mark.parametrize("off", [4, 8])
def test_fused_block_refuses_interior_pointers(pkg, ctx, bf, off):
    """check_ptrs: a pointer off 16 bytes is MBN_EUNSUPPORTED (the net runner then issues the two layers), whichever operand it is."""
    n, h, cin, cout = 1, 8, 32, 128
    es = 2 if bf else 4
    fn = ctx.lib.mbn_dwpw_fused_bf16 if bf else ctx.lib.mbn_dwpw_fused
    p = _block_args(ctx, cin, cout, bf)

    def call(out, x, wd=p[0].ptr):
        return fn(ctx.h, out, x, wd, p[1].ptr, p[2].ptr, p[3].ptr, p[4].ptr, p[5].ptr, n, h, h, h, h, cin, cout, 1, 1, 1, None)
    x, xo, wdo = _zeros(ctx, n * h * h * cin * es), _zeros(ctx, n * h * h * cin * es, off), _zeros(ctx, 36 * cin, off)
    out, outo = Slot(ctx, n * h * h * cout * es), Slot(ctx, n * h * h * cout * es, off)
    assert call(outo.ptr, x.ptr) == pkg.EUNSUPPORTED
    assert call(out.ptr, xo.ptr) == pkg.EUNSUPPORTED
    assert call(out.ptr, x.ptr, wdo.ptr) == pkg.EUNSUPPORTED
    ctx.sync()
    assert out.untouched() and outo.untouched(), "a refused call launched something"
    assert call(out.ptr, x.ptr) == pkg.OK               # the shape itself is inside the envelope: the refusals were about the pointers
    ctx.sync()
    assert not out.untouched()


def test_stem_fused_hw_refuses_interior_pointers(pkg, ctx):
    """mbn_stem_fused_hw: the output off 16 bytes or the fp32 image off 8 is MBN_EINVAL, a parameter off 16 bytes MBN_EUNSUPPORTED (mbn.h)."""
    n, res, c1, c3 = 1, 32, 16, 32
    par = [_zeros(ctx, nb) for nb in (4 * 27 * c1, 4 * c1, 4 * c1, 36 * c1, 4 * c1, 4 * c1, 4 * c1 * c3, 4 * c3, 4 * c3)]
    w1o = _zeros(ctx, 4 * 27 * c1, 8)
    img, imgo = _zeros(ctx, n * res * res * 3 * 4), _zeros(ctx, n * res * res * 3 * 4, 4)
    nb = n * (res // 2) * (res // 2) * c3 * 4
    out, outo4, outo8 = Slot(ctx, nb), Slot(ctx, nb, 4), Slot(ctx, nb, 8)

    def call(o, im, w1=par[0].ptr):
        return ctx.lib.mbn_stem_fused_hw(ctx.h, o, im, w1, *[q.ptr for q in par[1:]], n, res, res, c1, c3, 0, None)
    assert call(outo4.ptr, img.ptr) == pkg.EINVAL
    assert call(outo8.ptr, img.ptr) == pkg.EINVAL
    assert call(out.ptr, imgo.ptr) == pkg.EINVAL
    assert call(out.ptr, img.ptr, w1o.ptr) == pkg.EUNSUPPORTED
    ctx.sync()
    assert out.untouched() and outo4.untouched() and outo8.untouched(), "a refused call launched something"
    assert call(out.ptr, img.ptr) == pkg.OK
    ctx.sync()
    assert not out.untouched()


def _resident_params(pkg, ctx, shapes):
    arr = (pkg.BlockParams * len(shapes))()
    for i, (ci, co) in enumerate(shapes):
        q = [_zeros(ctx, nb) for nb in (36 * ci, 4 * ci, 4 * ci, 2 * ci * co, 4 * co, 4 * co)]
        arr[i].wd, arr[i].s2, arr[i].b2, arr[i].wp_bf16, arr[i].s3, arr[i].b3 = (t.ptr for t in q)
    return arr


@pytest.mark.parametrize("off", [4, 8])
def test_blocks_resident_bf16_refuses_interior_pointers(pkg, ctx, off):
    n, h, c = 1, 4, 256
    arr = _resident_params(pkg, ctx, [(c, c)])
    x, xo = _bf16_dev(pkg, ctx, np.zeros((n, h, h, c), np.float32)), _zeros(ctx, n * h * h * c * 2, off)
    out, outo = Slot(ctx, n * h * h * c * 2), Slot(ctx, n * h * h * c * 2, off)
    assert ctx.lib.mbn_blocks_resident_bf16(ctx.h, outo.ptr, x.ptr, arr, 1, n, h, h, c, None) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_blocks_resident_bf16(ctx.h, out.ptr, xo.ptr, arr, 1, n, h, h, c, None) == pkg.EUNSUPPORTED
    bad = _resident_params(pkg, ctx, [(c, c)])
    bad[0].b2 = _zeros(ctx, 4 * c, off).ptr
    assert ctx.lib.mbn_blocks_resident_bf16(ctx.h, out.ptr, x.ptr, bad, 1, n, h, h, c, None) == pkg.EUNSUPPORTED
    ctx.sync()
    assert out.untouched() and outo.untouched(), "a refused call launched something"
    assert ctx.lib.mbn_blocks_resident_bf16(ctx.h, out.ptr, x.ptr, arr, 1, n, h, h, c, None) == pkg.OK
    ctx.sync()
    assert not out.untouched()
    x.free()


@pytest.mark.parametrize("off", [4, 8])
def test_tail_resident_bf16_refuses_interior_pointers(pkg, ctx, off):
    """The input and the parameters are loaded 16 bytes at a time: off that, MBN_EUNSUPPORTED. The pooled output is stored per bf16 element and
    may sit on any of them."""
    n, h, c0, c1 = 1, 4, 256, 512
    arr = _resident_params(pkg, ctx, [(c0, c1), (c1, c1)])
    bad = _resident_params(pkg, ctx, [(c0, c1), (c1, c1)])
    bad[1].s3 = _zeros(ctx, 4 * c1, off).ptr
    x, xo = _zeros(ctx, n * h * h * c0 * 2), _zeros(ctx, n * h * h * c0 * 2, off)
    out, outo = Slot(ctx, n * c1 * 2), Slot(ctx, n * c1 * 2, off)
    assert ctx.lib.mbn_tail_resident_bf16(ctx.h, out.ptr, xo.ptr, arr, n, h, h, c0, c1, None) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_tail_resident_bf16(ctx.h, out.ptr, x.ptr, bad, n, h, h, c0, c1, None) == pkg.EUNSUPPORTED
    ctx.sync()
    assert out.untouched(), "a refused call launched something"
    assert ctx.lib.mbn_tail_resident_bf16(ctx.h, out.ptr, x.ptr, arr, n, h, h, c0, c1, None) == pkg.OK
    assert ctx.lib.mbn_tail_resident_bf16(ctx.h, outo.ptr, x.ptr, arr, n, h, h, c0, c1, None) == pkg.OK
    ctx.sync()
    a, b = out.read((n, c1), np.uint16, "resident tail"), outo.read((n, c1), np.uint16, "resident tail, out + %d" % off)
    assert np.array_equal(a, b) and (a != 0xFFFF).all()


@pytest.mark.parametrize("off", [4, 8])
def test_pool_fc_refuses_interior_pointers(pkg, ctx, off):
    """The filter and the workspace off 16 bytes: MBN_EUNSUPPORTED (the caller runs mbn_pool + mbn_pointwise). The map and the logits are read and
    written per element."""
    n, h, ch, classes = 1, 2, 64, 16
    nb = ctx.lib.mbn_pool_fc_workspace_bytes(ch, classes)
    x, w, wo, b = _zeros(ctx, n * h * h * ch * 4), _zeros(ctx, classes * ch * 4), _zeros(ctx, classes * ch * 4, off), _zeros(ctx, classes * 4)
    ws, wso = _zeros(ctx, nb), _zeros(ctx, nb, off)
    out = Slot(ctx, n * classes * 4)
    assert ctx.lib.mbn_pool_fc(ctx.h, out.ptr, x.ptr, wo.ptr, b.ptr, n, h, h, ch, classes, ws.ptr, nb, None) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_pool_fc(ctx.h, out.ptr, x.ptr, w.ptr, b.ptr, n, h, h, ch, classes, wso.ptr, nb, None) == pkg.EUNSUPPORTED
    ctx.sync()
    assert out.untouched(), "a refused call launched something"
    assert ctx.lib.mbn_pool_fc(ctx.h, out.ptr, x.ptr, w.ptr, b.ptr, n, h, h, ch, classes, ws.ptr, nb, None) == pkg.OK
    ctx.sync()
    assert (out.read((n, classes), np.float32, "pool_fc") == 0).all()


@pytest.mark.parametrize("off", [4, 8])
def test_convert_f32_to_bf16_refuses_interior_pointers(pkg, ctx, off):
    """Source off 16 bytes or destination off 8: MBN_EINVAL (mbn.h)."""
    count = 100
    src, srco = _zeros(ctx, count * 4), _zeros(ctx, count * 4, off)
    dst, dsto = Slot(ctx, count * 2), Slot(ctx, count * 2, 4)
    assert ctx.lib.mbn_convert_f32_to_bf16(ctx.h, dst.ptr, srco.ptr, count, None) == pkg.EINVAL
    assert ctx.lib.mbn_convert_f32_to_bf16(ctx.h, dsto.ptr, src.ptr, count, None) == pkg.EINVAL
    ctx.sync()
    assert dst.untouched() and dsto.untouched(), "a refused call launched something"
    assert ctx.lib.mbn_convert_f32_to_bf16(ctx.h, dst.ptr, src.ptr, count, None) == pkg.OK
    ctx.sync()
    assert (dst.read((count,), np.uint16, "convert") == 0).all()
    # the other direction converts per element: a bf16 source 2 bytes off into an fp32 destination 4 bytes off
    vals = np.arange(count, dtype=np.float32) - 50
    b16, f32o = Slot(ctx, count * 2, 2, pkg.f32_to_bf16_bits(vals)), Slot(ctx, count * 4, 4)
    assert ctx.lib.mbn_convert_bf16_to_f32(ctx.h, f32o.ptr, b16.ptr, count, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(f32o.read((count,), np.float32, "convert bf16 -> fp32"), vals)


@pytest.mark.parametrize("off", [4, 8])
def test_normalize_u8_to_f32_refuses_interior_pointers(pkg, ctx, off):
    """Output off 16 bytes or the uint8 input off 4: MBN_EINVAL (mbn.h)."""
    count = 100
    src, srco = _zeros(ctx, count), _zeros(ctx, count, 2)
    dst, dsto = Slot(ctx, count * 4), Slot(ctx, count * 4, off)
    assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, dsto.ptr, src.ptr, count, 1 / 127.5, -1.0, None) == pkg.EINVAL
    assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, dst.ptr, srco.ptr, count, 1 / 127.5, -1.0, None) == pkg.EINVAL
    ctx.sync()
    assert dst.untouched() and dsto.untouched(), "a refused call launched something"
    assert ctx.lib.mbn_normalize_u8_to_f32(ctx.h, dst.ptr, src.ptr, count, 1 / 127.5, -1.0, None) == pkg.OK
    ctx.sync()
    assert (dst.read((count,), np.float32, "normalize") == -1.0).all()


# ------------------------------------------------------------------------------------------------------------ net runner

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_net_forward_into_misaligned_buffers(pkg, ctx, tmp_path, dtype):
    """The case mbn_net_launches leaves open: `logits` / the last-layer buffer off 16 bytes. A fused launch that would write there answers
    MBN_EUNSUPPORTED and its layers run one by one; the single layers take whatever kernel the pointer allows. fp32: the same bits as the forward
    into an aligned buffer (the kernels of these layers — pw_gemm, the split-K kernel — do not look at `out`); bf16: within the network tolerance
    (a fused block becomes two launches, the streaming GEMM becomes pw_gemm). Nothing is written in front of or behind the tensor."""
    n, classes, res, bf = 3, 10, 64, dtype == "bf16"
    hw = _weights(pkg, tmp_path, 0.25, res, res, classes)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    if bf:
        net.set_dtype(pkg.DT_BF16)
    d_in = ctx.to_device(_images(n, res, res, 7))
    for last in (0, 3, 5, 27):
        l = hw.plan.layer[(last or hw.plan.n_layers) - 1]
        shape = (n, l.out_rows, l.out_cols, l.out_ch)
        b16 = bf and last != 0                               # activations are bf16, the logits stay fp32
        raw, es = (np.uint16, 2) if b16 else (np.uint32, 4)
        nb = int(np.prod(shape)) * es
        outs = []
        for off in [0, 4] + ([2] if b16 else []):
            o = Slot(ctx, nb, off)
            net.forward(d_in.ptr, o.ptr, n, last)
            ctx.sync()
            outs.append(o.read(shape, raw, "%s net, layer %d into buffer + %d" % (dtype, last, off)))
            o.free()
        val = pkg.bf16_bits_to_f32 if b16 else (lambda r: r.view(np.float32))
        assert float(np.abs(val(outs[0])).max()) > 0
        for got in outs[1:]:
            if bf:
                assert_close(val(got), val(outs[0]), TOL_BF16_NET, "bf16 net, layer %d into a misaligned buffer" % last)
            else:
                assert np.array_equal(got, outs[0]), "fp32 net, layer %d: a misaligned output buffer changes the result" % last
    net.destroy()
    hw.free()
