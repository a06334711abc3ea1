"""Every bf16 kernel (and the fp32 kernels that share its epilogues) bit for bit on exactly representable data.

tests/exact_ref.py builds inputs for which every product and partial sum of a layer is exact in fp32 in any order, with a
power-of-two scale and a 2^-7-grid shift per channel; the kernel's output must then equal bf16_rne(clip(exact, 0, 6)) — or the
exact fp32 value — bit for bit. No tolerance anywhere: a dropped k-term, a neighbouring channel's scale or shift, a clamp at the
wrong place, truncation, a wrong tie, an unrounded intermediate or a low-precision accumulator is a failed array_equal.
tests/test_exact_cpu.py passes every case of the lists below through the gate (sum|terms| < 2^24 grid units, fp32 evaluation in
two orders equal to float64, coverage of the clamps, of rounding and of ties) and shows that the six mutants are caught.

Each test is one kernel call with a 0xFF canary behind the output. Lab knobs skip on the shipped library.
"""
import functools

import numpy as np
import pytest

import exact_ref as E

pytestmark = pytest.mark.gpu

# ----------------------------------------------------------------------------- the cases (test_exact_cpu.py gates every one of them)

# (M, K, N). Default dispatch: the streaming kernel for K <= 128 (M >= 512), its 16x16x32 form from K = 256 up at every M; ragged last row tiles,
# more than one column group, more than one k-tile. (549, 64, 128) is also the lab ring kernel's shape (K = 64). The streaming kernel is persistent
# (2 workgroups per CU over 128 x 128 tiles): the first five shapes have 5 ... 16 tiles, one per workgroup at most; the two 16677-row shapes
# have 131 x 4 = 524 tiles, more than the 512 workgroups of a 256-CU part, so some workgroups walk on to a second tile (both MFMA forms).
PW_DEFAULT = [(512 + 37, 64, 128), (640, 192, 384), (2 * 196 + 5, 256, 256), (300, 512, 512), (3 * 49 + 1, 1024, 1024),
              (130 * 128 + 37, 64, 512), (130 * 128 + 37, 256, 512)]
PW_GENERIC = [(130, 8, 24), (77, 72, 40), (64, 6, 10)]       # pw_gemm<bf16> with ragged N, single k-tile, and the one-lane-per-element kernel (K = 6)
PW_FC = (5, 1024, 1000)
# lab routes: (knobs, shape, packed filter). pw_ring 1 = pw_gemm<bf16>, 2 = ring kernel, 4 = streaming kernel (32x32x16 form) wherever eligible,
# 6 = wide kernel (packed filter), 7 = big tile, 8 = register-filter kernel; misc 16 = the streaming kernel's 16x16x32 form on a short K.
# (misc = 32 is read by the fused block kernel only — see test_bf16_dwpw_fused_16x16x32_form_exact; for a pointwise call it changes nothing, so
# there is no such case here: the pointwise 16x16x32 routes are misc 16 and every K >= 256 shape of PW_DEFAULT.)
PW_LAB = [({"pw_ring": 1}, (549, 64, 128), False), ({"pw_ring": 1}, (397, 256, 256), False), ({"pw_ring": 1}, (300, 512, 512), False),
          ({"pw_ring": 2}, (549, 64, 128), False), ({"pw_ring": 2}, (640, 192, 384), False),
          ({"pw_ring": 4}, (549, 64, 128), False), ({"pw_ring": 4}, (640, 192, 384), False),
          ({"pw_ring": 6}, (4 * 196, 256, 256), True),
          ({"pw_ring": 7}, (66000, 128, 256), False),
          ({"pw_ring": 8}, (31, 512, 256), False), ({"pw_ring": 8}, (7 * 32 + 3, 512, 768), False),
          ({"pw_ring": 4, "misc": 16}, (549, 64, 128), False)]


def pw_route_eligible(knobs, shape, cus=256, act=2):
    """The envelope of the kernel a knob forces, copied from its launcher (which answers MBN_EUNSUPPORTED outside it and lets the call fall through
    to another kernel WITHOUT a sign): a forced-route case outside its envelope would test the default kernel twice. Checked for every case on the
    CPU side and, with the device's CU count, before every forced call. Buffers here are 16-byte aligned and far below the 32-bit offset limits.
      pw_ring 2  mbn_bf16_pw_ring.hip      ReLU6; K % 64 == 0; N % 128 == 0, N <= 1024; M >= 4 * (256 if K >= 256 else 128)
      pw_ring 4  mbn_bf16_pw_stream.hip    ReLU6; K % 64 == 0; N % 128 == 0; M >= 512   (+ misc 16: the same envelope, the 16x16x32 form)
      pw_ring 6  mbn_bf16_pw_wide.hip      ReLU6; packed filter; K in {256, 512, 1024}; N % 256 == 0; M >= 4 * 196
      pw_ring 7  mbn_launch_bf16_pw_big    ReLU6; K % 64 == 0, K >= 128; N % 256 == 0; whole rounds: floor(M / 256) * (N / 256) >= CUs
      pw_ring 8  mbn_bf16_pw_rf.hip        ReLU6; K == 512; N % 256 == 0; CUs >= 8 * N / 256
      pw_tile 9  mbn_f32_pw3.hip           fp32 ReLU6; K in {64, 128, 256, 512}; N % (64 if K == 512 else 128) == 0, N <= 1024; CUs >= 8 * slices
      pw_splitk 2  mbn_f32_pw_splitk.hip   fp32; K >= 128, K % 64 == 0; M <= 65536
      pw_emul 6  mbn_f32_pw_x6.hip         fp32; K % 32 == 0; with pw_tile 0 at least CUs tiles of 128 x 128 (fewer: pw_gemm fills the chip better), with a
                                           forced tile (11 = pre-split filter, 6, 7; pw_splitk 1 keeps split-K away, as test_parity_gpu.py's _emul_modes) any M, N"""
    m, k, n = shape
    ring = knobs.get("pw_ring", 0)
    if ring in (2, 4, 6, 7, 8) and act != 2:
        return False
    if ring == 2:
        return k % 64 == 0 and n % 128 == 0 and n <= 1024 and m >= 4 * (256 if k >= 256 else 128)
    if ring == 4:
        return k % 64 == 0 and n % 128 == 0 and m >= 512
    if ring == 6:
        return k in (256, 512, 1024) and n % 256 == 0 and m >= 4 * 196
    if ring == 7:
        tiles = (m // 256) * (n // 256) // cus * cus if n % 256 == 0 else 0
        return k % 64 == 0 and k >= 128 and n % 256 == 0 and tiles - tiles % (n // 256) >= cus       # (whole rounds, then whole row tiles)
    if ring == 8:
        return k == 512 and n % 256 == 0 and cus >= 8 * (n // 256)
    if knobs.get("pw_emul"):
        return k % 32 == 0 and (knobs.get("pw_tile") in (6, 7, 11) or -(-m // 128) * -(-n // 128) >= cus)
    if knobs.get("pw_tile") == 9:
        bn = 64 if k == 512 else 128
        return act == 2 and k in (64, 128, 256, 512) and n % bn == 0 and n <= 1024 and cus // (8 * (n // bn)) >= 1
    if knobs.get("pw_splitk") == 2:
        return k >= 128 and k % 64 == 0 and m <= 65536
    return True


def dw_lds_eligible(shape):
    """exp0 = 8, launch_dw_lds_bf16 (mbn_f32_dw.hip): stride 1 on an unpadded-size map (SAME pads of 1), channels % 64 == 0, one image row with its borders
    in a 64-pixel LDS ring row: ((cols + 3) & ~1) <= 64. Outside it the register kernel runs, silently."""
    n, h, c = shape
    return c % 64 == 0 and ((h + 3) & ~1) <= 64


# (batch, side, channels, stride, geometry)
DW_CASES = [(1, 9, 8, 2, {}), (1, 10, 6, 1, {}), (2, 14, 512, 1, {}), (2, 28, 64, 2, {}), (2, 7, 1024, 1, {}),
            (2, 12, 64, 2, dict(pad_top=1, pad_left=1)),
            (2, 14, 64, 1, dict(dilation=2)), (2, 14, 64, 1, dict(dilation=4))]
DW_LAB = [(3, 9, 64), (4, 14, 64)]                           # exp0 = 8: the LDS-staged form, dw_nseg 0 and 2
POOL_CASES = [(3, 4, 512), (2, 8, 256), (1, 2, 30)]

# (batch, side, Cin, Cout, stride)
BLOCK_CASES = [(1, 10, 32, 64, 1), (3, 14, 64, 128, 1), (3, 20, 64, 192, 2), (2, 28, 256, 256, 1), (1, 28, 256, 512, 2), (2, 14, 512, 512, 1)]
BLOCK_ASYM_N, BLOCK_ASYM_H, BLOCK_ASYM_W = 9, 6, 10          # as test_parity_gpu.py's DWPW_ASYM_*: tiles that span several images
BLOCK_ASYM = [((1, 1, 0, 6, 8), (64, 128)), ((2, 0, 1, 3, 6), (64, 128))]      # ((stride, pad_top, pad_left, out_rows, out_cols), (Cin, Cout))

# (batch, rows, cols, blocks); 600 images: four distinct ones tiled, so every pass of the persistent grid is checked exactly
RES_CASES = [(3, 10, 10, 1), (2, 7, 9, 1), (2, 6, 16, 1), (2, 1, 1, 1), (3, 10, 10, 2), (3, 10, 10, 3), (2, 6, 16, 2), (2, 6, 16, 3), (600, 10, 10, 1),
             (3, 10, 10, 5), (3, 10, 10, 8)]
TAIL_CASES = [(3, 8, 8), (2, 4, 4), (5, 8, 4)]               # pooled map 4 x 4, 2 x 2, 4 x 2: a power of two, the mean is exact
# (batch, rows, cols, c1, c3): alpha 1.0 and 0.5 at 32 x 32 and 32 x 64. The conv1 filter is fully dense (27 live taps): the gate is met as is.
STEM_CASES = [(2, 32, 32, 32, 64), (2, 32, 64, 32, 64), (2, 32, 32, 16, 32), (2, 32, 64, 16, 32)]

# fp32 pointwise (knobs, shape): the default dispatch on the three shapes; the forced routes only where their kernel takes the call (pw_route_eligible):
# (127, 36, 100) and (64, 6, 10) are outside every forced kernel's envelope and would run the default kernel again. pw_emul 6 on (1568, 128, 256)
# with each tile the shipped library has, and through its own dispatch on a shape with 128 x 2 = 256 tiles of 128 x 128 (K = 32: one k-tile).
F32_PW = [(2 * 784, 128, 256), (127, 36, 100), (64, 6, 10)]
F32_PW_EMUL_DEFAULT = (16384, 32, 256)
F32_PW_ROUTES = [({}, s) for s in F32_PW] + [({"pw_tile": 9}, F32_PW[0]), ({"pw_splitk": 2}, F32_PW[0])] + \
                [({"pw_emul": 6, "pw_splitk": 1, "pw_tile": t}, F32_PW[0]) for t in (11, 6, 7)] + [({"pw_emul": 6}, F32_PW_EMUL_DEFAULT)]
F32_DW = [(2, 11, 12, 2), (2, 28, 256, 1)]
F32_BLOCK = [(3, 14, 32, 128, 1), (5, 12, 96, 128, 2), (1, 28, 256, 512, 2)]
F32_CONV1 = [(2, 32, 32), (1, 33, 8)]                        # (batch, side, Cout)


@functools.lru_cache(maxsize=2)
def pw_layer(shape, act=2, fc=False, rounded=True):
    return E.pw_case(*shape, act=act, fc=fc, rounded=rounded)[0]


def dw_layer(case, rounded=True):
    n, h, c, stride, geom = case
    return E.dw_case(n, h, c, stride, rounded=rounded, **geom)[0]


def block_layers(shape, rounded=True):
    n, h, cin, cout, stride = shape
    return E.block_case(n, h, h, cin, cout, stride, rounded=rounded)


def block_asym_layers(case):
    (stride, pt, pl, oh, ow), (cin, cout) = case
    return E.block_case(BLOCK_ASYM_N, BLOCK_ASYM_H, BLOCK_ASYM_W, cin, cout, stride, pad_top=pt, pad_left=pl, out_rows=oh, out_cols=ow)


def res_layers(case):
    n, h, w, nblk = case
    return E.chain_case(n, h, w, [256] * (nblk + 1), [1] * nblk, images=4 if n > 16 else None)


def tail_layers(case):
    n, h, w = case
    return E.chain_case(n, h, w, [256, 512, 512], [2, 1], pool=True)


def stem_layers(case):
    return E.stem_case(*case)


# ----------------------------------------------------------------------------- helpers

def _lab(ctx):
    return ctx.lib.mbn_lab_build() == 1


def _tune_lab(ctx, key, value):
    """mbn_tune_set of a lab knob: skips the test on the shipped library (MBN_EUNSUPPORTED there by design)."""
    rc = ctx.lib.mbn_tune_set(key, value)
    if rc == -8:
        pytest.skip("lab knob %s: this is the shipped libmbn.so (run with MBN_LAB=1 for the lab build)" % key.decode())
    assert rc == 0, rc


LAB_KNOBS = ("pw_ring", "misc", "exp0", "dw_nseg", "dwpw_variant", "pw_xn", "exp1", "exp2")
MBN_STEM_BF16 = 2                                            # include/mbn.h


def _cus(ctx):
    import ctypes
    n = ctypes.c_int()
    assert ctx.lib.mbn_device_cus(ctx.h, ctypes.byref(n)) == 0
    return n.value


class Knobs:
    """mbn_tune_set for the body of a with block, everything back to 0 afterwards. Lab knobs skip on the shipped library before anything is set."""

    def __init__(self, ctx, knobs):
        self.ctx, self.knobs = ctx, knobs

    def __enter__(self):
        try:
            for k in sorted(self.knobs, key=lambda k: k not in LAB_KNOBS):      # lab knobs first: a skip on the shipped library comes before anything is set
                if k in LAB_KNOBS:
                    _tune_lab(self.ctx, k.encode(), self.knobs[k])
                else:
                    assert self.ctx.lib.mbn_tune_set(k.encode(), self.knobs[k]) == 0, k
        except BaseException:                                                   # a with block does not call __exit__ when __enter__ raises
            self.__exit__()
            raise

    def __exit__(self, *a):
        for k in self.knobs:
            self.ctx.lib.mbn_tune_set(k.encode(), 0)


class Dev:
    """Device buffers of one test, freed at the end of the with block."""

    def __init__(self, pkg, ctx):
        self.pkg, self.ctx, self.bufs = pkg, ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for b in self.bufs:
            b.free()

    def f32(self, a):
        a = np.asarray(a, np.float64)
        f = a.astype(np.float32)
        assert np.array_equal(f.astype(np.float64), a)
        self.bufs.append(self.ctx.to_device(f))
        return self.bufs[-1]

    def bf16(self, a):
        bits = E.bf16_rne_bits(a)
        assert np.array_equal(E.bf16_value(bits), np.asarray(a, np.float64)), "operand is not a bf16 value"
        self.bufs.append(self.ctx.to_device(bits))
        return self.bufs[-1]

    def packed(self, w):
        buf, flag = self.pkg.packed_filter_dev(self.ctx, np.asarray(w, np.float32))
        self.bufs.append(buf)
        return buf, flag

    def out(self, count, itemsize):
        """output of `count` elements with 64 bytes of 0xFF behind it (and under it)"""
        self.bufs.append(self.ctx.alloc(count * itemsize + 64))
        self.ctx.lib.mbn_memset(self.ctx.h, self.bufs[-1].ptr, 0xFF, count * itemsize + 64)
        return self.bufs[-1]

    def fetch(self, buf, count, dtype):
        self.ctx.sync()
        raw = buf.download((count * np.dtype(dtype).itemsize + 64,), np.uint8)
        assert np.all(raw[-64:] == 0xFF), "stores past the output"
        return raw[:-64].view(dtype)

    def params(self, l):
        """(wd or bf16 wp, scale, shift) of a layer on the device; None for a scale or shift the layer does not have (the call then passes NULL)"""
        w = self.bf16(l.w) if l.kind == "pw" else self.f32(l.w)
        return w, self.opt_f32(l.scale), self.opt_f32(l.shift)

    def opt_f32(self, a):
        return None if a is None else self.f32(a)


def ptr(buf):
    """the device pointer of a buffer, NULL for None"""
    return None if buf is None else buf.ptr


def same_bits(got, want, what):
    """array_equal on bit patterns; on failure the count and the first (index, got, want) triples"""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        as_f = (lambda b: float(E.bf16_value(np.array([b], np.uint16))[0])) if got.dtype == np.uint16 else (lambda b: float(np.array([b], np.uint32).view(np.float32)[0]))
        first = ["(%d, %#x = %r, %#x = %r)" % (i, got[i], as_f(got[i]), want[i], as_f(want[i])) for i in bad[:8]]
        print("%s: %d of %d differ; first (index, got, want): %s" % (what, bad.size, got.size, ", ".join(first)))
    assert bad.size == 0, "%s: %d of %d elements differ" % (what, bad.size, got.size)


def want_bits(pkg, l):
    """the layer's expected output: bf16 bits of the exact value (through the package's own host helper), or its fp32 bits"""
    y32 = l.y.astype(np.float32)
    assert np.array_equal(y32.astype(np.float64), l.y)
    return pkg.f32_to_bf16_bits(y32) if l.rounded else y32.view(np.uint32)


def block_params(dev, layers):
    """BlockParams array of a chain's (depthwise, pointwise) pairs"""
    pairs = [(layers[i], layers[i + 1]) for i in range(0, len(layers) - 1, 2) if layers[i].kind == "dw"]
    arr = (dev.pkg.BlockParams * len(pairs))()
    for i, (d, p) in enumerate(pairs):
        (wd, s2, b2), (wp, s3, b3) = dev.params(d), dev.params(p)
        arr[i].wd, arr[i].s2, arr[i].b2, arr[i].wp_bf16, arr[i].s3, arr[i].b3 = wd.ptr, s2.ptr, b2.ptr, wp.ptr, s3.ptr, b3.ptr
    return arr


# ----------------------------------------------------------------------------- bf16 pointwise

def _run_pw(pkg, ctx, l, knobs=None, packed=False, dtype=None, in_envelope=True):
    """One pointwise call, compared with the layer's exact bits; returns the bits. in_envelope False: the caller has shown that the forced kernel does
    NOT take this call (a planning CU count outside its envelope) and checks whatever kernel does."""
    m, k = l.x.reshape(-1, l.x.shape[-1]).shape
    n = l.w.shape[0]
    bf = dtype != "f32"
    assert pw_route_eligible(knobs or {}, (m, k, n), _cus(ctx), l.act) == in_envelope, "the forced kernel would %stake this call on this device: %s %s" % ("not " if in_envelope else "", knobs, (m, k, n))
    with Dev(pkg, ctx) as dev, Knobs(ctx, knobs or {}):
        d_x = dev.bf16(l.x) if bf else dev.f32(l.x)
        flag = 0
        if packed:
            d_f, flag = dev.packed(l.w)
            assert flag == pkg.IO_FILT_PACKED
        else:
            d_f = dev.bf16(l.w) if bf else dev.f32(l.w)
        d_sc, d_sh = dev.opt_f32(l.scale), dev.opt_f32(l.shift)
        out_f32 = not l.rounded
        d_o = dev.out(m * n, 4 if out_f32 else 2)
        ext = pkg.make_ext(dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=l.act, scale=ptr(d_sc), shift=ptr(d_sh),
                           io_flags=flag | (pkg.IO_OUT_F32 if (bf and out_f32) else 0))
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, k, n, ext)
        got = dev.fetch(d_o, m * n, np.uint32 if out_f32 else np.uint16)
    same_bits(got, want_bits(pkg, l), "pointwise (%d, %d, %d) act %d %s" % (m, k, n, l.act, knobs or ""))
    return got


@pytest.mark.parametrize("act", [2, 0])
@pytest.mark.parametrize("shape", PW_DEFAULT + PW_GENERIC)
def test_bf16_pointwise_exact(pkg, ctx, shape, act):
    """mbn_pointwise, DT_BF16, default dispatch. act 2: the streaming kernels' channel-paired epilogues (scale / shift index, clamp, RNE); act 0 takes
    pw_gemm<bf16>'s general epilogue, where values beyond +-6 pin the unclamped sign and magnitude."""
    _run_pw(pkg, ctx, pw_layer(shape, act))


def test_bf16_pointwise_fc_form_exact(pkg, ctx):
    """IO_OUT_F32, scale NULL, shift given, act 0: the fp32 bits of the unrounded exact value."""
    _run_pw(pkg, ctx, pw_layer(PW_FC, 0, True))


@pytest.mark.parametrize("case", PW_LAB, ids=lambda c: "%s-%s" % ("-".join("%s%d" % kv for kv in sorted(c[0].items())), "x".join(map(str, c[1]))))
def test_bf16_pointwise_lab_routes_exact(pkg, ctx, case):
    """LAB: every other bf16 pointwise kernel forced on the smallest shape it is eligible for (see PW_LAB)."""
    knobs, shape, packed = case
    _run_pw(pkg, ctx, pw_layer(shape), knobs, packed)


# ----------------------------------------------------------------------------- bf16 depthwise, pool

def _run_dw(pkg, ctx, l, knobs=None, dtype=None):
    n, h, w, c = l.x.shape
    g = l.geom
    oh, ow = l.acc.shape[1:3]
    bf = dtype != "f32"
    with Dev(pkg, ctx) as dev, Knobs(ctx, knobs or {}):
        d_x = dev.bf16(l.x) if bf else dev.f32(l.x)
        d_f, d_sc, d_sh = dev.params(l)
        d_o = dev.out(l.y.size, 2 if bf else 4)
        ext = pkg.make_ext(batch=n, dtype=pkg.DT_BF16 if bf else pkg.DT_F32, act=l.act, in_rows=h, in_cols=w, scale=ptr(d_sc), shift=ptr(d_sh),
                           pad_top=g.get("pad_top", -1), pad_left=g.get("pad_left", -1), dilation=g.get("dilation", 0))
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, oh, ow, 3, g["stride"], c, ext)
        got = dev.fetch(d_o, l.y.size, np.uint16 if bf else np.uint32)
    same_bits(got, want_bits(pkg, l), "depthwise %s %s %s" % (l.x.shape, g, knobs or ""))
    return got


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: "%dx%dx%d-s%d%s" % (c[0], c[1], c[2], c[3], "".join("-%s%d" % kv for kv in sorted(c[4].items()))))
def test_bf16_depthwise_exact(pkg, ctx, case):
    """mbn_depthwise, DT_BF16: the 8-channel register kernel, the generic one (6 channels), stride 2, explicit top / left pads, and the dilated
    kernel's bf16 form at rates 2 and 4. All nine taps live and different per channel, per-channel scale and shift."""
    _run_dw(pkg, ctx, dw_layer(case))


@pytest.mark.parametrize("nseg", [0, 2])
@pytest.mark.parametrize("shape", DW_LAB)
def test_bf16_depthwise_lds_staged_form_exact(pkg, ctx, shape, nseg):
    """LAB (exp0 = 8): the LDS-staged bf16 depthwise kernel, whole rows and two row segments."""
    n, h, c = shape
    assert dw_lds_eligible(shape)
    _run_dw(pkg, ctx, dw_layer((n, h, c, 1, {})), {"exp0": 8, "dw_nseg": nseg})


@pytest.mark.parametrize("shape", POOL_CASES)
def test_bf16_pool_exact(pkg, ctx, shape):
    """mbn_pool, DT_BF16, whole-map mean of a 4 x 4 / 8 x 8 / 2 x 2 map: the sum and the division by a power of two are exact, the result rounds to bf16 (RNE)."""
    n, h, c = shape
    l = E.pool_layer(E.pool_case(n, h, c))
    with Dev(pkg, ctx) as dev:
        d_x, d_o = dev.bf16(l.x), dev.out(n * c, 2)
        ctx.pool(d_o.ptr, d_x.ptr, h, h, h, c, pkg.make_ext(batch=n, dtype=pkg.DT_BF16, act=0))
        got = dev.fetch(d_o, n * c, np.uint16)
    same_bits(got, want_bits(pkg, l), "pool %s" % (shape,))


# ----------------------------------------------------------------------------- bf16 fused block, resident blocks, resident tail, fused stem

def _run_block(pkg, ctx, layers, knobs=None, dtype=None):
    d, p = layers
    n, h, w, cin = d.x.shape
    oh, ow = d.acc.shape[1:3]
    cout = p.w.shape[0]
    bf = dtype != "f32"
    _, _, pt, pl = E.dw_geom(h, w, **d.geom)
    with Dev(pkg, ctx) as dev, Knobs(ctx, knobs or {}):
        d_x = dev.bf16(d.x) if bf else dev.f32(d.x)
        wd, s2, b2 = dev.params(d)
        wp = dev.bf16(p.w) if bf else dev.f32(p.w)
        s3, b3 = dev.f32(p.scale), dev.f32(p.shift)
        d_o = dev.out(p.y.size, 2 if bf else 4)
        fn = ctx.lib.mbn_dwpw_fused_bf16 if bf else ctx.lib.mbn_dwpw_fused
        rc = fn(ctx.h, d_o.ptr, d_x.ptr, wd.ptr, s2.ptr, b2.ptr, wp.ptr, s3.ptr, b3.ptr, n, h, w, oh, ow, cin, cout, d.geom["stride"], pt, pl, None)
        assert rc == 0, rc
        got = dev.fetch(d_o, p.y.size, np.uint16 if bf else np.uint32)
    same_bits(got, want_bits(pkg, p), "fused block %s -> %s %s %s" % (d.x.shape, p.y.shape, d.geom, knobs or ""))
    return got


@pytest.mark.parametrize("shape", BLOCK_CASES)
def test_bf16_dwpw_fused_exact(pkg, ctx, shape):
    """mbn_dwpw_fused_bf16: nine live depthwise taps, per-channel BN on both stages, the depthwise intermediate rounded to bf16 as the contract says
    (the reference that skips that rounding differs in well over 1 % of the outputs: test_exact_cpu.py), 256- and 128-row tiles, Cin = 32 (half a K chunk),
    Cout = 64 and 192 (a padded column tile), both strides."""
    _run_block(pkg, ctx, block_layers(shape))


@pytest.mark.parametrize("case", BLOCK_ASYM, ids=lambda c: "s%d-pt%d-pl%d" % c[0][:3])
def test_bf16_dwpw_fused_asymmetric_pads_exact(pkg, ctx, case):
    """The same with padding on one side only and tiles that span several 6 x 10 images, one case per stride."""
    _run_block(pkg, ctx, block_asym_layers(case))


@pytest.mark.parametrize("shape", BLOCK_CASES[:3])
def test_bf16_dwpw_fused_16x16x32_form_exact(pkg, ctx, shape):
    """LAB (misc = 32): the block kernel's pointwise products on v_mfma_f32_16x16x32_bf16 (mbn_store_relu6_bf16_pair16's channel pairing)."""
    _run_block(pkg, ctx, block_layers(shape), {"misc": 32})


@pytest.mark.parametrize("case", RES_CASES, ids=lambda c: "%dx%dx%d-%dblk" % c)
def test_bf16_blocks_resident_exact(pkg, ctx, case):
    """mbn_blocks_resident_bf16, runs of 1, 2 and 3 blocks (256 channels), and the network's run of 5 and the envelope's 8. Later blocks take sparser
    filters (exact_ref.chain_case): the operand grid refines by a few bits per layer at first and then settles near 2^-16, because the bf16 rounding of
    every layer output drops the fine bits of all but its smallest values — the gate measures max sum|terms| = 2^22.2 grid units for 2, 3, 5 and 8 blocks
    alike (test_exact_cpu.py asserts it below 2^24 for each). 600 images are four distinct ones tiled: every image of every pass of the persistent grid
    is compared."""
    _run_res(pkg, ctx, case, res_layers(case))


def _run_res(pkg, ctx, case, layers):
    n, h, w, nblk = case
    x, y = layers[0].x, layers[-1]
    reps = -(-n // x.shape[0])
    with Dev(pkg, ctx) as dev:
        d_x = dev.bf16(np.tile(x, (reps, 1, 1, 1))[:n])
        arr = block_params(dev, layers)
        d_o = dev.out(n * h * w * 256, 2)
        rc = ctx.lib.mbn_blocks_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, nblk, n, h, w, 256, None)
        assert rc == 0, rc
        got = dev.fetch(d_o, n * h * w * 256, np.uint16)
    want = np.tile(want_bits(pkg, y).reshape(x.shape[0], -1), (reps, 1))[:n]
    same_bits(got, want, "resident blocks %s" % (case,))
    return got


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "%dx%dx%d" % c)
def test_bf16_tail_resident_exact(pkg, ctx, case):
    """mbn_tail_resident_bf16: depthwise stride 2 (256) -> pointwise 256 -> 512 -> depthwise -> pointwise 512 -> 512 -> whole-map mean, every stage
    rounded to bf16; the pooled map has a power-of-two pixel count, so the mean is exact before its rounding."""
    _run_tail(pkg, ctx, case, tail_layers(case))


def _run_tail(pkg, ctx, case, layers):
    n, h, w = case
    with Dev(pkg, ctx) as dev:
        d_x = dev.bf16(layers[0].x)
        arr = block_params(dev, layers)
        d_o = dev.out(n * 512, 2)
        rc = ctx.lib.mbn_tail_resident_bf16(ctx.h, d_o.ptr, d_x.ptr, arr, n, h, w, 256, 512, None)
        assert rc == 0, rc
        got = dev.fetch(d_o, n * 512, np.uint16)
    same_bits(got, want_bits(pkg, layers[-1]), "resident tail %s" % (case,))
    return got


@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: "%dx%dx%d-%d-%d" % c)
def test_bf16_fused_stem_exact(pkg, ctx, case):
    """mbn_stem_fused_hw with MBN_STEM_BF16 through the C-ABI: integer conv1 (all 27 taps live: no thinning was needed for the gate), depthwise and
    pointwise filters, the image on a 1/8 grid in [-1, 1], both on-chip intermediates rounded to bf16; alpha 1.0 and 0.5 channel counts, 32 x 32 and 32 x 64."""
    _run_stem(pkg, ctx, case, stem_layers(case))


def _run_stem(pkg, ctx, case, layers, dtype=None):
    """mbn_stem_fused_hw in bf16 (MBN_STEM_BF16) or, dtype "f32", in fp32 (layers built with rounded False: fp32 filter, fp32 bits out)"""
    n, rows, cols, c1, c3 = case
    a, d, p = layers
    bf = dtype != "f32"
    with Dev(pkg, ctx) as dev:
        d_img = dev.f32(a.x)
        w1, s1, b1 = dev.params(a)
        wd, s2, b2 = dev.params(d)
        wp, s3, b3 = dev.params(p) if bf else (dev.f32(p.w), dev.f32(p.scale), dev.f32(p.shift))
        d_o = dev.out(p.y.size, 2 if bf else 4)
        rc = ctx.lib.mbn_stem_fused_hw(ctx.h, d_o.ptr, d_img.ptr, w1.ptr, s1.ptr, b1.ptr, wd.ptr, s2.ptr, b2.ptr, wp.ptr, s3.ptr, b3.ptr,
                                       n, rows, cols, c1, c3, MBN_STEM_BF16 if bf else 0, None)
        assert rc == 0, rc
        got = dev.fetch(d_o, p.y.size, np.uint16 if bf else np.uint32)
    same_bits(got, want_bits(pkg, p), "%s fused stem %s" % ("bf16" if bf else "fp32", case))
    return got


# ----------------------------------------------------------------------------- fp32 kernels: same generators, nothing rounded

@pytest.mark.parametrize("route", F32_PW_ROUTES, ids=lambda r: "%s-%s" % ("-".join("%s%d" % kv for kv in sorted(r[0].items())) or "default", "x".join(map(str, r[1]))))
def test_f32_pointwise_exact(pkg, ctx, route):
    """mbn_pointwise in fp32 (mbn_store_relu6_f32's clamp and per-channel shift): default dispatch, the short-K resident-filter GEMM (pw_tile = 9), split-K
    forced on, and pw_emul = 6 (operands of at most 8 significant bits split exactly into bf16 planes: all six partial products are exact) on each of its
    shipped tiles and through its own dispatch. Every forced route runs on a shape inside its kernel's envelope (pw_route_eligible)."""
    knobs, shape = route
    _run_pw(pkg, ctx, pw_layer(shape, 2, False, False), knobs, dtype="f32")


@pytest.mark.parametrize("shape", F32_DW)
def test_f32_depthwise_exact(pkg, ctx, shape):
    n, h, c, stride = shape
    _run_dw(pkg, ctx, dw_layer((n, h, c, stride, {}), rounded=False), dtype="f32")


@pytest.mark.parametrize("shape", F32_BLOCK)
def test_f32_dwpw_fused_exact(pkg, ctx, shape):
    """mbn_dwpw_fused (mbn_store_relu6_f32_pair): fp32 bits of the exact pair, nothing rounded in between."""
    _run_block(pkg, ctx, block_layers(shape, rounded=False), dtype="f32")


@pytest.mark.parametrize("shape", F32_CONV1)
def test_f32_conv1_exact(pkg, ctx, shape):
    """fp32 conv1: the MFMA form (32 channels, 16 output columns) and the generic kernel (odd side, 8 channels)."""
    n, h, cout = shape
    (l,) = E.conv1_case(n, h, h, cout)
    with Dev(pkg, ctx) as dev:
        d_x = dev.f32(l.x)
        d_f, d_sc, d_sh = dev.params(l)
        d_o = dev.out(l.y.size, 4)
        ctx.convolute(d_o.ptr, d_x.ptr, None, None, d_f.ptr, h, h, 3, 2, cout, pkg.make_ext(batch=n, act=2, cin=3, scale=d_sc.ptr, shift=d_sh.ptr))
        got = dev.fetch(d_o, l.y.size, np.uint32)
    same_bits(got, want_bits(pkg, l), "conv1 %s" % (shape,))
