"""GPU tests of the int8 inference mode (MBN_DT_I8; arithmetic: include/mbn.h, "int8 inference mode"; numpy statement: tests/int8_ref.py).

Layer kernels (csrc/mbn_i8.hip) against the numpy integer reference bit for bit: every depthwise geometry of the network at three
widths plus odd maps, every pointwise (K, N) pair with a ragged pixel count, the FC with fp32 output, an exact GEMM with an asymmetric
filter, the pool; conv1 bit for bit on grid inputs whose fp32 sum is exact, and against float64 within one step otherwise; the pointwise forms and loop passes
chosen from the launch plan (mbn_i8_pw_plan) for the device's CU count. The net runner: every layer of a kept forward recomputed from the device's
previous layer, equivalences of streams / graph / last_layer, raw uint8 input, classify, the launch list, the C-ABI's error paths, and
the accuracy against the fp32 oracle. The new kernels index in 64 bits (no buffer descriptors), so they have no 32-bit offset guard."""
import ctypes as C

import numpy as np
import pytest

import int8_ref as ref

pytestmark = pytest.mark.gpu


def _ext(pkg, batch, scale=None, shift=None, act=None, io=0, in_rows=0, in_cols=0, cin=0, layout=None):
    e = pkg.make_ext(batch=batch, dtype=pkg.DT_I8, act=pkg.ACT_RELU6 if act is None else act, scale=scale, shift=shift, io_flags=io,
                     in_rows=in_rows, in_cols=in_cols, cin=cin)
    if layout is not None:
        e.layout = layout
    return e


def _params(ctx, rng, c, lo=2e-3, hi=8e-3):
    mult = rng.uniform(lo, hi, c).astype(np.float32)
    bias = rng.uniform(-40, 60, c).astype(np.float32)
    return mult, bias, ctx.to_device(mult), ctx.to_device(bias)


# the network's layer shapes (mbn_plan_build, host/mbn_plan.c): channels int(width * alpha), depthwise strides, maps from 224
_WIDTH = (32, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024)
_DSTRIDE = (1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1)


def _blocks(alpha, res=224):
    """(map, cin, cout, stride) of the 13 depthwise + pointwise blocks"""
    h, out = (res + 1) // 2, []
    for b in range(13):
        cin, cout = int(_WIDTH[b] * alpha), int(_WIDTH[b + 1] * alpha)
        out.append((h, cin, cout, _DSTRIDE[b]))
        h = (h + _DSTRIDE[b] - 1) // _DSTRIDE[b]
    return out


def _dw_geometries():
    out = set()
    for a in (1.0, 0.5, 0.25):
        out |= {(h, h, cin, s) for h, cin, _, s in _blocks(a)}
    out |= {(15, 15, 40, 2), (13, 9, 24, 1), (7, 11, 8, 2), (5, 5, 16, 1), (1, 1, 8, 2), (2, 3, 32, 1)}   # odd and tiny maps
    return sorted(out)


@pytest.mark.parametrize("geom", _dw_geometries())
def test_depthwise_bit_exact(pkg, ctx, geom):
    h, w, c, s = geom
    rng = np.random.default_rng(h * 7 + c + s)
    n = 2 if h * w * c <= 112 * 112 * 64 else 1
    x = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    wk = rng.integers(-127, 128, (3, 3, c), dtype=np.int8)
    mult, bias, dm, db = _params(ctx, rng, c)
    ho, wo = (h + s - 1) // s, (w + s - 1) // s
    dx, dw_, dout = ctx.to_device(x), ctx.to_device(wk), ctx.alloc(n * ho * wo * c)
    e = _ext(pkg, n, dm.ptr, db.ptr, in_rows=h, in_cols=w)
    ctx.depthwise(dout.ptr, dx.ptr, dw_.ptr, ho, wo, 3, s, c, e)
    ctx.sync()
    got = dout.download((n, ho, wo, c), np.uint8)
    want = ref.dw(x, wk, mult, bias, s)
    assert np.array_equal(got, want), "dw %s: %d of %d differ" % (geom, (got != want).sum(), got.size)
    assert 0 < got.mean() < 255
    for b in (dx, dw_, dout, dm, db):
        b.free()


def _pw_pairs():
    out = {(cin, cout) for a in (1.0, 0.5, 0.25) for _, cin, cout, _ in _blocks(a)}
    return sorted(out | {(8, 8), (16, 24), (1032, 40)})     # K = 1032: two K blocks of the largest form


@pytest.mark.parametrize("kn", _pw_pairs())
def test_pointwise_bit_exact(pkg, ctx, kn):
    k, nout = kn
    rng = np.random.default_rng(k * 3 + nout)
    m = 997 if k * nout <= 256 * 256 else 389                  # ragged: not a multiple of the 128-pixel tile
    x = rng.integers(0, 256, (m, k), dtype=np.uint8)
    wk = rng.integers(-127, 128, (nout, k), dtype=np.int8)
    mult, bias, dm, db = _params(ctx, rng, nout, 0.2 / k, 0.9 / k)
    dx, dw_, dout = ctx.to_device(x), ctx.to_device(wk), ctx.alloc(m * nout)
    ctx.pointwise(dout.ptr, dx.ptr, dw_.ptr, 1, m, k, nout, _ext(pkg, 1, dm.ptr, db.ptr))
    ctx.sync()
    got = dout.download((m, nout), np.uint8)
    want = ref.pw(x, wk, mult, bias)
    assert np.array_equal(got, want), "pw %s: %d of %d differ" % (kn, (got != want).sum(), got.size)
    assert 0 < got.mean() < 255
    for b in (dx, dw_, dout, dm, db):
        b.free()


def test_pointwise_operands_on_8_bytes(pkg, ctx):
    """Activations and filter 8- but not 16-byte aligned (interior pointers): the second GEMM form, same bits."""
    rng = np.random.default_rng(77)
    m, k, nout = 301, 64, 48
    x = rng.integers(0, 256, (m, k), dtype=np.uint8)
    wk = rng.integers(-127, 128, (nout, k), dtype=np.int8)
    mult, bias, dm, db = _params(ctx, rng, nout, 0.2 / k, 0.9 / k)
    dx, dw_, dout = ctx.alloc(m * k + 16), ctx.alloc(nout * k + 16), ctx.alloc(m * nout)
    pkg._chk(ctx.lib.mbn_upload(ctx.h, dx.ptr + 8, x.ctypes.data, x.nbytes))
    pkg._chk(ctx.lib.mbn_upload(ctx.h, dw_.ptr + 8, wk.ctypes.data, wk.nbytes))
    ctx.pointwise(dout.ptr, dx.ptr + 8, dw_.ptr + 8, 1, m, k, nout, _ext(pkg, 1, dm.ptr, db.ptr))
    ctx.sync()
    assert np.array_equal(dout.download((m, nout), np.uint8), ref.pw(x, wk, mult, bias))
    e = _ext(pkg, 1, dm.ptr, db.ptr)
    assert ctx.lib.mbn_pointwise(ctx.h, dout.ptr, dx.ptr + 4, dw_.ptr + 8, 1, m, k, nout, C.byref(e)) == pkg.EUNSUPPORTED   # 4 bytes: refused
    for b in (dx, dw_, dout, dm, db):
        b.free()


@pytest.mark.parametrize("k,nout,m", [(1024, 1000, 5), (256, 24, 3), (512, 10, 7), (8, 3, 2)])
def test_fc_fp32_logits_bit_exact(pkg, ctx, k, nout, m):
    rng = np.random.default_rng(k + nout)
    x = rng.integers(0, 256, (m, k), dtype=np.uint8)
    wk = rng.integers(-127, 128, (nout, k), dtype=np.int8)
    mult, bias, dm, db = _params(ctx, rng, nout, 1e-5, 1e-4)
    dx, dw_, dout = ctx.to_device(x), ctx.to_device(wk), ctx.alloc(m * nout * 4)
    ctx.pointwise(dout.ptr, dx.ptr, dw_.ptr, 1, 1, k, nout, _ext(pkg, m, dm.ptr, db.ptr, act=pkg.ACT_NONE, io=pkg.IO_OUT_F32))
    ctx.sync()
    got = dout.download((m, nout), np.float32)
    want = ref.pw(x, wk, mult, bias, out_f32=True)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_exact_gemm_with_asymmetric_filter(pkg, ctx):
    """mult = 1, bias = 0, fp32 out: the output IS the integer product; w[n][k] != w[k][n], so a row <-> column swap cannot pass."""
    m, k, nout = 77, 64, 96
    x = ((np.arange(m)[:, None] * 5 + np.arange(k)[None, :] * 11) % 256).astype(np.uint8)
    wk = (((np.arange(nout)[:, None] * 3 + np.arange(k)[None, :] * 7) % 255) - 127).astype(np.int8)
    one, zero = ctx.to_device(np.ones(nout, np.float32)), ctx.to_device(np.zeros(nout, np.float32))
    dx, dw_, dout = ctx.to_device(x), ctx.to_device(wk), ctx.alloc(m * nout * 4)
    ctx.pointwise(dout.ptr, dx.ptr, dw_.ptr, 1, m, k, nout, _ext(pkg, 1, one.ptr, zero.ptr, act=pkg.ACT_NONE, io=pkg.IO_OUT_F32))
    ctx.sync()
    got = dout.download((m, nout), np.float32)
    want = x.astype(np.int64) @ wk.astype(np.int64).T
    assert np.array_equal(got, want.astype(np.float32))


# ---- the pointwise launch plan (mbn_i8_pw_plan, host/mbn_envelope.c: what mbn_launch_i8_pointwise launches) decides each case's M, so the
# ---- cases below hold their intent on a device of any CU count

SENTINEL, GUARD = 0xA5, 4096


def _cus(ctx):
    n = C.c_int()
    assert ctx.lib.mbn_device_cus(ctx.h, C.byref(n)) == 0 and n.value > 0
    return n.value


def _plan_str(p, pkg):
    if p.form == pkg.I8_PW_PERSISTENT:
        return "persistent KS=%d G=%d pt=%d threads=%d ntiles=%d grid=%dx%d tiles/wg=%d..%d" % (
            p.ks, p.g, p.pt, p.threads, p.ntiles, p.gx, p.gy, p.ntiles // p.gx, -(-p.ntiles // p.gx))
    return "k-in-registers KS=%d G=%d nkb=%d pt=128 ntiles=%d cpg=%d ngroups=%d grid=%d" % (p.ks, p.g, p.nkb, p.ntiles, p.cpg, p.ngroups, p.gx)


def _run_pw_checked(pkg, ctx, x, wk, mult, bias, f32, off_in=0, off_w=0, off_out=0, off_par=0):
    """One mbn_pointwise call (operands at the given byte offsets inside their allocations) against int8_ref.pw in row blocks, bit for
    bit; the output is filled with a sentinel first and the bytes after it must keep it."""
    m, k = x.shape
    nout = wk.shape[0]
    es = 4 if f32 else 1
    out_bytes = m * nout * es
    dx, dw_, dout = ctx.alloc(x.nbytes + 16), ctx.alloc(wk.nbytes + 16), ctx.alloc(out_bytes + 16 + GUARD)
    dm, db = ctx.alloc(mult.nbytes + 16), ctx.alloc(bias.nbytes + 16)
    try:
        for d, off, a in ((dx, off_in, x), (dw_, off_w, wk), (dm, off_par, mult), (db, off_par, bias)):
            pkg._chk(ctx.lib.mbn_upload(ctx.h, d.ptr + off, a.ctypes.data, a.nbytes))
        pkg._chk(ctx.lib.mbn_memset(ctx.h, dout.ptr, SENTINEL, dout.nbytes))
        e = _ext(pkg, 1, dm.ptr + off_par, db.ptr + off_par, act=pkg.ACT_NONE if f32 else None, io=pkg.IO_OUT_F32 if f32 else 0)
        ctx.pointwise(dout.ptr + off_out, dx.ptr + off_in, dw_.ptr + off_w, 1, m, k, nout, e)
        ctx.sync()
        step = max(1, (64 << 20) // (nout * 8))
        got = np.empty((step, nout), np.float32 if f32 else np.uint8)
        mean = 0.0
        for i, want in ref.pw_blocks(x, wk, mult, bias, out_f32=f32, block=step):
            g = got[:len(want)]
            pkg._chk(ctx.lib.mbn_download(ctx.h, g.ctypes.data, dout.ptr + off_out + i * nout * es, g.nbytes))
            same = g.view(np.uint32) == want.view(np.uint32) if f32 else g == want
            assert same.all(), "rows %d..%d: %d elements differ, first at row %d" % (
                i, i + len(want) - 1, (~same).sum(), i + int(np.argmax(~same.all(axis=1))))
            mean += float(g.sum(dtype=np.float64))
        edge = np.empty(off_out + 0, np.uint8), np.empty(16 - off_out + GUARD, np.uint8)
        if off_out:
            pkg._chk(ctx.lib.mbn_download(ctx.h, edge[0].ctypes.data, dout.ptr, off_out))
        pkg._chk(ctx.lib.mbn_download(ctx.h, edge[1].ctypes.data, dout.ptr + off_out + out_bytes, len(edge[1])))
        assert np.all(edge[0] == SENTINEL) and np.all(edge[1] == SENTINEL), "stores outside the output"
        return mean / (m * nout)
    finally:
        for b in (dx, dw_, dout, dm, db):
            b.free()


def _pw_inputs(seed, m, k, nout, f32):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (m, k), dtype=np.uint8)
    wk = rng.integers(-127, 128, (nout, k), dtype=np.int8)
    mult = rng.uniform(1e-5, 1e-4, nout).astype(np.float32) if f32 else rng.uniform(0.2 / k, 0.9 / k, nout).astype(np.float32)
    bias = rng.uniform(-40, 60, nout).astype(np.float32)
    return x, wk, mult, bias


def _multipass_m(pkg, cus, k, nout, f32, threads=None):
    """The smallest ragged M (searched from the plan) at which some workgroups of the persistent form walk three tiles and some two, and the
    last tile is part-filled with a part-filled 32-pixel sub-tile."""
    def ok(m, ragged):
        p = pkg.i8_pw_plan(m, k, nout, cus, True, f32)
        good = p.form == pkg.I8_PW_PERSISTENT and p.ntiles > 2 * p.gx and (threads is None or p.threads == threads)
        return good and (not ragged or (p.ntiles % p.gx != 0 and m % p.pt % 32 != 0))
    lo, hi = 1, 64
    while not ok(hi, False):
        lo, hi = hi, hi * 2
        assert hi < 1 << 26, "no multi-pass M for %d -> %d" % (k, nout)
    while hi - lo > 1:                                # first M past two tiles per workgroup (the rule is monotone there)
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if ok(mid, False) else (mid, hi)
    m = hi
    while not ok(m, True):
        m += 1
        assert m < hi + 100000
    return m


def _assert_multipass(pkg, p, m):
    assert p.form == pkg.I8_PW_PERSISTENT
    assert p.ntiles > 2 * p.gx, "no workgroup walks three tiles"
    assert p.ntiles % p.gx != 0, "every workgroup walks the same number of tiles"
    assert m % p.pt != 0 and (m % p.pt) % 32 != 0, "the last tile is whole, or made of whole sub-tiles"


def _assert_distinct_tiles(x, pt):
    """No two tiles of the input are equal (their first rows already differ), so a tile read from the wrong buffer or pass cannot pass."""
    first = x[::pt]
    assert len(np.unique(first, axis=0)) == len(first)


# (K, N, fp32 output): every KS instantiation of i8_pw2_k on the fewest slots per column group (N = 1024; the FC's N = 1000, whose last chunk
# holds 8 channels, rows on the aligned float4 path), one N with N & 3 != 0 (scalar fp32 stores), and K = 24: 8-byte staging granules, a k step
# whose LDS bytes 24..31 are never written (they meet zeroed filter bytes)
_MULTIPASS = [(k, 1024, False) for k in (32, 64, 128, 256, 512, 1024)] + [(k, 1000, True) for k in (32, 64, 128, 256, 512, 1024)] + \
             [(1024, 1001, True), (24, 1024, False), (24, 1000, True)]


@pytest.mark.parametrize("k,nout,f32", _MULTIPASS)
def test_pointwise_persistent_two_and_three_tiles_per_workgroup(pkg, ctx, k, nout, f32):
    """i8_pw2_k past its first tile: the fetch(next) / put(cur ^ 1) / rotation half of the loop, a ragged last pass (some workgroups stop a
    tile earlier, so the run ends on either buffer) and a last tile with rows p >= m."""
    cus = _cus(ctx)
    m = _multipass_m(pkg, cus, k, nout, f32)
    p = pkg.i8_pw_plan(m, k, nout, cus, True, f32)
    _assert_multipass(pkg, p, m)
    assert p.ks == max(1, k // 32) and p.g == (16 if k % 16 == 0 else 8) and p.out_f32 == int(f32)
    print("pw %d -> %d %s m=%d: %s" % (k, nout, "f32" if f32 else "u8", m, _plan_str(p, pkg)))
    x, wk, mult, bias = _pw_inputs(k + nout, m, k, nout, f32)
    _assert_distinct_tiles(x, p.pt)
    mean = _run_pw_checked(pkg, ctx, x, wk, mult, bias, f32)
    assert f32 or 0 < mean < 255


@pytest.mark.parametrize("f32", [False, True])
def test_pointwise_persistent_three_subtile_groups_multipass(pkg, ctx, f32):
    """K = 256 -> N = 64 at large M: 384 threads, nrep = 3 (a wave's sub-tiles are sub0, sub0 + 96: one per 96-pixel tile), multi-pass."""
    cus = _cus(ctx)
    k, nout = 256, 64
    m = _multipass_m(pkg, cus, k, nout, f32, threads=384)
    p = pkg.i8_pw_plan(m, k, nout, cus, True, f32)
    _assert_multipass(pkg, p, m)
    assert (p.threads, p.cpw, p.rep, p.pt) == (384, 2, 3, 96)
    print("pw 256 -> 64 %s m=%d: %s" % ("f32" if f32 else "u8", m, _plan_str(p, pkg)))
    x, wk, mult, bias = _pw_inputs(384 + f32, m, k, nout, f32)
    _assert_distinct_tiles(x, p.pt)
    _run_pw_checked(pkg, ctx, x, wk, mult, bias, f32)


def test_pointwise_output_on_8_bytes_with_n_multiple_of_16(pkg, ctx):
    """Output at 8 mod 16 with N % 16 == 0 (inputs aligned): full16 is false, so whole chunks take the 4-byte store path."""
    m, k, nout = 301, 64, 48
    p = pkg.i8_pw_plan(m, k, nout, _cus(ctx), True, False)
    assert p.form == pkg.I8_PW_PERSISTENT and p.ntiles <= p.gx
    x, wk, mult, bias = _pw_inputs(48, m, k, nout, False)
    assert 0 < _run_pw_checked(pkg, ctx, x, wk, mult, bias, False, off_out=8) < 255


# (name, K, operand offset, N, M (None: from the plan), form expected: (KS, G, K blocks)). N = 72: three chunks, the last with 8 channels;
# M = 301: three 128-pixel tiles, the last ragged, and with so few tiles every chunk is a column group of its own (cpg = 1)
_KREG = [
    ("16x8", 256, 8, 72, 301, (16, 8, 1)),                      # K % 16 == 0 on 8-byte operands
    ("16x8_two_chunks_per_group", 256, 8, 72, None, (16, 8, 1)),   # enough tiles that a workgroup loops over two chunks (cpg = 2)
    ("32x8_one_block", 1024, 8, 72, 301, (32, 8, 1)),
    ("32x8_k520", 520, 0, 72, 301, (32, 8, 1)),                 # K % 16 == 8 above the persistent form's staging bound
    ("32x8_k1016", 1016, 0, 72, 301, (32, 8, 1)),
    ("32x16_two_blocks", 2048, 0, 72, 301, (32, 16, 2)),
    ("32x16_k1040", 1040, 0, 72, 301, (32, 16, 2)),             # a 16-byte second block
    ("32x8_k1032", 1032, 0, 72, 301, (32, 8, 2)),               # an 8-byte second block
    ("32x8_k1032_n70", 1032, 0, 70, 301, (32, 8, 2)),           # N & 3 != 0 (fp32 output only: scalar stores)
    ("16x16_cpw5", 256, 0, 136, None, (16, 16, 1)),             # aligned K <= 1024 that the persistent form gives up: 5 chunks per workgroup
    ("32x16_cpw5", 1024, 0, 136, 301, (32, 16, 1)),
]


@pytest.mark.parametrize("case,f32", [(c, f) for c in _KREG for f in (False, True) if f or c[3] % 8 == 0],
                         ids=lambda v: v[0] if isinstance(v, tuple) else ("f32" if v else "u8"))
def test_pointwise_k_in_registers_forms(pkg, ctx, case, f32):
    """Every reachable instantiation of i8_pw_k, uint8 and fp32 output, each asserted from the plan to be the one that runs."""
    name, k, off, nout, m, form = case
    cus = _cus(ctx)
    on16 = off % 16 == 0
    if m is None and name.startswith("16x16"):        # the first M the persistent form gives up, made ragged
        m = 1
        while pkg.i8_pw_plan(m, k, nout, cus, on16, f32).form != pkg.I8_PW_KREG:
            m += 128
            assert m < 1 << 22
        m += 45
    elif m is None:                                   # tiles > 2 CUs / 2: two column groups over three chunks
        m = 128 * (cus + 2) + 45
    p = pkg.i8_pw_plan(m, k, nout, cus, on16, f32)
    assert (p.form, p.ks, p.g, p.nkb) == (pkg.I8_PW_KREG,) + form, _plan_str(p, pkg)
    assert p.ngroups > 1 and m % 128 % 32 != 0 and nout % 32 != 0
    if "two_chunks" in name:
        assert p.cpg == 2 and p.ngroups == 2
    print("pw %s %s m=%d: %s" % (name, "f32" if f32 else "u8", m, _plan_str(p, pkg)))
    x, wk, mult, bias = _pw_inputs(k + nout + off, m, k, nout, f32)
    mean = _run_pw_checked(pkg, ctx, x, wk, mult, bias, f32, off_in=off, off_w=off)
    assert f32 or 0 < mean < 255


@pytest.mark.parametrize("shape", [(2, 7, 7, 1024), (3, 4, 4, 256), (1, 5, 3, 8), (4, 1, 1, 64)])
def test_pool_bit_exact(pkg, ctx, shape):
    n, h, w, c = shape
    x = np.random.default_rng(h * w + c).integers(0, 256, shape, dtype=np.uint8)
    dx, dout = ctx.to_device(x), ctx.alloc(n * c)
    ctx.pool(dout.ptr, dx.ptr, h, w, max(h, w), c, _ext(pkg, n, act=pkg.ACT_NONE))
    ctx.sync()
    assert np.array_equal(dout.download((n, c), np.uint8), ref.pool(x))


@pytest.mark.parametrize("u8in", [False, True])
def test_conv1_within_one_step(pkg, ctx, u8in):
    rng = np.random.default_rng(5 + u8in)
    n, res, c = 2, 64, 32
    raw = rng.integers(0, 256, (n, res, res, 3), dtype=np.uint8)
    img = raw.astype(np.float64) / 127.5 - 1.0
    wk = (rng.standard_normal((3, 3, 3, c)) * 0.4).astype(np.float32)
    mult = rng.uniform(20, 60, c).astype(np.float32)
    bias = rng.uniform(-30, 90, c).astype(np.float32)
    dm, db = ctx.to_device(mult), ctx.to_device(bias)
    dx = ctx.to_device(raw if u8in else img.astype(np.float32))
    dw_, dout = ctx.to_device(wk), ctx.alloc(n * (res // 2) ** 2 * c)
    e = _ext(pkg, n, dm.ptr, db.ptr, io=pkg.IO_IN_U8 if u8in else 0, cin=3)
    ctx.convolute(dout.ptr, dx.ptr, None, None, dw_.ptr, res, res, 3, 2, c, e)
    ctx.sync()
    got = dout.download((n, res // 2, res // 2, c), np.uint8).astype(np.int64)
    src = img if u8in else img.astype(np.float32).astype(np.float64)
    y = ref.conv1_y(src, wk, mult, bias)
    want = np.clip(np.rint(y), 0, 255).astype(np.int64)
    diff = got != want
    assert np.abs(got - want).max() <= 1
    yc = np.clip(y, 0, 255)
    assert np.all(np.abs(yc[diff] - (np.floor(yc[diff]) + 0.5)) < 2.0 ** -10), "mismatch away from a half-integer"
    assert diff.mean() < 1e-3 and 10 < got.mean() < 245


_CONV1_MAPS, _CONV1_PADS = ref.CONV1_MAPS, ref.CONV1_PADS


def _run_conv1(pkg, ctx, src, wk, mult, bias, stride, pads, u8in):
    n, h, w = src.shape[:3]
    c = wk.shape[-1]
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    nbytes = n * ho * wo * c
    dx, dw_, dm, db, dout = ctx.to_device(src), ctx.to_device(wk), ctx.to_device(mult), ctx.to_device(bias), ctx.alloc(nbytes + GUARD)
    try:
        pkg._chk(ctx.lib.mbn_memset(ctx.h, dout.ptr, SENTINEL, nbytes + GUARD))
        e = _ext(pkg, n, dm.ptr, db.ptr, io=pkg.IO_IN_U8 if u8in else 0, cin=3)
        if pads[0] is not None:
            e.pad_top, e.pad_left = pads
        ctx.convolute(dout.ptr, dx.ptr, None, None, dw_.ptr, h, w, 3, stride, c, e)
        ctx.sync()
        assert np.all(dout.download((nbytes + GUARD,), np.uint8)[nbytes:] == SENTINEL), "stores past the output"
        return dout.download((n, ho, wo, c), np.uint8)
    finally:
        for b in (dx, dw_, dm, db, dout):
            b.free()


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c", ref.CONV1_CHANNELS)
def test_conv1_bit_exact_on_grid_inputs(pkg, ctx, c, stride):
    """fp32-input conv1 bit for bit on inputs whose 27-term sum is exact in fp32 (int8_ref.conv1_exact_inputs): every NG (C = 8, 24: 1 with
    blockIdx.y up to 2; 16, 48: 2; 32: 4), both strides, three maps, SAME and explicit pads; each case reaches both clamps and the interior."""
    for h, w in _CONV1_MAPS:
        for pads in _CONV1_PADS:
            rng = np.random.default_rng(c * 100 + stride * 10 + h)
            img, wk, mult, bias = ref.conv1_exact_inputs(rng, 2, h, w, c)
            assert ref.conv1_grid_units(img, wk, stride, *pads) < 2 ** 24
            got = _run_conv1(pkg, ctx, img, wk, mult, bias, stride, pads, False)
            want = ref.conv1_exact(img, wk, mult, bias, stride, *pads)
            what = "conv1 C=%d s%d %dx%d pads %s" % (c, stride, h, w, pads)
            assert np.array_equal(got, want), "%s: %d of %d differ" % (what, (got != want).sum(), got.size)
            lo, hi = (got == 0).mean(), (got == 255).mean()
            assert lo > 0 and hi > 0 and lo + hi <= 0.5, "%s: shares at 0 / 255: %.3f / %.3f" % (what, lo, hi)


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c", ref.CONV1_CHANNELS)
def test_conv1_u8_input_within_one_step_every_form(pkg, ctx, c, stride):
    """Raw uint8 input (normalised in the kernel, so the sum is not exact) across the same channel counts, strides, maps and pads: within one
    step of the float64 value, different only at its half-integers."""
    for h, w in _CONV1_MAPS:
        for pads in _CONV1_PADS:
            rng = np.random.default_rng(c * 100 + stride * 10 + h + 1)
            raw = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
            wk = (rng.standard_normal((3, 3, 3, c)) * 0.4).astype(np.float32)
            mult = rng.uniform(20, 60, c).astype(np.float32)
            bias = rng.uniform(-30, 90, c).astype(np.float32)
            got = _run_conv1(pkg, ctx, raw, wk, mult, bias, stride, pads, True)
            y = ref.conv1_y(raw.astype(np.float64) / 127.5 - 1.0, wk, mult, bias, stride, *pads)
            if got.size >= 10000:
                ref.assert_conv1_one_step(got, y, "conv1 u8 C=%d s%d %dx%d pads %s" % (c, stride, h, w, pads))
            else:                                       # a 5 x 3 map: too few outputs for the mismatch share to mean anything
                d = got.astype(np.int64) != np.clip(np.rint(y), 0, 255)
                yc = np.clip(y, 0, 255)
                assert np.abs(got - np.clip(np.rint(y), 0, 255)).max() <= 1
                assert np.all(np.abs(yc[d] - (np.floor(yc[d]) + 0.5)) < 2.0 ** -10)
            assert 10 < got.mean() < 245


# ------------------------------------------------------------------------------------------------- depthwise: pads, map sizes, pointers

@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("pads", [(0, 1), (1, 0)])
def test_depthwise_explicit_pads_and_input_map(pkg, ctx, stride, pads):
    """Explicit pads with pad_top != pad_left, on an input map that is not rows * stride (one row and three columns more, one column less)."""
    c = 24
    for ho, wo, h, w in ((17, 13, 17 * stride + 1, 13 * stride + 3), (9, 13, 9 * stride, 13 * stride - 1)):
        rng = np.random.default_rng(ho + stride + pads[0])
        x = rng.integers(0, 256, (2, h, w, c), dtype=np.uint8)
        wk = rng.integers(-127, 128, (3, 3, c), dtype=np.int8)
        mult, bias, dm, db = _params(ctx, rng, c)
        dx, dw_, dout = ctx.to_device(x), ctx.to_device(wk), ctx.alloc(2 * ho * wo * c + GUARD)
        pkg._chk(ctx.lib.mbn_memset(ctx.h, dout.ptr, SENTINEL, dout.nbytes))
        e = _ext(pkg, 2, dm.ptr, db.ptr, in_rows=h, in_cols=w)
        e.pad_top, e.pad_left = pads
        ctx.depthwise(dout.ptr, dx.ptr, dw_.ptr, ho, wo, 3, stride, c, e)
        ctx.sync()
        want = ref.dw(x, wk, mult, bias, stride, pads[0], pads[1], ho, wo)
        assert np.array_equal(dout.download((2, ho, wo, c), np.uint8), want), (ho, wo, h, w)
        assert np.all(dout.download((dout.nbytes,), np.uint8)[want.size:] == SENTINEL)
        assert 0 < want.mean() < 255
        for b in (dx, dw_, dout, dm, db):
            b.free()


@pytest.mark.parametrize("stride", [1, 2])
def test_depthwise_interior_pointers(pkg, ctx, stride):
    """Input, filter and output 8 bytes into their allocations, mult / bias 4 bytes into theirs."""
    n, h, w, c = 2, 17, 13, 24
    ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
    rng = np.random.default_rng(170 + stride)
    x = rng.integers(0, 256, (n, h, w, c), dtype=np.uint8)
    wk = rng.integers(-127, 128, (3, 3, c), dtype=np.int8)
    mult = rng.uniform(2e-3, 8e-3, c).astype(np.float32)
    bias = rng.uniform(-40, 60, c).astype(np.float32)
    nbytes = n * ho * wo * c
    dx, dw_, dm, db, dout = ctx.alloc(x.nbytes + 16), ctx.alloc(wk.nbytes + 16), ctx.alloc(4 * c + 16), ctx.alloc(4 * c + 16), ctx.alloc(nbytes + 16 + GUARD)
    for d, off, a in ((dx, 8, x), (dw_, 8, wk), (dm, 4, mult), (db, 4, bias)):
        pkg._chk(ctx.lib.mbn_upload(ctx.h, d.ptr + off, a.ctypes.data, a.nbytes))
    pkg._chk(ctx.lib.mbn_memset(ctx.h, dout.ptr, SENTINEL, dout.nbytes))
    ctx.depthwise(dout.ptr + 8, dx.ptr + 8, dw_.ptr + 8, ho, wo, 3, stride, c, _ext(pkg, n, dm.ptr + 4, db.ptr + 4, in_rows=h, in_cols=w))
    ctx.sync()
    raw = dout.download((dout.nbytes,), np.uint8)
    assert np.array_equal(raw[8:8 + nbytes].reshape(n, ho, wo, c), ref.dw(x, wk, mult, bias, stride))
    assert np.all(raw[:8] == SENTINEL) and np.all(raw[8 + nbytes:] == SENTINEL)
    for b in (dx, dw_, dout, dm, db):
        b.free()


# ------------------------------------------------------------------------------------------------------------------- net runner

def _weights(pkg, tmp_path, alpha, res, classes, seed=7):
    path = str(tmp_path / ("w_%g_%d.h5" % (alpha, res)))
    pkg.synthetic_h5(path, alpha=alpha, classes=classes, seed=seed)
    hw = pkg.HostWeights(path, res=res)
    return hw


def _images(res, n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)


def _logits(ctx, net, d_in, batch, classes):
    d_out = ctx.alloc(batch * classes * 4)
    net.forward(d_in.ptr, d_out.ptr, batch)
    ctx.sync()
    out = d_out.download((batch, classes), np.float32)
    d_out.free()
    return out


@pytest.mark.parametrize("alpha,res,calibrate", [(1.0, 224, False), (0.5, 160, True), (0.25, 128, False), (0.25, 224, True)])
def test_net_every_layer_bit_exact(pkg, ctx, tmp_path, alpha, res, calibrate):
    classes, n = 40, 3
    hw = _weights(pkg, tmp_path, alpha, res, classes)
    plan = hw.plan
    net = pkg.Net(ctx, plan, hw.blob.copy(), 8)
    d_in = ctx.to_device(_images(res, n, 3))
    d_out = ctx.alloc(n * classes * 4)
    if calibrate:
        d_cal = ctx.to_device(_images(res, 8, 99))
        net.calibrate_i8(d_cal.ptr, 8)
        assert net.get_act_scales_i8()[0] != np.float32(6 / 255.0)
    net.set_dtype(pkg.DT_I8)
    net.keep_activations(True)
    net.forward(d_in.ptr, d_out.ptr, n)
    ctx.sync()
    got = d_out.download((n, classes), np.float32)
    scales = net.get_act_scales_i8()
    q = ref.quantize(plan, hw.blob, scales)
    p, _ = pkg.quantize_i8(plan, hw.blob, scales)
    prev = net.layer_output(1, n)
    assert prev.dtype == np.uint8 and 0 < prev.mean() < 255
    l0 = plan.layer[0]
    y = ref.conv1_y(_images(res, n, 3).astype(np.float64), hw.blob[l0.w_offset:l0.w_offset + l0.w_count].reshape(3, 3, 3, -1),
                    q[0]["mult"], q[0]["bias"], l0.stride, l0.pad_top, l0.pad_left)
    ref.assert_conv1_one_step(prev, y, "layer 1")
    for i in range(2, plan.n_layers + 1):
        l = plan.layer[i - 1]
        want = ref.layer_from_prev(l, q[i - 1], prev)
        dev = net.layer_output(i, n) if i < plan.n_layers else got     # the logits are the FC's output
        assert np.array_equal(dev.reshape(want.shape).view(np.uint8 if dev.dtype == np.uint8 else np.uint32),
                              want.view(np.uint8 if want.dtype == np.uint8 else np.uint32)), "layer %d" % i
        prev = dev if l.kind != ref.L_POOL else dev.reshape(n, 1, 1, l.out_ch)
    assert np.array_equal(got.view(np.uint32), np.asarray(prev).reshape(n, classes).view(np.uint32))
    assert np.isfinite(got).all() and got.std() > 0
    assert p.layer[1].in_scale == scales[0]
    d_out.free()
    net.destroy()
    hw.free()


@pytest.fixture(scope="module")
def net05(pkg, ctx, tmp_path_factory):
    hw = _weights(pkg, tmp_path_factory.mktemp("i8"), 0.5, 128, 24)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 16)
    net.set_dtype(pkg.DT_I8)
    imgs = _images(128, 16, 4)
    d_in = ctx.to_device(imgs)
    yield hw, net, imgs, d_in
    net.destroy()
    hw.free()


def test_launches_are_29_single_layers_and_that_is_what_runs(pkg, ctx, net05):
    hw, net, _, d_in = net05
    want = [(l, 1) for l in range(1, 30)]
    assert net.launches(16) == want and net.launches(1) == want
    net.set_fuse_blocks(0xFFFFFFFE)                 # the fused kinds have no I8 form, whatever the settings
    net.set_fuse_tail(True)
    net.set_fuse_stem(True)
    assert net.launches(2) == want and net.fused_layers() == 0
    d_out = ctx.alloc(16 * 24 * 4)
    ctx.profile_begin(64)
    try:
        net.forward(d_in.ptr, d_out.ptr, 2)
    finally:
        ran = ctx.profile_end(64)
    assert len(ran) == 29
    net.reset_fuse_blocks()
    net.set_fuse_tail(False)
    d_out.free()


def test_streams_graph_and_last_layer_are_bit_identical(pkg, ctx, net05):
    hw, net, _, d_in = net05
    ref_out = _logits(ctx, net, d_in, 16, 24)
    net.set_streams(2)
    assert np.array_equal(_logits(ctx, net, d_in, 16, 24), ref_out)
    net.set_streams(2, free_running=True)
    a = _logits(ctx, net, d_in, 16, 24)
    b = _logits(ctx, net, d_in, 16, 24)
    assert np.array_equal(a, ref_out) and np.array_equal(b, ref_out)
    net.set_streams(1)
    net.set_graph(True)
    for _ in range(2):                              # capture, then replay
        assert np.array_equal(_logits(ctx, net, d_in, 16, 24), ref_out)
    net.set_graph(False)
    net.keep_activations(True)
    _logits(ctx, net, d_in, 16, 24)
    kept = {i: net.layer_output(i, 16) for i in (5, 13, 27, 28)}
    net.keep_activations(False)
    plan = hw.plan
    for last in (5, 13, 27, 28):
        l = plan.layer[last - 1]
        d_out = ctx.alloc(16 * l.out_rows * l.out_cols * l.out_ch)
        net.forward(d_in.ptr, d_out.ptr, 16, last)
        ctx.sync()
        assert np.array_equal(d_out.download((16, l.out_rows, l.out_cols, l.out_ch), np.uint8), kept[last]), last
        d_out.free()
    d_out = ctx.alloc(16 * 24 * 4)
    ms = net.forward_timed(d_in.ptr, d_out.ptr, 16)
    ctx.sync()
    assert np.array_equal(d_out.download((16, 24), np.float32), ref_out)
    assert len(ms) == 29 and all(t > 0 for t in ms)
    d_out.free()


def test_u8_input_and_classify(pkg, ctx, net05):
    hw, net, _, _ = net05
    raw = np.random.default_rng(8).integers(0, 256, (6, 128, 128, 3), dtype=np.uint8)
    norm = (raw.astype(np.float32) * np.float32(1 / 127.5) - np.float32(1)).astype(np.float32)
    d_raw, d_norm = ctx.to_device(raw), ctx.to_device(norm)
    net.keep_activations(True)
    _logits(ctx, net, d_norm, 6, 24)
    l1_f32 = net.layer_output(1, 6).astype(np.int64)
    net.set_input_u8(True)
    logits_u8 = _logits(ctx, net, d_raw, 6, 24)
    l1_u8 = net.layer_output(1, 6).astype(np.int64)
    assert np.abs(l1_u8 - l1_f32).max() <= 1
    net.keep_activations(False)
    k = 5
    idx, prob = ctx.alloc(6 * k * 4), ctx.alloc(6 * k * 4)
    net.classify(d_raw.ptr, 6, k, idx.ptr, prob.ptr)
    ctx.sync()
    gi, gp = idx.download((6, k), np.int32), prob.download((6, k), np.float32)
    net.set_input_u8(False)
    z = logits_u8.astype(np.float64)
    sm = np.exp(z - z.max(axis=1, keepdims=True))
    sm /= sm.sum(axis=1, keepdims=True)
    assert np.array_equal(gi, np.argsort(-sm, axis=1, kind="stable")[:, :k])
    assert np.allclose(gp, np.take_along_axis(sm, gi.astype(np.int64), 1), rtol=1e-5, atol=1e-7)


def test_act_scale_setters_and_requantize(pkg, ctx, net05):
    hw, net, _, d_in = net05
    n = hw.plan.n_layers
    before = net.get_act_scales_i8()
    assert np.all(before == np.float32(6 / 255.0))
    base = _logits(ctx, net, d_in, 4, 24)
    s = before.copy()
    s[:27] = np.float32(3 / 255.0)
    net.set_act_scales_i8(s)                        # re-quantizes in I8 mode
    assert np.array_equal(net.get_act_scales_i8(), s)
    assert not np.array_equal(_logits(ctx, net, d_in, 4, 24), base)
    bad = s.copy()
    bad[3] = 0
    with pytest.raises(pkg.MbnError):
        net.set_act_scales_i8(bad)
    assert np.array_equal(net.get_act_scales_i8(), s)
    net.set_act_scales_i8(before)
    assert np.array_equal(_logits(ctx, net, d_in, 4, 24), base)
    assert ctx.lib.mbn_net_set_act_scales_i8(net.h, (C.c_float * n)(*before), n - 1) == pkg.EINVAL


def test_calibration_scales_from_fp32_maxima(pkg, ctx, tmp_path):
    """mbn_net_calibrate_i8 sets s_l = min(6, max_l) / 255 from the fp32 forward of the same images (6 / 255 where max_l = 0): compared
    layer by layer with the maxima of a kept fp32 forward. The 0.25x128 synthetic network has layers below 6 and layers at 6."""
    hw = _weights(pkg, tmp_path, 0.25, 128, 24)
    plan = hw.plan
    net = pkg.Net(ctx, plan, hw.blob.copy(), 8)
    d_in = ctx.to_device(_images(128, 8, 5))
    net.keep_activations(True)
    base = _logits(ctx, net, d_in, 8, 24)
    want = net.get_act_scales_i8().copy()
    for i in range(plan.n_layers):
        if plan.layer[i].kind in (ref.L_CONV, ref.L_DW, ref.L_PW):
            mx = np.float32(net.layer_output(i + 1, 8).max())
            want[i] = (min(mx, np.float32(6)) if mx > 0 else np.float32(6)) / np.float32(255)
    net.keep_activations(False)
    net.calibrate_i8(d_in.ptr, 8)
    got = net.get_act_scales_i8()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert (got[:27] < np.float32(6 / 255.0)).sum() >= 5 and (got[:27] == np.float32(6 / 255.0)).sum() >= 1
    # the dtype and the other settings are left as they were: still fp32 with kept activations, the same logits as before
    assert np.array_equal(_logits(ctx, net, d_in, 8, 24), base)
    net.keep_activations(True)
    assert np.array_equal(_logits(ctx, net, d_in, 8, 24), base) and net.layer_output(3, 8).dtype == np.float32
    net.destroy()
    hw.free()


def test_set_dtype_refused_leaves_the_net_as_it_was(pkg, ctx, tmp_path):
    """alpha 0.3: conv1 has 9 channels, outside the I8 kernels: set_dtype(I8) is refused and the net (and its Python mirror) stay fp32."""
    plan = pkg.plan_build(0.3, 64, 24)
    blob = (np.random.default_rng(3).standard_normal(plan.blob_floats) * 0.2).astype(np.float32)
    net = pkg.Net(ctx, plan, blob, 2)
    d_in = ctx.to_device(_images(64, 2, 6))
    base = _logits(ctx, net, d_in, 2, 24)
    with pytest.raises(pkg.MbnError) as ei:
        net.set_dtype(pkg.DT_I8)
    assert ei.value.code == pkg.EUNSUPPORTED
    assert getattr(net, "dtype", pkg.DT_F32) == pkg.DT_F32
    assert np.array_equal(_logits(ctx, net, d_in, 2, 24), base)
    net.keep_activations(True)
    _logits(ctx, net, d_in, 2, 24)
    assert net.layer_output(1, 2).dtype == np.float32
    net.destroy()


def test_c_abi_error_paths(pkg, ctx):
    lib, h = ctx.lib, ctx.h
    c, k = 16, 32
    x, w8, out = ctx.alloc(4 * 4 * c), ctx.alloc(9 * c), ctx.alloc(4 * 4 * c)
    m, b = ctx.to_device(np.ones(64, np.float32)), ctx.to_device(np.zeros(64, np.float32))
    ok = _ext(pkg, 1, m.ptr, b.ptr, in_rows=4, in_cols=4)
    assert lib.mbn_depthwise(h, out.ptr, x.ptr, w8.ptr, 4, 4, 3, 1, c, C.byref(ok)) == 0
    e = _ext(pkg, 1, m.ptr, b.ptr, in_rows=4, in_cols=4, layout=pkg.LAYOUT_NCHW_PLANAR)
    assert lib.mbn_depthwise(h, out.ptr, x.ptr, w8.ptr, 4, 4, 3, 1, c, C.byref(e)) == pkg.EUNSUPPORTED
    e = _ext(pkg, 1, None, b.ptr, in_rows=4, in_cols=4)                      # missing mult
    assert lib.mbn_depthwise(h, out.ptr, x.ptr, w8.ptr, 4, 4, 3, 1, c, C.byref(e)) == pkg.EINVAL
    e = _ext(pkg, 1, m.ptr, b.ptr, act=pkg.ACT_NONE, in_rows=4, in_cols=4)   # uint8 output with no clamp
    assert lib.mbn_depthwise(h, out.ptr, x.ptr, w8.ptr, 4, 4, 3, 1, c, C.byref(e)) == pkg.EINVAL
    e = _ext(pkg, 2, m.ptr, b.ptr, in_rows=4, in_cols=4)                      # undersized: two images in one-image buffers
    assert lib.mbn_depthwise(h, out.ptr, x.ptr, w8.ptr, 4, 4, 3, 1, c, C.byref(e)) == pkg.EINVAL
    assert lib.mbn_depthwise(h, out.ptr, x.ptr, w8.ptr, 4, 4, 3, 1, 12, C.byref(ok)) == pkg.EUNSUPPORTED   # channels % 8
    wp = ctx.alloc(k * c)
    e = _ext(pkg, 1, m.ptr, b.ptr)
    assert lib.mbn_pointwise(h, out.ptr, x.ptr, wp.ptr, 1, 16, c, k, C.byref(e)) == pkg.EINVAL                # output 16 x 32 > 256 bytes
    assert lib.mbn_pointwise(h, out.ptr, x.ptr, wp.ptr, 1, 8, c, k, C.byref(e)) == 0
    assert lib.mbn_pointwise(h, out.ptr, x.ptr, wp.ptr, 1, 1, 65544, 8, C.byref(e)) == pkg.EUNSUPPORTED      # K > 65536
    e = _ext(pkg, 1, m.ptr, None)                                             # missing bias
    assert lib.mbn_pointwise(h, out.ptr, x.ptr, wp.ptr, 1, 8, c, k, C.byref(e)) == pkg.EINVAL
    e = _ext(pkg, 1, m.ptr, b.ptr, act=pkg.ACT_NONE)                          # ACT_NONE only with fp32 output
    assert lib.mbn_pointwise(h, out.ptr, x.ptr, wp.ptr, 1, 8, c, k, C.byref(e)) == pkg.EINVAL
    e = _ext(pkg, 1, m.ptr, b.ptr, layout=pkg.LAYOUT_NCHW_PLANAR)
    assert lib.mbn_pointwise(h, out.ptr, x.ptr, wp.ptr, 1, 8, c, k, C.byref(e)) == pkg.EUNSUPPORTED
    for act in (pkg.ACT_RELU, pkg.ACT_RELU6):                                # fp32 logits take no activation
        e = _ext(pkg, 1, m.ptr, b.ptr, act=act, io=pkg.IO_OUT_F32)
        assert lib.mbn_pointwise(h, out.ptr, x.ptr, wp.ptr, 1, 1, c, k, C.byref(e)) == pkg.EINVAL
    e = _ext(pkg, 1, m.ptr, b.ptr, act=pkg.ACT_NONE, io=pkg.IO_OUT_F32)
    assert lib.mbn_pointwise(h, out.ptr, x.ptr, wp.ptr, 1, 1, c, k, C.byref(e)) == 0
    e = _ext(pkg, 1, None, None, cin=3)
    img, w1 = ctx.alloc(8 * 8 * 3 * 4), ctx.alloc(27 * c * 4)
    assert lib.mbn_convolute(h, out.ptr, img.ptr, None, None, w1.ptr, 8, 8, 3, 2, c, C.byref(e)) == pkg.EINVAL   # conv1 needs mult / bias
    e = _ext(pkg, 1, m.ptr, b.ptr, cin=3)
    assert lib.mbn_convolute(h, out.ptr, img.ptr, None, None, w1.ptr, 8, 8, 3, 2, c, C.byref(e)) == 0
    assert lib.mbn_convolute(h, out.ptr, img.ptr, None, None, w1.ptr, 16, 16, 3, 2, c, C.byref(e)) == pkg.EINVAL   # image too small
    e = _ext(pkg, 1, act=pkg.ACT_NONE)
    assert lib.mbn_pool(h, out.ptr, x.ptr, 4, 4, 4, c, C.byref(e)) == 0
    e = _ext(pkg, 1, act=pkg.ACT_NONE, layout=pkg.LAYOUT_NCHW_PLANAR)
    assert lib.mbn_pool(h, out.ptr, x.ptr, 4, 4, 4, c, C.byref(e)) == pkg.EUNSUPPORTED
    ctx.sync()
    for buf in (x, w8, out, m, b, wp, img, w1):
        buf.free()


def test_accuracy_against_fp32_oracle(pkg, ctx, orc, tmp_path):
    """1.0x224, synthetic weights: calibrated on 32 images, evaluated on 64 others against the fp32 oracle. Measured on an MI355X,
    default and calibrated alike: top-1 agreement 64 / 64, mean logit cosine 0.99980, max |dlogit| 0.075 (max |logit| 3.4). The two
    agree because every ReLU6 layer of this synthetic network reaches 6 on the calibration images, so calibration chooses 6 / 255 — the
    default — everywhere. The bounds below sit under the measured values with margin."""
    classes = 1000
    hw = _weights(pkg, tmp_path, 1.0, 224, classes, seed=2024)
    ev = _images(224, 64, 1234)
    cal = _images(224, 32, 4321)
    want, _ = orc.net_forward(orc.plan_build(1.0, 224, classes), hw.blob, ev, threads=orc.num_threads())
    want = np.asarray(want).reshape(64, classes).astype(np.float64)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 64)
    d_ev, d_cal = ctx.to_device(ev), ctx.to_device(cal)
    net.set_dtype(pkg.DT_I8)
    stats = {}
    for name in ("default", "calibrated"):
        if name == "calibrated":
            net.calibrate_i8(d_cal.ptr, 32)
        got = _logits(ctx, net, d_ev, 64, classes).astype(np.float64)
        top1 = float((got.argmax(1) == want.argmax(1)).mean())
        cos = float(np.mean((got * want).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(want, axis=1))))
        stats[name] = (top1, cos, float(np.abs(got - want).max()), float(np.abs(want).max()))
    print("int8 vs fp32 oracle (top-1 agreement, mean logit cosine, max |dlogit|, max |logit|):", stats)
    for name in stats:
        top1, cos, dmax, lmax = stats[name]
        assert top1 >= 0.9 and cos > 0.999 and dmax < 0.3, (name, stats[name])
    assert stats["calibrated"][1] >= stats["default"][1] - 1e-4       # calibration does no worse than the defaults
    assert np.all(net.get_act_scales_i8()[:27] <= np.float32(6 / 255.0))
    net.destroy()
    hw.free()
