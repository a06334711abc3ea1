"""Every buffer-descriptor kernel on both sides of its 32-bit offset limits.

The fast kernels address memory through buffer descriptors: a 32-bit num_records, 32-bit byte offsets, and a fixed "invalid" offset
that the range check drops past the end of a tensor. Each is safe only below a size limit, which its dispatch guard encodes; above it
the dispatch takes another form (or answers MBN_EUNSUPPORTED). Every row below has a case just inside and one just outside the limit.
A new descriptor-based kernel adds its row here.

| limit                                            | guard (file:line)                                  | below (case)                      | above (case)                                    |
|--------------------------------------------------|----------------------------------------------------|-----------------------------------|-------------------------------------------------|
| dwpw3 output + 32 px <= 2 GiB (ragged pairs      | mbn_f32_dwpw3.hip:517 (mbn_f32_dwpw3_eligible)     | 719 x 54^2, 128->256 (dwpw3_f32)  | 721 x 54^2, 128->256; 343 x 54^2, 128->1024     |
|   store at PO_INVALID = 0x80000000)              |                                                    |                                   |   (round-1 dwpw_f32)                            |
| input <= 0x70000000 (fp32 dwpw2 fast_off)        | host/mbn_envelope.c:35 (mbn_block_fast_offsets)    | 629 x 108^2 x 64, s2              | 630 x 108^2 x 64, s2 (general offsets)          |
| input <= 0x70000000 (bf16 dwpw2 fast_off)        | host/mbn_envelope.c:35 (mbn_block_fast_offsets)    | 1258 x 108^2 x 64, s2             | 1259 (general offsets)                          |
| input <= 0x70000000 (dwpw3 input)                | host/mbn_envelope.c:35, via mbn_f32_dwpw3.hip:513  | 1258 x 54^2, 128->128 (dwpw3)     | 1259: 128->128 (dwpw2), 128->256 (dwpw_f32)     |
| input < 0xF0000000 (fused block envelope)        | host/mbn_envelope.c:19 (mbn_block_envelope)        | 1348 x 108^2 x 64, s2             | 1349: MBN_EUNSUPPORTED; net batch 1399 unfused  |
| (output + 256 rows) < 4 GiB (fused envelope)     | host/mbn_envelope.c:22 (mbn_block_envelope)        | 359 x 54^2, 128->1024             | 360: MBN_EUNSUPPORTED                           |
| output < 4 GiB (pw_gemm fast_epi)                | mbn_f32_pw.hip:597                                 | m = 2^24 - 37, 32->64             | m = 2^24 + 37 (general epilogue)                |
| input, filter < 4 GiB (pw_gemm loop2)            | mbn_f32_pw.hip:593-594                             | m = 2^21 - 37, 512->64            | m = 2^21 + 37 (plain k-loop)                    |
| (m + 64) K 4, (m + 64) N 4 < 4 GiB (pw3)         | mbn_f32_pw3.hip:257                                | m = 2^22 - 101, 256->256 (pw3)    | m = 2^22 - 59 (pw_gemm)                         |
| m K 2 < 0xF0000000 (bf16 streaming pointwise)    | mbn_bf16_pw_stream.hip:421                         | K 128 -> 128, K 256 -> 128        | ~75 rows more (pw_gemm<bf16>)                   |
| (m + 256) N 2 < 4 GiB (bf16 streaming pointwise) | mbn_bf16_pw_stream.hip:421                         | K 64 -> 128, K 256 -> 512         | ~75 rows more (pw_gemm<bf16>)                   |
| one image < 2e9 B (dw3x3_lds)                    | mbn_f32_dw.hip:852                                 | 1 x 3952^2 x 32 (dw3x3_lds)       | 1 x 3954^2 x 32 (column march)                  |
| stride-2 input >= 512 MiB, >= 40 rows (2 rows    | mbn_f32_dw.hip:833                                 | 167 x 112^2 x 64                  | 168 x 112^2 x 64                                |
|   per segment)                                   |                                                    |                                   |                                                 |
| none (64-bit pointers): depthwise > 4 GiB        | mbn_f32_dw.hip (fp32, bf16x8)                      | the P-image twins                 | fp32 / bf16 at stride 1 and 2, 4.3 GB           |
| none (64-bit pointers): int8 pointwise > 4 GiB   | mbn_i8.hip (i8_pw2_k: input; uint8 and fp32 output)| the P-row twins (int8_ref.pw)     | K 1024 -> 8, K 8 -> 1024, K 8 -> 1000 fp32      |
| none (64-bit pointers): int8 depthwise > 4 GiB   | mbn_i8.hip (i8_dw_k<1>, <2>)                       | the P-image twins (int8_ref.dw)   | 5351 x 112^2 x 64 at stride 1 and 2, 4.3 GB     |
| input < 4 GiB (bf16 resident tail)               | host/mbn_envelope.c:59 (mbn_tail_envelope)         | 83 885 x 10^2 x 256               | 83 887: MBN_EUNSUPPORTED                        |
| stem / conv1 (64-bit pointers)                   | mbn_f32_stem.hip                                   | forward(7)                        | net batch 1399 (fp32 fused and unfused stem),   |
|                                                  |                                                    |                                   |   bf16 batch 2700                               |

Method (a multi-GB output is checked whole without a multi-GB CPU reference):
- periodic input: image (or row) i of the big tensor is base[i % P], P = 7. An odd period cannot line up with a power-of-two offset error,
  so a store misplaced by 2^31 bytes, or wrapped modulo 2^32, lands on data whose expected value is different;
- the small twin: the same entry point on the P base items alone, far below every limit, checked against the oracle;
- the big call against the twin bit for bit, every element, read back in chunks through interior device pointers. A row's arithmetic does
  not depend on the batch or on which shipped form ran (test_parity_gpu.py asserts it for each pair of forms). Twins of pointwise calls
  keep out of the split-K regime (pw_splitk = 1);
- guards: the output is filled with 0xFF first (an unwritten element stays a NaN pattern and fails the comparison) and 64 KiB past it must
  stay untouched.
Host transfers go in chunks of at most 256 MiB; device buffers are freed in `finally`.
"""
import numpy as np
import pytest

import int8_ref
from test_parity_gpu import TOL_BF16, TOL_DW, TOL_PW, assert_close, _make_net

pytestmark = pytest.mark.gpu

P = 7                   # period of the big inputs (odd prime)
CHUNK = 256 << 20       # host <-> device transfer size
GUARD = 64 << 10        # bytes past every output that must stay 0xFF
OOB = 0xF0000000
GIB4 = 1 << 32


def _chk(pkg, ctx, rc, what=""):
    assert rc == 0, "%s: mbn error %d %s" % (what, rc, ctx.last_error())


class _Bufs:
    """Device buffers of one test, freed together."""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def alloc(self, nbytes):
        b = self.ctx.alloc(nbytes)
        self.bufs.append(b)
        return b

    def dev(self, arr):
        return self.alloc(np.ascontiguousarray(arr).nbytes).upload(arr)

    def free(self):
        for b in self.bufs:
            b.free()
        self.ctx._bufs = [b for b in self.ctx._bufs if b.ptr]
        self.bufs = []


def _upload_periodic(ctx, ptr, base, count):
    """Device items [0, count) at ptr := base[i % P] (base: [P][...]), in whole periods of at most CHUNK bytes."""
    base = np.ascontiguousarray(base)
    item = base[0].nbytes
    reps = max(1, CHUNK // (item * len(base)))
    blk = np.ascontiguousarray(np.concatenate([base] * reps))
    per = len(blk)
    for i0 in range(0, count, per):
        k = min(per, count - i0)
        assert ctx.lib.mbn_upload(ctx.h, ptr + i0 * item, blk.ctypes.data, k * item) == 0


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _check_items(ctx, ptr, count, table, index, what):
    """Device items [0, count) at ptr equal table[index(i)] bit for bit (table: [T][...]; index maps an int64 array of item numbers to
    table rows). Read back in chunks of at most CHUNK bytes through interior pointers."""
    tb = _bits(table).reshape(len(table), -1)
    item = tb[0].nbytes
    per = max(1, CHUNK // item)
    per -= per % P if per > P else 0
    buf = np.empty((per, tb.shape[1]), tb.dtype)
    for i0 in range(0, count, per):
        k = min(per, count - i0)
        assert ctx.lib.mbn_download(ctx.h, buf.ctypes.data, ptr + i0 * item, k * item) == 0
        want = tb[index(np.arange(i0, i0 + k, dtype=np.int64))]
        bad = np.nonzero((buf[:k] != want).any(axis=1))[0]
        if len(bad):
            unwritten = int((buf[:k][bad] == (0xFFFF if tb.dtype == np.uint16 else 0xFFFFFFFF)).all(axis=1).sum())
            j = int(bad[0])
            byte = (i0 + j) * item
            raise AssertionError("%s: %d of items %d..%d differ (%d never written), first at item %d (byte offset %d = 0x%x)"
                                 % (what, len(bad), i0, i0 + k - 1, unwritten, i0 + j, byte, byte))


def _check_periodic(ctx, ptr, count, twin, what):
    _check_items(ctx, ptr, count, twin, lambda i: i % len(twin), what)


def _fill(ctx, buf, nbytes):
    assert ctx.lib.mbn_memset(ctx.h, buf.ptr, 0xFF, nbytes) == 0


def _check_guard(ctx, buf, nbytes, what):
    tail = np.empty(GUARD, np.uint8)
    assert ctx.lib.mbn_download(ctx.h, tail.ctypes.data, buf.ptr + nbytes, GUARD) == 0
    assert np.all(tail == 0xFF), "%s: stores past the end of the output (first at byte +%d)" % (what, int(np.argmax(tail != 0xFF)))


def _params_dwpw(rng, cin, cout):
    wd = rng.normal(0, 0.5, (3, 3, cin)).astype(np.float32)
    wp = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    s2, s3 = rng.uniform(0.5, 1.5, cin).astype(np.float32), rng.uniform(0.5, 1.5, cout).astype(np.float32)
    b2, b3 = rng.normal(0, 0.1, cin).astype(np.float32), rng.normal(0, 0.1, cout).astype(np.float32)
    return wd, s2, b2, wp, s3, b3


# =========================================================================== fused depthwise -> pointwise blocks

def _dwpw_geometry(h, stride):
    oh = (h + stride - 1) // stride
    pad = max((oh - 1) * stride + 3 - h, 0) // 2                       # TF-SAME: 1 for stride 1, 0 for stride 2 (even h)
    return oh, pad


def _run_dwpw_big(pkg, orc, ctx, n, h, cin, cout, stride, bf16=False):
    """mbn_dwpw_fused(_bf16) on n images with image i = base[i % P]: the P-image twin against the oracle, every output image against the twin
    bit for bit, nothing unwritten, nothing stored past the output."""
    oh, pad = _dwpw_geometry(h, stride)
    m = n * oh * oh
    assert m % 32 != 0, "not a ragged case"
    es = 2 if bf16 else 4
    rng = np.random.default_rng(n + h + cin + cout)
    if bf16:
        x = orc.bf16_round(rng.uniform(0, 4, (P, h, h, cin)).astype(np.float32))
        wd, s2, b2, wp, s3, b3 = _params_dwpw(rng, cin, cout)
        wp = orc.bf16_round(wp)
    else:
        x = rng.uniform(-1, 1, (P, h, h, cin)).astype(np.float32)
        wd, s2, b2, wp, s3, b3 = _params_dwpw(rng, cin, cout)
    fn = ctx.lib.mbn_dwpw_fused_bf16 if bf16 else ctx.lib.mbn_dwpw_fused
    host = (lambda a: pkg.f32_to_bf16_bits(a)) if bf16 else (lambda a: a)
    bufs = _Bufs(ctx)
    try:
        d_wd, d_s2, d_b2, d_s3, d_b3 = (bufs.dev(a) for a in (wd, s2, b2, s3, b3))
        d_wp = bufs.dev(host(wp))
        call = lambda out, inp, nb: fn(ctx.h, out, inp, d_wd.ptr, d_s2.ptr, d_b2.ptr, d_wp.ptr, d_s3.ptr, d_b3.ptr,
                                       nb, h, h, oh, oh, cin, cout, stride, pad, pad, None)
        # the twin: P images alone
        d_tx, d_to = bufs.dev(host(x)), bufs.alloc(P * oh * oh * cout * es)
        _chk(pkg, ctx, call(d_to.ptr, d_tx.ptr, P), "twin")
        ctx.sync()
        twin = d_to.download((P, oh, oh, cout), np.uint16 if bf16 else np.float32)
        mid = orc.f32_depthwise(x, wd, s2, b2, stride, 2, pad_top=pad, pad_left=pad)
        if bf16:
            mid = orc.bf16_round(mid)
        want = orc.f32_pointwise(mid.reshape(-1, cin), wp, s3, b3, 2).reshape(P, oh, oh, cout)
        got = pkg.bf16_bits_to_f32(twin) if bf16 else twin
        assert_close(got, orc.bf16_round(want) if bf16 else want, TOL_BF16 if bf16 else TOL_PW, "dwpw twin %s" % ((h, cin, cout, stride),))
        # the big call
        out_bytes = m * cout * es
        d_x, d_o = bufs.alloc(n * h * h * cin * es), bufs.alloc(out_bytes + GUARD)
        _upload_periodic(ctx, d_x.ptr, host(x), n)
        _fill(ctx, d_o, out_bytes + GUARD)
        _chk(pkg, ctx, call(d_o.ptr, d_x.ptr, n), "big")
        ctx.sync()
        what = "%s dwpw n=%d %dx%d %d->%d s%d" % ("bf16" if bf16 else "fp32", n, h, h, cin, cout, stride)
        _check_guard(ctx, d_o, out_bytes, what)
        _check_periodic(ctx, d_o.ptr, n, twin, what)
    finally:
        bufs.free()


DWPW_F32_CASES = [  # (name, batch, in side, Cin, Cout, stride): input / output bytes in the comment
    ("dwpw3_below_2g", 719, 54, 128, 256, 1),        # out 2 146 922 496: dwpw3_f32
    ("dwpw3_above_2g", 721, 54, 128, 256, 1),        # out 2 152 894 464 (> 2^31): the ragged pair's PO_INVALID store hit pixel 2 097 152
    ("dwpw3_above_2g_c1024", 343, 54, 128, 1024, 1), # out 4 096 770 048: PO_INVALID store hit pixel 524 288
    ("fast_off_below", 629, 108, 64, 128, 2),        # in 1 878 183 936 <= 0x70000000: dwpw2_f32 FO
    ("fast_off_above", 630, 108, 64, 128, 2),        # in 1 881 169 920: dwpw2_f32 general offsets
    ("dwpw3_in_below", 1258, 54, 128, 128, 1),       # in 1 878 183 936: dwpw3_f32
    ("dwpw3_in_above", 1259, 54, 128, 128, 1),       # in 1 879 676 928: dwpw2_f32 general offsets
    ("dwpw3_in_above_c256", 1259, 54, 128, 256, 1),  # out 3 759 353 856: round-1 dwpw_f32 (256-column tiles)
    ("envelope_in_below", 1348, 108, 64, 128, 2),    # in 4 025 106 432 < 0xF0000000: dwpw2_f32 general offsets
    ("envelope_out_below", 359, 54, 128, 1024, 1),   # (m + 256) * 4096 = 4 288 921 600 < 2^32
]


@pytest.mark.parametrize("case", DWPW_F32_CASES, ids=lambda c: c[0])
def test_f32_dwpw_fused_large(pkg, orc, ctx, case):
    _, n, h, cin, cout, stride = case
    _run_dwpw_big(pkg, orc, ctx, n, h, cin, cout, stride)


@pytest.mark.parametrize("n", [1258, 1259], ids=["fast_off_below", "fast_off_above"])
def test_bf16_dwpw_fused_large(pkg, orc, ctx, n):
    """bf16 dwpw2 on both sides of its fast_off limit (input 1 878 183 936 / 1 879 676 928 bytes against 0x70000000)."""
    _run_dwpw_big(pkg, orc, ctx, n, 108, 64, 128, 2, bf16=True)


@pytest.mark.parametrize("case", [(1349, 108, 64, 128, 2), (360, 54, 128, 1024, 1)], ids=["input_0xF0000000", "output_plus_256_rows_4g"])
def test_f32_dwpw_fused_envelope_above_is_unsupported(pkg, ctx, case):
    """Just above the fused block's input limit (4 029 078 400 bytes >= 0xF0000000) and its output + 256-row limit ((m + 256) * 4096 =
    4 300 800 000 >= 2^32) mbn_dwpw_fused answers MBN_EUNSUPPORTED and launches nothing (the buffer it was handed stays as it was); so does the
    bf16 form at twice the batch."""
    n, h, cin, cout, stride = case
    oh, pad = _dwpw_geometry(h, stride)
    bufs = _Bufs(ctx)
    try:
        d = bufs.alloc(1 << 20)
        _fill(ctx, d, 1 << 20)
        ctx.sync()
        for fn, nb in ((ctx.lib.mbn_dwpw_fused, n), (ctx.lib.mbn_dwpw_fused_bf16, 2 * n)):
            rc = fn(ctx.h, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, d.ptr, nb, h, h, oh, oh, cin, cout, stride, pad, pad, None)
            assert rc == pkg.EUNSUPPORTED, rc
        ctx.sync()
        assert np.all(d.download((1 << 20,), np.uint8) == 0xFF), "a refused call wrote"
    finally:
        bufs.free()


# =========================================================================== pointwise

def _run_pw_big(pkg, orc, ctx, m, cin, cout, bf16=False, twin_keys=()):
    """mbn_pointwise on m rows with row i = base[i % P]: the P-row twin (pw_splitk = 1 and twin_keys set) against the oracle, every output row
    against it bit for bit, nothing unwritten, nothing stored past the output."""
    assert m % 32 != 0 and m % P != 0
    es = 2 if bf16 else 4
    rng = np.random.default_rng(m + cin + cout)
    x = rng.uniform(-1, 1, (P, cin)).astype(np.float32)
    f = rng.normal(0, (2.0 / cin) ** 0.5, (cout, cin)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    sh = rng.normal(0, 0.1, cout).astype(np.float32)
    if bf16:
        x, f = orc.bf16_round(x), orc.bf16_round(f)
    host = (lambda a: pkg.f32_to_bf16_bits(a)) if bf16 else (lambda a: a)
    dt = pkg.DT_BF16 if bf16 else pkg.DT_F32
    bufs = _Bufs(ctx)
    try:
        d_f, d_sc, d_sh = bufs.dev(host(f)), bufs.dev(sc), bufs.dev(sh)
        ext = pkg.make_ext(batch=1, dtype=dt, act=2, scale=d_sc.ptr, shift=d_sh.ptr)
        d_tx, d_to = bufs.dev(host(x)), bufs.alloc(P * cout * es)
        try:
            assert ctx.lib.mbn_tune_set(b"pw_splitk", 1) == 0
            for k, v in twin_keys:
                assert ctx.lib.mbn_tune_set(k, v) == 0
            ctx.pointwise(d_to.ptr, d_tx.ptr, d_f.ptr, P, 1, cin, cout, ext)
            ctx.sync()
        finally:
            ctx.lib.mbn_tune_set(b"pw_splitk", 0)
            for k, _ in twin_keys:
                ctx.lib.mbn_tune_set(k, 0)
        twin = d_to.download((P, cout), np.uint16 if bf16 else np.float32)
        want = orc.f32_pointwise(x, f, sc, sh, 2)
        if bf16:
            assert_close(pkg.bf16_bits_to_f32(twin), orc.bf16_round(want), TOL_BF16, "bf16 pw twin")
        else:
            assert_close(twin, want, TOL_PW, "pw twin")
        out_bytes = m * cout * es
        d_x, d_o = bufs.alloc(m * cin * es), bufs.alloc(out_bytes + GUARD)
        _upload_periodic(ctx, d_x.ptr, host(x), m)
        _fill(ctx, d_o, out_bytes + GUARD)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
        ctx.sync()
        what = "%s pw m=%d %d->%d" % ("bf16" if bf16 else "fp32", m, cin, cout)
        _check_guard(ctx, d_o, out_bytes, what)
        _check_periodic(ctx, d_o.ptr, m, twin, what)
    finally:
        bufs.free()


PW_F32_CASES = [  # (name, m, K, N)
    ("fast_epi_below", (1 << 24) - 37, 32, 64),      # output 4 294 957 824 < 2^32
    ("fast_epi_above", (1 << 24) + 37, 32, 64),      # output 4 294 976 768: general epilogue
    ("loop2_below", (1 << 21) - 37, 512, 64),        # input 4 294 891 520 < 2^32: two-step k-loop
    ("loop2_above", (1 << 21) + 37, 512, 64),        # input 4 295 043 072: plain k-loop
    ("pw3_below", 4194240 - 37, 256, 256),           # (m + 64) * 1024 = 4 294 929 408 < 2^32: pw3
    ("pw3_above", 4194240 + 5, 256, 256),            # (m + 64) * 1024 = 4 294 972 416: pw_gemm
]


@pytest.mark.parametrize("case", PW_F32_CASES, ids=lambda c: c[0])
def test_f32_pointwise_large(pkg, orc, ctx, case):
    _, m, cin, cout = case
    _run_pw_big(pkg, orc, ctx, m, cin, cout)


PW_BF16_CASES = [  # (name, m, K, N): the streaming kernel's K <= 128 (32x32x16) and K >= 256 (16x16x32) branches, mbn_f32_pw.hip:651-658
    ("k128_in_below", 15728640 - 37, 128, 128),      # m K 2 = 4 026 522 368 < 0xF0000000
    ("k128_in_above", 15728640 + 37, 128, 128),      # 4 026 541 312: pw_gemm<bf16>
    ("k64_out_below", 16776960 - 37, 64, 128),       # (m + 256) N 2 = 4 294 957 824 < 2^32
    ("k64_out_above", 16776960 + 37, 64, 128),       # 4 294 976 768: pw_gemm<bf16>
    ("k256_in_below", 7864320 - 39, 256, 128),       # m K 2 = 4 026 511 872
    ("k256_in_above", 7864320 + 37, 256, 128),       # 4 026 550 784: pw_gemm<bf16>
    ("k256_out_below", 4194048 - 37, 256, 512),      # (m + 256) N 2 = 4 294 929 408
    ("k256_out_above", 4194048 + 39, 256, 512),      # 4 295 007 232: pw_gemm<bf16>
]


@pytest.mark.parametrize("case", PW_BF16_CASES, ids=lambda c: c[0])
def test_bf16_pointwise_large(pkg, orc, ctx, case):
    """bf16 pointwise on both sides of the streaming kernel's limits. Above them the call runs on pw_gemm<bf16>, against a twin on the streaming
    kernel (K >= 256: its 16x16x32 form)."""
    _, m, cin, cout = case
    _run_pw_big(pkg, orc, ctx, m, cin, cout, bf16=True)


# =========================================================================== depthwise

def _run_dw_big(pkg, orc, ctx, n, h, ch, stride, bf16=False):
    """mbn_depthwise on n images with image i = base[i % P] against the P-image twin (itself against the oracle), bit for bit."""
    oh = (h + stride - 1) // stride
    es = 2 if bf16 else 4
    rng = np.random.default_rng(n + h + ch + stride)
    x = rng.uniform(-1, 1, (P, h, h, ch)).astype(np.float32)
    if bf16:
        x = orc.bf16_round(x)
    f = rng.normal(0, 0.5, (3, 3, ch)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, ch).astype(np.float32), rng.normal(0, 0.1, ch).astype(np.float32)
    host = (lambda a: pkg.f32_to_bf16_bits(a)) if bf16 else (lambda a: a)
    dt = pkg.DT_BF16 if bf16 else pkg.DT_F32
    bufs = _Bufs(ctx)
    try:
        d_f, d_sc, d_sh = bufs.dev(f), bufs.dev(sc), bufs.dev(sh)
        ext = lambda nb: pkg.make_ext(batch=nb, dtype=dt, act=2, in_rows=h, in_cols=h, scale=d_sc.ptr, shift=d_sh.ptr)
        d_tx, d_to = bufs.dev(host(x)), bufs.alloc(P * oh * oh * ch * es)
        ctx.depthwise(d_to.ptr, d_tx.ptr, d_f.ptr, oh, oh, 3, stride, ch, ext(P))
        ctx.sync()
        twin = d_to.download((P, oh, oh, ch), np.uint16 if bf16 else np.float32)
        want = orc.f32_depthwise(x, f, sc, sh, stride, 2)
        if bf16:
            assert_close(pkg.bf16_bits_to_f32(twin), orc.bf16_round(want), TOL_BF16, "bf16 dw twin")
        else:
            assert_close(twin, want, TOL_DW, "dw twin")
        out_bytes = n * oh * oh * ch * es
        d_x, d_o = bufs.alloc(n * h * h * ch * es), bufs.alloc(out_bytes + GUARD)
        _upload_periodic(ctx, d_x.ptr, host(x), n)
        _fill(ctx, d_o, out_bytes + GUARD)
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, oh, oh, 3, stride, ch, ext(n))
        ctx.sync()
        what = "%s dw n=%d %dx%dx%d s%d" % ("bf16" if bf16 else "fp32", n, h, h, ch, stride)
        _check_guard(ctx, d_o, out_bytes, what)
        _check_periodic(ctx, d_o.ptr, n, twin, what)
    finally:
        bufs.free()


DW_CASES = [  # (name, batch, side, channels, stride, bf16)
    ("f32_s1_over_4g", 2693, 56, 128, 1, False),     # 4 323 966 976 bytes in and out: dw3x3_lds
    ("f32_s2_over_4g", 1343, 112, 64, 2, False),     # in 4 312 727 552: column march, two output rows per segment
    ("f32_s2_nseg_below", 167, 112, 64, 2, False),   # in 536 281 088 < 512 MiB: one segment per column
    ("f32_s2_nseg_above", 168, 112, 64, 2, False),   # in 539 492 352: two output rows per segment
    ("bf16_s1_over_4g", 5386, 56, 128, 1, True),     # 4 323 966 976 bytes in and out: dw3x3_nhwc_bf16x8
    ("bf16_s2_over_4g", 2686, 112, 64, 2, True),     # in 4 312 727 552
]


@pytest.mark.parametrize("case", DW_CASES, ids=lambda c: c[0])
def test_depthwise_large(pkg, orc, ctx, case):
    _, n, h, ch, stride, bf16 = case
    _run_dw_big(pkg, orc, ctx, n, h, ch, stride, bf16)


@pytest.mark.parametrize("h", [3952, 3954], ids=["lds_below_2e9", "lds_above_2e9"])
def test_f32_depthwise_one_image_around_2e9(pkg, orc, ctx, h):
    """One fp32 image on either side of dw3x3_lds's 2e9-byte image limit (3952^2 x 32 x 4 = 1 999 101 952; 3954^2 x 32 x 4 = 2 001 125 888: the
    column march). The image's rows are periodic (row r = base[r % P]), so every interior output row equals the twin's row of the same phase
    (a twin image of h' = h mod P rows, h' >= 2 P + 2); the first and last rows equal the twin's first and last."""
    ch = 32
    rng = np.random.default_rng(h)
    base = rng.uniform(-1, 1, (P, h, ch)).astype(np.float32)            # P rows of the image
    f = rng.normal(0, 0.5, (3, 3, ch)).astype(np.float32)
    sc, sh = rng.uniform(0.5, 1.5, ch).astype(np.float32), rng.normal(0, 0.1, ch).astype(np.float32)
    ht = 2 * P + 2 + (h - 2 * P - 2) % P
    assert ht % P == h % P
    xt = base[np.arange(ht) % P]
    bufs = _Bufs(ctx)
    try:
        d_f, d_sc, d_sh = bufs.dev(f), bufs.dev(sc), bufs.dev(sh)
        ext = lambda rows: pkg.make_ext(batch=1, act=2, in_rows=rows, in_cols=h, scale=d_sc.ptr, shift=d_sh.ptr)
        d_tx, d_to = bufs.dev(xt), bufs.alloc(xt.nbytes)
        ctx.depthwise(d_to.ptr, d_tx.ptr, d_f.ptr, ht, h, 3, 1, ch, ext(ht))
        ctx.sync()
        twin = d_to.download(xt.shape, np.float32)
        assert_close(twin, orc.f32_depthwise(xt[None], f, sc, sh, 1, 2)[0], TOL_DW, "dw one-image twin")
        nbytes = h * h * ch * 4
        d_x, d_o = bufs.alloc(nbytes), bufs.alloc(nbytes + GUARD)
        _upload_periodic(ctx, d_x.ptr, base, h)
        _fill(ctx, d_o, nbytes + GUARD)
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, h, h, 3, 1, ch, ext(h))
        ctx.sync()
        what = "fp32 dw one image %dx%dx%d" % (h, h, ch)
        _check_guard(ctx, d_o, nbytes, what)

        def index(y):
            t = 1 + (y - 1) % P                                          # interior row: the twin's row of the same phase
            t[y == 0] = 0
            t[y == h - 1] = ht - 1
            return t
        _check_items(ctx, d_o.ptr, h, twin, index, what)
    finally:
        bufs.free()


# =========================================================================== int8 mode: no descriptors, every index 64-bit

def _i8_ext(pkg, batch, dm, db, f32=False, **kw):
    return pkg.make_ext(batch=batch, dtype=pkg.DT_I8, act=pkg.ACT_NONE if f32 else pkg.ACT_RELU6, scale=dm.ptr, shift=db.ptr,
                        io_flags=pkg.IO_OUT_F32 if f32 else 0, **kw)


I8_PW_CASES = [  # (name, m, K, N, fp32 output): each crosses the 2^31 and the 2^32 byte offset of the named tensor
    ("input_over_4g", (1 << 22) + 37, 1024, 8, False),       # input 4 295 005 184 bytes
    ("u8_output_over_4g", (1 << 22) + 37, 8, 1024, False),   # output 4 295 005 184 bytes
    ("f32_output_over_4g", 1073780, 8, 1000, True),          # output 4 295 120 000 bytes
]


@pytest.mark.parametrize("case", I8_PW_CASES, ids=lambda c: c[0])
def test_i8_pointwise_large(pkg, ctx, case):
    """int8 pointwise on m rows with row i = base[i % P]: the P-row twin against int8_ref.pw bit for bit, every output row against the twin."""
    _, m, cin, cout, f32 = case
    assert m % 32 != 0 and m % P != 0 and max(m * cin, m * cout * (4 if f32 else 1)) > GIB4
    es = 4 if f32 else 1
    rng = np.random.default_rng(m + cin + cout)
    x = rng.integers(0, 256, (P, cin), dtype=np.uint8)
    f = rng.integers(-127, 128, (cout, cin), dtype=np.int8)
    mult = (rng.uniform(1e-5, 1e-4, cout) if f32 else rng.uniform(0.2 / cin, 0.9 / cin, cout)).astype(np.float32)
    bias = rng.uniform(-40, 60, cout).astype(np.float32)
    bufs = _Bufs(ctx)
    try:
        d_f, d_m, d_b = bufs.dev(f), bufs.dev(mult), bufs.dev(bias)
        ext = _i8_ext(pkg, 1, d_m, d_b, f32)
        d_tx, d_to = bufs.dev(x), bufs.alloc(P * cout * es)
        ctx.pointwise(d_to.ptr, d_tx.ptr, d_f.ptr, P, 1, cin, cout, ext)
        ctx.sync()
        twin = d_to.download((P, cout), np.float32 if f32 else np.uint8)
        want = int8_ref.pw(x, f, mult, bias, out_f32=f32)
        assert np.array_equal(_bits(twin), _bits(want)), "i8 pw twin"
        out_bytes = m * cout * es
        d_x, d_o = bufs.alloc(m * cin), bufs.alloc(out_bytes + GUARD)
        _upload_periodic(ctx, d_x.ptr, x, m)
        _fill(ctx, d_o, out_bytes + GUARD)
        ctx.pointwise(d_o.ptr, d_x.ptr, d_f.ptr, m, 1, cin, cout, ext)
        ctx.sync()
        what = "i8 pw m=%d %d->%d%s" % (m, cin, cout, " fp32" if f32 else "")
        _check_guard(ctx, d_o, out_bytes, what)
        _check_periodic(ctx, d_o.ptr, m, twin, what)
    finally:
        bufs.free()


@pytest.mark.parametrize("stride", [1, 2], ids=["s1_over_4g", "s2_over_4g"])
def test_i8_depthwise_large(pkg, ctx, stride):
    """int8 depthwise on 5351 images of 112 x 112 x 64 (input 4 295 868 416 bytes; the stride-1 output as large) with image i = base[i % P]:
    the P-image twin against int8_ref.dw bit for bit, every output image against the twin."""
    n, h, ch = 5351, 112, 64
    assert n * h * h * ch > GIB4 and n % P != 0
    oh = (h + stride - 1) // stride
    rng = np.random.default_rng(n + stride)
    x = rng.integers(0, 256, (P, h, h, ch), dtype=np.uint8)
    f = rng.integers(-127, 128, (3, 3, ch), dtype=np.int8)
    mult = rng.uniform(2e-3, 8e-3, ch).astype(np.float32)
    bias = rng.uniform(-40, 60, ch).astype(np.float32)
    bufs = _Bufs(ctx)
    try:
        d_f, d_m, d_b = bufs.dev(f), bufs.dev(mult), bufs.dev(bias)
        ext = lambda nb: _i8_ext(pkg, nb, d_m, d_b, in_rows=h, in_cols=h)
        d_tx, d_to = bufs.dev(x), bufs.alloc(P * oh * oh * ch)
        ctx.depthwise(d_to.ptr, d_tx.ptr, d_f.ptr, oh, oh, 3, stride, ch, ext(P))
        ctx.sync()
        twin = d_to.download((P, oh, oh, ch), np.uint8)
        assert np.array_equal(twin, int8_ref.dw(x, f, mult, bias, stride)), "i8 dw twin"
        out_bytes = n * oh * oh * ch
        d_x, d_o = bufs.alloc(n * h * h * ch), bufs.alloc(out_bytes + GUARD)
        _upload_periodic(ctx, d_x.ptr, x, n)
        _fill(ctx, d_o, out_bytes + GUARD)
        ctx.depthwise(d_o.ptr, d_x.ptr, d_f.ptr, oh, oh, 3, stride, ch, ext(n))
        ctx.sync()
        what = "i8 dw n=%d %dx%dx%d s%d" % (n, h, h, ch, stride)
        _check_guard(ctx, d_o, out_bytes, what)
        _check_periodic(ctx, d_o.ptr, n, twin, what)
    finally:
        bufs.free()


# =========================================================================== bf16 resident tail

def _tail_params(rng, bufs, pkg, orc):
    blocks = (pkg.BlockParams * 2)()
    host = []
    for i, (ci, co) in enumerate(((256, 512), (512, 512))):
        wd, s2, b2, wp, s3, b3 = _params_dwpw(rng, ci, co)
        wp = orc.bf16_round(wp)
        host.append((wd, s2, b2, wp, s3, b3))
        d = [bufs.dev(a) for a in (wd, s2, b2)] + [bufs.dev(pkg.f32_to_bf16_bits(wp))] + [bufs.dev(a) for a in (s3, b3)]
        blocks[i] = pkg.BlockParams(*(b.ptr for b in d))
    return blocks, host


def test_bf16_tail_resident_input_around_4g(pkg, orc, ctx):
    """mbn_tail_resident_bf16 (10 x 10 x 256 -> two blocks -> pool) with the input just below 4 GiB (83 885 images: 4 294 912 000 bytes) against
    its P-image twin bit for bit; at 83 887 images (4 295 014 400 bytes) MBN_EUNSUPPORTED and nothing written."""
    r, c0, c1 = 10, 256, 512
    rng = np.random.default_rng(83885)
    x = orc.bf16_round(rng.uniform(0, 4, (P, r, r, c0)).astype(np.float32))
    bufs = _Bufs(ctx)
    try:
        blocks, host = _tail_params(rng, bufs, pkg, orc)
        call = lambda out, inp, nb: ctx.lib.mbn_tail_resident_bf16(ctx.h, out, inp, blocks, nb, r, r, c0, c1, None)
        d_tx, d_to = bufs.dev(pkg.f32_to_bf16_bits(x)), bufs.alloc(P * c1 * 2)
        _chk(pkg, ctx, call(d_to.ptr, d_tx.ptr, P), "tail twin")
        ctx.sync()
        twin = d_to.download((P, c1), np.uint16)
        t = x
        for k, (wd, s2, b2, wp, s3, b3) in enumerate(host):
            stride = 2 if k == 0 else 1
            oh = t.shape[1] // stride
            pad = 0 if stride == 2 else 1
            mid = orc.bf16_round(orc.f32_depthwise(t, wd, s2, b2, stride, 2, pad_top=pad, pad_left=pad))
            t = orc.bf16_round(orc.f32_pointwise(mid.reshape(-1, mid.shape[-1]), wp, s3, b3, 2).reshape(P, oh, oh, -1))
        want = orc.bf16_round(t.mean(axis=(1, 2)))
        assert_close(pkg.bf16_bits_to_f32(twin), want, TOL_BF16, "tail twin")
        for n, ok in ((83885, True), (83887, False)):
            in_bytes = n * r * r * c0 * 2
            assert (in_bytes < GIB4) == ok
            d_x, d_o = bufs.alloc(in_bytes), bufs.alloc(n * c1 * 2 + GUARD)
            _fill(ctx, d_o, n * c1 * 2 + GUARD)
            if ok:
                _upload_periodic(ctx, d_x.ptr, pkg.f32_to_bf16_bits(x), n)
                _chk(pkg, ctx, call(d_o.ptr, d_x.ptr, n), "tail n=%d" % n)
                ctx.sync()
                _check_guard(ctx, d_o, n * c1 * 2, "tail n=%d" % n)
                _check_periodic(ctx, d_o.ptr, n, twin, "tail n=%d" % n)
            else:
                assert call(d_o.ptr, d_x.ptr, n) == pkg.EUNSUPPORTED
                ctx.sync()
                _check_items(ctx, d_o.ptr, 1024, np.full((1, c1), 0xFFFF, np.uint16), lambda i: 0 * i, "refused tail")
            d_x.free()
            d_o.free()
    finally:
        bufs.free()


# =========================================================================== whole network at large batch

def _net_case(pkg, ctx, tmp_path, n, dtype, spans_in, spans_out, layers, fuse_stem=True, streams=1):
    """1.0x224 synthetic net: forward(n) on images i = base[i % P] against forward(P) bit for bit (logits of every image, and the chunked outputs
    of `layers`), with the launch spans mbn_net_launches reports checked first."""
    hw, net = _make_net(pkg, ctx, tmp_path, 1.0, 224, 1000, n)
    bufs = _Bufs(ctx)
    try:
        if dtype == pkg.DT_BF16:
            net.set_dtype(pkg.DT_BF16)
        net.set_fuse_stem(fuse_stem)
        if streams > 1:
            net.set_streams(streams)
        spans = net.launches(n)
        for s in spans_in:
            assert s in spans, "expected launch %s at batch %d: %s" % (s, n, spans)
        for s in spans_out:
            assert s not in spans, "unexpected launch %s at batch %d: %s" % (s, n, spans)
        rng = np.random.default_rng(n)
        base = (rng.random((P, 224, 224, 3), dtype=np.float32) * 2.0 - 1.0).astype(np.float32)
        d_in = bufs.alloc(n * base[0].nbytes)
        _upload_periodic(ctx, d_in.ptr, base, n)
        es = 2 if dtype == pkg.DT_BF16 else 4
        for k in list(layers) + [0]:
            l = hw.plan.layer[(k or hw.plan.n_layers) - 1]
            per = l.out_rows * l.out_cols * l.out_ch * (es if k else 4)
            d_t, d_o = bufs.alloc(P * per), bufs.alloc(n * per + GUARD)
            net.forward(d_in.ptr, d_t.ptr, P, k)
            ctx.sync()
            twin = d_t.download((P, per // es if k else per // 4), np.uint16 if (k and es == 2) else np.float32)
            assert np.all(np.isfinite(pkg.bf16_bits_to_f32(twin) if twin.dtype == np.uint16 else twin))
            _fill(ctx, d_o, n * per + GUARD)
            net.forward(d_in.ptr, d_o.ptr, n, k)
            ctx.sync()
            what = "net batch %d %s" % (n, ("layer %d output" % k) if k else "logits")
            _check_guard(ctx, d_o, n * per, what)
            _check_periodic(ctx, d_o.ptr, n, twin, what)
            d_t.free()
            d_o.free()
    finally:
        net.destroy()
        bufs.free()
        hw.free()


def test_net_fp32_batch700_general_offset_block(pkg, ctx, tmp_path):
    """Block 4-5's input (700 x 112^2 x 64 x 4 = 2 247 884 800 bytes) is past 0x70000000: the net fuses it on dwpw2's general offsets."""
    _net_case(pkg, ctx, tmp_path, 700, pkg.DT_F32, [(1, 3), (4, 2), (6, 2)], [], [5])


@pytest.mark.parametrize("fuse_stem", [True, False], ids=["stem_fused", "stem_unfused"])
def test_net_fp32_batch1399_unfused_block(pkg, ctx, tmp_path, fuse_stem):
    """Block 4-5's input (1399 x 112^2 x 64 x 4 = 4 492 558 336 bytes) is past 0xF0000000: the block runs as two layers; layers 2-3 are past
    4 GiB (the stem's output 4 492 558 336 bytes)."""
    stem = [(1, 3)] if fuse_stem else [(1, 1), (2, 1), (3, 1)]
    _net_case(pkg, ctx, tmp_path, 1399, pkg.DT_F32, stem + [(4, 1), (5, 1), (6, 2)], [(4, 2)], [3, 5], fuse_stem=fuse_stem)


def test_net_fp32_batch1300_two_streams_envelope_per_sub_batch(pkg, ctx, tmp_path):
    """Two streams: the envelope is decided per sub-batch of 650 (block 4-5's input 2 087 321 600 bytes, fused on general offsets), where the
    whole batch (4 174 643 200 bytes) would be past 0xF0000000."""
    _net_case(pkg, ctx, tmp_path, 1300, pkg.DT_F32, [(1, 3), (4, 2)], [(4, 1)], [5], streams=2)


def test_net_bf16_batch2700(pkg, ctx, tmp_path):
    """bf16 at batch 2700: block 4-5's input (4 334 665 728 bytes) is past 0xF0000000 (two layers), blocks 6-7 and 8-9 (2 167 332 864 bytes) past
    the bf16 fast_off limit (general offsets), the stem's output past 4 GiB."""
    _net_case(pkg, ctx, tmp_path, 2700, pkg.DT_BF16, [(1, 3), (4, 1), (5, 1), (6, 2), (8, 2)], [(4, 2)], [5, 7])
