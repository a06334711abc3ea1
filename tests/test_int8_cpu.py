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


# ------------------------------------------------------------------------------------------- the pointwise launch plan (mbn_i8_pw_plan)

def _plan(pkg, m, k, n, cus=256, on16=True, f32=False):
    return pkg.i8_pw_plan(m, k, n, cus, on16, f32)


def test_pw_plan_first_second_tile_n1024(pkg):
    """N = 1024 on 256 CUs: 32 chunks = 4 column groups (gy) of cpw = 8 chunks, so 8 waves with rep = 1, one resident workgroup per CU
    and per_round = 256 * 1 / 4 = 64 slots per group. The largest tile is min(32768 / K, 160 KB / (2 (K + 16))) rounded down to 32 and
    capped at 1024: 1024, 512, 256, 128, 64, 32 pixels for K = 32 ... 1024 (the first term decides each). 64 such tiles hold 2^16,
    2^15, ... 2^11 pixels, so one pixel more is the first M that needs a second round: rounds = 2, and the tile shrinks to
    ceil(M / 128) rounded up to 32. The rows of the issue's table (a hand mirror; a few pixels above these) are multi-pass as well."""
    for k, ptmax, pt2, issue_m in ((32, 1024, 544, 65559), (64, 512, 288, 32777), (128, 256, 160, 16386), (256, 128, 96, 8209),
                                   (512, 64, 64, 4102), (1024, 32, 32, 2067)):
        last1 = 64 * ptmax
        p = _plan(pkg, last1, k, 1024)
        assert (p.form, p.pt, p.ntiles, p.gx, p.gy, p.rounds) == (pkg.I8_PW_PERSISTENT, ptmax, 64, 64, 4, 1), k
        p = _plan(pkg, last1 + 1, k, 1024)
        # 2 rounds x 64 slots: ceil((last1 + 1) / 128) = ptmax / 2 + 1 -> up to 32: ptmax / 2 + 32 (K = 512, 1024: the cap ptmax)
        assert p.pt == pt2 == min(ptmax, ptmax // 2 + 32) and p.rounds == 2, k
        assert (p.ntiles, p.gx) == (-(-(last1 + 1) // pt2), 64) and p.ntiles > p.gx, k
        assert (p.ks, p.kp, p.cpw, p.rep, p.resident, p.threads, p.per_round) == (k // 32, k, 8, 1, 1, 512, 64), k
        assert p.lds_bytes == 2 * pt2 * (k + 16) and p.g == 16 and p.maxg == (8 if k <= 128 else 4)
        q = _plan(pkg, issue_m, k, 1024)
        assert q.form == pkg.I8_PW_PERSISTENT and q.ntiles > q.gx == 64, k


def test_pw_plan_first_second_tile_n64(pkg):
    """N = 64: two chunks, one column group, cpw = 2, rep = 4 / 2 = 2 (four waves), resident = 12 / 4 = 3, per_round = 768. Largest tile:
    K = 32: min(1024, 54613 / 96 = 568) -> 544; K = 256: min(128, 54613 / 544 = 100) -> 96; K = 1024: 32. 768 of them hold 417 792,
    73 728 and 24 576 pixels: M must exceed those for a second tile."""
    for k, last1 in ((32, 417792), (256, 73728), (1024, 24576)):
        p = _plan(pkg, last1, k, 64)
        assert (p.form, p.rounds, p.per_round, p.resident, p.cpw) == (pkg.I8_PW_PERSISTENT, 1, 768, 3, 2) and p.ntiles <= p.gx
        p = _plan(pkg, last1 + 1, k, 64)
        assert p.rounds == 2 and p.ntiles > p.gx == 768, k


def test_pw_plan_three_subtile_groups_384_threads(pkg):
    """K = 256 -> N = 64, M = 150 000: cpw = 2, rep = 2, resident = 3, the largest tile 96 (above). ceil(150000 / 96) = 1563 tiles over 768
    slots: 3 rounds, and ceil(150000 / 2304) = 66 -> 96 keeps the tile. Staging 96 x (256 / 16) = 1536 granules > MAXG 4 x 256 threads:
    rep -> 3, 4 x 384 = 1536 fits. So 6 waves, nrep = 3."""
    p = _plan(pkg, 150000, 256, 64)
    assert (p.form, p.pt, p.rep, p.cpw, p.threads, p.ntiles, p.gx, p.rounds) == (pkg.I8_PW_PERSISTENT, 96, 3, 2, 384, 1563, 768, 3)
    assert p.lds_bytes == 2 * 96 * 272 and p.maxg == 4 and p.ks == 8


def test_pw_plan_tile_shrinks_for_short_maps(pkg):
    """14 x 14 x 512 -> 512 (M = 196): gy = 2, per_round = 128, largest tile 64: 4 tiles, one round; ceil(196 / 128) = 2 -> 32: 7 tiles of
    32 pixels on 7 slots instead of 4 of 64. 28 x 28 x 256 -> 256 (M = 784): largest tile 128, per_round 256, ceil(784 / 256) = 4 -> 32:
    25 tiles. 7 x 7 x 1024 -> 1024: the 32-pixel minimum, 2 tiles. An FC on 5 images: one tile."""
    p = _plan(pkg, 196, 512, 512)
    assert (p.pt, p.ntiles, p.gx, p.gy, p.rounds, p.lds_bytes) == (32, 7, 7, 2, 1, 2 * 32 * 528)
    p = _plan(pkg, 784, 256, 256)
    assert (p.pt, p.ntiles, p.gx, p.gy, p.rounds) == (32, 25, 25, 1, 1)
    p = _plan(pkg, 49, 1024, 1024)
    assert (p.pt, p.ntiles, p.gx, p.gy) == (32, 2, 2, 4)
    p = _plan(pkg, 5, 1024, 1000, f32=True)
    assert (p.form, p.ks, p.pt, p.ntiles, p.gx, p.gy, p.out_f32) == (pkg.I8_PW_PERSISTENT, 32, 32, 1, 1, 4, 1)


def test_pw_plan_k_in_registers_forms(pkg):
    """The K-in-registers form i8_pw_k<ks, g>: ks = 4 / 16 / 32 for K <= 128 / <= 512 / above, K blocks of 32 ks bytes.
    - K % 16 == 8 stages 8-byte granules, K / 8 per pixel. K = 504: 63 x 32 pixels = 2016 <= MAXG 4 x 512 threads = 2048: persistent, on
      8 waves (N = 40: cpw = 2, rep 4). K = 520: 65 x 32 = 2080 > 2048 even at 8 waves and the smallest tile: falls through; so does
      K = 1016 (127 x 32 = 4064). One K block of 1024 bytes each.
    - K > 1024: K = 2048 two whole blocks, K = 1040 a 16-byte second block (g = 16), K = 1032 an 8-byte one (g = 8).
    - operands on 8 but not 16 bytes with K % 16 == 0: K = 64 -> <4, 8>, 256 -> <16, 8>, 1024 -> <32, 8>, one block each.
    M = 997 is 8 tiles of 128; N = 40 two chunks; 2 x 256 CUs / 8 tiles asks for more groups than chunks: cpg = 1, 2 groups, 16 workgroups."""
    p = _plan(pkg, 997, 504, 40)
    assert (p.form, p.g, p.pt, p.threads, p.rep, p.ks) == (pkg.I8_PW_PERSISTENT, 8, 32, 512, 4, 16)
    for k, on16, ks, g, nkb in ((520, True, 32, 8, 1), (1016, True, 32, 8, 1), (2048, True, 32, 16, 2), (1040, True, 32, 16, 2),
                                (1032, True, 32, 8, 2), (64, False, 4, 8, 1), (256, False, 16, 8, 1), (1024, False, 32, 8, 1),
                                (2048, False, 32, 8, 2)):
        for f32 in (False, True):
            p = _plan(pkg, 997, k, 40, on16=on16, f32=f32)
            assert (p.form, p.ks, p.g, p.nkb, p.out_f32) == (pkg.I8_PW_KREG, ks, g, nkb, int(f32)), k
            assert (p.pt, p.threads, p.ntiles, p.nchunks, p.cpg, p.ngroups, p.gx, p.gy, p.lds_bytes) == (128, 256, 8, 2, 1, 2, 16, 1, 0)
    # many tiles: 2 * 256 / 4000 -> one group of all chunks
    p = _plan(pkg, 512000, 2048, 1000)
    assert (p.ntiles, p.nchunks, p.cpg, p.ngroups, p.gx) == (4000, 32, 32, 1, 4000)
    # the grid's 2^31 - 1 workgroups; shapes the C-ABI refuses
    host = pkg.host_lib()
    q = pkg.I8PwPlan()
    assert host.mbn_i8_pw_plan(1 << 40, 2048, 8, 256, 1, 0, C.byref(q)) == pkg.EUNSUPPORTED
    for bad in ((0, 64, 64, 256), (5, 12, 64, 256), (5, 0, 64, 256), (5, 65544, 64, 256), (5, 64, 0, 256), (5, 64, 64, 0)):
        assert host.mbn_i8_pw_plan(*bad, 1, 0, C.byref(q)) == pkg.EINVAL, bad
    assert host.mbn_i8_pw_plan(5, 64, 64, 256, 1, 0, None) == pkg.EINVAL


def test_pw_plan_aligned_small_k_forms(pkg):
    """Which K-in-registers forms operands on 16 bytes with K <= 1024, K % 16 == 0 can reach. <4, 16> (K <= 128): none in the sweep.
    <16, 16> and <32, 16> with one K block: reached when the chunks per workgroup are 3, 5, 6 or 7 (N in 65..96 or 129..224, and wherever
    else ceil(chunks / gy) is one of them) and a tile needs more staging threads than the waves have: `rep` is raised while cpw * rep < 8,
    lands on 9, 10, 12 or 14 waves, and the plan falls through instead of shrinking the tile. K = 256 -> N = 160 on 256 CUs: cpw = 5, resident 2, largest tile 128, per_round
    512: up to M = 32 768 the tile is <= 64 (64 x 16 = 1024 granules <= 4 x 320 threads), at M = 32 769 it is 96 (1536 > 1280)."""
    assert _plan(pkg, 32768, 256, 160).form == pkg.I8_PW_PERSISTENT
    p = _plan(pkg, 32769, 256, 160)
    assert (p.form, p.ks, p.g, p.nkb) == (pkg.I8_PW_KREG, 16, 16, 1)
    p = _plan(pkg, 1, 1024, 160)                  # K = 1024: 32 x 64 = 2048 granules > 4 x 320 at any M
    assert (p.form, p.ks, p.g, p.nkb) == (pkg.I8_PW_KREG, 32, 16, 1)
    seen = set()
    for cus in (1, 8, 104, 256, 304):
        for k in range(16, 1025, 16):
            for n in (8, 40, 64, 96, 136, 160, 192, 224, 264, 520, 1000, 1024, 1320):
                for m in (1, 33, 997, 4097, 32769, 150000, 1 << 22):
                    p = _plan(pkg, m, k, n, cus)
                    if p.form == pkg.I8_PW_KREG:
                        seen.add((p.ks, p.g))
                        chunks = (n + 31) // 32
                        gy = (chunks + 7) // 8
                        assert (chunks + gy - 1) // gy in (3, 5, 6, 7), (m, k, n, cus)
    assert seen == {(16, 16), (32, 16)}


def test_pw_plan_invariants_over_a_sweep(pkg):
    """Every persistent plan: whole 32-pixel sub-tiles, at most 8 waves made of cpw x rep, the staging bound the kernel's MAXG registers
    rely on, both LDS buffers within 160 KB, no workgroup without a first tile, the tiles cover M, and the KS instantiation holds K.
    Every K-in-registers plan: groups cover the chunks, grid = tiles x groups."""
    n_p = n_k = 0
    for cus in (1, 8, 104, 256, 304):
        for k in list(range(8, 257, 8)) + [384, 504, 512, 520, 768, 1000, 1016, 1024, 1032, 1040, 2048, 4104, 65536]:
            for n in (1, 3, 8, 24, 40, 64, 100, 128, 160, 256, 264, 1000, 1001, 1024, 2048):
                for m in (1, 31, 32, 33, 196, 997, 3136, 8209, 32777, 65559, 150000, 417793, (1 << 22) + 37):
                    for on16 in (True, False):
                        p = _plan(pkg, m, k, n, cus, on16)
                        chunks = (n + 31) // 32
                        if p.form == pkg.I8_PW_PERSISTENT:
                            n_p += 1
                            waves = p.cpw * p.rep
                            assert k <= 1024 and (on16 or k % 16) and p.g == (16 if k % 16 == 0 else 8)
                            assert p.pt % 32 == 0 and 32 <= p.pt <= 1024
                            assert 1 <= waves <= 8 and p.threads == 64 * waves      # (rep may exceed pt / 32: those waves only stage)
                            assert p.pt * (k // p.g) <= p.maxg * p.threads and p.maxg == (8 if p.ks <= 4 else 4)
                            assert p.kp % 32 == 0 and k <= p.kp < k + 32 and p.kp // 32 <= p.ks < 2 * max(1, p.kp // 32)
                            assert p.lds_bytes == 2 * p.pt * (p.kp + 16) <= 160 * 1024
                            assert p.ntiles == -(-m // p.pt) and 1 <= p.gx <= p.ntiles and p.gx <= p.per_round
                            assert p.gy * p.cpw >= chunks > (p.gy - 1) * p.cpw
                        else:
                            n_k += 1
                            assert p.form == pkg.I8_PW_KREG and p.pt == 128 and p.threads == 256 and p.lds_bytes == 0
                            assert p.ks == (4 if k <= 128 else 16 if k <= 512 else 32) and p.nkb == -(-k // (32 * p.ks))
                            assert p.g == (16 if (k % 16 == 0 and on16) else 8)
                            assert p.nchunks == chunks and p.ngroups * p.cpg >= chunks > (p.ngroups - 1) * p.cpg
                            assert p.ntiles == -(-m // 128) and p.gx == p.ntiles * p.ngroups
    assert n_p > 20000 and n_k > 10000


# ------------------------------------------------------------------------------------------------------------ conv1 on grid inputs

def test_conv1_grid_inputs_are_exact_in_fp32():
    """The gate of tests/test_int8_gpu.py::test_conv1_bit_exact_on_grid_inputs, on the very inputs it builds: max sum |term| in grid units
    (2^-13) stays below 2^24, so the fp32 sum is exact in any order and with any fusing; shown as well by summing the 27 terms in fp32 forwards
    and backwards against float64. The worst case the builder can produce is 27 x 2^7 x 2^7 = 442 368 units. Each case reaches both clamps and
    leaves at least half of its outputs between them."""
    assert 27 * (1 << ref.CONV1_IMG_BITS) * (2 << ref.CONV1_TAP_BITS) < 2 ** 24
    for c in ref.CONV1_CHANNELS:
        for stride in (1, 2):
            for h, w in ref.CONV1_MAPS:
                for pads in ref.CONV1_PADS:
                    rng = np.random.default_rng(c * 100 + stride * 10 + h)
                    img, wk, mult, bias = ref.conv1_exact_inputs(rng, 2, h, w, c)
                    assert np.abs(img).max() <= 1 and np.abs(wk).max() <= 2
                    assert ref.conv1_grid_units(img, wk, stride, *pads) < 2 ** 24
                    got = ref.conv1_exact(img, wk, mult, bias, stride, *pads)
                    lo, hi = (got == 0).mean(), (got == 255).mean()
                    assert lo > 0 and hi > 0 and lo + hi <= 0.5, (c, stride, h, w, pads, lo, hi)
    # one case term by term: fp32 sums in both orders equal the float64 sum
    rng = np.random.default_rng(1)
    img, wk, _, _ = ref.conv1_exact_inputs(rng, 1, 9, 7, 8)
    xp = np.zeros((11, 9, 3), np.float32)
    xp[1:10, 1:8] = img[0]
    for oy, ox in ((0, 0), (4, 3), (8, 6)):
        terms = (xp[oy:oy + 3, ox:ox + 3].reshape(27, 1) * wk.reshape(27, 8)).astype(np.float32)      # each product exact
        fwd = np.zeros(8, np.float32)
        bwd = np.zeros(8, np.float32)
        for t in range(27):
            fwd = (fwd + terms[t]).astype(np.float32)
            bwd = (bwd + terms[26 - t]).astype(np.float32)
        want = ref.conv1_acc(img, wk, 1)[0, oy, ox]
        assert np.array_equal(fwd.astype(np.float64), want) and np.array_equal(bwd.astype(np.float64), want)
