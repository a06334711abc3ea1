"""Every persistent kernel at small planning CU counts, bit for bit.

mbn_set_planning_cus lets a context plan its launches for fewer CUs than the device has. At a count of 3, 8, 20 or 72 a shape of a few thousand
rows drives a tile loop through what a 256-CU launch reaches only with tens of thousands: a workgroup walking on to a second and third tile, the
next tile's loads under the current epilogue, ring slots carried across tiles, full rounds against the remainder round of pw3 / dwpw3, workgroups
without a tile, the vb_end of the XCD-group split. A kernel's per-element arithmetic does not depend on which workgroup takes which tile, so the
output must be the same bits at every count — and, on the exactly representable data of tests/exact_ref.py, the exact bits.

Per case (tests/cu_cases.py; tests/test_cu_count_cpu.py gates each on the CPU): one kernel call per count in COUNTS, then one at the device's own
count, each with the 0xFF canary behind the output; (i) array_equal with the exact bits at every count, (ii) the canary intact, (iii) array_equal
between each count and count 0. Where a count is outside the forced kernel's envelope the model says so (the case's id names those counts) and
whatever kernel takes the call is checked the same way. The count is restored in a finally. Lab routes skip on the shipped library.
"""
import numpy as np
import pytest

import cu_cases as CC
import cu_model as M
import test_exact_gpu as G

pytestmark = pytest.mark.gpu

EINVAL = -1


def _set(ctx, cus):
    assert ctx.lib.mbn_set_planning_cus(ctx.h, cus) == 0, cus


def _run(pkg, ctx, c, cus, lab):
    """one kernel call of case c; the helpers of test_exact_gpu.py compare with the exact bits and check the canary; returns the bits"""
    ls = CC.layers(c)
    f32 = "f32" if c.kind.endswith("f32") else None
    if c.kind.startswith("pw_"):
        inside = G.pw_route_eligible(c.knobs, c.shape, cus)
        assert inside == (CC.plan(c, cus, lab)["route"] == c.route or not _forced(c)), "model and envelope disagree at count %d" % cus
        return G._run_pw(pkg, ctx, ls[0], c.knobs, c.packed, dtype=f32, in_envelope=inside)
    if c.kind.startswith("block_"):
        return G._run_block(pkg, ctx, list(ls), c.knobs, dtype=f32)
    if c.kind.startswith("dw_"):
        return G._run_dw(pkg, ctx, ls[0], c.knobs, dtype=f32)
    if c.kind.startswith("stem_"):
        return G._run_stem(pkg, ctx, c.shape, ls, dtype=f32)
    if c.kind == "res":
        return G._run_res(pkg, ctx, c.shape, list(ls))
    if c.kind == "tail":
        return G._run_tail(pkg, ctx, c.shape, list(ls))
    raise ValueError(c.kind)


def _forced(c):
    """the knobs force a kernel that has an envelope of its own (test_exact_gpu.pw_route_eligible)"""
    return bool(c.knobs.get("pw_ring") or c.knobs.get("pw_emul") or c.knobs.get("pw_tile") == 9 or c.knobs.get("pw_splitk") == 2)


@pytest.mark.parametrize("case", CC.EXACT_CASES, ids=CC.case_id)
def test_kernel_is_count_invariant_and_exact(pkg, ctx, case):
    lab = G._lab(ctx)
    if case.lab and not lab:
        pytest.skip("lab route: this is the shipped libmbn.so (run with MBN_LAB=1 for the lab build)")
    device = G._cus(ctx)
    got = {}
    try:
        for cus in CC.COUNTS:
            if cus > device:
                continue
            _set(ctx, cus)
            assert G._cus(ctx) == cus
            if cus == case.count:
                assert CC.plan(case, cus, lab)["route"] == case.route
            got[cus] = _run(pkg, ctx, case, cus, lab)
        _set(ctx, 0)
        assert G._cus(ctx) == device
        got[0] = _run(pkg, ctx, case, device, lab)
    finally:
        _set(ctx, 0)
    assert case.count in got
    for cus in got:
        G.same_bits(got[cus], got[0], "%s: count %d against the device's own count" % (CC.case_id(case), cus))


@pytest.mark.parametrize("case", CC.I8, ids=lambda c: "i8-%dx%d-%s-cus%d" % (c.shape[0], c.shape[1], "f32" if c.shape[2] else "u8", c.count))
def test_int8_persistent_pointwise_at_small_counts(pkg, ctx, case):
    """The int8 persistent pointwise against int8_ref.pw, bit for bit, at every count: M from the launch plan at the case's count (three tiles for
    some workgroups, a ragged last tile), the plan of every other count printed."""
    import test_int8_gpu as I8
    m, k, n, f32 = CC.i8_shape(pkg, case, I8)
    x, wk, mult, bias = I8._pw_inputs(k + n + case.count, m, k, n, f32)
    device = G._cus(ctx)
    try:
        for cus in CC.COUNTS + (0,):
            if cus > device:
                continue
            _set(ctx, cus)
            p = pkg.i8_pw_plan(m, k, n, G._cus(ctx), True, f32)
            if cus == case.count:
                I8._assert_multipass(pkg, p, m)
                I8._assert_distinct_tiles(x, p.pt)
            print("i8 %d -> %d m=%d count %d: %s" % (k, n, m, cus, I8._plan_str(p, pkg)))
            I8._run_pw_checked(pkg, ctx, x, wk, mult, bias, f32)
    finally:
        _set(ctx, 0)


def test_planning_count_error_paths(pkg, ctx):
    device = G._cus(ctx)
    lib = ctx.lib
    try:
        assert lib.mbn_set_planning_cus(ctx.h, -1) == EINVAL
        assert lib.mbn_set_planning_cus(ctx.h, device + 1) == EINVAL
        assert lib.mbn_set_planning_cus(None, 8) == EINVAL
        assert G._cus(ctx) == device                              # a refused count changes nothing
        assert lib.mbn_set_planning_cus(ctx.h, 1) == 0 and G._cus(ctx) == 1
        assert lib.mbn_set_planning_cus(ctx.h, device) == 0 and G._cus(ctx) == device
        assert lib.mbn_set_planning_cus(ctx.h, 8) == 0 and G._cus(ctx) == 8 and ctx.device_cus() == 8
        assert lib.mbn_set_planning_cus(ctx.h, 0) == 0 and G._cus(ctx) == device
        with pytest.raises(pkg.MbnError):
            ctx.set_planning_cus(device + 1)
    finally:
        _set(ctx, 0)


# ----------------------------------------------------------------------------- one net test

def _net_expected_fused(orc, net, hw, n, cus):
    """The depthwise + pointwise blocks (first layer, 2) the fp32 runner fuses by default for n images at a count: those an explicit mask fuses
    (inside the kernels' envelope), less the ones the few-tiles rule of block_fusable (host/mbn_net.c:354-358) leaves as two launches."""
    is_block = lambda l: l[1] == 2 and hw.plan.layer[l[0] - 1].kind == orc.L_DW          # launches are 1-based
    net.set_fuse_blocks(net.get_fuse_blocks())
    forced = [l for l in net.launches(n) if is_block(l)]
    net.reset_fuse_blocks()
    keep = []
    for first, span in forced:
        q = hw.plan.layer[first]                                  # the pointwise layer behind depthwise layer `first`
        if M.net_block_fused_f32(n, q.out_rows, q.out_cols, q.out_ch, cus):
            keep.append((first, span))
    return keep, is_block


@pytest.mark.parametrize("cfg", [(0.5, 64, 5), (1.0, 64, 2)], ids=lambda c: "alpha%g-%dx%d-batch%d" % (c[0], c[1], c[1], c[2]))
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_net_at_small_counts(pkg, orc, ctx, tmp_path, cfg, bf):
    """A net created AFTER the count is set plans with it (mbn_device_cus returns the planning count). At counts 8, 20 and the device's own: every
    layer of a kept forward against the oracle at the existing tolerances, the launch list equal to what a profiled forward issues and — in fp32 —
    to the few-tiles rule evaluated for that count, and the logits of the default (fused) forward bit-identical across the counts.
    pw_splitk = 1 in all runs: split-K sums K in another order than the tiled GEMM and its envelope depends on the count (mbn_f32_pw_splitk.hip:138).
    No other count-dependent choice between differently ordered kernels turned up: pw3, dwpw3, dwpw2 and dwpw reproduce pw_gemm's bits, and the bf16
    pointwise kernel is chosen from K and N alone."""
    import test_parity_gpu as P
    alpha, res, n = cfg
    classes = 40
    imgs = np.random.default_rng(11).uniform(-1, 1, (n, res, res, 3)).astype(np.float32)
    oplan = orc.plan_build(alpha, res, classes)
    device = G._cus(ctx)
    logits = {}
    try:
        with G.Knobs(ctx, {"pw_splitk": 1}):
            for cus in (8, 20, 0):
                _set(ctx, cus)
                planning = G._cus(ctx)
                hw, net = P._make_net(pkg, ctx, tmp_path, alpha, res, classes, n)
                try:
                    if bf:
                        net.set_dtype(pkg.DT_BF16)
                    d_in, d_out = ctx.to_device(imgs), ctx.alloc(n * classes * 4)
                    # the launch list: what runs, and what the fusion rule gives for this count
                    listed = net.launches(n)
                    assert P._launches_run(ctx, net, hw.plan, d_in, n, 0) == len(listed), (cus, listed)
                    if not bf:
                        want_fused, is_block = _net_expected_fused(orc, net, hw, n, planning)
                        assert [tuple(l) for l in listed if is_block(l)] == want_fused, (cus, listed, want_fused)
                        assert listed == net.launches(n)
                    print("count %d (%d): launches %s" % (cus, planning, listed))
                    net.forward(d_in.ptr, d_out.ptr, n)
                    ctx.sync()
                    logits[cus] = d_out.download((n, classes), np.float32)
                    # every layer, each fed by the device's own previous layer
                    net.keep_activations(True)
                    net.forward(d_in.ptr, d_out.ptr, n)
                    ctx.sync()
                    kept = d_out.download((n, 1, 1, classes), np.float32)
                    prev = imgs
                    for i in range(hw.plan.n_layers):
                        got = kept if i == hw.plan.n_layers - 1 else net.layer_output(i + 1, n)
                        if bf and oplan.layer[i].kind == orc.L_FC:
                            l = oplan.layer[i]
                            w = orc.bf16_round(hw.blob[l.w_offset:l.w_offset + l.w_count]).reshape(l.out_ch, l.in_ch)
                            want = orc.f32_pointwise(prev.reshape(n, -1), w, None, hw.blob[l.shift_offset:l.shift_offset + l.out_ch], orc.ACT_NONE).reshape(n, 1, 1, -1)
                            P.assert_close(got, want, P.TOL_PW, "count %d bf16 FC" % cus)
                        else:
                            want = P._oracle_layer(orc, oplan, hw.blob, i, prev, bf)
                            P.assert_close(got.reshape(want.shape), want, P.TOL_BF16 if bf else P.TOL_NET, "count %d layer %d" % (cus, i + 1))
                        prev = got
                    full, _ = orc.net_forward(oplan, hw.blob, imgs, bf16=bf)
                    P.assert_close(logits[cus], full.reshape(n, classes), P.TOL_BF16_NET if bf else P.TOL_NET, "count %d logits" % cus)
                finally:
                    net.destroy()
    finally:
        _set(ctx, 0)
    assert G._cus(ctx) == device
    for cus in (8, 20):
        G.same_bits(logits[cus].view(np.uint32), logits[0].view(np.uint32), "logits at count %d against the device's own count" % cus)
