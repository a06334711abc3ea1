"""No GPU: the inputs of tests/test_exact_gpu.py are what they claim to be, the float64 reference equals the committed oracle, and the
exact comparison catches what the tolerance comparison lets through.

(1) Every case the GPU file runs goes through exact_ref.check_gate: per layer max sum|terms| < 2^24 grid units, |acc * scale| + |shift| < 2^24
    units of its own grid, the fp32 evaluation in two opposite orders equal to the float64 one bit for bit; in every tensor that gets rounded
    >= 20 % of the elements changed by the rounding and >= 16 exact ties in each direction (>= 2 under 4096 elements); behind a ReLU6 >= 40 %
    strictly inside (0, 6), >= 10 % at 0 and >= 2 % at 6. (A tensor with no clamp in front of it — act 0, the pooled mean — has no clamp shares
    to ask for.) These are conditions on the inputs, not measurements of any kernel.
    The cases of tests/test_epilogue_gpu.py (every act with scale / shift given or NULL, 12 per route) pass the same gate, and in each at least
    10 % of z = acc * scale + shift lie below 0, 20 % inside (0, 6) and 2 % above 6: the three regions in which none / ReLU / ReLU6 differ.
(2) exact_ref == oracle.f32_* + bf16_round bit for bit on these inputs (both are exact, so equality), ReLU and the NULL forms included.
(3) Six mutants of the reference — what a subtly wrong kernel would compute — all differ from it under array_equal; on the random-data recipe
    of test_parity_gpu.py most of them pass that file's assert_close(..., TOL_BF16). Four more, (g) - (j), are wrong epilogues: the wrong
    activation, a parameter dropped, the activation before the affine; each differs in every combination it applies to.
"""
import numpy as np
import pytest

import exact_ref as E
import test_exact_gpu as G
import test_epilogue_gpu as P

TOL_BF16 = 1e-2


def old_yardstick_accepts(got, want):
    """test_parity_gpu.py's assert_close(got, want, TOL_BF16) as a predicate: max |got - want| <= 1e-2 max|want| + 1e-7"""
    return float(np.abs(got - want).max()) <= TOL_BF16 * max(float(np.abs(want).max()), 1e-6) + 1e-7


def _gate(layers, what):
    figs = E.check_gate(layers, what)
    for l, f in zip(layers, figs):
        assert E.fp32_orders_agree(l), "%s (%s): the fp32 evaluation depends on the order" % (what, l.kind)
        c = f["coverage"]
        print("%s %-5s grid 2^%d terms 2^%.1f epilogue 2^%.1f %s" % (what, l.kind, np.log2(f["grid"]), np.log2(f["terms"]), np.log2(f["epilogue"]),
              "" if c["act"] != 2 and not f["rounded"] else "inside %.2f at0 %.2f at6 %.2f changed %.2f ties +%d -%d of %d" % (c["inside"], c["at0"], c["at6"], c["changed"], c["ties_up"], c["ties_down"], c["n"])))
    return figs


# ----------------------------------------------------------------------------- (1) the gate on every GPU case

@pytest.mark.parametrize("shape", sorted(set(G.PW_DEFAULT + G.PW_GENERIC + [c[1] for c in G.PW_LAB])))
def test_gate_bf16_pointwise(shape):
    _gate([G.pw_layer(shape, 2)], "pw %s" % (shape,))
    if shape in G.PW_DEFAULT + G.PW_GENERIC:
        _gate([G.pw_layer(shape, 0)], "pw act 0 %s" % (shape,))


def test_gate_bf16_pointwise_fc_form():
    (f,) = _gate([G.pw_layer(G.PW_FC, 0, True)], "fc")
    assert not f["rounded"]                           # fp32 out: nothing is rounded


@pytest.mark.parametrize("case", G.DW_CASES + [(n, h, c, 1, {}) for n, h, c in G.DW_LAB], ids=str)
def test_gate_bf16_depthwise(case):
    _gate([G.dw_layer(case)], "dw %s" % (case,))


@pytest.mark.parametrize("shape", G.POOL_CASES)
def test_gate_bf16_pool(shape):
    _gate([E.pool_layer(E.pool_case(*shape))], "pool %s" % (shape,))


@pytest.mark.parametrize("shape", G.BLOCK_CASES)
def test_gate_bf16_block_and_its_intermediate_rounding(shape):
    d, p = layers = G.block_layers(shape)
    _gate(layers, "block %s" % (shape,))
    # the contract rounds the depthwise output to bf16; a kernel that forgets to must be visible: the reference without that rounding
    # differs from the one with it in at least 1 % of the outputs
    skipped = E.bf16_rne(E.bn_act(E.pw_acc(d.y, p.w)[0], p.scale, p.shift, p.act))
    assert np.mean(skipped != p.out) >= 0.01, shape


@pytest.mark.parametrize("case", G.BLOCK_ASYM, ids=str)
def test_gate_bf16_block_asymmetric_pads(case):
    _gate(G.block_asym_layers(case), "block %s" % (case,))


@pytest.mark.parametrize("case", G.RES_CASES, ids=str)
def test_gate_bf16_resident_blocks(case):
    layers = G.res_layers(case)
    assert len(layers) == 2 * case[3] and (case[0] <= 16 or layers[0].x.shape[0] == 4)
    _gate(layers, "resident blocks %s" % (case,))


@pytest.mark.parametrize("case", G.TAIL_CASES, ids=str)
def test_gate_bf16_resident_tail(case):
    layers = G.tail_layers(case)
    px = layers[-1].x.shape[1] * layers[-1].x.shape[2]
    assert px & (px - 1) == 0, "the pooled map must have a power-of-two pixel count"
    _gate(layers, "resident tail %s" % (case,))


@pytest.mark.parametrize("case", G.STEM_CASES, ids=str)
def test_gate_bf16_fused_stem(case):
    layers = G.stem_layers(case)
    assert np.all(layers[0].w != 0), "conv1 filter: all 27 taps live"
    _gate(layers, "stem %s" % (case,))


def test_gate_f32_cases():
    """The fp32 cases: same generators, nothing rounded, so the gate asks for the clamp shares only (the upper clamp and the per-channel shift of the
    fp32 epilogues are what these cases are for); pw_emul's split is exact for operands of <= 8 significant bits."""
    for shape in G.F32_PW + [G.F32_PW_EMUL_DEFAULT]:
        l = G.pw_layer(shape, 2, False, False)
        _gate([l], "f32 pw %s" % (shape,))
        for a in (l.x, l.w):
            assert np.array_equal(E.bf16_rne(a), a)
    for n, h, c, s in G.F32_DW:
        _gate([G.dw_layer((n, h, c, s, {}), rounded=False)], "f32 dw %s" % ((n, h, c, s),))
    for shape in G.F32_BLOCK:
        _gate(G.block_layers(shape, rounded=False), "f32 block %s" % (shape,))
    for n, h, cout in G.F32_CONV1:
        _gate(E.conv1_case(n, h, h, cout), "f32 conv1 %s" % ((n, h, cout),))


def test_forced_routes_are_inside_their_kernels_envelopes():
    """Every forced-route case lies inside the envelope of the kernel its knob forces (on a 256-CU part; the GPU tests repeat this with the device's
    count), and the combinations left out of the fp32 list are outside: they would only have run the default kernel a second time."""
    for knobs, shape, packed in G.PW_LAB:
        assert G.pw_route_eligible(knobs, shape), (knobs, shape)
        assert packed == (knobs.get("pw_ring") == 6)
    for knobs, shape in G.F32_PW_ROUTES:
        assert G.pw_route_eligible(knobs, shape), (knobs, shape)
    assert {tuple(sorted(k)) for k, _ in G.F32_PW_ROUTES} == {(), ("pw_tile",), ("pw_splitk",), ("pw_emul", "pw_splitk", "pw_tile"), ("pw_emul",)}
    for shape in G.F32_PW[1:]:
        for knobs in ({"pw_tile": 9}, {"pw_splitk": 2}, {"pw_emul": 6}, {"pw_emul": 6, "pw_tile": 11}):
            assert not G.pw_route_eligible(knobs, shape), (knobs, shape)
    assert not G.pw_route_eligible({"pw_emul": 6}, G.F32_PW[0])           # 13 x 2 tiles of 128 x 128: needs a forced tile
    assert all(G.dw_lds_eligible(s) for s in G.DW_LAB)
    tiles = lambda s: -(-s[0] // 128) * (s[2] // 128)
    assert [tiles(s) > 512 for s in G.PW_DEFAULT] == [False] * 5 + [True] * 2      # more than one tile per workgroup of the persistent streaming grid


# ----------------------------------------------------------------------------- (1b) the gate on every case of the epilogue matrix

def _gate_matrix(layers, what):
    """All 12 cases of one route: the gate (with exact_ref.Z_SHARES of z = acc * scale + shift below 0, inside (0, 6) and above 6), and that one upload
    of the filter, two of the activations and one of each parameter vector serve them all. Prints the three shares of every case."""
    down = P.shared_operands(layers)
    assert down is not None and down <= 1.0, what           # (1: conv1's accumulator of a [-1, 1] image has the wanted spread as it is)
    assert sorted(layers) == sorted(E.COMBOS)
    for (act, params), l in layers.items():
        assert l.epilogue_case and l.act == act
        (f,) = _gate([l], "%s act %d %-5s" % (what, act, params))
        c = f["coverage"]
        print("    z < 0 %.3f   0 < z < 6 %.3f   z > 6 %.3f" % (c["neg"], c["mid"], c["high"]))
        assert c["neg"] >= 0.10 and c["mid"] >= 0.20 and c["high"] >= 0.02, (what, act, params, c)
    for p in E.PARAMS:                                 # z does not depend on act, and the three acts differ on it
        ys = [layers[(a, p)].y for a in E.ACTS]
        assert np.array_equal(layers[(0, p)].z, layers[(2, p)].z)
        assert not np.array_equal(ys[0], ys[1]) and not np.array_equal(ys[1], ys[2])


@pytest.mark.parametrize("shape", sorted(set(s for _, s in P.F32_PW_ROUTES)))
def test_gate_epilogue_f32_pointwise(shape):
    layers = P.pw_matrix(shape, rounded=False)
    _gate_matrix(layers, "epilogue f32 pw %s" % (shape,))
    for a in (layers[(2, "both")].x, layers[(2, "none")].x, layers[(2, "both")].w):      # pw_emul's split is exact for <= 8 significant bits
        assert np.array_equal(E.bf16_rne(a), a)


@pytest.mark.parametrize("route", P.BF16_PW_ROUTES, ids=str)
def test_gate_epilogue_bf16_pointwise(route):
    shape, out_f32 = route
    _gate_matrix(P.pw_matrix(shape, rounded=not out_f32), "epilogue bf16 pw %s%s" % (shape, " fp32 out" if out_f32 else ""))


@pytest.mark.parametrize("rounded", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", P.DW_ROUTES + [P.DW_LDS_LAB], ids=str)
def test_gate_epilogue_depthwise(case, rounded):
    if case == P.DW_LDS_LAB and rounded:
        return                                         # the LDS-staged form is fp32 only
    _gate_matrix(P.dw_matrix(case, rounded), "epilogue %s dw %s" % ("bf16" if rounded else "f32", case))


@pytest.mark.parametrize("rounded", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", P.CONV_ROUTES, ids=str)
def test_gate_epilogue_conv1(case, rounded):
    _gate_matrix(P.conv_matrix(case, rounded), "epilogue %s conv1 %s" % ("bf16" if rounded else "f32", case))


def test_epilogue_routes_are_inside_their_kernels_envelopes():
    """The forced fp32 pointwise routes lie inside the envelope of the kernel their knob forces; the two bf16 shapes meant for the streaming kernels'
    launcher are inside its envelope with the default combination and outside it with every other act."""
    for knobs, shape in P.F32_PW_ROUTES:
        assert G.pw_route_eligible({"pw_splitk": 2} if knobs.get("pw_splitk", 0) > 1 else knobs, shape), (knobs, shape)
    assert G.pw_route_eligible({"pw_tile": 9}, P.PW_SHAPE, act=2) and not G.pw_route_eligible({"pw_tile": 9}, P.PW_SHAPE, act=1)
    m, k, n = P.PW_SHAPE                               # split-K's default regime: a 4-image form of the call covers less than half of 256 CUs
    assert -(-4 * m // 64) * -(-n // 64) * 2 <= 256 and k >= 128 and k % 64 == 0
    for shape in [(397, 256, 256), (549, 64, 128)]:
        assert (shape, False) in P.BF16_PW_ROUTES
        assert G.pw_route_eligible({"pw_ring": 4}, (max(shape[0], 512),) + shape[1:], act=2) and not G.pw_route_eligible({"pw_ring": 4}, shape, act=0)
    assert (549, 64, 128)[0] >= 512 and (397, 256, 256)[1] >= 256       # the 32x32x16 form needs M >= 512, the 16x16x32 form (K >= 256) takes every M


# ----------------------------------------------------------------------------- (2) the reference is the oracle

def _oracle_layer(orc, l):
    """Layer l through the committed oracle, fp32 in and out"""
    x, w = l.x.astype(np.float32), l.w.astype(np.float32)
    sc, sh = (None if a is None else a.astype(np.float32) for a in (l.scale, l.shift))
    if l.kind == "pw":
        return orc.f32_pointwise(x, w, sc, sh, l.act)
    if l.kind == "conv1":
        return orc.f32_conv(x, w, sc, sh, 2, l.act)
    if l.kind == "pool":
        return orc.f32_pool(x)
    g = l.geom
    oh, ow, pt, pl = E.dw_geom(x.shape[1], x.shape[2], **g)
    d = g.get("dilation", 1)
    return orc.f32_depthwise(x, E.inflate(w, d) if d > 1 else w, sc, sh, g["stride"], l.act, out_rows=oh, out_cols=ow, pad_top=pt, pad_left=pl)


def test_reference_equals_oracle(orc, pkg):
    layers = [G.pw_layer(s, 2) for s in G.PW_DEFAULT[:3] + G.PW_GENERIC] + [G.pw_layer(G.PW_GENERIC[1], 0), G.pw_layer(G.PW_FC, 0, True)]
    layers += [G.dw_layer(c) for c in G.DW_CASES]
    layers += G.block_layers(G.BLOCK_CASES[2]) + G.block_asym_layers(G.BLOCK_ASYM[1]) + G.res_layers(G.RES_CASES[7]) + G.tail_layers(G.TAIL_CASES[1])
    layers += G.stem_layers(G.STEM_CASES[2]) + E.conv1_case(1, 33, 33, 8)
    layers += [E.pool_layer(E.pool_case(*s)) for s in G.POOL_CASES]
    # the epilogue matrix: per kind, ReLU with both parameters and every NULL form (under ReLU, no activation and ReLU6 in turn)
    for matrix in (P.pw_matrix((130, 8, 24), True), P.dw_matrix(P.DW_ROUTES[0], True), P.dw_matrix(P.DW_ROUTES[4], False), P.conv_matrix(P.CONV_ROUTES[1], False)):
        layers += [matrix[(1, "both")], matrix[(1, "scale")], matrix[(0, "shift")], matrix[(2, "none")], matrix[(1, "none")]]
    for l in layers:
        if l.kind == "pool" and l.x.shape[1] != l.x.shape[2]:
            continue                                   # the oracle's pool window is square
        want = _oracle_layer(orc, l)
        assert np.array_equal(want.astype(np.float64), l.y), (l.kind, l.x.shape)
        if l.rounded:
            assert np.array_equal(orc.bf16_round(want).astype(np.float64), l.out), (l.kind, l.x.shape)
            # ... and the two bf16 roundings the GPU file relies on agree, ties included
            assert np.array_equal(pkg.f32_to_bf16_bits(want), E.bf16_rne_bits(l.y))


def test_bf16_rne_on_bits():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -7, 6.0, 0.0, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -20])
    assert list(E.bf16_rne(v)) == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 6.0, 0.0, -1.0, 1.0 + 2.0 ** -7]
    assert list(E.bf16_truncate(v)) == [1.0, 1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7, 6.0, 0.0, -1.0, 1.0]
    assert list(E.bf16_ties_away(v)) == [1.0, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 6.0, 0.0, -(1.0 + 2.0 ** -7), 1.0 + 2.0 ** -7]
    c = E.coverage(v[:6])
    assert (c["ties_up"], c["ties_down"], c["changed"]) == (1, 1, 2 / 6)


# ----------------------------------------------------------------------------- (3) the mutants

def _swap_pairs(v):
    s = v.copy()
    n = v.size // 2 * 2
    s[0:n:2], s[1:n:2] = v[1:n:2], v[0:n:2]
    return s


def _pw_mutants(x2, w, scale, shift, rnd=E.bf16_rne, f32=lambda y: y):
    """name -> output of a pointwise layer computed wrongly in one way (x2 [M][K], act ReLU6, bf16 out). f32: how the fp32 value comes about that
    the rounding starts from (the identity on exact data)"""
    acc = x2 @ w.T
    y = E.relu6(acc * scale + shift)
    return {
        "a truncation": E.bf16_truncate(f32(y)),
        "b ties away": E.bf16_ties_away(f32(y)),
        "c shift of the neighbouring channel": rnd(E.relu6(acc * scale + _swap_pairs(shift))),
        "d last k-term dropped": rnd(E.relu6((acc - x2[:, -1:] * w[None, :, -1]) * scale + shift)),
        "f clamp at 6 before the shift": rnd(np.maximum(np.minimum(acc * scale, 6.0) + shift, 0.0)),
    }


def _block_mutants(d_y, w, scale, shift, rnd=E.bf16_rne, f32=lambda y: y):
    """the same for the pointwise stage of a block, plus (e): the depthwise intermediate d_y used unrounded"""
    mid = rnd(d_y).reshape(-1, d_y.shape[-1])
    m = _pw_mutants(mid, w, scale, shift, rnd, f32)
    m["e unrounded depthwise intermediate"] = rnd(E.relu6((d_y.reshape(mid.shape) @ w.T) * scale + shift))
    return m


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def test_mutants_exact_comparison_catches_all_old_yardstick_few():
    """Each of (a) truncation, (b) ties away from zero, (c) shift swapped between channels 2c and 2c + 1, (d) last k-term dropped, (e) depthwise
    intermediate not rounded, (f) clamp at 6 before the shift — applied to the reference of one exact pointwise case (300, 512, 512) and one exact
    block case (3, 14, 64 -> 128) — differs from the true reference under array_equal. ((e) exists for the block only.)

    The same mutations on test_parity_gpu.py's random recipe (x ~ U(-1, 1) rounded to bf16, filter ~ N(0, 2 / K), scale in [0.5, 1.5], shift ~ N(0, 0.1))
    against assert_close(got, want, TOL_BF16), i.e. max |got - want| <= 1e-2 max|want|, same shapes:
      accepted: (a), (b)   at most one bf16 ulp, 2^-5 = 0.031 below 8, under the bound of about 0.05
                (e)        a depthwise value moves by half an ulp at most; times a filter row of norm ~ sqrt(2) far under the bound
                (f)        IDENTICAL to the reference: |acc * scale| stays below 6 on this recipe, the upper clamp is never reached at all
      rejected: (c)        the maximum over the tensor finds a channel pair whose shifts differ by several tenths
                (d)        likewise: max over all outputs of |x_K w_cK scale_c| reaches ~ 1 x 3.5 sigma_w x 1.5 = 0.3 at K = 512 — the "0.02" of a
                           TYPICAL element does not decide a max norm; the yardstick does see a dropped term at this K, if only in its worst elements
    so four of the six were invisible, and nothing pinned the clamp."""
    # exact data
    (l,) = [G.pw_layer((300, 512, 512), 2)]
    for name, got in _pw_mutants(l.x, l.w, l.scale, l.shift).items():
        assert not np.array_equal(got, l.out), "pointwise: mutant (%s) not caught" % name
    d, p = G.block_layers((3, 14, 64, 128, 1))
    for name, got in _block_mutants(d.y, p.w, p.scale, p.shift).items():
        assert not np.array_equal(got, p.out), "block: mutant (%s) not caught" % name
    # random data, the old yardstick
    rnd = lambda y: E.bf16_rne(_f32(y))
    rng = np.random.default_rng(300 + 512 + 512)
    x = rnd(rng.uniform(-1, 1, (300, 512)))
    w = rnd(rng.normal(0, (2.0 / 512) ** 0.5, (512, 512)))
    sc, sh = _f32(rng.uniform(0.5, 1.5, 512)), _f32(rng.normal(0, 0.1, 512))
    want = rnd(E.relu6((x @ w.T) * sc + sh))
    verdict = {name[0]: old_yardstick_accepts(got, want) for name, got in _pw_mutants(x, w, sc, sh, rnd, _f32).items()}
    assert verdict == {"a": True, "b": True, "c": False, "d": False, "f": True}, verdict
    assert np.array_equal(_pw_mutants(x, w, sc, sh, rnd, _f32)["f clamp at 6 before the shift"], want)          # the clamp is never exercised
    rng = np.random.default_rng(14 * 13 + 64 + 128 + 1)
    xb = rnd(rng.uniform(0, 4, (3, 14, 14, 64)))
    wd = _f32(rng.normal(0, 0.5, (3, 3, 64)))
    wp = rnd(rng.normal(0, (2.0 / 64) ** 0.5, (128, 64)))
    s2, s3 = _f32(rng.uniform(0.5, 1.5, 64)), _f32(rng.uniform(0.5, 1.5, 128))
    b2, b3 = _f32(rng.normal(0, 0.1, 64)), _f32(rng.normal(0, 0.1, 128))
    d_y = _f32(E.relu6(E.dw_acc(xb, wd, stride=1, pad_top=1, pad_left=1)[0] * s2 + b2))
    want = rnd(E.relu6((rnd(d_y).reshape(-1, 64) @ wp.T) * s3 + b3))
    verdict = {name[0]: old_yardstick_accepts(got, want) for name, got in _block_mutants(d_y, wp, s3, b3, rnd, _f32).items()}
    assert verdict["a"] and verdict["b"] and verdict["e"], verdict


def _epilogue_mutants(l):
    """name -> what a kernel with one wrong epilogue would give for layer l (before the bf16 rounding), or None where the mutation does not apply
    to l's combination: (g) ReLU6 where ReLU was asked, (h) ReLU where no activation was asked, (i) `ss = scale && shift` applied to the arithmetic:
    both parameters dropped when only one is NULL, (j) the activation applied before the affine."""
    sc = 1.0 if l.scale is None else l.scale
    sh = 0.0 if l.shift is None else l.shift
    act = lambda v, a=l.act: E.bn_act(v, None, None, a)
    return {
        "g ReLU6 for ReLU": E.relu6(l.z) if l.act == E.ACT_RELU else None,
        "h ReLU for none": np.maximum(l.z, 0.0) if l.act == E.ACT_NONE else None,
        "i both dropped when one is NULL": act(l.acc) if (l.scale is None) != (l.shift is None) else None,
        # (with a shift; or a scale alone under ReLU6, whose upper clamp does not commute with it. ReLU commutes with a positive scale.)
        "j activation before the affine": act(l.acc) * sc + sh if l.act != E.ACT_NONE and (l.shift is not None or (l.scale is not None and l.act == E.ACT_RELU6)) else None,
    }


def test_epilogue_mutants_are_caught_and_the_old_relu_test_was_blind():
    """(g) - (j) on one pointwise and one depthwise case of the epilogue matrix (the bf16 forms: the mutant's value is rounded as the reference's is):
    every mutant differs from the reference under array_equal in EVERY combination it applies to — (g) under ReLU with each of the four parameter
    forms, (h) under no activation with each of the four, (i) under each act with scale alone and with shift alone, (j) under ReLU and ReLU6 with
    both and with shift alone, and under ReLU6 with scale alone (under ReLU a positive scale alone commutes with the activation). On test_parity_gpu.py's ReLU recipe (test_f32_depthwise_explicit_padding_and_generic_path: x ~ U(-1, 1),
    filter ~ N(0, 0.5), stride 2, neither parameter) mutant (g) IS the reference: |acc| stays far below 6, so a kernel that clamps at 6 under ReLU
    passed that test whatever its tolerance."""
    for matrix, what in ((P.pw_matrix((130, 8, 24), True), "pointwise"), (P.dw_matrix(P.DW_ROUTES[0], True), "depthwise")):
        hit = {}
        for (a, p), l in matrix.items():
            for name, got in _epilogue_mutants(l).items():
                if got is not None:
                    assert not np.array_equal(E.bf16_rne(got), l.out), "%s act %d %s: mutant (%s) not caught" % (what, a, p, name)
                    assert not np.array_equal(got, l.y)
                    hit[name[0]] = hit.get(name[0], 0) + 1
        assert hit == {"g": 4, "h": 4, "i": 6, "j": 5}, hit
    rng = np.random.default_rng(3)
    for ch in (8, 6):
        x = _f32(rng.uniform(-1, 1, (2, 12, 12, ch)))
        f = _f32(rng.normal(0, 0.5, (3, 3, ch)))
        z = E.dw_acc(x, f, stride=2, pad_top=1, pad_left=1, out_rows=6, out_cols=6)[0]
        assert z.max() < 6.0 and z.min() < 0.0 < z.max()
        assert np.array_equal(E.relu6(z), np.maximum(z, 0.0))
