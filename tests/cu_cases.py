"""The cases of tests/test_cu_count_gpu.py: (kernel route, knobs, shape, planning CU count), each sized from tests/cu_model.py.

A case names the kernel it is for (`route`), the tune knobs that force or admit it, the smallest shape at which — at the planning count `count` —
the kernel's tile loop goes through what a 256-CU launch reaches only with tens of thousands of rows, and whether it needs the lab library.
plan(case, cus) evaluates the dispatch and the launcher for a count and returns the launch (route, tiles, grid, tiles per workgroup or wave, ...);
gate(case) asserts the conditions at the case's own count. tests/test_cu_count_cpu.py runs the gate and the exact-data gate for every case;
the GPU test runs every case at each of COUNTS and at the device's own count. Test infrastructure only; not a conftest.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import cu_model as M
import exact_ref as E
import test_exact_gpu as G

COUNTS = (3, 8, 20, 72)       # below one CU per XCD; one per XCD; a grid that is no multiple of 8; per_xcd = 9, not divisible by 2, 4 or 8
DEVICE = 256                  # the count the CPU side evaluates "count 0" with (MI355X); the GPU test asks the device

Case = namedtuple("Case", "kind route knobs shape count lab packed")


def case(kind, route, knobs, shape, count, lab=False, packed=False):
    return Case(kind, route, dict(knobs), tuple(shape), count, lab, packed)


def case_id(c):
    knobs = "-".join("%s%d" % kv for kv in sorted(c.knobs.items())) or "default"
    outside = [n for n in COUNTS + (DEVICE,) if plan(c, n)["route"] != c.route]
    return "%s-%s-%s-%s-cus%d%s" % (c.kind, c.route, knobs, "x".join(map(str, c.shape)), c.count,
                                      "-other_kernel_at_" + "_".join("%d" % n for n in outside) if outside else "")


# ----------------------------------------------------------------------------- the lists
# fp32 pointwise, (M, K, N). Sizes: 64 x 64 tiles at count 3 are 4 workgroups per CU = 12, so 15 x 2 = 30 tiles give 3, 3, ... 2 per workgroup;
# 128 x 128 tiles (2 per CU = 6 workgroups) take 7 x 2 = 14; pw3 at count 8 has per_round = 8 waves per XCD, so 155 tiles of 32 rows are 19 or 20 per
# XCD = 2 full rounds + 3 or 4; K = 512 runs 12 waves on 64-channel slices: N = 512 is 8 slices, count 72 gives per_xcd = 9 -> 8, 235 tiles = 29 or 30 per XCD.
PW_F32 = [
    case("pw_f32", "gemm3", {"pw_tile": 3}, (14 * 64 + 37, 64, 128), 3),
    case("pw_f32", "gemm1", {"pw_tile": 1}, (6 * 128 + 50, 64, 256), 3, lab=True),
    case("pw_f32", "gemm5", {"pw_tile": 10}, (16384 + 128 + 37, 64, 128), 8),            # pw3 off: the rule's 128 x 128 tile needs M > 16384
    case("pw_f32", "gemm3", {"pw_tile": 10}, (14 * 64 + 37, 128, 128), 3),               # ... and its 64 x 64 tile at K = 128 (4 k-tiles)
    case("pw_f32", "gemm-nbuf1", {"pw_tile": 3}, (130, 8, 24), 3),                       # single k-tile: one workgroup per tile at every count
    case("pw_f32", "gemm-xn2", {}, (8 * 64 + 37, 1024, 1024), 8),                        # a 4 MB filter: two XCD groups along n
    case("pw_f32", "pw3", {"pw_tile": 9}, (155 * 32 - 13, 64, 128), 8),
    case("pw_f32", "pw3", {"pw_tile": 9}, (155 * 32 - 13, 128, 128), 8),
    case("pw_f32", "pw3", {"pw_tile": 9}, (155 * 32 - 13, 256, 128), 8),
    case("pw_f32", "pw3", {"pw_tile": 9}, (155 * 32 - 13, 256, 256), 20),                # two slices: needs 16 CUs
    case("pw_f32", "pw3", {"pw_tile": 9}, (235 * 32 - 7, 512, 512), 72),
    case("pw_f32", "splitk", {"pw_splitk": 2}, (100, 128, 64), 8),                       # 7 x 4 tiles of 16 x 16: 32 x 32 tiles up to count 13
    case("pw_f32", "x6-11", {"pw_emul": 6, "pw_splitk": 1, "pw_tile": 11}, (6 * 128 + 50, 64, 256), 3),
    case("pw_f32", "x6-6", {"pw_emul": 6, "pw_splitk": 1, "pw_tile": 6}, (6 * 128 + 50, 64, 256), 3),
    case("pw_f32", "x6-7", {"pw_emul": 6, "pw_splitk": 1, "pw_tile": 7}, (6 * 128 + 50, 64, 192), 3),
]
# fp32 fused blocks, (batch, side, Cin, Cout, stride): 5 images of 14 x 14 outputs are 980 pixels = 8 row tiles of 128 on 3 workgroups; dwpw3 walks
# 32-pixel wave tiles: 25 images = 4900 pixels = 154 tiles
BLOCK_F32 = [
    case("block_f32", "dwpw2-128", {}, (5, 14, 64, 128, 1), 3),
    case("block_f32", "dwpw2-128", {}, (5, 28, 64, 128, 2), 3),
    case("block_f32", "dwpw2-256", {}, (5, 28, 64, 256, 2), 3),
    case("block_f32", "dwpw2-256", {"dwpw_variant": 2}, (5, 14, 64, 256, 1), 3, lab=True),
    case("block_f32", "dwpw-256", {}, (5, 14, 64, 256, 1), 3),
    case("block_f32", "dwpw-128", {"dwpw_variant": 1}, (5, 14, 64, 128, 1), 3, lab=True),
    case("block_f32", "dwpw-128", {"dwpw_variant": 1}, (5, 28, 64, 128, 2), 3, lab=True),
    case("block_f32", "dwpw-256", {"dwpw_variant": 1}, (5, 28, 64, 256, 2), 3, lab=True),
    case("block_f32", "dwpw3", {}, (25, 14, 128, 128, 1), 8),
    case("block_f32", "dwpw3", {}, (25, 14, 256, 256, 1), 20),
    case("block_f32", "x6-128", {"pw_emul": 6}, (5, 14, 64, 128, 1), 3),
]
# fp32 depthwise (batch, side, channels, stride): not persistent; the count moves the row segments (mbn_f32_dw.h). exp0 = 6: the LDS-staged form
DW_F32 = [
    case("dw_f32", "march", {}, (2, 28, 256, 1), 3),
    case("dw_f32", "lds", {"exp0": 6}, (2, 28, 64, 1), 3, lab=True),
]
# (batch, rows, cols, c1, c3): 2 tiles of 8 x 16 outputs per 32 x 32 image; 2 / 4 workgroups per CU
STEM_F32 = [
    case("stem_f32", "stem", {}, (7, 32, 32, 32, 64), 3),
    case("stem_f32", "stem", {}, (13, 32, 32, 16, 32), 3),
]

# bf16 pointwise. The streaming kernel runs 2 workgroups per CU on 128 x 128 tiles (3 A slots), ring / wide / big one per CU
PW_BF16 = [
    case("pw_bf16", "stream", {}, (13 * 128 + 37, 128, 128), 3),
    case("pw_bf16", "stream16", {}, (13 * 128 + 37, 256, 128), 3),
    case("pw_bf16", "ring", {"pw_ring": 2}, (7 * 128 + 37, 128, 128), 3, lab=True),
    case("pw_bf16", "ring", {"pw_ring": 2}, (7 * 256 + 37, 256, 128), 3, lab=True),
    case("pw_bf16", "wide", {"pw_ring": 6}, (7 * 196 + 50, 256, 256), 3, lab=True, packed=True),
    case("pw_bf16", "big", {"pw_ring": 7}, (10 * 256 + 37, 128, 256), 3, lab=True),
    case("pw_bf16", "rf", {"pw_ring": 8}, (37 * 32 - 5, 512, 256), 8, lab=True),
]
BLOCK_BF16 = [
    case("block_bf16", "dwpw2-128", {}, (5, 14, 64, 128, 1), 3),
    case("block_bf16", "dwpw2-128", {}, (5, 28, 64, 128, 2), 3),
    case("block_bf16", "dwpw2-256", {}, (5, 14, 64, 256, 1), 3),
    case("block_bf16", "dwpw2-h32", {}, (9, 14, 32, 64, 1), 3),                          # Cin = 32: 256-row tiles, 1764 pixels = 7 tiles
    case("block_bf16", "dwpw-128", {"dwpw_variant": 1}, (5, 14, 64, 128, 1), 3, lab=True),
]
DW_BF16 = [
    case("dw_bf16", "march", {}, (2, 14, 512, 1), 3),
    case("dw_bf16", "lds", {"exp0": 8}, (4, 14, 64, 1), 3, lab=True),
]
# (batch, rows, cols, blocks): a batch of 2 * count + 1 gives 3, 2, 2 ... images per workgroup; the tail takes two images per pass
RES = [case("res", "res", {}, (7, 10, 10, 2), 3), case("res", "res", {}, (17, 6, 16, 1), 8)]
TAIL = [case("tail", "tail", {}, (13, 8, 8), 3)]
STEM_BF16 = [
    case("stem_bf16", "stem", {}, (10, 32, 32, 32, 64), 3),
    case("stem_bf16", "stem", {}, (16, 32, 32, 16, 32), 3),
]
# int8 persistent pointwise (K, N, fp32 out): M comes from the launch plan at the case's count (test_int8_gpu._multipass_m)
I8 = [case("i8", "persistent", {}, (64, 64, 0), 3), case("i8", "persistent", {}, (256, 128, 0), 8), case("i8", "persistent", {}, (128, 32, 1), 20)]

EXACT_CASES = PW_F32 + BLOCK_F32 + DW_F32 + STEM_F32 + PW_BF16 + BLOCK_BF16 + DW_BF16 + RES + TAIL + STEM_BF16
ALL_CASES = EXACT_CASES + I8


# ----------------------------------------------------------------------------- exact layers of a case (shared, built once)

def layers(c):
    """The exact_ref layers of a case (built once per kind and shape); the last one is what the kernel's output is compared with."""
    return _layers(c.kind, c.shape)


@functools.lru_cache(maxsize=None)
def _layers(kind, shape):
    c = Case(kind, None, None, shape, None, None, None)
    f32 = c.kind.endswith("f32")
    if c.kind.startswith("pw_"):
        return (G.pw_layer(c.shape, 2, False, not f32),)
    if c.kind.startswith("block_"):
        n, h, cin, cout, stride = c.shape
        return tuple(E.block_case(n, h, h, cin, cout, stride, rounded=not f32))
    if c.kind.startswith("dw_"):
        n, h, ch, stride = c.shape
        return (G.dw_layer((n, h, ch, stride, {}), rounded=not f32),)
    if c.kind.startswith("stem_"):
        return tuple(E.stem_case(*c.shape, rounded=not f32))
    if c.kind == "res":
        return tuple(G.res_layers(c.shape))
    if c.kind == "tail":
        return tuple(G.tail_layers(c.shape))
    raise ValueError(c.kind)


# ----------------------------------------------------------------------------- the launch of a case at a count

def _strided_plan(route, nwg, grid, nk=1, depth=0, remap=True):
    per = M.strided(nwg, grid, remap)[2]
    return dict(route=route, tiles=nwg, grid=grid, per=per, nk=nk, depth=depth)


def _pw3_plan(route, tiles, nh, cus, nw):
    grid = M.pw3_grid(tiles, nh, cus)
    if grid is None:
        return None
    _, _, ntile, per_xcd = M.pw3_visits(tiles, nh, grid, nw)
    return dict(route=route, tiles=tiles, grid=grid, per=ntile.ravel(), units=grid * nw, per_xcd=per_xcd, nh=nh)


def _plan_pw_f32(c, cus, lab):
    m, k, n = c.shape
    kn = c.knobs
    tile = kn.get("pw_tile", 0)
    if kn.get("pw_emul") and G.pw_route_eligible(kn, c.shape, cus):                 # mbn_f32_pw.hip:604, mbn_f32_pw_x6.hip:663-690
        bm, bn, per_cu = M.x6_per_cu(tile)
        nwg = M.cdiv(m, bm) * M.cdiv(n, bn)
        return _strided_plan("x6-%d" % tile, nwg, M.persistent_grid(cus, per_cu, nwg), nk=k // 32)
    if tile == 0:                                                                 # mbn_f32_pw.hip:607
        tb = M.splitk_taken(m, k, n, 1, cus, kn.get("pw_splitk", 0))
        if tb:
            nwg = M.cdiv(m, 16 * tb) * M.cdiv(n, 16 * tb)
            return dict(route="splitk", tiles=nwg, grid=nwg, per=np.ones(nwg, np.int64), tb=tb)
    if (tile == 9 or (tile == 0 and M.pw3_default(m, k, n, cus))) and G.pw_route_eligible({"pw_tile": 9}, c.shape, cus):      # :658
        p = _pw3_plan("pw3", M.cdiv(m, 32), n // (64 if k == 512 else 128), cus, 12 if k == 512 else 8)
        if p:
            return p
    if tile in (9, 10) or (not lab and tile not in M.SHIPPED_PW_TILES):           # :666, :669
        tile = 0
    if tile == 0:
        tile = M.pw_gemm_rule_tile(m, k, n, cus)
    p = M.pw_gemm_plan(m, k, n, cus, M.PW_GEMM_F32_TILES[tile])
    wg, mi, ni, per = M.pw_gemm_visits(p)
    route = "gemm-nbuf1" if p["nbuf"] == 1 else "gemm-xn%d" % p["xn"] if p["xn"] > 1 else "gemm%d" % tile
    return dict(route=route, tiles=p["nwg"], grid=p["grid"], per=per, nk=p["nk"], depth=0, xn=p["xn"])


def _plan_pw_bf16(c, cus, lab):
    m, k, n = c.shape
    ring = c.knobs.get("pw_ring", 0) if lab else 0
    forced = ring in (2, 6, 7, 8) and G.pw_route_eligible(c.knobs, c.shape, cus)
    if forced and ring == 6:                                                      # mbn_bf16_pw_wide.hip:327-332
        nwg = M.cdiv(m, 196) * (n // 256)
        return _strided_plan("wide", nwg, M.persistent_grid(cus, 1, nwg), nk=k // 64, depth=3)
    if forced and ring == 7:                                                      # mbn_bf16_pw_stream.hip:453-481: whole rounds, one workgroup per CU
        tiles = M.big_tiles(m, n, cus)
        assert tiles
        return _strided_plan("big", tiles, cus, nk=k // 64, depth=2)
    if forced and ring == 8:                                                      # mbn_bf16_pw_rf.hip:196-206
        mt, nh = M.cdiv(m, 32), n // 256
        p = M.rf_plan(mt, nh, cus)
        _, _, nt = M.rf_visits(mt, nh, p["gq"], p["grid"])
        return dict(route="rf", tiles=mt, grid=p["grid"], per=nt, units=8 * p["gq"], gq=p["gq"])
    if k % 64 == 0 and n % 128 == 0 and (k >= 256 or (m >= 512 and (k <= 128 or ring == 4))) and ring in (0, 4, 6, 8):      # mbn_f32_pw.hip:642-650
        nwg = M.cdiv(m, 128) * (n // 128)
        return _strided_plan("stream16" if k >= 256 or c.knobs.get("misc") == 16 else "stream", nwg, M.persistent_grid(cus, 2, nwg), nk=k // 64, depth=3)
    if forced and ring == 2:                                                      # mbn_bf16_pw_ring.hip:235-257
        big = k >= 256
        nwg = M.cdiv(m, 256 if big else 128) * (n // 128)
        return _strided_plan("ring", nwg, M.persistent_grid(cus, 1, nwg), nk=k // 64, depth=3 if big else 4)
    tile = M.pw_gemm_rule_tile(m, k, n, cus, bf=True)
    cfg = M.PW_GEMM_BF16_TILES[tile] if (tile != 3 or n >= 128) else (64, 64, 32, 32)
    p = M.pw_gemm_plan(m, k, n, cus, cfg, esize=2)
    return dict(route="gemm%d" % tile, tiles=p["nwg"], grid=p["grid"], per=M.pw_gemm_visits(p)[3], nk=p["nk"], depth=0)


def _plan_block(c, cus, lab, bf):
    n, h, cin, cout, stride = c.shape
    oh = M.cdiv(h, stride)
    m = n * oh * oh
    dv = c.knobs.get("dwpw_variant", 0) if lab else 0
    mt = M.cdiv(m, 128)
    wide2 = cout % 256 == 0 and mt * (cout // 256) >= cus                         # mbn_f32_dwpw2.hip:641, mbn_bf16_dwpw2.hip:423
    if bf:                                                                        # mbn_abi.hip:1147-1153
        if dv == 1 and cout % 128 == 0 and cin % 64 == 0:
            bn = 256 if cout % 256 == 0 else 128                                  # mbn_bf16_dwpw.hip:217
            nwg = mt * (cout // bn)
            return _strided_plan("dwpw-%d" % bn, nwg, M.persistent_grid(cus, 1, nwg), nk=cin // 64)
        if cin == 32 and not wide2:                                               # mbn_bf16_dwpw2.hip:366-376: the 256-row tile of Cin = 32
            nwg = M.cdiv(m, 256) * M.cdiv(cout, 128)
            return _strided_plan("dwpw2-h32", nwg, M.persistent_grid(cus, 1, nwg))
        bn = 256 if wide2 else 128
        nwg = mt * M.cdiv(cout, bn)
        return _strided_plan("dwpw2-%d" % bn, nwg, M.persistent_grid(cus, 1, nwg), nk=M.cdiv(cin, 64))
    if c.knobs.get("pw_emul") and dv == 0 and cin <= 512:                         # mbn_abi.hip:1071, mbn_f32_dwpw2_x6.hip:283-284
        bn = 256 if (cout == 256 and cin <= 256 and mt >= cus) else 128
        nwg = mt * (cout // bn)
        return _strided_plan("x6-%d" % bn, nwg, M.persistent_grid(cus, 1, nwg), nk=cin // 32)
    if (dv == 11 or (dv == 0 and stride == 1 and cin >= 128)) and cin in (64, 128, 256) and cout % 128 == 0 and (lab or (stride == 1 and cin >= 128)):      # :1076
        p = _pw3_plan("dwpw3", M.cdiv(m, 32), cout // 128, cus, 8)
        if p:
            return p
    small = mt * (cout // 256) < cus                                              # mbn_abi.hip:1078-1085
    if dv != 1 and (dv >= 2 or cout % 256 != 0 or small or stride == 2):
        bn = 256 if wide2 else 128
        nwg = mt * (cout // bn)
        return _strided_plan("dwpw2-%d" % bn, nwg, M.persistent_grid(cus, 1, nwg), nk=cin // 32)
    bn = 256 if cout % 256 == 0 else 128                                          # mbn_f32_dwpw.hip:236
    nwg = mt * (cout // bn)
    return _strided_plan("dwpw-%d" % bn, nwg, M.persistent_grid(cus, 1, nwg), nk=cin // 32)


def _plan_dw(c, cus, lab, bf):
    n, h, ch, stride = c.shape
    rows = cols = M.cdiv(h, stride)
    e0 = c.knobs.get("exp0", 0) if lab else 0
    if bf and e0 == 8:
        seg = M.dw_lds_bf16_segments(n, rows, cols, ch, cus)
        if seg:
            return dict(route="lds", seg=seg)
    if not bf and e0 == 6:
        return dict(route="lds", seg=M.dw_lds_f32_segments(n, rows, cols, stride, ch, False, 0, cus))
    resident = n * (h * h + rows * cols) * ch * (2 if bf else 4) < 64 * 1048576
    row_lanes = n * M.cdiv(cols, 2) * (ch // (8 if bf else 4))
    return dict(route="march", seg=M.dw_march_segments(row_lanes, rows, stride, resident, cus))


def plan(c, cus, lab=True, pkg=None):
    """The launch case c makes on a context planning for `cus` CUs: route = the kernel that takes the call."""
    if c.kind == "pw_f32":
        return _plan_pw_f32(c, cus, lab)
    if c.kind == "pw_bf16":
        return _plan_pw_bf16(c, cus, lab)
    if c.kind in ("block_f32", "block_bf16"):
        return _plan_block(c, cus, lab, c.kind == "block_bf16")
    if c.kind in ("dw_f32", "dw_bf16"):
        return _plan_dw(c, cus, lab, c.kind == "dw_bf16")
    if c.kind in ("stem_f32", "stem_bf16"):
        n, rows, cols, c1, c3 = c.shape
        p = M.stem_plan(n, rows, cols, c1, c.kind == "stem_bf16", cus)
        return _strided_plan("stem", p["nwg"], p["grid"], remap=False)
    if c.kind == "res":
        _, per, grid = M.res_visits(c.shape[0], cus)
        return dict(route="res", tiles=c.shape[0], grid=grid, per=per, nk=1, depth=0)
    if c.kind == "tail":
        _, per, grid = M.tail_visits(c.shape[0], cus)
        return dict(route="tail", tiles=(c.shape[0] + 1) // 2, grid=grid, per=per, nk=1, depth=0)
    if c.kind == "i8":
        return dict(route="persistent")
    raise ValueError(c.kind)


def i8_shape(pkg, c, I8mod):
    """(M, K, N, f32) of an int8 case: the smallest ragged M whose plan at the case's count walks three tiles (test_int8_gpu._multipass_m)"""
    k, n, f32 = c.shape
    return I8mod._multipass_m(pkg, c.count, k, n, bool(f32)), k, n, bool(f32)


def gate(c, lab=True):
    """The conditions of a case at its own planning count (conditions, not measurements). Returns a line of figures."""
    p = plan(c, c.count, lab)
    assert p["route"] == c.route, "%s: at count %d the call runs %s" % (c, c.count, p["route"])
    if c.kind.startswith("dw_"):
        segs = {n: plan(c, n, lab)["seg"] for n in COUNTS + (DEVICE,)}
        assert len(set(segs.values())) >= 2, "the row segments do not move with the count: %s" % segs
        return "segments (rows per segment, segments) by count %s" % segs
    if c.route == "splitk":
        tbs = {n: plan(c, n, lab)["tb"] for n in COUNTS + (DEVICE,)}
        assert set(tbs.values()) == {1, 2}, tbs
        return "16 x 16 blocks per tile side by count %s" % tbs
    if c.route == "gemm-nbuf1":
        for n in COUNTS + (DEVICE,):
            q = plan(c, n, lab)
            assert q["route"] == c.route and q["grid"] == q["tiles"], "the single-k-tile launch moved with the count"
        return "tiles %d grid %d at every count" % (p["tiles"], p["grid"])
    per, tiles, grid = np.asarray(p["per"]), p["tiles"], p["grid"]
    units = p.get("units", grid)
    assert per.sum() == tiles * p.get("nh", 1)
    assert per.max() >= 3, "no workgroup or wave takes three tiles: %s" % per.max()
    if c.route != "big":                                 # (the big-tile form takes whole rounds by construction; its remainder rows go to pw_gemm)
        assert tiles % units != 0, "the tile count %d is a multiple of the grid %d" % (tiles, units)
    if c.route in ("pw3", "dwpw3"):
        assert any(full >= 2 and 0 < rem < pr for full, rem, pr in p["per_xcd"]), p["per_xcd"]
    if c.route == "rf":
        assert per.max() >= 5, "no stream runs past its 4-stage ring"
    if p.get("depth"):
        assert per.max() * p["nk"] > p["depth"], "the ring of %d slots never wraps" % p["depth"]
    if c.route == "gemm-xn2":
        assert p["xn"] == 2
    return "tiles %d grid %d max tiles per workgroup%s %d" % (tiles, grid, " wave" if "units" in p and c.route != "rf" else "", per.max())
