"""Segment by sliding window on the host (no GPU): mbn_slide_axis / mbn_slide_plan against the two-line rule and its three properties, every
status of the plan, of the read-out's envelope (hand-made plans among them) and of its launch plan through libmbn_host.so; the identities of the
reference the GPU tests compare with (tests/dense_slide_ref.py); the struct that must not move and the new symbols where they belong."""
import ctypes as C

import numpy as np
import pytest

import dense_any_ref
import dense_prob_ref
import dense_slide_ref as S


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def logits_for(n, h, w, classes, seed=0):
    return (3.0 * np.random.default_rng(seed).standard_normal((n, h, w, classes))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------ the plan

def _sweep():
    """tile 4..40, every stride in [ceil(tile / 2), tile], size up to 6 tile + 6: every fourth tile and every third size keep it to a second"""
    for tile in range(4, 41, 4):
        for stride in range((tile + 1) // 2, tile + 1):
            for size in range(tile, 6 * tile + 7, 3):
                yield size, tile, stride
    for tile in (5, 7, 33, 39):
        for stride in range((tile + 1) // 2, tile + 1):
            for size in (tile, tile + 1, 2 * tile - 1, 2 * tile, 3 * tile + 1, 6 * tile + 6):
                yield size, tile, stride


def test_slide_axis_is_the_rule_and_has_its_properties(pkg):
    lib = pkg.host_lib()
    pos, n = (C.c_int32 * 17)(), C.c_int32()
    checked = three = 0
    for size, tile, stride in _sweep():
        want = S.axis(size, tile, stride)
        pos[16] = -77
        rc = lib.mbn_slide_axis(size, tile, stride, pos, C.byref(n))
        assert pos[16] == -77
        if len(want) > pkg.SLIDE_MAX_AXIS:
            assert rc == pkg.EUNSUPPORTED
            continue
        assert rc == pkg.OK and list(pos[:n.value]) == want, (size, tile, stride)
        p = np.array(want)
        assert p[0] == 0 and p[-1] == size - tile and (np.diff(p) > 0).all() and (np.diff(p) <= tile).all()        # ascending, flush, no gap
        cover = (p[:, None] <= np.arange(size)[None, :]) & (np.arange(size)[None, :] < p[:, None] + tile)          # [tile][coordinate]
        count = cover.sum(0)
        assert count.min() >= 1 and count.max() <= 3
        first, last = cover.argmax(0), len(p) - 1 - cover[::-1].argmax(0)
        assert (last - first + 1 == count).all(), "the tiles over a coordinate are a contiguous index range"
        assert len(np.unique(np.concatenate([p, p + tile]))) - 1 <= 2 * len(p) - 1                                  # cells of constant coverage
        three += int(count.max() == 3)
        checked += 1
    assert checked > 2000 and three > 100
    assert pkg.slide_axis(1000, 512, 341) == [0, 341, 488]                                                          # three over 488..511
    assert pkg.slide_axis(85, 40, 20) == [0, 20, 40, 45] and pkg.slide_axis(131, 61, 31) == [0, 31, 62, 70]
    assert pkg.slide_axis(7, 7, 7) == [0]


def test_slide_axis_and_plan_statuses(pkg):
    lib = pkg.host_lib()
    pos, n = (C.c_int32 * 16)(*([-5] * 16)), C.c_int32(-5)
    for bad in [(0, 4, 4), (10, 0, 4), (10, 4, 0), (-1, 4, 4), (10, -4, 2), (10, 4, -2), (10, 4, 5)]:            # non-positive; stride > tile: gaps
        assert lib.mbn_slide_axis(*bad, pos, C.byref(n)) == pkg.EINVAL, bad
    assert lib.mbn_slide_axis(10, 4, 4, None, C.byref(n)) == pkg.EINVAL and lib.mbn_slide_axis(10, 4, 4, pos, None) == pkg.EINVAL
    assert lib.mbn_slide_axis(10, 11, 11, pos, C.byref(n)) == pkg.EUNSUPPORTED                                      # tile > size: the letterbox's
    assert lib.mbn_slide_axis(100, 9, 4, pos, C.byref(n)) == pkg.EUNSUPPORTED                                       # stride < ceil(9 / 2)
    assert lib.mbn_slide_axis(100, 9, 5, pos, C.byref(n)) == pkg.EUNSUPPORTED                                       # 20 tiles
    assert lib.mbn_slide_axis(4 + 15 * 4, 4, 4, pos, C.byref(n)) == pkg.OK and n.value == 16
    n.value = -5
    for i in range(16):
        pos[i] = -5
    assert lib.mbn_slide_axis(4 + 15 * 4 + 1, 4, 4, pos, C.byref(n)) == pkg.EUNSUPPORTED                            # 17 tiles
    assert lib.mbn_slide_axis(2147483647, 2147483647, 2147483647, pos, C.byref(n)) == pkg.OK and n.value == 1 and pos[0] == 0
    n.value = -5
    pos[0] = -5
    assert lib.mbn_slide_axis(2147483647, 1, 1, pos, C.byref(n)) == pkg.EUNSUPPORTED
    assert n.value == -5 and list(pos) == [-5] * 16, "nothing is written on a refusal"

    s = pkg.slide_plan(85, 131, 40, 61, 20, 31)
    assert C.sizeof(pkg.Slide) == 144
    assert (s.tile_rows, s.tile_cols, s.ny, s.nx) == (40, 61, 4, 4) and s.ys == [0, 20, 40, 45] and s.xs == [0, 31, 62, 70]
    assert list(s.y[4:]) == [0] * 12 and list(s.x[4:]) == [0] * 12
    raw = (C.c_uint8 * 144)(*([0xAB] * 144))
    as_slide = C.cast(raw, C.POINTER(pkg.Slide))
    assert lib.mbn_slide_plan(85, 131, 40, 61, 20, 62, as_slide) == pkg.EINVAL                                      # stride > tile on x
    assert lib.mbn_slide_plan(85, 131, 90, 61, 20, 62, as_slide) == pkg.EINVAL                                      # EINVAL of x before EUNSUPPORTED of y
    assert lib.mbn_slide_plan(85, 131, 90, 61, 45, 31, as_slide) == pkg.EUNSUPPORTED                                # tile > size on y
    assert lib.mbn_slide_plan(85, 131, 40, 61, 20, 30, as_slide) == pkg.EUNSUPPORTED                                # stride < ceil(61 / 2)
    assert lib.mbn_slide_plan(0, 131, 40, 61, 20, 31, as_slide) == pkg.EINVAL
    assert bytes(raw) == b"\xab" * 144, "nothing is written on a refusal"
    assert lib.mbn_slide_plan(85, 131, 40, 61, 20, 31, None) == pkg.EINVAL
    with pytest.raises(pkg.MbnError):
        pkg.slide_plan(85, 131, 40, 61, 20, 62)


# -------------------------------------------------------------------------------------------------------------------- the envelope

def test_envelope_of_hand_made_plans(pkg):
    env = pkg.resample_slide_envelope
    ok = (8, 12, [0, 4, 9], [0, 6, 13])                                 # 2 x 3 maps at the minimum ratio over 17 x 25
    assert env(2, 2, 3, 21, ok, 17, 25) == pkg.OK
    assert env(2, 2, 3, 21, (8, 12, [0, 2, 9], [0, 1, 13]), 17, 25) == pkg.OK      # irregular: legal
    assert env(2, 2, 3, 21, None, 17, 25) == pkg.EINVAL
    for bad in [(0, 2, 3, 21, 17, 25), (2, 0, 3, 21, 17, 25), (2, 2, 0, 21, 17, 25), (2, 2, 3, 0, 17, 25), (2, 2, 3, 21, 0, 25), (2, 2, 3, 21, 17, -1)]:
        assert env(*bad[:4], ok, *bad[4:]) == pkg.EINVAL, bad
    einval = {"gap": (8, 12, [0, 9], [0, 6, 13]), "not flush": (8, 12, [0, 4, 8], [0, 6, 13]), "not from 0": (8, 12, [1, 4, 9], [0, 6, 13]),
              "not ascending": (8, 12, [0, 4, 4, 9], [0, 6, 13]), "descending": (8, 12, [0, 5, 4, 9], [0, 6, 13]), "ny 0": (8, 12, [], [0, 6, 13]),
              "nx 17": (8, 1, [0, 4, 9], list(range(17))), "tile 0": (0, 12, [0, 4, 9], [0, 6, 13]), "negative tile": (8, -12, [0, 4, 9], [0, 6, 13]),
              "gap on x": (8, 12, [0, 4, 9], [0, 13])}
    for name, p in einval.items():
        H, W = (17, 25) if name != "nx 17" else (17, 17)
        assert env(2, 2, 3, 21, p, H, W) == pkg.EINVAL, name
    s = pkg.slide(ok)
    s.y[7] = 1
    assert env(2, 2, 3, 21, s, 17, 25) == pkg.EINVAL, "a non-zero unused entry"
    s.y[7] = 0
    s.x[15] = -1
    assert env(2, 2, 3, 21, s, 17, 25) == pkg.EINVAL
    four = (8, 12, [0, 2, 4, 6, 9], [0, 6, 13])                         # rows 6, 7 lie under tiles 0..3
    assert env(2, 2, 3, 21, four, 17, 25) == pkg.EUNSUPPORTED
    assert env(2, 2, 3, 21, (8, 12, [0, 2, 4, 6, 9], [0, 13]), 17, 25) == pkg.EINVAL, "an MBN_EINVAL of x goes before an MBN_EUNSUPPORTED of y"
    assert env(2, 2, 3, 21, (8, 12, [0, 3, 6, 8, 11], [0, 6, 13]), 19, 25) == pkg.OK           # y[i + 3] = y[i] + tile: three at most
    assert env(2, 2, 3, 21, (8, 12, [0, 3, 6, 8, 10], [0, 6, 13]), 18, 25) == pkg.EUNSUPPORTED # row 10 lies under tiles 1..4
    assert env(2, 3, 3, 21, ok, 17, 25) == pkg.EUNSUPPORTED             # tile_rows < 4 x rows
    assert env(2, 2, 4, 21, ok, 17, 25) == pkg.EUNSUPPORTED             # tile_cols < 4 x cols
    big = (16384, 12, [0, 1], [0, 6, 13])
    assert env(1, 2, 3, 21, big, 16385, 25) == pkg.EUNSUPPORTED         # a side above 16384
    assert env(1, 2, 3, 21, (16383, 12, [0, 1], [0, 6, 13]), 16384, 25) == pkg.OK
    assert env(1, 2, 3, 21, (16384, 16384, [0], [0]), 16384, 16384) == pkg.OK
    assert env(1, 2, 3, 2 ** 28, ok, 17, 25) == pkg.EUNSUPPORTED        # a tile's logits at 2^31 bytes and beyond
    assert env(7281, 2, 3, 21, ok, 17, 25) == pkg.OK and env(7282, 2, 3, 21, ok, 17, 25) == pkg.EUNSUPPORTED       # batch * 9 maps against 65535
    assert env(2 ** 31 - 1, 2, 3, 21, ok, 17, 25) == pkg.EUNSUPPORTED
    for name in S.GEOMETRY:
        h, w, p, H, W = S.geometry_plan(name)
        assert env(2, h, w, 64, p, H, W) == pkg.OK, name
        assert pkg.slide_plan(H, W, p[0], p[1], *S.GEOMETRY[name][2]).ys == p[2]


def test_launch_plan(pkg):
    lib = pkg.host_lib()
    # the usual case: tile = 32 x map: a 3 x 3 footprint, 128 classes a chunk; rows [0, 150, 288] have two tiles over a coordinate at most, the
    # columns [0, 150, .., 750, 800] three
    p = pkg.slide_plan(512, 1024, 224, 224, 150, 150)
    l = pkg.resample_slide_plan(7, 7, p, 512, 1024)
    assert p.ys == [0, 150, 288] and p.xs == [0, 150, 300, 450, 600, 750, 800]
    assert (l.fy, l.fx, l.ch) == (3, 3, 128) and l.lds_bytes == 2 * 3 * 9 * 132 * 4 and l.span == 512 * 1024
    # the worst case: the minimum ratio and nine tiles over a piece: 9 x 10 x 10 vectors of 8 classes
    p = (40, 40, [0, 14, 28, 42], [0, 14, 28, 42])
    assert pkg.resample_slide_envelope(1, 10, 10, 21, p, 82, 82) == pkg.OK
    l = pkg.resample_slide_plan(10, 10, p, 82, 82)
    assert (l.fy, l.fx, l.ch) == (10, 10, 8) and l.lds_bytes == 43200 and l.lds_bytes <= 65536
    # every plan of the sweep's corners stays in 64 KB, and the grid is the pieces of the cells
    for name in S.GEOMETRY:
        h, w, p, H, W = S.geometry_plan(name)
        l = pkg.resample_slide_plan(h, w, p, H, W)
        th, tw, ys, xs = p

        def pieces(pos, tile):
            e = sorted(set(pos) | {v + tile for v in pos})
            return sum(-(-(b - a) // 32) for a, b in zip(e, e[1:])), max(sum(1 for v in pos if v <= a < v + tile) for a in e[:-1])

        (ny, ky), (nx, kx) = pieces(ys, th), pieces(xs, tw)
        assert l.tiles == ny * nx and l.span == H * W, name
        assert (ky, kx) == (3, 3) and l.lds_bytes == 9 * l.fy * l.fx * (l.ch + 4) * 4 <= 65536
        assert l.ch in (8, 16, 32, 64, 128) and (l.ch == 128 or 9 * l.fy * l.fx * (2 * l.ch + 4) * 4 > 65536), "the largest chunk that fits"
    assert S.geometry_plan("B")[2][:2] == (8, 12) and pkg.resample_slide_plan(2, 3, S.geometry_plan("B")[2], 17, 25).fy == 2
    one = pkg.resample_slide_plan(5, 7, (100, 150, [0], [0]), 100, 150)
    plain = pkg.resample_plan(5, 7, 100, 150)                          # one tile: the plain read-out's footprint and grid
    assert (one.fy, one.fx, one.tiles) == (plain.fy, plain.fx, plain.tiles) and one.tiles == 4 * 5
    l = pkg.ResampleLaunch()
    assert lib.mbn_resample_slide_plan(2, 3, None, 17, 25, C.byref(l)) == pkg.EINVAL
    assert lib.mbn_resample_slide_plan(2, 3, C.byref(pkg.slide(S.geometry_plan("B")[2])), 17, 25, None) == pkg.EINVAL


def test_symbols_where_they_belong(pkg):
    names = pkg.declared_symbols()
    for n in ("mbn_slide_axis", "mbn_slide_plan", "mbn_resample_slide_f32", "mbn_net_resize_tiles", "mbn_net_segment_slide"):
        assert n in names, n
    host = pkg.host_lib()
    for n in ("mbn_slide_axis", "mbn_slide_plan", "mbn_slide_check", "mbn_slide_cells", "mbn_resample_slide_envelope", "mbn_resample_slide_plan"):
        assert hasattr(host, n), n
    assert "mbn_resample_slide_envelope" not in names, "the envelope is the host's, not the public header's"


# ------------------------------------------------------------------------------------------------------------------- the reference

def test_geometry_cases_reach_every_count():
    for name in S.GEOMETRY:
        h, w, p, H, W = S.geometry_plan(name)
        assert set(np.unique(S.count_map(p, H, W)).tolist()) == S.COUNTS, name
    assert S.geometry_plan("A")[2][2:] == ([0, 20, 40, 45], [0, 31, 62, 70])


def test_reference_one_tile_is_the_plain_read_out():
    x = logits_for(2, 5, 7, 21, seed=3)
    lab, sc, pr = S.slide(x[:, None], (37, 61, [0], [0]), 37, 61)
    want_lab, want_sc = dense_any_ref.resample_argmax(x, 37, 61)
    assert np.array_equal(lab, want_lab) and np.array_equal(_bits(sc), _bits(want_sc))
    _, _, want_pr = dense_prob_ref.resample_softmax(x, 37, 61)
    assert np.array_equal(pr, want_pr)


def test_reference_count_1_pixels_are_their_tiles_plain_read_out():
    h, w, p, H, W = S.geometry_plan("A")
    th, tw, ys, xs = p
    x = np.stack([logits_for(2, h, w, 21, seed=10 + t) for t in range(len(ys) * len(xs))], axis=1)
    lab, sc, _ = S.slide(x, p, H, W)
    count = S.count_map(p, H, W)
    seen = 0
    for iy, y in enumerate(ys):
        for ix, x0 in enumerate(xs):
            tl, ts = dense_any_ref.resample_argmax(x[:, iy * len(xs) + ix], th, tw)
            alone = count[y:y + th, x0:x0 + tw] == 1
            seen += int(alone.sum())
            assert np.array_equal(lab[:, y:y + th, x0:x0 + tw][:, alone], tl[:, alone])
            assert np.array_equal(_bits(sc[:, y:y + th, x0:x0 + tw][:, alone]), _bits(ts[:, alone]))
    assert seen == int((count == 1).sum()) > 0


def test_reference_sums_in_tile_order():
    x = S.order_input()
    p = (8, 12, [0], [0, 4, 8])                                   # columns 8..11 lie under all three tiles
    lab, sc, _ = S.slide(x, p, 8, 20)
    assert (S.count_map(p, 8, 20)[:, 8:12] == 3).all()
    assert (sc[0, :, 8:12] == np.float32(1.0) / np.float32(3.0)).all() and (lab[0, :, 8:12] == 1).all()
    lab, sc, _ = S.slide(np.ascontiguousarray(x[:, [0, 2, 1]]), p, 8, 20)
    assert (sc[0, :, 8:12] == 0).all()


def test_threshold_cases_cut_through_their_maps():
    for case in S.THRESHOLD_CASES:
        n, name, classes, seed, sigma, min_prob = case
        h, w, p, H, W = S.geometry_plan(name)
        _, _, pr = S.slide(S.threshold_input(case), p, H, W)
        out = dense_prob_ref.excluded(pr, min_prob, classes)
        assert out.mean() <= 0.01
        below = (pr < min_prob)[~out].mean()
        assert 0.02 < below < 0.98, (case, below)
