"""Score a segmentation at its boundaries on the GPU: mbn_boundary_depth / mbn_boundary_score_i32 and their ragged forms against
tests/boundary_ref.py. Everything is integer, so every comparison is exact; output buffers carry sentinel tails that must come back unchanged. The
shapes are the smallest that reach each way of going wrong: every size up to 9 x 9 and maps smaller than d, half-widths on both sides of the
template's classes (16 | 17) and at the limit, 2 x 2 tiles and a ragged remainder with single pixels placed at distance d and d + 1 across every
kind of seam, every alignment of labels and truth, ragged sets of both kinds with clamped per-item half-widths, planning CU counts, graph replay,
every refusal, the net runner and the C host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boundary_ref as BR
import confusion_ref as CR
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

TAIL = 8
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)
FILL = 0xA5                                                     # depth buffers start as this byte: no depth reaches it (d + 1 <= 65)
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
HALF_WIDTHS = [1, 2, 3, 12, 16, 17, 64]


# ---------------------------------------------------------------------------------------------------------------------------- helpers

def _table(ctx, cells, preset=None):
    host = np.zeros(cells + TAIL, np.uint64)
    if preset is not None:
        host[:cells] = np.asarray(preset, np.uint64).ravel()
    host[cells:] = SENTINEL
    return ctx.to_device(host)


def _read_table(buf, cells):
    got = buf.download((cells + TAIL,), np.uint64)
    assert (got[cells:] == SENTINEL).all(), "written past the last cell"
    return got[:cells]


def _tables(ctx, classes, trimap=None, biou=None):
    return _table(ctx, (classes + 1) ** 2, trimap), _table(ctx, classes * 3, biou)


def _read_tables(d_tri, d_bio, classes):
    return _read_table(d_tri, (classes + 1) ** 2).reshape(classes + 1, classes + 1), _read_table(d_bio, classes * 3).reshape(classes, 3)


def _depth_maps(ctx, maps, d, edge):
    """mbn_boundary_depth over a batch of equal-sized 2-D maps (one call); the depth buffer carries a tail"""
    stack = np.ascontiguousarray(np.stack(maps))
    n, rows, cols = stack.shape
    d_map = ctx.to_device(stack)
    d_out = ctx.to_device(np.full(stack.size + 64, FILL, np.uint8))
    ctx.boundary_depth(d_out.ptr, d_map.ptr, stack.dtype.itemsize, n, rows, cols, d, edge)
    ctx.sync()
    got = d_out.download((stack.size + 64,), np.uint8)
    assert (got[stack.size:] == FILL).all(), "depth written past the last map"
    d_map.free()
    d_out.free()
    return got[:stack.size].reshape(n, rows, cols)


def _palette_map(rng, rows, cols, dtype):
    """few values, the special ones among them, so that small maps have contours and constant stretches"""
    if dtype == np.uint8:
        values = rng.choice(np.array([0, 1, 2, 254, 255], np.uint8), 3, replace=False)
    else:
        values = rng.choice(np.array([0, 1, 255, -1, I32_MAX, I32_MIN, 256, -256], np.int32), 3, replace=False)
    return values[rng.integers(0, 3, (rows, cols))].astype(dtype)


def _blocky(rng, rows, cols, classes, block=7):
    m = np.kron(rng.integers(0, classes, ((rows + block - 1) // block, (cols + block - 1) // block)), np.ones((block, block), np.int64))
    return np.ascontiguousarray(m[:rows, :cols]).astype(np.int32)


def _pair(rng, kind, rows, cols, classes, dtype):
    """(labels int32, truth dtype) of one map: truth with void pixels, labels with abstained ones"""
    top = min(classes, 256) if dtype == np.uint8 else classes
    if kind == "constant":
        return np.full((rows, cols), classes - 1, np.int32), np.full((rows, cols), top - 1, dtype)
    if kind == "random":
        truth = rng.integers(0, top, (rows, cols)).astype(dtype)
        labels = rng.integers(0, classes, (rows, cols)).astype(np.int32)
    else:
        truth = (_blocky(rng, rows, cols, top)).astype(dtype)
        labels = np.roll(_blocky(rng, rows, cols, classes), 2, axis=1)
        keep = rng.random((rows, cols)) < 0.7                    # most of the prediction agrees with the truth, shifted contours apart
        labels = np.where(keep & (truth.astype(np.int64) < classes), np.roll(truth.astype(np.int32), 1, axis=0), labels).astype(np.int32)
    truth[rng.random((rows, cols)) < 0.04] = 255 if dtype == np.uint8 else rng.choice(np.array([-1, 255, I32_MAX, I32_MIN, classes], np.int64))
    pick = rng.random((rows, cols)) < 0.04
    labels[pick] = rng.choice(np.array([-1, classes, I32_MAX, I32_MIN], np.int64), int(pick.sum())).astype(np.int32)
    return labels, truth


def _score(ctx, labels, truth, classes, d, edge, trimap=True, biou=True, preset=None, calls=1):
    """mbn_boundary_score_i32 on [batch][rows][cols] stacks, `calls` times into one pair of tables"""
    labels, truth = np.ascontiguousarray(labels), np.ascontiguousarray(truth)
    n, rows, cols = labels.shape
    d_lab, d_tr = ctx.to_device(labels), ctx.to_device(truth)
    d_tri, d_bio = _tables(ctx, classes, *(preset or (None, None)))
    for _ in range(calls):
        ctx.boundary_score(d_tri.ptr if trimap else None, d_bio.ptr if biou else None, d_lab.ptr, d_tr.ptr, truth.dtype.itemsize, classes, n, rows, cols,
                           d, edge)
    ctx.sync()
    got = _read_tables(d_tri, d_bio, classes)
    for b in (d_lab, d_tr, d_tri, d_bio):
        b.free()
    return got


def _want(labels, truth, classes, d, edge):
    return BR.score_maps(list(zip(labels, truth)), classes, d, edge)


# --------------------------------------------------------------------------------------------------------------- depth, small shapes

SMALL_SHAPES = [(r, c) for r in range(1, 10) for c in range(1, 10)] + [(1, 70), (70, 1), (2, 130), (130, 2), (5, 40), (40, 5)]


@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_depth_per_pixel_at_small_shapes(pkg, ctx, dtype, edge):
    """every rows x cols up to 9 x 9, single rows and columns past a tile's width and height, maps smaller than d in one or both directions; three
    maps a shape in one call"""
    rng = np.random.default_rng(10 + edge)
    for rows, cols in SMALL_SHAPES:
        maps = [_palette_map(rng, rows, cols, dtype) for _ in range(2)] + [np.full((rows, cols), 255 if dtype == np.uint8 else -1, dtype)]
        for d in HALF_WIDTHS:
            got = _depth_maps(ctx, maps, d, edge)
            for k, m in enumerate(maps):
                want = BR.depth(m, d, edge)
                assert np.array_equal(got[k], want), "%d x %d, d = %d, map %d:\n%s\nwant\n%s" % (rows, cols, d, k, got[k], want)


# ------------------------------------------------------------------------------------------------------------------------ tile seams

def _seam_maps(tr, tc, d, rows, cols):
    """constant maps of 7 with ONE pixel of 9: (name, map, probe, expected depth of the probe without the frame)"""
    out = []

    def one(name, probe, q):
        if not (0 <= q[0] < rows and 0 <= q[1] < cols):
            return
        m = np.full((rows, cols), 7, np.int32)
        m[q] = 9
        dist = max(abs(q[0] - probe[0]), abs(q[1] - probe[1]))
        out.append((name, m, probe, min(dist, d + 1)))

    for gap in (d, d + 1):                                      # exactly in the band, exactly out of it
        r, c = tr - 1, tc - 1                                   # the last pixel of tile (0, 0); every partner lies in another tile
        one("right, gap %d" % gap, (r - 3, c), (r - 3, c + gap))
        one("left, gap %d" % gap, (r - 3, tc), (r - 3, tc - gap))
        one("down, gap %d" % gap, (r, c - 3), (r + gap, c - 3))
        one("up, gap %d" % gap, (tr, c - 3), (tr - gap, c - 3))
        one("corner down-right, gap %d" % gap, (r, c), (r + gap, c + gap))
        one("corner up-left, gap %d" % gap, (tr, tc), (tr - gap, tc - gap))
        one("corner, the shorter leg inside, gap %d" % gap, (r, c), (r + 1, c + gap))
        one("beside the frame, gap %d" % gap, (rows - 1, tc - 1), (rows - 1, tc - 1 + gap))
        one("from the map's corner, gap %d" % gap, (gap, cols - 1 - gap), (0, cols - 1))
        one("two tiles away, gap %d" % gap, (2 * tr, 2 * tc), (2 * tr - gap, 2 * tc - gap))
    return out


@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("d", [3, 16, 17])
def test_tile_seams(pkg, ctx, d, edge):
    """2 x 2 tiles and a ragged remainder; the tile is the library's own answer for this d"""
    tr, tc, _ = pkg.boundary_tile(d)
    rows, cols = 2 * tr + 5, 2 * tc + 7
    cases = _seam_maps(tr, tc, d, rows, cols)
    assert len(cases) >= 16
    quadrants = np.zeros((rows, cols), np.int32)                # a contour exactly on both seams
    quadrants[tr:, :] += 1
    quadrants[:, tc:] += 2
    stripes = (np.arange(cols)[None, :] // tc + 3 * (np.arange(rows)[:, None] // tr)).astype(np.int32)      # ... and on every seam
    maps = [m for _, m, _, _ in cases] + [quadrants, np.ascontiguousarray(stripes)]
    got = _depth_maps(ctx, maps, d, edge)
    for k, (name, m, probe, dist) in enumerate(cases):
        if not edge:
            assert got[k][probe] == dist, "%s: the probe %s has depth %d, its distance is %d" % (name, probe, got[k][probe], dist)
        want = BR.depth(m, d, edge)
        assert np.array_equal(got[k], want), "%s: %d pixels differ" % (name, int((got[k] != want).sum()))
    for k, m in ((len(cases), quadrants), (len(cases) + 1, stripes)):
        want = BR.depth(m, d, edge)
        assert np.array_equal(got[k], want), "contours on the seams: %d pixels differ" % int((got[k] != want).sum())
        assert want[tr - 1, 5] == 1 and want[tr, 5] == 1 and want[5, tc - 1] == 1 and want[5, tc] == 1


def test_depth_at_the_largest_half_width_across_tiles(pkg, ctx):
    """d = 64: the halo is as wide as the tile; one map of 2 x 2 tiles and a remainder, blocks of 50"""
    rng = np.random.default_rng(12)
    m = _blocky(rng, 150, 139, 3, block=50)
    for edge in (0, 1):
        got = _depth_maps(ctx, [m], 64, edge)[0]
        want = BR.depth(m, 64, edge)
        assert np.array_equal(got, want), "edge %d: %d pixels differ" % (edge, int((got != want).sum()))


# ----------------------------------------------------------------------------------------------------------------------------- score

@pytest.mark.parametrize("classes", [1, 3, 21, 150, 151, 1000])
def test_score_against_the_reference(pkg, ctx, classes):
    rows, cols, n = 45, 77, 2                                   # 2 x 2 tiles of the small class, ragged on both sides
    dtype = np.uint8 if classes <= 256 else np.int32
    rng = np.random.default_rng(classes)
    for kind in ("blocky", "random", "constant"):
        pairs = [_pair(rng, kind, rows, cols, classes, dtype) for _ in range(n)]
        labels, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        for d, edge in ((3, 1), (3, 0), (17, 1)):
            tri, bio = _score(ctx, labels, truth, classes, d, edge)
            want_tri, want_bio = _want(labels, truth, classes, d, edge)
            band = sum(int((BR.depth(t, d, edge) <= d).sum()) for t in truth)
            assert int(tri.sum()) == band, "%s, d %d, edge %d: the trimap sums to %d, the truth band has %d pixels" % (kind, d, edge, int(tri.sum()), band)
            assert np.array_equal(tri, want_tri), "%s, d %d, edge %d: %d trimap cells differ" % (kind, d, edge, int((tri != want_tri).sum()))
            assert np.array_equal(bio, want_bio), "%s, d %d, edge %d: biou\n%s\nwant\n%s" % (kind, d, edge, bio[bio != want_bio], want_bio[bio != want_bio])
            if kind == "constant" and edge == 0:
                assert not tri.any() and not bio.any(), "a constant map has no band without the frame"
            if kind == "constant" and edge == 1:
                assert tri.any() and bio.any()


def test_int32_truth_and_either_table_null(pkg, ctx):
    classes, d = 5, 2
    rng = np.random.default_rng(20)
    pairs = [_pair(rng, "blocky", 33, 70, classes, np.int32) for _ in range(2)]
    labels, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want_tri, want_bio = _want(labels, truth, classes, d, 1)
    assert want_tri[classes].any() and want_tri[:, classes].any(), "void truth and abstained labels are in the band"
    tri, bio = _score(ctx, labels, truth, classes, d, 1)
    assert np.array_equal(tri, want_tri) and np.array_equal(bio, want_bio)
    tri, bio = _score(ctx, labels, truth, classes, d, 1, biou=False)
    assert np.array_equal(tri, want_tri) and not bio.any()
    tri, bio = _score(ctx, labels, truth, classes, d, 1, trimap=False)
    assert not tri.any() and np.array_equal(bio, want_bio)


def test_accumulation_into_preset_tables(pkg, ctx):
    classes, d = 3, 3
    rng = np.random.default_rng(21)
    pairs = [_pair(rng, "blocky", 40, 66, classes, np.uint8) for _ in range(2)]
    labels, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    one_tri, one_bio = _want(labels, truth, classes, d, 1)
    tri, bio = _score(ctx, labels, truth, classes, d, 1, calls=2)
    assert np.array_equal(tri, 2 * one_tri) and np.array_equal(bio, 2 * one_bio), "two calls add"
    pre_tri = np.where(one_tri > 0, np.uint64(0xFFFFFFF0), np.uint64(7)).astype(np.uint64)
    pre_bio = np.where(one_bio > 0, np.uint64(0xFFFFFFF0), np.uint64(5)).astype(np.uint64)
    tri, bio = _score(ctx, labels, truth, classes, d, 1, preset=(pre_tri, pre_bio))
    assert np.array_equal(tri, pre_tri + one_tri) and np.array_equal(bio, pre_bio + one_bio)
    assert (one_tri >= 16).any() and (tri[one_tri >= 16] >= np.uint64(1 << 32)).all(), "the adds carry into the high word"


# ----------------------------------------------------------------------------------------------------------------- interior pointers

def test_interior_pointers_at_every_alignment(pkg, ctx):
    """labels at element offsets 0..3 of a 16-byte boundary x uint8 truth at byte offsets 0..3, the depth of a uint8 map at byte offsets 0..3 into
    an output at another offset: in-range data lies on both sides and must reach no band"""
    classes, d, rows, cols = 3, 2, 9, 13
    rng = np.random.default_rng(30)
    count = rows * cols
    lab = rng.integers(0, classes, count + 16).astype(np.int32)
    tr = rng.integers(0, classes, count + 16).astype(np.uint8)
    cases = [(lo, to) for lo in range(4) for to in range(4)]
    d_lab, d_tr = ctx.to_device(lab), ctx.to_device(tr)
    assert d_lab.ptr % 16 == 0 and d_tr.ptr % 16 == 0
    tris, bios = [], []
    for lo, to in cases:
        d_tri, d_bio = _tables(ctx, classes)
        ctx.boundary_score(d_tri.ptr, d_bio.ptr, d_lab.ptr + 4 * lo, d_tr.ptr + to, 1, classes, 1, rows, cols, d, 0)
        tris.append(d_tri)
        bios.append(d_bio)
    d_out = ctx.to_device(np.full(4 * (count + 16), FILL, np.uint8))
    for to in range(4):
        ctx.boundary_depth(d_out.ptr + to * (count + 16) + (3 - to), d_tr.ptr + to, 1, 1, rows, cols, d, 0)
    ctx.sync()
    for k, (lo, to) in enumerate(cases):
        got = _read_tables(tris[k], bios[k], classes)
        want = BR.score(lab[lo:lo + count].reshape(rows, cols), tr[to:to + count].reshape(rows, cols), classes, d, 0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "labels +%d, truth +%d" % (lo, to)
    out = d_out.download((4 * (count + 16),), np.uint8)
    for to in range(4):
        seg = out[to * (count + 16):(to + 1) * (count + 16)]
        at = 3 - to
        assert np.array_equal(seg[at:at + count].reshape(rows, cols), BR.depth(tr[to:to + count].reshape(rows, cols), d, 0)), "map +%d" % to
        assert (seg[:at] == FILL).all() and (seg[at + count:] == FILL).all(), "depth written outside its map"
    for b in [d_lab, d_tr, d_out] + tris + bios:
        b.free()


# ---------------------------------------------------------------------------------------------------------------------------- ragged

PLAIN_ITEMS = [(900, 37, 61), (0, 5, 7), (40, 4, 200), (3200, 70, 133), (12600, 4, 4)]            # any order, gaps between the maps
WINDOW_ITEMS = [(17, 1, 1, (3, 5, 1, 1)), (30, 1, 300, (0, 7, 64, 1)), (400, 37, 61, (0, 0, 64, 64)), (5000, 9, 1, (9, 0, 1, 64))]


@pytest.mark.parametrize("per_item", [False, True])
@pytest.mark.parametrize("kind", ["plain", "window"])
def test_ragged(pkg, ctx, kind, per_item):
    classes, d, edge = 5, 3, 1
    r = pkg.RaggedReadout(ctx, 8)
    if kind == "plain":
        items = PLAIN_ITEMS
        r.set(1, 1, 5, items)
    else:
        items = [it[:3] for it in WINDOW_ITEMS]
        r.set_window(1, 1, 5, 64, 64, WINDOW_ITEMS)
    ds = ([0, 1000, 2, 17, 5][:len(items)] if per_item else [d] * len(items))        # 0 and 1000: the kernel clamps into [1, 64]
    eff = [min(max(v, 1), pkg.BOUNDARY_MAX_D) for v in ds]
    span = max(off + rows * cols for off, rows, cols in items)
    rng = np.random.default_rng(len(items) + per_item)
    lab = rng.integers(0, classes, span + 5).astype(np.int32)   # the gaps hold in-range garbage
    tr = rng.integers(0, classes, span + 5).astype(np.uint8)
    for off, rows, cols in items:                               # blocky maps, so that larger half-widths have something to tell apart
        pl, pt = _pair(rng, "blocky", rows, cols, classes, np.uint8)
        lab[off:off + rows * cols], tr[off:off + rows * cols] = pl.ravel(), pt.ravel()
    d_lab, d_tr = ctx.to_device(lab), ctx.to_device(tr)
    d_items = ctx.to_device(np.array(ds, np.int32)) if per_item else None
    d_ptr = d_items.ptr if per_item else None
    d_tri, d_bio = _tables(ctx, classes)
    d_out = ctx.to_device(np.full(span + 5, FILL, np.uint8))
    d_out8 = ctx.to_device(np.full(span + 5, FILL, np.uint8))
    ctx.boundary_score_ragged(r, d_tri.ptr, d_bio.ptr, d_lab.ptr, d_tr.ptr, 1, classes, 9 if per_item else d, d_ptr, edge)     # d is ignored with d_items
    ctx.boundary_depth_ragged(r, d_out.ptr, d_lab.ptr, 4, d, d_ptr, edge)
    ctx.boundary_depth_ragged(r, d_out8.ptr, d_tr.ptr, 1, d, d_ptr, edge)
    ctx.sync()
    maps = [(lab[off:off + rows * cols].reshape(rows, cols), tr[off:off + rows * cols].reshape(rows, cols), eff[i])
            for i, (off, rows, cols) in enumerate(items)]
    want_tri, want_bio = BR.score_maps(maps, classes, d, edge)
    tri, bio = _read_tables(d_tri, d_bio, classes)
    assert np.array_equal(tri, want_tri) and np.array_equal(bio, want_bio)
    for buf, which in ((d_out, 0), (d_out8, 1)):
        got = buf.download((span + 5,), np.uint8)
        inside = np.zeros(span + 5, bool)
        for i, (off, rows, cols) in enumerate(items):
            inside[off:off + rows * cols] = True
            want = BR.depth(maps[i][which], eff[i], edge)
            assert np.array_equal(got[off:off + rows * cols].reshape(rows, cols), want), "item %d, d %d" % (i, eff[i])
        assert (got[~inside] == FILL).all(), "the gaps between the maps were written"
    if per_item:
        got = ctx.boundary_d_items(r, 0.02)
        assert list(got[:len(items)]) == [BR.half_width(rows, cols, 0.02) for _, rows, cols in items]
    # a captured launch belongs to its set: replayed after a later set it adds nothing
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_boundary_score_ragged_i32(r.h, d_tri.ptr, d_bio.ptr, d_lab.ptr, d_tr.ptr, 1, classes, d, d_ptr, edge, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(_read_tables(d_tri, d_bio, classes)[0], 2 * want_tri), "a replay under its own set adds"
    r.set(1, 1, 5, [(0, 4, 4)])
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    tri, bio = _read_tables(d_tri, d_bio, classes)
    assert np.array_equal(tri, 2 * want_tri) and np.array_equal(bio, 2 * want_bio), "a replay after a later set adds nothing"
    ctx.boundary_score_ragged(r, d_tri.ptr, d_bio.ptr, d_lab.ptr, d_tr.ptr, 1, classes, d, None, edge)      # the new set is what a new launch scores
    ctx.sync()
    new_tri, new_bio = BR.score(lab[:16].reshape(4, 4), tr[:16].reshape(4, 4), classes, d, edge)
    tri, bio = _read_tables(d_tri, d_bio, classes)
    assert np.array_equal(tri, 2 * want_tri + new_tri) and np.array_equal(bio, 2 * want_bio + new_bio)
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    for b in [d_lab, d_tr, d_tri, d_bio, d_out, d_out8] + ([d_items] if per_item else []):
        b.free()


# ------------------------------------------------------------------------------------------------------- planning CUs, graph replay

@pytest.mark.parametrize("classes", [21, 150])
def test_planning_cus_give_the_same_bytes(pkg, ctx, classes):
    """both counting forms: a workgroup's LDS bins (21 classes) and global atomics only (150)"""
    rows, cols, n = 100, 150, 3
    rng = np.random.default_rng(40)
    pairs = [_pair(rng, "blocky", rows, cols, classes, np.uint8) for _ in range(n)]
    labels, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    try:
        for d in (12, 20):
            want = _want(labels, truth, classes, d, 1)
            want_depth = np.stack([BR.depth(m, d, 1) for m in labels])
            for cus in (1, 2, 7, 0):
                assert ctx.lib.mbn_set_planning_cus(ctx.h, cus) == pkg.OK
                tri, bio = _score(ctx, labels, truth, classes, d, 1)
                assert np.array_equal(tri, want[0]) and np.array_equal(bio, want[1]), "d %d at %d planning CUs" % (d, cus)
                assert np.array_equal(_depth_maps(ctx, list(labels), d, 1), want_depth), "depth, d %d at %d planning CUs" % (d, cus)
    finally:
        assert ctx.lib.mbn_set_planning_cus(ctx.h, 0) == pkg.OK


def test_graph_capture_and_replay(pkg, ctx):
    classes, d, rows, cols = 21, 4, 70, 90
    rng = np.random.default_rng(41)
    labels, truth = _pair(rng, "blocky", rows, cols, classes, np.uint8)
    d_lab, d_tr = ctx.to_device(labels), ctx.to_device(truth)
    d_tri, d_bio = _tables(ctx, classes)
    d_out = ctx.to_device(np.full(rows * cols + 8, FILL, np.uint8))
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_boundary_score_i32(ctx.h, d_tri.ptr, d_bio.ptr, d_lab.ptr, d_tr.ptr, 1, classes, 1, rows, cols, d, 1, None)
    rc2 = ctx.lib.mbn_boundary_depth(ctx.h, d_out.ptr, d_lab.ptr, 4, 1, rows, cols, d, 1, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK and rc2 == pkg.OK
    ctx.sync()
    tri, bio = _read_tables(d_tri, d_bio, classes)
    assert not tri.any() and not bio.any() and (d_out.download((rows * cols + 8,), np.uint8) == FILL).all(), "the captured calls ran"
    want_tri, want_bio = BR.score(labels, truth, classes, d, 1)
    for k in (1, 2):
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        ctx.sync()
        tri, bio = _read_tables(d_tri, d_bio, classes)
        assert np.array_equal(tri, k * want_tri) and np.array_equal(bio, k * want_bio), "replay %d" % k
    got = d_out.download((rows * cols + 8,), np.uint8)
    assert np.array_equal(got[:rows * cols].reshape(rows, cols), BR.depth(labels, d, 1)) and (got[rows * cols:] == FILL).all()
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    for b in (d_lab, d_tr, d_tri, d_bio, d_out):
        b.free()


# ------------------------------------------------------------------------------------------------------------------ argument errors

def test_argument_errors(pkg, ctx):
    classes, rows, cols = 3, 10, 10
    count = rows * cols
    lab, tr = ctx.to_device(np.zeros(count, np.int32)), ctx.to_device(np.zeros(count, np.int32))
    d_tri, d_bio = _tables(ctx, classes)
    out = ctx.to_device(np.full(count, FILL, np.uint8))
    small = ctx.to_device(np.full(8, SENTINEL, np.uint64))       # one cell short of 3 x 3 biou cells, eight short of the trimap
    lib = ctx.lib
    EI, EU = pkg.EINVAL, pkg.EUNSUPPORTED

    def score(tri, bio, l, t, tb=1, c=classes, n=1, r=rows, w=cols, d=2, e=1):
        return lib.mbn_boundary_score_i32(ctx.h, tri, bio, l, t, tb, c, n, r, w, d, e, None)

    def depth(o, m, eb=4, n=1, r=rows, w=cols, d=2, e=1):
        return lib.mbn_boundary_depth(ctx.h, o, m, eb, n, r, w, d, e, None)

    assert score(None, None, lab.ptr, tr.ptr) == EI and score(d_tri.ptr, d_bio.ptr, None, tr.ptr) == EI and score(d_tri.ptr, d_bio.ptr, lab.ptr, None) == EI
    assert lib.mbn_boundary_score_i32(None, d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr, 1, classes, 1, rows, cols, 2, 1, None) == EI
    assert score(d_tri.ptr + 4, d_bio.ptr, lab.ptr, tr.ptr) == EI and score(d_tri.ptr, d_bio.ptr + 4, lab.ptr, tr.ptr) == EI      # tables off 8 bytes
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr + 2, tr.ptr, r=5) == EI                                                          # labels off 4
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr + 2, tb=4, r=5) == EI                                                    # an int32 truth off 4
    for kw in ({"c": 0}, {"c": -1}, {"n": 0}, {"r": 0}, {"w": -2}, {"d": 0}, {"d": -5}, {"e": 2}, {"e": -1}, {"tb": 2}, {"tb": 0}, {"tb": 8}):
        assert score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr, **kw) == EI, kw
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr, d=pkg.BOUNDARY_MAX_D + 1) == EU
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr, c=pkg.CONFUSION_MAX_CLASSES + 1) == EU
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr, r=16384, w=32768) == EU and score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr, n=65536) == EU
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr, d=pkg.BOUNDARY_MAX_D + 1, e=3) == EI, "a caller error goes before a limit"
    assert score(small.ptr, None, lab.ptr, tr.ptr) == EI and "boundary trimap" in ctx.last_error()
    assert score(None, small.ptr, lab.ptr, tr.ptr) == EI and "boundary biou" in ctx.last_error()
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr, n=2) == EI and "boundary labels" in ctx.last_error()
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr, tr.ptr + 4 * count - 50, tb=1) == EI and "boundary truth" in ctx.last_error()
    assert score(d_tri.ptr, d_bio.ptr, lab.ptr + 4, tr.ptr, tb=4) == EI                # an interior pointer: one element short
    assert depth(None, lab.ptr) == EI and depth(out.ptr, None) == EI and lib.mbn_boundary_depth(None, out.ptr, lab.ptr, 4, 1, rows, cols, 2, 1, None) == EI
    assert depth(out.ptr, lab.ptr + 2, r=5) == EI and depth(out.ptr, lab.ptr, eb=2) == EI and depth(out.ptr, lab.ptr, d=0) == EI and depth(out.ptr, lab.ptr, e=2) == EI
    assert depth(out.ptr, lab.ptr, d=65) == EU and depth(out.ptr, lab.ptr, n=65536) == EU
    assert depth(out.ptr, lab.ptr, n=2) == EI and "boundary" in ctx.last_error()
    assert depth(lab.ptr, lab.ptr) == EI and depth(lab.ptr + 4 * count - 1, lab.ptr) == EI and depth(lab.ptr + 50, lab.ptr + 60, eb=1) == EI, "depth over map"
    r = pkg.RaggedReadout(ctx, 4)
    d_items = ctx.to_device(np.array([2, 2], np.int32))

    def rscore(h, tri, l, t, tb=1, c=classes, d=2, di=None, e=1):
        return lib.mbn_boundary_score_ragged_i32(h, tri, d_bio.ptr, l, t, tb, c, d, di, e, None)

    assert rscore(r.h, d_tri.ptr, lab.ptr, tr.ptr) == EI and rscore(None, d_tri.ptr, lab.ptr, tr.ptr) == EI                   # no set, no handle
    assert lib.mbn_boundary_depth_ragged(r.h, out.ptr, lab.ptr, 4, 2, None, 1, None) == EI
    assert lib.mbn_boundary_d_items(r.h, 0.02, (C.c_int32 * 4)()) == EI
    r.set(1, 1, 5, [(2, 4, 5), (60, 5, 8)])
    assert rscore(r.h, d_tri.ptr, lab.ptr, tr.ptr, tb=2) == EI and rscore(r.h, d_tri.ptr, None, tr.ptr) == EI and rscore(r.h, d_tri.ptr, lab.ptr, tr.ptr, d=0) == EI
    assert rscore(r.h, d_tri.ptr, lab.ptr, tr.ptr, d=0, di=d_items.ptr) == pkg.OK, "d is not read with per-item half-widths"
    assert rscore(r.h, d_tri.ptr, lab.ptr, tr.ptr, di=d_items.ptr + 2) == EI                                                  # d_items off 4
    assert rscore(r.h, d_tri.ptr, lab.ptr, tr.ptr, di=d_items.ptr + 4) == EI and "boundary d_items" in ctx.last_error()       # one entry short
    assert rscore(r.h, d_tri.ptr, lab.ptr, tr.ptr, d=65) == EU and rscore(r.h, d_tri.ptr, lab.ptr, tr.ptr, c=4097) == EU
    assert rscore(r.h, d_tri.ptr, lab.ptr + 4, tr.ptr) == EI                                                                  # the set reaches element 100
    assert lib.mbn_boundary_depth_ragged(r.h, out.ptr + 1, lab.ptr, 4, 2, None, 1, None) == EI
    assert lib.mbn_boundary_depth_ragged(r.h, out.ptr, lab.ptr, 3, 2, None, 1, None) == EI
    assert lib.mbn_boundary_d_items(r.h, 0.0, (C.c_int32 * 4)()) == EI and lib.mbn_boundary_d_items(r.h, 0.02, None) == EI
    ctx.sync()
    tri, bio = _read_tables(d_tri, d_bio, classes)
    assert int(tri.sum()) == 56 and tri[0, 0] == 56, "only the one accepted call may have been launched (4 x 5 and 5 x 8: all but 4 pixels within 2 of the frame)"
    assert (out.download((count,), np.uint8) == FILL).all() and (small.download((8,), np.uint64) == SENTINEL).all()
    r.close()
    for b in (lab, tr, d_tri, d_bio, out, small, d_items):
        b.free()


# --------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS = 0.5, 21, 64, 96


def test_net_segment_boundary(pkg, ctx, tmp_path):
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, 16)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 8)
    net.set_input_u8(True)
    rng = np.random.default_rng(50)
    n, sh, sw = 2, 75, 130
    src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    npix = n * sh * sw
    truth = _blocky(rng, 1, npix + 64, CLASSES, block=1).astype(np.uint8).ravel()
    truth[:npix] = np.stack([_pair(rng, "blocky", sh, sw, CLASSES, np.uint8)[1] for _ in range(n)]).ravel()
    d_src, d_lab, d_tr = ctx.to_device(src), ctx.alloc(4 * (npix + 64)), ctx.to_device(truth)
    d_tri, d_bio = _tables(ctx, CLASSES)
    d_depth = ctx.to_device(np.full(npix + 64, FILL, np.uint8))
    assert ctx.lib.mbn_net_segment_boundary_score(net.h, d_lab.ptr, d_tr.ptr, 1, d_tri.ptr, d_bio.ptr, 0.02, 0, 1) == pkg.EINVAL, "before any segment call"
    assert ctx.lib.mbn_net_segment_boundary_depth(net.h, d_lab.ptr, d_depth.ptr, 0.02, 0, 1) == pkg.EINVAL
    total = [np.zeros((CLASSES + 1, CLASSES + 1), np.uint64), np.zeros((CLASSES, 3), np.uint64)]

    def check(what, ratio, d, edge, items=None):
        net.segment_boundary_score(d_lab.ptr, d_tr.ptr, 1, d_tri.ptr, d_bio.ptr, ratio=ratio, d=d, edge=edge)
        ctx.lib.mbn_memset(ctx.h, d_depth.ptr, FILL, npix + 64)
        net.segment_boundary_depth(d_lab.ptr, d_depth.ptr, ratio=ratio, d=d, edge=edge)
        ctx.sync()
        lab = d_lab.download((npix + 64,), np.int32)
        if items is None:
            items = [(i * sh * sw, sh, sw) for i in range(n)]
        maps = [(lab[off:off + r * c].reshape(r, c), truth[off:off + r * c].reshape(r, c), d if d > 0 else BR.half_width(r, c, ratio))
                for off, r, c in items]
        add = BR.score_maps(maps, CLASSES, 0, edge)
        total[0], total[1] = total[0] + add[0], total[1] + add[1]
        tri, bio = _read_tables(d_tri, d_bio, CLASSES)
        assert np.array_equal(tri, total[0]) and np.array_equal(bio, total[1]), what
        got = d_depth.download((npix + 64,), np.uint8)
        inside = np.zeros(npix + 64, bool)
        for (off, r, c), m in zip(items, maps):
            inside[off:off + r * c] = True
            assert np.array_equal(got[off:off + r * c].reshape(r, c), BR.depth(m[0], m[2], edge)), what
        assert (got[~inside] == FILL).all(), what
        return maps

    img = net.resize_input(d_src.ptr, n, sh, sw, pkg.FIT_STRETCH)
    net.segment_to(img, n, sh, sw, d_lab.ptr)
    maps = check("segment_to, ratio", 0.02, 0, 1)
    assert maps[0][2] == 3 and len(np.unique(maps[0][0])) > 1, "75 x 130 at 0.02: d = 3"
    check("segment_to, fixed d", 0.02, 5, 0)
    net.segment_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr)
    check("segment_fit, ratio", 0.05, 0, 1)
    check("segment_fit, fixed d", 0.5, 17, 1)
    rows, cols = [sh, 40], [sw, 50]
    offs, dst = [0, sh * sw * 3], [sh * sw + 11, 3]
    ctx.lib.mbn_memset(ctx.h, d_lab.ptr, 0xFF, 4 * (npix + 64))
    net.segment_images_fit(d_src.ptr, offs, rows, cols, pkg.FIT_PAD, d_lab.ptr, dst)
    items = [(dst[i], rows[i], cols[i]) for i in range(2)]
    maps = check("image call, ratio: each image its own half-width", 0.03, 0, 1, items=items)
    assert [m[2] for m in maps] == [5, 2], "150.08 * 0.03 and 64.03 * 0.03"
    check("image call, fixed d", 0.03, 4, 0, items=items)
    assert ctx.lib.mbn_net_segment_boundary_score(net.h, d_lab.ptr, d_tr.ptr, 1, d_tri.ptr, d_bio.ptr, 0.02, -1, 1) == pkg.EINVAL
    assert ctx.lib.mbn_net_segment_boundary_score(net.h, d_lab.ptr, d_tr.ptr, 1, d_tri.ptr, d_bio.ptr, 0.0, 0, 1) == pkg.EINVAL
    assert ctx.lib.mbn_net_segment_boundary_score(net.h, d_lab.ptr, d_tr.ptr, 1, d_tri.ptr, d_bio.ptr, 1.0, 0, 1) == pkg.EUNSUPPORTED
    ctx.sync()
    tri, bio = _read_tables(d_tri, d_bio, CLASSES)
    assert np.array_equal(tri, total[0]) and np.array_equal(bio, total[1]), "a refused call adds nothing"
    m, iou = pkg.boundary_metrics(total[1], CLASSES)
    want = BR.metrics(total[1], CLASSES)
    assert np.array_equal(iou, want["iou"], equal_nan=True) and m.classes_present == want["classes_present"] > 0
    net.destroy()
    for b in (d_src, d_lab, d_tr, d_tri, d_bio, d_depth):
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def _pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    w, h, maxval = (int(g) for g in m.groups())
    return np.frombuffer(raw[m.end():], ">u2" if maxval > 255 else np.uint8).astype(np.int32).reshape(h, w)


def _fields(out, key):
    m = re.search(r"^%s: (.*)$" % key, out, re.M)
    assert m, out
    return {k: float(v) for k, v in (f.split("=") for f in m.group(1).split())}


def test_c_host_boundary(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    sh, sw, classes = 75, 130, 1000                             # the host's synthetic weights have 1000 classes
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, plain, tta, band = str(tmp_path / "a.ppm"), str(tmp_path / "plain.pgm"), str(tmp_path / "tta.pgm"), str(tmp_path / "band.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", "3", "--alpha", "0.5", "--res", "%dx%d" % (ROWS, COLS), "--output-stride", "16", "--ppm", ppm, "--fit", "pad"]
    r = subprocess.run(common + ["--segment-source", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "boundary:" not in r.stdout, r.stdout + r.stderr
    r = subprocess.run(common + ["--segment-source", tta, "--tta-scales", "1,0.5", "--tta-flip", "--truth", plain, "--boundary-ratio", "0.02",
                                 "--boundary-map", band], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "score: pixels=" in r.stdout, r.stdout + r.stderr
    labels, truth = _pgm(tta), _pgm(plain)
    d = BR.half_width(sh, sw, 0.02)
    assert d == 3
    tri, bio = BR.score(labels, truth, classes, d, 1)
    want = BR.metrics(bio, classes)
    b = _fields(r.stdout, "boundary")
    assert (b["d"], b["edge"], b["classes_present"], b["truth_band"], b["pred_band"]) == (d, 1, want["classes_present"], want["truth_band_pixels"],
                                                                                         want["pred_band_pixels"])
    assert abs(b["boundary_miou"] - want["boundary_miou"]) <= classes * 2.0 ** -52 * abs(want["boundary_miou"]) and want["classes_present"] > 0
    per_class = {int(c): float(v) for c, v in re.findall(r"^boundary_iou: class (\d+) (\S+)$", r.stdout, re.M)}
    present = ~np.isnan(want["iou"])
    assert sorted(per_class) == list(np.flatnonzero(present)) and all(per_class[c] == want["iou"][c] for c in per_class)
    t = _fields(r.stdout, "trimap")
    tm = CR.metrics(tri, classes)
    for key, field in (("pixels", "pixels"), ("valid", "valid"), ("void", "void_pixels"), ("abstained", "abstained"),
                       ("classes_present", "classes_present"), ("pixel_acc", "pixel_accuracy")):
        assert t[key] == tm[field], (key, t[key], tm[field])
    assert abs(t["miou"] - tm["miou"]) <= classes * 2.0 ** -52 * abs(tm["miou"])
    assert t["pixels"] == int((BR.depth(truth, d, 1) <= d).sum())
    assert np.array_equal(_pgm(band), BR.depth(labels, d, 1)), "--boundary-map is the depth of the label map"
    # a fixed half-width without the frame; the map alone needs no truth
    r = subprocess.run(common + ["--segment-source", tta, "--boundary-d", "5", "--boundary-edge", "0", "--boundary-map", band], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "trimap:" not in r.stdout, r.stdout + r.stderr
    assert np.array_equal(_pgm(band), BR.depth(_pgm(tta), 5, 0))
    # both half-widths, neither, no --segment-source, a bad value
    for extra in (["--segment-source", tta, "--truth", plain, "--boundary-ratio", "0.02", "--boundary-d", "3"],
                  ["--segment-source", tta, "--truth", plain, "--boundary-edge", "0"],
                  ["--boundary-ratio", "0.02"],
                  ["--segment-source", tta, "--boundary-ratio", "0.02"],
                  ["--segment-source", tta, "--truth", plain, "--boundary-d", "65"],
                  ["--segment-source", tta, "--truth", plain, "--boundary-ratio", "1.5"]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "boundary:" not in r.stdout, (extra, r.stdout + r.stderr)
