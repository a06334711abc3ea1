"""Score a segmentation by surface distance on the GPU: mbn_surface_score_i32 and its ragged form against tests/surface_ref.py. Everything is
integer, so every comparison is exact; the tables carry sentinel tails, and dist2 a fill that must come back unchanged outside the maps. The shapes are
the smallest that reach each way of going wrong: every size up to 6 x 6 and single rows and columns past a wave's and a unit's pixels, one far pair
across the whole map, pairs at t and t^2 + 1 across every seam of the work units, every class and bin count at which the table changes shape,
every alignment, ragged sets of both kinds, planning CU counts, graph replay, every refusal, the net runner and the C host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import surface_ref as SR
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

TAIL = 8
SENTINEL = np.uint64(0xDEADBEEFCAFEF00D)
FILL = np.uint32(0xA5A5A5A5)                                    # dist2 buffers start as this: no result is it (d2 < 2^31, the two marks are above)
I32_MAX, I32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
H = SR.HEAD


# ---------------------------------------------------------------------------------------------------------------------------- helpers

def _cells(classes, bins):
    return classes * 2 * (H + bins)


def _table(ctx, cells, preset=None):
    host = np.zeros(cells + TAIL, np.uint64)
    if preset is not None:
        host[:cells] = np.asarray(preset, np.uint64).ravel()
    host[cells:] = SENTINEL
    return ctx.to_device(host)


def _read_table(buf, classes, bins):
    cells = _cells(classes, bins)
    got = buf.download((cells + TAIL,), np.uint64)
    assert (got[cells:] == SENTINEL).all(), "written past the last cell"
    return got[:cells].reshape(classes, 2, H + bins)


def _palette_map(rng, rows, cols, dtype):
    """few values, the special ones among them, so that small maps have contours and constant stretches"""
    if dtype == np.uint8:
        values = np.append(rng.choice(np.array([1, 2, 254, 255], np.uint8), 2, replace=False), np.uint8(0))
    else:
        values = np.append(rng.choice(np.array([1, 255, -1, I32_MAX, I32_MIN, 256, -256], np.int32), 2, replace=False), np.int32(0))
    return values[rng.integers(0, 3, (rows, cols))].astype(dtype)


def _blocky(rng, rows, cols, classes, block=7):
    m = np.kron(rng.integers(0, classes, ((rows + block - 1) // block, (cols + block - 1) // block)), np.ones((block, block), np.int64))
    return np.ascontiguousarray(m[:rows, :cols]).astype(np.int32)


def _pair(rng, kind, rows, cols, classes, dtype):
    """(labels int32, truth dtype) of one map: truth with void pixels, labels with abstained ones (the boundary test's pairs)"""
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


def _score(pkg, ctx, labels, truth, classes, bins, edge, dist2=True, preset=None, calls=1):
    """mbn_surface_score_i32 on [batch][rows][cols] stacks, `calls` times into one table: (table, dist2 [batch][rows][cols] or None)"""
    labels, truth = np.ascontiguousarray(labels), np.ascontiguousarray(truth)
    n, rows, cols = labels.shape
    h = pkg.Surface(ctx, n, labels.size, classes)
    d_lab, d_tr = ctx.to_device(labels), ctx.to_device(truth)
    d_surf = _table(ctx, _cells(classes, bins), preset)
    d_d2 = ctx.to_device(np.full(labels.size + 16, FILL, np.uint32))
    for _ in range(calls):
        ctx.surface_score(h, d_surf.ptr, d_lab.ptr, d_tr.ptr, truth.dtype.itemsize, classes, bins, n, rows, cols, edge, dist2=d_d2.ptr if dist2 else None)
    ctx.sync()
    got = _read_table(d_surf, classes, bins)
    d2 = d_d2.download((labels.size + 16,), np.uint32)
    assert (d2[labels.size:] == FILL).all(), "dist2 written past the last map"
    if not dist2:
        assert (d2 == FILL).all(), "dist2 written without being given"
    h.close()
    for b in (d_lab, d_tr, d_surf, d_d2):
        b.free()
    return got, (d2[:labels.size].reshape(n, rows, cols) if dist2 else None)


def _check(pkg, ctx, labels, truth, classes, bins, edge, what):
    got, d2 = _score(pkg, ctx, labels, truth, classes, bins, edge)
    want = SR.score_maps(list(zip(labels, truth)), classes, bins, edge)
    assert np.array_equal(got, want), "%s: %d cells differ\n%s\nwant\n%s" % (what, int((got != want).sum()), got[got != want][:16], want[got != want][:16])
    for k in range(len(labels)):
        wd = SR.dist2_map(labels[k], truth[k], classes, edge)
        assert np.array_equal(d2[k], wd), "%s, map %d: %d dist2 pixels differ" % (what, k, int((d2[k] != wd).sum()))
    return want


# ---------------------------------------------------------------------------------------------------------------------- small shapes

SMALL_SHAPES = [(r, c) for r in range(1, 7) for c in range(1, 7)] + [(1, 70), (70, 1), (2, 130), (130, 2)]


@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_small_shapes(pkg, ctx, dtype, edge):
    """every rows x cols up to 6 x 6, single rows and columns past a wave's 64 pixels, two rows and columns past a unit's 256; three map pairs a
    shape in one call: two of few values (0 and the special ones among them), one constant"""
    rng = np.random.default_rng(10 + edge)
    classes = 3
    for rows, cols in SMALL_SHAPES:
        labels = np.stack([_palette_map(rng, rows, cols, np.int32) for _ in range(2)] + [np.full((rows, cols), 1, np.int32)])
        truth = np.stack([_palette_map(rng, rows, cols, dtype) for _ in range(2)] + [np.full((rows, cols), 1, dtype)])
        _check(pkg, ctx, labels, truth, classes, 6, edge, "%d x %d" % (rows, cols))


# ------------------------------------------------------------------------------------------------------------ far and near distances

def test_opposite_corners(pkg, ctx):
    """a 70 x 130 map of class 0 with ONE pixel of class 1: at (0, 0) in the labels, at (69, 129) in the truth. d2 = 69^2 + 129^2 = 21402: the search
    runs over every ring of the map; max_d2 is that value and the query lands in the overflow bin"""
    rows, cols, bins = 70, 130, 64
    labels, truth = np.zeros((1, rows, cols), np.int32), np.zeros((1, rows, cols), np.uint8)
    labels[0, 0, 0], truth[0, rows - 1, cols - 1] = 1, 1
    for edge in (0, 1):
        want = _check(pkg, ctx, labels, truth, 2, bins, edge, "corners, edge %d" % edge)
        for k in range(2):
            assert list(want[1, k, :3]) == [1, 0, 69 * 69 + 129 * 129] and want[1, k, H + bins - 1] == 1


def _seam_pairs(rows, cols, unit, wave):
    """(name, query (r, c), match (r, c)): one pixel of class 1 a map, the query on one side of a seam of the flat pixel order and its match on the
    other, at a gap t (d2 = t^2) and one row off (d2 = t^2 + 1)"""
    out = []
    for seam in (wave, unit - wave, unit, unit + wave, 2 * unit, 2 * unit + wave):
        for t in (1, 3, 5):
            for a, b in ((seam - 1, seam - 1 + t), (seam, seam - t)):      # the last pixel before the seam, the first behind it
                q, g = divmod(a, cols), divmod(b, cols)
                if q[0] != g[0] or not (0 <= a < rows * cols and 0 <= b < rows * cols):
                    continue                                                # the pair must lie in one row for d2 = t^2
                out.append(("seam %d, gap %d" % (seam, t), q, g))
                if g[0] + 1 < rows:
                    out.append(("seam %d, gap %d, one row down" % (seam, t), q, (g[0] + 1, g[1])))
                if g[0] >= 1:
                    out.append(("seam %d, gap %d, one row up" % (seam, t), q, (g[0] - 1, g[1])))
    return out


def test_gaps_across_the_unit_seams(pkg, ctx):
    """a map of 2 units and a remainder in the kernel's flat pixel order (the library's own answer for the unit): pairs at d2 = t^2 and t^2 + 1 with
    the query on either side of every seam between waves and between units, and at the map's corner"""
    unit, wave = pkg.surface_tile()
    cols = 73                                                    # no divisor of the seams: they fall inside rows, at differing columns
    rows = (2 * unit + unit // 2) // cols + 1
    cases = _seam_pairs(rows, cols, unit, wave)
    cases += [("the map's corner, gap 4", (rows - 1, cols - 1), (rows - 1, cols - 5)), ("the map's corner, 4^2 + 1", (rows - 1, cols - 1), (rows - 2, cols - 5))]
    assert len(cases) >= 40
    labels, truth = np.zeros((len(cases), rows, cols), np.int32), np.zeros((len(cases), rows, cols), np.uint8)
    for k, (_, q, g) in enumerate(cases):
        labels[k][q], truth[k][g] = 1, 1
    bins = 8
    got, d2 = _score(pkg, ctx, labels, truth, 2, bins, 0)
    for k, (name, q, g) in enumerate(cases):
        want = (q[0] - g[0]) ** 2 + (q[1] - g[1]) ** 2
        assert d2[k][q] == want, "%s: the query %s has d2 %d, its match %s is at %d" % (name, q, d2[k][q], g, want)
        assert np.array_equal(d2[k], SR.dist2_map(labels[k], truth[k], 2, 0)), name
    assert np.array_equal(got, SR.score_maps(list(zip(labels, truth)), 2, bins, 0))
    t = got[1, 0, H:]
    assert t[1] and t[3] and t[4] and t[5] and t[6], "gaps of 1, 3 and 5 in their bins, 3^2 + 1 and 5^2 + 1 in the next"


def test_a_query_on_the_other_contour(pkg, ctx):
    """labels == truth: every query lies ON the other side's contour, d2 = 0, bin 0, sum256 = 0"""
    rng = np.random.default_rng(3)
    m = _blocky(rng, 40, 70, 4)
    want = _check(pkg, ctx, m[None], m[None].astype(np.uint8), 4, 4, 1, "identical maps")
    assert (want[:, :, 0] == want[:, :, H]).all() and not want[:, :, 1:4].any() and want[:, :, 0].all()


# ------------------------------------------------------------------------------------------------------------- against the reference

@pytest.mark.parametrize("bins", [2, 16, 4096])
@pytest.mark.parametrize("classes", [1, 3, 21, 1000, 4096])
def test_against_the_reference(pkg, ctx, classes, bins):
    rows, cols, n = 45, 77, 2                                   # 13 units and a remainder a map
    dtype = np.uint8 if classes <= 256 else np.int32
    rng = np.random.default_rng(classes + bins)
    for kind, edge in (("blocky", 1), ("blocky", 0), ("random", 1), ("constant", 1), ("constant", 0)):
        pairs = [_pair(rng, kind, rows, cols, classes, dtype) for _ in range(n)]
        labels, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
        if kind == "blocky":
            # the second image's truth loses class 0 to void: the labels' class 0 has nothing to match there, and has in the first image
            truth[1][truth[1] == 0] = 255 if dtype == np.uint8 else -1
        want = _check(pkg, ctx, labels, truth, classes, bins, edge, "%s, edge %d" % (kind, edge))
        if kind == "blocky":
            assert (want[:, :, 1] > 0).any() and (want[:, :, 0] > want[:, :, 1]).any(), "some class unmatched, some matched"
        if kind == "constant":
            assert want.any() == bool(edge), "a constant map has a contour only at the frame"


def test_dist2_null_gives_the_same_table(pkg, ctx):
    rng = np.random.default_rng(20)
    pairs = [_pair(rng, "blocky", 33, 70, 5, np.int32) for _ in range(2)]
    labels, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    with_map, _ = _score(pkg, ctx, labels, truth, 5, 16, 1)
    without, none = _score(pkg, ctx, labels, truth, 5, 16, 1, dist2=False)
    assert none is None and np.array_equal(with_map, without) and np.array_equal(without, SR.score_maps(list(zip(labels, truth)), 5, 16, 1))


def test_accumulation_into_preset_tables(pkg, ctx):
    classes, bins = 3, 8
    rng = np.random.default_rng(21)
    pairs = [_pair(rng, "blocky", 40, 66, classes, np.uint8) for _ in range(2)]
    labels, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    one = SR.score_maps(list(zip(labels, truth)), classes, bins, 1)
    got, _ = _score(pkg, ctx, labels, truth, classes, bins, 1, calls=2)
    twice = 2 * one
    twice[:, :, 2] = one[:, :, 2]
    assert np.array_equal(got, twice), "two calls add; max_d2 stays"
    pre = np.where(one > 0, np.uint64(0xFFFFFFF0), np.uint64(7)).astype(np.uint64)
    pre[:, 0, 2] = np.uint64(1 << 40)                           # direction 0: larger than any distance: it stays
    pre[:, 1, 2] = 0                                            # direction 1: smaller: replaced
    got, _ = _score(pkg, ctx, labels, truth, classes, bins, 1, preset=pre)
    want = pre + one
    want[:, 0, 2] = np.uint64(1 << 40)
    want[:, 1, 2] = one[:, 1, 2]
    assert np.array_equal(got, want)
    big = one >= 16
    big[:, :, 2] = False
    assert big.any() and (got[big] >= np.uint64(1 << 32)).all(), "the adds carry into the high word"
    assert (one[:, 1, 2] > 0).any()


# ----------------------------------------------------------------------------------------------------------------- interior pointers

def test_interior_pointers_at_every_alignment(pkg, ctx):
    """labels at element offsets 0..3 of a 16-byte boundary x uint8 truth at byte offsets 0..3: in-range data lies on both sides and must reach no
    result"""
    classes, bins, rows, cols = 3, 6, 9, 13
    rng = np.random.default_rng(30)
    count = rows * cols
    lab = rng.integers(0, classes, count + 16).astype(np.int32)
    tr = rng.integers(0, classes, count + 16).astype(np.uint8)
    cases = [(lo, to) for lo in range(4) for to in range(4)]
    d_lab, d_tr = ctx.to_device(lab), ctx.to_device(tr)
    assert d_lab.ptr % 16 == 0 and d_tr.ptr % 16 == 0
    h = pkg.Surface(ctx, 1, count, classes)
    tables, maps = [], []
    for lo, to in cases:
        d_surf = _table(ctx, _cells(classes, bins))
        d_d2 = ctx.to_device(np.full(count + 16, FILL, np.uint32))
        ctx.surface_score(h, d_surf.ptr, d_lab.ptr + 4 * lo, d_tr.ptr + to, 1, classes, bins, 1, rows, cols, 0, dist2=d_d2.ptr + 4 * lo)
        tables.append(d_surf)
        maps.append(d_d2)
    ctx.sync()
    for k, (lo, to) in enumerate(cases):
        l, t = lab[lo:lo + count].reshape(rows, cols), tr[to:to + count].reshape(rows, cols)
        assert np.array_equal(_read_table(tables[k], classes, bins), SR.score(l, t, classes, bins, 0)), "labels +%d, truth +%d" % (lo, to)
        got = maps[k].download((count + 16,), np.uint32)
        assert np.array_equal(got[lo:lo + count].reshape(rows, cols), SR.dist2_map(l, t, classes, 0)), "labels +%d, truth +%d" % (lo, to)
        assert (got[:lo] == FILL).all() and (got[lo + count:] == FILL).all(), "dist2 written outside its map"
    h.close()
    for b in [d_lab, d_tr] + tables + maps:
        b.free()


# ---------------------------------------------------------------------------------------------------------------------------- ragged

PLAIN_ITEMS = [(900, 37, 61), (0, 5, 7), (40, 4, 200), (3200, 70, 133), (12600, 4, 4)]            # any order, gaps between the maps
WINDOW_ITEMS = [(17, 1, 1, (3, 5, 1, 1)), (30, 1, 300, (0, 7, 64, 1)), (400, 37, 61, (0, 0, 64, 64)), (5000, 9, 1, (9, 0, 1, 64))]


@pytest.mark.parametrize("kind", ["plain", "window"])
def test_ragged(pkg, ctx, kind):
    classes, bins, edge = 5, 16, 1
    r = pkg.RaggedReadout(ctx, 8)
    if kind == "plain":
        items = PLAIN_ITEMS
        r.set(1, 1, 5, items)
    else:
        items = [it[:3] for it in WINDOW_ITEMS]
        r.set_window(1, 1, 5, 64, 64, WINDOW_ITEMS)
    span = max(off + rows * cols for off, rows, cols in items)
    pixels = sum(rows * cols for _, rows, cols in items)
    rng = np.random.default_rng(len(items))
    lab = rng.integers(0, classes, span + 5).astype(np.int32)   # the gaps hold in-range garbage
    tr = rng.integers(0, classes, span + 5).astype(np.uint8)
    for off, rows, cols in items:
        pl, pt = _pair(rng, "blocky", rows, cols, classes, np.uint8)
        lab[off:off + rows * cols], tr[off:off + rows * cols] = pl.ravel(), pt.ravel()
    h = pkg.Surface(ctx, len(items), pixels, classes)           # the pixels of the maps, not the span: the scratch has no gaps
    d_lab, d_tr = ctx.to_device(lab), ctx.to_device(tr)
    d_surf = _table(ctx, _cells(classes, bins))
    d_d2 = ctx.to_device(np.full(span + 5, FILL, np.uint32))
    ctx.surface_score_ragged(h, r, d_surf.ptr, d_lab.ptr, d_tr.ptr, 1, classes, bins, edge, dist2=d_d2.ptr)
    ctx.sync()
    maps = [(lab[off:off + rows * cols].reshape(rows, cols), tr[off:off + rows * cols].reshape(rows, cols)) for off, rows, cols in items]
    want = SR.score_maps(maps, classes, bins, edge)
    assert np.array_equal(_read_table(d_surf, classes, bins), want)
    got = d_d2.download((span + 5,), np.uint32)
    inside = np.zeros(span + 5, bool)
    for (off, rows, cols), m in zip(items, maps):
        inside[off:off + rows * cols] = True
        assert np.array_equal(got[off:off + rows * cols].reshape(rows, cols), SR.dist2_map(m[0], m[1], classes, edge)), (off, rows, cols)
    assert (got[~inside] == FILL).all(), "the gaps between the maps were written"

    def twice(k, extra=None):
        t = k * want if extra is None else k * want + extra
        t[:, :, 2] = want[:, :, 2] if extra is None else np.maximum(want[:, :, 2], extra[:, :, 2])
        return t

    # a captured launch belongs to its set: replayed after a later set it adds nothing
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_surface_score_ragged_i32(h.h, r.h, d_surf.ptr, None, d_lab.ptr, d_tr.ptr, 1, classes, bins, edge, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(_read_table(d_surf, classes, bins), twice(2)), "a replay under its own set adds"
    r.set(1, 1, 5, [(0, 4, 4)])
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    ctx.sync()
    assert np.array_equal(_read_table(d_surf, classes, bins), twice(2)), "a replay after a later set adds nothing"
    ctx.surface_score_ragged(h, r, d_surf.ptr, d_lab.ptr, d_tr.ptr, 1, classes, bins, edge)      # the new set is what a new launch scores
    ctx.sync()
    new = SR.score(lab[:16].reshape(4, 4), tr[:16].reshape(4, 4), classes, bins, edge)
    assert np.array_equal(_read_table(d_surf, classes, bins), twice(2, new))
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    h.close()
    for b in (d_lab, d_tr, d_surf, d_d2):
        b.free()


# ------------------------------------------------------------------------------------------------------- planning CUs, graph replay

@pytest.mark.parametrize("classes", [21, 150])
def test_planning_cus_give_the_same_bytes(pkg, ctx, classes):
    rows, cols, n, bins = 100, 150, 3, 32
    rng = np.random.default_rng(40)
    pairs = [_pair(rng, "blocky", rows, cols, classes, np.uint8) for _ in range(n)]
    labels, truth = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    want = SR.score_maps(list(zip(labels, truth)), classes, bins, 1)
    want_d2 = np.stack([SR.dist2_map(l, t, classes, 1) for l, t in zip(labels, truth)])
    try:
        for cus in (1, 2, 7, 0):
            assert ctx.lib.mbn_set_planning_cus(ctx.h, cus) == pkg.OK
            got, d2 = _score(pkg, ctx, labels, truth, classes, bins, 1)
            assert got.tobytes() == want.tobytes() and d2.tobytes() == want_d2.tobytes(), "%d planning CUs" % cus
    finally:
        assert ctx.lib.mbn_set_planning_cus(ctx.h, 0) == pkg.OK


def test_graph_capture_and_replay(pkg, ctx):
    classes, bins, rows, cols = 21, 16, 70, 90
    rng = np.random.default_rng(41)
    labels, truth = _pair(rng, "blocky", rows, cols, classes, np.uint8)
    h = pkg.Surface(ctx, 1, rows * cols, classes)
    d_lab, d_tr = ctx.to_device(labels), ctx.to_device(truth)
    d_surf = _table(ctx, _cells(classes, bins))
    d_d2 = ctx.to_device(np.full(rows * cols + 8, FILL, np.uint32))
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_surface_score_i32(h.h, d_surf.ptr, d_d2.ptr, d_lab.ptr, d_tr.ptr, 1, classes, bins, 1, rows, cols, 1, None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert not _read_table(d_surf, classes, bins).any() and (d_d2.download((rows * cols + 8,), np.uint32) == FILL).all(), "the captured call ran"
    want = SR.score(labels, truth, classes, bins, 1)
    for k in (1, 2, 3):
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        ctx.sync()
        t = k * want
        t[:, :, 2] = want[:, :, 2]
        assert np.array_equal(_read_table(d_surf, classes, bins), t), "replay %d" % k
    got = d_d2.download((rows * cols + 8,), np.uint32)
    assert np.array_equal(got[:rows * cols].reshape(rows, cols), SR.dist2_map(labels, truth, classes, 1)) and (got[rows * cols:] == FILL).all()
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    h.close()
    for b in (d_lab, d_tr, d_surf, d_d2):
        b.free()


# ------------------------------------------------------------------------------------------------------------------ argument errors

def test_argument_errors(pkg, ctx):
    classes, bins, rows, cols = 3, 4, 10, 10
    count = rows * cols
    lab, tr = ctx.to_device(np.zeros(count, np.int32)), ctx.to_device(np.zeros(count, np.int32))
    d_surf = _table(ctx, _cells(classes, bins))
    d_d2 = ctx.to_device(np.full(count, FILL, np.uint32))
    small = ctx.to_device(np.full(_cells(classes, bins) - 1, SENTINEL, np.uint64))       # one cell short
    short = ctx.to_device(np.full(count - 1, FILL, np.uint32))
    lib = ctx.lib
    EI, EU = pkg.EINVAL, pkg.EUNSUPPORTED
    h = pkg.Surface(ctx, 2, 2 * count, classes)

    def score(s, l, t, d2=None, hh=h.h, tb=1, c=classes, b=bins, n=1, r=rows, w=cols, e=1):
        return lib.mbn_surface_score_i32(hh, s, d2, l, t, tb, c, b, n, r, w, e, None)

    assert score(None, lab.ptr, tr.ptr) == EI and score(d_surf.ptr, None, tr.ptr) == EI and score(d_surf.ptr, lab.ptr, None) == EI
    assert score(d_surf.ptr, lab.ptr, tr.ptr, hh=None) == EI
    assert score(d_surf.ptr + 4, lab.ptr, tr.ptr) == EI                                                    # the table off 8 bytes
    assert score(d_surf.ptr, lab.ptr + 2, tr.ptr, r=5) == EI                                               # labels off 4
    assert score(d_surf.ptr, lab.ptr, tr.ptr + 2, tb=4, r=5) == EI                                         # an int32 truth off 4
    assert score(d_surf.ptr, lab.ptr, tr.ptr, d2=d_d2.ptr + 2, r=5) == EI                                  # dist2 off 4
    for kw in ({"c": 0}, {"c": -1}, {"b": 1}, {"b": 0}, {"n": 0}, {"r": 0}, {"w": -2}, {"e": 2}, {"e": -1}, {"tb": 2}, {"tb": 0}, {"tb": 8}):
        assert score(d_surf.ptr, lab.ptr, tr.ptr, **kw) == EI, kw
    assert score(d_surf.ptr, lab.ptr, tr.ptr, c=pkg.CONFUSION_MAX_CLASSES + 1) == EU and score(d_surf.ptr, lab.ptr, tr.ptr, b=pkg.SURFACE_MAX_BINS + 1) == EU
    assert score(d_surf.ptr, lab.ptr, tr.ptr, r=32768, w=1) == EU and score(d_surf.ptr, lab.ptr, tr.ptr, r=1, w=32768) == EU
    assert score(d_surf.ptr, lab.ptr, tr.ptr, r=16385, w=32767) == EU and score(d_surf.ptr, lab.ptr, tr.ptr, n=65536) == EU
    assert score(d_surf.ptr, lab.ptr, tr.ptr, c=pkg.CONFUSION_MAX_CLASSES + 1, e=3) == EI, "a caller error goes before a limit"
    # over what the handle was created for: batch, pixels, classes
    assert score(d_surf.ptr, lab.ptr, tr.ptr, n=3, r=2, w=2) == EU and score(d_surf.ptr, lab.ptr, tr.ptr, r=21, w=10) == EU
    assert score(d_surf.ptr, lab.ptr, tr.ptr, c=classes + 1) == EU
    assert score(small.ptr, lab.ptr, tr.ptr) == EI and "surface table" in ctx.last_error()
    assert score(d_surf.ptr, lab.ptr, tr.ptr, n=2) == EI and "surface labels" in ctx.last_error()
    assert score(d_surf.ptr, lab.ptr, tr.ptr + 4 * count - 50, tb=1) == EI and "surface truth" in ctx.last_error()
    assert score(d_surf.ptr, lab.ptr, tr.ptr, d2=short.ptr) == EI and "surface dist2" in ctx.last_error()
    assert score(d_surf.ptr, lab.ptr + 4, tr.ptr, tb=4) == EI                                              # an interior pointer: one element short
    assert score(d_surf.ptr, lab.ptr, tr.ptr, d2=d_d2.ptr + 4) == EI                                       # likewise
    assert score(d_surf.ptr, lab.ptr, tr.ptr, d2=lab.ptr) == EI and score(d_surf.ptr, lab.ptr, tr.ptr, d2=tr.ptr, tb=4) == EI, "dist2 over an input"
    assert score(d_surf.ptr, lab.ptr, tr.ptr, d2=lab.ptr + 4 * (count - 1)) == EI, "dist2 over the labels' last element"
    hh = C.c_void_p()
    assert lib.mbn_surface_create(ctx.h, 0, 10, 3, C.byref(hh)) == EI and lib.mbn_surface_create(ctx.h, 1, 0, 3, C.byref(hh)) == EI
    assert lib.mbn_surface_create(ctx.h, 1, 10, 0, C.byref(hh)) == EI and lib.mbn_surface_create(None, 1, 10, 3, C.byref(hh)) == EI
    assert lib.mbn_surface_create(ctx.h, 1, 10, 3, None) == EI
    assert lib.mbn_surface_create(ctx.h, 65536, 10, 3, C.byref(hh)) == EU and lib.mbn_surface_create(ctx.h, 1, 10, 4097, C.byref(hh)) == EU
    assert not hh.value and lib.mbn_surface_destroy(None) == pkg.OK
    r = pkg.RaggedReadout(ctx, 4)

    def rscore(rh, s, l, t, d2=None, hh=h.h, tb=1, c=classes, b=bins, e=1):
        return lib.mbn_surface_score_ragged_i32(hh, rh, s, d2, l, t, tb, c, b, e, None)

    assert rscore(r.h, d_surf.ptr, lab.ptr, tr.ptr) == EI and rscore(None, d_surf.ptr, lab.ptr, tr.ptr) == EI          # no set, no read-out
    r.set(1, 1, 5, [(2, 4, 5), (60, 5, 8)])
    assert rscore(r.h, d_surf.ptr, lab.ptr, tr.ptr, hh=None) == EI
    assert rscore(r.h, d_surf.ptr, lab.ptr, tr.ptr, tb=2) == EI and rscore(r.h, d_surf.ptr, None, tr.ptr) == EI and rscore(r.h, d_surf.ptr, lab.ptr, tr.ptr, b=1) == EI
    assert rscore(r.h, d_surf.ptr, lab.ptr, tr.ptr, c=4097) == EU and rscore(r.h, d_surf.ptr, lab.ptr, tr.ptr, b=4097) == EU
    assert rscore(r.h, d_surf.ptr, lab.ptr + 4, tr.ptr) == EI and "surface labels" in ctx.last_error()                  # the set reaches element 100
    assert rscore(r.h, d_surf.ptr, lab.ptr, tr.ptr, d2=short.ptr) == EI
    ctx.sync()
    assert not _read_table(d_surf, classes, bins).any(), "a refused call was launched"
    assert rscore(r.h, d_surf.ptr, lab.ptr, tr.ptr) == pkg.OK
    ctx.sync()
    got = _read_table(d_surf, classes, bins)
    # constant maps of 0, 4 x 5 and 5 x 8 with the frame: 14 + 22 queries a direction, all on the other contour
    assert list(got[0, 0]) == [36, 0, 0, 0, 36, 0, 0, 0] and list(got[0, 1]) == list(got[0, 0]) and not got[1:].any(), "only the one accepted call ran"
    assert (d_d2.download((count,), np.uint32) == FILL).all() and (short.download((count - 1,), np.uint32) == FILL).all()
    assert (small.download((_cells(classes, bins) - 1,), np.uint64) == SENTINEL).all()
    assert (lab.download((count,), np.int32) == 0).all() and (tr.download((count,), np.int32) == 0).all()
    r.close()
    h.close()
    for b in (lab, tr, d_surf, d_d2, small, short):
        b.free()


# --------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS = 0.5, 21, 64, 96


def test_net_segment_surface(pkg, ctx, tmp_path):
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, 16)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 8)
    net.set_input_u8(True)
    rng = np.random.default_rng(50)
    n, sh, sw, bins = 2, 75, 130, 32
    src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    npix = n * sh * sw
    truth = rng.integers(0, CLASSES, npix + 64).astype(np.uint8)
    truth[:npix] = np.stack([_pair(rng, "blocky", sh, sw, CLASSES, np.uint8)[1] for _ in range(n)]).ravel()
    d_src, d_lab, d_tr = ctx.to_device(src), ctx.alloc(4 * (npix + 64)), ctx.to_device(truth)
    d_surf = _table(ctx, _cells(CLASSES, bins))
    d_d2 = ctx.to_device(np.full(npix + 64, FILL, np.uint32))
    assert ctx.lib.mbn_net_segment_surface(net.h, d_lab.ptr, d_tr.ptr, 1, bins, 1, d_surf.ptr, d_d2.ptr) == pkg.EINVAL, "before any segment call"
    total = np.zeros((CLASSES, 2, H + bins), np.uint64)

    def check(what, edge, items=None):
        ctx.lib.mbn_memset(ctx.h, d_d2.ptr, 0xA5, 4 * (npix + 64))
        net.segment_surface(d_lab.ptr, d_tr.ptr, 1, d_surf.ptr, bins=bins, edge=edge, dist2_ptr=d_d2.ptr)
        ctx.sync()
        lab = d_lab.download((npix + 64,), np.int32)
        if items is None:
            items = [(i * sh * sw, sh, sw) for i in range(n)]
        maps = [(lab[off:off + r * c].reshape(r, c), truth[off:off + r * c].reshape(r, c)) for off, r, c in items]
        SR.add(total, SR.score_maps(maps, CLASSES, bins, edge))
        assert np.array_equal(_read_table(d_surf, CLASSES, bins), total), what
        got = d_d2.download((npix + 64,), np.uint32)
        inside = np.zeros(npix + 64, bool)
        for (off, r, c), m in zip(items, maps):
            inside[off:off + r * c] = True
            assert np.array_equal(got[off:off + r * c].reshape(r, c), SR.dist2_map(m[0], m[1], CLASSES, edge)), what
        assert (got[~inside] == FILL).all(), what
        return maps

    img = net.resize_input(d_src.ptr, n, sh, sw, pkg.FIT_STRETCH)
    net.segment_to(img, n, sh, sw, d_lab.ptr)
    maps = check("segment_to", 1)
    assert len(np.unique(maps[0][0])) > 1
    net.segment_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr)
    check("segment_fit, the pad fit", 0)
    rows, cols = [sh, 40], [sw, 50]
    offs, dst = [0, sh * sw * 3], [sh * sw + 11, 3]
    ctx.lib.mbn_memset(ctx.h, d_lab.ptr, 0xFF, 4 * (npix + 64))
    net.segment_images_fit(d_src.ptr, offs, rows, cols, pkg.FIT_PAD, d_lab.ptr, dst)
    check("image call", 1, items=[(dst[i], rows[i], cols[i]) for i in range(2)])
    assert total[:, :, 0].any() and (total[:, :, 0] > total[:, :, 1]).any()
    for bad in ((1, 1, 1), (2, bins, 1), (1, bins, 2), (1, pkg.SURFACE_MAX_BINS + 1, 1)):
        rc = ctx.lib.mbn_net_segment_surface(net.h, d_lab.ptr, d_tr.ptr, bad[0], bad[1], bad[2], d_surf.ptr, None)
        assert rc == (pkg.EUNSUPPORTED if bad[1] > pkg.SURFACE_MAX_BINS else pkg.EINVAL), bad
    ctx.sync()
    assert np.array_equal(_read_table(d_surf, CLASSES, bins), total), "a refused call adds nothing"
    m, hd, hdp, assd, nsd = pkg.surface_metrics(total, CLASSES, bins, 2, 95.0)
    want = SR.metrics(total, CLASSES, bins, 2, 95.0)
    assert m.classes_present == want["classes_present"] > 0 and m.classes_measurable == want["classes_measurable"]
    assert np.array_equal(np.isnan(hd), np.isnan(want["hd_c"])) and np.array_equal(hdp, want["hdp_c"], equal_nan=True)
    net.destroy()
    for b in (d_src, d_lab, d_tr, d_surf, d_d2):
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


def test_c_host_surface(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    sh, sw, classes = 75, 130, 1000                             # the host's synthetic weights have 1000 classes
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, plain, tta, smap = str(tmp_path / "a.ppm"), str(tmp_path / "plain.pgm"), str(tmp_path / "tta.pgm"), str(tmp_path / "surface.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", "3", "--alpha", "0.5", "--res", "%dx%d" % (ROWS, COLS), "--output-stride", "16", "--ppm", ppm, "--fit", "pad"]
    r = subprocess.run(common + ["--segment-source", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "surface:" not in r.stdout, r.stdout + r.stderr
    bins, tol, pct = 16, 1, 90.0
    r = subprocess.run(common + ["--segment-source", tta, "--tta-scales", "1,0.5", "--tta-flip", "--truth", plain, "--surface", "--surface-bins", str(bins),
                                 "--surface-tolerance", str(tol), "--surface-percentile", str(pct), "--surface-edge", "0", "--surface-map", smap],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "score: pixels=" in r.stdout, r.stdout + r.stderr
    labels, truth = _pgm(tta), _pgm(plain)
    surf = SR.score(labels, truth, classes, bins, 0)
    want = SR.metrics(surf, classes, bins, tol, pct)
    s = _fields(r.stdout, "surface")
    assert (s["bins"], s["tolerance"], s["percentile"], s["classes_present"], s["classes_measurable"], s["unmatched"], s["saturated"]) == \
        (bins, tol, pct, want["classes_present"], want["classes_measurable"], want["unmatched"], want["saturated"])
    assert want["classes_present"] > 0
    for key in ("hd", "hdp", "assd", "nsd"):
        assert s[key] == want[key] or abs(s[key] - want[key]) <= classes * 2.0 ** -52 * abs(want[key]), (key, s[key], want[key])
    per_class = {int(c): [float(v) for v in rest.split()] for c, rest in re.findall(r"^surface_class: class (\d+) (.*)$", r.stdout, re.M)}
    present = ~np.isnan(want["nsd_c"])
    assert sorted(per_class) == list(np.flatnonzero(present))
    for c, vals in per_class.items():
        for got, key in zip(vals, ("hd_c", "hdp_c", "assd_c", "nsd_c")):
            w = want[key][c]
            assert (np.isnan(got) and np.isnan(w)) or got == w or abs(got - w) <= classes * 2.0 ** -52 * abs(w), (c, key, got, w)
    assert np.array_equal(_pgm(smap), SR.surface_map(SR.dist2_map(labels, truth, classes, 0))), "--surface-map is the label map's contour"
    # the defaults: 64 bins, tolerance 2, percentile 95, the frame a contour
    r = subprocess.run(common + ["--segment-source", tta, "--truth", plain, "--surface"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    s = _fields(r.stdout, "surface")
    want = SR.metrics(SR.score(_pgm(tta), truth, classes, 64, 1), classes, 64, 2, 95.0)
    assert (s["bins"], s["tolerance"], s["percentile"], s["classes_present"], s["unmatched"]) == (64, 2, 95.0, want["classes_present"], want["unmatched"])
    # no --truth, no --segment-source, an option without --surface, bad values
    for extra in (["--segment-source", tta, "--surface"],
                  ["--truth", plain, "--surface"],
                  ["--segment-source", tta, "--truth", plain, "--surface-bins", "16"],
                  ["--segment-source", tta, "--truth", plain, "--surface", "--surface-bins", "1"],
                  ["--segment-source", tta, "--truth", plain, "--surface", "--surface-bins", "4097"],
                  ["--segment-source", tta, "--truth", plain, "--surface", "--surface-bins", "8", "--surface-tolerance", "7"],
                  ["--segment-source", tta, "--truth", plain, "--surface", "--surface-tolerance", "-1"],
                  ["--segment-source", tta, "--truth", plain, "--surface", "--surface-percentile", "0"],
                  ["--segment-source", tta, "--truth", plain, "--surface", "--surface-percentile", "101"],
                  ["--segment-source", tta, "--truth", plain, "--surface", "--surface-edge", "2"]):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "surface:" not in r.stdout, (extra, r.stdout + r.stderr)
