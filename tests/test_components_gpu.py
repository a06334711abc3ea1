"""Regions of a label map on the GPU: mbn_components_i32 / mbn_components_ragged_i32 against tests/components_ref.py. Everything is integer, so
every comparison is exact. Every output buffer carries a sentinel tail (and, in the ragged form, sentinel gaps) that must come back unchanged, and
the region table must hold the sentinel from record min(n, max_regions) on. The shapes are the smallest that reach each way of going wrong: sizes on
both sides of every tile seam (mbn_components_tile), patterns whose components cross the seams in every way, the min_area drop, a table too small,
every alignment, planning CU counts, graph replay, ragged sets of both kinds, an element offset above 2^30, the net runner and the C host."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_ref as R
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

TAIL = 16
SENT = np.int32(0x5A5A5A5A)
IGNORE = 255


@pytest.fixture(scope="module")
def tile(pkg):
    return pkg.components_tile()


@pytest.fixture(scope="module")
def comps(pkg, ctx):
    h = pkg.Components(ctx, 8, 1 << 18)
    yield h
    h.close()


def _want(maps, classes, conn, min_area=1, ignore=IGNORE):
    return [R.components(L, classes, conn, min_area, ignore) for L in maps]


def _run(ctx, comps, maps, classes, conn, min_area=1, ignore=IGNORE, max_regions=None, comp=True, out=True, want=None, offs=(0, 0, 0),
         what=""):
    """One mbn_components_i32 on freshly uploaded maps [batch][rows][cols], compared with the reference in full. offs: element offsets of labels,
    comp and labels_out from their (16-byte aligned) buffers. Returns the true region counts."""
    maps = np.ascontiguousarray(maps, np.int32)
    batch, rows, cols = maps.shape
    want = want or _want(maps, classes, conn, min_area, ignore)
    n_want = [len(w[1]) for w in want]
    if max_regions is None:
        max_regions = max(n_want) + 1
    count = maps.size
    host_lab = np.full(count + TAIL + 4, 1, np.int32)           # in-range garbage around the maps
    host_lab[offs[0]:offs[0] + count] = maps.ravel()
    d_lab = ctx.to_device(host_lab)
    d_comp = ctx.to_device(np.full(count + TAIL + 4, SENT, np.int32))
    d_out = ctx.to_device(np.full(count + TAIL + 4, SENT, np.int32))
    d_reg = ctx.to_device(np.full((batch * max_regions + 2) * 8, SENT, np.int32))
    d_n = ctx.to_device(np.full(batch + TAIL, SENT, np.int32))
    assert d_lab.ptr % 16 == 0 and d_comp.ptr % 16 == 0 and d_out.ptr % 16 == 0
    ctx.components(comps, d_lab.ptr + 4 * offs[0], batch, rows, cols, classes, d_n.ptr, comp=d_comp.ptr + 4 * offs[1] if comp else None,
                   regions=d_reg.ptr if max_regions else None, labels_out=d_out.ptr + 4 * offs[2] if out else None, connectivity=conn,
                   min_area=min_area, ignore_label=ignore, max_regions=max_regions)
    ctx.sync()
    got_n = d_n.download((batch + TAIL,), np.int32)
    got_comp = d_comp.download((count + TAIL + 4,), np.int32)
    got_out = d_out.download((count + TAIL + 4,), np.int32)
    got_reg = d_reg.download((batch * max_regions + 2, 8), np.int32)
    for b in (d_lab, d_comp, d_out, d_reg, d_n):
        b.free()
    assert (got_n[batch:] == SENT).all(), what + ": n_regions written past the batch"
    assert got_n[:batch].tolist() == n_want, what + ": n_regions %s, expected %s" % (got_n[:batch].tolist(), n_want)
    for name, got, off, on, k in (("comp", got_comp, offs[1], comp, 0), ("labels_out", got_out, offs[2], out, 2)):
        if not on:
            assert (got == SENT).all(), what + ": %s is NULL and was written" % name
            continue
        assert (got[:off] == SENT).all() and (got[off + count:] == SENT).all(), what + ": %s written outside the maps" % name
        body = got[off:off + count].reshape(batch, rows, cols)
        for i in range(batch):
            bad = int((body[i] != want[i][k]).sum())
            assert bad == 0, what + ": %s of image %d differs in %d pixels" % (name, i, bad)
    assert (got_reg[batch * max_regions:] == SENT).all(), what + ": the table written past its end"
    table = got_reg[:batch * max_regions].reshape(batch, max_regions, 8)
    for i in range(batch):
        k = min(n_want[i], max_regions)
        assert np.array_equal(table[i, :k], want[i][1][:k]), what + ": records of image %d" % i
        assert (table[i, k:] == SENT).all(), what + ": image %d: a record from min(n, max_regions) on was written" % i
    return n_want


# --------------------------------------------------------------------------------------------------------------------- sizes at the seams

def _seam_sizes(tile):
    tr, tc = tile
    return [1, 2, tr - 1, tr, tr + 1, 2 * tr + 1], [1, 2, 63, 64, 65, tc - 1, tc, tc + 1, 2 * tc + 1]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("batch", [1, 3])
def test_sizes_at_the_seams(pkg, ctx, comps, tile, conn, batch):
    rows_set, cols_set = _seam_sizes(tile)
    for rows in rows_set:
        for cols in sorted(set(cols_set)):
            # large blobs of three classes with some abstained pixels: components that cross every seam the size has, a different image per slot
            maps = np.stack([R.blocks(rows, cols, 3, seed=rows * 1000 + cols + i, side=3 + 2 * i) for i in range(batch)])
            rng = np.random.default_rng(rows + cols)
            maps[rng.random(maps.shape) < 0.05] = -1
            _run(ctx, comps, maps, 3, conn, what="%d x %d x %d" % (batch, rows, cols))


# --------------------------------------------------------------------------------------------------------------------------- patterns

@pytest.mark.parametrize("conn", [4, 8])
def test_patterns(pkg, ctx, comps, tile, conn):
    tr, tc = tile
    rows, cols = 2 * tr + 1, 2 * tc + 1                        # 3 x 3 tiles: two whole ones and a sliver each way
    for name, classes, L in R.patterns(rows, cols, tr, tc, seed=conn):
        n = _run(ctx, comps, L[None], classes, conn, what=name)
        if name == "constant":
            assert n == [1]
        if name == "checkerboard":
            assert n == ([rows * cols] if conn == 4 else [2])
        if name == "spiral":
            assert n == [2], "the path and the wall between its turns"
        if name.startswith("comb"):
            assert n[0] == 1 + ((cols if "row" in name else rows) + 1) // 2, "one comb, and the gaps at the even columns (rows) between its teeth"
        if name.startswith("corner"):
            assert n == ([3] if conn == 4 else [2])


def test_corner_pixels_at_every_tile_corner(pkg, ctx, comps, tile):
    """two pixels that touch only diagonally, both diagonals, at a corner where four tiles meet and at corners on the second seam"""
    tr, tc = tile
    rows, cols = 2 * tr + 2, 2 * tc + 2
    for r in (tr, 2 * tr):
        for c in (tc, 2 * tc):
            for anti in (False, True):
                L = R.corner_touch(rows, cols, r, c, anti)
                assert _run(ctx, comps, L[None], 2, 4, what="corner %d, %d" % (r, c)) == [3]
                assert _run(ctx, comps, L[None], 2, 8, what="corner %d, %d" % (r, c)) == [2]


# --------------------------------------------------------------------------------------------------------------------------- min_area

def test_min_area(pkg, ctx, comps, tile):
    tr, tc = tile
    rows, cols = tr + 5, tc + 9
    maps = np.stack([R.random_map(rows, cols, 3, seed=11, abstain=True), R.blocks(rows, cols, 5, seed=12, side=4), R.checkerboard(rows, cols)])
    for conn in (4, 8):
        largest = max(int(w[1][:, 1].max()) for w in _want(maps, 5, conn))
        kept = []
        for min_area in (1, 2, 5, largest + 1):
            want = _want(maps, 5, conn, min_area, IGNORE)
            kept.append(_run(ctx, comps, maps, 5, conn, min_area=min_area, want=want, what="min_area %d" % min_area))
            if min_area > largest:
                assert kept[-1] == [0, 0, 0] and all((w[0] == -1).all() for w in want)
                assert all((w[2][(maps[i] >= 0) & (maps[i] < 5)] == IGNORE).all() for i, w in enumerate(want)), "all valid pixels are dropped"
        assert kept[0][0] > kept[1][0] > kept[2][0] > 0, "the survivors are renumbered among fewer and fewer"
    _run(ctx, comps, maps, 5, 8, min_area=3, out=False, what="labels_out NULL")
    _run(ctx, comps, maps, 5, 8, min_area=3, comp=False, what="comp NULL")
    _run(ctx, comps, maps, 5, 4, min_area=2, comp=False, out=False, what="both NULL")
    _run(ctx, comps, maps, 5, 4, min_area=2, ignore=-7, what="a negative ignore_label")


def test_table_overflow(pkg, ctx, comps, tile):
    tr, tc = tile
    L = R.blocks(tr + 3, tc + 3, 4, seed=5, side=7)[None]
    n = len(_want(L, 4, 4)[0][1])
    assert n > 3
    for max_regions in (0, 1, n - 1, n, n + 1):
        assert _run(ctx, comps, L, 4, 4, max_regions=max_regions, what="max_regions %d of %d" % (max_regions, n)) == [n]
    # the drop comes before the table: with min_area the table holds the first survivors
    _run(ctx, comps, np.concatenate([L, L[:, ::-1]]), 4, 8, min_area=30, max_regions=2, what="min_area and a short table")


# -------------------------------------------------------------------------------------------------------------------------- alignment

def test_every_alignment(pkg, ctx, comps, tile):
    tr, tc = tile
    maps = np.stack([R.random_map(tr + 1, tc + 3, 3, seed=21, abstain=True), R.blocks(tr + 1, tc + 3, 3, seed=22, side=5)])
    want = _want(maps, 3, 8, 2, IGNORE)
    for lo in range(4):
        for co in range(4):
            for oo in range(4):
                _run(ctx, comps, maps, 3, 8, min_area=2, want=want, offs=(lo, co, oo), what="labels +%d, comp +%d, labels_out +%d" % (lo, co, oo))


# ---------------------------------------------------------------------------------------------------------------- planning CUs, graph

def _raw(ctx, comps, d, maps_shape, classes, conn, min_area, max_regions):
    """the four outputs of one call as bytes, from preset device buffers d = (lab, comp, reg, n, out)"""
    batch, rows, cols = maps_shape
    ctx.components(comps, d[0].ptr, batch, rows, cols, classes, d[3].ptr, comp=d[1].ptr, regions=d[2].ptr, labels_out=d[4].ptr, connectivity=conn,
                   min_area=min_area, ignore_label=IGNORE, max_regions=max_regions)
    ctx.sync()
    return (d[1].download((batch * rows * cols + TAIL,), np.int32), d[2].download((batch * max_regions, 8), np.int32),
            d[3].download((batch,), np.int32), d[4].download((batch * rows * cols + TAIL,), np.int32))


def _bufs(ctx, maps, max_regions):
    batch = maps.shape[0]
    return (ctx.to_device(maps), ctx.to_device(np.full(maps.size + TAIL, SENT, np.int32)), ctx.to_device(np.full(batch * max_regions * 8, SENT, np.int32)),
            ctx.to_device(np.full(batch, SENT, np.int32)), ctx.to_device(np.full(maps.size + TAIL, SENT, np.int32)))


def _expect(got, want, shape, max_regions, what):
    batch, rows, cols = shape
    comp, reg, n, out = got
    assert (comp[batch * rows * cols:] == SENT).all() and (out[batch * rows * cols:] == SENT).all(), what
    comp, out, reg = comp[:batch * rows * cols].reshape(shape), out[:batch * rows * cols].reshape(shape), reg.reshape(batch, max_regions, 8)
    for i in range(batch):
        k = len(want[i][1])
        assert n[i] == k and k <= max_regions, what
        assert np.array_equal(comp[i], want[i][0]) and np.array_equal(out[i], want[i][2]) and np.array_equal(reg[i, :k], want[i][1]), what
        assert (reg[i, k:] == SENT).all(), what


def test_planning_cus_give_the_same_bytes(pkg, ctx, comps, tile):
    tr, tc = tile
    shape = (3, 3 * tr + 7, 2 * tc + 31)
    maps = np.stack([R.random_map(shape[1], shape[2], 3, seed=31), R.random_map(shape[1], shape[2], 21, seed=32, abstain=True),
                     R.blocks(shape[1], shape[2], 21, seed=33)])
    want = _want(maps, 21, 8, 2, IGNORE)
    max_regions = max(len(w[1]) for w in want) + 1
    try:
        results = []
        for cus in (1, 2, 0):
            assert ctx.lib.mbn_set_planning_cus(ctx.h, cus) == pkg.OK
            d = _bufs(ctx, maps, max_regions)
            results.append(_raw(ctx, comps, d, shape, 21, 8, 2, max_regions))
            for b in d:
                b.free()
            _expect(results[-1], want, shape, max_regions, "%d planning CUs" % cus)
        for other in results[1:]:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(results[0], other)), "identical bytes in all four outputs"
    finally:
        assert ctx.lib.mbn_set_planning_cus(ctx.h, 0) == pkg.OK


def test_graph_capture_and_replay(pkg, ctx, comps, tile):
    tr, tc = tile
    shape = (2, tr + 9, tc + 17)
    first = np.stack([R.random_map(shape[1], shape[2], 3, seed=41), R.spiral(shape[1], shape[2])])
    second = np.stack([R.blocks(shape[1], shape[2], 3, seed=42, side=6), R.checkerboard(shape[1], shape[2])])
    max_regions = shape[1] * shape[2]
    d = _bufs(ctx, first, max_regions)
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_components_i32(comps.h, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, d[0].ptr, shape[0], shape[1], shape[2], 3, 4, 1, IGNORE, max_regions,
                                    None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    ctx.sync()
    assert (d[3].download((2,), np.int32) == SENT).all(), "the captured call ran"
    for maps in (first, second):
        d[0].upload(maps)
        d[2].upload(np.full(shape[0] * max_regions * 8, SENT, np.int32))
        assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
        ctx.sync()
        got = (d[1].download((maps.size + TAIL,), np.int32), d[2].download((shape[0] * max_regions, 8), np.int32), d[3].download((2,), np.int32),
               d[4].download((maps.size + TAIL,), np.int32))
        _expect(got, _want(maps, 3, 4), shape, max_regions, "replay")
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    for b in d:
        b.free()


# ----------------------------------------------------------------------------------------------------------------------------- ragged

def _ragged_items(tile, smallest):
    """five maps; `smallest`: the side of the smallest one (a plain set of a 1 x 1 coarse map takes maps of 4 x 4 at least, a window set any)"""
    tr, tc = tile
    sizes = [(tr + 1, tc + 1), (smallest, smallest), (5, 3 * tc + 8), (2 * tr + 6, 30), (2 * tr, 2 * tc)]
    order, off, items = [3, 0, 4, 1, 2], 7, [None] * 5            # any order in memory, gaps between the maps
    for i in order:
        items[i] = (off, sizes[i][0], sizes[i][1])
        off += sizes[i][0] * sizes[i][1] + 13 + i
    return items, off


@pytest.mark.parametrize("kind", ["plain", "window"])
def test_ragged(pkg, ctx, comps, tile, kind):
    items, span = _ragged_items(tile, 4 if kind == "plain" else 1)
    classes, conn, min_area, max_regions = 4, 8, 3, 1000
    rng = np.random.default_rng(51)
    lab = rng.integers(0, classes, span + TAIL).astype(np.int32)      # the gaps hold in-range garbage
    want = []
    for i, (off, rows, cols) in enumerate(items):
        L = R.blocks(rows, cols, classes, seed=60 + i, side=3) if i % 2 else R.random_map(rows, cols, classes, seed=60 + i, abstain=True)
        lab[off:off + rows * cols] = L.ravel()
        want.append(R.components(L, classes, conn, min_area, IGNORE))
        assert len(want[-1][1]) <= max_regions
    r = pkg.RaggedReadout(ctx, 8)
    if kind == "plain":
        r.set(1, 1, 5, items)                                   # the set's own class count is not the call's
    else:
        r.set_window(1, 1, 5, 64, 64, [it + ((3, 5, 1, 1),) for it in items])
    d_lab = ctx.to_device(lab)
    d_comp, d_out = ctx.to_device(np.full(span + TAIL, SENT, np.int32)), ctx.to_device(np.full(span + TAIL, SENT, np.int32))
    d_reg, d_n = ctx.to_device(np.full((5 * max_regions + 2) * 8, SENT, np.int32)), ctx.to_device(np.full(5 + TAIL, SENT, np.int32))

    def outputs():
        ctx.sync()
        return (d_comp.download((span + TAIL,), np.int32), d_out.download((span + TAIL,), np.int32), d_reg.download((5 * max_regions + 2, 8), np.int32),
                d_n.download((5 + TAIL,), np.int32))

    ctx.components_ragged(comps, r, d_lab.ptr, classes, d_n.ptr, comp=d_comp.ptr, regions=d_reg.ptr, labels_out=d_out.ptr, connectivity=conn,
                          min_area=min_area, ignore_label=IGNORE, max_regions=max_regions)
    comp, out, reg, n = outputs()
    inside = np.zeros(span + TAIL, bool)
    for i, (off, rows, cols) in enumerate(items):
        inside[off:off + rows * cols] = True
        k = len(want[i][1])
        assert n[i] == k, "map %d" % i
        assert np.array_equal(comp[off:off + rows * cols].reshape(rows, cols), want[i][0]), "comp of map %d" % i
        assert np.array_equal(out[off:off + rows * cols].reshape(rows, cols), want[i][2]), "labels_out of map %d" % i
        assert np.array_equal(reg[i * max_regions:i * max_regions + k], want[i][1]) and (reg[i * max_regions + k:(i + 1) * max_regions] == SENT).all()
        # each map equals the uniform call on that map alone
        _run(ctx, comps, lab[off:off + rows * cols].reshape(1, rows, cols), classes, conn, min_area=min_area, want=[want[i]], what="map %d alone" % i)
    assert (comp[~inside] == SENT).all() and (out[~inside] == SENT).all(), "the gaps and the tail keep the sentinel"
    assert (n[5:] == SENT).all() and (reg[5 * max_regions:] == SENT).all()
    # a captured launch belongs to its set: replayed after a later set it writes nothing
    g = C.c_void_p()
    assert ctx.lib.mbn_graph_begin(ctx.h, None) == pkg.OK
    rc = ctx.lib.mbn_components_ragged_i32(comps.h, r.h, d_comp.ptr, d_reg.ptr, d_n.ptr, d_out.ptr, d_lab.ptr, classes, conn, min_area, IGNORE, max_regions,
                                           None)
    assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g)) == pkg.OK and rc == pkg.OK
    fresh = [np.full(span + TAIL, SENT, np.int32), np.full(span + TAIL, SENT, np.int32), np.full((5 * max_regions + 2) * 8, SENT, np.int32),
             np.full(5 + TAIL, SENT, np.int32)]

    def reset():
        for b, a in zip((d_comp, d_out, d_reg, d_n), fresh):
            b.upload(a)

    reset()
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    again = outputs()
    assert all(np.array_equal(a, b) for a, b in zip(again, (comp, out, reg, n))), "a replay under its own set writes the same"
    reset()
    r.set(1, 1, 5, [(0, 4, 4)])
    assert ctx.lib.mbn_graph_launch(ctx.h, g, None) == pkg.OK
    assert all((a == SENT).all() for a in outputs()), "a replay after a later set writes nothing"
    assert ctx.lib.mbn_graph_destroy(ctx.h, g) == pkg.OK
    r.close()
    for b in (d_lab, d_comp, d_out, d_reg, d_n):
        b.free()


def test_ragged_offset_above_2_to_30(pkg, ctx, comps, tile):
    """one item whose dst_offset lies above 2^30 elements, so its byte offset is above 2^32: the buffers are allocated, not filled, and only the
    two small maps are touched"""
    tr, tc = tile
    far = (1 << 30) + 11
    items = [(far, tr + 1, tc + 1), (3, 5, 7)]
    total = far + items[0][1] * items[0][2]
    bufs = []
    for _ in range(3):
        p = C.c_void_p()
        rc = ctx.lib.mbn_alloc(ctx.h, 4 * (total + TAIL), C.byref(p))
        if rc == pkg.ENOMEM:
            for q in bufs:
                ctx.lib.mbn_free(ctx.h, q)
            pytest.skip("not enough device memory for three buffers of %d bytes" % (4 * total))
        assert rc == pkg.OK
        bufs.append(p)
    d_lab, d_comp, d_out = (b.value for b in bufs)
    classes, max_regions = 3, 400
    maps = [R.random_map(rows, cols, classes, seed=70 + i, abstain=True) for i, (_, rows, cols) in enumerate(items)]
    want = [R.components(L, classes, 4, 2, IGNORE) for L in maps]
    for (off, rows, cols), L in zip(items, maps):
        pad = np.full(rows * cols + 2 * TAIL, SENT, np.int32)   # sentinels around each map in the outputs
        for dst in (d_comp, d_out):
            assert ctx.lib.mbn_upload(ctx.h, dst + 4 * (off - (TAIL if off >= TAIL else off)), pad.ctypes.data,
                                      4 * (rows * cols + TAIL + min(off, TAIL))) == pkg.OK
        assert ctx.lib.mbn_upload(ctx.h, d_lab + 4 * off, L.ctypes.data, L.nbytes) == pkg.OK
    d_reg, d_n = ctx.to_device(np.full(2 * max_regions * 8, SENT, np.int32)), ctx.to_device(np.full(2 + TAIL, SENT, np.int32))
    r = pkg.RaggedReadout(ctx, 4)
    r.set(1, 1, 5, items)
    ctx.components_ragged(comps, r, d_lab, classes, d_n.ptr, comp=d_comp, regions=d_reg.ptr, labels_out=d_out, connectivity=4, min_area=2,
                          ignore_label=IGNORE, max_regions=max_regions)
    ctx.sync()
    n, reg = d_n.download((2 + TAIL,), np.int32), d_reg.download((2, max_regions, 8), np.int32)
    assert (n[2:] == SENT).all()
    for i, ((off, rows, cols), w) in enumerate(zip(items, want)):
        lead = min(off, TAIL)
        for dst, k in ((d_comp, 0), (d_out, 2)):
            got = np.empty(lead + rows * cols + TAIL, np.int32)
            assert ctx.lib.mbn_download(ctx.h, got.ctypes.data, dst + 4 * (off - lead), got.nbytes) == pkg.OK
            assert (got[:lead] == SENT).all() and (got[lead + rows * cols:] == SENT).all(), "written outside map %d" % i
            assert np.array_equal(got[lead:lead + rows * cols].reshape(rows, cols), w[k]), "map %d" % i
        assert n[i] == len(w[1]) and np.array_equal(reg[i, :n[i]], w[1]) and (reg[i, n[i]:] == SENT).all()
    r.close()
    for b in (d_reg, d_n):
        b.free()
    for q in bufs:
        ctx.lib.mbn_free(ctx.h, q)


# -------------------------------------------------------------------------------------------------------------------- argument errors

def test_argument_errors(pkg, ctx, tile):
    lib = ctx.lib
    rows, cols, count = 6, 10, 60
    h = pkg.Components(ctx, 2, 2 * count)
    lab = ctx.to_device(np.zeros(2 * count, np.int32))
    outs = [ctx.to_device(np.full(2 * count, SENT, np.int32)) for _ in range(2)]
    reg, n = ctx.to_device(np.full(2 * 4 * 8, SENT, np.int32)), ctx.to_device(np.full(2, SENT, np.int32))
    comp, out = outs

    def call(hh=h.h, c=comp.ptr, rg=reg.ptr, nn=n.ptr, o=out.ptr, l=lab.ptr, batch=2, r=rows, cl=cols, classes=3, conn=4, min_area=1, mr=4):
        return lib.mbn_components_i32(hh, c, rg, nn, o, l, batch, r, cl, classes, conn, min_area, IGNORE, mr, None)

    assert call(hh=None) == pkg.EINVAL and call(l=None) == pkg.EINVAL and call(nn=None) == pkg.EINVAL
    assert call(rg=None) == pkg.EINVAL, "regions NULL with max_regions > 0"
    for conn in (6, 0, 5):
        assert call(conn=conn) == pkg.EINVAL
    assert call(min_area=0) == pkg.EINVAL and call(mr=-1) == pkg.EINVAL and call(classes=0) == pkg.EINVAL
    assert call(batch=0) == pkg.EINVAL and call(r=0) == pkg.EINVAL and call(cl=-3) == pkg.EINVAL
    assert call(l=lab.ptr + 2) == pkg.EINVAL and call(c=comp.ptr + 1) == pkg.EINVAL and call(o=out.ptr + 2) == pkg.EINVAL
    assert call(o=lab.ptr) == pkg.EINVAL and call(o=lab.ptr + 4 * (count - 1), batch=1) == pkg.EINVAL, "labels_out overlaps labels"
    assert call(o=lab.ptr + 4 * count, batch=1, mr=0, rg=None, c=None) == pkg.OK, "the half behind a one-image call does not"
    ctx.sync()
    assert (lab.download((2 * count,), np.int32)[count:] == 0).all() and n.download((2,), np.int32).tolist() == [1, int(SENT)]
    n.upload(np.full(2, SENT, np.int32))
    lab.upload(np.zeros(2 * count, np.int32))
    assert call(l=lab.ptr + 4) == pkg.EINVAL and "components labels" in ctx.last_error(), "an interior pointer: one element short"
    assert call(c=comp.ptr + 4) == pkg.EINVAL and "components comp" in ctx.last_error()
    assert call(o=out.ptr + 4) == pkg.EINVAL and "components labels_out" in ctx.last_error()
    assert call(mr=5) == pkg.EINVAL and "components regions" in ctx.last_error()
    assert call(nn=n.ptr + 4) == pkg.EINVAL and "components n_regions" in ctx.last_error()
    assert call(batch=3, r=2, cl=2) == pkg.EINVAL, "a batch beyond the handle"
    assert call(batch=1, r=11, cl=11) == pkg.EINVAL, "more pixels than the handle holds"
    assert call(batch=1, r=1 << 14, cl=1 << 15) == pkg.EUNSUPPORTED and call(mr=(1 << 24) + 1) == pkg.EUNSUPPORTED
    r = pkg.RaggedReadout(ctx, 4)

    def ragged(hh=h.h, rr=r.h, l=lab.ptr, nn=n.ptr, conn=8, o=out.ptr):
        return lib.mbn_components_ragged_i32(hh, rr, comp.ptr, reg.ptr, nn, o, l, 3, conn, 1, IGNORE, 4, None)

    assert ragged() == pkg.EINVAL, "a handle without a set"
    assert ragged(rr=None) == pkg.EINVAL and ragged(hh=None) == pkg.EINVAL
    r.set(1, 1, 5, [(2, 4, 5), (60, 5, 8)])
    assert ragged(l=None) == pkg.EINVAL and ragged(nn=None) == pkg.EINVAL and ragged(conn=6) == pkg.EINVAL and ragged(o=lab.ptr + 8) == pkg.EINVAL
    assert ragged(l=lab.ptr + 4 * 21) == pkg.EINVAL and "components labels" in ctx.last_error()      # the set reaches element 100 of 120
    r.set(1, 1, 5, [(0, 4, 5), (20, 4, 5), (40, 4, 5)])
    assert ragged() == pkg.EINVAL, "a set of more maps than the handle holds"
    r.set(1, 1, 5, [(0, 11, 11)])
    assert ragged() == pkg.EINVAL, "a set of more pixels than the handle holds"
    created = C.c_void_p()
    assert lib.mbn_components_create(ctx.h, 0, 10, C.byref(created)) == pkg.EINVAL and lib.mbn_components_create(ctx.h, 1, 0, C.byref(created)) == pkg.EINVAL
    assert lib.mbn_components_create(None, 1, 10, C.byref(created)) == pkg.EINVAL and lib.mbn_components_create(ctx.h, 1, 10, None) == pkg.EINVAL
    assert lib.mbn_components_create(ctx.h, 65536, 10, C.byref(created)) == pkg.EUNSUPPORTED
    assert lib.mbn_components_create(ctx.h, 1, (1 << 34) + 1, C.byref(created)) == pkg.EUNSUPPORTED and not created.value
    assert lib.mbn_components_destroy(None) == pkg.OK
    ctx.sync()
    for b in (comp, out, reg, n):
        assert (b.download((b.nbytes // 4,), np.int32) == SENT).all(), "a refused call wrote"
    r.close()
    h.close()
    for b in (lab, comp, out, reg, n):
        b.free()


# -------------------------------------------------------------------------------------------------------------------------- the net

ALPHA, CLASSES, ROWS, COLS = 0.5, 21, 64, 96


def test_net_segment_regions(pkg, ctx, tmp_path):
    hw = _weights_os(pkg, tmp_path, ALPHA, ROWS, COLS, CLASSES, 16)
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), 8)
    net.set_input_u8(True)
    rng = np.random.default_rng(6)
    n, sh, sw = 2, 75, 130
    src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
    npix, max_regions = n * sh * sw, 64
    d_src, d_lab, d_pr = ctx.to_device(src), ctx.alloc(4 * (npix + 64)), ctx.alloc(4 * (npix + 64))
    d_comp, d_out = ctx.alloc(4 * (npix + 64)), ctx.alloc(4 * (npix + 64))
    d_reg, d_n = ctx.alloc(32 * n * max_regions), ctx.alloc(4 * n)
    assert ctx.lib.mbn_net_segment_regions(net.h, d_lab.ptr, d_comp.ptr, d_reg.ptr, d_n.ptr, d_out.ptr, 4, 1, IGNORE, max_regions) == pkg.EINVAL, \
        "before any segment call"

    def check(what, conn, min_area, items):
        for b in (d_comp, d_out):
            b.upload(np.full(npix + 64, SENT, np.int32))
        d_reg.upload(np.full(8 * n * max_regions, SENT, np.int32))
        net.segment_regions(d_lab.ptr, d_n.ptr, comp_ptr=d_comp.ptr, regions_ptr=d_reg.ptr, labels_out_ptr=d_out.ptr, connectivity=conn,
                            min_area=min_area, ignore_label=IGNORE, max_regions=max_regions)
        ctx.sync()
        lab, comp, out = (b.download((npix + 64,), np.int32) for b in (d_lab, d_comp, d_out))
        reg, cnt = d_reg.download((n, max_regions, 8), np.int32), d_n.download((n,), np.int32)
        inside = np.zeros(npix + 64, bool)
        for i, (off, rows, cols) in enumerate(items):
            inside[off:off + rows * cols] = True
            w = R.components(lab[off:off + rows * cols].reshape(rows, cols), CLASSES, conn, min_area, IGNORE)
            k = min(len(w[1]), max_regions)
            assert cnt[i] == len(w[1]) and np.array_equal(reg[i, :k], w[1][:k]) and (reg[i, k:] == SENT).all(), what
            assert np.array_equal(comp[off:off + rows * cols].reshape(rows, cols), w[0]), what
            assert np.array_equal(out[off:off + rows * cols].reshape(rows, cols), w[2]), what
        assert (comp[~inside] == SENT).all() and (out[~inside] == SENT).all(), what
        return cnt

    net.segment_fit(d_src.ptr, n, sh, sw, pkg.FIT_PAD, d_lab.ptr)
    cnt = check("segment_fit", 4, 1, [(i * sh * sw, sh, sw) for i in range(n)])
    assert (cnt > 1).all(), "the tiny net's maps have more than one region"
    check("segment_fit, cleaned", 8, 20, [(i * sh * sw, sh, sw) for i in range(n)])
    # an image call: the regions of the net's own ragged set, at the labels' offsets; with a threshold about half of the pixels abstain
    rows, cols = [sh, 40], [sw, 50]
    offs, dst = [0, sh * sw * 3], [sh * sw + 11, 3]
    ctx.lib.mbn_memset(ctx.h, d_lab.ptr, 0xFF, 4 * (npix + 64))
    net.segment_prob_images_fit(d_src.ptr, offs, rows, cols, pkg.FIT_PAD, d_lab.ptr, dst, d_pr.ptr)
    ctx.sync()
    prob = d_pr.download((npix + 64,), np.float32)
    min_prob = float(np.median(np.concatenate([prob[dst[i]:dst[i] + rows[i] * cols[i]] for i in range(2)])))
    net.segment_prob_images_fit(d_src.ptr, offs, rows, cols, pkg.FIT_PAD, d_lab.ptr, dst, d_pr.ptr, min_prob=min_prob, ignore_label=IGNORE)
    check("segment_prob_images_fit", 8, 1, [(dst[i], rows[i], cols[i]) for i in range(2)])
    check("segment_prob_images_fit, cleaned", 4, 6, [(dst[i], rows[i], cols[i]) for i in range(2)])
    net.destroy()
    for b in (d_src, d_lab, d_pr, d_comp, d_out, d_reg, d_n):
        b.free()
    hw.free()


# --------------------------------------------------------------------------------------------------------------------- the C host

def _pgm(path):
    raw = open(path, "rb").read()
    m = re.match(rb"P5\n(\d+) (\d+)\n(\d+)\n", raw)
    w, h, maxval = (int(g) for g in m.groups())
    return np.frombuffer(raw[m.end():], ">u2" if maxval > 255 else np.uint8).astype(np.int32).reshape(h, w)


def _region_lines(out):
    counts = [int(m.group(2)) for m in re.finditer(r"^regions: image (\d+) count (\d+)$", out, re.M)]
    rows = [[int(v) for v in m.groups()] for m in re.finditer(r"^region (\d+) class (\d+) area (\d+) box (\d+) (\d+) (\d+) (\d+)$", out, re.M)]
    return counts, np.array(rows, np.int32).reshape(len(rows), 7)       # i, class, area, min_row, min_col, max_row, max_col


def test_c_host_regions(pkg, ctx, tmp_path):
    exe = os.path.join(pkg.PKG_DIR, "mobilenet")
    assert os.path.exists(exe)
    sh, sw, classes = 75, 130, 1000                             # the host's synthetic weights have 1000 classes
    src = np.random.default_rng(41).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    ppm, plain, clean = str(tmp_path / "a.ppm"), str(tmp_path / "plain.pgm"), str(tmp_path / "clean.pgm")
    assert pkg.load().mbn_write_ppm(ppm.encode(), src.ctypes.data, sw, sh) == 0
    common = [exe, "--synthetic", "3", "--alpha", "0.5", "--res", "%dx%d" % (ROWS, COLS), "--output-stride", "16", "--ppm", ppm, "--fit", "pad"]
    r = subprocess.run(common + ["--segment-source", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "regions:" not in r.stdout, r.stdout + r.stderr
    L = _pgm(plain)
    # the regions of the map as it is: the written map is the plain one
    r = subprocess.run(common + ["--segment-source", clean, "--regions", "--max-regions", "100000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    counts, rows = _region_lines(r.stdout)
    want = R.components(L, classes, 4, 1, classes)
    assert counts == [len(want[1])] and np.array_equal(rows[:, 0], np.arange(len(rows)))
    assert np.array_equal(rows[:, 1:3], want[1][:, 0:2]) and np.array_equal(rows[:, 3:], want[1][:, 4:])
    assert np.array_equal(_pgm(clean), L)
    # --min-area: the written map is the cleaned one (dropped pixels hold the class count), a short table prints its first records only,
    # and --truth scores the cleaned map: against the plain map every kept pixel agrees and every dropped one abstains
    min_area = max(2, int(np.median(want[1][:, 1])) + 1)        # about half of the regions go
    r = subprocess.run(common + ["--segment-source", clean, "--regions", "--connectivity", "8", "--min-area", str(min_area), "--max-regions", "3",
                                 "--truth", plain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    counts, rows = _region_lines(r.stdout)
    comp, regions, out = R.components(L, classes, 8, min_area, classes)
    assert 0 < len(regions) < len(want[1]) and counts == [len(regions)] and len(rows) == min(3, len(regions))
    assert np.array_equal(rows[:, 1:3], regions[:3][:, 0:2]) and np.array_equal(rows[:, 3:], regions[:3][:, 4:])
    assert np.array_equal(_pgm(clean), out)
    s = {k: float(v) for k, v in (f.split("=") for f in re.search(r"^score: (.*)$", r.stdout, re.M).group(1).split())}
    assert s["pixel_acc"] == int((comp >= 0).sum()) / (sh * sw) and s["abstained"] == int((comp < 0).sum())
    for bad in (["--regions"], ["--segment-source", clean, "--min-area", "3"], ["--segment-source", clean, "--regions", "--connectivity", "6"],
                ["--segment-source", clean, "--regions", "--min-area", "0"], ["--segment-source", clean, "--regions", "--max-regions", "-1"]):
        r = subprocess.run(common + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and "regions:" not in r.stdout, (bad, r.stdout + r.stderr)
