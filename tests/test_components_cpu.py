"""Regions of a label map, the host side (no GPU): the two references of tests/components_ref.py against each other on every pattern the GPU tests
use, hand-written cases with their expected tables written out, and the pure host functions of libmbn_host.so (envelope, tile, scratch bytes)."""
import ctypes as C

import numpy as np
import pytest

import components_ref as R

I32_MAX = np.iinfo(np.int32).max


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 9), (7, 1), (9, 13), (40, 40), (33, 37)])
def test_the_two_references_agree(rows, cols):
    for name, classes, L in R.patterns(rows, cols, rows // 2, cols // 2, seed=rows + cols):
        for conn in (4, 8):
            for min_area in (1, 2, 5):
                got = R.components(L, classes, conn, min_area, 255)
                assert _same(got, R.components_flood(L, classes, conn, min_area, 255)), (name, conn, min_area)
                comp, regions, out = got
                assert int((comp >= 0).sum()) == int(regions[:, 1].sum()), "the areas are the pixels of the regions"
                assert (regions[:, 1] >= min_area).all()


def _both(L, classes, conn, min_area=1, ignore_label=255):
    a = R.components(L, classes, conn, min_area, ignore_label)
    assert _same(a, R.components_flood(L, classes, conn, min_area, ignore_label))
    return a


def test_a_diagonal_pair():
    L = np.array([[1, 0], [0, 1]], np.int32)
    comp, regions, _ = _both(L, 2, 4)
    assert comp.tolist() == [[0, 1], [2, 3]]
    assert regions.tolist() == [[1, 1, 0, 0, 0, 0, 0, 0], [0, 1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 1, 0, 1, 0], [1, 1, 1, 1, 1, 1, 1, 1]]
    comp, regions, _ = _both(L, 2, 8)
    assert comp.tolist() == [[0, 1], [1, 0]]
    assert regions.tolist() == [[1, 2, 0, 0, 0, 0, 1, 1], [0, 2, 0, 1, 0, 0, 1, 1]]


def test_a_ring_around_a_hole():
    L = np.array([[2, 2, 2], [2, 0, 2], [2, 2, 2]], np.int32)
    for conn in (4, 8):
        comp, regions, out = _both(L, 3, conn)
        assert comp.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
        assert regions.tolist() == [[2, 8, 0, 0, 0, 0, 2, 2], [0, 1, 1, 1, 1, 1, 1, 1]]
        assert np.array_equal(out, L)


def test_an_abstained_line_cuts_a_class_in_two():
    L = np.ones((3, 5), np.int32)
    L[:, 2] = [255, -1, I32_MAX]                                # three kinds of abstained value: none connects, none is a region
    for conn in (4, 8):
        comp, regions, out = _both(L, 2, conn, min_area=1, ignore_label=7)
        assert comp.tolist() == [[0, 0, -1, 1, 1]] * 3
        assert regions.tolist() == [[1, 6, 0, 0, 0, 0, 2, 1], [1, 6, 0, 3, 0, 3, 2, 4]]
        assert np.array_equal(out, L), "abstained pixels are copied, not replaced"


def test_the_drop_rule_at_the_threshold():
    L = np.array([[0, 0, 0, 1, 1], [2, 2, 2, 2, 2]], np.int32)      # areas 3, 2, 5
    comp, regions, out = _both(L, 3, 4, min_area=3, ignore_label=9)
    assert regions[:, :2].tolist() == [[0, 3], [2, 5]], "area == min_area stays, area == min_area - 1 goes"
    assert comp.tolist() == [[0, 0, 0, -1, -1], [1, 1, 1, 1, 1]], "the survivors are numbered among themselves"
    assert out.tolist() == [[0, 0, 0, 9, 9], [2, 2, 2, 2, 2]]
    comp, regions, out = _both(L, 3, 4, min_area=6, ignore_label=9)
    assert len(regions) == 0 and (comp == -1).all() and (out == 9).all()


def test_a_dropped_region_does_not_merge_its_neighbours():
    L = np.array([[1, 1, 0, 1, 1]], np.int32)
    comp, regions, out = _both(L, 2, 4, min_area=2, ignore_label=255)
    assert comp.tolist() == [[0, 0, -1, 1, 1]] and regions[:, 1].tolist() == [2, 2]
    assert out.tolist() == [[1, 1, 255, 1, 1]]


# ------------------------------------------------------------------------------------------------------------------- libmbn_host.so

def test_envelope_statuses(pkg):
    env = pkg.components_envelope
    assert env(1, 1, 1, 1, 4, 1, 0) == pkg.OK and env(65535, 375, 500, 1000, 8, 50, 1 << 24) == pkg.OK
    for bad in [(0, 4, 4, 2, 4, 1, 0), (1, 0, 4, 2, 4, 1, 0), (1, 4, -1, 2, 4, 1, 0), (1, 4, 4, 0, 4, 1, 0), (1, 4, 4, 2, 4, 0, 0),
                (1, 4, 4, 2, 4, 1, -1)]:
        assert env(*bad) == pkg.EINVAL, bad
    for conn in (0, 1, 5, 6, 7, 9, -4):
        assert env(1, 4, 4, 2, conn, 1, 0) == pkg.EINVAL, conn
    # an image's map stays below 2^31 bytes: 2^29 - 1 pixels is the last size inside
    assert env(1, 1, (1 << 29) - 1, 2, 4, 1, 0) == pkg.OK and env(1, 1 << 14, 1 << 15, 2, 4, 1, 0) == pkg.EUNSUPPORTED
    assert env(1, 1, 1 << 29, 2, 4, 1, 0) == pkg.EUNSUPPORTED and env(1, I32_MAX, I32_MAX, 2, 8, 1, 0) == pkg.EUNSUPPORTED
    assert env(65536, 4, 4, 2, 4, 1, 0) == pkg.EUNSUPPORTED
    assert env(1, 4, 4, 2, 4, 1, (1 << 24) + 1) == pkg.EUNSUPPORTED
    assert env(65536, 4, 4, 2, 6, 1, 0) == pkg.EINVAL and env(1, 1, 1 << 29, 2, 4, 0, 0) == pkg.EINVAL     # a caller error goes before a limit


def test_tile_and_scratch_bytes(pkg):
    tr, tc = pkg.components_tile()
    assert tr >= 2 and tc >= 2 and tc % 64 == 0, "a wave holds whole rows of a tile"
    lib = pkg.host_lib()
    one = C.c_int()
    assert lib.mbn_components_tile(None, C.byref(one)) == pkg.EINVAL and lib.mbn_components_tile(C.byref(one), None) == pkg.EINVAL
    sb = pkg.components_scratch_bytes
    for batch, pixels in [(1, 1), (3, 1000), (32, 32 * 375 * 500), (65535, 1 << 34)]:
        tiles = (pixels + tr * tc - 1) // (tr * tc) + batch
        assert 8 * pixels <= sb(batch, pixels) <= 8 * pixels + 16 * tiles + 256, "8 bytes per pixel and a term per tile"
    assert sb(4, 2000) >= sb(4, 1000) and sb(8, 1000) >= sb(4, 1000)
    for bad in [(0, 10), (-1, 10), (1, 0), (1, -1), (65536, 10), (1, (1 << 34) + 1)]:
        assert sb(*bad) == 0, bad


def test_symbols_and_struct(pkg):
    names = pkg.declared_symbols()
    host, lib = pkg.host_lib(), pkg.load()
    for n in ("mbn_components_envelope", "mbn_components_tile", "mbn_components_scratch_bytes"):
        assert n in names and hasattr(host, n) and hasattr(lib, n), n
    for n in ("mbn_components_create", "mbn_components_destroy", "mbn_components_i32", "mbn_components_ragged_i32", "mbn_net_segment_regions"):
        assert n in names and hasattr(lib, n) and not hasattr(host, n), n
    assert C.sizeof(pkg.Region) == 32 and pkg.REGION_DTYPE.itemsize == 32
    assert [f[0] for f in pkg.Region._fields_] == list(R.FIELDS) == list(pkg.REGION_DTYPE.names)
    for cls, name in ((pkg.Context, "components"), (pkg.Context, "components_ragged"), (pkg.Net, "segment_regions"), (pkg.Components, "close")):
        assert callable(getattr(cls, name))
