"""Segment with test-time augmentation on the host (no GPU): mbn_fit_view against the rule written out independently and against the rectangles
Pillow pasted into (tests/golden/resize_pillow_views.npz); the identities of the reference the GPU tests compare with (tests/dense_ensemble_ref.py);
mbn_resample_ensemble_envelope and mbn_resample_ensemble_plan through libmbn_host.so; the view form of the resize plan; the struct that must not
move and the new symbols where they belong."""
import ctypes as C
import os

import numpy as np
import pytest

import dense_ensemble_ref as E
import dense_prob_ref
import dense_window_ref
import resize_filters_ref as R
from test_dense_cpu import logits_for

HERE = os.path.dirname(os.path.abspath(__file__))
_FIXTURE = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fixture():
    """tests/golden/resize_pillow_views.npz, read once: [(name, source, (oh, ow), view (x, y, iw, ih, mirror), scale, {filter: canvas})], the fill"""
    if not _FIXTURE:
        z = np.load(os.path.join(HERE, "golden", "resize_pillow_views.npz"))
        _FIXTURE["fill"] = tuple(int(v) for v in z["fill"])
        _FIXTURE["cases"] = [(n, z[n + "_in"], tuple(int(v) for v in z[n + "_canvas"]), tuple(int(v) for v in z[n + "_view"]), float(z[n + "_scale"]),
                              {f: z[n + "_" + R.NAMES[f]] for f in R.FILTERS}) for n in (str(s) for s in z["names"])]
    return _FIXTURE["cases"], _FIXTURE["fill"]


def view_canvas_ref(f, img, oh, ow, view, fill):
    """the normative statement: a canvas of `fill`, the whole image resized into the view's rectangle, mirrored when the view says so"""
    x, y, iw, ih, mirror = view
    out = np.empty((oh, ow, 3), np.uint8)
    out[:] = np.array(fill, np.uint8)
    inner = R.resize(f, img, ih, iw)
    out[y:y + ih, x:x + iw] = inner[:, ::-1] if mirror else inner
    return out


# ------------------------------------------------------------------------------------------------------------------------ fit_view

def test_fixture_is_the_issues_cases():
    cases, fill = fixture()
    assert fill == (128, 7, 255) and len(cases) == 18
    scaled = [c for c in cases if c[4] > 0]
    assert sorted({(c[1].shape[:2], c[2]) for c in scaled}) == [((45, 60), (64, 96)), ((60, 45), (64, 96))]
    assert sorted({(c[4], c[3][4]) for c in scaled}) == [(s, m) for s in (0.5, 0.75, 1.0) for m in (0, 1)] and len(scaled) == 12
    given = {c[0][:-3]: c for c in cases if c[4] == 0 and c[3][4] == 1}
    x, y, iw, ih, _ = given["four_borders_odd_x"][3]
    oh, ow = given["four_borders_odd_x"][2]
    assert x % 2 == 1 and x > 0 and y > 0 and x + iw < ow and y + ih < oh
    assert given["one_column"][3][2] == 1
    up = given["upscale"]
    assert up[3][2] > up[1].shape[1] and up[3][3] > up[1].shape[0]


def test_reference_canvases_equal_pillows():
    """the rule + resize_filters_ref against Pillow's recorded bytes: what the GPU test may use for the images Pillow did not see"""
    cases, fill = fixture()
    for name, img, (oh, ow), view, _, canvases in cases:
        for f in R.FILTERS:
            assert np.array_equal(view_canvas_ref(f, img, oh, ow, view, fill), canvases[f]), (name, R.NAMES[f])


def test_fit_view_against_the_fixture_and_the_rule(pkg):
    cases, _ = fixture()
    for name, img, (oh, ow), view, scale, _ in cases:
        if scale > 0:
            v = pkg.fit_view(img.shape[0], img.shape[1], oh, ow, scale, view[4])
            assert (v.x, v.y, v.iw, v.ih, v.mirror) == view, name
            assert tuple(v.reserved) == (0, 0, 0)
    rng = np.random.default_rng(7)
    for _ in range(4000):
        H, W, oh, ow = (int(v) for v in rng.integers(1, 700, 4))
        scale = float(np.float32(rng.choice([1.0, 0.75, 0.5, 0.25, float(rng.uniform(0.01, 1.0))])))
        mirror = int(rng.integers(0, 2))
        want = E.fit_view(H, W, oh, ow, scale, mirror)
        v = pkg.View()
        rc = pkg.host_lib().mbn_fit_view(H, W, oh, ow, scale, mirror, C.byref(v))
        if want is None:
            assert rc == pkg.EINVAL, (H, W, oh, ow, scale)
        else:
            assert rc == pkg.OK and (v.x, v.y, v.iw, v.ih, v.mirror) == want, (H, W, oh, ow, scale, want)
            assert v.x >= 0 and v.y >= 0 and v.x + v.iw <= ow and v.y + v.ih <= oh


def test_fit_view_scale_1_is_fit_pad_and_the_mirror_keeps_the_rectangle(pkg):
    for H, W, oh, ow in [(45, 60, 64, 96), (60, 45, 64, 96), (33, 100, 32, 32), (375, 500, 224, 224), (64, 96, 64, 96)]:
        assert pkg.fit_view(H, W, oh, ow, 1.0, 0).rect == pkg.fit_pad(H, W, oh, ow)
        for s in (1.0, 0.75, 0.5):
            assert pkg.fit_view(H, W, oh, ow, s, 1).rect == pkg.fit_view(H, W, oh, ow, s, 0).rect
            assert pkg.fit_view(H, W, oh, ow, s, 1).mirror == 1


def test_fit_view_refusals(pkg):
    lib, v = pkg.host_lib(), pkg.View()
    ok = (45, 60, 64, 96)
    assert lib.mbn_fit_view(*ok, 1.0, 0, C.byref(v)) == pkg.OK
    for scale in (0.0, -0.5, 1.5, float(np.nextafter(np.float32(1), np.float32(2))), float("nan"), float("inf")):
        assert lib.mbn_fit_view(*ok, scale, 0, C.byref(v)) == pkg.EINVAL, scale
    for mirror in (2, -1):
        assert lib.mbn_fit_view(*ok, 1.0, mirror, C.byref(v)) == pkg.EINVAL
    assert lib.mbn_fit_view(*ok, 0.005, 0, C.byref(v)) == pkg.EINVAL           # sr = rint(0.32) = 0
    assert lib.mbn_fit_view(*ok, 1.0, 0, None) == pkg.EINVAL
    for bad in [(0, 60, 64, 96), (45, 0, 64, 96), (45, 60, 0, 96), (45, 60, 64, -1)]:
        assert lib.mbn_fit_view(*bad, 1.0, 0, C.byref(v)) == pkg.EINVAL
    assert lib.mbn_fit_view(8192, 1, 32, 32, 1.0, 0, C.byref(v)) == pkg.EINVAL  # an empty inner side, as mbn_fit_pad


def test_view_struct_is_32_bytes(pkg):
    assert C.sizeof(pkg.View) == 32 and pkg.View.mirror.offset == 16 and pkg.View.reserved.offset == 20
    assert pkg.ENSEMBLE_MAX_VIEWS == 8


# -------------------------------------------------------------------------------------------------------- the reference's identities

VIEW_FULL = (0, 0, 224, 160, 0)
VIEWS3 = [(0, 0, 224, 160, 0), (28, 20, 168, 120, 0), (56, 40, 112, 80, 1)]


def test_reference_one_view_is_the_window_reference():
    x = logits_for((2, 5, 7, 21, 0), seed=11)
    for view in VIEWS3[:2]:
        lab, sc, prob = E.ensemble(x[None], 160, 224, [view], 37, 61)
        want_lab, want_sc = dense_window_ref.resample_argmax_window(x, 160, 224, view[:4], 37, 61)
        assert np.array_equal(lab, want_lab) and np.array_equal(_bits(sc), _bits(want_sc))
        assert np.array_equal(prob, dense_prob_ref.resample_softmax_window(x, 160, 224, view[:4], 37, 61)[2])
    # a mirrored view is the window reference read from right to left
    lab, sc, _ = E.ensemble(x[None], 160, 224, [VIEWS3[2]], 37, 61)
    want_lab, want_sc = dense_window_ref.resample_argmax_window(x, 160, 224, VIEWS3[2][:4], 37, 61)
    assert np.array_equal(lab, want_lab[:, :, ::-1]) and np.array_equal(_bits(sc), _bits(want_sc[:, :, ::-1]))


@pytest.mark.parametrize("copies", [2, 4])
def test_reference_copies_of_one_view_are_that_view(copies):
    """v + v and its product by 1/2 are exact, and so are ((v + v) + v) + v ... no: 3 v rounds; 2 and 4 copies are sums of powers of two times v"""
    x = logits_for((1, 5, 7, 21, 0), seed=12)
    view = VIEWS3[1]
    lab, sc, prob = E.ensemble(np.stack([x] * copies), 160, 224, [view] * copies, 45, 70)
    want_lab, want_sc, want_prob = E.ensemble(x[None], 160, 224, [view], 45, 70)
    assert np.array_equal(lab, want_lab) and np.array_equal(_bits(sc), _bits(want_sc)) and np.array_equal(prob, want_prob)


def order_input(h=2, w=3, classes=4):
    """three view maps whose sum depends on the order: 1e8, -1e8 and 1 on class 0 (1e8 + 1 rounds to 1e8), small values elsewhere"""
    x = np.full((3, 1, h, w, classes), -5.0, np.float32)
    x[0, ..., 0], x[1, ..., 0], x[2, ..., 0] = 1e8, -1e8, 1.0
    return x


def test_reference_is_sensitive_to_the_view_order():
    x = order_input()
    views = [(0, 0, 96, 64, 0)] * 3
    _, sc, _ = E.ensemble(x, 64, 96, views, 9, 13)
    assert (sc == np.float32(1.0) / np.float32(3.0)).all()                    # (1e8 - 1e8) + 1
    _, sc_perm, _ = E.ensemble(x[[0, 2, 1]], 64, 96, views, 9, 13)
    assert (sc_perm == 0).all()                                               # (1e8 + 1) - 1e8
    assert (_bits(sc) != _bits(sc_perm)).any()


@pytest.mark.parametrize("case", E.THRESHOLD_CASES)
def test_threshold_cases_leave_out_at_most_one_percent(case):
    n, h, w, classes, views, H, W, _, _, min_prob = case
    _, _, prob = E.ensemble(E.threshold_input(case), 32 * h, 32 * w, views, H, W)
    out = dense_prob_ref.excluded(prob, min_prob, classes)
    assert out.mean() <= 0.01, out.mean()
    below = (prob < min_prob).mean()
    assert 0.02 < below < 0.98, below                                         # the threshold cuts through the map


# ------------------------------------------------------------------------------------------------------------------ envelope and plan

def test_envelope_follows_the_window_envelope_of_every_view(pkg):
    h, w, classes, R, Cc, H, W = 5, 7, 21, 160, 224, 37, 61
    assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, VIEWS3, H, W) == pkg.OK
    for k in range(1, 9):
        assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, [VIEWS3[i % 3] for i in range(k)], H, W) == pkg.OK
    # one bad view refuses the set, wherever it stands
    under_ratio = (0, 0, 224, 160, 0)
    for at in range(3):
        views = list(VIEWS3)
        views[at] = (0, 0, 225, 160, 0)                                        # past the input
        assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, views, H, W) == pkg.EINVAL
        views[at] = (5, 5, 10, 0, 0)                                           # an empty side
        assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, views, H, W) == pkg.EINVAL
        views[at] = (28, 20, 168, 120, 2)                                      # mirror
        assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, views, H, W) == pkg.EINVAL
        views = list(VIEWS3)
        views[at] = under_ratio
        assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, views, 19, 61) == pkg.EUNSUPPORTED      # 19 < 4 * 5 for the full view only
    # an MBN_EINVAL of any view goes before an MBN_EUNSUPPORTED of another
    assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, [under_ratio, (0, 0, 225, 160, 0)], 19, 61) == pkg.EINVAL
    arr = pkg.views(VIEWS3)
    arr[1].reserved[2] = 1
    assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, arr, H, W) == pkg.EINVAL
    # the count, the sizes, the pointer
    for n_views in (0, 9, -1):
        assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, pkg.views([VIEW_FULL] * 9), H, W, n_views=n_views) == pkg.EINVAL
    assert pkg.host_lib().mbn_resample_ensemble_envelope(2, h, w, classes, R, Cc, None, 1, H, W) == pkg.EINVAL
    for bad in [(0, h, w, classes), (2, 0, w, classes), (2, h, 0, classes), (2, h, w, 0)]:
        assert pkg.resample_ensemble_envelope(*bad, R, Cc, VIEWS3, H, W) == pkg.EINVAL
    assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, VIEWS3, 0, W) == pkg.EINVAL
    # the logits hold batch * n_views maps: 65535 at most
    assert pkg.resample_ensemble_envelope(21845, h, w, classes, R, Cc, VIEWS3, H, W) == pkg.OK
    assert pkg.resample_ensemble_envelope(21846, h, w, classes, R, Cc, VIEWS3, H, W) == pkg.EUNSUPPORTED
    assert pkg.resample_ensemble_envelope(2 ** 30, h, w, classes, R, Cc, VIEWS3, H, W) == pkg.EUNSUPPORTED
    # one view: the window envelope's answer
    for rect, Ho, Wo in [((0, 0, 224, 160), 37, 61), ((0, 0, 224, 160), 19, 61), ((7, 5, 204, 151), 45, 70), ((0, 0, 224, 161), 45, 70)]:
        assert pkg.resample_ensemble_envelope(2, h, w, classes, R, Cc, [rect + (0,)], Ho, Wo) == \
            pkg.resample_window_envelope(2, h, w, classes, R, Cc, rect, Ho, Wo)


def _chunk(nv):
    for ch in (128, 64, 32, 16):
        if nv * (ch + 4) * 4 <= 65536:
            return ch
    raise AssertionError(nv)


def test_plan_sweep(pkg):
    """maps 2 x 3 .. 10 x 14 of a 32 h x 32 w input, output = ratio x the map under the full view, K = 1 .. 8 views of shrinking rectangles"""
    seen = set()
    for h, w in [(2, 3), (3, 5), (5, 7), (7, 7), (10, 14)]:
        R, Cc = 32 * h, 32 * w
        for ratio in (4, 5, 8, 11, 16):
            H, W = ratio * h, ratio * w
            for K in range(1, 9):
                views = [(k * Cc // 20, k * R // 20, Cc - k * Cc // 10, R - k * R // 10, k & 1) for k in range(K)]
                assert pkg.resample_ensemble_envelope(1, h, w, 21, R, Cc, views, H, W) == pkg.OK
                l = pkg.resample_ensemble_plan(h, w, R, Cc, views, H, W)
                each = [pkg.resample_window_plan(h, w, R, Cc, v[:4], H, W) for v in views]
                assert (l.fy, l.fx) == (max(p.fy for p in each), max(p.fx for p in each))
                assert l.ch == _chunk(K * l.fy * l.fx)
                assert l.lds_bytes == K * l.fy * l.fx * (l.ch + 4) * 4 and l.lds_bytes <= 65536
                assert l.tiles == each[0].tiles and l.span == H * W
                seen.add(l.ch)
    assert seen == {128, 64, 32, 16}


def test_plan_of_the_largest_staging(pkg):
    """eight views at ratio exactly 4 on a 10 x 14 map: 10 x 10 vectors per view, 16 classes per chunk, 64 000 bytes"""
    h, w, R, Cc, H, W = 10, 14, 320, 448, 20, 28
    views = [(32 * (k % 4) * 2, 32 * (k // 4) * 5, 224, 160, k & 1) for k in range(8)]
    assert all(H * R == 4 * v[3] * h and W * Cc == 4 * v[2] * w for v in views)
    assert pkg.resample_ensemble_envelope(1, h, w, 21, R, Cc, views, H, W) == pkg.OK
    l = pkg.resample_ensemble_plan(h, w, R, Cc, views, H, W)
    assert (l.fy, l.fx, l.ch, l.lds_bytes) == (10, 10, 16, 64000)
    # one view of the same kind keeps 128 classes per chunk
    l = pkg.resample_ensemble_plan(h, w, R, Cc, views[:1], H, W)
    assert (l.fy, l.fx, l.ch, l.lds_bytes) == (10, 10, 128, 52800)
    lib, rec = pkg.host_lib(), pkg.ResampleLaunch()
    assert lib.mbn_resample_ensemble_plan(h, w, R, Cc, pkg.views(views), 0, H, W, C.byref(rec)) == pkg.EINVAL
    assert lib.mbn_resample_ensemble_plan(h, w, R, Cc, pkg.views(views), 9, H, W, C.byref(rec)) == pkg.EINVAL
    assert lib.mbn_resample_ensemble_plan(h, w, R, Cc, None, 1, H, W, C.byref(rec)) == pkg.EINVAL
    assert lib.mbn_resample_ensemble_plan(h, w, R, Cc, pkg.views(views), 8, H, W, None) == pkg.EINVAL


# ------------------------------------------------------------------------------------------------------------- the view resize plan

def test_view_table_plan_is_the_plan_of_the_inner_resize(pkg):
    lib = pkg.host_lib()
    cases, _ = fixture()
    for name, img, (oh, ow), view, _, _ in cases:
        H, W = img.shape[:2]
        x, y, iw, ih, _ = view
        for f in R.FILTERS:
            p = pkg.ResizePadPlan()
            assert lib.mbn_resize_view_table_plan_filter(f, H, W, oh, ow, pkg.views([view]), C.byref(p)) == pkg.OK, name
            inner = pkg.resize_table_plan(H, W, ih, iw, filter=f)
            assert bytes(p.plan) == bytes(inner) and (p.x, p.y, p.iw, p.ih) == (x, y, iw, ih)
            assert p.fill_rows == (oh if iw < ow else oh - ih) and p.fill_wgs == (p.fill_rows + 31) // 32
    # fit_pad's rectangle: the letterbox's own plan
    p, q = pkg.ResizePadPlan(), pkg.resize_pad_table_plan(45, 60, 64, 96)
    assert lib.mbn_resize_view_table_plan_filter(R.BILINEAR, 45, 60, 64, 96, pkg.views([pkg.fit_view(45, 60, 64, 96)]), C.byref(p)) == pkg.OK
    assert bytes(p) == bytes(q)
    for bad in [(-1, 0, 10, 10, 0), (0, -1, 10, 10, 0), (0, 0, 0, 10, 0), (0, 0, 10, 0, 0), (90, 0, 10, 10, 0), (0, 60, 10, 10, 0), (0, 0, 10, 10, 2),
                (0, 0, 10, 10, -1)]:
        assert lib.mbn_resize_view_table_plan_filter(R.BILINEAR, 45, 60, 64, 96, pkg.views([bad]), C.byref(p)) == pkg.EINVAL, bad
    arr = pkg.views([(0, 0, 10, 10, 0)])
    arr[0].reserved[0] = 7
    assert lib.mbn_resize_view_table_plan_filter(R.BILINEAR, 45, 60, 64, 96, arr, C.byref(p)) == pkg.EINVAL
    assert lib.mbn_resize_view_table_plan_filter(R.BILINEAR, 45, 60, 64, 96, None, C.byref(p)) == pkg.EINVAL
    assert lib.mbn_resize_view_table_plan_filter(9, 45, 60, 64, 96, pkg.views([(0, 0, 10, 10, 0)]), C.byref(p)) == pkg.EINVAL
    # the envelope of the inner size: a 100x downscale of a column
    assert lib.mbn_resize_view_table_plan_filter(R.BILINEAR, 8000, 60, 64, 96, pkg.views([(0, 0, 10, 10, 0)]), C.byref(p)) == pkg.EUNSUPPORTED


def test_new_symbols_where_they_belong(pkg):
    lib, host = pkg.load(), pkg.host_lib()
    names = pkg.declared_symbols()
    for n in ("mbn_fit_view", "mbn_resizer_create_view", "mbn_resample_ensemble_f32", "mbn_net_resize_views", "mbn_net_segment_views_fit"):
        assert n in names and hasattr(lib, n), n
    for n in ("mbn_fit_view", "mbn_resample_ensemble_envelope", "mbn_resample_ensemble_plan", "mbn_resize_view_table_plan_filter"):
        assert hasattr(host, n) and hasattr(lib, n), n
    for n in ("mbn_resample_ensemble_f32", "mbn_resizer_create_view", "mbn_net_segment_views_fit"):
        assert not hasattr(host, n), n
