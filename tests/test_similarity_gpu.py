"""The nearest-neighbour search on the GPU against tests/similarity_ref.py: indices and score bits EQUAL on exactly summable inputs, the header's
bounds on normal ones, NaN / -inf / short galleries, the same bytes at every planning CU count and on graph replay, the net runner, refusals."""
import ctypes as C

import numpy as np
import pytest

import similarity_ref as ref
from test_dilation_gpu import _weights_os

pytestmark = pytest.mark.gpu

TAIL, IDX_FILL, SC_FILL = 8, -77, 7.25


def _search(pkg, ctx, q, g, k, q_scale=None, g_scale=None, launch=None):
    """(idx [Q][k] int32, score [Q][k] fp32) of the device; the sentinels behind the last row must stay. launch(call): runs call() its own way."""
    (Q, D), G = q.shape, g.shape[0]
    bufs = [ctx.to_device(a) for a in (np.full(Q * k + TAIL, IDX_FILL, np.int32), np.full(Q * k + TAIL, SC_FILL, np.float32), q, g)]
    d_qs, d_gs = (None if s is None else ctx.to_device(np.asarray(s, np.float32)) for s in (q_scale, g_scale))
    d_ws = ctx.alloc(pkg.similarity_workspace_bytes(Q, G, D, k))
    call = lambda: ctx.similarity_topk(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, Q, G, D, k, d_ws.ptr, d_qs and d_qs.ptr, d_gs and d_gs.ptr)
    outs = []
    for _ in (launch(call) if launch else [call()]):
        ctx.sync()
        idx, sc = bufs[0].download((Q * k + TAIL,), np.int32), bufs[1].download((Q * k + TAIL,), np.float32)
        assert (idx[Q * k:] == IDX_FILL).all() and (sc[Q * k:] == SC_FILL).all(), "written past the last row"
        outs.append((idx[:Q * k].reshape(Q, k), sc[:Q * k].reshape(Q, k)))
        bufs[0].upload(np.full(Q * k + TAIL, IDX_FILL, np.int32)), bufs[1].upload(np.full(Q * k + TAIL, SC_FILL, np.float32))
    [b.free() for b in bufs + [d_ws, d_qs, d_gs] if b is not None]
    return outs if launch else outs[0]


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].astype(np.float32).view(np.uint32))


def _normal_case(pkg, ctx, Q=33, k=8, D=1024):
    rng = np.random.default_rng(11)
    G = 3 * pkg.similarity_tile(Q, D)[1] + 5
    q, g = (rng.standard_normal((n, D)).astype(np.float32) for n in (Q, G))
    q[2] = 0                                        # a zero row: inverse norm 0, every score 0
    d_x, d_inv = ctx.to_device(np.concatenate([q, g])), ctx.alloc((Q + G) * 4)
    ctx.row_inv_norm(d_inv.ptr, d_x.ptr, Q + G, D)
    ctx.sync()
    inv = d_inv.download((Q + G,), np.float32)
    d_x.free(), d_inv.free()
    return q, g, k, inv[:Q], inv[Q:]


@pytest.mark.parametrize("name", ref.CASES)
def test_exact(pkg, ctx, name):
    D, Q = ref.CASES[name][:2]
    q, g, k, ties = ref.exact_case(name, pkg.similarity_tile(Q, D)[1])
    want = ref.rank(ref.scores(q, g), k)
    got = _search(pkg, ctx, q, g, k)
    assert np.array_equal(got[0], want[0]), "%s: %d of %d indices differ" % (name, int((got[0] != want[0]).sum()), want[0].size)
    assert _same(got, want), name + ": score bits"
    assert got[0][0, :min(k, len(ties))].tolist() == ties[:k], "the lowest index wins every tie"
    scales = np.float32([2.0, -0.5, 0.25])          # powers of two: still exact, and another order
    qs, gs = scales[np.arange(Q) % 3], scales[np.arange(len(g)) % 2]
    assert _same(_search(pkg, ctx, q, g, k, qs, gs), ref.rank(ref.scores(q, g, qs, gs), k)), name + ": scaled"


def test_bounded(pkg, ctx):
    q, g, k, qs, gs = _normal_case(pkg, ctx)
    D = q.shape[1]
    for x, inv in ((q, qs), (g, gs)):
        want = ref.inv_norm(x)
        err = np.abs(inv - want) / np.where(want > 0, want, 1.0)
        print("inverse norm: relative error %.3g of %.3g allowed" % (err.max(), ref.inv_norm_bound(D)))
        assert (err <= ref.inv_norm_bound(D)).all() and (inv[want == 0] == 0).all()
    idx, sc = _search(pkg, ctx, q, g, k, qs, gs)
    s64, bound = ref.scores(q, g, qs, gs), ref.score_bound(q, g, qs, gs)
    rows = np.arange(len(q))[:, None]
    err = np.abs(sc - s64[rows, idx])
    print("score: error %.3g where %.3g is the smallest bound of a returned pair" % (err.max(), bound[rows, idx][bound[rows, idx] > 0].min()))
    assert (idx >= 0).all() and (err <= bound[rows, idx]).all(), "a score outside the header's bound"
    kth = np.argsort(s64, axis=1)[:, -k][:, None]                                        # the true k-th best: its score and its own bound
    assert (s64[rows, idx] >= s64[rows, kth] - bound[rows, kth] - bound[rows, idx]).all(), "an index that is not among the k best within the two bounds"
    assert all(len(set(r)) == k for r in idx.tolist()), "an index repeated"
    assert idx[2].tolist() == list(range(k)) and (sc[2] == 0).all(), "a zero row scores 0 everywhere: ranked by index"


def test_special(pkg, ctx):
    nan, inf = np.nan, np.inf
    rng = np.random.default_rng(3)
    q, g = (rng.uniform(0.5, 2.0, (n, 36)).astype(np.float32) for n in (4, 7))          # every dot positive
    gs = np.float32([1, -inf, 1, -inf, 1, 1, -inf])
    g[4, 17] = nan                                                                      # a NaN gallery row
    want = ref.rank(ref.scores(q, g, None, gs), 8)                                      # G = 7 < k = 8
    got = _search(pkg, ctx, q, g, 8, None, gs)
    assert np.array_equal(got[0], want[0]) and (got[0][:, 3:6] == [1, 3, 6]).all() and (got[0][:, 6:] == -1).all() and (got[0] != 4).all()
    assert (got[1][:, 3:6] == -inf).all() and (got[1][:, 6:] == 0).all()
    q2 = q.copy()
    q2[1, 5] = nan                                                                      # a NaN query row: nothing ranked, the others untouched
    got2 = _search(pkg, ctx, q2, g, 8, None, gs)
    assert (got2[0][1] == -1).all() and (got2[1][1] == 0).all()
    assert all(np.array_equal(a[[0, 2, 3]].view(np.uint32), b[[0, 2, 3]].view(np.uint32)) for a, b in zip(got2, got))


@pytest.mark.parametrize("case", ["exact", "bounded"])
def test_split_independence(pkg, ctx, case):
    if case == "exact":
        (q, g, k, _), qs, gs = ref.exact_case("long rows", pkg.similarity_tile(31, 1024)[1]), None, None
    else:
        q, g, k, qs, gs = _normal_case(pkg, ctx)
    first = _search(pkg, ctx, q, g, k, qs, gs)
    g_exec = C.c_void_p()

    def replayed(call):
        assert ctx.lib.mbn_graph_begin(ctx.h, None) == 0
        call()
        assert ctx.lib.mbn_graph_end(ctx.h, None, C.byref(g_exec)) == 0
        for _ in range(2):
            assert ctx.lib.mbn_graph_launch(ctx.h, g_exec, None) == 0
            yield
    try:
        for cus in (1, 3, 8, 0):
            ctx.set_planning_cus(cus)
            assert _same(_search(pkg, ctx, q, g, k, qs, gs), first), "%s: other bytes at %d planning CUs" % (case, cus)
        for rep, got in enumerate(_search(pkg, ctx, q, g, k, qs, gs, launch=replayed)):
            assert _same(got, first), "%s: other bytes on graph replay %d" % (case, rep)
    finally:
        ctx.set_planning_cus(0)
        if g_exec.value:
            assert ctx.lib.mbn_graph_destroy(ctx.h, g_exec) == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_net_embed_and_nearest(pkg, ctx, tmp_path, dtype):
    hw = _weights_os(pkg, tmp_path, 0.25, 32, 32, 10, 32)
    n, k, D = 3, 5, hw.plan.layer[hw.plan.n_layers - 2].out_ch
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_dtype(pkg.DT_BF16 if dtype == "bf16" else pkg.DT_F32)
    rng = np.random.default_rng(9)
    d_img = ctx.to_device(rng.uniform(-1, 1, (n, 32, 32, 3)).astype(np.float32))
    d_emb, d_inv = ctx.alloc(n * D * 4), ctx.alloc(n * 4)
    try:
        net.embed(d_img.ptr, n, d_emb.ptr, d_inv.ptr)
        ctx.sync()
        emb, inv = d_emb.download((n, D), np.float32), d_inv.download((n,), np.float32)
        assert np.isfinite(emb).all() and emb.any(1).all() and (np.abs(inv - ref.inv_norm(emb)) <= ref.inv_norm_bound(D) * ref.inv_norm(emb)).all()
        G = 40                                      # a gallery that holds the batch's own embeddings at rows 7, 17, 27
        g = rng.standard_normal((G, D)).astype(np.float32)
        own = [7, 17, 27]
        g[own] = emb
        g_inv = ref.inv_norm(g).astype(np.float32)
        d_g, d_gs = ctx.to_device(g), ctx.to_device(g_inv)
        outs = [ctx.to_device(np.full(n * k, f, t)) for _ in range(2) for f, t in ((IDX_FILL, np.int32), (SC_FILL, np.float32))]
        net.nearest(d_img.ptr, n, d_g.ptr, G, k, outs[0].ptr, outs[1].ptr, d_gs.ptr)
        d_ws = ctx.alloc(pkg.similarity_workspace_bytes(n, G, D, k))
        ctx.similarity_topk(outs[2].ptr, outs[3].ptr, d_emb.ptr, d_g.ptr, n, G, D, k, d_ws.ptr, d_inv.ptr, d_gs.ptr)
        ctx.sync()
        got, want = ([b.download((n, k), np.uint32) for b in outs[i:i + 2]] for i in (0, 2))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), dtype + ": nearest differs from embed + similarity_topk"
        bound = ref.score_bound(emb, g, inv, g_inv)[np.arange(n), own] + 2 * ref.inv_norm_bound(D)       # the two norms' own errors on a cosine of 1
        assert got[0].view(np.int32)[:, 0].tolist() == own and (np.abs(got[1].view(np.float32)[:, 0] - 1.0) <= bound).all()
        net.set_dtype(pkg.DT_I8)
        assert ctx.lib.mbn_net_embed(net.h, d_img.ptr, n, d_emb.ptr, d_inv.ptr) == pkg.EUNSUPPORTED
        assert ctx.lib.mbn_net_nearest(net.h, d_img.ptr, n, d_g.ptr, d_gs.ptr, G, k, outs[0].ptr, outs[1].ptr) == pkg.EUNSUPPORTED
        [b.free() for b in [d_g, d_gs, d_ws] + outs]
    finally:
        net.destroy()
        [b.free() for b in (d_img, d_emb, d_inv)]
        hw.free()


def test_refusals(pkg, ctx):
    Q, G, D, k = 3, 5, 8, 2
    d_q, d_g, d_ws = ctx.alloc(Q * D * 4 + 16), ctx.alloc(G * D * 4 + 16), ctx.alloc(pkg.similarity_workspace_bytes(Q, G, D, k) + 16)
    d_idx, d_sc = ctx.to_device(np.full(Q * k, IDX_FILL, np.int32)), ctx.to_device(np.full(Q * k, SC_FILL, np.float32))

    def call(q=d_q.ptr, g=d_g.ptr, ws=d_ws.ptr, idx=d_idx.ptr, D=D, k=k, Q=Q):
        return ctx.lib.mbn_similarity_topk_f32(ctx.h, idx, d_sc.ptr, q, g, None, None, Q, G, D, k, ws, None)
    assert call(D=6) == pkg.EUNSUPPORTED and call(k=0) == pkg.EINVAL and call(k=9) == pkg.EINVAL and call(Q=0) == pkg.EINVAL
    assert call(q=d_q.ptr + 4) == pkg.EUNSUPPORTED and call(g=d_g.ptr + 8) == pkg.EUNSUPPORTED and call(ws=d_ws.ptr + 8) == pkg.EUNSUPPORTED
    assert call(idx=d_idx.ptr + 2) == pkg.EINVAL and call(q=None) == pkg.EINVAL and call(ws=None) == pkg.EINVAL
    assert pkg.similarity_envelope(2 ** 19, G, 1024, k) == pkg.EUNSUPPORTED                 # Q * D * 4 at 2^31: nothing allocated
    assert ctx.lib.mbn_embed_rows(ctx.h, d_q.ptr, None, d_g.ptr, pkg.DT_I8, Q, D, None) == pkg.EUNSUPPORTED
    assert ctx.lib.mbn_row_inv_norm_f32(ctx.h, d_sc.ptr, d_q.ptr + 4, Q, D, None) == pkg.EUNSUPPORTED
    ctx.sync()
    assert (d_idx.download((Q * k,), np.int32) == IDX_FILL).all() and (d_sc.download((Q * k,), np.float32) == SC_FILL).all()
    [b.free() for b in (d_q, d_g, d_ws, d_idx, d_sc)]
