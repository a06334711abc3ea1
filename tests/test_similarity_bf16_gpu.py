"""The search on a bf16 gallery on the GPU against tests/similarity_bf16_ref.py: exact cases bit for bit, the header's bound B(D), special values, split independence, the net runner."""
import ctypes as C

import numpy as np
import pytest

import similarity_bf16_ref as ref
from test_dilation_gpu import _weights_os
from test_similarity_gpu import IDX_FILL, SC_FILL, _same, _search as _search_f32

pytestmark = pytest.mark.gpu


class _Bf16:
    """pkg or ctx with the search's two names pointing at their bf16 forms, so test_similarity_gpu's _search (sentinels, launch) drives this kernel."""
    def __init__(self, inner): self.inner = inner
    def __getattr__(self, name): return getattr(self.inner, name + "_bf16" if name in ("similarity_topk", "similarity_workspace_bytes") else name)


def _search(pkg, ctx, q, gb, k, *scales, **launch): return _search_f32(_Bf16(pkg), _Bf16(ctx), q, gb, k, *scales, **launch)


def _packed_case(pkg, ctx, Q=33, k=8, D=1024):
    """Normal fp32 queries and a gallery PACKED ON THE DEVICE from normal fp32 rows: (q, g fp32, gallery bits, k, q inverse norms, packed rows' norms)."""
    rng = np.random.default_rng(11)
    G = 3 * pkg.similarity_tile_bf16(Q, D)[1] + 5
    q, g = (rng.standard_normal((n, D)).astype(np.float32) for n in (Q, G))
    d_q, d_g, d_gb, d_inv = ctx.to_device(q), ctx.to_device(g), ctx.alloc(G * D * 2), ctx.alloc((Q + G) * 4)
    ctx.row_inv_norm(d_inv.ptr, d_q.ptr, Q, D)
    ctx.embed_rows_bf16(d_gb.ptr, d_inv.ptr + Q * 4, d_g.ptr, pkg.DT_F32, G, D)
    ctx.sync()
    inv, gb = d_inv.download((Q + G,), np.float32), d_gb.download((G, D), np.uint16)
    [b.free() for b in (d_q, d_g, d_gb, d_inv)]
    return q, g, gb, k, inv[:Q], inv[Q:]


@pytest.mark.parametrize("name", ref.CASES)
def test_exact(pkg, ctx, name):
    D, Q = ref.CASES[name][:2]
    q, gb, k, ties = ref.exact_case(name, pkg.similarity_tile_bf16(Q, D)[1])
    want, got = ref.rank(ref.scores(q, ref.widen(gb)), k), _search(pkg, ctx, q, gb, k)
    assert np.array_equal(got[0], want[0]), "%s: %d of %d indices differ" % (name, int((got[0] != want[0]).sum()), want[0].size)
    assert _same(got, want), name + ": score bits"
    assert Q == 1 or got[0][0, :min(k, len(ties))].tolist() == ties[:k], "the lowest index wins every tie"
    if name == "tile + rest":                       # once more under powers of two of both signs: still exact, and another order
        scales = np.float32([2.0, -0.5, 0.25])
        qs, gs = scales[np.arange(Q) % 3], scales[np.arange(len(gb)) % 2]
        assert _same(_search(pkg, ctx, q, gb, k, qs, gs), ref.rank(ref.scores(q, ref.widen(gb), qs, gs), k)), name + ": scaled"


def test_bounded(pkg, ctx):
    q, g, gb, k, qs, gs = _packed_case(pkg, ctx)
    D, gw = q.shape[1], ref.widen(gb)
    assert np.array_equal(gb, ref.to_bf16(g)), "the packed bytes are not the rows rounded to nearest even"
    err = np.abs(gs - ref.inv_norm(gw)) / ref.inv_norm(gw)
    print("inverse norm of the packed rows: relative error %.3g of %.3g allowed" % (err.max(), ref.inv_norm_bound(D)))
    assert (err <= ref.inv_norm_bound(D)).all()
    idx, sc = _search(pkg, ctx, q, gb, k, qs, gs)
    s64, bound, rows = ref.scores(q, gw, qs, gs), ref.score_bound(q, gw, qs, gs), np.arange(len(q))[:, None]
    err = np.abs(sc - s64[rows, idx])
    print("score: largest error over its bound %.4f (error %.3g)" % ((err / bound[rows, idx]).max(), err.max()))
    assert (idx >= 0).all() and (err <= bound[rows, idx]).all(), "a score outside the header's bound"
    kth = np.argsort(s64, axis=1)[:, -k][:, None]                                        # the true k-th best: its score and its own bound
    assert (s64[rows, idx] >= s64[rows, kth] - bound[rows, kth] - bound[rows, idx]).all(), "an index that is not among the k best within the two bounds"
    assert all(len(set(r)) == k for r in idx.tolist()), "an index repeated"


def test_special(pkg, ctx):
    inf, rng = np.inf, np.random.default_rng(3)
    q = rng.uniform(0.5, 2.0, (4, 40)).astype(np.float32)                               # every dot positive
    gb = ref.to_bf16(rng.uniform(0.5, 2.0, (7, 40)).astype(np.float32))
    gs = np.float32([1, -inf, 1, -inf, 1, 1, -inf])
    gb[4, 17] = 0x7fc0                                                                  # a NaN gallery row
    want = ref.rank(ref.scores(q, ref.widen(gb), None, gs), 8)                          # G = 7 < k = 8
    got = _search(pkg, ctx, q, gb, 8, None, gs)
    assert np.array_equal(got[0], want[0]) and (got[0][:, 3:6] == [1, 3, 6]).all() and (got[0][:, 6:] == -1).all() and (got[0] != 4).all()
    assert (got[1][:, 3:6] == -inf).all() and (got[1][:, 6:] == 0).all()
    q2 = np.where(np.arange(q.size).reshape(q.shape) == 45, np.float32(np.nan), q)                                                                  # a NaN query row: nothing ranked, the others untouched
    got2 = _search(pkg, ctx, q2, gb, 8, None, gs)
    assert (got2[0][1] == -1).all() and (got2[1][1] == 0).all()
    assert all(np.array_equal(a[[0, 2, 3]].view(np.uint32), b[[0, 2, 3]].view(np.uint32)) for a, b in zip(got2, got))


@pytest.mark.parametrize("case", ["exact", "bounded"])
def test_split_independence(pkg, ctx, case):
    if case == "exact":
        (q, gb, k, _), qs, gs = ref.exact_case("ring wrap", pkg.similarity_tile_bf16(65, 192)[1]), None, None
    else:
        q, _, gb, k, qs, gs = _packed_case(pkg, ctx)
    first = _search(pkg, ctx, q, gb, k, qs, gs)
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
            assert _same(_search(pkg, ctx, q, gb, k, qs, gs), first), "%s: other bytes at %d planning CUs" % (case, cus)
        for rep, got in enumerate(_search(pkg, ctx, q, gb, k, qs, gs, launch=replayed)):
            assert _same(got, first), "%s: other bytes on graph replay %d" % (case, rep)
    finally:
        ctx.set_planning_cus(0)
        assert not g_exec.value or ctx.lib.mbn_graph_destroy(ctx.h, g_exec) == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_net_embed_and_nearest_bf16(pkg, ctx, tmp_path, dtype):
    hw = _weights_os(pkg, tmp_path, 0.25, 32, 32, 10, 32)
    n, k, D = 3, 5, hw.plan.layer[hw.plan.n_layers - 2].out_ch
    net = pkg.Net(ctx, hw.plan, hw.blob.copy(), n)
    net.set_dtype(pkg.DT_BF16 if dtype == "bf16" else pkg.DT_F32)
    rng = np.random.default_rng(9)
    d_img = ctx.to_device(rng.uniform(-1, 1, (n, 32, 32, 3)).astype(np.float32))
    d_emb, d_inv, d_eb, d_ginv = ctx.alloc(n * D * 4), ctx.alloc(n * 4), ctx.alloc(n * D * 2), ctx.alloc(n * 4)
    try:
        net.embed(d_img.ptr, n, d_emb.ptr, d_inv.ptr)
        net.embed(d_img.ptr, n, d_eb.ptr, d_ginv.ptr, gallery_dtype=pkg.DT_BF16)
        ctx.sync()
        emb, inv, eb, ginv = d_emb.download((n, D), np.float32), d_inv.download((n,), np.float32), d_eb.download((n, D), np.uint16), d_ginv.download((n,), np.float32)
        want = ref.inv_norm(ref.widen(eb))
        assert np.array_equal(eb, ref.to_bf16(emb)) and emb.any(1).all() and (np.abs(ginv - want) <= ref.inv_norm_bound(D) * want).all()
        G, own = 40, [7, 17, 27]                    # a gallery that holds the batch's own packed embeddings at these rows
        gb = ref.to_bf16(rng.standard_normal((G, D)).astype(np.float32))
        gb[own] = eb
        g_inv = ref.inv_norm(ref.widen(gb)).astype(np.float32)
        d_g, d_gs = ctx.to_device(gb), ctx.to_device(g_inv)
        outs = [ctx.to_device(np.full(n * k, f, t)) for _ in range(2) for f, t in ((IDX_FILL, np.int32), (SC_FILL, np.float32))]
        net.nearest(d_img.ptr, n, d_g.ptr, G, k, outs[0].ptr, outs[1].ptr, d_gs.ptr, gallery_dtype=pkg.DT_BF16)
        d_ws = ctx.alloc(pkg.similarity_workspace_bytes_bf16(n, G, D, k))
        ctx.similarity_topk_bf16(outs[2].ptr, outs[3].ptr, d_emb.ptr, d_g.ptr, n, G, D, k, d_ws.ptr, d_inv.ptr, d_gs.ptr)
        ctx.sync()
        got, want = ([b.download((n, k), np.uint32) for b in outs[i:i + 2]] for i in (0, 2))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), dtype + ": nearest differs from embed + similarity_topk_bf16"
        # a cosine of 1 within: the score's bound, the two norms' errors, and a row against its rounding (elements move by 2^-9 at most: 1 - cos <= 2^-18)
        bound = ref.score_bound(emb, ref.widen(gb), inv, g_inv)[np.arange(n), own] + 2 * ref.inv_norm_bound(D) + 2.0 ** -18
        assert got[0].view(np.int32)[:, 0].tolist() == own and (np.abs(got[1].view(np.float32)[:, 0] - 1.0) <= bound).all()
        net.set_dtype(pkg.DT_I8)
        assert [ctx.lib.mbn_net_embed_bf16(net.h, d_img.ptr, n, d_eb.ptr, d_inv.ptr),
                ctx.lib.mbn_net_nearest_bf16(net.h, d_img.ptr, n, d_g.ptr, d_gs.ptr, G, k, outs[0].ptr, outs[1].ptr)] == [pkg.EUNSUPPORTED] * 2
        [b.free() for b in [d_g, d_gs, d_ws] + outs]
    finally:
        net.destroy()
        [b.free() for b in (d_img, d_emb, d_inv, d_eb, d_ginv)]
        hw.free()


def test_refusals(pkg, ctx):
    Q, G, D, k = 3, 5, 8, 2
    d_q, d_g, d_ws = ctx.alloc(Q * D * 4 + 16), ctx.alloc(G * D * 2 + 16), ctx.alloc(pkg.similarity_workspace_bytes_bf16(Q, G, D, k) + 16)
    d_idx, d_sc = ctx.to_device(np.full(Q * k, IDX_FILL, np.int32)), ctx.to_device(np.full(Q * k, SC_FILL, np.float32))

    def call(q=d_q.ptr, g=d_g.ptr, ws=d_ws.ptr, idx=d_idx.ptr, D=D, k=k, Q=Q):
        return ctx.lib.mbn_similarity_topk_bf16(ctx.h, idx, d_sc.ptr, q, g, None, None, Q, G, D, k, ws, None)
    assert call(D=4) == pkg.EUNSUPPORTED and call(D=12) == pkg.EUNSUPPORTED and call(k=0) == pkg.EINVAL and call(k=9) == pkg.EINVAL
    assert call(Q=0) == pkg.EINVAL and call(q=d_q.ptr + 4) == pkg.EUNSUPPORTED and call(g=d_g.ptr + 8) == pkg.EUNSUPPORTED
    assert call(ws=d_ws.ptr + 8) == pkg.EUNSUPPORTED and call(idx=d_idx.ptr + 2) == pkg.EINVAL and call(g=None) == pkg.EINVAL and call(ws=None) == pkg.EINVAL
    pack = lambda out, dtype, D: ctx.lib.mbn_embed_rows_bf16(ctx.h, out, None, d_q.ptr, dtype, Q, D, None)
    assert [pack(d_g.ptr, pkg.DT_I8, D), pack(d_g.ptr, pkg.DT_F32, 4), pack(d_g.ptr + 8, pkg.DT_F32, D), pack(None, pkg.DT_F32, D)] == [pkg.EUNSUPPORTED] * 3 + [pkg.EINVAL]
    ctx.sync()
    assert (d_idx.download((Q * k,), np.int32) == IDX_FILL).all() and (d_sc.download((Q * k,), np.float32) == SC_FILL).all()
    [b.free() for b in (d_q, d_g, d_ws, d_idx, d_sc)]
