"""Nearest-neighbour search without a device: the envelope and workspace at their edges, refusals that need no device, the symbols in the right
library, and the reference's ranking on a hand-written case."""
import ctypes as C

import numpy as np

import similarity_ref as ref


def test_envelope_and_workspace_edges(pkg):
    env, ws = pkg.similarity_envelope, pkg.similarity_workspace_bytes
    assert env(1, 1, 4, 1) == pkg.OK and env(3, 5, 4096, 8) == pkg.OK
    for bad in ((0, 5, 8, 1), (3, 0, 8, 1), (3, 5, 0, 1), (3, 5, 8, 0), (3, 5, 8, 9), (-1, 5, 8, 1)):
        assert env(*bad) == pkg.EINVAL and ws(*bad) == 0, bad
    for off in ((3, 5, 6, 1), (3, 5, 4100, 1), (3, 5, 2, 1)):
        assert env(*off) == pkg.EUNSUPPORTED and ws(*off) == 0, off
    assert env(2 ** 19 - 1, 5, 1024, 1) == pkg.OK and env(2 ** 19, 5, 1024, 1) == pkg.EUNSUPPORTED          # Q * D * 4 at 2^31
    assert env(1, 2 ** 20 - 1, 1024, 1) == pkg.OK and env(1, 2 ** 20, 1024, 1) == pkg.EUNSUPPORTED          # G * D * 4 at 2^32
    assert env(2 ** 26, 2 ** 20 - 512, 4, 1) == pkg.OK and env(2 ** 26, 2 ** 20, 4, 1) == pkg.EUNSUPPORTED  # 2^20 query tiles x 2^11 chunks: 2^31 units
    for Q, D in ((1, 4), (32, 1024), (33, 1024), (4096, 128)):
        qt, gt = pkg.similarity_tile(Q, D)
        assert qt == (32 if Q <= 32 else 64) and gt % 128 == 0 and (qt, gt) == pkg.similarity_tile(Q, D)
        for G in (1, gt, gt + 1, 3 * gt + 5):
            assert ws(Q, G, D, 5) == -(-G // gt) * Q * 5 * 8
    lib = pkg.host_lib()
    assert lib.mbn_similarity_tile(None, None, 1, 4) == pkg.EINVAL
    assert [lib.mbn_embed_envelope(*a) for a in ((3, 8, pkg.DT_F32), (3, 8, pkg.DT_BF16), (3, 8, pkg.DT_I8), (3, 6, pkg.DT_F32), (0, 8, pkg.DT_F32))] == \
        [pkg.OK, pkg.OK, pkg.EUNSUPPORTED, pkg.EUNSUPPORTED, pkg.EINVAL]


def test_symbols_in_the_right_library(pkg):
    host, full = C.CDLL(pkg.HOST_LIB_PATH), C.CDLL(pkg.LIB_PATH)
    for name in ("mbn_similarity_envelope", "mbn_embed_envelope", "mbn_similarity_tile", "mbn_similarity_workspace_bytes"):
        assert hasattr(host, name) and hasattr(full, name), name
    for name in ("mbn_similarity_topk_f32", "mbn_row_inv_norm_f32", "mbn_embed_rows", "mbn_net_embed", "mbn_net_nearest"):
        assert hasattr(full, name) and not hasattr(host, name), name


def test_reference_ranking_by_hand():
    nan, inf = np.nan, np.inf
    s = np.array([[1.0, 3.0, 3.0, nan, -inf],          # a tie: the lower index first; the NaN never; -inf last
                  [nan, nan, nan, nan, nan],           # nothing to rank
                  [-inf, 2.0, -inf, inf, 2.0]])
    idx, sc = ref.rank(s, 6)                           # G = 5 < k = 6
    assert idx.tolist() == [[1, 2, 0, 4, -1, -1], [-1] * 6, [3, 1, 4, 0, 2, -1]]
    assert sc.tolist() == [[3.0, 3.0, 1.0, -inf, 0.0, 0.0], [0.0] * 6, [inf, 2.0, 2.0, -inf, -inf, 0.0]]
    q, g = np.array([[1, 2, 0, -1]], np.float32), np.array([[1, 1, 1, 1], [0, 4, 0, 0]], np.float32)
    assert ref.scores(q, g, np.float32([0.5]), np.float32([1, -1])).tolist() == [[1.0, -4.0]]
    assert ref.score_bound(q, g).tolist() == [[8 * ref.U * 4, 8 * ref.U * 8]] and ref.inv_norm(np.float32([[3, 4], [0, 0]])).tolist() == [0.2, 0.0]
