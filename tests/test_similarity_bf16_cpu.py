"""The search on a bf16 gallery without a device: envelope, tile and workspace at their limits, the ctypes signatures, the reference's rounding against torch's (ties to even
both ways, just off a tie, overflow to infinity, the largest finite value, NaNs, subnormals, zeros, a random block)."""
import ctypes as C

import numpy as np
import pytest
import torch

import similarity_bf16_ref as ref


def test_envelope_tile_and_workspace_limits(pkg):
    env, ws = pkg.similarity_envelope_bf16, pkg.similarity_workspace_bytes_bf16
    assert env(1, 1, 8, 1) == pkg.OK and env(3, 5, 4096, 8) == pkg.OK
    for bad in ((0, 5, 8, 1), (3, 0, 8, 1), (3, 5, 0, 1), (3, 5, 8, 0), (3, 5, 8, 9), (-1, 5, 8, 1)):
        assert env(*bad) == pkg.EINVAL and ws(*bad) == 0, bad
    for off in ((3, 5, 4, 1), (3, 5, 12, 1), (3, 5, 4104, 1)):
        assert env(*off) == pkg.EUNSUPPORTED and ws(*off) == 0, off
    assert env(2 ** 19 - 1, 5, 1024, 1) == pkg.OK and env(2 ** 19, 5, 1024, 1) == pkg.EUNSUPPORTED          # Q * D * 4 at 2^31
    assert env(1, 2 ** 21 - 1, 1024, 1) == pkg.OK and env(1, 2 ** 21, 1024, 1) == pkg.EUNSUPPORTED          # G * D * 2 at 2^32
    assert env(2 ** 25, 2 ** 21 - 512, 8, 1) == pkg.OK and env(2 ** 25, 2 ** 21, 8, 1) == pkg.EUNSUPPORTED  # 2^19 query tiles x 2^12 chunks: 2^31 units
    for Q, D in ((1, 8), (32, 1024), (33, 1024), (4096, 128)):
        qt, gt = pkg.similarity_tile_bf16(Q, D)
        assert qt == (32 if Q <= 32 else 64) and gt % 128 == 0
        assert all(ws(Q, G, D, 5) == -(-(-(-G // gt) * Q * 5 * 8) // 16) * 16 + Q * 3 * D * 2 for G in (1, gt, gt + 1, 3 * gt + 5))
    lib = pkg.host_lib()
    assert lib.mbn_similarity_tile_bf16(None, None, 1, 8) == pkg.EINVAL and lib.mbn_similarity_workspace_bytes_bf16.restype is C.c_size_t
    assert [lib.mbn_embed_envelope_bf16(*a) for a in ((3, 8, pkg.DT_F32), (3, 8, pkg.DT_BF16), (3, 8, pkg.DT_I8), (3, 4, pkg.DT_F32), (0, 8, pkg.DT_F32))] == \
        [pkg.OK, pkg.OK, pkg.EUNSUPPORTED, pkg.EUNSUPPORTED, pkg.EINVAL]


def test_symbols_and_signatures(pkg):
    host, full, lib = C.CDLL(pkg.HOST_LIB_PATH), C.CDLL(pkg.LIB_PATH), pkg.load()
    for name in ("mbn_similarity_envelope_bf16", "mbn_embed_envelope_bf16", "mbn_similarity_tile_bf16", "mbn_similarity_workspace_bytes_bf16"):
        assert hasattr(host, name) and hasattr(full, name), name
    for name, nargs in (("mbn_similarity_topk_bf16", 13), ("mbn_embed_rows_bf16", 8), ("mbn_net_embed_bf16", 5), ("mbn_net_nearest_bf16", 9)):
        assert hasattr(full, name) and not hasattr(host, name) and len(getattr(lib, name).argtypes) == nargs, name


@pytest.mark.parametrize("bits", [0x3f800000, 0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0xbf818000, 0x7f7fffff, 0x7f7f7fff, 0x7f800000,
                                  0x7fc00000, 0x7f800001, 0x00000001, 0x80008000, 0])
def test_reference_rounding_is_torch_rounding(bits):
    x = np.array([bits], np.uint32).view(np.float32)
    got, want = ref.to_bf16(x), torch.tensor(x).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert (np.isnan(ref.widen(got)).all() and np.isnan(ref.widen(want)).all()) if np.isnan(x).all() else np.array_equal(got, want)
    r = np.random.default_rng(bits).standard_normal(256).astype(np.float32)
    assert np.array_equal(ref.to_bf16(r), torch.tensor(r).bfloat16().view(torch.int16).numpy().view(np.uint16))
