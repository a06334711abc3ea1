/*
 * mbn_similarity.c — the host side of the nearest-neighbour search (include/mbn.h, "Nearest neighbours"): the shapes the kernels of
 * csrc/mbn_f32_similarity.hip and csrc/mbn_bf16_similarity.hip take, the tile they work on and the workspace they need. Plain C, no device call: part of libmbn_host.so.
 */
#include <stddef.h>

#include "mbn.h"
#include "mbn_envelope.h"

int mbn_similarity_envelope(int Q, int G, int D, int k)
{
    if (Q <= 0 || G <= 0 || D <= 0 || k < 1 || k > MBN_SIMILARITY_MAX_K) return MBN_EINVAL;
    if (D % 4 || D < 4 || D > MBN_SIMILARITY_MAX_D) return MBN_EUNSUPPORTED;
    if ((int64_t)Q * D * 4 >= (int64_t)1 << 31) return MBN_EUNSUPPORTED;          /* the queries sit behind one buffer descriptor */
    if ((int64_t)G * D * 4 >= (int64_t)1 << 32) return MBN_EUNSUPPORTED;          /* follow-up: the panels' 64-bit bases already reach further */
    int q_tile, g_tile;                                                           /* the kernel counts its work units in an int */
    (void)mbn_similarity_tile(&q_tile, &g_tile, Q, D);
    if ((int64_t)((Q + q_tile - 1) / q_tile) * ((G + g_tile - 1) / g_tile) >= (int64_t)1 << 31) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_embed_envelope(int N, int D, int dtype)
{
    if (N <= 0 || D <= 0) return MBN_EINVAL;
    if (dtype != MBN_DT_F32 && dtype != MBN_DT_BF16) return MBN_EUNSUPPORTED;     /* MBN_DT_I8 needs the activation scale: a follow-up */
    if (D % 4 || D > MBN_SIMILARITY_MAX_D) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

/* The one place that chooses between the kernel's instantiations. Up to 32 queries are bound by reading the gallery once: one 32-query block,
 * the fewest MFMAs per gallery byte. More queries are bound by MFMA issue: two blocks share every gallery fragment read from LDS. A chunk is one
 * 128-row panel where a row is long (the unit-end merge is small beside D / 2 MFMAs per row block, and 100 000 rows make 782 units for the grid),
 * four panels where it is short. Neither depends on G or on the planning CU count: the workspace layout, and with it every byte, is theirs */
int mbn_similarity_tile(int *q_tile, int *g_tile, int Q, int D)
{
    if (!q_tile || !g_tile || Q <= 0 || D <= 0) return MBN_EINVAL;
    *q_tile = Q <= 32 ? 32 : 64;
    *g_tile = D >= 512 ? 128 : 512;
    return MBN_OK;
}

size_t mbn_similarity_workspace_bytes(int Q, int G, int D, int k)
{
    int q_tile, g_tile;
    if (mbn_similarity_envelope(Q, G, D, k) != MBN_OK || mbn_similarity_tile(&q_tile, &g_tile, Q, D) != MBN_OK) return 0;
    return (size_t)((G + g_tile - 1) / g_tile) * (size_t)Q * (size_t)k * 8;      /* [chunks][Q][k] pairs of (index, score) */
}

/* The bf16 gallery (csrc/mbn_bf16_similarity.hip): queries stay fp32, so their limit is the fp32 search's (the split image, 1.5 times their
 * bytes, sits behind one buffer descriptor of 2^32); a gallery row is D * 2 bytes, read 16 bytes at a time */
int mbn_similarity_envelope_bf16(int Q, int G, int D, int k)
{
    if (Q <= 0 || G <= 0 || D <= 0 || k < 1 || k > MBN_SIMILARITY_MAX_K) return MBN_EINVAL;
    if (D % 8 || D > MBN_SIMILARITY_MAX_D) return MBN_EUNSUPPORTED;
    if ((int64_t)Q * D * 4 >= (int64_t)1 << 31) return MBN_EUNSUPPORTED;
    if ((int64_t)G * D * 2 >= (int64_t)1 << 32) return MBN_EUNSUPPORTED;          /* follow-up, as for fp32 */
    int q_tile, g_tile;
    (void)mbn_similarity_tile_bf16(&q_tile, &g_tile, Q, D);
    if ((int64_t)((Q + q_tile - 1) / q_tile) * ((G + g_tile - 1) / g_tile) >= (int64_t)1 << 31) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_embed_envelope_bf16(int N, int D, int dtype)
{
    if (N <= 0 || D <= 0) return MBN_EINVAL;
    if (dtype != MBN_DT_F32 && dtype != MBN_DT_BF16) return MBN_EUNSUPPORTED;
    if (D % 8 || D > MBN_SIMILARITY_MAX_D) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

/* The tile of the bf16 kernel's instantiations. Up to 32 queries: one 32-query block over four waves of 32 gallery rows, bound by reading the
 * gallery once. More: 64 queries as 2 x 2 waves, a wave owning two gallery row blocks per query fragment. The chunk follows the fp32 search: one
 * 128-row panel where a row is long, four where it is short. Neither depends on G or on the planning CU count */
int mbn_similarity_tile_bf16(int *q_tile, int *g_tile, int Q, int D)
{
    if (!q_tile || !g_tile || Q <= 0 || D <= 0) return MBN_EINVAL;
    *q_tile = Q <= 32 ? 32 : 64;
    *g_tile = D >= 512 ? 128 : 512;
    return MBN_OK;
}

/* the workspace: [chunks][Q][k] pairs of (index, score), then on the next 16 bytes the queries' split image [Q][3][D] bf16 */
size_t mbn_similarity_split_offset_bf16(int Q, int G, int D, int k)
{
    int q_tile, g_tile;
    if (mbn_similarity_envelope_bf16(Q, G, D, k) != MBN_OK || mbn_similarity_tile_bf16(&q_tile, &g_tile, Q, D) != MBN_OK) return 0;
    return ((size_t)((G + g_tile - 1) / g_tile) * (size_t)Q * (size_t)k * 8 + 15) & ~(size_t)15;
}

size_t mbn_similarity_workspace_bytes_bf16(int Q, int G, int D, int k)
{
    const size_t lists = mbn_similarity_split_offset_bf16(Q, G, D, k);
    return lists ? lists + (size_t)Q * 3 * (size_t)D * 2 : 0;
}
