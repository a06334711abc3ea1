/*
 * mbn_regions.c — the host side of "regions of a label map" (include/mbn.h): what mbn_components_i32 accepts, the tile its first kernel works on
 * and the scratch a handle holds. Pure C, no HIP: libmbn_host.so carries it.
 */
#include <stddef.h>

#include "mbn.h"
#include "mbn_envelope.h"

int mbn_components_envelope(int batch, int rows, int cols, int classes, int connectivity, int min_area, int max_regions)
{
    if (batch < 1 || rows < 1 || cols < 1 || classes < 1 || (connectivity != 4 && connectivity != 8) || min_area < 1 || max_regions < 0)
        return MBN_EINVAL;
    /* indices and areas are int32 and a map stays below 2^31 bytes; the batch is bounded like every dense call's */
    if ((int64_t)rows * cols >= MBN_COMPONENTS_MAX_MAP || batch > MBN_DENSE_MAX_BATCH || max_regions > MBN_COMPONENTS_MAX_REGIONS)
        return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_components_tile(int *tile_rows, int *tile_cols)
{
    if (!tile_rows || !tile_cols) return MBN_EINVAL;
    *tile_rows = MBN_COMPONENTS_TILE_ROWS;
    *tile_cols = MBN_COMPONENTS_TILE_COLS;
    return MBN_OK;
}

/* parent and area / rank, one int32 each per pixel, and one int32 per chunk of the scan: an image has at most pixels / CHUNK + 1 chunks.
 * Rounded up to 256 bytes. 0 for arguments mbn_components_create refuses */
int64_t mbn_components_scratch_bytes(int max_batch, int64_t max_pixels)
{
    if (max_batch < 1 || max_pixels < 1 || max_batch > MBN_DENSE_MAX_BATCH || max_pixels > MBN_COMPONENTS_MAX_PIXELS) return 0;
    const int64_t bytes = 8 * max_pixels + 4 * (max_pixels / MBN_COMPONENTS_CHUNK + max_batch);
    return (bytes + 255) / 256 * 256;
}
