/*
 * mbn_boundary.c — the host side of "score a segmentation at its boundaries" (include/mbn.h): the half-width of an image size, what the device
 * calls accept, the tile and LDS footprint the kernel takes at a half-width, and the boundary IoU of a biou table. Pure C, no HIP:
 * libmbn_host.so carries it.
 */
#include <math.h>
#include <stddef.h>

#include "mbn.h"
#include "mbn_envelope.h"

/* int (round (ratio * diagonal)) of the official boundary IoU: Python's round is to nearest with ties to even, and so is nearbyint under the
 * default rounding mode. The product is formed in double exactly as Python forms it */
int mbn_boundary_d(int rows, int cols, double ratio)
{
    if (rows < 1 || cols < 1 || !(ratio > 0.0 && ratio <= 1.0)) return MBN_EINVAL;
    const double r = nearbyint(ratio * sqrt((double)rows * (double)rows + (double)cols * (double)cols));
    if (r > (double)MBN_BOUNDARY_MAX_D) return MBN_EUNSUPPORTED;
    return r < 1.0 ? 1 : (int)r;
}

int mbn_boundary_envelope(int elem_bytes, int classes, int batch, int rows, int cols, int d, int edge)
{
    if ((elem_bytes != 1 && elem_bytes != 4) || classes < 1 || batch < 1 || rows < 1 || cols < 1 || d < 1 || (edge != 0 && edge != 1))
        return MBN_EINVAL;
    if (d > MBN_BOUNDARY_MAX_D || classes > MBN_CONFUSION_MAX_CLASSES || (int64_t)rows * cols >= MBN_BOUNDARY_MAX_MAP ||
        batch > MBN_BOUNDARY_MAX_BATCH)
        return MBN_EUNSUPPORTED;
    return MBN_OK;
}

/* one switch point between the two half-width classes; within a class the LDS grows with the d rows above and below the tile */
int mbn_boundary_tile(int d, int *tile_rows, int *tile_cols, int *lds_bytes)
{
    if (d < 1) return MBN_EINVAL;
    if (d > MBN_BOUNDARY_MAX_D) return MBN_EUNSUPPORTED;
    const int rows = d <= MBN_BOUNDARY_SMALL_D ? MBN_BOUNDARY_SMALL_ROWS : MBN_BOUNDARY_LARGE_ROWS;
    if (tile_rows) *tile_rows = rows;
    if (tile_cols) *tile_cols = MBN_BOUNDARY_TILE_COLS;
    if (lds_bytes) *lds_bytes = MBN_BOUNDARY_TABLE_BYTES + 2 * (rows + 2 * d) * MBN_BOUNDARY_TILE_COLS * MBN_BOUNDARY_PIXEL_BYTES;
    return MBN_OK;
}

int mbn_boundary_metrics(const uint64_t *biou, int classes, mbn_boundary_metrics_t *m, double *iou)
{
    if (!biou || !m || classes < 1) return MBN_EINVAL;
    if (classes > MBN_CONFUSION_MAX_CLASSES) return MBN_EUNSUPPORTED;
    /* sums of integers in doubles: exact below 2^53 */
    double sum = 0.0, truth_band = 0.0, pred_band = 0.0;
    int present = 0;
    for (int c = 0; c < classes; c++) {
        const double t = (double)biou[3 * (size_t)c], p = (double)biou[3 * (size_t)c + 1], both = (double)biou[3 * (size_t)c + 2];
        const double den = t + p - both;
        const double v = den > 0.0 ? both / den : (double)NAN;
        if (iou) iou[c] = v;
        if (den > 0.0) {
            present++;
            sum += v;
        }
        truth_band += t;
        pred_band += p;
    }
    m->boundary_miou = present ? sum / (double)present : 0.0;
    m->truth_band_pixels = truth_band;
    m->pred_band_pixels = pred_band;
    m->classes_present = present;
    m->reserved = 0;
    return MBN_OK;
}
