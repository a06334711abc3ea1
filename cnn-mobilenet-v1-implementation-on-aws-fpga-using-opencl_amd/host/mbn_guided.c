/*
 * mbn_guided.c — the host side of the guided read-out (include/mbn.h, "segment along the image's edges"): the table of range weights and the
 * envelope of the block-mean kernel. Plain C, no device call: part of libmbn_host.so.
 */
#include <math.h>

#include "mbn.h"
#include "mbn_envelope.h"

int mbn_guided_lut(float sigma, float lut[MBN_GUIDED_LUT])
{
    if (!lut || !(sigma > 0.0f) || isinf(sigma)) return MBN_EINVAL;      /* a NaN fails the compare */
    const double two_s2 = 2.0 * (double)sigma * (double)sigma;
    const float floor_w = 0x1p-60f;
    for (int d = 0; d < MBN_GUIDED_LUT; d++) {
        const float g = (float)exp(-(double)d * (double)d / two_s2);     /* one rounding to fp32; d = 0 gives 1 exactly */
        lut[d] = g > floor_w ? g : floor_w;
    }
    return MBN_OK;
}

int mbn_guide_reduce_envelope(int batch, int in_rows, int in_cols, int S)
{
    if (batch <= 0 || in_rows <= 0 || in_cols <= 0 || S < 1 || in_rows % S || in_cols % S) return MBN_EINVAL;
    /* the sizes of the read-out it feeds; a block's sum 255 S^2 stays inside 32 bits */
    if (batch > MBN_DENSE_MAX_BATCH || in_rows > MBN_RESAMPLE_MAX_OUT || in_cols > MBN_RESAMPLE_MAX_OUT || S > 2048) return MBN_EUNSUPPORTED;
    return MBN_OK;
}
