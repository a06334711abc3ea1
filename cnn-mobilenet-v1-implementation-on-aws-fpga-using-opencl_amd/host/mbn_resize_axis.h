/*
 * mbn_resize_axis.h — the tap arithmetic of one axis of the resize front-end (include/mbn.h, "resize front-end", is the normative statement),
 * written once for the C host (host/mbn_resize.c: the tables, the windows, the tile plans) and for the device (csrc/mbn_u8_resize_ragged.hip: the
 * taps a workgroup forms for its tile, and mbn_resize_taps_device). Both sides must give the same bits, so everything that decides them is here: the
 * extent in float32 and the rest in double, casts that truncate toward zero, w_0 + w_1 + ... summed in order, and no contraction (the host build,
 * baseline x86-64, has no fused multiply-add; the fp64 division is correctly rounded on both sides). No argument is checked: what a box or a size
 * must satisfy, and the status codes, are mbn_resize.c's. tests/resize_ref.py is the independent numpy statement the two are compared with.
 */
#pragma once
#include <stdint.h>

#include "mbn_envelope.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MBN_AXIS_FN __host__ __device__ __forceinline__
#define MBN_AXIS_EXTENT float                /* the device has no excess precision */
#else
#define MBN_AXIS_FN static inline
#define MBN_AXIS_EXTENT volatile float       /* rounded to float32 whatever the compiler's excess precision */
#endif

#ifdef __clang__
#pragma clang fp contract(off)
#endif

typedef struct mbn_axis {
    double b0, scale, fs;            /* fs = support = max(scale, 1) */
    int in_size;
} mbn_axis;

/* the outputs 0..out_size-1 of an axis take [b0, b1) of in_size source positions */
MBN_AXIS_FN mbn_axis mbn_axis_of(int in_size, float b0, float b1, int out_size)
{
    const MBN_AXIS_EXTENT extent = b1 - b0;  /* the subtraction in float32, everything behind it in double */
    mbn_axis a;
    a.in_size = in_size;
    a.b0 = (double)b0;
    a.scale = (double)extent / (double)out_size;
    a.fs = a.scale < 1.0 ? 1.0 : a.scale;
    return a;
}

/* [lo, hi): the source positions output i reaches; returns its centre. lo and hi grow with i (every floating operation in them is monotonic), so a
 * tile's first and last outputs bound the windows of all of them */
MBN_AXIS_FN double mbn_axis_span(const mbn_axis *a, int i, int *lo, int *hi)
{
    const double center = a->b0 + ((double)i + 0.5) * a->scale;
    const int l = (int)(center - a->fs + 0.5), h = (int)(center + a->fs + 0.5);       /* the casts truncate toward zero */
    *lo = l > 0 ? l : 0;
    *hi = h < a->in_size ? h : a->in_size;
    return center;
}

MBN_AXIS_FN double mbn_axis_weight(const mbn_axis *a, int pos, double center)
{
    double x = ((double)pos - center + 0.5) / a->fs;
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

/* the taps of output i: k[0, ksize) = its MBN_RESIZE_BITS-bit weights, zero padded; *first = its first source position; returns the count (at most
 * ksize). Two passes over the taps, the weight formed again in the second: a lane has no room for 67 doubles, and the same expression gives the
 * same bits */
MBN_AXIS_FN int mbn_axis_taps(const mbn_axis *a, int i, int ksize, int32_t *k, int32_t *first)
{
    int lo, hi;
    const double center = mbn_axis_span(a, i, &lo, &hi);
    int n = hi - lo > 0 ? hi - lo : 0;
    n = n < ksize ? n : ksize;
    double sum = 0.0;
    for (int t = 0; t < n; t++) sum += mbn_axis_weight(a, t + lo, center);     /* w_0 + w_1 + ... in order */
    for (int t = 0; t < n; t++) {
        double w = mbn_axis_weight(a, t + lo, center);
        if (sum != 0.0) w /= sum;
        k[t] = (int32_t)(w * (double)(1 << MBN_RESIZE_BITS) + 0.5);
    }
    for (int t = n; t < ksize; t++) k[t] = 0;
    *first = lo;
    return n;
}
