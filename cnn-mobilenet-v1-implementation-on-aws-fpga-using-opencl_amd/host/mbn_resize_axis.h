/*
 * mbn_resize_axis.h — the tap arithmetic of one axis of the resize front-end (include/mbn.h, "resize front-end", is the normative statement),
 * written once for the C host (host/mbn_resize.c: the tables, the windows, the tile plans) and for the device (csrc/mbn_u8_resize_ragged.hip: the
 * taps a workgroup forms for its tile, and mbn_resize_taps_device). Both sides must give the same bits, so everything that decides them is here: the
 * extent in float32 and the rest in double, casts that truncate toward zero, w_0 + w_1 + ... summed in order, and no contraction (the host build,
 * baseline x86-64, has no fused multiply-add; the fp64 division is correctly rounded on both sides). No argument is checked: what a box or a size
 * must satisfy, and the status codes, are mbn_resize.c's. tests/resize_ref.py (bilinear) and tests/resize_filters_ref.py (every filter) are the
 * independent numpy statements the two are compared with.
 */
#pragma once
#include <math.h>
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
    double b0, scale, fs;            /* fs = max(scale, 1) */
    double support;                  /* S * fs: S = 0.5 (box), 1 (bilinear, hamming), 2 (bicubic), 3 (lanczos); NEAREST has none (0) */
    int in_size, filter;             /* MBN_FILTER_* */
} mbn_axis;

/* the outputs 0..out_size-1 of an axis take [b0, b1) of in_size source positions under `filter` (one of MBN_FILTER_*: the caller has checked) */
MBN_AXIS_FN mbn_axis mbn_axis_of_filter(int filter, int in_size, float b0, float b1, int out_size)
{
    const MBN_AXIS_EXTENT extent = b1 - b0;  /* the subtraction in float32, everything behind it in double */
    mbn_axis a;
    a.in_size = in_size;
    a.filter = filter;
    a.b0 = (double)b0;
    a.scale = (double)extent / (double)out_size;
    a.fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = filter == MBN_FILTER_BOX ? 0.5 * a.fs : filter == MBN_FILTER_BICUBIC ? 2.0 * a.fs : filter == MBN_FILTER_LANCZOS ? 3.0 * a.fs :
                filter == MBN_FILTER_NEAREST ? 0.0 : a.fs;
    return a;
}

MBN_AXIS_FN mbn_axis mbn_axis_of(int in_size, float b0, float b1, int out_size)
{
    return mbn_axis_of_filter(MBN_FILTER_BILINEAR, in_size, b0, b1, out_size);
}

/* [lo, hi): the source positions output i reaches; returns its centre. lo and hi grow with i (every floating operation in them is monotonic), so a
 * tile's first and last outputs bound the windows of all of them. A convolution filter's axis (not NEAREST) */
MBN_AXIS_FN double mbn_axis_span(const mbn_axis *a, int i, int *lo, int *hi)
{
    const double center = a->b0 + ((double)i + 0.5) * a->scale;
    const int l = (int)(center - a->support + 0.5), h = (int)(center + a->support + 0.5);       /* the casts truncate toward zero */
    *lo = l > 0 ? l : 0;
    *hi = h < a->in_size ? h : a->in_size;
    return center;
}

#define MBN_AXIS_PI 3.14159265358979323846   /* M_PI */

#ifndef __HIP_DEVICE_COMPILE__
static inline double mbn_axis_sinc(double x)
{
    if (x == 0.0) return 1.0;
    x = x * MBN_AXIS_PI;
    return sin(x) / x;
}
#endif

/* Pillow's filter functions, in double. The device forms box, bilinear and bicubic only (plain arithmetic: the same bits as the host); hamming and
 * lanczos need sin / cos bit-equal to the host's libm, which device math does not promise, so no device code evaluates them (the ragged path refuses
 * the two filters) and they are host code only */
MBN_AXIS_FN double mbn_axis_filter(int filter, double x)
{
    switch (filter) {
    case MBN_FILTER_BOX:
        return x > -0.5 && x <= 0.5 ? 1.0 : 0.0;
    case MBN_FILTER_BICUBIC: {
        const double a = -0.5;
        if (x < 0.0) x = -x;
        if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
        if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
        return 0.0;
    }
#ifndef __HIP_DEVICE_COMPILE__
    case MBN_FILTER_HAMMING:
        if (x < 0.0) x = -x;
        if (x == 0.0) return 1.0;
        if (x >= 1.0) return 0.0;
        x = x * MBN_AXIS_PI;
        return sin(x) / x * (0.54 + 0.46 * cos(x));
    case MBN_FILTER_LANCZOS:
        return -3.0 <= x && x < 3.0 ? mbn_axis_sinc(x) * mbn_axis_sinc(x / 3.0) : 0.0;
#endif
    default:
        return 0.0;
    }
}

/* the weight of source position pos. Bilinear divides by fs (its tables are pinned as integers and do not move); every other filter multiplies by
 * the reciprocal 1.0 / fs, a true division formed again at each call: Pillow's own form */
MBN_AXIS_FN double mbn_axis_weight(const mbn_axis *a, int pos, double center)
{
    if (a->filter == MBN_FILTER_BILINEAR) {
        double x = ((double)pos - center + 0.5) / a->fs;
        if (x < 0.0) x = -x;
        return x < 1.0 ? 1.0 - x : 0.0;
    }
    return mbn_axis_filter(a->filter, ((double)pos - center + 0.5) * (1.0 / a->fs));
}

/* the taps of output i: k[0, ksize) = its MBN_RESIZE_BITS-bit weights, zero padded; *first = its first source position; returns the count (at most
 * ksize). Two passes over the taps, the weight formed again in the second: a lane has no room for 67 doubles, and the same expression gives the
 * same bits. A weight below zero (bicubic, lanczos, hamming) rounds away from zero like the others: - 0.5 before the truncating cast */
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
        /* box and bilinear have no weight below zero: where the filter is known when the code is compiled, they keep the one rounding they had */
        const int signed_w = a->filter != MBN_FILTER_BILINEAR && a->filter != MBN_FILTER_BOX;
        k[t] = signed_w && w < 0.0 ? (int32_t)(w * (double)(1 << MBN_RESIZE_BITS) - 0.5) : (int32_t)(w * (double)(1 << MBN_RESIZE_BITS) + 0.5);
    }
    for (int t = n; t < ksize; t++) k[t] = 0;
    *first = lo;
    return n;
}

/* NEAREST (Pillow's scaled-affine path, no convolution): the source position of output i is (int)xo_i with xo_0 = b0 + scale * 0.5 and
 * xo_(i+1) = xo_i + scale, the sum ACCUMULATED: the closed form b0 + scale * (i + 0.5) rounds differently and gives other indices. So output i costs
 * i dependent additions wherever it is formed alone, and no cheaper form gives the same bits. Clamped into the source for memory safety only: for
 * a box inside the image it never leaves it */
MBN_AXIS_FN double mbn_axis_nearest_start(const mbn_axis *a)
{
    return a->b0 + a->scale * 0.5;
}

MBN_AXIS_FN int mbn_axis_nearest_clamp(const mbn_axis *a, double xo)
{
    const int v = xo < 0.0 ? 0 : (int)xo;
    return v < a->in_size ? v : a->in_size - 1;
}

MBN_AXIS_FN int mbn_axis_nearest_index(const mbn_axis *a, int i)
{
    double xo = mbn_axis_nearest_start(a);
    for (int j = 0; j < i; j++) xo += a->scale;
    return mbn_axis_nearest_clamp(a, xo);
}
