/*
 * mbn_resize.c — host side of the resize front-end (include/mbn.h, "resize front-end"): the tap tables of Pillow's 8-bit bilinear
 * resize for one axis, and the box a fit mode selects. Plain C, no device: also in libmbn_host.so (tests/test_resize_cpu.py compares
 * the tables with tests/resize_ref.py as int32, exactly). Behind them the planner of the ragged resize (mbn_envelope.h: mbn_resize_window,
 * mbn_resize_ragged_plan, _plan_batch): per image O(tiles) evaluations of lo / hi and no table (tests/test_resize_ragged_cpu.py).
 *
 * The reference has no counterpart: decode_image (MobileNet.c:49-57) reads 224*224*3 raw bytes and nothing resizes them.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "mbn.h"
#include "mbn_envelope.h"

#define RESIZE_BITS 22        /* fractional bits of a weight: 32 - 8 - 2 */
#define RESIZE_MAX_TAPS 4096  /* mbn_resize_taps: the longest row of weights it builds (a 2047x downscale; the device takes 67) */

/* scale of an axis, or a status: the box edges are float32 and their difference is formed in float32 */
static int axis_scale(int in_size, float b0, float b1, int out_size, double *scale)
{
    if (in_size <= 0 || out_size <= 0) return MBN_EINVAL;
    if (!(b0 >= 0.0f) || !(b1 <= (float)in_size) || !(b1 > b0)) return MBN_EINVAL;      /* a NaN fails every comparison */
    const volatile float extent = b1 - b0;         /* volatile: rounded to float32 whatever the compiler's excess precision */
    *scale = (double)extent / out_size;
    return MBN_OK;
}

int mbn_resize_ksize(int in_size, float b0, float b1, int out_size)
{
    double scale;
    const int rc = axis_scale(in_size, b0, b1, out_size, &scale);
    if (rc != MBN_OK) return rc;
    const double fs = scale < 1.0 ? 1.0 : scale;
    if (fs > 1.0e6) return MBN_EUNSUPPORTED;
    return (int)ceil(fs) * 2 + 1;
}

/* [lo, hi): the source positions output i of an axis reaches, and its centre. The ONE host statement of these expressions: the tables below and the
 * ragged planner's tile windows both come from here, and csrc/mbn_u8_resize_ragged.hip restates them for the device (axis_span) */
static double axis_span(int in_size, float b0, double scale, double support, int i, int *lo_out, int *hi_out)
{
    const double center = (double)b0 + (i + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > in_size) hi = in_size;
    *lo_out = lo;
    *hi_out = hi;
    return center;
}

int mbn_resize_taps(int in_size, float b0, float b1, int out_size, int32_t *first, int32_t *count, int32_t *weights)
{
    if (!first || !count || !weights) return MBN_EINVAL;
    const int ksize = mbn_resize_ksize(in_size, b0, b1, out_size);
    if (ksize < 0) return ksize;
    double scale = 1.0;
    (void)axis_scale(in_size, b0, b1, out_size, &scale);
    const double fs = scale < 1.0 ? 1.0 : scale, support = fs;
    if (ksize > RESIZE_MAX_TAPS) return MBN_EUNSUPPORTED;
    double w[RESIZE_MAX_TAPS];
    for (int i = 0; i < out_size; i++) {
        int lo, hi;
        const double center = axis_span(in_size, b0, scale, support, i, &lo, &hi);
        const int n = hi - lo;
        double sum = 0.0;
        for (int t = 0; t < n; t++) {
            double x = (t + lo - center + 0.5) / fs;
            if (x < 0.0) x = -x;
            w[t] = x < 1.0 ? 1.0 - x : 0.0;
            sum += w[t];
        }
        int32_t *k = weights + (size_t)i * ksize;
        for (int t = 0; t < n; t++) {
            if (sum != 0.0) w[t] /= sum;
            k[t] = (int32_t)(w[t] * (double)(1 << RESIZE_BITS) + 0.5);
        }
        for (int t = n > 0 ? n : 0; t < ksize; t++) k[t] = 0;
        first[i] = lo;
        count[i] = n > 0 ? n : 0;
    }
    return ksize;
}

int mbn_fit_box(int in_rows, int in_cols, int out_rows, int out_cols, int fit, float crop_fraction, float box[4])
{
    if (!box || in_rows <= 0 || in_cols <= 0 || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    const double W = in_cols, H = in_rows;
    if (fit == MBN_FIT_STRETCH) {
        box[0] = 0.0f; box[1] = 0.0f; box[2] = (float)in_cols; box[3] = (float)in_rows;
        return MBN_OK;
    }
    if (fit != MBN_FIT_CROP || !(crop_fraction > 0.0f) || !(crop_fraction <= 1.0f)) return MBN_EINVAL;
    const double fitw = H * out_cols / out_rows;
    const double bw = (W < fitw ? W : fitw) * (double)crop_fraction, bh = bw * out_rows / out_cols;
    const double left = (W - bw) / 2, upper = (H - bh) / 2;
    box[0] = (float)left; box[1] = (float)upper; box[2] = (float)(left + bw); box[3] = (float)(upper + bh);
    if (box[0] < 0.0f) box[0] = 0.0f;
    if (box[1] < 0.0f) box[1] = 0.0f;
    if (box[2] > (float)in_cols) box[2] = (float)in_cols;
    if (box[3] > (float)in_rows) box[3] = (float)in_rows;
    return MBN_OK;
}

int mbn_resize_envelope(int in_rows, int in_cols, const float *box, int out_rows, int out_cols)
{
    if (in_rows <= 0 || in_cols <= 0 || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    const float whole[4] = { 0.0f, 0.0f, (float)in_cols, (float)in_rows };
    const float *b = box ? box : whole;
    const int kx = mbn_resize_ksize(in_cols, b[0], b[2], out_cols), ky = mbn_resize_ksize(in_rows, b[1], b[3], out_rows);
    if (kx == MBN_EINVAL || ky == MBN_EINVAL) return MBN_EINVAL;
    if (in_rows > MBN_RESIZE_MAX_IN || in_cols > MBN_RESIZE_MAX_IN || out_rows > MBN_RESIZE_MAX_OUT || out_cols > MBN_RESIZE_MAX_OUT) return MBN_EUNSUPPORTED;
    if (kx < 0 || ky < 0 || kx > MBN_RESIZE_MAX_KSIZE || ky > MBN_RESIZE_MAX_KSIZE) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

/* ---- the ragged resize (csrc/mbn_u8_resize_ragged.hip): what the host plans per image. No table is built: a tile's window is the exact lo of its first
 * output and the exact hi of its last one, which the kernel derives again from the same expressions */

int mbn_resize_window(int in_size, float b0, float b1, int out_size, int o_first, int o_last, int32_t *lo, int32_t *hi)
{
    double scale;
    const int rc = axis_scale(in_size, b0, b1, out_size, &scale);
    if (rc != MBN_OK) return rc;
    if (!lo || !hi || o_first < 0 || o_last < o_first || o_last >= out_size) return MBN_EINVAL;
    const double support = scale < 1.0 ? 1.0 : scale;
    int l, h, unused;
    (void)axis_span(in_size, b0, scale, support, o_first, &l, &unused);
    (void)axis_span(in_size, b0, scale, support, o_last, &unused, &h);
    *lo = l;
    *hi = h;
    return MBN_OK;
}

/* most source positions a tile of `t` outputs reaches along an axis: exact at every tile's two edge outputs */
static int axis_most(int in_size, float b0, double scale, int out_size, int t)
{
    const double support = scale < 1.0 ? 1.0 : scale;
    int most = 0;
    for (int o = 0; o < out_size; o += t) {
        const int last = (o + t < out_size ? o + t : out_size) - 1;
        int lo, hi, unused;
        (void)axis_span(in_size, b0, scale, support, o, &lo, &unused);
        (void)axis_span(in_size, b0, scale, support, last, &unused, &hi);
        if (hi - lo > most) most = hi - lo;
    }
    return most;
}

int mbn_resize_ragged_plan(const mbn_resize_item *it, int out_rows, int out_cols, mbn_resize_desc *d)
{
    if (!it || !d || it->src_offset < 0) return MBN_EINVAL;
    const int rc = mbn_resize_envelope(it->rows, it->cols, it->box, out_rows, out_cols);
    if (rc != MBN_OK) return rc;
    double sx = 1.0, sy = 1.0;
    (void)axis_scale(it->cols, it->box[0], it->box[2], out_cols, &sx);
    (void)axis_scale(it->rows, it->box[1], it->box[3], out_rows, &sy);
    memset(d, 0, sizeof *d);
    d->src_offset = it->src_offset;
    d->rows = it->rows;
    d->cols = it->cols;
    memcpy(d->box, it->box, sizeof d->box);
    d->kx = mbn_resize_ksize(it->cols, it->box[0], it->box[2], out_cols);
    d->ky = mbn_resize_ksize(it->rows, it->box[1], it->box[3], out_rows);
    const int tow = MBN_RESIZE_TOW(out_cols);
    /* a staged row: the widest tile's segment + kx pixels of slack (the horizontal loop runs kx taps for every column) + 3 (the address's offset in its dword) */
    d->seg_stride = ((axis_most(it->cols, it->box[0], sx, out_cols, tow) + d->kx) * 3 + 3 + 3) & ~3;
    /* the tallest tile whose tables + 4 staged rows + window fit; one output row reaches at most ky <= 67 source rows (13 KB of window), which always fits */
    int toh = out_rows < MBN_RESIZE_TOH ? out_rows : MBN_RESIZE_TOH;
    for (;; toh--) {
        d->toh = toh;
        d->tmp_off = (MBN_RESIZE_STAGE_OFF(tow, d->kx, toh, d->ky) + MBN_RESIZE_WAVES * d->seg_stride + 15) & ~15;
        d->lds_bytes = d->tmp_off + axis_most(it->rows, it->box[1], sy, out_rows, toh) * tow * 3;
        if (d->lds_bytes <= MBN_RESIZE_LDS || toh == 1) break;
    }
    if (d->lds_bytes > MBN_RESIZE_LDS) return MBN_EUNSUPPORTED;
    d->tiles_y = (out_rows + toh - 1) / toh;
    return MBN_OK;
}

int mbn_resize_ragged_plan_batch(const mbn_resize_item *items, int batch, int out_rows, int out_cols, mbn_resize_desc *desc, int32_t *total_wgs,
                                 int32_t *lds_bytes, int64_t *src_span)
{
    if (!items || !desc || !total_wgs || !lds_bytes || !src_span || batch <= 0) return MBN_EINVAL;
    const int tiles_x = (out_cols + MBN_RESIZE_TOW(out_cols) - 1) / MBN_RESIZE_TOW(out_cols);
    int64_t wgs = 0, span = 0;
    int lds = 0;
    for (int i = 0; i < batch; i++) {
        const int rc = mbn_resize_ragged_plan(&items[i], out_rows, out_cols, &desc[i]);
        if (rc != MBN_OK) return rc;
        desc[i].wg0 = (int32_t)wgs;
        wgs += (int64_t)desc[i].tiles_y * tiles_x;
        if (wgs > INT32_MAX) return MBN_EUNSUPPORTED;
        const int64_t end = items[i].src_offset + (int64_t)items[i].rows * items[i].cols * 3;
        if (end < items[i].src_offset) return MBN_EINVAL;
        if (end > span) span = end;
        if (desc[i].lds_bytes > lds) lds = desc[i].lds_bytes;
    }
    *total_wgs = (int32_t)wgs;
    *lds_bytes = lds;
    *src_span = span;
    return MBN_OK;
}
