/*
 * mbn_resize.c — host side of the resize front-end (include/mbn.h, "resize front-end"): the tap tables of Pillow's 8-bit resize for
 * one axis under each of its filters (the _filter entry points; the older names are their MBN_FILTER_BILINEAR calls), NEAREST's index array,
 * and the box a fit mode selects. Plain C, no device: also in libmbn_host.so (tests/test_resize_cpu.py compares
 * the tables with tests/resize_ref.py as int32, exactly). Behind them the tile plans of both resize kernels (mbn_envelope.h: mbn_resize_window,
 * mbn_resize_table_plan, mbn_resize_ragged_plan, _plan_batch): O(tiles) evaluations of lo / hi and no table (tests/test_resize_cpu.py,
 * tests/test_resize_ragged_cpu.py). The arithmetic of an axis is mbn_resize_axis.h's, shared with the device; what a box and a size must satisfy,
 * and the status codes, are here.
 *
 * The reference has no counterpart: decode_image (MobileNet.c:49-57) reads 224*224*3 raw bytes and nothing resizes them.
 */
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "mbn.h"
#include "mbn_envelope.h"
#include "mbn_resize_axis.h"

#define RESIZE_MAX_TAPS 4096  /* mbn_resize_taps: the longest row of weights it builds (a 2047x downscale; the device takes 67) */

static int filter_ok(int filter)
{
    return filter >= MBN_FILTER_NEAREST && filter <= MBN_FILTER_HAMMING;
}

/* an axis, or a status: the box edges are float32 */
static int axis_make(int filter, int in_size, float b0, float b1, int out_size, mbn_axis *a)
{
    if (!filter_ok(filter) || in_size <= 0 || out_size <= 0) return MBN_EINVAL;
    if (!(b0 >= 0.0f) || !(b1 <= (float)in_size) || !(b1 > b0)) return MBN_EINVAL;      /* a NaN fails every comparison */
    *a = mbn_axis_of_filter(filter, in_size, b0, b1, out_size);
    return MBN_OK;
}

int mbn_resize_ksize_filter(int filter, int in_size, float b0, float b1, int out_size)
{
    mbn_axis a;
    const int rc = axis_make(filter, in_size, b0, b1, out_size, &a);
    if (rc != MBN_OK) return rc;
    if (filter == MBN_FILTER_NEAREST) return 1;              /* one source position per output, whatever the factor */
    if (a.fs > 1.0e6) return MBN_EUNSUPPORTED;
    return (int)ceil(a.support) * 2 + 1;
}

int mbn_resize_ksize(int in_size, float b0, float b1, int out_size)
{
    return mbn_resize_ksize_filter(MBN_FILTER_BILINEAR, in_size, b0, b1, out_size);
}

int mbn_resize_nearest_index(int in_size, float b0, float b1, int out_size, int32_t *index)
{
    mbn_axis a;
    const int rc = axis_make(MBN_FILTER_NEAREST, in_size, b0, b1, out_size, &a);
    if (rc != MBN_OK) return rc;
    if (!index) return MBN_EINVAL;
    double xo = mbn_axis_nearest_start(&a);
    for (int i = 0; i < out_size; i++) {                     /* the sum accumulated: one addition per output */
        index[i] = mbn_axis_nearest_clamp(&a, xo);
        xo += a.scale;
    }
    return MBN_OK;
}

int mbn_resize_taps_filter(int filter, int in_size, float b0, float b1, int out_size, int32_t *first, int32_t *count, int32_t *weights)
{
    if (!first || !count || !weights) return MBN_EINVAL;
    const int ksize = mbn_resize_ksize_filter(filter, in_size, b0, b1, out_size);
    if (ksize < 0) return ksize;
    if (ksize > RESIZE_MAX_TAPS) return MBN_EUNSUPPORTED;
    if (filter == MBN_FILTER_NEAREST) {                      /* as a table: the index, one tap, the whole weight */
        const int rc = mbn_resize_nearest_index(in_size, b0, b1, out_size, first);
        if (rc != MBN_OK) return rc;
        for (int i = 0; i < out_size; i++) { count[i] = 1; weights[i] = 1 << MBN_RESIZE_BITS; }
        return ksize;
    }
    const mbn_axis a = mbn_axis_of_filter(filter, in_size, b0, b1, out_size);
    for (int i = 0; i < out_size; i++) count[i] = mbn_axis_taps(&a, i, ksize, weights + (size_t)i * ksize, &first[i]);
    return ksize;
}

int mbn_resize_taps(int in_size, float b0, float b1, int out_size, int32_t *first, int32_t *count, int32_t *weights)
{
    return mbn_resize_taps_filter(MBN_FILTER_BILINEAR, in_size, b0, b1, out_size, first, count, weights);
}

int mbn_fit_box(int in_rows, int in_cols, int out_rows, int out_cols, int fit, float crop_fraction, float box[4])
{
    if (!box || in_rows <= 0 || in_cols <= 0 || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    const double W = in_cols, H = in_rows;
    if (fit == MBN_FIT_STRETCH || fit == MBN_FIT_PAD) {        /* a letterbox resizes the whole image as well (mbn_fit_pad says where to) */
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

/* PIL.ImageOps.contain + pad, centering (0.5, 0.5) (include/mbn.h): doubles throughout, the quotient formed before the product, rint in the default
 * rounding mode = Python's round (half to even) */
int mbn_fit_pad(int in_rows, int in_cols, int out_rows, int out_cols, int32_t rect[4])
{
    if (!rect || in_rows <= 0 || in_cols <= 0 || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    const double W = in_cols, H = in_rows, ow = out_cols, oh = out_rows;
    const double im_ratio = W / H, dest_ratio = ow / oh;
    double iw = ow, ih = oh, x = 0.0, y = 0.0;
    if (im_ratio != dest_ratio) {
        if (im_ratio > dest_ratio) ih = rint(H / W * ow);
        else iw = rint(W / H * oh);
    }
    if (iw < 1.0 || ih < 1.0 || iw > ow || ih > oh) return MBN_EINVAL;       /* above the canvas: no ratio gives it; the kernels' bounds rest on it */
    if (iw != ow) x = rint((ow - iw) * 0.5);
    else if (ih != oh) y = rint((oh - ih) * 0.5);
    rect[0] = (int32_t)x; rect[1] = (int32_t)y; rect[2] = (int32_t)iw; rect[3] = (int32_t)ih;
    return MBN_OK;
}

/* one view of test-time augmentation (include/mbn.h): mbn_fit_pad into the canvas scaled by `scale`, centred in the canvas itself */
int mbn_fit_view(int in_rows, int in_cols, int out_rows, int out_cols, float scale, int mirror, mbn_view *v)
{
    if (!v || in_rows <= 0 || in_cols <= 0 || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    if (!(scale > 0.0f && scale <= 1.0f) || (mirror != 0 && mirror != 1)) return MBN_EINVAL;                 /* a NaN fails both compares */
    const int sc = (int)rint((double)out_cols * (double)scale), sr = (int)rint((double)out_rows * (double)scale);
    if (sr < 1 || sc < 1) return MBN_EINVAL;
    int32_t rect[4];
    const int rc = mbn_fit_pad(in_rows, in_cols, sr, sc, rect);
    if (rc != MBN_OK) return rc;
    memset(v, 0, sizeof *v);
    v->x = rect[0] + (out_cols - sc) / 2;
    v->y = rect[1] + (out_rows - sr) / 2;
    v->iw = rect[2];
    v->ih = rect[3];
    v->mirror = mirror;
    return MBN_OK;
}

int mbn_resize_envelope_filter(int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols)
{
    if (!filter_ok(filter) || in_rows <= 0 || in_cols <= 0 || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    const float whole[4] = { 0.0f, 0.0f, (float)in_cols, (float)in_rows };
    const float *b = box ? box : whole;
    const int kx = mbn_resize_ksize_filter(filter, in_cols, b[0], b[2], out_cols), ky = mbn_resize_ksize_filter(filter, in_rows, b[1], b[3], out_rows);
    if (kx == MBN_EINVAL || ky == MBN_EINVAL) return MBN_EINVAL;
    if (in_rows > MBN_RESIZE_MAX_IN || in_cols > MBN_RESIZE_MAX_IN || out_rows > MBN_RESIZE_MAX_OUT || out_cols > MBN_RESIZE_MAX_OUT) return MBN_EUNSUPPORTED;
    if (kx < 0 || ky < 0 || kx > MBN_RESIZE_MAX_KSIZE || ky > MBN_RESIZE_MAX_KSIZE) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_resize_envelope(int in_rows, int in_cols, const float *box, int out_rows, int out_cols)
{
    return mbn_resize_envelope_filter(MBN_FILTER_BILINEAR, in_rows, in_cols, box, out_rows, out_cols);
}

/* ---- the tile plans of the two kernels (csrc/mbn_u8_resize.hip, csrc/mbn_u8_resize_ragged.hip). No table is built: a tile's window is the exact lo of
 * its first output and the exact hi of its last one, which the ragged kernel derives again from the same expressions and the table kernel reads from
 * its tables (tests/test_resize_ragged_cpu.py pins the two equal) */

int mbn_resize_window_filter(int filter, int in_size, float b0, float b1, int out_size, int o_first, int o_last, int32_t *lo, int32_t *hi)
{
    mbn_axis a;
    const int rc = axis_make(filter, in_size, b0, b1, out_size, &a);
    if (rc != MBN_OK) return rc;
    if (!lo || !hi || o_first < 0 || o_last < o_first || o_last >= out_size) return MBN_EINVAL;
    if (filter == MBN_FILTER_NEAREST) {                      /* the indices grow with the output: the two edge outputs bound the others */
        *lo = mbn_axis_nearest_index(&a, o_first);
        *hi = mbn_axis_nearest_index(&a, o_last) + 1;
        return MBN_OK;
    }
    int l, h, unused;
    (void)mbn_axis_span(&a, o_first, &l, &unused);
    (void)mbn_axis_span(&a, o_last, &unused, &h);
    *lo = l;
    *hi = h;
    return MBN_OK;
}

int mbn_resize_window(int in_size, float b0, float b1, int out_size, int o_first, int o_last, int32_t *lo, int32_t *hi)
{
    return mbn_resize_window_filter(MBN_FILTER_BILINEAR, in_size, b0, b1, out_size, o_first, o_last, lo, hi);
}

/* most source positions a tile of `t` outputs reaches along an axis: exact at every tile's two edge outputs */
static int axis_most(const mbn_axis *a, int out_size, int t)
{
    int most = 0;
    for (int o = 0; o < out_size; o += t) {
        const int last = (o + t < out_size ? o + t : out_size) - 1;
        int lo, hi, unused;
        (void)mbn_axis_span(a, o, &lo, &unused);
        (void)mbn_axis_span(a, last, &unused, &hi);
        if (hi - lo > most) most = hi - lo;
    }
    return most;
}

/* The tile of a geometry inside mbn_resize_envelope. In front of the staged rows stand the tile's horizontal weights alone (the table kernel), or
 * with all_taps every table of the tile (the ragged kernel: MBN_RESIZE_STAGE_OFF, which grows with the tile's height) */
static int tile_fit(int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, int all_taps, mbn_resize_plan_t *p)
{
    const mbn_axis ax = mbn_axis_of_filter(filter, in_cols, box[0], box[2], out_cols), ay = mbn_axis_of_filter(filter, in_rows, box[1], box[3], out_rows);
    p->kx = mbn_resize_ksize_filter(filter, in_cols, box[0], box[2], out_cols);
    p->ky = mbn_resize_ksize_filter(filter, in_rows, box[1], box[3], out_rows);
    p->tow = MBN_RESIZE_TOW(out_cols);
    p->tiles_x = (out_cols + p->tow - 1) / p->tow;
    if (filter == MBN_FILTER_NEAREST) {
        /* a gather: no weights, no staged rows, no window. The table kernel reads its indices from memory; the ragged kernel forms a tile's
         * tow + toh indices in LDS */
        p->toh = out_rows < MBN_RESIZE_TOH ? out_rows : MBN_RESIZE_TOH;
        p->tiles_y = (out_rows + p->toh - 1) / p->toh;
        p->seg_stride = 0;
        p->stage_off = p->tmp_off = p->lds_bytes = all_taps ? (4 * (p->tow + p->toh) + 15) & ~15 : 0;
        return MBN_OK;
    }
    /* a staged row: the widest tile's segment + kx pixels of slack (the horizontal loop runs kx taps for every column) + 3 (the address's offset in its dword) */
    p->seg_stride = ((axis_most(&ax, out_cols, p->tow) + p->kx) * 3 + 3 + 3) & ~3;
    /* the tallest tile whose tables + 4 staged rows + window fit; one output row reaches at most ky <= 67 source rows (13 KB of window), which always fits */
    for (p->toh = out_rows < MBN_RESIZE_TOH ? out_rows : MBN_RESIZE_TOH;; p->toh--) {
        p->stage_off = all_taps ? MBN_RESIZE_STAGE_OFF(p->tow, p->kx, p->toh, p->ky) : (p->tow * p->kx * 4 + 15) & ~15;
        p->tmp_off = (p->stage_off + MBN_RESIZE_WAVES * p->seg_stride + 15) & ~15;
        p->lds_bytes = p->tmp_off + axis_most(&ay, out_rows, p->toh) * p->tow * 3;
        if (p->lds_bytes <= MBN_RESIZE_LDS || p->toh == 1) break;
    }
    p->tiles_y = (out_rows + p->toh - 1) / p->toh;
    return p->lds_bytes <= MBN_RESIZE_LDS ? MBN_OK : MBN_EUNSUPPORTED;
}

int mbn_resize_table_plan_filter(int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resize_plan_t *plan)
{
    if (!plan) return MBN_EINVAL;
    const int rc = mbn_resize_envelope_filter(filter, in_rows, in_cols, box, out_rows, out_cols);
    if (rc != MBN_OK) return rc;
    const float whole[4] = { 0.0f, 0.0f, (float)in_cols, (float)in_rows };
    return tile_fit(filter, in_rows, in_cols, box ? box : whole, out_rows, out_cols, 0, plan);
}

int mbn_resize_table_plan(int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resize_plan_t *plan)
{
    return mbn_resize_table_plan_filter(MBN_FILTER_BILINEAR, in_rows, in_cols, box, out_rows, out_cols, plan);
}

int mbn_resize_ragged_plan_filter(int filter, const mbn_resize_item *it, int out_rows, int out_cols, mbn_resize_desc *d)
{
    if (!it || !d || it->src_offset < 0 || !filter_ok(filter)) return MBN_EINVAL;
    /* the kernel would have to form their weights with a sin / cos bit-equal to the host's libm, which device math does not promise */
    if (filter == MBN_FILTER_HAMMING || filter == MBN_FILTER_LANCZOS) return MBN_EUNSUPPORTED;
    int rc = mbn_resize_envelope_filter(filter, it->rows, it->cols, it->box, out_rows, out_cols);
    if (rc != MBN_OK) return rc;
    mbn_resize_plan_t p;
    rc = tile_fit(filter, it->rows, it->cols, it->box, out_rows, out_cols, 1, &p);
    memset(d, 0, sizeof *d);
    d->src_offset = it->src_offset;
    d->rows = it->rows;
    d->cols = it->cols;
    memcpy(d->box, it->box, sizeof d->box);
    d->kx = p.kx;
    d->ky = p.ky;
    d->toh = p.toh;
    d->tiles_y = p.tiles_y;
    d->seg_stride = p.seg_stride;
    d->tmp_off = p.tmp_off;
    d->lds_bytes = p.lds_bytes;
    return rc;
}

int mbn_resize_ragged_plan(const mbn_resize_item *it, int out_rows, int out_cols, mbn_resize_desc *d)
{
    return mbn_resize_ragged_plan_filter(MBN_FILTER_BILINEAR, it, out_rows, out_cols, d);
}

int mbn_resize_ragged_plan_batch_filter(int filter, const mbn_resize_item *items, int batch, int out_rows, int out_cols, mbn_resize_desc *desc,
                                        int32_t *total_wgs, int32_t *lds_bytes, int64_t *src_span)
{
    if (!items || !desc || !total_wgs || !lds_bytes || !src_span || batch <= 0) return MBN_EINVAL;
    const int tiles_x = (out_cols + MBN_RESIZE_TOW(out_cols) - 1) / MBN_RESIZE_TOW(out_cols);
    int64_t wgs = 0, span = 0;
    int lds = 0;
    for (int i = 0; i < batch; i++) {
        const int rc = mbn_resize_ragged_plan_filter(filter, &items[i], out_rows, out_cols, &desc[i]);
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

int mbn_resize_ragged_plan_batch(const mbn_resize_item *items, int batch, int out_rows, int out_cols, mbn_resize_desc *desc, int32_t *total_wgs,
                                 int32_t *lds_bytes, int64_t *src_span)
{
    return mbn_resize_ragged_plan_batch_filter(MBN_FILTER_BILINEAR, items, batch, out_rows, out_cols, desc, total_wgs, lds_bytes, src_span);
}

/* ---- the letterbox: the plans above for (H, W) -> (ih, iw), and the border's workgroups (mbn_envelope.h) */

static void pad_border(const int32_t rect[4], int out_rows, int out_cols, int32_t *fill_rows, int32_t *fill_wgs)
{
    *fill_rows = rect[2] < out_cols ? out_rows : out_rows - rect[3];
    *fill_wgs = (*fill_rows + MBN_RESIZE_FILL_ROWS - 1) / MBN_RESIZE_FILL_ROWS;
}

/* the whole image into the rectangle rect of the canvas, which holds it (the callers have checked) */
static int rect_table_plan(int filter, int in_rows, int in_cols, int out_rows, int out_cols, const int32_t rect[4], mbn_resize_pad_plan_t *plan)
{
    if (out_rows > MBN_RESIZE_MAX_OUT || out_cols > MBN_RESIZE_MAX_OUT) return MBN_EUNSUPPORTED;        /* the canvas: a batch of them is grid.y x fill_wgs */
    const int rc = mbn_resize_table_plan_filter(filter, in_rows, in_cols, NULL, rect[3], rect[2], &plan->plan);
    if (rc != MBN_OK) return rc;
    plan->x = rect[0]; plan->y = rect[1]; plan->iw = rect[2]; plan->ih = rect[3];
    pad_border(rect, out_rows, out_cols, &plan->fill_rows, &plan->fill_wgs);
    return MBN_OK;
}

int mbn_resize_pad_table_plan_filter(int filter, int in_rows, int in_cols, int out_rows, int out_cols, mbn_resize_pad_plan_t *plan)
{
    if (!plan || !filter_ok(filter)) return MBN_EINVAL;
    int32_t rect[4];
    const int rc = mbn_fit_pad(in_rows, in_cols, out_rows, out_cols, rect);
    if (rc != MBN_OK) return rc;
    return rect_table_plan(filter, in_rows, in_cols, out_rows, out_cols, rect, plan);
}

int mbn_resize_view_table_plan_filter(int filter, int in_rows, int in_cols, int out_rows, int out_cols, const mbn_view *view,
                                      mbn_resize_pad_plan_t *plan)
{
    if (!plan || !view || !filter_ok(filter) || in_rows <= 0 || in_cols <= 0 || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    if ((view->mirror != 0 && view->mirror != 1) || view->reserved[0] || view->reserved[1] || view->reserved[2]) return MBN_EINVAL;
    if (view->x < 0 || view->y < 0 || view->iw < 1 || view->ih < 1 || (int64_t)view->x + view->iw > out_cols || (int64_t)view->y + view->ih > out_rows)
        return MBN_EINVAL;
    const int32_t rect[4] = { view->x, view->y, view->iw, view->ih };
    return rect_table_plan(filter, in_rows, in_cols, out_rows, out_cols, rect, plan);
}

int mbn_resize_pad_ragged_plan_filter(int filter, const mbn_resize_item *it, int out_rows, int out_cols, mbn_resize_pad_desc *d)
{
    if (!it || !d || !filter_ok(filter)) return MBN_EINVAL;
    if (filter == MBN_FILTER_HAMMING || filter == MBN_FILTER_LANCZOS) return MBN_EUNSUPPORTED;
    /* a pad of a box is not built: the item says the whole image, as mbn_fit_box(MBN_FIT_PAD) gives it */
    if (!(it->box[0] == 0.0f) || !(it->box[1] == 0.0f) || !(it->box[2] == (float)it->cols) || !(it->box[3] == (float)it->rows)) return MBN_EINVAL;
    int32_t rect[4];
    int rc = mbn_fit_pad(it->rows, it->cols, out_rows, out_cols, rect);
    if (rc != MBN_OK) return rc;
    if (out_rows > MBN_RESIZE_MAX_OUT || out_cols > MBN_RESIZE_MAX_OUT) return MBN_EUNSUPPORTED;
    rc = mbn_resize_ragged_plan_filter(filter, it, rect[3], rect[2], &d->img);
    if (rc != MBN_OK) return rc;
    d->x = rect[0]; d->y = rect[1]; d->iw = rect[2]; d->ih = rect[3];
    d->tow = MBN_RESIZE_TOW(d->iw);
    d->tiles_x = (d->iw + d->tow - 1) / d->tow;
    pad_border(rect, out_rows, out_cols, &d->fill_rows, &d->fill_wgs);
    return MBN_OK;
}

int mbn_resize_pad_ragged_plan_batch_filter(int filter, const mbn_resize_item *items, int batch, int out_rows, int out_cols, mbn_resize_pad_desc *desc,
                                            int32_t *total_wgs, int32_t *lds_bytes, int64_t *src_span)
{
    if (!items || !desc || !total_wgs || !lds_bytes || !src_span || batch <= 0) return MBN_EINVAL;
    int64_t wgs = 0, span = 0;
    int lds = 0;
    for (int i = 0; i < batch; i++) {
        const int rc = mbn_resize_pad_ragged_plan_filter(filter, &items[i], out_rows, out_cols, &desc[i]);
        if (rc != MBN_OK) return rc;
        desc[i].img.wg0 = (int32_t)wgs;
        wgs += (int64_t)desc[i].img.tiles_y * desc[i].tiles_x + desc[i].fill_wgs;
        if (wgs > INT32_MAX) return MBN_EUNSUPPORTED;
        const int64_t end = items[i].src_offset + (int64_t)items[i].rows * items[i].cols * 3;
        if (end < items[i].src_offset) return MBN_EINVAL;
        if (end > span) span = end;
        if (desc[i].img.lds_bytes > lds) lds = desc[i].img.lds_bytes;
    }
    *total_wgs = (int32_t)wgs;
    *lds_bytes = lds;
    *src_span = span;
    return MBN_OK;
}
