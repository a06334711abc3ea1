/* mbn_envelope.c — the shape envelopes of the fused kernels (mbn_envelope.h). The byte bounds are the kernels' 32-bit buffer
 * offsets: tests/test_large_tensors_gpu.py runs each on both sides. */
#include "mbn_envelope.h"
#include "mbn.h"

#include <stddef.h>
#include <stdlib.h>
#include <string.h>

int mbn_block_envelope(const mbn_block_shape *s, int dtype)
{
    const int bf = dtype == MBN_DT_BF16;
    if (!bf && dtype != MBN_DT_F32) return MBN_EUNSUPPORTED;
    if (s->batch <= 0 || (s->stride != 1 && s->stride != 2) || s->cin > MBN_CMAX || s->cout > MBN_COUT_MAX || (s->out_cols & 1) ||
        s->out_rows <= 0 || s->out_cols <= 0 || s->in_rows <= 0 || s->in_cols <= 0 || s->pad_top < 0 || s->pad_left < 0)
        return MBN_EUNSUPPORTED;
    /* fp32: whole 32-channel depthwise chunks, whole 128-column tiles; bf16: whole 64-channel K chunks (or one half chunk, padded),
     * 64-column remainders on a padded tile */
    if (bf ? (s->cin != 32 && (s->cin < 64 || (s->cin % 64) != 0)) || s->cout < 64 || (s->cout % 64) != 0
           : s->cin < 32 || (s->cin % 32) != 0 || s->cout < 128 || (s->cout % 128) != 0)
        return MBN_EUNSUPPORTED;
    const double es = bf ? 2.0 : 4.0;
    if (es * s->batch * s->in_rows * s->in_cols * s->cin >= (double)MBN_OOB) return MBN_EUNSUPPORTED;          /* input offsets below the zero-load offset */
    if ((long)s->batch * s->out_rows * s->out_cols > 0x7fffff00L) return MBN_EUNSUPPORTED;                    /* 32-bit pixel index */
    /* buffer stores; + a row tile of head room: ragged rows must not wrap (32-bit offsets) */
    if (es * ((double)s->batch * s->out_rows * s->out_cols + 256.0) * s->cout >= 4294967296.0) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

/* The range in which csrc/mbn_block_window.h's full-rate offsets equal the general ones:
 *  - every input byte offset PLUS a left-pad column below MBN_OFF_BAD_COL: a left-pad tap of image 0 / row 0 has base = -pad_left * (pixel
 *    stride), and its sum with MBN_OFF_BAD_COL must stay beyond num_records without wrapping into the descriptor's range;
 *  - (image * in_rows + row) in __mul24 range, in_cols in its 16-bit factor;
 *  - the float-reciprocal row / image quotients exact: out_cols, out_rows < 2^15;
 *  - at most one pad column on the left (the term above counts one). */
int mbn_block_fast_offsets(const mbn_block_shape *s, int dtype)
{
    const double es = dtype == MBN_DT_BF16 ? 2.0 : 4.0;
    if (es * s->batch * s->in_rows * s->in_cols * s->cin + (s->pad_left + 1) * es * s->cin > (double)MBN_OFF_BAD_COL) return MBN_EUNSUPPORTED;
    if ((double)s->batch * s->in_rows >= 8388000.0 || s->in_cols >= 32768 || s->out_cols >= 32768 || s->out_rows >= 32768 || s->pad_left > 1)
        return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_resident_envelope(const mbn_block_shape *s, int nblocks)
{
    if (s->cin != 256 || s->cout != 256 || s->stride != 1 || s->pad_top != 1 || s->pad_left != 1 || s->in_rows < 1 || s->in_cols < 1 ||
        s->out_rows != s->in_rows || s->out_cols != s->in_cols || nblocks < 1 || nblocks > MBN_RES_MAXBLK)
        return MBN_EUNSUPPORTED;
    if (s->in_rows * s->in_cols > MBN_RES_YROWS || (s->in_rows + 2) * (s->in_cols + 2) > MBN_RES_XPIX) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_tail_envelope(const mbn_block_shape *b0, const mbn_block_shape *b1)
{
    const int h = b0->in_rows, w = b0->in_cols;
    if (b0->cin != 256 || b0->cout != 512 || h < 2 || w < 2 || h > MBN_TAIL_MAXSIDE || w > MBN_TAIL_MAXSIDE || (h & 1) || (w & 1))
        return MBN_EUNSUPPORTED;
    if (b0->stride != 2 || b0->pad_top != 0 || b0->pad_left != 0 || b0->out_rows != h / 2 || b0->out_cols != w / 2) return MBN_EUNSUPPORTED;
    if (b1->batch != b0->batch || b1->cin != b0->cout || b1->cout != b0->cout || b1->stride != 1 || b1->pad_top != 1 || b1->pad_left != 1 ||
        b1->in_rows != b0->out_rows || b1->in_cols != b0->out_cols || b1->out_rows != b1->in_rows || b1->out_cols != b1->in_cols)
        return MBN_EUNSUPPORTED;
    if (2.0 * b0->batch * h * w * b0->cin >= 4294967296.0) return MBN_EUNSUPPORTED;                              /* the input's 32-bit offsets */
    return MBN_OK;
}

int mbn_stem_envelope(int batch, int res, int c1, int c3)
{
    return mbn_stem_envelope_hw(batch, res, res, c1, c3);
}

int mbn_stem_envelope_hw(int batch, int rows, int cols, int c1, int c3)
{
    if (!((c1 == 32 && c3 == 64) || (c1 == 16 && c3 == 32)) || rows < 32 || (rows % 32) != 0 || cols < 32 || (cols % 32) != 0 || batch <= 0)
        return MBN_EUNSUPPORTED;
    if ((long)batch * (rows / 2 / MBN_STEM_TH) * (cols / 2 / MBN_STEM_TW) >= 0x7fffffffL) return MBN_EUNSUPPORTED;   /* 32-bit tile index */
    /* per-image buffer offsets (input loads and output stores) are 32-bit */
    if (4.0 * rows * cols * 3 >= (double)MBN_OOB || 4.0 * (rows / 2) * (cols / 2) * c3 >= 4294967296.0) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_upsample_argmax_envelope(int batch, int rows, int cols, int classes, int factor)
{
    if ((factor != 8 && factor != 16 && factor != 32) || batch <= 0 || batch > MBN_DENSE_MAX_BATCH || rows <= 0 || cols <= 0 || classes <= 0)
        return MBN_EUNSUPPORTED;
    if (4.0 * rows * cols * classes >= 2147483648.0) return MBN_EUNSUPPORTED;                                   /* an image's logits */
    if (4.0 * rows * factor * cols * factor >= 2147483648.0) return MBN_EUNSUPPORTED;                           /* an image's labels / scores */
    /* (both sides of the output map are now below 2^29, so the tile counts are ints) */
    if ((long)MBN_DENSE_TILES(rows, factor) * MBN_DENSE_TILES(cols, factor) > MBN_DENSE_MAX_TILES) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_softmax_readout_check(int have_prob, float min_prob)
{
    if (!(min_prob >= 0.0f && min_prob <= 1.0f)) return MBN_EINVAL;      /* a NaN fails both compares */
    if (!have_prob && min_prob == 0.0f) return MBN_EINVAL;
    return MBN_OK;
}

/* The read-out at any output size has ONE geometry, the window's: the whole map is the window that covers the whole input, rect = (0, 0, cols, rows)
 * of in = (rows, cols). There the ratio test is out >= 4 x coarse and MBN_RESAMPLE_WINDOW_FOOT is MBN_RESAMPLE_FOOT, so the plain functions are the
 * window functions of that rectangle: same status for every argument, same launch (tests/test_dense_window_cpu.py sweeps both). */
int mbn_resample_window_envelope(int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows,
                                 int out_cols)
{
    if (batch <= 0 || rows <= 0 || cols <= 0 || classes <= 0 || in_rows <= 0 || in_cols <= 0 || out_rows <= 0 || out_cols <= 0 || !rect)
        return MBN_EINVAL;
    const int64_t x = rect[0], y = rect[1], iw = rect[2], ih = rect[3];
    if (x < 0 || y < 0 || iw < 1 || ih < 1 || x + iw > in_cols || y + ih > in_rows || in_rows < rows || in_cols < cols) return MBN_EINVAL;
    if (batch > MBN_DENSE_MAX_BATCH || out_rows > MBN_RESAMPLE_MAX_OUT || out_cols > MBN_RESAMPLE_MAX_OUT || in_rows > MBN_RESAMPLE_MAX_OUT ||
        in_cols > MBN_RESAMPLE_MAX_OUT)
        return MBN_EUNSUPPORTED;
    /* the ratio of the output to the coarse samples under the window: N R >= 4 l n */
    if ((int64_t)out_rows * in_rows < MBN_RESAMPLE_MIN_RATIO * ih * rows || (int64_t)out_cols * in_cols < MBN_RESAMPLE_MIN_RATIO * iw * cols)
        return MBN_EUNSUPPORTED;
    if (4.0 * rows * cols * classes >= 2147483648.0) return MBN_EUNSUPPORTED;                                   /* an image's logits */
    if (4.0 * out_rows * out_cols >= 2147483648.0) return MBN_EUNSUPPORTED;                                     /* an image's labels / scores */
    if ((long)((out_rows + MBN_RESAMPLE_TILE - 1) / MBN_RESAMPLE_TILE) * ((out_cols + MBN_RESAMPLE_TILE - 1) / MBN_RESAMPLE_TILE) > MBN_DENSE_MAX_TILES)
        return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_resample_argmax_envelope(int batch, int rows, int cols, int classes, int out_rows, int out_cols)
{
    const int32_t full[4] = { 0, 0, cols, rows };
    return mbn_resample_window_envelope(batch, rows, cols, classes, rows, cols, full, out_rows, out_cols);
}

void mbn_resample_window_plan(int rows, int cols, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols,
                              mbn_resample_launch_t *l)
{
    const int fy = MBN_RESAMPLE_WINDOW_FOOT(rows, out_rows, in_rows, rect[3]), fx = MBN_RESAMPLE_WINDOW_FOOT(cols, out_cols, in_cols, rect[2]);
    const int tiles = ((out_rows + MBN_RESAMPLE_TILE - 1) / MBN_RESAMPLE_TILE) * ((out_cols + MBN_RESAMPLE_TILE - 1) / MBN_RESAMPLE_TILE);
    if (fy > l->fy) l->fy = fy;
    if (fx > l->fx) l->fx = fx;
    if (tiles > l->tiles) l->tiles = tiles;
    if ((int64_t)out_rows * out_cols > l->span) l->span = (int64_t)out_rows * out_cols;
    l->ch = MBN_RESAMPLE_CH(l->fy * l->fx);
    l->lds_bytes = l->fy * l->fx * (l->ch + 4) * 4;
}

void mbn_resample_plan(int rows, int cols, int out_rows, int out_cols, mbn_resample_launch_t *l)
{
    const int32_t full[4] = { 0, 0, cols, rows };
    mbn_resample_window_plan(rows, cols, rows, cols, full, out_rows, out_cols, l);
}

int mbn_resample_ensemble_envelope(int batch, int rows, int cols, int classes, int in_rows, int in_cols, const mbn_view *views, int n_views,
                                   int out_rows, int out_cols)
{
    if (!views || n_views < 1 || n_views > MBN_ENSEMBLE_MAX_VIEWS || batch <= 0) return MBN_EINVAL;
    int status = MBN_OK;
    for (int k = 0; k < n_views; k++) {
        const mbn_view *v = &views[k];
        if ((v->mirror != 0 && v->mirror != 1) || v->reserved[0] || v->reserved[1] || v->reserved[2]) return MBN_EINVAL;
        const int32_t rect[4] = { v->x, v->y, v->iw, v->ih };
        /* the logits hold batch * n_views maps (64-bit: the product may pass int) */
        const int64_t maps = (int64_t)batch * n_views;
        const int rc = mbn_resample_window_envelope(maps > MBN_DENSE_MAX_BATCH ? MBN_DENSE_MAX_BATCH + 1 : (int)maps, rows, cols, classes, in_rows, in_cols,
                                                    rect, out_rows, out_cols);
        if (rc == MBN_EINVAL) return rc;
        if (rc != MBN_OK) status = rc;
    }
    return status;
}

int mbn_resample_ensemble_plan(int rows, int cols, int in_rows, int in_cols, const mbn_view *views, int n_views, int out_rows, int out_cols,
                               mbn_resample_launch_t *l)
{
    if (!views || !l || n_views < 1 || n_views > MBN_ENSEMBLE_MAX_VIEWS) return MBN_EINVAL;
    const mbn_resample_launch_t zero = { 0, 0, 0, 0, 0, 0 };
    *l = zero;
    for (int k = 0; k < n_views; k++) {
        const int32_t rect[4] = { views[k].x, views[k].y, views[k].iw, views[k].ih };
        mbn_resample_window_plan(rows, cols, in_rows, in_cols, rect, out_rows, out_cols, l);            /* the largest footprint over the views */
    }
    const int nv = n_views * l->fy * l->fx;
    l->ch = MBN_RESAMPLE_ENSEMBLE_CH(nv);
    l->lds_bytes = nv * (l->ch + 4) * 4;
    return MBN_OK;
}

int mbn_slide_axis(int size, int tile, int stride, int32_t *pos, int32_t *n)
{
    if (size <= 0 || tile <= 0 || stride <= 0 || !pos || !n || stride > tile) return MBN_EINVAL;
    if (tile > size || stride < tile - tile / 2) return MBN_EUNSUPPORTED;                           /* ceil(tile / 2) without overflow */
    const int64_t count = (size > tile ? ((int64_t)size - tile + stride - 1) / stride : 0) + 1;
    if (count > MBN_SLIDE_MAX_AXIS) return MBN_EUNSUPPORTED;
    for (int i = 0; i < (int)count; i++) {
        const int64_t p = (int64_t)i * stride;
        pos[i] = (int32_t)(p < size - tile ? p : size - tile);
    }
    *n = (int32_t)count;
    return MBN_OK;
}

int mbn_slide_plan(int in_rows, int in_cols, int tile_rows, int tile_cols, int stride_rows, int stride_cols, mbn_slide *s)
{
    if (!s) return MBN_EINVAL;
    mbn_slide t;
    memset(&t, 0, sizeof t);
    /* an MBN_EINVAL of either axis goes before an MBN_EUNSUPPORTED of the other, as in the read-out's envelope */
    const int ry = mbn_slide_axis(in_rows, tile_rows, stride_rows, t.y, &t.ny), rx = mbn_slide_axis(in_cols, tile_cols, stride_cols, t.x, &t.nx);
    if (ry == MBN_EINVAL || rx == MBN_EINVAL) return MBN_EINVAL;
    if (ry != MBN_OK) return ry;
    if (rx != MBN_OK) return rx;
    t.tile_rows = tile_rows; t.tile_cols = tile_cols;
    *s = t;
    return MBN_OK;
}

/* one axis of a plan against the rules of include/mbn.h, "segment by sliding window" (pos has MBN_SLIDE_MAX_AXIS entries) */
static int slide_axis_check(const int32_t *pos, int n, int tile, int size)
{
    if (n < 1 || n > MBN_SLIDE_MAX_AXIS || tile <= 0 || size <= 0) return MBN_EINVAL;
    if (pos[0] != 0 || (int64_t)pos[n - 1] + tile != size) return MBN_EINVAL;
    for (int i = 0; i + 1 < n; i++)
        if (pos[i + 1] <= pos[i] || (int64_t)pos[i + 1] > (int64_t)pos[i] + tile) return MBN_EINVAL;
    for (int i = n; i < MBN_SLIDE_MAX_AXIS; i++)
        if (pos[i] != 0) return MBN_EINVAL;
    for (int i = 0; i + 3 < n; i++)
        if ((int64_t)pos[i + 3] < (int64_t)pos[i] + tile) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_slide_check(const mbn_slide *s, int out_rows, int out_cols)
{
    if (!s || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    const int ry = slide_axis_check(s->y, s->ny, s->tile_rows, out_rows), rx = slide_axis_check(s->x, s->nx, s->tile_cols, out_cols);
    if (ry == MBN_EINVAL || rx == MBN_EINVAL) return MBN_EINVAL;                                  /* of either axis, before an MBN_EUNSUPPORTED of the other */
    return ry != MBN_OK ? ry : rx;
}

int mbn_resample_slide_envelope(int batch, int rows, int cols, int classes, const mbn_slide *s, int out_rows, int out_cols)
{
    if (batch <= 0 || rows <= 0 || cols <= 0 || classes <= 0) return MBN_EINVAL;
    const int rc = mbn_slide_check(s, out_rows, out_cols);
    if (rc != MBN_OK) return rc;
    if (out_rows > MBN_RESAMPLE_MAX_OUT || out_cols > MBN_RESAMPLE_MAX_OUT) return MBN_EUNSUPPORTED;
    if (4.0 * out_rows * out_cols >= 2147483648.0) return MBN_EUNSUPPORTED;                                     /* an image's labels / scores */
    /* every tile is one read-out to tile_rows x tile_cols: its ratio and bytes; the logits hold batch * ny * nx maps (64-bit: the product may pass int) */
    const int64_t maps = (int64_t)batch * s->ny * s->nx;
    return mbn_resample_argmax_envelope(maps > MBN_DENSE_MAX_BATCH ? MBN_DENSE_MAX_BATCH + 1 : (int)maps, rows, cols, classes, s->tile_rows, s->tile_cols);
}

int mbn_slide_cells(const int32_t *pos, int n, int tile, int32_t edge[MBN_SLIDE_MAX_CELLS + 1], int32_t pieces[MBN_SLIDE_MAX_CELLS + 1], int32_t *kmax)
{
    /* the starts and the ends are each ascending: merge them, equal values once */
    int cells = -1, a = 0, b = 0;
    while (a < n || b < n) {
        const int32_t v = a < n && pos[a] <= pos[b] + tile ? pos[a++] : pos[b++] + tile;              /* b <= a: pos[b] is read only while b < n */
        if (cells < 0 || edge[cells] != v) edge[++cells] = v;
    }
    *kmax = 0;
    pieces[0] = 0;
    for (int c = 0; c < cells; c++) {
        int k = 0;
        for (int i = 0; i < n; i++) k += pos[i] <= edge[c] && edge[c] < pos[i] + tile;
        if (k > *kmax) *kmax = k;
        pieces[c + 1] = pieces[c] + (edge[c + 1] - edge[c] + MBN_RESAMPLE_TILE - 1) / MBN_RESAMPLE_TILE;
    }
    for (int c = cells + 1; c <= MBN_SLIDE_MAX_CELLS; c++) edge[c] = pieces[c] = 0;
    return cells;
}

int mbn_resample_slide_plan(int rows, int cols, const mbn_slide *s, int out_rows, int out_cols, mbn_resample_launch_t *l)
{
    if (!s || !l) return MBN_EINVAL;
    int32_t edge[MBN_SLIDE_MAX_CELLS + 1], py[MBN_SLIDE_MAX_CELLS + 1], px[MBN_SLIDE_MAX_CELLS + 1], ky, kx;
    const int cy = mbn_slide_cells(s->y, s->ny, s->tile_rows, edge, py, &ky), cx = mbn_slide_cells(s->x, s->nx, s->tile_cols, edge, px, &kx);
    const mbn_resample_launch_t zero = { 0, 0, 0, 0, 0, 0 };
    *l = zero;
    l->fy = MBN_RESAMPLE_FOOT(rows, s->tile_rows);
    l->fx = MBN_RESAMPLE_FOOT(cols, s->tile_cols);
    const int nv = ky * kx * l->fy * l->fx;
    l->ch = MBN_RESAMPLE_SLIDE_CH(nv);
    l->lds_bytes = nv * (l->ch + 4) * 4;
    l->tiles = py[cy] * px[cx];
    l->span = (int64_t)out_rows * out_cols;
    return MBN_OK;
}

static int cmp_i64_pair(const void *a, const void *b)
{
    const int64_t x = *(const int64_t *)a, y = *(const int64_t *)b;
    return x < y ? -1 : x > y;
}

/* Both kinds of ragged set: `items` holds `batch` items of item_bytes each, mbn_label_item or mbn_label_window_item, which begins with the former's
 * fields. A plain item's rectangle is the whole in_rows x in_cols input (the caller passes rows x cols) */
_Static_assert(offsetof(mbn_label_window_item, x) == sizeof(mbn_label_item), "a window item is a label item and its rectangle");
static int ragged_check(int rows, int cols, int classes, int in_rows, int in_cols, const void *items, size_t item_bytes, int batch, int64_t *sort,
                        mbn_resample_launch_t *l)
{
    if (!items || !sort || !l || batch <= 0) return MBN_EINVAL;
    const mbn_resample_launch_t zero = { 0, 0, 0, 0, 0, 0 };
    mbn_resample_launch_t acc = zero;
    int64_t span = 0;
    for (int i = 0; i < batch; i++) {
        const char *at = (const char *)items + (size_t)i * item_bytes;
        mbn_label_item it;
        int32_t rect[4] = { 0, 0, in_cols, in_rows };
        memcpy(&it, at, sizeof it);
        if (item_bytes == sizeof(mbn_label_window_item)) memcpy(rect, at + sizeof it, sizeof rect);
        if (it.dst_offset < 0) return MBN_EINVAL;
        const int rc = mbn_resample_window_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, it.rows, it.cols);
        if (rc != MBN_OK) return rc;
        mbn_resample_window_plan(rows, cols, in_rows, in_cols, rect, it.rows, it.cols, &acc);
        sort[2 * i] = it.dst_offset;
        sort[2 * i + 1] = it.dst_offset + (int64_t)it.rows * it.cols;
        if (sort[2 * i + 1] > span) span = sort[2 * i + 1];
    }
    qsort(sort, (size_t)batch, 2 * sizeof(int64_t), cmp_i64_pair);
    for (int i = 0; i + 1 < batch; i++)
        if (sort[2 * i + 1] > sort[2 * i + 2]) return MBN_EINVAL;                                               /* two maps overlap */
    acc.span = span;
    *l = acc;
    return MBN_OK;
}

int mbn_resample_ragged_check(int rows, int cols, int classes, const mbn_label_item *items, int batch, int64_t *sort, mbn_resample_launch_t *l)
{
    return ragged_check(rows, cols, classes, rows, cols, items, sizeof *items, batch, sort, l);
}

int mbn_resample_ragged_window_check(int rows, int cols, int classes, int in_rows, int in_cols, const mbn_label_window_item *items, int batch,
                                     int64_t *sort, mbn_resample_launch_t *l)
{
    return ragged_check(rows, cols, classes, in_rows, in_cols, items, sizeof *items, batch, sort, l);
}

/* what the two top-k forms share: k against the classes, and the k planes against MBN_TOPK_MAX_ELEMENTS */
static int topk_planes(int classes, int k, int64_t plane, int shape)
{
    if (k < 1 || k > MBN_TOPK_MAX || shape == MBN_EINVAL || k > classes) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    return plane > MBN_TOPK_MAX_ELEMENTS / k ? MBN_EUNSUPPORTED : MBN_OK;
}

int mbn_resample_topk_envelope(int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows,
                               int out_cols, int k)
{
    const int shape = rect ? mbn_resample_window_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols)
                           : mbn_resample_argmax_envelope(batch, rows, cols, classes, out_rows, out_cols);
    return topk_planes(classes, k, shape == MBN_OK ? (int64_t)batch * out_rows * out_cols : 0, shape);
}

int mbn_resample_topk_ragged_check(int classes, int64_t span, int k, int64_t plane_stride)
{
    if (classes < 1 || span < 1 || plane_stride < span) return MBN_EINVAL;
    return topk_planes(classes, k, plane_stride, MBN_OK);
}

/* what the two NLL forms share: the truth's width and the temperatures in front of the shape's own answer, then the classes and the planes */
static int nll_planes(int classes, int truth_bytes, int temps, int64_t plane, int shape)
{
    if ((truth_bytes != 1 && truth_bytes != 4) || temps < 1 || temps > MBN_NLL_MAX_TEMPS || shape == MBN_EINVAL) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    if (classes > MBN_CONFUSION_MAX_CLASSES) return MBN_EUNSUPPORTED;
    return plane > MBN_TOPK_MAX_ELEMENTS / temps ? MBN_EUNSUPPORTED : MBN_OK;
}

int mbn_resample_nll_envelope(int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t rect[4], int out_rows, int out_cols,
                              int truth_bytes, int temps)
{
    const int shape = rect ? mbn_resample_window_envelope(batch, rows, cols, classes, in_rows, in_cols, rect, out_rows, out_cols)
                           : mbn_resample_argmax_envelope(batch, rows, cols, classes, out_rows, out_cols);
    return nll_planes(classes, truth_bytes, temps, shape == MBN_OK ? (int64_t)batch * out_rows * out_cols : 0, shape);
}

int mbn_resample_nll_ragged_check(int classes, int64_t span, int truth_bytes, int temps, int64_t plane_stride)
{
    if (classes < 1 || span < 1 || plane_stride < span) return MBN_EINVAL;
    return nll_planes(classes, truth_bytes, temps, plane_stride, MBN_OK);
}

/* a beta the NLL read-out takes: finite and in [1/16, 16] (a NaN fails both compares) */
int mbn_nll_temps_check(const float *inv_temps, int temps)
{
    if (!inv_temps || temps < 1 || temps > MBN_NLL_MAX_TEMPS) return MBN_EINVAL;
    for (int j = 0; j < temps; j++)
        if (!(inv_temps[j] >= 0.0625f && inv_temps[j] <= 16.0f)) return MBN_EINVAL;
    return MBN_OK;
}

static long lmin(long a, long b) { return a < b ? a : b; }

int mbn_i8_pw_plan(long m, int cin, int op_size, int num_cus, int operands_on_16, int out_f32, mbn_i8_pw_plan_t *p)
{
    if (!p || m <= 0 || cin <= 0 || (cin % 8) != 0 || cin > 65536 || op_size <= 0 || num_cus <= 0) return MBN_EINVAL;
    const mbn_i8_pw_plan_t zero = { 0 };
    *p = zero;
    p->out_f32 = out_f32 != 0;
    const int g16 = (cin % 16) == 0 && operands_on_16;
    const int nchunks = (op_size + 31) / 32;
    if (cin <= 1024 && (g16 || (cin % 16) != 0)) {
        /* persistent form: per workgroup up to 8 waves = 32-column chunks x groups of pixel sub-tiles */
        const int kp = (cin + 31) / 32 * 32, maxw = MBN_I8_PW_MAXWAVES, gb = cin % 16 == 0 ? 16 : 8;
        const int ngy = (nchunks + maxw - 1) / maxw, cpw = (nchunks + ngy - 1) / ngy;
        const int maxg = kp / 32 <= 4 ? 8 : 4;                               /* the kernel's MAXG (granules per thread and tile) */
        const long str = kp + 16;
        /* waves: cpw chunks x rep groups of 32-pixel sub-tiles, four waves where the chunks allow */
        int rep = cpw >= 4 ? 1 : 4 / cpw;
        /* workgroups a CU holds at once: about 12 waves of these register counts; the tile's two LDS buffers are sized to fit them */
        const int resident = cpw * rep >= 8 ? 1 : 12 / (cpw * rep);
        int pt = (int)lmin(32768 / kp, ((long)MBN_I8_PW_LDS_MAX / resident) / (2 * str)) / 32 * 32;   /* ~32 KB tiles */
        if (pt > 1024) pt = 1024;
        if (pt < 32) pt = 32;
        /* the fewest rounds of the resident slots the largest tile allows, then the smallest tile that keeps to them (short layers,
         * the 14 x 14 and smaller maps: one round, every slot busy, no straggling second round) */
        long per_round = (long)num_cus * resident / ngy;
        if (per_round < 1) per_round = 1;
        const long rounds = ((m + pt - 1) / pt + per_round - 1) / per_round;
        pt = (int)lmin(pt, ((m + rounds * per_round - 1) / (rounds * per_round) + 31) / 32 * 32);
        if (rep > pt / 32) rep = pt / 32;
        /* more waves where staging a tile needs them */
        while (cpw * rep < maxw && (long)pt * (cin / gb) > (long)maxg * 64 * cpw * rep) rep++;
        while (pt > 32 && (long)pt * (cin / gb) > (long)maxg * 64 * cpw * rep) pt -= 32;
        const int waves = cpw * rep, threads = 64 * waves;
        if (waves <= maxw && (long)pt * (cin / gb) <= (long)maxg * threads) {
            const int ks = kp / 32;
            p->form = MBN_I8_PW_PERSISTENT;
            p->ks = ks <= 1 ? 1 : ks <= 2 ? 2 : ks <= 4 ? 4 : ks <= 8 ? 8 : ks <= 16 ? 16 : 32;
            p->g = gb;
            p->pt = pt;
            p->threads = threads;
            p->gy = ngy;
            p->lds_bytes = (int)(2 * (long)pt * str);
            p->ntiles = (m + pt - 1) / pt;
            p->gx = lmin(p->ntiles, per_round);                              /* persistent: the resident slots */
            p->kp = kp; p->cpw = cpw; p->rep = rep; p->resident = resident; p->maxg = maxg;
            p->per_round = per_round; p->rounds = rounds;
            return MBN_OK;
        }
        /* K % 16 == 8 above 512: a 32-pixel tile's 8-byte granules outnumber what 512 threads stage */
    }
    p->form = MBN_I8_PW_KREG;
    p->ks = cin <= 128 ? 4 : cin <= 512 ? 16 : 32;
    p->g = g16 ? 16 : 8;
    p->pt = 128;
    p->threads = 256;
    p->gy = 1;
    p->nkb = (cin + 32 * p->ks - 1) / (32 * p->ks);
    p->nchunks = nchunks;
    p->ntiles = (m + p->pt - 1) / p->pt;
    /* column groups: split the chunks over workgroups until the grid holds two workgroups per CU (the pixels are then read once per
     * group, the later reads from the L2 / MALL) */
    long ng = (2L * num_cus + p->ntiles - 1) / p->ntiles;
    if (ng > nchunks) ng = nchunks;
    if (ng < 1) ng = 1;
    p->cpg = (int)((nchunks + ng - 1) / ng);
    p->ngroups = (nchunks + p->cpg - 1) / p->cpg;
    p->gx = p->ntiles * p->ngroups;
    if (p->gx > 0x7fffffffL) return MBN_EUNSUPPORTED;
    return MBN_OK;
}
