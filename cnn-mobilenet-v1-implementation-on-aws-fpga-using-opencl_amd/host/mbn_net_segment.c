/*
 * mbn_net_segment.c — segmentation on the net runner: the staging of sources of any size, the segment calls (all of them one pipeline,
 * segment_run) and the consumers that score the maps a call wrote. Plain C over mbn.h and the kernels' shape envelopes, like mbn_net.c.
 */
#include <stdlib.h>
#include <string.h>

#include "mbn_net_internal.h"
#include "mbn_envelope.h"

/* ------------------------------------------------------------------------------------------------------------------------------- staging */
int mbn_net_set_resize_filter(mbn_net *net, int filter)
{
    if (!net || filter < MBN_FILTER_NEAREST || filter > MBN_FILTER_HAMMING) return MBN_EINVAL;
    net->seg.resize_filter = filter;                          /* the kept resizers are rebuilt by the next call that finds another filter in them */
    return MBN_OK;
}

int mbn_net_get_resize_filter(const mbn_net *net, int *filter)
{
    if (!net || !filter) return MBN_EINVAL;
    *filter = net->seg.resize_filter;
    return MBN_OK;
}

int mbn_net_set_pad_color(mbn_net *net, int r, int g, int b)
{
    if (!net || r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255) return MBN_EINVAL;
    net->seg.pad_color[0] = (uint8_t)r; net->seg.pad_color[1] = (uint8_t)g; net->seg.pad_color[2] = (uint8_t)b;     /* a kept letterbox of another colour is rebuilt */
    return MBN_OK;
}

int mbn_net_get_pad_color(const mbn_net *net, int *r, int *g, int *b)
{
    if (!net || !r || !g || !b) return MBN_EINVAL;
    *r = net->seg.pad_color[0]; *g = net->seg.pad_color[1]; *b = net->seg.pad_color[2];
    return MBN_OK;
}

/* the staging buffer every resize call writes, [max_batch][rows][cols][3] uint8, allocated on first use */
static int staging_buffer(mbn_net *net, void **buf)
{
    if (!net->seg.resize_buf) {
        const mbn_layer_desc *in = &net->plan.layer[0];
        const int rc = mbn_alloc(net->ctx, (size_t)net->max_batch * in->in_rows * in->in_cols * 3, &net->seg.resize_buf);
        if (rc != MBN_OK) { net->seg.resize_buf = NULL; return rc; }
    }
    *buf = net->seg.resize_buf;
    return MBN_OK;
}

int mbn_net_resize_input(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, float crop_fraction, void **images_u8)
{
    if (!net || !src_u8 || !images_u8 || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    *images_u8 = NULL;
    struct mbn_net_seg *s = &net->seg;
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    if (fit == MBN_FIT_STRETCH || fit == MBN_FIT_PAD) crop_fraction = 1.0f;
    if (!s->resizer || s->rs_rows != in_rows || s->rs_cols != in_cols || s->rs_fit != fit || s->rs_fraction != crop_fraction ||
        s->rs_filter != s->resize_filter || (fit == MBN_FIT_PAD && memcmp(s->rs_color, s->pad_color, 3) != 0)) {
        float box[4];
        mbn_resizer *r = NULL;
        int rc = mbn_fit_box(in_rows, in_cols, rows, cols, fit, crop_fraction, box);
        if (rc == MBN_OK)
            rc = fit == MBN_FIT_PAD ? mbn_resizer_create_pad(net->ctx, s->resize_filter, in_rows, in_cols, rows, cols, s->pad_color, &r)
                                    : mbn_resizer_create_filter(net->ctx, s->resize_filter, in_rows, in_cols, box, rows, cols, &r);
        if (rc != MBN_OK) return rc;                          /* the resizer of the previous geometry stays */
        if (s->resizer) mbn_resizer_destroy(s->resizer);      /* waits for the stream: a resize still running reads its tables */
        s->resizer = r;
        s->rs_rows = in_rows; s->rs_cols = in_cols; s->rs_fit = fit; s->rs_fraction = crop_fraction; s->rs_filter = s->resize_filter;
        memcpy(s->rs_color, s->pad_color, 3);
    }
    void *buf;
    int rc = staging_buffer(net, &buf);
    if (rc == MBN_OK) rc = mbn_resize_u8(s->resizer, buf, src_u8, batch, NULL);
    if (rc == MBN_OK) *images_u8 = buf;
    return rc;
}

/* the items the ragged resizer is set from, [max_batch], allocated on first use; NULL when they cannot be had */
static mbn_resize_item *ragged_items(mbn_net *net)
{
    if (!net->seg.ragged_items) net->seg.ragged_items = malloc((size_t)net->max_batch * sizeof(mbn_resize_item));
    return net->seg.ragged_items;
}

/* The first n of those items through the net's ragged resizer, one launch into the staging buffer. The resizer is the one of (the current filter,
 * letterbox or not, and for a letterbox the current pad colour), made again when any of them differs: the new handle first, so a refusal
 * (HAMMING / LANCZOS: MBN_EUNSUPPORTED) leaves the previous one in place. */
static int ragged_stage(mbn_net *net, int pad, int n, const void *src_u8, void **staged)
{
    struct mbn_net_seg *s = &net->seg;
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    if (!s->ragged || s->ragged_filter != s->resize_filter || s->ragged_pad != pad || (pad && memcmp(s->ragged_color, s->pad_color, 3) != 0)) {
        mbn_ragged_resizer *r = NULL;
        const int rc = pad ? mbn_ragged_resizer_create_pad(net->ctx, s->resize_filter, net->max_batch, rows, cols, s->pad_color, &r)
                           : mbn_ragged_resizer_create_filter(net->ctx, s->resize_filter, net->max_batch, rows, cols, &r);
        if (rc != MBN_OK) return rc;
        if (s->ragged) mbn_ragged_resizer_destroy(s->ragged);           /* waits for its last launch */
        s->ragged = r; s->ragged_filter = s->resize_filter; s->ragged_pad = pad;
        memcpy(s->ragged_color, s->pad_color, 3);
    }
    void *buf;
    int rc = staging_buffer(net, &buf);
    if (rc == MBN_OK) rc = mbn_ragged_resizer_set(s->ragged, s->ragged_items, n, NULL);
    if (rc == MBN_OK) rc = mbn_resize_ragged_u8(s->ragged, buf, src_u8, NULL);
    if (rc == MBN_OK) *staged = buf;
    return rc;
}

int mbn_net_resize_inputs(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols, int batch, int fit,
                          float crop_fraction, void **images_u8)
{
    if (!net || !src_u8 || !offsets || !in_rows || !in_cols || !images_u8 || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    *images_u8 = NULL;
    if (fit == MBN_FIT_STRETCH || fit == MBN_FIT_PAD) crop_fraction = 1.0f;
    mbn_resize_item *items = ragged_items(net);
    if (!items) return MBN_ENOMEM;
    for (int i = 0; i < batch; i++) {
        mbn_resize_item *it = &items[i];
        it->src_offset = offsets[i];
        it->rows = in_rows[i];
        it->cols = in_cols[i];
        const int rc = mbn_fit_box(in_rows[i], in_cols[i], net->plan.layer[0].in_rows, net->plan.layer[0].in_cols, fit, crop_fraction, it->box);
        if (rc != MBN_OK) return rc;
    }
    return ragged_stage(net, fit == MBN_FIT_PAD, batch, src_u8, images_u8);
}

/* the views of (scales[k], mirrors[k]) for a source of in_rows x in_cols: what both view calls check first */
static int views_of(const mbn_net *net, int batch, int in_rows, int in_cols, const float *scales, const int32_t *mirrors, int n_views, mbn_view *views)
{
    if (!scales || !mirrors || n_views < 1 || n_views > MBN_ENSEMBLE_MAX_VIEWS || batch <= 0 || in_rows <= 0 || in_cols <= 0) return MBN_EINVAL;
    if ((int64_t)batch * n_views > net->max_batch) return MBN_EINVAL;
    for (int k = 0; k < n_views; k++) {
        const int rc = mbn_fit_view(in_rows, in_cols, net->plan.layer[0].in_rows, net->plan.layer[0].in_cols, scales[k], mirrors[k], &views[k]);
        if (rc != MBN_OK) return rc;
    }
    return MBN_OK;
}

/* the kept resizer of one view, made on first use; the least recently used slot makes room (a call has at most as many views as there are slots and
 * stamps each with the call's own clock, so it never takes a slot from itself) */
static int view_resizer(mbn_net *net, int in_rows, int in_cols, float scale, const mbn_view *view, mbn_resizer **out)
{
    struct mbn_net_seg *s = &net->seg;
    struct mbn_view_slot *oldest = NULL;                          /* where a new one goes: an empty slot, else the least recently used */
    for (int i = 0; i < MBN_ENSEMBLE_MAX_VIEWS; i++) {
        struct mbn_view_slot *v = &s->view_cache[i];
        if (v->r && v->rows == in_rows && v->cols == in_cols && v->scale == scale && v->mirror == view->mirror && v->filter == s->resize_filter &&
            memcmp(v->color, s->pad_color, 3) == 0) {
            v->used = s->view_clock;
            *out = v->r;
            return MBN_OK;
        }
        if (!oldest || (oldest->r && (!v->r || (int)(v->used - oldest->used) < 0))) oldest = v;
    }
    mbn_resizer *r = NULL;
    const int rc = mbn_resizer_create_view(net->ctx, s->resize_filter, in_rows, in_cols, net->plan.layer[0].in_rows, net->plan.layer[0].in_cols, view,
                                           s->pad_color, &r);
    if (rc != MBN_OK) return rc;
    if (oldest->r) mbn_resizer_destroy(oldest->r);                /* waits for the stream: a resize still running reads its tables */
    oldest->r = r;
    oldest->rows = in_rows; oldest->cols = in_cols; oldest->scale = scale; oldest->mirror = view->mirror; oldest->filter = s->resize_filter;
    memcpy(oldest->color, s->pad_color, 3);
    oldest->used = s->view_clock;
    *out = r;
    return MBN_OK;
}

static int resize_views(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const float *scales, const mbn_view *views, int n_views,
                        void **staged)
{
    const size_t canvas = (size_t)net->plan.layer[0].in_rows * net->plan.layer[0].in_cols * 3;
    void *buf;
    int rc = staging_buffer(net, &buf);
    if (rc != MBN_OK) return rc;
    net->seg.view_clock++;
    for (int k = 0; k < n_views; k++) {
        mbn_resizer *r = NULL;
        rc = view_resizer(net, in_rows, in_cols, scales[k], &views[k], &r);
        /* view-major: view k's canvases are images k * batch .. of the staging buffer */
        if (rc == MBN_OK) rc = mbn_resize_u8(r, (uint8_t *)buf + (size_t)k * batch * canvas, src_u8, batch, NULL);
        if (rc != MBN_OK) return rc;
    }
    *staged = buf;
    return MBN_OK;
}

int mbn_net_resize_views(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const float *scales, const int32_t *mirrors,
                         int n_views, void **staged)
{
    if (!net || !src_u8 || !staged) return MBN_EINVAL;
    *staged = NULL;
    mbn_view views[MBN_ENSEMBLE_MAX_VIEWS];
    const int rc = views_of(net, batch, in_rows, in_cols, scales, mirrors, n_views, views);
    if (rc != MBN_OK) return rc;
    return resize_views(net, src_u8, batch, in_rows, in_cols, scales, views, n_views, staged);
}

/* the tiles of a plan the caller has checked: batch * ny * nx <= max_batch items on the net's plain ragged handle, one launch */
static int resize_tiles(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const mbn_slide *s, void **staged)
{
    mbn_resize_item *items = ragged_items(net);
    if (!items) return MBN_ENOMEM;
    int n = 0;
    for (int b = 0; b < batch; b++)
        for (int iy = 0; iy < s->ny; iy++)
            for (int ix = 0; ix < s->nx; ix++) {
                mbn_resize_item *it = &items[n++];                      /* image b * ny * nx + iy * nx + ix of the staging buffer */
                it->src_offset = (int64_t)b * in_rows * in_cols * 3;
                it->rows = in_rows;
                it->cols = in_cols;
                it->box[0] = (float)s->x[ix]; it->box[1] = (float)s->y[iy];
                it->box[2] = (float)(s->x[ix] + s->tile_cols); it->box[3] = (float)(s->y[iy] + s->tile_rows);
            }
    return ragged_stage(net, 0, n, src_u8, staged);
}

/* what both slide calls check first: the plan against the source size, its tiles against max_batch */
static int slide_status(const mbn_net *net, int batch, int in_rows, int in_cols, const mbn_slide *s)
{
    if (batch <= 0 || in_rows <= 0 || in_cols <= 0) return MBN_EINVAL;
    const int rc = mbn_slide_check(s, in_rows, in_cols);
    if (rc != MBN_OK) return rc;
    return (int64_t)batch * s->ny * s->nx > net->max_batch ? MBN_EINVAL : MBN_OK;
}

int mbn_net_resize_tiles(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const mbn_slide *s, void **staged)
{
    if (!net || !src_u8 || !s || !staged) return MBN_EINVAL;
    *staged = NULL;
    const int rc = slide_status(net, batch, in_rows, in_cols, s);
    if (rc != MBN_OK) return rc;
    return resize_tiles(net, src_u8, batch, in_rows, in_cols, s, staged);
}

/* ------------------------------------------------------------------------------------------------------------------------- the segment calls */
/* the softmax read-out of a call: labels and prob (a pixel under min_prob holds ignore_label). A call without one is the argmax read-out */
typedef struct readout_prob { void *prob; float min_prob; int ignore_label; } readout_prob;

/* the rule of the calls that take all three outputs (views, slide): no prob map and no threshold is the argmax form */
static int softmax_form(const void *prob_f32, float min_prob)
{
    return prob_f32 || !(min_prob == 0.0f);
}

/* the arguments of a segment call, as its public function got them; from P_FIT on, src holds uint8 sources that the call stages */
enum { P_INPUT, P_TO, P_FIT, P_IMAGES, P_VIEWS, P_SLIDE };
typedef struct seg_call {
    int path;
    const void *src;
    void *labels, *score;
    const readout_prob *q;                              /* NULL: the argmax read-out */
    int batch, rows, cols, fit;                         /* rows x cols: the size of every map it writes (P_IMAGES: the items carry theirs); fit: 0 is STRETCH */
    const int64_t *offsets, *dst_offsets;               /* P_IMAGES: per image, with rows_of and cols_of */
    const int32_t *rows_of, *cols_of, *mirrors;
    const float *scales;                                /* P_VIEWS: per view, with mirrors */
    int n_views;
    int tile[2], stride[2];                             /* P_SLIDE: rows, cols */
    int topk;                                           /* P_FIT, P_IMAGES: 0, or the k of the top-k read-out: labels, score and prob hold k planes, */
    int64_t plane_stride;                               /* for P_IMAGES this many elements apart */
} seg_call;

/* The net's read-out set from the items of an image call: each image's map at its own size, through its letterbox window under MBN_FIT_PAD. The set
 * checks every item, so a refusal comes before the resize and the forward run; its upload is ordered by the stream. */
static int readout_set(mbn_net *net, const seg_call *c, const mbn_layer_desc *feat, const mbn_layer_desc *fc, int64_t *pixels)
{
    struct mbn_net_seg *s = &net->seg;
    const int pad = c->fit == MBN_FIT_PAD, rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    if (!s->label_items) {
        s->label_items = malloc((size_t)net->max_batch * sizeof(mbn_label_window_item));        /* either kind of item */
        if (!s->label_items) return MBN_ENOMEM;
    }
    /* a window item is a label item and then its rectangle: the first item_bytes of `it` are the item of either kind */
    const size_t item_bytes = pad ? sizeof(mbn_label_window_item) : sizeof(mbn_label_item);
    for (int i = 0; i < c->batch; i++) {
        *pixels += (int64_t)c->rows_of[i] * c->cols_of[i];
        int32_t rect[4] = { 0, 0, 0, 0 };
        if (pad) {
            const int rc = mbn_fit_pad(c->rows_of[i], c->cols_of[i], rows, cols, rect);
            if (rc != MBN_OK) return rc;
        }
        const mbn_label_window_item it = { c->dst_offsets[i], c->rows_of[i], c->cols_of[i], rect[0], rect[1], rect[2], rect[3] };
        memcpy((char *)s->label_items + (size_t)i * item_bytes, &it, item_bytes);
    }
    if (!s->readout) {
        const int rc = mbn_ragged_readout_create(net->ctx, net->max_batch, &s->readout);
        if (rc != MBN_OK) { s->readout = NULL; return rc; }
    }
    return pad ? mbn_ragged_readout_set_window(s->readout, feat->out_rows, feat->out_cols, fc->out_ch, rows, cols, s->label_items, c->batch, NULL)
               : mbn_ragged_readout_set(s->readout, feat->out_rows, feat->out_cols, fc->out_ch, s->label_items, c->batch, NULL);
}

/* the dense logits of `batch` images into net->seg.dense_logits, [max_batch][h][w][classes] fp32, allocated on first use */
static int dense_forward(mbn_net *net, const mbn_layer_desc *feat, const mbn_layer_desc *fc, const void *images, int batch)
{
    if (!net->seg.dense_logits) {
        const int rc = mbn_alloc(net->ctx, (size_t)net->max_batch * feat->out_rows * feat->out_cols * fc->out_ch * sizeof(float), &net->seg.dense_logits);
        if (rc != MBN_OK) { net->seg.dense_logits = NULL; return rc; }
    }
    return mbn_net_forward_dense(net, images, net->seg.dense_logits, batch);
}

/* Every segment call. The order is the contract: (1) everything that can refuse, and nothing before the end of it touches the device, a kept
 * handle or the record, so a refused call leaves all three as they were; (2) the staging; (3) ONE forward pass, on n_images; (4) the read-out;
 * (5) the record the consumers read, only after a read-out that succeeded. The cases of a switch are what is a path's own. */
static int segment_run(mbn_net *net, const seg_call *c)
{
    if (!net || !c->src || !c->labels) return MBN_EINVAL;
    if (c->path >= P_FIT && !net->input_u8) return MBN_EINVAL;         /* the staged images are uint8: the net must take them as such */
    const readout_prob *q = c->q;
    if (q && ((uintptr_t)q->prob % 4 || mbn_softmax_readout_check(q->prob != NULL, q->min_prob) != MBN_OK)) return MBN_EINVAL;
    const int in_rows = net->plan.layer[0].in_rows, in_cols = net->plan.layer[0].in_cols, batch = c->batch;
    const int rows = c->path == P_INPUT ? in_rows : c->rows, cols = c->path == P_INPUT ? in_cols : c->cols;
    const int aligned = (((uintptr_t)c->labels | (uintptr_t)c->score | (uintptr_t)(q ? q->prob : NULL)) % 4) == 0;
    int n_images = batch, factor = 0, rc = MBN_OK;
    int64_t pixels = 0;
    int32_t pad[4];
    const int32_t *rect = NULL;                                        /* the window of a letterbox; NULL: the whole map */
    mbn_view views[MBN_ENSEMBLE_MAX_VIEWS];
    mbn_slide slide;
    /* (1a) the arguments, and what follows from them alone */
    switch (c->path) {
    case P_VIEWS:
        if (!aligned) return MBN_EINVAL;
        rc = views_of(net, batch, rows, cols, c->scales, c->mirrors, c->n_views, views);
        n_images = batch * c->n_views;
        break;
    case P_SLIDE:
        if (!aligned || batch <= 0) return MBN_EINVAL;
        rc = mbn_slide_plan(rows, cols, c->tile[0], c->tile[1], c->stride[0], c->stride[1], &slide);
        if (rc == MBN_OK) rc = slide_status(net, batch, rows, cols, &slide);
        if (rc == MBN_OK) n_images = batch * slide.ny * slide.nx;
        break;
    default:
        if (batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
        if (c->path == P_IMAGES ? (!c->offsets || !c->rows_of || !c->cols_of || !c->dst_offsets) : (rows <= 0 || cols <= 0)) return MBN_EINVAL;
        /* the fits a source-size read-out exists for; a crop's box is fractional and the network never saw the rest of the image */
        if (c->fit != MBN_FIT_STRETCH && c->fit != MBN_FIT_PAD) return c->fit == MBN_FIT_CROP ? MBN_EUNSUPPORTED : MBN_EINVAL;
    }
    /* (1b) the plan's dense head, then the path's envelope (the image path: its set) */
    const mbn_layer_desc *feat, *fc;
    if (rc == MBN_OK) rc = mbn_net_dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    const int h = feat->out_rows, w = feat->out_cols, classes = fc->out_ch;
    switch (c->path) {
    case P_INPUT:
        factor = rows / h;
        if (factor * h != rows || factor * w != cols || (factor != 8 && factor != 16 && factor != 32)) rc = MBN_EUNSUPPORTED;
        break;
    case P_TO:
    case P_FIT:
        if (c->fit == MBN_FIT_PAD) {
            rect = pad;
            rc = mbn_fit_pad(rows, cols, in_rows, in_cols, pad);
            if (rc == MBN_OK) rc = mbn_resample_window_envelope(batch, h, w, classes, in_rows, in_cols, rect, rows, cols);
        } else if (mbn_resample_argmax_envelope(batch, h, w, classes, rows, cols) != MBN_OK)
            rc = MBN_EUNSUPPORTED;                                     /* every size is positive here: what the plain shape can miss is a limit */
        if (rc == MBN_OK && c->topk) rc = mbn_resample_topk_envelope(batch, h, w, classes, in_rows, in_cols, rect, rows, cols, c->topk);
        break;
    case P_IMAGES:
        if (c->topk) {
            /* k and the plane stride against the span the set will have, in front of the set: a refused call leaves the handle's set as it was */
            int64_t span = 1;
            for (int i = 0; i < batch; i++) {
                const int64_t end = c->dst_offsets[i] + (int64_t)c->rows_of[i] * c->cols_of[i];
                if (end > span) span = end;
            }
            rc = mbn_resample_topk_ragged_check(classes, span, c->topk, c->plane_stride);
            if (rc != MBN_OK) break;
        }
        rc = readout_set(net, c, feat, fc, &pixels);
        break;
    case P_VIEWS:  rc = mbn_resample_ensemble_envelope(batch, h, w, classes, in_rows, in_cols, views, c->n_views, rows, cols); break;
    case P_SLIDE:  rc = mbn_resample_slide_envelope(batch, h, w, classes, &slide, rows, cols); break;
    }
    if (rc != MBN_OK) return rc;
    /* (2) the staging and (3) the forward pass */
    void *images = (void *)c->src;
    switch (c->path) {
    case P_FIT:    rc = mbn_net_resize_input(net, c->src, batch, rows, cols, c->fit, 1.0f, &images); break;
    case P_IMAGES: rc = mbn_net_resize_inputs(net, c->src, c->offsets, c->rows_of, c->cols_of, batch, c->fit, 1.0f, &images); break;
    case P_VIEWS:  rc = resize_views(net, c->src, batch, rows, cols, c->scales, views, c->n_views, &images); break;
    case P_SLIDE:  rc = resize_tiles(net, c->src, batch, rows, cols, &slide, &images); break;
    }
    if (rc == MBN_OK) rc = dense_forward(net, feat, fc, images, n_images);
    if (rc != MBN_OK) return rc;
    /* (4) the read-out: the one place that chooses among the public read-out calls */
    const void *logits = net->seg.dense_logits;
    void *prob = q ? q->prob : NULL;
    const float min_prob = q ? q->min_prob : 0.0f;
    const int ignore = q ? q->ignore_label : 0;                        /* (an argmax read-out takes none of the three) */
    switch (c->path) {
    case P_INPUT:  rc = mbn_upsample_argmax_f32(net->ctx, c->labels, c->score, logits, batch, h, w, classes, factor, NULL); break;
    case P_IMAGES:
        if (c->topk)
            rc = mbn_resample_topk_ragged_f32(net->seg.readout, c->labels, prob, c->score, logits, c->topk, c->plane_stride, min_prob, ignore, NULL);
        else
            rc = q ? mbn_resample_softmax_ragged_f32(net->seg.readout, c->labels, prob, NULL, logits, min_prob, ignore, NULL)
                   : mbn_resample_argmax_ragged_f32(net->seg.readout, c->labels, c->score, logits, NULL);
        break;
    case P_VIEWS:
        rc = mbn_resample_ensemble_f32(net->ctx, c->labels, prob, c->score, logits, batch, h, w, classes, in_rows, in_cols, views, c->n_views, rows, cols,
                                       min_prob, ignore, NULL);
        break;
    case P_SLIDE:
        rc = mbn_resample_slide_f32(net->ctx, c->labels, prob, c->score, logits, batch, h, w, classes, &slide, rows, cols, min_prob, ignore, NULL);
        break;
    default:
        if (c->topk)
            rc = mbn_resample_topk_f32(net->ctx, c->labels, prob, c->score, logits, batch, h, w, classes, in_rows, in_cols, rect, rows, cols, c->topk,
                                       min_prob, ignore, NULL);
        else if (q && rect)
            rc = mbn_resample_softmax_window_f32(net->ctx, c->labels, prob, NULL, logits, batch, h, w, classes, in_rows, in_cols, rect, rows, cols,
                                                 min_prob, ignore, NULL);
        else if (q) rc = mbn_resample_softmax_f32(net->ctx, c->labels, prob, NULL, logits, batch, h, w, classes, rows, cols, min_prob, ignore, NULL);
        else if (rect)
            rc = mbn_resample_argmax_window_f32(net->ctx, c->labels, c->score, logits, batch, h, w, classes, in_rows, in_cols, rect, rows, cols, NULL);
        else rc = mbn_resample_argmax_f32(net->ctx, c->labels, c->score, logits, batch, h, w, classes, rows, cols, NULL);
    }
    if (rc != MBN_OK) return rc;
    /* (5) the record */
    if (c->path != P_IMAGES) pixels = (int64_t)batch * rows * cols;    /* (an image call has rows = cols = 0, and the pixels of its items) */
    net->seg.last = (struct mbn_seg_maps){ c->path == P_IMAGES ? MBN_SEG_RAGGED : MBN_SEG_UNIFORM, batch, rows, cols, classes, pixels, c->topk,
                                           c->path == P_IMAGES ? c->plane_stride : pixels,
                                           c->path == P_IMAGES ? MBN_SEG_GEOM_SET : c->path == P_VIEWS || c->path == P_SLIDE ? MBN_SEG_GEOM_MANY
                                           : rect ? MBN_SEG_GEOM_RECT : MBN_SEG_GEOM_WHOLE,
                                           { rect ? rect[0] : 0, rect ? rect[1] : 0, rect ? rect[2] : 0, rect ? rect[3] : 0 } };
    return MBN_OK;
}

int mbn_net_segment(mbn_net *net, const void *images, int batch, void *labels_i32, void *score_f32)
{
    const seg_call c = { .path = P_INPUT, .src = images, .labels = labels_i32, .score = score_f32, .batch = batch };
    return segment_run(net, &c);
}

int mbn_net_segment_to(mbn_net *net, const void *images, int batch, int out_rows, int out_cols, void *labels_i32, void *score_f32)
{
    const seg_call c = { .path = P_TO, .src = images, .labels = labels_i32, .score = score_f32, .batch = batch, .rows = out_rows, .cols = out_cols };
    return segment_run(net, &c);
}

int mbn_net_segment_prob_to(mbn_net *net, const void *images, int batch, int out_rows, int out_cols, void *labels_i32, void *prob_f32, float min_prob,
                            int ignore_label)
{
    const readout_prob q = { prob_f32, min_prob, ignore_label };
    const seg_call c = { .path = P_TO, .src = images, .labels = labels_i32, .q = &q, .batch = batch, .rows = out_rows, .cols = out_cols };
    return segment_run(net, &c);
}

int mbn_net_segment_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, void *labels_i32, void *score_f32)
{
    const seg_call c = { .path = P_FIT, .src = src_u8, .labels = labels_i32, .score = score_f32, .batch = batch, .rows = in_rows, .cols = in_cols, .fit = fit };
    return segment_run(net, &c);
}

int mbn_net_segment_prob_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, void *labels_i32, void *prob_f32,
                             float min_prob, int ignore_label)
{
    const readout_prob q = { prob_f32, min_prob, ignore_label };
    const seg_call c = { .path = P_FIT, .src = src_u8, .labels = labels_i32, .q = &q, .batch = batch, .rows = in_rows, .cols = in_cols, .fit = fit };
    return segment_run(net, &c);
}

int mbn_net_segment_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols, int batch,
                               int fit, void *labels_i32, const int64_t *dst_offsets, void *score_f32)
{
    const seg_call c = { .path = P_IMAGES, .src = src_u8, .labels = labels_i32, .score = score_f32, .batch = batch, .fit = fit, .offsets = offsets,
                         .dst_offsets = dst_offsets, .rows_of = in_rows, .cols_of = in_cols };
    return segment_run(net, &c);
}

int mbn_net_segment_images(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols, int batch,
                           void *labels_i32, const int64_t *dst_offsets, void *score_f32)
{
    return mbn_net_segment_images_fit(net, src_u8, offsets, in_rows, in_cols, batch, MBN_FIT_STRETCH, labels_i32, dst_offsets, score_f32);
}

int mbn_net_segment_prob_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols,
                                    int batch, int fit, void *labels_i32, const int64_t *dst_offsets, void *prob_f32, float min_prob,
                                    int ignore_label)
{
    const readout_prob q = { prob_f32, min_prob, ignore_label };
    const seg_call c = { .path = P_IMAGES, .src = src_u8, .labels = labels_i32, .q = &q, .batch = batch, .fit = fit, .offsets = offsets, .dst_offsets = dst_offsets,
                         .rows_of = in_rows, .cols_of = in_cols };
    return segment_run(net, &c);
}

/* the two top-k calls: the _prob_fit / _prob_images_fit paths with the top-k read-out; k outside 1..MBN_TOPK_MAX is refused here, so that 0 never
 * reads as "no top-k" */
int mbn_net_segment_topk_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, int k, void *labels_i32, void *prob_f32,
                             void *score_f32, float min_prob, int ignore_label)
{
    if (k < 1 || k > MBN_TOPK_MAX) return MBN_EINVAL;
    const readout_prob given = { prob_f32, min_prob, ignore_label };
    const seg_call c = { .path = P_FIT, .src = src_u8, .labels = labels_i32, .score = score_f32, .q = softmax_form(prob_f32, min_prob) ? &given : NULL,
                         .batch = batch, .rows = in_rows, .cols = in_cols, .fit = fit, .topk = k };
    return segment_run(net, &c);
}

int mbn_net_segment_topk_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols,
                                    int batch, int fit, int k, int64_t plane_stride, void *labels_i32, const int64_t *dst_offsets, void *prob_f32,
                                    void *score_f32, float min_prob, int ignore_label)
{
    if (k < 1 || k > MBN_TOPK_MAX) return MBN_EINVAL;
    const readout_prob given = { prob_f32, min_prob, ignore_label };
    const seg_call c = { .path = P_IMAGES, .src = src_u8, .labels = labels_i32, .score = score_f32, .q = softmax_form(prob_f32, min_prob) ? &given : NULL,
                         .batch = batch, .fit = fit, .offsets = offsets, .dst_offsets = dst_offsets, .rows_of = in_rows, .cols_of = in_cols, .topk = k,
                         .plane_stride = plane_stride };
    return segment_run(net, &c);
}

int mbn_net_segment_views_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const float *scales, const int32_t *mirrors,
                              int n_views, void *labels_i32, void *prob_f32, void *score_f32, float min_prob, int ignore_label)
{
    const readout_prob given = { prob_f32, min_prob, ignore_label };
    const seg_call c = { .path = P_VIEWS, .src = src_u8, .labels = labels_i32, .score = score_f32, .q = softmax_form(prob_f32, min_prob) ? &given : NULL,
                         .batch = batch, .rows = in_rows, .cols = in_cols, .scales = scales, .mirrors = mirrors, .n_views = n_views };
    return segment_run(net, &c);
}

int mbn_net_segment_slide(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int tile_rows, int tile_cols, int stride_rows,
                          int stride_cols, void *labels_i32, void *prob_f32, void *score_f32, float min_prob, int ignore_label)
{
    const readout_prob given = { prob_f32, min_prob, ignore_label };
    const seg_call c = { .path = P_SLIDE, .src = src_u8, .labels = labels_i32, .score = score_f32, .q = softmax_form(prob_f32, min_prob) ? &given : NULL,
                         .batch = batch, .rows = in_rows, .cols = in_cols, .tile = { tile_rows, tile_cols }, .stride = { stride_rows, stride_cols } };
    return segment_run(net, &c);
}

/* ------------------------------------------------------------------------------------------------------------------------------ the consumers */
/* what the last successful segment call wrote, or NULL when there is none: what every consumer asks first. (The classes are the record's: the
 * call that left it has passed mbn_net_dense_layers on this plan, so a consumer has nothing to refuse there.) */
static const struct mbn_seg_maps *last_maps(const mbn_net *net)
{
    return net && net->seg.last.kind != MBN_SEG_NONE ? &net->seg.last : NULL;
}

int mbn_net_segment_score(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, void *counts_u64)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m) return MBN_EINVAL;
    if (m->kind == MBN_SEG_RAGGED) return mbn_confusion_ragged_i32(net->seg.readout, counts_u64, labels_i32, truth, truth_bytes, m->classes, NULL);
    return mbn_confusion_i32(net->ctx, counts_u64, labels_i32, truth, truth_bytes, m->classes, m->count, NULL);
}

int mbn_net_segment_topk_score(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, void *ranks_u64)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m || !m->topk) return MBN_EINVAL;                             /* the last call wrote one plane: there are no ranks to score */
    if (m->kind == MBN_SEG_RAGGED)
        return mbn_topk_rank_ragged_i32(net->seg.readout, ranks_u64, labels_i32, m->topk, m->plane_stride, truth, truth_bytes, m->classes, NULL);
    return mbn_topk_rank_i32(net->ctx, ranks_u64, labels_i32, m->topk, m->plane_stride, truth, truth_bytes, m->classes, m->count, NULL);
}

int mbn_net_segment_calibration(mbn_net *net, const void *labels_i32, const void *prob_f32, const void *truth, int truth_bytes, int bins,
                                void *calib_u64)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m) return MBN_EINVAL;
    if (m->kind == MBN_SEG_RAGGED)
        return mbn_calibration_ragged_f32(net->seg.readout, calib_u64, labels_i32, prob_f32, truth, truth_bytes, m->classes, bins, NULL);
    return mbn_calibration_f32(net->ctx, calib_u64, labels_i32, prob_f32, truth, truth_bytes, m->classes, bins, m->count, NULL);
}

/* NLL and Brier score of the last call's probabilities: the read-out of net->seg.dense_logits once more, under the geometry the call used, with
 * the truth in the class loop. The factor path's maps are the plain kernel's at out = factor x map bit for bit, so the whole-map call serves it */
int mbn_net_segment_nll(mbn_net *net, const void *truth, int truth_bytes, const float *inv_temps, int temps, void *nll_u64, void *nll_f32,
                        void *brier_f32, int64_t plane_stride)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m) return MBN_EINVAL;
    if (m->geometry == MBN_SEG_GEOM_MANY) return MBN_EUNSUPPORTED;     /* several presentations of an image: another probability model */
    const void *logits = net->seg.dense_logits;
    if (m->geometry == MBN_SEG_GEOM_SET)
        return mbn_resample_nll_ragged_f32(net->seg.readout, nll_u64, nll_f32, brier_f32, plane_stride, logits, truth, truth_bytes, inv_temps, temps, NULL);
    const mbn_layer_desc *feat, *fc;
    const int rc = mbn_net_dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    return mbn_resample_nll_f32(net->ctx, nll_u64, nll_f32, brier_f32, logits, truth, truth_bytes, m->batch, feat->out_rows, feat->out_cols, m->classes,
                                net->plan.layer[0].in_rows, net->plan.layer[0].in_cols, m->geometry == MBN_SEG_GEOM_RECT ? m->rect : NULL, m->rows,
                                m->cols, inv_temps, temps, NULL);
}

/* the net's one mbn_components handle holds at least the maps m */
static int components_ready(mbn_net *net, const struct mbn_seg_maps *m)
{
    struct mbn_net_seg *s = &net->seg;
    if (s->components && m->batch <= s->components_batch && m->count <= s->components_pixels) return MBN_OK;
    /* the new handle first: when it cannot be had, the old one stays */
    const int batch = m->batch > s->components_batch ? m->batch : s->components_batch;
    const int64_t pixels = m->count > s->components_pixels ? m->count : s->components_pixels;
    mbn_components *h = NULL;
    const int rc = mbn_components_create(net->ctx, batch, pixels, &h);
    if (rc != MBN_OK) return rc;
    if (s->components) mbn_components_destroy(s->components);
    s->components = h; s->components_batch = batch; s->components_pixels = pixels;
    return MBN_OK;
}

int mbn_net_segment_regions(mbn_net *net, const void *labels_i32, void *comp_i32, mbn_region *regions, void *n_regions_i32, void *labels_out_i32,
                            int connectivity, int min_area, int ignore_label, int max_regions)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m) return MBN_EINVAL;
    const int rc = components_ready(net, m);
    if (rc != MBN_OK) return rc;
    if (m->kind == MBN_SEG_RAGGED)
        return mbn_components_ragged_i32(net->seg.components, net->seg.readout, comp_i32, regions, n_regions_i32, labels_out_i32, labels_i32, m->classes,
                                         connectivity, min_area, ignore_label, max_regions, NULL);
    return mbn_components_i32(net->seg.components, comp_i32, regions, n_regions_i32, labels_out_i32, labels_i32, m->batch, m->rows, m->cols, m->classes,
                              connectivity, min_area, ignore_label, max_regions, NULL);
}

int mbn_net_set_panoptic_regions(mbn_net *net, int max_regions)
{
    if (!net || max_regions < 1) return MBN_EINVAL;
    if (max_regions > MBN_COMPONENTS_MAX_REGIONS) return MBN_EUNSUPPORTED;
    net->seg.panoptic_max_regions = max_regions;
    return MBN_OK;
}

static void panoptic_release(mbn_net *net)
{
    struct mbn_net_seg *s = &net->seg;
    if (s->panoptic) mbn_panoptic_destroy(s->panoptic);
    s->panoptic = NULL;
    void **bufs[] = { &s->panoptic_comp[0], &s->panoptic_comp[1], &s->panoptic_wide, &s->panoptic_table[0], &s->panoptic_table[1], &s->panoptic_n[0],
                      &s->panoptic_n[1] };
    for (size_t i = 0; i < sizeof bufs / sizeof bufs[0]; i++) {
        if (*bufs[i]) mbn_free(net->ctx, *bufs[i]);
        *bufs[i] = NULL;
    }
    s->panoptic_batch = s->panoptic_regions = 0; s->panoptic_span = 0;
}

/* the handle and the buffers of mbn_net_segment_panoptic hold `batch` images whose maps span `span` elements, with tables of the net's setting.
 * Everything is made again when a call needs more of any of them; a failure leaves nothing behind and the net usable */
static int panoptic_ready(mbn_net *net, int batch, int64_t span)
{
    struct mbn_net_seg *s = &net->seg;
    const int regions = s->panoptic_max_regions;
    if (s->panoptic && batch <= s->panoptic_batch && span <= s->panoptic_span && regions == s->panoptic_regions) return MBN_OK;
    if (batch < s->panoptic_batch) batch = s->panoptic_batch;
    if (span < s->panoptic_span) span = s->panoptic_span;
    panoptic_release(net);                                         /* waits for the device: an earlier call may still read them */
    int rc = mbn_panoptic_create(net->ctx, batch, (int64_t)batch * regions, &s->panoptic);
    if (rc != MBN_OK) s->panoptic = NULL;
    for (int k = 0; k < 2 && rc == MBN_OK; k++) {
        rc = mbn_alloc(net->ctx, (size_t)span * 4, &s->panoptic_comp[k]);
        if (rc == MBN_OK) rc = mbn_alloc(net->ctx, (size_t)batch * regions * sizeof(mbn_region), &s->panoptic_table[k]);
        if (rc == MBN_OK) rc = mbn_alloc(net->ctx, (size_t)batch * 4, &s->panoptic_n[k]);
    }
    if (rc == MBN_OK) rc = mbn_alloc(net->ctx, (size_t)span * 4, &s->panoptic_wide);
    if (rc != MBN_OK) { panoptic_release(net); return rc; }
    s->panoptic_batch = batch; s->panoptic_span = span; s->panoptic_regions = regions;
    return MBN_OK;
}

int mbn_net_segment_panoptic(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, int connectivity, int min_area, void *pq_u64,
                             void *scored_i32)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m || !labels_i32 || !truth || !pq_u64 || !scored_i32) return MBN_EINVAL;
    if ((truth_bytes != 1 && truth_bytes != 4) || (truth_bytes == 4 && (uintptr_t)truth % 4)) return MBN_EINVAL;
    struct mbn_net_seg *s = &net->seg;
    const int ragged = m->kind == MBN_SEG_RAGGED, batch = m->batch, classes = m->classes;
    const int64_t span = ragged ? mbn_ragged_readout_span(s->readout) : m->count;
    if (span < 1) return MBN_EINVAL;
    int rc = components_ready(net, m);
    if (rc == MBN_OK) rc = panoptic_ready(net, batch, span);
    if (rc != MBN_OK) return rc;
    const int regions = s->panoptic_regions;
    const void *maps[2] = { labels_i32, truth };
    if (truth_bytes == 1) {
        /* the flat span: the gaps of a ragged set are widened too, into this private buffer only, and nothing reads them there */
        rc = mbn_widen_u8_i32(net->ctx, s->panoptic_wide, truth, span, NULL);
        if (rc != MBN_OK) return rc;
        maps[1] = s->panoptic_wide;
    }
    /* the two calls share the components handle's scratch: they are ordered by the context's stream */
    for (int k = 0; k < 2; k++) {
        rc = ragged ? mbn_components_ragged_i32(s->components, s->readout, s->panoptic_comp[k], (mbn_region *)s->panoptic_table[k], s->panoptic_n[k], NULL,
                                                maps[k], classes, connectivity, min_area, 0, regions, NULL)
                    : mbn_components_i32(s->components, s->panoptic_comp[k], (mbn_region *)s->panoptic_table[k], s->panoptic_n[k], NULL, maps[k], batch,
                                         m->rows, m->cols, classes, connectivity, min_area, 0, regions, NULL);
        if (rc != MBN_OK) return rc;
    }
    if (ragged)
        return mbn_panoptic_ragged_i32(s->panoptic, s->readout, pq_u64, scored_i32, NULL, NULL, NULL, NULL, s->panoptic_comp[0],
                                       (const mbn_region *)s->panoptic_table[0], s->panoptic_n[0], regions, s->panoptic_comp[1],
                                       (const mbn_region *)s->panoptic_table[1], s->panoptic_n[1], regions, classes, NULL);
    return mbn_panoptic_i32(s->panoptic, pq_u64, scored_i32, NULL, NULL, NULL, NULL, s->panoptic_comp[0], (const mbn_region *)s->panoptic_table[0],
                            s->panoptic_n[0], regions, s->panoptic_comp[1], (const mbn_region *)s->panoptic_table[1], s->panoptic_n[1], regions, batch,
                            m->rows, m->cols, classes, NULL);
}

/* The half-width of the two boundary calls: d > 0 as given; d == 0 from ratio, for a uniform call mbn_boundary_d of the map size (*d_out), for
 * an image call every image's own, uploaded to net->seg.boundary_d (*d_items; *d_out is not read by the ragged forms then) */
static int boundary_half_width(mbn_net *net, const struct mbn_seg_maps *m, double ratio, int d, int *d_out, const void **d_items)
{
    *d_out = d;
    *d_items = NULL;
    if (d < 0) return MBN_EINVAL;
    if (d > 0) return MBN_OK;
    if (m->kind == MBN_SEG_UNIFORM) {
        const int w = mbn_boundary_d(m->rows, m->cols, ratio);
        if (w < 0) return w;
        *d_out = w;
        return MBN_OK;
    }
    int32_t *host = (int32_t *)malloc((size_t)net->max_batch * sizeof(int32_t));
    if (!host) return MBN_ENOMEM;
    int rc = mbn_boundary_d_items(net->seg.readout, ratio, host);
    if (rc == MBN_OK && !net->seg.boundary_d) rc = mbn_alloc(net->ctx, (size_t)net->max_batch * sizeof(int32_t), &net->seg.boundary_d);
    if (rc == MBN_OK) rc = mbn_upload(net->ctx, net->seg.boundary_d, host, (size_t)m->batch * sizeof(int32_t));
    free(host);
    *d_out = 1;
    *d_items = net->seg.boundary_d;
    return rc;
}

int mbn_net_segment_boundary_score(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, void *trimap_u64, void *biou_u64,
                                   double ratio, int d, int edge)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m) return MBN_EINVAL;
    const void *d_items;
    const int rc = boundary_half_width(net, m, ratio, d, &d, &d_items);
    if (rc != MBN_OK) return rc;
    if (m->kind == MBN_SEG_RAGGED)
        return mbn_boundary_score_ragged_i32(net->seg.readout, trimap_u64, biou_u64, labels_i32, truth, truth_bytes, m->classes, d, d_items, edge, NULL);
    return mbn_boundary_score_i32(net->ctx, trimap_u64, biou_u64, labels_i32, truth, truth_bytes, m->classes, m->batch, m->rows, m->cols, d, edge, NULL);
}

int mbn_net_segment_boundary_depth(mbn_net *net, const void *labels_i32, void *depth_u8, double ratio, int d, int edge)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m) return MBN_EINVAL;
    const void *d_items;
    const int rc = boundary_half_width(net, m, ratio, d, &d, &d_items);
    if (rc != MBN_OK) return rc;
    if (m->kind == MBN_SEG_RAGGED) return mbn_boundary_depth_ragged(net->seg.readout, depth_u8, labels_i32, 4, d, d_items, edge, NULL);
    return mbn_boundary_depth(net->ctx, depth_u8, labels_i32, 4, m->batch, m->rows, m->cols, d, edge, NULL);
}

/* the net's one mbn_surface handle holds at least the maps m at the plan's classes */
static int surface_ready(mbn_net *net, const struct mbn_seg_maps *m)
{
    struct mbn_net_seg *s = &net->seg;
    if (s->surface && m->batch <= s->surface_batch && m->count <= s->surface_pixels && m->classes <= s->surface_classes) return MBN_OK;
    /* the new handle first: when it cannot be had, the old one stays. It is made for max_batch, so only more pixels or classes make it again */
    const int batch = net->max_batch > m->batch ? net->max_batch : m->batch;
    const int classes = m->classes > s->surface_classes ? m->classes : s->surface_classes;
    const int64_t pixels = m->count > s->surface_pixels ? m->count : s->surface_pixels;
    mbn_surface *h = NULL;
    const int rc = mbn_surface_create(net->ctx, batch, pixels, classes, &h);
    if (rc != MBN_OK) return rc;
    if (s->surface) mbn_surface_destroy(s->surface);
    s->surface = h; s->surface_batch = batch; s->surface_pixels = pixels; s->surface_classes = classes;
    return MBN_OK;
}

int mbn_net_segment_surface(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, int bins, int edge, void *surf_u64,
                            void *dist2_u32)
{
    const struct mbn_seg_maps *m = last_maps(net);
    if (!m) return MBN_EINVAL;
    const int rc = surface_ready(net, m);
    if (rc != MBN_OK) return rc;
    if (m->kind == MBN_SEG_RAGGED)
        return mbn_surface_score_ragged_i32(net->seg.surface, net->seg.readout, surf_u64, dist2_u32, labels_i32, truth, truth_bytes, m->classes, bins,
                                            edge, NULL);
    return mbn_surface_score_i32(net->seg.surface, surf_u64, dist2_u32, labels_i32, truth, truth_bytes, m->classes, bins, m->batch, m->rows, m->cols,
                                 edge, NULL);
}

void mbn_net_seg_release(mbn_net *net)
{
    struct mbn_net_seg *s = &net->seg;
    if (s->dense_logits) mbn_free(net->ctx, s->dense_logits);
    if (s->resize_buf) mbn_free(net->ctx, s->resize_buf);
    if (s->resizer) mbn_resizer_destroy(s->resizer);
    if (s->ragged) mbn_ragged_resizer_destroy(s->ragged);
    for (int i = 0; i < MBN_ENSEMBLE_MAX_VIEWS; i++)
        if (s->view_cache[i].r) mbn_resizer_destroy(s->view_cache[i].r);
    if (s->readout) mbn_ragged_readout_destroy(s->readout);
    free(s->ragged_items); free(s->label_items);
    if (s->components) mbn_components_destroy(s->components);
    if (s->boundary_d) mbn_free(net->ctx, s->boundary_d);
    if (s->surface) mbn_surface_destroy(s->surface);
    panoptic_release(net);
}
