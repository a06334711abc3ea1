/*
 * mbn_net.c — the C host that sequences MobileNet-V1 through the C-ABI (include/mbn.h).
 *
 * Counterpart of the reference's main(): MobileNet.c:240-2763 is 29 hand-unrolled blocks, each doing
 * clCreateKernel -> readSquezeNetKernel -> clCreateBuffer x3 -> blocking H2D x2 -> clSetKernelArg ->
 * clEnqueueNDRangeKernel -> clFinish -> blocking D2H (template at MobileNet.c:322-403). Here the same
 * layer order is a loop over the plan; weights are uploaded once, activations ping-pong between two buffers
 * that stay in HBM, every call is asynchronous on the context's stream, and nothing crosses PCIe between layers.
 *
 * Plain C: this file uses nothing but the functions declared in mbn.h and the kernels' shape envelopes (mbn_envelope.h).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "mbn.h"
#include "mbn_envelope.h"

struct mbn_net {
    mbn_context *ctx;
    mbn_plan plan;
    int max_batch;
    int num_cus;               /* compute units of the context's GPU (small-batch fusion rule) */
    void *dev_blob;
    int own_blob;
    void *act[2];
    int keep;
    int dtype;                 /* MBN_DT_F32, MBN_DT_BF16 or MBN_DT_I8 */
    int fuse_stem;             /* mbn_net_set_fuse_stem (default 1) */
    int input_u8;              /* mbn_net_set_input_u8: images are raw uint8 HWC */
    unsigned fuse_blocks;      /* mbn_net_set_fuse_blocks: bit L = run the depthwise layer L and the pointwise layer L+1 as one launch */
    int fuse_blocks_set;       /* the caller chose a mask; otherwise the default of the current dtype applies */
    int use_graph;             /* mbn_net_set_graph */
    void *graph;               /* instantiated hipGraph of one forward, valid for the key below */
    int g_emul;                /* pw_emul value the graph was captured under */
    const void *g_images;
    void *g_logits;
    int g_batch, g_last, g_dtype, g_keep;
    int free_running;          /* no fork dependency on the context's stream (mbn_net_set_free_running) */
    const void *fr_images;     /* free-running: the (images, logits, batch, last_layer) of the previous forward; a call that */
    void *fr_logits;           /* differs re-inserts the fork wait, because sub-batch slices of act[] move with the batch */
    int fr_batch, fr_last, fr_ns, fr_stagger;
    int nstreams;              /* sub-batch pipelining (mbn_net_set_streams); 1 = everything on the context's stream */
    void *streams[8];
    void *bf16_filt[MBN_MAX_LAYERS];   /* bf16 copies of the pointwise / FC filters (bf16 mode) */
    unsigned char bf16_packed[MBN_MAX_LAYERS];   /* the copy is followed by its packed image (mbn_pack_filter_bf16) */
    void *keep_buf[MBN_MAX_LAYERS];
    void *logits_buf;          /* mbn_net_classify: [max_batch][classes] fp32 */
    void *dense_feat;          /* mbn_net_forward_dense: the activation in front of the pool, [max_batch][h][w][channels] at fp32 size */
    void *dense_logits;        /* mbn_net_segment: [max_batch][h][w][classes] fp32 */
    mbn_resizer *resizer;      /* mbn_net_resize_input: the resizer of the geometry below, rebuilt when it changes */
    int rs_rows, rs_cols, rs_fit, rs_filter;
    float rs_fraction;
    int resize_filter;         /* mbn_net_set_resize_filter: MBN_FILTER_* of both resizers (MBN_FILTER_BILINEAR until it is called) */
    int ragged_filter;         /* the filter `ragged` was made for */
    uint8_t pad_color[3];      /* mbn_net_set_pad_color: the border of MBN_FIT_PAD, R, G, B (black until it is called) */
    uint8_t rs_color[3], ragged_color[3];       /* the colour `resizer` / `ragged` was made for, when it is a letterbox */
    int ragged_pad;            /* `ragged` is a letterbox handle (mbn_ragged_resizer_create_pad) */
    void *resize_buf;          /* mbn_net_resize_input / _inputs: [max_batch][rows][cols][3] uint8, the resized images */
    mbn_ragged_resizer *ragged;     /* mbn_net_resize_inputs: one ragged resizer of max_batch images, made on the first call */
    mbn_resize_item *ragged_items;  /* ... and the items it is set from, [max_batch] */
    mbn_ragged_readout *readout;    /* mbn_net_segment_images: one ragged read-out of max_batch images, made on the first call */
    void *label_items;              /* ... and the items it is set from, [max_batch] mbn_label_window_item (or as many mbn_label_item) */
    int score_kind;                 /* mbn_net_segment_score: what the last successful source-size segment call wrote: SCORE_NONE, _UNIFORM, _RAGGED */
    int64_t score_count;            /* SCORE_UNIFORM: its batch * out_rows * out_cols pixels; SCORE_RAGGED: the pixels of its maps */
    int score_batch, score_rows, score_cols;   /* its batch, and SCORE_UNIFORM: the size of one map */
    mbn_components *components;     /* mbn_net_segment_regions: one handle, made on first use and again when a call needs more */
    int components_batch;           /* ... and what it holds */
    int64_t components_pixels;
    /* mbn_net_segment_panoptic: its handle and what it holds, the table size of both sides (mbn_net_set_panoptic_regions), and the buffers: both
     * segment maps and a widened uint8 truth ([panoptic_span] int32 each), both tables and both counts ([panoptic_batch] images) */
    mbn_panoptic *panoptic;
    int panoptic_batch, panoptic_regions, panoptic_max_regions;
    int64_t panoptic_span;
    void *panoptic_comp[2], *panoptic_wide, *panoptic_table[2], *panoptic_n[2];
    void *boundary_d;               /* mbn_net_segment_boundary_*: [max_batch] int32 on the device, the per-image half-widths of an image call */
    /* mbn_net_resize_views: the view resizers kept, each made for one (source size, scale, mirror, filter, pad colour); used = the clock of its last use */
    struct view_slot {
        mbn_resizer *r;
        int rows, cols, mirror, filter;
        float scale;
        uint8_t color[3];
        unsigned used;
    } view_cache[MBN_ENSEMBLE_MAX_VIEWS];
    unsigned view_clock;
    void *poolfc_ws;           /* workspace of mbn_pool_fc (1...4 images: pool + FC in one launch), allocated and zeroed at creation */
    size_t poolfc_ws_bytes;
    int fuse_tail;             /* mbn_net_set_fuse_tail (default 0) */
    int fuse_resident;         /* mbn_net_set_fuse_resident (default 1): runs of equal bf16 blocks on a small map as one launch, the map resident in LDS */
    void *last_out[MBN_MAX_LAYERS];
    /* I8 mode (mbn_quantize_i8): the quantized blob on the device, its layout, the activation scales it was made with, and the
     * host copy of the fp32 blob it is quantized from (downloaded once) */
    void *i8_blob;
    mbn_i8_params i8;
    float act_scale[MBN_MAX_LAYERS];
    float *host_blob;
};

static void panoptic_release(mbn_net *net)
{
    if (net->panoptic) mbn_panoptic_destroy(net->panoptic);
    net->panoptic = NULL;
    void **bufs[] = { &net->panoptic_comp[0], &net->panoptic_comp[1], &net->panoptic_wide, &net->panoptic_table[0], &net->panoptic_table[1],
                      &net->panoptic_n[0], &net->panoptic_n[1] };
    for (size_t i = 0; i < sizeof bufs / sizeof bufs[0]; i++) {
        if (*bufs[i]) mbn_free(net->ctx, *bufs[i]);
        *bufs[i] = NULL;
    }
    net->panoptic_batch = net->panoptic_regions = 0;
    net->panoptic_span = 0;
}

static const float *blob_at(const mbn_net *net, int64_t off)
{
    return off < 0 ? NULL : (const float *)net->dev_blob + off;
}

static int net_alloc_common(mbn_context *ctx, const mbn_plan *plan, int max_batch, mbn_net **out)
{
    if (!ctx || !plan || !out || max_batch <= 0 || plan->n_layers <= 0 || plan->n_layers > MBN_MAX_LAYERS)
        return MBN_EINVAL;
    mbn_net *net = (mbn_net *)calloc(1, sizeof(*net));
    if (!net) return MBN_ENOMEM;
    net->ctx = ctx;
    net->dtype = MBN_DT_F32;
    net->nstreams = 1;
    net->fuse_stem = 1;
    net->fuse_blocks = MBN_FUSE_BLOCKS_DEFAULT;
    net->resize_filter = MBN_FILTER_BILINEAR;
    net->panoptic_max_regions = MBN_NET_PANOPTIC_REGIONS;
    net->plan = *plan;
    net->max_batch = max_batch;
    net->num_cus = 256;
    (void)mbn_device_cus(ctx, &net->num_cus);
    size_t bytes = (size_t)plan->max_act_floats * (size_t)max_batch * sizeof(float);
    int rc = mbn_alloc(ctx, bytes, &net->act[0]);
    if (rc == MBN_OK) rc = mbn_alloc(ctx, bytes, &net->act[1]);
    net->fuse_tail = 0;            /* measured slower than the two launches (mbn.h: mbn_net_set_fuse_tail): opt-in */
    net->fuse_resident = 1;
    for (int i = 0; i < MBN_MAX_LAYERS; i++) net->act_scale[i] = 6.0f / 255.0f;
    if (rc == MBN_OK && plan->n_layers >= 2 && plan->layer[plan->n_layers - 2].kind == MBN_L_POOL &&
        plan->layer[plan->n_layers - 1].kind == MBN_L_FC) {
        const mbn_layer_desc *fc = &plan->layer[plan->n_layers - 1];
        net->poolfc_ws_bytes = mbn_pool_fc_workspace_bytes(fc->in_ch, fc->out_ch);     /* 0: channels outside the kernel's envelope */
        if (net->poolfc_ws_bytes) {
            rc = mbn_alloc(ctx, net->poolfc_ws_bytes, &net->poolfc_ws);
            if (rc == MBN_OK) rc = mbn_memset(ctx, net->poolfc_ws, 0, net->poolfc_ws_bytes);
        }
    }
    if (rc != MBN_OK) { mbn_net_destroy(net); return rc; }
    *out = net;
    return MBN_OK;
}

int mbn_net_create(mbn_context *ctx, const mbn_weights *w, int max_batch, mbn_net **out)
{
    if (!w || !w->blob || !out) return MBN_EINVAL;
    *out = NULL;
    mbn_net *net = NULL;
    int rc = net_alloc_common(ctx, &w->plan, max_batch, &net);
    if (rc != MBN_OK) return rc;
    size_t bytes = (size_t)w->plan.blob_floats * sizeof(float);
    rc = mbn_alloc(ctx, bytes, &net->dev_blob);
    if (rc == MBN_OK) { net->own_blob = 1; rc = mbn_upload(ctx, net->dev_blob, w->blob, bytes); }   /* once, not per layer */
    if (rc != MBN_OK) { mbn_net_destroy(net); return rc; }
    *out = net;
    return MBN_OK;
}

int mbn_net_create_from_device_blob(mbn_context *ctx, const mbn_plan *plan, const void *dev_blob, int max_batch,
                                    mbn_net **out)
{
    if (!dev_blob || !out) return MBN_EINVAL;
    *out = NULL;
    mbn_net *net = NULL;
    int rc = net_alloc_common(ctx, plan, max_batch, &net);
    if (rc != MBN_OK) return rc;
    net->dev_blob = (void *)dev_blob;
    net->own_blob = 0;
    *out = net;
    return MBN_OK;
}

int mbn_net_destroy(mbn_net *net)
{
    if (!net) return MBN_OK;
    mbn_sync(net->ctx);
    if (net->graph) mbn_graph_destroy(net->ctx, net->graph);
    if (net->logits_buf) mbn_free(net->ctx, net->logits_buf);
    if (net->dense_feat) mbn_free(net->ctx, net->dense_feat);
    if (net->dense_logits) mbn_free(net->ctx, net->dense_logits);
    if (net->poolfc_ws) mbn_free(net->ctx, net->poolfc_ws);
    if (net->resizer) mbn_resizer_destroy(net->resizer);
    if (net->ragged) mbn_ragged_resizer_destroy(net->ragged);
    for (int i = 0; i < MBN_ENSEMBLE_MAX_VIEWS; i++)
        if (net->view_cache[i].r) mbn_resizer_destroy(net->view_cache[i].r);
    free(net->ragged_items);
    if (net->readout) mbn_ragged_readout_destroy(net->readout);
    if (net->components) mbn_components_destroy(net->components);
    if (net->boundary_d) mbn_free(net->ctx, net->boundary_d);
    panoptic_release(net);
    free(net->label_items);
    if (net->resize_buf) mbn_free(net->ctx, net->resize_buf);
    for (int j = 0; j < 8; j++)
        if (net->streams[j]) mbn_stream_destroy(net->ctx, net->streams[j]);
    for (int i = 0; i < MBN_MAX_LAYERS; i++) {
        if (net->keep_buf[i]) mbn_free(net->ctx, net->keep_buf[i]);
        if (net->bf16_filt[i]) mbn_free(net->ctx, net->bf16_filt[i]);
    }
    if (net->i8_blob) mbn_free(net->ctx, net->i8_blob);
    free(net->host_blob);
    if (net->act[0]) mbn_free(net->ctx, net->act[0]);
    if (net->act[1]) mbn_free(net->ctx, net->act[1]);
    if (net->own_blob && net->dev_blob) mbn_free(net->ctx, net->dev_blob);
    else if (net->dev_blob) mbn_forget(net->ctx, net->dev_blob, (size_t)net->plan.blob_floats * sizeof(float));   /* images derived from the caller's blob */
    free(net);
    return MBN_OK;
}

int mbn_net_plan(const mbn_net *net, mbn_plan *plan)
{
    if (!net || !plan) return MBN_EINVAL;
    *plan = net->plan;
    return MBN_OK;
}

/* I8: quantize the fp32 blob with the current activation scales and upload the result (mbn_quantize_i8). The fp32 blob is downloaded
 * once; the device blob is allocated once (its size does not depend on the scales) and rewritten after the device has gone idle. */
static int i8_quantize(mbn_net *net)
{
    mbn_i8_params p;
    int rc = mbn_quantize_i8(&net->plan, NULL, net->act_scale, &p, NULL);
    if (rc != MBN_OK) return rc;
    const size_t fbytes = (size_t)net->plan.blob_floats * sizeof(float);
    if (!net->host_blob) {
        net->host_blob = (float *)malloc(fbytes ? fbytes : 1);
        if (!net->host_blob) return MBN_ENOMEM;
        rc = mbn_download(net->ctx, net->host_blob, net->dev_blob, fbytes);
        if (rc != MBN_OK) { free(net->host_blob); net->host_blob = NULL; return rc; }
    }
    void *h = calloc(1, (size_t)p.blob_bytes ? (size_t)p.blob_bytes : 1);
    if (!h) return MBN_ENOMEM;
    rc = mbn_quantize_i8(&net->plan, net->host_blob, net->act_scale, &p, h);
    if (rc == MBN_OK) rc = mbn_sync(net->ctx);          /* no forward still reads the previous blob */
    if (rc == MBN_OK && !net->i8_blob) rc = mbn_alloc(net->ctx, (size_t)p.blob_bytes, &net->i8_blob);
    if (rc == MBN_OK) rc = mbn_upload(net->ctx, net->i8_blob, h, (size_t)p.blob_bytes);
    free(h);
    if (rc == MBN_OK) net->i8 = p;
    return rc;
}

static const void *i8_at(const mbn_net *net, int64_t off)
{
    return off < 0 ? NULL : (const char *)net->i8_blob + off;
}

int mbn_net_set_dtype(mbn_net *net, int dtype)
{
    if (!net || (dtype != MBN_DT_F32 && dtype != MBN_DT_BF16 && dtype != MBN_DT_I8)) return MBN_EINVAL;
    if (dtype == MBN_DT_I8) {
        int rc = i8_quantize(net);
        if (rc != MBN_OK) return rc;
    }
    if (dtype == MBN_DT_BF16) {
        for (int i = 0; i < net->plan.n_layers; i++) {
            const mbn_layer_desc *l = &net->plan.layer[i];
            if ((l->kind != MBN_L_PW && l->kind != MBN_L_FC) || net->bf16_filt[i]) continue;
            /* lab build only (the wide-tile GEMM measured slower and is not shipped): wide pointwise layers (Cout % 256 == 0,
             * Cin % 64 == 0) carry the packed image of their filter behind the plain bf16 copy (MBN_IO_FILT_PACKED) */
            const size_t pk = (l->kind == MBN_L_PW && mbn_lab_build()) ? mbn_packed_filter_offset(l->out_ch, l->in_ch) : 0;
            int rc = mbn_alloc(net->ctx, pk ? pk + (size_t)l->w_count * 2 : (size_t)l->w_count * 2, &net->bf16_filt[i]);
            if (rc == MBN_OK)
                rc = mbn_convert_f32_to_bf16(net->ctx, net->bf16_filt[i], blob_at(net, l->w_offset), (size_t)l->w_count, NULL);
            if (rc == MBN_OK && pk) rc = mbn_pack_filter_bf16(net->ctx, net->bf16_filt[i], l->out_ch, l->in_ch, NULL);
            if (rc != MBN_OK) return rc;
            net->bf16_packed[i] = pk != 0;
        }
        int rc = mbn_sync(net->ctx);     /* the copies are ready before any (possibly free-running) sub-stream reads them */
        if (rc != MBN_OK) return rc;
    }
    /* kept activations change element size with the dtype: drop them */
    if (dtype != net->dtype) {
        mbn_sync(net->ctx);
        for (int i = 0; i < MBN_MAX_LAYERS; i++)
            if (net->keep_buf[i]) { mbn_free(net->ctx, net->keep_buf[i]); net->keep_buf[i] = NULL; }
    }
    net->dtype = dtype;
    return MBN_OK;
}

int mbn_net_set_act_scales_i8(mbn_net *net, const float *scales, int n)
{
    if (!net || !scales || n != net->plan.n_layers) return MBN_EINVAL;
    for (int i = 0; i < n; i++) {
        const int k = net->plan.layer[i].kind;
        if (k != MBN_L_POOL && k != MBN_L_FC && !(scales[i] > 0.f && isfinite(scales[i]))) return MBN_EINVAL;
    }
    float prev[MBN_MAX_LAYERS];
    memcpy(prev, net->act_scale, sizeof(prev));
    memcpy(net->act_scale, scales, (size_t)n * sizeof(float));
    if (net->dtype != MBN_DT_I8) return MBN_OK;
    const int rc = i8_quantize(net);
    if (rc != MBN_OK) memcpy(net->act_scale, prev, sizeof(prev));
    return rc;
}

int mbn_net_get_act_scales_i8(const mbn_net *net, float *scales, int n)
{
    if (!net || !scales || n != net->plan.n_layers) return MBN_EINVAL;
    memcpy(scales, net->act_scale, (size_t)n * sizeof(float));
    return MBN_OK;
}

static int forward_impl(mbn_net *net, const void *images, void *logits, int batch, int last_layer, float *layer_ms, int n_layer_ms);
static void drop_graph(mbn_net *net);

/* max of n fp32 values (activations after ReLU6: finite, >= 0) */
static float max_f32(const float *x, size_t n)
{
    float m = 0.f;
    for (size_t i = 0; i < n; i++)
        if (x[i] > m) m = x[i];
    return m;
}

int mbn_net_calibrate_i8(mbn_net *net, const void *images, int batch)
{
    if (!net || !images || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    const int n = net->plan.n_layers;
    /* an fp32 forward with every layer's output kept, one stream, no graph; the settings are put back afterwards */
    const int dtype = net->dtype, keep = net->keep, ns = net->nstreams, graph = net->use_graph;
    drop_graph(net);                                    /* a captured forward may hold kept buffers this pass frees */
    int rc = mbn_sync(net->ctx);
    if (rc != MBN_OK) return rc;
    const mbn_layer_desc *fc = &net->plan.layer[n - 1];
    if (!net->logits_buf) rc = mbn_alloc(net->ctx, (size_t)net->max_batch * fc->out_ch * sizeof(float), &net->logits_buf);
    net->dtype = MBN_DT_F32; net->keep = 1; net->nstreams = 1; net->use_graph = 0;
    if (rc == MBN_OK) rc = forward_impl(net, images, net->logits_buf, batch, 0, NULL, 0);
    if (rc == MBN_OK) rc = mbn_sync(net->ctx);
    float scales[MBN_MAX_LAYERS];
    float *h = NULL;
    size_t cap = 0;
    for (int i = 0; i < n && rc == MBN_OK; i++) {
        const mbn_layer_desc *l = &net->plan.layer[i];
        scales[i] = net->act_scale[i];
        if (l->kind == MBN_L_POOL || l->kind == MBN_L_FC) continue;
        const size_t cnt = (size_t)l->out_rows * l->out_cols * l->out_ch * (size_t)batch;
        if (cnt > cap) {
            free(h);
            h = (float *)malloc(cnt * sizeof(float));
            cap = h ? cnt : 0;
            if (!h) { rc = MBN_ENOMEM; break; }
        }
        rc = mbn_download(net->ctx, h, net->last_out[i], cnt * sizeof(float));
        if (rc != MBN_OK) break;
        const float mx = max_f32(h, cnt);
        scales[i] = (mx > 0.f ? (mx < 6.f ? mx : 6.f) : 6.f) / 255.0f;
    }
    free(h);
    /* the kept fp32 buffers were made for this pass only */
    if (!keep || dtype != MBN_DT_F32)
        for (int i = 0; i < MBN_MAX_LAYERS; i++)
            if (net->keep_buf[i]) { mbn_free(net->ctx, net->keep_buf[i]); net->keep_buf[i] = NULL; }
    for (int i = 0; i < MBN_MAX_LAYERS; i++) net->last_out[i] = NULL;
    net->dtype = dtype; net->keep = keep; net->nstreams = ns; net->use_graph = graph;
    if (rc != MBN_OK) return rc;
    return mbn_net_set_act_scales_i8(net, scales, n);
}

int mbn_net_set_streams(mbn_net *net, int n)
{
    if (!net || n < 1 || n > 8) return MBN_EINVAL;
    for (int j = 0; j < n; j++)
        if (!net->streams[j]) {
            int rc = mbn_stream_create(net->ctx, &net->streams[j]);
            if (rc != MBN_OK) return rc;
        }
    net->nstreams = n;
    net->fr_images = NULL;             /* the next multi-stream forward orders itself behind the previous one's tails again */
    return MBN_OK;
}

/* The fused kernels load their parameters with 16-byte accesses and answer MBN_EUNSUPPORTED otherwise: the filter, scale and
 * shift segments of layer i must exist and start on 16 bytes. The plan's own segments are 256-byte aligned in the blob; a
 * caller's plan or device blob need not be. */
static int seg_aligned(const mbn_net *net, int64_t off)
{
    return off >= 0 && ((uintptr_t)blob_at(net, off) % 16) == 0;
}

static int layer_aligned(const mbn_net *net, int i)
{
    const mbn_layer_desc *l = &net->plan.layer[i];
    return seg_aligned(net, l->w_offset) && seg_aligned(net, l->scale_offset) && seg_aligned(net, l->shift_offset);
}

/* layers 1-3 can go through mbn_stem_fused: conv 3x3 s2 -> dw s1 -> pw inside the kernel's envelope, fp32 or bf16, nothing kept */
static int stem_fusable(const mbn_net *net, int count, int last_layer)
{
    const mbn_layer_desc *l = net->plan.layer;
    return net->fuse_stem && !net->keep && last_layer >= 3 && net->plan.n_layers >= 3 &&
           (net->dtype == MBN_DT_F32 || (net->dtype == MBN_DT_BF16 && net->bf16_filt[2])) &&
           l[0].kind == MBN_L_CONV && l[1].kind == MBN_L_DW && l[2].kind == MBN_L_PW && l[0].in_ch == 3 && l[1].stride == 1 && l[1].dilation <= 1 &&
           mbn_stem_envelope_hw(count, l[0].in_rows, l[0].in_cols, l[0].out_ch, l[2].out_ch) == MBN_OK &&
           layer_aligned(net, 0) && layer_aligned(net, 1) && layer_aligned(net, 2);
}

/* a captured graph bakes the launch list in: drop it when the fusion settings change */
static void drop_graph(mbn_net *net)
{
    if (net->graph) {
        mbn_sync(net->ctx);
        mbn_graph_destroy(net->ctx, net->graph);
        net->graph = NULL;
    }
}

int mbn_net_set_fuse_stem(mbn_net *net, int enabled)
{
    if (!net) return MBN_EINVAL;
    if (net->fuse_stem != (enabled != 0)) drop_graph(net);
    net->fuse_stem = enabled != 0;
    return MBN_OK;
}

/* the mask in force: the caller's, or the measured default of the current dtype (mbn.h) */
static unsigned fuse_mask(const mbn_net *net)
{
    if (net->fuse_blocks_set) return net->fuse_blocks;
    return net->dtype == MBN_DT_BF16 ? MBN_FUSE_BLOCKS_DEFAULT_BF16 : MBN_FUSE_BLOCKS_DEFAULT;
}

/* the block of depthwise layer i (0-based) and pointwise layer i+1 on `count` images */
static mbn_block_shape block_shape(const mbn_net *net, int i, int count)
{
    const mbn_layer_desc *d = &net->plan.layer[i], *p = d + 1;
    const mbn_block_shape s = { count, d->in_rows, d->in_cols, d->out_rows, d->out_cols, d->in_ch, p->out_ch, d->stride, d->pad_top, d->pad_left };
    return s;
}

/* layers i+1 (depthwise) and i+2 (pointwise), 0-based index i, can go through mbn_dwpw_fused(_bf16) for `count` images: fp32
 * or bf16, nothing kept, enabled in the mask, and inside the kernel's envelope (mbn_block_envelope) */
static int block_fusable(const mbn_net *net, int i, int count, int last_layer)
{
    const int bf = net->dtype == MBN_DT_BF16;
    if ((net->dtype != MBN_DT_F32 && !bf) || net->keep || i + 2 > last_layer || i + 1 >= net->plan.n_layers || i + 1 >= 32) return 0;
    if (bf && !net->bf16_filt[i + 1]) return 0;
    if (!((fuse_mask(net) >> (i + 1)) & 1u)) return 0;
    /* bf16 default: the block kernel recomputes the depthwise chunk once per 256-column tile and is bound by that VALU work,
     * so a block wider than one tile measures slower fused than as two launches; an explicit mask overrides */
    if (bf && !net->fuse_blocks_set && net->plan.layer[i + 1].out_ch > 256) return 0;
    /* default, fp32: a block kernel workgroup walks 128 output pixels through the WHOLE block (all depthwise chunks, then
     * K/2 matrix instructions per chunk, one after the other), so when the launch has fewer 128 x 128 output tiles than half
     * the compute units the two separate launches — more, shorter workgroups — are faster (batch 1: -28 us per forward,
     * break-even at batch 4-8 for blocks 4-7 and 16 for blocks 8-11: profiles/r02/i_small_batch.txt). fp32 results are
     * bit-identical either way, so the choice may depend on the batch. In bf16 the fused blocks stay (measured faster at every
     * batch from 1 up: the stand-alone bf16 pointwise has no few-tile form). */
    if (!bf && !net->fuse_blocks_set) {
        const mbn_layer_desc *q = &net->plan.layer[i + 1];
        const long tiles = (((long)count * q->out_rows * q->out_cols + 127) / 128) * ((q->out_ch + 127) / 128);
        if (tiles * 2 < net->num_cus) return 0;
    }
    const mbn_layer_desc *d = &net->plan.layer[i], *p = &net->plan.layer[i + 1];
    if (d->kind != MBN_L_DW || p->kind != MBN_L_PW || p->in_ch != d->out_ch) return 0;
    if (d->dilation > 1) return 0;                      /* no fused kernel has a dilation: a dilated depthwise layer is its own launch */
    if (!layer_aligned(net, i) || !layer_aligned(net, i + 1)) return 0;
    const mbn_block_shape s = block_shape(net, i, count);
    return mbn_block_envelope(&s, net->dtype) == MBN_OK;
}

/* Blocks starting at layer index i (0-based; depthwise, pointwise, depthwise, ...) that can run as ONE launch with the map resident in LDS
 * (mbn_blocks_resident_bf16, round 6): bf16, each of them fusable under the mask in force and inside mbn_resident_envelope, all on the first
 * block's map. Returns the number of blocks (2 or more) or 0. The five 256 -> 256 blocks on the 10 x 10 map of the 0.5x160 network (layers 14-23). */
static int resident_run(const mbn_net *net, int i, int count, int last_layer)
{
    if (net->dtype != MBN_DT_BF16 || !net->fuse_resident || net->keep) return 0;
    const mbn_layer_desc *d0 = &net->plan.layer[i];
    int k = 0;
    while (block_fusable(net, i + 2 * k, count, last_layer)) {      /* (never a dilated block: block_fusable refuses it) */
        const mbn_layer_desc *d = &net->plan.layer[i + 2 * k];
        const mbn_block_shape s = block_shape(net, i + 2 * k, count);
        if (d->in_rows != d0->in_rows || d->in_cols != d0->in_cols || mbn_resident_envelope(&s, k + 1) != MBN_OK) break;
        k++;
    }
    return k >= 2 ? k : 0;
}

/* Layers i+1 ... i+5 (0-based index i) are the network's last two blocks and the global pool in the shape mbn_tail_resident_bf16 takes (round 6): bf16, nothing
 * kept, resident launches enabled, both blocks enabled in the mask in force and inside mbn_tail_envelope, the pool over the whole map of the second block
 * (layers 24-28 of the 0.5x160 network). The kernel takes only (rows, cols, c0, c1) and assumes the rest, so the layers' chain is checked here. */
static int tail_run(const mbn_net *net, int i, int count, int last_layer)
{
    if (net->dtype != MBN_DT_BF16 || !net->fuse_resident || net->keep || i + 5 > last_layer || i + 5 > net->plan.n_layers || i + 4 >= 32) return 0;
    const mbn_layer_desc *d0 = &net->plan.layer[i], *p0 = &net->plan.layer[i + 1], *d1 = &net->plan.layer[i + 2], *p1 = &net->plan.layer[i + 3],
                         *po = &net->plan.layer[i + 4];
    if (d0->kind != MBN_L_DW || p0->kind != MBN_L_PW || d1->kind != MBN_L_DW || p1->kind != MBN_L_PW || po->kind != MBN_L_POOL) return 0;
    if (d0->dilation > 1 || d1->dilation > 1) return 0;     /* an output_stride 16 / 8 plan: the kernel has no dilation */
    if (!net->bf16_filt[i + 1] || !net->bf16_filt[i + 3]) return 0;
    const unsigned mask = fuse_mask(net);
    if (!((mask >> (i + 1)) & 1u) || !((mask >> (i + 3)) & 1u)) return 0;
    for (int k = i; k < i + 4; k++)
        if (!layer_aligned(net, k)) return 0;
    if (p0->in_ch != d0->out_ch || p1->in_ch != d1->out_ch) return 0;
    if (po->in_rows != d1->out_rows || po->in_cols != d1->out_cols || po->out_ch != p1->out_ch || po->out_rows != 1 || po->out_cols != 1) return 0;
    const mbn_block_shape b0 = block_shape(net, i, count), b1 = block_shape(net, i + 2, count);
    return mbn_tail_envelope(&b0, &b1) == MBN_OK;
}

/* layers i+1 (pool) and i+2 (FC), 0-based index i, as one launch: fp32, 1...4 images, nothing kept, the last two layers of the call */
static int tail_fusable(const mbn_net *net, int i, int count, int last_layer)
{
    if (!net->fuse_tail || !net->poolfc_ws || net->dtype != MBN_DT_F32 || net->keep || count < 1 || count > 4) return 0;
    if (i + 2 != last_layer || last_layer != net->plan.n_layers) return 0;
    return net->plan.layer[i].kind == MBN_L_POOL && net->plan.layer[i + 1].kind == MBN_L_FC && seg_aligned(net, net->plan.layer[i + 1].w_offset);
}

/* Launch kinds, in the order next_launch tries them */
enum { K_STEM, K_RESIDENT, K_TAIL, K_BLOCK, K_POOLFC, K_SINGLE };

/* The launch that starts at 0-based layer i for `count` images: returns its kind, *span = the layers it covers (stem 3, resident
 * run 2k, resident tail 5, block 2, pool + FC 2, single 1). Kinds in the bit set `excluded` are skipped (the forward excludes a
 * fused kind whose call answered MBN_EUNSUPPORTED); fused_ok = 0 (per-layer timing) = single layers only. The forward, the
 * launch list and the fused-stem report all decide here, so they cannot disagree. */
static int next_launch(const mbn_net *net, int i, int count, int last_layer, int fused_ok, unsigned excluded, int *span)
{
    int k = 0;
    *span = 2;
    if (fused_ok) {
        if (i == 0 && !(excluded & (1u << K_STEM)) && stem_fusable(net, count, last_layer)) { *span = 3; return K_STEM; }
        if (!(excluded & (1u << K_RESIDENT)) && (k = resident_run(net, i, count, last_layer))) { *span = 2 * k; return K_RESIDENT; }
        if (!(excluded & (1u << K_TAIL)) && tail_run(net, i, count, last_layer)) { *span = 5; return K_TAIL; }
        if (!(excluded & (1u << K_BLOCK)) && block_fusable(net, i, count, last_layer)) return K_BLOCK;
        if (!(excluded & (1u << K_POOLFC)) && tail_fusable(net, i, count, last_layer)) return K_POOLFC;
    }
    *span = 1;
    return K_SINGLE;
}

/* the sub-batch streams a forward of `batch` images uses: per-layer timing serialises; sub-batches of fewer than 5 images are not
 * forked: they would take the 1..4-image kernels (mbn_f32_pw_splitk.hip), whose summation order differs from the single-stream
 * forward of the whole batch */
static int streams_used(const mbn_net *net, int batch, int timed)
{
    return (timed || batch < 5 * net->nstreams) ? 1 : net->nstreams;
}

int mbn_net_fused_layers(const mbn_net *net, int last_layer, int *count)
{
    if (!net || !count) return MBN_EINVAL;
    if (last_layer <= 0 || last_layer > net->plan.n_layers) last_layer = net->plan.n_layers;
    int span;
    *count = next_launch(net, 0, net->max_batch, last_layer, 1, 0, &span) == K_STEM ? 3 : 0;
    return MBN_OK;
}

int mbn_net_set_input_u8(mbn_net *net, int enabled)
{
    if (!net) return MBN_EINVAL;
    if (net->input_u8 != (enabled != 0)) drop_graph(net);
    net->input_u8 = enabled != 0;
    return MBN_OK;
}

int mbn_net_set_fuse_blocks(mbn_net *net, unsigned mask)
{
    if (!net) return MBN_EINVAL;
    /* an explicit mask also switches off the default-only rules of block_fusable (few tiles in fp32, wide blocks in bf16),
     * so the launch list can change even when the mask's value does not */
    if (fuse_mask(net) != mask || !net->fuse_blocks_set) drop_graph(net);
    net->fuse_blocks = mask;
    net->fuse_blocks_set = 1;
    return MBN_OK;
}

int mbn_net_set_fuse_tail(mbn_net *net, int enabled)
{
    if (!net) return MBN_EINVAL;
    if (net->fuse_tail != (enabled != 0)) drop_graph(net);
    net->fuse_tail = enabled != 0;
    return MBN_OK;
}

int mbn_net_set_fuse_resident(mbn_net *net, int enabled)
{
    if (!net) return MBN_EINVAL;
    if (net->fuse_resident != (enabled != 0)) drop_graph(net);
    net->fuse_resident = enabled != 0;
    return MBN_OK;
}

int mbn_net_reset_fuse_blocks(mbn_net *net)
{
    if (!net) return MBN_EINVAL;
    if (net->fuse_blocks_set) drop_graph(net);
    net->fuse_blocks_set = 0;
    net->fuse_blocks = MBN_FUSE_BLOCKS_DEFAULT;
    return MBN_OK;
}

int mbn_net_get_fuse_blocks(const mbn_net *net, unsigned *mask)
{
    if (!net || !mask) return MBN_EINVAL;
    *mask = fuse_mask(net);
    return MBN_OK;
}

int mbn_net_launches(const mbn_net *net, int batch, int last_layer, int *first_layer, int *n_layers, int capacity, int *count)
{
    if (!net || !count || batch <= 0) return MBN_EINVAL;
    if (last_layer <= 0 || last_layer > net->plan.n_layers) last_layer = net->plan.n_layers;
    const int ns = streams_used(net, batch, 0);
    const int sub = batch / ns + (batch % ns ? 1 : 0);      /* the largest sub-batch decides the envelope */
    int n = 0, span;
    for (int i = 0; i < last_layer; i += span, n++) {
        (void)next_launch(net, i, sub, last_layer, 1, 0, &span);
        if (first_layer && n_layers && n < capacity) { first_layer[n] = i + 1; n_layers[n] = span; }
    }
    *count = n;
    return MBN_OK;
}

int mbn_net_set_graph(mbn_net *net, int enabled)
{
    if (!net) return MBN_EINVAL;
    net->use_graph = enabled != 0;
    if (!enabled) drop_graph(net);
    return MBN_OK;
}

int mbn_net_set_free_running(mbn_net *net, int enabled)
{
    if (!net) return MBN_EINVAL;
    net->free_running = enabled != 0;
    net->fr_images = NULL;
    return MBN_OK;
}

int mbn_net_set_keep_activations(mbn_net *net, int keep)
{
    if (!net) return MBN_EINVAL;
    net->keep = keep != 0;
    return MBN_OK;
}

int mbn_net_layer_output(mbn_net *net, int index, void **dptr, size_t *floats_per_image)
{
    if (!net || index < 1 || index > net->plan.n_layers || !dptr) return MBN_EINVAL;
    const mbn_layer_desc *l = &net->plan.layer[index - 1];
    *dptr = net->last_out[index - 1];
    if (floats_per_image) *floats_per_image = (size_t)l->out_rows * l->out_cols * l->out_ch;
    return *dptr ? MBN_OK : MBN_ENOTFOUND;
}

/* One layer through the C-ABI: the positional arguments are kernel.cl's (see mbn.h). The FC runs on an fc_rows x fc_cols map: 1 x 1 in the
 * network's own sequence, the map in front of the pool for the dense head (mbn_net_forward_dense). */
static int run_layer_on(mbn_net *net, const mbn_layer_desc *l, const void *src, void *dst, int batch, void *stream, int fc_rows, int fc_cols)
{
    const int bf = net->dtype == MBN_DT_BF16, i8 = net->dtype == MBN_DT_I8;
    mbn_layer_ext ext;
    memset(&ext, 0, sizeof(ext));
    ext.struct_size = sizeof(ext);
    ext.batch = batch;
    ext.dtype = net->dtype;
    ext.layout = MBN_LAYOUT_NHWC;
    ext.act = MBN_ACT_RELU6;
    ext.pad_top = l->pad_top;
    ext.pad_left = l->pad_left;
    ext.scale = blob_at(net, l->scale_offset);
    ext.shift = blob_at(net, l->shift_offset);
    ext.stream = stream;
    const void *filt = blob_at(net, l->w_offset);
    if (bf && (l->kind == MBN_L_PW || l->kind == MBN_L_FC)) filt = net->bf16_filt[l->index - 1];
    if (i8) {                              /* int8 filters, mult / bias from the i8 blob; conv1 keeps its fp32 filter */
        const mbn_i8_layer *q = &net->i8.layer[l->index - 1];
        if (l->kind != MBN_L_CONV) filt = i8_at(net, q->w_offset);
        ext.scale = i8_at(net, q->mult_offset);
        ext.shift = i8_at(net, q->bias_offset);
    }
    switch (l->kind) {
    case MBN_L_CONV:                       /* MobileNet.c:268-292: rows/cols = input size, stride 2 */
        ext.cin = l->in_ch;
        if (bf) ext.io_flags = MBN_IO_IN_F32;          /* the normalised image is fp32 */
        if (net->input_u8) ext.io_flags = MBN_IO_IN_U8; /* raw image, normalised at load */
        return mbn_convolute(net->ctx, dst, src, NULL, NULL, filt, l->in_rows, l->in_cols, 3, l->stride, l->out_ch, &ext);
    case MBN_L_DW:                         /* MobileNet.c:326-381 */
        ext.in_rows = l->in_rows;
        ext.in_cols = l->in_cols;
        ext.dilation = l->dilation;        /* 0 = none; 2 / 4 on the late layers of an output_stride 16 / 8 plan */
        return mbn_depthwise(net->ctx, dst, src, filt, l->out_rows, l->out_cols, 3, l->stride, l->out_ch, &ext);
    case MBN_L_PW:                         /* MobileNet.c:417-470, with filtersize = true Cin (B3) */
        if (bf && net->bf16_packed[l->index - 1]) ext.io_flags |= MBN_IO_FILT_PACKED;
        return mbn_pointwise(net->ctx, dst, src, filt, l->out_rows, l->out_cols, l->in_ch, l->out_ch, &ext);
    case MBN_L_POOL:                       /* MobileNet.c:2603-2656; the window is clamped per side: the whole rows x cols plane */
        ext.act = MBN_ACT_NONE;
        return mbn_pool(net->ctx, dst, src, l->in_rows, l->in_cols, l->in_rows > l->in_cols ? l->in_rows : l->in_cols, l->out_ch, &ext);
    case MBN_L_FC:                         /* MobileNet.c:2682-2739: pointwise with rows = cols = 1; bias, no ReLU (B15) */
        ext.act = MBN_ACT_NONE;
        if (bf || i8) ext.io_flags = MBN_IO_OUT_F32;   /* logits stay fp32 */
        return mbn_pointwise(net->ctx, dst, src, filt, fc_rows, fc_cols, l->in_ch, l->out_ch, &ext);
    default:
        return MBN_EINVAL;
    }
}

static int run_layer(mbn_net *net, const mbn_layer_desc *l, const void *src, void *dst, int batch, void *stream)
{
    return run_layer_on(net, l, src, dst, batch, stream, 1, 1);
}

/* bytes per element of layer i's output in the current mode (FC logits are fp32 in every mode) */
static size_t out_esize(const mbn_net *net, const mbn_layer_desc *l)
{
    if (l->kind == MBN_L_FC) return 4;
    return net->dtype == MBN_DT_BF16 ? 2 : net->dtype == MBN_DT_I8 ? 1 : 4;
}

/* the parameters of the `nblocks` blocks from layer i on (depthwise i + 2k, pointwise i + 2k + 1) for the bf16 resident kernels */
static void block_params(const mbn_net *net, int i, int nblocks, mbn_block_params *bp)
{
    for (int k = 0; k < nblocks; k++) {
        const mbn_layer_desc *d = &net->plan.layer[i + 2 * k], *p = d + 1;
        bp[k].wd = blob_at(net, d->w_offset); bp[k].s2 = blob_at(net, d->scale_offset); bp[k].b2 = blob_at(net, d->shift_offset);
        bp[k].wp_bf16 = net->bf16_filt[i + 2 * k + 1]; bp[k].s3 = blob_at(net, p->scale_offset); bp[k].b3 = blob_at(net, p->shift_offset);
    }
}

/* layer i's buffer for kept activations (max_batch images at fp32 size), allocated on first use */
static int alloc_keep(mbn_net *net, int i)
{
    const mbn_layer_desc *l = &net->plan.layer[i];
    if (net->keep_buf[i]) return MBN_OK;
    return mbn_alloc(net->ctx, (size_t)l->out_rows * l->out_cols * l->out_ch * sizeof(float) * (size_t)net->max_batch, &net->keep_buf[i]);
}

/* Layers 1..last_layer for images [first, first+count) on `stream` (NULL = the context's stream). Sub-batches use
 * disjoint slices of the two ping-pong buffers, so several of them can be in flight on different streams. */
static int forward_range(mbn_net *net, const void *images, void *logits, int first, int count, int last_layer,
                         void *stream, float *layer_ms, int n_layer_ms, void *next_stream, int stagger)
{
    const size_t img_floats = (size_t)net->plan.layer[0].in_rows * net->plan.layer[0].in_cols * 3;   /* [rows][cols][3] per image */
    const char *src = (const char *)images + (size_t)first * img_floats * (net->input_u8 ? 1 : sizeof(float));
    const size_t slot = (size_t)first * (size_t)net->plan.max_act_floats * sizeof(float);
    const int bf = net->dtype == MBN_DT_BF16;
    const mbn_layer_desc *L = net->plan.layer;
    int which = 0, span;
    unsigned excluded = 0;
    for (int i = 0; i < last_layer; i += span) {
        const int kind = next_launch(net, i, count, last_layer, !layer_ms, excluded, &span);
        const int last = i + span - 1;                      /* the launch's last layer: its output is the launch's */
        const mbn_layer_desc *l = &L[i], *lp = &L[last];
        const size_t per_img = (size_t)lp->out_rows * lp->out_cols * lp->out_ch * out_esize(net, lp);
        char *dst;
        int flip = 0;
        if (last == last_layer - 1) dst = (char *)logits + (size_t)first * per_img;
        else if (net->keep) {                               /* single layers only: every fused kind refuses kept activations */
            int rc = alloc_keep(net, i);
            if (rc != MBN_OK) return rc;
            dst = (char *)net->keep_buf[i] + (size_t)first * per_img;
        } else {
            dst = (char *)net->act[which] + slot;
            flip = 1;
        }
        mbn_block_params bp[MBN_RES_MAXBLK];
        int rc;
        switch (kind) {
        case K_STEM:            /* layers 1-3 in one kernel; the 112x112x32 intermediates stay on chip */
            rc = mbn_stem_fused_hw(net->ctx, dst, src, blob_at(net, L[0].w_offset), blob_at(net, L[0].scale_offset),
                                   blob_at(net, L[0].shift_offset), blob_at(net, L[1].w_offset), blob_at(net, L[1].scale_offset),
                                   blob_at(net, L[1].shift_offset), bf ? net->bf16_filt[2] : blob_at(net, L[2].w_offset),
                                   blob_at(net, L[2].scale_offset), blob_at(net, L[2].shift_offset), count, L[0].in_rows, L[0].in_cols,
                                   L[0].out_ch, L[2].out_ch, (net->input_u8 ? MBN_STEM_IN_U8 : 0) | (bf ? MBN_STEM_BF16 : 0), stream);
            break;
        case K_RESIDENT:        /* span / 2 blocks in one launch, the map resident in LDS from the first block's input to the last block's output */
            block_params(net, i, span / 2, bp);
            rc = mbn_blocks_resident_bf16(net->ctx, dst, src, bp, span / 2, count, l->in_rows, l->in_cols, l->in_ch, stream);
            break;
        case K_TAIL:            /* the last two blocks and the pool in one launch, an image's maps resident in LDS */
            block_params(net, i, 2, bp);
            rc = mbn_tail_resident_bf16(net->ctx, dst, src, bp, count, l->in_rows, l->in_cols, l->in_ch, lp->out_ch, stream);
            break;
        case K_BLOCK:           /* depthwise + pointwise in one kernel; the depthwise output stays in LDS */
            rc = (bf ? mbn_dwpw_fused_bf16 : mbn_dwpw_fused)(
                net->ctx, dst, src, blob_at(net, l->w_offset), blob_at(net, l->scale_offset), blob_at(net, l->shift_offset),
                bf ? net->bf16_filt[i + 1] : blob_at(net, lp->w_offset), blob_at(net, lp->scale_offset),
                blob_at(net, lp->shift_offset), count, l->in_rows, l->in_cols, l->out_rows, l->out_cols, l->in_ch, lp->out_ch,
                l->stride, l->pad_top, l->pad_left, stream);
            break;
        case K_POOLFC:          /* pool + FC in one launch (1...4 images: the forward is launch-bound there) */
            rc = mbn_pool_fc(net->ctx, dst, src, blob_at(net, lp->w_offset), blob_at(net, lp->shift_offset), count, l->in_rows,
                             l->in_cols, l->out_ch, lp->out_ch, net->poolfc_ws, net->poolfc_ws_bytes, stream);
            break;
        default:
            rc = run_layer(net, l, src, dst, count, stream);
            if (rc == MBN_OK && layer_ms && i < n_layer_ms) rc = mbn_last_kernel_ms(net->ctx, &layer_ms[i]);
        }
        if (rc == MBN_EUNSUPPORTED && kind != K_SINGLE) {   /* outside the kernel's envelope: the next kind at the same layer */
            excluded |= 1u << kind;
            span = 0;
            continue;
        }
        if (rc != MBN_OK) return rc;
        excluded = 0;
        which ^= flip;
        if (first == 0) {
            for (int k = i; k < last; k++) net->last_out[k] = NULL;
            net->last_out[last] = dst;
        }
        src = dst;
        /* stagger: the next sub-batch's stream may start only when this one has finished `stagger` layers, so the
         * streams run a layer or two apart and unlike kernels (HBM-bound vs MFMA-bound) meet each other */
        if (next_stream && i < stagger && stagger <= i + span) {
            rc = mbn_stream_wait(net->ctx, next_stream, stream);
            if (rc != MBN_OK) return rc;
        }
    }
    return MBN_OK;
}

static int forward_impl(mbn_net *net, const void *images, void *logits, int batch, int last_layer, float *layer_ms, int n_layer_ms)
{
    if (!net || !images || !logits || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    const int n = net->plan.n_layers;
    if (last_layer <= 0 || last_layer > n) last_layer = n;
    const int ns = streams_used(net, batch, layer_ms != NULL);
    if (ns <= 1) net->fr_images = NULL;                /* a single-stream forward in between: the next multi-stream one forks again */
    if (ns <= 1 && net->use_graph && !layer_ms) {
        /* launch-bound batches: replay the 29 launches as one hipGraph; re-capture when the call's key changes */
        int emul = 0;
        (void)mbn_tune_get("pw_emul", &emul);              /* the arithmetic form of the pointwise layers is baked into the capture */
        if (net->g_images != images || net->g_logits != logits || net->g_batch != batch || net->g_last != last_layer ||
            net->g_dtype != net->dtype || net->g_keep != net->keep || net->g_emul != emul)
            drop_graph(net);
        if (!net->graph) {
            /* one eager pass first: kernels that allocate a workspace on first use (the pre-split filter images of pw_emul) and
             * the kept-activation buffers must have been allocated before the capture, inside which nothing may be allocated */
            int rc = forward_range(net, images, logits, 0, batch, last_layer, NULL, NULL, 0, NULL, 0);
            if (rc != MBN_OK) return rc;
            rc = mbn_graph_begin(net->ctx, NULL);
            if (rc != MBN_OK) return rc;
            rc = forward_range(net, images, logits, 0, batch, last_layer, NULL, NULL, 0, NULL, 0);
            void *g = NULL;
            int rc2 = mbn_graph_end(net->ctx, NULL, &g);     /* always close the capture */
            if (rc != MBN_OK || rc2 != MBN_OK) { if (g) mbn_graph_destroy(net->ctx, g); return rc != MBN_OK ? rc : rc2; }
            net->graph = g;
            net->g_images = images; net->g_logits = logits; net->g_batch = batch; net->g_last = last_layer;
            net->g_dtype = net->dtype; net->g_keep = net->keep; net->g_emul = emul;
        }
        return mbn_graph_launch(net->ctx, net->graph, NULL);
    }
    if (ns <= 1) return forward_range(net, images, logits, 0, batch, last_layer, NULL, layer_ms, n_layer_ms, NULL, 0);
    int stagger = 2;
    (void)mbn_tune_get("net_stagger", &stagger);
    if (stagger > last_layer) stagger = last_layer;
    /* fork: every sub-stream starts after what is already queued on the context's stream (e.g. the producer of
     * `images`); sub-batches are launched stream after stream, which staggers them by a layer or two so that one
     * stream's depthwise (HBM-bound) meets another's pointwise (MFMA-bound); join: the context's stream waits for all. */
    const int q = batch / ns, r = batch % ns;
    int first = 0;
    /* free-running skips the fork only between IDENTICAL consecutive calls: with another batch the sub-batch slices of the
     * ping-pong buffers move, with other images/logits the caller may have queued their producer/consumer on the context's
     * stream — both need the ordering back; another stream count or stagger moves the slices too */
    const int fork = !net->free_running || net->fr_images != images || net->fr_logits != logits || net->fr_batch != batch ||
                     net->fr_last != last_layer || net->fr_ns != ns || net->fr_stagger != stagger;
    net->fr_images = images; net->fr_logits = logits; net->fr_batch = batch; net->fr_last = last_layer;
    net->fr_ns = ns; net->fr_stagger = stagger;
    if (fork && net->free_running)
        for (int j = 0; j < ns; j++) {                       /* the previous free-running forward's tails, on every sub-stream */
            int rc = mbn_stream_wait(net->ctx, NULL, net->streams[j]);
            if (rc != MBN_OK) return rc;
        }
    for (int j = 0; j < ns; j++) {
        const int count = q + (j < r ? 1 : 0);
        int rc = fork ? mbn_stream_wait(net->ctx, net->streams[j], NULL) : MBN_OK;
        if (rc == MBN_OK)
            rc = forward_range(net, images, logits, first, count, last_layer, net->streams[j], NULL, 0,
                               j + 1 < ns ? net->streams[j + 1] : NULL, stagger);
        if (rc != MBN_OK) return rc;
        first += count;
    }
    for (int j = 0; j < ns; j++) {
        int rc = mbn_stream_wait(net->ctx, NULL, net->streams[j]);
        if (rc != MBN_OK) return rc;
    }
    return MBN_OK;
}

int mbn_net_forward(mbn_net *net, const void *images, void *logits, int batch, int last_layer)
{
    return forward_impl(net, images, logits, batch, last_layer, NULL, 0);
}

int mbn_net_classify(mbn_net *net, const void *images, int batch, int k, void *topk_idx_i32, void *topk_prob_f32)
{
    if (!net || !images || !topk_idx_i32 || !topk_prob_f32 || batch <= 0 || batch > net->max_batch || k < 1 || k > 8)
        return MBN_EINVAL;
    const mbn_layer_desc *fc = &net->plan.layer[net->plan.n_layers - 1];
    if (!net->logits_buf) {
        int rc = mbn_alloc(net->ctx, (size_t)net->max_batch * fc->out_ch * sizeof(float), &net->logits_buf);
        if (rc != MBN_OK) return rc;
    }
    int rc = forward_impl(net, images, net->logits_buf, batch, 0, NULL, 0);
    if (rc != MBN_OK) return rc;
    return mbn_softmax_topk_f32(net->ctx, NULL, topk_idx_i32, topk_prob_f32, net->logits_buf, batch, fc->out_ch, k, NULL);
}

/* the dense head's layers: *feat = the layer in front of the pool, *fc = the FC; MBN_EUNSUPPORTED for a plan that does not end in pool, FC */
static int dense_layers(const mbn_net *net, const mbn_layer_desc **feat, const mbn_layer_desc **fc)
{
    const int n = net->plan.n_layers;
    if (n < 3 || net->plan.layer[n - 2].kind != MBN_L_POOL || net->plan.layer[n - 1].kind != MBN_L_FC) return MBN_EUNSUPPORTED;
    *feat = &net->plan.layer[n - 3];
    *fc = &net->plan.layer[n - 1];
    if ((*fc)->in_ch != (*feat)->out_ch || (*feat)->out_rows <= 0 || (*feat)->out_cols <= 0) return MBN_EUNSUPPORTED;
    return MBN_OK;
}

int mbn_net_forward_dense(mbn_net *net, const void *images, void *dense_logits, int batch)
{
    if (!net || !images || !dense_logits || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    const mbn_layer_desc *feat, *fc;
    int rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    if (!net->dense_feat) {
        rc = mbn_alloc(net->ctx, (size_t)net->max_batch * feat->out_rows * feat->out_cols * feat->out_ch * sizeof(float), &net->dense_feat);
        if (rc != MBN_OK) { net->dense_feat = NULL; return rc; }
    }
    rc = forward_impl(net, images, net->dense_feat, batch, net->plan.n_layers - 2, NULL, 0);
    if (rc != MBN_OK) return rc;
    /* the sub-batch streams have joined the context's stream: the FC over every pixel follows on it */
    return run_layer_on(net, fc, net->dense_feat, dense_logits, batch, NULL, feat->out_rows, feat->out_cols);
}

/* the dense logits of `batch` images into net->dense_logits, [max_batch][h][w][classes] fp32, allocated on first use */
static int dense_forward(mbn_net *net, const mbn_layer_desc *feat, const mbn_layer_desc *fc, const void *images, int batch)
{
    if (!net->dense_logits) {
        const int rc = mbn_alloc(net->ctx, (size_t)net->max_batch * feat->out_rows * feat->out_cols * fc->out_ch * sizeof(float), &net->dense_logits);
        if (rc != MBN_OK) { net->dense_logits = NULL; return rc; }
    }
    return mbn_net_forward_dense(net, images, net->dense_logits, batch);
}

/* mbn_net_segment_score's record: every source-size segment call ends in one of these two, so only a successful read-out changes it */
enum { SCORE_NONE = 0, SCORE_UNIFORM = 1, SCORE_RAGGED = 2 };

static int scored_uniform(mbn_net *net, int rc, int batch, int out_rows, int out_cols)
{
    if (rc == MBN_OK) {
        net->score_kind = SCORE_UNIFORM;
        net->score_count = (int64_t)batch * out_rows * out_cols;
        net->score_batch = batch; net->score_rows = out_rows; net->score_cols = out_cols;
    }
    return rc;
}

static int scored_ragged(mbn_net *net, int rc, int batch, int64_t pixels)
{
    if (rc == MBN_OK) {
        net->score_kind = SCORE_RAGGED;
        net->score_count = pixels;
        net->score_batch = batch; net->score_rows = net->score_cols = 0;
    }
    return rc;
}

int mbn_net_segment(mbn_net *net, const void *images, int batch, void *labels_i32, void *score_f32)
{
    if (!net || !images || !labels_i32 || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    const mbn_layer_desc *feat, *fc;
    int rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols, h = feat->out_rows, w = feat->out_cols;
    const int factor = rows / h;
    if (factor * h != rows || factor * w != cols || (factor != 8 && factor != 16 && factor != 32)) return MBN_EUNSUPPORTED;
    rc = dense_forward(net, feat, fc, images, batch);
    if (rc != MBN_OK) return rc;
    return scored_uniform(net, mbn_upsample_argmax_f32(net->ctx, labels_i32, score_f32, net->dense_logits, batch, h, w, fc->out_ch, factor, NULL), batch,
                          rows, cols);
}

/* The read-out of the three source-size paths below: q = NULL is the argmax read-out (labels and score), q given the softmax read-out
 * (mbn_net_segment_prob_*: labels and prob, no score). One body per path, so both families run the same checks, resize and forward. */
typedef struct readout_prob {
    void *prob;
    float min_prob;
    int ignore_label;
} readout_prob;

/* the softmax read-out's own argument check, in front of everything else */
static int prob_status(const readout_prob *q)
{
    if (!q) return MBN_OK;
    if ((uintptr_t)q->prob % 4) return MBN_EINVAL;
    return mbn_softmax_readout_check(q->prob != NULL, q->min_prob);
}

/* The uniform read-out of the net's dense logits at out_rows x out_cols: of the window `rect` of the network's input, or (rect = NULL) of the whole
 * map. uniform_envelope is asked before the resize and the forward run; uniform_readout is the one place that chooses among the four public calls. */
static int uniform_envelope(const mbn_net *net, const mbn_layer_desc *feat, const mbn_layer_desc *fc, int batch, const int32_t *rect, int out_rows,
                            int out_cols)
{
    if (rect)
        return mbn_resample_window_envelope(batch, feat->out_rows, feat->out_cols, fc->out_ch, net->plan.layer[0].in_rows, net->plan.layer[0].in_cols,
                                            rect, out_rows, out_cols);
    /* every size is positive here (the callers' checks, dense_layers): what the plain shape can miss is a limit */
    return mbn_resample_argmax_envelope(batch, feat->out_rows, feat->out_cols, fc->out_ch, out_rows, out_cols) != MBN_OK ? MBN_EUNSUPPORTED : MBN_OK;
}

static int uniform_readout(mbn_net *net, const mbn_layer_desc *feat, const mbn_layer_desc *fc, int batch, const int32_t *rect, int out_rows,
                           int out_cols, void *labels_i32, void *score_f32, const readout_prob *q)
{
    const int h = feat->out_rows, w = feat->out_cols, rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    if (q && rect)
        return mbn_resample_softmax_window_f32(net->ctx, labels_i32, q->prob, NULL, net->dense_logits, batch, h, w, fc->out_ch, rows, cols, rect,
                                               out_rows, out_cols, q->min_prob, q->ignore_label, NULL);
    if (q)
        return mbn_resample_softmax_f32(net->ctx, labels_i32, q->prob, NULL, net->dense_logits, batch, h, w, fc->out_ch, out_rows, out_cols, q->min_prob,
                                        q->ignore_label, NULL);
    if (rect)
        return mbn_resample_argmax_window_f32(net->ctx, labels_i32, score_f32, net->dense_logits, batch, h, w, fc->out_ch, rows, cols, rect, out_rows,
                                              out_cols, NULL);
    return mbn_resample_argmax_f32(net->ctx, labels_i32, score_f32, net->dense_logits, batch, h, w, fc->out_ch, out_rows, out_cols, NULL);
}

static int segment_to(mbn_net *net, const void *images, int batch, int out_rows, int out_cols, void *labels_i32, void *score_f32, const readout_prob *q)
{
    if (!net || !images || !labels_i32 || batch <= 0 || batch > net->max_batch || out_rows <= 0 || out_cols <= 0) return MBN_EINVAL;
    if (prob_status(q) != MBN_OK) return MBN_EINVAL;
    const mbn_layer_desc *feat, *fc;
    int rc = dense_layers(net, &feat, &fc);
    if (rc == MBN_OK) rc = uniform_envelope(net, feat, fc, batch, NULL, out_rows, out_cols);
    if (rc == MBN_OK) rc = dense_forward(net, feat, fc, images, batch);
    if (rc != MBN_OK) return rc;
    return scored_uniform(net, uniform_readout(net, feat, fc, batch, NULL, out_rows, out_cols, labels_i32, score_f32, q), batch, out_rows, out_cols);
}

int mbn_net_segment_to(mbn_net *net, const void *images, int batch, int out_rows, int out_cols, void *labels_i32, void *score_f32)
{
    return segment_to(net, images, batch, out_rows, out_cols, labels_i32, score_f32, NULL);
}

int mbn_net_segment_prob_to(mbn_net *net, const void *images, int batch, int out_rows, int out_cols, void *labels_i32, void *prob_f32, float min_prob,
                            int ignore_label)
{
    const readout_prob q = { prob_f32, min_prob, ignore_label };
    return segment_to(net, images, batch, out_rows, out_cols, labels_i32, NULL, &q);
}

/* MBN_OK for the fits a source-size read-out exists for; a crop's box is fractional and the network never saw the rest of the image */
static int segment_fit_status(int fit)
{
    if (fit == MBN_FIT_STRETCH || fit == MBN_FIT_PAD) return MBN_OK;
    return fit == MBN_FIT_CROP ? MBN_EUNSUPPORTED : MBN_EINVAL;
}

static int segment_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, void *labels_i32, void *score_f32,
                       const readout_prob *q)
{
    if (!net || !src_u8 || !labels_i32 || batch <= 0 || batch > net->max_batch || in_rows <= 0 || in_cols <= 0) return MBN_EINVAL;
    if (!net->input_u8) return MBN_EINVAL;                    /* the resized images are uint8: the net must take them as such */
    if (prob_status(q) != MBN_OK) return MBN_EINVAL;
    int rc = segment_fit_status(fit);
    if (rc != MBN_OK) return rc;
    const mbn_layer_desc *feat, *fc;
    rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    int32_t pad[4];
    const int32_t *rect = NULL;                               /* a stretch reads out the whole map */
    if (fit == MBN_FIT_PAD) {
        rc = mbn_fit_pad(in_rows, in_cols, net->plan.layer[0].in_rows, net->plan.layer[0].in_cols, pad);
        if (rc != MBN_OK) return rc;
        rect = pad;
    }
    rc = uniform_envelope(net, feat, fc, batch, rect, in_rows, in_cols);
    if (rc != MBN_OK) return rc;
    void *images = NULL;
    rc = mbn_net_resize_input(net, src_u8, batch, in_rows, in_cols, fit, 1.0f, &images);
    if (rc == MBN_OK) rc = dense_forward(net, feat, fc, images, batch);
    if (rc != MBN_OK) return rc;
    return scored_uniform(net, uniform_readout(net, feat, fc, batch, rect, in_rows, in_cols, labels_i32, score_f32, q), batch, in_rows, in_cols);
}

int mbn_net_segment_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, void *labels_i32, void *score_f32)
{
    return segment_fit(net, src_u8, batch, in_rows, in_cols, fit, labels_i32, score_f32, NULL);
}

int mbn_net_segment_prob_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, void *labels_i32, void *prob_f32,
                             float min_prob, int ignore_label)
{
    const readout_prob q = { prob_f32, min_prob, ignore_label };
    return segment_fit(net, src_u8, batch, in_rows, in_cols, fit, labels_i32, NULL, &q);
}

int mbn_net_segment_images(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols, int batch,
                           void *labels_i32, const int64_t *dst_offsets, void *score_f32)
{
    return mbn_net_segment_images_fit(net, src_u8, offsets, in_rows, in_cols, batch, MBN_FIT_STRETCH, labels_i32, dst_offsets, score_f32);
}

static int segment_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols, int batch,
                              int fit, void *labels_i32, const int64_t *dst_offsets, void *score_f32, const readout_prob *q)
{
    if (!net || !src_u8 || !offsets || !in_rows || !in_cols || !labels_i32 || !dst_offsets || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    if (!net->input_u8) return MBN_EINVAL;                    /* the resized images are uint8: the net must take them as such */
    if (prob_status(q) != MBN_OK) return MBN_EINVAL;
    int rc = segment_fit_status(fit);
    if (rc != MBN_OK) return rc;
    const mbn_layer_desc *feat, *fc;
    rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    if (!net->label_items) {
        net->label_items = malloc((size_t)net->max_batch * sizeof(mbn_label_window_item));       /* either kind of item */
        if (!net->label_items) return MBN_ENOMEM;
    }
    /* a window item is a label item and then its rectangle: the first item_bytes of `it` are the item of either kind */
    const size_t item_bytes = fit == MBN_FIT_PAD ? sizeof(mbn_label_window_item) : sizeof(mbn_label_item);
    int64_t pixels = 0;
    for (int i = 0; i < batch; i++) {
        pixels += (int64_t)in_rows[i] * in_cols[i];
        int32_t rect[4] = { 0, 0, 0, 0 };
        if (fit == MBN_FIT_PAD) {
            rc = mbn_fit_pad(in_rows[i], in_cols[i], rows, cols, rect);
            if (rc != MBN_OK) return rc;
        }
        const mbn_label_window_item it = { dst_offsets[i], in_rows[i], in_cols[i], rect[0], rect[1], rect[2], rect[3] };
        memcpy((char *)net->label_items + (size_t)i * item_bytes, &it, item_bytes);
    }
    if (!net->readout) {
        rc = mbn_ragged_readout_create(net->ctx, net->max_batch, &net->readout);
        if (rc != MBN_OK) { net->readout = NULL; return rc; }
    }
    /* the set first: it checks every item, so a refusal comes before the resize and the forward run; its upload is ordered by the stream */
    rc = fit == MBN_FIT_PAD ? mbn_ragged_readout_set_window(net->readout, feat->out_rows, feat->out_cols, fc->out_ch, rows, cols, net->label_items, batch, NULL)
                            : mbn_ragged_readout_set(net->readout, feat->out_rows, feat->out_cols, fc->out_ch, net->label_items, batch, NULL);
    if (rc != MBN_OK) return rc;
    void *images = NULL;
    rc = mbn_net_resize_inputs(net, src_u8, offsets, in_rows, in_cols, batch, fit, 1.0f, &images);
    if (rc == MBN_OK) rc = dense_forward(net, feat, fc, images, batch);
    if (rc != MBN_OK) return rc;
    if (q)
        return scored_ragged(net, mbn_resample_softmax_ragged_f32(net->readout, labels_i32, q->prob, NULL, net->dense_logits, q->min_prob,
                                                                  q->ignore_label, NULL), batch, pixels);
    return scored_ragged(net, mbn_resample_argmax_ragged_f32(net->readout, labels_i32, score_f32, net->dense_logits, NULL), batch, pixels);
}

int mbn_net_segment_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols, int batch,
                               int fit, void *labels_i32, const int64_t *dst_offsets, void *score_f32)
{
    return segment_images_fit(net, src_u8, offsets, in_rows, in_cols, batch, fit, labels_i32, dst_offsets, score_f32, NULL);
}

int mbn_net_segment_prob_images_fit(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols,
                                    int batch, int fit, void *labels_i32, const int64_t *dst_offsets, void *prob_f32, float min_prob,
                                    int ignore_label)
{
    const readout_prob q = { prob_f32, min_prob, ignore_label };
    return segment_images_fit(net, src_u8, offsets, in_rows, in_cols, batch, fit, labels_i32, dst_offsets, NULL, &q);
}

int mbn_net_set_resize_filter(mbn_net *net, int filter)
{
    if (!net || filter < MBN_FILTER_NEAREST || filter > MBN_FILTER_HAMMING) return MBN_EINVAL;
    net->resize_filter = filter;                              /* the kept resizers are rebuilt by the next call that finds another filter in them */
    return MBN_OK;
}

int mbn_net_get_resize_filter(const mbn_net *net, int *filter)
{
    if (!net || !filter) return MBN_EINVAL;
    *filter = net->resize_filter;
    return MBN_OK;
}

int mbn_net_set_pad_color(mbn_net *net, int r, int g, int b)
{
    if (!net || r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255) return MBN_EINVAL;
    net->pad_color[0] = (uint8_t)r; net->pad_color[1] = (uint8_t)g; net->pad_color[2] = (uint8_t)b;     /* a kept letterbox of another colour is rebuilt */
    return MBN_OK;
}

int mbn_net_get_pad_color(const mbn_net *net, int *r, int *g, int *b)
{
    if (!net || !r || !g || !b) return MBN_EINVAL;
    *r = net->pad_color[0]; *g = net->pad_color[1]; *b = net->pad_color[2];
    return MBN_OK;
}

int mbn_net_resize_input(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int fit, float crop_fraction, void **images_u8)
{
    if (!net || !src_u8 || !images_u8 || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    *images_u8 = NULL;
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    if (fit == MBN_FIT_STRETCH || fit == MBN_FIT_PAD) crop_fraction = 1.0f;
    if (!net->resizer || net->rs_rows != in_rows || net->rs_cols != in_cols || net->rs_fit != fit || net->rs_fraction != crop_fraction ||
        net->rs_filter != net->resize_filter || (fit == MBN_FIT_PAD && memcmp(net->rs_color, net->pad_color, 3) != 0)) {
        float box[4];
        mbn_resizer *r = NULL;
        int rc = mbn_fit_box(in_rows, in_cols, rows, cols, fit, crop_fraction, box);
        if (rc == MBN_OK)
            rc = fit == MBN_FIT_PAD ? mbn_resizer_create_pad(net->ctx, net->resize_filter, in_rows, in_cols, rows, cols, net->pad_color, &r)
                                    : mbn_resizer_create_filter(net->ctx, net->resize_filter, in_rows, in_cols, box, rows, cols, &r);
        if (rc != MBN_OK) return rc;                          /* the resizer of the previous geometry stays */
        if (net->resizer) mbn_resizer_destroy(net->resizer);  /* waits for the stream: a resize still running reads its tables */
        net->resizer = r;
        net->rs_rows = in_rows; net->rs_cols = in_cols; net->rs_fit = fit; net->rs_fraction = crop_fraction; net->rs_filter = net->resize_filter;
        memcpy(net->rs_color, net->pad_color, 3);
    }
    if (!net->resize_buf) {
        int rc = mbn_alloc(net->ctx, (size_t)net->max_batch * rows * cols * 3, &net->resize_buf);
        if (rc != MBN_OK) { net->resize_buf = NULL; return rc; }
    }
    int rc = mbn_resize_u8(net->resizer, net->resize_buf, src_u8, batch, NULL);
    if (rc == MBN_OK) *images_u8 = net->resize_buf;
    return rc;
}

int mbn_net_resize_inputs(mbn_net *net, const void *src_u8, const int64_t *offsets, const int32_t *in_rows, const int32_t *in_cols, int batch, int fit,
                          float crop_fraction, void **images_u8)
{
    if (!net || !src_u8 || !offsets || !in_rows || !in_cols || !images_u8 || batch <= 0 || batch > net->max_batch) return MBN_EINVAL;
    *images_u8 = NULL;
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    const int pad = fit == MBN_FIT_PAD;
    if (fit == MBN_FIT_STRETCH || pad) crop_fraction = 1.0f;
    if (!net->ragged_items) {
        net->ragged_items = malloc((size_t)net->max_batch * sizeof(mbn_resize_item));
        if (!net->ragged_items) return MBN_ENOMEM;
    }
    for (int i = 0; i < batch; i++) {
        mbn_resize_item *it = &net->ragged_items[i];
        it->src_offset = offsets[i];
        it->rows = in_rows[i];
        it->cols = in_cols[i];
        const int rc = mbn_fit_box(in_rows[i], in_cols[i], rows, cols, fit, crop_fraction, it->box);
        if (rc != MBN_OK) return rc;
    }
    if (!net->ragged || net->ragged_filter != net->resize_filter || net->ragged_pad != pad || (pad && memcmp(net->ragged_color, net->pad_color, 3) != 0)) {
        mbn_ragged_resizer *r = NULL;                         /* HAMMING / LANCZOS: MBN_EUNSUPPORTED, and the resizer of the previous filter stays */
        const int rc = pad ? mbn_ragged_resizer_create_pad(net->ctx, net->resize_filter, net->max_batch, rows, cols, net->pad_color, &r)
                           : mbn_ragged_resizer_create_filter(net->ctx, net->resize_filter, net->max_batch, rows, cols, &r);
        if (rc != MBN_OK) return rc;
        if (net->ragged) mbn_ragged_resizer_destroy(net->ragged);       /* waits for its last launch */
        net->ragged = r;
        net->ragged_filter = net->resize_filter;
        net->ragged_pad = pad;
        memcpy(net->ragged_color, net->pad_color, 3);
    }
    if (!net->resize_buf) {
        const int rc = mbn_alloc(net->ctx, (size_t)net->max_batch * rows * cols * 3, &net->resize_buf);
        if (rc != MBN_OK) { net->resize_buf = NULL; return rc; }
    }
    int rc = mbn_ragged_resizer_set(net->ragged, net->ragged_items, batch, NULL);
    if (rc == MBN_OK) rc = mbn_resize_ragged_u8(net->ragged, net->resize_buf, src_u8, NULL);
    if (rc == MBN_OK) *images_u8 = net->resize_buf;
    return rc;
}

/* the views of (scales[k], mirrors[k]) for a source of in_rows x in_cols: what both calls below check first */
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
    struct view_slot *oldest = NULL;                              /* where a new one goes: an empty slot, else the least recently used */
    for (int i = 0; i < MBN_ENSEMBLE_MAX_VIEWS; i++) {
        struct view_slot *v = &net->view_cache[i];
        if (v->r && v->rows == in_rows && v->cols == in_cols && v->scale == scale && v->mirror == view->mirror && v->filter == net->resize_filter &&
            memcmp(v->color, net->pad_color, 3) == 0) {
            v->used = net->view_clock;
            *out = v->r;
            return MBN_OK;
        }
        if (!oldest || (oldest->r && (!v->r || (int)(v->used - oldest->used) < 0))) oldest = v;
    }
    mbn_resizer *r = NULL;
    const int rc = mbn_resizer_create_view(net->ctx, net->resize_filter, in_rows, in_cols, net->plan.layer[0].in_rows, net->plan.layer[0].in_cols, view,
                                           net->pad_color, &r);
    if (rc != MBN_OK) return rc;
    if (oldest->r) mbn_resizer_destroy(oldest->r);                /* waits for the stream: a resize still running reads its tables */
    oldest->r = r;
    oldest->rows = in_rows; oldest->cols = in_cols; oldest->scale = scale; oldest->mirror = view->mirror; oldest->filter = net->resize_filter;
    memcpy(oldest->color, net->pad_color, 3);
    oldest->used = net->view_clock;
    *out = r;
    return MBN_OK;
}

static int resize_views(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const float *scales, const mbn_view *views, int n_views,
                        void **staged)
{
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    if (!net->resize_buf) {
        const int rc = mbn_alloc(net->ctx, (size_t)net->max_batch * rows * cols * 3, &net->resize_buf);
        if (rc != MBN_OK) { net->resize_buf = NULL; return rc; }
    }
    net->view_clock++;
    for (int k = 0; k < n_views; k++) {
        mbn_resizer *r = NULL;
        int rc = view_resizer(net, in_rows, in_cols, scales[k], &views[k], &r);
        /* view-major: view k's canvases are images k * batch .. of the staging buffer */
        if (rc == MBN_OK) rc = mbn_resize_u8(r, (uint8_t *)net->resize_buf + (size_t)k * batch * rows * cols * 3, src_u8, batch, NULL);
        if (rc != MBN_OK) return rc;
    }
    *staged = net->resize_buf;
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

int mbn_net_segment_views_fit(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const float *scales, const int32_t *mirrors,
                              int n_views, void *labels_i32, void *prob_f32, void *score_f32, float min_prob, int ignore_label)
{
    if (!net || !src_u8 || !labels_i32) return MBN_EINVAL;
    if (!net->input_u8) return MBN_EINVAL;                    /* the staged canvases are uint8: the net must take them as such */
    if (((uintptr_t)labels_i32 | (uintptr_t)prob_f32 | (uintptr_t)score_f32) % 4) return MBN_EINVAL;
    /* the ensemble call's own rule: no prob map and no threshold is the argmax form */
    if ((prob_f32 || !(min_prob == 0.0f)) && mbn_softmax_readout_check(prob_f32 != NULL, min_prob) != MBN_OK) return MBN_EINVAL;
    mbn_view views[MBN_ENSEMBLE_MAX_VIEWS];
    int rc = views_of(net, batch, in_rows, in_cols, scales, mirrors, n_views, views);
    if (rc != MBN_OK) return rc;
    const mbn_layer_desc *feat, *fc;
    rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    rc = mbn_resample_ensemble_envelope(batch, feat->out_rows, feat->out_cols, fc->out_ch, rows, cols, views, n_views, in_rows, in_cols);
    if (rc != MBN_OK) return rc;
    void *images = NULL;
    rc = resize_views(net, src_u8, batch, in_rows, in_cols, scales, views, n_views, &images);
    if (rc == MBN_OK) rc = dense_forward(net, feat, fc, images, batch * n_views);
    if (rc != MBN_OK) return rc;
    return scored_uniform(net, mbn_resample_ensemble_f32(net->ctx, labels_i32, prob_f32, score_f32, net->dense_logits, batch, feat->out_rows,
                                                         feat->out_cols, fc->out_ch, rows, cols, views, n_views, in_rows, in_cols, min_prob,
                                                         ignore_label, NULL), batch, in_rows, in_cols);
}

/* the tiles of a plan the caller has checked: batch * ny * nx <= max_batch items on the net's stretch handle, one launch */
static int resize_tiles(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, const mbn_slide *s, void **staged)
{
    const int rows = net->plan.layer[0].in_rows, cols = net->plan.layer[0].in_cols;
    if (!net->ragged_items) {
        net->ragged_items = malloc((size_t)net->max_batch * sizeof(mbn_resize_item));
        if (!net->ragged_items) return MBN_ENOMEM;
    }
    int n = 0;
    for (int b = 0; b < batch; b++)
        for (int iy = 0; iy < s->ny; iy++)
            for (int ix = 0; ix < s->nx; ix++) {
                mbn_resize_item *it = &net->ragged_items[n++];          /* image b * ny * nx + iy * nx + ix of the staging buffer */
                it->src_offset = (int64_t)b * in_rows * in_cols * 3;
                it->rows = in_rows;
                it->cols = in_cols;
                it->box[0] = (float)s->x[ix]; it->box[1] = (float)s->y[iy];
                it->box[2] = (float)(s->x[ix] + s->tile_cols); it->box[3] = (float)(s->y[iy] + s->tile_rows);
            }
    if (!net->ragged || net->ragged_filter != net->resize_filter || net->ragged_pad) {
        mbn_ragged_resizer *r = NULL;                         /* HAMMING / LANCZOS: MBN_EUNSUPPORTED, and the resizer of the previous filter stays */
        const int rc = mbn_ragged_resizer_create_filter(net->ctx, net->resize_filter, net->max_batch, rows, cols, &r);
        if (rc != MBN_OK) return rc;
        if (net->ragged) mbn_ragged_resizer_destroy(net->ragged);       /* waits for its last launch */
        net->ragged = r;
        net->ragged_filter = net->resize_filter;
        net->ragged_pad = 0;
    }
    if (!net->resize_buf) {
        const int rc = mbn_alloc(net->ctx, (size_t)net->max_batch * rows * cols * 3, &net->resize_buf);
        if (rc != MBN_OK) { net->resize_buf = NULL; return rc; }
    }
    int rc = mbn_ragged_resizer_set(net->ragged, net->ragged_items, n, NULL);
    if (rc == MBN_OK) rc = mbn_resize_ragged_u8(net->ragged, net->resize_buf, src_u8, NULL);
    if (rc == MBN_OK) *staged = net->resize_buf;
    return rc;
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

int mbn_net_segment_slide(mbn_net *net, const void *src_u8, int batch, int in_rows, int in_cols, int tile_rows, int tile_cols, int stride_rows,
                          int stride_cols, void *labels_i32, void *prob_f32, void *score_f32, float min_prob, int ignore_label)
{
    if (!net || !src_u8 || !labels_i32) return MBN_EINVAL;
    if (!net->input_u8) return MBN_EINVAL;                    /* the staged tiles are uint8: the net must take them as such */
    if (((uintptr_t)labels_i32 | (uintptr_t)prob_f32 | (uintptr_t)score_f32) % 4) return MBN_EINVAL;
    /* the read-out's own rule: no prob map and no threshold is the argmax form */
    if ((prob_f32 || !(min_prob == 0.0f)) && mbn_softmax_readout_check(prob_f32 != NULL, min_prob) != MBN_OK) return MBN_EINVAL;
    if (batch <= 0) return MBN_EINVAL;
    mbn_slide s;
    int rc = mbn_slide_plan(in_rows, in_cols, tile_rows, tile_cols, stride_rows, stride_cols, &s);
    if (rc == MBN_OK) rc = slide_status(net, batch, in_rows, in_cols, &s);
    if (rc != MBN_OK) return rc;
    const mbn_layer_desc *feat, *fc;
    rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    rc = mbn_resample_slide_envelope(batch, feat->out_rows, feat->out_cols, fc->out_ch, &s, in_rows, in_cols);
    if (rc != MBN_OK) return rc;
    void *images = NULL;
    rc = resize_tiles(net, src_u8, batch, in_rows, in_cols, &s, &images);
    if (rc == MBN_OK) rc = dense_forward(net, feat, fc, images, batch * s.ny * s.nx);
    if (rc != MBN_OK) return rc;
    return scored_uniform(net, mbn_resample_slide_f32(net->ctx, labels_i32, prob_f32, score_f32, net->dense_logits, batch, feat->out_rows,
                                                      feat->out_cols, fc->out_ch, &s, in_rows, in_cols, min_prob, ignore_label, NULL), batch, in_rows,
                          in_cols);
}

int mbn_net_segment_score(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, void *counts_u64)
{
    if (!net || net->score_kind == SCORE_NONE) return MBN_EINVAL;
    const mbn_layer_desc *feat, *fc;
    const int rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    if (net->score_kind == SCORE_RAGGED) return mbn_confusion_ragged_i32(net->readout, counts_u64, labels_i32, truth, truth_bytes, fc->out_ch, NULL);
    return mbn_confusion_i32(net->ctx, counts_u64, labels_i32, truth, truth_bytes, fc->out_ch, net->score_count, NULL);
}

/* the net's one mbn_components handle holds at least the maps of the last segment call */
static int components_ready(mbn_net *net)
{
    if (net->components && net->score_batch <= net->components_batch && net->score_count <= net->components_pixels) return MBN_OK;
    /* the new handle first: when it cannot be had, the old one stays */
    const int batch = net->score_batch > net->components_batch ? net->score_batch : net->components_batch;
    const int64_t pixels = net->score_count > net->components_pixels ? net->score_count : net->components_pixels;
    mbn_components *h = NULL;
    const int rc = mbn_components_create(net->ctx, batch, pixels, &h);
    if (rc != MBN_OK) return rc;
    if (net->components) mbn_components_destroy(net->components);
    net->components = h;
    net->components_batch = batch;
    net->components_pixels = pixels;
    return MBN_OK;
}

int mbn_net_segment_regions(mbn_net *net, const void *labels_i32, void *comp_i32, mbn_region *regions, void *n_regions_i32, void *labels_out_i32,
                            int connectivity, int min_area, int ignore_label, int max_regions)
{
    if (!net || net->score_kind == SCORE_NONE) return MBN_EINVAL;
    const mbn_layer_desc *feat, *fc;
    int rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    rc = components_ready(net);
    if (rc != MBN_OK) return rc;
    if (net->score_kind == SCORE_RAGGED)
        return mbn_components_ragged_i32(net->components, net->readout, comp_i32, regions, n_regions_i32, labels_out_i32, labels_i32, fc->out_ch,
                                         connectivity, min_area, ignore_label, max_regions, NULL);
    return mbn_components_i32(net->components, comp_i32, regions, n_regions_i32, labels_out_i32, labels_i32, net->score_batch, net->score_rows,
                              net->score_cols, fc->out_ch, connectivity, min_area, ignore_label, max_regions, NULL);
}

int mbn_net_set_panoptic_regions(mbn_net *net, int max_regions)
{
    if (!net || max_regions < 1) return MBN_EINVAL;
    if (max_regions > MBN_COMPONENTS_MAX_REGIONS) return MBN_EUNSUPPORTED;
    net->panoptic_max_regions = max_regions;
    return MBN_OK;
}

/* the handle and the buffers of mbn_net_segment_panoptic hold `batch` images whose maps span `span` elements, with tables of the net's setting.
 * Everything is made again when a call needs more of any of them; a failure leaves nothing behind and the net usable */
static int panoptic_ready(mbn_net *net, int batch, int64_t span)
{
    const int regions = net->panoptic_max_regions;
    if (net->panoptic && batch <= net->panoptic_batch && span <= net->panoptic_span && regions == net->panoptic_regions) return MBN_OK;
    if (batch < net->panoptic_batch) batch = net->panoptic_batch;
    if (span < net->panoptic_span) span = net->panoptic_span;
    panoptic_release(net);                                         /* waits for the device: an earlier call may still read them */
    int rc = mbn_panoptic_create(net->ctx, batch, (int64_t)batch * regions, &net->panoptic);
    if (rc != MBN_OK) net->panoptic = NULL;
    for (int k = 0; k < 2 && rc == MBN_OK; k++) {
        rc = mbn_alloc(net->ctx, (size_t)span * 4, &net->panoptic_comp[k]);
        if (rc == MBN_OK) rc = mbn_alloc(net->ctx, (size_t)batch * regions * sizeof(mbn_region), &net->panoptic_table[k]);
        if (rc == MBN_OK) rc = mbn_alloc(net->ctx, (size_t)batch * 4, &net->panoptic_n[k]);
    }
    if (rc == MBN_OK) rc = mbn_alloc(net->ctx, (size_t)span * 4, &net->panoptic_wide);
    if (rc != MBN_OK) { panoptic_release(net); return rc; }
    net->panoptic_batch = batch;
    net->panoptic_span = span;
    net->panoptic_regions = regions;
    return MBN_OK;
}

int mbn_net_segment_panoptic(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, int connectivity, int min_area, void *pq_u64,
                             void *scored_i32)
{
    if (!net || net->score_kind == SCORE_NONE || !labels_i32 || !truth || !pq_u64 || !scored_i32) return MBN_EINVAL;
    if ((truth_bytes != 1 && truth_bytes != 4) || (truth_bytes == 4 && (uintptr_t)truth % 4)) return MBN_EINVAL;
    const mbn_layer_desc *feat, *fc;
    int rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    const int ragged = net->score_kind == SCORE_RAGGED, batch = net->score_batch, classes = fc->out_ch;
    const int64_t span = ragged ? mbn_ragged_readout_span(net->readout) : net->score_count;
    if (span < 1) return MBN_EINVAL;
    rc = components_ready(net);
    if (rc == MBN_OK) rc = panoptic_ready(net, batch, span);
    if (rc != MBN_OK) return rc;
    const int regions = net->panoptic_regions;
    const void *maps[2] = { labels_i32, truth };
    if (truth_bytes == 1) {
        /* the flat span: the gaps of a ragged set are widened too, into this private buffer only, and nothing reads them there */
        rc = mbn_widen_u8_i32(net->ctx, net->panoptic_wide, truth, span, NULL);
        if (rc != MBN_OK) return rc;
        maps[1] = net->panoptic_wide;
    }
    /* the two calls share the components handle's scratch: they are ordered by the context's stream */
    for (int k = 0; k < 2; k++) {
        rc = ragged ? mbn_components_ragged_i32(net->components, net->readout, net->panoptic_comp[k], (mbn_region *)net->panoptic_table[k],
                                                net->panoptic_n[k], NULL, maps[k], classes, connectivity, min_area, 0, regions, NULL)
                    : mbn_components_i32(net->components, net->panoptic_comp[k], (mbn_region *)net->panoptic_table[k], net->panoptic_n[k], NULL, maps[k],
                                         batch, net->score_rows, net->score_cols, classes, connectivity, min_area, 0, regions, NULL);
        if (rc != MBN_OK) return rc;
    }
    if (ragged)
        return mbn_panoptic_ragged_i32(net->panoptic, net->readout, pq_u64, scored_i32, NULL, NULL, NULL, NULL, net->panoptic_comp[0],
                                       (const mbn_region *)net->panoptic_table[0], net->panoptic_n[0], regions, net->panoptic_comp[1],
                                       (const mbn_region *)net->panoptic_table[1], net->panoptic_n[1], regions, classes, NULL);
    return mbn_panoptic_i32(net->panoptic, pq_u64, scored_i32, NULL, NULL, NULL, NULL, net->panoptic_comp[0], (const mbn_region *)net->panoptic_table[0],
                            net->panoptic_n[0], regions, net->panoptic_comp[1], (const mbn_region *)net->panoptic_table[1], net->panoptic_n[1], regions,
                            batch, net->score_rows, net->score_cols, classes, NULL);
}

/* The half-width of the two boundary calls: d > 0 as given; d == 0 from ratio, for a uniform call mbn_boundary_d of the map size (*d_out), for
 * an image call every image's own, uploaded to net->boundary_d (*d_items; *d_out is not read by the ragged forms then) */
static int boundary_half_width(mbn_net *net, double ratio, int d, int *d_out, const void **d_items)
{
    *d_out = d;
    *d_items = NULL;
    if (d < 0) return MBN_EINVAL;
    if (d > 0) return MBN_OK;
    if (net->score_kind == SCORE_UNIFORM) {
        const int w = mbn_boundary_d(net->score_rows, net->score_cols, ratio);
        if (w < 0) return w;
        *d_out = w;
        return MBN_OK;
    }
    int32_t *host = (int32_t *)malloc((size_t)net->max_batch * sizeof(int32_t));
    if (!host) return MBN_ENOMEM;
    int rc = mbn_boundary_d_items(net->readout, ratio, host);
    if (rc == MBN_OK && !net->boundary_d) rc = mbn_alloc(net->ctx, (size_t)net->max_batch * sizeof(int32_t), &net->boundary_d);
    if (rc == MBN_OK) rc = mbn_upload(net->ctx, net->boundary_d, host, (size_t)net->score_batch * sizeof(int32_t));
    free(host);
    *d_out = 1;
    *d_items = net->boundary_d;
    return rc;
}

int mbn_net_segment_boundary_score(mbn_net *net, const void *labels_i32, const void *truth, int truth_bytes, void *trimap_u64, void *biou_u64,
                                   double ratio, int d, int edge)
{
    if (!net || net->score_kind == SCORE_NONE) return MBN_EINVAL;
    const mbn_layer_desc *feat, *fc;
    int rc = dense_layers(net, &feat, &fc);
    if (rc != MBN_OK) return rc;
    const void *d_items;
    rc = boundary_half_width(net, ratio, d, &d, &d_items);
    if (rc != MBN_OK) return rc;
    if (net->score_kind == SCORE_RAGGED)
        return mbn_boundary_score_ragged_i32(net->readout, trimap_u64, biou_u64, labels_i32, truth, truth_bytes, fc->out_ch, d, d_items, edge, NULL);
    return mbn_boundary_score_i32(net->ctx, trimap_u64, biou_u64, labels_i32, truth, truth_bytes, fc->out_ch, net->score_batch, net->score_rows,
                                  net->score_cols, d, edge, NULL);
}

int mbn_net_segment_boundary_depth(mbn_net *net, const void *labels_i32, void *depth_u8, double ratio, int d, int edge)
{
    if (!net || net->score_kind == SCORE_NONE) return MBN_EINVAL;
    const void *d_items;
    const int rc = boundary_half_width(net, ratio, d, &d, &d_items);
    if (rc != MBN_OK) return rc;
    if (net->score_kind == SCORE_RAGGED) return mbn_boundary_depth_ragged(net->readout, depth_u8, labels_i32, 4, d, d_items, edge, NULL);
    return mbn_boundary_depth(net->ctx, depth_u8, labels_i32, 4, net->score_batch, net->score_rows, net->score_cols, d, edge, NULL);
}

int mbn_net_forward_timed(mbn_net *net, const void *images, void *logits, int batch, float *layer_ms, int n_layer_ms)
{
    if (!net || !layer_ms || n_layer_ms <= 0) return MBN_EINVAL;
    int rc = mbn_set_profiling(net->ctx, 1);
    if (rc != MBN_OK) return rc;
    rc = forward_impl(net, images, logits, batch, 0, layer_ms, n_layer_ms);
    mbn_set_profiling(net->ctx, 0);
    return rc;
}
