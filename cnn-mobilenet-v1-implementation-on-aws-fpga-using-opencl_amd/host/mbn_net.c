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

#include "mbn_net_internal.h"
#include "mbn_envelope.h"

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
    net->seg.resize_filter = MBN_FILTER_BILINEAR;
    net->seg.panoptic_max_regions = MBN_NET_PANOPTIC_REGIONS;
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
    if (net->poolfc_ws) mbn_free(net->ctx, net->poolfc_ws);
    mbn_net_seg_release(net);
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
int mbn_net_dense_layers(const mbn_net *net, const mbn_layer_desc **feat, const mbn_layer_desc **fc)
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
    int rc = mbn_net_dense_layers(net, &feat, &fc);
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

int mbn_net_forward_timed(mbn_net *net, const void *images, void *logits, int batch, float *layer_ms, int n_layer_ms)
{
    if (!net || !layer_ms || n_layer_ms <= 0) return MBN_EINVAL;
    int rc = mbn_set_profiling(net->ctx, 1);
    if (rc != MBN_OK) return rc;
    rc = forward_impl(net, images, logits, batch, 0, layer_ms, n_layer_ms);
    mbn_set_profiling(net->ctx, 0);
    return rc;
}
