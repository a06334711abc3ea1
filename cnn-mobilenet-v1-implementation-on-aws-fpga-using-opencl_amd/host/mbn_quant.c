/*
 * mbn_quant.c — the host quantizer of the int8 inference mode (MBN_DT_I8; arithmetic: include/mbn.h, "int8 inference mode").
 *
 * From the plan's fp32 blob (BatchNorm folded, mbn_plan.c) and one activation scale per layer it writes the i8 blob:
 * per layer, in order, [int8 filter][mult (out_ch fp32)][bias (out_ch fp32)], each segment 256-byte aligned like the
 * fp32 blob's. conv1 keeps its fp32 filter in the fp32 blob (no filter segment here); the pool has no segment.
 */
#include <math.h>
#include <string.h>

#include "mbn.h"

#define I8_DEFAULT_SCALE (6.0f / 255.0f)

static int64_t align_bytes(int64_t x) { return (x + 255) & ~(int64_t)255; }

static int8_t quant_w(float w, float inv)
{
    float q = rintf(w * inv);                   /* float product, round half to even (default rounding mode) */
    if (q > 127.f) q = 127.f;
    if (q < -127.f) q = -127.f;
    return (int8_t)q;
}

/* the kernels' coverage (mbn.h): channel counts multiples of 8, K <= 65536, no dilated depthwise */
static int layer_supported(const mbn_layer_desc *l, int i)
{
    switch (l->kind) {
    case MBN_L_CONV: return i == 0 && l->out_ch % 8 == 0 && l->in_ch > 0 && l->stride >= 1 && l->stride <= 2;
    case MBN_L_DW:   return l->in_ch == l->out_ch && l->out_ch % 8 == 0 && (l->stride == 1 || l->stride == 2) && l->dilation <= 1;
    case MBN_L_PW:   return l->in_ch % 8 == 0 && l->out_ch % 8 == 0 && l->in_ch <= 65536;
    case MBN_L_POOL: return l->in_ch % 8 == 0;
    case MBN_L_FC:   return l->in_ch % 8 == 0 && l->in_ch <= 65536 && l->out_ch > 0;
    default:         return 0;
    }
}

int mbn_quantize_i8(const mbn_plan *plan, const float *blob, const float *act_scales, mbn_i8_params *p, void *i8_blob)
{
    if (!plan || !p || (i8_blob && !blob)) return MBN_EINVAL;
    if (plan->n_layers <= 0 || plan->n_layers > MBN_MAX_LAYERS) return MBN_EINVAL;
    for (int i = 0; i < plan->n_layers; i++) {
        const mbn_layer_desc *l = &plan->layer[i];
        if (!layer_supported(l, i)) return MBN_EUNSUPPORTED;
        if (act_scales && l->kind != MBN_L_POOL && l->kind != MBN_L_FC && !(act_scales[i] > 0.f && isfinite(act_scales[i])))
            return MBN_EINVAL;
    }
    memset(p, 0, sizeof(*p));
    p->n_layers = plan->n_layers;
    int64_t off = 0;
    float s_prev = 1.0f;                        /* scale of the current activation tensor: conv1 reads the fp32 image */
    for (int i = 0; i < plan->n_layers; i++) {
        const mbn_layer_desc *l = &plan->layer[i];
        mbn_i8_layer *q = &p->layer[i];
        q->w_offset = q->mult_offset = q->bias_offset = -1;
        q->in_scale = s_prev;
        if (l->kind == MBN_L_POOL) {            /* keeps its input's scale */
            q->out_scale = s_prev;
            continue;
        }
        const int fc = l->kind == MBN_L_FC;
        const float s_out = fc ? 0.0f : (act_scales ? act_scales[i] : I8_DEFAULT_SCALE);
        q->out_scale = s_out;
        if (l->kind != MBN_L_CONV) { q->w_offset = off; off = align_bytes(off + l->w_count); }
        q->mult_offset = off; off = align_bytes(off + 4 * (int64_t)l->out_ch);
        q->bias_offset = off; off = align_bytes(off + 4 * (int64_t)l->out_ch);
        s_prev = s_out;
        if (!i8_blob) continue;

        char *b = (char *)i8_blob;
        int8_t *w8 = q->w_offset >= 0 ? (int8_t *)(b + q->w_offset) : NULL;
        float *mult = (float *)(b + q->mult_offset), *bias = (float *)(b + q->bias_offset);
        const float *w = blob + l->w_offset;
        const int C = l->out_ch;
        /* channel c's taps: pointwise / FC row c of [Cout][Cin]; depthwise [3][3][C] column c */
        const int64_t taps = l->kind == MBN_L_DW ? 9 : (l->kind == MBN_L_CONV ? 0 : l->in_ch);
        const int64_t tap_stride = l->kind == MBN_L_DW ? C : 1;
        for (int c = 0; c < C; c++) {
            const int64_t base = l->kind == MBN_L_DW ? c : (int64_t)c * taps;
            double s_w = 1.0;
            if (l->kind != MBN_L_CONV) {
                float absmax = 0.f;
                for (int64_t k = 0; k < taps; k++) {
                    const float a = fabsf(w[base + k * tap_stride]);
                    if (a > absmax) absmax = a;
                }
                if (absmax > 0.f) {
                    const float inv = 127.0f / absmax;
                    for (int64_t k = 0; k < taps; k++) w8[base + k * tap_stride] = quant_w(w[base + k * tap_stride], inv);
                    s_w = (double)absmax / 127.0;
                } else {
                    for (int64_t k = 0; k < taps; k++) w8[base + k * tap_stride] = 0;
                }
            }
            const double s_in = l->kind == MBN_L_CONV ? 1.0 : (double)q->in_scale;
            const double bn_scale = l->scale_offset >= 0 ? (double)blob[l->scale_offset + c] : 1.0;
            const double bn_shift = l->shift_offset >= 0 ? (double)blob[l->shift_offset + c] : 0.0;
            const double so = fc ? 1.0 : (double)s_out;
            mult[c] = (float)(s_w * s_in * bn_scale / so);
            bias[c] = (float)(bn_shift / so);
        }
    }
    p->blob_bytes = off;
    return MBN_OK;
}
