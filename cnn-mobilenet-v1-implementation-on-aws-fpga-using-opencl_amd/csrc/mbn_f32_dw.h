// mbn_f32_dw.h — what the NHWC depthwise kernel files share (mbn_f32_dw.hip: the 3x3 column march, the LDS-staged forms and the
// generic fallback; mbn_f32_dw_dil.hip: the dilated column march): the kernel arguments, the 4-channel load / fma / activation
// helpers whose fma order fixes the bits every form must reproduce, and the row-segment rule of a column march.
#pragma once
#include "mbn_internal.h"
#include "mbn_device.h"

struct DwArgs {
    void *out;
    const void *in;
    const float *filt, *scale, *shift;
    int batch, in_rows, in_cols, rows, cols, ch, pad_top, pad_left, act;
    int seg_rows, nseg;     // output rows per segment / segments per image (dilated march: rows of one phase, segments per phase)
    int prio;               // wave priority of the whole kernel (3: a memory-bound kernel beside another stream's MFMA-streaming GEMM gets its few VALU slots)
    int cw;                 // lanes along channels inside a slab (channels per slab = 4*cw)
    int nslab;              // ch / (4*cw)
    int lcols;              // lane-columns per row = ceil(cols / TW) (dilated march: D * ceil(ceil(cols / D) / TW), the column phase fastest)
    long total;             // lanes with work
};

namespace {

__device__ __forceinline__ f4 ld4(const float *p) { return *reinterpret_cast<const f4 *>(p); }
__device__ __forceinline__ f4 ld4(const __bf16 *p)
{
    const bf4 v = *reinterpret_cast<const bf4 *>(p);
    return f4{ (float)v.x, (float)v.y, (float)v.z, (float)v.w };
}
__device__ __forceinline__ f4 fma4(f4 a, f4 b, f4 c)
{
    return f4{ fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w) };
}
__device__ __forceinline__ f4 act4(f4 v, int act)
{
    if (act == MBN_ACT_RELU6) {
        v.x = fminf(fmaxf(v.x, 0.f), 6.f); v.y = fminf(fmaxf(v.y, 0.f), 6.f);
        v.z = fminf(fmaxf(v.z, 0.f), 6.f); v.w = fminf(fmaxf(v.w, 0.f), 6.f);
    } else if (act == MBN_ACT_RELU) {
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    return v;
}

// Row segments of a column march whose lanes walk `rows` output rows each; row_lanes = the lanes of a full-height march.
// Every extra segment re-reads 2 (stride 1) or 1 (stride 2) halo rows from HBM — measured as 19-36 % over-fetch (FETCH_SIZE,
// profiles/r01) when segmenting for "two full rounds" of lanes — so segment only when a full-height march leaves the chip
// under-filled: ~12 waves/CU for stride 1, ~6 for stride 2 (whose lanes keep 10 loads in flight per step), and keep >= 4 output
// rows per segment ...
// ... unless even that leaves less than one wave per CU (a few images): then the launch is bound by the length of a lane's row
// march (one dependent memory round trip per row: 9-10 us for a 14-row map at batch 1), not by bytes, and one output row per
// segment is best
// ... or the tensors sit in L2 / Infinity Cache anyway (input + output under 64 MB: 5 ... 64 images on the 14 x 14 and 7 x 7 maps):
// the halo rows an extra segment re-reads come from cache, and shorter marches are what the launch is short of — measured 1-5 us
// per launch, 2.5-4.5 % of a forward at 8 ... 32 images (profiles/r03/w_depthwise_segments_small_batch.txt).
// tools/layer_bench.py --tune dw_nseg=... is the sweep.
inline int dw_march_segments(const mbn_call &c, long row_lanes, int rows, int stride, bool cache_resident)
{
    const long target = (long)c.ctx->num_cus * 64 * (stride == 1 ? 12 : 6);
    int nseg = 1;
    if (g_mbn_tune.dw_nseg > 0) nseg = g_mbn_tune.dw_nseg;
    else if (row_lanes < target) {
        nseg = (int)((target + row_lanes - 1) / row_lanes);
        int max_seg = rows / 4 > 0 ? rows / 4 : 1;
        if (row_lanes * max_seg < (long)c.ctx->num_cus * 64 || cache_resident) max_seg = rows;
        if (nseg > max_seg) nseg = max_seg;
    }
    return nseg;
}

}   // namespace

// The dilated 3x3 column march (mbn_f32_dw_dil.hip): stride 1, dilation 2 or 4, channels % 4 == 0, pointers aligned as launch_dw's
// fast forms require; `a` carries the shape, the pads and the pointers. bf16 != 0: bf16 storage.
int mbn_launch_dw_dilated(const mbn_call &c, DwArgs &a, int dilation, int bf16);
