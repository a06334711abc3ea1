// mbn_f32_dw_dil.hip — dilated (atrous) 3x3 depthwise, stride 1, rate D = 2 or 4, NHWC, + folded-BN scale/shift + ReLU/ReLU6 for
// gfx950 (fp32 or bf16 storage, fp32 arithmetic): the depthwise layers behind the point where output_stride 16 / 8 stops
// subsampling (mbn_plan_build_os). As HBM-bound as the undilated layers, on maps four times the pixels at output_stride 8.
//
// Polyphase column march. A rate-D convolution is D x D independent ordinary 3x3 convolutions on the sub-grids of rows = py and
// columns = px (mod D): output (oy, ox) reads inputs (oy + (ky - 1) D, ox + (kx - 1) D), all of its own phase. So the lane of
// dw3x3_nhwc (mbn_f32_dw.hip) is kept as it is — 4 consecutive channels of TW = 2 output columns, a 3 x (TW + 2) fp32 window in
// registers, one new input row per output row, each input element requested (TW + 2) / TW times — and only its pitches change:
// the lane's columns are D apart, and it walks down the rows of its row phase in steps of D. The window therefore does not grow
// with D (a ring of 2 D + 1 rows would: 9 rows x 4 columns x 4 channels = 144 VGPRs for D = 4, beside 44 for the taps and
// scale / shift, against the 48 + 44 this form shares with dw3x3_nhwc — the register budget that lets four and more waves per
// SIMD keep their row loads in flight).
// Lane layout: CW lanes along channels (CW * 16 contiguous bytes of one pixel, as in dw3x3_nhwc), then the column phase px, then
// the lane-column inside the phase — so D neighbouring lane groups read D neighbouring pixels and a wave's loads of one window
// column cover runs of D whole pixels; the left / right window columns of a lane are the centre columns of the lanes TW * D
// pixels away, in the same workgroup or the next, and come from its L1. Then slab, row phase, row segment, image.
// Same taps in the same order as dw3x3_nhwc and dw_generic_nhwc (ky, kx from 0, then fma(acc, scale, shift), then the
// activation); a tap outside the image contributes fmaf(0, w, acc) = acc: the three forms and the zero-inflated (2 D + 1)^2
// filter on the generic kernel give the same bits.
#include "mbn_f32_dw.h"

namespace {

// One input row for a lane: NC channel-quads at columns ix0, ix0 + D, ..., ix0 + (NC - 1) D; zero outside the image.
template <int D, int NC, typename T>
__device__ __forceinline__ void load_row_dil(const DwArgs &a, const T *img, int iy, int ix0, int c, f4 (&r)[NC])
{
    const bool rowok = iy >= 0 && iy < a.in_rows;
    const T *row = img + ((long)iy * a.in_cols) * a.ch + c;
#pragma unroll
    for (int j = 0; j < NC; j++) {
        const int ix = ix0 + j * D;
        r[j] = (rowok && ix >= 0 && ix < a.in_cols) ? ld4(row + (long)ix * a.ch) : f4{ 0.f, 0.f, 0.f, 0.f };
    }
}

template <int D, int TW, typename T>
__global__ __launch_bounds__(256) void dw3x3_dil_nhwc(DwArgs a)
{
    constexpr int NC = TW + 2;
    if (a.prio) __builtin_amdgcn_s_setprio(3);
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.total) return;
    // lane -> (channel-in-slab fastest, column phase, lane-column of the phase, slab, row phase, segment, image)
    const int cl = (int)(t % a.cw);
    long q = t / a.cw;
    const int u = (int)(q % a.lcols);
    q /= a.lcols;
    const int slab = (int)(q % a.nslab);
    q /= a.nslab;
    const int py = (int)(q % D);
    q /= D;
    const int seg = (int)(q % a.nseg);
    const int n = (int)(q / a.nseg);
    const int c = (slab * a.cw + cl) << 2;
    const int ox0 = (u % D) + (u / D) * (TW * D);          // first output column: phase px = u % D, TW columns D apart
    // output rows py + D k of this lane: k0 <= k < k1 (a phase has ceil((rows - py) / D) rows; none when the map is shorter than D)
    const int prows = (a.rows - py + D - 1) / D;
    const int k0 = seg * a.seg_rows;
    const int k1 = min(k0 + a.seg_rows, prows);
    if (ox0 >= a.cols || k0 >= k1) return;

    f4 w[9];
#pragma unroll
    for (int k = 0; k < 9; k++) w[k] = ld4(a.filt + (long)k * a.ch + c);
    const f4 sc = a.scale ? ld4(a.scale + c) : f4{ 1.f, 1.f, 1.f, 1.f };
    const f4 sh = a.shift ? ld4(a.shift + c) : f4{ 0.f, 0.f, 0.f, 0.f };

    const T *img = reinterpret_cast<const T *>(a.in) + (long)n * a.in_rows * a.in_cols * a.ch;
    T *op = reinterpret_cast<T *>(a.out) + (((long)n * a.rows) * a.cols + ox0) * a.ch + c;
    const int ix0 = ox0 - a.pad_left;

    f4 r0[NC], r1[NC], r2[NC];
    int iy = py + k0 * D - a.pad_top;                      // tap row ky of output row oy: oy + ky D - pad_top
    load_row_dil<D, NC, T>(a, img, iy, ix0, c, r0);
    load_row_dil<D, NC, T>(a, img, iy + D, ix0, c, r1);

    for (int k = k0; k < k1; k++) {
        const int oy = py + k * D;
        load_row_dil<D, NC, T>(a, img, oy + 2 * D - a.pad_top, ix0, c, r2);
#pragma unroll
        for (int p = 0; p < TW; p++) {
            f4 acc = f4{ 0.f, 0.f, 0.f, 0.f };
            acc = fma4(r0[p], w[0], acc); acc = fma4(r0[p + 1], w[1], acc); acc = fma4(r0[p + 2], w[2], acc);
            acc = fma4(r1[p], w[3], acc); acc = fma4(r1[p + 1], w[4], acc); acc = fma4(r1[p + 2], w[5], acc);
            acc = fma4(r2[p], w[6], acc); acc = fma4(r2[p + 1], w[7], acc); acc = fma4(r2[p + 2], w[8], acc);
            acc = act4(fma4(acc, sc, sh), a.act);
            if (ox0 + p * D < a.cols) mbn_st4(op + ((long)oy * a.cols + p * D) * a.ch, acc);
        }
#pragma unroll
        for (int j = 0; j < NC; j++) { r0[j] = r1[j]; r1[j] = r2[j]; }
    }
}

template <int D, typename T>
int launch_dil(const mbn_call &c, DwArgs &a)
{
    constexpr int TW = 2;
    const int c4 = a.ch / 4;
    int cw = c4 > 16 ? 16 : c4;                            // slab of <= 16 lanes along channels (must divide C/4), as launch_dw
    while (c4 % cw) cw--;
    a.cw = cw;
    a.nslab = c4 / cw;
    const int pcols = (a.cols + D - 1) / D, prows = (a.rows + D - 1) / D;     // columns / rows of the largest phase
    a.lcols = D * ((pcols + TW - 1) / TW);
    // the row-segment rule of launch_dw per phase: the D row phases are lanes of their own, a lane's march is a phase's rows
    const bool cache_resident = (double)c.batch * ((double)a.in_rows * a.in_cols + (double)a.rows * a.cols) * a.ch * sizeof(T) < 64.0 * 1048576;
    const long row_lanes = (long)c.batch * a.lcols * c4 * D;
    int nseg = dw_march_segments(c, row_lanes, prows, 1, cache_resident);
    if (nseg > prows) nseg = prows;
    a.seg_rows = (prows + nseg - 1) / nseg;
    a.nseg = (prows + a.seg_rows - 1) / a.seg_rows;
    a.total = row_lanes * a.nseg;
    if ((a.total + 255) / 256 >= 2147483647L) return MBN_EUNSUPPORTED;
    hipLaunchKernelGGL((dw3x3_dil_nhwc<D, TW, T>), dim3((unsigned)((a.total + 255) / 256)), dim3(256), 0, c.stream, a);
    return MBN_OK;
}

}   // namespace

int mbn_launch_dw_dilated(const mbn_call &c, DwArgs &a, int dilation, int bf16)
{
    if (dilation == 2) return bf16 ? launch_dil<2, __bf16>(c, a) : launch_dil<2, float>(c, a);
    if (dilation == 4) return bf16 ? launch_dil<4, __bf16>(c, a) : launch_dil<4, float>(c, a);
    return MBN_EUNSUPPORTED;
}
