// mbn_i8.hip — the int8 inference mode (MBN_DT_I8) on gfx950: uint8 NHWC activations, int8 per-channel filters, exact integer sums,
// one fp32 requantization per output (include/mbn.h, "int8 inference mode", is the normative statement of the arithmetic).
//
//   conv1      fp32 3x3 convolution of the fp32 (or raw uint8) 3-channel image, requantized to uint8. A lane owns one pixel and up to 32
//              channels (a workgroup shares them, so the filter taps are wave-uniform loads); the sums are packed fp32 pairs.
//   depthwise  3x3, stride 1 / 2, TF-SAME: the column march of mbn_f32_dw.hip. A lane owns one output column and four channels (one dword
//              of the uint8 map) and walks down a segment of output rows with a three-row window in registers, loading `stride` new input
//              rows per output row. Bytes become fp32 on load (v_cvt_f32_ubyte0..3: exact), the 9 taps accumulate in packed fp32: every
//              partial sum is an integer below 9 * 255 * 127 < 2^24, so the fp32 sum IS the int32 sum.
//   pointwise  v_mfma_i32_32x32x32_i8, A = filter rows (output channels), B = pixels, the lane map proven in mbn_literal.hip. uint8
//              activations enter the signed MFMA as x ^ 0x80 = x - 128 and 128 * sum(w) is added back in int32: exact for any order and
//              tiling. Two forms. i8_pw2_k (K <= 1024: every layer of the network): persistent, a wave keeps one 32-column chunk's filter
//              rows in registers and the workgroup streams pixel tiles through two LDS buffers. i8_pw_k (K > 1024, or operands on 8 but
//              not 16 bytes, or where the staging bound of the first form fails): a wave keeps 32 pixels' K in registers (K blocks streamed
//              beyond 32 * KS) and reads the filter rows from L2. Which form, tile and grid: mbn_i8_pw_plan (host/mbn_envelope.c).
//   pool       global average: exact int32 sums of four channels per lane, one fp32 multiply by 1 / (rows * cols).
// Every index is 64-bit (plain global loads and stores, no buffer descriptors): no 32-bit offset limit.
#include "mbn_internal.h"
#include "mbn_device.h"

#include <algorithm>

namespace {

constexpr float I8_NORM_SCALE = 1.0f / 127.5f, I8_NORM_BIAS = -1.0f;

// y = acc * mult + bias, two roundings: contraction into an FMA is switched off here (the build contracts by default)
__device__ __forceinline__ float i8_affine(float acc, float m, float b)
{
#pragma clang fp contract(off)
    return acc * m + b;
}

// ... rounded half to even and clamped to [0, 255] (the ReLU6 of the layer)
__device__ __forceinline__ unsigned i8_requant(float acc, float m, float b)
{
    float y = rintf(i8_affine(acc, m, b));
    y = fminf(fmaxf(y, 0.0f), 255.0f);
    return (unsigned)y;
}

// ------------------------------------------------------------------------------------------------------------------------ conv1
// thread = one output pixel of one image and 8 * NG output channels; workgroup row blockIdx.y = which 8 * NG channels (the filter taps are
// wave-uniform loads). The 27 inputs of the pixel are loaded once; the sums are packed fp32 pairs. cin = 3.
template <bool U8IN, int NG>
__global__ __launch_bounds__(256) void i8_conv_k(uint8_t *__restrict__ out, const void *__restrict__ in_, const float *__restrict__ w,
                                                 const float *__restrict__ mult, const float *__restrict__ bias, long npix, int h, int wd,
                                                 int ho, int wo, int cout, int stride, int pad_top, int pad_left)
{
    const long pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    const int c0 = 8 * NG * blockIdx.y;
    const int ox = (int)(pix % wo);
    const long t = pix / wo;
    const int oy = (int)(t % ho);
    const long n = t / ho;
    float x[27];
#pragma unroll
    for (int ky = 0; ky < 3; ky++) {
        const int iy = oy * stride - pad_top + ky;
#pragma unroll
        for (int kx = 0; kx < 3; kx++) {
            const int ix = ox * stride - pad_left + kx;
            const bool in = iy >= 0 && iy < h && ix >= 0 && ix < wd;
            const long base = ((n * h + iy) * (long)wd + ix) * 3;
#pragma unroll
            for (int ci = 0; ci < 3; ci++) {
                float v = 0.f;
                if (in) {
                    if (U8IN) v = __fmaf_rn((float)((const uint8_t *)in_)[base + ci], I8_NORM_SCALE, I8_NORM_BIAS);
                    else v = ((const float *)in_)[base + ci];
                }
                x[(ky * 3 + kx) * 3 + ci] = v;
            }
        }
    }
    f2 acc[4 * NG];
#pragma unroll
    for (int j = 0; j < 4 * NG; j++) acc[j] = f2{ 0.f, 0.f };
#pragma unroll
    for (int tp = 0; tp < 27; tp++) {
        const f2 xx = { x[tp], x[tp] };
        const float *wr = w + (long)tp * cout + c0;
#pragma unroll
        for (int j = 0; j < 4 * NG; j++) acc[j] = __builtin_elementwise_fma(xx, f2{ wr[2 * j], wr[2 * j + 1] }, acc[j]);
    }
#pragma unroll
    for (int g = 0; g < NG; g++) {
        unsigned q[2];
#pragma unroll
        for (int h2 = 0; h2 < 2; h2++) {
            const int cb = c0 + 8 * g + 4 * h2;
            const f2 p0 = acc[4 * g + 2 * h2], p1 = acc[4 * g + 2 * h2 + 1];
            q[h2] = i8_requant(p0.x, mult[cb], bias[cb]) | (i8_requant(p0.y, mult[cb + 1], bias[cb + 1]) << 8) |
                    (i8_requant(p1.x, mult[cb + 2], bias[cb + 2]) << 16) | (i8_requant(p1.y, mult[cb + 3], bias[cb + 3]) << 24);
        }
        *reinterpret_cast<uint2 *>(out + pix * cout + c0 + 8 * g) = make_uint2(q[0], q[1]);   // cout % 8 == 0: 8-byte aligned
    }
}

// ------------------------------------------------------------------------------------------------------------------- depthwise
struct DwArgs {
    uint8_t *out;
    const uint8_t *in;
    const int8_t *w;        // [3][3][C]
    const float *mult, *bias;
    long cols_total;        // batch * wo * (C / 4): lanes of one row segment
    int h, wd, ho, wo, c4;  // c4 = C / 4
    int pad_top, pad_left, seg_rows;
};

// one input row of the window: the dwords of taps kx = 0..2 of four channels (0 outside the map), issued ahead of their use ...
// col = this lane's dword of input column ix0 in row 0 of its image; okx = which of the three columns lie inside the map
__device__ __forceinline__ void dw_fetch(unsigned (&v)[3], const DwArgs &a, const unsigned *col, const bool (&okx)[3], int iy)
{
    const bool oky = iy >= 0 && iy < a.h;
    const unsigned *r = col + (long)iy * a.wd * a.c4;
#pragma unroll
    for (int kx = 0; kx < 3; kx++) v[kx] = (oky && okx[kx]) ? r[kx * a.c4] : 0u;
}
// ... and converted to fp32 pairs (v_cvt_f32_ubyte0..3) once the row before has been computed
__device__ __forceinline__ void dw_cvt(f2 (&r)[6], const unsigned (&v)[3])
{
#pragma unroll
    for (int kx = 0; kx < 3; kx++) {
        r[2 * kx] = f2{ (float)(v[kx] & 0xffu), (float)((v[kx] >> 8) & 0xffu) };
        r[2 * kx + 1] = f2{ (float)((v[kx] >> 16) & 0xffu), (float)(v[kx] >> 24) };
    }
}

__device__ __forceinline__ void dw_emit(const f2 (&r0)[6], const f2 (&r1)[6], const f2 (&r2)[6], const f2 (&wf)[18],
                                        const float (&m)[4], const float (&b)[4], uint8_t *dst)
{
    f2 lo = { 0.f, 0.f }, hi = { 0.f, 0.f };
#pragma unroll
    for (int kx = 0; kx < 3; kx++) {
        lo = __builtin_elementwise_fma(r0[2 * kx], wf[2 * kx], lo);
        hi = __builtin_elementwise_fma(r0[2 * kx + 1], wf[2 * kx + 1], hi);
        lo = __builtin_elementwise_fma(r1[2 * kx], wf[6 + 2 * kx], lo);
        hi = __builtin_elementwise_fma(r1[2 * kx + 1], wf[6 + 2 * kx + 1], hi);
        lo = __builtin_elementwise_fma(r2[2 * kx], wf[12 + 2 * kx], lo);
        hi = __builtin_elementwise_fma(r2[2 * kx + 1], wf[12 + 2 * kx + 1], hi);
    }
    const unsigned q = i8_requant(lo.x, m[0], b[0]) | (i8_requant(lo.y, m[1], b[1]) << 8) | (i8_requant(hi.x, m[2], b[2]) << 16) |
                       (i8_requant(hi.y, m[3], b[3]) << 24);
    *reinterpret_cast<unsigned *>(dst) = q;
}

template <int S>
__global__ __launch_bounds__(256) void i8_dw_k(DwArgs a)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.cols_total) return;
    const int cg = (int)(t % a.c4);
    const long u = t / a.c4;
    const int ox = (int)(u % a.wo);
    const long n = u / a.wo;
    const int oy0 = blockIdx.y * a.seg_rows;
    int oy1 = oy0 + a.seg_rows;
    if (oy1 > a.ho) oy1 = a.ho;
    if (oy0 >= oy1) return;
    const int C = 4 * a.c4;
    f2 wf[18];                            // [ky][kx][channel pair]
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const unsigned v = reinterpret_cast<const unsigned *>(a.w + (long)k * C)[cg];
        wf[2 * k] = f2{ (float)(int8_t)(v & 0xffu), (float)(int8_t)((v >> 8) & 0xffu) };
        wf[2 * k + 1] = f2{ (float)(int8_t)((v >> 16) & 0xffu), (float)(int8_t)(v >> 24) };
    }
    float m[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { m[j] = a.mult[4 * cg + j]; b[j] = a.bias[4 * cg + j]; }
    const int ix0 = ox * S - a.pad_left;
    const unsigned *col = reinterpret_cast<const unsigned *>(a.in) + (n * a.h * (long)a.wd + ix0) * a.c4 + cg;
    const bool okx[3] = { ix0 >= 0 && ix0 < a.wd, ix0 + 1 >= 0 && ix0 + 1 < a.wd, ix0 + 2 >= 0 && ix0 + 2 < a.wd };
    uint8_t *dst = a.out + ((n * a.ho + oy0) * (long)a.wo + ox) * C + 4 * cg;
    const long row_step = (long)a.wo * C;
    f2 A[6], B[6], Cr[6];
    unsigned v0[3], v1[3];
    int iy = oy0 * S - a.pad_top;         // first input row of the window
    dw_fetch(v0, a, col, okx, iy); dw_cvt(A, v0);
    dw_fetch(v0, a, col, okx, iy + 1); dw_cvt(B, v0);
    dw_fetch(v0, a, col, okx, iy + 2); dw_cvt(Cr, v0);
    // the window rotates through (A,B,C) -> (B,C,A) -> (C,A,B) (stride 1) or (A,B,C) -> (C,A,B) -> (B,C,A) (stride 2): period 3.
    // The next output row's new input rows are fetched before this row is computed, and converted into the freed slots after it.
#define DW_STEP(R0, R1, R2, N0, N1)                                                          \
    {                                                                                       \
        const bool more = oy + 1 < oy1;                                                     \
        if (more) {                                                                         \
            if (S == 1) dw_fetch(v0, a, col, okx, iy + 3);                         \
            else { dw_fetch(v0, a, col, okx, iy + 3); dw_fetch(v1, a, col, okx, iy + 4); } \
        }                                                                                   \
        dw_emit(R0, R1, R2, wf, m, b, dst);                                                 \
        if (!more) break;                                                                   \
        if (S == 1) dw_cvt(N0, v0);                                                         \
        else { dw_cvt(N0, v0); dw_cvt(N1, v1); }                                            \
        oy++; dst += row_step; iy += S;                                                     \
    }
    int oy = oy0;
    for (;;) {
        if (S == 1) {
            DW_STEP(A, B, Cr, A, A)
            DW_STEP(B, Cr, A, B, B)
            DW_STEP(Cr, A, B, Cr, Cr)
        } else {
            DW_STEP(A, B, Cr, A, B)
            DW_STEP(Cr, A, B, Cr, A)
            DW_STEP(B, Cr, A, B, Cr)
        }
    }
#undef DW_STEP
}

// ------------------------------------------------------------------------------------------------------------------- pointwise
constexpr int PW_WAVES = 4, PW_PIX = 32 * PW_WAVES;

struct PwArgs {
    void *out;              // uint8 [M][N] or fp32 [M][N]
    const uint8_t *in;      // [M][K]
    const int8_t *w;        // [N][K]
    const float *mult, *bias;
    long m;
    int k, n;
    int nchunks, cpg, ngroups;   // 32-column chunks, chunks per workgroup, workgroups per pixel tile
};

// 8 or 16 bytes of a row at byte offset o (< limit), zero past the row; G = granule (16 when K % 16 == 0, else 8)
template <int G>
__device__ __forceinline__ i4v pw_load(const uint8_t *row, int o, int limit)
{
    i4v v = { 0, 0, 0, 0 };
    if (G == 16) {
        if (o < limit) v = *reinterpret_cast<const i4v *>(row + o);
    } else {
        if (o < limit) { const uint2 x = *reinterpret_cast<const uint2 *>(row + o); v[0] = (int)x.x; v[1] = (int)x.y; }
        if (o + 8 < limit) { const uint2 x = *reinterpret_cast<const uint2 *>(row + o + 8); v[2] = (int)x.x; v[3] = (int)x.y; }
    }
    return v;
}

__device__ __forceinline__ int pw_bytesum(i4v v)
{
    int s = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) s = __builtin_amdgcn_sdot4(v[j], 0x01010101, s, false);
    return s;
}

// KS = 32-wide k steps per K block (registers of B: 4 * KS); G = global load granule; OUTF32 = fp32 logits.
// A wave owns 32 pixels; per 32-column chunk its A operand (16 filter bytes per lane and k step) comes straight from the L2-resident filter,
// the per-row weight sums from v_dot4 over the same fragments, mult / bias / sums reach the lanes that store them by cross-lane reads.
template <int KS, int G, bool OUTF32>
__global__ __launch_bounds__(64 * PW_WAVES) void i8_pw_k(PwArgs a)
{
    constexpr int KB = 32 * KS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const long tile = blockIdx.x / a.ngroups;
    const int grp = (int)(blockIdx.x % a.ngroups);
    const long p = tile * PW_PIX + wave * 32 + li;         // this lane's pixel (B column)
    const bool pok = p < a.m;
    const uint8_t *xrow = a.in + (pok ? p : 0) * (long)a.k;
    const int nkb = (a.k + KB - 1) / KB;
    i4v bx[KS];
    auto load_b = [&](int kb) {
        const int lim = pok ? a.k - kb * KB : 0;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const i4v v = pw_load<G>(xrow + kb * KB, 32 * s + 16 * lh, lim);
#pragma unroll
            for (int j = 0; j < 4; j++) bx[s][j] = v[j] ^ (int)0x80808080u;
        }
    };
    if (nkb == 1) load_b(0);
    const int c_end = min(a.nchunks, (grp + 1) * a.cpg);
    for (int ch = grp * a.cpg; ch < c_end; ch++) {
        const int oc0 = 32 * ch, oc = oc0 + li;
        const bool ook = oc < a.n;
        const uint8_t *wr = reinterpret_cast<const uint8_t *>(a.w) + (long)(ook ? oc : 0) * a.k;
        i16v acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0;
        int ws = 0;
        for (int kb = 0; kb < nkb; kb++) {
            if (nkb > 1) load_b(kb);
            const int kv = min(KB, a.k - kb * KB);
            const int ksteps = (kv + 31) / 32, lim = ook ? kv : 0;
#pragma unroll
            for (int s = 0; s < KS; s++)
                if (s < ksteps) {
                    const i4v av = pw_load<G>(wr + (long)kb * KB, 32 * s + 16 * lh, lim);
                    ws = __builtin_amdgcn_sdot4(av[0], 0x01010101, ws, false);
                    ws = __builtin_amdgcn_sdot4(av[1], 0x01010101, ws, false);
                    ws = __builtin_amdgcn_sdot4(av[2], 0x01010101, ws, false);
                    ws = __builtin_amdgcn_sdot4(av[3], 0x01010101, ws, false);
                    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bx[s], acc, 0, 0, 0);
                }
        }
        ws += __shfl_xor(ws, 32);                            // both k halves: lane li (and li + 32) holds the sum of row oc0 + li
        const float mv = ook ? a.mult[oc] : 0.f, bv = ook ? a.bias[oc] : 0.f;
        // lane: pixel p, output channels oc0 + 8 g + 4 lh + (0..3) in acc[4 g + 0..3]
#pragma unroll
        for (int g = 0; g < 4; g++) {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int r = 8 * g + 4 * lh + j;
                const int wsum = __shfl(ws, r), exact = (int)((unsigned)acc[4 * g + j] + 128u * (unsigned)wsum);
                y[j] = i8_affine((float)exact, __shfl(mv, r), __shfl(bv, r));
            }
            const int oq = oc0 + 8 * g + 4 * lh;
            if (!pok || oq >= a.n) continue;
            if (OUTF32) {
                float *o = reinterpret_cast<float *>(a.out) + p * (long)a.n + oq;
                if ((a.n & 3) == 0 && ((uintptr_t)o & 15) == 0) *reinterpret_cast<float4 *>(o) = make_float4(y[0], y[1], y[2], y[3]);
                else
                    for (int j = 0; j < 4 && oq + j < a.n; j++) o[j] = y[j];
            } else {
                unsigned q = 0;
#pragma unroll
                for (int j = 0; j < 4; j++) q |= (unsigned)fminf(fmaxf(rintf(y[j]), 0.0f), 255.0f) << (8 * j);
                *reinterpret_cast<unsigned *>(reinterpret_cast<uint8_t *>(a.out) + p * (long)a.n + oq) = q;   // n % 8 == 0
            }
        }
    }
}

// Persistent form for K <= 1024 (every layer of the network): a wave owns one 32-column chunk and holds its filter rows (the A operand of
// every k step), their sums, mult and bias in registers for the whole launch; the workgroup's waves (chunks x groups of 32-pixel sub-tiles,
// at most 8) walk pixel
// tiles of PT pixels (grid-strided). A tile's activations are read from HBM once, x ^ 0x80 applied, into one of two LDS buffers while the
// waves multiply the other one: one barrier per tile.
struct Pw2Args {
    void *out;
    const uint8_t *in;
    const int8_t *w;
    const float *mult, *bias;
    long m, ntiles;
    int k, kp, n, pt;       // kp = K rounded up to 32; pt = pixels per tile (multiple of 32)
    int cpw;                // 32-column chunks per workgroup; the workgroup's waves are cpw x (waves / cpw): chunk x pixel sub-tile group
};

template <int KS, int MAXT, bool OUTF32>
__global__ __launch_bounds__(MAXT) void i8_pw2_k(Pw2Args a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t xs[];   // 2 x [pt][kp + 16]
    const int nthr = blockDim.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int nrep = (nthr >> 6) / a.cpw, sub0 = 32 * (wave / a.cpw);   // this wave takes sub-tiles sub0, sub0 + 32 nrep, ...
    const int oc0 = 32 * (blockIdx.y * a.cpw + wave % a.cpw), oc = oc0 + li;
    const bool ook = oc < a.n;
    const int ksteps = a.kp / 32, str = a.kp + 16, g16 = a.k % 16 == 0;
    long tile = blockIdx.x;
    if (tile >= a.ntiles) return;
    // staging: granules of 16 (8) bytes of the tile's [pt][k] activations, row by row
    const int gb = g16 ? 16 : 8, gpr = a.k / gb, ngr = a.pt * gpr;
    constexpr int MAXG = KS <= 4 ? 8 : 4;            // granules per thread and tile (the launcher sizes pt for it)
    i4v pre[MAXG];
    auto fetch = [&](long t) {
#pragma unroll
        for (int i = 0; i < MAXG; i++) {
            const int g = tid + i * nthr;
            pre[i] = i4v{ 0, 0, 0, 0 };
            if (g < ngr) {
                const long px = t * a.pt + g / gpr;
                if (px < a.m) {
                    const uint8_t *src = a.in + px * a.k + (long)(g % gpr) * gb;
                    if (g16) pre[i] = *reinterpret_cast<const i4v *>(src);
                    else { const uint2 x = *reinterpret_cast<const uint2 *>(src); pre[i][0] = (int)x.x; pre[i][1] = (int)x.y; }
                }
            }
        }
    };
    fetch(tile);                                     // the first tile's loads overlap the filter's
    // the chunk's filter rows: lane (li, lh) holds row oc, bytes 32 s + 16 lh .. + 15 of every k step s
    i4v av[KS];
    int ws = 0;
    {
        const uint8_t *wr = reinterpret_cast<const uint8_t *>(a.w) + (long)(ook ? oc : 0) * a.k;
        const int lim = ook ? a.k : 0;
#pragma unroll
        for (int s = 0; s < KS; s++) {
            av[s] = g16 ? pw_load<16>(wr, 32 * s + 16 * lh, lim) : pw_load<8>(wr, 32 * s + 16 * lh, lim);
#pragma unroll
            for (int j = 0; j < 4; j++) ws = __builtin_amdgcn_sdot4(av[s][j], 0x01010101, ws, false);
        }
    }
    ws += __shfl_xor(ws, 32);
    const float mv = ook ? a.mult[oc] : 0.f, bv = ook ? a.bias[oc] : 0.f;
    // the 16 rows this lane stores (8 g + 4 lh + j, r = 4 g + j): sum, mult and bias, gathered once — except with K > 512, where the
    // filter fragments fill the registers and the epilogue reads them across lanes instead
    constexpr bool PRE = KS < 32;
    int wsr[16];
    float mr[16], br[16];
    if (PRE)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = 8 * (r >> 2) + 4 * lh + (r & 3);
            wsr[r] = __shfl(ws, row); mr[r] = __shfl(mv, row); br[r] = __shfl(bv, row);
        }
    auto y_of = [&](int r, int accv) {
        const int row = 8 * (r >> 2) + 4 * lh + (r & 3);
        const int wsum = PRE ? wsr[r] : __shfl(ws, row);
        return i8_affine((float)(int)((unsigned)accv + 128u * (unsigned)wsum), PRE ? mr[r] : __shfl(mv, row), PRE ? br[r] : __shfl(bv, row));
    };
    const bool full16 = oc0 + 32 <= a.n && a.n % 16 == 0 && ((uintptr_t)a.out & 15) == 0;   // wave-uniform
    auto put = [&](int buf) {
        uint8_t *base = xs + (long)buf * a.pt * str;
#pragma unroll
        for (int i = 0; i < MAXG; i++) {
            const int g = tid + i * nthr;
            if (g < ngr) {
                uint8_t *d = base + (g / gpr) * str + (g % gpr) * gb;
                const i4v v = pre[i] ^ (int)0x80808080u;
                if (g16) *reinterpret_cast<i4v *>(d) = v;
                else *reinterpret_cast<uint2 *>(d) = make_uint2((unsigned)v[0], (unsigned)v[1]);
            }
        }
    };
    put(0);
    int cur = 0;
    for (; tile < a.ntiles; tile += gridDim.x) {
        const long next = tile + gridDim.x;
        if (next < a.ntiles) fetch(next);             // in flight while this tile is multiplied
        __syncthreads();
        const uint8_t *xb = xs + (long)cur * a.pt * str;
        for (int sub = sub0; sub < a.pt; sub += 32 * nrep) {
            i16v acc;
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = 0;
            const uint8_t *brow = xb + (sub + li) * str + 16 * lh;
            // With K % 32 != 0 the last k step reads row bytes [K, kp) that put() never writes (whatever the LDS held). They meet filter
            // bytes that pw_load zeroed past K, so they add nothing to acc or ws: exactness rests on that zero fill, not on the LDS.
#pragma unroll
            for (int s = 0; s < KS; s++)
                if (s < ksteps) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[s], *reinterpret_cast<const i4v *>(brow + 32 * s), acc, 0, 0, 0);
            const long p = tile * a.pt + sub + li;
            uint8_t *orow = OUTF32 ? nullptr : reinterpret_cast<uint8_t *>(a.out) + p * (long)a.n + oc0;
            if (!OUTF32 && full16) {
                // whole chunk, 16-byte aligned rows: lane (li, 0) gathers channels 0..15 of pixel li, lane (li, 1) channels 16..31 — each
                // sends the partner the two groups it does not store — and writes them with one 16-byte store
                unsigned q[4];
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    q[g] = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        q[g] |= (unsigned)fminf(fmaxf(rintf(y_of(4 * g + j, acc[4 * g + j])), 0.0f), 255.0f) << (8 * j);
                }
                const unsigned s0 = lh ? q[0] : q[2], s1 = lh ? q[1] : q[3];      // groups the partner stores
                const unsigned r0 = (unsigned)__shfl_xor((int)s0, 32), r1 = (unsigned)__shfl_xor((int)s1, 32);
                if (p < a.m) {
                    const uint4 v = lh ? make_uint4(r0, q[2], r1, q[3]) : make_uint4(q[0], r0, q[1], r1);
                    *reinterpret_cast<uint4 *>(orow + 16 * lh) = v;
                }
                continue;
            }
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int oq = oc0 + 8 * g + 4 * lh;
                float y[4];
#pragma unroll
                for (int j = 0; j < 4; j++) y[j] = y_of(4 * g + j, acc[4 * g + j]);   // every lane: y_of may read across lanes
                if (p >= a.m || oq >= a.n) continue;
                if (OUTF32) {
                    float *o = reinterpret_cast<float *>(a.out) + p * (long)a.n + oq;
                    if ((a.n & 3) == 0 && ((uintptr_t)o & 15) == 0) *reinterpret_cast<float4 *>(o) = make_float4(y[0], y[1], y[2], y[3]);
                    else
                        for (int j = 0; j < 4 && oq + j < a.n; j++) o[j] = y[j];
                } else {
                    unsigned q = 0;
#pragma unroll
                    for (int j = 0; j < 4; j++) q |= (unsigned)fminf(fmaxf(rintf(y[j]), 0.0f), 255.0f) << (8 * j);
                    *reinterpret_cast<unsigned *>(reinterpret_cast<uint8_t *>(a.out) + p * (long)a.n + oq) = q;   // n % 8 == 0
                }
            }
        }
        if (next < a.ntiles) put(cur ^ 1);            // the other buffer was last read before this iteration's barrier
        cur ^= 1;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ pool
__global__ __launch_bounds__(256) void i8_pool_k(uint8_t *__restrict__ out, const uint8_t *__restrict__ in, long total, int rows, int cols, int fr,
                                                 int fc, int c4, float inv)
{
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int cg = (int)(t % c4);
    const long n = t / c4;
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    const unsigned *src = reinterpret_cast<const unsigned *>(in) + n * rows * (long)cols * c4 + cg;
    const int npx = fr * fc;
#pragma unroll 8
    for (int i = 0; i < npx; i++) {                 // independent loads: unrolled so that eight are in flight
        const int y = i / fc, x = i - y * fc;
        const unsigned v = src[((long)y * cols + x) * c4];
        s0 += v & 0xffu; s1 += (v >> 8) & 0xffu; s2 += (v >> 16) & 0xffu; s3 += v >> 24;
    }
    auto q = [&](int s) {
        float y = rintf((float)s * inv);
        return (unsigned)fminf(fmaxf(y, 0.0f), 255.0f);
    };
    reinterpret_cast<unsigned *>(out)[t] = q(s0) | (q(s1) << 8) | (q(s2) << 16) | (q(s3) << 24);
}

}   // namespace

// ---------------------------------------------------------------------------------------------------------------------- launchers
int mbn_launch_i8_conv(const mbn_call &c, uint8_t *out, const void *in, const float *filt, int rows, int cols, int stride, int op_size)
{
    const int ho = (rows + stride - 1) / stride, wo = (cols + stride - 1) / stride;
    const int pt = c.pad_top >= 0 ? c.pad_top : (((ho - 1) * stride + 3 - rows) > 0 ? ((ho - 1) * stride + 3 - rows) / 2 : 0);
    const int pl = c.pad_left >= 0 ? c.pad_left : (((wo - 1) * stride + 3 - cols) > 0 ? ((wo - 1) * stride + 3 - cols) / 2 : 0);
    const long npix = (long)c.batch * ho * wo;
    const int g8 = op_size / 8, ng = g8 % 4 == 0 ? 4 : g8 % 2 == 0 ? 2 : 1;    // 8-channel groups per thread
    const dim3 grid((unsigned)((npix + 255) / 256), (unsigned)(g8 / ng));
    const bool u8 = (c.io_flags & MBN_IO_IN_U8) != 0;
#define I8_CONV(U, NG) hipLaunchKernelGGL((i8_conv_k<U, NG>), grid, dim3(256), 0, c.stream, out, in, filt, c.scale, c.shift, npix, rows, cols, ho, wo, \
                                          op_size, stride, pt, pl)
    if (u8) { if (ng == 4) I8_CONV(true, 4); else if (ng == 2) I8_CONV(true, 2); else I8_CONV(true, 1); }
    else { if (ng == 4) I8_CONV(false, 4); else if (ng == 2) I8_CONV(false, 2); else I8_CONV(false, 1); }
#undef I8_CONV
    return MBN_OK;
}

int mbn_launch_i8_depthwise(const mbn_call &c, uint8_t *out, const uint8_t *in, const int8_t *filt, int rows, int cols, int stride, int channels)
{
    DwArgs a;
    a.out = out; a.in = in; a.w = filt; a.mult = c.scale; a.bias = c.shift;
    a.h = c.in_rows; a.wd = c.in_cols; a.ho = rows; a.wo = cols; a.c4 = channels / 4;
    auto same = [&](int in_sz, int out_sz) { const int tot = (out_sz - 1) * stride + 3 - in_sz; return tot > 0 ? tot / 2 : 0; };
    a.pad_top = c.pad_top >= 0 ? c.pad_top : same(a.h, rows);
    a.pad_left = c.pad_left >= 0 ? c.pad_left : same(a.wd, cols);
    a.cols_total = (long)c.batch * cols * a.c4;
    // row segments: enough lanes for every CU to hold 64 waves over the launch (the tail of the last round stays short), each segment
    // at least 8 rows (a segment re-reads the 2 rows above it)
    const long want = (long)c.ctx->num_cus * 4096;
    int segs = (int)((want + a.cols_total - 1) / a.cols_total);
    if (segs > rows / 8) segs = rows / 8;
    if (segs < 1) segs = 1;
    a.seg_rows = (rows + segs - 1) / segs;
    segs = (rows + a.seg_rows - 1) / a.seg_rows;
    const dim3 grid((unsigned)((a.cols_total + 255) / 256), (unsigned)segs);
    if (stride == 1) hipLaunchKernelGGL(i8_dw_k<1>, grid, dim3(256), 0, c.stream, a);
    else hipLaunchKernelGGL(i8_dw_k<2>, grid, dim3(256), 0, c.stream, a);
    return MBN_OK;
}

template <int KS, int G>
static void pw_launch(const mbn_call &c, const PwArgs &a, unsigned blocks, bool f32)
{
    if (f32) hipLaunchKernelGGL((i8_pw_k<KS, G, true>), dim3(blocks), dim3(64 * PW_WAVES), 0, c.stream, a);
    else hipLaunchKernelGGL((i8_pw_k<KS, G, false>), dim3(blocks), dim3(64 * PW_WAVES), 0, c.stream, a);
}

template <int KS, int MAXT>
static void pw2_launch(const mbn_call &c, const Pw2Args &a, dim3 grid, int threads, size_t lds, bool f32)
{
    if (f32) hipLaunchKernelGGL((i8_pw2_k<KS, MAXT, true>), grid, dim3(threads), lds, c.stream, a);
    else hipLaunchKernelGGL((i8_pw2_k<KS, MAXT, false>), grid, dim3(threads), lds, c.stream, a);
}

int mbn_launch_i8_pointwise(const mbn_call &c, void *out, const uint8_t *in, const int8_t *filt, long m, int cin, int op_size)
{
    // every number of the launch comes from mbn_i8_pw_plan (host/mbn_envelope.c): the form, the tile, the grid, the instantiation
    const bool f32 = (c.io_flags & MBN_IO_OUT_F32) != 0;
    mbn_i8_pw_plan_t pl;
    const int rc = mbn_i8_pw_plan(m, cin, op_size, c.ctx->num_cus, (uintptr_t)in % 16 == 0 && (uintptr_t)filt % 16 == 0, f32, &pl);
    if (rc != MBN_OK) return rc;
    if (pl.form == MBN_I8_PW_PERSISTENT) {
        Pw2Args a;
        a.out = out; a.in = in; a.w = filt; a.mult = c.scale; a.bias = c.shift;
        a.m = m; a.k = cin; a.kp = pl.kp; a.n = op_size;
        a.cpw = pl.cpw;
        a.pt = pl.pt;
        a.ntiles = pl.ntiles;
        const dim3 grid((unsigned)pl.gx, (unsigned)pl.gy);
        const size_t lds = (size_t)pl.lds_bytes;
        switch (pl.ks) {
        case 1: pw2_launch<1, 512>(c, a, grid, pl.threads, lds, f32); break;
        case 2: pw2_launch<2, 512>(c, a, grid, pl.threads, lds, f32); break;
        case 4: pw2_launch<4, 512>(c, a, grid, pl.threads, lds, f32); break;
        case 8: pw2_launch<8, 512>(c, a, grid, pl.threads, lds, f32); break;
        case 16: pw2_launch<16, 512>(c, a, grid, pl.threads, lds, f32); break;
        default: pw2_launch<32, 512>(c, a, grid, pl.threads, lds, f32); break;
        }
        return MBN_OK;
    }
    PwArgs a;
    a.out = out; a.in = in; a.w = filt; a.mult = c.scale; a.bias = c.shift;
    a.m = m; a.k = cin; a.n = op_size;
    a.nchunks = pl.nchunks;
    a.cpg = pl.cpg;
    a.ngroups = pl.ngroups;
    if (pl.pt != PW_PIX || pl.threads != 64 * PW_WAVES) return MBN_EINVAL;   // the kernel's own tile: 4 waves x 32 pixels
    const unsigned blocks = (unsigned)pl.gx;
    const bool g16 = pl.g == 16;
    if (pl.ks == 4) { if (g16) pw_launch<4, 16>(c, a, blocks, f32); else pw_launch<4, 8>(c, a, blocks, f32); }
    else if (pl.ks == 16) { if (g16) pw_launch<16, 16>(c, a, blocks, f32); else pw_launch<16, 8>(c, a, blocks, f32); }
    else { if (g16) pw_launch<32, 16>(c, a, blocks, f32); else pw_launch<32, 8>(c, a, blocks, f32); }
    return MBN_OK;
}

int mbn_launch_i8_pool(const mbn_call &c, uint8_t *out, const uint8_t *in, int rows, int cols, int fs, int channels)
{
    const int fr = fs < rows ? fs : rows, fc = fs < cols ? fs : cols;
    const long total = (long)c.batch * (channels / 4);
    const float inv = 1.0f / (float)(fr * fc);
    hipLaunchKernelGGL(i8_pool_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.stream, out, in, total, rows, cols, fr, fc, channels / 4, inv);
    return MBN_OK;
}
