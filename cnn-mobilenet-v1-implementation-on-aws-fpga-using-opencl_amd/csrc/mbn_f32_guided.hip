// mbn_f32_guided.hip — the dense head's read-out along the image's edges on gfx950: joint bilateral upsampling (Kopf et al. 2007) of the per-pixel
// logits to the source size and the argmax over the classes, in one kernel (mbn_resample_guided_f32; include/mbn.h, "segment along the image's
// edges", is the normative statement of the arithmetic), and the block mean that gives the low-resolution guide (mbn_guide_reduce_u8).
//
// The four coarse neighbours of an output pixel are the bilinear ones of mbn_f32_resample.hip; each one's spatial weight wy_j * wx_k is multiplied
// by a range weight lut[d], d the L1 colour distance between the pixel of the source image (guide_hi) and the neighbour's low-resolution colour
// (guide_lo), and the four are normalised to sum 1. The weights do not depend on the class: a lane forms them ONCE in front of the class loop and
// the loop runs on registers; [out_rows][out_cols][classes] is never in memory.
//   tile    a workgroup of 256 lanes owns the 32 x 32 output tile of the resample kernels and the same fy x fx footprint of class vectors
//           (mbn_resample_window_plan: one envelope, one plan). The launch's LDS holds the footprint of one class chunk and, behind it, the
//           footprint's guide_lo colours, fy x fx x 3 bytes staged once per tile
//   weights a lane owns one output column and four consecutive rows. Four rows span less than one coarse row, so their neighbours come from the
//           3 x 2 set (ya, ya + 1, ya + 2) x (x0, x0 + 1), clamped. The six colours are read from LDS once, packed one per dword; the lane's four
//           guide_hi pixels are three byte loads each (any byte pointer). d is ONE v_sad_u8 per neighbour, g a table load, then per row the four
//           products (wy * wx) * g, their sum in the stated order and the four quotients: sixteen b in registers
//   reduce  per group of four classes the lane reads the 3 x 2 set from LDS once for its four rows (two rows of it where no row of the wave
//           crosses a coarse row). A row that crosses interpolates between (ya + 1, ya + 2) instead of (ya, ya + 1): the MIDDLE coarse row belongs
//           to every row, so only the OTHER row's two values are selected per row and class (2 v_cndmask instead of 4), and the row's weights are
//           swapped once in front of the loop: v = (bo0 * xo0 + bo1 * xo1) + (bm0 * xm0 + bm1 * xm1), which for a row that crosses is the stated sum
//           with its two halves exchanged: an fp32 add commutes, so the bits are the stated ones. Row 0 never crosses (ya is its own i0)
//   v       four products and three sums per pixel and class, each rounded on its own (contraction off), then the strict compare in ascending
//           class order: no cross-lane reduction. PROB adds the lazy-reference softmax sum of mbn_f32_resample.hip over the same v
// The index / weight rule (plain and window), the stage pass, the softmax sum and the store are restated from mbn_f32_resample.hip: that file's
// kernels are pinned to their register counts, so nothing is shared through it. Scalar fp32 VALU only: the file is compiled with the packed fp32
// operations switched off (every product is pinned on its own; see the Makefile).
#include "mbn_internal.h"
#include "mbn_device.h"

namespace {

constexpr int GD_TILE = MBN_RESAMPLE_TILE;   // output tile side of a workgroup
constexpr int GD_ROWS = 4;                   // output rows of a lane
constexpr float GD_MARGIN = 16.0f;           // the lazy reference moves when a logit exceeds it by more than this

struct GuidedArgs {
    int *labels;
    float *score, *prob;     // either may be null (prob: PROB instantiations only)
    const float *logits;
    const uint8_t *guide_lo; // [batch][rows][cols][3]
    const uint8_t *guide_hi; // [batch][out_rows][out_cols][3]
    const float *lut;        // 766 range weights
    int rows, cols, classes; // the coarse map
    int out_rows, out_cols, tiles_x;
    int fy, fx, ch;          // the launch's LDS footprint in vectors and the class chunk (mbn_resample_window_plan)
    int in_rows, in_cols;    // WIN: the network-input pixels the coarse map covers, and the window
    int wx, wy, wiw, wih;
    float min_prob;
    int ignore_label;
};

struct GdWindow {
    int R, b, l;
};

// the normative index / weight rule of mbn_resample_argmax_f32 for output coordinate o of an axis with n coarse samples and N outputs
__device__ __forceinline__ void gd_axis(int o, int n, int N, int *i0, float *w1)
{
    const int num = max((2 * o + 1) * n - N, 0), den = 2 * N;
    *i0 = num / den;
    *w1 = (float)((double)(num % den) / (double)den);       // fp64 quotient, rounded once
}

// the same for a window [b, b + l) of the R input pixels (mbn_resample_argmax_window_f32): 64-bit integers, both fp64 operands exact
__device__ __forceinline__ void gd_axis_win(int o, int n, int N, const GdWindow &w, int *i0, float *w1)
{
    const int64_t num = max((int64_t)(2 * o + 1) * w.l * n + 2 * (int64_t)w.b * n * N - (int64_t)N * w.R, (int64_t)0), den = 2 * (int64_t)N * w.R;
    const int64_t q = num / den;
    *i0 = (int)q;
    *w1 = (float)((double)(num - q * den) / (double)den);   // fp64 quotient, rounded once
}

template <bool WIN>
__device__ __forceinline__ void gd_coord(int o, int n, int N, const GdWindow &w, int *i0, float *w1)
{
    if (WIN) gd_axis_win(o, n, N, w, i0, w1);
    else gd_axis(o, n, N, i0, w1);
}

// exp(d) for the softmax sum: d <= GD_MARGIN, -inf gives 0
__device__ __forceinline__ float gd_exp(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896341f); }

// three bytes of a guide as one dword, R | G << 8 | B << 16: what v_sad_u8 takes
__device__ __forceinline__ unsigned gd_rgb(const uint8_t *p) { return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16; }

// The four normalised weights of one pixel: spatial weights (wy0, wy1) x (wx0, wx1), range weights g[j][k]. Every product, the three sums and the
// four quotients round on their own; the quotient is the correctly rounded fp32 one (v_div_scale / v_div_fmas / v_div_fixup: what `/` compiles to
// here; a, A are normal or zero inside the envelope, A > 0)
__device__ __forceinline__ void gd_weights(float wy0, float wy1, float wx0, float wx1, const float (&g)[2][2], float (&b)[2][2])
{
#pragma clang fp contract(off)
    const float a00 = (wy0 * wx0) * g[0][0], a01 = (wy0 * wx1) * g[0][1], a10 = (wy1 * wx0) * g[1][0], a11 = (wy1 * wx1) * g[1][1];
    const float A = ((a00 + a01) + a10) + a11;
    b[0][0] = a00 / A; b[0][1] = a01 / A; b[1][0] = a10 / A; b[1][1] = a11 / A;
}

// The stage pass of one class chunk (mbn_f32_resample.hip's): the nv = fy x fx vectors from (ybase, xbase) on, clamped to the map, go to s_x, ld
// floats apart. VEC: 16-byte loads; else dword loads, the classes past cn staged as NaN, which never wins
template <bool VEC>
__device__ __forceinline__ void gd_stage(float *s_x, const float *__restrict__ src, int ybase, int xbase, int fx, int nv, int ld, int cols, int classes,
                                         int last_y, int last_x, int c0, int cn, int cn4, int tid)
{
    if (VEC) {
        const int q = cn4 >> 2;                  // classes % 4 == 0: cn4 == cn
        for (int e = tid; e < nv * q; e += 256) {
            const int v = e / q, c = (e - v * q) << 2;
            const int ry = min(ybase + v / fx, last_y), rx = min(xbase + v % fx, last_x);
            *reinterpret_cast<f4 *>(s_x + v * ld + c) = *reinterpret_cast<const f4 *>(src + (unsigned)((ry * cols + rx) * classes + c0 + c));
        }
    } else {
        const float nan = __builtin_nanf("");
        for (int e = tid; e < nv * cn4; e += 256) {
            const int v = e / cn4, c = e - v * cn4;
            const int ry = min(ybase + v / fx, last_y), rx = min(xbase + v % fx, last_x);
            s_x[v * ld + c] = c < cn ? src[(unsigned)((ry * cols + rx) * classes + c0 + c)] : nan;
        }
    }
}

// The reduce pass of one staged chunk for a lane's four rows. xm: the middle coarse row's two vectors, xo: the other row's, the row above for a row
// that does not cross (x0) and the row below for one that does (x2, CROSS only). bo / bm: the row's weights for (xo, xm), swapped by the caller.
template <bool CROSS, bool PROB>
__device__ __forceinline__ void gd_reduce(const float *(&p)[3][2], int cn4, int c0, const float (&bo)[GD_ROWS][2], const float (&bm)[GD_ROWS][2],
                                          const bool (&up)[GD_ROWS], float (&best)[GD_ROWS], int (&label)[GD_ROWS], float (&ref)[GD_ROWS],
                                          float (&sum)[GD_ROWS])
{
#pragma clang fp contract(off)
    for (int c = 0; c < cn4; c += 4) {
        f4 x0[2], xm[2], x2[2];
        float vv[GD_ROWS][4];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            x0[k] = *reinterpret_cast<const f4 *>(p[0][k] + c);
            xm[k] = *reinterpret_cast<const f4 *>(p[1][k] + c);
            if (CROSS) x2[k] = *reinterpret_cast<const f4 *>(p[2][k] + c);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int r = 0; r < GD_ROWS; r++) {
                const bool u = CROSS && r > 0 && up[r];
                const float xo0 = u ? x2[0][k] : x0[0][k], xo1 = u ? x2[1][k] : x0[1][k];
                const float po0 = bo[r][0] * xo0, po1 = bo[r][1] * xo1, pm0 = bm[r][0] * xm[0][k], pm1 = bm[r][1] * xm[1][k];
                const float so = po0 + po1, sm = pm0 + pm1;
                const float v = so + sm;
                if (v > best[r]) { best[r] = v; label[r] = c0 + c + k; }
                vv[r][k] = v;
            }
        }
        if (PROB) {
#pragma unroll
            for (int r = 0; r < GD_ROWS; r++) {
                // the reference moves at most once per four classes, to their maximum m (the maxima drop NaNs; an all-NaN m fails the compare, and
                // so does -inf - -inf): everything seen so far is then at most GD_MARGIN above ref, the four included
                const float m = __builtin_fmaxf(__builtin_fmaxf(vv[r][0], vv[r][1]), __builtin_fmaxf(vv[r][2], vv[r][3]));
                if (m - ref[r] > GD_MARGIN) { sum[r] *= gd_exp(ref[r] - m); ref[r] = m; }
#pragma unroll
                for (int k = 0; k < 4; k++) sum[r] += gd_exp(__builtin_fmaxf(vv[r][k] - ref[r], -200.0f));     // a NaN difference adds exp(-200) = 0
            }
        }
    }
}

template <bool VEC, bool WIN, bool PROB>
__global__ __launch_bounds__(256) void resample_guided_f32(const GuidedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_gd[];
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const size_t img = (size_t)blockIdx.y;                                                      // 64-bit bases, 32-bit offsets inside an image
    const size_t map = (size_t)a.out_rows * a.out_cols;
    const int H = a.out_rows, W = a.out_cols;
    const int ld = a.ch + 4, nv = a.fy * a.fx;
    const int last_y = a.rows - 1, last_x = a.cols - 1;
    const float *__restrict__ src = a.logits + img * ((size_t)a.rows * a.cols * a.classes);
    uint8_t *s_lo = reinterpret_cast<uint8_t *>(s_gd + nv * ld);                                // the footprint's guide_lo colours, 3 bytes a vector
    const GdWindow wy = { a.in_rows, a.wy, a.wih }, wx = { a.in_cols, a.wx, a.wiw };            // read by the WIN instantiations only

    int ybase, xbase;
    float unused;
    gd_coord<WIN>(GD_TILE * ty, a.rows, H, wy, &ybase, &unused);
    gd_coord<WIN>(GD_TILE * tx, a.cols, W, wx, &xbase, &unused);

    // ---- the footprint's low-resolution colours, once per tile
    {
        const uint8_t *__restrict__ lo = a.guide_lo + img * ((size_t)a.rows * a.cols * 3);
        for (int e = tid; e < nv * 3; e += 256) {
            const int v = e / 3, k = e - v * 3;
            const int ry = min(ybase + v / a.fx, last_y), rx = min(xbase + v % a.fx, last_x);
            s_lo[e] = lo[(size_t)(ry * a.cols + rx) * 3 + k];
        }
    }
    __syncthreads();

    // ---- this lane's pixels: column ox, rows oy0 .. oy0 + 3 (a coordinate past the image is evaluated at the last one and not stored)
    const int ox = GD_TILE * tx + (tid & 31), oy0 = GD_TILE * ty + GD_ROWS * (tid >> 5);
    const bool active = ox < W && oy0 < H;
    const int oxc = min(ox, W - 1);
    int x0, ya = 0;
    float wx1, wy1[GD_ROWS];
    bool up[GD_ROWS];                         // row r interpolates between (ya + 1, ya + 2) instead of (ya, ya + 1)
    gd_coord<WIN>(oxc, a.cols, W, wx, &x0, &wx1);
    const float wx0 = 1.0f - wx1;
#pragma unroll
    for (int r = 0; r < GD_ROWS; r++) {
        int r0;
        gd_coord<WIN>(min(oy0 + r, H - 1), a.rows, H, wy, &r0, &wy1[r]);
        if (r == 0) ya = r0;
        up[r] = r0 != ya;                     // r0 is ya or ya + 1: four rows span less than one coarse row
    }
    const bool cross = __ballot(up[1] || up[2] || up[3]) != 0;
    // LDS slots of the six vectors: rows ya, min(ya + 1, rows - 1), min(ya + 2, rows - 1) x columns x0, min(x0 + 1, cols - 1). Inside the staged
    // block by construction; the clamps keep every read inside the launch's LDS whatever the arguments.
    int slot[3][2];
    const float *p[3][2];
    unsigned lo[3][2];                        // their colours
    {
        const int sx0 = min(max(x0 - xbase, 0), a.fx - 1), sx1 = min(max(min(x0 + 1, last_x) - xbase, 0), a.fx - 1);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int sy = min(max(min(ya + j, last_y) - ybase, 0), a.fy - 1);
            slot[j][0] = sy * a.fx + sx0;
            slot[j][1] = sy * a.fx + sx1;
#pragma unroll
            for (int k = 0; k < 2; k++) {
                p[j][k] = s_gd + slot[j][k] * ld;
                lo[j][k] = gd_rgb(s_lo + slot[j][k] * 3);
            }
        }
    }
    // ---- the sixteen weights, already ordered for the loop: bo for the other coarse row (above, or below for a row that crosses), bm for the middle
    float bo[GD_ROWS][2], bm[GD_ROWS][2];
    {
        const uint8_t *__restrict__ hi = a.guide_hi + img * (map * 3);
#pragma unroll
        for (int r = 0; r < GD_ROWS; r++) {
            const unsigned px = gd_rgb(hi + ((size_t)min(oy0 + r, H - 1) * W + oxc) * 3);
            float g[2][2], b[2][2];
#pragma unroll
            for (int j = 0; j < 2; j++) {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const unsigned c = up[r] ? lo[j + 1][k] : lo[j][k];
                    g[j][k] = a.lut[min(__builtin_amdgcn_sad_u8(px, c, 0u), 765u)];            // |dR| + |dG| + |dB| <= 765: the min costs nothing
                }
            }
            gd_weights(1.0f - wy1[r], wy1[r], wx0, wx1, g, b);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                bo[r][k] = up[r] ? b[1][k] : b[0][k];
                bm[r][k] = up[r] ? b[0][k] : b[1][k];
            }
        }
    }

    float best[GD_ROWS], ref[GD_ROWS], sum[GD_ROWS];      // ref, sum: the PROB instantiations' lazy reference and softmax sum
    int label[GD_ROWS];
#pragma unroll
    for (int r = 0; r < GD_ROWS; r++) { best[r] = ref[r] = -__builtin_inff(); sum[r] = 0.0f; label[r] = 0; }

    for (int c0 = 0; c0 < a.classes; c0 += a.ch) {
        const int cn = min(a.ch, a.classes - c0), cn4 = (cn + 3) & ~3;
        gd_stage<VEC>(s_gd, src, ybase, xbase, a.fx, nv, ld, a.cols, a.classes, last_y, last_x, c0, cn, cn4, tid);
        __syncthreads();
        if (active) {
            if (cross) gd_reduce<true, PROB>(p, cn4, c0, bo, bm, up, best, label, ref, sum);
            else gd_reduce<false, PROB>(p, cn4, c0, bo, bm, up, best, label, ref, sum);
        }
        __syncthreads();
    }
    if (!active) return;

    // ---- the store (mbn_f32_resample.hip's): the label, the score (may be null) and, PROB, the probability with the threshold on the value stored
    int *__restrict__ labels = a.labels + img * map;
    float *__restrict__ score = a.score ? a.score + img * map : nullptr;
    float *__restrict__ prob = PROB && a.prob ? a.prob + img * map : nullptr;
    const unsigned out = (unsigned)(oy0 * W + ox);        // 32-bit inside an image: its map is below 2^31 bytes
#pragma unroll
    for (int r = 0; r < GD_ROWS; r++) {
        if (oy0 + r >= H) break;
        if (PROB) {
            // a finite best has a finite ref <= best <= ref + GD_MARGIN and a sum >= 1 that holds best's own term: 0 < pr <= 1
            const float pr = __builtin_fabsf(best[r]) < __builtin_inff() ? gd_exp(best[r] - ref[r]) / sum[r] : 0.0f;
            if (pr < a.min_prob) label[r] = a.ignore_label;                                     // strict, on the value stored below
            if (prob) prob[out + (unsigned)(r * W)] = pr;
        }
        labels[out + (unsigned)(r * W)] = label[r];
        if (score) score[out + (unsigned)(r * W)] = best[r];
    }
}

// the eight kernels by [prob][win][vec]; vec: `logits` on 16 bytes and classes % 4 == 0, so that every class vector starts on 16 bytes
typedef void (*GdKernel)(const GuidedArgs);
const GdKernel gd_kernels[2][2][2] = {
    { { resample_guided_f32<false, false, false>, resample_guided_f32<true, false, false> },
      { resample_guided_f32<false, true, false>, resample_guided_f32<true, true, false> } },
    { { resample_guided_f32<false, false, true>, resample_guided_f32<true, false, true> },
      { resample_guided_f32<false, true, true>, resample_guided_f32<true, true, true> } },
};

// ---- mbn_guide_reduce_u8: guide_lo = the rounded mean of every S x S block of the canvas, per channel. One wave per coarse cell: lane l takes the
// block's pixels l, l + 64, ... (row-major inside the block, so a wave reads runs of consecutive bytes), three sums in registers, a butterfly over
// the wave, and lane 0 stores the three bytes (sum + S^2 / 2) / S^2. A sum is at most 255 S^2 < 2^32 for S <= 2048 (the envelope).
struct ReduceArgs {
    uint8_t *lo;
    const uint8_t *canvas;
    int rows, cols, S;       // the coarse map and the block side; the canvas is rows * S x cols * S
    int cells;               // rows * cols
};

__global__ __launch_bounds__(256) void guide_reduce_u8(const ReduceArgs a)
{
    const int cell = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
    if (cell >= a.cells) return;              // whole waves leave: the butterfly below runs on full ones
    const int cy = cell / a.cols, cx = cell - cy * a.cols;
    const size_t row_bytes = (size_t)a.cols * a.S * 3;
    const uint8_t *__restrict__ blk = a.canvas + (size_t)blockIdx.y * ((size_t)a.rows * a.S * row_bytes) + (size_t)cy * a.S * row_bytes + (size_t)cx * a.S * 3;
    unsigned s[3] = { 0u, 0u, 0u };
    for (int e = lane; e < a.S * a.S; e += 64) {
        const int y = e / a.S, x = e - y * a.S;
        const uint8_t *px = blk + (size_t)y * row_bytes + (size_t)x * 3;
        s[0] += px[0]; s[1] += px[1]; s[2] += px[2];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s[k] += (unsigned)__shfl_xor((int)s[k], d, 64);
    }
    if (lane == 0) {
        const unsigned n = (unsigned)(a.S * a.S);
        uint8_t *o = a.lo + ((size_t)blockIdx.y * a.cells + cell) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) o[k] = (uint8_t)((s[k] + n / 2) / n);
    }
}

}   // namespace

// rect = (x, y, iw, ih) of the in_rows x in_cols network input: the window kernels; null: the whole map, the plain rule (in_rows, in_cols are not
// read). The shape is inside mbn_resample_window_envelope (without a rect: mbn_resample_argmax_envelope) and the pointers are checked (the caller).
// q = null: the argmax kernels. The plan is the bilinear read-out's; the launch's LDS adds the footprint's colours behind it.
int mbn_launch_f32_resample_guided(mbn_context *, hipStream_t s, int32_t *labels, float *score, const float *logits, const uint8_t *guide_lo,
                                   const uint8_t *guide_hi, const float *lut, int batch, int rows, int cols, int classes, int in_rows, int in_cols,
                                   const int32_t *rect, int out_rows, int out_cols, const mbn_readout_prob *q)
{
    mbn_resample_launch_t l = { 0, 0, 0, 0, 0, 0 };
    if (rect) mbn_resample_window_plan(rows, cols, in_rows, in_cols, rect, out_rows, out_cols, &l);
    else mbn_resample_plan(rows, cols, out_rows, out_cols, &l);
    GuidedArgs a = {};
    a.labels = labels; a.score = score; a.logits = logits;
    a.guide_lo = guide_lo; a.guide_hi = guide_hi; a.lut = lut;
    a.rows = rows; a.cols = cols; a.classes = classes;
    a.out_rows = out_rows; a.out_cols = out_cols;
    a.tiles_x = (out_cols + GD_TILE - 1) / GD_TILE;
    a.fy = l.fy; a.fx = l.fx; a.ch = l.ch;
    a.in_rows = in_rows; a.in_cols = in_cols;
    if (rect) { a.wx = rect[0]; a.wy = rect[1]; a.wiw = rect[2]; a.wih = rect[3]; }
    if (q) { a.prob = q->prob; a.min_prob = q->min_prob; a.ignore_label = q->ignore_label; }
    const bool vec = ((uintptr_t)logits % 16) == 0 && (classes % 4) == 0;
    const size_t lds = (size_t)l.lds_bytes + (size_t)((l.fy * l.fx * 3 + 3) & ~3);
    hipLaunchKernelGGL(gd_kernels[q != nullptr][rect != nullptr][vec], dim3((unsigned)l.tiles, (unsigned)batch), dim3(256), lds, s, a);
    return MBN_OK;
}

// the arguments are inside mbn_guide_reduce_envelope and the pointers non-null (the caller has checked both)
int mbn_launch_u8_guide_reduce(mbn_context *, hipStream_t s, uint8_t *guide_lo, const uint8_t *canvas, int batch, int in_rows, int in_cols, int S)
{
    ReduceArgs a = {};
    a.lo = guide_lo; a.canvas = canvas;
    a.rows = in_rows / S; a.cols = in_cols / S; a.S = S;
    a.cells = a.rows * a.cols;
    hipLaunchKernelGGL(guide_reduce_u8, dim3((unsigned)((a.cells + 3) / 4), (unsigned)batch), dim3(256), 0, s, a);
    return MBN_OK;
}
