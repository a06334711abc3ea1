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
//           class order: no cross-lane reduction. PROB adds the lazy-reference softmax sum (rs_softmax_group) over the same v
// The tile, the index / weight rule (plain and window), the lane state, the stage pass, the softmax sum and the store are mbn_readout_tile.h's.
// Scalar fp32 VALU only: the file is compiled with the packed fp32 operations switched off (every product is pinned on its own; see the Makefile).
#include "mbn_internal.h"
#include "mbn_device.h"
#include "mbn_readout_tile.h"

namespace {

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

// The reduce pass of one staged chunk for a lane's four rows. xm: the middle coarse row's two vectors, xo: the other row's, the row above for a row
// that does not cross (x0) and the row below for one that does (x2, CROSS only). bo / bm: the row's weights for (xo, xm), swapped by the caller.
template <bool CROSS, bool PROB>
__device__ __forceinline__ void gd_reduce(const float *s_x, const int (&off)[3][2], int cn4, int c0, const float (&bo)[RS_ROWS][2], const float (&bm)[RS_ROWS][2],
                                          const bool (&up)[RS_ROWS], float (&best)[RS_ROWS], int (&label)[RS_ROWS], float (&ref)[RS_ROWS],
                                          float (&sum)[RS_ROWS])
{
#pragma clang fp contract(off)
    for (int c = 0; c < cn4; c += 4) {
        f4 x0[2], xm[2], x2[2];
        float vv[RS_ROWS][4];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            x0[k] = *reinterpret_cast<const f4 *>(s_x + off[0][k] + c);
            xm[k] = *reinterpret_cast<const f4 *>(s_x + off[1][k] + c);
            if (CROSS) x2[k] = *reinterpret_cast<const f4 *>(s_x + off[2][k] + c);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                const bool u = CROSS && r > 0 && up[r];
                const float xo0 = u ? x2[0][k] : x0[0][k], xo1 = u ? x2[1][k] : x0[1][k];
                const float po0 = bo[r][0] * xo0, po1 = bo[r][1] * xo1, pm0 = bm[r][0] * xm[0][k], pm1 = bm[r][1] * xm[1][k];
                const float so = po0 + po1, sm = pm0 + pm1;
                const float v = so + sm;
                if (v > best[r]) { best[r] = v; label[r] = c0 + c + k; }
                vv[r][k] = v;
            }
        }
        if (PROB) rs_softmax_group(vv, ref, sum);
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
    const RsWindow wy = { a.in_rows, a.wy, a.wih }, wx = { a.in_cols, a.wx, a.wiw };            // read by the WIN instantiations only
    RsLane n;
    rs_lane<WIN>(n, a.rows, a.cols, a.fy, a.fx, ld, H, W, ty, tx, wy, wx);
    const int ox = n.ox, oy0 = n.oy0, oxc = min(ox, W - 1);
    const bool active = n.active;

    // ---- the footprint's low-resolution colours, once per tile
    {
        const uint8_t *__restrict__ lo = a.guide_lo + img * ((size_t)a.rows * a.cols * 3);
        for (int e = tid; e < nv * 3; e += 256) {
            const int v = e / 3, k = e - v * 3;
            const int ry = min(n.ybase + v / a.fx, last_y), rx = min(n.xbase + v % a.fx, last_x);
            s_lo[e] = lo[(size_t)(ry * a.cols + rx) * 3 + k];
        }
    }
    __syncthreads();

    // ---- the colours of the lane's six vectors, by their slots
    unsigned lo[3][2];
#pragma unroll
    for (int j = 0; j < 3; j++) {
#pragma unroll
        for (int k = 0; k < 2; k++) lo[j][k] = gd_rgb(s_lo + n.slot[j][k] * 3);
    }
    // ---- the sixteen weights, already ordered for the loop: bo for the other coarse row (above, or below for a row that crosses), bm for the middle
    float bo[RS_ROWS][2], bm[RS_ROWS][2];
    {
        const uint8_t *__restrict__ hi = a.guide_hi + img * (map * 3);
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) {
            const unsigned px = gd_rgb(hi + ((size_t)min(oy0 + r, H - 1) * W + oxc) * 3);
            float g[2][2], b[2][2];
#pragma unroll
            for (int j = 0; j < 2; j++) {
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const unsigned c = n.up[r] ? lo[j + 1][k] : lo[j][k];
                    g[j][k] = a.lut[min(__builtin_amdgcn_sad_u8(px, c, 0u), 765u)];            // |dR| + |dG| + |dB| <= 765: the min costs nothing
                }
            }
            gd_weights(n.wy0[r], n.wy1[r], n.wx0, n.wx1, g, b);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                bo[r][k] = n.up[r] ? b[1][k] : b[0][k];
                bm[r][k] = n.up[r] ? b[0][k] : b[1][k];
            }
        }
    }

    float best[RS_ROWS], ref[RS_ROWS], sum[RS_ROWS];      // ref, sum: the PROB instantiations' lazy reference and softmax sum
    int label[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) { best[r] = ref[r] = -__builtin_inff(); sum[r] = 0.0f; label[r] = 0; }

    for (int c0 = 0; c0 < a.classes; c0 += a.ch) {
        const int cn = min(a.ch, a.classes - c0), cn4 = (cn + 3) & ~3;
        rs_stage<VEC>(s_gd, src, n.ybase, n.xbase, a.fx, nv, ld, a.cols, a.classes, last_y, last_x, c0, cn, cn4, tid);
        __syncthreads();
        if (active) {
            if (n.cross) gd_reduce<true, PROB>(s_gd, n.off, cn4, c0, bo, bm, n.up, best, label, ref, sum);
            else gd_reduce<false, PROB>(s_gd, n.off, cn4, c0, bo, bm, n.up, best, label, ref, sum);
        }
        __syncthreads();
    }
    if (!active) return;
    rs_store<PROB>(a.labels + img * map, a.score ? a.score + img * map : nullptr, PROB && a.prob ? a.prob + img * map : nullptr, H, W, oy0, ox, best,
                   label, ref, sum, a.min_prob, a.ignore_label);
}

// the eight kernels by [prob][win][vec]
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
    rs_fill(a, labels, score, logits, rows, cols, classes, l, q);
    rs_fill_uniform(a, out_rows, out_cols, in_rows, in_cols, rect);
    a.guide_lo = guide_lo; a.guide_hi = guide_hi; a.lut = lut;
    const size_t lds = (size_t)l.lds_bytes + (size_t)((l.fy * l.fx * 3 + 3) & ~3);
    hipLaunchKernelGGL(gd_kernels[q != nullptr][rect != nullptr][rs_vec(logits, classes)], dim3((unsigned)l.tiles, (unsigned)batch), dim3(256), lds, s, a);
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
