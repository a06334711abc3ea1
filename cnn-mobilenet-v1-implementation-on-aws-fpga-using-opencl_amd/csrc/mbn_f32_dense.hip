// mbn_f32_dense.hip — the dense head's read-out on gfx950: bilinear upsample of the per-pixel logits by the output stride and the argmax
// over the classes, in one kernel (mbn_upsample_argmax_f32; include/mbn.h, "dense head", is the normative statement of the arithmetic).
// The reference has no counterpart: its only read-out is the host softmax + argmax over 1000 pooled logits (MobileNet.c:2771-2792).
//
// The upsampled tensor [rows*S][cols*S][classes] is never formed in memory. With half-pixel centres the output rows
// [S*k - S/2, S*k + S/2) all lie between the coarse rows k-1 and k (clamped at the borders), so an S x S output patch on that shifted grid
// interpolates between exactly four class vectors. A workgroup of 256 lanes owns a 32 x 32 output tile on the shifted grid: P x P patches
// (P = 32 / S: 4, 2, 1) and therefore the (P+1) x (P+1) coarse class vectors around them. It walks the classes in chunks of DENSE_CH:
//   stage   the chunk of every one of those vectors goes from global memory to LDS once (16-byte loads when `logits` is on 16 bytes and
//           classes % 4 == 0, else dword loads; classes past the end read as NaN, which never wins);
//   reduce  a lane owns one output column and four consecutive rows of the tile (one patch: 4 | S). Per class it forms the two horizontal
//           interpolants t0 / t1 of its column once and reuses them down its four rows; each row keeps a running (best, label) in registers.
// Classes are visited in ascending order with a strict compare, which IS the definition (lowest index wins a tie, NaN never wins), so there
// is no cross-lane reduction. A coarse logit is read from global memory once per workgroup that touches it: at most four times in all (nine
// along the borders of S = 32 tiles), from L2 after the first.
// Borders need no special case: every lane evaluates the normative index / weight formula for its own pixel, and the staged vectors are the
// clamped rows / columns the formula names. The top and left tiles are part empty (the grid starts S/2 before the image).
// Every product and sum rounds on its own: contraction into FMA is switched off where they are formed (the build contracts by default).
#include "mbn_internal.h"
#include "mbn_device.h"

namespace {

constexpr int DENSE_TILE = 32;     // output tile side of a workgroup
constexpr int DENSE_ROWS = 4;      // output rows of a lane
constexpr int DENSE_CH = 128;      // classes per chunk
constexpr int DENSE_LD = DENSE_CH + 4;   // LDS row of a staged vector: 16-byte aligned rows, consecutive vectors 4 banks apart

struct DenseArgs {
    int *labels;
    float *score;            // may be null
    const float *logits;
    int rows, cols, classes; // the coarse map
    int tiles_x;
};

// a * wa + b * wb with three roundings
__device__ __forceinline__ float dense_lerp(float a, float wa, float b, float wb)
{
#pragma clang fp contract(off)
    const float p = a * wa, q = b * wb;
    return p + q;
}

// the normative index / weight rule for output coordinate o of an axis with n coarse samples: i0, i1 and the weight of i1
template <int S>
__device__ __forceinline__ void dense_axis(int o, int n, int *i0, int *i1, float *w1)
{
    const int num = max(2 * o + 1 - S, 0);
    *i0 = num / (2 * S);
    *i1 = min(*i0 + 1, n - 1);
    *w1 = (float)(num % (2 * S)) * (1.0f / (float)(2 * S));       // exact: a dyadic fraction
}

template <int S, bool VEC>
__global__ __launch_bounds__(256) void upsample_argmax_f32(const DenseArgs a)
{
    constexpr int P = DENSE_TILE / S, NV = (P + 1) * (P + 1);
    __shared__ __attribute__((aligned(16))) float s_x[NV * DENSE_LD];
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int H = a.rows * S, W = a.cols * S;
    const size_t img = (size_t)blockIdx.y;
    const float *__restrict__ src = a.logits + img * ((size_t)a.rows * a.cols * a.classes);   // 64-bit base, 32-bit offsets inside an image
    // first staged coarse row / column; vector (j, i) is row min(ybase + j, rows - 1), column min(xbase + i, cols - 1)
    const int ybase = max(P * ty - 1, 0), xbase = max(P * tx - 1, 0);

    // this lane's pixels: column ox, rows oy0 .. oy0 + 3 (all inside or all outside the image: S/2, H and the row groups are multiples of 4)
    const int ox = DENSE_TILE * tx - S / 2 + (tid & 31), oy0 = DENSE_TILE * ty - S / 2 + DENSE_ROWS * (tid >> 5);
    const bool active = ox >= 0 && ox < W && oy0 >= 0 && oy0 < H;
    int x0, x1, y0, y1;
    float wx1, wy1[DENSE_ROWS], wy0[DENSE_ROWS];
    dense_axis<S>(active ? ox : 0, a.cols, &x0, &x1, &wx1);
    const float wx0 = 1.0f - wx1;
#pragma unroll
    for (int r = 0; r < DENSE_ROWS; r++) {
        int r0, r1;
        dense_axis<S>(active ? oy0 + r : 0, a.rows, &r0, &r1, &wy1[r]);
        wy0[r] = 1.0f - wy1[r];
        if (r == 0) { y0 = r0; y1 = r1; }           // the four rows share a patch, hence y0 / y1
    }
    // LDS word offsets of the four vectors (the slots are inside the staged block by construction; the clamp costs nothing)
    const int sy0 = min(max(y0 - ybase, 0), P), sy1 = min(max(y1 - ybase, 0), P);
    const int sx0 = min(max(x0 - xbase, 0), P), sx1 = min(max(x1 - xbase, 0), P);
    const float *p00 = s_x + (sy0 * (P + 1) + sx0) * DENSE_LD, *p01 = s_x + (sy0 * (P + 1) + sx1) * DENSE_LD;
    const float *p10 = s_x + (sy1 * (P + 1) + sx0) * DENSE_LD, *p11 = s_x + (sy1 * (P + 1) + sx1) * DENSE_LD;

    float best[DENSE_ROWS];
    int label[DENSE_ROWS];
#pragma unroll
    for (int r = 0; r < DENSE_ROWS; r++) { best[r] = -__builtin_inff(); label[r] = 0; }
    const float nan = __builtin_nanf("");

    for (int c0 = 0; c0 < a.classes; c0 += DENSE_CH) {
        const int cn = min(DENSE_CH, a.classes - c0), cn4 = (cn + 3) & ~3;
        // ---- stage: NV vectors x cn4 classes
        if (VEC) {
            const int q = cn4 >> 2;                  // classes % 4 == 0: cn4 == cn
            for (int e = tid; e < NV * q; e += 256) {
                const int v = e / q, c = (e - v * q) << 2;
                const int ry = min(ybase + v / (P + 1), a.rows - 1), rx = min(xbase + v % (P + 1), a.cols - 1);
                *reinterpret_cast<f4 *>(s_x + v * DENSE_LD + c) =
                    *reinterpret_cast<const f4 *>(src + ((size_t)ry * a.cols + rx) * a.classes + c0 + c);
            }
        } else {
            for (int e = tid; e < NV * cn4; e += 256) {
                const int v = e / cn4, c = e - v * cn4;
                const int ry = min(ybase + v / (P + 1), a.rows - 1), rx = min(xbase + v % (P + 1), a.cols - 1);
                s_x[v * DENSE_LD + c] = c < cn ? src[((size_t)ry * a.cols + rx) * a.classes + c0 + c] : nan;
            }
        }
        __syncthreads();
        // ---- reduce
        if (active) {
            for (int c = 0; c < cn4; c += 4) {
                const f4 a00 = *reinterpret_cast<const f4 *>(p00 + c), a01 = *reinterpret_cast<const f4 *>(p01 + c);
                const f4 a10 = *reinterpret_cast<const f4 *>(p10 + c), a11 = *reinterpret_cast<const f4 *>(p11 + c);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const float t0 = dense_lerp(a00[k], wx0, a01[k], wx1);      // horizontal first
                    const float t1 = dense_lerp(a10[k], wx0, a11[k], wx1);
#pragma unroll
                    for (int r = 0; r < DENSE_ROWS; r++) {
                        const float v = dense_lerp(t0, wy0[r], t1, wy1[r]);     // then vertical
                        if (v > best[r]) { best[r] = v; label[r] = c0 + c + k; }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    const size_t out = img * ((size_t)H * W) + (size_t)oy0 * W + ox;
#pragma unroll
    for (int r = 0; r < DENSE_ROWS; r++) {
        a.labels[out + (size_t)r * W] = label[r];
        if (a.score) a.score[out + (size_t)r * W] = best[r];
    }
}

template <int S>
void launch(hipStream_t s, const DenseArgs &a, dim3 grid, bool vec)
{
    if (vec) hipLaunchKernelGGL((upsample_argmax_f32<S, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((upsample_argmax_f32<S, false>), grid, dim3(256), 0, s, a);
}

}   // namespace

// The shape is inside mbn_upsample_argmax_envelope and the pointers are non-null multiples of 4 (the caller has checked both).
int mbn_launch_f32_upsample_argmax(mbn_context *, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows,
                                   int cols, int classes, int factor)
{
    DenseArgs a;
    a.labels = labels; a.score = score; a.logits = logits;
    a.rows = rows; a.cols = cols; a.classes = classes;
    a.tiles_x = MBN_DENSE_TILES(cols, factor);
    const dim3 grid((unsigned)(a.tiles_x * MBN_DENSE_TILES(rows, factor)), (unsigned)batch);
    const bool vec = ((uintptr_t)logits % 16) == 0 && (classes % 4) == 0;      // every class vector then starts on 16 bytes
    switch (factor) {
    case 8: launch<8>(s, a, grid, vec); break;
    case 16: launch<16>(s, a, grid, vec); break;
    case 32: launch<32>(s, a, grid, vec); break;
    default: return MBN_EUNSUPPORTED;
    }
    return MBN_OK;
}
