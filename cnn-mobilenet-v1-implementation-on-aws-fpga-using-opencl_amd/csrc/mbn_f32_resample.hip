// mbn_f32_resample.hip — the dense head's read-out at ANY output size on gfx950: bilinear resample of the per-pixel logits from rows x cols to
// out_rows x out_cols and the argmax over the classes, in one kernel (mbn_resample_argmax_f32 and its ragged form; include/mbn.h, "dense head at
// the source resolution", is the normative statement of the arithmetic). mbn_f32_dense.hip is the integer-factor sibling and stays mbn_net_segment's:
// its structure rests on the factor (a lane's four rows share one patch, a tile owns (P+1)^2 vectors on a grid shifted by S/2); neither holds here.
//
// The resampled tensor [out_rows][out_cols][classes] is never formed in memory. A workgroup of 256 lanes owns a 32 x 32 output tile (unshifted: tile
// (ty, tx) starts at output (32 ty, 32 tx)). The envelope's ratio (out >= 4 x coarse on both axes) bounds what a tile touches: along an axis the
// source span of 32 outputs is 31 n / N < 8, so i0 takes at most floor(31 n / N) + 2 values and i1 one more: MBN_RESAMPLE_FOOT(n, N) <= 10 coarse
// rows / columns, fy x fx class vectors. The launch's dynamic LDS holds exactly that footprint (6 x 6 at ratio 8, 10 x 10 only at ratio 4).
//   stage   per class chunk the fy x fx vectors go from global memory to LDS once (16-byte loads when `logits` is on 16 bytes and classes % 4 == 0,
//           else dword loads; classes past the end are staged as NaN, which never wins). Vector (j, i) is coarse row min(ybase + j, rows - 1),
//           column min(xbase + i, cols - 1), ybase / xbase = i0 of the tile's first output row / column;
//   reduce  a lane owns one output column and four consecutive output rows. Four rows span 3 n / N < 1 of the source, so their i0 is ya or ya + 1
//           and they touch at most the three coarse rows ya, ya + 1, ya + 2 (clamped). Per class the lane forms the three horizontal interpolants
//           t0, t1, t2 of its column once; row r takes (t0, t1) or (t1, t2) by a per-row select and keeps a running (best, label) in registers.
//           A wave neither of whose two row groups crosses a coarse row (a group crosses with probability about 3 n / N; none does at an integer
//           factor, where i0 steps at multiples of 4) takes the loop without t2 and without the selects: the same products and sums.
// Classes are visited in ascending order with a strict compare, which IS the definition, so there is no cross-lane reduction. Borders are no special
// case: every lane evaluates the normative index / weight rule for its own pixel, the weight's quotient in fp64 rounded once to fp32.
// Every product and sum rounds on its own: contraction into FMA is switched off where they are formed (the build contracts by default).
// The class chunk is the launch's (MBN_RESAMPLE_CH): 128 while the footprint still leaves eight workgroups on a CU's 160 KB, else 64.
// The uniform and the ragged form share the tile body; they differ in where a workgroup finds its image's (out_rows, out_cols, destination).
// WIN (mbn_resample_argmax_window_f32, mbn_ragged_readout_set_window): the outputs resample a rectangle of the network's input, the letterbox's
// inner image, instead of the whole map. Only the index / weight rule differs (rs_axis_win: 64-bit integers, still one fp64 division per axis
// coordinate, once per lane in front of the class loop); the footprint bound holds with n / N replaced by l n / (N R) (host/mbn_envelope.h), so
// stage, reduce, the cross ballot, the store and the LDS layout are the same code. The other instantiations compile to what they were without it.
// On the host the whole map is the window that covers the whole input (host/mbn_envelope.c: one envelope, one plan), and here one launch entry
// takes an optional rectangle. The device keeps both rules: the window rule's 64-bit divisions cost 0.6-0.7 % at equal footprint (profiles/LOG.md,
// "Through the letterbox"), so WIN stays a compile-time parameter and a null rectangle launches the plain kernels.
// PROB (mbn_resample_softmax_f32, _window_f32, _ragged_f32; include/mbn.h, "segment with confidence"): the same tile body also keeps the softmax
// denominator of each of the lane's four pixels and writes prob = 1 / sum_c exp(v_c - best) beside the label; labels and scores are the argmax
// instantiations' bit for bit (the same v, the same compare). The sum is ONE pass with a LAZY reference: per row a reference `ref` and
// sum = sum_c exp(v_c - ref). Per four classes the row's maximum m of the four is compared with ref: more than RS_MARGIN = 16 above it, m becomes
// the reference and the old sum is rescaled by exp(ref - m) < e^-16; then the four add exp(v - ref). So every v seen is at most 16 above ref,
// best - ref stays in [0, 16], ref is itself a v seen (its term is exp(0) = 1: sum >= 1), and a part of the sum that went through k rescales
// weighs below classes * e^(-16 (k - 1)) of it: only the first rescale of a part counts, and an ascending ramp costs one rescale per 16 units of
// logit instead of one per class. That is what keeps the error bound of include/mbn.h for every input. The alternative, a second pass with the
// final best, stages every chunk and forms every interpolant twice: about 10 plain VALU per pixel and class on top of the same exp, against
// about 7 issue slots here (subtract, max, multiply, add, v_exp_f32 at two slots, and a quarter of the group's three maxima, subtract and
// compare). prob = exp(best - ref) / sum at the end, 0 when best is not finite. A NaN v (the padding classes of the dword path among them) is
// dropped by the maxima, and its difference is replaced by -200 by a max that drops the NaN: it adds exp(-200) = 0, exactly.
// ENSEMBLE (mbn_resample_ensemble_f32; include/mbn.h, "segment with test-time augmentation"): K views read out as one map, kernels of their own on
// the same tile, stage pass, lerps, softmax sum and store; described where they stand, behind rs_launch.
// SLIDE (mbn_resample_slide_f32; include/mbn.h, "segment by sliding window"): a grid of overlapping tiles read out as one map, the ensemble's sibling
// on pieces of constant coverage; described where it stands, behind the ensemble.
// TOPK (mbn_resample_topk_f32, _ragged_f32; include/mbn.h, "segment with runners-up"): the k best classes of every pixel, rank-major, kernels of
// their own on the same tile; described where they stand, behind the slide.
#include "mbn_internal.h"
#include "mbn_device.h"
#include "mbn_label_set.h"

#include <new>
#include <type_traits>

namespace {

constexpr int RS_TILE = MBN_RESAMPLE_TILE;   // output tile side of a workgroup
constexpr int RS_ROWS = 4;                   // output rows of a lane

struct ResampleArgs {
    int *labels;
    float *score;            // may be null
    const float *logits;
    int rows, cols, classes; // the coarse map
    int out_rows, out_cols;  // uniform form: every image's output
    int tiles_x;             // of the launch's grid.x (ragged: of the widest item)
    int fy, fx;              // the launch's LDS footprint in vectors; every tile's own is inside it
    int ch;                  // classes per chunk, a multiple of 4; an LDS row is ch + 4 floats
    const mbn_label_set_head *head;   // ragged form (mbn_label_set.h)
    const mbn_label_item *items;
    int generation;
    // WIN instantiations only (behind everything the others read, whose kernel arguments stay where they were)
    int in_rows, in_cols;    // R, C: the network-input pixels the coarse map covers
    int wx, wy, wiw, wih;    // uniform form: the window, ordered as mbn_fit_pad writes it
    const mbn_label_window_item *witems;   // ragged form
    // PROB instantiations only (likewise behind everything else)
    float *prob;             // may be null when min_prob > 0
    float min_prob;          // a pixel whose stored prob is below it gets ignore_label
    int ignore_label;
};

constexpr float RS_MARGIN = 16.0f;           // the lazy reference moves when a logit exceeds it by more than this

// a window of the network's input along one axis: [b, b + l) of the R pixels the n coarse samples cover
struct RsWindow {
    int R, b, l;
};

// a * wa + b * wb with three roundings
__device__ __forceinline__ float rs_lerp(float a, float wa, float b, float wb)
{
#pragma clang fp contract(off)
    const float p = a * wa, q = b * wb;
    return p + q;
}

// the normative index / weight rule for output coordinate o of an axis with n coarse samples and N outputs: i0 and the weight of i1
__device__ __forceinline__ void rs_axis(int o, int n, int N, int *i0, float *w1)
{
    const int num = max((2 * o + 1) * n - N, 0), den = 2 * N;
    *i0 = num / den;
    *w1 = (float)((double)(num % den) / (double)den);       // fp64 quotient, rounded once
}

// The same for a window (include/mbn.h, "segment through the letterbox"): output o of N sits at input coordinate b + (o + 1/2) l / N. 64-bit integers
// (num < 2^46, den <= 2^29 inside the envelope: both exact in fp64); evaluated once per lane and axis coordinate, outside the class loop.
__device__ __forceinline__ void rs_axis_win(int o, int n, int N, const RsWindow &w, int *i0, float *w1)
{
    const int64_t num = max((int64_t)(2 * o + 1) * w.l * n + 2 * (int64_t)w.b * n * N - (int64_t)N * w.R, (int64_t)0), den = 2 * (int64_t)N * w.R;
    const int64_t q = num / den;
    *i0 = (int)q;
    *w1 = (float)((double)(num - q * den) / (double)den);   // fp64 quotient, rounded once
}

template <bool WIN>
__device__ __forceinline__ void rs_coord(int o, int n, int N, const RsWindow &w, int *i0, float *w1)
{
    if (WIN) rs_axis_win(o, n, N, w, i0, w1);
    else rs_axis(o, n, N, i0, w1);
}

// exp(d) for the softmax sum: d <= RS_MARGIN, -inf gives 0. One multiply and v_exp_f32 (1 ulp; a result below 2^-126 may flush to 0, far below
// the bound against a sum of at least 1).
__device__ __forceinline__ float rs_exp(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896341f); }

// The lazy-reference softmax sum (the file's head) of a lane's four rows over one group of four classes, vv[r][k] = row r's v of the group's class k:
// the ensemble kernels' copy of what rs_reduce does in place. rs_reduce keeps its own text because the sixteen kernels built from it are pinned to
// the registers they had before the ensemble existed, and calling this from there moved the softmax ones from 102 to 98 VGPRs
__device__ __forceinline__ void rs_softmax_group(const float (&vv)[RS_ROWS][4], float (&ref)[RS_ROWS], float (&sum)[RS_ROWS])
{
#pragma clang fp contract(off)                      // the same operations in every instantiation: a pixel's prob does not depend on the kernel
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        // the reference moves at most once per four classes, to their maximum m (the maxima drop NaNs; an all-NaN m fails the compare, and
        // so does -inf - -inf): everything seen so far is then at most RS_MARGIN above ref, the four included
        const float m = __builtin_fmaxf(__builtin_fmaxf(vv[r][0], vv[r][1]), __builtin_fmaxf(vv[r][2], vv[r][3]));
        if (m - ref[r] > RS_MARGIN) { sum[r] *= rs_exp(ref[r] - m); ref[r] = m; }
#pragma unroll
        for (int k = 0; k < 4; k++) sum[r] += rs_exp(__builtin_fmaxf(vv[r][k] - ref[r], -200.0f));     // a NaN difference adds exp(-200) = 0
    }
}

// The reduce pass of one staged chunk of cn4 classes for a lane's four rows. CROSS: some row of the wave interpolates between (ya + 1, ya + 2), so
// the third interpolant and the per-row selects are needed; otherwise every row of the wave uses (t0, t1) and neither is formed. The same products
// and sums in the same order either way. PROB: each row's lazy reference and softmax sum follow v (the file's head); untouched otherwise.
template <bool CROSS, bool PROB>
__device__ __forceinline__ void rs_reduce(const float *(&p)[3][2], int cn4, int c0, float wx0, float wx1, const float (&wy0)[RS_ROWS],
                                          const float (&wy1)[RS_ROWS], const bool (&up)[RS_ROWS], float (&best)[RS_ROWS], int (&label)[RS_ROWS],
                                          float (&ref)[RS_ROWS], float (&sum)[RS_ROWS])
{
    constexpr int NT = CROSS ? 3 : 2;
    for (int c = 0; c < cn4; c += 4) {
        f4 v0[NT], v1[NT];
        float vv[RS_ROWS][4];                                                               // PROB: the four classes' v of each row
#pragma unroll
        for (int j = 0; j < NT; j++) {
            v0[j] = *reinterpret_cast<const f4 *>(p[j][0] + c);
            v1[j] = *reinterpret_cast<const f4 *>(p[j][1] + c);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float t[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) t[j] = rs_lerp(v0[j][k], wx0, v1[j][k], wx1);      // horizontal first
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                const float ta = CROSS && up[r] ? t[1] : t[0], tb = CROSS && up[r] ? t[NT - 1] : t[1];
                const float v = rs_lerp(ta, wy0[r], tb, wy1[r]);                            // then vertical
                if (v > best[r]) { best[r] = v; label[r] = c0 + c + k; }
                if (PROB) vv[r][k] = v;
            }
        }
        if (PROB) {
#pragma clang fp contract(off)                      // the same operations in every instantiation: a pixel's prob does not depend on the kernel
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                // the reference moves at most once per four classes, to their maximum m (the maxima drop NaNs; an all-NaN m fails the compare, and
                // so does -inf - -inf): everything seen so far is then at most RS_MARGIN above ref, the four included
                const float m = __builtin_fmaxf(__builtin_fmaxf(vv[r][0], vv[r][1]), __builtin_fmaxf(vv[r][2], vv[r][3]));
                if (m - ref[r] > RS_MARGIN) { sum[r] *= rs_exp(ref[r] - m); ref[r] = m; }
#pragma unroll
                for (int k = 0; k < 4; k++) sum[r] += rs_exp(__builtin_fmaxf(vv[r][k] - ref[r], -200.0f));     // a NaN difference adds exp(-200) = 0
            }
        }
    }
}

// The stage pass of one class chunk (classes c0 .. c0 + cn - 1, cn4 = cn rounded up to 4): the nv = fy x fx vectors of one image's map, from
// (ybase, xbase) on and clamped to the map, go to s_x, ld floats apart. VEC: 16-byte loads; else dword loads, the classes past cn staged as NaN
template <bool VEC>
__device__ __forceinline__ void rs_stage(float *s_x, const float *__restrict__ src, int ybase, int xbase, int fx, int nv, int ld, int cols, int classes,
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

// What an active lane stores for its column ox and rows oy0 .. oy0 + 3 (those inside the H x W map): the label, the score (may be null) and, PROB,
// the probability (may be null) with the threshold on the value stored
template <bool PROB>
__device__ __forceinline__ void rs_store(int *__restrict__ labels, float *__restrict__ score, float *__restrict__ prob, int H, int W, int oy0, int ox,
                                         const float (&best)[RS_ROWS], int (&label)[RS_ROWS], const float (&ref)[RS_ROWS],
                                         const float (&sum)[RS_ROWS], float min_prob, int ignore_label)
{
    const unsigned out = (unsigned)(oy0 * W + ox);        // 32-bit inside an image: its map is below 2^31 bytes
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        if (oy0 + r >= H) break;
        if (PROB) {
            // a finite best has a finite ref <= best <= ref + RS_MARGIN and a sum >= 1 that holds best's own term: 0 < pr <= 1
            const float pr = __builtin_fabsf(best[r]) < __builtin_inff() ? rs_exp(best[r] - ref[r]) / sum[r] : 0.0f;
            if (pr < min_prob) label[r] = ignore_label;                                     // strict, on the value stored below
            if (prob) prob[out + (unsigned)(r * W)] = pr;
        }
        labels[out + (unsigned)(r * W)] = label[r];
        if (score) score[out + (unsigned)(r * W)] = best[r];
    }
}

// One 32 x 32 tile of one image: src = the image's logits, labels / score = the image's output maps (score may be null), H x W their size.
// WIN: the outputs resample the window (wy, wx) of the network's input instead of the whole map; only the index / weight rule differs.
// PROB: prob = the image's probability map (may be null), written beside the score; a pixel below a.min_prob stores a.ignore_label.
template <bool VEC, bool WIN, bool PROB>
__device__ __forceinline__ void resample_tile(const ResampleArgs &a, const float *__restrict__ src, int *__restrict__ labels,
                                              float *__restrict__ score, float *__restrict__ prob, int H, int W, int ty, int tx, float *s_x,
                                              const RsWindow &wy, const RsWindow &wx)
{
    const int tid = threadIdx.x;
    const int ld = a.ch + 4;                  // 16-byte aligned rows, consecutive vectors 4 banks apart
    const int nv = a.fy * a.fx;
    int ybase, xbase;
    float unused;
    rs_coord<WIN>(RS_TILE * ty, a.rows, H, wy, &ybase, &unused);
    rs_coord<WIN>(RS_TILE * tx, a.cols, W, wx, &xbase, &unused);

    // this lane's pixels: column ox, rows oy0 .. oy0 + 3 (a coordinate past the image is evaluated at the last one and not stored)
    const int ox = RS_TILE * tx + (tid & 31), oy0 = RS_TILE * ty + RS_ROWS * (tid >> 5);
    const bool active = ox < W && oy0 < H;
    int x0, ya = 0;
    float wx1, wy1[RS_ROWS], wy0[RS_ROWS];
    bool up[RS_ROWS];                         // row r interpolates between (ya + 1, ya + 2) instead of (ya, ya + 1)
    rs_coord<WIN>(min(ox, W - 1), a.cols, W, wx, &x0, &wx1);
    const float wx0 = 1.0f - wx1;
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        int r0;
        rs_coord<WIN>(min(oy0 + r, H - 1), a.rows, H, wy, &r0, &wy1[r]);
        wy0[r] = 1.0f - wy1[r];
        if (r == 0) ya = r0;
        up[r] = r0 != ya;                     // r0 is ya or ya + 1: four rows span less than one coarse row
    }
    // the same for every lane of the wave (its two groups of rows): at ratio r about 3 / r of the groups cross a coarse row
    const bool cross = __ballot(up[1] || up[2] || up[3]) != 0;
    // LDS word offsets of the six vectors: rows ya, min(ya + 1, rows - 1), min(ya + 2, rows - 1) x columns x0, min(x0 + 1, cols - 1). The slots are
    // inside the staged block by construction; the clamps cost nothing and keep every read inside the launch's LDS whatever the arguments.
    const int last_y = a.rows - 1, last_x = a.cols - 1;
    const int sx0 = min(max(x0 - xbase, 0), a.fx - 1), sx1 = min(max(min(x0 + 1, last_x) - xbase, 0), a.fx - 1);
    const float *p[3][2];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int sy = min(max(min(ya + j, last_y) - ybase, 0), a.fy - 1);
        p[j][0] = s_x + (sy * a.fx + sx0) * ld;
        p[j][1] = s_x + (sy * a.fx + sx1) * ld;
    }

    float best[RS_ROWS], ref[RS_ROWS], sum[RS_ROWS];      // ref, sum: the PROB instantiations' lazy reference and softmax sum
    int label[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) { best[r] = ref[r] = -__builtin_inff(); sum[r] = 0.0f; label[r] = 0; }

    for (int c0 = 0; c0 < a.classes; c0 += a.ch) {
        const int cn = min(a.ch, a.classes - c0), cn4 = (cn + 3) & ~3;
        // ---- stage: nv vectors x cn4 classes
        rs_stage<VEC>(s_x, src, ybase, xbase, a.fx, nv, ld, a.cols, a.classes, last_y, last_x, c0, cn, cn4, tid);
        __syncthreads();
        // ---- reduce
        if (active) {
            if (cross) rs_reduce<true, PROB>(p, cn4, c0, wx0, wx1, wy0, wy1, up, best, label, ref, sum);
            else rs_reduce<false, PROB>(p, cn4, c0, wx0, wx1, wy0, wy1, up, best, label, ref, sum);
        }
        __syncthreads();
    }
    if (!active) return;
    rs_store<PROB>(labels, score, prob, H, W, oy0, ox, best, label, ref, sum, a.min_prob, a.ignore_label);
}

template <bool VEC, bool WIN, bool PROB>
__device__ __forceinline__ void resample_uniform(const ResampleArgs &a, float *s_rs)
{
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const size_t img = (size_t)blockIdx.y;                                                      // 64-bit base, 32-bit offsets inside an image
    const size_t map = (size_t)a.out_rows * a.out_cols;
    const RsWindow wy = { a.in_rows, a.wy, a.wih }, wx = { a.in_cols, a.wx, a.wiw };          // read by the WIN instantiations only
    resample_tile<VEC, WIN, PROB>(a, a.logits + img * ((size_t)a.rows * a.cols * a.classes), a.labels + img * map,
                                  a.score ? a.score + img * map : nullptr, PROB && a.prob ? a.prob + img * map : nullptr, a.out_rows, a.out_cols, ty, tx,
                                  s_rs, wy, wx);
}

template <bool VEC, bool WIN>
__global__ __launch_bounds__(256) void resample_argmax_f32(const ResampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rs[];
    resample_uniform<VEC, WIN, false>(a, s_rs);
}

template <bool VEC, bool WIN>
__global__ __launch_bounds__(256) void resample_softmax_f32(const ResampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rs[];
    resample_uniform<VEC, WIN, true>(a, s_rs);
}

// A ragged set holds one kind of item, which WIN selects; rs_windows gives an item's windows along y and x (read by the WIN instantiations only).
template <bool WIN>
using RsItem = typename std::conditional<WIN, mbn_label_window_item, mbn_label_item>::type;
__device__ __forceinline__ void rs_windows(const ResampleArgs &, const mbn_label_item &, RsWindow *wy, RsWindow *wx) { *wy = *wx = RsWindow{ 0, 0, 0 }; }
__device__ __forceinline__ void rs_windows(const ResampleArgs &a, const mbn_label_window_item &it, RsWindow *wy, RsWindow *wx)
{
    *wy = RsWindow{ a.in_rows, it.y, it.ih };
    *wx = RsWindow{ a.in_cols, it.x, it.iw };
}

// grid = (tiles of the largest item, batch): a workgroup past its own image's tiles returns before any load or barrier
template <bool VEC, bool WIN, bool PROB>
__device__ __forceinline__ void resample_ragged(const ResampleArgs &a, float *s_rs)
{
    // a replay of a captured launch after another set: the items are no longer the ones its grid, LDS and spans were checked for
    if (a.head->generation != a.generation || (int)blockIdx.y >= a.head->batch) return;
    const RsItem<WIN> it = (WIN ? (const RsItem<WIN> *)a.witems : (const RsItem<WIN> *)a.items)[blockIdx.y];
    const int tiles_x = (it.cols + RS_TILE - 1) / RS_TILE, tiles_y = (it.rows + RS_TILE - 1) / RS_TILE;
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    if (ty >= tiles_y) return;
    const size_t img = (size_t)blockIdx.y;
    RsWindow wy, wx;
    rs_windows(a, it, &wy, &wx);
    resample_tile<VEC, WIN, PROB>(a, a.logits + img * ((size_t)a.rows * a.cols * a.classes), a.labels + it.dst_offset,
                                  a.score ? a.score + it.dst_offset : nullptr, PROB && a.prob ? a.prob + it.dst_offset : nullptr, it.rows, it.cols,
                                  ty, tx, s_rs, wy, wx);
}

template <bool VEC, bool WIN>
__global__ __launch_bounds__(256) void resample_argmax_ragged_f32(const ResampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rs[];
    resample_ragged<VEC, WIN, false>(a, s_rs);
}

template <bool VEC, bool WIN>
__global__ __launch_bounds__(256) void resample_softmax_ragged_f32(const ResampleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rs[];
    resample_ragged<VEC, WIN, true>(a, s_rs);
}

// The sixteen kernels by [ragged][prob][win][vec]; vec: `logits` on 16 bytes and classes % 4 == 0, so that every class vector starts on 16 bytes
typedef void (*RsKernel)(const ResampleArgs);
const RsKernel rs_kernels[2][2][2][2] = {
    { { { resample_argmax_f32<false, false>, resample_argmax_f32<true, false> }, { resample_argmax_f32<false, true>, resample_argmax_f32<true, true> } },
      { { resample_softmax_f32<false, false>, resample_softmax_f32<true, false> }, { resample_softmax_f32<false, true>, resample_softmax_f32<true, true> } } },
    { { { resample_argmax_ragged_f32<false, false>, resample_argmax_ragged_f32<true, false> },
        { resample_argmax_ragged_f32<false, true>, resample_argmax_ragged_f32<true, true> } },
      { { resample_softmax_ragged_f32<false, false>, resample_softmax_ragged_f32<true, false> },
        { resample_softmax_ragged_f32<false, true>, resample_softmax_ragged_f32<true, true> } } },
};

// What every form's launch carries: the buffers, the coarse map, the launch's plan, the network input a window lies in (WIN) and q, the softmax
// read-out's extras (null for the argmax read-out). The form adds its own: the output size and rectangle, or the handle's items.
ResampleArgs rs_args(int32_t *labels, float *score, const float *logits, int rows, int cols, int classes, const mbn_resample_launch_t &l, int in_rows,
                     int in_cols, const mbn_readout_prob *q)
{
    ResampleArgs a = {};
    a.labels = labels; a.score = score; a.logits = logits;
    a.rows = rows; a.cols = cols; a.classes = classes;
    a.fy = l.fy; a.fx = l.fx; a.ch = l.ch;
    a.in_rows = in_rows; a.in_cols = in_cols;
    if (q) { a.prob = q->prob; a.min_prob = q->min_prob; a.ignore_label = q->ignore_label; }
    return a;
}

void rs_launch(bool ragged, bool prob, bool win, int batch, const mbn_resample_launch_t &l, hipStream_t s, const ResampleArgs &a)
{
    const bool vec = ((uintptr_t)a.logits % 16) == 0 && (a.classes % 4) == 0;
    hipLaunchKernelGGL(rs_kernels[ragged][prob][win][vec], dim3((unsigned)l.tiles, (unsigned)batch), dim3(256), (size_t)l.lds_bytes, s, a);
}

// ---- ENSEMBLE (mbn_resample_ensemble_f32; include/mbn.h, "segment with test-time augmentation"): K views of the same images, each a window of the
// network's input and possibly mirrored, are read out as ONE map: per class and pixel the K interpolants are summed in view order, the sum is scaled
// by 1 / K, and the compare (and the softmax sum) sees that mean. The tile is resample_tile's: 32 x 32 outputs per workgroup, a lane one column and
// four rows, the same index / weight rule (rs_coord<true>), the same lerps, the same lazy-reference sum, the same store. What differs:
//   stage   per class chunk ALL K footprints go to LDS, view k's fy x fx vectors at k * fy * fx, each from its own (ybase, xbase): the rectangles
//           differ, so the views' footprints lie elsewhere in the map. The chunk is smaller for it (host/mbn_envelope.h, MBN_RESAMPLE_ENSEMBLE_CH)
//   reduce  per group of four classes the views are visited in order and the four rows' sums stay in registers; the compare runs once per class
//           on the mean. A view takes the two-interpolant form when none of the wave's rows crosses a coarse row IN THAT VIEW (a ballot per view)
//   mirror  a mirrored view evaluates its columns at W - 1 - ox: the lane's column of that view, and the tile's xbase from its LAST column
// A lane's per-view state (LDS offsets, weights, up bits) is indexed at compile time only: K is a template parameter and every loop over the views
// is unrolled, so the state stays in registers (a runtime index would send it to scratch). The views travel by value in the kernel's arguments.
struct EnsembleArgs {
    int *labels;
    float *score, *prob;     // either may be null (prob: PROB instantiations only)
    const float *logits;     // [K][batch][rows][cols][classes]
    int rows, cols, classes, batch;
    int out_rows, out_cols, tiles_x;
    int fy, fx, ch;          // the launch's footprint PER VIEW and the class chunk: mbn_resample_ensemble_plan
    int in_rows, in_cols;
    float inv_k, min_prob;   // 1.0f / (float)K
    int ignore_label;
    mbn_view views[MBN_ENSEMBLE_MAX_VIEWS];
};
static_assert(sizeof(mbn_view) == 32, "a view is 32 bytes: eight of them travel in the kernel's arguments");

// a lane's state for one view
struct EnsView {
    int off[3][2];           // LDS word offsets of the six vectors, as resample_tile's p
    float wx1, wy1[RS_ROWS]; // the weights of i1; those of i0 are formed where they are used (1.0f - w1: the same value every time)
    unsigned up;             // bit r: row r interpolates between (ya + 1, ya + 2); one register per view instead of four lane masks
    bool cross;              // some row of the wave has a bit set in this view
};

// adds one view's interpolants of the four classes at c to the lane's sums (first: they ARE the sums); rs_reduce's products and sums
template <bool CROSS>
__device__ __forceinline__ void ens_add(const float *s_x, const EnsView &e, int c, bool first, float (&s)[RS_ROWS][4])
{
#pragma clang fp contract(off)
    constexpr int NT = CROSS ? 3 : 2;
    const float wx0 = 1.0f - e.wx1;
    f4 v0[NT], v1[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
        v0[j] = *reinterpret_cast<const f4 *>(s_x + e.off[j][0] + c);
        v1[j] = *reinterpret_cast<const f4 *>(s_x + e.off[j][1] + c);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float t[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) t[j] = rs_lerp(v0[j][k], wx0, v1[j][k], e.wx1);            // horizontal first
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) {
            const bool up = CROSS && (e.up >> r & 1u);
            const float ta = up ? t[1] : t[0], tb = up ? t[NT - 1] : t[1];
            const float v = rs_lerp(ta, 1.0f - e.wy1[r], tb, e.wy1[r]);                         // then vertical
            s[r][k] = first ? v : s[r][k] + v;                                                  // view order, one rounding per view
        }
    }
}

template <int K, bool VEC, bool PROB>
__global__ __launch_bounds__(256) void resample_ensemble_f32(const EnsembleArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rs[];
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const size_t img = (size_t)blockIdx.y;                                                      // 64-bit bases, 32-bit offsets inside a map
    const size_t map = (size_t)a.out_rows * a.out_cols, lmap = (size_t)a.rows * a.cols * a.classes;
    const int H = a.out_rows, W = a.out_cols;
    const int ld = a.ch + 4, nv = a.fy * a.fx;
    const int last_y = a.rows - 1, last_x = a.cols - 1;
    const int ox = RS_TILE * tx + (tid & 31), oy0 = RS_TILE * ty + RS_ROWS * (tid >> 5);
    const bool active = ox < W && oy0 < H;
    const int oxc = min(ox, W - 1), xe = min(RS_TILE * tx + RS_TILE - 1, W - 1);                // this lane's column, the tile's last one

    EnsView e[K];
    int ybase[K], xbase[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const mbn_view &vw = a.views[k];
        const RsWindow wy = { a.in_rows, vw.y, vw.ih }, wx = { a.in_cols, vw.x, vw.iw };
        const bool mirror = vw.mirror != 0;
        float unused;
        rs_coord<true>(RS_TILE * ty, a.rows, H, wy, &ybase[k], &unused);
        // i0 grows with the coordinate: the tile's leftmost source column belongs to its first output, mirrored to its last one
        rs_coord<true>(mirror ? W - 1 - xe : RS_TILE * tx, a.cols, W, wx, &xbase[k], &unused);
        int x0, ya = 0;
        rs_coord<true>(mirror ? W - 1 - oxc : oxc, a.cols, W, wx, &x0, &e[k].wx1);
        e[k].up = 0;
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) {
            int r0;
            rs_coord<true>(min(oy0 + r, H - 1), a.rows, H, wy, &r0, &e[k].wy1[r]);
            if (r == 0) ya = r0;
            e[k].up |= (unsigned)(r0 != ya) << r; // r0 is ya or ya + 1: four rows span less than one coarse row
        }
        e[k].cross = __ballot(e[k].up != 0) != 0;
        // inside view k's staged block by construction; the clamps keep every read inside the launch's LDS whatever the arguments
        const int sx0 = min(max(x0 - xbase[k], 0), a.fx - 1), sx1 = min(max(min(x0 + 1, last_x) - xbase[k], 0), a.fx - 1);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int sy = min(max(min(ya + j, last_y) - ybase[k], 0), a.fy - 1);
            e[k].off[j][0] = (k * nv + sy * a.fx + sx0) * ld;
            e[k].off[j][1] = (k * nv + sy * a.fx + sx1) * ld;
        }
    }

    float best[RS_ROWS], ref[RS_ROWS], sum[RS_ROWS];
    int label[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) { best[r] = ref[r] = -__builtin_inff(); sum[r] = 0.0f; label[r] = 0; }

    for (int c0 = 0; c0 < a.classes; c0 += a.ch) {
        const int cn = min(a.ch, a.classes - c0), cn4 = (cn + 3) & ~3;
#pragma unroll
        for (int k = 0; k < K; k++)
            rs_stage<VEC>(s_rs + k * nv * ld, a.logits + ((size_t)k * a.batch + img) * lmap, ybase[k], xbase[k], a.fx, nv, ld, a.cols, a.classes, last_y,
                          last_x, c0, cn, cn4, tid);
        __syncthreads();
        if (active) {
            for (int c = 0; c < cn4; c += 4) {
                float s[RS_ROWS][4] = {}, vv[RS_ROWS][4];
#pragma unroll
                for (int k = 0; k < K; k++) {
                    if (e[k].cross) ens_add<true>(s_rs, e[k], c, k == 0, s);
                    else ens_add<false>(s_rs, e[k], c, k == 0, s);
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
#pragma unroll
                    for (int r = 0; r < RS_ROWS; r++) {
#pragma clang fp contract(off)
                        const float t = s[r][k] * a.inv_k;                                      // the mean: one rounding
                        if (t > best[r]) { best[r] = t; label[r] = c0 + c + k; }
                        vv[r][k] = t;
                    }
                }
                if (PROB) rs_softmax_group(vv, ref, sum);
            }
        }
        __syncthreads();
    }
    if (!active) return;
    rs_store<PROB>(a.labels + img * map, a.score ? a.score + img * map : nullptr, PROB && a.prob ? a.prob + img * map : nullptr, H, W, oy0, ox, best,
                   label, ref, sum, a.min_prob, a.ignore_label);
}

// the thirty-two ensemble kernels by [K - 1][prob][vec]
typedef void (*EnsKernel)(const EnsembleArgs);
#define ENS_K(K) { { resample_ensemble_f32<K, false, false>, resample_ensemble_f32<K, true, false> },   \
                   { resample_ensemble_f32<K, false, true>, resample_ensemble_f32<K, true, true> } }
const EnsKernel ens_kernels[MBN_ENSEMBLE_MAX_VIEWS][2][2] = { ENS_K(1), ENS_K(2), ENS_K(3), ENS_K(4), ENS_K(5), ENS_K(6), ENS_K(7), ENS_K(8) };
#undef ENS_K

// ---- SLIDE (mbn_resample_slide_f32; include/mbn.h, "segment by sliding window"): a grid of overlapping tiles of the same images, each read out by
// the plain rule to its own tile_rows x tile_cols rectangle of the output, is read out as ONE map: per class and pixel the interpolants of the tiles
// over the pixel are summed in tile order, the sum is scaled by 1 / count, and the compare (and the softmax sum) sees that mean. A sibling of the
// ensemble: the same lane layout, stage pass, lerps (ens_add), softmax sum and store. What differs:
//   pieces  a view covers the whole output, a tile only its rectangle, and the number of tiles over a pixel varies. The tile edges cut each axis into
//           cells of constant coverage (at most 31); a workgroup takes a PIECE, at most 32 x 32 outputs that start at a cell's corner and end at its
//           far borders, so all its pixels have the same Ky x Kx <= 3 x 3 tiles over them. grid.x = pieces along y x pieces along x; a workgroup
//           finds its cell in the per-axis prefix tables of its arguments (host/mbn_envelope.c, mbn_slide_cells). A piece need not start at a
//           multiple of 32 of its tile: MBN_RESAMPLE_FOOT bounds what ANY 32 consecutive outputs touch
//   rule    each tile is an image of its own: the plain rule (rs_axis, 32-bit) at the coordinate inside the tile
//   state   a lane's state is separable: per tile ROW over the piece the four rows' weights, up bits and LDS row offsets, per tile COLUMN the
//           column's weight and LDS offsets: 3 x 8 + 3 x 3 words instead of nine views' 9 x 12. The loops over the tile rows and columns are unrolled
//           to three with a uniform guard, so the state is indexed at compile time only and stays in registers
//   stage   per class chunk the Ky x Kx footprints go to LDS, tile (ky, kx) of the piece at (ky * Kx + kx) * fy * fx vectors
struct SlideArgs {
    int *labels;
    float *score, *prob;     // either may be null (prob: PROB instantiations only)
    const float *logits;     // [batch][ny * nx][rows][cols][classes]
    int rows, cols, classes;
    int out_rows, out_cols;
    int fy, fx, ch;          // the launch's footprint PER TILE and the class chunk: mbn_resample_slide_plan
    int cells_y, cells_x;
    float min_prob;
    int ignore_label;
    float inv[10];           // inv[count] = 1.0f / (float)count
    mbn_slide s;
    int edge_y[MBN_SLIDE_MAX_CELLS + 1], pieces_y[MBN_SLIDE_MAX_CELLS + 1];      // mbn_slide_cells of the two axes
    int edge_x[MBN_SLIDE_MAX_CELLS + 1], pieces_x[MBN_SLIDE_MAX_CELLS + 1];
};
static_assert(sizeof(mbn_slide) == 144, "a plan is 144 bytes: it travels in the kernel's arguments");

constexpr int SL_K = 3;      // tiles over a coordinate at most

// a workgroup's piece along one axis: its first output, its outputs (1..32), the first tile over it and how many are
struct SlidePiece {
    int o0, lim, k0, K;
};

// piece b of an axis: the cell is found in the prefix table (uniform, at most 31 steps); the tiles over it are those that hold its first output
__device__ __forceinline__ SlidePiece slide_piece(const int *edge, const int *pieces, int cells, const int *pos, int n, int tile, int b)
{
    int c = 0;
    while (c + 1 < cells && pieces[c + 1] <= b) c++;
    SlidePiece p;
    p.o0 = edge[c] + RS_TILE * (b - pieces[c]);
    p.lim = min(RS_TILE, edge[c + 1] - p.o0);
    p.k0 = p.K = 0;
    for (int i = 0; i < n; i++) {
        if (pos[i] + tile <= p.o0) p.k0 = i + 1;      // the positions ascend: the tiles that end in front of the piece are the first ones
        else if (pos[i] <= p.o0) p.K++;
    }
    p.K = min(max(p.K, 1), SL_K);                     // 1..3 inside the envelope; the clamp keeps the staged slots inside the launch's LDS anyway
    p.k0 = min(p.k0, n - p.K);
    return p;
}

template <bool VEC, bool PROB>
__global__ __launch_bounds__(256) void resample_slide_f32(const SlideArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rs[];
    const int tid = threadIdx.x;
    const int pieces_x = a.pieces_x[a.cells_x];
    const int by = (int)blockIdx.x / pieces_x, bx = (int)blockIdx.x - by * pieces_x;
    const SlidePiece py = slide_piece(a.edge_y, a.pieces_y, a.cells_y, a.s.y, a.s.ny, a.s.tile_rows, by);
    const SlidePiece px = slide_piece(a.edge_x, a.pieces_x, a.cells_x, a.s.x, a.s.nx, a.s.tile_cols, bx);
    const size_t img = (size_t)blockIdx.y;                                                      // 64-bit bases, 32-bit offsets inside a map
    const size_t map = (size_t)a.out_rows * a.out_cols, lmap = (size_t)a.rows * a.cols * a.classes;
    const int ld = a.ch + 4, nv = a.fy * a.fx;
    const int last_y = a.rows - 1, last_x = a.cols - 1;
    const int lx = tid & 31, ly0 = RS_ROWS * (tid >> 5);
    const bool active = lx < px.lim && ly0 < py.lim;
    const int ox = px.o0 + lx, oy0 = py.o0 + ly0;
    const int oxc = px.o0 + min(lx, px.lim - 1), y_end = py.o0 + py.lim;                       // a coordinate past the piece is evaluated at its last one

    // per tile column over the piece: the footprint's first coarse column, the lane's weight and its two LDS offsets inside a tile's block
    int xbase[SL_K], col[SL_K][2];
    float wx1[SL_K];
#pragma unroll
    for (int kx = 0; kx < SL_K; kx++) {
        const int t0 = a.s.x[px.k0 + (kx < px.K ? kx : 0)];                                     // past the last tile: the first one's, never used
        int x0;
        float unused;
        rs_axis(px.o0 - t0, a.cols, a.s.tile_cols, &xbase[kx], &unused);
        rs_axis(oxc - t0, a.cols, a.s.tile_cols, &x0, &wx1[kx]);
        // inside the tile's staged block by construction; the clamps keep every read inside the launch's LDS whatever the arguments
        col[kx][0] = (kx * nv + min(max(x0 - xbase[kx], 0), a.fx - 1)) * ld;
        col[kx][1] = (kx * nv + min(max(min(x0 + 1, last_x) - xbase[kx], 0), a.fx - 1)) * ld;
    }
    // per tile row: the footprint's first coarse row, the four rows' weights and up bits, the LDS offsets of the three coarse rows
    int ybase[SL_K], row[SL_K][3];
    float wy1[SL_K][RS_ROWS];
    unsigned up[SL_K];
    bool cross[SL_K];
#pragma unroll
    for (int ky = 0; ky < SL_K; ky++) {
        const int t0 = a.s.y[py.k0 + (ky < py.K ? ky : 0)];
        int ya = 0;
        float unused;
        rs_axis(py.o0 - t0, a.rows, a.s.tile_rows, &ybase[ky], &unused);
        up[ky] = 0;
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) {
            int r0;
            rs_axis(min(oy0 + r, y_end - 1) - t0, a.rows, a.s.tile_rows, &r0, &wy1[ky][r]);
            if (r == 0) ya = r0;
            up[ky] |= (unsigned)(r0 != ya) << r;      // r0 is ya or ya + 1: four rows span less than one coarse row
        }
        cross[ky] = __ballot(up[ky] != 0) != 0;
#pragma unroll
        for (int j = 0; j < 3; j++) row[ky][j] = (ky * px.K * nv + min(max(min(ya + j, last_y) - ybase[ky], 0), a.fy - 1) * a.fx) * ld;
    }
    const float inv = a.inv[py.K * px.K];
    const float *tiles = a.logits + (img * (size_t)(a.s.ny * a.s.nx) + (size_t)(py.k0 * a.s.nx + px.k0)) * lmap;      // the piece's first tile

    float best[RS_ROWS], ref[RS_ROWS], sum[RS_ROWS];
    int label[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) { best[r] = ref[r] = -__builtin_inff(); sum[r] = 0.0f; label[r] = 0; }

    for (int c0 = 0; c0 < a.classes; c0 += a.ch) {
        const int cn = min(a.ch, a.classes - c0), cn4 = (cn + 3) & ~3;
#pragma unroll
        for (int ky = 0; ky < SL_K; ky++) {
            if (ky >= py.K) break;
#pragma unroll
            for (int kx = 0; kx < SL_K; kx++) {
                if (kx >= px.K) break;
                rs_stage<VEC>(s_rs + (ky * px.K + kx) * nv * ld, tiles + (size_t)(ky * a.s.nx + kx) * lmap, ybase[ky], xbase[kx], a.fx, nv, ld, a.cols,
                              a.classes, last_y, last_x, c0, cn, cn4, tid);
            }
        }
        __syncthreads();
        if (active) {
            for (int c = 0; c < cn4; c += 4) {
                float s[RS_ROWS][4] = {}, vv[RS_ROWS][4];
#pragma unroll
                for (int ky = 0; ky < SL_K; ky++) {
                    if (ky >= py.K) break;
#pragma unroll
                    for (int kx = 0; kx < SL_K; kx++) {
                        if (kx >= px.K) break;
                        EnsView e;
#pragma unroll
                        for (int j = 0; j < 3; j++) { e.off[j][0] = row[ky][j] + col[kx][0]; e.off[j][1] = row[ky][j] + col[kx][1]; }
                        e.wx1 = wx1[kx];
#pragma unroll
                        for (int r = 0; r < RS_ROWS; r++) e.wy1[r] = wy1[ky][r];
                        e.up = up[ky];
                        if (cross[ky]) ens_add<true>(s_rs, e, c, ky == 0 && kx == 0, s);        // tile order: ascending iy, then ix
                        else ens_add<false>(s_rs, e, c, ky == 0 && kx == 0, s);
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
#pragma unroll
                    for (int r = 0; r < RS_ROWS; r++) {
#pragma clang fp contract(off)
                        const float t = s[r][k] * inv;                                          // the mean: one rounding
                        if (t > best[r]) { best[r] = t; label[r] = c0 + c + k; }
                        vv[r][k] = t;
                    }
                }
                if (PROB) rs_softmax_group(vv, ref, sum);
            }
        }
        __syncthreads();
    }
    if (!active) return;
    // the rows of the piece end at y_end: rs_store's H
    rs_store<PROB>(a.labels + img * map, a.score ? a.score + img * map : nullptr, PROB && a.prob ? a.prob + img * map : nullptr, y_end, a.out_cols, oy0, ox,
                   best, label, ref, sum, a.min_prob, a.ignore_label);
}

// the four slide kernels by [prob][vec]
typedef void (*SlideKernel)(const SlideArgs);
const SlideKernel slide_kernels[2][2] = { { resample_slide_f32<false, false>, resample_slide_f32<true, false> },
                                          { resample_slide_f32<false, true>, resample_slide_f32<true, true> } };

// ---- TOPK (mbn_resample_topk_f32, _ragged_f32; include/mbn.h, "segment with runners-up"): the k best classes of every output pixel with their
// scores and probabilities, rank-major. Kernels of their own on resample_tile's tile: the same stage pass, coordinates, lerps, lazy-reference
// softmax sum and store pattern. What differs:
//   rule    one index / weight rule, the window's (rs_coord<true>), as in the ensemble: the whole map is the window that covers the whole input
//           (include/mbn.h: bit-equal), so a null rectangle and a plain set travel as that window and there is no plain instantiation
//   state   per row K slots (val, lab), sorted by value descending, instead of (best, label). K is a template CAPACITY: every loop over the slots
//           is unrolled and the slots are indexed at compile time only, so they stay in registers (4 rows x K x 2 words). By the prefix property
//           (the first k' slots of a capacity-K state are the k'-slot state) capacity K serves every k <= K and stores the first k slots
//   compare per class and row ONE compare, against the last slot: the cost of the argmax compare. A class that passes is inserted by a chain of
//           K selects from the bottom up (tk_insert): the rare, divergent path on real logits, the common one on an ascending ramp
//   form    uniform and ragged are one kernel: a.head says which, and a.item_bytes which kind of item the set holds (uniform branches at the head)
struct TopkArgs {
    int *labels;
    float *score, *prob;     // either may be null (prob: PROB instantiations only)
    const float *logits;
    int rows, cols, classes;
    int out_rows, out_cols, tiles_x;      // uniform form
    int fy, fx, ch;
    int k;                   // the slots stored, 1 .. K
    long long plane;         // elements from rank j to rank j + 1 of the three outputs
    float min_prob;
    int ignore_label;
    int in_rows, in_cols;    // the network input the windows lie in (a plain set: rows, cols)
    int wx, wy, wiw, wih;    // uniform form: the window
    const mbn_label_set_head *head;       // ragged form, else null
    int generation, item_bytes;
};

// v > val[K - 1] (the caller's compare): v goes to the smallest j with v > val[j] and the slots from there move down one. From the bottom up slot j
// takes its upper neighbour's content when v belongs above it, v itself when v belongs exactly there; the strict compares keep equal values in
// ascending class order and keep a NaN out
template <int K>
__device__ __forceinline__ void tk_insert(float (&val)[K], int (&lab)[K], float v, int c)
{
#pragma unroll
    for (int j = K - 1; j > 0; j--) {
        const bool above = v > val[j - 1], here = v > val[j];
        val[j] = above ? val[j - 1] : here ? v : val[j];
        lab[j] = above ? lab[j - 1] : here ? c : lab[j];
    }
    if (v > val[0]) { val[0] = v; lab[0] = c; }
}

// rs_reduce with the K slots in the place of (best, label); the same products and sums in the same order, the softmax sum by rs_softmax_group
template <int K, bool CROSS, bool PROB>
__device__ __forceinline__ void tk_reduce(const float *(&p)[3][2], int cn4, int c0, float wx0, float wx1, const float (&wy0)[RS_ROWS],
                                          const float (&wy1)[RS_ROWS], const bool (&up)[RS_ROWS], float (&val)[RS_ROWS][K], int (&lab)[RS_ROWS][K],
                                          float (&ref)[RS_ROWS], float (&sum)[RS_ROWS])
{
    constexpr int NT = CROSS ? 3 : 2;
    for (int c = 0; c < cn4; c += 4) {
        f4 v0[NT], v1[NT];
        float vv[RS_ROWS][4];
#pragma unroll
        for (int j = 0; j < NT; j++) {
            v0[j] = *reinterpret_cast<const f4 *>(p[j][0] + c);
            v1[j] = *reinterpret_cast<const f4 *>(p[j][1] + c);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float t[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) t[j] = rs_lerp(v0[j][k], wx0, v1[j][k], wx1);      // horizontal first
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                const float ta = CROSS && up[r] ? t[1] : t[0], tb = CROSS && up[r] ? t[NT - 1] : t[1];
                const float v = rs_lerp(ta, wy0[r], tb, wy1[r]);                            // then vertical
                if (v > val[r][K - 1]) tk_insert<K>(val[r], lab[r], v, c0 + c + k);
                if (PROB) vv[r][k] = v;
            }
        }
        if (PROB) rs_softmax_group(vv, ref, sum);
    }
}

template <int K, bool VEC, bool PROB>
__global__ __launch_bounds__(256) void resample_topk_f32(const TopkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rs[];
    const int tid = threadIdx.x;
    // ---- this workgroup's image: its output size, its place in a plane, its windows and its tile
    int H = a.out_rows, W = a.out_cols, tiles_x = a.tiles_x;
    size_t dst = (size_t)blockIdx.y * ((size_t)a.out_rows * a.out_cols);                          // 64-bit bases, 32-bit offsets inside a map
    RsWindow wy = { a.in_rows, a.wy, a.wih }, wx = { a.in_cols, a.wx, a.wiw };
    if (a.head) {
        // a replay of a captured launch after another set: the items are no longer the ones its grid, LDS and spans were checked for
        if (a.head->generation != a.generation || (int)blockIdx.y >= a.head->batch) return;
        const char *at = (const char *)(a.head + 1) + (size_t)blockIdx.y * a.item_bytes;
        const mbn_label_item it = *(const mbn_label_item *)at;
        H = it.rows; W = it.cols;
        dst = (size_t)it.dst_offset;
        tiles_x = (W + RS_TILE - 1) / RS_TILE;
        if (a.item_bytes == (int)sizeof(mbn_label_window_item)) {
            const mbn_label_window_item wi = *(const mbn_label_window_item *)at;
            wy.b = wi.y; wy.l = wi.ih; wx.b = wi.x; wx.l = wi.iw;
        }
    }
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    if (ty >= (H + RS_TILE - 1) / RS_TILE) return;                                              // ragged: past this image's tiles
    const float *__restrict__ src = a.logits + (size_t)blockIdx.y * ((size_t)a.rows * a.cols * a.classes);

    // ---- resample_tile's lane state under the window rule
    const int ld = a.ch + 4, nv = a.fy * a.fx;
    int ybase, xbase;
    float unused;
    rs_coord<true>(RS_TILE * ty, a.rows, H, wy, &ybase, &unused);
    rs_coord<true>(RS_TILE * tx, a.cols, W, wx, &xbase, &unused);
    const int ox = RS_TILE * tx + (tid & 31), oy0 = RS_TILE * ty + RS_ROWS * (tid >> 5);
    const bool active = ox < W && oy0 < H;
    int x0, ya = 0;
    float wx1, wy1[RS_ROWS], wy0[RS_ROWS];
    bool up[RS_ROWS];
    rs_coord<true>(min(ox, W - 1), a.cols, W, wx, &x0, &wx1);
    const float wx0 = 1.0f - wx1;
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        int r0;
        rs_coord<true>(min(oy0 + r, H - 1), a.rows, H, wy, &r0, &wy1[r]);
        wy0[r] = 1.0f - wy1[r];
        if (r == 0) ya = r0;
        up[r] = r0 != ya;                     // r0 is ya or ya + 1: four rows span less than one coarse row
    }
    const bool cross = __ballot(up[1] || up[2] || up[3]) != 0;
    // inside the staged block by construction; the clamps keep every read inside the launch's LDS whatever the arguments
    const int last_y = a.rows - 1, last_x = a.cols - 1;
    const int sx0 = min(max(x0 - xbase, 0), a.fx - 1), sx1 = min(max(min(x0 + 1, last_x) - xbase, 0), a.fx - 1);
    const float *p[3][2];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int sy = min(max(min(ya + j, last_y) - ybase, 0), a.fy - 1);
        p[j][0] = s_rs + (sy * a.fx + sx0) * ld;
        p[j][1] = s_rs + (sy * a.fx + sx1) * ld;
    }

    float val[RS_ROWS][K], ref[RS_ROWS], sum[RS_ROWS];
    int lab[RS_ROWS][K];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        ref[r] = -__builtin_inff(); sum[r] = 0.0f;
#pragma unroll
        for (int j = 0; j < K; j++) { val[r][j] = -__builtin_inff(); lab[r][j] = -1; }     // unfilled, wherever an insertion moves it (rank 0: the store)
    }

    for (int c0 = 0; c0 < a.classes; c0 += a.ch) {
        const int cn = min(a.ch, a.classes - c0), cn4 = (cn + 3) & ~3;
        rs_stage<VEC>(s_rs, src, ybase, xbase, a.fx, nv, ld, a.cols, a.classes, last_y, last_x, c0, cn, cn4, tid);
        __syncthreads();
        if (active) {
            if (cross) tk_reduce<K, true, PROB>(p, cn4, c0, wx0, wx1, wy0, wy1, up, val, lab, ref, sum);
            else tk_reduce<K, false, PROB>(p, cn4, c0, wx0, wx1, wy0, wy1, up, val, lab, ref, sum);
        }
        __syncthreads();
    }
    if (!active) return;

    // ---- store: rs_store's pattern, once per rank. Rank 0 is rs_store's own text on (val[0], lab[0]): the same prob bits, the same threshold
    const unsigned out = (unsigned)(oy0 * W + ox);        // 32-bit inside an image: its map is below 2^31 bytes
#pragma unroll
    for (int j = 0; j < K; j++) {
        if (j >= a.k) break;
        int *__restrict__ labels = a.labels + (size_t)j * (size_t)a.plane + dst;
        float *__restrict__ score = a.score ? a.score + (size_t)j * (size_t)a.plane + dst : nullptr;
        float *__restrict__ prob = PROB && a.prob ? a.prob + (size_t)j * (size_t)a.plane + dst : nullptr;
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) {
            if (oy0 + r >= H) break;
            int l = lab[r][j];
            if (j == 0 && !(val[r][0] > -__builtin_inff())) l = 0;                              // nothing won: the argmax rule's label 0
            if (PROB) {
                // a finite best has a finite ref <= best <= ref + RS_MARGIN and a sum >= 1; val[j] <= best; an unfilled slot (-inf) gives exp = 0
                const float pr = __builtin_fabsf(val[r][0]) < __builtin_inff() ? rs_exp(val[r][j] - ref[r]) / sum[r] : 0.0f;
                if (j == 0 && pr < a.min_prob) l = a.ignore_label;                              // plane 0 only; strict, on the value stored below
                if (prob) prob[out + (unsigned)(r * W)] = pr;
            }
            labels[out + (unsigned)(r * W)] = l;
            if (score) score[out + (unsigned)(r * W)] = val[r][j];
        }
    }
}

// the eight top-k kernels by [capacity 8 instead of 4][prob][vec]; k <= 4 takes capacity 4
typedef void (*TopkKernel)(const TopkArgs);
const TopkKernel topk_kernels[2][2][2] = {
    { { resample_topk_f32<4, false, false>, resample_topk_f32<4, true, false> }, { resample_topk_f32<4, false, true>, resample_topk_f32<4, true, true> } },
    { { resample_topk_f32<8, false, false>, resample_topk_f32<8, true, false> }, { resample_topk_f32<8, false, true>, resample_topk_f32<8, true, true> } },
};

void topk_launch(hipStream_t s, int batch, const mbn_resample_launch_t &l, TopkArgs &a, const float *logits, int rows, int cols, int classes, int k,
                 int64_t plane, int32_t *labels, float *score, const mbn_readout_prob *q)
{
    a.labels = labels; a.score = score; a.logits = logits;
    a.rows = rows; a.cols = cols; a.classes = classes;
    a.fy = l.fy; a.fx = l.fx; a.ch = l.ch;
    a.k = k; a.plane = plane;
    if (q) { a.prob = q->prob; a.min_prob = q->min_prob; a.ignore_label = q->ignore_label; }
    const bool vec = ((uintptr_t)logits % 16) == 0 && (classes % 4) == 0;
    hipLaunchKernelGGL(topk_kernels[k > 4][q != nullptr][vec], dim3((unsigned)l.tiles, (unsigned)batch), dim3(256), (size_t)l.lds_bytes, s, a);
}

// ---- NLL (mbn_resample_nll_f32, _ragged_f32; include/mbn.h, "score the probabilities"): the negative log-likelihood and the Brier score of every
// output pixel's softmax distribution against a ground truth at the output resolution, at up to eight inverse temperatures in one pass, stored as
// maps and added to the table [temps][classes + 1][4]. Kernels of their own on resample_tile's tile, under the top-k's conventions: one index /
// weight rule (the window's), uniform and ragged in one kernel (a.set.head says which). What differs:
//   passes  TWO over the class chunks. Pass 1 is the argmax loop itself (rs_reduce without PROB: best and label have the argmax read-out's bits).
//           Pass 2 forms every v again (a launch of one chunk finds it still staged; more chunks are staged again) and, with d = v - best <= 0,
//           adds e = exp2(d * k_j) to S[r][j] and e * e to Q[r][j] for every temperature j, k_j = fp32(beta_j * log2 e) from the host; the
//           truth's own interpolant v_t is picked where c == t. Nothing overflows at beta = 16, and the lerps are shared by the temperatures
//   state   T is a template CAPACITY (1, 4 or 8), as the top-k's K: the loops over the temperatures are unrolled with a uniform guard, so the
//           4 x T x 2 accumulators are indexed at compile time only and stay in registers. The operations of one temperature are written once
//           (nl_diff, nl_term, nl_score), contraction off: its bits do not depend on the capacity or on the other temperatures
//   table   64-bit integer atomics, aggregated per wave: the lanes that hold one truth class elect the first of them, which adds the wave's
//           count, both fixed-point sums and the correct count once per temperature (mbn_f32_calibration.hip's election, here over a lane's four
//           rows). Label maps are coherent, so a wave holds one to three classes as a rule; after NL_LEADERS rounds what is left adds on its own.
//           Every lane of a workgroup stays to the end for it (no early return of the lanes past the image)
struct NllArgs {
    unsigned long long *table;
    float *nll, *brier;      // either may be null
    const float *logits;
    const uint8_t *truth;    // element 0 of the truth, uint8 or int32
    int truth_bytes;
    int rows, cols, classes;
    int out_rows, out_cols, tiles_x;      // uniform form
    int fy, fx, ch;
    int temps;               // 1 .. T
    long long plane;         // elements from temperature j to j + 1 of the two maps
    int in_rows, in_cols;    // the network input the windows lie in (a plain set: rows, cols)
    int wx, wy, wiw, wih;    // uniform form: the window
    mbn_label_set set;       // ragged form (mbn_label_set.h), else a null head
    float beta[MBN_NLL_MAX_TEMPS], k2[MBN_NLL_MAX_TEMPS];      // beta_j and fp32(beta_j * log2 e)
};

constexpr int NL_LEADERS = 4;             // distinct truth classes a wave aggregates

// d = v - best for the exponent: <= 0 under a finite best. A NaN v (a padding class among them) gives -3e38, whose term is exp2(-inf) = 0 exactly
__device__ __forceinline__ float nl_diff(float v, float best)
{
#pragma clang fp contract(off)
    return __builtin_fmaxf(v - best, -3.0e38f);
}

// e = exp(beta d) as exp2(d * k): one product, v_exp_f32 (a result below 2^-126 may flush to 0, against S >= 1)
__device__ __forceinline__ float nl_term(float d, float k)
{
#pragma clang fp contract(off)
    return __builtin_amdgcn_exp2f(d * k);
}

// the stored (nll, brier) of one pixel at one temperature from its sums, its truth's interpolant vt (NaN: none was picked) and best
__device__ __forceinline__ void nl_score(float S, float Q, float vt, float best, float beta, float k, float *nll, float *brier)
{
#pragma clang fp contract(off)
    const bool have = vt > -__builtin_inff();                                                  // not for a NaN, not for -inf
    const float inv = 1.0f / S;
    const float xt = beta * (vt - best);
    const float et = have ? nl_term(nl_diff(vt, best), k) : 0.0f;                               // the term the sums hold for the truth
    float n = have ? __builtin_amdgcn_logf(S) * 0.693147180559945309f - xt : MBN_NLL_CAP;       // v_log_f32 is log2; S >= 1 is normal
    const float p = et * inv, q = (Q * inv) * inv;
    float b = (1.0f - 2.0f * p) + q;
    if (!(__builtin_fabsf(best) < __builtin_inff())) { n = MBN_NLL_CAP; b = 1.0f; }             // nothing won, or a +inf winner
    *nll = __builtin_fminf(__builtin_fmaxf(n, 0.0f), MBN_NLL_CAP);
    *brier = __builtin_fminf(__builtin_fmaxf(b, 0.0f), 2.0f);
}

// the sum of v over the 64 lanes of a wave; every lane of the wave is active (the caller)
__device__ __forceinline__ unsigned long long nl_wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, d, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), d, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// pass 2 over one staged chunk: rs_reduce's products and sums in the same order, then per temperature the two sums
template <int T, bool CROSS>
__device__ __forceinline__ void nl_reduce(const float *(&p)[3][2], int cn4, int c0, float wx0, float wx1, const float (&wy0)[RS_ROWS],
                                          const float (&wy1)[RS_ROWS], const bool (&up)[RS_ROWS], const float (&best)[RS_ROWS], const int (&t)[RS_ROWS],
                                          const NllArgs &a, float (&vt)[RS_ROWS], float (&S)[RS_ROWS][T], float (&Q)[RS_ROWS][T])
{
    constexpr int NT = CROSS ? 3 : 2;
    for (int c = 0; c < cn4; c += 4) {
        f4 v0[NT], v1[NT];
        float d[RS_ROWS][4];
#pragma unroll
        for (int j = 0; j < NT; j++) {
            v0[j] = *reinterpret_cast<const f4 *>(p[j][0] + c);
            v1[j] = *reinterpret_cast<const f4 *>(p[j][1] + c);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float h[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) h[j] = rs_lerp(v0[j][k], wx0, v1[j][k], wx1);      // horizontal first
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                const float ta = CROSS && up[r] ? h[1] : h[0], tb = CROSS && up[r] ? h[NT - 1] : h[1];
                const float v = rs_lerp(ta, wy0[r], tb, wy1[r]);                            // then vertical
                if (c0 + c + k == t[r]) vt[r] = v;
                d[r][k] = nl_diff(v, best[r]);
            }
        }
#pragma unroll
        for (int j = 0; j < T; j++) {
            if (j >= a.temps) break;
            const float kj = a.k2[j];
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
#pragma clang fp contract(off)
                    const float e = nl_term(d[r][k], kj);
                    S[r][j] += e;                                                           // ascending class order
                    Q[r][j] += e * e;
                }
            }
        }
    }
}

// what one key (a truth class, or `classes`: void) adds to plane j of the table: n pixels, `right` of them labelled correctly, the fixed-point sums
__device__ __forceinline__ void nl_add(const NllArgs &a, int j, int key, unsigned n, unsigned right, unsigned long long qn, unsigned long long qb)
{
    unsigned long long *row = a.table + ((size_t)j * (size_t)(a.classes + 1) + (size_t)key) * 4;
    atomicAdd(row, (unsigned long long)n);
    if (key == a.classes) return;                                                           // void: the count alone
    if (qn) atomicAdd(row + 1, qn);
    if (qb) atomicAdd(row + 2, qb);
    if (right) atomicAdd(row + 3, (unsigned long long)right);
}

template <int T, bool VEC>
__global__ __launch_bounds__(256) void resample_nll_f32(const NllArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_rs[];
    const int tid = threadIdx.x;
    // ---- this workgroup's image: its output size, its place in a plane, its windows and its tile (resample_topk_f32's)
    int H = a.out_rows, W = a.out_cols, tiles_x = a.tiles_x;
    size_t dst = (size_t)blockIdx.y * ((size_t)a.out_rows * a.out_cols);                          // 64-bit bases, 32-bit offsets inside a map
    RsWindow wy = { a.in_rows, a.wy, a.wih }, wx = { a.in_cols, a.wx, a.wiw };
    if (a.set.head) {
        // a replay of a captured launch after another set: the items are no longer the ones its grid, LDS and spans were checked for
        if (mbn_label_set_stale(a.set) || (int)blockIdx.y >= a.set.head->batch) return;
        const mbn_label_item *at = mbn_label_set_item(a.set, (int)blockIdx.y);
        const mbn_label_item it = *at;
        H = it.rows; W = it.cols;
        dst = (size_t)it.dst_offset;
        tiles_x = (W + RS_TILE - 1) / RS_TILE;
        if (a.set.item_bytes == (int)sizeof(mbn_label_window_item)) {
            const mbn_label_window_item wi = *(const mbn_label_window_item *)at;
            wy.b = wi.y; wy.l = wi.ih; wx.b = wi.x; wx.l = wi.iw;
        }
    }
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    if (ty >= (H + RS_TILE - 1) / RS_TILE) return;                                              // ragged: past this image's tiles
    const float *__restrict__ src = a.logits + (size_t)blockIdx.y * ((size_t)a.rows * a.cols * a.classes);

    // ---- resample_tile's lane state under the window rule
    const int ld = a.ch + 4, nv = a.fy * a.fx;
    int ybase, xbase;
    float unused;
    rs_coord<true>(RS_TILE * ty, a.rows, H, wy, &ybase, &unused);
    rs_coord<true>(RS_TILE * tx, a.cols, W, wx, &xbase, &unused);
    const int ox = RS_TILE * tx + (tid & 31), oy0 = RS_TILE * ty + RS_ROWS * (tid >> 5);
    const bool active = ox < W && oy0 < H;
    int x0, ya = 0;
    float wx1, wy1[RS_ROWS], wy0[RS_ROWS];
    bool up[RS_ROWS];
    rs_coord<true>(min(ox, W - 1), a.cols, W, wx, &x0, &wx1);
    const float wx0 = 1.0f - wx1;
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        int r0;
        rs_coord<true>(min(oy0 + r, H - 1), a.rows, H, wy, &r0, &wy1[r]);
        wy0[r] = 1.0f - wy1[r];
        if (r == 0) ya = r0;
        up[r] = r0 != ya;                     // r0 is ya or ya + 1: four rows span less than one coarse row
    }
    const bool cross = __ballot(up[1] || up[2] || up[3]) != 0;
    // inside the staged block by construction; the clamps keep every read inside the launch's LDS whatever the arguments
    const int last_y = a.rows - 1, last_x = a.cols - 1;
    const int sx0 = min(max(x0 - xbase, 0), a.fx - 1), sx1 = min(max(min(x0 + 1, last_x) - xbase, 0), a.fx - 1);
    const float *p[3][2];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int sy = min(max(min(ya + j, last_y) - ybase, 0), a.fy - 1);
        p[j][0] = s_rs + (sy * a.fx + sx0) * ld;
        p[j][1] = s_rs + (sy * a.fx + sx1) * ld;
    }

    // ---- the truth of the lane's pixels: a class, `classes` for a void pixel, -1 where the lane has no pixel (past the image)
    const unsigned out = (unsigned)(oy0 * W + ox);        // 32-bit inside an image: its map is below 2^31 bytes
    int t[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        t[r] = -1;
        if (active && oy0 + r < H) {
            const size_t e = dst + out + (unsigned)(r * W);
            const int v = a.truth_bytes == 1 ? (int)a.truth[e] : ((const int32_t *)a.truth)[e];
            t[r] = (unsigned)v < (unsigned)a.classes ? v : a.classes;
        }
    }

    // ---- pass 1: the argmax loop
    float best[RS_ROWS], ref[RS_ROWS], sum[RS_ROWS];      // ref, sum: rs_reduce's PROB state, unused
    int label[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) { best[r] = ref[r] = -__builtin_inff(); sum[r] = 0.0f; label[r] = 0; }
    for (int c0 = 0; c0 < a.classes; c0 += a.ch) {
        const int cn = min(a.ch, a.classes - c0), cn4 = (cn + 3) & ~3;
        rs_stage<VEC>(s_rs, src, ybase, xbase, a.fx, nv, ld, a.cols, a.classes, last_y, last_x, c0, cn, cn4, tid);
        __syncthreads();
        if (active) {
            if (cross) rs_reduce<true, false>(p, cn4, c0, wx0, wx1, wy0, wy1, up, best, label, ref, sum);
            else rs_reduce<false, false>(p, cn4, c0, wx0, wx1, wy0, wy1, up, best, label, ref, sum);
        }
        if (a.classes > a.ch) __syncthreads();            // one chunk: it stays staged for pass 2
    }

    // ---- pass 2: the sums of every temperature under the final best
    float S[RS_ROWS][T], Q[RS_ROWS][T], vt[RS_ROWS];
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        vt[r] = __builtin_nanf("");
#pragma unroll
        for (int j = 0; j < T; j++) S[r][j] = Q[r][j] = 0.0f;
    }
    for (int c0 = 0; c0 < a.classes; c0 += a.ch) {
        const int cn = min(a.ch, a.classes - c0), cn4 = (cn + 3) & ~3;
        if (a.classes > a.ch) {
            rs_stage<VEC>(s_rs, src, ybase, xbase, a.fx, nv, ld, a.cols, a.classes, last_y, last_x, c0, cn, cn4, tid);
            __syncthreads();
        }
        if (active) {
            if (cross) nl_reduce<T, true>(p, cn4, c0, wx0, wx1, wy0, wy1, up, best, t, a, vt, S, Q);
            else nl_reduce<T, false>(p, cn4, c0, wx0, wx1, wy0, wy1, up, best, t, a, vt, S, Q);
        }
        if (a.classes > a.ch) __syncthreads();
    }

    // ---- the scores, the maps (a void pixel: -1) and the fixed-point terms of the table, from the values stored
    unsigned qn[RS_ROWS][T], qb[RS_ROWS][T];
#pragma unroll
    for (int j = 0; j < T; j++) {
        if (j >= a.temps) break;
        float *__restrict__ nll = a.nll ? a.nll + (size_t)j * (size_t)a.plane + dst : nullptr;
        float *__restrict__ brier = a.brier ? a.brier + (size_t)j * (size_t)a.plane + dst : nullptr;
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) {
            float n, b;
            nl_score(S[r][j], Q[r][j], vt[r], best[r], a.beta[j], a.k2[j], &n, &b);
            qn[r][j] = (unsigned)(n * 65536.0f);                                            // exact: powers of two; at most 2^31 and 2^25
            qb[r][j] = (unsigned)(b * 16777216.0f);
            if (t[r] < 0) continue;
            const bool scored = t[r] < a.classes;
            if (nll) nll[out + (unsigned)(r * W)] = scored ? n : -1.0f;
            if (brier) brier[out + (unsigned)(r * W)] = scored ? b : -1.0f;
        }
    }

    // ---- the table: every lane of the wave is here; one add per distinct truth class and temperature, by the first lane that still holds one
    unsigned todo = 0;
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) todo |= (unsigned)(t[r] >= 0) << r;
    for (int it = 0; it < NL_LEADERS; it++) {
        int mine = -1;
#pragma unroll
        for (int r = RS_ROWS - 1; r >= 0; r--)
            if (todo >> r & 1u) mine = t[r];
        const unsigned long long pending = __ballot(mine >= 0);
        if (!pending) break;
        const int first = __ffsll((long long)pending) - 1;
        const int lead = __builtin_amdgcn_readlane(mine, first);
        unsigned match = 0, counts = 0;                    // counts: the lane's pixels of the class, and in the high half the correct ones
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) {
            if ((todo >> r & 1u) && t[r] == lead) {
                match |= 1u << r;
                counts += 1u + ((unsigned)(label[r] == lead) << 16);
            }
        }
        const unsigned long long both = nl_wave_sum(counts);                                // at most 256 each
        const bool leader = (int)__lane_id() == first;
#pragma unroll
        for (int j = 0; j < T; j++) {
            if (j >= a.temps) break;
            unsigned long long sn = 0, sb = 0;
            if (lead != a.classes) {
#pragma unroll
                for (int r = 0; r < RS_ROWS; r++) {
                    if (match >> r & 1u) { sn += qn[r][j]; sb += qb[r][j]; }
                }
                sn = nl_wave_sum(sn);
                sb = nl_wave_sum(sb);
            }
            if (leader) nl_add(a, j, lead, (unsigned)both & 0xffffu, (unsigned)(both >> 16) & 0xffffu, sn, sb);
        }
        todo &= ~match;
    }
    // what is left after the rounds (a wave with many classes): every pixel on its own
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        if (!(todo >> r & 1u)) continue;
#pragma unroll
        for (int j = 0; j < T; j++) {
            if (j >= a.temps) break;
            nl_add(a, j, t[r], 1u, (unsigned)(label[r] == t[r]), qn[r][j], qb[r][j]);
        }
    }
}

// the six NLL kernels by [capacity: 1, 4, 8][vec]
typedef void (*NllKernel)(const NllArgs);
const NllKernel nll_kernels[3][2] = { { resample_nll_f32<1, false>, resample_nll_f32<1, true> },
                                      { resample_nll_f32<4, false>, resample_nll_f32<4, true> },
                                      { resample_nll_f32<8, false>, resample_nll_f32<8, true> } };

void nll_launch(hipStream_t s, int batch, const mbn_resample_launch_t &l, NllArgs &a, void *table, float *nll, float *brier, int64_t plane,
                const float *logits, const void *truth, int truth_bytes, int rows, int cols, int classes, const float *inv_temps, int temps)
{
    a.table = (unsigned long long *)table; a.nll = nll; a.brier = brier; a.plane = plane;
    a.logits = logits; a.truth = (const uint8_t *)truth; a.truth_bytes = truth_bytes;
    a.rows = rows; a.cols = cols; a.classes = classes;
    a.fy = l.fy; a.fx = l.fx; a.ch = l.ch;
    a.temps = temps;
    for (int j = 0; j < temps; j++) {
        a.beta[j] = inv_temps[j];
        a.k2[j] = (float)((double)inv_temps[j] * 1.44269504088896341);                      // one rounding
    }
    const bool vec = ((uintptr_t)logits % 16) == 0 && (classes % 4) == 0;
    hipLaunchKernelGGL(nll_kernels[temps > 4 ? 2 : temps > 1][vec], dim3((unsigned)l.tiles, (unsigned)batch), dim3(256), (size_t)l.lds_bytes, s, a);
}

}   // namespace

// rect = null: the whole map, the window (0, 0, cols, rows) of a rows x cols input. The shape is inside mbn_resample_nll_envelope, the temperatures
// inside mbn_nll_temps_check and the pointers checked (the caller); nll / brier may be null
int mbn_launch_f32_resample_nll(mbn_context *, hipStream_t s, void *table, float *nll, float *brier, const float *logits, const void *truth,
                                int truth_bytes, int batch, int rows, int cols, int classes, int in_rows, int in_cols, const int32_t *rect,
                                int out_rows, int out_cols, const float *inv_temps, int temps)
{
    const int32_t full[4] = { 0, 0, cols, rows };
    if (!rect) { rect = full; in_rows = rows; in_cols = cols; }
    mbn_resample_launch_t l = { 0, 0, 0, 0, 0, 0 };
    mbn_resample_window_plan(rows, cols, in_rows, in_cols, rect, out_rows, out_cols, &l);
    NllArgs a = {};
    a.out_rows = out_rows; a.out_cols = out_cols;
    a.tiles_x = (out_cols + RS_TILE - 1) / RS_TILE;
    a.in_rows = in_rows; a.in_cols = in_cols;
    a.wx = rect[0]; a.wy = rect[1]; a.wiw = rect[2]; a.wih = rect[3];
    nll_launch(s, batch, l, a, table, nll, brier, (int64_t)batch * out_rows * out_cols, logits, truth, truth_bytes, rows, cols, classes, inv_temps,
               temps);
    return MBN_OK;
}

// the handle has a batch, plane_stride covers the set's span, the temperatures and the pointers are checked and the spans fit (the caller)
int mbn_launch_f32_resample_nll_ragged(mbn_ragged_readout *r, hipStream_t s, void *table, float *nll, float *brier, int64_t plane_stride,
                                       const float *logits, const void *truth, int truth_bytes, const float *inv_temps, int temps)
{
    NllArgs a = {};
    a.tiles_x = 1;                                              // unused: a workgroup takes its image's own
    // a plain set's items are the full window of a rows x cols input (what its check planned them as)
    a.in_rows = r->window ? r->in_rows : r->rows; a.in_cols = r->window ? r->in_cols : r->cols;
    a.wx = 0; a.wy = 0; a.wiw = a.in_cols; a.wih = a.in_rows;
    a.set = mbn_ragged_readout_view(r);
    nll_launch(s, r->batch, r->launch, a, table, nll, brier, plane_stride, logits, truth, truth_bytes, r->rows, r->cols, r->classes, inv_temps, temps);
    mbn_ragged_readout_mark_done(r, s);
    return MBN_OK;
}

// rect = null: the whole map, the window (0, 0, cols, rows) of a rows x cols input. The shape is inside mbn_resample_topk_envelope and the pointers
// are non-null multiples of 4 (the caller has checked both). q = null: the logit form, no exponential
int mbn_launch_f32_resample_topk(mbn_context *, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows, int cols,
                                 int classes, int in_rows, int in_cols, const int32_t *rect, int out_rows, int out_cols, int k,
                                 const mbn_readout_prob *q)
{
    const int32_t full[4] = { 0, 0, cols, rows };
    if (!rect) { rect = full; in_rows = rows; in_cols = cols; }
    mbn_resample_launch_t l = { 0, 0, 0, 0, 0, 0 };
    mbn_resample_window_plan(rows, cols, in_rows, in_cols, rect, out_rows, out_cols, &l);
    TopkArgs a = {};
    a.out_rows = out_rows; a.out_cols = out_cols;
    a.tiles_x = (out_cols + RS_TILE - 1) / RS_TILE;
    a.in_rows = in_rows; a.in_cols = in_cols;
    a.wx = rect[0]; a.wy = rect[1]; a.wiw = rect[2]; a.wih = rect[3];
    topk_launch(s, batch, l, a, logits, rows, cols, classes, k, (int64_t)batch * out_rows * out_cols, labels, score, q);
    return MBN_OK;
}

// the handle has a batch, the pointers are non-null multiples of 4, plane_stride covers the set's span and the spans fit (the caller has checked)
int mbn_launch_f32_resample_topk_ragged(mbn_ragged_readout *r, hipStream_t s, int32_t *labels, float *score, const float *logits, int k,
                                        int64_t plane_stride, const mbn_readout_prob *q)
{
    TopkArgs a = {};
    a.tiles_x = 1;                                              // unused: a workgroup takes its image's own
    // a plain set's items are the full window of a rows x cols input (what its check planned them as)
    a.in_rows = r->window ? r->in_rows : r->rows; a.in_cols = r->window ? r->in_cols : r->cols;
    a.wx = 0; a.wy = 0; a.wiw = a.in_cols; a.wih = a.in_rows;
    a.head = (const mbn_label_set_head *)r->dev;
    a.generation = r->generation;
    a.item_bytes = mbn_ragged_readout_item_bytes(r);
    topk_launch(s, r->batch, r->launch, a, logits, r->rows, r->cols, r->classes, k, plane_stride, labels, score, q);
    mbn_ragged_readout_mark_done(r, s);
    return MBN_OK;
}

// The plan is inside mbn_resample_slide_envelope and the pointers are non-null multiples of 4 (the caller has checked both)
int mbn_launch_f32_resample_slide(mbn_context *, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows, int cols,
                                  int classes, const mbn_slide *plan, int out_rows, int out_cols, const mbn_readout_prob *q)
{
    mbn_resample_launch_t l;
    const int rc = mbn_resample_slide_plan(rows, cols, plan, out_rows, out_cols, &l);
    if (rc != MBN_OK) return rc;
    SlideArgs a = {};
    a.labels = labels; a.score = score; a.logits = logits;
    a.rows = rows; a.cols = cols; a.classes = classes;
    a.out_rows = out_rows; a.out_cols = out_cols;
    a.fy = l.fy; a.fx = l.fx; a.ch = l.ch;
    if (q) { a.prob = q->prob; a.min_prob = q->min_prob; a.ignore_label = q->ignore_label; }
    for (int k = 1; k < 10; k++) a.inv[k] = 1.0f / (float)k;
    a.s = *plan;
    int32_t kmax;
    a.cells_y = mbn_slide_cells(plan->y, plan->ny, plan->tile_rows, a.edge_y, a.pieces_y, &kmax);
    a.cells_x = mbn_slide_cells(plan->x, plan->nx, plan->tile_cols, a.edge_x, a.pieces_x, &kmax);
    const bool vec = ((uintptr_t)logits % 16) == 0 && (classes % 4) == 0;
    hipLaunchKernelGGL(slide_kernels[q != nullptr][vec], dim3((unsigned)l.tiles, (unsigned)batch), dim3(256), (size_t)l.lds_bytes, s, a);
    return MBN_OK;
}

// The views are inside mbn_resample_ensemble_envelope and the pointers are non-null multiples of 4 (the caller has checked both)
int mbn_launch_f32_resample_ensemble(mbn_context *, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows, int cols,
                                     int classes, int in_rows, int in_cols, const mbn_view *views, int n_views, int out_rows, int out_cols,
                                     const mbn_readout_prob *q)
{
    mbn_resample_launch_t l;
    const int rc = mbn_resample_ensemble_plan(rows, cols, in_rows, in_cols, views, n_views, out_rows, out_cols, &l);
    if (rc != MBN_OK) return rc;
    EnsembleArgs a = {};
    a.labels = labels; a.score = score; a.logits = logits;
    a.rows = rows; a.cols = cols; a.classes = classes; a.batch = batch;
    a.out_rows = out_rows; a.out_cols = out_cols;
    a.tiles_x = (out_cols + RS_TILE - 1) / RS_TILE;
    a.fy = l.fy; a.fx = l.fx; a.ch = l.ch;
    a.in_rows = in_rows; a.in_cols = in_cols;
    a.inv_k = 1.0f / (float)n_views;
    if (q) { a.prob = q->prob; a.min_prob = q->min_prob; a.ignore_label = q->ignore_label; }
    for (int k = 0; k < n_views; k++) a.views[k] = views[k];
    const bool vec = ((uintptr_t)logits % 16) == 0 && (classes % 4) == 0;
    hipLaunchKernelGGL(ens_kernels[n_views - 1][q != nullptr][vec], dim3((unsigned)l.tiles, (unsigned)batch), dim3(256), (size_t)l.lds_bytes, s, a);
    return MBN_OK;
}

// rect = (x, y, iw, ih) of the in_rows x in_cols network input: the window kernels; null: the whole map, the plain kernels (in_rows, in_cols are not
// read). The shape is inside mbn_resample_window_envelope, without a rect mbn_resample_argmax_envelope, and the pointers are non-null multiples of 4
// (the caller has checked both).
int mbn_launch_f32_resample_argmax(mbn_context *, hipStream_t s, int32_t *labels, float *score, const float *logits, int batch, int rows, int cols,
                                   int classes, int in_rows, int in_cols, const int32_t *rect, int out_rows, int out_cols, const mbn_readout_prob *q)
{
    mbn_resample_launch_t l = { 0, 0, 0, 0, 0, 0 };
    if (rect) mbn_resample_window_plan(rows, cols, in_rows, in_cols, rect, out_rows, out_cols, &l);
    else mbn_resample_plan(rows, cols, out_rows, out_cols, &l);
    ResampleArgs a = rs_args(labels, score, logits, rows, cols, classes, l, in_rows, in_cols, q);
    a.out_rows = out_rows; a.out_cols = out_cols;
    a.tiles_x = (out_cols + RS_TILE - 1) / RS_TILE;
    if (rect) { a.wx = rect[0]; a.wy = rect[1]; a.wiw = rect[2]; a.wih = rect[3]; }
    rs_launch(false, q != nullptr, rect != nullptr, batch, l, s, a);
    return MBN_OK;
}

int mbn_ragged_readout_build(mbn_context *ctx, int max_batch, mbn_ragged_readout **out)
{
    mbn_ragged_readout *r = new (std::nothrow) mbn_ragged_readout();
    if (!r) return MBN_ENOMEM;
    r->ctx = ctx;
    r->max_batch = max_batch;
    const size_t bytes = sizeof(mbn_label_set_head) + sizeof(mbn_label_window_item) * (size_t)max_batch;     // the larger kind of item
    r->sort = new (std::nothrow) int64_t[2 * (size_t)max_batch];
    (void)hipSetDevice(ctx->device);
    hipError_t e = r->sort ? hipMalloc(&r->dev, bytes) : hipErrorOutOfMemory;
    if (e == hipSuccess) e = hipHostMalloc(&r->host, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        mbn_ragged_readout_release(r);
        return e == hipErrorOutOfMemory ? MBN_ENOMEM : mbn_record_hip_error(ctx, e, "ragged read-out buffers");
    }
    *out = r;
    return MBN_OK;
}

void mbn_ragged_readout_release(mbn_ragged_readout *r)
{
    if (r->done) (void)hipEventDestroy(r->done);
    if (r->host) (void)hipHostFree(r->host);
    if (r->dev) (void)hipFree(r->dev);
    delete[] r->sort;
    delete r;
}

// Checks the batch first and touches nothing when it is refused: the previous set stays. Then the batch becomes the handle's set: waits for what
// still reads either copy (the previous upload and every launch since), writes the items into the pinned copy and enqueues its upload.
// window: the items are mbn_label_window_item, each with its own rectangle of the in_rows x in_cols network input; else mbn_label_item.
int mbn_ragged_readout_plan(mbn_ragged_readout *r, hipStream_t s, int rows, int cols, int classes, int window, int in_rows, int in_cols,
                            const void *items, int batch)
{
    mbn_context *ctx = r->ctx;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return MBN_EINVAL;      // a set is not part of a graph
    mbn_resample_launch_t l = { 0, 0, 0, 0, 0, 0 };
    const int rc = window ? mbn_resample_ragged_window_check(rows, cols, classes, in_rows, in_cols, (const mbn_label_window_item *)items, batch, r->sort, &l)
                          : mbn_resample_ragged_check(rows, cols, classes, (const mbn_label_item *)items, batch, r->sort, &l);
    if (rc != MBN_OK) return rc;
    const size_t item_bytes = window ? sizeof(mbn_label_window_item) : sizeof(mbn_label_item);
    MBN_HIP_TRY(ctx, hipEventSynchronize(r->done));
    mbn_label_set_head *h = (mbn_label_set_head *)r->host;
    memset(h, 0, sizeof *h);
    h->batch = batch; h->generation = r->generation + 1;
    memcpy(h + 1, items, (size_t)batch * item_bytes);
    r->batch = 0;                                               // from here on a failure leaves the handle without a batch
    MBN_HIP_TRY(ctx, hipMemcpyAsync(r->dev, r->host, sizeof(mbn_label_set_head) + (size_t)batch * item_bytes, hipMemcpyHostToDevice, s));
    MBN_HIP_TRY(ctx, hipEventRecord(r->done, s));
    r->generation = h->generation;
    r->rows = rows; r->cols = cols; r->classes = classes;
    r->window = window; r->in_rows = in_rows; r->in_cols = in_cols;
    r->launch = l;
    r->batch = batch;
    return MBN_OK;
}

// the handle has a batch, the pointers are non-null multiples of 4 and the spans fit (the caller has checked)
int mbn_launch_f32_resample_argmax_ragged(mbn_ragged_readout *r, hipStream_t s, int32_t *labels, float *score, const float *logits,
                                          const mbn_readout_prob *q)
{
    ResampleArgs a = rs_args(labels, score, logits, r->rows, r->cols, r->classes, r->launch, r->in_rows, r->in_cols, q);
    a.tiles_x = 1;                                              // unused: a workgroup takes its image's own
    a.head = (const mbn_label_set_head *)r->dev;
    a.items = (const mbn_label_item *)(a.head + 1);
    a.witems = (const mbn_label_window_item *)(a.head + 1);     // the last set decides which of the two the block holds
    a.generation = r->generation;
    rs_launch(true, q != nullptr, r->window != 0, r->batch, r->launch, s, a);
    mbn_ragged_readout_mark_done(r, s);
    return MBN_OK;
}
