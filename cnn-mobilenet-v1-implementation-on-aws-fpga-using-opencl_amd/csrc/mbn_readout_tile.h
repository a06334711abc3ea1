// mbn_readout_tile.h — the tile every read-out kernel of the dense head runs on (mbn_f32_resample.hip: argmax, softmax, ragged, window, ensemble,
// slide, top-k, NLL; mbn_f32_guided.hip), each part written once: the constants, the index / weight rule, the lane state per axis, the stage pass,
// the interpolation of one group of four classes, the softmax sum and the store. include/mbn.h, "dense head at the source resolution", is the
// normative statement of the arithmetic; a family adds its own state and its own use of every interpolant, nothing of what stands here.
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
// WIN: the outputs resample a rectangle of the network's input, the letterbox's inner image, instead of the whole map. Only the index / weight rule
// differs (rs_axis_win: 64-bit integers, still one fp64 division per axis coordinate, once per lane in front of the class loop); the footprint bound
// holds with n / N replaced by l n / (N R) (host/mbn_envelope.h), so everything else here is the same code. The window rule's 64-bit divisions cost
// 0.6-0.7 % at equal footprint (profiles/LOG.md, "Through the letterbox"), so WIN stays a compile-time parameter.
// PROB (include/mbn.h, "segment with confidence"): the softmax denominator of each of the lane's four pixels, prob = 1 / sum_c exp(v_c - best) beside
// the label; labels and scores are the argmax instantiations' bit for bit (the same v, the same compare). The sum is ONE pass with a LAZY reference:
// per row a reference `ref` and sum = sum_c exp(v_c - ref). Per four classes the row's maximum m of the four is compared with ref: more than
// RS_MARGIN = 16 above it, m becomes the reference and the old sum is rescaled by exp(ref - m) < e^-16; then the four add exp(v - ref). So every v
// seen is at most 16 above ref, best - ref stays in [0, 16], ref is itself a v seen (its term is exp(0) = 1: sum >= 1), and a part of the sum that
// went through k rescales weighs below classes * e^(-16 (k - 1)) of it: only the first rescale of a part counts, and an ascending ramp costs one
// rescale per 16 units of logit instead of one per class. That is what keeps the error bound of include/mbn.h for every input. The alternative, a
// second pass with the final best, stages every chunk and forms every interpolant twice: about 10 plain VALU per pixel and class on top of the same
// exp, against about 7 issue slots here (subtract, max, multiply, add, v_exp_f32 at two slots, and a quarter of the group's three maxima, subtract
// and compare). prob = exp(best - ref) / sum at the end, 0 when best is not finite. A NaN v (the padding classes of the dword path among them) is
// dropped by the maxima, and its difference is replaced by -200 by a max that drops the NaN: it adds exp(-200) = 0, exactly.
#pragma once

#include "mbn_internal.h"
#include "mbn_device.h"

constexpr int RS_TILE = MBN_RESAMPLE_TILE;   // output tile side of a workgroup
constexpr int RS_ROWS = 4;                   // output rows of a lane
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

// One coordinate of either rule. It is also a lane's COLUMN state: x0 and wx1 of the column handed in (clamped to the image, mirrored, or taken
// inside a slide tile by the caller), and the tile's ybase / xbase from its first output
template <bool WIN>
__device__ __forceinline__ void rs_coord(int o, int n, int N, const RsWindow &w, int *i0, float *w1)
{
    if (WIN) rs_axis_win(o, n, N, w, i0, w1);
    else rs_axis(o, n, N, i0, w1);
}

// A lane's ROW state: its four rows from oy0 on, a row past y_last evaluated there (and not stored). ya = row 0's i0, wy1 the rows' weights of i1,
// up[r]: row r interpolates between (ya + 1, ya + 2) instead of (ya, ya + 1). Returns whether some row of the WAVE does (every lane calls this): at
// ratio r about 3 / r of a wave's two row groups cross a coarse row
template <bool WIN>
__device__ __forceinline__ bool rs_rows(int oy0, int y_last, int n, int N, const RsWindow &w, int *ya, float (&wy1)[RS_ROWS], bool (&up)[RS_ROWS])
{
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        int r0;
        rs_coord<WIN>(min(oy0 + r, y_last), n, N, w, &r0, &wy1[r]);
        if (r == 0) *ya = r0;
        up[r] = r0 != *ya;                    // r0 is ya or ya + 1: four rows span less than one coarse row
    }
    return __ballot(up[1] || up[2] || up[3]) != 0;
}

// The slot of coarse index i along an axis whose staged block starts at `base` and holds f: inside the block by construction; the clamps cost
// nothing and keep every read inside the launch's LDS whatever the arguments
__device__ __forceinline__ int rs_slot(int i, int base, int f) { return min(max(i - base, 0), f - 1); }

// The slots (vector indices inside the staged fy x fx block) of a lane's six vectors: rows ya, min(ya + 1, rows - 1), min(ya + 2, rows - 1) x columns
// x0, min(x0 + 1, cols - 1). Slots, not addresses: a vector's floats are slot * ld words into the block, and the guided read-out finds its colours
// by the same slot
__device__ __forceinline__ void rs_slots(int ya, int x0, int ybase, int xbase, int last_y, int last_x, int fy, int fx, int (&slot)[3][2])
{
    const int sx0 = rs_slot(x0, xbase, fx), sx1 = rs_slot(min(x0 + 1, last_x), xbase, fx);
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int sy = rs_slot(min(ya + j, last_y), ybase, fy);
        slot[j][0] = sy * fx + sx0;
        slot[j][1] = sy * fx + sx1;
    }
}

// The state of a lane of tile (ty, tx) of an H x W image, for the kernels that read ONE map per pixel (the plain / window / ragged tile, NLL,
// guided): the three helpers above in a row. The slide runs them per tile row and tile column instead; the ensemble and the top-k keep this run
// in their own text (mbn_f32_resample.hip says why).
struct RsLane {
    int ybase, xbase;        // i0 of the tile's first output row / column: where its staged block starts
    int ox, oy0;             // the lane's column and first row (a coordinate past the image is evaluated at the last one and not stored)
    bool active, cross;      // the lane has a pixel; some row of its wave has an up bit
    float wx0, wx1, wy0[RS_ROWS], wy1[RS_ROWS];
    bool up[RS_ROWS];
    int slot[3][2], off[3][2];             // the six vectors' slots and their first words in the staged block, slot * ld
};

template <bool WIN>
__device__ __forceinline__ void rs_lane(RsLane &n, int rows, int cols, int fy, int fx, int ld, int H, int W, int ty, int tx, const RsWindow &wy,
                                        const RsWindow &wx)
{
    const int tid = threadIdx.x;
    float unused;
    rs_coord<WIN>(RS_TILE * ty, rows, H, wy, &n.ybase, &unused);
    rs_coord<WIN>(RS_TILE * tx, cols, W, wx, &n.xbase, &unused);
    n.ox = RS_TILE * tx + (tid & 31);
    n.oy0 = RS_TILE * ty + RS_ROWS * (tid >> 5);
    n.active = n.ox < W && n.oy0 < H;
    int x0, ya = 0;
    rs_coord<WIN>(min(n.ox, W - 1), cols, W, wx, &x0, &n.wx1);
    n.wx0 = 1.0f - n.wx1;
    n.cross = rs_rows<WIN>(n.oy0, H - 1, rows, H, wy, &ya, n.wy1, n.up);
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) n.wy0[r] = 1.0f - n.wy1[r];
    rs_slots(ya, x0, n.ybase, n.xbase, rows - 1, cols - 1, fy, fx, n.slot);
#pragma unroll
    for (int j = 0; j < 3; j++) { n.off[j][0] = n.slot[j][0] * ld; n.off[j][1] = n.slot[j][1] * ld; }
}

// exp(d) for the softmax sum: d <= RS_MARGIN, -inf gives 0. One multiply and v_exp_f32 (1 ulp; a result below 2^-126 may flush to 0, far below
// the bound against a sum of at least 1).
__device__ __forceinline__ float rs_exp(float d) { return __builtin_amdgcn_exp2f(d * 1.44269504088896341f); }

// The lazy-reference softmax sum (the file's head) of a lane's four rows over one group of four classes, vv[r][k] = row r's v of the group's class k
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

// The interpolants of a lane's four rows for the four classes at word c of the six staged vectors, whose first words are off[][] into s_x: six f4
// reads, the horizontal lerps first, then the vertical ones. CROSS: some row of the wave interpolates between (ya + 1, ya + 2), so the third
// horizontal interpolant and the per-row selects are needed; otherwise every row of the wave uses (t0, t1) and neither is formed. The same products
// and sums in the same order either way. Every v goes to use(r, k, v), class by class and row by row inside a class: what a family does with it (the
// argmax compare, the NLL's pick of the truth's v and its difference to best) stands there, inlined where this loop forms v
template <bool CROSS, typename Use>
__device__ __forceinline__ void rs_interp(const float *s_x, const int (&off)[3][2], int c, float wx0, float wx1, const float (&wy0)[RS_ROWS],
                                          const float (&wy1)[RS_ROWS], const bool (&up)[RS_ROWS], Use use)
{
    constexpr int NT = CROSS ? 3 : 2;
    f4 v0[NT], v1[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
        v0[j] = *reinterpret_cast<const f4 *>(s_x + off[j][0] + c);
        v1[j] = *reinterpret_cast<const f4 *>(s_x + off[j][1] + c);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        float t[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) t[j] = rs_lerp(v0[j][k], wx0, v1[j][k], wx1);              // horizontal first
#pragma unroll
        for (int r = 0; r < RS_ROWS; r++) {
            const float ta = CROSS && up[r] ? t[1] : t[0], tb = CROSS && up[r] ? t[NT - 1] : t[1];
            use(r, k, rs_lerp(ta, wy0[r], tb, wy1[r]));                                         // then vertical
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

// VEC on the host: `logits` on 16 bytes and classes % 4 == 0, so that every class vector starts on 16 bytes
inline bool rs_vec(const float *logits, int classes) { return ((uintptr_t)logits % 16) == 0 && (classes % 4) == 0; }

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

// What every launch fills alike, from the fields the argument structs name alike: the buffers, the coarse map, the launch's plan and q, the softmax
// read-out's extras (null for the argmax read-out); and a uniform launch's output size and rectangle of the in_rows x in_cols network input
template <typename Args>
inline void rs_fill(Args &a, int32_t *labels, float *score, const float *logits, int rows, int cols, int classes, const mbn_resample_launch_t &l,
                    const mbn_readout_prob *q)
{
    a.labels = labels; a.score = score; a.logits = logits;
    a.rows = rows; a.cols = cols; a.classes = classes;
    a.fy = l.fy; a.fx = l.fx; a.ch = l.ch;
    if (q) { a.prob = q->prob; a.min_prob = q->min_prob; a.ignore_label = q->ignore_label; }
}

template <typename Args>
inline void rs_fill_uniform(Args &a, int out_rows, int out_cols, int in_rows, int in_cols, const int32_t *rect)
{
    a.out_rows = out_rows; a.out_cols = out_cols;
    a.tiles_x = (out_cols + RS_TILE - 1) / RS_TILE;
    a.in_rows = in_rows; a.in_cols = in_cols;
    if (rect) { a.wx = rect[0]; a.wy = rect[1]; a.wiw = rect[2]; a.wih = rect[3]; }        // null: the plain rule, which reads no window
}
