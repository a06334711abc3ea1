// mbn_f32_groups.hip — the dense head's read-out by CLASS GROUPS on gfx950: bilinear resample of the per-pixel logits to any output size, the
// softmax over the kept classes, the sum of the probabilities of every group's members and the argmax over the GROUPS, in one kernel
// (mbn_resample_groups_f32; include/mbn.h, "segment by class groups", is the normative statement of the arithmetic). 1000 fine classes become the
// handful of labels the scoring stages are built for, and neither [out_rows][out_cols][classes] nor a per-group plane is ever in memory.
//
// The tile is mbn_readout_tile.h's: 256 lanes own a 32 x 32 output tile, a lane one column and four rows, the fy x fx footprint staged per chunk
// (mbn_resample_window_plan: one envelope, one plan), rs_lane / rs_interp / rs_exp unchanged, so every interpolant has the bits the argmax and
// softmax kernels of mbn_f32_resample.hip give it. What is this file's own:
//   layout  the host orders the kept classes by group (mbn_class_groups_layout): SLOTS, each group padded to a multiple of four with slot_class =
//           -1, and quad_group[q] = g when the four slots of quad q are the last of group g, else -1. Both tables live on the device, uploaded once
//           per grouping (mbn_class_groups_create)
//   stage   a chunk is ch slots. Slot s of vector (ry, rx) is logits[(ry * cols + rx) * classes + slot_class[s]], a pad slot a NaN, which the tile
//           defines as "never the maximum, adds exp(-200) = 0". It is a GATHER: consecutive slots of a group are ascending classes but not
//           consecutive ones (c % 21 puts them 21 floats apart), so four slots are not 16 contiguous bytes and a 16-byte path does not exist
//           here whatever the alignment of `logits`: dword loads only. Across a wave the loads of one vector still fall into the few cache lines
//           of that vector's classes, and every line is used in full over the chunks of a tile
//   reduce  per quad of four slots the lane forms its four rows' interpolants (rs_interp), moves each row's lazy reference by the RS_MARGIN rule
//           (a move rescales the row's THREE sums by the same factor, so every compare stays under one reference) and adds the four rs_exp terms
//           to the OPEN group's sum. Then quad_group of the quad is read: the index is the same in every lane, so it is one scalar load and the
//           close-of-group branch is taken by a whole wave or by none. Closing group g: tot += gsum; if (gsum > bsum) { bsum = gsum; blabel = g }
//           (strict: ties go to the lowest group, the groups come in ascending order); gsum = 0. A group may straddle any number of chunks:
//           its sum is register state across the chunk loop
//   store   prob = bsum / tot, score = ref + ln(bsum) (the winning group's log-sum-exp), the label replaced by ignore_label iff the stored
//           prob < min_prob. A pixel whose largest kept interpolant is not finite stores prob 0, the lowest non-empty group and that interpolant
// Per slot the loop is the softmax kernel's less the argmax compare; per quad it adds one scalar load and a uniform branch.
#include "mbn_internal.h"
#include "mbn_device.h"
#include "mbn_readout_tile.h"

#include <new>

namespace {

struct GroupsArgs {
    int *labels;
    float *score, *prob;     // either may be null
    const float *logits;
    const int *slot_class;   // [slots]: the class of a slot, -1 for a pad slot
    const int *quad_group;   // [slots / 4]: the group that ends with the quad, else -1
    int slots, first_group;  // a multiple of 4; the lowest non-empty group
    int rows, cols, classes; // the coarse map
    int out_rows, out_cols, tiles_x;
    int fy, fx, ch;          // the launch's LDS footprint in vectors and the slot chunk (mbn_resample_window_plan)
    int in_rows, in_cols;    // WIN: the network-input pixels the coarse map covers, and the window
    int wx, wy, wiw, wih;
    float min_prob;
    int ignore_label;
};

// a lane's four rows: the lazy reference, the open group's sum, the closed groups' sum, the best closed group and the largest interpolant seen
struct GroupsRows {
    float ref[RS_ROWS], gsum[RS_ROWS], tot[RS_ROWS], bsum[RS_ROWS], vmax[RS_ROWS];
    int blabel[RS_ROWS];
};

// The reduce pass of one staged chunk of sn slots (a multiple of 4) that starts at quad q0 of the layout
template <bool CROSS>
__device__ __forceinline__ void gr_reduce(const float *s_x, const RsLane &n, int sn, int q0, const int *__restrict__ quad_group, GroupsRows &st)
{
    for (int c = 0; c < sn; c += 4) {
        float vv[RS_ROWS][4];
        rs_interp<CROSS>(s_x, n.off, c, n.wx0, n.wx1, n.wy0, n.wy1, n.up, [&](int r, int k, float v) __attribute__((always_inline)) { vv[r][k] = v; });
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                // the RS_MARGIN rule of rs_softmax_group, for three sums: the maxima drop NaNs, an all-NaN m and -inf - -inf fail the compare
                const float m = __builtin_fmaxf(__builtin_fmaxf(vv[r][0], vv[r][1]), __builtin_fmaxf(vv[r][2], vv[r][3]));
                st.vmax[r] = __builtin_fmaxf(st.vmax[r], m);
                if (m - st.ref[r] > RS_MARGIN) {
                    const float f = rs_exp(st.ref[r] - m);
                    st.gsum[r] *= f; st.tot[r] *= f; st.bsum[r] *= f;
                    st.ref[r] = m;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) st.gsum[r] += rs_exp(__builtin_fmaxf(vv[r][k] - st.ref[r], -200.0f));     // a NaN difference adds 0
            }
        }
        const int g = quad_group[q0 + (c >> 2)];                // the same address in every lane: a scalar load, a wave-uniform branch
        if (g >= 0) {
#pragma clang fp contract(off)
#pragma unroll
            for (int r = 0; r < RS_ROWS; r++) {
                st.tot[r] += st.gsum[r];
                if (st.gsum[r] > st.bsum[r]) { st.bsum[r] = st.gsum[r]; st.blabel[r] = g; }
                st.gsum[r] = 0.0f;
            }
        }
    }
}

template <bool WIN>
__global__ __launch_bounds__(256) void resample_groups_f32(const GroupsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float s_x[];
    const int tid = threadIdx.x;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const size_t img = (size_t)blockIdx.y;                                                      // 64-bit base, 32-bit offsets inside an image
    const size_t map = (size_t)a.out_rows * a.out_cols;
    const float *__restrict__ src = a.logits + img * ((size_t)a.rows * a.cols * a.classes);
    const int H = a.out_rows, W = a.out_cols;
    const int ld = a.ch + 4, nv = a.fy * a.fx;
    const int last_y = a.rows - 1, last_x = a.cols - 1;
    const RsWindow wy = { a.in_rows, a.wy, a.wih }, wx = { a.in_cols, a.wx, a.wiw };          // read by the WIN instantiation only
    RsLane n;
    rs_lane<WIN>(n, a.rows, a.cols, a.fy, a.fx, ld, H, W, ty, tx, wy, wx);

    GroupsRows st;
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
        st.ref[r] = st.vmax[r] = -__builtin_inff();
        st.gsum[r] = st.tot[r] = st.bsum[r] = 0.0f;
        st.blabel[r] = a.first_group;
    }

    const float nan = __builtin_nanf("");
    for (int s0 = 0; s0 < a.slots; s0 += a.ch) {
        const int sn = min(a.ch, a.slots - s0);                 // slots and ch are multiples of 4
        // ---- stage by gather: nv vectors x sn slots, dword loads
        for (int e = tid; e < nv * sn; e += 256) {
            const int v = e / sn, s = e - v * sn;
            const int ry = min(n.ybase + v / a.fx, last_y), rx = min(n.xbase + v % a.fx, last_x);
            const int cls = a.slot_class[s0 + s];
            s_x[v * ld + s] = cls >= 0 ? src[(unsigned)((ry * a.cols + rx) * a.classes + cls)] : nan;
        }
        __syncthreads();
        // ---- reduce
        if (n.active) {
            if (n.cross) gr_reduce<true>(s_x, n, sn, s0 >> 2, a.quad_group, st);
            else gr_reduce<false>(s_x, n, sn, s0 >> 2, a.quad_group, st);
        }
        __syncthreads();
    }
    if (!n.active) return;

    int *__restrict__ labels = a.labels + img * map;
    float *__restrict__ score = a.score ? a.score + img * map : nullptr, *__restrict__ prob = a.prob ? a.prob + img * map : nullptr;
    const unsigned out = (unsigned)(n.oy0 * W + n.ox);          // 32-bit inside an image: its map is below 2^31 bytes
#pragma unroll
    for (int r = 0; r < RS_ROWS; r++) {
#pragma clang fp contract(off)
        if (n.oy0 + r >= H) break;
        // a finite vmax: ref is finite, its own term exp(0) = 1 is in tot, and the best group holds at least tot / groups: 0 < pr <= 1
        const bool finite = __builtin_fabsf(st.vmax[r]) < __builtin_inff();
        const float pr = finite ? st.bsum[r] / st.tot[r] : 0.0f;
        const float sc = finite ? st.ref[r] + __builtin_amdgcn_logf(st.bsum[r]) * 0.693147180559945309f : st.vmax[r];
        int label = finite ? st.blabel[r] : a.first_group;
        if (pr < a.min_prob) label = a.ignore_label;            // strict, on the value stored below
        if (prob) prob[out + (unsigned)(r * W)] = pr;
        labels[out + (unsigned)(r * W)] = label;
        if (score) score[out + (unsigned)(r * W)] = sc;
    }
}

}   // namespace

// group_of is inside mbn_class_groups_layout's rules (the caller has checked it): the tables are built on the host and uploaded once
int mbn_class_groups_build(mbn_context *ctx, int classes, int groups, const int32_t *group_of, mbn_class_groups **out)
{
    mbn_class_groups *g = new (std::nothrow) mbn_class_groups();
    const size_t cap = (size_t)classes + 3 * (size_t)groups;                                    // slots <= classes + 3 * groups
    int32_t *host = new (std::nothrow) int32_t[cap + cap / 4 + 1];
    if (!g || !host) { delete g; delete[] host; return MBN_ENOMEM; }
    g->ctx = ctx; g->classes = classes; g->groups = groups;
    int rc = mbn_class_groups_layout(classes, groups, group_of, host, host + cap, &g->slots);
    if (rc == MBN_OK) {
        for (int q = 0; q < g->slots / 4; q++) host[g->slots + q] = host[cap + q];             // quad_group right behind slot_class
        g->first_group = group_of[host[0]];
        (void)hipSetDevice(ctx->device);
        const size_t bytes = sizeof(int32_t) * (size_t)(g->slots + g->slots / 4);
        hipError_t e = hipMalloc(&g->dev, bytes);
        if (e == hipSuccess) e = hipMemcpy(g->dev, host, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = e == hipErrorOutOfMemory ? MBN_ENOMEM : mbn_record_hip_error(ctx, e, "class groups tables");
    }
    delete[] host;
    if (rc != MBN_OK) { mbn_class_groups_release(g); return rc; }
    *out = g;
    return MBN_OK;
}

void mbn_class_groups_release(mbn_class_groups *g)
{
    if (g->dev) (void)hipFree(g->dev);
    delete g;
}

// the arguments are inside mbn_resample_groups_envelope and the pointers checked (the caller has done both); rect = null: the whole map
int mbn_launch_f32_resample_groups(mbn_context *, hipStream_t s, const mbn_class_groups *g, int32_t *labels, float *prob, float *score,
                                   const float *logits, int batch, int rows, int cols, int in_rows, int in_cols, const int32_t *rect, int out_rows,
                                   int out_cols, float min_prob, int ignore_label)
{
    mbn_resample_launch_t l = { 0, 0, 0, 0, 0, 0 };
    if (rect) mbn_resample_window_plan(rows, cols, in_rows, in_cols, rect, out_rows, out_cols, &l);
    else mbn_resample_plan(rows, cols, out_rows, out_cols, &l);
    GroupsArgs a = {};
    const mbn_readout_prob q = { prob, min_prob, ignore_label };
    rs_fill(a, labels, score, logits, rows, cols, g->classes, l, &q);
    rs_fill_uniform(a, out_rows, out_cols, in_rows, in_cols, rect);
    a.slot_class = (const int *)g->dev; a.quad_group = a.slot_class + g->slots;
    a.slots = g->slots; a.first_group = g->first_group;
    hipLaunchKernelGGL(rect ? resample_groups_f32<true> : resample_groups_f32<false>, dim3((unsigned)l.tiles, (unsigned)batch), dim3(256),
                       (size_t)l.lds_bytes, s, a);
    return MBN_OK;
}
