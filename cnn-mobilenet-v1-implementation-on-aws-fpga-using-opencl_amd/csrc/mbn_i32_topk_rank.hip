// mbn_i32_topk_rank.hip — "is the truth among the k best" on the device (gfx950): per truth class the rank at which the ground truth appears among the
// k rank-major label planes mbn_resample_topk_f32 writes, accumulated into uint64 ranks [classes + 1][k + 1] (mbn_topk_rank_i32 and its ragged form;
// include/mbn.h, "rank score"). The dense counterpart of top-5 accuracy. The arithmetic is integer: every pixel adds exactly 1 to
// exactly one cell, so the result is the same whatever order the atomics arrive in, at every planning CU count and in both forms below.
//
// The structure is mbn_i32_confusion.hip's. A SPAN is n consecutive pixels: the whole call (uniform form) or one item of a ragged set; a CHUNK is
// 1024 consecutive pixels of a span, one per lane of a workgroup. A lane loads its truth and then the label planes in rank order until one equals
// the truth (a wave stops when all its lanes have: on real maps most after plane 0), so every load of a wave is one coalesced run of dwords or
// bytes; no alignment beyond the elements' own is assumed. The row is the truth by mbn_confusion_i32's rule (outside [0, classes): the void row
// `classes`); the column is the smallest j with labels[j] == truth, else k: every void pixel, and every pixel whose truth is in no plane. A label
// outside [0, classes) never equals the truth of a valid row, so ignore_label and -1 match nothing without a compare of their own.
//
// The grid is persistent: num_cus * 2 workgroups, workgroup b takes the chunks c with (c + rot) % grid == b, rot = the chunks of the items before.
// Two forms (mbn_topk_rank_form, host/mbn_score.c):
//   LDS     a workgroup counts into a private table of (classes + 1) * (k + 1) 32-bit bins in LDS and adds its non-zero bins to `ranks` with 64-bit
//           global atomics: after every TR_EPOCH chunks (so a bin never holds 2^32) and at the end
//   global  64-bit global atomics on `ranks` directly
// Wave aggregation, both forms: truth maps are piecewise constant and most pixels hit at rank 0, so most lanes of a wave hold the same cell. A
// leader per distinct cell (readfirstlane + ballot) adds the popcount once; the lanes left over after TR_LEADERS rounds add on their own.
#include "mbn_internal.h"
#include "mbn_label_set.h"

namespace {

constexpr int TR_THREADS = 1024;          // lanes of a workgroup = pixels of a chunk
constexpr int TR_EPOCH = 1 << 20;         // chunks between two flushes of the LDS table: 2^20 * 1024 pixels < 2^32
constexpr int TR_LEADERS = 8;             // distinct cells a wave aggregates per chunk

struct RankArgs {
    unsigned long long *ranks;
    const int32_t *labels;     // plane 0
    const uint8_t *truth;      // element 0 of the truth, uint8 or int32
    int classes, k;
    long long plane;           // elements from plane j to plane j + 1
    long long count;           // uniform form: the span
    mbn_label_set set;         // ragged form: the view of the handle's set
};

template <bool LDS>
__device__ __forceinline__ void tr_add(const RankArgs &a, unsigned *s_bins, int cell, unsigned w)
{
    if (LDS) (void)__hip_atomic_fetch_add(&s_bins[cell], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else (void)__hip_atomic_fetch_add(&a.ranks[cell], (unsigned long long)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void tr_flush(const RankArgs &a, unsigned *s_bins, int bins)
{
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += TR_THREADS) {
        const unsigned v = s_bins[i];
        if (v) {
            (void)__hip_atomic_fetch_add(&a.ranks[i], (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_bins[i] = 0;
        }
    }
    __syncthreads();
}

template <int TB, bool LDS, bool RAGGED>
__global__ __launch_bounds__(TR_THREADS) void topk_rank_i32(const RankArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned s_bins[];
    const int classes = a.classes, k = a.k, bins = (classes + 1) * (k + 1);
    int batch = 1;
    if (RAGGED) {
        if (mbn_label_set_stale(a.set)) return;                                // captured under an earlier set: nothing to score
        batch = a.set.head->batch;
    }
    if (LDS) {
        for (int i = threadIdx.x; i < bins; i += TR_THREADS) s_bins[i] = 0;
        __syncthreads();
    }
    const unsigned G = gridDim.x, b = blockIdx.x;
    unsigned rot = 0;
    int epoch = 0;
    for (int i = 0; i < batch; i++) {
        long long off = 0, n = a.count;
        if (RAGGED) {
            const mbn_label_item *it = mbn_label_set_item(a.set, i);
            off = it->dst_offset;
            n = (long long)it->rows * it->cols;
        }
        const int32_t *lab = a.labels + off;
        const uint8_t *tr = a.truth + off * TB;
        const long long chunks = (n + TR_THREADS - 1) / TR_THREADS;
        for (long long c = (b + G - rot) % G; c < chunks; c += G) {
            const long long e = c * TR_THREADS + threadIdx.x;
            if (e < n) {
                const int t = TB == 1 ? (int)tr[e] : ((const int32_t *)tr)[e];
                const bool valid = (unsigned)t < (unsigned)classes;
                int col = k;
                if (valid) {
                    for (int j = 0; j < k; j++)
                        if (lab[(long long)j * a.plane + e] == t) { col = j; break; }
                }
                const int cell = (valid ? t : classes) * (k + 1) + col;
                // one add per distinct cell of the wave's active lanes, by the first lane that holds it
                bool done = false;
                for (int it = 0; it < TR_LEADERS && !done; it++) {
                    const int lead = __builtin_amdgcn_readfirstlane(cell);
                    if (cell == lead) {
                        const unsigned long long m = __ballot(1);
                        if ((int)(__lane_id()) == __ffsll((long long)m) - 1) tr_add<LDS>(a, s_bins, lead, (unsigned)__popcll(m));
                        done = true;
                    }
                }
                if (!done) tr_add<LDS>(a, s_bins, cell, 1u);
            }
            if (LDS && ++epoch == TR_EPOCH) {
                tr_flush(a, s_bins, bins);
                epoch = 0;
            }
        }
        rot = (unsigned)((rot + chunks % G) % G);
    }
    if (LDS) tr_flush(a, s_bins, bins);
}

// the eight kernels by [ragged][form][int32 truth]
using Kernel = void (*)(const RankArgs);
const Kernel tr_kernels[2][2][2] = {
    { { topk_rank_i32<1, true, false>, topk_rank_i32<4, true, false> }, { topk_rank_i32<1, false, false>, topk_rank_i32<4, false, false> } },
    { { topk_rank_i32<1, true, true>, topk_rank_i32<4, true, true> }, { topk_rank_i32<1, false, true>, topk_rank_i32<4, false, true> } },
};

// The persistent grid: two workgroups (32 waves) on a CU; the LDS table is at most MBN_TOPK_RANK_LDS = 48 KB, inside what a launch gets without
// asking. Never more workgroups than there are chunks (+ one per item)
void tr_launch(mbn_context *ctx, hipStream_t s, bool ragged, const RankArgs &a, int truth_bytes, long long pixels, int items)
{
    const int form = mbn_topk_rank_form(a.classes, a.k);
    const int lds_bytes = form == MBN_CONFUSION_FORM_LDS ? (a.classes + 1) * (a.k + 1) * 4 : 0;
    const unsigned grid = mbn_persistent_grid(ctx->num_cus, 2, pixels / TR_THREADS + items);
    hipLaunchKernelGGL(tr_kernels[ragged][form][truth_bytes == 4], dim3(grid), dim3(TR_THREADS), (size_t)lds_bytes, s, a);
}

RankArgs tr_args(void *ranks, const void *labels, int k, int64_t plane_stride, const void *truth, int classes)
{
    RankArgs a = {};
    a.ranks = (unsigned long long *)ranks;
    a.labels = (const int32_t *)labels;
    a.truth = (const uint8_t *)truth;
    a.classes = classes; a.k = k;
    a.plane = plane_stride;
    return a;
}

}   // namespace

// the arguments are inside mbn_topk_rank_envelope and the pointers are checked (the caller)
int mbn_launch_i32_topk_rank(mbn_context *ctx, hipStream_t s, void *ranks, const void *labels, int k, int64_t plane_stride, const void *truth,
                             int truth_bytes, int classes, int64_t count)
{
    RankArgs a = tr_args(ranks, labels, k, plane_stride, truth, classes);
    a.count = count;
    tr_launch(ctx, s, false, a, truth_bytes, count, 1);
    return MBN_OK;
}

// the handle has a batch; the spans of the label planes and of the truth reach r->launch.span elements (the caller has checked them)
int mbn_launch_i32_topk_rank_ragged(mbn_ragged_readout *r, hipStream_t s, void *ranks, const void *labels, int k, int64_t plane_stride,
                                    const void *truth, int truth_bytes, int classes)
{
    RankArgs a = tr_args(ranks, labels, k, plane_stride, truth, classes);
    a.set = mbn_ragged_readout_view(r);
    tr_launch(r->ctx, s, true, a, truth_bytes, r->launch.span, r->batch);
    mbn_ragged_readout_mark_done(r, s);
    return MBN_OK;
}
