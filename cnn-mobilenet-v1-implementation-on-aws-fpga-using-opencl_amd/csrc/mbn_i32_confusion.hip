// mbn_i32_confusion.hip — score a segmentation on the device (gfx950): the confusion matrix of int32 label maps against a uint8 or int32 ground
// truth, accumulated into uint64 counts [classes + 1][classes + 1] (mbn_confusion_i32 and its ragged form; include/mbn.h, "score a segmentation";
// DESIGN.md 7d.4). The arithmetic is integer: every pixel adds exactly 1 to exactly one cell, so the result is the same whatever order the atomics
// arrive in, at every planning CU count and in both forms below.
//
// A SPAN is n consecutive pixels: the whole call (uniform form) or one item of a ragged set. It is cut into a scalar head, a body of groups of four
// pixels and a scalar tail: the head brings `labels` onto 16 bytes, so a lane loads its group's labels as one 16-byte vector. The truth of the same
// group is, for int32 truth, one 16-byte load from a pointer that is only on 4 bytes, and for uint8 truth its four bytes as one dword: directly
// where they lie on 4 bytes, else from the two aligned dwords around them. The head and the tail are widened (to 7 pixels at most) until both of
// those dwords lie wholly inside the span, so nothing outside [0, n) of either array is read. A CHUNK is 1024 consecutive groups, one per lane
// of a workgroup; the head and the tail belong to chunk 0.
//
// The grid is persistent: num_cus * (workgroups per CU) workgroups, workgroup b takes the chunks k with (k + rot) % grid == b, rot = the chunks of
// the items before (so a ragged set of many small maps spreads over the grid as one long span would).
//
// Two forms (mbn_confusion_form, host/mbn_score.c):
//   LDS     a workgroup counts into a private table of (classes + 1)^2 32-bit bins in LDS (ds_add_u32) and adds its non-zero bins to `counts` with
//           64-bit global atomics: after every MBN_CONFUSION_EPOCH chunks (so a bin never holds 2^32: an epoch is 2^21 pixels) and at the end.
//   global  64-bit global atomics on `counts` directly.
// Wave aggregation, both forms: label maps are piecewise constant, so most lanes hold four equal (truth, label) pairs and most waves few distinct
// ones. The lanes whose four cells agree elect a leader per distinct cell (readfirstlane + ballot) and the leader adds 4 * popcount once: a constant
// map costs one atomic per wave and chunk (256 pixels), not 256. Lanes whose four cells differ add them one by one.
#include "mbn_internal.h"
#include "mbn_label_set.h"

namespace {

constexpr int CF_THREADS = 1024;          // lanes of a workgroup = groups of a chunk
constexpr int CF_EPOCH = 512;             // chunks between two flushes of the LDS table: 512 * 4096 pixels < 2^32
constexpr int CF_LEADERS = 16;            // distinct cells a wave aggregates per chunk; the lanes left over add on their own

struct __attribute__((packed, aligned(4))) I32x4 { int32_t x, y, z, w; };      // four int32 on 4 bytes: one global_load_dwordx4

struct ConfusionArgs {
    unsigned long long *counts;
    const int32_t *labels;
    const uint8_t *truth;      // element 0 of the truth, uint8 or int32
    int classes;
    long long count;           // uniform form: the span
    mbn_label_set set;         // ragged form: the view of the handle's set
};

template <bool LDS>
__device__ __forceinline__ void bin_add(const ConfusionArgs &a, unsigned *s_bins, int cell, unsigned w)
{
    if (LDS) (void)__hip_atomic_fetch_add(&s_bins[cell], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else (void)__hip_atomic_fetch_add(&a.counts[cell], (unsigned long long)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// row or column of a value: itself inside [0, classes), else the void row / abstained column `classes` (negative values included)
__device__ __forceinline__ int cf_clamp(int v, int classes) { return (unsigned)v < (unsigned)classes ? v : classes; }
__device__ __forceinline__ int cf_cell(int t, int p, int classes) { return cf_clamp(t, classes) * (classes + 1) + cf_clamp(p, classes); }

template <bool LDS>
__device__ __forceinline__ void flush_bins(const ConfusionArgs &a, unsigned *s_bins, int bins)
{
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += CF_THREADS) {
        const unsigned v = s_bins[i];
        if (v) {
            (void)__hip_atomic_fetch_add(&a.counts[i], (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            s_bins[i] = 0;
        }
    }
    __syncthreads();
}

// how a span of n pixels at (lab, tr) is cut: `head` scalar pixels, nb groups of four, `tail` scalar pixels; s = the byte misalignment of a
// group's uint8 truth (0: one aligned dword)
struct SpanCut {
    int head, tail, s;
    long long nb;
};

template <int TB>
__device__ __forceinline__ SpanCut span_cut(const int32_t *lab, const uint8_t *tr, long long n)
{
    SpanCut c;
    c.head = (int)((0 - ((uintptr_t)lab >> 2)) & 3);                       // pixels up to the next 16-byte boundary of the labels
    c.s = TB == 1 ? (int)(((uintptr_t)tr + c.head) & 3) : 0;
    if (c.s && c.head < c.s) c.head += 4;                                      // the aligned dword in front of group 0 starts inside the span
    if (c.head > n) c.head = (int)n;
    const long long rem = n - c.head;
    c.nb = rem >> 2;
    if (c.s && c.nb > 0 && 4 * c.nb + 4 - c.s > rem) c.nb--;                   // ... and the one behind the last group ends inside it
    c.tail = (int)(rem - 4 * c.nb);
    return c;
}

template <int TB>
__device__ __forceinline__ int truth_at(const uint8_t *tr, long long i)
{
    return TB == 1 ? (int)tr[i] : ((const int32_t *)tr)[i];
}

// chunk k of a span: one group per lane, and in chunk 0 the head (lanes 0 ..) and the tail (lanes 64 ..) a pixel per lane
template <int TB, bool LDS>
__device__ __forceinline__ void score_chunk(const ConfusionArgs &a, unsigned *s_bins, const int32_t *lab, const uint8_t *tr, const SpanCut &c,
                                            long long k)
{
    const int classes = a.classes, tid = threadIdx.x;
    if (k == 0) {
        long long i = -1;
        if (tid < c.head) i = tid;
        else if (tid >= 64 && tid < 64 + c.tail) i = c.head + 4 * c.nb + (tid - 64);
        if (i >= 0) bin_add<LDS>(a, s_bins, cf_cell(truth_at<TB>(tr, i), lab[i], classes), 1u);
    }
    const long long g = k * CF_THREADS + tid;
    if (g >= c.nb) return;
    const long long e = c.head + 4 * g;                                        // the group's first pixel
    const int4 p = *(const int4 *)(lab + e);
    int t0, t1, t2, t3;
    if (TB == 4) {
        const I32x4 t = *(const I32x4 *)((const int32_t *)tr + e);
        t0 = t.x; t1 = t.y; t2 = t.z; t3 = t.w;
    } else {
        unsigned v;
        if (c.s == 0) {
            v = *(const unsigned *)(tr + e);
        } else {
            const unsigned *w = (const unsigned *)(tr + e - c.s);
            v = (w[0] >> (8 * c.s)) | (w[1] << (32 - 8 * c.s));
        }
        t0 = (int)(v & 255u); t1 = (int)((v >> 8) & 255u); t2 = (int)((v >> 16) & 255u); t3 = (int)(v >> 24);
    }
    const int c0 = cf_cell(t0, p.x, classes), c1 = cf_cell(t1, p.y, classes), c2 = cf_cell(t2, p.z, classes), c3 = cf_cell(t3, p.w, classes);
    if (c0 == c1 && c1 == c2 && c2 == c3) {
        // the lanes whose four pixels agree: one add per distinct cell of the wave, by the first lane that holds it
        bool done = false;
        for (int it = 0; it < CF_LEADERS && !done; it++) {
            const int lead = __builtin_amdgcn_readfirstlane(c0);
            if (c0 == lead) {
                const unsigned long long m = __ballot(1);
                if ((int)(__lane_id()) == __ffsll((long long)m) - 1) bin_add<LDS>(a, s_bins, lead, 4u * (unsigned)__popcll(m));
                done = true;
            }
        }
        if (!done) bin_add<LDS>(a, s_bins, c0, 4u);
    } else {
        bin_add<LDS>(a, s_bins, c0, 1u);
        bin_add<LDS>(a, s_bins, c1, 1u);
        bin_add<LDS>(a, s_bins, c2, 1u);
        bin_add<LDS>(a, s_bins, c3, 1u);
    }
}

template <int TB, bool LDS, bool RAGGED>
__global__ __launch_bounds__(CF_THREADS) void confusion_i32(const ConfusionArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned s_bins[];
    const int bins = (a.classes + 1) * (a.classes + 1);
    int batch = 1;
    if (RAGGED) {
        if (mbn_label_set_stale(a.set)) return;                                // captured under an earlier set: nothing to score
        batch = a.set.head->batch;
    }
    if (LDS) {
        for (int i = threadIdx.x; i < bins; i += CF_THREADS) s_bins[i] = 0;
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
        const SpanCut c = span_cut<TB>(lab, tr, n);
        const long long chunks = c.nb > CF_THREADS ? (c.nb + CF_THREADS - 1) / CF_THREADS : 1;
        for (long long k = (b + G - rot) % G; k < chunks; k += G) {
            score_chunk<TB, LDS>(a, s_bins, lab, tr, c, k);
            if (LDS && ++epoch == CF_EPOCH) {
                flush_bins<LDS>(a, s_bins, bins);
                epoch = 0;
            }
        }
        rot = (unsigned)((rot + chunks % G) % G);
    }
    if (LDS) flush_bins<LDS>(a, s_bins, bins);
}

// the eight kernels by [ragged][form][int32 truth]
using Kernel = void (*)(const ConfusionArgs);
const Kernel cf_kernels[2][2][2] = {
    { { confusion_i32<1, true, false>, confusion_i32<4, true, false> }, { confusion_i32<1, false, false>, confusion_i32<4, false, false> } },
    { { confusion_i32<1, true, true>, confusion_i32<4, true, true> }, { confusion_i32<1, false, true>, confusion_i32<4, false, true> } },
};

// The persistent grid: a CU holds two workgroups (32 waves) unless the LDS table is above half of a CU's LDS, then one; never more
// workgroups than there are chunks (+ one per item, whose chunk 0 exists even without a body)
void cf_launch(mbn_context *ctx, hipStream_t s, bool ragged, const ConfusionArgs &a, int truth_bytes, long long pixels, int items)
{
    const int form = mbn_confusion_form(a.classes);
    const int lds_bytes = form == MBN_CONFUSION_FORM_LDS ? (a.classes + 1) * (a.classes + 1) * 4 : 0;
    const int per_cu = 2 * lds_bytes > MBN_CONFUSION_CU_LDS ? 1 : 2;
    const unsigned grid = mbn_persistent_grid(ctx->num_cus, per_cu, pixels / (4 * CF_THREADS) + items);
    // the LDS form's table reaches 91 204 bytes: above the 64 KB a launch gets without asking (once per process; not a stream operation)
    static std::once_flag asked;
    std::call_once(asked, [] {
        for (int rg = 0; rg < 2; rg++)
            for (int tb = 0; tb < 2; tb++)
                (void)hipFuncSetAttribute((const void *)cf_kernels[rg][MBN_CONFUSION_FORM_LDS][tb], hipFuncAttributeMaxDynamicSharedMemorySize,
                                          MBN_CONFUSION_LDS);
    });
    hipLaunchKernelGGL(cf_kernels[ragged][form][truth_bytes == 4], dim3(grid), dim3(CF_THREADS), (size_t)lds_bytes, s, a);
}

}   // namespace

static_assert(CF_EPOCH == MBN_CONFUSION_EPOCH, "the epoch the header documents");

// the arguments are inside mbn_confusion_envelope and the pointers are checked (the caller)
int mbn_launch_i32_confusion(mbn_context *ctx, hipStream_t s, void *counts, const void *labels, const void *truth, int truth_bytes, int classes,
                             int64_t count)
{
    ConfusionArgs a = {};
    a.counts = (unsigned long long *)counts;
    a.labels = (const int32_t *)labels;
    a.truth = (const uint8_t *)truth;
    a.classes = classes;
    a.count = count;
    cf_launch(ctx, s, false, a, truth_bytes, count, 1);
    return MBN_OK;
}

// the handle has a batch; the spans of labels and truth reach r->launch.span elements (the caller has checked them)
int mbn_launch_i32_confusion_ragged(mbn_ragged_readout *r, hipStream_t s, void *counts, const void *labels, const void *truth, int truth_bytes,
                                    int classes)
{
    ConfusionArgs a = {};
    a.counts = (unsigned long long *)counts;
    a.labels = (const int32_t *)labels;
    a.truth = (const uint8_t *)truth;
    a.classes = classes;
    a.set = mbn_ragged_readout_view(r);
    cf_launch(r->ctx, s, true, a, truth_bytes, r->launch.span, r->batch);
    mbn_ragged_readout_mark_done(r, s);
    return MBN_OK;
}
