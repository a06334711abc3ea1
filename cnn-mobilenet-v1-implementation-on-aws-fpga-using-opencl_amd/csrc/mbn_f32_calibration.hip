// mbn_f32_calibration.hip — "is the probability worth anything" on the device (gfx950): the reliability table of int32 label maps and their fp32
// softmax probabilities against a uint8 or int32 ground truth, accumulated into uint64 calib [bins + 1][4] (mbn_calibration_f32 and its ragged
// form; include/mbn.h, "calibration score"). Per probability bin: the pixels answered, those answered correctly, the sum of their
// probabilities in 2^-24 fixed point, and the pixels abstained; row `bins` counts the void pixels. Once a pixel's bin and its fixed-point
// probability are formed (one fp32 multiply each, the second exact) everything is integer, so the result is the same whatever order the atomics
// arrive in and at every planning CU count.
//
// The structure is mbn_i32_topk_rank.hip's. A SPAN is n consecutive pixels: the whole call (uniform form) or one item of a ragged set; a CHUNK is
// 1024 consecutive pixels of a span, one per lane of a workgroup. A lane loads its truth, and only for a valid truth its label and probability
// (what lies under a void pixel is never read), so every load of a wave is one coalesced run of dwords or bytes; no alignment beyond the
// elements' own is assumed. An abstained pixel's fixed-point probability is not formed.
//
// The grid is persistent: num_cus * 2 workgroups, workgroup b takes the chunks c with (c + rot) % grid == b, rot = the chunks of the items before.
// One form: a workgroup counts into a private table of (bins + 1) * 4 64-bit cells in LDS (ds_add_u64; at most 32 800 bytes, inside what a launch
// gets without asking) and adds its non-zero cells to `calib` with 64-bit global atomics once, at the end: a 64-bit cell holds whatever a call
// within the envelope can add, so there is no epoch flush.
// Wave aggregation: confident regions put most lanes of a wave into the same bin, usually the last. All 64 lanes of a wave walk CB_LEADERS rounds
// together; in each, the first lane not yet counted names its (bin, answered / abstained / void) key, the lanes that hold the same key are
// balloted, and that first lane adds their popcounts once and, for an answered key, the sum of their fixed-point probabilities: each at most
// 2^24, 64 lanes, so a 32-bit wave reduction cannot overflow. Lanes that all hold one probability (a saturated region: 1.0) need no reduction, the
// sum is a product. The lanes left over add on their own. A wave whose first key holds less than a quarter of its pixels does not aggregate at
// all: with the bins spread over the lanes the rounds cost more than the adds they save (measured: profiles/LOG.md, "Calibration score").
// The plain form (every lane adds on its own) exists in the lab build only (exp0 = 1010; profiles/LOG.md, "Calibration score").
#include "mbn_internal.h"
#include "mbn_label_set.h"

namespace {

constexpr int CB_THREADS = 1024;          // lanes of a workgroup = pixels of a chunk
constexpr int CB_LEADERS = 4;             // distinct keys a wave aggregates per chunk
constexpr unsigned CB_SPREAD = 4;         // a wave aggregates when its first key holds at least 1 / CB_SPREAD of its pixels
constexpr int CB_LAB_PLAIN = 1010;        // lab exp0: no wave aggregation
struct CalibArgs {
    unsigned long long *calib;
    const int32_t *labels;
    const float *prob;
    const uint8_t *truth;      // element 0 of the truth, uint8 or int32
    int classes, bins;
    long long count;           // uniform form: the span
    mbn_label_set set;         // ragged form: the view of the handle's set
};

__device__ __forceinline__ void cb_add(unsigned long long *s_tab, int cell, unsigned long long w)
{
    (void)__hip_atomic_fetch_add(&s_tab[cell], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// what a key (row * 2 + abstained; the void row has no abstained half) adds: n pixels, `correct` of them right, their fixed-point sum q
__device__ __forceinline__ void cb_add_key(unsigned long long *s_tab, int bins, int key, unsigned n, unsigned correct, unsigned q)
{
    const int row = key >> 1;
    if (row == bins || !(key & 1)) {
        cb_add(s_tab, row * 4, n);                                             // answered, or void
        if (correct) cb_add(s_tab, row * 4 + 1, correct);
        if (q) cb_add(s_tab, row * 4 + 2, q);
    } else {
        cb_add(s_tab, row * 4 + 3, n);                                         // abstained
    }
}

// the sum of v over the 64 lanes of a wave; every lane of the wave is active (the caller)
__device__ __forceinline__ unsigned cb_wave_sum(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (unsigned)__shfl_xor((int)v, d, 64);
    return v;
}

template <int TB, bool RAGGED, bool AGG>
__global__ __launch_bounds__(CB_THREADS) void calibration_f32(const CalibArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long s_tab[];
    const int classes = a.classes, bins = a.bins, cells = (bins + 1) * 4;
    const float fbins = (float)bins;
    int batch = 1;
    if (RAGGED) {
        if (mbn_label_set_stale(a.set)) return;                                // captured under an earlier set: nothing to score
        batch = a.set.head->batch;
    }
    for (int i = threadIdx.x; i < cells; i += CB_THREADS) s_tab[i] = 0;
    __syncthreads();
    const unsigned G = gridDim.x, b = blockIdx.x;
    unsigned rot = 0;
    for (int i = 0; i < batch; i++) {
        long long off = 0, n = a.count;
        if (RAGGED) {
            const mbn_label_item *it = mbn_label_set_item(a.set, i);
            off = it->dst_offset;
            n = (long long)it->rows * it->cols;
        }
        const int32_t *lab = a.labels + off;
        const float *pr = a.prob + off;
        const uint8_t *tr = a.truth + off * TB;
        const long long chunks = (n + CB_THREADS - 1) / CB_THREADS;
        for (long long c = (b + G - rot) % G; c < chunks; c += G) {
            const long long e = c * CB_THREADS + threadIdx.x;
            const bool live = e < n;
            int key = bins * 2;                                                // void
            bool correct = false;
            unsigned q = 0;
            if (live) {
                const int t = TB == 1 ? (int)tr[e] : ((const int32_t *)tr)[e];
                if ((unsigned)t < (unsigned)classes) {
                    const int l = lab[e];
                    const float x = pr[e];
                    const float p = x > 1.0f ? 1.0f : (x >= 0.0f ? x : 0.0f);  // a NaN fails both compares: 0
                    const int bin = min(bins - 1, (int)(p * fbins));
                    const bool answered = (unsigned)l < (unsigned)classes;
                    key = bin * 2 + (answered ? 0 : 1);
                    if (answered) {
                        correct = l == t;
                        q = (unsigned)(p * 16777216.0f);                       // exact: a power of two
                    }
                }
            }
            bool todo = live;
            if (AGG) {
                // every lane of the wave is here: one add per distinct key, by the first lane that still holds one
                unsigned long long pending = __ballot(todo);
                for (int it = 0; it < CB_LEADERS && pending; it++) {
                    const int first = __ffsll((long long)pending) - 1;
                    const int lead = __builtin_amdgcn_readlane(key, first);
                    const bool mine = todo && key == lead;
                    const unsigned long long m = __ballot(mine);
                    const unsigned cnt = (unsigned)__popcll(m);
                    // the first key holds less than a quarter of the wave: the bins are spread, rounds would cost more than they save
                    if (it == 0 && cnt * CB_SPREAD < (unsigned)__popcll(pending)) break;
                    unsigned right = 0, qsum = q;
                    if (!(lead & 1) && lead != bins * 2) {                     // an answered key (the same in every lane)
                        right = (unsigned)__popcll(__ballot(mine && correct));
                        // a saturated region holds one probability (1.0 as a rule): its sum is a product, else the wave reduces
                        const unsigned qlead = (unsigned)__builtin_amdgcn_readlane((int)q, first);
                        if (__ballot(mine && q == qlead) == m) qsum = cnt * qlead;
                        else qsum = cb_wave_sum(mine ? q : 0u);
                    }
                    if ((int)__lane_id() == first) cb_add_key(s_tab, bins, lead, cnt, right, qsum);
                    todo = todo && !mine;
                    pending &= ~m;
                }
            }
            if (todo) cb_add_key(s_tab, bins, key, 1u, correct ? 1u : 0u, q);
        }
        rot = (unsigned)((rot + chunks % G) % G);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += CB_THREADS) {
        const unsigned long long v = s_tab[i];
        if (v) (void)__hip_atomic_fetch_add(&a.calib[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the kernels by [plain (lab only)][ragged][int32 truth]
using Kernel = void (*)(const CalibArgs);
const Kernel cb_kernels[1 + MBN_LAB_BUILD][2][2] = {
    { { calibration_f32<1, false, true>, calibration_f32<4, false, true> }, { calibration_f32<1, true, true>, calibration_f32<4, true, true> } },
#if MBN_LAB_BUILD
    { { calibration_f32<1, false, false>, calibration_f32<4, false, false> }, { calibration_f32<1, true, false>, calibration_f32<4, true, false> } },
#endif
};

// The persistent grid: two workgroups (32 waves) on a CU, each with its table of (bins + 1) * 32 bytes; never more workgroups than there are
// chunks (+ one per item)
void cb_launch(mbn_context *ctx, hipStream_t s, bool ragged, const CalibArgs &a, int truth_bytes, long long pixels, int items)
{
    const int plain = MBN_LAB_BUILD && g_mbn_tune.exp0 == CB_LAB_PLAIN ? 1 : 0;
    const size_t lds_bytes = (size_t)(a.bins + 1) * 4 * sizeof(unsigned long long);
    const unsigned grid = mbn_persistent_grid(ctx->num_cus, 2, pixels / CB_THREADS + items);
    hipLaunchKernelGGL(cb_kernels[plain][ragged][truth_bytes == 4], dim3(grid), dim3(CB_THREADS), lds_bytes, s, a);
}

CalibArgs cb_args(void *calib, const void *labels, const void *prob, const void *truth, int classes, int bins)
{
    CalibArgs a = {};
    a.calib = (unsigned long long *)calib;
    a.labels = (const int32_t *)labels;
    a.prob = (const float *)prob;
    a.truth = (const uint8_t *)truth;
    a.classes = classes; a.bins = bins;
    return a;
}

}   // namespace

static_assert((MBN_CALIBRATION_MAX_BINS + 1) * 4 * 8 <= 48 * 1024, "the table fits the LDS a launch gets without asking");

// the arguments are inside mbn_calibration_envelope and the pointers are checked (the caller)
int mbn_launch_f32_calibration(mbn_context *ctx, hipStream_t s, void *calib, const void *labels, const void *prob, const void *truth, int truth_bytes,
                               int classes, int bins, int64_t count)
{
    CalibArgs a = cb_args(calib, labels, prob, truth, classes, bins);
    a.count = count;
    cb_launch(ctx, s, false, a, truth_bytes, count, 1);
    return MBN_OK;
}

// the handle has a batch; the spans of labels, prob and truth reach r->launch.span elements (the caller has checked them)
int mbn_launch_f32_calibration_ragged(mbn_ragged_readout *r, hipStream_t s, void *calib, const void *labels, const void *prob, const void *truth,
                                      int truth_bytes, int classes, int bins)
{
    CalibArgs a = cb_args(calib, labels, prob, truth, classes, bins);
    a.set = mbn_ragged_readout_view(r);
    cb_launch(r->ctx, s, true, a, truth_bytes, r->launch.span, r->batch);
    mbn_ragged_readout_mark_done(r, s);
    return MBN_OK;
}
