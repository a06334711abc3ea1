// mbn_i32_panoptic.hip — score a segmentation by its regions on the device (gfx950): panoptic quality of a predicted against a true segment map
// (mbn_panoptic_i32 and its ragged form; include/mbn.h, "score a segmentation by its regions"), with the C-ABI of the handle and
// the two calls, and the widening of a uint8 truth the net runner needs in front of the components call.
//
// No table of (predicted, truth) pairs is built: their number is unbounded. A truth segment g can match a predicted segment p only if
// inter (p, g) > (area (p) - void (p)) / 2: g is then the STRICT MAJORITY among the truth numbers of p's non-void pixels, and each bit of a strict
// majority element is the majority of that bit. So per predicted segment a handful of counters finds the one candidate, and a second pass counts
// its intersection exactly. A candidate that is no real majority is harmless: `decide` checks the exact counts.
// A call is six kernels on one stream; order between phases comes from the kernel boundaries only. No workgroup ever waits for another. A word
// that several workgroups change during one kernel (a slot's counters, the cells of pq_u64) is changed by integer atomic adds on vector memory
// only and read in a later kernel: every result is a function of the input alone, whatever order the atomics arrive in.
//   1 clear      scored_i32; the slots in use: the counters of a predicted slot become 0, a truth slot's match -1
//   2 vote       per pixel of a predicted segment p: non-void or void, and for each bit b of the truth number (only the bits n_truth - 1 has) whether
//                b is set. The lanes of a wave that share p add once: a ballot per counter, and ONE atomic instruction in which lane w carries
//                word w of the slot. A wave inside one segment issues that one instruction for its 64 pixels
//                (of its image); a wave keeps what it owes a slot in registers until it meets another slot
//   3 candidate  per predicted slot: cand = the bits with 2 * count > non-void pixels
//   4 intersect  per pixel: inter (p) += (comp_truth == cand (p)), aggregated per wave the same way
//   5 decide     per predicted slot: the match rule in int64, the per-segment outputs, the truth slot's match, and tp and S, or fp, of its class
//   6 truth      per truth slot: match_truth; an unmatched slot adds fn to its class
// An image with n_pred > max_pred or n_truth > max_truth is skipped by every kernel but the first, which writes scored = 0: each kernel decides
// that from n_*_i32 itself. The units of a pixel kernel (chunks of 1024 pixels) are dealt round robin to a grid sized from the planning CU count;
// the grid of a slot kernel is batch x the workgroups of one image, each striding over the slots of its one image.
#include "mbn_internal.h"
#include "mbn_label_set.h"

namespace {

constexpr int PQ_THREADS = 256;
constexpr int CHUNK = MBN_PANOPTIC_CHUNK;
constexpr int WORDS = MBN_PANOPTIC_SLOT_WORDS;      // of a predicted slot: the four below, then one counter per bit of the truth number
constexpr int W_LIVE = 0, W_VOID = 1, W_INTER = 2, W_BIT0 = 3;
constexpr int PQ_LDS_CLASSES = MBN_PANOPTIC_LDS_CLASSES;  // up to here a workgroup of `decide` / `truth` counts its classes in LDS (32 bytes a class)
constexpr int PQ_LEADERS = 16;                      // distinct keys a wave aggregates per step; the lanes left over act on their own
constexpr int PQ_WGS_PER_CU = 8;
static_assert(CHUNK == 4 * PQ_THREADS, "four pixels per lane and chunk");
static_assert(WORDS <= 64 && W_BIT0 + MBN_PANOPTIC_BITS == WORDS, "lane w of a wave carries word w of a slot");
static_assert((1 << MBN_PANOPTIC_BITS) >= MBN_COMPONENTS_MAX_REGIONS, "a truth number fits the counted bits");

struct PqArgs {
    const int32_t *comp_pred, *comp_truth;
    const int32_t *pred, *truth;              // the records, eight int32 each: [0] label, [1] area
    const int32_t *n_pred, *n_truth;
    unsigned long long *pq;
    int32_t *scored, *match_pred, *match_truth, *inter, *voided;
    int32_t *slots, *tslots, *cands;          // the handle's scratch: [batch][max_pred][WORDS], [batch][max_truth] and [batch][max_pred]
    int batch, rows, cols;                    // batch: both forms (the ragged set's); rows, cols: uniform form
    mbn_label_set set;                        // ragged form: the view of the read-out handle's set
    long long chunks;                         // units of a pixel kernel over the whole call
    int max_pred, max_truth, classes;
};

__host__ __device__ inline long long pq_chunks(int rows, int cols) { return ((long long)rows * cols + CHUNK - 1) / CHUNK; }

// chunk u of the call: the image it lies in (off: its first element in comp_pred / comp_truth) and its number inside that image. Uniform across
// the workgroup (u is)
using Unit = mbn_label_unit;
template <bool RAGGED>
__device__ __forceinline__ bool pq_unit(const PqArgs &a, long long u, Unit &w)
{
    return mbn_label_set_unit<RAGGED, pq_chunks>(a.set, a.batch, a.rows, a.cols, u, w);
}

// what every kernel reads of an image: its two counts (a negative one counts as 0) and whether its tables hold them
struct Image {
    int n_pred, n_truth, bits;
    bool scored;
};

__device__ __forceinline__ Image pq_image(const PqArgs &a, int i)
{
    Image im;
    const int np = a.n_pred[i], nt = a.n_truth[i];
    im.scored = np <= a.max_pred && nt <= a.max_truth;
    im.n_pred = np > 0 ? np : 0;
    im.n_truth = nt > 0 ? nt : 0;
    im.bits = im.n_truth > 1 ? 32 - __clz(im.n_truth - 1) : 0;            // the bits the numbers 0 .. n_truth - 1 have: at most MBN_PANOPTIC_BITS
    return im;
}

// A slot kernel's grid is batch x (workgroups per image): a workgroup reads the counts of ONE image and strides over that image's slots
struct Share {
    int image;
    long long first, stride;      // of the workgroup: its first slot and the slots from one of its rounds to the next
};

__device__ __forceinline__ Share pq_share(const PqArgs &a)
{
    Share s;
    s.image = (int)(blockIdx.x % (unsigned)a.batch);
    s.first = (long long)(blockIdx.x / (unsigned)a.batch) * PQ_THREADS;
    s.stride = (long long)(gridDim.x / (unsigned)a.batch) * PQ_THREADS;
    return s;
}

__device__ __forceinline__ void add_i32(int32_t *p, int v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void add_u64(unsigned long long *p, unsigned long long v)
{
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// -------------------------------------------------------------------------------------------------------------------------- 1 clear
template <bool RAGGED>
__global__ __launch_bounds__(PQ_THREADS) void pq_clear(const PqArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;                  // captured under an earlier set: nothing to do
    const Share sh = pq_share(a);
    const Image im = pq_image(a, sh.image);
    if (sh.first == 0 && threadIdx.x == 0) a.scored[sh.image] = im.scored;
    if (!im.scored) return;
    int32_t *slots = a.slots + (long long)sh.image * a.max_pred * WORDS, *tslots = a.tslots + (long long)sh.image * a.max_truth;
    for (long long k = sh.first + threadIdx.x; k < (long long)im.n_pred * WORDS; k += sh.stride) slots[k] = 0;
    for (long long k = sh.first + threadIdx.x; k < im.n_truth; k += sh.stride) tslots[k] = -1;
}

// --------------------------------------------------------------------------------------------------------------------------- 2 vote
template <bool RAGGED>
__global__ __launch_bounds__(PQ_THREADS) void pq_vote(const PqArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const int lane = threadIdx.x & 63;
    // what the wave still owes the slot it met last: lane w holds word w's count. It is added when the wave meets another slot, and at the end:
    // a wave that stays inside one segment, over all its chunks, issues one atomic instruction
    long long owed_slot = -1;
    int owed = 0;
    for (long long u = blockIdx.x; u < a.chunks; u += gridDim.x) {
        Unit w;
        if (!pq_unit<RAGGED>(a, u, w)) break;
        const Image im = pq_image(a, w.image);
        if (!im.scored) continue;
        const int n = w.rows * w.cols;
        const long long slot0 = (long long)w.image * a.max_pred;
        for (int j = 0; j < CHUNK / PQ_THREADS; j++) {                                     // a wave holds 64 consecutive pixels
            const int px = w.unit * CHUNK + j * PQ_THREADS + (int)threadIdx.x;
            int p = -1, t = -1;
            if (px < n) {
                p = a.comp_pred[w.off + px];
                t = a.comp_truth[w.off + px];
                if ((unsigned)p >= (unsigned)im.n_pred) p = -1;                            // no predicted segment
            }
            // the lanes that share p add once. Every lane of the wave runs this loop (the ballots are wave-uniform)
            bool pending = p >= 0;
            for (int it = 0; it < PQ_LEADERS; it++) {
                const unsigned long long left = __ballot(pending);
                if (!left) break;
                const int lead = __shfl(p, __ffsll((long long)left) - 1);
                const bool same = pending && p == lead, live = same && t >= 0;
                if (slot0 + lead != owed_slot) {                                           // wave-uniform
                    if (owed) add_i32(&a.slots[owed_slot * WORDS + lane], owed);           // owed != 0 only in a lane < WORDS and with owed_slot >= 0
                    owed_slot = slot0 + lead;
                    owed = 0;
                }
                int c = (int)__popcll(__ballot(live));
                if (lane == W_LIVE) owed += c;
                c = (int)__popcll(__ballot(same && t < 0));
                if (lane == W_VOID) owed += c;
                for (int b = 0; b < im.bits; b++) {
                    c = (int)__popcll(__ballot(live && ((t >> b) & 1)));
                    if (lane == W_BIT0 + b) owed += c;
                }
                if (same) pending = false;
            }
            if (pending) {
                int32_t *slot = a.slots + (slot0 + p) * WORDS;
                add_i32(&slot[t >= 0 ? W_LIVE : W_VOID], 1);
                if (t >= 0)
                    for (int b = 0; b < im.bits; b++)
                        if ((t >> b) & 1) add_i32(&slot[W_BIT0 + b], 1);
            }
        }
    }
    if (owed) add_i32(&a.slots[owed_slot * WORDS + lane], owed);
}

// ---------------------------------------------------------------------------------------------------------------------- 3 candidate
// cand lives in an array of its own: `intersect` reads it with plain loads while the slots' own lines are under atomic adds
template <bool RAGGED>
__global__ __launch_bounds__(PQ_THREADS) void pq_candidate(const PqArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const Share sh = pq_share(a);
    const Image im = pq_image(a, sh.image);
    if (!im.scored) return;
    const int32_t *slots = a.slots + (long long)sh.image * a.max_pred * WORDS;
    int32_t *cands = a.cands + (long long)sh.image * a.max_pred;
    for (long long s = sh.first + threadIdx.x; s < im.n_pred; s += sh.stride) {
        const int32_t *slot = slots + s * WORDS;
        const int total = slot[W_LIVE];
        int cand = 0;
        for (int b = 0; b < im.bits; b++)
            if (2 * slot[W_BIT0 + b] > total) cand |= 1 << b;                              // counts stay below 2^29
        cands[s] = cand;
    }
}

// ---------------------------------------------------------------------------------------------------------------------- 4 intersect
template <bool RAGGED>
__global__ __launch_bounds__(PQ_THREADS) void pq_intersect(const PqArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const int lane = threadIdx.x & 63;
    long long owed_slot = -1;                                                              // as in `vote`; lane 0 holds the count
    int owed = 0;
    for (long long u = blockIdx.x; u < a.chunks; u += gridDim.x) {
        Unit w;
        if (!pq_unit<RAGGED>(a, u, w)) break;
        const Image im = pq_image(a, w.image);
        if (!im.scored) continue;
        const int n = w.rows * w.cols;
        const long long slot0 = (long long)w.image * a.max_pred;
        for (int j = 0; j < CHUNK / PQ_THREADS; j++) {
            const int px = w.unit * CHUNK + j * PQ_THREADS + (int)threadIdx.x;
            int p = -1;
            bool hit = false;
            if (px < n) {
                p = a.comp_pred[w.off + px];
                if ((unsigned)p >= (unsigned)im.n_pred) p = -1;
                if (p >= 0) hit = a.comp_truth[w.off + px] == a.cands[slot0 + p];         // cand >= 0: a void pixel never hits
            }
            bool pending = p >= 0;
            for (int it = 0; it < PQ_LEADERS; it++) {
                const unsigned long long left = __ballot(pending);
                if (!left) break;
                const int lead = __shfl(p, __ffsll((long long)left) - 1);
                const bool same = pending && p == lead;
                if (slot0 + lead != owed_slot) {
                    if (owed) add_i32(&a.slots[owed_slot * WORDS + W_INTER], owed);
                    owed_slot = slot0 + lead;
                    owed = 0;
                }
                const int c = (int)__popcll(__ballot(same && hit));
                if (lane == 0) owed += c;
                if (same) pending = false;
            }
            if (pending && hit) add_i32(&a.slots[(slot0 + p) * WORDS + W_INTER], 1);
        }
    }
    if (owed) add_i32(&a.slots[owed_slot * WORDS + W_INTER], owed);
}

// The cells of pq_u64 a workgroup of `decide` or `truth` adds to. Up to PQ_LDS_CLASSES classes it counts in LDS (s_pq [classes][4], cleared by
// pq_begin) and brings each cell it touched to memory once, in pq_end; above, where the adds spread over many cells anyway, each lane adds
// to memory itself. Every thread of the workgroup calls all three.
__device__ __forceinline__ void pq_begin(const PqArgs &a, unsigned long long *s_pq)
{
    if (a.classes > PQ_LDS_CLASSES) return;
    for (int k = threadIdx.x; k < 4 * a.classes; k += PQ_THREADS) s_pq[k] = 0;
    __syncthreads();
}

__device__ __forceinline__ void pq_add(const PqArgs &a, unsigned long long *s_pq, int key, int col, unsigned long long s)
{
    if (key < 0) return;
    if (a.classes > PQ_LDS_CLASSES) {
        add_u64(&a.pq[4 * (long long)key + col], 1);
        if (s) add_u64(&a.pq[4 * (long long)key + 3], s);
        return;
    }
    (void)__hip_atomic_fetch_add(&s_pq[4 * key + col], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (s) (void)__hip_atomic_fetch_add(&s_pq[4 * key + 3], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void pq_end(const PqArgs &a, unsigned long long *s_pq)
{
    if (a.classes > PQ_LDS_CLASSES) return;
    __syncthreads();
    for (int k = threadIdx.x; k < 4 * a.classes; k += PQ_THREADS) {
        const unsigned long long v = s_pq[k];
        if (v) add_u64(&a.pq[k], v);
    }
}

// ------------------------------------------------------------------------------------------------------------------------- 5 decide
template <bool RAGGED>
__global__ __launch_bounds__(PQ_THREADS) void pq_decide(const PqArgs a)
{
    extern __shared__ unsigned long long s_pq[];
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const Share sh = pq_share(a);
    const Image im = pq_image(a, sh.image);
    if (!im.scored) return;                                                                // the whole workgroup
    const int i = sh.image;
    const int32_t *slots = a.slots + (long long)i * a.max_pred * WORDS, *cands = a.cands + (long long)i * a.max_pred;
    const int32_t *pred = a.pred + (long long)i * a.max_pred * 8, *truth = a.truth + (long long)i * a.max_truth * 8;
    int32_t *tslots = a.tslots + (long long)i * a.max_truth;
    pq_begin(a, s_pq);
    for (long long s = sh.first + threadIdx.x; s < im.n_pred; s += sh.stride) {
        const int32_t *slot = slots + s * WORDS;
        const int voided = slot[W_VOID], inter = slot[W_INTER], cand = cands[s];
        const int label = pred[s * 8], area = pred[s * 8 + 1];
        bool match = false;
        long long uni = 0;
        if (cand < im.n_truth && inter > 0 && truth[(long long)cand * 8] == label) {
            uni = (long long)area - voided + truth[(long long)cand * 8 + 1] - inter;
            match = uni >= inter && 2ll * inter > uni;                                     // uni < inter: areas that are not the maps' (mbn.h): no match
        }
        int m = -1, col = 1;
        unsigned long long S = 0;
        if (match) {
            m = cand;
            col = 0;
            tslots[cand] = (int)s;                                                         // its only writer: a truth segment has at most one match (areas as mbn.h asks)
            S = ((unsigned long long)inter << 32) / (unsigned long long)uni;               // uni >= inter > 0
        } else if (2ll * voided > (long long)area) {
            m = -2;                                                                        // excused: counts nowhere
        }
        pq_add(a, s_pq, m != -2 && (unsigned)label < (unsigned)a.classes ? label : -1, col, S);
        const long long o = (long long)i * a.max_pred + s;
        if (a.match_pred) a.match_pred[o] = m;
        if (a.inter) a.inter[o] = match ? inter : 0;
        if (a.voided) a.voided[o] = voided;
    }
    pq_end(a, s_pq);
}

// -------------------------------------------------------------------------------------------------------------------------- 6 truth
template <bool RAGGED>
__global__ __launch_bounds__(PQ_THREADS) void pq_truth(const PqArgs a)
{
    extern __shared__ unsigned long long s_pq[];
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const Share sh = pq_share(a);
    const Image im = pq_image(a, sh.image);
    if (!im.scored) return;
    const int i = sh.image;
    const int32_t *truth = a.truth + (long long)i * a.max_truth * 8, *tslots = a.tslots + (long long)i * a.max_truth;
    pq_begin(a, s_pq);
    for (long long s = sh.first + threadIdx.x; s < im.n_truth; s += sh.stride) {
        const int m = tslots[s];
        if (a.match_truth) a.match_truth[(long long)i * a.max_truth + s] = m;
        const int label = truth[s * 8];
        pq_add(a, s_pq, m < 0 && (unsigned)label < (unsigned)a.classes ? label : -1, 2, 0ull);
    }
    pq_end(a, s_pq);
}

// a uint8 map widened to int32, value for value (255 stays 255)
__global__ __launch_bounds__(PQ_THREADS) void widen_u8(int32_t *dst, const uint8_t *src, long long count)
{
    for (long long k = (long long)blockIdx.x * PQ_THREADS + threadIdx.x; k < count; k += (long long)gridDim.x * PQ_THREADS) dst[k] = src[k];
}

// a slot kernel: `batch` times the workgroups of one image, as many as its units want and the planning CU count gives (one at least)
unsigned pq_slot_grid(const mbn_context *ctx, int batch, long long units)
{
    long long per = (long long)(ctx->num_cus > 0 ? ctx->num_cus : 1) * PQ_WGS_PER_CU / batch;
    if (per > units) per = units;
    return (unsigned)batch * (unsigned)(per > 0 ? per : 1);
}

template <bool RAGGED>
void pq_launch(mbn_context *ctx, hipStream_t s, const PqArgs &a, int batch)
{
    const dim3 block(PQ_THREADS);
    const long long most = a.max_pred > a.max_truth ? a.max_pred : a.max_truth;
    const unsigned slot_grid = pq_slot_grid(ctx, batch, (most + PQ_THREADS - 1) / PQ_THREADS);
    const unsigned word_grid = pq_slot_grid(ctx, batch, (most * WORDS + PQ_THREADS - 1) / PQ_THREADS);
    const unsigned lds = a.classes <= PQ_LDS_CLASSES ? 32u * a.classes : 0u;
    hipLaunchKernelGGL(pq_clear<RAGGED>, dim3(word_grid), block, 0, s, a);
    hipLaunchKernelGGL(pq_vote<RAGGED>, dim3(mbn_persistent_grid(ctx->num_cus, PQ_WGS_PER_CU, a.chunks)), block, 0, s, a);
    hipLaunchKernelGGL(pq_candidate<RAGGED>, dim3(slot_grid), block, 0, s, a);
    hipLaunchKernelGGL(pq_intersect<RAGGED>, dim3(mbn_persistent_grid(ctx->num_cus, PQ_WGS_PER_CU, a.chunks)), block, 0, s, a);
    hipLaunchKernelGGL(pq_decide<RAGGED>, dim3(slot_grid), block, lds, s, a);
    hipLaunchKernelGGL(pq_truth<RAGGED>, dim3(slot_grid), block, lds, s, a);
}

// What the two calls share once the shape is known: `shape` = the envelope's answer, `span` = the elements of the maps
int pq_call(mbn_panoptic *h, mbn_ragged_readout *r, PqArgs &a, int shape, int batch, double span, void *stream)
{
    mbn_context *ctx = h->ctx;
    if (shape == MBN_EINVAL) return shape;
    if ((uintptr_t)a.pq % 8) return MBN_EINVAL;
    const void *const words[] = { a.scored, a.match_pred, a.match_truth, a.inter, a.voided, a.comp_pred, a.pred, a.n_pred, a.comp_truth, a.truth, a.n_truth };
    for (const void *p : words)
        if ((uintptr_t)p % 4) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    const int most = a.max_pred > a.max_truth ? a.max_pred : a.max_truth;
    if (batch > h->max_batch || (int64_t)batch * most > h->capacity) return MBN_EINVAL;
    const double np = (double)batch * a.max_pred, nt = (double)batch * a.max_truth;
    const mbn_span sp[] = { { a.pq, 32.0 * a.classes, "panoptic pq" }, { a.scored, 4.0 * batch, "panoptic scored" },
                        { a.match_pred, 4.0 * np, "panoptic match_pred" }, { a.match_truth, 4.0 * nt, "panoptic match_truth" },
                        { a.inter, 4.0 * np, "panoptic inter" }, { a.voided, 4.0 * np, "panoptic void" },
                        { a.comp_pred, 4.0 * span, "panoptic comp_pred" }, { a.pred, 32.0 * np, "panoptic pred" },
                        { a.n_pred, 4.0 * batch, "panoptic n_pred" }, { a.comp_truth, 4.0 * span, "panoptic comp_truth" },
                        { a.truth, 32.0 * nt, "panoptic truth" }, { a.n_truth, 4.0 * batch, "panoptic n_truth" } };
    const int rc = mbn_span_check(ctx, sp, (int)(sizeof sp / sizeof sp[0]));
    if (rc != MBN_OK) return rc;
    a.slots = (int32_t *)h->scratch;
    a.tslots = a.slots + h->capacity * WORDS;
    a.cands = a.tslots + h->capacity;
    a.batch = batch;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    (void)hipSetDevice(ctx->device);
    if (r) {
        pq_launch<true>(ctx, s, a, batch);
        mbn_ragged_readout_mark_done(r, s);
    } else {
        pq_launch<false>(ctx, s, a, batch);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MBN_OK : mbn_record_hip_error(ctx, e, "panoptic launch");
}

PqArgs pq_args(void *pq_u64, void *scored_i32, void *match_pred_i32, void *match_truth_i32, void *inter_i32, void *void_i32, const void *comp_pred_i32,
               const mbn_region *pred, const void *n_pred_i32, int max_pred, const void *comp_truth_i32, const mbn_region *truth,
               const void *n_truth_i32, int max_truth, int classes)
{
    PqArgs a = {};
    a.pq = (unsigned long long *)pq_u64;
    a.scored = (int32_t *)scored_i32; a.match_pred = (int32_t *)match_pred_i32; a.match_truth = (int32_t *)match_truth_i32;
    a.inter = (int32_t *)inter_i32; a.voided = (int32_t *)void_i32;
    a.comp_pred = (const int32_t *)comp_pred_i32; a.pred = (const int32_t *)pred; a.n_pred = (const int32_t *)n_pred_i32;
    a.comp_truth = (const int32_t *)comp_truth_i32; a.truth = (const int32_t *)truth; a.n_truth = (const int32_t *)n_truth_i32;
    a.max_pred = max_pred; a.max_truth = max_truth; a.classes = classes;
    return a;
}

bool pq_required(const PqArgs &a)
{
    return a.pq && a.scored && a.comp_pred && a.pred && a.n_pred && a.comp_truth && a.truth && a.n_truth;
}

}   // namespace

extern "C" {

int mbn_panoptic_create(mbn_context *ctx, int max_batch, int64_t max_slots, mbn_panoptic **h)
{
    return mbn_scratch_create(ctx, max_batch, max_slots, mbn_panoptic_scratch_bytes(max_batch, max_slots), h);
}

int mbn_panoptic_destroy(mbn_panoptic *h) { return mbn_scratch_destroy(h); }

int mbn_panoptic_i32(mbn_panoptic *h, void *pq_u64, void *scored_i32, void *match_pred_i32, void *match_truth_i32, void *inter_i32, void *void_i32,
                     const void *comp_pred_i32, const mbn_region *pred, const void *n_pred_i32, int max_pred, const void *comp_truth_i32,
                     const mbn_region *truth, const void *n_truth_i32, int max_truth, int batch, int rows, int cols, int classes, void *stream)
{
    PqArgs a = pq_args(pq_u64, scored_i32, match_pred_i32, match_truth_i32, inter_i32, void_i32, comp_pred_i32, pred, n_pred_i32, max_pred,
                       comp_truth_i32, truth, n_truth_i32, max_truth, classes);
    if (!h || !pq_required(a)) return MBN_EINVAL;
    const int shape = mbn_panoptic_envelope(batch, rows, cols, classes, max_pred, max_truth);
    double pixels = 0.0;
    if (shape == MBN_OK) {
        a.batch = batch; a.rows = rows; a.cols = cols;
        a.chunks = batch * pq_chunks(rows, cols);
        pixels = (double)batch * rows * cols;
    }
    return pq_call(h, nullptr, a, shape, batch, pixels, stream);
}

int mbn_panoptic_ragged_i32(mbn_panoptic *h, mbn_ragged_readout *r, void *pq_u64, void *scored_i32, void *match_pred_i32, void *match_truth_i32,
                            void *inter_i32, void *void_i32, const void *comp_pred_i32, const mbn_region *pred, const void *n_pred_i32, int max_pred,
                            const void *comp_truth_i32, const mbn_region *truth, const void *n_truth_i32, int max_truth, int classes, void *stream)
{
    PqArgs a = pq_args(pq_u64, scored_i32, match_pred_i32, match_truth_i32, inter_i32, void_i32, comp_pred_i32, pred, n_pred_i32, max_pred,
                       comp_truth_i32, truth, n_truth_i32, max_truth, classes);
    if (!h || !r || r->ctx != h->ctx || r->batch <= 0 || !pq_required(a)) return MBN_EINVAL;                   // no set: nothing to score
    a.set = mbn_ragged_readout_view(r);
    // the items of the last set, as the handle's pinned block still holds them: every map inside the envelope, and the units of the call
    const int shape = mbn_ragged_readout_envelope(r, [&](const mbn_label_item &it) {
        const int rc = mbn_panoptic_envelope(r->batch, it.rows, it.cols, classes, max_pred, max_truth);
        if (rc == MBN_OK) a.chunks += pq_chunks(it.rows, it.cols);
        return rc;
    });
    return pq_call(h, r, a, shape, r->batch, (double)r->launch.span, stream);
}

int64_t mbn_ragged_readout_span(const mbn_ragged_readout *r)
{
    return r && r->batch > 0 ? (int64_t)r->launch.span : 0;
}

int mbn_widen_u8_i32(mbn_context *ctx, void *dst_i32, const void *src_u8, int64_t count, void *stream)
{
    if (!ctx || !dst_i32 || !src_u8 || count < 1 || (uintptr_t)dst_i32 % 4) return MBN_EINVAL;
    const mbn_span sp[] = { { dst_i32, 4.0 * (double)count, "widen dst" }, { src_u8, (double)count, "widen src" } };
    const int rc = mbn_span_check(ctx, sp, 2);
    if (rc != MBN_OK) return rc;
    (void)hipSetDevice(ctx->device);
    const unsigned grid = mbn_persistent_grid(ctx->num_cus, PQ_WGS_PER_CU, (count + CHUNK - 1) / CHUNK);
    hipLaunchKernelGGL(widen_u8, dim3(grid), dim3(PQ_THREADS), 0, stream ? (hipStream_t)stream : ctx->stream, (int32_t *)dst_i32,
                       (const uint8_t *)src_u8, (long long)count);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MBN_OK : mbn_record_hip_error(ctx, e, "widen launch");
}

}   // extern "C"
