// mbn_i32_surface.hip — score a segmentation by surface distance on the device (gfx950): for every contour pixel of a class in one map the exact
// squared Euclidean distance to the nearest contour pixel of the same class in the other map of the image, accumulated per class and direction into
// the table Hausdorff, HD95, ASSD and NSD are read from (mbn_surface_score_i32 and its ragged form; include/mbn.h, "score a segmentation by
// surface distance"). Squared distances between pixels are integers and both roots are fixed up in integers, so the result does
// not depend on the order in which the atomics arrive, nor on the grid.
//
// Three kernels on the stream, no host decision between them:
//   CLEAR    the presence table of the handle, [2 sides][batch][classes] words.
//   CONTOUR  (pass A) a lane per pixel of both maps: the pixel and its eight neighbours are read from the caller's maps; the two scratch CONTOUR
//            MAPS get the value where the pixel is a contour pixel of a class in range, else -1, and the presence entry of (side, image, class)
//            is set. The scratch is indexed by the pixels of the images in front, not by the caller's element offsets: a ragged set's gaps cost
//            nothing there.
//   SEARCH   (pass B) a wave owns 64 consecutive pixels of a map and both directions. A ballot finds its queries; the wave takes them one after the
//            other. A query whose class has no presence entry on the other side is unmatched without a search. Otherwise the 7 x 7 window around
//            the query (Chebyshev rings 0..3) is read by 49 lanes at once, then rings k = 4, 5, ... follow, each as its four sides CLIPPED to the
//            map and dealt over the 64 lanes. A lane keeps its own minimum; the wave reduces only in a ring in which some lane improved. The
//            search ends as soon as k * k >= best: uncapped, and exact. (Measured against every LANE reading the window of its own query
//            first, 49 loads a lane, and the wave taking only what that leaves: 16 % slower on block maps, 3 % faster on random ones; not
//            taken. DESIGN.md 7d.11.) The result returns to the query's lane; after the last query every lane forms its roots and the wave adds: lanes of one class elect a leader
//            for n, unmatched, max_d2 and sum256 (up to SF_LEADERS classes a wave and direction), the bins go through the same election by cell.
//            Lanes left over add on their own.
// Queries are found by ballot over the wave's own pixels, not from a compacted queue: a queue needs a fourth kernel, a counter and 12 bytes a query,
// and was not built, so there is no measurement of it; a persistent grid of small units (MBN_SURFACE_UNIT pixels) spreads the expensive chunks instead.
// The grids are persistent, sized from the planning CU count; no workgroup waits for another and no wave of a workgroup for its neighbours (there
// is no barrier and no LDS). Indices inside a map are below 2^29 and a squared distance below 2^31 (the envelope).
#include "mbn_internal.h"
#include "mbn_label_set.h"

// mbn_surface_create's handle: capacity = max_pixels; scratch = contour maps [2][max_pixels] int32, presence [2][max_batch][max_classes] int32
struct mbn_surface : mbn_scratch {
    int max_classes = 0;
};

namespace {

constexpr int SF_THREADS = MBN_SURFACE_UNIT;           // a unit of both pixel kernels: this many consecutive pixels of one map, a wave per 64
constexpr int SF_WGS_PER_CU = 2048 / SF_THREADS;
constexpr int SF_LEADERS = 8;                          // distinct classes (and bin cells) a wave aggregates per direction
constexpr int SF_NEAR = 3;                             // the rings of the window the wave reads at once: (2 * 3 + 1)^2 = 49 <= 64 lanes
constexpr int SF_NONE = 0x7fffffff;                    // no distance yet: above every d2 of the envelope
constexpr unsigned SF_NOT_QUERY = 0xFFFFFFFFu, SF_UNMATCHED = 0xFFFFFFFEu;
static_assert(SF_THREADS % 64 == 0 && MBN_SURFACE_HEAD == 4, "whole waves; the four head cells the adds below name");

struct SurfaceArgs {
    unsigned long long *surf;
    unsigned *dist2;                       // or null
    const int32_t *labels;
    const uint8_t *truth;
    int32_t *contour[2];                   // scratch: side 0 = labels, side 1 = truth
    int32_t *presence;                     // scratch: [2][batch][classes]
    int classes, bins, batch, rows, cols, edge;
    mbn_label_set set;                     // ragged form
};

MBN_SET_FN long long sf_units(int rows, int cols) { return ((long long)rows * cols + SF_THREADS - 1) / SF_THREADS; }

__global__ __launch_bounds__(SF_THREADS) void surface_clear(int32_t *presence, int words)
{
    for (int i = blockIdx.x * SF_THREADS + threadIdx.x; i < words; i += gridDim.x * SF_THREADS) presence[i] = 0;
}

template <int EB>
__device__ __forceinline__ int sf_value(const uint8_t *map, long long i)
{
    return EB == 1 ? (int)map[i] : ((const int32_t *)map)[i];
}

// the pixel (r, c) of a map whose element 0 is `map`: its value where it is a contour pixel of a class in range, else -1
template <int EB>
__device__ __forceinline__ int sf_contour(const uint8_t *map, int rows, int cols, int r, int c, int edge, int classes)
{
    const int v = sf_value<EB>(map, (long long)r * cols + c);
    bool contour = false;
#pragma unroll
    for (int dr = -1; dr <= 1; dr++)
#pragma unroll
        for (int dc = -1; dc <= 1; dc++) {
            if (!dr && !dc) continue;
            const int rr = r + dr, cc = c + dc;
            if (rr < 0 || rr >= rows || cc < 0 || cc >= cols) contour |= edge != 0;
            else contour |= sf_value<EB>(map, (long long)rr * cols + cc) != v;
        }
    return contour && (unsigned)v < (unsigned)classes ? v : -1;
}

// ------------------------------------------------------------------------------------------------------------------------- pass A
template <int EB, bool RAGGED>
__global__ __launch_bounds__(SF_THREADS) void surface_contour(const SurfaceArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;          // captured under an earlier set: nothing to do
    for (long long u = blockIdx.x;; u += gridDim.x) {
        mbn_label_unit w;
        if (!mbn_label_set_unit<RAGGED, sf_units>(a.set, a.batch, a.rows, a.cols, u, w)) break;
        const int n = w.rows * w.cols, p = w.unit * SF_THREADS + (int)threadIdx.x;
        if (p >= n) continue;
        const int r = p / w.cols, c = p - r * w.cols;
        const int l = sf_contour<4>((const uint8_t *)(a.labels + w.off), w.rows, w.cols, r, c, a.edge, a.classes);
        const int t = sf_contour<EB>(a.truth + w.off * EB, w.rows, w.cols, r, c, a.edge, a.classes);
        a.contour[0][w.pixels + p] = l;
        a.contour[1][w.pixels + p] = t;
        // every writer of an entry writes the same 1
        if (l >= 0) a.presence[(long long)w.image * a.classes + l] = 1;
        if (t >= 0) a.presence[((long long)a.batch + w.image) * a.classes + t] = 1;
    }
}

// ------------------------------------------------------------------------------------------------------------------------- pass B
__device__ __forceinline__ int wave_min(int v)
{
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// The smallest squared distance from (r, c) to a pixel of `other` (one map's contour map, rows x cols) that holds cls; SF_NONE when there is none.
// Every argument is the same in all lanes of the wave, and so is the answer. Every index read lies inside [0, rows * cols)
__device__ __forceinline__ int sf_search(const int32_t *other, int rows, int cols, int r, int c, int cls)
{
    const int lane = threadIdx.x & 63;
    int best = SF_NONE, mine = SF_NONE;
    {
        // rings 0..SF_NEAR at once: lane j < 49 takes (r - 3 + j / 7, c - 3 + j % 7)
        constexpr int side = 2 * SF_NEAR + 1;
        const int dr = lane / side - SF_NEAR, dc = lane % side - SF_NEAR, rr = r + dr, cc = c + dc;
        if (lane < side * side && rr >= 0 && rr < rows && cc >= 0 && cc < cols && other[rr * cols + cc] == cls) mine = dr * dr + dc * dc;
        if (__ballot(mine < best)) best = wave_min(mine);
    }
    // ring k can hold nothing nearer than k: the search is over at k * k >= best. Past the last ring that meets the map there is nothing to read
    const int last = max(max(r, rows - 1 - r), max(c, cols - 1 - c));
    for (int k = SF_NEAR + 1; k <= last && (long long)k * k < best; k++) {
        const int c_lo = max(c - k, 0), c_hi = min(c + k, cols - 1), r_lo = max(r - k + 1, 0), r_hi = min(r + k - 1, rows - 1);
        const int l_row = c_hi - c_lo + 1, l_col = max(r_hi - r_lo + 1, 0);
        const int top = r - k >= 0 ? l_row : 0, bottom = top + (r + k < rows ? l_row : 0);
        const int left = bottom + (c - k >= 0 ? l_col : 0), total = left + (c + k < cols ? l_col : 0);
        for (int j = lane; j < total; j += 64) {
            int rr, cc;
            if (j < top) { rr = r - k; cc = c_lo + j; }
            else if (j < bottom) { rr = r + k; cc = c_lo + (j - top); }
            else if (j < left) { rr = r_lo + (j - bottom); cc = c - k; }
            else { rr = r_lo + (j - left); cc = c + k; }
            if (other[rr * cols + cc] == cls) {
                const int dr = rr - r, dc = cc - c;
                mine = min(mine, dr * dr + dc * dc);
            }
        }
        if (__ballot(mine < best)) best = wave_min(mine);
    }
    return best;
}

// floor (sqrt (v)) for v < 2^48: the double root, fixed up in integers
__device__ __forceinline__ unsigned sf_isqrt(unsigned long long v)
{
    unsigned long long t = (unsigned long long)sqrt((double)v);
    while (t * t > v) t--;
    while ((t + 1) * (t + 1) <= v) t++;
    return (unsigned)t;
}

__device__ __forceinline__ void sf_add(unsigned long long *cell, unsigned long long w)
{
    (void)__hip_atomic_fetch_add(cell, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The adds of a wave's queries of one direction: q = the lane's class or -1, res = its d2 or SF_UNMATCHED. Every lane of the wave calls it
__device__ __forceinline__ void sf_accumulate(const SurfaceArgs &a, int dir, int q, unsigned res)
{
    const int lane = threadIdx.x & 63, stride = MBN_SURFACE_HEAD + a.bins;
    const bool query = q >= 0, matched = query && res != SF_UNMATCHED;
    const unsigned d2 = matched ? res : 0u;
    const unsigned s256 = matched ? sf_isqrt((unsigned long long)d2 << 16) : 0u;      // floor (256 d) < 2^24: 64 of them fit 32 bits
    const unsigned root = matched ? sf_isqrt(d2) : 0u;
    const int bin = min((int)(root + (root * root < d2)), a.bins - 1);                // ceil (d), the last bin takes the rest
    const long long base = ((long long)(query ? q : 0) * 2 + dir) * stride;
    // the head cells, a leader per class
    bool active = query;
    unsigned long long pending = __ballot(active);
    for (int it = 0; it < SF_LEADERS && pending; it++) {       // wave-uniform
        const int src = __ffsll((long long)pending) - 1;
        const int lead = __shfl(q, src);
        const bool same = active && q == lead;
        const unsigned long long m = __ballot(same);
        const unsigned n = (unsigned)__popcll(m), hit = (unsigned)__popcll(__ballot(same && matched));
        const int far = wave_max(same && matched ? (int)d2 : 0);
        const unsigned sum = wave_sum(same ? s256 : 0u);
        if (lane == src) {
            unsigned long long *cell = a.surf + base;
            sf_add(cell, n);
            if (n > hit) sf_add(cell + 1, n - hit);
            // a maximum and a sum of 0 change nothing: a map scored against itself leaves two adds a class, not four, on its few cells
            if (far) (void)__hip_atomic_fetch_max(cell + 2, (unsigned long long)far, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (sum) sf_add(cell + 3, sum);
        }
        if (same) active = false;
        pending &= ~m;
    }
    if (active) {
        unsigned long long *cell = a.surf + base;
        sf_add(cell, 1);
        if (!matched) sf_add(cell + 1, 1);
        else if (d2) {
            (void)__hip_atomic_fetch_max(cell + 2, (unsigned long long)d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sf_add(cell + 3, s256);
        }
    }
    // the bins, a leader per cell
    const long long mine = base + MBN_SURFACE_HEAD + bin;
    active = matched;
    pending = __ballot(active);
    for (int it = 0; it < SF_LEADERS && pending; it++) {
        const int src = __ffsll((long long)pending) - 1;
        const long long lead = __shfl(mine, src);
        const bool same = active && mine == lead;
        const unsigned long long m = __ballot(same);
        if (lane == src) sf_add(a.surf + lead, (unsigned long long)__popcll(m));
        if (same) active = false;
        pending &= ~m;
    }
    if (active) sf_add(a.surf + mine, 1);
}

template <bool RAGGED>
__global__ __launch_bounds__(SF_THREADS) void surface_search(const SurfaceArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const int lane = threadIdx.x & 63;
    for (long long u = blockIdx.x;; u += gridDim.x) {
        mbn_label_unit w;
        if (!mbn_label_set_unit<RAGGED, sf_units>(a.set, a.batch, a.rows, a.cols, u, w)) break;
        const int n = w.rows * w.cols, p = w.unit * SF_THREADS + (int)threadIdx.x;
        if (p - lane >= n) continue;                           // wave-uniform: the wave's 64 pixels lie past the map
        const bool in = p < n;
        const int r = in ? p / w.cols : 0, c = in ? p - r * w.cols : 0;
        for (int dir = 0; dir < 2; dir++) {
            const int32_t *other = a.contour[1 - dir] + w.pixels;
            const int32_t *there = a.presence + ((long long)(1 - dir) * a.batch + w.image) * a.classes;
            const int q = in ? a.contour[dir][w.pixels + p] : -1;
            unsigned res = SF_NOT_QUERY;
            for (unsigned long long pending = __ballot(q >= 0); pending; pending &= pending - 1) {
                const int src = __ffsll((long long)pending) - 1;
                const int cls = __shfl(q, src);
                int best = SF_NONE;
                if (there[cls]) best = sf_search(other, w.rows, w.cols, __shfl(r, src), __shfl(c, src), cls);
                if (lane == src) res = best == SF_NONE ? SF_UNMATCHED : (unsigned)best;
            }
            sf_accumulate(a, dir, q, res);
            if (dir == 0 && a.dist2 && in) a.dist2[w.off + p] = res;
        }
    }
}

int sf_call(mbn_surface *h, mbn_ragged_readout *r, SurfaceArgs &a, int shape, int truth_bytes, int batch, double span, double pixels, double units,
            void *stream)
{
    mbn_context *ctx = h->ctx;
    if (shape == MBN_EINVAL) return shape;
    if ((uintptr_t)a.surf % 8 || (uintptr_t)a.dist2 % 4 || (uintptr_t)a.labels % 4 || (truth_bytes == 4 && (uintptr_t)a.truth % 4)) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    if (batch > h->max_batch || pixels > (double)h->capacity || a.classes > h->max_classes) return MBN_EUNSUPPORTED;
    if (mbn_spans_overlap(a.dist2, 4.0 * span, a.labels, 4.0 * span) || mbn_spans_overlap(a.dist2, 4.0 * span, a.truth, span * truth_bytes))
        return MBN_EINVAL;
    const mbn_span sp[] = { { a.surf, 16.0 * a.classes * (MBN_SURFACE_HEAD + a.bins), "surface table" }, { a.labels, 4.0 * span, "surface labels" },
                        { a.truth, span * truth_bytes, "surface truth" }, { a.dist2, 4.0 * span, "surface dist2" } };
    const int rc = mbn_span_check(ctx, sp, (int)(sizeof sp / sizeof sp[0]));
    if (rc != MBN_OK) return rc;
    a.batch = batch;
    a.contour[0] = (int32_t *)h->scratch;
    a.contour[1] = a.contour[0] + h->capacity;
    a.presence = a.contour[1] + h->capacity;
    const int words = 2 * batch * a.classes;                   // <= 2 * 65535 * 4096 < 2^31
    const unsigned grid = mbn_persistent_grid(ctx->num_cus, SF_WGS_PER_CU, (long long)units);
    const unsigned clear_grid = mbn_persistent_grid(ctx->num_cus, SF_WGS_PER_CU, (words + SF_THREADS - 1) / SF_THREADS);
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    (void)hipSetDevice(ctx->device);
    hipLaunchKernelGGL(surface_clear, dim3(clear_grid), dim3(SF_THREADS), 0, s, a.presence, words);
    if (r) {
        if (truth_bytes == 4) hipLaunchKernelGGL((surface_contour<4, true>), dim3(grid), dim3(SF_THREADS), 0, s, a);
        else hipLaunchKernelGGL((surface_contour<1, true>), dim3(grid), dim3(SF_THREADS), 0, s, a);
        hipLaunchKernelGGL(surface_search<true>, dim3(grid), dim3(SF_THREADS), 0, s, a);
        mbn_ragged_readout_mark_done(r, s);
    } else {
        if (truth_bytes == 4) hipLaunchKernelGGL((surface_contour<4, false>), dim3(grid), dim3(SF_THREADS), 0, s, a);
        else hipLaunchKernelGGL((surface_contour<1, false>), dim3(grid), dim3(SF_THREADS), 0, s, a);
        hipLaunchKernelGGL(surface_search<false>, dim3(grid), dim3(SF_THREADS), 0, s, a);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MBN_OK : mbn_record_hip_error(ctx, e, "surface launch");
}

}   // namespace

extern "C" {

int mbn_surface_create(mbn_context *ctx, int max_batch, int64_t max_pixels, int max_classes, mbn_surface **h)
{
    if (!h) return MBN_EINVAL;
    *h = nullptr;
    if (max_classes < 1) return MBN_EINVAL;
    const int rc = mbn_scratch_create(ctx, max_batch, max_pixels, mbn_surface_scratch_bytes(max_batch, max_pixels, max_classes), h);
    if (rc == MBN_OK) (*h)->max_classes = max_classes;
    return rc;
}

int mbn_surface_destroy(mbn_surface *h) { return mbn_scratch_destroy(h); }

int mbn_surface_score_i32(mbn_surface *h, void *surf_u64, void *dist2_u32, const void *labels_i32, const void *truth, int truth_bytes, int classes,
                          int bins, int batch, int rows, int cols, int edge, void *stream)
{
    if (!h || !surf_u64 || !labels_i32 || !truth) return MBN_EINVAL;
    const int shape = mbn_surface_envelope(truth_bytes, classes, bins, batch, rows, cols, edge);
    SurfaceArgs a = {};
    a.surf = (unsigned long long *)surf_u64; a.dist2 = (unsigned *)dist2_u32;
    a.labels = (const int32_t *)labels_i32; a.truth = (const uint8_t *)truth;
    a.classes = classes; a.bins = bins; a.rows = rows; a.cols = cols; a.edge = edge;
    const double pixels = shape == MBN_OK ? (double)batch * rows * cols : 0.0;
    return sf_call(h, nullptr, a, shape, truth_bytes, batch, pixels, pixels, shape == MBN_OK ? (double)batch * (double)sf_units(rows, cols) : 0.0, stream);
}

int mbn_surface_score_ragged_i32(mbn_surface *h, mbn_ragged_readout *r, void *surf_u64, void *dist2_u32, const void *labels_i32, const void *truth,
                                 int truth_bytes, int classes, int bins, int edge, void *stream)
{
    if (!h || !r || r->ctx != h->ctx || r->batch <= 0 || !surf_u64 || !labels_i32 || !truth) return MBN_EINVAL;    // no set: no maps
    SurfaceArgs a = {};
    a.surf = (unsigned long long *)surf_u64; a.dist2 = (unsigned *)dist2_u32;
    a.labels = (const int32_t *)labels_i32; a.truth = (const uint8_t *)truth;
    a.classes = classes; a.bins = bins; a.edge = edge;
    a.set = mbn_ragged_readout_view(r);
    double pixels = 0.0, units = 0.0;
    const int shape = mbn_ragged_readout_envelope(r, [&](const mbn_label_item &it) {
        const int rc = mbn_surface_envelope(truth_bytes, classes, bins, r->batch, it.rows, it.cols, edge);
        if (rc == MBN_OK) {
            pixels += (double)it.rows * it.cols;
            units += (double)sf_units(it.rows, it.cols);
        }
        return rc;
    });
    return sf_call(h, r, a, shape, truth_bytes, r->batch, (double)r->launch.span, pixels, units, stream);
}

}   // extern "C"
