// mbn_i32_components.hip — regions of a label map on the device (gfx950): connected-component labelling of int32 label maps (mbn_components_i32
// and its ragged form; include/mbn.h, "regions of a label map"), with the C-ABI of the handle and the two calls.
//
// Block-based union-find whose root is the SMALLEST linear index of the set. parent [p] is an index inside p's own image (-1: abstained).
//   INVARIANT  parent [x] <= x at every moment, and parent [x] == x exactly for a root. A word is only ever changed by atomicMin (a union, on a
//              word that held a value <= its index) or, in the flatten kernel, replaced by the root of its own set, which is <= every member.
//              So `find` walks strictly downward and ends at a root after at most x steps; `unite` retries only with a pair whose larger member
//              is strictly smaller than before, so it ends too. The smallest index of a set can never be linked below itself: when the unions
//              are done it is the root, whatever order the atomics arrived in. That makes every output a function of the input alone.
// A call is seven kernels on one stream; order between phases comes from the kernel boundaries only. No workgroup ever waits for another: there is
// no look-back, no grid barrier, no flag. A word that another workgroup may change during the same kernel (parent in `seams` and `flatten`, area
// in `flatten`, a region's box in `write`) is read and written with agent-scope atomics only, never with a plain load.
//   1 tile     a workgroup takes a tile of TR x TC pixels into LDS. A wave holds one row of the tile (TC = 64 lanes): a ballot of the lanes whose left
//              neighbour differs gives every lane the start of its horizontal run, with no atomic at all. Then vertical (and, under connectivity 8,
//              diagonal) neighbours are united with LDS atomicMin; a pair whose left neighbours are the same pair is skipped, so a constant tile
//              costs TR unions, not TR * TC. Each pixel then finds its root and writes it as an image index; area is cleared.
//   2 seams    the pixels of a tile's first row, first column and (connectivity 8) last column unite with their earlier neighbours (left, up,
//              up-left, up-right) that lie in ANOTHER tile, in global memory. Every adjacent pair that crosses a tile border is such a pair
//              exactly once: the four tiles of a corner included.
//   3 flatten  every pixel finds its root and stores it; the area of each root is counted: the lanes of a wave that share a root add once.
//   4 count    per chunk of 1024 pixels: the roots with area >= min_area
//   5 scan     per image, one workgroup: the exclusive prefix sum of its chunks' counts, in place; the total is n_regions
//   6 number   per chunk: the rank of each surviving root in raster order; its record (label, area, first pixel; the box starts as the first pixel);
//              area [root] becomes the rank, or -1 for a dropped root
//   7 write    comp, labels_out, and the boxes: integer atomic min / max per region, once per wave and region and only where a bound can move
//              (min_row is the first pixel's row)
// The units of a kernel (tiles, chunks or images) are dealt round robin to a grid sized from the planning CU count.
#include "mbn_internal.h"
#include "mbn_label_set.h"

namespace {

constexpr int TR = MBN_COMPONENTS_TILE_ROWS, TC = MBN_COMPONENTS_TILE_COLS;
constexpr int CC_THREADS = 256, CC_WAVES = CC_THREADS / 64;
constexpr int CHUNK = MBN_COMPONENTS_CHUNK;
constexpr int CC_LEADERS = 16;            // distinct keys a wave aggregates per step; the lanes left over act on their own
constexpr int CC_WGS_PER_CU = 8;          // 32 waves and 8 x 16 KB of LDS on a CU
static_assert(TC == 64, "a wave holds one row of a tile");
static_assert(CHUNK == 4 * CC_THREADS, "four pixels per lane and chunk");

struct CcArgs {
    const int32_t *labels;
    int32_t *comp, *labels_out, *regions, *n_regions;
    int32_t *parent, *area, *chunk;           // the handle's scratch
    int batch, rows, cols;                    // uniform form
    mbn_label_set set;                        // ragged form: the view of the read-out handle's set
    long long tiles, chunks;                  // units of the whole call
    int classes, conn8, min_area, ignore_label, max_regions;
};

__host__ __device__ inline long long cc_tiles(int rows, int cols) { return (long long)((rows + TR - 1) / TR) * ((cols + TC - 1) / TC); }
__host__ __device__ inline long long cc_chunks(int rows, int cols) { return ((long long)rows * cols + CHUNK - 1) / CHUNK; }

// unit u of a kernel whose units are tiles, chunks (PER = cc_tiles, cc_chunks) or images. Uniform across the workgroup (u is). In Unit, off is
// the image's first element in labels / comp / labels_out, pixels that in parent / area, and sum that in chunk: the chunks of the images before it
using Unit = mbn_label_unit;
template <bool RAGGED, mbn_label_units_fn PER>
__device__ __forceinline__ bool cc_unit(const CcArgs &a, long long u, Unit &w)
{
    return mbn_label_set_unit<RAGGED, PER, cc_chunks>(a.set, a.batch, a.rows, a.cols, u, w);
}

// a label as the union-find sees it: itself inside [0, classes), else -1 (abstained: equal to no valid label)
__device__ __forceinline__ int cc_valid(int v, int classes) { return (unsigned)v < (unsigned)classes ? v : -1; }

// ---- union-find in LDS (one workgroup) and in global memory (any workgroup). The loops end by the INVARIANT at the top of the file.
__device__ __forceinline__ int lds_find(int *p, int x)
{
    for (;;) {
        const int q = __hip_atomic_load(&p[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);     // q <= x
        if (q == x) return x;
        x = q;                                                                                       // strictly downward
    }
}

__device__ __forceinline__ void lds_unite(int *p, int x, int y)
{
    for (;;) {
        x = lds_find(p, x);
        y = lds_find(p, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }                                                // x > y: the larger root goes below the smaller
        const int old = __hip_atomic_fetch_min(&p[x], y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == x) return;                                                                        // x was still a root: linked
        x = old;                                                                                     // x had been linked to old < x meanwhile: unite that with y
    }
}

__device__ __forceinline__ int g_find(int32_t *p, int x)
{
    for (;;) {
        const int q = __hip_atomic_load(&p[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         // q <= x
        if (q == x) return x;
        x = q;                                                                                       // strictly downward
    }
}

__device__ __forceinline__ void g_unite(int32_t *p, int x, int y)
{
    for (;;) {
        x = g_find(p, x);
        y = g_find(p, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }
        const int old = __hip_atomic_fetch_min(&p[x], y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == x) return;
        x = old;                                                                                     // old < x: the pair's larger member has shrunk
    }
}

// exclusive prefix sum of v over the workgroup in lane order, and the workgroup's total in every lane. s_w: CC_WAVES ints of LDS
__device__ __forceinline__ int block_scan(int v, int *s_w, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                                                                 // the previous use of s_w is over
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < CC_WAVES; w++) {
        const int t = s_w[w];
        if (w < wave) before += t;
        total += t;
    }
    return before + inc - v;
}

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

// ------------------------------------------------------------------------------------------------------------------------- 1 tile
template <bool RAGGED>
__global__ __launch_bounds__(CC_THREADS) void cc_tile(const CcArgs a)
{
    __shared__ int s_lab[TR * TC], s_par[TR * TC];
    if (RAGGED && mbn_label_set_stale(a.set)) return;                  // captured under an earlier set: nothing to do
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long u = blockIdx.x; u < a.tiles; u += gridDim.x) {
        Unit w;
        if (!cc_unit<RAGGED, cc_tiles>(a, u, w)) break;
        const int tiles_x = (w.cols + TC - 1) / TC;
        const int r0 = w.unit / tiles_x * TR, c0 = w.unit % tiles_x * TC;
        const int32_t *lab = a.labels + w.off;
        // horizontal runs: every lane of a run points at the run's first lane
        for (int rr = wave; rr < TR; rr += CC_WAVES) {
            const int r = r0 + rr, c = c0 + lane;
            int l = -1;
            if (r < w.rows && c < w.cols) l = cc_valid(lab[r * w.cols + c], a.classes);
            const int left = __shfl_up(l, 1);
            const unsigned long long starts = __ballot(lane == 0 || left != l);            // bit 0 is always set
            const int start = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane))));
            s_lab[rr * TC + lane] = l;
            s_par[rr * TC + lane] = l >= 0 ? rr * TC + start : -1;
        }
        __syncthreads();
        // vertical and diagonal neighbours of the row above. A pair (pixel, up) whose left neighbours are the same kind of pair is united there
        for (int rr = wave; rr < TR; rr += CC_WAVES) {
            if (rr == 0) continue;
            const int i = rr * TC + lane, l = s_lab[i];
            if (l < 0) continue;
            if (s_lab[i - TC] == l) {
                if (!(lane > 0 && s_lab[i - 1] == l && s_lab[i - TC - 1] == l)) lds_unite(s_par, i, i - TC);
            } else if (a.conn8) {                                                          // up == l joins both diagonals through the row above
                if (lane > 0 && s_lab[i - TC - 1] == l) lds_unite(s_par, i, i - TC - 1);
                if (lane < TC - 1 && s_lab[i - TC + 1] == l) lds_unite(s_par, i, i - TC + 1);
            }
        }
        __syncthreads();
        // nothing changes s_par from here on: each pixel's root, as an index of its image. The smallest index of the tile's part is the smallest there too
        for (int rr = wave; rr < TR; rr += CC_WAVES) {
            const int r = r0 + rr, c = c0 + lane;
            if (r >= w.rows || c >= w.cols) continue;
            const int i = rr * TC + lane;
            int root = -1;
            if (s_lab[i] >= 0) {
                const int t = lds_find(s_par, i);
                root = (r0 + t / TC) * w.cols + c0 + t % TC;
            }
            a.parent[w.pixels + r * w.cols + c] = root;
            a.area[w.pixels + r * w.cols + c] = 0;
        }
        __syncthreads();                                                                   // the next tile overwrites the LDS
    }
}

// ------------------------------------------------------------------------------------------------------------------------ 2 seams
template <bool RAGGED>
__global__ __launch_bounds__(CC_THREADS) void cc_seams(const CcArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const int t = threadIdx.x;
    // the pixel of this lane: first row (64), first column below it (31), last column below the first row (31, connectivity 8 only)
    int rr = 0, cc = 0;
    bool mine = true;
    if (t < TC) cc = t;
    else if (t < TC + TR) { rr = t - TC; mine = rr > 0; }
    else if (t < TC + 2 * TR) { rr = t - TC - TR; cc = TC - 1; mine = rr > 0 && a.conn8; }
    else mine = false;
    if (!mine) return;                                                                     // no barrier and no wave operation below
    for (long long u = blockIdx.x; u < a.tiles; u += gridDim.x) {
        Unit w;
        if (!cc_unit<RAGGED, cc_tiles>(a, u, w)) break;
        const int tiles_x = (w.cols + TC - 1) / TC;
        const int r = w.unit / tiles_x * TR + rr, c = w.unit % tiles_x * TC + cc, cols = w.cols;
        if (r >= w.rows || c >= cols) continue;
        const int32_t *lab = a.labels + w.off;
        int32_t *par = a.parent + w.pixels;
        const int p = r * cols + c;
        const int l = cc_valid(lab[p], a.classes);
        if (l < 0) continue;
        const bool has_up = r > 0, has_left = c > 0, has_right = c + 1 < cols;
        const bool up = has_up && cc_valid(lab[p - cols], a.classes) == l;
        const bool left = has_left && cc_valid(lab[p - 1], a.classes) == l;
        const bool upleft = has_up && has_left && cc_valid(lab[p - cols - 1], a.classes) == l;
        // up crosses a border iff this is the tile's first row. Skipped when the left neighbours are the same kind of pair inside the same two tiles:
        // they are united by the lane to the left, and each row's run is already one set
        if (up && rr == 0 && !(cc > 0 && left && upleft)) g_unite(par, p, p - cols);
        // left crosses iff this is the tile's first column; skipped likewise when the pair above is the same kind of pair
        if (left && cc == 0 && !(rr > 0 && up && upleft)) g_unite(par, p, p - 1);
        if (a.conn8) {
            // a diagonal matters only where no edge neighbour joins the two: up or left == l join up-left, up == l joins up-right
            if (upleft && (rr == 0 || cc == 0) && !up && !left) g_unite(par, p, p - cols - 1);
            if (has_up && has_right && (rr == 0 || cc == TC - 1) && !up && cc_valid(lab[p - cols + 1], a.classes) == l) g_unite(par, p, p - cols + 1);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------- 3 flatten
template <bool RAGGED>
__global__ __launch_bounds__(CC_THREADS) void cc_flatten(const CcArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const int lane = threadIdx.x & 63;
    for (long long u = blockIdx.x; u < a.chunks; u += gridDim.x) {
        Unit w;
        if (!cc_unit<RAGGED, cc_chunks>(a, u, w)) break;
        const int n = w.rows * w.cols;
        int32_t *par = a.parent + w.pixels, *area = a.area + w.pixels;
        for (int j = 0; j < CHUNK / CC_THREADS; j++) {                                     // a wave holds 64 consecutive pixels
            const int p = w.unit * CHUNK + j * CC_THREADS + (int)threadIdx.x;
            int root = -1;
            if (p < n && __hip_atomic_load(&par[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0) {
                root = g_find(par, p);
                // another workgroup's find may read this word meanwhile: before or after, it leads to the same root
                __hip_atomic_store(&par[p], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            // the lanes that share a root add once. Every lane of the wave runs this loop (the ballots are wave-uniform)
            bool pending = root >= 0;
            for (int it = 0; it < CC_LEADERS; it++) {
                const unsigned long long left = __ballot(pending);
                if (!left) break;
                const int first = __ffsll((long long)left) - 1;
                const int lead = __shfl(root, first);
                const bool same = pending && root == lead;
                const unsigned long long m = __ballot(same);
                if (lane == first) (void)__hip_atomic_fetch_add(&area[lead], (int)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (same) pending = false;
            }
            if (pending) (void)__hip_atomic_fetch_add(&area[root], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// a surviving root: nothing writes parent or area during the kernels that ask (count and number read area [p] before number replaces it)
__device__ __forceinline__ bool cc_survivor(const int32_t *par, const int32_t *area, int p, int n, int min_area)
{
    return p < n && par[p] == p && area[p] >= min_area;
}

// ------------------------------------------------------------------------------------------------------------------------ 4 count
template <bool RAGGED>
__global__ __launch_bounds__(CC_THREADS) void cc_count(const CcArgs a)
{
    __shared__ int s_w[CC_WAVES];
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    for (long long u = blockIdx.x; u < a.chunks; u += gridDim.x) {
        Unit w;
        if (!cc_unit<RAGGED, cc_chunks>(a, u, w)) break;
        const int n = w.rows * w.cols;
        const int32_t *par = a.parent + w.pixels, *area = a.area + w.pixels;
        int v = 0;
        for (int j = 0; j < 4; j++) v += cc_survivor(par, area, w.unit * CHUNK + 4 * (int)threadIdx.x + j, n, a.min_area);
        int total;
        (void)block_scan(v, s_w, total);
        if (threadIdx.x == 0) a.chunk[w.sum + w.unit] = total;
    }
}

// ------------------------------------------------------------------------------------------------------------------------- 5 scan
template <bool RAGGED>
__global__ __launch_bounds__(CC_THREADS) void cc_scan(const CcArgs a)
{
    __shared__ int s_w[CC_WAVES];
    int batch = a.batch;
    if (RAGGED) {
        if (mbn_label_set_stale(a.set)) return;
        batch = a.set.head->batch;
    }
    for (long long u = blockIdx.x; u < batch; u += gridDim.x) {
        Unit w;
        if (!cc_unit<RAGGED, mbn_label_units_image>(a, u, w)) break;
        const int chunks = (int)cc_chunks(w.rows, w.cols);
        int32_t *cnt = a.chunk + w.sum;
        int running = 0;                                                                   // the same in every lane
        for (int base = 0; base < chunks; base += CC_THREADS) {
            const int i = base + (int)threadIdx.x;
            const int v = i < chunks ? cnt[i] : 0;
            int total;
            const int before = block_scan(v, s_w, total);
            if (i < chunks) cnt[i] = running + before;
            running += total;
        }
        if (threadIdx.x == 0) a.n_regions[w.image] = running;
    }
}

// ----------------------------------------------------------------------------------------------------------------------- 6 number
template <bool RAGGED>
__global__ __launch_bounds__(CC_THREADS) void cc_number(const CcArgs a)
{
    __shared__ int s_w[CC_WAVES];
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    for (long long u = blockIdx.x; u < a.chunks; u += gridDim.x) {
        Unit w;
        if (!cc_unit<RAGGED, cc_chunks>(a, u, w)) break;
        const int n = w.rows * w.cols;
        const int32_t *par = a.parent + w.pixels;
        int32_t *area = a.area + w.pixels;
        const int p0 = w.unit * CHUNK + 4 * (int)threadIdx.x;
        bool keep[4];
        int v = 0;
        for (int j = 0; j < 4; j++) {
            keep[j] = cc_survivor(par, area, p0 + j, n, a.min_area);
            v += keep[j];
        }
        int total;
        int rank = a.chunk[w.sum + w.unit] + block_scan(v, s_w, total);
        for (int j = 0; j < 4; j++) {
            const int p = p0 + j;
            if (keep[j]) {
                if (rank < a.max_regions) {
                    int32_t *rec = a.regions + ((long long)w.image * a.max_regions + rank) * 8;
                    const int r = p / w.cols, c = p - r * w.cols;
                    rec[0] = a.labels[w.off + p];
                    rec[1] = area[p];
                    rec[2] = r; rec[3] = c;
                    rec[4] = r; rec[5] = c; rec[6] = r; rec[7] = c;
                }
                area[p] = rank++;                                                          // each root belongs to one lane
            } else if (p < n && par[p] == p) {
                area[p] = -1;                                                              // a dropped root
            }
        }
    }
}

// A region's box only grows: min_col falls, max_row and max_col rise. A value that cannot move a bound needs no atomic. The bound is read with an
// atomic load and may already be older than the word: it is then further in than the word, so an atomic may be issued needlessly but is never
// skipped wrongly. On a large region all but the first waves of a row skip all three
__device__ __forceinline__ void box_grow(int32_t *rec, int cmin, int rmax, int cmax)
{
    if (cmin < __hip_atomic_load(&rec[5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)__hip_atomic_fetch_min(&rec[5], cmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (rmax > __hip_atomic_load(&rec[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)__hip_atomic_fetch_max(&rec[6], rmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cmax > __hip_atomic_load(&rec[7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        (void)__hip_atomic_fetch_max(&rec[7], cmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------------------------------ 7 write
template <bool RAGGED>
__global__ __launch_bounds__(CC_THREADS) void cc_write(const CcArgs a)
{
    if (RAGGED && mbn_label_set_stale(a.set)) return;
    const int lane = threadIdx.x & 63;
    for (long long u = blockIdx.x; u < a.chunks; u += gridDim.x) {
        Unit w;
        if (!cc_unit<RAGGED, cc_chunks>(a, u, w)) break;
        const int n = w.rows * w.cols;
        const int32_t *par = a.parent + w.pixels, *rank_of = a.area + w.pixels;
        for (int j = 0; j < CHUNK / CC_THREADS; j++) {                                     // a wave holds 64 consecutive pixels
            const int p = w.unit * CHUNK + j * CC_THREADS + (int)threadIdx.x;
            int rank = -1, r = 0, c = 0;
            if (p < n) {
                const int root = par[p];
                if (root >= 0) rank = rank_of[root];
                if (a.comp) a.comp[w.off + p] = rank;
                if (a.labels_out) a.labels_out[w.off + p] = root >= 0 && rank < 0 ? a.ignore_label : a.labels[w.off + p];
                r = p / w.cols;
                c = p - r * w.cols;
            }
            // the boxes of the regions in the table: per wave and region one lane brings the extremes. The rows of a wave's pixels ascend with the lane;
            // min_row is the first pixel's row and already there. Every lane of the wave runs this loop
            bool pending = rank >= 0 && rank < a.max_regions;
            for (int it = 0; it < CC_LEADERS; it++) {
                const unsigned long long left = __ballot(pending);
                if (!left) break;
                const int first = __ffsll((long long)left) - 1;
                const int lead = __shfl(rank, first);
                const bool same = pending && rank == lead;
                const unsigned long long m = __ballot(same);
                const int cmin = wave_min(same ? c : 0x7fffffff), cmax = wave_max(same ? c : -1);
                const int rmax = __shfl(r, 63 - __clzll((long long)m));
                if (lane == first) box_grow(a.regions + ((long long)w.image * a.max_regions + lead) * 8, cmin, rmax, cmax);
                if (same) pending = false;
            }
            if (pending) box_grow(a.regions + ((long long)w.image * a.max_regions + rank) * 8, c, r, c);
        }
    }
}

template <bool RAGGED>
void cc_launch(mbn_context *ctx, hipStream_t s, const CcArgs &a, int batch)
{
    const dim3 block(CC_THREADS);
    const auto grid = [ctx](long long units) { return mbn_persistent_grid(ctx->num_cus, CC_WGS_PER_CU, units); };
    hipLaunchKernelGGL(cc_tile<RAGGED>, dim3(grid(a.tiles)), block, 0, s, a);
    hipLaunchKernelGGL(cc_seams<RAGGED>, dim3(grid(a.tiles)), block, 0, s, a);
    hipLaunchKernelGGL(cc_flatten<RAGGED>, dim3(grid(a.chunks)), block, 0, s, a);
    hipLaunchKernelGGL(cc_count<RAGGED>, dim3(grid(a.chunks)), block, 0, s, a);
    hipLaunchKernelGGL(cc_scan<RAGGED>, dim3(grid(batch)), block, 0, s, a);
    hipLaunchKernelGGL(cc_number<RAGGED>, dim3(grid(a.chunks)), block, 0, s, a);
    hipLaunchKernelGGL(cc_write<RAGGED>, dim3(grid(a.chunks)), block, 0, s, a);
}

// What the two calls share once the shape is known: `shape` = the envelope's answer, `span` = the elements of the maps, `pixels` = those inside maps
int cc_call(mbn_components *h, mbn_ragged_readout *r, CcArgs &a, int shape, int batch, double span, double pixels, void *stream)
{
    mbn_context *ctx = h->ctx;
    if (shape == MBN_EINVAL) return shape;
    if (!a.regions && a.max_regions > 0) return MBN_EINVAL;
    if ((uintptr_t)a.labels % 4 || (uintptr_t)a.comp % 4 || (uintptr_t)a.labels_out % 4 || (uintptr_t)a.regions % 4 || (uintptr_t)a.n_regions % 4)
        return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    if (batch > h->max_batch || pixels > (double)h->capacity) return MBN_EINVAL;
    const double map_bytes = 4.0 * span;
    if (mbn_spans_overlap(a.labels, map_bytes, a.labels_out, map_bytes) || mbn_spans_overlap(a.labels, map_bytes, a.comp, map_bytes)) return MBN_EINVAL;
    const mbn_span sp[] = { { a.labels, 4.0 * span, "components labels" }, { a.comp, 4.0 * span, "components comp" },
                        { a.labels_out, 4.0 * span, "components labels_out" },
                        { a.regions, 32.0 * batch * a.max_regions, "components regions" }, { a.n_regions, 4.0 * batch, "components n_regions" } };
    const int rc = mbn_span_check(ctx, sp, (int)(sizeof sp / sizeof sp[0]));
    if (rc != MBN_OK) return rc;
    a.parent = (int32_t *)h->scratch;
    a.area = a.parent + h->capacity;
    a.chunk = a.area + h->capacity;
    hipStream_t s = stream ? (hipStream_t)stream : ctx->stream;
    (void)hipSetDevice(ctx->device);
    if (r) {
        cc_launch<true>(ctx, s, a, batch);
        mbn_ragged_readout_mark_done(r, s);
    } else {
        cc_launch<false>(ctx, s, a, batch);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MBN_OK : mbn_record_hip_error(ctx, e, "components launch");
}

}   // namespace

extern "C" {

int mbn_components_create(mbn_context *ctx, int max_batch, int64_t max_pixels, mbn_components **h)
{
    return mbn_scratch_create(ctx, max_batch, max_pixels, mbn_components_scratch_bytes(max_batch, max_pixels), h);
}

int mbn_components_destroy(mbn_components *h) { return mbn_scratch_destroy(h); }

int mbn_components_i32(mbn_components *h, void *comp_i32, mbn_region *regions, void *n_regions_i32, void *labels_out_i32, const void *labels_i32,
                       int batch, int rows, int cols, int classes, int connectivity, int min_area, int ignore_label, int max_regions, void *stream)
{
    if (!h || !labels_i32 || !n_regions_i32) return MBN_EINVAL;
    const int shape = mbn_components_envelope(batch, rows, cols, classes, connectivity, min_area, max_regions);
    CcArgs a = {};
    a.labels = (const int32_t *)labels_i32;
    a.comp = (int32_t *)comp_i32; a.labels_out = (int32_t *)labels_out_i32; a.regions = (int32_t *)regions; a.n_regions = (int32_t *)n_regions_i32;
    a.classes = classes; a.conn8 = connectivity == 8; a.min_area = min_area; a.ignore_label = ignore_label; a.max_regions = max_regions;
    double pixels = 0.0;
    if (shape == MBN_OK) {
        a.batch = batch; a.rows = rows; a.cols = cols;
        a.tiles = batch * cc_tiles(rows, cols);
        a.chunks = batch * cc_chunks(rows, cols);
        pixels = (double)batch * rows * cols;
    }
    return cc_call(h, nullptr, a, shape, batch, pixels, pixels, stream);
}

int mbn_components_ragged_i32(mbn_components *h, mbn_ragged_readout *r, void *comp_i32, mbn_region *regions, void *n_regions_i32,
                              void *labels_out_i32, const void *labels_i32, int classes, int connectivity, int min_area, int ignore_label,
                              int max_regions, void *stream)
{
    if (!h || !r || r->ctx != h->ctx || r->batch <= 0 || !labels_i32 || !n_regions_i32) return MBN_EINVAL;   // no set: nothing to label
    CcArgs a = {};
    a.labels = (const int32_t *)labels_i32;
    a.comp = (int32_t *)comp_i32; a.labels_out = (int32_t *)labels_out_i32; a.regions = (int32_t *)regions; a.n_regions = (int32_t *)n_regions_i32;
    a.classes = classes; a.conn8 = connectivity == 8; a.min_area = min_area; a.ignore_label = ignore_label; a.max_regions = max_regions;
    a.set = mbn_ragged_readout_view(r);
    // the items of the last set, as the handle's pinned block still holds them: every map inside the envelope, and the units of the call
    double pixels = 0.0;
    const int shape = mbn_ragged_readout_envelope(r, [&](const mbn_label_item &it) {
        const int rc = mbn_components_envelope(r->batch, it.rows, it.cols, classes, connectivity, min_area, max_regions);
        if (rc == MBN_OK) {
            a.tiles += cc_tiles(it.rows, it.cols);
            a.chunks += cc_chunks(it.rows, it.cols);
            pixels += (double)it.rows * it.cols;
        }
        return rc;
    });
    return cc_call(h, r, a, shape, r->batch, (double)r->launch.span, pixels, stream);
}

}   // extern "C"
