// mbn_i32_boundary.hip — score a segmentation at its boundaries on the device (gfx950): the DEPTH of every pixel of a label map (its Chebyshev
// distance to the nearest pixel of another value, capped at d + 1), and from the depths of truth and prediction the trimap confusion matrix and
// the boundary-IoU counts (mbn_boundary_depth, mbn_boundary_score_i32 and their ragged forms; include/mbn.h, "score a segmentation at its
// boundaries"). The arithmetic is integer, so the result does not depend on the order in which the atomics arrive, nor on the grid.
//
// One TILE BODY serves all kernels. A tile is TR x 64 pixels of one map (TR = 32 for the half-width class d <= 16, 64 above); a workgroup of
// four waves owns it.
//   ROW PASS    for every map row of the tile and of the d rows above and below it, one wave reads the columns of the tile and d on each side (two
//               or three 64-lane words). A ballot MARKS column x where L (x) != L (x - 1), and under `edge` x = 0 and x = cols (the frame).
//               The first mark to the right of column c is the first pixel that differs from L (c); the last mark at or left of c is one past
//               the nearest differing pixel on the left. So h (c), the horizontal distance to the nearest differing pixel, is a count of
//               trailing / leading zeros in a 64-bit window of the mark words: no loop over d. The wave stores the value (int32, a uint8
//               zero-extended) and h (one byte, capped at d + 1) of the tile's 64 columns to LDS: (TR + 2 d) x 64 x 5 bytes per map.
//   COLUMN PASS a lane owns a column. D = h of the pixel itself; for k = 1 .. while k < D: the pixel k rows above and the one k rows below give
//               max (k, same value ? h there : 0), a row outside the map gives k under `edge` and nothing otherwise. The loop ends as soon as k
//               reaches the minimum so far, so band pixels next to a contour cost a step or two and only deep interior pixels walk all d rows.
// LDS reads of the column pass are 64 consecutive dwords or bytes per wave: no bank conflict.
//
// The score kernel runs the row pass for truth and labels into two such images, then forms both depths per pixel in registers: they never reach
// memory. Only band pixels count. Each of the four adds (the trimap cell, and the three biou columns) goes through a WAVE ELECTION as in
// mbn_i32_confusion.hip: the lanes that hold the same cell elect a leader which adds their number once, up to BD_LEADERS distinct cells per
// wave and row; lanes left over add on their own. Up to MBN_BOUNDARY_LDS_CLASSES classes the adds of a tile go to 32-bit bins in LDS and the
// non-zero bins to the tables with 64-bit global atomics after the tile; above, every add is a 64-bit global atomic (many cells, little contention).
//
// The grid is persistent: num_cus * (workgroups per CU by LDS) workgroups; workgroup b takes the tiles k with (k + rot) % grid == b, rot = the tiles
// of the maps before. No workgroup waits for another. Indices inside a map are below 2^29 (the envelope); a map's element offset is 64-bit.
#include "mbn_internal.h"
#include "mbn_label_set.h"

#include <mutex>

namespace {

constexpr int BD_WAVES = 4;
constexpr int BD_THREADS = 64 * BD_WAVES;
constexpr int BD_TC = MBN_BOUNDARY_TILE_COLS;          // one lane per column
constexpr int BD_LEADERS = 16;                         // distinct cells a wave aggregates per add; the lanes left over add on their own
static_assert(BD_TC == 64, "a lane per tile column");

template <int HW>
struct Geo {
    static constexpr int TR = HW <= MBN_BOUNDARY_SMALL_D ? MBN_BOUNDARY_SMALL_ROWS : MBN_BOUNDARY_LARGE_ROWS;
    static constexpr int NW = (BD_TC + 2 * HW + 63) / 64;          // 64-lane words of a row's window: the tile's columns and HW on each side
};

struct BoundaryArgs {
    unsigned long long *trimap, *biou;     // score: either may be null
    uint8_t *depth;                        // depth
    const uint8_t *map;                    // depth: the map (uint8 or int32); score: the truth
    const int32_t *labels;                 // score
    int classes, batch, rows, cols;        // uniform form
    int d, edge;
    int lds_form;                          // score: a workgroup counts a tile in LDS bins (classes <= MBN_BOUNDARY_LDS_CLASSES)
    const int32_t *d_items;                // ragged form: per-item half-widths or null
    mbn_label_set set;                     // ragged form: the view of the handle's set
};

template <int EB>
__device__ __forceinline__ int load_value(const uint8_t *map, long long i)
{
    return EB == 1 ? (int)map[i] : ((const int32_t *)map)[i];
}

__device__ __forceinline__ unsigned long long funnel(unsigned long long lo, unsigned long long hi, int sh)
{
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// ROW PASS of one map over the rows [r0 - d, r0 + TR + d) that lie inside it: s_val [rr][lane], s_h [rr][lane] for rr = row - (r0 - d).
// `map` is element 0 of this map; every index read is inside [0, rows * cols)
template <int EB, int HW>
__device__ __forceinline__ void row_pass(const uint8_t *map, int rows, int cols, int r0, int c0, int d, int edge, int32_t *s_val, uint8_t *s_h)
{
    constexpr int TR = Geo<HW>::TR, NW = Geo<HW>::NW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int window = BD_TC + 2 * d;                      // window position j is column c0 - d + j
    for (int rr = wave; rr < TR + 2 * d; rr += BD_WAVES) {
        const int r = r0 - d + rr;
        if (r < 0 || r >= rows) continue;                  // wave-uniform
        const long long row = (long long)r * cols;
        unsigned long long p[NW + 3];                      // the mark words behind one zero word and in front of two
        p[0] = 0; p[NW + 1] = 0; p[NW + 2] = 0;
        int mine = 0, before = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const int j = 64 * w + lane, x = c0 - d + j;
            int v = 0;
            if (j < window && x >= 0 && x < cols) v = load_value<EB>(map, row + x);
            int left = __shfl_up(v, 1);
            const int last = __shfl(before, 63);           // the word before's last lane
            if (lane == 0) left = last;
            bool mark = false;
            if (j >= 1 && j < window) {
                if (x > 0 && x < cols) mark = v != left;   // x - 1 is inside the map and inside the window: loaded
                else if (x == 0 || x == cols) mark = edge != 0;
            }
            p[1 + w] = __ballot(mark);
            before = v;
            const int got = __shfl(v, (d + lane) & 63);    // the lane's own column sits at window position d + lane
            if (((d + lane) >> 6) == w) mine = got;
        }
        // bit 63 of `lw` is the lane's own position, bit 0 of `rw` the one right of it
        const int at = d + lane + 1, wi = at >> 6, sh = at & 63;
        unsigned long long a = 0, b = 0, c = 0;
#pragma unroll
        for (int k = 0; k <= NW; k++)
            if (wi == k) { a = p[k]; b = p[k + 1]; c = p[k + 2]; }
        const unsigned long long lw = funnel(a, b, sh), rw = funnel(b, c, sh);
        int h = d + 1;
        if (lw) h = min(h, __clzll((long long)lw) + 1);
        if (rw) h = min(h, __ffsll((long long)rw));
        s_val[rr * BD_TC + lane] = mine;
        s_h[rr * BD_TC + lane] = (uint8_t)h;
    }
}

// COLUMN PASS for the pixel of tile row i (map row r) in the lane's column: min (D, d + 1)
__device__ __forceinline__ int column_depth(const int32_t *s_val, const uint8_t *s_h, int i, int r, int rows, int d, int edge)
{
    const int at = (i + d) * BD_TC + (threadIdx.x & 63);
    const int v = s_val[at];
    int depth = s_h[at];
    for (int k = 1; k < depth; k++) {                      // depth <= d + 1: k <= d, rows i + d - k and i + d + k are in the image
        int up = depth, down = depth;
        if (r - k < 0) {
            if (edge) up = k;
        } else {
            const int o = at - k * BD_TC;
            up = s_val[o] == v ? max(k, (int)s_h[o]) : k;
        }
        if (r + k >= rows) {
            if (edge) down = k;
        } else {
            const int o = at + k * BD_TC;
            down = s_val[o] == v ? max(k, (int)s_h[o]) : k;
        }
        depth = min(depth, min(up, down));
    }
    return depth;
}

__device__ __forceinline__ int bd_clamp(int v, int classes) { return (unsigned)v < (unsigned)classes ? v : classes; }

// One add of w to a cell: of the workgroup's LDS bins (the LDS form: `bins` non-null, the cell's bin is base + cell) or of the table in memory
__device__ __forceinline__ void cell_add(unsigned *bins, int base, unsigned long long *table, int cell, unsigned w)
{
    if (bins) (void)__hip_atomic_fetch_add(&bins[base + cell], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else (void)__hip_atomic_fetch_add(&table[cell], (unsigned long long)w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// table [cell] += the number of active lanes that hold `cell`; every lane of the wave calls it
__device__ __forceinline__ void elect_add(unsigned *bins, int base, unsigned long long *table, int cell, bool active)
{
    const int lane = threadIdx.x & 63;
    unsigned long long pending = __ballot(active);
    for (int it = 0; it < BD_LEADERS && pending; it++) {   // wave-uniform
        const int src = __ffsll((long long)pending) - 1;
        const int lead = __shfl(cell, src);
        const bool same = active && cell == lead;
        const unsigned long long m = __ballot(same);
        if (lane == src) cell_add(bins, base, table, lead, (unsigned)__popcll(m));
        if (same) active = false;
        pending &= ~m;
    }
    if (active) cell_add(bins, base, table, cell, 1u);
}

// one map of the call: its element offset, size and half-width
struct Item {
    long long off;
    int rows, cols, d;
};

template <bool RAGGED>
__device__ __forceinline__ Item item_of(const BoundaryArgs &a, int i)
{
    Item m;
    if (RAGGED) {
        const mbn_label_item *it = mbn_label_set_item(a.set, i);
        m.off = it->dst_offset;
        m.rows = it->rows;
        m.cols = it->cols;
        m.d = a.d_items ? min(max(a.d_items[i], 1), MBN_BOUNDARY_MAX_D) : a.d;
    } else {
        m.off = (long long)i * a.rows * a.cols;
        m.rows = a.rows;
        m.cols = a.cols;
        m.d = a.d;
    }
    return m;
}

// SCORE = false: depth_u8 of a.map (EB bytes an element). SCORE = true: the tables of a.labels against a.map (the truth, EB bytes an element).
// Dynamic LDS: (score) MBN_BOUNDARY_TABLE_BYTES of 32-bit bins, then per map image (TR + 2 d) x 64 values, then as many bytes of h; d = the largest
// half-width of the call. The LDS form (a.lds_form: classes <= MBN_BOUNDARY_LDS_CLASSES) counts a tile in the bins, (classes + 1)^2 of the trimap
// and 3 * classes of biou, and adds the non-zero ones to the tables after the tile's last barrier: a bin holds at most a tile's 4096 pixels
template <int EB, int HW, bool RAGGED, bool SCORE>
__global__ __launch_bounds__(BD_THREADS) void boundary_i32(const BoundaryArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int32_t s_lds[];
    constexpr int TR = Geo<HW>::TR, MAPS = SCORE ? 2 : 1, TABLE = SCORE ? MBN_BOUNDARY_TABLE_BYTES / 4 : 0;
    unsigned *const s_bins = SCORE && a.lds_form ? (unsigned *)s_lds : nullptr;
    const int tri_cells = (a.classes + 1) * (a.classes + 1), bins = tri_cells + 3 * a.classes;
    int batch = a.batch;
    if (RAGGED) {
        if (mbn_label_set_stale(a.set)) return;            // captured under an earlier set: nothing to do
        batch = a.set.head->batch;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned G = gridDim.x, b = blockIdx.x;
    unsigned rot = 0;
    if (s_bins)
        for (int i = threadIdx.x; i < bins; i += BD_THREADS) s_bins[i] = 0;     // the first tile's barrier stands between this and the first add
    for (int n = 0; n < batch; n++) {
        const Item m = item_of<RAGGED>(a, n);
        const int d = min(m.d, HW);                        // the launcher chose HW >= every half-width of the call
        const int image = (TR + 2 * d) * BD_TC;
        int32_t *s_val = s_lds + TABLE;
        uint8_t *s_h = (uint8_t *)(s_val + MAPS * image);
        const int across = (m.cols + BD_TC - 1) / BD_TC, tiles = ((m.rows + TR - 1) / TR) * across;
        for (int k = (int)((b + G - rot) % G); k < tiles; k += (int)G) {
            const int r0 = (k / across) * TR, c0 = (k % across) * BD_TC;
            row_pass<EB, HW>(a.map + m.off * EB, m.rows, m.cols, r0, c0, d, a.edge, s_val, s_h);
            if (SCORE) row_pass<4, HW>((const uint8_t *)(a.labels + m.off), m.rows, m.cols, r0, c0, d, a.edge, s_val + image, s_h + image);
            __syncthreads();
            const int c = c0 + lane;
            for (int i = wave; i < TR; i += BD_WAVES) {    // wave-uniform
                const int r = r0 + i;
                if (r >= m.rows) break;
                const bool in = c < m.cols;
                if (!SCORE) {
                    if (in) a.depth[m.off + (long long)r * m.cols + c] = (uint8_t)column_depth(s_val, s_h, i, r, m.rows, d, a.edge);
                } else {
                    int t = 0, p = 0;
                    bool tb = false, pb = false;
                    if (in) {
                        t = s_val[(i + d) * BD_TC + lane];
                        p = s_val[image + (i + d) * BD_TC + lane];
                        tb = column_depth(s_val, s_h, i, r, m.rows, d, a.edge) <= d;
                        pb = column_depth(s_val + image, s_h + image, i, r, m.rows, d, a.edge) <= d;
                    }
                    const int C = a.classes;
                    const bool tv = (unsigned)t < (unsigned)C, pv = (unsigned)p < (unsigned)C;
                    if (a.trimap) elect_add(s_bins, 0, a.trimap, bd_clamp(t, C) * (C + 1) + bd_clamp(p, C), tb);
                    if (a.biou) {
                        const int tc = 3 * bd_clamp(t, C), pc = 3 * bd_clamp(p, C);       // an inactive lane's cell is never added to
                        elect_add(s_bins, tri_cells, a.biou, tc, tb && tv);
                        elect_add(s_bins, tri_cells, a.biou, pc + 1, pb && pv && tv);
                        elect_add(s_bins, tri_cells, a.biou, tc + 2, tb && pb && tv && t == p);
                    }
                }
            }
            __syncthreads();                               // the next tile's row pass overwrites the images; every add of this tile is in the bins
            if (s_bins) {
                // a non-zero bin belongs to a table that was given; the next tile's adds come behind its own barrier
                for (int i = threadIdx.x; i < bins; i += BD_THREADS) {
                    const unsigned v = s_bins[i];
                    if (v) {
                        unsigned long long *cell = i < tri_cells ? a.trimap + i : a.biou + (i - tri_cells);
                        (void)__hip_atomic_fetch_add(cell, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        s_bins[i] = 0;
                    }
                }
            }
        }
        rot = (rot + (unsigned)tiles % G) % G;
    }
}

using Kernel = void (*)(const BoundaryArgs);
// by [score][ragged][large half-width][4-byte elements]
const Kernel bd_kernels[2][2][2][2] = {
    { { { boundary_i32<1, 16, false, false>, boundary_i32<4, 16, false, false> }, { boundary_i32<1, 64, false, false>, boundary_i32<4, 64, false, false> } },
      { { boundary_i32<1, 16, true, false>, boundary_i32<4, 16, true, false> }, { boundary_i32<1, 64, true, false>, boundary_i32<4, 64, true, false> } } },
    { { { boundary_i32<1, 16, false, true>, boundary_i32<4, 16, false, true> }, { boundary_i32<1, 64, false, true>, boundary_i32<4, 64, false, true> } },
      { { boundary_i32<1, 16, true, true>, boundary_i32<4, 16, true, true> }, { boundary_i32<1, 64, true, true>, boundary_i32<4, 64, true, true> } } },
};
static_assert(MBN_BOUNDARY_SMALL_D == 16 && MBN_BOUNDARY_MAX_D == 64, "the two half-width classes instantiated above");
static_assert(((MBN_BOUNDARY_LDS_CLASSES + 1) * (MBN_BOUNDARY_LDS_CLASSES + 1) + 3 * MBN_BOUNDARY_LDS_CLASSES) * 4 <= MBN_BOUNDARY_TABLE_BYTES &&
              MBN_BOUNDARY_TABLE_BYTES % 16 == 0, "the bins of the largest LDS class count fit their part of the LDS");

// The launch of all four calls. d_alloc = the largest half-width of the call (MBN_BOUNDARY_MAX_D with per-item half-widths); tiles = an upper
// bound of its tiles, which only caps the grid
int bd_launch(mbn_context *ctx, mbn_ragged_readout *r, hipStream_t s, const BoundaryArgs &a, bool score, int elem_bytes, int d_alloc, double tiles)
{
    int lds = 0;
    if (mbn_boundary_tile(d_alloc, nullptr, nullptr, &lds) != MBN_OK) return MBN_EUNSUPPORTED;
    if (!score) lds = (lds - MBN_BOUNDARY_TABLE_BYTES) / 2;
    const bool large = d_alloc > MBN_BOUNDARY_SMALL_D;
    int per_cu = MBN_BOUNDARY_CU_LDS / lds;
    if (per_cu > 2048 / BD_THREADS) per_cu = 2048 / BD_THREADS;
    // tiles is a sum of whole numbers: a map inside the envelope has fewer than 2^29 tiles (one per pixel at most, rows * cols < 2^29), a uniform call
    // at most 65535 maps and a set fewer than 2^31 items, so the sum is below 2^60 and its conversion cannot overflow; wherever it is too large for
    // a double to hold exactly (above 2^53) it is far above num_cus * per_cu, which is then the grid either way
    const unsigned grid = mbn_persistent_grid(ctx->num_cus, per_cu, (long long)tiles);
    // the large class reaches 122 880 bytes: above the 64 KB a launch gets without asking (once per process; not a stream operation)
    static std::once_flag asked;
    std::call_once(asked, [] {
        int most = 0;
        (void)mbn_boundary_tile(MBN_BOUNDARY_MAX_D, nullptr, nullptr, &most);
        for (int sc = 0; sc < 2; sc++)
            for (int rg = 0; rg < 2; rg++)
                for (int eb = 0; eb < 2; eb++)
                    (void)hipFuncSetAttribute((const void *)bd_kernels[sc][rg][1][eb], hipFuncAttributeMaxDynamicSharedMemorySize, most);
    });
    (void)hipSetDevice(ctx->device);
    hipLaunchKernelGGL(bd_kernels[score][r != nullptr][large][elem_bytes == 4], dim3(grid), dim3(BD_THREADS), (size_t)lds, s, a);
    if (r) mbn_ragged_readout_mark_done(r, s);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MBN_OK : mbn_record_hip_error(ctx, e, "boundary launch");
}

double bd_tiles(int rows, int cols, int d)
{
    const int tr = d <= MBN_BOUNDARY_SMALL_D ? MBN_BOUNDARY_SMALL_ROWS : MBN_BOUNDARY_LARGE_ROWS;
    return (double)((rows + tr - 1) / tr) * (double)((cols + BD_TC - 1) / BD_TC);
}

// The shape of a ragged call from the handle's pinned items: the envelope's answer over every map (MBN_EINVAL first), its tiles
int bd_ragged_shape(const mbn_ragged_readout *r, int elem_bytes, int classes, int d, const void *d_items, int edge, double *tiles)
{
    const int d_each = d_items ? MBN_BOUNDARY_MAX_D : d;
    *tiles = 0.0;
    return mbn_ragged_readout_envelope(r, [&](const mbn_label_item &it) {
        const int rc = mbn_boundary_envelope(elem_bytes, classes, 1, it.rows, it.cols, d_each, edge);
        if (rc == MBN_OK) *tiles += bd_tiles(it.rows, it.cols, d_each);
        return rc;
    });
}

// What the two depth calls share once the shape is known; span = the elements of the maps
int depth_call(mbn_context *ctx, mbn_ragged_readout *r, BoundaryArgs &a, int shape, int elem_bytes, double span, int d_alloc, double tiles, void *stream)
{
    if (shape == MBN_EINVAL) return shape;
    if ((elem_bytes == 4 && (uintptr_t)a.map % 4) || (uintptr_t)a.d_items % 4) return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    if (mbn_spans_overlap(a.depth, span, a.map, span * elem_bytes)) return MBN_EINVAL;
    const mbn_span sp[] = { { a.depth, span, "boundary depth" }, { a.map, span * elem_bytes, "boundary map" },
                        { a.d_items, 4.0 * (r ? r->batch : 0), "boundary d_items" } };
    const int rc = mbn_span_check(ctx, sp, (int)(sizeof sp / sizeof sp[0]));
    if (rc != MBN_OK) return rc;
    return bd_launch(ctx, r, stream ? (hipStream_t)stream : ctx->stream, a, false, elem_bytes, d_alloc, tiles);
}

int score_call(mbn_context *ctx, mbn_ragged_readout *r, BoundaryArgs &a, int shape, int truth_bytes, double span, int d_alloc, double tiles, void *stream)
{
    if (shape == MBN_EINVAL) return shape;
    if ((uintptr_t)a.trimap % 8 || (uintptr_t)a.biou % 8 || (uintptr_t)a.labels % 4 || (truth_bytes == 4 && (uintptr_t)a.map % 4) ||
        (uintptr_t)a.d_items % 4)
        return MBN_EINVAL;
    if (shape != MBN_OK) return shape;
    const mbn_span sp[] = { { a.trimap, 8.0 * (a.classes + 1) * (a.classes + 1), "boundary trimap" }, { a.biou, 24.0 * a.classes, "boundary biou" },
                        { a.labels, 4.0 * span, "boundary labels" }, { a.map, span * truth_bytes, "boundary truth" },
                        { a.d_items, 4.0 * (r ? r->batch : 0), "boundary d_items" } };
    const int rc = mbn_span_check(ctx, sp, (int)(sizeof sp / sizeof sp[0]));
    if (rc != MBN_OK) return rc;
    return bd_launch(ctx, r, stream ? (hipStream_t)stream : ctx->stream, a, true, truth_bytes, d_alloc, tiles);
}

void ragged_args(BoundaryArgs &a, const mbn_ragged_readout *r, const void *d_items)
{
    a.d_items = (const int32_t *)d_items;
    a.set = mbn_ragged_readout_view(r);
}

}   // namespace

extern "C" {

int mbn_boundary_d_items(mbn_ragged_readout *r, double ratio, int32_t *d_host)
{
    if (!r || !d_host || r->batch <= 0) return MBN_EINVAL;
    int status = MBN_OK;
    for (int i = 0; i < r->batch; i++) {
        const mbn_label_item *it = mbn_ragged_readout_item(r, i);
        const int d = mbn_boundary_d(it->rows, it->cols, ratio);
        if (d == MBN_EINVAL || (d < 0 && status == MBN_OK)) status = d;
    }
    if (status != MBN_OK) return status;
    for (int i = 0; i < r->batch; i++) {
        const mbn_label_item *it = mbn_ragged_readout_item(r, i);
        d_host[i] = mbn_boundary_d(it->rows, it->cols, ratio);
    }
    return MBN_OK;
}

int mbn_boundary_depth(mbn_context *ctx, void *depth_u8, const void *map, int elem_bytes, int batch, int rows, int cols, int d, int edge, void *stream)
{
    if (!ctx || !depth_u8 || !map) return MBN_EINVAL;
    const int shape = mbn_boundary_envelope(elem_bytes, 1, batch, rows, cols, d, edge);
    BoundaryArgs a = {};
    a.depth = (uint8_t *)depth_u8;
    a.map = (const uint8_t *)map;
    a.batch = batch; a.rows = rows; a.cols = cols; a.d = d; a.edge = edge;
    const double span = shape == MBN_OK ? (double)batch * rows * cols : 0.0;
    return depth_call(ctx, nullptr, a, shape, elem_bytes, span, d, shape == MBN_OK ? batch * bd_tiles(rows, cols, d) : 0.0, stream);
}

int mbn_boundary_depth_ragged(mbn_ragged_readout *r, void *depth_u8, const void *map, int elem_bytes, int d, const void *d_items_i32, int edge,
                              void *stream)
{
    if (!r || r->batch <= 0 || !depth_u8 || !map) return MBN_EINVAL;                   // no set: no maps
    BoundaryArgs a = {};
    a.depth = (uint8_t *)depth_u8;
    a.map = (const uint8_t *)map;
    a.d = d_items_i32 ? MBN_BOUNDARY_MAX_D : d; a.edge = edge;
    ragged_args(a, r, d_items_i32);
    double tiles = 0.0;
    const int shape = bd_ragged_shape(r, elem_bytes, 1, d, d_items_i32, edge, &tiles);
    return depth_call(r->ctx, r, a, shape, elem_bytes, (double)r->launch.span, a.d, tiles, stream);
}

int mbn_boundary_score_i32(mbn_context *ctx, void *trimap_u64, void *biou_u64, const void *labels_i32, const void *truth, int truth_bytes, int classes,
                           int batch, int rows, int cols, int d, int edge, void *stream)
{
    if (!ctx || (!trimap_u64 && !biou_u64) || !labels_i32 || !truth) return MBN_EINVAL;
    const int shape = mbn_boundary_envelope(truth_bytes, classes, batch, rows, cols, d, edge);
    BoundaryArgs a = {};
    a.trimap = (unsigned long long *)trimap_u64;
    a.biou = (unsigned long long *)biou_u64;
    a.labels = (const int32_t *)labels_i32;
    a.map = (const uint8_t *)truth;
    a.classes = classes; a.batch = batch; a.rows = rows; a.cols = cols; a.d = d; a.edge = edge;
    a.lds_form = classes <= MBN_BOUNDARY_LDS_CLASSES;
    const double span = shape == MBN_OK ? (double)batch * rows * cols : 0.0;
    return score_call(ctx, nullptr, a, shape, truth_bytes, span, d, shape == MBN_OK ? batch * bd_tiles(rows, cols, d) : 0.0, stream);
}

int mbn_boundary_score_ragged_i32(mbn_ragged_readout *r, void *trimap_u64, void *biou_u64, const void *labels_i32, const void *truth, int truth_bytes,
                                  int classes, int d, const void *d_items_i32, int edge, void *stream)
{
    if (!r || r->batch <= 0 || (!trimap_u64 && !biou_u64) || !labels_i32 || !truth) return MBN_EINVAL;
    BoundaryArgs a = {};
    a.trimap = (unsigned long long *)trimap_u64;
    a.biou = (unsigned long long *)biou_u64;
    a.labels = (const int32_t *)labels_i32;
    a.map = (const uint8_t *)truth;
    a.classes = classes; a.d = d_items_i32 ? MBN_BOUNDARY_MAX_D : d; a.edge = edge;
    a.lds_form = classes <= MBN_BOUNDARY_LDS_CLASSES;
    ragged_args(a, r, d_items_i32);
    double tiles = 0.0;
    const int shape = bd_ragged_shape(r, truth_bytes, classes, d, d_items_i32, edge, &tiles);
    return score_call(r->ctx, r, a, shape, truth_bytes, (double)r->launch.span, a.d, tiles, stream);
}

}   // extern "C"
