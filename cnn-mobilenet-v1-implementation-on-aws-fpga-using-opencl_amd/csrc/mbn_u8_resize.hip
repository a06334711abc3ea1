// mbn_u8_resize.hip — the table kernels of the resize front-end: `batch` uint8 HWC images of ONE geometry, whose tap tables the host built
// (host/mbn_resize.c, mbn_resize_taps_filter: one kernel for the five convolution filters, which differ in their tables alone) and the handle keeps
// in device memory; MBN_FILTER_NEAREST has no taps and a gather kernel of its own (resize_nearest_u8, below). The tile body is mbn_u8_resize.h's and the tile plan
// mbn_resize_table_plan's (host/mbn_resize.c); what is this file's own: the tables' addressing, their validation, and the handle.
// The reference has no counterpart: decode_image (MobileNet.c:49-57) reads 224*224*3 raw bytes and nothing resizes them.
//
// A tile's window comes from the tables at its first and last outputs. Its horizontal weights are copied to LDS; the vertical first rows, counts and
// weights stay in memory, where a wave reads its output row's as scalars. Nothing here clamps: axis_ok has checked at create time what the bounds rest on.
#include "mbn_u8_resize.h"

#include <algorithm>
#include <new>

namespace {

// Where the oh x ow outputs of an image go: out_img bytes from one image's first output to the next one's, out_ld from a row to the next, the first
// one out_org bytes into the image's part of `out` (PAD only). oh * ow * 3, ow * 3 and 0, what the kernels used to compute, except under a letterbox
// (mbn_resizer_create_pad): there an image's part of `out` is a canvas_rows x canvas_cols canvas, the outputs are its rectangle at (x, y), and the PAD
// instantiations of the kernels run fill_wgs more workgroups per image behind the `tiles` that resize, which write the canvas outside the rectangle
// (resize_fill_rows: no taps, no LDS, no barrier; they touch no byte the tiles write)
struct ResizeDest {
    size_t out_img, out_org;
    int out_ld;
    int tiles;                               // grid.x of the plain launch
    int canvas_cols, x, y, fill_rows;        // letterbox only
    ResizeFill fill;
};

// letterbox: true when this workgroup was one of the border's (and is done); the whole workgroup takes the same way
__device__ __forceinline__ bool resize_border(const ResizeDest &d, uint8_t *out, int iw, int ih, int lane, int wave)
{
    const int b = (int)blockIdx.x - d.tiles;
    if (b < 0) return false;
    resize_fill_rows(out + (size_t)blockIdx.y * d.out_img, d.canvas_cols, d.x, d.y, iw, ih, b * MBN_RESIZE_FILL_ROWS, d.fill_rows, d.fill, lane, wave);
    return true;
}

struct ResizeArgs {
    uint8_t *out;
    const uint8_t *in;
    const int32_t *fx, *cx, *wx, *fy, *cy, *wy;
    int h, w, oh, ow, kx, ky;
    int tow, toh, tiles_x;
    int seg_stride, stage_off, tmp_off;      // mbn_resize_plan_t
    ResizeDest d;
};

// MIRROR (mbn_resizer_create_view with mirror = 1; PAD only): the inner image is the resize's, its columns in reverse order. A tile still resizes
// the columns [ox0, ox0 + oxn) of the tables, with the same window and the same plan; it forms them from right to left (its weights are copied to LDS
// in reverse column order and a lane's element takes the mirrored column's first tap) and lands at the mirrored place, column ow - ox0 - oxn
template <bool PAD, bool MIRROR = false>
__global__ __launch_bounds__(256, 8) void resize_u8(const ResizeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    int32_t *s_wx = reinterpret_cast<int32_t *>(s_mem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (PAD)
        if (resize_border(a.d, a.out, a.ow, a.oh, lane, wave)) return;       // before anything indexes the tables with a tile that is none
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int ox0 = tx * a.tow, oxn = min(a.tow, a.ow - ox0), oy0 = ty * a.toh, oyn = min(a.toh, a.oh - oy0);
    const int row_e = oxn * 3;                                   // horizontal sums of a source row
    // first and count grow with the output index, so the tile's first and last outputs bound its window
    const int xs0 = a.fx[ox0], xs1 = a.fx[ox0 + oxn - 1] + a.cx[ox0 + oxn - 1];
    const int y0 = a.fy[oy0], y1 = a.fy[oy0 + oyn - 1] + a.cy[oy0 + oyn - 1];
    const int nrows = y1 - y0, nb = (xs1 - xs0) * 3;
    const size_t img = (size_t)blockIdx.y;
    const uint8_t *__restrict__ src = a.in + img * ((size_t)a.h * a.w * 3);
    uint8_t *__restrict__ dst = a.out + img * a.d.out_img + (PAD ? a.d.out_org : 0);
    uint8_t *s_row = s_mem + a.stage_off + wave * a.seg_stride;
    uint8_t *s_tmp = s_mem + a.tmp_off;
    const int tmp_ld = a.tow * 3;

    if constexpr (MIRROR) {
        for (int e = tid; e < oxn * a.kx; e += 256) {
            const int ox = e / a.kx;
            s_wx[e] = a.wx[(ox0 + oxn - 1 - ox) * a.kx + (e - ox * a.kx)];
        }
    } else {
        for (int e = tid; e < oxn * a.kx; e += 256) s_wx[e] = a.wx[ox0 * a.kx + e];
    }
    int lo[RESIZE_EPL], wofs[RESIZE_EPL];
    resize_lane_elems(lo, wofs, lane, row_e, a.kx, [&](int ox) { return a.fx[ox0 + (MIRROR ? oxn - 1 - ox : ox)] - xs0; });
    __syncthreads();                                             // the weights are in place
    for (int r = wave; r < nrows; r += MBN_RESIZE_WAVES) {
        const uint8_t *s_seg = resize_stage_row(s_row, src + ((size_t)(y0 + r) * a.w + xs0) * 3, nb, lane);
        resize_row_sums(s_tmp + r * tmp_ld, s_seg, s_wx, lo, wofs, a.kx, row_e, lane);
    }
    __syncthreads();                                             // the window is complete
    resize_vertical(dst + (size_t)oy0 * a.d.out_ld + (MIRROR ? a.ow - ox0 - oxn : ox0) * 3, (size_t)a.d.out_ld, s_tmp, tmp_ld, oyn, row_e, lane, wave, [&](int oy, int &f, int &n) {
        f = a.fy[oy0 + oy] - y0;
        n = a.cy[oy0 + oy];
        return a.wy + (size_t)(oy0 + oy) * a.ky;
    });
}

// MBN_FILTER_NEAREST: no taps, the uploaded indices ix [ow], iy [oh]. A workgroup takes MBN_RESIZE_WAVES whole output rows of one image, a wave a row
// (resize_nearest_rows: tow = ow). index_ok has checked the indices at create time; they are clamped here anyway, for memory safety only
struct NearestArgs {
    uint8_t *out;
    const uint8_t *in;
    const int32_t *ix, *iy;
    int h, w, oh, ow;
    ResizeDest d;
};

template <bool PAD>
__global__ __launch_bounds__(256) void resize_nearest_u8(const NearestArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if constexpr (PAD)
        if (resize_border(a.d, a.out, a.ow, a.oh, lane, wave)) return;
    const int oy0 = (int)blockIdx.x * MBN_RESIZE_WAVES, oyn = min(MBN_RESIZE_WAVES, a.oh - oy0);
    const size_t img = (size_t)blockIdx.y;
    const uint8_t *__restrict__ src = a.in + img * ((size_t)a.h * a.w * 3);
    uint8_t *__restrict__ dst = a.out + img * a.d.out_img + (PAD ? a.d.out_org : 0);
    resize_nearest_rows(dst + (size_t)oy0 * a.d.out_ld, (size_t)a.d.out_ld, src, a.w, oyn, a.ow * 3, lane, wave,
                        [&](int ox) { return min(max(a.ix[ox], 0), a.w - 1); }, [&](int oy) { return min(max(a.iy[oy0 + oy], 0), a.h - 1); });
}

bool index_ok(const int32_t *index, int out_size, int in_size)
{
    for (int i = 0; i < out_size; i++)
        if (index[i] < 0 || index[i] >= in_size || (i && index[i] < index[i - 1])) return false;
    return true;
}

// an axis's tables are what the kernel's bounds rest on: every tap inside the source, first and first + count growing with the index
bool axis_ok(const int32_t *first, const int32_t *count, int out_size, int in_size, int ksize)
{
    for (int i = 0; i < out_size; i++) {
        if (first[i] < 0 || count[i] < 1 || count[i] > ksize || first[i] + count[i] > in_size) return false;
        if (i && (first[i] < first[i - 1] || first[i] + count[i] < first[i - 1] + count[i - 1])) return false;
    }
    return true;
}

}   // namespace

// The geometry is inside mbn_resize_envelope (the caller has checked it). Plans the tile, builds the tables and uploads them: blocking.
int mbn_resizer_build(mbn_context *ctx, int filter, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, bool mirror,
                      mbn_resizer **out)
{
    const float whole[4] = { 0.0f, 0.0f, (float)in_cols, (float)in_rows };
    const float *b = box ? box : whole;
    mbn_resize_plan_t p;
    int rc = mbn_resize_table_plan_filter(filter, in_rows, in_cols, b, out_rows, out_cols, &p);
    if (rc != MBN_OK) return rc;
    // one host block, the layout of the device block: fx, cx, fy, cy, wx, wy; NEAREST: ix, iy
    const bool nearest = filter == MBN_FILTER_NEAREST;
    const size_t n32 = nearest ? (size_t)out_cols + (size_t)out_rows
                               : 2 * (size_t)out_cols + 2 * (size_t)out_rows + (size_t)out_cols * p.kx + (size_t)out_rows * p.ky;
    std::vector<int32_t> tab;
    try { tab.resize(n32); } catch (const std::bad_alloc &) { return MBN_ENOMEM; }
    if (nearest) {
        int32_t *ix = tab.data(), *iy = ix + out_cols;
        rc = mbn_resize_nearest_index(in_cols, b[0], b[2], out_cols, ix);
        if (rc == MBN_OK) rc = mbn_resize_nearest_index(in_rows, b[1], b[3], out_rows, iy);
        if (rc != MBN_OK) return rc;
        if (!index_ok(ix, out_cols, in_cols) || !index_ok(iy, out_rows, in_rows)) return MBN_EINVAL;
        if (mirror) std::reverse(ix, ix + out_cols);         // a gather: the mirror is the column indices in reverse order (the kernel asks them no order)
    } else {
        int32_t *fx = tab.data(), *cx = fx + out_cols, *fy = cx + out_cols, *cy = fy + out_rows, *wx = cy + out_rows, *wy = wx + (size_t)out_cols * p.kx;
        rc = mbn_resize_taps_filter(filter, in_cols, b[0], b[2], out_cols, fx, cx, wx);
        if (rc >= 0) rc = mbn_resize_taps_filter(filter, in_rows, b[1], b[3], out_rows, fy, cy, wy);
        if (rc < 0) return rc;
        if (!axis_ok(fx, cx, out_cols, in_cols, p.kx) || !axis_ok(fy, cy, out_rows, in_rows, p.ky)) return MBN_EINVAL;
    }

    mbn_resizer *r = new (std::nothrow) mbn_resizer();
    if (!r) return MBN_ENOMEM;
    r->ctx = ctx;
    r->filter = filter;
    r->mirror = mirror;
    r->in_rows = in_rows; r->in_cols = in_cols; r->out_rows = out_rows; r->out_cols = out_cols;
    r->canvas_rows = out_rows; r->canvas_cols = out_cols;
    r->plan = p;
    (void)hipSetDevice(ctx->device);
    hipError_t e = hipMalloc(&r->tables, n32 * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(r->tables, tab.data(), n32 * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (r->tables) (void)hipFree(r->tables);
        delete r;
        return e == hipErrorOutOfMemory ? MBN_ENOMEM : mbn_record_hip_error(ctx, e, "resizer tables");
    }
    *out = r;
    return MBN_OK;
}

// The handle of the whole image -> pp.ih x pp.iw (mirrored or not), and where that lies in the out_rows x out_cols canvas
static int build_in_canvas(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const mbn_resize_pad_plan_t &pp, bool mirror,
                           const uint8_t fill[3], mbn_resizer **out)
{
    const int rc = mbn_resizer_build(ctx, filter, in_rows, in_cols, nullptr, pp.ih, pp.iw, mirror, out);
    if (rc != MBN_OK) return rc;
    mbn_resizer *r = *out;
    r->canvas_rows = out_rows; r->canvas_cols = out_cols;
    r->pad = true;
    r->pad_x = pp.x; r->pad_y = pp.y; r->fill_rows = pp.fill_rows; r->fill_wgs = pp.fill_wgs;
    memcpy(r->fill, fill, 3);
    return MBN_OK;
}

// The letterbox: the rectangle is mbn_fit_pad's. fill is non-null (the caller has checked)
int mbn_resizer_build_pad(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const uint8_t fill[3], mbn_resizer **out)
{
    mbn_resize_pad_plan_t pp;
    const int rc = mbn_resize_pad_table_plan_filter(filter, in_rows, in_cols, out_rows, out_cols, &pp);
    if (rc != MBN_OK) return rc;
    return build_in_canvas(ctx, filter, in_rows, in_cols, out_rows, out_cols, pp, false, fill, out);
}

// A view: the rectangle is the caller's, the inner image mirrored when the view says so. view and fill are non-null (the caller has checked)
int mbn_resizer_build_view(mbn_context *ctx, int filter, int in_rows, int in_cols, int out_rows, int out_cols, const mbn_view *view, const uint8_t fill[3],
                           mbn_resizer **out)
{
    mbn_resize_pad_plan_t pp;
    const int rc = mbn_resize_view_table_plan_filter(filter, in_rows, in_cols, out_rows, out_cols, view, &pp);
    if (rc != MBN_OK) return rc;
    return build_in_canvas(ctx, filter, in_rows, in_cols, out_rows, out_cols, pp, view->mirror != 0, fill, out);
}

void mbn_resizer_release(mbn_resizer *r)
{
    if (r->tables) (void)hipFree(r->tables);
    delete r;
}

// in [batch][in_rows][in_cols][3] -> out [batch][canvas_rows][canvas_cols][3]; batch in 1..MBN_RESIZE_MAX_BATCH, pointers non-null (the caller has
// checked). A letterbox handle: the PAD instantiation of the same kernel, with the canvas's strides and fill_wgs more workgroups per image
int mbn_launch_u8_resize(const mbn_resizer *r, hipStream_t s, uint8_t *out, const uint8_t *in, int batch)
{
    const mbn_resize_plan_t &p = r->plan;
    const int32_t *t = (const int32_t *)r->tables;
    const bool nearest = r->filter == MBN_FILTER_NEAREST;
    ResizeDest d;
    d.out_img = (size_t)r->canvas_rows * r->canvas_cols * 3;
    d.out_org = ((size_t)r->pad_y * r->canvas_cols + r->pad_x) * 3;
    d.out_ld = r->canvas_cols * 3;
    d.tiles = nearest ? (r->out_rows + MBN_RESIZE_WAVES - 1) / MBN_RESIZE_WAVES : p.tiles_x * p.tiles_y;
    d.canvas_cols = r->canvas_cols; d.x = r->pad_x; d.y = r->pad_y; d.fill_rows = r->fill_rows;
    d.fill = resize_fill_of(r->fill);
    const dim3 grid((unsigned)(d.tiles + r->fill_wgs), (unsigned)batch), block(256);
    if (nearest) {
        NearestArgs n;
        n.out = out; n.in = in;
        n.ix = t; n.iy = t + r->out_cols;
        n.h = r->in_rows; n.w = r->in_cols; n.oh = r->out_rows; n.ow = r->out_cols;
        n.d = d;
        if (r->pad) hipLaunchKernelGGL(resize_nearest_u8<true>, grid, block, 0, s, n);
        else hipLaunchKernelGGL(resize_nearest_u8<false>, grid, block, 0, s, n);
        return MBN_OK;
    }
    ResizeArgs a;
    a.out = out; a.in = in;
    a.fx = t; a.cx = a.fx + r->out_cols; a.fy = a.cx + r->out_cols; a.cy = a.fy + r->out_rows;
    a.wx = a.cy + r->out_rows; a.wy = a.wx + (size_t)r->out_cols * p.kx;
    a.h = r->in_rows; a.w = r->in_cols; a.oh = r->out_rows; a.ow = r->out_cols; a.kx = p.kx; a.ky = p.ky;
    a.tow = p.tow; a.toh = p.toh; a.tiles_x = p.tiles_x;
    a.seg_stride = p.seg_stride; a.stage_off = p.stage_off; a.tmp_off = p.tmp_off;
    a.d = d;
    if (r->pad && r->mirror) hipLaunchKernelGGL((resize_u8<true, true>), grid, block, (size_t)p.lds_bytes, s, a);
    else if (r->pad) hipLaunchKernelGGL(resize_u8<true>, grid, block, (size_t)p.lds_bytes, s, a);
    else hipLaunchKernelGGL(resize_u8<false>, grid, block, (size_t)p.lds_bytes, s, a);
    return MBN_OK;
}
