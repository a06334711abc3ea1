// mbn_u8_resize_ragged.hip — the ragged resize on gfx950: ONE launch takes `batch` uint8 HWC images, each with its own rows, cols and box, to one common
// [batch][oh][ow][3], byte for byte the arithmetic of include/mbn.h ("resize front-end"). mbn_u8_resize.hip is its single-geometry sibling and stays the
// path of uniform batches; the tile body is mbn_u8_resize.h's for both. What is this file's own:
//   taps        no table exists anywhere. The workgroup forms its tile's taps itself, straight into LDS: lane c of wave 0 runs output column c of the
//               tile, lane r of wave 1 output row r, each its <= 67 taps one after the other (mbn_axis_taps of host/mbn_resize_axis.h: the host's own
//               expressions, in fp64 with contraction off). The vertical weights, first rows and counts sit in LDS as well;
//   filters     the handle's: MBN_FILTER_BOX, _BILINEAR and _BICUBIC are instantiations of one kernel (plain fp64 arithmetic, the reciprocal 1.0 / fs
//               a true division: the host's bits), MBN_FILTER_NEAREST is a gather kernel of its own. HAMMING and LANCZOS have no device form: their
//               weights need sin / cos bit-equal to the host's libm, which device math does not promise (the plan answers MBN_EUNSUPPORTED);
//   geometry    per image, from a 64-byte descriptor in device memory (mbn_resize_desc, host/mbn_envelope.h): the caller's item and what the host
//               planned without a table (host/mbn_resize.c, mbn_resize_ragged_plan): ksize per axis, the tile height, the staged row's stride, the
//               window's LDS offset, and the image's first workgroup;
//   mapping     the grid is 1-D, one workgroup per tile of the batch and none idle: workgroup w belongs to the last image whose first workgroup is
//               <= w, found by a 64-ary search of the descriptors (each lane probes one, a ballot counts: one probe round up to 64 images, two up to
//               4096). A (most tiles, batch) grid with early exit would launch batch x out_rows x tiles_x workgroups as soon as ONE image of the
//               batch is a steep downscale with one-row tiles;
//   letterbox   (mbn_ragged_resizer_create_pad) the PAD instantiations of the same kernels: an image's outputs are its own ih x iw, at (x, y) of its
//               canvas (mbn_resize_pad_desc: the plain descriptor of (rows, cols) -> (ih, iw), then the rectangle, the image's tow and tiles_x and
//               its border), so the axes, the tile counts and the search run on those descriptors. Behind an image's tiles its share of the grid has
//               fill_wgs more workgroups, which write the canvas outside the rectangle (resize_fill_rows) and need no taps, no LDS and no barrier.
// The tile's window comes from mbn_axis_span at its edge outputs, as the host's plan did (mbn_resize_window): the same code on both sides. Should
// they ever disagree, the kernel's capacity clamps turn that into wrong bytes (which the tests compare) and never into an access outside LDS, the
// images or the output.
#include "mbn_resize_axis.h"
#include "mbn_u8_resize.h"

#include <new>

namespace {

// head of the device block, in front of the descriptors; 64 bytes like them
struct RaggedHead {
    int32_t batch, total_wgs, lds_bytes, generation;
    int32_t pad[12];
};
static_assert(sizeof(RaggedHead) == 64 && sizeof(mbn_resize_desc) == 64 && sizeof(mbn_resize_item) == 32, "device layout");
static_assert(sizeof(mbn_resize_pad_desc) == 96 && offsetof(mbn_resize_pad_desc, img) == 0, "device layout");

struct RaggedArgs {
    uint8_t *out;
    const uint8_t *src;
    const RaggedHead *head;
    const mbn_resize_desc *desc;             // the plain launch's descriptors, or
    const mbn_resize_pad_desc *pdesc;        // the letterbox's (the other one is null)
    int oh, ow, tow, tiles_x;                // what `out` holds per image; tow and tiles_x belong to it in a plain launch, to each image under a letterbox
    int lds_bytes;           // the launch's dynamic LDS
    int generation;          // of the set this launch was issued (or captured) for
    ResizeFill fill;         // letterbox: the border's colour
};

template <bool PAD>
__device__ __forceinline__ int ragged_wg0(const RaggedArgs &a, int i)
{
    if constexpr (PAD) return a.pdesc[i].img.wg0;
    else return a.desc[i].wg0;
}

// the image of workgroup wg: the last one whose first workgroup is <= wg, among [base, base + n). wg0 of image `base` <= wg holds throughout (image 0: 0)
template <bool PAD>
__device__ __forceinline__ int ragged_image(const RaggedArgs &a, int wg, int lane)
{
    int base = 0, n = a.head->batch;
    while (n > 1) {
        const int stride = (n + 63) >> 6;
        const bool le = lane * stride < n && ragged_wg0<PAD>(a, base + lane * stride) <= wg;
        const int step = (max(__popcll(__ballot(le)), 1) - 1) * stride;      // wg0 grows with the index: the lanes that say yes are the first ones
        base += step;
        n = min(stride, n - step);
    }
    return __builtin_amdgcn_readfirstlane(base);
}

// What the workgroups of image `img` work on: its descriptor, its oh x ow outputs and their tiles, and its first output byte (output rows are a.ow * 3
// bytes apart in either case). Under a letterbox the outputs are the rectangle of the image's canvas
struct RaggedGeo {
    const mbn_resize_desc *d;
    int oh, ow, tow, tiles_x;
    uint8_t *dst;
};

template <bool PAD>
__device__ __forceinline__ RaggedGeo ragged_geo(const RaggedArgs &a, int img)
{
    RaggedGeo g;
    uint8_t *canvas = a.out + (size_t)img * ((size_t)a.oh * a.ow * 3);
    if constexpr (PAD) {
        const mbn_resize_pad_desc &p = a.pdesc[img];
        g.d = &p.img; g.oh = p.ih; g.ow = p.iw; g.tow = p.tow; g.tiles_x = p.tiles_x;
        g.dst = canvas + ((size_t)p.y * a.ow + p.x) * 3;
    } else {
        g.d = &a.desc[img]; g.oh = a.oh; g.ow = a.ow; g.tow = a.tow; g.tiles_x = a.tiles_x;
        g.dst = canvas;
    }
    return g;
}

// Letterbox: workgroup `tile` of image `img` when it lies behind the image's tiles: border workgroup tile - tiles_x * tiles_y of the canvas. True when
// the workgroup was one of those (and is done); the whole workgroup takes the same way
__device__ __forceinline__ bool ragged_border(const RaggedArgs &a, int img, int tile, int lane, int wave)
{
    const mbn_resize_pad_desc &p = a.pdesc[img];
    const int b = tile - p.tiles_x * p.img.tiles_y;
    if (b < 0) return false;
    if (b < p.fill_wgs)
        resize_fill_rows(a.out + (size_t)img * ((size_t)a.oh * a.ow * 3), a.ow, p.x, p.y, p.iw, p.ih, b * MBN_RESIZE_FILL_ROWS, p.fill_rows, a.fill, lane, wave);
    return true;
}

// FILTER = MBN_FILTER_BOX, _BILINEAR or _BICUBIC: a template argument, so the weight function's dispatch (mbn_axis_weight) is decided when the kernel is
// compiled and the tap loops carry no branch on it. PAD: the letterbox's descriptors and border workgroups (above); nothing else differs
template <int FILTER, bool PAD>
__global__ __launch_bounds__(256, 8) void resize_ragged_u8(const RaggedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = (int)blockIdx.x;
    // a replay of a captured launch after another set: the descriptors are no longer the ones its grid, LDS and spans were checked for
    if (a.head->generation != a.generation || wg >= a.head->total_wgs) return;
    const int img = ragged_image<PAD>(a, wg, lane);
    const RaggedGeo g = ragged_geo<PAD>(a, img);
    const mbn_resize_desc &d = *g.d;
    const int kx = d.kx, ky = d.ky, toh = d.toh, tow = g.tow;
    const int tile = wg - d.wg0, ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    if (tile < 0) return;
    if constexpr (PAD)
        if (ragged_border(a, img, tile, lane, wave)) return;
    if (ty >= d.tiles_y) return;
    const int ox0 = tx * tow, oxn = min(tow, g.ow - ox0), oy0 = ty * toh, oyn = min(toh, g.oh - oy0);
    const int row_e = oxn * 3;                                   // horizontal sums of a source row
    const mbn_axis gx = mbn_axis_of_filter(FILTER, d.cols, d.box[0], d.box[2], g.ow), gy = mbn_axis_of_filter(FILTER, d.rows, d.box[1], d.box[3], g.oh);
    int xs0, xs1, y0, y1, unused;
    (void)mbn_axis_span(&gx, ox0, &xs0, &unused);
    (void)mbn_axis_span(&gx, ox0 + oxn - 1, &unused, &xs1);
    (void)mbn_axis_span(&gy, oy0, &y0, &unused);
    (void)mbn_axis_span(&gy, oy0 + oyn - 1, &unused, &y1);
    // the LDS image of a tile (host/mbn_envelope.h)
    int32_t *s_wx = reinterpret_cast<int32_t *>(s_mem), *s_wy = s_wx + tow * kx, *s_fx = s_wy + toh * ky, *s_fy = s_fx + tow, *s_cy = s_fy + toh;
    uint8_t *s_row = s_mem + MBN_RESIZE_STAGE_OFF(tow, kx, toh, ky) + wave * d.seg_stride;
    uint8_t *s_tmp = s_mem + d.tmp_off;
    const int tmp_ld = tow * 3;
    // what the plan left room for: the host derived the same windows, so neither clamp binds
    const int nb = max(min((xs1 - xs0) * 3, d.seg_stride - 3 - kx * 3), 0);
    const int nrows = max(min(y1 - y0, (a.lds_bytes - d.tmp_off) / tmp_ld), 0);

    // ---- the tile's taps: wave 0 a column per lane, wave 1 a row per lane (toh <= 32)
    if (tid < oxn) {
        (void)mbn_axis_taps(&gx, ox0 + tid, kx, s_wx + tid * kx, &s_fx[tid]);
    } else if (tid >= 64 && tid - 64 < oyn) {
        const int r = tid - 64;
        s_cy[r] = mbn_axis_taps(&gy, oy0 + r, ky, s_wy + r * ky, &s_fy[r]);
    }
    __syncthreads();                                             // the taps are in place

    const uint8_t *__restrict__ src = a.src + d.src_offset;
    uint8_t *__restrict__ dst = g.dst;
    int lo[RESIZE_EPL], wofs[RESIZE_EPL];
    const int last = max(nb / 3 - 1, 0);                         // the last pixel the staged segment holds
    resize_lane_elems(lo, wofs, lane, row_e, kx, [&](int ox) { return min(max(s_fx[ox] - xs0, 0), last); });
    for (int r = wave; r < nrows; r += MBN_RESIZE_WAVES) {
        const uint8_t *s_seg = resize_stage_row(s_row, src + ((size_t)(y0 + r) * d.cols + xs0) * 3, nb, lane);
        resize_row_sums(s_tmp + r * tmp_ld, s_seg, s_wx, lo, wofs, kx, row_e, lane);
    }
    __syncthreads();                                             // the window is complete
    resize_vertical(dst + ((size_t)oy0 * a.ow + ox0) * 3, (size_t)a.ow * 3, s_tmp, tmp_ld, oyn, row_e, lane, wave, [&](int oy, int &f, int &n) {
        f = min(max(__builtin_amdgcn_readfirstlane(s_fy[oy]) - y0, 0), max(nrows - 1, 0));
        n = min(__builtin_amdgcn_readfirstlane(s_cy[oy]), nrows - f);
        return s_wy + oy * ky;
    });
}

// MBN_FILTER_NEAREST: the same grid, descriptors and mapping; a tile is a gather (resize_nearest_rows of mbn_u8_resize.h). Its LDS image is the tile's
// indices alone, ix [tow] then iy [toh]: lane c of wave 0 forms column ox0 + c, lane r of wave 1 row oy0 + r, each with its OWN chain of ox0 + c
// (oy0 + r) dependent fp64 additions from xo_0 (mbn_axis_nearest_index: at most 4095, 223 for this network's outputs). The index is defined by that
// accumulated sum, additions do not associate, and the closed form b0 + a * (i + 0.5) gives other indices: no cheaper form gives the same bits
template <bool PAD>
__global__ __launch_bounds__(256) void resize_ragged_nearest_u8(const RaggedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = (int)blockIdx.x;
    if (a.head->generation != a.generation || wg >= a.head->total_wgs) return;
    const int img = ragged_image<PAD>(a, wg, lane);
    const RaggedGeo g = ragged_geo<PAD>(a, img);
    const mbn_resize_desc &d = *g.d;
    const int tow = g.tow, toh = min(d.toh, a.lds_bytes / 4 - tow);      // what the launch's LDS has room for: the plan's toh, so the clamp does not bind
    const int tile = wg - d.wg0, ty = tile / g.tiles_x, tx = tile - ty * g.tiles_x;
    if (tile < 0) return;
    if constexpr (PAD)
        if (ragged_border(a, img, tile, lane, wave)) return;
    if (ty >= d.tiles_y || toh < 1) return;
    const int ox0 = tx * tow, oxn = min(tow, g.ow - ox0), oy0 = ty * toh, oyn = min(toh, g.oh - oy0);
    int32_t *s_ix = reinterpret_cast<int32_t *>(s_mem), *s_iy = s_ix + tow;
    if (tid < oxn) {
        const mbn_axis gx = mbn_axis_of_filter(MBN_FILTER_NEAREST, d.cols, d.box[0], d.box[2], g.ow);
        s_ix[tid] = mbn_axis_nearest_index(&gx, ox0 + tid);
    } else if (tid >= 64 && tid - 64 < oyn) {
        const mbn_axis gy = mbn_axis_of_filter(MBN_FILTER_NEAREST, d.rows, d.box[1], d.box[3], g.oh);
        s_iy[tid - 64] = mbn_axis_nearest_index(&gy, oy0 + tid - 64);
    }
    __syncthreads();                                             // the indices are in place
    const uint8_t *__restrict__ src = a.src + d.src_offset;
    uint8_t *__restrict__ dst = g.dst;
    resize_nearest_rows(dst + ((size_t)oy0 * a.ow + ox0) * 3, (size_t)a.ow * 3, src, d.cols, oyn, oxn * 3, lane, wave,
                        [&](int ox) { return s_ix[ox]; }, [&](int oy) { return s_iy[oy]; });
}

// mbn_resize_taps_device_filter: the tables of one axis from mbn_axis_taps, an output per lane. NEAREST: first = the index (the lane's own chain of
// additions, as in the kernel above), one tap, the whole weight
template <int FILTER>
__global__ __launch_bounds__(64) void resize_taps_k(int in_size, float b0, float b1, int out_size, int ksize, int32_t *first, int32_t *count, int32_t *weights)
{
    const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (i >= out_size) return;
    const mbn_axis a = mbn_axis_of_filter(FILTER, in_size, b0, b1, out_size);
    if (FILTER == MBN_FILTER_NEAREST) {
        first[i] = mbn_axis_nearest_index(&a, i);
        count[i] = 1;
        weights[i] = 1 << MBN_RESIZE_BITS;
    } else {
        count[i] = mbn_axis_taps(&a, i, ksize, weights + (size_t)i * ksize, &first[i]);
    }
}

}   // namespace

// filter: MBN_FILTER_NEAREST, _BOX, _BILINEAR or _BICUBIC (the caller has checked). fill: NULL, or the colour of a letterbox handle
int mbn_ragged_resizer_build(mbn_context *ctx, int filter, int max_batch, int out_rows, int out_cols, const uint8_t *fill, mbn_ragged_resizer **out)
{
    mbn_ragged_resizer *r = new (std::nothrow) mbn_ragged_resizer();
    if (!r) return MBN_ENOMEM;
    r->ctx = ctx;
    r->filter = filter;
    r->max_batch = max_batch; r->out_rows = out_rows; r->out_cols = out_cols;
    r->tow = MBN_RESIZE_TOW(out_cols);
    r->tiles_x = (out_cols + r->tow - 1) / r->tow;
    if (fill) {
        r->pad = true;
        memcpy(r->fill, fill, 3);
    }
    const size_t bytes = sizeof(RaggedHead) + (size_t)max_batch * (r->pad ? sizeof(mbn_resize_pad_desc) : sizeof(mbn_resize_desc));
    (void)hipSetDevice(ctx->device);
    hipError_t e = hipMalloc(&r->dev, bytes);
    if (e == hipSuccess) e = hipHostMalloc(&r->host, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        mbn_ragged_resizer_release(r);
        return e == hipErrorOutOfMemory ? MBN_ENOMEM : mbn_record_hip_error(ctx, e, "ragged resizer buffers");
    }
    *out = r;
    return MBN_OK;
}

void mbn_ragged_resizer_release(mbn_ragged_resizer *r)
{
    if (r->done) (void)hipEventDestroy(r->done);
    if (r->host) (void)hipHostFree(r->host);
    if (r->dev) (void)hipFree(r->dev);
    delete r;
}

// Plans into the pinned copy and enqueues its upload. Waits first for what still reads either copy: the previous upload and every launch since
int mbn_ragged_resizer_plan(mbn_ragged_resizer *r, hipStream_t s, const mbn_resize_item *items, int batch)
{
    mbn_context *ctx = r->ctx;
    r->batch = 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return MBN_EINVAL;      // a set is not part of a graph
    MBN_HIP_TRY(ctx, hipEventSynchronize(r->done));
    RaggedHead *h = (RaggedHead *)r->host;
    int32_t total = 0, lds = 0;
    int64_t span = 0;
    const int rc = r->pad ? mbn_resize_pad_ragged_plan_batch_filter(r->filter, items, batch, r->out_rows, r->out_cols, (mbn_resize_pad_desc *)(h + 1),
                                                                    &total, &lds, &span)
                          : mbn_resize_ragged_plan_batch_filter(r->filter, items, batch, r->out_rows, r->out_cols, (mbn_resize_desc *)(h + 1), &total,
                                                                &lds, &span);
    if (rc != MBN_OK) return rc;
    const size_t bytes = sizeof(RaggedHead) + (size_t)batch * (r->pad ? sizeof(mbn_resize_pad_desc) : sizeof(mbn_resize_desc));
    memset(h, 0, sizeof *h);
    h->batch = batch; h->total_wgs = total; h->lds_bytes = lds; h->generation = r->generation + 1;
    MBN_HIP_TRY(ctx, hipMemcpyAsync(r->dev, r->host, bytes, hipMemcpyHostToDevice, s));
    MBN_HIP_TRY(ctx, hipEventRecord(r->done, s));
    r->generation = h->generation;
    r->total_wgs = total; r->lds_bytes = lds; r->src_span = span;
    r->batch = batch;
    return MBN_OK;
}

// the handle has a batch, the pointers are non-null and the spans fit (the caller has checked)
int mbn_launch_u8_resize_ragged(mbn_ragged_resizer *r, hipStream_t s, uint8_t *out, const uint8_t *src)
{
    RaggedArgs a;
    a.out = out; a.src = src;
    a.head = (const RaggedHead *)r->dev;
    a.desc = r->pad ? nullptr : (const mbn_resize_desc *)(a.head + 1);
    a.pdesc = r->pad ? (const mbn_resize_pad_desc *)(a.head + 1) : nullptr;
    a.fill = resize_fill_of(r->fill);
    a.oh = r->out_rows; a.ow = r->out_cols; a.tow = r->tow; a.tiles_x = r->tiles_x;
    a.lds_bytes = r->lds_bytes; a.generation = r->generation;
    const dim3 grid((unsigned)r->total_wgs), block(256);
    const size_t lds = (size_t)r->lds_bytes;
    switch (r->filter * 2 + (r->pad ? 1 : 0)) {
    case MBN_FILTER_NEAREST * 2: hipLaunchKernelGGL(resize_ragged_nearest_u8<false>, grid, block, lds, s, a); break;
    case MBN_FILTER_BOX * 2: hipLaunchKernelGGL((resize_ragged_u8<MBN_FILTER_BOX, false>), grid, block, lds, s, a); break;
    case MBN_FILTER_BILINEAR * 2: hipLaunchKernelGGL((resize_ragged_u8<MBN_FILTER_BILINEAR, false>), grid, block, lds, s, a); break;
    case MBN_FILTER_BICUBIC * 2: hipLaunchKernelGGL((resize_ragged_u8<MBN_FILTER_BICUBIC, false>), grid, block, lds, s, a); break;
    case MBN_FILTER_NEAREST * 2 + 1: hipLaunchKernelGGL(resize_ragged_nearest_u8<true>, grid, block, lds, s, a); break;
    case MBN_FILTER_BOX * 2 + 1: hipLaunchKernelGGL((resize_ragged_u8<MBN_FILTER_BOX, true>), grid, block, lds, s, a); break;
    case MBN_FILTER_BILINEAR * 2 + 1: hipLaunchKernelGGL((resize_ragged_u8<MBN_FILTER_BILINEAR, true>), grid, block, lds, s, a); break;
    case MBN_FILTER_BICUBIC * 2 + 1: hipLaunchKernelGGL((resize_ragged_u8<MBN_FILTER_BICUBIC, true>), grid, block, lds, s, a); break;
    default: return MBN_EUNSUPPORTED;                            // no handle has another filter
    }
    // the next set waits for this launch; inside a capture there is nothing to wait for (the replays are the caller's to order)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) (void)hipEventRecord(r->done, s);
    return MBN_OK;
}

// the geometry is inside the device's envelope and ksize is the axis's (the caller has checked)
int mbn_launch_resize_taps(hipStream_t s, int filter, int in_size, float b0, float b1, int out_size, int ksize, int32_t *first, int32_t *count, int32_t *weights)
{
    const dim3 grid((unsigned)((out_size + 63) / 64)), block(64);
    switch (filter) {
    case MBN_FILTER_NEAREST: hipLaunchKernelGGL(resize_taps_k<MBN_FILTER_NEAREST>, grid, block, 0, s, in_size, b0, b1, out_size, ksize, first, count, weights); break;
    case MBN_FILTER_BOX: hipLaunchKernelGGL(resize_taps_k<MBN_FILTER_BOX>, grid, block, 0, s, in_size, b0, b1, out_size, ksize, first, count, weights); break;
    case MBN_FILTER_BILINEAR: hipLaunchKernelGGL(resize_taps_k<MBN_FILTER_BILINEAR>, grid, block, 0, s, in_size, b0, b1, out_size, ksize, first, count, weights); break;
    case MBN_FILTER_BICUBIC: hipLaunchKernelGGL(resize_taps_k<MBN_FILTER_BICUBIC>, grid, block, 0, s, in_size, b0, b1, out_size, ksize, first, count, weights); break;
    default: return MBN_EUNSUPPORTED;
    }
    return MBN_OK;
}
