// mbn_u8_resize.hip — the resize front-end on gfx950: Pillow's 8-bit bilinear resize of a box of uint8 HWC images, both passes in ONE launch
// (include/mbn.h, "resize front-end", is the normative statement of the arithmetic; host/mbn_resize.c builds the tap tables).
// The reference has no counterpart: decode_image (MobileNet.c:49-57) reads 224*224*3 raw bytes and nothing resizes them.
//
// A workgroup of 256 lanes (4 waves) owns a tile of `toh` output rows x `tow` output columns of one image. The tap tables say which source rows
// [y0, y1) and columns [xs0, xs1) the tile needs, and nothing else is read:
//   horizontal  the waves take the source rows of the window in turn, each at its own pace. A wave stages its row's segment [xs0, xs1) in LDS — bytewise up to the first
//               4-byte boundary of the ADDRESS, 4 bytes per lane from there, bytewise for the rest, so any byte pointer and any W * 3 give the same
//               bytes — and then forms the tile's `tow` x 3 horizontal sums of that row from LDS, each rounded to uint8 as Pillow rounds its
//               intermediate image, into the window s_tmp [y1 - y0][tow * 3] in LDS. The tile's horizontal weights sit in LDS as well, and every column runs
//               all kx taps: those past its count carry the tables' zero padding (the staged row has kx pixels of slack for them);
//   vertical    the waves take the tile's output rows in turn: a row's first source row, count and weights are scalars of the wave, a lane sums three
//               bytes of the row's segment over s_tmp, rounds to uint8 and stores to `out` (consecutive lanes, consecutive bytes).
// The uint8 intermediate never reaches memory. The host sizes the tile from the geometry so that weights + 4 staged rows + window fit RESIZE_LDS
// bytes (a 32x downscale has 67 taps per axis: its window alone is 67 + rows, so tiles get flatter as the factor grows; `toh` = 1 always fits).
// Images are addressed through 64-bit offsets; offsets inside LDS and inside a tile are 32-bit.
#include "mbn_internal.h"

#include <new>

namespace {

constexpr int RESIZE_WAVES = 4;
constexpr int RESIZE_TOW = 64;               // output columns of a tile at most (32 when the output is no wider)
constexpr int RESIZE_EPL = RESIZE_TOW * 3 / 64;   // horizontal sums of a row per lane at most
constexpr int RESIZE_TOH = 32;               // output rows of a tile at most
constexpr int RESIZE_LDS = 60 * 1024;
constexpr int RESIZE_HALF = 1 << 21, RESIZE_SHIFT = 22;

struct ResizeArgs {
    uint8_t *out;
    const uint8_t *in;
    const int32_t *fx, *cx, *wx, *fy, *cy, *wy;
    int h, w, oh, ow, kx, ky;
    int tow, toh, tiles_x;
    int seg_stride;          // bytes of a wave's staged source row: the longest segment + kx pixels of slack + 3 (the address's offset in its dword), a multiple of 4
    int stage_off, tmp_off;  // LDS byte offsets behind the weights
};

// orders a wave's LDS writes before its later LDS reads (and the reverse) for data that only this wave touches
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint8_t resize_round(int acc)
{
    return (uint8_t)min(max(acc >> RESIZE_SHIFT, 0), 255);
}

__global__ __launch_bounds__(256, 8) void resize_u8(const ResizeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];
    int32_t *s_wx = reinterpret_cast<int32_t *>(s_mem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = (int)blockIdx.x / a.tiles_x, tx = (int)blockIdx.x - ty * a.tiles_x;
    const int ox0 = tx * a.tow, oxn = min(a.tow, a.ow - ox0), oy0 = ty * a.toh, oyn = min(a.toh, a.oh - oy0);
    const int row_e = oxn * 3;                                   // horizontal sums of a source row
    // first and count grow with the output index, so the tile's first and last outputs bound its window
    const int xs0 = a.fx[ox0], xs1 = a.fx[ox0 + oxn - 1] + a.cx[ox0 + oxn - 1];
    const int y0 = a.fy[oy0], y1 = a.fy[oy0 + oyn - 1] + a.cy[oy0 + oyn - 1];
    const int nrows = y1 - y0, nb = (xs1 - xs0) * 3;
    const size_t img = (size_t)blockIdx.y;
    const uint8_t *__restrict__ src = a.in + img * ((size_t)a.h * a.w * 3);
    uint8_t *__restrict__ dst = a.out + img * ((size_t)a.oh * a.ow * 3);
    uint8_t *s_row = s_mem + a.stage_off + wave * a.seg_stride;
    uint8_t *s_tmp = s_mem + a.tmp_off;
    const int tmp_ld = a.tow * 3;

    for (int e = tid; e < oxn * a.kx; e += 256) s_wx[e] = a.wx[ox0 * a.kx + e];
    // this lane's horizontal sums: element e = lane + 64 j of a row is column e / 3, channel e % 3
    int lo[RESIZE_EPL], wofs[RESIZE_EPL];
#pragma unroll
    for (int j = 0; j < RESIZE_EPL; j++) {
        const int e = lane + 64 * j, ox = e / 3;
        const bool on = e < row_e;
        lo[j] = on ? (a.fx[ox0 + ox] - xs0) * 3 + (e - 3 * ox) : 0;
        wofs[j] = ox * a.kx;
    }

    __syncthreads();                                             // the weights are in place
    // ---- horizontal: wave v takes rows y0 + v, y0 + v + 4, ... The staged row is the wave's own and a wave's LDS accesses complete in the order it
    // issues them, so between staging and summing only the compiler has to keep that order (wave_sync); the waves do not wait for each other
    for (int r = wave; r < nrows; r += RESIZE_WAVES) {
        const uint8_t *g = src + ((size_t)(y0 + r) * a.w + xs0) * 3;
        const int off = (int)((uintptr_t)g & 3);                 // byte j of the segment goes to s_row[off + j]: a dword of memory is a dword of LDS
        const int head = min(nb, (4 - off) & 3), body = (nb - head) >> 2, tail0 = head + 4 * body;
        if (lane < head) s_row[off + lane] = g[lane];
        for (int i = lane; i < body; i += 64)
            *reinterpret_cast<uint32_t *>(s_row + off + head + 4 * i) = *reinterpret_cast<const uint32_t *>(g + head + 4 * i);
        if (tail0 + lane < nb) s_row[off + tail0 + lane] = g[tail0 + lane];
        wave_sync();
#pragma unroll
        for (int j = 0; j < RESIZE_EPL; j++) {
            const int e = lane + 64 * j;
            if (e < row_e) {
                int acc = RESIZE_HALF;
                const uint8_t *p = s_row + off + lo[j];
                const int32_t *k = s_wx + wofs[j];
                for (int t = 0; t < a.kx; t++) acc += (int)p[3 * t] * k[t];      // past this column's count: a zero weight times a byte of the slack
                s_tmp[r * tmp_ld + e] = resize_round(acc);
            }
        }
        wave_sync();                                             // the next row is staged over this one
    }
    __syncthreads();                                             // the window is complete

    // ---- vertical: wave v takes output rows v, v + 4, ... of the tile, a lane the bytes lane, lane + 64, lane + 128 of the row's segment. The row is the
    // wave's, so its first row, count and weights are scalars
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    int idx[RESIZE_EPL];
#pragma unroll
    for (int j = 0; j < RESIZE_EPL; j++) idx[j] = lane + 64 * j < row_e ? lane + 64 * j : 0;
    for (int oy = wv; oy < oyn; oy += RESIZE_WAVES) {
        const int n = a.cy[oy0 + oy];
        const int32_t *__restrict__ k = a.wy + (size_t)(oy0 + oy) * a.ky;
        const uint8_t *p = s_tmp + (a.fy[oy0 + oy] - y0) * tmp_ld;
        int acc[RESIZE_EPL];
#pragma unroll
        for (int j = 0; j < RESIZE_EPL; j++) acc[j] = RESIZE_HALF;
        for (int t = 0; t < n; t++) {
            const int kt = k[t];
#pragma unroll
            for (int j = 0; j < RESIZE_EPL; j++) acc[j] += (int)p[t * tmp_ld + idx[j]] * kt;
        }
        uint8_t *d = dst + ((size_t)(oy0 + oy) * a.ow + ox0) * 3;
#pragma unroll
        for (int j = 0; j < RESIZE_EPL; j++)
            if (lane + 64 * j < row_e) d[lane + 64 * j] = resize_round(acc[j]);
    }
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

// most source positions a tile of `t` outputs reaches along an axis
int axis_window(const int32_t *first, const int32_t *count, int out_size, int t)
{
    int most = 0;
    for (int o = 0; o < out_size; o += t) {
        const int last = (o + t < out_size ? o + t : out_size) - 1;
        const int span = first[last] + count[last] - first[o];
        if (span > most) most = span;
    }
    return most;
}

}   // namespace

// The geometry is inside mbn_resize_envelope (the caller has checked it). Builds the tables, picks the tile and uploads: blocking.
int mbn_resizer_build(mbn_context *ctx, int in_rows, int in_cols, const float *box, int out_rows, int out_cols, mbn_resizer **out)
{
    const float whole[4] = { 0.0f, 0.0f, (float)in_cols, (float)in_rows };
    const float *b = box ? box : whole;
    const int kx = mbn_resize_ksize(in_cols, b[0], b[2], out_cols), ky = mbn_resize_ksize(in_rows, b[1], b[3], out_rows);
    if (kx < 0 || ky < 0) return kx < 0 ? kx : ky;
    // one host block, the layout of the device block: fx, cx, fy, cy, wx, wy
    const size_t n32 = 2 * (size_t)out_cols + 2 * (size_t)out_rows + (size_t)out_cols * kx + (size_t)out_rows * ky;
    std::vector<int32_t> tab;
    try { tab.resize(n32); } catch (const std::bad_alloc &) { return MBN_ENOMEM; }
    int32_t *fx = tab.data(), *cx = fx + out_cols, *fy = cx + out_cols, *cy = fy + out_rows, *wx = cy + out_rows, *wy = wx + (size_t)out_cols * kx;
    int rc = mbn_resize_taps(in_cols, b[0], b[2], out_cols, fx, cx, wx);
    if (rc >= 0) rc = mbn_resize_taps(in_rows, b[1], b[3], out_rows, fy, cy, wy);
    if (rc < 0) return rc;
    if (!axis_ok(fx, cx, out_cols, in_cols, kx) || !axis_ok(fy, cy, out_rows, in_rows, ky)) return MBN_EINVAL;

    mbn_resizer *r = new (std::nothrow) mbn_resizer();
    if (!r) return MBN_ENOMEM;
    r->ctx = ctx;
    r->in_rows = in_rows; r->in_cols = in_cols; r->out_rows = out_rows; r->out_cols = out_cols;
    r->kx = kx; r->ky = ky;
    r->tow = out_cols <= RESIZE_TOW / 2 ? RESIZE_TOW / 2 : RESIZE_TOW;
    const int wx_bytes = (r->tow * kx * 4 + 15) & ~15;
    r->seg_stride = ((axis_window(fx, cx, out_cols, r->tow) + kx) * 3 + 3 + 3) & ~3;      // + kx pixels of slack: the horizontal loop runs kx taps for every column
    r->stage_off = wx_bytes;
    r->tmp_off = (wx_bytes + RESIZE_WAVES * r->seg_stride + 15) & ~15;
    // the tallest tile whose window fits; one output row reaches at most ky <= 67 source rows: 13 KB of window, which always fits
    r->toh = out_rows < RESIZE_TOH ? out_rows : RESIZE_TOH;
    while (r->toh > 1 && r->tmp_off + axis_window(fy, cy, out_rows, r->toh) * r->tow * 3 > RESIZE_LDS) r->toh--;
    r->lds_bytes = r->tmp_off + axis_window(fy, cy, out_rows, r->toh) * r->tow * 3;
    if (r->lds_bytes > RESIZE_LDS) { delete r; return MBN_EUNSUPPORTED; }
    r->tiles_x = (out_cols + r->tow - 1) / r->tow;
    r->tiles_y = (out_rows + r->toh - 1) / r->toh;

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

void mbn_resizer_release(mbn_resizer *r)
{
    if (r->tables) (void)hipFree(r->tables);
    delete r;
}

// in [batch][in_rows][in_cols][3] -> out [batch][out_rows][out_cols][3]; batch in 1..MBN_RESIZE_MAX_BATCH, pointers non-null (the caller has checked)
int mbn_launch_u8_resize(const mbn_resizer *r, hipStream_t s, uint8_t *out, const uint8_t *in, int batch)
{
    ResizeArgs a;
    a.out = out; a.in = in;
    const int32_t *t = (const int32_t *)r->tables;
    a.fx = t; a.cx = a.fx + r->out_cols; a.fy = a.cx + r->out_cols; a.cy = a.fy + r->out_rows;
    a.wx = a.cy + r->out_rows; a.wy = a.wx + (size_t)r->out_cols * r->kx;
    a.h = r->in_rows; a.w = r->in_cols; a.oh = r->out_rows; a.ow = r->out_cols; a.kx = r->kx; a.ky = r->ky;
    a.tow = r->tow; a.toh = r->toh; a.tiles_x = r->tiles_x;
    a.seg_stride = r->seg_stride; a.stage_off = r->stage_off; a.tmp_off = r->tmp_off;
    hipLaunchKernelGGL(resize_u8, dim3((unsigned)(r->tiles_x * r->tiles_y), (unsigned)batch), dim3(256), (size_t)r->lds_bytes, s, a);
    return MBN_OK;
}
