// mbn_u8_resize.h — the tile body of the resize front-end on gfx950, shared by the table kernel (mbn_u8_resize.hip) and the ragged kernel
// (mbn_u8_resize_ragged.hip): Pillow's 8-bit resize of a box of a uint8 HWC image, both passes in ONE launch (include/mbn.h, "resize
// front-end", is the normative statement of the arithmetic). Each kernel brings its own geometry and its own source of first / count / weights.
// The filter is in the weights alone (bilinear, box, hamming, bicubic, lanczos): nothing here assumes a weight >= 0 or a row of them summing to
// 2^22, and both passes clamp. MBN_FILTER_NEAREST has no weights and its own body at the end of this file (resize_nearest_rows).
//
// A workgroup of 256 lanes (MBN_RESIZE_WAVES waves) owns a tile of `toh` output rows x `tow` output columns of one image. The taps say which source
// rows [y0, y1) and columns [xs0, xs1) the tile needs, and nothing else is read:
//   horizontal  the waves take the source rows of the window in turn (wave v the rows y0 + v, y0 + v + 4, ...), each at its own pace. A wave stages its
//               row's segment [xs0, xs1) in LDS (resize_stage_row) and then forms the tile's `tow` x 3 horizontal sums of that row from LDS, each rounded
//               to uint8 as Pillow rounds its intermediate image, into the window s_tmp [y1 - y0][tow * 3] in LDS (resize_row_sums). The tile's horizontal
//               weights sit in LDS as well, and every column runs all kx taps: those past its count carry zero padding (the staged row has kx pixels of
//               slack for them). The staged row is the wave's own and a wave's LDS accesses complete in the order it issues them, so between staging and
//               summing only the compiler has to keep that order (wave_sync); the waves do not wait for each other;
//   vertical    behind a barrier the waves take the tile's output rows in turn (resize_vertical): a row's first source row, count and weights are scalars of
//               the wave, a lane sums three bytes of the row's segment over s_tmp, rounds to uint8 and stores (consecutive lanes, consecutive bytes).
// The uint8 intermediate never reaches memory. The host sizes the tile so that tables + 4 staged rows + window fit MBN_RESIZE_LDS bytes
// (host/mbn_resize.c; a 32x downscale has 67 taps per axis: its window alone is 67 + rows, so tiles get flatter as the factor grows; `toh` = 1 always
// fits). Images are addressed through 64-bit offsets; offsets inside LDS and inside a tile are 32-bit.
#pragma once
#include "mbn_internal.h"

namespace {

constexpr int RESIZE_EPL = MBN_RESIZE_TOW(MBN_RESIZE_MAX_OUT) * 3 / 64;      // horizontal sums of a row per lane at most

// orders a wave's LDS writes before its later LDS reads (and the reverse) for data that only this wave touches
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint8_t resize_round(int acc)
{
    return (uint8_t)min(max(acc >> MBN_RESIZE_BITS, 0), 255);
}

// This lane's horizontal sums: element e = lane + 64 j of a row of the tile (row_e of them) is column e / 3, channel e % 3. lo[j] = its first byte in
// the staged segment, wofs[j] = its weights in s_wx [tow][kx]; first(column) = the column's first source column, counted from the segment's
template <class First>
__device__ __forceinline__ void resize_lane_elems(int (&lo)[RESIZE_EPL], int (&wofs)[RESIZE_EPL], int lane, int row_e, int kx, First first)
{
#pragma unroll
    for (int j = 0; j < RESIZE_EPL; j++) {
        const int e = lane + 64 * j, ox = e / 3;
        const bool on = e < row_e;
        lo[j] = on ? first(ox) * 3 + (e - 3 * ox) : 0;
        wofs[j] = on ? ox * kx : 0;
    }
}

// Stages the nb bytes at g in the wave's row and returns where byte 0 went: bytewise up to the first 4-byte boundary of the ADDRESS, 4 bytes per lane
// from there, bytewise for the rest, so any byte pointer and any W * 3 give the same bytes. s_row is on 4 bytes and has nb + 3 bytes of room
__device__ __forceinline__ const uint8_t *resize_stage_row(uint8_t *s_row, const uint8_t *g, int nb, int lane)
{
    const int off = (int)((uintptr_t)g & 3);                     // byte j of the segment goes to s_row[off + j]: a dword of memory is a dword of LDS
    const int head = min(nb, (4 - off) & 3), body = (nb - head) >> 2, tail0 = head + 4 * body;
    if (lane < head) s_row[off + lane] = g[lane];
    for (int i = lane; i < body; i += 64)
        *reinterpret_cast<uint32_t *>(s_row + off + head + 4 * i) = *reinterpret_cast<const uint32_t *>(g + head + 4 * i);
    if (tail0 + lane < nb) s_row[off + tail0 + lane] = g[tail0 + lane];
    wave_sync();
    return s_row + off;
}

// the horizontal sums of the staged row s_seg into its row s_out of the window
__device__ __forceinline__ void resize_row_sums(uint8_t *s_out, const uint8_t *s_seg, const int32_t *s_wx, const int (&lo)[RESIZE_EPL],
                                                const int (&wofs)[RESIZE_EPL], int kx, int row_e, int lane)
{
#pragma unroll
    for (int j = 0; j < RESIZE_EPL; j++) {
        const int e = lane + 64 * j;
        if (e < row_e) {
            int acc = MBN_RESIZE_HALF;
            const uint8_t *p = s_seg + lo[j];
            const int32_t *k = s_wx + wofs[j];
            for (int t = 0; t < kx; t++) acc += (int)p[3 * t] * k[t];            // past this column's count: a zero weight times a byte of the slack
            s_out[e] = resize_round(acc);
        }
    }
    wave_sync();                                                 // the next row is staged over this one
}

// The vertical pass out of the finished window s_tmp [rows][tmp_ld]: wave v takes output rows v, v + 4, ... of the tile's oyn, a lane the bytes lane,
// lane + 64, lane + 128 of the row's row_e. dst = the tile's first output byte, dst_ld = bytes of an output row. row(oy, f, n) gives the row's weights
// and sets f = its first row in the window and n = its count: the row is the wave's, so all three are the same for all its lanes. dst is __restrict__
// (the output is no table and no LDS): only then can the compiler prove that the stores leave the table kernel's counts and weights alone and read
// them with scalar loads (s_load_dwordx8 for eight taps); without it they are per-lane loads of one address and a v_readfirstlane
template <class Row>
__device__ __forceinline__ void resize_vertical(uint8_t *__restrict__ dst, size_t dst_ld, const uint8_t *s_tmp, int tmp_ld, int oyn, int row_e, int lane,
                                                int wave, Row row)
{
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    int idx[RESIZE_EPL];
#pragma unroll
    for (int j = 0; j < RESIZE_EPL; j++) idx[j] = lane + 64 * j < row_e ? lane + 64 * j : 0;
    for (int oy = wv; oy < oyn; oy += MBN_RESIZE_WAVES) {
        int f, n;
        const int32_t *__restrict__ k = row(oy, f, n);
        const uint8_t *p = s_tmp + f * tmp_ld;
        int acc[RESIZE_EPL];
#pragma unroll
        for (int j = 0; j < RESIZE_EPL; j++) acc[j] = MBN_RESIZE_HALF;
        for (int t = 0; t < n; t++) {
            const int kt = k[t];
#pragma unroll
            for (int j = 0; j < RESIZE_EPL; j++) acc[j] += (int)p[t * tmp_ld + idx[j]] * kt;
        }
        uint8_t *d = dst + oy * dst_ld;
#pragma unroll
        for (int j = 0; j < RESIZE_EPL; j++)
            if (lane + 64 * j < row_e) d[lane + 64 * j] = resize_round(acc[j]);
    }
}

// MBN_FILTER_NEAREST, the rows of a tile: a gather of 3-byte pixels and nothing else. Wave v takes output rows v, v + 4, ... of the tile's oyn; a row's
// segment is row_e consecutive bytes at dst + oy * dst_ld, byte e of it channel e % 3 of the source pixel (iy(oy), ix(e / 3)) of src [..][w][3]
// (ix, iy: the tile's indices, already inside the source). Stored as resize_stage_row loads: bytewise up to the first 4-byte boundary of the
// ADDRESS, a dword per lane from there (consecutive lanes, consecutive dwords), bytewise for the rest, so any byte pointer and any ow * 3 write
// the same bytes and none beside them
template <class Ix, class Iy>
__device__ __forceinline__ void resize_nearest_rows(uint8_t *__restrict__ dst, size_t dst_ld, const uint8_t *__restrict__ src, int w, int oyn, int row_e,
                                                    int lane, int wave, Ix ix, Iy iy)
{
    for (int oy = wave; oy < oyn; oy += MBN_RESIZE_WAVES) {
        uint8_t *d = dst + oy * dst_ld;
        const uint8_t *row = src + (size_t)iy(oy) * w * 3;
        auto byte = [&](int e) -> uint32_t { const int p = e / 3; return row[ix(p) * 3 + (e - 3 * p)]; };
        const int off = (int)((uintptr_t)d & 3);
        const int head = min(row_e, (4 - off) & 3), body = (row_e - head) >> 2, tail0 = head + 4 * body;
        if (lane < head) d[lane] = (uint8_t)byte(lane);
        for (int i = lane; i < body; i += 64) {
            const int e = head + 4 * i;
            *reinterpret_cast<uint32_t *>(d + e) = byte(e) | byte(e + 1) << 8 | byte(e + 2) << 16 | byte(e + 3) << 24;
        }
        if (tail0 + lane < row_e) d[tail0 + lane] = (uint8_t)byte(tail0 + lane);
    }
}

// The letterbox's border (mbn_fit_pad, include/mbn.h): the fill colour as the three dwords an RGB run can start with. w[c] holds channels c, c + 1, c + 2, c
// (mod 3) from its low byte up: what the four bytes at a position of channel c are, and its low byte is channel c itself
struct ResizeFill {
    uint32_t w[3];
};

inline ResizeFill resize_fill_of(const uint8_t rgb[3])
{
    ResizeFill f;
    for (int c = 0; c < 3; c++)
        f.w[c] = (uint32_t)rgb[c] | (uint32_t)rgb[(c + 1) % 3] << 8 | (uint32_t)rgb[(c + 2) % 3] << 16 | (uint32_t)rgb[c] << 24;
    return f;
}

// nb bytes of fill at d, byte 0 a pixel's first channel (every border run starts with a pixel). The store shape of resize_nearest_rows: bytewise up to
// the first 4-byte boundary of the ADDRESS, a dword per lane from there, bytewise for the rest, so any byte pointer works and no byte beside the run is
// touched. One wave; nothing is read
__device__ __forceinline__ void resize_fill_run(uint8_t *__restrict__ d, int nb, const ResizeFill &f, int lane)
{
    auto word = [&](int e) -> uint32_t { const int c = e % 3; return c == 0 ? f.w[0] : c == 1 ? f.w[1] : f.w[2]; };
    const int off = (int)((uintptr_t)d & 3);
    const int head = min(nb, (4 - off) & 3), body = (nb - head) >> 2, tail0 = head + 4 * body;
    if (lane < head) d[lane] = (uint8_t)word(lane);
    for (int i = lane; i < body; i += 64) *reinterpret_cast<uint32_t *>(d + head + 4 * i) = word(head + 4 * i);
    if (tail0 + lane < nb) d[tail0 + lane] = (uint8_t)word(tail0 + lane);
}

// Border rows k0 .. k0 + MBN_RESIZE_FILL_ROWS - 1 (below fill_rows) of one oh x ow canvas around the rectangle (x, y, iw, ih), which lies inside it
// (mbn_fit_pad): wave v takes the rows k0 + v, k0 + v + 4, ... A row outside the rectangle is one run of ow pixels, a row through it the runs left
// and right of it. What is inside the rectangle is the tiles' to write
__device__ __forceinline__ void resize_fill_rows(uint8_t *__restrict__ canvas, int ow, int x, int y, int iw, int ih, int k0, int fill_rows,
                                                 const ResizeFill &f, int lane, int wave)
{
    const int kn = min(k0 + MBN_RESIZE_FILL_ROWS, fill_rows);
    for (int k = k0 + wave; k < kn; k += MBN_RESIZE_WAVES) {
        const int r = MBN_RESIZE_FILL_ROW(k, y, iw, ih, ow);
        uint8_t *d = canvas + (size_t)r * ow * 3;
        if (r < y || r >= y + ih) {
            resize_fill_run(d, ow * 3, f, lane);
        } else {
            resize_fill_run(d, x * 3, f, lane);
            resize_fill_run(d + (x + iw) * 3, (ow - x - iw) * 3, f, lane);
        }
    }
}

}   // namespace
