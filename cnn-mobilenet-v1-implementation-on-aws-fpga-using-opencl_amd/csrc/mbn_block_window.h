// mbn_block_window.h — the address arithmetic the fused depthwise -> pointwise block kernels share (mbn_f32_dwpw*.hip, mbn_bf16_dwpw*.hip):
// output pixel -> byte offsets of its 3 x XC input window, in the general and in the full-rate form, and the unified-wave kernels' copy of
// the block's constants into LDS. The kernels differ in bytes per element, channels per lane and lane masks; those are arguments here.
//
// Common to every helper:
//   S, XC   depthwise stride and input columns feeding a lane's 2 adjacent output pixels (XC = S + 3)
//   a       the kernel's argument struct; read are the geometry fields the structs name alike (mbn_block_args): h, w, ho, wo, pad_top, pad_left,
//           wo_m, wo_s, ho_m, ho_s and, in the full-rate form, inv_wo, inv_ho
//   cs      pixel stride of the input in bytes (Cin x element size)
//   cb      byte offset of the lane's first channel inside a pixel
// A tap outside the image (or of a lane that is masked out) gets an offset beyond the descriptor's num_records: the buffer unit returns zeros
// there, so zero padding costs no VALU and no branches.
#pragma once

#include "mbn_device.h"
#include "mbn_envelope.h"

// General form: valid for every shape inside mbn_block_envelope. m = the lane's first output pixel of mtot; lane_ok = false masks the lane
// out whatever its pixel (bf16, Cin = 32: lanes whose channels do not exist).
// (n, y, x) of the pixel by multiply-high division (host-computed magic numbers), then every tap offset as base + dy * row stride + j * column
// stride: this runs once per tile per lane and used to cost ~400 VALU instructions (two 32-bit divisions + 12-15 independent offset
// computations). Still two v_mul_hi_u32 and six v_mul_lo_u32 (quarter rate), a 64-bit mad, and 12-15 compare / select pairs under exec-mask
// branches: ~1100-1250 cycles per tile on a SIMD's two waves in the stamps (profiles/r05/d_*).
template <int S, int XC, typename Args>
__device__ __forceinline__ void mbn_window_offsets(unsigned (&off)[3][XC], const Args &a, unsigned cs, unsigned cb, unsigned m, unsigned mtot, bool lane_ok)
{
    const bool ok = m < mtot && lane_ok;
    const unsigned q = a.wo_m ? __umulhi(m, a.wo_m) >> a.wo_s : m;
    const unsigned x = m - q * (unsigned)a.wo;
    const unsigned n = a.ho_m ? __umulhi(q, a.ho_m) >> a.ho_s : q;
    const unsigned y = q - n * (unsigned)a.ho;
    const int iy0 = (int)y * S - a.pad_top, ix0 = (int)x * S - a.pad_left;
    const unsigned rs = (unsigned)a.w * cs;                                               // row stride in bytes
    const unsigned base = ((n * a.h + iy0) * a.w + ix0) * cs + cb;                        // wraps for taps that are masked out below
#pragma unroll
    for (int dy = 0; dy < 3; dy++) {
        const bool rok = ok && (unsigned)(iy0 + dy) < (unsigned)a.h;
#pragma unroll
        for (int j = 0; j < XC; j++) {
            const bool tap = rok && (unsigned)(ix0 + j) < (unsigned)a.w;
            off[dy][j] = tap ? base + dy * rs + j * cs : MBN_OOB;
        }
    }
}

// Full-rate form, legal exactly where mbn_block_fast_offsets (host/mbn_envelope.c) says so; the offset of tap (dy, j) is rowv[dy] + colv[j].
// The tail: from the lane's pixel (image n, output row y, column x) and ok = the pixel exists and the lane is not masked out. ONE 32-bit multiply for the byte offset ((n h + iy0) < 2^23,
// w < 2^16: __mul24); validity separable by row and column: an invalid row is MBN_OFF_BAD_ROW and an invalid column MBN_OFF_BAD_COL, so that any
// sum with an invalid term lies in [MBN_OFF_BAD_COL, 0xF0005000) — beyond num_records (the input plus a left-pad column ends below
// MBN_OFF_BAD_COL) and without wrapping. Same offsets as the general form for every valid tap, zeros for every other: bit-identical results.
template <int S, int XC, typename Args>
__device__ __forceinline__ void mbn_window_rowcol(unsigned (&rowv)[3], unsigned (&colv)[XC], const Args &a, unsigned cs, unsigned cb, unsigned n,
                                                  unsigned y, unsigned x, bool ok)
{
    const int iy0 = (int)y * S - a.pad_top, ix0 = (int)x * S - a.pad_left;
    const unsigned rs = (unsigned)a.w * cs;
    const int pix = __mul24((int)(n * (unsigned)a.h) + iy0, a.w) + ix0;
    const unsigned base = (unsigned)pix * cs + cb;
#pragma unroll
    for (int dy = 0; dy < 3; dy++) rowv[dy] = (ok && (unsigned)(iy0 + dy) < (unsigned)a.h) ? base + dy * rs : MBN_OFF_BAD_ROW;
#pragma unroll
    for (int j = 0; j < XC; j++) colv[j] = ((unsigned)(ix0 + j) < (unsigned)a.w) ? j * cs : MBN_OFF_BAD_COL;
}

// The whole full-rate form for a tile of consecutive pixels: m0 = the tile's first pixel (wave-uniform), dm = the lane's first pixel inside the
// tile (< 256). (n, y, x) of m0 on the scalar unit (magic division); the lane's own pixel from it by two float reciprocal divisions of small
// numbers (r < wo + 256, exact: (r + 0.5) / wo is >= 0.5 / wo away from an integer, the float error is < 2e-5; q1 < 2^8 and wo < 2^16 are in
// mul24 range; a tile that spans several images has q2 > 0), then the tail above.
template <int S, int XC, typename Args>
__device__ __forceinline__ void mbn_window_offsets_fast(unsigned (&off)[3][XC], const Args &a, unsigned cs, unsigned cb, unsigned m0, unsigned dm, unsigned mtot,
                                                        bool lane_ok)
{
    const unsigned q0 = a.wo_m ? __umulhi(m0, a.wo_m) >> a.wo_s : m0;                      // wave-uniform: scalar unit
    const unsigned x0 = m0 - q0 * (unsigned)a.wo;
    const unsigned n0 = a.ho_m ? __umulhi(q0, a.ho_m) >> a.ho_s : q0;
    const unsigned y0 = q0 - n0 * (unsigned)a.ho;
    const unsigned r = x0 + dm;
    const unsigned q1 = (unsigned)__builtin_fmaf((float)r, a.inv_wo, 0.5f * a.inv_wo);
    const unsigned x = r - q1 * (unsigned)a.wo;
    const unsigned yy = y0 + q1;
    const unsigned q2 = (unsigned)__builtin_fmaf((float)yy, a.inv_ho, 0.5f * a.inv_ho);
    const unsigned y = yy - q2 * (unsigned)a.ho;
    const unsigned n = n0 + q2;
    unsigned rowv[3], colv[XC];
    mbn_window_rowcol<S>(rowv, colv, a, cs, cb, n, y, x, m0 + dm < mtot && lane_ok);
#pragma unroll
    for (int dy = 0; dy < 3; dy++)
#pragma unroll
        for (int j = 0; j < XC; j++) off[dy][j] = rowv[dy] + colv[j];
}

// Prologue of the unified-wave kernels (NT threads): the depthwise taps wd[9][cin], scale | shift s2 | b2 and the pointwise scale, shift s3, b3
// of the whole block into LDS at wd_s — 9 CM + 2 CM + NO + NO floats, the layout the kernels carve — then the workgroup barrier.
template <int NT, int CM, int NO, typename Args>
__device__ __forceinline__ void mbn_block_constants_to_lds(const Args &a, int tid, float *wd_s)
{
    float *const sb_s = wd_s + 9 * CM, *const sc3_s = sb_s + 2 * CM, *const sh3_s = sc3_s + NO;
    for (int i = tid * 4; i < 9 * a.cin; i += NT * 4) *reinterpret_cast<f4 *>(wd_s + i) = *reinterpret_cast<const f4 *>(a.wd + i);
    for (int i = tid * 4; i < a.cin; i += NT * 4) {
        *reinterpret_cast<f4 *>(sb_s + i) = *reinterpret_cast<const f4 *>(a.s2 + i);
        *reinterpret_cast<f4 *>(sb_s + a.cin + i) = *reinterpret_cast<const f4 *>(a.b2 + i);
    }
    for (int i = tid; i < a.cout; i += NT) { sc3_s[i] = a.s3[i]; sh3_s[i] = a.b3[i]; }
    __syncthreads();
}
