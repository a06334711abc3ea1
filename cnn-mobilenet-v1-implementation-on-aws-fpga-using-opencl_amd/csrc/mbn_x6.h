// mbn_x6.h — what the opt-in pw_emul kernels (mbn_f32_pw_x6.hip, mbn_f32_dwpw2_x6.hip, the X6 phase of mbn_f32_stem.hip) must agree on bit
// for bit: the exact three-way bf16 split of an fp32 value and the list of plane products. The kernels consume each other's data — the fused
// block and the stem multiply activations they split themselves by the filter image split_filter wrote — so each has one definition.
#pragma once

#include "mbn_device.h"

// x -> h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), two values per word (RNE; exact: h + m + l == x for 2^-110 <= |x| < 2^127,
// see mbn_f32_pw_x6.hip)
__device__ __forceinline__ void mbn_x6_split2(float x0, float x1, unsigned &h, unsigned &m, unsigned &l)
{
    const f2 v = f2{ x0, x1 };
    const bf2 hh = __builtin_convertvector(v, bf2);
    const f2 r = v - __builtin_convertvector(hh, f2);
    const bf2 mm = __builtin_convertvector(r, bf2);
    const f2 lo = r - __builtin_convertvector(mm, f2);
    h = __builtin_bit_cast(unsigned, hh);
    m = __builtin_bit_cast(unsigned, mm);
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(lo, bf2));
}
// 4 / 8 consecutive values -> 2 / 4 words of each plane (u2 / u4)
__device__ __forceinline__ void mbn_x6_split4(f4 v, u2 &h, u2 &m, u2 &l)
{
    const float x[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
    for (int j = 0; j < 2; j++) {
        unsigned hj, mj, lj;
        mbn_x6_split2(x[2 * j], x[2 * j + 1], hj, mj, lj);
        h[j] = hj; m[j] = mj; l[j] = lj;
    }
}
__device__ __forceinline__ void mbn_x6_split8(f4 v0, f4 v1, u4 &h, u4 &m, u4 &l)
{
    const float x[8] = { v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w };
#pragma unroll
    for (int j = 0; j < 4; j++) {
        unsigned hj, mj, lj;
        mbn_x6_split2(x[2 * j], x[2 * j + 1], hj, mj, lj);
        h[j] = hj; m[j] = mj; l[j] = lj;
    }
}

// product list of a k16-step: plane of A, plane of B (0 = h, 1 = m, 2 = l); smallest terms first
template <int NP> struct Prod;
template <> struct Prod<9> { static constexpr int pa[9] = { 2, 2, 1, 2, 0, 1, 1, 0, 0 }, pb[9] = { 2, 1, 2, 0, 2, 1, 0, 1, 0 }; };
template <> struct Prod<6> { static constexpr int pa[6] = { 2, 0, 1, 1, 0, 0 }, pb[6] = { 0, 2, 1, 0, 1, 0 }; };
#ifdef MBN_LAB
template <> struct Prod<3> { static constexpr int pa[3] = { 1, 0, 0 }, pb[3] = { 0, 1, 0 }; };      // measurement only: 2^-16
template <> struct Prod<1> { static constexpr int pa[1] = { 0 }, pb[1] = { 0 }; };                  // measurement only: bf16 operands
#endif
