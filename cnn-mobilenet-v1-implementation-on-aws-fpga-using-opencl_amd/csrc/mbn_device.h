// mbn_device.h — the device helpers every kernel file shares: vector types, buffer descriptors, the persistent grids' tile
// order, the LDS swizzles, bf16 widening, the ReLU6 epilogue, counted waits and the 16-byte store hazard. Several of these are
// formats the kernels must agree on byte for byte (the fused blocks' LDS image is that of pw_gemm), so each has one definition.
// What only a family of kernels shares sits on top of this header: mbn_epilogue.h (buffer-store epilogues), mbn_block_window.h (the fused
// blocks' window offsets and prologue), mbn_x6.h (the pw_emul kernels' operand split and product list).
#pragma once

#include <hip/hip_runtime.h>

typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));     // C/D of v_mfma_f32_32x32x*: 16 accumulators per lane
typedef unsigned u2 __attribute__((ext_vector_type(2)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef int i4v __attribute__((ext_vector_type(4)));
typedef int i16v __attribute__((ext_vector_type(16)));

__device__ __forceinline__ __amdgpu_buffer_rsrc_t mbn_make_rsrc(const void *base, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, bytes, 0x00020000);
}

// virtual block id -> logical tile id of a persistent grid: ids that share vb % 8 (one XCD) get a contiguous range of tiles
// (bijective for any tile count, cdna guide T1)
__device__ __forceinline__ int mbn_xcd_remap(int vb, int nwg)
{
    const int q8 = nwg >> 3, r8 = nwg & 7, xcd = vb & 7;
    return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (vb >> 3);
}

// LDS word offset of 16-byte chunk `chunk` of row `row` in a tile of 128-byte rows (32 words), chunks XORed by row / 2:
// the layout of pw_gemm's tiles, which the fused blocks reproduce byte for byte
__device__ __forceinline__ int mbn_swz(int row, int chunk) { return (row << 5) + (((chunk ^ (row >> 1)) & 7) << 2); }
// the split-operand (x6) form: one bf16 plane row is 64 bytes (16 words), 16-byte chunks XORed by row / 4
__device__ __forceinline__ int mbn_pswz(int row, int c) { return row * 16 + (((c ^ (row >> 2)) & 3) << 2); }

// 8 packed bf16 -> 8 fp32 (exact: a shift or a mask per element)
__device__ __forceinline__ f8 mbn_widen8(u4 p)
{
    f8 r;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        r[2 * i] = __builtin_bit_cast(float, p[i] << 16);
        r[2 * i + 1] = __builtin_bit_cast(float, p[i] & 0xffff0000u);
    }
    return r;
}
__device__ __forceinline__ f8 mbn_ld8(const float *p)
{
    const f4 a = *reinterpret_cast<const f4 *>(p), b = *reinterpret_cast<const f4 *>(p + 4);
    return f8{ a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
}

__device__ __forceinline__ float mbn_relu6(float v) { return fminf(fmaxf(v, 0.f), 6.f); }
// BN + ReLU6 of 4 channels, one fmaf per component
__device__ __forceinline__ f4 mbn_bn_relu6(f4 a, f4 s, f4 b)
{
    return f4{ mbn_relu6(fmaf(a.x, s.x, b.x)), mbn_relu6(fmaf(a.y, s.y, b.y)), mbn_relu6(fmaf(a.z, s.z, b.z)), mbn_relu6(fmaf(a.w, s.w, b.w)) };
}

__device__ __forceinline__ void mbn_st4(float *p, f4 v) { *reinterpret_cast<f4 *>(p) = v; }
__device__ __forceinline__ void mbn_st4(__bf16 *p, f4 v)
{
    *reinterpret_cast<bf4 *>(p) = bf4{ (__bf16)v.x, (__bf16)v.y, (__bf16)v.z, (__bf16)v.w };   // RNE
}

// Counted wait, by default followed by the workgroup barrier: wait until at most VM_LEFT vector-memory operations of this wave
// are outstanding (VM_LEFT < 0: no vmcnt wait), with LGKM until its LDS operations are done (lgkmcnt(0)), then, with BAR,
// s_barrier. Why not __syncthreads(): it is a workgroup-scope fence over every address space, and with global loads in flight
// the waitcnt pass drains them (s_waitcnt vmcnt(0)) in front of every barrier (also with the "local"-only fence form). That
// serialises a prefetch issued for the NEXT step with the hand-over of this one. A counted wait lets the VM_LEFT youngest
// operations (the prefetch, stores of an earlier epilogue) stay in flight while the older ones it guards (an LDS-DMA) have
// landed: vmcnt retires in order. The asm is volatile with a memory clobber, so the compiler moves no LDS or global access
// across it.
template <int VM_LEFT, bool BAR = true, bool LGKM = true>
__device__ __forceinline__ void mbn_waitcnt()
{
    static_assert(VM_LEFT < 64, "vmcnt is a 6-bit field");
    static_assert(VM_LEFT >= 0 || (BAR && LGKM), "the form without a vmcnt wait is lgkmcnt(0) + s_barrier");
    if constexpr (VM_LEFT < 0) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else if constexpr (BAR && LGKM) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(VM_LEFT) : "memory");
    else if constexpr (LGKM) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(VM_LEFT) : "memory");
    else if constexpr (BAR) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(VM_LEFT) : "memory");
    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VM_LEFT) : "memory");
}

// gfx950 store-data hazard (found in mbn_f32_dwpw3.hip, profiles/r06/a_*): a buffer_store_dwordx4 followed directly by a VALU
// write of its first data register stores the NEW value in lanes 12-15 of every 16 (the ">64-bit store data" hazard). LLVM pads
// only the immediate-soffset form, not a store whose soffset is an SGPR. So the 16-byte stores go out in pairs behind a
// sched_barrier(0), and this follows each pair: two wait states, and nothing is scheduled across them.
__device__ __forceinline__ void mbn_store_hazard_wait()
{
    asm volatile("s_nop 1" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
