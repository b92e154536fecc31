// Device primitives of the 16-bit kernels that stage their operands through LDS by DMA and multiply on the 32x32x16 MFMA:
// one definition of each, for every conv_*.hip that used to carry a prefixed copy.  Where two spellings are kept they generate
// different code and each says when it is the one to use.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef short s16x4_t __attribute__((ext_vector_type(4)));          // what the transposing LDS read returns

// ---------------------------------------------------------------- 32x32x16 MFMA
// D[i][j] += sum_k A[i][k] * B[j][k] over 16 k: every lane supplies 8 elements of its A row and 8 of its B row (lane = 32 h + r: row r,
// k-half h); D layout: lane holds D[i = 8 (reg >> 2) + 4 h + (reg & 3)][j = r].  (Elem<T>::ONES is the all-ones operand of the column sums.)
// run() accumulates in place; mad() returns the result, for an addend that is not the destination (conv_stem.hip starts from the bias).
template <typename T> struct Mma32;
template <> struct Mma32<__bf16> {
    static __device__ __forceinline__ void run(const i32x4_t& a, const i32x4_t& b, f32x16_t& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16_t mad(const i32x4_t& a, const i32x4_t& b, const f32x16_t& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    }
};
template <> struct Mma32<_Float16> {
    static __device__ __forceinline__ void run(const i32x4_t& a, const i32x4_t& b, f32x16_t& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x16_t mad(const i32x4_t& a, const i32x4_t& b, const f32x16_t& c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    }
};

// ---------------------------------------------------------------- LDS-DMA: 16 bytes per lane, memory -> LDS, no staging registers
// m0 = wave-uniform LDS destination; lane l lands at m0 + 16 l; voff = the lane's byte offset into the buffer (beyond num_records,
// e.g. URSO_OOB_SHIFT: zeros land).
// Why inline asm and not the builtin: through the builtin hipcc waits vmcnt(0) before the next LDS read of ANY buffer (it cannot tell the
// DMA's destination from the buffer being multiplied), which serialises the copy of K-tile k+1 with the MFMAs of K-tile k.  Issued behind
// the compiler's back, the copy is ordered by hand: wait_vm<N>() with N = the number of younger vector-memory operations, before the
// barrier that publishes the buffer.  Every compiler-visible load has to be consumed only after one of those hand-placed waits has
// covered it, so that the compiler's own (weaker) counts are harmless.
// m0 is not saved: nothing else in these kernels uses it (DS instructions need no m0 on gfx9+), and hipcc itself sets it afresh before
// every LDS-DMA it emits.
__device__ __forceinline__ void lds_dma16(const i32x4_t& rsrc, uint32_t lds_byte, uint32_t voff) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, 0 offen lds" :: "v"(voff), "s"(lds_byte), "s"(rsrc) : "memory");
}
// The same with the destination forced into an SGPR.  Under SGPR pressure hipcc has been seen (conv_halo2.hip) to keep this wave-uniform
// value in a VGPR and hand it to the "s" operand as such.  Use it where that has been observed; every user of the plain form has the
// same exposure, and its generated code is to be read after a change that raises SGPR pressure.
__device__ __forceinline__ void lds_dma16_sgpr(const i32x4_t& rsrc, uint32_t lds_byte, uint32_t voff) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, 0 offen lds" :: "v"(voff), "s"(__builtin_amdgcn_readfirstlane(lds_byte)), "s"(rsrc) : "memory");
}

// Raw buffer descriptor (base, num_records = bytes, 32-bit raw addressing) as the four integers the asm above takes in SGPRs.
// common.h's make_rsrc is the builtin's form of the same descriptor, for the buf_load16 / buf_store16 builtins.
__device__ __forceinline__ i32x4_t raw_rsrc(const void* p, uint32_t bytes) {
    const uint64_t a = (uint64_t)p;
    return i32x4_t{(int)(uint32_t)a, (int)(uint32_t)((a >> 32) & 0xFFFFu), (int)bytes, 0x00020000};
}
// The same through readfirstlane, for a pointer the compiler cannot prove wave-uniform (conv_hwgrad.hip: the paired launch selects its
// argument set per block).
__device__ __forceinline__ i32x4_t raw_rsrc_sgpr(const void* p, uint32_t bytes) {
    const uint64_t a = (uint64_t)p;
    return i32x4_t{__builtin_amdgcn_readfirstlane((int)(uint32_t)a), __builtin_amdgcn_readfirstlane((int)(uint32_t)((a >> 32) & 0xFFFFu)),
                   __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000};
}

// At most N of this wave's vector-memory operations (copies, loads, stores) are still in flight.  N is an immediate of the instruction:
// a kernel whose count is known only at run time branches over the values it can take (conv_pairx.hip wait_vm_uniform).
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }

// Workgroup barrier that orders LDS traffic only, as ONE asm statement, opaque to the compiler: nothing is scheduled between the wait
// and the barrier.  For the kernels that order their LDS-DMA by hand.  common.h's lds_barrier() goes through the barrier builtin, which
// hipcc's own wait-count insertion and scheduler see (it compiles differently); use that one where the compiler sees every load.
__device__ __forceinline__ void lds_barrier_asm() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ds_read_b64_tr_b16 at this lane's address p: lane (c = l & 15, g = l >> 4) receives the four 16-bit elements {row0 + 4 g .. + 3} of
// column c of a row-major tile -- the LDS transposes (conv_wgrad.hip describes the MFMA operand map built from two of them).
__device__ __forceinline__ i32x2_t lds_read_tr16(const char* p) {
    return __builtin_bit_cast(i32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p));
}

// ---------------------------------------------------------------- halo tiles (conv_halo.hip, conv_halo2.hip)
// [rows][128 B] tiles with the XOR swizzle slot = chunk ^ ((row >> 1) & 7): a ds_read_b128 lane group of the 32x32x16 operand layout
// reads ONE chunk of 16 rows out of 32 consecutive ones, which this swizzle spreads over all 16 slots of the 256-byte bank row for ANY
// start row -- the tap shift of a 3x3 filter costs no bank conflicts.
// Byte offset of (row, 16-byte chunk 2*k16 + h) inside such a tile is  halo_rd(row, h) ^ (k16 << 5).
__device__ __forceinline__ uint32_t halo_rd(int row, int h) {
    const int s = (row >> 1) & 7;
    return (uint32_t)(row * 128 + ((s >> 1) << 5) + ((h ^ (s & 1)) << 4));
}
// MFMA row rho of a 32-filter sub-tile <-> filter offset: lane half h then holds filters 8h..8h+7 in accumulators 0..7 and 16+8h.. in 8..15
// (the filter rows are permuted on the DMA source side, so the epilogue stores 16-byte vectors straight from registers)
__device__ __forceinline__ int halo_perm(int rho) {
    const int g = rho >> 3, hh = (rho >> 2) & 1, e = rho & 3;
    return 16 * (g >> 1) + 8 * hh + 4 * (g & 1) + e;
}
