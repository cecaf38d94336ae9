// Device building blocks shared by the MFMA GEMM kernels and encoder_fused.hip: LDS-DMA, counted waits, and the accumulator
// staging of the epilogues.  Main loops and epilogues stay in the kernels' own files: their schedules are deliberately different.
#pragma once
#include "smd_common.h"

typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;

// LDS-DMA of 16 B per lane (global_load_lds_dwordx4): destination = wave-uniform LDS base + lane*16.  Pointer form: per-lane source address.
__device__ __forceinline__ void glds16(const bf16_t* g, unsigned char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((glb_void_t*)g, (lds_void_t*)lds_wave_base, 16, 0, 0);
}
// Buffer form: source = buffer descriptor base + per-lane voffset + wave-uniform soffset (rows past the descriptor's range read as zeros).
__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t rsrc, uint32_t voff, uint32_t soff, unsigned char* lds_wave_base) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)lds_wave_base, 16, voff, soff, 0, 0);
}

#define SMD_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define SMD_LGKMCNT(n) asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory")
#define SMD_PIN() __builtin_amdgcn_sched_barrier(0)
#define SMD_BAR() __builtin_amdgcn_s_barrier()
template <int N_> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory"); }

template <int... Es> struct IntSeq {};
typedef IntSeq<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15> Seq16;
// One 32x32 MFMA accumulator tile into an fp32 LDS stage of LD floats per row.
// 32x32 MFMA C layout: col = lane&31, row = (e&3) + 8*(e>>2) + 4*(lane>>5)
template <int LD, int... Es>
__device__ __forceinline__ void stage_tile(const f32x16_t& acc, float* stage, int row0, int col, IntSeq<Es...>) {
  ((stage[(row0 + (Es & 3) + 8 * (Es >> 2)) * LD + col] = acc[Es]), ...);
}
template <int LD, int... Es>
__device__ __forceinline__ void stage_tile_add(const f32x16_t& acc, float* stage, int row0, int col, IntSeq<Es...>) {
  ((stage[(row0 + (Es & 3) + 8 * (Es >> 2)) * LD + col] += acc[Es]), ...);
}
