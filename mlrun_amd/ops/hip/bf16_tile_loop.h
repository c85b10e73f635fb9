// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// What the bf16 output-tile kernels share: gemm_bf16_tile_kernel
// (gemm_bf16_tile.hip, where the design is described) and
// lm_head_logprobs_kernel (lm_head_logprobs.hip).  The helpers are here;
// the K loop itself is bf16_tile_kloop.inc, program text that both kernel
// bodies include, so that both compute every accumulator in one order.
//
// No fp32 VALU arithmetic happens here, so nothing carries a target
// attribute and everything inlines as plain always_inline code.

#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

typedef __attribute__((ext_vector_type(4))) float b16t_f32x4;
typedef __attribute__((ext_vector_type(8))) short b16t_bf16x8;

#define B16T_DEV __device__ __attribute__((always_inline)) inline

#define B16T_BM 128   // rows of a workgroup tile
#define B16T_ROW 128  // bytes of a row per stage (64 k)

typedef __attribute__((address_space(3))) void* b16t_lds_ptr;

B16T_DEV unsigned short b16t_f2bf(float f) {  // round-to-nearest-even
  union { float f; uint32_t i; } v;
  v.f = f;
  return (unsigned short)((v.i + 0x7fffu + ((v.i >> 16) & 1u)) >> 16);
}

B16T_DEV void b16t_barrier() {  // __syncthreads()
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

B16T_DEV void b16t_wait_dma() {  // every LDS-DMA of this wave has landed
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One stage of a wave: KSTEPS (2, or 1 in the 32-k tail) k-steps, each 16
// bytes of each of its 4 x 16 activation rows and NI x 16 weight rows, then
// 4 x NI MFMAs.  ap / wp point at this lane's row of the first sub-tile;
// x[s] is the byte offset of its (swizzled) chunk of k-step s.
template <int NI, int KSTEPS>
B16T_DEV void b16t_stage(b16t_f32x4 (&acc)[4][NI], const unsigned char* ap,
                         const unsigned char* wp, const int (&x)[2]) {
  b16t_bf16x8 af[KSTEPS][4], wf[KSTEPS][NI];
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      af[s][j] = *reinterpret_cast<const b16t_bf16x8*>(
          ap + j * 16 * B16T_ROW + x[s]);
#pragma unroll
    for (int i = 0; i < NI; ++i)
      wf[s][i] = *reinterpret_cast<const b16t_bf16x8*>(
          wp + i * 16 * B16T_ROW + x[s]);
  }
  // (the host pass cannot type-check the MFMA builtin)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s)  // ascending k: the summation order
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < NI; ++i)
        acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf[s][i], af[s][j], acc[j][i], 0, 0, 0);
#endif
}
