// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// bf16 PREFILL GEMM for gfx950:
//   C[M, N] bf16 = bf16(A[M, K] . W[N, K]^T), fp32 accumulation, one
//   rounding, for any M >= 1 and N >= 1 and K % 32 == 0.
//
// Decomposition.  Split by OUTPUT TILE only, as gemm_fp8_tile_kernel:
//   grid (ceil(N / BN), ceil(M / 128)), 256 threads = 4 waves in a 2 x 2
//   grid; a wave owns 64 rows x BN/2 columns = 4 x BN/32 accumulators of
//   v_mfma_f32_16x16x32_bf16.  BN = 128 (64 accumulator registers per
//   lane) or 64.  No split-K, no atomics.
//
// Summation order (the contract).  Every C element has ONE accumulator,
// which takes the 32-k blocks of its row pair in ascending k, one MFMA
// each, in both tile widths.  The bits of C[m, n] therefore depend on
// A[m, :], W[n, :] and K alone: not on M, N, the position of the row or
// column in its tile, BN, or what else is in the call.
//
// K loop, one stage = 64 k = 128 bytes of a row, two k-steps of 32.  In
// the 16x16x32 MFMA lane (lq, lh) = (lane & 15, lane >> 4) supplies the 8
// consecutive k  8 lh .. 8 lh + 7  of row lq: 16 contiguous bytes, one
// ds_read_b128.  k-step s of a stage reads source chunk 4 s + lh.  Per
// stage and wave at BN = 128: 8 global_load_lds_dwordx4, 16 ds_read_b128,
// 32 MFMAs; every fragment is used four times.
//
// Operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4), never
// through VGPRs.  A wave instruction writes 1 KiB lane-linearly = 8 whole
// 128 B rows; a wave issues (128 + BN) / 32 of them per stage.  TWO LDS
// stages and ONE barrier per stage:
//   s_waitcnt vmcnt(0)   this wave's share of stage t has landed
//   barrier              ... and everybody else's; all waves are done
//                        reading stage t - 1, whose buffer is free now
//   issue DMA(t + 1)     into the buffer of stage t - 1
//   read fragments of stage t, 8 * BN/32 MFMAs
// 2 x (16 + 16) KiB = 64 KiB at BN = 128, 48 KiB at BN = 64: two
// workgroups per CU.  A third stage (96 / 72 KiB, one workgroup per CU at
// BN = 128) was built and measured slower, 16 .. 36 % at BN = 128 and
// M = 2048 (docs/kernels.md), and is not kept.
//
// LDS layout: that of gemm_fp8_tile_kernel, whose bank argument carries
// over unchanged (the row is 128 B and a lane group reads one source chunk
// of 16 consecutive rows there too): row-major, 128 B rows, no padding,
// the eight 16 B chunks of a row XOR-permuted with swz(row) = (row >> 1)
// & 7.  LDS chunk position p of a row holds source chunk p ^ swz(row),
// applied on the SOURCE address of the DMA lane, and again on the read.
// The 16 lanes of a ds_read_b128 group read rows r0 .. r0 + 15 (r0 % 16
// == 0) at one source chunk c, i.e. byte (row & 1) * 128 + ((c ^ (row >>
// 1)) & 7) * 16 of the 256 B bank row: the 16 lanes cover its 16 chunk
// positions once.
//
// K % 64 == 32: the last stage has 64 bytes per row.  Its DMA lanes keep
// their source chunk inside those 64 bytes (chunk & 3), so nothing past a
// row is read; LDS position p then holds source chunk (p ^ swz) & 3, and
// k-step 0 (source chunks 0 .. 3, found at position c ^ swz) reads what it
// should.  k-step 1 is SKIPPED in that stage: the duplicate and stale
// bytes never reach an MFMA.
//
// The product runs transposed (MFMA A operand = W rows, B operand =
// activation rows): a lane then holds four CONSECUTIVE n of one output
// row and stores them as one 8 B word when N % 4 == 0.
//
// Edges: rows >= M and >= N are clamped on load (they repeat the last
// row and stay inside the tensors) and never stored; a wave whose whole
// sub-tile lies outside skips its fragment reads and MFMAs but keeps
// issuing its share of the DMA and meeting the barriers.  Capture-safe:
// no allocation, no sync.
//
// No fp32 VALU arithmetic happens here (the rounding is integer code), so
// the kernel needs no target attribute and its helpers inline as they are.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "bf16_tile_loop.h"  // helpers shared with lm_head_logprobs.hip
#include "kernels.h"

template <int BN>
__global__ __launch_bounds__(256) void gemm_bf16_tile_kernel(
    unsigned short* __restrict__ C, const unsigned char* __restrict__ A,
    const unsigned char* __restrict__ W, int M, int N, int K) {
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15;
  const int lh = lane >> 4;
  const int m0 = blockIdx.y * B16T_BM;
  const int n0 = blockIdx.x * BN;
  const int wm0 = m0 + (wave >> 1) * 64;  // this wave's sub-tile
  const int wn0 = n0 + (wave & 1) * (BN / 2);
  const bool active = wm0 < M && wn0 < N;  // wave-uniform
#include "bf16_tile_kloop.inc"  // the K loop: declares lds and acc

  // --- epilogue: acc[j][i][r] = C[wm0 + 16 j + lq][wn0 + 16 i + 4 lh + r]
  if (!active) return;
  const bool wide = (N & 3) == 0;  // then n < N means n + 3 < N, 8 B aligned
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = wm0 + 16 * j + lq;
    if (m >= M) continue;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = wn0 + 16 * i + 4 * lh;
      if (n >= N) continue;
      unsigned short o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) o[r] = b16t_f2bf(acc[j][i][r]);
      unsigned short* cp = C + (size_t)m * N + n;
      if (wide) {
        ushort4 v;
        v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
        *reinterpret_cast<ushort4*>(cp) = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) cp[r] = o[r];
      }
    }
  }
}

// bn: 128 or 64 forces the tile width; 0 picks 64 while the 64-wide grid
// is at most 512 workgroups, two per CU, one round of the 256 CUs: the
// rule of gemm_fp8_tile_kernel, re-measured here (docs/kernels.md).
void launch_gemm_bf16_tile(void* out_bf16, const void* A, const void* W,
                           int M, int N, int K, int bn, void* stream) {
  const int mtiles = (M + B16T_BM - 1) / B16T_BM;
  if (bn == 0) bn = (long long)mtiles * ((N + 63) / 64) <= 512 ? 64 : 128;
  auto kern =
      bn == 64 ? gemm_bf16_tile_kernel<64> : gemm_bf16_tile_kernel<128>;
  hipLaunchKernelGGL(kern, dim3((N + bn - 1) / bn, mtiles), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out_bf16,
                     (const unsigned char*)A, (const unsigned char*)W, M, N,
                     K);
}
