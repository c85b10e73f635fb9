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

#include "kernels.h"

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

template <int BN>
__global__ __launch_bounds__(256) void gemm_bf16_tile_kernel(
    unsigned short* __restrict__ C, const unsigned char* __restrict__ A,
    const unsigned char* __restrict__ W, int M, int N, int K) {
  constexpr int NI = BN / 32;              // 16-wide n sub-tiles of a wave
  constexpr int A_B = B16T_BM * B16T_ROW;  // bytes of the A tile of a stage
  constexpr int STAGE_B = A_B + BN * B16T_ROW;
  constexpr int NDMA_A = B16T_BM / 32;     // DMA instructions of a wave
  constexpr int NDMA_W = BN / 32;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * STAGE_B];

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
  const size_t row_b = (size_t)K * 2;      // bytes of an operand row

  // --- DMA of one wave: instruction i covers the 8 tile rows
  // 8 * (NDMA * wave + i) ..; lane l writes LDS chunk position l & 7 of
  // row l >> 3 and fetches source chunk (l & 7) ^ swz(row) for it
  const unsigned char* asrc[NDMA_A];
  const unsigned char* wsrc[NDMA_W];
  int acol[NDMA_A], wcol[NDMA_W];
#pragma unroll
  for (int i = 0; i < NDMA_A; ++i) {
    const int row = 8 * (NDMA_A * wave + i) + (lane >> 3);
    acol[i] = (((lane & 7) ^ (row >> 1)) & 7) * 16;
    asrc[i] = A + (size_t)min(m0 + row, M - 1) * row_b;
  }
#pragma unroll
  for (int i = 0; i < NDMA_W; ++i) {
    const int row = 8 * (NDMA_W * wave + i) + (lane >> 3);
    wcol[i] = (((lane & 7) ^ (row >> 1)) & 7) * 16;
    wsrc[i] = W + (size_t)min(n0 + row, N - 1) * row_b;
  }
  const int nfull = K >> 6;          // 64-k stages
  const bool tail = (K & 32) != 0;   // plus one of 32 k
  const int nstages = nfull + (tail ? 1 : 0);
  // stage s -> buffer `buf`.  A full stage masks its column with 127; the
  // 64-byte tail stage (s == nfull) with 63, which keeps its lanes inside
  // the row's last 64 bytes
  auto issue = [&](int s, int buf) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t k0 = (size_t)s * B16T_ROW;
    const int colmask = s == nfull ? 63 : 127;
    unsigned char* dst = lds + buf * STAGE_B;
#pragma unroll
    for (int i = 0; i < NDMA_A; ++i)
      __builtin_amdgcn_global_load_lds(
          asrc[i] + k0 + (acol[i] & colmask),
          (b16t_lds_ptr)(dst + (NDMA_A * wave + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < NDMA_W; ++i)
      __builtin_amdgcn_global_load_lds(
          wsrc[i] + k0 + (wcol[i] & colmask),
          (b16t_lds_ptr)(dst + A_B + (NDMA_W * wave + i) * 1024), 16, 0, 0);
#else
    (void)s; (void)buf;
#endif
  };

  b16t_f32x4 acc[4][NI];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[j][i] = b16t_f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment rows of this lane: row lq of each 16-row sub-tile, source
  // chunk 4 s + lh in k-step s (sub-tile bases are multiples of 16, so the
  // swizzle of the row is that of lq)
  const int swz = (lq >> 1) & 7;
  const int x[2] = {(lh ^ swz) * 16, ((4 + lh) ^ swz) * 16};
  const int aoff = ((wave >> 1) * 64 + lq) * B16T_ROW;
  const int woff = A_B + ((wave & 1) * (BN / 2) + lq) * B16T_ROW;

  issue(0, 0);
  int buf = 0;  // buffer of stage t
  for (int t = 0; t < nfull; ++t) {
    b16t_wait_dma();
    b16t_barrier();
    if (t + 1 < nstages) issue(t + 1, buf ^ 1);
    if (active)
      b16t_stage<NI, 2>(acc, lds + buf * STAGE_B + aoff,
                        lds + buf * STAGE_B + woff, x);
    buf ^= 1;
  }
  if (tail) {
    b16t_wait_dma();
    b16t_barrier();
    if (active)
      b16t_stage<NI, 1>(acc, lds + buf * STAGE_B + aoff,
                        lds + buf * STAGE_B + woff, x);
  }

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
