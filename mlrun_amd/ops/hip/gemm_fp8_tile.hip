// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// FP8 (OCP e4m3) PREFILL GEMM for gfx950:
//   C[M, N] bf16 = bf16((A8 . W8^T)[m, n] * a_scale[m] * w_scale[n])
// on the activation codes of quant_fp8_rows and the weight packs of
// quantize_fp8_weight, for any M and N and K % 64 == 0.
//
// Layout.  Both operands carry the same pair-swizzled k order inside
// every 64-k group, and a dot product does not care in which order its
// terms are paired as long as both operands agree.  The kernel therefore
// treats a row as opaque bytes: byte i of an A row always meets byte i of
// a W row, and nothing is unswizzled anywhere.
//
// Decomposition.  Hundreds of rows make this a compute-shaped GEMM, so
// the work is split by OUTPUT TILE, not by K:
//   grid (ceil(N / BN), ceil(M / 128)), 256 threads = 4 waves in a 2 x 2
//   grid; a wave owns 64 rows x BN/2 columns = 4 x BN/32 accumulators.
//   BN = 128 (64 accumulator registers per lane) or 64.  No split-K, no
//   atomics: every C element has one writer and one summation order,
//   whatever the grid.
//
// K loop, 128 bytes (= 128 k) per step, one
// v_mfma_scale_f32_16x16x128_f8f6f4 per accumulator and step with unit
// E8M0 scales (0x7f): a lane supplies 32 contiguous bytes of a row per
// operand, two ds_read_b128.  Sixteen MFMAs of a wave meet sixteen such
// reads (BN = 128): every fragment is used four times.
//
// Operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4), never
// through VGPRs: fp8 needs no conversion on the way.  A wave instruction
// writes 1 KiB lane-linearly = 8 whole 128 B rows; a wave issues
// (128 + BN) / 32 of them per step.  TWO LDS stages: the DMA of step t+1
// is issued right after the single barrier of step t and flies under the
// fragment reads and MFMAs of step t.  Per step:
//   s_waitcnt vmcnt(0)   this wave's share of stage t has landed
//   barrier              ... and everybody else's; all waves are done
//                        reading stage t-1, whose buffer is free now
//   issue DMA(t+1)       into the buffer of stage t-1
//   read fragments of stage t, 16 MFMAs
// 2 x (16 + 16) KiB = 64 KiB at BN = 128, 48 KiB at BN = 64.
//
// LDS layout: row-major, 128 B rows, no padding (padding would not fit
// the 64 KiB and the DMA writes lane-linearly anyway).  The eight 16 B
// chunks of a row are XOR-permuted with swz(row) = (row >> 1) & 7: LDS
// chunk position p of a row holds source chunk p ^ swz(row), applied on
// the SOURCE address of the DMA lane, and the same XOR is applied to the
// read address.  Bank arithmetic: the 64 banks are 256 B = two rows wide.
// The 16 lanes of a ds_read_b128 group read rows r0 .. r0 + 15 (r0 % 16
// == 0) at one source chunk c, i.e. byte (row & 1) * 128 +
// ((c ^ (row >> 1)) & 7) * 16 of the bank row: row & 1 picks the half,
// row >> 1 runs through 0 .. 7 and the XOR maps it one-to-one onto the 8
// chunk positions, so the 16 lanes cover the 16 positions once: no
// conflict.  The DMA writes are lane-linear and conflict-free by
// construction.  (The permutation is per ROW, so it cannot be left to
// the read side alone: the MFMA pairs byte i of A row m with byte i of W
// row n for all m, n, which needs one k order for all rows.)
//
// K % 128 == 64: the last step has 64 bytes per row.  Its DMA lanes keep
// their source chunk inside those 64 bytes (chunk & 3), so nothing past a
// row is read, and the lanes that would supply bytes 64 .. 127 (lane >> 4
// >= 2) feed ZERO fragments for BOTH operands: 0 x 0, so stale LDS bytes
// never meet anything, NaN codes included.
//
// The product runs transposed (MFMA A operand = W rows, B operand =
// activation rows): a lane then holds four CONSECUTIVE n of one output
// row and stores them as one 8 B word when N % 4 == 0.
//
// Epilogue: (acc * a_scale[m]) * w_scale[n], the expression and order of
// skinny_gemm_fp8_kernel, one bf16 rounding (round-to-nearest-even).
//
// Edges: rows >= M and >= N are clamped on load (they repeat the last
// row and stay inside the tensors) and never stored; a wave whose whole
// sub-tile lies outside skips its fragment reads and MFMAs but keeps
// issuing its share of the DMA and meeting the barriers.  Capture-safe:
// no allocation, no sync.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

typedef __attribute__((ext_vector_type(4))) float f32x4v;
typedef __attribute__((ext_vector_type(4))) int i32x4v;
typedef __attribute__((ext_vector_type(8))) int i32x8v;

// Built with the packed f32 VALU forms (v_pk_add / mul / fma_f32) off, as
// gemm_mxfp4_tile_kernel is.  A function inlines only into one with the
// same target features, so every helper carries the attribute too;
// without that they become real calls and the fragments go through
// scratch.  The host pass does not know the feature.
#if defined(__HIP_DEVICE_COMPILE__)
#define F8T_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define F8T_NO_PK_F32
#endif
#define F8T_DEV __device__ F8T_NO_PK_F32 __attribute__((always_inline)) inline

#define F8T_BM 128   // rows of a workgroup tile
#define F8T_ROW 128  // bytes (= k) of a row per step

typedef __attribute__((address_space(3))) void* f8t_lds_ptr;

F8T_DEV unsigned short f8t_f2bf(float f) {  // round-to-nearest-even
  union { float f; uint32_t i; } v;
  v.f = f;
  return (unsigned short)((v.i + 0x7fffu + ((v.i >> 16) & 1u)) >> 16);
}

F8T_DEV void f8t_barrier() {  // __syncthreads() for such a kernel
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

F8T_DEV void f8t_wait_dma() {  // every LDS-DMA of this wave has landed
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One K step of a wave: 32 bytes of each of its 4 x 16 activation rows
// and NI x 16 weight rows from the LDS stage, then 4 x NI MFMAs.  ap / wp
// point at this lane's row of the first sub-tile, x0 / x1 are the byte
// offsets of its two (swizzled) chunks.  TAIL: lanes with `dead` feed
// zeros for both operands.
template <int NI, bool TAIL>
F8T_DEV void f8t_step(f32x4v (&acc)[4][NI], const unsigned char* ap,
                      const unsigned char* wp, int x0, int x1, bool dead) {
  i32x8v af[4], wf[NI];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const i32x4v lo =
        *reinterpret_cast<const i32x4v*>(ap + j * 16 * F8T_ROW + x0);
    const i32x4v hi =
        *reinterpret_cast<const i32x4v*>(ap + j * 16 * F8T_ROW + x1);
    af[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const i32x4v lo =
        *reinterpret_cast<const i32x4v*>(wp + i * 16 * F8T_ROW + x0);
    const i32x4v hi =
        *reinterpret_cast<const i32x4v*>(wp + i * 16 * F8T_ROW + x1);
    wf[i] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
  if (TAIL) {
    const i32x8v zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) af[j] = dead ? zero : af[j];
#pragma unroll
    for (int i = 0; i < NI; ++i) wf[i] = dead ? zero : wf[i];
  }
  // (the host pass cannot type-check the MFMA builtin)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < NI; ++i)
      acc[j][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          wf[i], af[j], acc[j][i], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
#endif
}

template <int BN>
__global__ __launch_bounds__(256) F8T_NO_PK_F32 void gemm_fp8_tile_kernel(
    unsigned short* __restrict__ C, const unsigned char* __restrict__ A8,
    const float* __restrict__ a_scale, const unsigned char* __restrict__ W8,
    const float* __restrict__ w_scale, int M, int N, int K) {
  constexpr int NI = BN / 32;            // 16-wide n sub-tiles of a wave
  constexpr int A_B = F8T_BM * F8T_ROW;  // bytes of the A tile of a stage
  constexpr int STAGE_B = A_B + BN * F8T_ROW;
  constexpr int NDMA_A = F8T_BM / 32;    // DMA instructions of a wave
  constexpr int NDMA_W = BN / 32;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * STAGE_B];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15;
  const int lh = lane >> 4;
  const int m0 = blockIdx.y * F8T_BM;
  const int n0 = blockIdx.x * BN;
  const int wm0 = m0 + (wave >> 1) * 64;  // this wave's sub-tile
  const int wn0 = n0 + (wave & 1) * (BN / 2);
  const bool active = wm0 < M && wn0 < N;  // wave-uniform

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
    asrc[i] = A8 + (size_t)min(m0 + row, M - 1) * K;
  }
#pragma unroll
  for (int i = 0; i < NDMA_W; ++i) {
    const int row = 8 * (NDMA_W * wave + i) + (lane >> 3);
    wcol[i] = (((lane & 7) ^ (row >> 1)) & 7) * 16;
    wsrc[i] = W8 + (size_t)min(n0 + row, N - 1) * K;
  }
  // colmask 127: a full step; 63: the 64-byte tail step, whose lanes stay
  // inside the row's last 64 bytes
  auto issue = [&](int k0, int buf, int colmask) F8T_NO_PK_F32 {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned char* dst = lds + buf * STAGE_B;
#pragma unroll
    for (int i = 0; i < NDMA_A; ++i)
      __builtin_amdgcn_global_load_lds(
          asrc[i] + k0 + (acol[i] & colmask),
          (f8t_lds_ptr)(dst + (NDMA_A * wave + i) * 1024), 16, 0, 0);
#pragma unroll
    for (int i = 0; i < NDMA_W; ++i)
      __builtin_amdgcn_global_load_lds(
          wsrc[i] + k0 + (wcol[i] & colmask),
          (f8t_lds_ptr)(dst + A_B + (NDMA_W * wave + i) * 1024), 16, 0, 0);
#else
    (void)k0; (void)buf; (void)colmask;
#endif
  };

  f32x4v acc[4][NI];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[j][i] = f32x4v{0.f, 0.f, 0.f, 0.f};

  // fragment rows of this lane: row lq of each 16-row sub-tile, source
  // chunks 2 lh and 2 lh + 1 (sub-tile bases are multiples of 16, so the
  // swizzle of the row is that of lq)
  const int swz = (lq >> 1) & 7;
  const int x0 = ((2 * lh) ^ swz) * 16;
  const int x1 = ((2 * lh + 1) ^ swz) * 16;
  const int aoff = ((wave >> 1) * 64 + lq) * F8T_ROW;
  const int woff = A_B + ((wave & 1) * (BN / 2) + lq) * F8T_ROW;

  const int nfull = K >> 7;           // 128-byte steps
  const bool tail = (K & 64) != 0;    // plus one of 64 bytes
  if (nfull > 0) issue(0, 0, 127); else issue(0, 0, 63);
  int buf = 0;
  for (int t = 0; t < nfull; ++t) {
    f8t_wait_dma();
    f8t_barrier();
    const int k1 = (t + 1) << 7;
    if (t + 1 < nfull) issue(k1, buf ^ 1, 127);
    else if (tail) issue(k1, buf ^ 1, 63);
    if (active)
      f8t_step<NI, false>(acc, lds + buf * STAGE_B + aoff,
                          lds + buf * STAGE_B + woff, x0, x1, false);
    buf ^= 1;
  }
  if (tail) {
    f8t_wait_dma();
    f8t_barrier();
    if (active)
      f8t_step<NI, true>(acc, lds + buf * STAGE_B + aoff,
                         lds + buf * STAGE_B + woff, x0, x1, lh >= 2);
  }

  // --- epilogue: acc[j][i][r] = C[wm0 + 16 j + lq][wn0 + 16 i + 4 lh + r]
  if (!active) return;
  const bool wide = (N & 3) == 0;  // then n < N means n + 3 < N, 8 B aligned
  float ws[NI][4];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      ws[i][r] = w_scale[min(wn0 + 16 * i + 4 * lh + r, N - 1)];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = wm0 + 16 * j + lq;
    if (m >= M) continue;
    const float sa = a_scale[m];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = wn0 + 16 * i + 4 * lh;
      if (n >= N) continue;
      unsigned short o[4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        o[r] = f8t_f2bf(acc[j][i][r] * sa * ws[i][r]);
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
// is at most 512 workgroups, two per CU, which is what co-resides of the
// 48 KiB instance: one round of the 256 CUs.  Measured (docs/kernels.md):
// the mxfp4 tile kernel's limit of 256 chose the slower width at 4 of 15
// cells here, 512 the faster at all 15.
void launch_gemm_fp8_tile(void* out_bf16, const void* A8, const void* a_scale,
                          const void* W8, const void* w_scale, int M, int N,
                          int K, int bn, void* stream) {
  const int mtiles = (M + F8T_BM - 1) / F8T_BM;
  if (bn == 0) bn = (long long)mtiles * ((N + 63) / 64) <= 512 ? 64 : 128;
  auto kern = bn == 64 ? gemm_fp8_tile_kernel<64> : gemm_fp8_tile_kernel<128>;
  hipLaunchKernelGGL(kern, dim3((N + bn - 1) / bn, mtiles), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out_bf16,
                     (const unsigned char*)A8, (const float*)a_scale,
                     (const unsigned char*)W8, (const float*)w_scale, M, N, K);
}
