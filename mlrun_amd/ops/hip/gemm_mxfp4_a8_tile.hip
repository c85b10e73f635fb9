// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// W4A8 PREFILL GEMM for gfx950 on the native block-scaled MFMA:
//   C[m, n] bf16 = bf16(a_scale[m] * sum_blk 2^(e[n, blk] - 127) *
//                       sum_{k in blk} a8[m, k] * fp4(w4[n, k]))
// a8 / a_scale are the e4m3 codes of quant_fp8_rows(swizzle=False), i.e.
// in NATURAL k order; w4 / w_scale a pack of quantize_mxfp4_weight, as it
// is: two e2m1 codes per byte (even k in the low nibble), E8M0 scale bytes
// in the grouped order of _mxfp4_scale_order.  Any M, N >= 1, K % 128 == 0
// (the pack's rule, so there is no partial step).
//
// Nothing is converted: v_mfma_scale_f32_16x16x128_f8f6f4 takes the fp4
// codes as its A operand (cbsz = 4), the fp8 codes as its B operand
// (blgp = 0) and the weight's own E8M0 byte as the A scale.  The two
// formats do NOT share a lane map (measured with one-hot operands, see
// docs/kernels.md).  Lane (lq = lane & 15, g = lane >> 4) supplies
//   fp4: the 32 codes k0 + 32 g .. k0 + 32 g + 31 of weight row lq, 16 B,
//        and ONE scale byte, which applies to exactly those 32 k: one MX
//        block, so the scale operand is the pack's byte for (row lq, block
//        k0 / 32 + g);
//   fp8: two 16-byte halves of activation row lq: dwords 0 .. 3 hold
//        k0 + 16 g .. k0 + 16 g + 15, dwords 4 .. 7 hold
//        k0 + 64 + 16 g .. k0 + 64 + 16 g + 15.
// With activations in natural k order that is a choice of LDS chunks and
// costs nothing.  The activation scale is pinned to 0x7f (2^0), the
// per-row a_scale is applied in the epilogue.
//
// Decomposition: that of gemm_fp8_tile_kernel.  Grid (ceil(N / BN),
// ceil(M / 128)), 256 threads = 2 x 2 waves, a wave owns 64 rows x BN/2
// columns = 4 x BN/32 accumulators; BN = 128 or 64.  No split-K, no
// atomics: one writer and one summation order per output, whatever the
// grid.  The product runs transposed (MFMA A operand = W rows), so a lane
// holds four consecutive n of one output row and stores 8 B when
// N % 4 == 0.
//
// K loop, 128 k per step, one MFMA per accumulator and step.  Fragments:
// the weight's 32 codes are 16 B = one ds_read_b128 into the low four
// dwords of the operand (the fp4 form reads no more), the activation's
// two halves two ds_read_b128 (source chunks g and 4 + g of the row).  Per step and wave at BN = 128: 4 + 8 reads for
// 16 MFMAs.
//
// Operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4), two
// stages, one barrier per step, exactly the fp8 kernel's schedule:
//   s_waitcnt vmcnt(0); barrier; issue DMA(t + 1); reads + MFMAs of t.
// A tile: 128 rows x 128 B, a wave instruction covers 8 rows, 4 per wave.
// W tile: BN rows x 64 B, a wave instruction covers 16 rows, BN/64 per
// wave.  A stage is 16 KiB + BN * 64 B: 2 x 24 KiB at BN = 128, 2 x 20 KiB
// at BN = 64.
//
// LDS layout.  A: the fp8 kernel's, 128 B rows whose eight 16 B chunks are
// XOR-permuted with (row >> 1) & 7 on the DMA source address and on the
// read; its bank argument is in gemm_fp8_tile.hip.  W: 64 B rows whose
// FOUR chunks are permuted with (row >> 2) & 3, again on the source
// address of the DMA lane and on the read.  Bank arithmetic: the 64 banks
// are 256 B = FOUR W rows wide.  The 16 lanes of a ds_read_b128 group read
// rows r0 .. r0 + 15 (r0 % 16 == 0) at one source chunk g, i.e. byte
// (row & 3) * 64 + ((g ^ (row >> 2)) & 3) * 16 of the bank row: row & 3
// picks the quarter, row >> 2 runs through 0 .. 3 and the XOR maps it
// one-to-one onto the four chunk positions, so the 16 lanes cover the 16
// positions of the bank row once: no conflict.  DMA writes are
// lane-linear.
//
// Scales do not go through LDS.  Below K & ~511 the pack stores the 16
// scale bytes of four consecutive steps as [g][step]: ONE dword per
// weight row and lane group serves four steps, and the instruction's
// op_sel (an immediate: byte 0 .. 3 of the scale register) picks the
// step's byte, so the step loop is unrolled by four there.  The K/128 % 4
// steps after the last full group are stored [step][g] and take a byte
// load and op_sel 0.  The scales of the NEXT unit (group or tail step) are
// loaded before the MFMAs of this one.  They are ordinary global loads on
// the same vmcnt as the DMA; the vmcnt(0) in front of every barrier lands
// them, and they are moved into the registers the MFMAs read right after
// that wait, so no wait sits between the DMA issue and the fragment
// reads.
//
// Epilogue: acc * a_scale[m], one bf16 rounding (round-to-nearest-even).
//
// Edges: rows >= M and >= N are clamped on load (operands and scales; they
// repeat the last row and stay inside the tensors) and never stored; a
// wave whose whole sub-tile lies outside skips fragment reads and MFMAs
// but keeps its DMA share and the barriers.  Capture-safe: no allocation,
// no sync.

#include <hip/hip_runtime.h>
#include <cstdint>

#include "kernels.h"

typedef __attribute__((ext_vector_type(4))) float f32x4v;
typedef __attribute__((ext_vector_type(4))) int i32x4v;
typedef __attribute__((ext_vector_type(8))) int i32x8v;

// Packed f32 VALU forms off, as in the sibling tile kernels; every helper
// and lambda carries the attribute, or it does not inline and the
// fragments go through scratch.  The host pass does not know the feature.
#if defined(__HIP_DEVICE_COMPILE__)
#define X4A8_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define X4A8_NO_PK_F32
#endif
#define X4A8_DEV __device__ X4A8_NO_PK_F32 __attribute__((always_inline)) inline

#define X4A8_BM 128    // rows of a workgroup tile
#define X4A8_AROW 128  // bytes of an activation row per step (128 k)
#define X4A8_WROW 64   // bytes of a weight row per step (128 codes)

typedef __attribute__((address_space(3))) void* x4a8_lds_ptr;

X4A8_DEV unsigned short x4a8_f2bf(float f) {  // round-to-nearest-even
  union { float f; uint32_t i; } v;
  v.f = f;
  return (unsigned short)((v.i + 0x7fffu + ((v.i >> 16) & 1u)) >> 16);
}

X4A8_DEV void x4a8_barrier() {  // __syncthreads() for such a kernel
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

// every LDS-DMA and scale load of this wave has landed
X4A8_DEV void x4a8_wait_vm() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One K step of a wave: 32 bytes of each of its 4 x 16 activation rows and
// 32 codes of each of its NI x 16 weight rows from the LDS stage, then
// 4 x NI scaled MFMAs.  ap / wp point at this lane's row of the first
// sub-tile; x0 / x1 are the byte offsets of its two (permuted) activation
// chunks (the operand's low and high half), xw that of its weight chunk.  sc[i] holds the lane's E8M0 byte
// for sub-tile i in byte SEL.
template <int NI, int SEL>
X4A8_DEV void x4a8_step(f32x4v (&acc)[4][NI], const unsigned char* ap,
                        const unsigned char* wp, int x0, int x1, int xw,
                        const int (&sc)[NI]) {
  i32x8v af[4], wf[NI];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const i32x4v lo =
        *reinterpret_cast<const i32x4v*>(ap + j * 16 * X4A8_AROW + x0);
    const i32x4v hi =
        *reinterpret_cast<const i32x4v*>(ap + j * 16 * X4A8_AROW + x1);
    af[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const i32x4v lo =
        *reinterpret_cast<const i32x4v*>(wp + i * 16 * X4A8_WROW + xw);
    // the fp4 form reads the low four dwords only
    wf[i] = __builtin_shufflevector(lo, lo, 0, 1, 2, 3, -1, -1, -1, -1);
  }
  // (the host pass cannot type-check the MFMA builtin)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < NI; ++i)
      acc[j][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          wf[i], af[j], acc[j][i], /*cbsz: A is fp4*/ 4, /*blgp: B is fp8*/ 0,
          SEL, sc[i], 0, 0x7f7f7f7f);
#else
  (void)sc;
#endif
}

template <int BN>
__global__ __launch_bounds__(256) X4A8_NO_PK_F32 void
gemm_mxfp4_a8_tile_kernel(unsigned short* __restrict__ C,
                          const unsigned char* __restrict__ A8,
                          const float* __restrict__ a_scale,
                          const unsigned char* __restrict__ W4,
                          const unsigned char* __restrict__ WS, int M, int N,
                          int K) {
  constexpr int NI = BN / 32;              // 16-wide n sub-tiles of a wave
  constexpr int A_B = X4A8_BM * X4A8_AROW;  // bytes of the A tile of a stage
  constexpr int STAGE_B = A_B + BN * X4A8_WROW;
  constexpr int NDMA_A = X4A8_BM / 32;     // DMA instructions of a wave
  constexpr int NDMA_W = BN / 64;
  __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * STAGE_B];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15;
  const int lh = lane >> 4;
  const int m0 = blockIdx.y * X4A8_BM;
  const int n0 = blockIdx.x * BN;
  const int wm0 = m0 + (wave >> 1) * 64;  // this wave's sub-tile
  const int wn0 = n0 + (wave & 1) * (BN / 2);
  const bool active = wm0 < M && wn0 < N;  // wave-uniform

  // --- DMA of one wave.  A: instruction i covers the 8 tile rows
  // 8 * (NDMA_A * wave + i) ..; lane l writes chunk position l & 7 of row
  // l >> 3 and fetches source chunk (l & 7) ^ ((row >> 1) & 7) for it.
  // W: instruction i covers the 16 tile rows 16 * (NDMA_W * wave + i) ..;
  // lane l writes position l & 3 of row l >> 2 and fetches source chunk
  // (l & 3) ^ ((row >> 2) & 3)
  const unsigned char* asrc[NDMA_A];
  const unsigned char* wsrc[NDMA_W];
#pragma unroll
  for (int i = 0; i < NDMA_A; ++i) {
    const int row = 8 * (NDMA_A * wave + i) + (lane >> 3);
    asrc[i] = A8 + (size_t)min(m0 + row, M - 1) * K +
              (((lane & 7) ^ (row >> 1)) & 7) * 16;
  }
#pragma unroll
  for (int i = 0; i < NDMA_W; ++i) {
    const int row = 16 * (NDMA_W * wave + i) + (lane >> 2);
    wsrc[i] = W4 + (size_t)min(n0 + row, N - 1) * (K >> 1) +
              (((lane & 3) ^ (row >> 2)) & 3) * 16;
  }
  auto issue = [&](int k0, int buf) X4A8_NO_PK_F32 {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned char* dst = lds + buf * STAGE_B;
#pragma unroll
    for (int i = 0; i < NDMA_A; ++i)
      __builtin_amdgcn_global_load_lds(
          asrc[i] + k0, (x4a8_lds_ptr)(dst + (NDMA_A * wave + i) * 1024), 16,
          0, 0);
#pragma unroll
    for (int i = 0; i < NDMA_W; ++i)
      __builtin_amdgcn_global_load_lds(
          wsrc[i] + (k0 >> 1),
          (x4a8_lds_ptr)(dst + A_B + (NDMA_W * wave + i) * 1024), 16, 0, 0);
#else
    (void)k0; (void)buf;
#endif
  };

  // --- scales: a row's K/32 bytes are `ngroups` grouped units of 16
  // ([g][step], one dword per lane group) and `ntail` tail steps of 4
  // ([step][g], one byte per lane group); unit u < ngroups is a group
  const int nsteps = K >> 7;
  const int ngroups = nsteps >> 2;
  const int ntail = nsteps & 3;
  const unsigned char* sp[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
    sp[i] = WS + (size_t)min(wn0 + 16 * i + lq, N - 1) * (K >> 5);
  auto load_scales = [&](int u, int (&dst)[NI]) X4A8_NO_PK_F32 {
    if (u < ngroups) {
#pragma unroll
      for (int i = 0; i < NI; ++i)
        dst[i] = *reinterpret_cast<const int*>(sp[i] + u * 16 + lh * 4);
    } else {
      const int off = ngroups * 16 + (u - ngroups) * 4 + lh;
#pragma unroll
      for (int i = 0; i < NI; ++i) dst[i] = sp[i][off];
    }
  };

  f32x4v acc[4][NI];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[j][i] = f32x4v{0.f, 0.f, 0.f, 0.f};

  // fragment rows of this lane: row lq of each 16-row sub-tile (sub-tile
  // bases are multiples of 16, so the permutation of the row is that of
  // lq); activation source chunks lh and 4 + lh (the fp8 operand's two
  // halves), weight chunk lh
  const int aswz = (lq >> 1) & 7;
  const int x0 = (lh ^ aswz) * 16;
  const int x1 = ((4 + lh) ^ aswz) * 16;
  const int xw = (lh ^ ((lq >> 2) & 3)) * 16;
  const int aoff = ((wave >> 1) * 64 + lq) * X4A8_AROW;
  const int woff = A_B + ((wave & 1) * (BN / 2) + lq) * X4A8_WROW;

  int scur[NI], snext[NI];
  int t = 0, buf = 0;
  // Head of step t: this wave's share of stage t (and any scale load)
  // has landed; at the first step of unit u >= 0 snext becomes the unit's
  // scales and the next unit's are requested, to land at the next wait;
  // the barrier frees stage t - 1, which is refilled with step t + 1
  auto advance = [&](int u) X4A8_NO_PK_F32 {
    x4a8_wait_vm();
    if (u >= 0) {
#pragma unroll
      for (int i = 0; i < NI; ++i) scur[i] = snext[i];
      if (u + 1 < ngroups + ntail) load_scales(u + 1, snext);
    }
    x4a8_barrier();
    if (t + 1 < nsteps) issue((t + 1) << 7, buf ^ 1);
  };
#define X4A8_STEP(SEL)                                                     \
  do {                                                                     \
    if (active)                                                            \
      x4a8_step<NI, SEL>(acc, lds + buf * STAGE_B + aoff,                  \
                         lds + buf * STAGE_B + woff, x0, x1, xw, scur);    \
    buf ^= 1;                                                              \
    ++t;                                                                   \
  } while (0)

  issue(0, 0);
  load_scales(0, snext);
  for (int u = 0; u < ngroups; ++u) {
    advance(u);
    X4A8_STEP(0);
    advance(-1);
    X4A8_STEP(1);
    advance(-1);
    X4A8_STEP(2);
    advance(-1);
    X4A8_STEP(3);
  }
  for (int u = ngroups; u < ngroups + ntail; ++u) {
    advance(u);
    X4A8_STEP(0);
  }
#undef X4A8_STEP

  // --- epilogue: acc[j][i][r] = C[wm0 + 16 j + lq][wn0 + 16 i + 4 lh + r]
  if (!active) return;
  const bool wide = (N & 3) == 0;  // then n < N means n + 3 < N, 8 B aligned
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
      for (int r = 0; r < 4; ++r) o[r] = x4a8_f2bf(acc[j][i][r] * sa);
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

// bn: 128 or 64 forces the tile width; 0 picks by the fp8 tile launcher's
// rule: 64 while the 64-wide grid is at most 512 workgroups
void launch_gemm_mxfp4_a8_tile(void* out_bf16, const void* A8,
                               const void* a_scale, const void* W4,
                               const void* w_scale, int M, int N, int K,
                               int bn, void* stream) {
  const int mtiles = (M + X4A8_BM - 1) / X4A8_BM;
  if (bn == 0) bn = (long long)mtiles * ((N + 63) / 64) <= 512 ? 64 : 128;
  auto kern = bn == 64 ? gemm_mxfp4_a8_tile_kernel<64>
                       : gemm_mxfp4_a8_tile_kernel<128>;
  hipLaunchKernelGGL(kern, dim3((N + bn - 1) / bn, mtiles), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out_bf16,
                     (const unsigned char*)A8, (const float*)a_scale,
                     (const unsigned char*)W4, (const unsigned char*)w_scale,
                     M, N, K);
}
