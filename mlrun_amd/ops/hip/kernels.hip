// Copyright 2026 mlrun_amd authors
//
// Licensed under the Apache License, Version 2.0 (the "License");
// you may not use this file except in compliance with the License.
//
// CDNA4 (gfx950 / MI355X) serving & training kernels.
//
// Design notes (see SURVEY.md §2.3/§2.6 — the reference has
// no GPU kernels; this kernel surface is defined by the north-star
// serving/training configs):
//  - wave = 64 lanes everywhere; all bf16 global loads vectorized as
//    short8/ushort2 (16B / 4B per lane)
//  - decode GEMM (M<=16 activations x [N,K] weights) on MFMA
//    v_mfma_f32_16x16x32_bf16, K-split across workgroups so the grid
//    fills 256 CUs: each split stores its own f32 slab (plain stores)
//    and reduce_cast or the consumer kernel folds them
//  - decode attention: one workgroup per (batch, kv-head), one wave
//    per grouped q-head, online softmax, LDS score buffer
//  - norm/rope/swiglu fused elementwise kernels at HBM rate
// All kernels are hipGraph-capture safe: no allocation, no sync.

#include <hip/hip_fp8.h>
#include <hip/hip_runtime.h>
#include <atomic>
#include <cfloat>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "kernels.h"

typedef __attribute__((ext_vector_type(8))) short short8v;
typedef __attribute__((ext_vector_type(4))) float f32x4v;
typedef __attribute__((ext_vector_type(2))) float f32x2v;

#define DEV __device__ __forceinline__

DEV float bf2f(unsigned short u) {
  union { uint32_t i; float f; } v;
  v.i = uint32_t(u) << 16;
  return v.f;
}

DEV unsigned short f2bf(float f) {
  union { float f; uint32_t i; } v;
  v.f = f;
  uint32_t x = v.i;
  // round-to-nearest-even
  uint32_t r = (x + 0x7fffu + ((x >> 16) & 1u)) >> 16;
  return (unsigned short)r;
}

struct ushort8 { unsigned short v[8]; };
struct ushort2v { unsigned short x, y; };

// ---------------------------------------------------------------------
// fused residual-add + RMSNorm (bf16):
//   residual <- x + residual ; out <- rmsnorm(residual) * weight
// one workgroup per row; vectorized short8 loads (guide G13).
// ---------------------------------------------------------------------
// out8/out_scale (optional): also emit the normalized row quantized
// to fp8 e4m3 in the GEMM's pair-swizzled layout — feeds the
// fp8-weight decode path without a separate quant launch.
__global__ void fused_add_rmsnorm_kernel(
    unsigned short* __restrict__ out, unsigned short* __restrict__ residual,
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ weight, int hidden, float eps,
    int has_residual, unsigned char* __restrict__ out8,
    float* __restrict__ out_scale) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;
  const unsigned short* xr = x + (size_t)row * hidden;
  unsigned short* rr = residual ? residual + (size_t)row * hidden : nullptr;
  unsigned short* outr = out + (size_t)row * hidden;

  float sumsq = 0.f;
  for (int i = tid * 8; i < hidden; i += nthreads * 8) {
    ushort8 xv = *reinterpret_cast<const ushort8*>(xr + i);
    float z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = bf2f(xv.v[j]);
    if (has_residual) {
      ushort8 rv = *reinterpret_cast<const ushort8*>(rr + i);
      ushort8 zv;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        z[j] += bf2f(rv.v[j]);
        zv.v[j] = f2bf(z[j]);
      }
      *reinterpret_cast<ushort8*>(rr + i) = zv;  // updated residual
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) sumsq += z[j] * z[j];
  }
  // block reduce
  __shared__ float red[32];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    sumsq += __shfl_down(sumsq, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = sumsq;
  __syncthreads();
  if (tid < (nthreads >> 6)) sumsq = red[tid];
  else sumsq = 0.f;
  if (tid < 64) {
#pragma unroll
    for (int off = 2; off > 0; off >>= 1)
      sumsq += __shfl_down(sumsq, off, 64);
  }
  if (tid == 0) red[0] = sumsq;
  __syncthreads();
  const float inv = rsqrtf(red[0] / hidden + eps);

  const unsigned short* zsrc = has_residual ? rr : xr;
  float amax = 0.f;
  for (int i = tid * 8; i < hidden; i += nthreads * 8) {
    ushort8 zv = *reinterpret_cast<const ushort8*>(zsrc + i);
    ushort8 wv = *reinterpret_cast<const ushort8*>(weight + i);
    ushort8 ov;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float value = bf2f(zv.v[j]) * inv * bf2f(wv.v[j]);
      ov.v[j] = f2bf(value);
      amax = fmaxf(amax, fabsf(value));
    }
    *reinterpret_cast<ushort8*>(outr + i) = ov;
  }
  if (out8 == nullptr) return;
  // fp8 sidecar: block-reduce amax, then re-emit the row quantized
  // into the gemm's pair-swizzled layout (row data is L1/L2 hot)
  __syncthreads();  // red[] still feeds inv on slower threads
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = amax;
  __syncthreads();
  float gmax = 0.f;
  for (int w = 0; w < (nthreads >> 6); ++w) gmax = fmaxf(gmax, red[w]);
  const float qscale = gmax > 0.f ? gmax / 448.f : 1.f;
  const float qinv = 1.f / qscale;
  if (tid == 0) out_scale[row] = qscale;
  unsigned char* out8r = out8 + (size_t)row * hidden;
  for (int i = tid * 8; i < hidden; i += nthreads * 8) {
    ushort8 ov = *reinterpret_cast<const ushort8*>(outr + i);
    unsigned char q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      __hip_fp8_e4m3 f8(bf2f(ov.v[j]) * qinv);
      q[j] = f8.__x;
    }
    const int sblk = i >> 5;
    const int c = (i >> 3) & 3;
    const int dst = ((sblk >> 1) << 6) + (c << 4) + ((sblk & 1) << 3);
    *reinterpret_cast<uint64_t*>(out8r + dst) =
        *reinterpret_cast<const uint64_t*>(q);
  }
}

void launch_fused_add_rmsnorm(void* out, void* residual, const void* x,
                              const void* weight, int rows, int hidden,
                              float eps, void* out8, void* out_scale,
                              void* stream) {
  int threads = hidden >= 2048 ? 256 : 64;
  hipLaunchKernelGGL(fused_add_rmsnorm_kernel, dim3(rows), dim3(threads), 0,
                     (hipStream_t)stream, (unsigned short*)out,
                     (unsigned short*)residual, (const unsigned short*)x,
                     (const unsigned short*)weight, hidden, eps,
                     residual != nullptr ? 1 : 0, (unsigned char*)out8,
                     (float*)out_scale);
}

// ---------------------------------------------------------------------
// RoPE (neox / llama style, rotate-half):
//   for i < D/2: (q_i, q_{i+D/2}) <- (q_i c - q_{i+D/2} s,
//                                     q_{i+D/2} c + q_i s)
// cos_sin: [max_pos, D/2, 2] f32 precomputed host-side (guide B:
// on-device trig turns memory-bound into VALU-bound).
// q: [T, heads, D]; positions: [T].
// ---------------------------------------------------------------------
__global__ void rope_kernel(unsigned short* __restrict__ q,
                            const int* __restrict__ positions,
                            const float* __restrict__ cos_sin, int heads,
                            int dim, long long row_stride) {
  const int t = blockIdx.x;
  const int h = blockIdx.y;
  const int i = threadIdx.x;  // 0..D/2-1
  const int half = dim >> 1;
  if (i >= half) return;
  const int pos = positions[t];
  const float c = cos_sin[((size_t)pos * half + i) * 2];
  const float s = cos_sin[((size_t)pos * half + i) * 2 + 1];
  unsigned short* base = q + (size_t)t * row_stride + (size_t)h * dim;
  float a = bf2f(base[i]);
  float b = bf2f(base[i + half]);
  base[i] = f2bf(a * c - b * s);
  base[i + half] = f2bf(b * c + a * s);
}

void launch_rope(void* q, const void* positions, const void* cos_sin, int T,
                 int heads, int dim, long long row_stride, void* stream) {
  hipLaunchKernelGGL(rope_kernel, dim3(T, heads), dim3(dim / 2), 0,
                     (hipStream_t)stream, (unsigned short*)q,
                     (const int*)positions, (const float*)cos_sin, heads, dim,
                     row_stride);
}

// ---------------------------------------------------------------------
// SwiGLU: out = silu(gate) * up   (bf16, flat, vectorized)
// gate/up are halves of one [rows, 2*inter] tensor or separate ptrs.
// ---------------------------------------------------------------------
__global__ void silu_mul_kernel(unsigned short* __restrict__ out,
                                const unsigned short* __restrict__ gate,
                                const unsigned short* __restrict__ up,
                                long long n) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  long long stride = (long long)gridDim.x * blockDim.x * 8;
  for (; i < n; i += stride) {
    ushort8 g = *reinterpret_cast<const ushort8*>(gate + i);
    ushort8 u = *reinterpret_cast<const ushort8*>(up + i);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gf = bf2f(g.v[j]);
      float s = gf / (1.f + __expf(-gf));
      o.v[j] = f2bf(s * bf2f(u.v[j]));
    }
    *reinterpret_cast<ushort8*>(out + i) = o;
  }
}

// SwiGLU over a fused gate|up buffer: gu [rows, 2*inter] ->
// out [rows, inter] = silu(gu[:, :inter]) * gu[:, inter:]
__global__ void swiglu_fused_kernel(unsigned short* __restrict__ out,
                                    const unsigned short* __restrict__ gu,
                                    int rows, int inter) {
  const long long total = (long long)rows * inter / 8;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const long long flat = i * 8;
    const int r = (int)(flat / inter);
    const int c = (int)(flat % inter);
    const unsigned short* row = gu + (size_t)r * 2 * inter;
    ushort8 g = *reinterpret_cast<const ushort8*>(row + c);
    ushort8 u = *reinterpret_cast<const ushort8*>(row + inter + c);
    ushort8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float gf = bf2f(g.v[j]);
      float s = gf / (1.f + __expf(-gf));
      o.v[j] = f2bf(s * bf2f(u.v[j]));
    }
    *reinterpret_cast<ushort8*>(out + (size_t)r * inter + c) = o;
  }
}

void launch_swiglu_fused(void* out, const void* gu, int rows, int inter,
                         void* stream) {
  long long blocks = ((long long)rows * inter / 8 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(swiglu_fused_kernel, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out,
                     (const unsigned short*)gu, rows, inter);
}

void launch_silu_mul(void* out, const void* gate, const void* up,
                     long long n, void* stream) {
  long long blocks = (n / 8 + 255) / 256;
  if (blocks > 2048) blocks = 2048;  // grid-stride (guide G11)
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(silu_mul_kernel, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out,
                     (const unsigned short*)gate, (const unsigned short*)up,
                     n);
}

// ---------------------------------------------------------------------
// Skinny GEMM (decode projections):  C[M,N] (+)= A[M,K] @ W[N,K]^T
// M <= 16 (decode batch), bf16 inputs, f32 C.
// MFMA 16x16x32: each wave owns a 32-wide n-tile (2 B-fragments),
// 4 waves/block -> 128 n per block; K split across gridDim.y, one f32
// slab per split (SPLIT below).
// Fragment layout (verified on HW by tests/gpu):
//   A: lane l holds A[l&15][(l>>4)*8 + j]   j=0..7
//   B: lane l holds W[n0 + (l&15)][(l>>4)*8 + j] (B^T = W row-major)
//   C: lane l, reg r -> C[(l>>4)*4 + r][l&15]
// ---------------------------------------------------------------------
// SPLIT=false: ksplit==1, epilogue writes bf16 straight to `out`.
// SPLIT=true:  blockIdx.y writes its f32 partial slab part[y][M][N]
//              (plain stores — no atomics, no pre-zero, deterministic);
//              reduce_cast_kernel folds the slabs to bf16.
template <bool SPLIT, int MT>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(
    void* __restrict__ out, const unsigned short* __restrict__ A,
    const unsigned short* __restrict__ W, int M, int N, int K, int ksplit) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 128 + wave * 32;  // this wave's n-tile
  if (n0 >= N) return;
  int kbegin = 0, kend = K;
  if (SPLIT) {
    const int kchunk = (K / ksplit + 31) & ~31;  // multiple of 32
    kbegin = blockIdx.y * kchunk;
    kend = kbegin + kchunk;
    if (kend > K) kend = K;
  }

  // K-loop notes (measured via .s dumps):
  //  - any branch or pragma-driven unroll in the loop kept it ROLLED
  //    with a vmcnt(0) drain per iteration -> latency-serialized;
  //    the manual unrolled block issues all its loads before the
  //    first MFMA waits, so a wave keeps ~384B in flight
  //  - out-of-range rows are CLAMPED, not masked: their products land
  //    only in C cells (m>=M / n>=N) the epilogue never writes
  //  - MT in {1,2} A-row tiles: M<=16 or 17..32 (decode batch 32
  //    doubles served requests per weight pass at equal HBM traffic)
  const int arow = lane & 15;
  const int kb = (lane >> 4) * 8;
  const int brow0 = n0 + (lane & 15);
  const int brow1 = brow0 + 16;

  f32x4v acc0[MT], acc1[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc0[t] = {0.f, 0.f, 0.f, 0.f};
    acc1[t] = {0.f, 0.f, 0.f, 0.f};
  }

  const unsigned short* aptr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
    aptr[t] = A + (size_t)min(arow + 16 * t, M - 1) * K + kb;
  const unsigned short* bptr0 =
      W + (size_t)min(brow0, N - 1) * K + kb;
  const unsigned short* bptr1 =
      W + (size_t)min(brow1, N - 1) * K + kb;

#ifndef MLRUN_GEMM_UNR1
#define MLRUN_GEMM_UNR1 16
#endif
  constexpr int UNR = (MT == 1) ? MLRUN_GEMM_UNR1 : (MT == 2 ? 4 : 2);
  int k = kbegin;
  const int kend8 = kbegin + ((kend - kbegin) & ~(UNR * 32 - 1));
  for (; k < kend8; k += UNR * 32) {
    short8v af[UNR][MT], bf0[UNR], bf1[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        af[u][t] =
            *reinterpret_cast<const short8v*>(aptr[t] + k + u * 32);
      bf0[u] = *reinterpret_cast<const short8v*>(bptr0 + k + u * 32);
      bf1[u] = *reinterpret_cast<const short8v*>(bptr1 + k + u * 32);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[u][t], bf0[u], acc0[t], 0, 0, 0);
        acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[u][t], bf1[u], acc1[t], 0, 0, 0);
      }
    }
  }
  for (; k < kend; k += 32) {
    short8v bf0 = *reinterpret_cast<const short8v*>(bptr0 + k);
    short8v bf1 = *reinterpret_cast<const short8v*>(bptr1 + k);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      short8v af = *reinterpret_cast<const short8v*>(aptr[t] + k);
      acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf0, acc0[t],
                                                        0, 0, 0);
      acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf1, acc1[t],
                                                        0, 0, 0);
    }
  }

  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
  const bool b0_valid = brow0 < N;
  const bool b1_valid = brow1 < N;
  if (SPLIT) {
    float* part = (float*)out + (size_t)blockIdx.y * M * N;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * t + crow_base + r;
        if (m >= M) continue;
        if (b0_valid) part[(size_t)m * N + n0 + ccol] = acc0[t][r];
        if (b1_valid) part[(size_t)m * N + n0 + 16 + ccol] = acc1[t][r];
      }
  } else {
    unsigned short* dst = (unsigned short*)out;
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = 16 * t + crow_base + r;
        if (m >= M) continue;
        if (b0_valid) dst[(size_t)m * N + n0 + ccol] = f2bf(acc0[t][r]);
        if (b1_valid)
          dst[(size_t)m * N + n0 + 16 + ccol] = f2bf(acc1[t][r]);
      }
  }
}

// Wave-split-K variant: the 4 waves of a workgroup cooperate on ONE
// 32-wide n-tile, each covering K/4 of the k-chunk, combining through
// LDS.  4x the workgroup count of skinny_gemm_kernel at the same
// split-K slab traffic -> 4x the waves/SIMD for latency hiding
// (profile: N=4096 projections were latency-bound at 2 waves/SIMD).
template <bool SPLIT, int MT, int UNR2 = 4, int NB = 2>
__global__ __launch_bounds__(256) void skinny_gemm_ws_kernel(
    void* __restrict__ out, const unsigned short* __restrict__ A,
    const unsigned short* __restrict__ W, int M, int N, int K, int ksplit) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int NT = 16 * NB;      // n-tile width (16 or 32)
  const int n0 = blockIdx.x * NT;
  if (n0 >= N) return;
  int cbegin = 0, cend = K;
  if (SPLIT) {
    const int kchunk = (K / ksplit + 31) & ~31;
    cbegin = blockIdx.y * kchunk;
    cend = cbegin + kchunk;
    if (cend > K) cend = K;
  }
  // each wave covers a quarter of [cbegin, cend)
  const int clen = cend - cbegin;
  const int per_wave = ((clen / 4) + 31) & ~31;
  int kbegin = cbegin + wave * per_wave;
  int kend = kbegin + per_wave;
  if (kend > cend) kend = cend;

  // K-loop notes (measured via .s dumps):
  //  - any branch or pragma-driven unroll in the loop kept it ROLLED
  //    with a vmcnt(0) drain per iteration -> latency-serialized;
  //    the manual unrolled block issues all its loads before the
  //    first MFMA waits, so a wave keeps ~384B in flight
  //  - out-of-range rows are CLAMPED, not masked: their products land
  //    only in C cells (m>=M / n>=N) the epilogue never writes
  //  - MT in {1,2} A-row tiles: M<=16 or 17..32 (decode batch 32
  //    doubles served requests per weight pass at equal HBM traffic)
  //  - NB=1 halves the n-tile to 16: double the workgroup count at
  //    UNCHANGED per-wave K length (grid-starved shapes like qkv) at
  //    the cost of re-reading A once more (L2-resident, tiny)
  const int arow = lane & 15;
  const int kb = (lane >> 4) * 8;
  const int brow0 = n0 + (lane & 15);
  const int brow1 = brow0 + 16;

  f32x4v acc0[MT], acc1[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc0[t] = {0.f, 0.f, 0.f, 0.f};
    acc1[t] = {0.f, 0.f, 0.f, 0.f};
  }

  const unsigned short* aptr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
    aptr[t] = A + (size_t)min(arow + 16 * t, M - 1) * K + kb;
  const unsigned short* bptr0 =
      W + (size_t)min(brow0, N - 1) * K + kb;
  const unsigned short* bptr1 =
      W + (size_t)min(NB == 2 ? brow1 : brow0, N - 1) * K + kb;

#ifndef MLRUN_GEMM_UNR1
#define MLRUN_GEMM_UNR1 16
#endif
  constexpr int UNR = (MT == 1) ? MLRUN_GEMM_UNR1
                                : (MT == 2 ? (NB == 1 ? 8 : UNR2) : 2);
  int k = kbegin;
  const int kend8 = kbegin + ((kend - kbegin) & ~(UNR * 32 - 1));
  for (; k < kend8; k += UNR * 32) {
    short8v af[UNR][MT], bf0[UNR], bf1[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        af[u][t] =
            *reinterpret_cast<const short8v*>(aptr[t] + k + u * 32);
      bf0[u] = *reinterpret_cast<const short8v*>(bptr0 + k + u * 32);
      if (NB == 2)
        bf1[u] = *reinterpret_cast<const short8v*>(bptr1 + k + u * 32);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[u][t], bf0[u], acc0[t], 0, 0, 0);
        if (NB == 2)
          acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              af[u][t], bf1[u], acc1[t], 0, 0, 0);
      }
    }
  }
  for (; k < kend; k += 32) {
    short8v bf0 = *reinterpret_cast<const short8v*>(bptr0 + k);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      short8v af = *reinterpret_cast<const short8v*>(aptr[t] + k);
      acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf0, acc0[t],
                                                        0, 0, 0);
      if (NB == 2) {
        short8v bf1 = *reinterpret_cast<const short8v*>(bptr1 + k);
        acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf1,
                                                          acc1[t], 0, 0,
                                                          0);
      }
    }
  }

  // combine the 4 waves' partials through LDS
  __shared__ float comb[4][16 * MT][NT];  // [wave][m][n] 4-16 KiB
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      comb[wave][16 * t + crow_base + r][ccol] = acc0[t][r];
      if (NB == 2)
        comb[wave][16 * t + crow_base + r][ccol + 16] = acc1[t][r];
    }
  __syncthreads();
  if (wave == 0) {
    // 64 lanes fold 16*MT x NT cells: lane covers 4*MT*NB cells
    constexpr int CPL = 4 * MT * NB;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int cell = lane * CPL + c;
      const int m = cell / NT;
      const int n = cell % NT;
      if (m >= M || n0 + n >= N) continue;
      float sum = comb[0][m][n] + comb[1][m][n] + comb[2][m][n] +
                  comb[3][m][n];
      if (SPLIT) {
        float* part = (float*)out + (size_t)blockIdx.y * M * N;
        part[(size_t)m * N + n0 + n] = sum;
      } else {
        ((unsigned short*)out)[(size_t)m * N + n0 + n] = f2bf(sum);
      }
    }
  }
}

// Software-pipelined wave-split variant (round-2 design doc §1, built
// in C++ instead of inline asm): a DEPTH-stage rotating register ring
// of one 32-K step each (MT A-vecs + NB B-rows).  The fully-unrolled
// ring gives LLVM's waitcnt pass compile-time register stages, so it
// emits PARTIAL vmcnt waits (retire the oldest stage while
// (MT+NB)*(DEPTH-1) newer loads stay in flight) — steady-state loads
// in flight instead of the base kernel's issue-burst-then-drain
// blocks.  Staging VGPRs = DEPTH * (MT+NB) * 4; DEPTH<=4 stays under
// the round-1 occupancy backfire threshold (64 staging VGPRs).
template <bool SPLIT, int MT, int DEPTH, int NB = 2>
__global__ __launch_bounds__(256) void skinny_gemm_ws_pipe_kernel(
    void* __restrict__ out, const unsigned short* __restrict__ A,
    const unsigned short* __restrict__ W, int M, int N, int K, int ksplit) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  constexpr int NT = 16 * NB;
  const int n0 = blockIdx.x * NT;
  if (n0 >= N) return;
  int cbegin = 0, cend = K;
  if (SPLIT) {
    const int kchunk = (K / ksplit + 31) & ~31;
    cbegin = blockIdx.y * kchunk;
    cend = cbegin + kchunk;
    if (cend > K) cend = K;
  }
  const int clen = cend - cbegin;
  const int per_wave = ((clen / 4) + 31) & ~31;
  int kbegin = cbegin + wave * per_wave;
  int kend = kbegin + per_wave;
  if (kend > cend) kend = cend;

  const int arow = lane & 15;
  const int kb = (lane >> 4) * 8;
  const int brow0 = n0 + (lane & 15);
  const int brow1 = brow0 + 16;

  f32x4v acc0[MT], acc1[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc0[t] = {0.f, 0.f, 0.f, 0.f};
    acc1[t] = {0.f, 0.f, 0.f, 0.f};
  }
  const unsigned short* aptr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
    aptr[t] = A + (size_t)min(arow + 16 * t, M - 1) * K + kb;
  const unsigned short* bptr0 =
      W + (size_t)min(brow0, N - 1) * K + kb;
  const unsigned short* bptr1 =
      W + (size_t)min(NB == 2 ? brow1 : brow0, N - 1) * K + kb;

  short8v a_ring[DEPTH][MT], b0_ring[DEPTH], b1_ring[DEPTH];
  const int nsteps_total = (kend - kbegin) / 32;
  // main region: a multiple of DEPTH steps; the rest runs in the tail
  const int ngroups = nsteps_total / DEPTH;
  const int nsteps = ngroups > 0 ? ngroups * DEPTH : 0;
  int kload = kbegin;
  int k = kbegin + nsteps * 32;
  if (nsteps) {
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        a_ring[s][t] =
            *reinterpret_cast<const short8v*>(aptr[t] + kload);
      b0_ring[s] = *reinterpret_cast<const short8v*>(bptr0 + kload);
      if (NB == 2)
        b1_ring[s] = *reinterpret_cast<const short8v*>(bptr1 + kload);
      kload += 32;
    }
    for (int g = DEPTH; g < nsteps; g += DEPTH) {
#pragma unroll
      for (int s = 0; s < DEPTH; ++s) {
#pragma unroll
        for (int t = 0; t < MT; ++t) {
          acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_ring[s][t], b0_ring[s], acc0[t], 0, 0, 0);
          if (NB == 2)
            acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a_ring[s][t], b1_ring[s], acc1[t], 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < MT; ++t)
          a_ring[s][t] =
              *reinterpret_cast<const short8v*>(aptr[t] + kload);
        b0_ring[s] = *reinterpret_cast<const short8v*>(bptr0 + kload);
        if (NB == 2)
          b1_ring[s] = *reinterpret_cast<const short8v*>(bptr1 + kload);
        kload += 32;
      }
    }
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a_ring[s][t], b0_ring[s], acc0[t], 0, 0, 0);
        if (NB == 2)
          acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_ring[s][t], b1_ring[s], acc1[t], 0, 0, 0);
      }
    }
  }
  for (; k < kend; k += 32) {
    short8v bf0 = *reinterpret_cast<const short8v*>(bptr0 + k);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      short8v af = *reinterpret_cast<const short8v*>(aptr[t] + k);
      acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf0, acc0[t],
                                                        0, 0, 0);
      if (NB == 2) {
        short8v bf1 = *reinterpret_cast<const short8v*>(bptr1 + k);
        acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf1,
                                                          acc1[t], 0, 0,
                                                          0);
      }
    }
  }

  __shared__ float comb[4][16 * MT][NT];
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      comb[wave][16 * t + crow_base + r][ccol] = acc0[t][r];
      if (NB == 2)
        comb[wave][16 * t + crow_base + r][ccol + 16] = acc1[t][r];
    }
  __syncthreads();
  if (wave == 0) {
    constexpr int CPL = 4 * MT * NB;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int cell = lane * CPL + c;
      const int m = cell / NT;
      const int n = cell % NT;
      if (m >= M || n0 + n >= N) continue;
      float sum = comb[0][m][n] + comb[1][m][n] + comb[2][m][n] +
                  comb[3][m][n];
      if (SPLIT) {
        float* part = (float*)out + (size_t)blockIdx.y * M * N;
        part[(size_t)m * N + n0 + n] = sum;
      } else {
        ((unsigned short*)out)[(size_t)m * N + n0 + n] = f2bf(sum);
      }
    }
  }
}

// LDS-DMA ring variant of skinny_gemm_ws_pipe_kernel<SPLIT, 2, *, 2>
// (docs/kernels.md "LDS-DMA operand rings"): same decomposition, same
// per-wave [kbegin, kend), same 32-k step order and MFMA operand map,
// so its results are bit-identical; only the way the operands reach
// the MFMA differs.  Every wave owns DEPTH private LDS slots; a slot
// holds one stage = STAGE_K columns of the wave's 32 weight rows and
// of the 32 A rows.  Both are filled by global_load_lds_dwordx4 (W
// with nt, A cached), so bytes in flight cost LDS instead of VGPRs and
// one wave-instruction fetches whole STAGE_K*2-byte row segments
// (>= one 128-B line per row).  No other wave touches a wave's slots:
// the K-loop has no workgroup barrier, only hand-counted vmcnt waits.
//
// LDS image of one operand tile: row-major [32][STAGE_K] bf16; one DMA
// instruction writes 1 KiB lane-linearly = 1024/(2*STAGE_K) whole
// rows.  The 16-B chunks of a row are XOR-permuted on the SOURCE
// address (inside the row's contiguous segment) and the same XOR is
// applied to the read address, which makes the ds_read_b128 fragment
// reads (16 rows x one chunk per 16-lane group) conflict-free.
template <int STAGE_K>
DEV int lds_ring_swz(int row) {
  // 128-B rows: two rows share a 256-B bank row -> 8 chunk positions
  // per row, keyed by row>>1; 256-B rows: 16 positions keyed by row
  return STAGE_K == 64 ? ((row >> 1) & 7) : (row & 15);
}

template <int N>
DEV void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

typedef __attribute__((address_space(3))) void* lds_void_ptr;

template <bool SPLIT, int STAGE_K, int DEPTH>
__global__ __launch_bounds__(256) void skinny_gemm_ws_lds_kernel(
    void* __restrict__ out, const unsigned short* __restrict__ A,
    const unsigned short* __restrict__ W, int M, int N, int K, int ksplit) {
  constexpr int MT = 2, NT = 32;
  constexpr int ROW_B = STAGE_K * 2;       // bytes of one row per stage
  constexpr int OP_B = 32 * ROW_B;         // one operand tile
  constexpr int SLOT_B = 2 * OP_B;         // W tile then A tile
  constexpr int WAVE_B = DEPTH * SLOT_B;   // a wave's private ring
  constexpr int LPR = ROW_B / 16;          // lanes (chunks) per row
  constexpr int RPI = 64 / LPR;            // rows per DMA instruction
  constexpr int NDMA_OP = 32 / RPI;        // DMA instructions per tile
  constexpr int NDMA = 2 * NDMA_OP;        // ... per stage
  constexpr int SPS = STAGE_K / 32;        // 32-k steps per stage
  static_assert(WAVE_B >= 4 * 16 * MT * NT, "comb aliases the ring");
  extern __shared__ __attribute__((aligned(1024))) unsigned char lds_ring[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n0 = blockIdx.x * NT;
  if (n0 >= N) return;
  int cbegin = 0, cend = K;
  if (SPLIT) {
    const int kchunk = (K / ksplit + 31) & ~31;
    cbegin = blockIdx.y * kchunk;
    cend = cbegin + kchunk;
    if (cend > K) cend = K;
  }
  const int clen = cend - cbegin;
  const int per_wave = ((clen / 4) + 31) & ~31;
  int kbegin = cbegin + wave * per_wave;
  int kend = kbegin + per_wave;
  if (kend > cend) kend = cend;
  // whole stages go through the ring; an empty or short range runs none
  const int nst = kend > kbegin ? (kend - kbegin) / STAGE_K : 0;

  f32x4v acc0[MT], acc1[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc0[t] = {0.f, 0.f, 0.f, 0.f};
    acc1[t] = {0.f, 0.f, 0.f, 0.f};
  }

  // DMA source: instruction i, lane l -> tile row i*RPI + l/LPR, LDS
  // chunk position l%LPR, which receives source chunk pos ^ swz(row).
  // Rows past N-1 / M-1 are clamped, chunks stay inside the stage.
  const unsigned short* wsrc[NDMA_OP];
  const unsigned short* asrc[NDMA_OP];
#pragma unroll
  for (int i = 0; i < NDMA_OP; ++i) {
    const int row = i * RPI + lane / LPR;
    const int chunk = (lane % LPR) ^ lds_ring_swz<STAGE_K>(row);
    wsrc[i] = W + (size_t)min(n0 + row, N - 1) * K + kbegin + chunk * 8;
    asrc[i] = A + (size_t)min(row, M - 1) * K + kbegin + chunk * 8;
  }
  // fragment read: lane l holds row l&15, source chunk (l>>4) + 4*step
  unsigned char* const ring = lds_ring + wave * WAVE_B;
  int rd_off[SPS];
#pragma unroll
  for (int s = 0; s < SPS; ++s) {
    const int row = lane & 15;
    rd_off[s] = row * ROW_B +
                ((((lane >> 4) + 4 * s) ^ lds_ring_swz<STAGE_K>(row)) << 4);
  }

  auto issue = [&](int stage, int slot) {
    unsigned char* dst = ring + slot * SLOT_B;
    const int koff = stage * STAGE_K;
    // (the host pass cannot type-check the DMA builtin)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int i = 0; i < NDMA_OP; ++i)
      __builtin_amdgcn_global_load_lds(wsrc[i] + koff,
                                       (lds_void_ptr)(dst + i * 1024), 16,
                                       0, 2);  // nt: read once per step
#pragma unroll
    for (int i = 0; i < NDMA_OP; ++i)
      __builtin_amdgcn_global_load_lds(asrc[i] + koff,
                                       (lds_void_ptr)(dst + OP_B + i * 1024),
                                       16, 0, 0);
#else
    (void)dst;
    (void)koff;
#endif
  };
  // consume slot `slot`; refill it with stage `refill` (< 0: none) once
  // its fragments sit in registers
  auto consume = [&](int slot, int refill) {
    const unsigned char* src = ring + slot * SLOT_B;
    short8v bf0[SPS], bf1[SPS], af[SPS][MT];
#pragma unroll
    for (int s = 0; s < SPS; ++s) {
      bf0[s] = *reinterpret_cast<const short8v*>(src + rd_off[s]);
      bf1[s] =
          *reinterpret_cast<const short8v*>(src + rd_off[s] + 16 * ROW_B);
#pragma unroll
      for (int t = 0; t < MT; ++t)
        af[s][t] = *reinterpret_cast<const short8v*>(
            src + OP_B + rd_off[s] + 16 * t * ROW_B);
    }
    // the reads must have returned before a DMA may overwrite the slot
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (refill >= 0) issue(refill, slot);
#pragma unroll
    for (int s = 0; s < SPS; ++s)
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[s][t], bf0[s], acc0[t], 0, 0, 0);
        acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af[s][t], bf1[s], acc1[t], 0, 0, 0);
      }
  };

#pragma unroll
  for (int s = 0; s < DEPTH; ++s)
    if (s < nst) issue(s, s);
  int j = 0, slot = 0;
  // steady state: DEPTH-1 younger stages stay in flight behind stage j
  for (; j + DEPTH < nst; ++j) {
    wait_vmcnt<NDMA*(DEPTH - 1)>();
    consume(slot, j + DEPTH);
    slot = slot + 1 == DEPTH ? 0 : slot + 1;
  }
  // drain: nst - j <= DEPTH stages are left and all of them are issued
  static_assert(DEPTH == 2 || DEPTH == 3, "drain is written for 2 and 3");
  if (DEPTH == 3 && nst - j == 3) {
    wait_vmcnt<2 * NDMA>();
    consume(slot, -1);
    slot = slot + 1 == DEPTH ? 0 : slot + 1;
    ++j;
  }
  if (nst - j == 2) {
    wait_vmcnt<NDMA>();
    consume(slot, -1);
    slot = slot + 1 == DEPTH ? 0 : slot + 1;
    ++j;
  }
  if (nst - j == 1) {
    wait_vmcnt<0>();
    consume(slot, -1);
  }

  // the rest of the range (< STAGE_K, a multiple of 32) as plain 32-k
  // steps; no DMA is pending here, so ordinary loads wait normally
  if (kend > kbegin) {
    const int arow = lane & 15;
    const int kb = (lane >> 4) * 8;
    const unsigned short* aptr0 = A + (size_t)min(arow, M - 1) * K + kb;
    const unsigned short* aptr1 =
        A + (size_t)min(arow + 16, M - 1) * K + kb;
    const unsigned short* bptr0 =
        W + (size_t)min(n0 + arow, N - 1) * K + kb;
    const unsigned short* bptr1 =
        W + (size_t)min(n0 + arow + 16, N - 1) * K + kb;
    for (int k = kbegin + nst * STAGE_K; k < kend; k += 32) {
      short8v bf0 = *reinterpret_cast<const short8v*>(bptr0 + k);
      short8v bf1 = *reinterpret_cast<const short8v*>(bptr1 + k);
      short8v af0 = *reinterpret_cast<const short8v*>(aptr0 + k);
      short8v af1 = *reinterpret_cast<const short8v*>(aptr1 + k);
      acc0[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af0, bf0, acc0[0],
                                                        0, 0, 0);
      acc1[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af0, bf1, acc1[0],
                                                        0, 0, 0);
      acc0[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af1, bf0, acc0[1],
                                                        0, 0, 0);
      acc1[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af1, bf1, acc1[1],
                                                        0, 0, 0);
    }
  }

  // fold through LDS: a wave's partial goes to the head of its OWN
  // drained ring, so no barrier is needed before these writes
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  typedef float comb_t[16 * MT][NT];
  comb_t& mine = *reinterpret_cast<comb_t*>(ring);
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      mine[16 * t + crow_base + r][ccol] = acc0[t][r];
      mine[16 * t + crow_base + r][ccol + 16] = acc1[t][r];
    }
  __syncthreads();
  if (wave == 0) {
    const comb_t& c0 = *reinterpret_cast<const comb_t*>(lds_ring);
    const comb_t& c1 = *reinterpret_cast<const comb_t*>(lds_ring + WAVE_B);
    const comb_t& c2 =
        *reinterpret_cast<const comb_t*>(lds_ring + 2 * WAVE_B);
    const comb_t& c3 =
        *reinterpret_cast<const comb_t*>(lds_ring + 3 * WAVE_B);
    constexpr int CPL = 4 * MT * 2;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int cell = lane * CPL + c;
      const int m = cell / NT;
      const int n = cell % NT;
      if (m >= M || n0 + n >= N) continue;
      float sum = c0[m][n] + c1[m][n] + c2[m][n] + c3[m][n];
      if (SPLIT) {
        float* part = (float*)out + (size_t)blockIdx.y * M * N;
        part[(size_t)m * N + n0 + n] = sum;
      } else {
        ((unsigned short*)out)[(size_t)m * N + n0 + n] = f2bf(sum);
      }
    }
  }
}

// fold ksplit partial slabs [ksplit, M, N] f32 -> bf16 [M, N]
__global__ void reduce_cast_kernel(unsigned short* __restrict__ out,
                                   const float* __restrict__ part,
                                   long long mn, int ksplit) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (; i + 3 < mn; i += stride) {
    f32x4v sum = *reinterpret_cast<const f32x4v*>(part + i);
    for (int s = 1; s < ksplit; ++s) {
      f32x4v v = *reinterpret_cast<const f32x4v*>(part + (size_t)s * mn + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) sum[j] += v[j];
    }
    unsigned short o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = f2bf(sum[j]);
    *reinterpret_cast<uint64_t*>(out + i) =
        *reinterpret_cast<const uint64_t*>(o);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (long long t = (mn & ~3LL); t < mn; ++t) {
      float sum = part[t];
      for (int s = 1; s < ksplit; ++s) sum += part[(size_t)s * mn + t];
      out[t] = f2bf(sum);
    }
  }
}

// the split-K fold of the bf16 and the fp8 GEMM
static void launch_reduce_cast(void* out_bf16, const void* part_f32, int M,
                               int N, int ksplit, void* stream) {
  long long mn = (long long)M * N;
  long long blocks = (mn / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(reduce_cast_kernel, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out_bf16,
                     (const float*)part_f32, mn, ksplit);
}

// ---------------------------------------------------------------------
// FP8 (OCP e4m3) decode GEMM — the opt-in fp8-weight serving mode.
// Decode is weight-read bound, so fp8 weights halve the dominant
// traffic; activations quantize per-row (dynamic) to fp8, MFMA runs
// native v_mfma_f32_16x16x32_fp8_fp8 (same rate as bf16 — we're after
// the BYTES, not the FLOPs), and the f32 accumulator is rescaled by
// a_scale[m] * w_scale[n] in the epilogue.  Wave-split-K structure
// mirrors skinny_gemm_ws_kernel.
// ---------------------------------------------------------------------
template <bool SPLIT, int MT>
__global__ __launch_bounds__(256) void skinny_gemm_fp8_kernel(
    void* __restrict__ out, const unsigned char* __restrict__ A8,
    const float* __restrict__ a_scale,
    const unsigned char* __restrict__ W8,
    const float* __restrict__ w_scale, int M, int N, int K, int ksplit) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 32;
  if (n0 >= N) return;
  int cbegin = 0, cend = K;
  if (SPLIT) {
    const int kchunk = (K / ksplit + 63) & ~63;
    cbegin = blockIdx.y * kchunk;
    cend = cbegin + kchunk;
    if (cend > K) cend = K;
  }
  const int clen = cend - cbegin;
  const int per_wave = ((clen / 4) + 63) & ~63;  // k-pair aligned
  int kbegin = cbegin + wave * per_wave;
  int kend = kbegin + per_wave;
  if (kend > cend) kend = cend;

  // PAIR-SWIZZLED layout: A8/W8 are stored so each lane's 16B load
  // carries its fragments for TWO consecutive K-steps
  // (new[(s/2)*64 + c*16 + (s%2)*8 + j] = orig[s*32 + c*8 + j]).
  // fp8 at the plain layout measured EQUAL to bf16 time: halving
  // bytes/load doesn't help a latency-bound loop — halving the LOAD
  // COUNT does.  K must be a multiple of 64.
  const int arow = lane & 15;
  const int kb2 = (lane >> 4) * 16;  // 16B per lane per k-PAIR
  const int brow0 = n0 + (lane & 15);
  const int brow1 = brow0 + 16;

  f32x4v acc0[MT], acc1[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    acc0[t] = {0.f, 0.f, 0.f, 0.f};
    acc1[t] = {0.f, 0.f, 0.f, 0.f};
  }
  typedef __attribute__((ext_vector_type(2))) long long2v;
  const unsigned char* aptr[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)
    aptr[t] = A8 + (size_t)min(arow + 16 * t, M - 1) * K + kb2;
  const unsigned char* bptr0 = W8 + (size_t)min(brow0, N - 1) * K + kb2;
  const unsigned char* bptr1 = W8 + (size_t)min(brow1, N - 1) * K + kb2;

  constexpr int UNR = (MT == 1) ? 8 : (MT == 2 ? 4 : 2);  // k-pairs
  int k = kbegin;
  const int kend8 = kbegin + ((kend - kbegin) & ~(UNR * 64 - 1));
  for (; k < kend8; k += UNR * 64) {
    long2v af[UNR][MT], bf0[UNR], bf1[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int t = 0; t < MT; ++t)
        af[u][t] =
            *reinterpret_cast<const long2v*>(aptr[t] + k + u * 64);
      bf0[u] = *reinterpret_cast<const long2v*>(bptr0 + k + u * 64);
      bf1[u] = *reinterpret_cast<const long2v*>(bptr1 + k + u * 64);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
            af[u][t][0], bf0[u][0], acc0[t], 0, 0, 0);
        acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
            af[u][t][0], bf1[u][0], acc1[t], 0, 0, 0);
        acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
            af[u][t][1], bf0[u][1], acc0[t], 0, 0, 0);
        acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
            af[u][t][1], bf1[u][1], acc1[t], 0, 0, 0);
      }
    }
  }
  for (; k < kend; k += 64) {
    long2v bf0 = *reinterpret_cast<const long2v*>(bptr0 + k);
    long2v bf1 = *reinterpret_cast<const long2v*>(bptr1 + k);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      long2v af = *reinterpret_cast<const long2v*>(aptr[t] + k);
      acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
          af[0], bf0[0], acc0[t], 0, 0, 0);
      acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
          af[0], bf1[0], acc1[t], 0, 0, 0);
      acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
          af[1], bf0[1], acc0[t], 0, 0, 0);
      acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(
          af[1], bf1[1], acc1[t], 0, 0, 0);
    }
  }

  __shared__ float comb[4][16 * MT][32];
  const int crow_base = (lane >> 4) * 4;
  const int ccol = lane & 15;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      comb[wave][16 * t + crow_base + r][ccol] = acc0[t][r];
      comb[wave][16 * t + crow_base + r][ccol + 16] = acc1[t][r];
    }
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int c = 0; c < 8 * MT; ++c) {
      const int cell = lane * 8 * MT + c;
      const int m = cell >> 5;
      const int n = cell & 31;
      if (m >= M || n0 + n >= N) continue;
      float sum = (comb[0][m][n] + comb[1][m][n] + comb[2][m][n] +
                   comb[3][m][n]) * a_scale[m] * w_scale[n0 + n];
      if (SPLIT) {
        float* part = (float*)out + (size_t)blockIdx.y * M * N;
        part[(size_t)m * N + n0 + n] = sum;
      } else {
        ((unsigned short*)out)[(size_t)m * N + n0 + n] = f2bf(sum);
      }
    }
  }
}

// one launch of the M class's kernel: out is bf16 [M, N], or f32 slabs
// when SPLIT
template <bool SPLIT>
static void dispatch_skinny_gemm_fp8(void* out, const void* A8,
                                     const void* a_scale, const void* W8,
                                     const void* w_scale, int M, int N,
                                     int K, int ksplit, void* stream) {
  auto kern = M > 32   ? skinny_gemm_fp8_kernel<SPLIT, 4>
              : M > 16 ? skinny_gemm_fp8_kernel<SPLIT, 2>
                       : skinny_gemm_fp8_kernel<SPLIT, 1>;
  const dim3 grid((N + 31) / 32, ksplit > 1 ? ksplit : 1);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, out,
                     (const unsigned char*)A8, (const float*)a_scale,
                     (const unsigned char*)W8, (const float*)w_scale, M, N,
                     K, ksplit);
}

void launch_skinny_gemm_fp8(void* out_bf16, void* part_f32, const void* A8,
                            const void* a_scale, const void* W8,
                            const void* w_scale, int M, int N, int K,
                            int ksplit, void* stream) {
  if (ksplit <= 1) {
    dispatch_skinny_gemm_fp8<false>(out_bf16, A8, a_scale, W8, w_scale, M, N,
                                    K, ksplit, stream);
  } else {
    dispatch_skinny_gemm_fp8<true>(part_f32, A8, a_scale, W8, w_scale, M, N,
                                   K, ksplit, stream);
    launch_reduce_cast(out_bf16, part_f32, M, N, ksplit, stream);
  }
}

// dynamic per-row fp8 quantization of bf16 activations:
// a8[r][k] = round(a[r][k] / (amax_r / 448)); a_scale[r] = amax_r / 448
__global__ void quant_fp8_rows_kernel(unsigned char* __restrict__ a8,
                                      float* __restrict__ a_scale,
                                      const unsigned short* __restrict__ a,
                                      int cols) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const unsigned short* ar = a + (size_t)row * cols;
  unsigned char* outr = a8 + (size_t)row * cols;
  float amax = 0.f;
  for (int i = tid * 8; i < cols; i += blockDim.x * 8) {
    ushort8 v = *reinterpret_cast<const ushort8*>(ar + i);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(bf2f(v.v[j])));
  }
  __shared__ float red[32];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = amax;
  __syncthreads();
  float gmax = 0.f;
  for (int w = 0; w < (blockDim.x >> 6); ++w) gmax = fmaxf(gmax, red[w]);
  const float scale = gmax > 0.f ? gmax / 448.f : 1.f;
  const float inv = 1.f / scale;
  if (tid == 0) a_scale[row] = scale;
  for (int i = tid * 8; i < cols; i += blockDim.x * 8) {
    ushort8 v = *reinterpret_cast<const ushort8*>(ar + i);
    unsigned char q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float scaled = bf2f(v.v[j]) * inv;
      __hip_fp8_e4m3 f8(scaled);
      q[j] = f8.__x;
    }
    // pair-swizzled destination (matches skinny_gemm_fp8_kernel):
    // orig chunk i = s*32 + c*8 -> (s/2)*64 + c*16 + (s%2)*8
    const int s = i >> 5;
    const int c = (i >> 3) & 3;
    const int dst = ((s >> 1) << 6) + (c << 4) + ((s & 1) << 3);
    *reinterpret_cast<uint64_t*>(outr + dst) =
        *reinterpret_cast<const uint64_t*>(q);
  }
}

void launch_quant_fp8_rows(void* a8, void* a_scale, const void* a, int rows,
                           int cols, void* stream) {
  int threads = cols >= 2048 ? 256 : 64;
  hipLaunchKernelGGL(quant_fp8_rows_kernel, dim3(rows), dim3(threads), 0,
                     (hipStream_t)stream, (unsigned char*)a8,
                     (float*)a_scale, (const unsigned short*)a, cols);
}

// MT=2 wave-split K-loop unroll depth (4 default; 8 doubles the
// in-flight bytes per wave at +64 VGPRs) — env knob for e2e A/B.
static int gemm_unr2_env() {
  static int v = [] {
    const char* e = getenv("MLRUN_GEMM_UNR2");
    return e ? atoi(e) : 4;
  }();
  return v;
}

// MLRUN_GEMM_PIPE=0|3|4|6 selects the software-pipelined ring kernel
// (ring depth) for the M in (16,32] decode shapes.  Default 4:
// measured +1.1% e2e over the burst-unrolled kernel at B=32
// (gpurun_out/pipe_ab.log — the per-wave outstanding-bytes wall caps
// the gain, as docs/round2_kernel_designs.md §1 predicted); numerics
// verified vs fp32 on all decode shapes (scripts/check_gemm_pipe.py).
static int gemm_pipe_env() {
  static int v = [] {
    const char* e = getenv("MLRUN_GEMM_PIPE");
    return e ? atoi(e) : 4;
  }();
  return v;
}

// MLRUN_GEMM_LDS_RING=64x2|64x3|128x2 selects the (STAGE_K, DEPTH) ring
// of the variant-4 LDS-DMA kernel: 64, 96 or 128 KiB of LDS per
// workgroup.  Read once.  Default 64x2: two workgroups fit a CU, and it
// won the end-to-end A/B (profiles/README.md, "LDS-DMA operand rings").
static int gemm_lds_ring_env() {
  static int v = [] {
    const char* e = getenv("MLRUN_GEMM_LDS_RING");
    if (e && !strcmp(e, "64x3")) return 1;
    if (e && !strcmp(e, "128x2")) return 2;
    return 0;  // 64x2
  }();
  return v;
}

// every bf16 skinny GEMM kernel: (out, A, W, M, N, K, ksplit)
typedef void (*skinny_gemm_kern_t)(void*, const unsigned short*,
                                   const unsigned short*, int, int, int,
                                   int);

template <int STAGE_K, int DEPTH>
constexpr int lds_ring_bytes() {
  return 4 * DEPTH * 2 * 32 * STAGE_K * 2;
}

// The rings need more dynamic LDS than the 64 KiB a kernel gets by
// default.  The first variant-4 call on a device raises the limit of
// all six instantiations under a lock, so engine replicas that start
// on several threads at once never change a kernel's attributes while
// another thread launches it.  This is not a stream operation; the
// first call is expected outside graph capture (engines warm up
// eagerly before they capture).
static void lds_ring_allow_all() {
  static std::mutex mu;
  static std::atomic<bool> done[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
  if (done[dev].load(std::memory_order_acquire)) return;
  std::lock_guard<std::mutex> lock(mu);
  if (done[dev].load(std::memory_order_relaxed)) return;
  const struct { skinny_gemm_kern_t kern; int bytes; } all[] = {
      {skinny_gemm_ws_lds_kernel<false, 64, 2>, lds_ring_bytes<64, 2>()},
      {skinny_gemm_ws_lds_kernel<true, 64, 2>, lds_ring_bytes<64, 2>()},
      {skinny_gemm_ws_lds_kernel<false, 64, 3>, lds_ring_bytes<64, 3>()},
      {skinny_gemm_ws_lds_kernel<true, 64, 3>, lds_ring_bytes<64, 3>()},
      {skinny_gemm_ws_lds_kernel<false, 128, 2>, lds_ring_bytes<128, 2>()},
      {skinny_gemm_ws_lds_kernel<true, 128, 2>, lds_ring_bytes<128, 2>()},
  };
  for (const auto& k : all)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k.kern),
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              k.bytes);
  done[dev].store(true, std::memory_order_release);
}

// The one dispatch of the bf16 skinny GEMM: pick the kernel of this
// (variant, M class, env knobs) cell and launch it once on the grid
// (n-tiles, ksplit).  out is bf16 [M, N], or ksplit f32 slabs when SPLIT.
template <bool SPLIT>
static void dispatch_skinny_gemm(void* out, const void* A, const void* W,
                                 int M, int N, int K, int ksplit,
                                 int variant, void* stream) {
  const int nblocks = variant == 3 ? (N + 15) / 16
                      : variant >= 1 ? (N + 31) / 32 : (N + 127) / 128;
  const int mt = M > 32 ? 4 : M > 16 ? 2 : 1;  // 16-row M tiles per wave
  skinny_gemm_kern_t kern;
  int lds_bytes = 0;
  if (variant == 4 && mt == 2) {
    lds_ring_allow_all();
    switch (gemm_lds_ring_env()) {
      case 1:
        kern = skinny_gemm_ws_lds_kernel<SPLIT, 64, 3>;
        lds_bytes = lds_ring_bytes<64, 3>();
        break;
      case 2:
        kern = skinny_gemm_ws_lds_kernel<SPLIT, 128, 2>;
        lds_bytes = lds_ring_bytes<128, 2>();
        break;
      default:
        kern = skinny_gemm_ws_lds_kernel<SPLIT, 64, 2>;
        lds_bytes = lds_ring_bytes<64, 2>();
    }
  } else if (variant == 3) {
    // 16-wide n-tiles: 2x the workgroups at unchanged per-wave K
    kern = mt == 4   ? skinny_gemm_ws_kernel<SPLIT, 4, 4, 1>
           : mt == 2 ? skinny_gemm_ws_kernel<SPLIT, 2, 4, 1>
                     : skinny_gemm_ws_kernel<SPLIT, 1, 4, 1>;
  } else if (variant >= 1) {
    const int depth = gemm_pipe_env();
    if (mt == 4)
      kern = skinny_gemm_ws_kernel<SPLIT, 4>;
    else if (mt == 1)
      kern = skinny_gemm_ws_kernel<SPLIT, 1>;
    else if (depth >= 2)  // the software-pipelined ring
      kern = depth >= 6   ? skinny_gemm_ws_pipe_kernel<SPLIT, 2, 6>
             : depth >= 4 ? skinny_gemm_ws_pipe_kernel<SPLIT, 2, 4>
                          : skinny_gemm_ws_pipe_kernel<SPLIT, 2, 3>;
    else
      kern = gemm_unr2_env() >= 8 ? skinny_gemm_ws_kernel<SPLIT, 2, 8>
                                  : skinny_gemm_ws_kernel<SPLIT, 2, 4>;
  } else {
    kern = mt == 4   ? skinny_gemm_kernel<SPLIT, 4>
           : mt == 2 ? skinny_gemm_kernel<SPLIT, 2>
                     : skinny_gemm_kernel<SPLIT, 1>;
  }
  hipLaunchKernelGGL(kern, dim3(nblocks, ksplit), dim3(256), lds_bytes,
                     (hipStream_t)stream, out, (const unsigned short*)A,
                     (const unsigned short*)W, M, N, K, ksplit);
}

// emit split-K slabs only (a consumer kernel folds them)
void launch_skinny_gemm_slabs(void* part_f32, const void* A, const void* W,
                              int M, int N, int K, int ksplit, int variant,
                              void* stream) {
  dispatch_skinny_gemm<true>(part_f32, A, W, M, N, K, ksplit, variant,
                             stream);
}

void launch_skinny_gemm(void* out_bf16, void* part_f32, const void* A,
                        const void* W, int M, int N, int K, int ksplit,
                        int variant, void* stream) {
  if (ksplit <= 1) {
    dispatch_skinny_gemm<false>(out_bf16, A, W, M, N, K, 1, variant, stream);
  } else {
    dispatch_skinny_gemm<true>(part_f32, A, W, M, N, K, ksplit, variant,
                               stream);
    launch_reduce_cast(out_bf16, part_f32, M, N, ksplit, stream);
  }
}

// f32 -> bf16 flat cast (epilogue after k-split accumulate)
__global__ void cast_f32_bf16_kernel(unsigned short* __restrict__ out,
                                     const float* __restrict__ in,
                                     long long n) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (; i + 3 < n; i += stride) {
    f32x4v v = *reinterpret_cast<const f32x4v*>(in + i);
    unsigned short o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = f2bf(v[j]);
    *reinterpret_cast<uint64_t*>(out + i) =
        *reinterpret_cast<const uint64_t*>(o);
  }
  // tail
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (long long t = (n & ~3LL); t < n; ++t) out[t] = f2bf(in[t]);
  }
}

void launch_cast_f32_bf16(void* out, const void* in, long long n,
                          void* stream) {
  long long blocks = (n / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out,
                     (const float*)in, n);
}

// zero f32 buffer (before atomic k-split accumulate)
__global__ void zero_f32_kernel(float* __restrict__ p, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = 0.f;
}

void launch_zero_f32(void* p, long long n, void* stream) {
  long long blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(zero_f32_kernel, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, (float*)p, n);
}

// ---------------------------------------------------------------------
// Slab-consumer fusions: when a decode GEMM runs split-K, its f32
// partial slabs are folded INSIDE the consuming kernel instead of a
// separate reduce_cast pass — one less launch and one less bf16
// round-trip per projection (profile: reduce_cast was ~8% of decode).
// slabs layout: [ksplit, rows, cols] f32.
// ---------------------------------------------------------------------

DEV float slab_sum(const float* __restrict__ slabs, size_t idx,
                   size_t slab_stride, int ksplit) {
  float sum = slabs[idx];
  for (int s = 1; s < ksplit; ++s) sum += slabs[idx + s * slab_stride];
  return sum;
}

// residual <- sum(slabs) + residual; out <- rmsnorm(residual) * weight
__global__ void fused_add_rmsnorm_slab_kernel(
    unsigned short* __restrict__ out, unsigned short* __restrict__ residual,
    const float* __restrict__ slabs,
    const unsigned short* __restrict__ weight, int hidden, float eps,
    int ksplit) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const int nthreads = blockDim.x;
  const size_t rowbase = (size_t)row * hidden;
  const size_t slab_stride = (size_t)gridDim.x * hidden;
  unsigned short* rr = residual + rowbase;
  unsigned short* outr = out + rowbase;

  float sumsq = 0.f;
  for (int i = tid * 4; i < hidden; i += nthreads * 4) {
    float z[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      z[j] = slab_sum(slabs, rowbase + i + j, slab_stride, ksplit);
    unsigned short rv[4];
    *reinterpret_cast<uint64_t*>(rv) =
        *reinterpret_cast<const uint64_t*>(rr + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      z[j] += bf2f(rv[j]);
      rv[j] = f2bf(z[j]);
      sumsq += z[j] * z[j];
    }
    *reinterpret_cast<uint64_t*>(rr + i) =
        *reinterpret_cast<const uint64_t*>(rv);
  }
  __shared__ float red[32];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    sumsq += __shfl_down(sumsq, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = sumsq;
  __syncthreads();
  if (tid < (nthreads >> 6)) sumsq = red[tid];
  else sumsq = 0.f;
  if (tid < 64) {
#pragma unroll
    for (int off = 2; off > 0; off >>= 1)
      sumsq += __shfl_down(sumsq, off, 64);
  }
  if (tid == 0) red[0] = sumsq;
  __syncthreads();
  const float inv = rsqrtf(red[0] / hidden + eps);
  for (int i = tid * 8; i < hidden; i += nthreads * 8) {
    ushort8 zv = *reinterpret_cast<const ushort8*>(rr + i);
    ushort8 wv = *reinterpret_cast<const ushort8*>(weight + i);
    ushort8 ov;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      ov.v[j] = f2bf(bf2f(zv.v[j]) * inv * bf2f(wv.v[j]));
    *reinterpret_cast<ushort8*>(outr + i) = ov;
  }
}

void launch_fused_add_rmsnorm_slab(void* out, void* residual,
                                   const void* slabs, const void* weight,
                                   int rows, int hidden, float eps,
                                   int ksplit, void* stream) {
  int threads = hidden >= 2048 ? 256 : 64;
  hipLaunchKernelGGL(fused_add_rmsnorm_slab_kernel, dim3(rows),
                     dim3(threads), 0, (hipStream_t)stream,
                     (unsigned short*)out, (unsigned short*)residual,
                     (const float*)slabs, (const unsigned short*)weight,
                     hidden, eps, ksplit);
}

// out[r, c] = silu(sum gate_slab) * sum(up_slab); slabs [ks, rows, 2I]
__global__ void swiglu_slab_kernel(unsigned short* __restrict__ out,
                                   const float* __restrict__ slabs,
                                   int rows, int inter, int ksplit) {
  const size_t slab_stride = (size_t)rows * 2 * inter;
  const long long total = (long long)rows * inter / 4;
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const long long flat = i * 4;
    const int r = (int)(flat / inter);
    const int c = (int)(flat % inter);
    const size_t base = (size_t)r * 2 * inter + c;
    unsigned short o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float g = slab_sum(slabs, base + j, slab_stride, ksplit);
      const float u = slab_sum(slabs, base + inter + j, slab_stride,
                               ksplit);
      const float s = g / (1.f + __expf(-g));
      o[j] = f2bf(s * u);
    }
    *reinterpret_cast<uint64_t*>(out + (size_t)r * inter + c) =
        *reinterpret_cast<const uint64_t*>(o);
  }
}

void launch_swiglu_slab(void* out, const void* slabs, int rows, int inter,
                        int ksplit, void* stream) {
  long long blocks = ((long long)rows * inter / 4 + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(swiglu_slab_kernel, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out,
                     (const float*)slabs, rows, inter, ksplit);
}

// qkv slab -> rope(q,k) + KV append + q written to the bf16 qkv buffer
// slabs [ks, B, qkv_row]; qkv_row = (Hq + 2*Hkv) * D
__global__ void rope_kv_slab_kernel(
    unsigned short* __restrict__ qkv, unsigned short* __restrict__ Kc,
    unsigned short* __restrict__ Vc, const float* __restrict__ slabs,
    const int* __restrict__ positions, const float* __restrict__ cos_sin,
    int Hq, int Hkv, int Smax, int D, int qkv_row, int ksplit) {
  const int b = blockIdx.x;
  const int y = blockIdx.y;
  const int i = threadIdx.x;  // 0..D/2-1
  const int half = D >> 1;
  const int pos = positions[b];
  const size_t slab_stride = (size_t)gridDim.x * qkv_row;
  const size_t base = (size_t)b * qkv_row + (size_t)y * D;
  const float lo_f = slab_sum(slabs, base + i, slab_stride, ksplit);
  const float hi_f = slab_sum(slabs, base + i + half, slab_stride, ksplit);
  if (y < Hq + Hkv) {
    const float c = cos_sin[((size_t)pos * half + i) * 2];
    const float s = cos_sin[((size_t)pos * half + i) * 2 + 1];
    const unsigned short lo = f2bf(lo_f * c - hi_f * s);
    const unsigned short hi = f2bf(hi_f * c + lo_f * s);
    if (y < Hq) {  // q: written back for the attention kernel
      unsigned short* qrow = qkv + (size_t)b * qkv_row + (size_t)y * D;
      qrow[i] = lo;
      qrow[i + half] = hi;
    } else {       // k: straight into the cache
      const int kvh = y - Hq;
      unsigned short* dst =
          Kc + (((size_t)b * Hkv + kvh) * Smax + pos) * D;
      dst[i] = lo;
      dst[i + half] = hi;
    }
  } else {         // v: cache only
    const int kvh = y - Hq - Hkv;
    unsigned short* dst = Vc + (((size_t)b * Hkv + kvh) * Smax + pos) * D;
    dst[i] = f2bf(lo_f);
    dst[i + half] = f2bf(hi_f);
  }
}

void launch_rope_kv_slab(void* qkv, void* Kc, void* Vc, const void* slabs,
                         const void* positions, const void* cos_sin, int B,
                         int Hq, int Hkv, int Smax, int D, int qkv_row,
                         int ksplit, void* stream) {
  hipLaunchKernelGGL(rope_kv_slab_kernel, dim3(B, Hq + 2 * Hkv),
                     dim3(D / 2), 0, (hipStream_t)stream,
                     (unsigned short*)qkv, (unsigned short*)Kc,
                     (unsigned short*)Vc, (const float*)slabs,
                     (const int*)positions, (const float*)cos_sin, Hq, Hkv,
                     Smax, D, qkv_row, ksplit);
}

// ---------------------------------------------------------------------
// Fused decode RoPE + KV-cache append: one launch per layer replaces
// {rope(q), rope(k), kv_append}.  qkv is the fused projection buffer
// [B, row_stride] with q at offset 0, k at Hq*D, v at (Hq+Hkv)*D.
// grid: (B, Hq + 2*Hkv); block: D/2 threads.
//  y < Hq:          rope q head in place
//  Hq <= y < +Hkv:  rope k head in place, then copy into Kc[pos]
//  else:            copy v head into Vc[pos]
// ---------------------------------------------------------------------
__global__ void rope_kv_fused_kernel(
    unsigned short* __restrict__ qkv, unsigned short* __restrict__ Kc,
    unsigned short* __restrict__ Vc, const int* __restrict__ positions,
    const float* __restrict__ cos_sin, int Hq, int Hkv, int Smax, int D,
    long long row_stride) {
  const int b = blockIdx.x;
  const int y = blockIdx.y;
  const int i = threadIdx.x;  // 0..D/2-1
  const int half = D >> 1;
  const int pos = positions[b];
  unsigned short* row = qkv + (size_t)b * row_stride;
  if (y < Hq + Hkv) {
    // rope a q or k head
    unsigned short* head = row + (size_t)y * D;
    const float c = cos_sin[((size_t)pos * half + i) * 2];
    const float s = cos_sin[((size_t)pos * half + i) * 2 + 1];
    const float a = bf2f(head[i]);
    const float bvf = bf2f(head[i + half]);
    const unsigned short lo = f2bf(a * c - bvf * s);
    const unsigned short hi = f2bf(bvf * c + a * s);
    head[i] = lo;
    head[i + half] = hi;
    if (y >= Hq) {
      const int kvh = y - Hq;
      unsigned short* dst = Kc +
          (((size_t)b * Hkv + kvh) * Smax + pos) * D;
      dst[i] = lo;
      dst[i + half] = hi;
    }
  } else {
    const int kvh = y - Hq - Hkv;
    const unsigned short* src = row + (size_t)(Hq + Hkv + kvh) * D;
    unsigned short* dst = Vc + (((size_t)b * Hkv + kvh) * Smax + pos) * D;
    dst[i] = src[i];
    dst[i + half] = src[i + half];
  }
}

// fp8-KV variant: same rope + append, but the caches hold OCP e4m3
// bytes with one f32 scale per row (token): scale = row amax / 448.
// Halves KV-cache HBM traffic and memory; decode attention dequants
// while staging through LDS.
__global__ void rope_kv_fused_q8_kernel(
    unsigned short* __restrict__ qkv, unsigned char* __restrict__ Kc8,
    unsigned char* __restrict__ Vc8, float* __restrict__ kscale,
    float* __restrict__ vscale, const int* __restrict__ positions,
    const float* __restrict__ cos_sin, int Hq, int Hkv, int Smax, int D,
    long long row_stride) {
  const int b = blockIdx.x;
  const int y = blockIdx.y;
  const int i = threadIdx.x;  // 0..D/2-1 (one wave when D=128)
  const int half = D >> 1;
  const int pos = positions[b];
  unsigned short* row = qkv + (size_t)b * row_stride;
  float lo_f = 0.f, hi_f = 0.f;
  if (y < Hq + Hkv) {
    unsigned short* head = row + (size_t)y * D;
    const float c = cos_sin[((size_t)pos * half + i) * 2];
    const float sn = cos_sin[((size_t)pos * half + i) * 2 + 1];
    const float a = bf2f(head[i]);
    const float bvf = bf2f(head[i + half]);
    lo_f = a * c - bvf * sn;
    hi_f = bvf * c + a * sn;
    head[i] = f2bf(lo_f);
    head[i + half] = f2bf(hi_f);
    if (y < Hq) return;
  } else {
    const unsigned short* src = row + (size_t)y * D;
    lo_f = bf2f(src[i]);
    hi_f = bf2f(src[i + half]);
  }
  // wave-reduce the row amax (D/2 lanes x 2 values)
  float amax = fmaxf(fabsf(lo_f), fabsf(hi_f));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    amax = fmaxf(amax, __shfl_xor(amax, off, 64));
  const float qs = (amax > 0.f) ? amax / 448.f : 1.f;
  const float qinv = 1.f / qs;
  const bool is_k = (y < Hq + Hkv);
  const int kvh = is_k ? (y - Hq) : (y - Hq - Hkv);
  const size_t rowi = ((size_t)b * Hkv + kvh) * Smax + pos;
  unsigned char* dst = (is_k ? Kc8 : Vc8) + rowi * D;
  __hip_fp8_e4m3 lo8(lo_f * qinv), hi8(hi_f * qinv);
  dst[i] = lo8.__x;
  dst[i + half] = hi8.__x;
  if (i == 0) (is_k ? kscale : vscale)[rowi] = qs;
}

void launch_rope_kv_fused(void* qkv, void* Kc, void* Vc,
                          const void* positions, const void* cos_sin, int B,
                          int Hq, int Hkv, int Smax, int D,
                          long long row_stride, void* stream) {
  hipLaunchKernelGGL(rope_kv_fused_kernel, dim3(B, Hq + 2 * Hkv),
                     dim3(D / 2), 0, (hipStream_t)stream,
                     (unsigned short*)qkv, (unsigned short*)Kc,
                     (unsigned short*)Vc, (const int*)positions,
                     (const float*)cos_sin, Hq, Hkv, Smax, D, row_stride);
}

void launch_rope_kv_fused_q8(void* qkv, void* Kc8, void* Vc8,
                             void* kscale, void* vscale,
                             const void* positions, const void* cos_sin,
                             int B, int Hq, int Hkv, int Smax, int D,
                             long long row_stride, void* stream) {
  hipLaunchKernelGGL(rope_kv_fused_q8_kernel, dim3(B, Hq + 2 * Hkv),
                     dim3(D / 2), 0, (hipStream_t)stream,
                     (unsigned short*)qkv, (unsigned char*)Kc8,
                     (unsigned char*)Vc8, (float*)kscale, (float*)vscale,
                     (const int*)positions, (const float*)cos_sin, Hq,
                     Hkv, Smax, D, row_stride);
}

// ---------------------------------------------------------------------
// Decode attention (single new token per sequence, GQA):
//   O[b,h,:] = softmax(Q[b,h,:] K[b,kvh,:len,:]^T * scale) V[b,kvh,:len,:]
// One workgroup per (b, kv-head); one wave per grouped q-head.
//
// K/V chunks are staged through LDS by ALL waves cooperatively: the G
// grouped q-heads attend to the SAME kv rows, so per-wave global reads
// would issue the identical K and V bytes G times (L2 absorbs the
// reuse but the kernel becomes issue/latency-bound — measured 2.5
// TB/s apparent).  One cooperative load + G waves reading LDS cuts
// vector-memory traffic G-fold.  dim must be 128 (llama head_dim).
// ---------------------------------------------------------------------
#define ATTN_SCHUNK 64  // default rows staged per LDS buffer
#define ATTN_MAXG 8

struct AttnState {
  float m, l, acc0, acc1;
};

// shared chunk loop: stage [s_begin, s_final) through kbuf/vbuf and
// accumulate the online-softmax state for this wave's head
struct uchar16v { unsigned char v[16]; };

#define ATTN_LDS_PAD 8  // halves; rows start on different banks
template <int SCHUNK, bool KVQ>
__device__ __forceinline__ AttnState attn_chunk_loop(
    const void* __restrict__ kbase_, const void* __restrict__ vbase_,
    const float* __restrict__ kscale, const float* __restrict__ vscale,
    const float* qf, float scale, int s_begin, int s_final,
    int wave, int lane, int tid, int nthreads,
    unsigned short (*kbuf)[128 + ATTN_LDS_PAD],
    unsigned short (*vbuf)[128 + ATTN_LDS_PAD],
    float (*scores)[SCHUNK]) {
  constexpr int D = 128;
  AttnState st = {-FLT_MAX, 0.f, 0.f, 0.f};
  const int d0 = lane * 2;
  for (int s0 = s_begin; s0 < s_final; s0 += SCHUNK) {
    const int cnt = min(SCHUNK, s_final - s0);
    if (!KVQ) {
      // --- cooperative stage: every thread loads 16B K/V vectors
      const unsigned short* kbase = (const unsigned short*)kbase_;
      const unsigned short* vbase = (const unsigned short*)vbase_;
      const int total_vec = cnt * (D / 8);
      for (int i = tid; i < total_vec; i += nthreads) {
        const int row = i >> 4;
        const int col = (i & 15) * 8;
        const size_t off = (size_t)(s0 + row) * D + col;
        *reinterpret_cast<ushort8*>(&kbuf[row][col]) =
            *reinterpret_cast<const ushort8*>(kbase + off);
        *reinterpret_cast<ushort8*>(&vbuf[row][col]) =
            *reinterpret_cast<const ushort8*>(vbase + off);
      }
    } else {
      // --- fp8 cache: 16B loads carry 16 dims; dequant into LDS bf16
      const unsigned char* k8 = (const unsigned char*)kbase_;
      const unsigned char* v8 = (const unsigned char*)vbase_;
      const int total_vec = cnt * (D / 16);
      for (int i = tid; i < total_vec; i += nthreads) {
        const int row = i >> 3;
        const int col = (i & 7) * 16;
        const size_t off = (size_t)(s0 + row) * D + col;
        const uchar16v kq = *reinterpret_cast<const uchar16v*>(k8 + off);
        const uchar16v vq = *reinterpret_cast<const uchar16v*>(v8 + off);
        const float ks = kscale[s0 + row];
        const float vs = vscale[s0 + row];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          __hip_fp8_e4m3 kf8, vf8;
          kf8.__x = kq.v[j];
          vf8.__x = vq.v[j];
          kbuf[row][col + j] = f2bf(float(kf8) * ks);
          vbuf[row][col + j] = f2bf(float(vf8) * vs);
        }
      }
    }
    __syncthreads();
    // --- scores from LDS (16-lane groups each cover all 128 dims)
    for (int si = lane >> 4; si < cnt; si += 4) {
      const unsigned short* kp = &kbuf[si][(lane & 15) * 8];
      ushort8 kv = *reinterpret_cast<const ushort8*>(kp);
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) dot += qf[j] * bf2f(kv.v[j]);
#pragma unroll
      for (int off = 8; off > 0; off >>= 1)
        dot += __shfl_xor(dot, off, 64);
      if ((lane & 15) == 0) scores[wave][si] = dot * scale;
    }
    __syncthreads();
    // --- chunk max (wave-wide) ---
    float cm = -FLT_MAX;
    for (int si = lane; si < cnt; si += 64)
      cm = fmaxf(cm, scores[wave][si]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      cm = fmaxf(cm, __shfl_xor(cm, off, 64));
    const float m_new = fmaxf(st.m, cm);
    const float rescale = (st.m == -FLT_MAX) ? 0.f : __expf(st.m - m_new);
    st.acc0 *= rescale;
    st.acc1 *= rescale;
    st.l *= rescale;
    // --- p * V from LDS (lane owns dims d0, d0+1) ---
    for (int si = 0; si < cnt; ++si) {
      const float p = __expf(scores[wave][si] - m_new);
      st.l += p;
      const ushort2v vv =
          *reinterpret_cast<const ushort2v*>(&vbuf[si][d0]);
      st.acc0 += p * bf2f(vv.x);
      st.acc1 += p * bf2f(vv.y);
    }
    st.m = m_new;
    __syncthreads();
  }
  return st;
}

template <int SCHUNK, bool KVQ = false>
__global__ void attn_decode_kernel(
    unsigned short* __restrict__ O, const unsigned short* __restrict__ Q,
    const void* __restrict__ Kc, const void* __restrict__ Vc,
    const float* __restrict__ kscale, const float* __restrict__ vscale,
    const int* __restrict__ seq_lens, int B, int Hq, int Hkv, int Smax,
    float scale, long long q_row_stride) {
  constexpr int D = 128;
  const int b = blockIdx.x / Hkv;
  const int kvh = blockIdx.x % Hkv;
  const int G = Hq / Hkv;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int h = kvh * G + wave;
  const int len = seq_lens[b];

  __shared__ float scores[ATTN_MAXG][SCHUNK];
  __shared__ __align__(16) unsigned short kbuf[SCHUNK][D + ATTN_LDS_PAD];
  __shared__ __align__(16) unsigned short vbuf[SCHUNK][D + ATTN_LDS_PAD];

  // q fragment: lane holds 8 consecutive dims at (lane&15)*8 for the
  // K-dot phase (16-lane groups each cover all 128 dims)
  const unsigned short* qp = Q + (size_t)b * q_row_stride +
                             (size_t)h * D + (lane & 15) * 8;
  float qf[8];
  {
    ushort8 qv = *reinterpret_cast<const ushort8*>(qp);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = bf2f(qv.v[j]);
  }

  const size_t kv_row = ((size_t)b * Hkv + kvh) * Smax;
  const AttnState st = attn_chunk_loop<SCHUNK, KVQ>(
      (const char*)Kc + kv_row * D * (KVQ ? 1 : 2),
      (const char*)Vc + kv_row * D * (KVQ ? 1 : 2),
      kscale ? kscale + kv_row : nullptr,
      vscale ? vscale + kv_row : nullptr, qf, scale, 0, len, wave, lane,
      threadIdx.x, G * 64, kbuf, vbuf, scores);

  const float inv = (st.l > 0.f) ? 1.f / st.l : 0.f;
  unsigned short* op = O + ((size_t)b * Hq + h) * D + lane * 2;
  op[0] = f2bf(st.acc0 * inv);
  op[1] = f2bf(st.acc1 * inv);
}

// ---------------------------------------------------------------------
// Flash-decode split-S: nsplit workgroups per (b, kv-head) each cover
// a slice of the sequence and write an unnormalized partial
// (acc[D], m, l) to the workspace; a combine kernel folds the slices.
// Fills the chip even at small B*Hkv (the single-workgroup variant
// peaked at 128 workgroups on 256 CUs).
// partial layout: [B, Hq, nsplit, D+2] f32
// ---------------------------------------------------------------------
template <int SCHUNK, bool KVQ = false>
__global__ void attn_decode_split_kernel(
    float* __restrict__ partial, const unsigned short* __restrict__ Q,
    const void* __restrict__ Kc, const void* __restrict__ Vc,
    const float* __restrict__ kscale, const float* __restrict__ vscale,
    const int* __restrict__ seq_lens, int B, int Hq, int Hkv, int Smax,
    float scale, long long q_row_stride, int nsplit) {
  constexpr int D = 128;
  const int b = blockIdx.x / Hkv;
  const int kvh = blockIdx.x % Hkv;
  const int split = blockIdx.y;
  const int G = Hq / Hkv;
  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int h = kvh * G + wave;
  const int len = seq_lens[b];
  const int per = (len + nsplit - 1) / nsplit;
  const int s_begin = split * per;
  const int s_final = min(len, s_begin + per);
  float* prow = partial + (((size_t)b * Hq + h) * nsplit + split) * (D + 2);

  __shared__ float scores[ATTN_MAXG][SCHUNK];
  __shared__ __align__(16) unsigned short kbuf[SCHUNK][D + ATTN_LDS_PAD];
  __shared__ __align__(16) unsigned short vbuf[SCHUNK][D + ATTN_LDS_PAD];

  const unsigned short* qp = Q + (size_t)b * q_row_stride +
                             (size_t)h * D + (lane & 15) * 8;
  float qf[8];
  {
    ushort8 qv = *reinterpret_cast<const ushort8*>(qp);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = bf2f(qv.v[j]);
  }
  const size_t kv_row = ((size_t)b * Hkv + kvh) * Smax;
  const AttnState st = attn_chunk_loop<SCHUNK, KVQ>(
      (const char*)Kc + kv_row * D * (KVQ ? 1 : 2),
      (const char*)Vc + kv_row * D * (KVQ ? 1 : 2),
      kscale ? kscale + kv_row : nullptr,
      vscale ? vscale + kv_row : nullptr, qf, scale, s_begin, s_final,
      wave, lane, threadIdx.x, G * 64, kbuf, vbuf, scores);

  prow[lane * 2] = st.acc0;
  prow[lane * 2 + 1] = st.acc1;
  if (lane == 0) {
    prow[D] = st.m;
    prow[D + 1] = st.l;
  }
}

// fold the nsplit partials: one wave per (b, h)
__global__ void attn_decode_combine_kernel(
    unsigned short* __restrict__ O, const float* __restrict__ partial,
    int Hq, int nsplit) {
  constexpr int D = 128;
  const int bh = blockIdx.x;
  const int lane = threadIdx.x;
  const float* base = partial + (size_t)bh * nsplit * (D + 2);
  float m_star = -FLT_MAX;
  for (int s = 0; s < nsplit; ++s)
    m_star = fmaxf(m_star, base[s * (D + 2) + D]);
  float l_total = 0.f, a0 = 0.f, a1 = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float* prow = base + s * (D + 2);
    const float ms = prow[D];
    if (ms == -FLT_MAX) continue;
    const float wgt = __expf(ms - m_star);
    l_total += wgt * prow[D + 1];
    a0 += wgt * prow[lane * 2];
    a1 += wgt * prow[lane * 2 + 1];
  }
  const float inv = (l_total > 0.f) ? 1.f / l_total : 0.f;
  unsigned short* op = O + (size_t)bh * D + lane * 2;
  op[0] = f2bf(a0 * inv);
  op[1] = f2bf(a1 * inv);
}

// staged-chunk rows: 32 halves LDS/WG (16.5 KB -> ~8 WGs/CU = 8
// waves/SIMD) vs 64 (33 KB -> 4 waves/SIMD); selectable for sweeps
// via MLRUN_ATTN_SCHUNK, default chosen by measurement.
static int attn_schunk_env() {
  static int v = [] {
    const char* e = getenv("MLRUN_ATTN_SCHUNK");
    return e ? atoi(e) : 32;
  }();
  return v;
}

void launch_attn_decode(void* O, const void* Q, const void* Kc,
                        const void* Vc, const void* kscale,
                        const void* vscale, const void* seq_lens, int B,
                        int Hq, int Hkv, int Smax, float scale,
                        long long q_row_stride, float* partial_ws,
                        int nsplit, void* stream) {
  const int G = Hq / Hkv;
  const bool c64 = attn_schunk_env() >= 64;
  const bool kvq = kscale != nullptr;
  if (nsplit <= 1 || partial_ws == nullptr) {
    auto* kern = kvq ? (c64 ? attn_decode_kernel<64, true>
                            : attn_decode_kernel<32, true>)
                     : (c64 ? attn_decode_kernel<64, false>
                            : attn_decode_kernel<32, false>);
    hipLaunchKernelGGL(kern, dim3(B * Hkv), dim3(G * 64), 0,
                       (hipStream_t)stream, (unsigned short*)O,
                       (const unsigned short*)Q, Kc, Vc,
                       (const float*)kscale, (const float*)vscale,
                       (const int*)seq_lens, B,
                       Hq, Hkv, Smax, scale, q_row_stride);
    return;
  }
  auto* kern = kvq ? (c64 ? attn_decode_split_kernel<64, true>
                          : attn_decode_split_kernel<32, true>)
                   : (c64 ? attn_decode_split_kernel<64, false>
                          : attn_decode_split_kernel<32, false>);
  hipLaunchKernelGGL(kern, dim3(B * Hkv, nsplit),
                     dim3(G * 64), 0, (hipStream_t)stream, partial_ws,
                     (const unsigned short*)Q, Kc, Vc,
                     (const float*)kscale, (const float*)vscale,
                     (const int*)seq_lens, B, Hq,
                     Hkv, Smax, scale, q_row_stride, nsplit);
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3(B * Hq), dim3(64), 0,
                     (hipStream_t)stream, (unsigned short*)O, partial_ws,
                     Hq, nsplit);
}

// ---------------------------------------------------------------------
// KV-cache append: scatter the new token's K/V into the cache at
// position seq_lens[b] (pre-increment positions computed host-side).
// knew/vnew: [B, Hkv, D]; cache: [B, Hkv, Smax, D]
// ---------------------------------------------------------------------
__global__ void kv_append_kernel(unsigned short* __restrict__ Kc,
                                 unsigned short* __restrict__ Vc,
                                 const unsigned short* __restrict__ knew,
                                 const unsigned short* __restrict__ vnew,
                                 const int* __restrict__ positions, int Hkv,
                                 int Smax, int D, long long src_row_stride) {
  const int b = blockIdx.x;
  const int kvh = blockIdx.y;
  const int pos = positions[b];
  const size_t src = (size_t)b * src_row_stride + (size_t)kvh * D;
  const size_t dst = (((size_t)b * Hkv + kvh) * Smax + pos) * D;
  for (int i = threadIdx.x * 8; i < D; i += blockDim.x * 8) {
    *reinterpret_cast<ushort8*>(Kc + dst + i) =
        *reinterpret_cast<const ushort8*>(knew + src + i);
    *reinterpret_cast<ushort8*>(Vc + dst + i) =
        *reinterpret_cast<const ushort8*>(vnew + src + i);
  }
}

void launch_kv_append(void* Kc, void* Vc, const void* knew, const void* vnew,
                      const void* positions, int B, int Hkv, int Smax, int D,
                      long long src_row_stride, void* stream) {
  hipLaunchKernelGGL(kv_append_kernel, dim3(B, Hkv), dim3(D / 8), 0,
                     (hipStream_t)stream, (unsigned short*)Kc,
                     (unsigned short*)Vc, (const unsigned short*)knew,
                     (const unsigned short*)vnew, (const int*)positions, Hkv,
                     Smax, D, src_row_stride);
}

// ---------------------------------------------------------------------
// Packed (varlen) prefill, part 1: RoPE + KV append over a packed token
// stream.  Same math as rope_kv_fused_kernel; the only difference is
// that token t's cache row is tok_slot[t] rather than the row index,
// so tokens of several sequences share one launch.  bf16 caches only.
// grid: (T, Hq + 2*Hkv); block: D/2 threads.
// A token whose slot or position is out of range is left untouched.
// ---------------------------------------------------------------------
__global__ void rope_kv_varlen_kernel(
    unsigned short* __restrict__ qkv, unsigned short* __restrict__ Kc,
    unsigned short* __restrict__ Vc, const int* __restrict__ positions,
    const int* __restrict__ tok_slot, const float* __restrict__ cos_sin,
    int B, int Hq, int Hkv, int Smax, int D, int max_pos,
    long long row_stride) {
  const int t = blockIdx.x;
  const int y = blockIdx.y;
  const int i = threadIdx.x;  // 0..D/2-1
  const int half = D >> 1;
  const int pos = positions[t];
  const int slot = tok_slot[t];
  if (pos < 0 || pos >= max_pos || pos >= Smax ||
      (unsigned)slot >= (unsigned)B)
    return;
  unsigned short* row = qkv + (size_t)t * row_stride;
  if (y < Hq + Hkv) {
    unsigned short* head = row + (size_t)y * D;
    const float c = cos_sin[((size_t)pos * half + i) * 2];
    const float s = cos_sin[((size_t)pos * half + i) * 2 + 1];
    const float a = bf2f(head[i]);
    const float bvf = bf2f(head[i + half]);
    const unsigned short lo = f2bf(a * c - bvf * s);
    const unsigned short hi = f2bf(bvf * c + a * s);
    head[i] = lo;
    head[i + half] = hi;
    if (y >= Hq) {
      const int kvh = y - Hq;
      unsigned short* dst = Kc +
          (((size_t)slot * Hkv + kvh) * Smax + pos) * D;
      dst[i] = lo;
      dst[i + half] = hi;
    }
  } else {
    const int kvh = y - Hq - Hkv;
    const unsigned short* src = row + (size_t)(Hq + Hkv + kvh) * D;
    unsigned short* dst =
        Vc + (((size_t)slot * Hkv + kvh) * Smax + pos) * D;
    dst[i] = src[i];
    dst[i + half] = src[i + half];
  }
}

void launch_rope_kv_varlen(void* qkv, void* Kc, void* Vc,
                           const void* positions, const void* tok_slot,
                           const void* cos_sin, int T, int B, int Hq,
                           int Hkv, int Smax, int D, int max_pos,
                           long long row_stride, void* stream) {
  hipLaunchKernelGGL(rope_kv_varlen_kernel, dim3(T, Hq + 2 * Hkv),
                     dim3(D / 2), 0, (hipStream_t)stream,
                     (unsigned short*)qkv, (unsigned short*)Kc,
                     (unsigned short*)Vc, (const int*)positions,
                     (const int*)tok_slot, (const float*)cos_sin, B, Hq,
                     Hkv, Smax, D, max_pos, row_stride);
}

// ---------------------------------------------------------------------
// Prefix cache: copy 32-token KV blocks between two 5-d bf16 tensors,
// src [L, Rs, Hkv, Ss, D] -> dst [L, Rd, Hkv, Sd, D].  Entry e moves rows
// [src_blk[e]*32, +32) of src[:, src_row[e]] to rows [dst_blk[e]*32, +32)
// of dst[:, dst_row[e]], for every layer and KV head, K and V alike.
// The block pool is [L, N, Hkv, 32, D] and the engine cache
// [L, B, Hkv, Smax, D], so one kernel gathers (pool -> slot) and
// scatters (slot -> pool).  The 32 rows of one (layer, row, head) are
// contiguous: a workgroup copies 32*D*2 bytes per tensor in 16-byte
// pieces.  All element offsets are 64-bit (an 8B cache passes 2^31).
// grid: (n, L*Hkv); block: 256 threads.
// An entry whose row is out of range, or whose block would reach past
// Ss or Sd, is left untouched as a whole.  Destinations are distinct.
// ---------------------------------------------------------------------
constexpr int KV_BLOCK_TOKENS = 32;

__global__ void kv_block_copy_kernel(
    const unsigned short* __restrict__ srcK,
    const unsigned short* __restrict__ srcV,
    unsigned short* __restrict__ dstK, unsigned short* __restrict__ dstV,
    const int* __restrict__ src_row, const int* __restrict__ src_blk,
    const int* __restrict__ dst_row, const int* __restrict__ dst_blk,
    int Hkv, int Rs, int Ss, int Rd, int Sd, int D) {
  const int e = blockIdx.x;
  const int layer = blockIdx.y / Hkv;
  const int kvh = blockIdx.y % Hkv;
  const int sr = src_row[e], sb = src_blk[e];
  const int dr = dst_row[e], db = dst_blk[e];
  if ((unsigned)sr >= (unsigned)Rs || (unsigned)dr >= (unsigned)Rd ||
      sb < 0 || db < 0 ||
      ((long long)sb + 1) * KV_BLOCK_TOKENS > (long long)Ss ||
      ((long long)db + 1) * KV_BLOCK_TOKENS > (long long)Sd)
    return;
  const size_t src =
      ((((size_t)layer * Rs + sr) * Hkv + kvh) * Ss +
       (size_t)sb * KV_BLOCK_TOKENS) * D;
  const size_t dst =
      ((((size_t)layer * Rd + dr) * Hkv + kvh) * Sd +
       (size_t)db * KV_BLOCK_TOKENS) * D;
  const int elems = KV_BLOCK_TOKENS * D;  // D % 8 == 0 (host-checked)
  for (int i = threadIdx.x * 8; i < elems; i += blockDim.x * 8) {
    *reinterpret_cast<ushort8*>(dstK + dst + i) =
        *reinterpret_cast<const ushort8*>(srcK + src + i);
    *reinterpret_cast<ushort8*>(dstV + dst + i) =
        *reinterpret_cast<const ushort8*>(srcV + src + i);
  }
}

void launch_kv_block_copy(const void* srcK, const void* srcV, void* dstK,
                          void* dstV, const void* src_row,
                          const void* src_blk, const void* dst_row,
                          const void* dst_blk, int n, int L, int Hkv,
                          int Rs, int Ss, int Rd, int Sd, int D,
                          void* stream) {
  hipLaunchKernelGGL(kv_block_copy_kernel, dim3(n, L * Hkv), dim3(256), 0,
                     (hipStream_t)stream, (const unsigned short*)srcK,
                     (const unsigned short*)srcV, (unsigned short*)dstK,
                     (unsigned short*)dstV, (const int*)src_row,
                     (const int*)src_blk, (const int*)dst_row,
                     (const int*)dst_blk, Hkv, Rs, Ss, Rd, Sd, D);
}

// ---------------------------------------------------------------------
// Packed (varlen) prefill, part 2: causal GQA flash-attention forward
// over the slot-indexed KV cache.
//
//   query j of sequence i sits at position p = kv_start[i] + j and
//   attends to rows 0..p of cache[slots[i], h / G].
//
// grid (ceil(max_q_len / 64), Hq, n); block 256 = 4 waves.  A workgroup
// owns 64 query rows of one (sequence, q-head); each wave owns 16 rows,
// one MFMA M-tile.  KV is walked in 64-row tiles up to the workgroup's
// last query position only; tiles above the diagonal are never visited,
// and a wave skips the MFMAs of a tile that lies wholly above its own
// 16 rows.  Only tiles that reach past a wave's first row apply the
// element mask.
//
// Both products run TRANSPOSED on v_mfma_f32_16x16x32_bf16:
//   S^T = K . Q^T   A = K rows from LDS (one 16 B row read per lane),
//                   B = the Q fragments, loaded once, kept in registers
//   O^T += V^T . P^T
// The transposed score tile has its query on the lane (col = lane & 15)
// and its keys in the registers (row = 4*(lane >> 4) + reg), which is
// already the B-operand shape of the second product once a lane's
// registers of two 16-key tiles are packed to 8 bf16: P never leaves
// the registers, so there is no LDS round trip for it.  The k order
// inside such a 32-key step is permuted (slot 8h+j = key 16*(j>>2) +
// 4h + (j&3)); the V^T operand is read in the same order by two
// ds_read_b64_tr_b16 per fragment, which transpose a 4-key x 16-dim
// block of the row-major V tile on the way out of LDS, so V is staged
// exactly as it lies in the cache (no transposed stage, no 2-byte
// scatter writes).  With the query on the lane, the softmax row max
// and sum are a register reduction plus two cross-lane steps (the 4
// lanes lane&15, +16, +32, +48 share a row) and the rescale factor is
// a per-lane scalar.
//
// K/V tiles are fetched with 16 B global loads into registers while the
// previous tile is being consumed and written to LDS after the barrier
// (rows padded, like the decode kernel's ATTN_LDS_PAD).  Cache rows at
// or past the sequence's end are never loaded: they are staged as
// zeros, so stale Inf/NaN in the cache cannot reach either MFMA.
// ---------------------------------------------------------------------
#define PF_BM 64
#define PF_BN 64
// LDS row = 128 halves + 16 of padding (288 B): consecutive rows start
// 8 banks apart, which makes both the 16 B K row reads and the 8 B
// transposed V reads conflict-free within their lane groups.
#define PF_ROW (128 + 16)

typedef __attribute__((ext_vector_type(4))) short short4v;

DEV short4v pf_read_tr16(const unsigned short* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (__attribute__((address_space(3))) short4v*)p);
}

// f32 -> bf16, round-to-nearest-even like f2bf, but through the
// compiler's conversion so that gfx950's packed hardware convert is
// used (16 of these per KV tile sit between the two MFMA blocks)
DEV short pf_f2bf(float f) {
  return __builtin_bit_cast(short, (__bf16)f);
}

// ---- the tile pipeline shared by attn_prefill and attn_verify --------

// Q fragments of one lane: loaded once, live across the whole tile loop
DEV void pf_load_q(short8v (&qf)[4], const unsigned short* qp) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    qf[ks] = *reinterpret_cast<const short8v*>(qp + ks * 32);
}

// K/V staging of one thread: a 64-row tile is 64 x 16 chunks of 16 B,
// 4 chunks of K and 4 of V per thread, held in registers between the
// global load (issue) and the LDS write (commit)
struct PfStage {
  const unsigned short* kbase;  // cache rows of this (slot, kv head)
  const unsigned short* vbase;
  unsigned short* kbuf;
  unsigned short* vbuf;
  int kv_end;  // rows at or past it are staged as zeros
  int tid;
  short8v kreg[4], vreg[4];

  DEV void issue(int tile0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      const int key = tile0 + (c >> 4);
      const short8v zero = {0, 0, 0, 0, 0, 0, 0, 0};
      kreg[i] = zero;
      vreg[i] = zero;
      if (key < kv_end) {
        const size_t off = (size_t)key * 128 + (c & 15) * 8;
        kreg[i] = *reinterpret_cast<const short8v*>(kbase + off);
        vreg[i] = *reinterpret_cast<const short8v*>(vbase + off);
      }
    }
  }
  DEV void commit() const {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      const int off = (c >> 4) * PF_ROW + (c & 15) * 8;
      *reinterpret_cast<short8v*>(kbuf + off) = kreg[i];
      *reinterpret_cast<short8v*>(vbuf + off) = vreg[i];
    }
  }
};

// One 64-key tile for one wave's 16 columns: both products and the
// online softmax between them.  `pos` is the lane's query position;
// need_mask (wave-uniform) says whether the tile reaches past the
// lowest position of the wave, so that keys > pos must be masked.
DEV void pf_tile(const unsigned short* kbuf, const unsigned short* vbuf,
                 const short8v (&qf)[4], f32x4v (&o)[8], float& m, float& l,
                 int tile0, bool need_mask, int pos, float scale_log2e,
                 int lq, int lh) {
  // --- S^T = K . Q^T : 4 key tiles x 4 k-steps
  f32x4v s[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    s[kt] = f32x4v{0.f, 0.f, 0.f, 0.f};
    const unsigned short* kp = kbuf + (kt * 16 + lq) * PF_ROW + lh * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const short8v kf = *reinterpret_cast<const short8v*>(kp + ks * 32);
      s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[ks], s[kt], 0,
                                                      0, 0);
    }
  }
  // --- scale, causal mask, tile max
  float mx = -__builtin_inff();
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float x = s[kt][r] * scale_log2e;
      if (need_mask && tile0 + kt * 16 + lh * 4 + r > pos)
        x = -__builtin_inff();
      s[kt][r] = x;
      mx = fmaxf(mx, x);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  // --- online softmax: rescale everything held at the old max.  A
  // column with no visible key in this tile has mx = -inf: m stays put,
  // alpha = 1 and every p = exp2(-inf) = 0
  const float m_new = fmaxf(m, mx);
  const float alpha = __builtin_amdgcn_exp2f(m - m_new);
  m = m_new;
  float psum = 0.f;
  short8v pb[2];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f(s[kt][r] - m_new);
      psum += p;
      pb[kt >> 1][(kt & 1) * 4 + r] = pf_f2bf(p);
    }
  }
  l = l * alpha + psum;
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) o[dt] *= alpha;
  // --- O^T += V^T . P^T : 8 dim tiles x 2 k-steps of 32 keys
  const unsigned short* vp =
      vbuf + (lh * 4 + (lq >> 2)) * PF_ROW + (lq & 3) * 4;
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const short4v lo = pf_read_tr16(vp + (ks * 32) * PF_ROW + dt * 16);
      const short4v hi =
          pf_read_tr16(vp + (ks * 32 + 16) * PF_ROW + dt * 16);
      const short8v vf =
          __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb[ks], o[dt], 0,
                                                      0, 0);
    }
  }
}

// finish a column's sum across the 4 lanes that share it
DEV float pf_finish_l(float l) {
  l += __shfl_xor(l, 16, 64);
  return l + __shfl_xor(l, 32, 64);
}

// normalised bf16 output of one lane: 4 dims of each of the 8 dim tiles
DEV void pf_store_bf16(unsigned short* op, const f32x4v (&o)[8], float inv) {
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) {
    ushort4 w;
    w.x = f2bf(o[dt][0] * inv);
    w.y = f2bf(o[dt][1] * inv);
    w.z = f2bf(o[dt][2] * inv);
    w.w = f2bf(o[dt][3] * inv);
    *reinterpret_cast<ushort4*>(op + dt * 16) = w;
  }
}

__global__ __launch_bounds__(256) void attn_prefill_kernel(
    unsigned short* __restrict__ O, const unsigned short* __restrict__ Q,
    const unsigned short* __restrict__ Kc,
    const unsigned short* __restrict__ Vc,
    const int* __restrict__ cu_seqlens, const int* __restrict__ slots,
    const int* __restrict__ kv_start, int T, int B, int Hq, int Hkv,
    int Smax, float scale_log2e, long long q_row_stride) {
  constexpr int D = 128;
  __shared__ __attribute__((aligned(16)))
      unsigned short lds[2 * PF_BN * PF_ROW];
  unsigned short* kbuf = lds;
  unsigned short* vbuf = lds + PF_BN * PF_ROW;

  const int seq = blockIdx.z;
  const int h = blockIdx.y;
  const int q0 = blockIdx.x * PF_BM;
  // --- block-uniform setup and early exits (before any barrier)
  const int row0 = cu_seqlens[seq];
  int qlen = cu_seqlens[seq + 1] - row0;
  if (row0 < 0) return;
  qlen = min(qlen, T - row0);
  if (q0 >= qlen) return;  // tile past this sequence's end
  const int slot = slots[seq];
  const int start = kv_start[seq];
  if ((unsigned)slot >= (unsigned)B || start < 0) return;
  const int q_hi = min(q0 + PF_BM, qlen);      // one past the last row
  const int kv_end = min(start + q_hi, Smax);  // keys this block sees
  const int ntiles = (kv_end + PF_BN - 1) / PF_BN;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int lq = lane & 15;  // query column of the transposed tiles
  const int lh = lane >> 4;
  const int wrow0 = q0 + wave * 16;
  const bool wave_active = wrow0 < qlen;
  const int qr = wrow0 + lq;
  const bool row_valid = qr < qlen;
  const int pos = start + qr;                       // this lane's query
  const int wave_min_pos = start + wrow0;
  const int wave_max_pos = start + min(wrow0 + 15, qlen - 1);

  short8v qf[4];
  pf_load_q(qf, Q + (size_t)(row0 + min(qr, qlen - 1)) * q_row_stride +
                    (size_t)h * D + lh * 8);

  const int kvh = h / (Hq / Hkv);
  const size_t cbase = ((size_t)slot * Hkv + kvh) * Smax * D;
  PfStage st{Kc + cbase, Vc + cbase, kbuf, vbuf, kv_end, tid};

  f32x4v o[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) o[dt] = f32x4v{0.f, 0.f, 0.f, 0.f};
  float m = -1e30f;  // running row max (log2 domain), finite on purpose
  float l = 0.f;     // this lane's share of the row sum

  st.issue(0);
  for (int t = 0; t < ntiles; ++t) {
    const int tile0 = t * PF_BN;
    __syncthreads();  // everyone is done reading the previous tile
    st.commit();
    __syncthreads();
    if (t + 1 < ntiles) st.issue(tile0 + PF_BN);  // flies under the MFMAs
    if (!wave_active || tile0 > wave_max_pos) continue;
    // causal mask on diagonal tiles only
    const bool need_mask = tile0 + PF_BN - 1 > wave_min_pos;
    pf_tile(kbuf, vbuf, qf, o, m, l, tile0, need_mask, pos, scale_log2e, lq,
            lh);
  }

  // --- epilogue
  l = pf_finish_l(l);
  if (!row_valid) return;
  pf_store_bf16(O + ((size_t)(row0 + qr) * Hq + h) * D + lh * 4, o,
                1.f / l);
}

void launch_attn_prefill(void* O, const void* Q, const void* Kc,
                         const void* Vc, const void* cu_seqlens,
                         const void* slots, const void* kv_start, int T,
                         int nseq, int B, int Hq, int Hkv, int Smax,
                         float scale, long long q_row_stride,
                         int max_q_len, void* stream) {
  const int qtiles = (max_q_len + PF_BM - 1) / PF_BM;
  if (qtiles <= 0 || nseq <= 0) return;
  hipLaunchKernelGGL(attn_prefill_kernel, dim3(qtiles, Hq, nseq),
                     dim3(256), 0, (hipStream_t)stream,
                     (unsigned short*)O, (const unsigned short*)Q,
                     (const unsigned short*)Kc, (const unsigned short*)Vc,
                     (const int*)cu_seqlens, (const int*)slots,
                     (const int*)kv_start, T, B, Hq, Hkv, Smax,
                     scale * 1.4426950408889634f, q_row_stride);
}

// ---------------------------------------------------------------------
// Speculative verify attention: QL (1..8) query rows per sequence
// against a long cached prefix.
//
//   query j of batch row b sits at position base_lens[b] + j and
//   attends to rows 0..base_lens[b]+j of cache[b, h / G]; the QL new
//   K/V rows are already in the cache (rope_kv_varlen).
//
// grid (nsplit, Hkv, B); block 256 = 4 waves.  A workgroup owns ONE
// (batch row, KV head): the G x QL (q-head, query) pairs that share this
// KV head are the columns of attn_prefill's transposed tiles
// (column c = g * QL + j, <= 64 of them, 16 per wave), so K/V are read
// from HBM once per KV head instead of once per q-head, and a column
// tile is as full as G x QL allows (G=4, QL=4: exactly 16).  The two
// products, the register-resident P and the transposed V read (pf_tile)
// and the staging (PfStage, zeros at and past base + QL) are the code
// attn_prefill runs.  Waves
// whose column tile is empty only help with staging: the kernel is
// bound by the K/V stream, not by the MFMAs of its one or two busy
// waves (32 MFMAs per 32 KB tile).
//
// The causal mask is per column (key > base + j) and is applied only
// on tiles that reach past `base`.  A column that sees no key in a
// tile keeps m = -1e30, l = 0, o = 0 (finite, zero weight).
//
// Split-S: the row's 64-key tiles are dealt to ns = min(nsplit, tiles)
// splits in contiguous ranges (never an empty range); blocks of the
// remaining splits exit at once, and the combine kernel derives the
// same ns from base_lens.  A split writes unnormalised f32 partials
// (o[128], m, l; m in the log2 domain) per column with plain stores;
// attn_verify_combine_kernel folds them with exp2.  nsplit == 1 writes
// bf16 directly.  A row with base < 0 or base + QL > Smax is skipped in
// both kernels (block-uniform, before any barrier).
// ---------------------------------------------------------------------
#define VF_WS_ROW (128 + 4)  // o[128], m, l, pad: rows stay 16 B aligned

template <bool SPLIT>
__global__ __launch_bounds__(256) void attn_verify_kernel(
    unsigned short* __restrict__ O, float* __restrict__ ws,
    const unsigned short* __restrict__ Q,
    const unsigned short* __restrict__ Kc,
    const unsigned short* __restrict__ Vc,
    const int* __restrict__ base_lens, int QL, int Hq, int Hkv, int Smax,
    float scale_log2e, long long q_row_stride, int nsplit) {
  constexpr int D = 128;
  __shared__ __attribute__((aligned(16)))
      unsigned short lds[2 * PF_BN * PF_ROW];
  unsigned short* kbuf = lds;
  unsigned short* vbuf = lds + PF_BN * PF_ROW;

  const int split = blockIdx.x;
  const int kvh = blockIdx.y;
  const int b = blockIdx.z;
  // --- block-uniform setup and early exits (before any barrier)
  const int base = base_lens[b];
  if (base < 0 || base + QL > Smax) return;
  const int kv_end = base + QL;  // keys this row sees, <= Smax
  const int ntiles = (kv_end + PF_BN - 1) / PF_BN;
  const int ns = min(nsplit, ntiles);
  if (split >= ns) return;
  const int t_begin = (split * ntiles) / ns;
  const int t_end = ((split + 1) * ntiles) / ns;

  const int G = Hq / Hkv;
  const int ncols = G * QL;
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int lq = lane & 15;  // column of the transposed tiles
  const int lh = lane >> 4;
  const bool wave_active = wave * 16 < ncols;
  const int col = wave * 16 + lq;
  const bool col_valid = col < ncols;
  const int cc = min(col, ncols - 1);
  const int g = cc / QL;
  const int j = cc - g * QL;
  const int h = kvh * G + g;
  const int pos = base + j;  // this lane's query position
  const size_t qrow = (size_t)b * QL + j;

  short8v qf[4];
  pf_load_q(qf, Q + qrow * q_row_stride + (size_t)h * D + lh * 8);

  const size_t cbase = ((size_t)b * Hkv + kvh) * Smax * D;
  PfStage st{Kc + cbase, Vc + cbase, kbuf, vbuf, kv_end, tid};

  f32x4v o[8];
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) o[dt] = f32x4v{0.f, 0.f, 0.f, 0.f};
  float m = -1e30f;  // running column max (log2 domain), finite on purpose
  float l = 0.f;     // this lane's share of the column sum

  st.issue(t_begin * PF_BN);
  for (int t = t_begin; t < t_end; ++t) {
    const int tile0 = t * PF_BN;
    __syncthreads();  // everyone is done reading the previous tile
    st.commit();
    __syncthreads();
    if (t + 1 < t_end) st.issue(tile0 + PF_BN);  // flies under the MFMAs
    if (!wave_active) continue;
    // per-column causal mask on the tiles past `base`
    const bool need_mask = tile0 + PF_BN - 1 > base;
    pf_tile(kbuf, vbuf, qf, o, m, l, tile0, need_mask, pos, scale_log2e, lq,
            lh);
  }

  // --- epilogue
  l = pf_finish_l(l);
  if (!col_valid) return;
  const size_t orow = qrow * Hq + h;
  if (!SPLIT) {
    pf_store_bf16(O + orow * D + lh * 4, o, (l > 0.f) ? 1.f / l : 0.f);
  } else {
    float* prow = ws + (orow * nsplit + split) * VF_WS_ROW;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
      *reinterpret_cast<f32x4v*>(prow + dt * 16 + lh * 4) = o[dt];
    if (lh == 0) {
      prow[D] = m;
      prow[D + 1] = l;
    }
  }
}

// fold the split partials: one wave per output row (b, j, h); the same
// guard and the same split count as attn_verify_kernel
__global__ void attn_verify_combine_kernel(
    unsigned short* __restrict__ O, const float* __restrict__ ws,
    const int* __restrict__ base_lens, int QL, int Hq, int Smax,
    int nsplit) {
  constexpr int D = 128;
  const int row = blockIdx.x;  // (b * QL + j) * Hq + h
  const int lane = threadIdx.x;
  const int base = base_lens[row / (QL * Hq)];
  if (base < 0 || base + QL > Smax) return;
  const int ntiles = (base + QL + PF_BN - 1) / PF_BN;
  const int ns = min(nsplit, ntiles);
  const float* part = ws + (size_t)row * nsplit * VF_WS_ROW;
  float m_star = -1e30f;
  for (int s = 0; s < ns; ++s)
    m_star = fmaxf(m_star, part[s * VF_WS_ROW + D]);
  float l_total = 0.f, a0 = 0.f, a1 = 0.f;
  for (int s = 0; s < ns; ++s) {
    const float* prow = part + s * VF_WS_ROW;
    // log2 domain, like the partials; an empty column (m = -1e30)
    // weighs exp2(-huge) = 0 against any real max
    const float wgt = __builtin_amdgcn_exp2f(prow[D] - m_star);
    l_total += wgt * prow[D + 1];
    a0 += wgt * prow[lane * 2];
    a1 += wgt * prow[lane * 2 + 1];
  }
  const float inv = (l_total > 0.f) ? 1.f / l_total : 0.f;
  unsigned short* op = O + (size_t)row * D + lane * 2;
  op[0] = f2bf(a0 * inv);
  op[1] = f2bf(a1 * inv);
}

void launch_attn_verify(void* O, const void* Q, const void* Kc,
                        const void* Vc, const void* base_lens, int B,
                        int QL, int Hq, int Hkv, int Smax, float scale,
                        long long q_row_stride, float* partial_ws,
                        int nsplit, void* stream) {
  if (B <= 0) return;
  const float sl2 = scale * 1.4426950408889634f;
  if (nsplit <= 1 || partial_ws == nullptr) {
    hipLaunchKernelGGL(attn_verify_kernel<false>, dim3(1, Hkv, B),
                       dim3(256), 0, (hipStream_t)stream,
                       (unsigned short*)O, (float*)nullptr,
                       (const unsigned short*)Q, (const unsigned short*)Kc,
                       (const unsigned short*)Vc, (const int*)base_lens, QL,
                       Hq, Hkv, Smax, sl2, q_row_stride, 1);
    return;
  }
  hipLaunchKernelGGL(attn_verify_kernel<true>, dim3(nsplit, Hkv, B),
                     dim3(256), 0, (hipStream_t)stream, (unsigned short*)O,
                     partial_ws, (const unsigned short*)Q,
                     (const unsigned short*)Kc, (const unsigned short*)Vc,
                     (const int*)base_lens, QL, Hq, Hkv, Smax, sl2,
                     q_row_stride, nsplit);
  hipLaunchKernelGGL(attn_verify_combine_kernel, dim3(B * QL * Hq),
                     dim3(64), 0, (hipStream_t)stream, (unsigned short*)O,
                     (const float*)partial_ws, (const int*)base_lens, QL,
                     Hq, Smax, nsplit);
}

// ---------------------------------------------------------------------
// Prompt-lookup (n-gram) drafter, device side: for each row find the
// LATEST earlier occurrence of the row's last n tokens and propose the
// k tokens that followed it.
//   len = clamp(hist_lens[b], 0, L)
//   p*  = max p with p + n < len and hist[p..p+n) == hist[len-n..len)
//   drafts[b, j] = hist[p* + n + j] while p* + n + j < len,
//                  else hist[len - 1]   (also when there is no match)
//   len == 0 -> zeros
// One workgroup (256 threads) per row: lanes scan the candidate
// positions, a max-reduction picks the latest match.
// ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void ngram_draft_kernel(
    long long* __restrict__ drafts, const long long* __restrict__ history,
    const int* __restrict__ hist_lens, int L, int k, int n) {
  __shared__ int wave_best[4];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const long long* hist = history + (size_t)b * L;
  const int len = max(0, min(hist_lens[b], L));
  int best = -1;
  if (len >= n + 1) {
    const long long* tail = hist + (len - n);
    for (int p = tid; p + n < len; p += 256) {
      bool eq = true;
      for (int i = 0; i < n; ++i) eq = eq && (hist[p + i] == tail[i]);
      if (eq) best = p;  // p grows: the last hit is this lane's latest
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    best = max(best, __shfl_xor(best, off, 64));
  if ((tid & 63) == 0) wave_best[tid >> 6] = best;
  __syncthreads();
  best = max(max(wave_best[0], wave_best[1]),
             max(wave_best[2], wave_best[3]));
  for (int j = tid; j < k; j += 256) {
    long long tok = 0;
    if (len > 0) {
      const int src = (best >= 0) ? best + n + j : len;
      tok = hist[src < len ? src : len - 1];
    }
    drafts[(size_t)b * k + j] = tok;
  }
}

void launch_ngram_draft(void* drafts, const void* history,
                        const void* hist_lens, int B, int L, int k, int n,
                        void* stream) {
  if (B <= 0 || k <= 0) return;
  hipLaunchKernelGGL(ngram_draft_kernel, dim3(B), dim3(256), 0,
                     (hipStream_t)stream, (long long*)drafts,
                     (const long long*)history, (const int*)hist_lens, L, k,
                     n);
}

// ---------------------------------------------------------------------
// Multi-LoRA decode: batched gather mat-vec (BGMV) pair.  Row b of a
// decode batch uses adapter idx[b] of the tables A [NA, R, K] and
// Bm [NA, N, R] (bf16; alpha / r is folded into Bm at load time):
//   shrink: t[b, j] = sum_k x[b, k] * A[idx[b], j, k]           (f32)
//   expand: y[b, n] = bf16(float(y[b, n]) + sum_j t[b, j] * Bm[idx[b], n, j])
// idx is read on the device, so a captured graph follows whatever ids
// the host wrote last.  A row whose id is outside [0, NA) is skipped:
// its workgroup returns before any barrier (the test is block-uniform)
// and touches neither t nor y.
// ---------------------------------------------------------------------
#define LORA_SHRINK_THREADS 256
#define LORA_EXPAND_THREADS 128
#define LORA_EXPAND_TILE (2 * LORA_EXPAND_THREADS)  // n per workgroup

// One workgroup per (j, b): its 256 lanes sweep K in 16 B pieces, then
// wave shuffles and a 4-entry LDS fold give one f32 in a fixed order.
__global__ __launch_bounds__(LORA_SHRINK_THREADS) void lora_shrink_kernel(
    float* __restrict__ t, const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ A, const int* __restrict__ idx,
    int NA, int R, int K) {
  __shared__ float wave_sum[LORA_SHRINK_THREADS / 64];
  const int j = blockIdx.x;
  const int b = blockIdx.y;
  const int a = idx[b];
  if (a < 0 || a >= NA) return;
  const int tid = threadIdx.x;
  const unsigned short* xr = x + (size_t)b * K;
  const unsigned short* ar = A + ((size_t)a * R + j) * K;
  float acc = 0.f;
#pragma unroll 4
  for (int k = tid * 8; k < K; k += LORA_SHRINK_THREADS * 8) {
    const short8v xv = *reinterpret_cast<const short8v*>(xr + k);
    const short8v av = *reinterpret_cast<const short8v*>(ar + k);
#pragma unroll
    for (int i = 0; i < 8; ++i)
      acc += bf2f((unsigned short)xv[i]) * bf2f((unsigned short)av[i]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) wave_sum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0)
    t[(size_t)b * R + j] =
        (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// One workgroup per (256-wide n tile, b); a thread owns two adjacent
// outputs (one dword of y) and reads their two Bm rows, 2 * R bf16 in a
// row, with 16 B loads.  t[b, :] is staged in LDS.
template <int R>
__global__ __launch_bounds__(LORA_EXPAND_THREADS) void lora_expand_kernel(
    unsigned short* __restrict__ y, const float* __restrict__ t,
    const unsigned short* __restrict__ Bm, const int* __restrict__ idx,
    int NA, int N) {
  __shared__ float ts[R];
  const int b = blockIdx.y;
  const int a = idx[b];
  if (a < 0 || a >= NA) return;
  const int tid = threadIdx.x;
  if (tid < R) ts[tid] = t[(size_t)b * R + tid];
  __syncthreads();
  const int n = (blockIdx.x * LORA_EXPAND_THREADS + tid) * 2;
  if (n >= N) return;  // N is even: n + 1 < N as well
  const unsigned short* rows = Bm + ((size_t)a * N + n) * R;
  float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
  for (int j = 0; j < R; j += 8) {
    const short8v r0 = *reinterpret_cast<const short8v*>(rows + j);
    const short8v r1 = *reinterpret_cast<const short8v*>(rows + R + j);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      acc0 += ts[j + i] * bf2f((unsigned short)r0[i]);
      acc1 += ts[j + i] * bf2f((unsigned short)r1[i]);
    }
  }
  ushort2v* yp = reinterpret_cast<ushort2v*>(y + (size_t)b * N + n);
  ushort2v v = *yp;
  v.x = f2bf(bf2f(v.x) + acc0);
  v.y = f2bf(bf2f(v.y) + acc1);
  *yp = v;
}

void launch_lora_shrink(void* t, const void* x, const void* A,
                        const void* idx, int B, int NA, int R, int K,
                        void* stream) {
  if (B <= 0 || NA <= 0) return;
  hipLaunchKernelGGL(lora_shrink_kernel, dim3(R, B),
                     dim3(LORA_SHRINK_THREADS), 0, (hipStream_t)stream,
                     (float*)t, (const unsigned short*)x,
                     (const unsigned short*)A, (const int*)idx, NA, R, K);
}

void launch_lora_expand(void* y, const void* t, const void* Bm,
                        const void* idx, int B, int NA, int R, int N,
                        void* stream) {
  if (B <= 0 || NA <= 0) return;
  const dim3 grid((N + LORA_EXPAND_TILE - 1) / LORA_EXPAND_TILE, B);
#define LORA_EXPAND_CASE(RR)                                              \
  case RR:                                                                \
    hipLaunchKernelGGL(lora_expand_kernel<RR>, grid,                      \
                       dim3(LORA_EXPAND_THREADS), 0, (hipStream_t)stream, \
                       (unsigned short*)y, (const float*)t,               \
                       (const unsigned short*)Bm, (const int*)idx, NA, N); \
    break;
  switch (R) {
    LORA_EXPAND_CASE(8)
    LORA_EXPAND_CASE(16)
    LORA_EXPAND_CASE(32)
    LORA_EXPAND_CASE(64)
    default: break;  // the binding rejects other ranks
  }
#undef LORA_EXPAND_CASE
}

// ---------------------------------------------------------------------
// Fused per-request sampler.  One workgroup per logits row [V] bf16;
// every parameter of the row is read on the device, so a captured graph
// follows whatever the host wrote last.  Semantics (shared with the CPU
// reference in ops/__init__.py), z_i = float(logits[i]):
//   T == 0: argmax z, lowest index on ties (filters ignored).  So is
//           any T at which m = zmax / T is not a finite positive-T
//           quotient (T < 0, NaN, or so small that the division
//           overflows): no score can then be NaN or +inf.
//   else  : s_i = z_i / T, m = max s, e_i = expf(s_i - m),
//           q_i = floor(e_i * 2^32 + 0.5) as u64 (exact in double),
//           Q = sum q_i.  A token is kept if its logit passes the top_k
//           threshold (k-th largest value), the top_p threshold (largest
//           value whose tail mass reaches ceil(p * Q)) and the min_p
//           bound (q_i >= min_p * 2^32).  need is at least 1, and a row
//           whose filters keep nothing (min_p > 1) falls back to the
//           argmax with kept = 1, so the token is always below V.
//           The draw is the argmax over the
//           kept tokens of s_i + g_i, g_i Gumbel noise from Philox4x32-10
//           keyed by the row's seed with counter (i >> 2, pos, 0, 0).
// bf16 has 65536 values, so an order-preserving 16-bit key and a
// two-level 256-bin histogram in LDS (integer counts for top_k, u64
// masses for top_p) give both thresholds exactly, without a sort and in
// any summation order.  The row (256 KB for llama-3) is re-read through
// the caches in each pass.  Histograms are kept in SAMPLE_COPIES lane-striped
// copies: randn-like logits put a third of a row into one bin, and 64
// lanes adding to one LDS word serialise.
// A row whose pos is negative is skipped before any barrier.
// ---------------------------------------------------------------------
#define SAMPLE_THREADS 1024
#define SAMPLE_WAVES (SAMPLE_THREADS / 64)
#define SAMPLE_COPIES 16

// order-preserving 16-bit key of a bf16 bit pattern (-0 counts as +0)
DEV unsigned int sample_key(unsigned short raw) {
  unsigned int b = raw;
  if (b == 0x8000u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xFFFFu) : (b | 0x8000u);
}

DEV float sample_key_value(unsigned int key) {
  const unsigned int b = (key & 0x8000u) ? (key & 0x7FFFu) : (~key & 0xFFFFu);
  return bf2f((unsigned short)b);
}

DEV unsigned int sample_f32_ordered(float f) {
  union { float f; uint32_t i; } v;
  v.f = f;
  return (v.i & 0x80000000u) ? ~v.i : (v.i | 0x80000000u);
}

// (key, index) packed so that a u64 max picks the largest key and, among
// equal keys, the lowest index
DEV unsigned long long sample_pack(unsigned int key, unsigned int index) {
  return ((unsigned long long)key << 32) | (0xFFFFFFFFu - index);
}

DEV unsigned long long sample_mass(float e) {
  return (unsigned long long)floor((double)e * 4294967296.0 + 0.5);
}

DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                       uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Gumbel noise of one random word: u = ((r >> 8) + 0.5) * 2^-24 in f32
// (round to nearest even), kept below 1 so that g stays finite
DEV float sample_gumbel(uint32_t r) {
  float u = ((float)(r >> 8) + 0.5f) * 5.9604644775390625e-08f;
  u = fminf(u, 0.99999994f);
  return -logf(-logf(u));
}

DEV unsigned long long sample_block_max(unsigned long long v,
                                        unsigned long long* red, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  __syncthreads();  // red may still be read from an earlier reduction
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  unsigned long long r = red[0];
#pragma unroll
  for (int w = 1; w < SAMPLE_WAVES; ++w) r = red[w] > r ? red[w] : r;
  return r;
}

DEV unsigned long long sample_block_sum(unsigned long long v,
                                        unsigned long long* red, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  unsigned long long r = 0;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) r += red[w];
  return r;
}

// fixed-order f32 sum: lane tree, then the wave partials in wave order
DEV float sample_block_sumf(float v, float* red, int tid) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int w = 0; w < SAMPLE_WAVES; ++w) r += red[w];
  return r;
}

// hist holds 256 bins in SAMPLE_COPIES copies (bin * COPIES + copy).
// Finds the highest bin at which the total of that bin and all bins
// above it reaches `want` (>= 1); leaves the bin in sel[0] and the
// total strictly above it in *above.  Called by the whole workgroup.
template <typename T>
DEV void sample_select(T* hist, T want, unsigned int* sel, T* above,
                       int tid) {
  __syncthreads();  // all adds to hist have landed
  T total = 0;
  if (tid < 256) {
#pragma unroll
    for (int c = 0; c < SAMPLE_COPIES; ++c)
      total += hist[tid * SAMPLE_COPIES + c];
    hist[tid * SAMPLE_COPIES] = total;  // own bin only
  }
  __syncthreads();
  if (tid < 256) {
    T over = 0;
    for (int j = tid + 1; j < 256; ++j) over += hist[j * SAMPLE_COPIES];
    if (over < want && over + total >= want) {
      sel[0] = (unsigned int)tid;
      *above = over;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_tokens_kernel(
    const unsigned short* __restrict__ logits, const int* __restrict__ pos,
    const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const float* __restrict__ min_p,
    const long long* __restrict__ seed, long long* __restrict__ out_tokens,
    float* __restrict__ out_logprob, int* __restrict__ out_kept, int V) {
  __shared__ unsigned long long mass[256 * SAMPLE_COPIES];
  __shared__ unsigned int cnt[256 * SAMPLE_COPIES];
  __shared__ unsigned long long red64[SAMPLE_WAVES];
  __shared__ float redf[SAMPLE_WAVES];
  __shared__ unsigned int sel_k[1], sel_p[1];
  __shared__ unsigned int above_k;
  __shared__ unsigned long long above_p;

  const int b = blockIdx.x;
  const int position = pos[b];
  if (position < 0) return;  // block-uniform, before any barrier
  const int tid = threadIdx.x;
  const int copy = tid & (SAMPLE_COPIES - 1);
  const unsigned short* row = logits + (size_t)b * V;
  const float T = temperature[b];
  const int k = top_k[b];
  const float p = top_p[b];
  const float mp = min_p[b];
  // pass 1 counts for top_k before the row is known to be sampled
  const bool k_count = T > 0.f && k > 0 && k < V;
  const double mp_bound = (double)mp * 4294967296.0;

  for (int i = tid; i < 256 * SAMPLE_COPIES; i += SAMPLE_THREADS) {
    cnt[i] = 0u;
    mass[i] = 0ull;
  }
  if (tid == 0) {
    sel_k[0] = 0u; sel_p[0] = 0u; above_k = 0u; above_p = 0ull;
  }
  __syncthreads();

  // pass 1: the row maximum (lowest index on ties) and, for top_k, the
  // counts by the high byte of the key
  unsigned long long best = 0ull;
  for (int v = tid * 8; v < V; v += SAMPLE_THREADS * 8) {
    const short8v x = *reinterpret_cast<const short8v*>(row + v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const unsigned int key = sample_key((unsigned short)x[j]);
      const unsigned long long packed = sample_pack(key, (unsigned)(v + j));
      best = packed > best ? packed : best;
      if (k_count) atomicAdd(&cnt[(key >> 8) * SAMPLE_COPIES + copy], 1u);
    }
  }
  best = sample_block_max(best, red64, tid);
  const unsigned int max_key = (unsigned int)(best >> 32);
  const unsigned int max_index = 0xFFFFFFFFu - (unsigned int)best;
  const float zmax = sample_key_value(max_key);
  // greedy unless zmax / T is finite at T > 0: then every s_i <= m is
  // finite or -inf, and no mass or score below can be NaN
  const bool sampled = T > 0.f && isfinite(zmax / T);
  const float m = sampled ? zmax / T : 0.f;
  const bool k_on = sampled && k_count;
  const bool p_on = sampled && p < 1.f;
  const bool mp_on = sampled && mp > 0.f;

  // pass 2: the T = 1 softmax denominator for the logprob and, for
  // top_p, the fixed-point masses by the high byte of the key
  float lsum = 0.f;
  unsigned long long q_sum = 0ull;
  for (int v = tid * 8; v < V; v += SAMPLE_THREADS * 8) {
    const short8v x = *reinterpret_cast<const short8v*>(row + v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float z = bf2f((unsigned short)x[j]);
      lsum += expf(z - zmax);
      if (p_on) {
        const unsigned int key = sample_key((unsigned short)x[j]);
        const unsigned long long q = sample_mass(expf(z / T - m));
        q_sum += q;
        atomicAdd(&mass[(key >> 8) * SAMPLE_COPIES + copy], q);
      }
    }
  }
  lsum = sample_block_sumf(lsum, redf, tid);

  unsigned int threshold = 0u;  // keep keys >= threshold
  if (k_on || p_on) {
    unsigned long long need = 0ull;
    if (p_on) {
      const unsigned long long Q = sample_block_sum(q_sum, red64, tid);
      if (p > 0.f) need = (unsigned long long)ceil((double)p * (double)Q);
      need = need > 0ull ? need : 1ull;  // p <= 0 keeps the maximum
    }
    if (k_on) sample_select(cnt, (unsigned int)k, sel_k, &above_k, tid);
    if (p_on) sample_select(mass, need, sel_p, &above_p, tid);
    const unsigned int bin_k = sel_k[0], bin_p = sel_p[0];
    const unsigned int want_k = (unsigned int)k - above_k;
    const unsigned long long want_p = need - above_p;
    __syncthreads();  // everyone holds the level-1 result
    for (int i = tid; i < 256 * SAMPLE_COPIES; i += SAMPLE_THREADS) {
      cnt[i] = 0u;
      mass[i] = 0ull;
    }
    __syncthreads();
    // pass 3: the same two histograms by the low byte, inside the bins
    // that hold the thresholds
    for (int v = tid * 8; v < V; v += SAMPLE_THREADS * 8) {
      const short8v x = *reinterpret_cast<const short8v*>(row + v);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned int key = sample_key((unsigned short)x[j]);
        if (k_on && (key >> 8) == bin_k)
          atomicAdd(&cnt[(key & 255u) * SAMPLE_COPIES + copy], 1u);
        if (p_on && (key >> 8) == bin_p) {
          const float z = bf2f((unsigned short)x[j]);
          atomicAdd(&mass[(key & 255u) * SAMPLE_COPIES + copy],
                    sample_mass(expf(z / T - m)));
        }
      }
    }
    if (k_on) {
      sample_select(cnt, want_k, sel_k, &above_k, tid);
      threshold = (bin_k << 8) | sel_k[0];
    }
    if (p_on) {
      sample_select(mass, want_p, sel_p, &above_p, tid);
      const unsigned int t = (bin_p << 8) | sel_p[0];
      threshold = t > threshold ? t : threshold;
    }
  }

  unsigned int token = max_index;
  unsigned int kept = 1u;
  if (sampled) {
    // pass 4: Gumbel-max over the kept tokens; a Philox block serves
    // the four tokens 4c .. 4c + 3 and is skipped when none is kept
    const unsigned long long sd = (unsigned long long)seed[b];
    const uint32_t key0 = (uint32_t)sd, key1 = (uint32_t)(sd >> 32);
    unsigned long long top = 0ull;
    kept = 0u;
    for (int v = tid * 8; v < V; v += SAMPLE_THREADS * 8) {
      const short8v x = *reinterpret_cast<const short8v*>(row + v);
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        bool keep[4];
        float s[4];
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned short raw = (unsigned short)x[half * 4 + j];
          s[j] = bf2f(raw) / T;
          keep[j] = sample_key(raw) >= threshold;
          if (mp_on && keep[j])
            keep[j] = (double)sample_mass(expf(s[j] - m)) >= mp_bound;
          any = any || keep[j];
        }
        if (!any) continue;
        uint32_t r[4];
        philox4x32_10((uint32_t)(v >> 2) + half, (uint32_t)position, 0u, 0u,
                      key0, key1, r);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!keep[j]) continue;
          ++kept;
          const float score = s[j] + sample_gumbel(r[j]);
          const unsigned long long packed = sample_pack(
              sample_f32_ordered(score), (unsigned)(v + half * 4 + j));
          top = packed > top ? packed : top;
        }
      }
    }
    top = sample_block_max(top, red64, tid);
    kept = (unsigned int)sample_block_sum(kept, red64, tid);
    token = 0xFFFFFFFFu - (unsigned int)top;
    if (kept == 0u || token >= (unsigned int)V) {  // nothing kept: argmax
      token = max_index;
      kept = 1u;
    }
  }
  if (tid == 0) {
    out_tokens[b] = (long long)token;
    if (out_kept) out_kept[b] = (int)kept;
    if (out_logprob)
      out_logprob[b] = (bf2f(row[token]) - zmax) - logf(lsum);
  }
}

void launch_sample_tokens(const void* logits, const void* pos,
                          const void* temperature, const void* top_k,
                          const void* top_p, const void* min_p,
                          const void* seed, void* out_tokens,
                          void* out_logprob, void* out_kept, int B, int V,
                          void* stream) {
  if (B <= 0 || V <= 0) return;
  hipLaunchKernelGGL(sample_tokens_kernel, dim3(B), dim3(SAMPLE_THREADS), 0,
                     (hipStream_t)stream, (const unsigned short*)logits,
                     (const int*)pos, (const float*)temperature,
                     (const int*)top_k, (const float*)top_p,
                     (const float*)min_p, (const long long*)seed,
                     (long long*)out_tokens, (float*)out_logprob,
                     (int*)out_kept, V);
}

// ---------------------------------------------------------------------
// Logit processors: repetition / presence / frequency penalties and a
// logit bias, applied in place to the logits a sampler reads next, from
// a per-sequence token-state table that this kernel also maintains:
//   state[r, v] = 2 * (times v was generated) + (v is in the prompt)
// Grid (column tiles, B), 256 threads, 8 adjacent columns per thread: one
// 16 B vector of logits and two of state.  Every logit and every state
// word has exactly one owner, so there are no atomics and no thread
// reads global memory that another wrote in this launch; the owner of
// the pending token's column adds 2 to the word it holds and stores it.
// A neutral row (r == 1, p == 0, f == 0, no live bias) and a row whose
// state row is out of range leave before any load or barrier.
// Per column, c = state word, n = c >> 1, z = float(logit):
//   c != 0 and r != 1:  z = z > 0 ? z / r : z * r
//   n > 0:              z = (z - f * float(n)) - p
//   v is a live id:     z = z + bias
// Each step is one separately rounded f32 operation, bit for bit what
// ops.logit_processors computes on the CPU.  The build's default
// contraction would fuse z - f * n into an fma, so contraction is
// switched off for this kernel's body (#pragma clang fp contract(off))
// rather than spelling every operation as an intrinsic.
// Bias: wave 0 alone fills the LDS tile with -0.0f (z + -0.0f == z for
// every z, -0.0f included) and then scatters the live entries of this
// tile into it; LDS operations of one wave complete in issue order, so
// one workgroup barrier publishes the tile.  Rows without live entries
// skip tile and barrier, block-uniformly.
// ---------------------------------------------------------------------
constexpr int LOGIT_THREADS = 256;
constexpr int LOGIT_TILE = LOGIT_THREADS * 8;
constexpr int LOGIT_BIAS_MAX = 64;
typedef __attribute__((ext_vector_type(4))) int int4v;

__global__ __launch_bounds__(LOGIT_THREADS) void logit_processors_kernel(
    unsigned short* __restrict__ logits, int* __restrict__ state,
    const float* __restrict__ penalties, const int* __restrict__ bias_ids,
    const float* __restrict__ bias_val, const int* __restrict__ bias_n,
    const long long* __restrict__ tokens, const int* __restrict__ rows,
    int V, int S) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float tile[LOGIT_TILE];

  const int b = blockIdx.y;
  const int srow = rows ? rows[b] : b;
  if (srow < 0 || srow >= S) return;  // block-uniform, before any barrier
  const float rep = penalties[b * 3 + 0];
  const float pres = penalties[b * 3 + 1];
  const float freq = penalties[b * 3 + 2];
  int live = bias_n[b];
  live = live < 0 ? 0 : (live > LOGIT_BIAS_MAX ? LOGIT_BIAS_MAX : live);
  if (rep == 1.f && pres == 0.f && freq == 0.f && live == 0) return;

  const int tid = threadIdx.x;
  const int base = blockIdx.x * LOGIT_TILE;
  if (live > 0) {
    if (tid < 64) {  // wave 0: LOGIT_BIAS_MAX == one wave
      const f32x4v neg0 = {-0.f, -0.f, -0.f, -0.f};
#pragma unroll
      for (int i = 0; i < LOGIT_TILE / (64 * 4); ++i)
        *reinterpret_cast<f32x4v*>(&tile[(i * 64 + tid) * 4]) = neg0;
      // the scatter below may hit a word another lane has just filled
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (tid < live) {
        const int id = bias_ids[b * LOGIT_BIAS_MAX + tid];
        // id < V also keeps a last, partial tile inside the vocabulary
        if (id >= base && id < base + LOGIT_TILE && id < V)
          tile[id - base] = bias_val[b * LOGIT_BIAS_MAX + tid];
      }
    }
    __syncthreads();
  }
  const int v = base + tid * 8;
  if (v >= V) return;  // V % 8 == 0: a thread's 8 columns are in or out

  unsigned short* lrow = logits + (size_t)b * V + v;
  int* srow_ptr = state + (size_t)srow * V + v;
  const short8v x = *reinterpret_cast<const short8v*>(lrow);
  const int4v c_lo = *reinterpret_cast<const int4v*>(srow_ptr);
  const int4v c_hi = *reinterpret_cast<const int4v*>(srow_ptr + 4);
  int c[8] = {c_lo[0], c_lo[1], c_lo[2], c_lo[3],
              c_hi[0], c_hi[1], c_hi[2], c_hi[3]};
  // count the pending token first: its column is evaluated with it
  const long long t = tokens ? tokens[b] : -1ll;
  if (t >= (long long)v && t < (long long)v + 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (t == (long long)(v + j)) {
        c[j] += 2;
        srow_ptr[j] = c[j];
      }
    }
  }
  f32x4v add_lo = {-0.f, -0.f, -0.f, -0.f}, add_hi = add_lo;
  if (live > 0) {
    add_lo = *reinterpret_cast<const f32x4v*>(&tile[tid * 8]);
    add_hi = *reinterpret_cast<const f32x4v*>(&tile[tid * 8 + 4]);
  }
  short8v y;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float z = bf2f((unsigned short)x[j]);
    const int n = c[j] >> 1;
    if (c[j] != 0 && rep != 1.f) z = z > 0.f ? z / rep : z * rep;
    if (n > 0) {
      const float scaled = freq * (float)n;
      z = z - scaled;
      z = z - pres;
    }
    if (live > 0) z = z + (j < 4 ? add_lo[j & 3] : add_hi[j & 3]);
    y[j] = (short)f2bf(z);
  }
  *reinterpret_cast<short8v*>(lrow) = y;
}

void launch_logit_processors(void* logits, void* state,
                             const void* penalties, const void* bias_ids,
                             const void* bias_val, const void* bias_n,
                             const void* tokens, const void* rows, int B,
                             int V, int S, void* stream) {
  if (B <= 0 || V <= 0 || S <= 0) return;
  const dim3 grid((V + LOGIT_TILE - 1) / LOGIT_TILE, B);
  hipLaunchKernelGGL(logit_processors_kernel, grid, dim3(LOGIT_THREADS), 0,
                     (hipStream_t)stream, (unsigned short*)logits,
                     (int*)state, (const float*)penalties,
                     (const int*)bias_ids, (const float*)bias_val,
                     (const int*)bias_n, (const long long*)tokens,
                     (const int*)rows, V, S);
}

// ---------------------------------------------------------------------
// Row softmax (bf16 in/out, online single pass over LDS-staged row,
// used by classic-model servers & tests)
// ---------------------------------------------------------------------
__global__ void softmax_kernel(unsigned short* __restrict__ out,
                               const unsigned short* __restrict__ in,
                               int cols) {
  const int row = blockIdx.x;
  const int tid = threadIdx.x;
  const unsigned short* inr = in + (size_t)row * cols;
  unsigned short* outr = out + (size_t)row * cols;

  float lmax = -FLT_MAX;
  for (int i = tid; i < cols; i += blockDim.x)
    lmax = fmaxf(lmax, bf2f(inr[i]));
  __shared__ float red[64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    lmax = fmaxf(lmax, __shfl_xor(lmax, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = lmax;
  __syncthreads();
  float gmax = -FLT_MAX;
  for (int w = 0; w < (blockDim.x >> 6); ++w) gmax = fmaxf(gmax, red[w]);

  float lsum = 0.f;
  for (int i = tid; i < cols; i += blockDim.x)
    lsum += __expf(bf2f(inr[i]) - gmax);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    lsum += __shfl_xor(lsum, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = lsum;
  __syncthreads();
  float gsum = 0.f;
  for (int w = 0; w < (blockDim.x >> 6); ++w) gsum += red[w];
  const float inv = 1.f / gsum;
  for (int i = tid; i < cols; i += blockDim.x)
    outr[i] = f2bf(__expf(bf2f(inr[i]) - gmax) * inv);
}

void launch_softmax(void* out, const void* in, int rows, int cols,
                    void* stream) {
  hipLaunchKernelGGL(softmax_kernel, dim3(rows), dim3(256), 0,
                     (hipStream_t)stream, (unsigned short*)out,
                     (const unsigned short*)in, cols);
}

// ---------------------------------------------------------------------
// Tree-ensemble inference (XGBoost/GBDT-style), for the classic-model
// serving config.  Trees in flattened SoA node arrays; each lane
// evaluates one sample through all trees (depth-bound loop).
// features: [n_samples, n_features] f32; out: [n_samples] f32
// ---------------------------------------------------------------------
__global__ void tree_ensemble_kernel(
    float* __restrict__ out, const float* __restrict__ features,
    const int* __restrict__ feature_idx,    // per node: feature (-1 = leaf)
    const float* __restrict__ threshold,    // per node: split threshold
    const int* __restrict__ left,           // per node: left child index
    const int* __restrict__ right,          // per node: right child index
    const float* __restrict__ leaf_value,   // per node: value if leaf
    const int* __restrict__ tree_offsets,   // [n_trees+1] node offsets
    int n_trees, int n_samples, int n_features, float base_score) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n_samples; i += stride) {
    const float* frow = features + i * n_features;
    float score = base_score;
    for (int t = 0; t < n_trees; ++t) {
      int node = tree_offsets[t];
      int fidx = feature_idx[node];
      while (fidx >= 0) {
        node = (frow[fidx] < threshold[node]) ? left[node] : right[node];
        fidx = feature_idx[node];
      }
      score += leaf_value[node];
    }
    out[i] = score;
  }
}

void launch_tree_ensemble(void* out, const void* features,
                          const void* feature_idx, const void* threshold,
                          const void* left, const void* right,
                          const void* leaf_value, const void* tree_offsets,
                          int n_trees, int n_samples, int n_features,
                          float base_score, void* stream) {
  long long blocks = (n_samples + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(tree_ensemble_kernel, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, (float*)out,
                     (const float*)features, (const int*)feature_idx,
                     (const float*)threshold, (const int*)left,
                     (const int*)right, (const float*)leaf_value,
                     (const int*)tree_offsets, n_trees, n_samples, n_features,
                     base_score);
}

// ---------------------------------------------------------------------
// Feature-store sliding-window aggregation:
// For each (key, feature): ring buffer of per-period partial aggregates
// resident in HBM; this kernel folds a batch of events into the ring
// and emits current window aggregates (sum/count/min/max -> avg
// derived host-side).
// events: keys[n] int32 (dense key ids), values[n] f32, periods[n] int32
// ring: [n_keys, n_feats?, n_periods, 4] (sum, count, min, max) f32
// Batched: one lane per event; atomics within the period cell.
// ---------------------------------------------------------------------
__global__ void window_ingest_kernel(float* __restrict__ ring,
                                     const int* __restrict__ keys,
                                     const float* __restrict__ values,
                                     const int* __restrict__ period_idx,
                                     long long n_events, int n_periods) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n_events; i += stride) {
    const int key = keys[i];
    const int p = period_idx[i] % n_periods;
    float* cell = ring + ((size_t)key * n_periods + p) * 4;
    const float v = values[i];
    atomicAdd(cell + 0, v);             // sum
    atomicAdd(cell + 1, 1.f);           // count
    // min/max are tracked per-batch host-side (they are not
    // decomposable over ring periods for sliding windows anyway)
  }
}

// window reduce: sum the last `window_periods` period cells per key
// ring: [n_keys, n_periods, 4]; out: [n_keys, 4]
__global__ void window_reduce_kernel(float* __restrict__ out,
                                     const float* __restrict__ ring,
                                     int n_keys, int n_periods,
                                     int window_periods, int current_period) {
  int key = blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= n_keys) return;
  float sum = 0.f, count = 0.f;
  for (int w = 0; w < window_periods; ++w) {
    int p = (current_period - w) % n_periods;
    if (p < 0) p += n_periods;
    const float* cell = ring + ((size_t)key * n_periods + p) * 4;
    sum += cell[0];
    count += cell[1];
  }
  out[key * 4 + 0] = sum;
  out[key * 4 + 1] = count;
  out[key * 4 + 2] = count > 0.f ? sum / count : 0.f;  // avg
  out[key * 4 + 3] = 0.f;
}

// ---------------------------------------------------------------------
// Per-period min/max cells: float atomic min/max via the ordered-int
// transform (monotone map f32 -> u32 so unsigned atomics give float
// order).  Per-period cells make min/max DECOMPOSABLE for the
// bucket-quantized sliding windows served by window_reduce — unlike
// the running aggregates the round-1 path fell back to.
// ring_mm: [n_keys, n_periods, 2] u32 (ordered-min, ordered-max),
// empty cells hold 0xFFFFFFFF / 0x00000000.
// ---------------------------------------------------------------------
__device__ __forceinline__ unsigned int f32_to_ordered(float v) {
  unsigned int bits = __float_as_uint(v);
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__device__ __forceinline__ float ordered_to_f32(unsigned int key) {
  unsigned int bits = (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
  return __uint_as_float(bits);
}

__global__ void window_ingest_mm_kernel(unsigned int* __restrict__ ring_mm,
                                        const int* __restrict__ keys,
                                        const float* __restrict__ values,
                                        const int* __restrict__ period_idx,
                                        long long n_events, int n_periods) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n_events; i += stride) {
    const int key = keys[i];
    const int p = period_idx[i] % n_periods;
    unsigned int* cell = ring_mm + ((size_t)key * n_periods + p) * 2;
    const unsigned int ov = f32_to_ordered(values[i]);
    atomicMin(cell + 0, ov);
    atomicMax(cell + 1, ov);
  }
}

// first/last per period: packed u64 = (ts << 32) | ordered(value);
// atomicMin gives the earliest event (ties broken by value order),
// atomicMax the latest.  ts fits 31 bits until 2038 (unix seconds).
// ring_fl: [n_keys, n_periods, 2] u64, empty = (ULLONG_MAX, 0).
__global__ void window_ingest_fl_kernel(
    unsigned long long* __restrict__ ring_fl,
    const int* __restrict__ keys, const float* __restrict__ values,
    const int* __restrict__ timestamps, const int* __restrict__ period_idx,
    long long n_events, int n_periods) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n_events; i += stride) {
    const int key = keys[i];
    const int p = period_idx[i] % n_periods;
    unsigned long long* cell = ring_fl + ((size_t)key * n_periods + p) * 2;
    const unsigned long long pack =
        ((unsigned long long)(unsigned int)timestamps[i] << 32) |
        f32_to_ordered(values[i]);
    atomicMin(cell + 0, pack);  // first = earliest pack
    atomicMax(cell + 1, pack);  // last = latest pack
  }
}

// reduce min/max + first/last over the covered window cells.
// out_mmfl: [n_keys, 4] f32 (min, max, first, last); count==0 rows are
// left as written (caller masks by count from window_reduce).
__global__ void window_reduce_mmfl_kernel(
    float* __restrict__ out, const unsigned int* __restrict__ ring_mm,
    const unsigned long long* __restrict__ ring_fl, int n_keys,
    int n_periods, int window_periods, int current_period) {
  int key = blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= n_keys) return;
  unsigned int omin = 0xFFFFFFFFu, omax = 0u;
  unsigned long long first_pack = 0xFFFFFFFFFFFFFFFFull, last_pack = 0ull;
  for (int w = 0; w < window_periods; ++w) {
    int p = (current_period - w) % n_periods;
    if (p < 0) p += n_periods;
    const unsigned int* mm = ring_mm + ((size_t)key * n_periods + p) * 2;
    omin = min(omin, mm[0]);
    omax = max(omax, mm[1]);
    const unsigned long long* fl =
        ring_fl + ((size_t)key * n_periods + p) * 2;
    first_pack = min(first_pack, fl[0]);
    last_pack = max(last_pack, fl[1]);
  }
  float* row = out + (size_t)key * 4;
  row[0] = omin == 0xFFFFFFFFu ? 0.f : ordered_to_f32(omin);
  row[1] = omax == 0u ? 0.f : ordered_to_f32(omax);
  row[2] = first_pack == 0xFFFFFFFFFFFFFFFFull
               ? 0.f
               : ordered_to_f32((unsigned int)(first_pack & 0xFFFFFFFFull));
  row[3] = last_pack == 0ull
               ? 0.f
               : ordered_to_f32((unsigned int)(last_pack & 0xFFFFFFFFull));
}

// f64 variants for the sum-of-squares ring: the stdvar formula
// sumsq/n - mean^2 cancels catastrophically in f32 when values are
// large and var is small — f64 accumulation keeps ~16 digits
// (atomicAdd(double) is native on CDNA4 HBM).
__global__ void window_ingest64_kernel(double* __restrict__ ring,
                                       const int* __restrict__ keys,
                                       const float* __restrict__ values,
                                       const int* __restrict__ period_idx,
                                       long long n_events, int n_periods) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long stride = (long long)gridDim.x * blockDim.x;
  for (; i < n_events; i += stride) {
    const int key = keys[i];
    const int p = period_idx[i] % n_periods;
    double* cell = ring + ((size_t)key * n_periods + p) * 4;
    const double v = (double)values[i];
    atomicAdd(cell + 0, v * v);  // sum of squares
    atomicAdd(cell + 1, 1.0);    // count
    atomicAdd(cell + 2, v);      // f64 sum (variance needs f64 mean)
  }
}

__global__ void window_reduce64_kernel(double* __restrict__ out,
                                       const double* __restrict__ ring,
                                       int n_keys, int n_periods,
                                       int window_periods,
                                       int current_period) {
  int key = blockIdx.x * blockDim.x + threadIdx.x;
  if (key >= n_keys) return;
  double sumsq = 0.0, count = 0.0, sum = 0.0;
  for (int w = 0; w < window_periods; ++w) {
    int p = (current_period - w) % n_periods;
    if (p < 0) p += n_periods;
    const double* cell = ring + ((size_t)key * n_periods + p) * 4;
    sumsq += cell[0];
    count += cell[1];
    sum += cell[2];
  }
  out[key * 4 + 0] = sumsq;
  out[key * 4 + 1] = count;
  out[key * 4 + 2] = sum;
  out[key * 4 + 3] = 0.0;
}

void launch_window_ingest64(void* ring, const void* keys,
                            const void* values, const void* period_idx,
                            long long n_events, int n_periods,
                            void* stream) {
  long long blocks = (n_events + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(window_ingest64_kernel, dim3((int)blocks), dim3(256),
                     0, (hipStream_t)stream, (double*)ring,
                     (const int*)keys, (const float*)values,
                     (const int*)period_idx, n_events, n_periods);
}

void launch_window_reduce64(void* out, const void* ring, int n_keys,
                            int n_periods, int window_periods,
                            int current_period, void* stream) {
  int blocks = (n_keys + 255) / 256;
  hipLaunchKernelGGL(window_reduce64_kernel, dim3(blocks), dim3(256), 0,
                     (hipStream_t)stream, (double*)out,
                     (const double*)ring, n_keys, n_periods,
                     window_periods, current_period);
}

void launch_window_ingest_mm(void* ring_mm, const void* keys,
                             const void* values, const void* period_idx,
                             long long n_events, int n_periods,
                             void* stream) {
  long long blocks = (n_events + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(window_ingest_mm_kernel, dim3((int)blocks), dim3(256),
                     0, (hipStream_t)stream, (unsigned int*)ring_mm,
                     (const int*)keys, (const float*)values,
                     (const int*)period_idx, n_events, n_periods);
}

void launch_window_ingest_fl(void* ring_fl, const void* keys,
                             const void* values, const void* timestamps,
                             const void* period_idx, long long n_events,
                             int n_periods, void* stream) {
  long long blocks = (n_events + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(window_ingest_fl_kernel, dim3((int)blocks), dim3(256),
                     0, (hipStream_t)stream,
                     (unsigned long long*)ring_fl, (const int*)keys,
                     (const float*)values, (const int*)timestamps,
                     (const int*)period_idx, n_events, n_periods);
}

void launch_window_reduce_mmfl(void* out, const void* ring_mm,
                               const void* ring_fl, int n_keys,
                               int n_periods, int window_periods,
                               int current_period, void* stream) {
  int blocks = (n_keys + 255) / 256;
  hipLaunchKernelGGL(window_reduce_mmfl_kernel, dim3(blocks), dim3(256), 0,
                     (hipStream_t)stream, (float*)out,
                     (const unsigned int*)ring_mm,
                     (const unsigned long long*)ring_fl, n_keys, n_periods,
                     window_periods, current_period);
}

void launch_window_ingest(void* ring, const void* keys, const void* values,
                          const void* period_idx, long long n_events,
                          int n_periods, void* stream) {
  long long blocks = (n_events + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(window_ingest_kernel, dim3((int)blocks), dim3(256), 0,
                     (hipStream_t)stream, (float*)ring, (const int*)keys,
                     (const float*)values, (const int*)period_idx, n_events,
                     n_periods);
}

void launch_window_reduce(void* out, const void* ring, int n_keys,
                          int n_periods, int window_periods,
                          int current_period, void* stream) {
  int blocks = (n_keys + 255) / 256;
  hipLaunchKernelGGL(window_reduce_kernel, dim3(blocks), dim3(256), 0,
                     (hipStream_t)stream, (float*)out, (const float*)ring,
                     n_keys, n_periods, window_periods, current_period);
}
